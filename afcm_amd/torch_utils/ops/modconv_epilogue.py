"""modconv_epilogue: everything the CoModGAN ``SynthesisLayer`` does after its convolution, in one pass (C ABI
afcm_modconv_epilogue_fwd / _bwd, csrc/modconv_epilogue.hip):

    y[n, o, u i + py, u j + px] = clamp(lrelu(t[n, (py u + px) O + o, i, j] * dcoefs[n, o] + noise * noise_strength + bias[o]) * gain, +-clamp)

-- demodulation, noise, bias, leaky ReLU, gain and clamp (layers.py:59-62 and :302-304 of the reference: ``fma`` then ``bias_act``), and for
``up=2`` the depth-to-space interleave of the four phase convolutions (networks_comodgan.fold_up2_weights).  fp32 only; first-order
gradients for t, dcoefs, bias and noise_strength (the generator is never differentiated twice), the reductions in float64 in a fixed order.
"""
import torch

from ... import _lib


def _check(t, dcoefs, bias, noise, noise_strength, up):
    _lib.require_gpu(t, dcoefs, bias, noise, noise_strength)
    if up not in (1, 2):
        raise RuntimeError(f'modconv_epilogue: up is 1 or 2, got {up}')
    if t.ndim != 4 or t.shape[1] % (up * up):
        raise RuntimeError(f'modconv_epilogue: t must be [N, {up * up} * O, H, W], got {tuple(t.shape)}')
    n, o, h, w = int(t.shape[0]), int(t.shape[1]) // (up * up), int(t.shape[2]), int(t.shape[3])
    if tuple(dcoefs.shape) != (n, o) or tuple(bias.shape) != (o,):
        raise RuntimeError(f'modconv_epilogue: dcoefs must be [{n}, {o}] and bias [{o}], got {tuple(dcoefs.shape)} and {tuple(bias.shape)}')
    per_sample = 0
    if (noise is None) != (noise_strength is None):
        raise RuntimeError('modconv_epilogue: noise and noise_strength come together')
    if noise is not None:
        if tuple(noise.shape) == (n, 1, up * h, up * w):
            per_sample = 1
        elif tuple(noise.shape) != (up * h, up * w):
            raise RuntimeError(f'modconv_epilogue: noise must be [{up * h}, {up * w}] or [{n}, 1, {up * h}, {up * w}], got {tuple(noise.shape)}')
        if noise_strength.numel() != 1:
            raise RuntimeError('modconv_epilogue: noise_strength is one number')
    for v in (t, dcoefs, bias, noise, noise_strength):
        if v is not None and v.dtype != torch.float32:
            raise RuntimeError(f'modconv_epilogue: float32 tensors only, got {v.dtype}')
    return n, o, h, w, per_sample


class _ModconvEpilogue(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, dcoefs, bias, noise, noise_strength, up, alpha, gain, clamp):
        n, o, h, w, per_sample = _check(t, dcoefs, bias, noise, noise_strength, up)
        lib = _lib.load()
        t, dcoefs, bias = t.detach().contiguous(), dcoefs.detach().contiguous(), bias.detach().contiguous()
        # (a contiguous view of t or noise at an odd offset is taken as it is: the entry points fall back to 4-byte accesses for it)
        noise = None if noise is None else noise.detach().contiguous()
        strength = None if noise_strength is None else noise_strength.detach().reshape(1).contiguous()
        y = torch.empty([n, o, up * h, up * w], dtype=torch.float32, device=t.device)
        _lib.launched(lib.afcm_modconv_epilogue_fwd(y.data_ptr(), t.data_ptr(), dcoefs.data_ptr(), bias.data_ptr(), _lib.ptr(noise), _lib.ptr(strength),
                                                    per_sample, n, o, h, w, up, alpha, gain, clamp, _lib.stream_ptr(t)), 'modconv_epilogue_fwd')
        ctx.save_for_backward(y, t, dcoefs, noise)
        ctx.cfg = (n, o, h, w, per_sample, up, alpha, gain, clamp, None if noise_strength is None else tuple(noise_strength.shape))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        y, t, dcoefs, noise = ctx.saved_tensors
        n, o, h, w, per_sample, up, alpha, gain, clamp, strength_shape = ctx.cfg
        lib = _lib.load()
        dy = dy.to(torch.float32).contiguous()
        if dy.data_ptr() % 16:                 # a contiguous view at an odd offset: the kernel reads dy in 8- / 16-byte pieces
            dy = dy.clone()
        dev = y.device
        d_t = torch.empty_like(t)
        d_dcoefs = torch.empty_like(dcoefs)
        d_bias = torch.empty([o], dtype=torch.float32, device=dev)
        d_strength = torch.empty([1], dtype=torch.float32, device=dev) if noise is not None else None
        ws = torch.empty([lib.afcm_modconv_epilogue_workspace_bytes(n, o, h, w) // 8], dtype=torch.float64, device=dev)
        _lib.launched(lib.afcm_modconv_epilogue_bwd(d_t.data_ptr(), d_dcoefs.data_ptr(), d_bias.data_ptr(), _lib.ptr(d_strength), ws.data_ptr(),
                                                    dy.data_ptr(), y.data_ptr(), t.data_ptr(), dcoefs.data_ptr(), _lib.ptr(noise), per_sample,
                                                    n, o, h, w, up, alpha, gain, clamp, _lib.stream_ptr(y)), 'modconv_epilogue_bwd')
        if d_strength is not None:
            d_strength = d_strength.reshape(strength_shape)
        return d_t, d_dcoefs, d_bias, None, d_strength, None, None, None, None


def modconv_epilogue(t, dcoefs, bias, noise=None, noise_strength=None, up=1, alpha=0.2, gain=1.0, clamp=None):
    """t [N, up^2 O, H, W] -> y [N, O, up H, up W] (see the module docstring).  ``noise``: None, [up H, up W] or [N, 1, up H, up W] (no gradient);
    ``noise_strength``: a one-element device tensor; ``clamp``: None or >= 0, applied after the gain."""
    if clamp is not None and not clamp >= 0:
        raise RuntimeError(f'modconv_epilogue: clamp is None or >= 0, got {clamp}')
    return _ModconvEpilogue.apply(t, dcoefs, bias, noise, noise_strength, int(up), float(alpha), float(gain), float(clamp if clamp is not None else -1))
