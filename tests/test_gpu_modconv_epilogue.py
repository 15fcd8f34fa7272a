"""The modulated-conv epilogue kernel (csrc/modconv_epilogue.hip, torch_utils/ops/modconv_epilogue.py) element by element against a float64
restatement of its definition

    y[n, o, u i + py, u j + px] = clamp(lrelu(t[n, (py u + px) O + o, i, j] * dcoefs[n, o] + noise * strength + bias[o]) * gain, +-clamp)

Bounds: forward and d_t within 2 fp32 ulps of the float64 value; the three reductions (d_dcoefs, d_bias, d_noise_strength), which the kernel
accumulates in float64, within 1 fp32 ulp of the float64 sum; two launches give the same bits.  Conventions at the kinks are bias_act's: the
negative slope AT y == 0, no gradient AT |y| == clamp.  Every figure is printed before it is asserted.

Shapes: u in {1, 2}; N in {1, 3}; O in {1, 5}; noise none / one plane / per sample; clamp off / on; gain 1 and sqrt(1/2); planes
  1x1, 3x5, 17x9   odd widths: the element path (one pixel per thread), one partly filled 256-thread chunk
  20x23            the element path over two chunks, the second partly filled
  4x4              widths that are a multiple of 4: the vector path for u = 1 (4 pixels per thread) and u = 2 (2 pixels per thread)
  5x6              even, no multiple of 4: the vector path for u = 2, the element path for u = 1
  24x44            the vector path over two (u = 1: 264 threads) and three (u = 2: 528 threads) chunks, the last partly filled
and once each path on tensors that are contiguous views at an odd offset (the entry points fall back to the element path)."""
import itertools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ALPHA = 0.2
PLANES = [(1, 1), (3, 5), (4, 4), (17, 9), (20, 23), (24, 44), (5, 6)]


def _d2s(t, u):
    """[N, u u O, H, W] -> [N, O, u H, u W] in the kernel's channel order."""
    n, c, h, w = t.shape
    o = c // (u * u)
    return t.reshape(n, u, u, o, h, w).permute(0, 3, 4, 1, 5, 2).reshape(n, o, u * h, u * w)


def _s2d(y, u):
    n, o, hh, ww = y.shape
    h, w = hh // u, ww // u
    return y.reshape(n, o, h, u, w, u).permute(0, 3, 5, 1, 2, 4).reshape(n, u * u * o, h, w)


def _ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def _forward64(t, d, b, noise, s, u, gain, clamp):
    pre = _d2s(t.double(), u) * d.double()[:, :, None, None] + b.double()[None, :, None, None]
    if noise is not None:
        nz = noise.double() if noise.ndim == 4 else noise.double()[None, None]
        pre = pre + nz * s.double()
    act = torch.where(pre > 0, pre, pre * ALPHA) * gain
    if clamp is not None:
        c = float(np.float32(clamp))
        act = act.clamp(-c, c)
    return act


def _backward64(dy, y, t, d, noise, u, gain, clamp):
    """From dy and the SAVED y (the kernel's own output), as the kernel does."""
    one, slope = torch.tensor(1.0, dtype=torch.float64), torch.tensor(ALPHA, dtype=torch.float64)     # (python scalars would make a float32 0.2)
    g = dy.double() * torch.where(y > 0, one, slope) * gain
    if clamp is not None:
        c = float(np.float32(clamp))
        g = g * ((y > -c) & (y < c)).double()
    d_t = _s2d(g * d.double()[:, :, None, None], u)
    terms_d = g * _d2s(t.double(), u)
    out = {'d_t': d_t, 'd_dcoefs': terms_d.sum([2, 3]), 'd_bias': g.sum([0, 2, 3])}
    if noise is not None:
        nz = noise.double() if noise.ndim == 4 else noise.double()[None, None]
        out['d_strength'] = (g * nz).sum()
    return out


def _inputs(u, n, o, h, w, noise_kind, seed):
    gen = torch.Generator().manual_seed(seed)
    t = torch.randn(n, u * u * o, h, w, generator=gen)
    d = torch.rand(n, o, generator=gen) + 0.5
    b = torch.randn(o, generator=gen) * 0.3
    noise = s = None
    if noise_kind == 'const':
        noise = torch.randn(u * h, u * w, generator=gen)
    if noise_kind == 'sample':
        noise = torch.randn(n, 1, u * h, u * w, generator=gen)
    if noise is not None:
        s = torch.tensor(0.37)
    dy = torch.randn(n, o, u * h, u * w, generator=gen)
    return t, d, b, noise, s, dy


def _run(t, d, b, noise, s, dy, u, gain, clamp):
    from afcm_amd.torch_utils.ops.modconv_epilogue import modconv_epilogue
    leaves = [v.cuda().requires_grad_(True) for v in (t, d, b)]
    sg = s.cuda().requires_grad_(True) if s is not None else None
    y = modconv_epilogue(leaves[0], leaves[1], leaves[2], None if noise is None else noise.cuda(), sg, up=u, alpha=ALPHA, gain=gain, clamp=clamp)
    grads = torch.autograd.grad(y, leaves + ([sg] if sg is not None else []), dy.cuda())
    return y.detach().cpu(), [g.cpu() for g in grads]


@pytest.mark.parametrize('plane', PLANES)
@pytest.mark.parametrize('u', [1, 2])
def test_against_float64(u, plane):
    h, w = plane
    worst = {}
    for n, o, noise_kind, clamp, gain in itertools.product((1, 3), (1, 5), ('none', 'const', 'sample'), (None, 1.25), (1.0, math.sqrt(0.5))):
        t, d, b, noise, s, dy = _inputs(u, n, o, h, w, noise_kind, seed=1 + 7 * n + 11 * o + 100 * h + w)
        y, grads = _run(t, d, b, noise, s, dy, u, gain, clamp)
        y2, grads2 = _run(t, d, b, noise, s, dy, u, gain, clamp)
        assert torch.equal(y, y2) and all(torch.equal(a, c) for a, c in zip(grads, grads2)), 'two launches, different bits'
        want = _forward64(t, d, b, noise, s, u, gain, clamp)
        assert y.shape == want.shape == (n, o, u * h, u * w)
        e = float(((y.double() - want).abs().numpy() / _ulp32(want.numpy())).max())
        worst['y'] = max(worst.get('y', 0.0), e)
        if clamp is not None:
            assert float(y.abs().max()) <= np.float32(clamp)
        ref = _backward64(dy, y, t, d, noise, u, gain, clamp)
        names = ['d_t', 'd_dcoefs', 'd_bias'] + (['d_strength'] if noise is not None else [])
        for name, got in zip(names, grads):
            r = ref[name].numpy()
            assert tuple(got.shape) == r.shape, (name, got.shape, r.shape)
            e = float((np.abs(got.double().numpy() - r) / _ulp32(r)).max())
            worst[name] = max(worst.get(name, 0.0), e)
    print(f'u {u} plane {plane}: worst error in fp32 ulps of the float64 value:', {k: round(v, 3) for k, v in worst.items()})
    assert worst['y'] <= 2 and worst['d_t'] <= 2
    assert worst['d_dcoefs'] <= 1 and worst['d_bias'] <= 1 and worst['d_strength'] <= 1


@pytest.mark.parametrize('u', [1, 2])
def test_contiguous_views_at_an_odd_offset(u):
    """t, the noise and dy as contiguous views one float into their buffers (4-byte aligned only) on a shape that otherwise takes the vector path:
    the same y and d_t bit for bit as from aligned tensors, the sums within 1 fp32 ulp of float64."""
    from afcm_amd.torch_utils.ops.modconv_epilogue import modconv_epilogue
    n, o, h, w = 3, 5, 4, 8
    t, d, b, noise, s, dy = _inputs(u, n, o, h, w, 'sample', seed=77)
    y0, g0 = _run(t, d, b, noise, s, dy, u, 1.0, 1.25)

    def shifted(v):
        buf = torch.zeros(v.numel() + 1, device='cuda')
        buf[1:] = v.reshape(-1).cuda()
        out = buf[1:].view(v.shape)
        assert out.is_contiguous() and out.data_ptr() % 16 == 4
        return out
    tt = shifted(t).requires_grad_(True)
    dd, bb, ss = d.cuda().requires_grad_(True), b.cuda().requires_grad_(True), s.cuda().requires_grad_(True)
    y = modconv_epilogue(tt, dd, bb, shifted(noise), ss, up=u, alpha=ALPHA, gain=1.0, clamp=1.25)
    grads = [g.cpu() for g in torch.autograd.grad(y, [tt, dd, bb, ss], shifted(dy))]
    assert torch.equal(y.detach().cpu(), y0) and torch.equal(grads[0], g0[0])
    ref = _backward64(dy, y0, t, d, noise, u, 1.0, 1.25)
    for name, got in zip(('d_dcoefs', 'd_bias', 'd_strength'), grads[1:]):
        r = ref[name].numpy()
        assert float((np.abs(got.double().numpy() - r) / _ulp32(r)).max()) <= 1, name


@pytest.mark.parametrize('u', [1, 2])
def test_conventions_at_the_kink_and_at_the_clamp(u):
    """dcoefs = 1, bias = 0, no noise, gain 1, clamp 2: t planted at 0 (y == 0: the gradient takes the NEGATIVE slope), at +-2 (y == +-clamp exactly:
    no gradient), just inside +-2 (gradient) and beyond (clamped, no gradient)."""
    inside = float(np.nextafter(np.float32(2), np.float32(0)))
    vals = [0.0, -0.0, 2.0, -10.0, inside, -inside * 5, 2.5, -11.0, 1.0, -1.0]         # the negative side reaches -2 at t = -10 (slope 0.2)
    n, o, h, w = 1, 2, 3, 5
    t = torch.tensor(vals * (u * u * o * h * w // len(vals) + 1))[:u * u * o * h * w].reshape(n, u * u * o, h, w).contiguous()
    d, b = torch.ones(n, o), torch.zeros(o)
    dy = torch.full((n, o, u * h, u * w), 3.0)
    y, grads = _run(t, d, b, None, None, dy, u, 1.0, 2.0)
    ts = _d2s(t, u)
    want_y = _forward64(t, d, b, None, None, u, 1.0, 2.0)
    assert float(((y.double() - want_y).abs().numpy() / _ulp32(want_y.numpy())).max()) <= 2
    assert bool((y[ts == 0] == 0).all()) and bool((y[ts == 2.0] == 2.0).all()) and bool((y[ts == -10.0] == -2.0).all())
    g = _d2s(grads[0], u)
    assert bool((g[ts == 0] == np.float32(3.0 * 0.2)).all()), 'the negative slope at y == 0'
    assert bool((g[ts == 2.0] == 0).all()) and bool((g[ts == -10.0] == 0).all()), 'no gradient at the clamp'
    assert bool((g[ts == 2.5] == 0).all()) and bool((g[ts == -11.0] == 0).all()), 'no gradient beyond the clamp'
    assert bool((g[ts == np.float32(inside)] == 3.0).all()) and bool((g[ts == 1.0] == 3.0).all()) and bool((g[ts == -1.0] == np.float32(0.6)).all())


def test_invalid_arguments_are_refused_by_the_entry_point():
    from afcm_amd import _lib
    lib = _lib.load()
    n, o, h, w, u = 1, 2, 3, 4, 2
    y = torch.full((n, o, u * h + 1, u * w), -7.0, device='cuda')           # one spare row: room for the misaligned call's pointer
    t = torch.zeros(n, u * u * o, h, w, device='cuda')
    d, b, s = torch.ones(n, o, device='cuda'), torch.zeros(o, device='cuda'), torch.zeros(1, device='cuda')
    nz = torch.zeros(u * h, u * w, device='cuda')
    st = _lib.stream_ptr(y)

    def fwd(yp=y.data_ptr(), tp=t.data_ptr(), noise=None, strength=None, per=0, n=n, o=o, h=h, w=w, u=u, gain=1.0, clamp=-1.0):
        return lib.afcm_modconv_epilogue_fwd(yp, tp, d.data_ptr(), b.data_ptr(), noise, strength, per, n, o, h, w, u, 0.2, gain, clamp, st)
    bad = [dict(u=3), dict(u=0), dict(yp=None), dict(tp=None), dict(n=0), dict(h=0), dict(gain=0.0), dict(gain=float('inf')), dict(clamp=float('nan')),
           dict(noise=nz.data_ptr()), dict(strength=s.data_ptr()), dict(noise=nz.data_ptr(), strength=s.data_ptr(), per=2),
           dict(yp=y.data_ptr() + 4), dict(h=1 << 16, w=1 << 15)]
    for kw in bad:
        assert fwd(**kw) == _lib.E_INVALID, kw
        assert lib.afcm_last_error().startswith(b'modconv_epilogue_fwd'), kw
    ws = torch.zeros(lib.afcm_modconv_epilogue_workspace_bytes(n, o, h, w) // 8, dtype=torch.float64, device='cuda')
    assert ws.numel() == (n * o * 1 + n * o) * 3
    dt, dd, db = torch.full_like(t, -7.0), torch.full_like(d, -7.0), torch.full_like(b, -7.0)
    dy = torch.zeros(n, o, u * h, u * w, device='cuda')

    def bwd(dtp=dt.data_ptr(), wsp=ws.data_ptr(), noise=None, dstrength=None, u=u, gain=1.0, dyp=dy.data_ptr()):
        return lib.afcm_modconv_epilogue_bwd(dtp, dd.data_ptr(), db.data_ptr(), dstrength, wsp, dyp, dy.data_ptr(), t.data_ptr(), d.data_ptr(), noise, 0,
                                             n, o, h, w, u, 0.2, gain, -1.0, st)
    for kw in [dict(dtp=None), dict(wsp=None), dict(wsp=ws.data_ptr() + 4), dict(noise=nz.data_ptr()), dict(dstrength=s.data_ptr()), dict(u=4),
               dict(gain=-1.0), dict(dyp=dy.data_ptr() + 4)]:
        assert bwd(**kw) == _lib.E_INVALID, kw
        assert lib.afcm_last_error().startswith(b'modconv_epilogue_bwd'), kw
    torch.cuda.synchronize()
    for v in (y, dt, dd, db):
        assert bool((v == -7.0).all()), 'a refused call launched something'
    assert fwd() == 0 and bwd() == 0                                         # and the same arguments, valid, run
    torch.cuda.synchronize()
    assert bool((y.reshape(-1)[:n * o * u * h * u * w] == 0).all())          # lrelu(0 * 1 + 0): the valid call wrote its n o (u h)(u w) elements
    from afcm_amd.torch_utils.ops.modconv_epilogue import modconv_epilogue
    for call in (lambda: modconv_epilogue(t, d, b, up=3), lambda: modconv_epilogue(t, d.double(), b, up=2), lambda: modconv_epilogue(t, d, b, noise=nz, up=2),
                 lambda: modconv_epilogue(t.cpu(), d.cpu(), b.cpu(), up=2), lambda: modconv_epilogue(t, d, b, up=2, clamp=-1.0)):
        with pytest.raises(RuntimeError):
            call()
