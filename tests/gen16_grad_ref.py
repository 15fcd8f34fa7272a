"""End-to-end gradients of the 16-bit generator: the float64 reference, its storage-rounded twin (the yardstick) and the criterion
(test-only; no GPU).  Used by tests/test_gpu_generator_grad16.py; tests/test_gen16_grad_ref_cpu.py proves without a GPU that the
criterion has teeth.

What is graded.  The tiny 128^2 generator of tests/test_gpu_generator_configs.py (TINY, oracle.generator.random_state_dict(seed=0),
inputs from torch.Generator().manual_seed(1)) in the cases of CASES; the loss is (y * r).sum().  For the output and for every
parameter k

    err(g, ref) = |g - ref| / max(|ref|, 1e-6 sqrt(numel))          (L2 norms; the floor of the fp32 end-to-end tests)

with `ref` the exact float64 oracle ON THE SAME leaky-ReLU / clamp branch decisions as the run being graded (codes imposed,
oracle.aten_ops.filtered_lrelu; oracle.generator._plain_lrelu for the bottleneck's two plain leaky ReLUs, PLAIN): a pre-activation
within rounding distance of a kink that takes the other branch is a property of the rounding, not of the wiring, and is held separately
(branch_report).

The yardstick.  Y[k] = err of the STORAGE-ROUNDED oracle: the same float64 program with a straight-through rounding to the 16-bit type
(values on the way forward, cotangents on the way back) at every tensor a 16-bit implementation keeps in 16 bits --
oracle.generator.synthesis(store=...): the padded input image, every conv output, every filtered_lrelu output after the skip add.  All
arithmetic between two stores stays float64, so Y is what ONE rounding per stored tensor costs end to end; nothing in it comes from the
code under test.  The run under test passes when

    err_dev[k] <= MARGIN * max(Y[k], median_k Y)   for every parameter k,      err_dev[output] <= MARGIN * Y[output]

MARGIN = 4: the device also rounds the pre-scaled copy of an activation and the per-plane factors -- under 2x in quadrature -- and a
further 2x covers the draw-to-draw spread of the 8- and 32-element tensors of the tiny network.  The median term keeps a parameter
whose own yardstick happens to be small on one draw (a 1-element bias) from being held tighter than the typical parameter.  (The output
has no such neighbours: it is held to its own yardstick alone, the stricter reading.)

Stores added after the first measurement on the MI355X (is_internal; `storage(dtype, internal=False)` is the list above alone).  With
the HBM tensors alone the device stood at 5 - 45 x Y on most of the network.  Two causes, neither in the wiring:
  * the plain leaky ReLUs of e_16x16 and fc_in keep no sign tensor, so their decisions were not imposed: fc_in has 1024 outputs per
    sample, and ONE of them on the other branch moves every gradient upstream of it (fc_in, e_16x16, the encoder below the skips) by
    2 % relative L2 -- in f16 as in bf16.  They are imposed now, read off the device's stored outputs the way its backward reads
    them (y > 0: an f16 output that underflowed to 0 takes the slope; tests/test_gpu_generator_grad16.py);
  * 16-bit values the kernels verifiably form that the list lacked: inside filtered_lrelu x + b, the result of the first pass of
    each filter, the pre-activation, the activation and both coefficient sets (csrc/filtered_lrelu_mfma.hip, filtered_lrelu_wave.hip;
    the list "every quantity a kernel family stores in 16 bits" of tests/flrelu_exact_ref.py), the conv weights as the matrix units
    read them (fused_layer.py: conv2d.pack_weights_both(w, x.dtype); value only, their gradient stays fp32), and e_16x16's activation
    (networks_stylegan3.Conv2dLayer.forward: bias_act on the 16-bit conv output).

Measured on the CPU, default, batch 2, the oracle's own codes imposed (Y median / Y max over the parameters / output relative L2):
    HBM tensors alone    bf16 1.3e-2 / 5.9e-2 (encoder_13.bias) / 5.8e-3     f16 9.2e-4 / 8.4e-3 (L0_36_8.weight) / 7.2e-4
    with the additions   bf16 1.7e-2 / 9.0e-2 (L1_36_8.weight)  / 1.1e-2     f16 2.4e-3 / 1.1e-2 (L5_52_8.bias)   / 2.5e-3
clamp1 (conv_clamp 1: 10 of the 29 layers clamp, up to 14 % of a layer's elements), HBM tensors alone:
                         bf16 2.8e-3 / 1.4e-2 / 5.3e-3                       f16 7.6e-4 / 6.0e-3 / 6.6e-4
The f16 maximum of the HBM-only yardstick sits on the 36^2 / 52^2 decoder layers L0 - L3.  It is NOT cotangent underflow: rounding
the cotangents alone (values exact) gives 1.2e-2 there, and scaling the cotangents by 4096 before the rounding (and back after)
moves the maximum from 8.4e-3 to 7.9e-3 only.  It is the ordinary 11-bit rounding of cotangents whose few large entries (4e-2 against a
median of 1e-4 on those layers) enter weight-gradient sums that cancel.
"""
import functools
import math

import numpy as np
import torch

import flrelu_read_ref as R
from oracle import generator as ogen
from test_gpu_generator_configs import CONFIGS, TINY

MARGIN = 4.0
DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16}

# case -> (configuration of test_gpu_generator_configs.CONFIGS, batch, further synthesis overrides)
CASES = {
    'default-b2': ('default', 2, {}),
    'default-b3': ('default', 3, {}),       # 8 of the 14 weight gradients have a split count that is no multiple of 3: their <g, z> comes from plane_dot
    'nocond-b2': ('nocond', 2, {}),
    'margin11-b2': ('margin11', 2, {}),
    'w36-b2': ('w36', 2, {}),
    'clamp1-b2': ('default', 2, dict(conv_clamp=1.0)),
}


@functools.lru_cache(maxsize=None)
def setup(case):
    """(plan, state dict, (z, c, x, r), (z_dim, c_dim, w_dim), synthesis kwargs) of a case; shared, never modified."""
    name, batch, extra = CASES[case]
    z_dim, c_dim, w_dim, over = CONFIGS[name]
    skw = dict(TINY, **over)
    skw.update(extra)
    pl = ogen.plan(128, 4, 1, {k: v for k, v in skw.items() if k not in ('use_radial_filters', 'magnitude_ema_beta')})
    sd = ogen.random_state_dict(pl, z_dim, c_dim, w_dim, 2, seed=0)
    g = torch.Generator().manual_seed(1)
    z = torch.randn(batch, z_dim, generator=g)
    c = torch.rand(batch, c_dim, generator=g) if c_dim else None
    x = torch.randn(batch, 4, 128, 128, generator=g)
    r = torch.randn(batch, 1, 128, 128, generator=g)
    return pl, sd, (z, c, x, r), (z_dim, c_dim, w_dim), skw


def param_names(sd):
    """The state dict's trainable entries, in its order (the buffers are the magnitude EMAs and w_avg)."""
    return [k for k in sd if not k.endswith('magnitude_ema') and k != 'mapping.w_avg']


def layers(pl):
    return pl['enc'] + pl['dec']


# the bottleneck's two plain leaky ReLUs (bias_act, no sign tensor): their branch decisions are imposed too, read off the device's
# stored outputs as its backward reads them (positive branch where y > 0).  fc_in has 1024 outputs per sample: ONE flipped decision
# there moves the gradient of everything upstream of it (fc_in, e_16x16, the encoder below the skips) by 2 % relative L2.
PLAIN = ('e_16x16', 'fc_in')


def activation(L):
    """(gain, slope) of a layer's leaky ReLU."""
    return (1.0, 1.0) if L.get('torgb', False) else (math.sqrt(2), 0.2)


# ------------------------------------------------------------------------------------------------- interventions at the stores
class _Round(torch.autograd.Function):
    """Straight-through rounding to `dtype`: the value forward, the cotangent backward."""

    @staticmethod
    def forward(ctx, x, dtype):
        ctx.dtype = dtype
        return x.to(dtype).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dtype).to(g.dtype), None


class _ScaleCotangent(torch.autograd.Function):
    """Identity forward; the cotangent times s backward: one deliberate wiring error (a wrong per-plane factor on one arm)."""

    @staticmethod
    def forward(ctx, x, s):
        ctx.s = s
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.s, None


class _RoundValue(torch.autograd.Function):
    """Rounding to `dtype` forward, identity backward: a weight packed to 16 bits whose gradient stays fp32."""

    @staticmethod
    def forward(ctx, x, dtype):
        return x.to(dtype).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g, None


def is_internal(name):
    """Stores the yardstick gained after the first measurement on the device (module docstring): inside filtered_lrelu, e_16x16's
    activation, the packed conv weights."""
    return '.flr.' in name or name == 'e_16x16' or name.endswith('.weight')


def storage(dtype, internal=True):
    """The `store` of the storage-rounded oracle.  ``internal=False``: the HBM activation tensors alone (input, conv outputs, layer
    outputs)."""
    def store(x, name):
        if is_internal(name) and not internal:
            return x
        return (_RoundValue if name.endswith('.weight') else _Round).apply(x, dtype)
    return store


def cotangent_error(at, s):
    """A `store` that leaves every tensor alone and multiplies the cotangent entering the tensor named `at` by s."""
    return lambda x, name: _ScaleCotangent.apply(x, s) if name == at else x


# ------------------------------------------------------------------------------------------------- the oracle runs
def run_oracle(case, codes=None, store=None, preact=None, grads=True):
    """One float64 run of a case -> {'output': y, parameter name: gradient of (y * r).sum() or None}."""
    pl, sd, (z, c, x, r), _, _ = setup(case)
    names = param_names(sd)
    osd = {k: v.double() for k, v in sd.items()}
    for k in names:
        osd[k].requires_grad_(grads)
    with torch.set_grad_enabled(grads):
        y = ogen.generator(osd, pl, z.double(), None if c is None else c.double(), x.double(), mapping_layers=2, codes=codes,
                           preact=preact, store=store)
    out = {'output': y.detach()}
    if grads:
        gs = torch.autograd.grad((y * r.double()).sum(), [osd[k] for k in names], allow_unused=True)
        out.update(zip(names, gs))
    return out


# ------------------------------------------------------------------------------------------------- branch decisions
def own_codes(pl, preact):
    """The 2-bit codes a kernel would write for the oracle's own pre-activations (`preact` as oracle.generator fills it): 1 = negative
    branch, 2 = clamped (the kernels write 2, never 3, for a clamped element of either sign).  A pre-activation of exactly 0 -- the
    zero padding of a layer without bias -- gets the negative branch: that is the derivative aten's leaky_relu takes there (the
    kernels take the positive one; the value is 0 either way), so that imposing these codes changes nothing at all."""
    out = {}
    for L in layers(pl):
        u = preact[L['name']][0]
        gain, slope = activation(L)
        neg = u <= 0
        v = (u * torch.where(neg, slope, 1.0) * gain).abs()
        out[L['name']] = torch.where(v > pl['conv_clamp'], 2, neg.to(torch.int64)).to(torch.uint8)
    for k in PLAIN:
        out[k] = (preact[k][0] <= 0).to(torch.uint8)
    return out


def codes_from_signs(pl, records):
    """[(sign tensor, layout)] of the sign-writing filtered_lrelu calls of one forward, in layer order -> the oracle's `codes=`."""
    names = [L['name'] for L in layers(pl)]
    assert len(records) == len(names), f'{len(records)} sign-writing calls for {len(names)} layers'
    return {k: torch.from_numpy(np.ascontiguousarray(R.decode_codes(np.asarray(s), layout))) for k, (s, layout) in zip(names, records)}


def branch_report(pl, codes, pre_own, pre_exact, pre_round):
    """Per layer (name, decisions that differ, of those outside the allowance).  `codes`: the run under test; `pre_own`: the exact oracle's
    pre-activations on its own decisions; `pre_exact` / `pre_round`: the exact and the storage-rounded oracle's with `codes` imposed.  A
    code may differ from the oracle's own decision only where the oracle's pre-activation lies within 4 x max |pre_round - pre_exact| of
    that layer from the kink -- from 0, or from the value at which the activation reaches the clamp."""
    rows = []
    for L in layers(pl):
        u = pre_own[L['name']][0]
        cd = codes[L['name']]
        hh, ww = min(u.shape[2], cd.shape[2]), min(u.shape[3], cd.shape[3])
        assert (hh, ww) == tuple(u.shape[2:]), f'{L["name"]}: codes {tuple(cd.shape)} do not cover the {tuple(u.shape)} grid'
        cd = cd[:, :, :hh, :ww]
        gain, slope = activation(L)
        tol = MARGIN * float((pre_round[L['name']][0] - pre_exact[L['name']][0]).abs().max())
        neg = u < 0
        knee = pl['conv_clamp'] / (gain * torch.where(neg, slope, 1.0))          # |u| at which the activation reaches the clamp
        own_clamped = u.abs() > knee
        dev_clamped = (cd & 2) != 0
        diff = dev_clamped != own_clamped
        near = (u.abs() - knee).abs() <= tol
        if slope != 1.0:                                                         # (ToRGB: both branches are the same function)
            diff |= ~dev_clamped & ~own_clamped & (((cd & 1) != 0) != neg)
            near |= u.abs() <= tol
        rows.append((L['name'], int(diff.sum()), int((diff & ~near).sum())))
    for k in PLAIN:
        u = pre_own[k][0]
        tol = MARGIN * float((pre_round[k][0] - pre_exact[k][0]).abs().max())
        diff = (codes[k] != 0) != (u < 0)
        rows.append((k, int(diff.sum()), int((diff & (u.abs() > tol)).sum())))
    return rows


# ------------------------------------------------------------------------------------------------- the criterion
def err(g, ref):
    g, ref = g.detach().double().cpu(), ref.detach().double().cpu()
    return float((g - ref).norm()) / max(float(ref.norm()), 1e-6 * math.sqrt(ref.numel()))


def grade(got, exact, yard):
    """-> (passed, worst err_dev / Y, table) for a run `got` against the exact oracle and the storage-rounded oracle (all three dicts
    of run_oracle's form, on the same codes).  The table has one (key, err_dev, Y, bound) per graded tensor -- the output and every
    parameter the oracle has a gradient for; a parameter has a gradient in `got` exactly where it has one in `exact`."""
    keys = [k for k in exact if k != 'output']
    for k in keys:
        assert (got[k] is None) == (exact[k] is None), f'{k}: gradient {"missing" if got[k] is None else "present"}, the oracle\'s is not'
        assert (yard[k] is None) == (exact[k] is None), k
    keys = [k for k in keys if exact[k] is not None]
    Y = {k: err(yard[k], exact[k]) for k in ['output'] + keys}
    med = float(np.median([Y[k] for k in keys]))
    table = [('output', err(got['output'], exact['output']), Y['output'], MARGIN * Y['output'])]
    table += [(k, err(got[k], exact[k]), Y[k], MARGIN * max(Y[k], med)) for k in keys]
    passed = all(e <= bound for _, e, _, bound in table)
    worst = max(e / max(y, 1e-300) for _, e, y, _ in table)
    return passed, worst, table


def format_table(table):
    return '\n'.join(f'{k:40s} err {e:.3e}  Y {y:.3e}  ratio {e / max(y, 1e-300):6.2f}  bound {b:.3e}{"" if e <= b else "   <-- over"}'
                     for k, e, y, b in table)
