"""Shared by test_disc16_cpu.py and test_gpu_disc16.py: the float64 references of the discriminator's 16-bit path, the comparison rule,
and the case definitions (seeds and shapes), so that the CPU file and the GPU file look at the same tensors.

Two references per case, both float64 on the CPU, built from torch.nn.functional and oracle/ only:
  pure      the operation on the operands the kernel multiplies (activations as given, weights and biases rounded to the 16-bit type);
  emulated  the same graph with a rounding node (``rnd``) wherever the product stores a 16-bit tensor.
``E = relL2(emulated - pure)`` is what rounding alone does; every bar that is not one of the project's own (1.05 ulp of one
rounding, 1e-4 / 2e-4 of fp32 sums) is computed from it (``judge``).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import aten_ops as ops
from oracle import discriminator as odisc

DTYPES = [torch.bfloat16, torch.float16]
ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}       # one rounding of an fp32 sum, relative to the largest binade
ONE_ROUNDING = 1.05           # tests/test_gpu_conv.py test_stride2_conv_equals_the_decimated_stride1_result
FP32_BAR = 1e-4               # tests/test_gpu_conv.py test_scaled_conv_vs_oracle, fp32 row
FP32_BAR_DW = 2e-4            # tests/test_gpu_conv.py _close(dw, ..., 2e-4)
E_FACTOR = 0.25               # relL2(kernel - emulated) <= E / 4 + floor
GOLDEN_FACTOR = 2.0           # relL2(kernel - fp32 golden) <= 2 E
SIGN_SHARE_CAP = 1e-3         # the references alone must disagree on fewer leaky-ReLU branches than this
FILT = [1, 3, 3, 1]
SQH = math.sqrt(0.5)


# ---------------------------------------------------------------------------------------------------------------- rounding
def quantize(x, dtype):
    """float64 -> the 16-bit type -> float64, through float32 (the kernels round fp32 accumulators)."""
    return x.to(torch.float32).to(dtype).to(torch.float64)


class _Round(torch.autograd.Function):
    """y = x rounded to ``dtype``; the backward applies the node itself to the incoming gradient, so it is differentiable any number
    of times and rounds first- and second-order cotangents as the product's 16-bit gradient tensors are rounded."""

    @staticmethod
    def forward(ctx, x, dtype):
        ctx.dtype = dtype
        return quantize(x, dtype)

    @staticmethod
    def backward(ctx, g):
        return _Round.apply(g, ctx.dtype), None


def rnd(x, dtype):
    return _Round.apply(x, dtype)


class _RoundGrad(torch.autograd.Function):
    """The identity whose backward is the rounding node: a value the product never stores (x + b inside bias_act) whose gradient it
    does store (dx, which the bias gradient then sums)."""

    @staticmethod
    def forward(ctx, x, dtype):
        ctx.dtype = dtype
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return _Round.apply(g, ctx.dtype), None


def ste(x, q):
    """The value ``q`` (a rounded x) with the gradient of x: an operand the product rounds without storing a 16-bit gradient."""
    return x + (q - x).detach()


class Lowp:
    """What oracle.discriminator asks of its ``lowp`` argument.  ``emulate=False``: the pure reference (operands rounded, nothing
    else); ``emulate=True``: a rounding node at every tensor the product stores in 16 bit.  ``trace``: every layer's output by prefix."""

    def __init__(self, dtype, emulate):
        self.dtype, self.emulate, self.trace = dtype, emulate, {}

    def store(self, x):
        return rnd(x, self.dtype) if self.emulate else x

    def cast(self, x):
        # x.to(dtype) of a tensor whose gradient comes back as a stored 16-bit tensor
        return rnd(x, self.dtype) if self.emulate else ste(x, quantize(x.detach(), self.dtype))

    def grad(self, x):
        # identity; the gradient that comes back through it is a stored 16-bit tensor
        return _RoundGrad.apply(x, self.dtype) if self.emulate else x

    def weight(self, w, gain):
        # `weight * weight_gain` in fp32, rounded to the activation dtype by the packing kernel; the weight gradient stays fp32
        q = (w.detach().to(torch.float32) * float(gain)).to(self.dtype).to(torch.float64)
        return ste(w * float(gain), q)

    def bias(self, b):
        # bias.to(dtype): the bias gradient is a 16-bit tensor (the fp32 plane sums cast to the activation dtype)
        return self.cast(b)


def references(dtype):
    return Lowp(dtype, False), Lowp(dtype, True)


# ---------------------------------------------------------------------------------------------------------------- comparison
def f64(t):
    return None if t is None else t.detach().to(torch.float64).cpu()


def rel_l2(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def floor_of(name):
    return FP32_BAR_DW if name.split('/')[-1] in ('dw', 'dweight') or name.endswith('weight') else FP32_BAR


def judge(rule, name, k, p, e, dtype, factor=E_FACTOR, floor_norm=None):
    """One quantity by the rule of its group; returns a record (name, rule, E, err, bar, ratio = err / E where that means something).
    rule 'ulp'   a 16-bit tensor that is one node's output from exact operands: max|k - p| <= 1.05 ulp max|p|
         'fp32'  an fp32 tensor from exact 16-bit operands: max|k - p| <= 1e-4 (2e-4: weight gradients) max|p|
         'e4'    downstream of a stored 16-bit tensor: ||k - e|| <= factor ||e - p|| + floor max(||e||, floor_norm)
                 (floor_norm: the norm a tensor of this size would have at the scale of the group's largest tensor)
         'zero'  identically zero in the reference: None or exactly zero."""
    rec = dict(name=name, rule=rule, E=None, ratio=None)
    if rule == 'zero':
        assert p is None or float(p.abs().max()) == 0.0, (name, 'the reference is not identically zero')
        rec.update(err=0.0 if k is None else float(k.abs().max()), bar=0.0)
    elif rule in ('ulp', 'fp32'):
        scale = float(p.abs().max())
        bar = (ONE_ROUNDING * ULP[dtype] if rule == 'ulp' else floor_of(name)) * scale
        rec.update(err=float((k - p).abs().max()), bar=bar)
    else:
        assert rule == 'e4' and 0 < factor <= 1.0
        dist, noise = float((k - e).norm()), float((e - p).norm())
        norm = max(float(e.norm()), floor_norm or 0.0, 1e-300)
        rec.update(E=noise / max(float(p.norm()), 1e-300), err=dist / norm, bar=(factor * noise + floor_of(name) * norm) / norm,
                   ratio=dist / noise if noise > 0 else float('inf'))
    rec['ok'] = rec['err'] <= rec['bar']
    return rec


def chain_rule(p, e, name):
    """The rule of a quantity downstream of stored tensors: 'e4', or 'zero' where both references are identically zero (a leaky
    ReLU has no second derivative: sum g^2 and <g, q> do not depend on a bias)."""
    dead = all(t[name] is None or float(t[name].abs().max()) == 0.0 for t in (p, e))
    return 'zero' if dead else 'e4'


def check(records, what):
    """Print every figure, then assert."""
    for r in records:
        print(f"{what} {r['name']:<28s} {r['rule']:<5s} err {r['err']:.3e} bar {r['bar']:.3e}"
              + (f" E {r['E']:.3e} (k-e)/E {r['ratio']:.3f}" if r['E'] is not None else ''))
    bad = [r for r in records if not r['ok']]
    assert not bad, (what, [(r['name'], r['rule'], r['err'], r['bar'], r['E']) for r in bad])


def summarize(records):
    """(largest E, largest ||k - e|| / ||e - p||) over the records under the E rule -- the figures of DESIGN.md's table."""
    e4 = [r for r in records if r['rule'] == 'e4']
    return (max(r['E'] for r in e4), max(r['ratio'] for r in e4)) if e4 else (None, None)


def sign_share(a, b):
    return float(((a < 0) != (b < 0)).double().mean())


def branch_allowance(p, e):
    """The share of an activation's outputs on which the kernels may take another leaky-ReLU branch than the emulated reference:
    the share on which the two references disagree with each other, never more than SIGN_SHARE_CAP, plus two elements."""
    return min(sign_share(e, p), SIGN_SHARE_CAP) + 2.0 / e.numel()


def check_signs(k, p, e, what, sharp=True):
    """Leaky-ReLU branch decisions at an activation's output, by ``branch_allowance``; returns the number of elements that differ.
    ``sharp``: the references alone are below the cap (every case whose seed is chosen here; not every layer of the golden network)."""
    cap = sign_share(e, p)
    got = sign_share(k, e)
    print(f'{what} branch disagreement: kernel/emulated {got:.3e}, emulated/pure {cap:.3e} of {e.numel()}')
    assert not sharp or cap < SIGN_SHARE_CAP, (what, cap)
    assert got <= branch_allowance(p, e), (what, got, cap)
    return int(round(got * e.numel()))


# ---------------------------------------------------------------------------------------------------------------- inputs
def randn16(shape, dtype, seed, scale=1.0):
    """Seeded N(0, scale^2) float64 values that are representable in ``dtype``."""
    g = torch.Generator().manual_seed(int(seed))
    return quantize(torch.randn(shape, generator=g, dtype=torch.float32).double() * scale, dtype)


def randn32(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(int(seed))
    return (torch.randn(shape, generator=g, dtype=torch.float32) * scale).double()


def r1_quantities(fn, leaves, xname, others, r, q, f32=lambda t: t, x_second=False):
    """Forward y = fn(leaves), the first-order gradients of <y, r> w.r.t. ``xname`` and ``others``, and the R1 pattern:
    g = d<y, r>/dx with create_graph, then the gradients of sum g^2 ('sq/') and of <g, q> ('q/') w.r.t. ``others`` and r.
    ``f32``: the cast the caller of a 16-bit network applies before the loss (``.float()`` on the GPU, nothing in float64).
    ``x_second``: the second-order gradients w.r.t. x too (an op that is not linear in x)."""
    y = fn(leaves)
    names = [xname] + list(others)
    first = torch.autograd.grad((f32(y) * r).sum(), [leaves[n] for n in names], create_graph=True, allow_unused=True)
    out = {'y': y}
    out.update({'d' + n: g for n, g in zip(names, first)})
    g = first[0]
    wrt = ([xname] if x_second else []) + list(others) + ['r']
    targets = [leaves[n] for n in wrt[:-1]] + [r]
    for tag, s in (('sq', f32(g).square().sum()), ('q', (f32(g) * q).sum())):
        second = torch.autograd.grad(s, targets, retain_graph=True, allow_unused=True)
        out.update({f'{tag}/d{n}': t for n, t in zip(wrt, second)})
    return {k: f64(v) for k, v in out.items()}


def both_references(fn, make_leaves, xname, others, r, q, dtype, x_second=False):
    """(pure, emulated, lowp objects): r1_quantities of ``fn(leaves, lowp)`` for the two references."""
    res = []
    lps = references(dtype)
    for lp in lps:
        leaves = {k: v.clone().requires_grad_(True) for k, v in make_leaves().items()}
        res.append(r1_quantities(lambda lv: fn(lv, lp), leaves, xname, others, r.clone().requires_grad_(True), q, x_second=x_second))
    return res[0], res[1], lps


# ---------------------------------------------------------------------------------------------------------------- conv cases
def choose_tile_s2(p, q, patch_max=704):
    """The stride-2 kernel's tile of TH x TW output pixels (csrc/conv2d.hip choose_tile_s2), restated to SELECT shapes: 128 slots,
    a ((TH - 1) 2 + 3) x round4((TW - 1) 2 + 4) patch of at most ``patch_max`` elements, the best share of useful slots."""
    best, tile = -1.0, None
    for tw in range(2, 65, 2):
        th = min(128 // tw, p)
        while th >= 1:
            pwl = ((tw - 1) * 2 + 4 + 3) // 4 * 4
            if ((th - 1) * 2 + 3) * pwl > patch_max:
                th -= 1
                continue
            tiles = -(-p // th) * -(-q // tw)
            score = p * q / (tiles * 128) + 1e-4 * tw + (0.03 if tw % 8 == 0 else 0.0)
            if score > best:
                best, tile = score, (th, tw)
            break
    return tile


def down_out(size):
    """Output size of a 3x3 down=2 layer with padding 1 and the [1, 3, 3, 1] filter: blurred size + 1, stride-2 windows of 3."""
    return (size + 1 - 3) // 2 + 1


# mode 'down3': conv2d_resample 3x3, down 2, [1,3,3,1], padding 1 (blur + _StridedConv2d).  (id, n, cin, cout, h, w, expected tile)
# The expected tile is what choose_tile_s2 gives for the output plane -- asserted in the CPU test, so the list stays what it says.
DOWN3 = [
    ('prod256', 1, 64, 128, 256, 256, (2, 64)),        # production planes at N = 1: blurred widths 258 / 130 / 66 / 34
    ('prod128', 1, 128, 256, 128, 128, (2, 64)),
    ('prod64', 1, 256, 512, 64, 64, (4, 32)),
    ('prod32', 1, 512, 512, 32, 32, (8, 16)),
    ('tw2_ragged_y', 1, 5, 128, 128, 4, (43, 2)),      # tile width 2; 64 rows in tiles of 43; cin below a K block
    ('tw14_ragged_xy', 2, 37, 127, 35, 19, (9, 14)),   # odd input height and width (ey / ex = 0, odd blurred size handled by the crop)
    ('tw64_ragged_y', 1, 16, 129, 6, 128, (2, 64)),    # 3 rows in tiles of 2
    ('tw64_ragged_x', 1, 8, 200, 4, 130, (2, 64)),     # 65 columns in tiles of 64
    ('short_plane', 1, 5, 1, 18, 10, (9, 8)),          # P = 9 below the 16 rows an 8-wide tile could hold; ragged x; cout 1
    ('tw16_ragged_x', 3, 64, 128, 32, 24, (8, 16)),    # 12 columns in a 16-wide tile
    ('odd_blur', 2, 16, 24, 9, 22, (4, 32)),           # odd input height: even blurred height, no extra row; even width: extra column
]

# mode 's2': strided_conv2d called directly (pads 1 and 2 never arise through conv2d_resample).  (id, n, cin, cout, h, w, pad, one_tap)
# one_tap: the backward zero-stuffs with the one-tap up=2 upfirdn2d (fw and dy's width even), else by slice assignment.
S2 = [
    ('p1_onetap_even', 2, 16, 16, 20, 36, 1, True),    # fh 20: fh - 2P = 0
    ('p1_onetap_odd', 1, 37, 40, 21, 36, 1, True),     # fh 21: fh - 2P = -1, a crop in upfirdn2d's trailing padding
    ('p2_onetap_odd', 1, 16, 130, 13, 14, 2, True),    # fw 16, Q 8; fh 15
    ('p0_slice', 2, 32, 64, 34, 36, 0, False),         # fw 34, Q 17
    ('p2_slice', 1, 8, 24, 10, 12, 2, False),          # fw 14, Q 7
]

# modes 'plain3' (3x3 pad 1), 'plain1' (1x1), 'down1' (1x1 + down 2: upfirdn2d first, the skip layer).  (id, mode, n, cin, cout, h, w)
PLAIN = [
    ('conv0_91_130', 'plain3', 1, 91, 130, 20, 34),
    ('conv0_130_37', 'plain3', 2, 130, 37, 18, 66),
    ('fromrgb_5', 'plain1', 2, 5, 24, 32, 32),
    ('1x1_91_130', 'plain1', 1, 91, 130, 12, 20),
    ('skip_130_37', 'down1', 2, 130, 37, 24, 40),
    ('skip_91_130', 'down1', 1, 91, 130, 16, 16),
]

# the gate: odd width (or odd output width) in 16 bit goes to the framework convolution.  (id, mode, n, cin, cout, h, w)
GATE = [
    ('odd_width_3x3', 'plain3', 1, 16, 16, 9, 15),
    ('odd_width_1x1', 'plain1', 2, 8, 12, 6, 7),
]

# _ConvWgrad as a node.  (id, n, cin, cout, ks, h, w, pad): widths of CASES in test_gpu_conv.py -- around the 16-pixel groups and the
# 64-pixel chunks of the weight-gradient kernels
WGRAD = [
    ('q66_pad2', 1, 64, 64, 3, 6, 64, 2),
    ('q100_pad2_n3', 3, 64, 128, 3, 6, 98, 2),
    ('q34_pad1', 1, 64, 96, 3, 20, 34, 1),
    ('q98_pad0', 1, 37, 91, 3, 9, 100, 0),
    ('q150_pad2_n3', 3, 40, 48, 3, 10, 148, 2),
    ('k1_torgb_n3', 3, 64, 1, 1, 32, 32, 0),
    ('k1_q70', 1, 130, 100, 1, 14, 70, 0),
]


def conv_inputs(dtype, seed, n, cin, cout, h, w, ks):
    """x, w (fp32 master weights at the scale Conv2dLayer gives them), and the seeds' cotangents are drawn once the output shape is known."""
    return dict(x=randn16([n, cin, h, w], dtype, seed), w=randn32([cout, cin, ks, ks], seed + 1, 1.0 / (ks * math.sqrt(cin))))


def conv_reference(mode, pad=0):
    """fn(leaves, lowp) -> y for a conv case, as oracle/discriminator.py composes the layer.  ``lowp.cast`` on the (representable) input
    changes no value: it is where the product stores the 16-bit input gradient."""
    filt = odisc.setup_filter(FILT)
    if mode == 's2':
        return lambda lv, lp: lp.store(F.conv2d(lp.cast(lv['x']), lp.weight(lv['w'], 1.0), stride=2, padding=pad))
    ks = 1 if mode.endswith('1') else 3
    down = 2 if mode.startswith('down') else 1
    return lambda lv, lp: odisc.conv2d_resample(lp.cast(lv['x']), lp.weight(lv['w'], 1.0), f=filt if down > 1 else None, down=down, padding=ks // 2, lowp=lp)


def conv_rules(mode):
    """Single node from exact operands: the project's own bars where they apply; a down=2 layer is two nodes: the E rule throughout."""
    if mode in ('down3', 'down1'):
        return {k: 'e4' for k in ('y', 'dx', 'dw', 'sq/dw', 'sq/dr', 'q/dw', 'q/dr')}
    # <g, q> with a representable q: its gradients are again one node from exact operands (wgrad(r, q) and conv(q, w))
    return {'y': 'ulp', 'dx': 'ulp', 'dw': 'fp32', 'sq/dw': 'e4', 'sq/dr': 'e4', 'q/dw': 'fp32', 'q/dr': 'ulp'}


def cotangents(dtype, seed, y_shape, x_shape):
    return randn16(y_shape, dtype, seed + 2), randn16(x_shape, dtype, seed + 3)


def wgrad_reference(ks, pad):
    """dw of a stride-1 correlation as a function of (dy, x): the weight gradient autograd gives F.conv2d, kept differentiable."""
    def fn(dy, x):
        w0 = torch.zeros([dy.shape[1], x.shape[1], ks, ks], dtype=torch.float64, requires_grad=True)
        dw, = torch.autograd.grad((F.conv2d(x, w0, padding=pad) * dy).sum(), w0, create_graph=True)
        return dw
    return fn


# ---------------------------------------------------------------------------------------------------------------- bias_act cases
# (id, shape, act, gain, clamp, with bias).  Vector path: inner size a multiple of 8; element path: not, and the 2-D [N, C] input.
BIAS_ACT = [
    ('lrelu_d_vec', (2, 16, 12, 16), 'lrelu', math.sqrt(2) * SQH, 256 * SQH, True),      # the discriminator's conv1 values
    ('lrelu_d_elem', (3, 7, 5, 6), 'lrelu', math.sqrt(2) * SQH, 256 * SQH, True),
    ('lrelu_bite_vec', (2, 8, 16, 24), 'lrelu', math.sqrt(2), 1.0, True),                 # clamp that bites on the positive side (x + b > 0.71: a quarter of the elements)
    ('lrelu_bite_elem', (3, 5, 7, 9), 'lrelu', math.sqrt(2), 1.0, True),
    ('lrelu_nc', (24, 40), 'lrelu', math.sqrt(2), 1.0, True),
    ('linear_skip_vec', (2, 8, 8, 8), 'linear', SQH, None, False),                        # the skip layer: gain, no bias
    ('linear_skip_elem', (1, 3, 5, 7), 'linear', SQH, None, False),
    ('swish_vec', (2, 6, 10, 12), 'swish', math.sqrt(2), 1.5, True),                      # a real second derivative: grad = 2 mode, _SumPlanes
    ('swish_elem', (3, 5, 7, 9), 'swish', math.sqrt(2), None, True),
    ('swish_nc', (24, 40), 'swish', math.sqrt(2), 1.5, True),
]
MARGIN_ULPS = 4


def bias_act_margins(x, b, act, gain, clamp, dtype):
    """(elements whose x + b lies within 4 ulp of |x| of the kink, elements whose |y| lies within 4 ulp of the clamp)."""
    shape = [1, -1] + [1] * (x.ndim - 2)
    z = x + (b.reshape(shape) if b is not None else 0.0)
    kink = (z.abs() < MARGIN_ULPS * ULP[dtype] * x.abs().clamp_min(1e-30)) if act == 'lrelu' else torch.zeros_like(x, dtype=torch.bool)
    edge = torch.zeros_like(kink)
    if clamp is not None:
        y = ops.bias_act(x, b, act=act, gain=gain)
        edge = (y.abs() - clamp).abs() < MARGIN_ULPS * ULP[dtype] * clamp
    return kink, edge


def bias_act_inputs(case, dtype):
    """x, b (both representable) built so that no element sits within the margins of the leaky-ReLU kink or of the clamp: offenders
    are MOVED (x + 1/2 near the kink, x / 2 near the clamp), never dropped.  The caller asserts the margins."""
    cid, shape, act, gain, clamp, with_b = case
    seed = 100 + [c[0] for c in BIAS_ACT].index(cid)
    x = randn16(shape, dtype, seed)
    b = randn16([shape[1]], dtype, seed + 1, 0.3) if with_b else None
    for _ in range(8):
        kink, edge = bias_act_margins(x, b, act, gain, clamp, dtype)
        if not bool(kink.any() or edge.any()):
            break
        x = quantize(torch.where(kink, x + 0.5, torch.where(edge, x * 0.5, x)), dtype)
    return x, b


def bias_act_reference(case):
    _, _, act, gain, clamp, _ = case

    def fn(lv, lp):
        # the bias is added in fp32 inside the kernel (no rounding of x + b); bias_act's dx is stored, and db is the sum of that tensor
        z = lp.cast(lv['x'])
        if 'b' in lv:
            z = lp.grad(z + lp.bias(lv['b']).reshape([1, -1] + [1] * (z.ndim - 2)))
        return lp.store(ops.bias_act(z, None, act=act, gain=gain, clamp=clamp))
    return fn


def bias_act_rules(case):
    """y, dx, and the gradients of <g, q> are one launch from exact operands; bias gradients sum STORED 16-bit tensors; sum g^2
    differentiates a stored g.  Leaky ReLU and the linear layer have no second derivative w.r.t. x and b."""
    _, _, act, _, _, with_b = case
    smooth = act == 'swish'
    rules = {'y': 'ulp', 'dx': 'ulp', 'sq/dr': 'e4', 'q/dr': 'ulp', 'sq/dx': 'e4' if smooth else 'zero', 'q/dx': 'ulp' if smooth else 'zero'}
    if with_b:
        rules.update({'db': 'e4', 'sq/db': 'e4' if smooth else 'zero', 'q/db': 'e4' if smooth else 'zero'})
    return rules


# ---------------------------------------------------------------------------------------------------------------- upfirdn2d cases
# (id, shape, up, down, padding [px0, px1, py0, py1], one-tap filter instead of [1,3,3,1] x [1,3,3,1])
UPFIRDN = [
    ('skip_down2', (2, 6, 16, 24), 1, 2, [1, 1, 1, 1], False),            # the skip layer's decimation
    ('skip_down2_odd', (1, 5, 13, 18), 1, 2, [1, 1, 1, 1], False),
    ('blur_even', (2, 4, 16, 32), 1, 1, [2, 3, 2, 3], False),             # the blur before the stride-2 conv: [2, 2 + ex, 2, 2 + ey]
    ('blur_odd', (1, 6, 9, 21), 1, 1, [2, 2, 2, 2], False),
    ('blur_mixed', (1, 3, 9, 22), 1, 1, [2, 3, 2, 2], False),
    ('stuff_even', (2, 5, 10, 18), 2, 1, [0, 0, 0, 0], True),             # zero-stuffing of _StridedConv2d.backward: fh - 2P = 0
    ('stuff_crop', (1, 7, 11, 8), 2, 1, [0, 0, 0, -1], True),             # ... = -1: a crop of the last row
]


def upfirdn_filter(one_tap):
    return torch.ones([1, 1], dtype=torch.float32) if one_tap else torch.outer(odisc.setup_filter(FILT), odisc.setup_filter(FILT))


def upfirdn_reference(case):
    _, _, up, down, padding, one_tap = case
    f = upfirdn_filter(one_tap)
    return lambda lv, lp: lp.store(ops.upfirdn2d(lp.cast(lv['x']), f, up=up, down=down, padding=padding))


def upfirdn_rules(case):
    """Linear: d<g, q>/dr is the forward op on q.  The one-tap zero-stuffing only copies: nothing is rounded, E would be zero, and
    every result is held to the single-launch bar."""
    return {'y': 'ulp', 'dx': 'ulp', 'sq/dr': 'ulp' if case[5] else 'e4', 'q/dr': 'ulp'}


# ---------------------------------------------------------------------------------------------------------------- blocks, network
# (id, n, in_channels (0: first block, fromrgb from a 5-channel image), tmp_channels, out_channels, resolution)
BLOCKS = [
    ('tiny_first', 3, 0, 8, 16, 32),
    ('tiny_inner', 3, 8, 8, 16, 32),
    ('prod_inner', 1, 64, 64, 128, 64),          # production width at a reduced plane
    ('prod_first', 1, 0, 64, 128, 64),
]
BLOCK_CLAMP = 256
BLOCK_LAYERS = ('fromrgb', 'conv0', 'conv1')     # the layers with an activation (skip is linear)


# seeds: chosen so that the two references alone disagree on fewer than SIGN_SHARE_CAP of the leaky-ReLU branches at every activation
# (asserted in test_disc16_cpu.py); 310 put tiny_inner's conv1 in bfloat16 at 1.06e-3
BLOCK_SEEDS = {'tiny_first': 300, 'tiny_inner': 410, 'prod_inner': 320, 'prod_first': 330}


def block_state(case):
    """The block's parameters as float64 copies of fp32 values: N(0, 1) weights (the initialisation) and 0.3 N(0, 1) biases."""
    cid, n, cin, tmp, cout, res = case
    seed = BLOCK_SEEDS[cid]
    sd = {}
    if cin == 0:
        sd['fromrgb.weight'], sd['fromrgb.bias'] = randn32([tmp, 5, 1, 1], seed), randn32([tmp], seed + 1, 0.3)
    sd['conv0.weight'], sd['conv0.bias'] = randn32([tmp, tmp, 3, 3], seed + 2), randn32([tmp], seed + 3, 0.3)
    sd['conv1.weight'], sd['conv1.bias'] = randn32([cout, tmp, 3, 3], seed + 4), randn32([cout], seed + 5, 0.3)
    sd['skip.weight'] = randn32([cout, tmp, 1, 1], seed + 6)
    return sd


def block_input(case, dtype):
    cid, n, cin, tmp, cout, res = case
    seed = BLOCK_SEEDS[cid]
    return randn16([n, cin or 5, res, res], dtype, seed + 7)


def block_reference(case):
    first = case[2] == 0

    def fn(lv, lp):
        sd = {'b.' + k: v for k, v in lv.items() if k != 'x'}
        lp.trace.clear()
        return odisc.discriminator_block(sd, 'b.', None if first else lv['x'], lv['x'] if first else None, conv_clamp=BLOCK_CLAMP, lowp=lp)
    return fn


NETWORK = 'D2_tiny128_clamp'
NETWORK_FP16_RES = 3

def network_state(g):
    return {k[3:]: torch.from_numpy(np.array(v)).double() for k, v in g.items() if k.startswith('sd/')}


def network_quantities(D, params, fake, real, f32=lambda t: t):
    """The discriminator half of the step and the generator's term through D (oracle.discriminator.d_losses' composition), for any
    callable ``D(img) -> logits`` and dict of parameter leaves: logits, the R1 image gradient, and per parameter tensor the gradients
    of the R1 term, of the real term and of the fake term; the image gradient of the G term."""
    names = list(params)
    out = {}
    gen_logits = f32(D(fake))
    out['gen_logits'] = gen_logits
    dense = lambda k, t: torch.zeros_like(params[k]) if t is None else t            # a parameter the term does not reach
    for k, t in zip(names, torch.autograd.grad(F.softplus(gen_logits).mean(), [params[k] for k in names], allow_unused=True)):
        out['gfake/' + k] = dense(k, t)
    real_tmp = real.detach().clone().requires_grad_(True)
    real_logits = f32(D(real_tmp))
    out['real_logits'] = real_logits
    r1, = torch.autograd.grad([real_logits.sum()], [real_tmp], create_graph=True)
    out['r1_grads'] = r1
    loss_r1 = f32(r1).square().sum([1, 2, 3]).mean() * 0.5
    for k, t in zip(names, torch.autograd.grad(loss_r1, [params[k] for k in names], retain_graph=True, allow_unused=True)):
        out['gr1/' + k] = dense(k, t)
    for k, t in zip(names, torch.autograd.grad(F.softplus(-real_logits).mean(), [params[k] for k in names], allow_unused=True)):
        out['greal/' + k] = dense(k, t)
    img = fake.detach().clone().requires_grad_(True)
    out['g_img'], = torch.autograd.grad(F.softplus(-f32(D(img))).mean(), img)
    return {k: f64(v) for k, v in out.items()}


def network_references(g, dtype):
    """(pure, emulated, lowp objects) of ``network_quantities`` for the golden network with its highest-resolution blocks in ``dtype``."""
    res, n, cb, cm, group, clamp = [int(v) for v in g['meta']]
    fake, real = torch.from_numpy(g['fake']).double(), torch.from_numpy(g['real']).double()
    names = [str(k) for k in g['names']]
    out = []
    lps = references(dtype)
    for lp in lps:
        sd = network_state(g)
        params = {k: sd[k].requires_grad_(True) for k in names}
        lp.passes = []                                                 # the traces of the fake, real and G-term passes, in this order

        def D(img, sd=sd, lp=lp):
            y = odisc.discriminator(sd, img, res, mbstd_group_size=group, conv_clamp=clamp, lowp=lp, num_fp16_res=NETWORK_FP16_RES)
            lp.passes.append(dict(lp.trace))
            return y
        out.append(network_quantities(D, params, fake, real))
    return out[0], out[1], lps


# The branch condition of the network test is asserted at EVERY activation of the network (fp32 blocks included) in all three passes
# (0: fake image, 1: real image, 2: the G term's fake image), with the allowance bounded by SIGN_SHARE_CAP everywhere.  In the golden
# network the two bfloat16 references alone disagree on MORE than the cap at the layers below (share in 1e-3; rounding accumulated
# over 4 .. 14 stored tensors, and 4 of b8.conv0's 1536 outputs are 2.6e-3), which is why the allowance is min(share, cap) and not
# the share; float16 stays below the cap everywhere (at most 0.65e-3, one of b16.conv1's 1536 outputs).  test_disc16_cpu.py asserts
# this table.
NETWORK_WIDE = {
    torch.bfloat16: {(0, 'b128.conv1.'): 1.01, (0, 'b64.conv0.'): 1.68, (0, 'b64.conv1.'): 1.38, (0, 'b32.conv0.'): 1.14, (0, 'b16.conv0.'): 1.30,
                     (0, 'b8.conv0.'): 2.60, (1, 'b64.conv0.'): 1.38, (1, 'b64.conv1.'): 1.02, (1, 'b32.conv0.'): 1.63},
    torch.float16: {},
}
NETWORK_WIDE[torch.bfloat16].update({(2, k): v for (n, k), v in list(NETWORK_WIDE[torch.bfloat16].items()) if n == 0})   # the same image

# The factor of the E rule for the network: E / 4, except for the gradients that pass through an activation at which kernels and
# emulated reference take different branches (within the branch condition); those get 1, the ceiling -- for this cause: the golden
# network's deep layers are tiny (b16.conv0: 6144 outputs), and ONE element on the other side of a leaky-ReLU kink scales its
# 3 x 3 x C gradient patch by 5.  Measured, float16: the forward results agree to 2.5e-4, two of b16.conv0's 6144 outputs (both
# references put them within rounding of 0) take the other branch in the real pass, the gradient entering that activation then
# differs by 5.3e-2 and the R1 image gradient by 1.5e-2 = 0.65 E, while every tensor of the backward pass agrees to fp32 accuracy
# up to that activation.  bfloat16: no element flips, and the R1 image gradient is 0.008 E from the emulated reference.
BRANCH_FLIP_FACTOR = 1.0
_STAGES = {'fromrgb': 0, 'skip': 1, 'conv0': 1, 'conv1': 2, 'conv': 0, 'fc': 1, 'out': 2}


def _passes_through(layer, flipped):
    """Does the cotangent that reaches ``layer``'s pre-activation pass through the activation of ``flipped`` (both 'b64.conv0.')?
    Blocks run b128, b64, ..., b4; inside a block fromrgb -> (skip | conv0 -> conv1); the skip layer is linear and bypasses conv0 / conv1."""
    (bl, sl), (bf, sf) = (x.rstrip('.').split('.') for x in (layer, flipped))
    if bl != bf:
        return int(bf[1:]) < int(bl[1:])                 # a later (lower-resolution) block
    if sl == 'skip':
        return False
    return _STAGES[sf] >= _STAGES[sl]


def network_factor(name, flipped):
    """E-rule factor of one network quantity, given ``flipped[pass]`` = the activations at which a branch decision differed.
    Logits are continuous in the pre-activations: always E / 4.  First-order gradients (pass 0: gfake/*; 1: greal/*; 2: g_img): the
    ceiling only where the cotangent passes through a flipped activation.  The R1 term differentiates the whole backward pass of
    pass 1: any flip there reaches all of gr1/* and r1_grads."""
    group, _, tensor = name.partition('/')
    if group in ('gen_logits', 'real_logits'):
        return E_FACTOR
    n_pass = {'gfake': 0, 'greal': 1, 'gr1': 1, 'r1_grads': 1, 'g_img': 2}[group]
    if group in ('gr1', 'r1_grads', 'g_img'):            # the image's cotangent passes through every activation
        hit = bool(flipped[n_pass])
    else:
        layer = tensor.rsplit('.', 1)[0] + '.'
        hit = any(_passes_through(layer, f) for f in flipped[n_pass])
    return BRANCH_FLIP_FACTOR if hit else E_FACTOR


def group_norms(e, prefix):
    """floor_norm per tensor of a group of parameter gradients: the norm a tensor of its size has at the RMS of the group's largest."""
    keys = [k for k in e if k.startswith(prefix)]
    rms = max(float(e[k].norm()) / math.sqrt(e[k].numel()) for k in keys)
    return {k: rms * math.sqrt(e[k].numel()) for k in keys}
