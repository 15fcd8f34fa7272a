"""Integer-valued operands and the float64 reference for the exact conv2d tests (test_conv_exact_ref_cpu.py, test_gpu_conv_exact.py).

Every conv2d kernel multiplies exactly (16-bit x 16-bit products, or fp32 MFMA) and accumulates in fp32.  With operands that are small
integers times powers of two, every partial sum of every summation order is a multiple of one power of two q and smaller than
2^24 q, hence exact: K-chunking, split-K slabs, split-operand terms and the persistent loop cannot change a bit, and the result
equals the float64 one.  So each element has ONE right answer and the GPU tests compare with ``torch.equal``.

The conditions that make this true are conditions on the INPUTS, checked here on the float64 reference and never on the code under
test (``Node.check``): every tensor the chain stores in 16 bits is representable in that type, and the sum of the absolute values of the
terms of every fp32 sum, counted in units of q, stays below 2^24.  A draw that fails them is redrawn from the next seed, then from
the next narrower operand set (``make_node``; a case that no draw satisfies is an error, the conditions are never relaxed).
No GPU, no library needed -- except for the plan queries at the end, which are pure host calls.
"""
import collections
import ctypes

import torch
import torch.nn.functional as F

LIMIT = float(1 << 24)
F64 = torch.float64


# ---- operand makers --------------------------------------------------------------------------------------------------------------
def gen(seed):
    g = torch.Generator()
    g.manual_seed(int(seed))
    return g


def pick(shape, values, g):
    """A dense float64 tensor of values drawn uniformly from ``values``."""
    v = torch.tensor([float(t) for t in values], dtype=F64)
    return v[torch.randint(0, len(values), tuple(shape), generator=g)]


def pm1(shape, g):
    """Dense +-1: every term of a sum over them is odd, so a dropped or doubled term flips the parity of the sum."""
    return pick(shape, (-1, 1), g)


def pow2(shape, exponents, g):
    return pick(shape, [2.0 ** e for e in exponents], g)


# ---- conditions on the inputs -----------------------------------------------------------------------------------------------------
def representable(t, dtype):
    """Is every element of the float64 tensor ``t`` a value of ``dtype``?"""
    return bool((t.to(dtype).double() == t).all())


def quantum(t):
    """The largest power of two (up to 2^8) that divides every element of ``t``."""
    for e in range(8, -41, -1):
        u = t / 2.0 ** e
        if bool((u == u.round()).all()):
            return 2.0 ** e
    raise AssertionError('not a tensor of small dyadic numbers')


def dot_units(a, b, terms):
    """Upper bound, in units of the products' quantum, of the absolute sum of ``terms`` products a * b: below 2^24 every fp32 partial
    sum of every order is exact."""
    return terms * float(a.abs().max()) * float(b.abs().max()) / (quantum(a) * quantum(b))


def plane_dot_units(a, b):
    """The largest per-plane absolute sum of a * b over H, W, in units of the products' quantum."""
    return float((a.abs() * b.abs()).sum([2, 3]).max()) / (quantum(a) * quantum(b))


# ---- the float64 reference ----------------------------------------------------------------------------------------------------------
def conv_ref(x, w, s=None, d=None, b=None, pad=0, stride=1):
    """y = d * conv(w, s * x) + b on float64 tensors (s [N, I], d [N, O], b [O]; None: absent)."""
    xs = x if s is None else x * s[:, :, None, None]
    y = F.conv2d(xs, w, padding=pad, stride=stride)
    if d is not None:
        y = y * d[:, :, None, None]
    if b is not None:
        y = y + b[None, :, None, None]
    return y


def conv_units(x, w, s=None, d=None, b=None, pad=0, stride=1):
    """The absolute sum behind the largest element of ``conv_ref`` (accumulation, scaling and bias), in units of its quantum."""
    a = conv_ref(x.abs(), w.abs(), None if s is None else s.abs(), None if d is None else d.abs(), None if b is None else b.abs(), pad, stride)
    xs = x if s is None else x * s[:, :, None, None]
    q = quantum(xs) * quantum(w) * (1.0 if d is None else quantum(d))
    if b is not None:
        q = min(q, quantum(b))
    return float(a.max()) / q


class Node:
    """Operands, cotangent and float64 results of one conv node  y = d * conv(w, s * x) + b  (stride 1 or 2).  ``grads`` False: the
    forward only."""

    def __init__(self, x, w, s, d, b, dy_of, pad, stride=1, grads=True):
        self.pad, self.stride, self.grads = pad, stride, grads
        self.x, self.w, self.s, self.d, self.b = x, w, s, d, b
        leaves = {k: v.clone().requires_grad_(grads) for k, v in dict(x=x, w=w, s=s, d=d).items() if v is not None}
        xs = leaves['x'] if s is None else leaves['x'] * leaves['s'][:, :, None, None]
        c = F.conv2d(xs, leaves['w'], padding=pad, stride=stride)
        y = c if d is None else c * leaves['d'][:, :, None, None]
        if b is not None:
            y = y + b[None, :, None, None]
        self.xs, self.c, self.y = xs.detach(), c.detach(), y.detach()
        if not grads:
            return
        self.dy = dy_of(self.y.shape)
        self.dys = self.dy if d is None else self.dy * d[:, :, None, None]
        names = list(leaves)
        grads = torch.autograd.grad((y * self.dy).sum(), [leaves[k] for k in names] + ([xs] if s is not None else []))
        g = dict(zip(names + ['xs'], grads))
        self.dx, self.dw, self.ds, self.dd = g['x'], g['w'], g.get('s'), g.get('d')
        self.dxs = g.get('xs', self.dx)                # gradient with respect to the product s * x (prescaled=True)

    def forward_variants(self):
        """{(scaled, biased): y} for every combination of the output scale and the bias on the same accumulators."""
        out = {}
        for sc in ((False, True) if self.d is not None else (False,)):
            for bi in ((False, True) if self.b is not None else (False,)):
                y = self.c * self.d[:, :, None, None] if sc else self.c
                out[(sc, bi)] = y + self.b[None, :, None, None] if bi else y
        return out

    def failures(self, dtype, need=('y', 'dx', 'dw', 'ds', 'dd')):
        """What of this node is not exact in ``dtype`` arithmetic (empty: every result in ``need`` has one right answer per element).
        'y': the forward with and without scale and bias; 'dw': the weight gradient of (dys, xs) alone, whatever y is."""
        bad = []
        store = dtype if dtype in (torch.float16, torch.bfloat16) else torch.float32
        stored = {'x': self.x, 'xs': self.xs, 'w': self.w}
        sums = {}
        n, cout, p, q = self.y.shape
        taps = self.w.shape[2] * self.w.shape[3]
        if 'y' in need:
            stored.update({f'y{k}': v for k, v in self.forward_variants().items()})
            sums['y'] = conv_units(self.x, self.w, self.s, self.d, self.b, self.pad, self.stride)
        if self.grads and set(need) - {'y'}:
            stored.update(dy=self.dy, dys=self.dys)
        if 'dx' in need:
            stored.update(dx=self.dx, dxs=self.dxs)
            # data gradient: cout * taps terms of dys * w, then the factor s
            sums['dx'] = dot_units(self.dys, self.w, cout * taps) * (1.0 if self.s is None else float(self.s.abs().max()) / quantum(self.s))
        if 'dw' in need:
            sums['dw'] = dot_units(self.dys, self.xs, n * p * q)
        if 'ds' in need and self.s is not None:
            stored.update(dx=self.dx)
            sums['ds'] = plane_dot_units(self.xs, self.dx) / quantum(self.s) ** 2
        if 'dd' in need and self.d is not None:
            stored.update(y=self.y)
            sums['dd'] = plane_dot_units(self.dy, self.y) / quantum(self.d)
        for name, t in stored.items():
            if not representable(t, store):
                bad.append(f'{name} is not representable in {store}')
        for name, u in sums.items():
            if not u < LIMIT:
                bad.append(f'the fp32 sums of {name} reach {u:.3g} units (limit 2^24)')
        return bad

    def check(self, dtype, need=('y', 'dx', 'dw', 'ds', 'dd')):
        bad = self.failures(dtype, need)
        assert not bad, bad


# Operand sets, widest first.  'small': activations from {+-1, +-2, +-3}, weights from {+-1, +-2} (small K).  'pm1': dense +-1
# activations and weights (large K: every term is odd, so a dropped or doubled term flips the parity of the sum).  Scales are powers of
# two, biases and cotangents integers.  bfloat16 keeps 8 significant bits: every value it stores must stay below 256 quanta, so its sets
# are narrower (activations {+-1, +-2}; two neighbouring powers of two per scale, the second one rare) and a case whose K is too large
# for one set moves on to the next (``make_node``).
_WIDE = dict(s=(-1, 0, 1), d=(-1, 0, 1), b=(-3, -2, -1, 1, 2, 3), dy=(-1, 1))
_NARROW = dict(s=(0, 0, 0, 1), d=(0, 0, 0, 1), b=(-2, -1, 1, 2), dy=(-1, 1))
_RARE = dict(s=(0,) * 7 + (1,), d=(0,) * 7 + (1,), b=(-1, 1), dy=(-1, 1))
_LADDER = {
    False: [('small', dict(x=(-3, -2, -1, 1, 2, 3), w=(-2, -1, 1, 2), **_WIDE)), ('pm1', dict(x=(-1, 1), w=(-1, 1), **_WIDE))],
    True: [('small', dict(x=(-2, -1, 1, 2), w=(-2, -1, 1, 2), **_NARROW)), ('pm1', dict(x=(-1, 1), w=(-1, 1), **_NARROW)),
           ('pm1', dict(x=(-1, 1), w=(-1, 1), **_RARE))],
}


def ladder(kind, dtype):
    """The operand sets to try for a case of this kind, in order."""
    rungs = _LADDER[dtype == torch.bfloat16]
    first = next(i for i, (k, _) in enumerate(rungs) if k == kind)
    return [st for _, st in rungs[first:]]


def draw_node(shape, st, seed, scales=True, bias=True, ks=3, stride=1, grads=True, in_scale=True):
    n, cin, cout, h, w, pad = shape
    g = gen(seed)
    x = pick([n, cin, h, w], st['x'], g)
    wt = pick([cout, cin, ks, ks], st['w'], g)
    s = pow2([n, cin], st['s'], g) if (scales and in_scale) else None
    d = pow2([n, cout], st['d'], g) if scales else None
    b = pick([cout], st['b'], g) if bias else None
    return Node(x, wt, s, d, b, lambda shp: pick(shp, st['dy'], g), pad, stride, grads)


_NODES = {}


def make_node(shape, kind, dtype, need=('y', 'dx', 'dw', 'ds', 'dd'), scales=True, bias=True, ks=3, stride=1, in_scale=True, seed=0):
    """The node of a case: the first draw -- operand sets of ``ladder`` in order, three seeds each -- whose results ``need`` are exact in
    ``dtype`` (module-level cache: one reference per case, shared by the tests and left unchanged)."""
    key = (tuple(shape), kind, dtype, tuple(need), scales, bias, ks, stride, in_scale, seed)
    if key not in _NODES:
        why = None
        for rung, st in enumerate(ladder(kind, dtype)):
            for k in range(3):
                node = draw_node(shape, st, seed + 1000 * k, scales, bias, ks, stride, grads=tuple(need) != ('y',), in_scale=in_scale)
                why = node.failures(dtype, need)
                if not why:
                    node.seed, node.rung = seed + 1000 * k, rung
                    _NODES[key] = node
                    break
            if key in _NODES:
                break
        else:
            raise AssertionError(f'no exact draw for {key}: {why}')
    return _NODES[key]


def r1_ref(x, w, dy, pad):
    """R1-style double backward of the unscaled conv: (dx, gradient of sum(dx^2) with respect to w), dx = dL/dx for L = <conv(w, x), dy>."""
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, padding=pad)
    dx, = torch.autograd.grad((y * dy).sum(), xr, create_graph=True)
    gw, = torch.autograd.grad(dx.square().sum(), wr)
    return dx.detach(), gw


def case_id(v):
    """pytest id of a table entry or parameter."""
    shape = getattr(v, 'shape', v)
    if isinstance(shape, tuple) and all(isinstance(k, (int, type(None))) for k in shape):
        return 'x'.join('N' if k is None else str(k) for k in shape)
    return str(v).replace('torch.', '')


# ---- failure messages ---------------------------------------------------------------------------------------------------------------
def mismatch(got, ref, what=''):
    """None when ``got`` equals the float64 ``ref`` cast to its dtype bit for bit, else a message with the count and the first indices."""
    want = ref.to(got.dtype)
    got = got.detach().cpu()
    if got.shape != want.shape:
        return f'{what}: shape {tuple(got.shape)} instead of {tuple(want.shape)}'
    if torch.equal(got, want):
        return None
    bad = (got != want) | torch.isnan(got)
    idx = bad.nonzero()
    first = ', '.join(f'{tuple(i.tolist())}: {got[tuple(i)].item()!r} != {want[tuple(i)].item()!r}' for i in idx[:6])
    return f'{what}: {int(bad.sum())} of {bad.numel()} elements differ; first {first}'


def assert_exact(got, ref, what=''):
    msg = mismatch(got, ref, what)
    assert msg is None, msg


# ---- the case tables: (n, cin, cout, h, w, pad), operand kind, expected plan ------------------------------------------------------------
# conv plan families / kernels and weight-gradient kernels / reductions (include/afcm_hip.h: afcm_conv2d_plan, afcm_conv2d_wgrad_plan)
DIRECT, ROWS96, ROWS128_64, ROWS64, ROWS128 = 0, 1, 2, 3, 4
K_X16, K_GENERAL16, K_F32, K_DIRECT, K_SPLIT = 0, 1, 2, 3, 4
WG_F32, WG_DWORD, WG_GRANULE = 0, 1, 2
RED_SCALAR, RED4_256, RED4_64, RED4_16, RED_DOTS = 0, 1, 2, 3, 4

Fwd = collections.namedtuple('Fwd', 'shape kind family fast')            # batch None: the smallest with a ragged second round
FWD16 = [
    # 64-row persistent, one round, general epilogue, ragged tiles on all four edges
    Fwd((2, 8, 64, 30, 46, 1), 'small', ROWS64, 0),
    Fwd((1, 8, 64, 38, 38, 2), 'small', ROWS64, 0),
    Fwd((2, 8, 64, 30, 30, 0), 'small', ROWS64, 0),                    # pad 0
    Fwd((2, 40, 64, 6, 14, 2), 'small', ROWS64, 1),                    # K tail: a second chunk with 8 live channels
    Fwd((1, 181, 64, 6, 14, 2), 'pm1', ROWS64, 1),                     # K tail: 181 channels
    Fwd((None, 8, 16, 126, 126, 2), 'small', ROWS64, 1),               # second round with a ragged last round, fast epilogue
    Fwd((None, 8, 16, 94, 94, 1), 'small', ROWS64, 0),                 # ... general epilogue
    Fwd((None, 8, 80, 126, 126, 2), 'small', ROWS96, 1),               # 96-row persistent, second round
    Fwd((1, 8, 65, 12, 150, 2), 'small', ROWS96, 0),                   # 96-row, one round, dead last fragment
    Fwd((1, 8, 128, 30, 30, 2), 'small', ROWS128, 1),
    Fwd((2, 8, 200, 14, 30, 2), 'small', ROWS128, 1),
    Fwd((2, 40, 130, 22, 26, 2), 'small', ROWS128_64, 0),              # 128 + 64 (o_base launch)
    Fwd((3, 3, 20, 17, 70, 2), 'small', DIRECT, 0),
    Fwd((2, 1, 64, 40, 130, 1), 'small', DIRECT, 0),
]
SECOND_ROUND_AT_256_CUS = {(8, 16, 126, 126, 2): 13, (8, 16, 94, 94, 1): 22, (8, 80, 126, 126, 2): 9}
# row-pitched input and output, one per epilogue (output rows of 64 elements: the 48-wide tiles of the first then take the fast
# epilogue, the 40-wide tiles of the second the general one)
PITCHED16 = [Fwd((2, 8, 64, 30, 46, 1), 'small', ROWS64, 1), Fwd((1, 8, 64, 38, 38, 2), 'small', ROWS64, 0)]
FWD16_1X1 = [Fwd((2, 37, 70, 9, 12, 0), 'small', ROWS128, 0), Fwd((2, 20, 130, 7, 10, 0), 'small', ROWS64, 0), Fwd((1, 64, 1, 32, 32, 0), 'small', ROWS64, 0)]
FWD32_SPLIT = [Fwd((2, 8, 64, 30, 46, 1), 'small', ROWS64, 0), Fwd((1, 40, 130, 22, 26, 2), 'small', ROWS64, 0),
               Fwd((None, 8, 16, 94, 94, 1), 'small', ROWS64, 0)]
FWD32_NATIVE = [Fwd((2, 12, 70, 9, 11, 0), 'small', ROWS128, 0), Fwd((2, 12, 70, 9, 11, 1), 'small', ROWS128, 0),
                Fwd((2, 12, 70, 9, 11, 2), 'small', ROWS128, 0), Fwd((1, 8, 130, 7, 9, 2), 'small', ROWS64, 0)]
FWD32_NATIVE_1X1 = [Fwd((2, 37, 70, 9, 12, 0), 'small', ROWS128, 0)]
STRIDE2 = [((3, 8, 200, 9, 12, 2), 'small'), ((2, 16, 16, 20, 36, 1), 'small'), ((1, 37, 130, 67, 130, 0), 'small')]

Wg = collections.namedtuple('Wg', 'shape ks kind kernel x16')
WGRAD16_GRANULE = [
    # 3x3 pad 2, 16x16x32 form: the last 64-pixel chunk of Q holds 1..32 or 49..64 pixels
    Wg((2, 64, 64, 6, 14, 2), 3, 'small', WG_GRANULE, 1), Wg((1, 64, 64, 6, 64, 2), 3, 'small', WG_GRANULE, 1),
    Wg((3, 40, 72, 4, 148, 2), 3, 'small', WG_GRANULE, 1),
    # 32x32x16 form: 33..48 pixels
    Wg((2, 64, 64, 5, 36, 2), 3, 'small', WG_GRANULE, 0), Wg((1, 91, 91, 7, 100, 2), 3, 'small', WG_GRANULE, 0),
    # 1x1 pad 0
    Wg((2, 37, 70, 9, 12, 0), 1, 'small', WG_GRANULE, 1), Wg((4, 64, 1, 32, 256, 0), 1, 'small', WG_GRANULE, 1),
    # the scalar reduction: 5 * 7 * 9 = 315 elements
    Wg((1, 5, 7, 6, 14, 2), 3, 'small', WG_GRANULE, 1),
]
WGRAD16_DWORD = ([Wg((2, 64, 64, 6, q + 2 - 2 * p, p), 3, 'small', WG_DWORD, None) for p in (0, 1) for q in (16, 62, 64, 66, 100)]
                 + [Wg((2, 91, 130, 7, 22, p), 3, 'small', WG_DWORD, None) for p in (0, 1)]
                 + [Wg((3, 16, 16, 9, 20, p), 3, 'small', WG_DWORD, None) for p in (0, 1)])
WGRAD32 = [Wg((2, 12, 70, 9, 11, 0), 3, 'small', WG_F32, None), Wg((2, 12, 70, 9, 11, 1), 3, 'small', WG_F32, None),
           Wg((2, 12, 70, 9, 11, 2), 3, 'small', WG_F32, None), Wg((2, 37, 70, 9, 12, 0), 1, 'small', WG_F32, None)]
WGRAD_DOTS = [(2, 24, 40, 30, 36, 2), (3, 16, 16, 90, 20, 2)]
WGRAD_DOTS_NONE = (3, 16, 16, 200, 20, 2)                              # split count not a multiple of the batch: no image-aligned form
NODES = [(2, 8, 64, 30, 46, 1), (2, 40, 130, 22, 26, 2)]
R1_CASE = (2, 8, 16, 12, 14, 1)


# ---- plan queries (pure host calls of the built library) ------------------------------------------------------------------------------
_CODES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
ConvPlan = collections.namedtuple('ConvPlan', 'family rows th tw items grid fast kernel')
WgradPlan = collections.namedtuple('WgradPlan', 'kernel pad_odd x16 small splits steps reduce splits_img')


def conv_plan(lib, dtype, n, cin, cout, h, w, ks, pad, x_pitch=0, y_pitch=0, split=False):
    out = (ctypes.c_int32 * 8)()
    rc = lib.afcm_conv2d_plan(_CODES[dtype], n, cin, cout, h, w, ks, pad, x_pitch, y_pitch, int(split), out)
    assert rc == 0, (rc, lib.afcm_last_error())
    return ConvPlan(*out)


def wgrad_plan(lib, dtype, n, cin, cout, h, w, ks, pad, dots=False):
    """The plan, or None where the image-aligned form (``dots``) is not available."""
    out = (ctypes.c_int32 * 8)()
    rc = lib.afcm_conv2d_wgrad_plan(_CODES[dtype], n, cin, cout, h, w, ks, pad, 0, 0, int(dots), out)
    if rc == -1:
        return None
    assert rc == 0, (rc, lib.afcm_last_error())
    return WgradPlan(*out)


def second_round_batch(lib, dtype, cin, cout, h, w, pad, split=False):
    """The smallest batch at which the persistent launch takes a second round whose last round is ragged: items > grid, items % grid != 0."""
    for n in range(1, 257):
        pl = conv_plan(lib, dtype, n, cin, cout, h, w, 3, pad, split=split)
        if pl.items > pl.grid and pl.items % pl.grid != 0:
            return n
    raise AssertionError('no batch up to 256 reaches a second round')


def with_batch(lib, case, dtype, split=False):
    """The case's shape with a None batch replaced by ``second_round_batch``."""
    n, cin, cout, h, w, pad = case.shape
    if n is None:
        n = second_round_batch(lib, dtype, cin, cout, h, w, pad, split)
    return (n, cin, cout, h, w, pad)


def shape_at_256(case):
    """The case's shape with a None batch replaced by the second-round batch of a 256-compute-unit device (tests without a GPU)."""
    shape = tuple(case.shape)
    return (SECOND_ROUND_AT_256_CUS[shape[1:]],) + shape[1:] if shape[0] is None else shape


def forward_node(shape, case, dtype, ks=3, in_scale=False, bias=True):
    """The forward-only node of a forward case (output scale and bias; ``in_scale``: the input scale too)."""
    return make_node(shape, case.kind, dtype, need=('y',), ks=ks, in_scale=in_scale, bias=bias)


def wgrad_node(case, dtype):
    """Operands of a weight-gradient case: dy and x as they are (no scales, no bias)."""
    return make_node(case.shape, case.kind, dtype, need=('dw',), scales=False, bias=False, ks=case.ks)


def onebyone_node(case, dtype):
    """A 1x1 16-bit case: the forward (output scale, bias) and the data gradient conv^T(w, d * dy)."""
    return make_node(case.shape, case.kind, dtype, need=('y', 'dx'), ks=1, in_scale=False)


def dots_node(shape, dtype):
    """An image-aligned weight-gradient case: dw and dots[n, i] = <x[n, i], conv^T(w, dy)[n, i]>, the latter summed from the per-image
    weight-gradient slabs (cout * 9 terms of w * dW_n, dW_n itself a sum over the image's pixels)."""
    node = make_node(shape, 'small', dtype, need=('dx', 'dw'), scales=False, bias=False)
    n, cout, p, q = node.y.shape
    per_image = dot_units(node.dy, node.x, p * q)
    assert per_image * cout * 9 * float(node.w.abs().max()) < LIMIT
    node.dots = (node.x * node.dx).sum([2, 3])
    return node


def stride2_node(shape, kind, dtype):
    return make_node(shape, kind, dtype, need=('y', 'dx', 'dw'), scales=False, bias=False, stride=2)


def full_node(shape, dtype):
    """An autograd-node case: input and output scales, no bias, all five results."""
    return make_node(shape, 'small', dtype, bias=False)
