"""float64 restatement of the modulation kernels (afcm_amd/csrc/modulation.hip: weight_norm_{fwd,bwd}, style_coefs_{fwd,bwd1,bwd2} and their
modulation_bank_* forms), the case tables of tests/test_gpu_modulation.py and the bars the kernels are held to.  No GPU, nothing from the reference.

``weight_norm`` and ``style_coefs`` are written from the header comment of include/afcm_hip.h and NET:41-57, one function per forward ABI call; they
run in the dtype of their arguments, so float64 arguments and torch autograd give the exact backward of each ABI call for any set of output gradients
(``weight_norm_bwd``, ``style_coefs_bwd``: a gradient that is None leaves that output out of the loss, as a NULL pointer does), and float32 arguments
give the eager composition the bars are measured from.

The kernels' decisions the tables are built around (tests/test_modulation_ref_cpu.py recomputes them and checks every seam is reached):
  256 threads per workgroup; weight rows of cin k^2 <= 1024 / <= 4608 / longer are the classes PT = 4 / 18 / 0 (registers per thread, 0 = three passes);
  style_coefs_fwd: workgroups (n, chunk of 32 output channels), a wave per 8 channels, rows past cout read clamped and dropped; the batch mean takes
  four loads per trip while j + 768 < n cin (trips of 1024), then single loads; style_coefs_bwd1: workgroups (n, chunk of 64 input channels), the sum
  over cout split over 4 waves; bwd2: one workgroup per sample, then one per output channel for g_wsq.

Bars.  EAGER_FWD / EAGER_GRAD are the worst errors of the float32 eager composition on the CPU (this file's functions on float32 tensors, call by call,
and the composed NET:41-57 expression end to end) against float64, over every SEAM_SHAPES entry with ordinary and with floor inputs and all gradients,
every ABI GRAD_SETS combination on BWD_SHAPES and every BANK_ORDERS entry: per element relative for the forward tensors (sums of like-signed terms),
per row -- |error| / max |reference| over the element's own output channel (dw, g_wsq) or sample (dt) -- for the gradients, which cancel.
test_modulation_ref_cpu.py::test_eager_float32_sits_within_a_quarter_of_the_bars repeats the measurement.  The kernels' bars are 4 x these: the margin
is for another summation order (shuffle trees and four-way partials against aten's) and the device rsqrtf."""
import collections
import itertools

import torch

F32, F64 = torch.float32, torch.float64
EPS = 1e-8                                              # NET:51
THREADS, OC_CHUNK, WAVE_CHANNELS, IC_CHUNK, O_WAVES = 256, 32, 8, 64, 4
MEAN_TRIP, MEAN_LEAD = 1024, 768
BANK_MAX = 16                                           # AFCM_MODULATION_MAX
CHANNELS_MAX = 16384

EAGER_FWD = 4.8e-7                                      # measured 4.47e-7 (a wsq element) and 4.99e-6 (a dt row at cin = 1, four styles in
EAGER_GRAD = 5.2e-6                                     # the whole batch), rounded up a few per cent for another CPU's summation order
BAR_FWD = 4 * EAGER_FWD
BAR_GRAD = 4 * EAGER_GRAD


def row_class(cin, k):
    """PT of weight_norm_{fwd,bwd}: registers per thread that hold a weight row, 0 for the three-pass form."""
    n = cin * k * k
    return 4 if n <= THREADS * 4 else 18 if n <= THREADS * 18 else 0


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def weight_norm(w):
    """afcm_weight_norm_fwd: w [O, I, k, k] -> (w_hat, wsq [O, I], scale [O])."""
    scale = w.square().mean([1, 2, 3]).rsqrt()                                  # NET:42
    w_hat = w * scale[:, None, None, None]
    return w_hat, w_hat.square().sum([2, 3]), scale


def style_coefs(t, wsq, magnitude, demodulate):
    """afcm_style_coefs_fwd: t [N, I], wsq [O, I] (any values: an input of the call), magnitude [] or None -> (s_eff [N, I], d [N, O] or None, r [1])."""
    r = t.square().mean().rsqrt() if demodulate else torch.ones([], dtype=t.dtype)   # NET:43, whole batch
    s_hat = t * r
    d = (s_hat.square() @ wsq.t() + EPS).rsqrt() if demodulate else None            # NET:50-52, factorised
    s_eff = s_hat if magnitude is None else s_hat * magnitude.rsqrt()               # NET:346, 55-57
    return s_eff, d, r.reshape(1)


def composed(w, t, magnitude, demodulate):
    """NET:41-57 as the reference writes it, per-sample weights and all: (w_hat, s_eff, d or None)."""
    d = None
    if demodulate:
        w = w * w.square().mean([1, 2, 3], keepdim=True).rsqrt()
        t = t * t.square().mean().rsqrt()
        d = ((w.unsqueeze(0) * t[:, None, :, None, None]).square().sum([2, 3, 4]) + EPS).rsqrt()
    if magnitude is not None:
        t = t * magnitude.rsqrt()
    return w, t, d


def _grads(outs, cots, wrt):
    loss = sum((o * g).sum() for o, g in zip(outs, cots) if o is not None and g is not None)
    if not torch.is_tensor(loss) or not loss.requires_grad:
        return [torch.zeros_like(x) for x in wrt]
    got = torch.autograd.grad(loss, wrt, allow_unused=True)
    return [torch.zeros_like(x) if g is None else g for x, g in zip(wrt, got)]


def weight_norm_bwd(w, g_hat, g_wsq):
    """afcm_weight_norm_bwd: dw for the loss <w_hat, g_hat> + <wsq, g_wsq>; None = that output is not in the loss."""
    w = w.detach().requires_grad_(True)
    w_hat, wsq, _ = weight_norm(w)
    return _grads((w_hat, wsq), (g_hat, g_wsq), [w])[0]


def style_coefs_bwd(t, wsq, magnitude, demodulate, g_s, g_d):
    """afcm_style_coefs_bwd: (dt, g_wsq or None) for the loss <s_eff, g_s> + <d, g_d>."""
    t = t.detach().requires_grad_(True)
    wsq = wsq.detach().requires_grad_(True) if demodulate else None
    s_eff, d, _ = style_coefs(t, wsq, magnitude, demodulate)
    got = _grads((s_eff, d), (g_s, g_d), [t] + ([wsq] if demodulate else []))
    return got[0], (got[1] if demodulate else None)


def composed_bwd(w, t, magnitude, demodulate, g_hat, g_s, g_d):
    """(dw, dt) of the composed expression for the loss <w_hat, g_hat> + <s_eff, g_s> + <d, g_d>."""
    w, t = w.detach().requires_grad_(True), t.detach().requires_grad_(True)
    w_hat, s_eff, d = composed(w, t, magnitude, demodulate)
    return _grads((w_hat if demodulate else None, s_eff, d), (g_hat, g_s, g_d), [w, t])


# ---- where a per-row bar has nothing to hold on to --------------------------------------------------------------------------------------------------
def row_is_one_element(shape):
    """cin k^2 = 1: w_hat = sign(w) whatever |w|, so dw is zero by identity and any float32 evaluation leaves the rounding residue of g - w_hat^2 g.
    Such a row is held to BAR_GRAD of the cancelling terms, scale (|g_hat| + 2 |g_wsq|), not of the (zero) reference."""
    return shape[1] * shape[2] * shape[2] == 1


def floor_composes(shape):
    """Whether floor inputs may run through weight_norm and style_coefs CHAINED (the bank, the autograd ops, the composed expression): the floor
    has to come from the styles (n >= 3), and cin > 1 -- at cin = 1, wsq[o, 0] = k^2 whatever w, the path from wsq back to w cancels by identity,
    and the floor sample's gradient on wsq (of the order of d^3) leaves a residue there that swamps g_hat's part of dw.  Call by call, where g_wsq
    is an operand of its own, every shape takes floor inputs."""
    return shape[3] >= 3 and shape[1] > 1


# ---- comparison: the worst ratio of an error to its bar (<= 1 passes) ---------------------------------------------------------------------------
def forward_ratio(got, want, bar):
    """Per element: |got - want| <= bar |want|; an element whose reference is zero must be zero."""
    got, want = got.detach().to(F64).cpu().reshape(-1), want.detach().to(F64).cpu().reshape(-1)
    assert got.shape == want.shape
    if not bool(torch.isfinite(got).all()):
        return float('inf')
    err, lim = (got - want).abs(), bar * want.abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / lim)
    return float(ratio.max())


def row_ratio(got, want, bar):
    """Per row (first dimension): |got - want| <= bar max |want| over the row; a row whose reference is all zero must be exactly zero."""
    assert got.shape == want.shape
    got, want = got.detach().to(F64).cpu().flatten(1), want.detach().to(F64).cpu().flatten(1)
    if not bool(torch.isfinite(got).all()):
        return float('inf')
    err, lim = (got - want).abs().amax(1), bar * want.abs().amax(1)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / lim)
    return float(ratio.max())


# ---- case tables -----------------------------------------------------------------------------------------------------------------------------------
# name -> (cout, cin, k, n); the name says which seam the entry sits on (others ride along: test_modulation_ref_cpu.py lists what is reached)
SEAM_SHAPES = {
    'row_1': (1, 1, 1, 4),                  # one element: cin k^2 = 1, cout = 1, cin = 1
    'row_9': (6, 1, 3, 4),                  # a 3x3 row shorter than a wave
    'row_255': (2, 255, 1, 3),
    'row_256': (3, 256, 1, 3),              # one pass of 256 threads exactly; n cin = 768
    'row_257': (4, 257, 1, 2),
    'row_1023': (5, 1023, 1, 1),            # n cin = 1023
    'row_1024': (7, 1024, 1, 1),            # last row of PT = 4; n cin = 1024
    'row_1025': (8, 1025, 1, 1),            # first row of PT = 18; n cin = 1025
    'row_113x9': (9, 113, 3, 3),            # 1017: a 3x3 row that ends inside PT = 4, j / 9 crosses the register slots
    'row_114x9': (3, 114, 3, 2),            # 1026: the same row in PT = 18
    'row_512x9': (2, 512, 3, 3),            # 4608: last row of PT = 18
    'row_513x9': (2, 513, 3, 3),            # 4617: the three-pass form
    'cout_31': (31, 20, 3, 3),
    'cout_32': (32, 20, 1, 3),              # one workgroup's channels exactly
    'cout_33': (33, 65, 3, 17),             # ragged in every chunk: 32 + 1 channels, 64 + 1 inputs, 17 samples
    'cout_65': (65, 24, 1, 3),              # three chunks, the last with one row
    'cin_63': (4, 63, 3, 3),
    'cin_64': (5, 64, 1, 12),               # one bwd1 chunk exactly; n cin = 768
    'cin_65': (2, 65, 1, 2),
    'ncin_769': (3, 769, 1, 1),             # first n cin that takes a four-load trip
    'ncin_1792': (2, 256, 1, 7),            # 7 x 256: one trip, then three single loads
    'ncin_1793': (2, 1793, 1, 1),           # two trips
}
BWD_SHAPES = ('cout_33', 'row_113x9', 'row_114x9', 'row_513x9')     # ragged everywhere; then k = 3 in each PT class

_B = (False, True)
GRAD_SETS = {
    'weight_norm_bwd': list(itertools.product(_B, _B)),                         # (g_hat, g_wsq) given
    'style_coefs_bwd_demodulating': list(itertools.product(_B, _B, _B, _B)),    # (g_s, g_d, g_wsq wanted, magnitude) given
    'style_coefs_bwd_plain': list(itertools.product(_B, _B)),                   # (g_s, magnitude) given
    # (outputs in the loss out of 'w' w_hat / 's' s_eff / 'd' d, weight frozen, styles frozen)
    'autograd': [(''.join(c), fw, ft) for r in (1, 2, 3) for c in itertools.combinations('wsd', r)
                 for fw, ft in ((False, False), (True, False), (False, True))],
}

# one bank layer: a SEAM_SHAPES name (its cout, cin, k; the batch is the order's), demodulate, magnitude given, outputs in the loss, weight frozen
Layer = collections.namedtuple('Layer', 'seam demodulate magnitude outputs frozen')
_D = lambda seam, outputs='wsd', magnitude=True, frozen=False: Layer(seam, True, magnitude, outputs, frozen)
_P = lambda seam, outputs='s', magnitude=True: Layer(seam, False, magnitude, outputs, True)
# name -> (n, layers).  A layer that does not demodulate has no workgroup in the norm launches (equal neighbours in blk[]), nor has a frozen one
# in the backward's; every order leaves one layer out of the loss where it has more than one.
BANK_ORDERS = {
    'plain_first': (4, [_P('cin_63'), _D('row_114x9'), _D('cout_31', ''), _D('cout_33', 'd', frozen=True)]),
    'plain_last': (4, [_D('cout_65', 'sd'), _D('row_9', '', magnitude=False), _P('row_255')]),
    'plain_middle': (17, [_D('cout_33', 'wd'), _P('cin_65', ''), _D('cout_32', 'ws', magnitude=False)]),
    'plain_adjacent': (4, [_D('row_113x9'), _P('row_257', magnitude=False), _P('row_1', ''), _D('row_513x9', 'w', frozen=False)]),
    'all_plain': (4, [_P('cin_64'), _P('row_1025', ''), _P('cout_33', magnitude=False)]),
    'one_demodulating': (4, [_D('cout_33')]),
    'one_plain': (2, [_P('cin_65')]),
    # the first layer sets the launches' dynamic LDS sizes (max cin forward, max cout backward): the small ones after it use a corner of it
    'small_after_large': (4, [_D('row_1025', 'sd'), _D('cout_65'), _D('row_1', 'wd'), _P('row_9'), _D('cout_31', '', frozen=True), _D('row_9', 'wd')]),
    'frozen_neighbours': (4, [_D('cout_31', 'd', frozen=True), _D('cin_63', 'sd', frozen=True), _D('cout_32'), _D('row_9', '', frozen=True), _D('row_255', 's', frozen=True)]),
    'full_16': (4, [_D('row_1'), _P('row_9'), _D('cout_31', 'wd'), _D('row_113x9', 'sd', frozen=True), _D('cout_32', magnitude=False), _P('cin_63', ''),
                    _D('cout_65', 'd'), _D('row_256', ''), _D('cin_64', 'ws'), _P('row_255', magnitude=False), _D('row_114x9'), _D('cin_65', 's', frozen=True),
                    _D('cout_33'), _P('row_257'), _D('row_9', 'wsd'), _D('row_1', 'w')]),
}


# ---- inputs: float32 values (the kernels' operands), deterministic -------------------------------------------------------------------------------
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (k if isinstance(k, int) else sum(ord(c) * 131 ** j for j, c in enumerate(str(k))))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def ordinary_inputs(shape, seed):
    """(w [O, I, k, k], t [N, I]) float32: normal weights, styles randn + 1 as at initialisation."""
    o, i, k, n = shape
    g = _gen('ordinary', o, i, k, n, seed)
    return torch.randn(o, i, k, k, generator=g), torch.randn(n, i, generator=g) + 1.0


def magnitude(seed):
    return torch.rand([], generator=_gen('magnitude', seed)) + 0.5


def cotangents(shape, seed):
    """(g_hat [O, I, k, k], g_wsq [O, I], g_s [N, I], g_d [N, O]) float32."""
    o, i, k, n = shape
    g = _gen('cotangents', o, i, k, n, seed)
    return tuple(torch.randn(s, generator=g) for s in ((o, i, k, k), (o, i), (n, i), (n, o)))


Floor = collections.namedtuple('Floor', 'w t wsq_gain scaled zero')
FLOOR_WINDOW = (EPS / 4, 4 * EPS)


def floor_q(f):
    """q[n, o] = sum_i s_hat^2 wsq of floor inputs, float64, with the gain on wsq."""
    _, wsq, _ = weight_norm(f.w.to(F64))
    t = f.t.to(F64)
    return (t * t.square().mean().rsqrt()).square() @ (wsq * float(f.wsq_gain)).t()


def floor_inputs(shape, seed):
    """Inputs that put the + 1e-8 of NET:51 to work.  Styles are randn + 1; sample ``zero`` (the first) is exactly zero, so its d is rsqrt(1e-8)
    whatever the weights; sample ``scaled`` (the last) is one such row times a constant chosen in float64 so that its q[n, o] = sum_i s_hat^2 wsq lies
    in [1e-8 / 4, 4e-8] for every o -- the magnitudes of that one row are held to [0.6, 1.9], which bounds the spread of q over o by 10.

    The batch-wide normalisation (NET:43) undoes any scale common to the whole batch, so a sample can only be small NEXT TO an ordinary one: with
    n >= 3 the constant is on the styles and ``wsq_gain`` is 1.  With n = 2 (scaled + zero) and n = 1 (scaled alone) no style can reach the floor;
    there the row keeps its size and ``wsq_gain`` (a float32 number) is to be multiplied into wsq before style_coefs sees it -- wsq is a free input
    of afcm_style_coefs_{fwd,bwd}.  Asserts the window and the zero sample itself."""
    o, i, k, n = shape
    w, t = ordinary_inputs(shape, seed)
    scaled, zero = n - 1, (0 if n > 1 else None)
    row = t[scaled].to(F64)
    row = torch.where(row < 0, -torch.ones_like(row), torch.ones_like(row)) * row.abs().clamp(0.6, 1.9)
    _, wsq, _ = weight_norm(w.to(F64))
    a = row.square() @ wsq.t()                                                  # [O]
    mid = float((a.min() * a.max()).sqrt())
    if zero is not None:
        t[zero] = 0.0
    gain = torch.ones([], dtype=F32)
    if n >= 3:
        others = float(t.to(F64).square().sum() - t[scaled].to(F64).square().sum())
        rr = float(row.square().sum())
        # r^2 c^2 mid = EPS with r^2 = n i / (others + c^2 rr)
        c2 = EPS * others / (n * i * mid - EPS * rr)
        t[scaled] = (row * c2 ** 0.5).to(F32)
    else:
        t[scaled] = row.to(F32)
        r2 = n * i / float(t.to(F64).square().sum())
        gain = torch.tensor(EPS / (r2 * mid), dtype=F32)
    f = Floor(w, t, gain, scaled, zero)
    q = floor_q(f)
    assert bool((q[scaled] >= FLOOR_WINDOW[0]).all()) and bool((q[scaled] <= FLOOR_WINDOW[1]).all()), (shape, q[scaled].min(), q[scaled].max())
    assert zero is None or (bool((t[zero] == 0).all()) and bool((q[zero] == 0).all())), shape
    return f
