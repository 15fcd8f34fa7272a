"""Shared by test_bias_act_ref_cpu.py and test_gpu_bias_act.py: the float64 restatement of bias_act, the per-element bar, and the inputs.

The contract restated (the docstring of afcm_amd/torch_utils/ops/bias_act.py, its activation table, the header of csrc/bias_act.hip):
  mode 0   y  = clamp(act(x + b) * gain, -clamp, clamp)
  mode 1   dx = x * act'  * gain * dy      x is the forwarded operand (the incoming gradient), dy is 1 where absent
  mode 2   d2 = x * act'' * gain * dy
The derivatives of the 'y' activations are read from the saved output ``yref / gain`` (0 where the gain is 0), so the side of a kink is the
sign of the SAVED output; swish reads them from the saved input ``xref + b``.  With a clamp, modes 1 and 2 are zero wherever the saved
output lies outside the open interval (-clamp, clamp); for swish the saved output is recomputed from the saved input.  alpha, gain and
clamp cross the C ABI as floats, so they are rounded to float32 before use.

Selections are written as IEEE selections (a comparison with NaN is false and takes the second value): relu(NaN) = 0, a clamped NaN is
-clamp, every other activation hands NaN on; infinities go to the activation's limit.

Derivatives use forms that cannot overflow and do not cancel: sigmoid(z) and sigmoid(-z) for swish, expm1 / log1p elsewhere.  ``evaluate``
takes the arithmetic type, so that the CPU test can run the very same formulas in float32 and hold them to ``bar``.
"""
import math

import numpy as np
import torch

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = [F32, F16, BF16]
DTYPE_ID = {F32: 'fp32', F16: 'fp16', BF16: 'bf16'}
ACTS = ['linear', 'relu', 'lrelu', 'tanh', 'sigmoid', 'elu', 'selu', 'softplus', 'swish']
INDEX = {a: i + 1 for i, a in enumerate(ACTS)}                       # the plugin's activation numbers
DEF_ALPHA = {a: (0.2 if a == 'lrelu' else 0.0) for a in ACTS}
DEF_GAIN = {a: (math.sqrt(2) if a in ('relu', 'lrelu', 'swish') else 1.0) for a in ACTS}
SECOND = ('tanh', 'sigmoid', 'elu', 'selu', 'softplus', 'swish')     # activations with a second derivative
SELU_SCALE = 1.0507009873554804934193349852946
SELU_ALPHA = 1.6732632423543772848170429916717

UNIT = {F32: 2.0 ** -24, F16: 2.0 ** -11, BF16: 2.0 ** -8}           # u_T: one rounding of the result
TINY = {F32: 2.0 ** -126, F16: 2.0 ** -14, BF16: 2.0 ** -126}        # m_T: the smallest normal (subnormal results, a flush)
EPS32 = 2.0 ** -24
# C of the bar.  Measured worst err / (2^-24 F): 0.84 for float32 numpy (test_bias_act_ref_cpu.py), 1.40 for the kernels on an MI355X
# (table in test_gpu_bias_act.py); the smallest power of two at or above four times the GPU's worst.
C = 8.0
SWISH_MARGIN = 64 * EPS32                                            # relative distance a recomputed swish output keeps from the clamp

GRID_THREADS = 2048 * 256                                            # lanes of a full grid of either kernel


# ---------------------------------------------------------------------------------------------------------------- plumbing
def f64(t):
    """torch tensor of any float type (or None) -> float64 numpy array."""
    return None if t is None else t.detach().to(torch.float64).cpu().numpy()


def quantize(a, dtype):
    """float64 numpy -> ``dtype`` (through float32, as the kernels round fp32 results) -> float64 numpy."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.float32).to(dtype).to(torch.float64).numpy()


def tensor(a, dtype):
    """float64 numpy array of representable values -> CPU tensor of ``dtype``."""
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dtype)


def rounded(shape, dtype, seed, scale=1.0):
    """Seeded N(0, scale^2) float64 values that are exactly representable in ``dtype``."""
    g = torch.Generator().manual_seed(int(seed))
    return quantize((torch.randn(shape, generator=g, dtype=torch.float32).double() * scale).numpy(), dtype)


def _bias(b, ndim, dim):
    shape = [1] * ndim
    shape[dim] = -1
    return b.reshape(shape)


# ---------------------------------------------------------------------------------------------------------------- the restatement
def _sig(z, one):
    with np.errstate(over='ignore'):
        return one / (one + np.exp(-z))                 # exp(-z) = inf gives 0: accurate in relative terms on both sides


def _value(act, z, alpha, dt):
    one, zero = dt(1), dt(0)
    if act == 'linear':
        return z
    if act == 'relu':
        return np.where(z > zero, z, zero)
    if act == 'lrelu':
        return np.where(z > zero, z, z * alpha)
    if act == 'tanh':
        return np.tanh(z)
    if act == 'sigmoid':
        return _sig(z, one)
    if act == 'elu':
        return np.where(z >= zero, z, np.expm1(np.minimum(z, zero)))
    if act == 'selu':
        return np.where(z >= zero, dt(SELU_SCALE) * z, dt(SELU_SCALE * SELU_ALPHA) * np.expm1(np.minimum(z, zero)))
    if act == 'softplus':
        return np.maximum(z, zero) + np.log1p(np.exp(-np.abs(z)))
    assert act == 'swish'
    with np.errstate(invalid='ignore'):
        return np.where(z == -np.inf, zero, z * _sig(z, one))          # the limit at -inf, not -inf * 0


def _derivative(act, order, yy, z, alpha, dt):
    """act' (order 1) or act'' (order 2): from the saved output over the gain ``yy``, or from the saved biased input ``z`` (swish)."""
    one, zero, two = dt(1), dt(0), dt(2)
    if act == 'linear':
        return np.full_like(yy, one if order == 1 else zero)
    if act == 'relu':
        return np.where(yy > zero, one, zero) if order == 1 else np.zeros_like(yy)
    if act == 'lrelu':
        return np.where(yy > zero, one, alpha) if order == 1 else np.zeros_like(yy)
    if act == 'tanh':
        d1 = (one - yy) * (one + yy)
        return d1 if order == 1 else -two * yy * d1
    if act == 'sigmoid':
        d1 = yy * (one - yy)
        return d1 if order == 1 else d1 * (one - two * yy)
    if act == 'elu':
        return np.where(yy >= zero, one if order == 1 else zero, yy + one)
    if act == 'selu':
        return np.where(yy >= zero, dt(SELU_SCALE) if order == 1 else zero, yy + dt(SELU_SCALE * SELU_ALPHA))
    if act == 'softplus':                                                # y = log(1 + e^x): sigmoid(x) = 1 - e^-y
        s = -np.expm1(-yy)
        return s if order == 1 else s * np.exp(-yy)
    assert act == 'swish'
    s, sm = _sig(z, one), _sig(-z, one)                                  # sm = 1 - s without the cancellation
    return s * (one + z * sm) if order == 1 else s * sm * (two + z * (sm - s))


def evaluate(mode, act, x, b, xref, yref, dy, dim, alpha, gain, clamp, dt=np.float64):
    """The restatement in the arithmetic ``dt``.  Operands: numpy arrays (or None, as the plugin's empty tensors); returns a ``dt`` array."""
    x = np.asarray(x, dtype=dt)
    alpha, gain, clamp = (dt(np.float32(v)) for v in (alpha, gain, -1.0 if clamp is None else clamp))
    bb = dt(0) if b is None else _bias(np.asarray(b, dtype=dt), x.ndim, dim)
    if mode == 0:
        y = _value(act, x + bb, alpha, dt) * gain
        if clamp >= 0:
            y = np.where((y > -clamp) & (y < clamp), y, np.where(y >= dt(0), clamp, -clamp))
        return y
    assert mode in (1, 2)
    z = (np.zeros_like(x) if xref is None else np.asarray(xref, dtype=dt)) + bb
    saved = np.zeros_like(x) if yref is None else np.asarray(yref, dtype=dt)
    yy = saved / gain if gain != 0 else np.zeros_like(x)
    y = x * _derivative(act, mode, yy, z, alpha, dt) * gain
    if dy is not None:
        y = y * np.asarray(dy, dtype=dt)
    if clamp >= 0:
        if act == 'swish':
            saved = _value('swish', z, alpha, dt) * gain
        y = np.where((saved > -clamp) & (saved < clamp), y, dt(0))
    return y


def ref(mode, act, x, b, xref, yref, dy, dim, alpha, gain, clamp):
    """float64 result of one kernel mode on the kernel's own operands (torch tensors or numpy arrays; None where the plugin gets an empty one)."""
    a = [t if (t is None or isinstance(t, np.ndarray)) else f64(t) for t in (x, b, xref, yref, dy)]
    return evaluate(mode, act, a[0], a[1], a[2], a[3], a[4], dim, alpha, gain, clamp, np.float64)


# ---------------------------------------------------------------------------------------------------------------- the bar
def scale_f(mode, want, x, b, xref, dy, dim, gain):
    """F_i = |want_i| + |gain dy_i| (1 + |x_i| max(1, |xref_i + b|)); x after the bias in mode 0; dy = 1 and xref + b = 0 where absent."""
    a = [t if (t is None or isinstance(t, np.ndarray)) else f64(t) for t in (x, b, xref, dy)]
    x, b, xref, dy = a
    bb = 0.0 if b is None else _bias(b, x.ndim, dim)
    fwd = np.abs(x + bb) if mode == 0 else np.abs(x)
    fwd = np.where(np.isfinite(fwd), fwd, 0.0)          # at a non-finite input the result is a limit value: no input-sized slack
    z = np.abs(xref + bb) if (mode != 0 and xref is not None) else np.zeros_like(x)
    g = abs(float(np.float32(gain))) * (np.abs(dy) if dy is not None else 1.0)
    return np.abs(want) + g * (1.0 + fwd * np.maximum(1.0, z))


def bar(mode, want, x, b, xref, dy, dim, gain, dtype, c=None):
    """|got_i - want_i| <= u_T |want_i| + C 2^-24 F_i + m_T."""
    c = C if c is None else c
    return UNIT[dtype] * np.abs(want) + c * EPS32 * scale_f(mode, want, x, b, xref, dy, dim, gain) + TINY[dtype]


def needed_c(got, want, f, dtype=F32):
    """Worst (|got - want| - u_T |want| - m_T) / (2^-24 F) over the finite elements: the C this result needs."""
    ok = np.isfinite(want) & np.isfinite(f) & np.isfinite(got) & (f > 0)
    if not ok.any():
        return 0.0
    err = np.abs(got[ok] - want[ok]) - UNIT[dtype] * np.abs(want[ok]) - TINY[dtype]
    return float(np.max(np.maximum(err, 0.0) / (EPS32 * f[ok])))


def mismatch(got, want, allowed, where=None):
    """None, or a description of the first and of the worst element at which ``got`` leaves the bar.  NaN must meet NaN, an infinity the
    same infinity; every other element |got - want| <= allowed.  ``where``: flat index -> words (the trip of a grid-stride loop)."""
    got, want, allowed = (np.asarray(t, dtype=np.float64).reshape(-1) for t in (got, want, np.broadcast_to(allowed, np.shape(want))))
    assert got.shape == want.shape, (got.shape, want.shape)
    nan_w, nan_g = np.isnan(want), np.isnan(got)
    inf_w = np.isinf(want)
    with np.errstate(invalid='ignore'):
        err = np.abs(got - want)
        bad = np.where(nan_w | nan_g, nan_w != nan_g, np.where(inf_w | np.isinf(got), got != want, ~(err <= allowed)))
    if not bad.any():
        return None
    idx = np.flatnonzero(bad)
    first = int(idx[0])
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(bad & np.isfinite(err) & (allowed > 0), err / allowed, np.where(bad, np.inf, 0.0))
    worst = int(np.argmax(ratio))
    msg = (f'{idx.size} of {got.size} elements outside the bar; first at {first}: got {float(got[first])!r} want {float(want[first])!r} '
           f'bar {allowed[first]:.3e}; worst at {worst}: got {float(got[worst])!r} want {float(want[worst])!r} bar {allowed[worst]:.3e}')
    if where is not None:
        msg += f'; first is {where(first)}, last at {int(idx[-1])} is {where(int(idx[-1]))}'
    return msg


# ---------------------------------------------------------------------------------------------------------------- which kernel, which trip
def vector_width(dtype):
    return 4 if dtype == F32 else 8


def kernel_of(shape, dim, dtype, with_b, aligned=True):
    """The host's choice restated (launch_bias_act): 16-byte vectors when the size, every pointer and the bias run allow it."""
    numel, v = int(np.prod(shape)), vector_width(dtype)
    inner = int(np.prod(shape[dim + 1:])) if with_b else 1
    return 'vector' if (numel % v == 0 and aligned and (not with_b or inner % v == 0)) else 'element'


def position(kernel, numel, dtype):
    """flat index -> 'trip k' of the grid-stride loop (0 is the first), or the element kernel's tail."""
    def where(i):
        if kernel == 'vector':
            return f'trip {(i // vector_width(dtype)) // GRID_THREADS} of the vector loop'
        body = (numel >> 2) << 2
        if i < body:
            return f'trip {(i >> 2) // GRID_THREADS} of the element loop'
        return f'tail element {i - body} of {numel - body} (after {-(-(numel >> 2) // GRID_THREADS)} trips)'
    return where


def trips(kernel, numel, dtype):
    per = vector_width(dtype) if kernel == 'vector' else 4
    return -(-(numel // per) // GRID_THREADS)


# ---------------------------------------------------------------------------------------------------------------- inputs
GAIN = 1.3
ALPHA = 0.3
# a clamp that bites on a fifth to a half of N(0, 1) inputs at gain 1.3; representable in bfloat16, so that a clamped 16-bit output is
# stored ON the clamp and modes 1 and 2 mask it (0.9 would be stored as 0.8999 in float16: inside the open interval)
CLAMP = {'linear': 1.0, 'relu': 1.0, 'lrelu': 1.0, 'tanh': 0.875, 'sigmoid': 0.75, 'elu': 1.0, 'selu': 1.0, 'softplus': 1.25, 'swish': 0.6875}

# (id, shape, dim): the vector kernel; the element kernel with numel % 4 = 1, 2, 3 (its tail loop) and on the 2-D [N, C] input
LAYOUTS = [
    ('vec', (3, 5, 12, 16), 1),
    ('elem_tail1', (3, 5, 9, 19), 1),
    ('elem_tail2', (2, 7, 9, 23), 1),
    ('elem_tail3', (3, 5, 11, 19), 1),
    ('elem_nc', (480, 6), 1),
]

# second trips: (id, kernel, shape by dtype)
SECOND_TRIP = [
    ('vec', 'vector', {F32: (2, 3, 700, 504), F16: (4, 3, 700, 504), BF16: (4, 3, 700, 504)}),
    ('elem', 'element', {F32: (2, 3, 701, 503), F16: (2, 3, 701, 503), BF16: (2, 3, 701, 503)}),
]


def swish_margin_count(xref, b, dim, gain, clamp):
    """Elements whose float64 swish output lies within SWISH_MARGIN (relative) of the clamp: where the kernel's fp32 recomputation of the
    saved output could fall on the other side."""
    if clamp is None or clamp < 0:
        return 0
    c = float(np.float32(clamp))
    y = evaluate(0, 'swish', xref, b, None, None, None, dim, 0.0, gain, None)
    return int(np.count_nonzero(~(np.abs(np.abs(y) - c) > SWISH_MARGIN * c)))


def clear_swish_margin(xref, b, dim, gain, clamp, dtype):
    """``xref`` with the offenders of swish_margin_count MOVED (halved; exact in every type), never dropped."""
    if clamp is None or clamp < 0:
        return xref
    c = float(np.float32(clamp))
    for _ in range(8):
        y = evaluate(0, 'swish', xref, b, None, None, None, dim, 0.0, gain, None)
        near = ~(np.abs(np.abs(y) - c) > SWISH_MARGIN * c)
        if not near.any():
            break
        xref = quantize(np.where(near, xref * 0.5, xref), dtype)
    return xref


def operands(act, shape, dim, dtype, seed, gain=GAIN, alpha=ALPHA, clamp='default', with_b=True, nb_scale=0.3):
    """Everything the three modes take, all representable in ``dtype``, as float64 numpy arrays:
      x      the forward input (also the saved input xref of modes 1 and 2)
      b      the bias along ``dim``
      y      the saved output: the float64 forward result rounded to ``dtype`` (what a forward launch stores)
      g, q   the operands modes 1 and 2 forward (the incoming gradient and the incoming second-order term); g is also mode 2's dy
    Swish with a clamp: x is moved off the clamp margin."""
    clamp = CLAMP[act] if clamp == 'default' else clamp
    x = rounded(shape, dtype, seed)
    b = rounded([shape[dim]], dtype, seed + 1, nb_scale) if with_b else None
    if act == 'swish':
        x = clear_swish_margin(x, b, dim, gain, clamp, dtype)
    y = quantize(evaluate(0, act, x, b, None, None, None, dim, alpha, gain, clamp), dtype)
    g = rounded(shape, dtype, seed + 2)
    q = rounded(shape, dtype, seed + 3)
    return dict(x=x, b=b, y=y, g=g, q=q, dim=dim, alpha=alpha, gain=gain, clamp=clamp, act=act, dtype=dtype)


def layout_operands(act, layout, dtype):
    """The operands of test (a) for one activation, layout of LAYOUTS and type: 3 to 7 bias channels, gain 1.3, the biting clamp."""
    lid, shape, dim = layout
    seed = 1000 + 100 * ACTS.index(act) + 10 * [l[0] for l in LAYOUTS].index(lid) + DTYPES.index(dtype)
    return operands(act, shape, dim, dtype, seed)


def second_trip_operands(case, dtype):
    """The operands of test (b): swish (mode 2 reads every operand) with bias and clamp on a tensor past one full grid."""
    cid, _, shapes = case
    return operands('swish', shapes[dtype], 1, dtype, 7000 + 10 * [c[0] for c in SECOND_TRIP].index(cid) + DTYPES.index(dtype))


# host dispatch, test (d): (id, shape, dim, with bias, kernel in fp32, kernel in 16 bit)
DISPATCH = [
    ('no_bias_ragged', (3, 5, 7, 9), 1, False, 'element', 'element'),        # numel 945: b = None and numel % V != 0
    ('no_bias_odd_inner', (8, 3, 5, 7), 1, False, 'vector', 'vector'),       # numel 840 = 8 * 105: no bias, so the odd inner does not matter
    ('below_one_vector', (3,), 0, True, 'element', 'element'),
    ('one_element', (1,), 0, True, 'element', 'element'),
]
DISPATCH_ACTS = ['tanh', 'swish']
OFFSET_SHAPE = (3, 5, 12, 16)                                                # vector-eligible: only the pointer sends it to the element kernel

# layouts through the autograd op, test (e): (shape, dim)
AUTOGRAD_LAYOUTS = [((7,), 0), ((6, 5), 0), ((6, 5), 1), ((2, 3, 4, 8), 0), ((2, 3, 4, 8), 2), ((2, 3, 4, 8), 3),
                    ((2, 3, 2, 4, 8), 0), ((2, 3, 2, 4, 8), 2), ((2, 3, 2, 4, 8), 4)]
AUTOGRAD_ACTS = ['tanh', 'swish', 'lrelu']
AUTOGRAD_DTYPES = [F32, BF16]


def dispatch_operands(case, act, dtype):
    cid, shape, dim, with_b = case[:4]
    seed = 3000 + 100 * [c[0] for c in DISPATCH].index(cid) + 10 * ACTS.index(act) + DTYPES.index(dtype)
    return operands(act, shape, dim, dtype, seed, with_b=with_b)


def offset_operands(dtype):
    return operands('tanh', OFFSET_SHAPE, 1, dtype, 3900 + DTYPES.index(dtype))


def autograd_operands(act, shape, dim, dtype):
    seed = 4000 + 100 * AUTOGRAD_LAYOUTS.index((shape, dim)) + 10 * ACTS.index(act) + DTYPES.index(dtype)
    return operands(act, shape, dim, dtype, seed)


def swish_clamp_cases():
    """(name, operands) of every case of test_gpu_bias_act.py that runs swish with a clamp in mode 1 or 2."""
    for layout in LAYOUTS:
        for dtype in DTYPES:
            yield f'a/{layout[0]}/{DTYPE_ID[dtype]}', layout_operands('swish', layout, dtype)
    for case in SECOND_TRIP:
        for dtype in DTYPES:
            yield f'b/{case[0]}/{DTYPE_ID[dtype]}', second_trip_operands(case, dtype)
    for case in DISPATCH:
        for dtype in DTYPES:
            yield f'd/{case[0]}/{DTYPE_ID[dtype]}', dispatch_operands(case, 'swish', dtype)
    for shape, dim in AUTOGRAD_LAYOUTS:
        for dtype in AUTOGRAD_DTYPES:
            yield f'e/{shape}/{dim}/{DTYPE_ID[dtype]}', autograd_operands('swish', shape, dim, dtype)


def mode_operands(o, mode):
    """(x, b, xref, yref, dy) of one mode from ``operands``' dict: what autograd hands the kernel."""
    if mode == 0:
        return o['x'], o['b'], None, None, None
    if mode == 1:
        return o['g'], o['b'], o['x'], o['y'], None
    return o['q'], o['b'], o['x'], o['y'], o['g']


# ---------------------------------------------------------------------------------------------------------------- saturation grids
SATURATION_MODES = {'tanh': (0,), 'sigmoid': (0,), 'softplus': (0,), 'swish': (0, 1, 2)}      # the modes with a |x| > 80 or xref > 40 branch
GRID_GAIN = 0.75              # keeps 6e4 * 1.1 (the largest swish slope) inside float16
_GRID_POINTS = (20, 29.5, 30, 35, 39.5, 40, 44, 79, 80, 81, 88, 100)


def _neighbours(v, dtype):
    ulp = 2.0 ** math.floor(math.log2(v)) * 2 * UNIT[dtype]
    return [v - ulp, v + ulp]


def saturation_points(dtype):
    """The values around the kernel's cuts, both signs: the listed points, +-80 and +-40 with their representable neighbours on both sides,
    0 and +-1 as ordinary company; +-1000 in 16 bit and +-65504 in float16."""
    pts = list(_GRID_POINTS) + _neighbours(40.0, dtype) + _neighbours(80.0, dtype) + [1.0]
    if dtype != F32:
        pts.append(1000.0)
    if dtype == F16:
        pts.append(65504.0)
    pts = np.array(sorted(pts))
    grid = quantize(np.concatenate([-pts[::-1], [0.0], pts]), dtype)
    assert np.unique(grid).size == grid.size, 'a neighbour collapsed onto its point'
    return grid


def forwarded_magnitudes(dtype):
    mags = [1.0, 1e3, 7e3, 6e4] + ([1e30] if dtype != F16 else [])
    return quantize(np.array(mags), dtype)


def saturation_case(act, mode, dtype):
    """1-D operands (x, b, xref, yref, dy) of a saturation grid: mode 0 runs the points themselves; swish modes 1 and 2 cross the
    points (as saved input) with the forwarded magnitudes, signs alternating."""
    pts = saturation_points(dtype)
    if mode == 0:
        return pts, None, None, None, None
    assert act == 'swish'
    mags = forwarded_magnitudes(dtype)
    xref = np.repeat(pts, mags.size)
    x = np.tile(mags, pts.size) * np.where(np.arange(xref.size) % 3 == 2, -1.0, 1.0)
    return x, None, xref, None, None
