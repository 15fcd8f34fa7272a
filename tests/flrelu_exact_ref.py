"""Operands for which filtered_lrelu has ONE right answer, the float64 reference, and the check that makes it so
(tests/test_flrelu_exact_ref_cpu.py proves the conditions without a GPU, tests/test_gpu_flrelu_exact.py compares with ``torch.equal``).

The other tests of the 16-bit kernels allow 4e-2 (bfloat16) / 6e-3 (float16) of max(1, |ref|max): honest about 16-bit rounding of
operands and intermediates, and 10 - 100 times an outer tap of the Kaiser filters, a tap dropped at a seam, a polyphase offset wrong
for one row parity, a K window one row short or a `>` for a `>=` at the clamp.  Around its one nonlinearity the op is linear and the filters, the
gain and the slope are call arguments, so the data can be chosen such that nothing a kernel rounds is rounded:

**Representability rule.**  Integer filters (every tap +-1 or +-2, none zero, no two neighbours equal, not symmetric), inputs in
{-1, 0, 1}, gain 1 (so that every factor the host derives from it -- gain up^2, gain up^2 / down^2 -- is a power of two), a slope
that is a power of two, a clamp that is infinite or a power of two, integer bias and skip, power-of-two plane factors.  ``representable``
then computes in int64, for both pass orders (columns first, rows first), every quantity a kernel family stores in 16 bits

    x + b | X1 (one up pass) | X2 (both, times gain up^2) | lrelu(X2) clamped, relu(X2) | X3 (one down pass)
    the coefficient sets  UV gain up^2 | slope DV | (1 - slope) DV | slope DV UV gain up^2 (the wave kernels' composite operator)

-- and for the transposed (sign-reading) call the same list with the roles swapped and the factor {1, slope, 0} looked up by code in
place of the leaky ReLU (X2 f and X2 [code 0], the two operands its kernels form) -- and returns the share of elements whose odd part
fits the significand of the dtype (11 bits float16, 8 bits bfloat16, 24 bits float32) inside its normal range.  Where that share is
1.0 every product is exact, every fp32 partial sum of every summation order is a multiple of one quantum and below 2^24 of it
(``accumulation_units``, a bound on the absolute sums: 2^21 at most here), hence exact, and the one rounding left is the output's: the reference is the float64 definition (oracle.direct_np; flrelu_read_ref.read_reference with the
written codes for the transposed call) rounded ONCE to nearest even, and a kernel either equals it or is wrong.  The condition is
checked on the reference, never on the code under test; a case that misses it gets another seed (SEEDS, searched on the CPU), never
an excuse.

**Probed widths** (significand bits of the widest element over both calls and both pass orders; 2 x 2 planes per case; ``widths``):

    float16 (11 bits), dense {-1, 0, 1}, slope 1/4:      X1 3 - 5, X2 5 - 7, X3 8 - 11 (11: the cases with a bias, the down-4 read calls)
    bfloat16 (8 bits), +-1 at 3 % (up 4: 5 %), slope 1/2: X1 1 - 3, X2 3 - 5, X3 6 - 8
    float32 strip kernel, dense, slope 1/4:               X3 10, outputs 11 - 13 of 24 bits
    fp32 accumulators of the 16-bit outputs:              9 - 14 of 24 bits

bfloat16 at 6 - 8 % density, or with taps up to +-3, needs 9 bits for X3: the bfloat16 cases stay sparse, and their bias is zero (a
dense x + b pushes X3 past 8 bits); at 3 % a fifth of the outputs of an up-4 call are 0, hence its 5 %.  Slope 1/2 makes slope =
1 - slope; the float16 cases, at 1/4, tell the two coefficient sets apart.  Every case passes with the first draw but two (SEEDS: fewer than 90 % of the outputs non-zero).
The plane sums of the transposed call are compared where the UNROUNDED dx is representable too: the float32 cases and the float16
cases with a 4 % cotangent (`sparseg`); in bfloat16 a single product of two composite taps already needs more than 8 bits.

**Paths at one ulp instead of equality:** none.
"""
import functools
import zlib

import numpy as np

from oracle import direct_np as dnp

import flrelu_read_ref as R

INF = R.INF
SIG_BITS = {'float16': 11, 'bfloat16': 8, 'float32': 24}
MIN_EXP = {'float16': -14, 'bfloat16': -126, 'float32': -126}            # smallest normal exponent
MAX_EXP = {'float16': 15, 'bfloat16': 127, 'float32': 127}
GAIN = 1.0
SLOPE = {'float16': 0.25, 'bfloat16': 0.5, 'float32': 0.25}
DENSITY = {'float16': None, 'bfloat16': 0.03, 'float32': None}             # None: dense {-1, 0, 1}
# up 4 spreads an input over 16 upsampled positions with a quarter of the taps each: at 3 % a fifth of its bfloat16 outputs are 0,
# and X3 stays within 8 bits up to 5 %
DENSITY_UP4 = {'bfloat16': 0.05}
# cotangents of the plane-sum cases: sparse enough that the UNROUNDED dx is a tensor of the dtype's values
DENSITY_SPARSE_G = {'float16': 0.04}

# Integer filters in the roles of f12 / f24 / f24u of flrelu_read_ref.KERNELS: +-1 with a few +-2, no zero tap, no two neighbours
# equal (a swap of adjacent taps always changes the filter), the overlap of the filter with any shift of itself differs (no tap
# offset maps it onto itself), not symmetric (test_flrelu_exact_ref_cpu.py::test_filters).
FILTERS = {
    'f12': (1, -1, 1, 2, -1, 1, -2, 1, -1, 1, -1, 2),
    'f24': (1, -1, 2, -1, 1, -1, 1, -2, 1, -1, 1, 2, -1, 1, -1, -2, 1, -1, 2, 1, -1, 1, -2, 2),
    'f24u': (-1, 1, -2, 1, -1, 2, 1, -1, 1, -1, 1, -1, 2, -1, 1, -2, -1, 1, -1, 1, 2, -1, 2, -2),
}


def filt(name):
    return np.asarray(FILTERS[name], dtype=np.float32)


# ------------------------------------------------------------------------------------------------- int64 passes
def _taps(f, flip):
    """Correlation taps of a call: the filter itself when flipped, else reversed (oracle.direct_np.upfirdn2d)."""
    f = np.asarray(f, dtype=np.int64)
    return f if flip else f[::-1]


def _place(x, up, lo, hi, axis):
    """Along `axis`: sample i at i up, zeros between, then lo / hi zeros in front / behind (negative: crop).  int64."""
    x = np.moveaxis(x, axis, -1)
    n = x.shape[-1]
    total = n * up + lo + hi
    out = np.zeros(x.shape[:-1] + (max(total, 0),), dtype=np.int64)
    for i in range(n):
        d = i * up + lo
        if 0 <= d < total:
            out[..., d] = x[..., i]
    return np.moveaxis(out, -1, axis)


def _fir(z, taps, down, axis):
    """out[o] = sum_k taps[k] z[o down + k] along `axis`, int64."""
    z = np.moveaxis(z, axis, -1)
    k = len(taps)
    full = z.shape[-1] - k + 1
    assert full >= 1
    nout = (full + down - 1) // down
    out = np.zeros(z.shape[:-1] + (nout,), dtype=np.int64)
    for t in range(k):
        out += int(taps[t]) * z[..., t:t + (nout - 1) * down + 1:down]
    return np.moveaxis(out, -1, axis)


def _up(x, taps, up, lo, hi, axis):
    return _fir(_place(x, up, lo, hi, axis), taps, 1, axis)


UNIT = 1 << 8                # fixed point of the factors: gain up^2 and the slope are whole multiples of 1 / 256


def _fixed(v):
    q = v * UNIT
    assert q == int(q) and int(q) != 0 and (int(q) & (int(q) - 1)) == 0, f'{v} is no power of two within 2^-8'
    return int(q)


def fits(q, log2_unit, dtype):
    """Per element of the int64 array q (values q 2^log2_unit): is it a value of `dtype` -- odd part within the significand, the
    leading bit inside the normal range."""
    a = np.abs(q.astype(np.int64))
    low = a & -a                                                    # lowest set bit (0 for 0)
    odd = np.where(a == 0, 0, a // np.maximum(low, 1))
    ok = odd < (1 << SIG_BITS[dtype])
    top = np.floor(np.log2(np.maximum(a, 1).astype(np.float64))).astype(np.int64) + log2_unit
    bottom = np.log2(np.maximum(low, 1).astype(np.float64)).astype(np.int64) + log2_unit
    return (a == 0) | (ok & (top <= MAX_EXP[dtype]) & (bottom >= MIN_EXP[dtype] - (SIG_BITS[dtype] - 1)) & (top >= MIN_EXP[dtype]))


def width(q):
    """Significand bits of the widest element of q (its odd part's bit length)."""
    a = np.abs(q.astype(np.int64)).ravel()
    a = a[a != 0]
    if a.size == 0:
        return 0
    return int((a // (a & -a)).max()).bit_length()


def _chain(x, fu, fd, up, down, padding, flip, gain_total, act):
    """Every rounded quantity of one call as [(name, int64 array, log2 of its unit)].  x: int64 [N, C, H, W] (bias added);
    gain_total = gain up^2; act(X2 in units of 1 / 256) -> [(name, array in units of 2^-16)], the first of which feeds the
    down passes."""
    px0, px1, py0, py1 = padding
    tu, td = _taps(fu, flip), _taps(fd, flip)
    g = _fixed(gain_total)
    out = [('x + b', x, 0)]
    x1x = _up(x, tu, up, px0, px1, 3)
    x1y = _up(x, tu, up, py0, py1, 2)
    out += [('X1 columns first', x1x, 0), ('X1 rows first', x1y, 0)]
    x2 = _up(x1x, tu, up, py0, py1, 2)
    assert np.array_equal(x2, _up(x1y, tu, up, px0, px1, 3))
    x2 = x2 * g
    out.append(('X2', x2, -8))
    acts = act(x2)
    out += [(n, a, -16) for n, a in acts]
    v = acts[0][1]
    x3y, x3x = _fir(v, td, down, 2), _fir(v, td, down, 3)
    out += [('X3 rows first', x3y, -16), ('X3 columns first', x3x, -16)]
    y = _fir(x3y, td, down, 3)
    assert np.array_equal(y, _fir(x3x, td, down, 2))
    out.append(('y (fp32 accumulator)', y, -16))
    return out


def _coefficients(fu, fd, up, down, padding, flip, gain_total, slope, shape):
    """The coefficient sets a matrix-core kernel stores in 16 bits: UV gain up^2, slope DV, (1 - slope) DV, and the composite
    slope DV UV gain up^2 of the wave kernels -- every entry of the operator `down pass . up pass` along each axis, from the
    identity."""
    tu, td = _taps(fu, flip), _taps(fd, flip)
    g, s = _fixed(gain_total), _fixed(slope)
    out = [('UV gain', tu * g, -8), ('slope DV', td * s, -8), ('(1 - slope) DV', td * (UNIT - s), -8)]
    for n, lo, hi, name in ((shape[2], padding[2], padding[3], 'rows'), (shape[3], padding[0], padding[1], 'columns')):
        comp = _fir(_up(np.eye(n, dtype=np.int64), tu, up, lo, hi, 0), td, down, 0)
        out.append((f'slope DV UV gain, {name}', comp * g * s, -16))
    return out


def _forward_act(slope, clamp):
    s = _fixed(slope)

    def act(x2):
        v = np.where(x2 < 0, x2 * s, x2 * UNIT)                                  # units of 2^-16
        if clamp != INF:
            c = int(clamp * UNIT * UNIT)
            v = np.clip(v, -c, c)
        return [('lrelu(X2)', v), ('relu(X2)', np.maximum(x2, 0) * UNIT)]
    return act


def _read_act(slope, codes, sx, sy):
    s = _fixed(slope)

    def act(x2):
        c = R.window_codes(codes, x2.shape[2], x2.shape[3], sx, sy)
        f = np.array([UNIT, s, 0, 0], dtype=np.int64)[c]
        return [('X2 f(code)', x2 * f), ('X2 [code 0]', np.where(c == 0, x2, 0) * UNIT)]
    return act


def quantities(case, which='forward'):
    """[(name, int64 array, log2 unit)] of the forward of `case`, or of the sign-reading call behind its backward."""
    d = data(case)
    if which == 'forward':
        x = d['x'].astype(np.int64)
        if d['b'] is not None:
            x = x + d['b'].astype(np.int64).reshape(1, -1, 1, 1)
        up, down = case['up'], case['down']
        gt = GAIN * up * up
        return (_chain(x, d['fu'], d['fd'], up, down, case['padding'], case['flip'], gt, _forward_act(case['slope'], case['clamp']))
                + _coefficients(d['fu'], d['fd'], up, down, case['padding'], case['flip'], gt, case['slope'], x.shape))
    bcfg = backward_cfg(case)
    up, down, px0, px1, py0, py1, gg, slope, _, flip, sx, sy = bcfg[:12]
    g = d['g'].astype(np.int64)
    gt = gg * up * up
    return (_chain(g, d['fd'], d['fu'], up, down, [px0, px1, py0, py1], flip, gt, _read_act(slope, reference(case)['codes'], sx, sy))
            + _coefficients(d['fd'], d['fu'], up, down, [px0, px1, py0, py1], flip, gt, slope, g.shape))


def representable(case):
    """Share of the elements of every quantity a kernel rounds to the case's dtype, forward and transposed call, both pass orders,
    that the dtype holds exactly.  The fp32 accumulators of the outputs are held to float32."""
    good = total = 0
    for which in ('forward', 'backward'):
        for name, q, lg in quantities(case, which):
            ok = fits(q, lg, 'float32' if name.startswith('y ') else case['dtype'])
            good, total = good + int(ok.sum()), total + ok.size
    return good / total


def accumulation_units(case):
    """Upper bound of the absolute value of every fp32 partial sum of both calls, whatever the order of summation, in units of the
    terms' quantum: the op on |x|, |taps| without slope or clamp, over slope gain up^2 (every activated value, and every
    coefficient of the composite operator times an X1, is a whole multiple of that; the passes before it sum integers).  Below
    2^24 no partial sum can round."""
    d = data(case)
    worst = 0.0
    for which in ('forward', 'backward'):
        if which == 'forward':
            x = np.abs(d['x']) + (0 if d['b'] is None else np.abs(d['b']).reshape(1, -1, 1, 1))
            fu, fd, up, down, padding, gt, slope = d['fu'], d['fd'], case['up'], case['down'], case['padding'], GAIN * case['up'] ** 2, case['slope']
        else:
            bcfg = backward_cfg(case)
            x, fu, fd, up, down, padding, gt, slope = np.abs(d['g']), d['fd'], d['fu'], bcfg[0], bcfg[1], list(bcfg[2:6]), bcfg[6] * bcfg[0] ** 2, bcfg[7]
        big = _chain(x.astype(np.int64), np.abs(fu), np.abs(fd), up, down, padding, False, gt, lambda x2: [('|X2|', x2 * UNIT)])
        worst = max(worst, float(big[-1][1].max()) * 2.0 ** -16 / (slope * gt))
    if d['skip'] is not None:
        worst = (worst + float(np.abs(d['skip']).max()) / (slope * gt)) * float(d['oscale'].max() / d['oscale'].min())
    return worst


def widths(case):
    """{quantity: significand bits of its widest element} -- what the module docstring quotes."""
    out = {}
    for which in ('forward', 'backward'):
        for name, q, _ in quantities(case, which):
            out[f'{which}: {name}'] = width(q)
    return out


# ------------------------------------------------------------------------------------------------- geometry
def _odd_geometry(kern, h, w):
    """Padding of a layout-0 case from its input size (flrelu_read_ref.direct_case: px0 = taps - 3, py0 = taps - 4), px1 / py1 the
    first values >= px0 / py0 with a valid output whose width is ODD: a 16-bit call of odd width runs the exact tile kernels."""
    up, down, fu, fd = R.KERNELS[kern]
    fut, fdt = len(FILTERS[fu]), len(FILTERS[fd])
    px0, py0 = fut - 1 - 2, fut - 1 - 3
    px1 = px0
    while R.out_size(w, up, down, px0, px1, fut, fdt) < 1 or R.out_size(w, up, down, px0, px1, fut, fdt) % 2 == 0:
        px1 += 1
    py1 = R.first_pad(h, up, down, py0, fut, fdt, False)
    return [px0, px1, py0, py1]


def make_case(family, kern, dtype, yh=None, yw=None, hw=None, flip=False, clamp=None, bias=None, epilogue=False, sparse_g=False, tag=''):
    """One case.  family: 'wave' (layout 2) | 'mfma_tile' (layout 1, through a bias operand) | 'tile' (layout 0: 16-bit, odd width) |
    'strip' (layout 0, float32).  Matrix-core families: the output size is given and flrelu_read_ref.geometry finds the input
    and the padding; layout-0 families: the input size is given (flrelu_read_ref.layout0_cases)."""
    up, down, fu, fd = R.KERNELS[kern]
    fut, fdt = len(FILTERS[fu]), len(FILTERS[fd])
    if hw is None:
        h, w, padding = R.geometry(kern, yh, yw, mx={20: 13, 36: 9, 52: 13}.get(yw, 5))       # (mx by width: see _setup of test_gpu_flrelu_lead_edges.py)
    else:
        h, w = hw
        padding = _odd_geometry(kern, h, w)
        yh = R.out_size(h, up, down, padding[2], padding[3], fut, fdt)
        yw = R.out_size(w, up, down, padding[0], padding[1], fut, fdt)
    clamp = INF if clamp is None else clamp * up * up              # (the clamp cases: a multiple of gain up^2, the unit of gain X2)
    layout = {'wave': 2, 'mfma_tile': 1, 'tile': 0, 'strip': 0}[family]
    cid = f'{family}-{kern}-{yh}x{yw}-{dtype}' + (f'-{tag}' if tag else '')
    return dict(id=cid, family=family, layout=layout, kern=kern, dtype=dtype, up=up, down=down, fu=fu, fd=fd, n=2, c=2, h=h, w=w,
                yh=yh, yw=yw, padding=padding, flip=flip, clamp=clamp, bias=bias, epilogue=epilogue, slope=SLOPE[dtype], gain=GAIN,
                density=DENSITY_UP4.get(dtype, DENSITY[dtype]) if up == 4 else DENSITY[dtype],
                g_density=DENSITY_SPARSE_G[dtype] if sparse_g else (DENSITY_UP4.get(dtype, DENSITY[dtype]) if down == 4 else DENSITY[dtype]),
                seed=SEEDS.get(cid, 0))


# Seeds of the draws, searched on the CPU (the first seed for which representable(case) == 1.0 and the coverage conditions of
# test_flrelu_exact_ref_cpu.py hold); a case not listed uses 0.
SEEDS = {'tile-u4d2-37x43-bfloat16': 1, 'tile-u4d2-37x43-bfloat16-flip-clamp': 3}

# Clamps of the clamp cases in units of gain up^2: a power of two that some |gain X2| equal and others exceed (asserted in the CPU
# module).
CLAMP = {'float16': 4.0, 'bfloat16': 2.0}


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for dtype in ('float16', 'bfloat16'):
        for kern in R.KERNELS:
            # wave family: narrower than one piece | the one-tile 48-row strip (up 2 / down 2) | three strips, four column blocks
            out.append(make_case('wave', kern, dtype, 4, 20))
            out.append(make_case('wave', kern, dtype, 36, 36))
            out.append(make_case('wave', kern, dtype, 70, 52))
            out.append(make_case('wave', kern, dtype, 36, 36, flip=True, tag='flip'))
            out.append(make_case('wave', kern, dtype, 36, 36, epilogue=True, tag='skip'))
            out.append(make_case('wave', kern, dtype, 36, 36, clamp=CLAMP[dtype], tag='clamp'))
            if dtype == 'float16':            # (a product of two 5-bit composite taps already exceeds bfloat16's 8 bits)
                out.append(make_case('wave', kern, dtype, 36, 36, sparse_g=True, tag='sparseg'))
            # LDS-tile matrix-core family, through its bias operand (beyond the issue's table: the clamp and the flipped filters in
            # every other family too, one case per kernel)
            bias = (1, -2) if dtype == 'float16' else (0, 0)
            out.append(make_case('mfma_tile', kern, dtype, 36, 36, bias=bias))
            out.append(make_case('mfma_tile', kern, dtype, 70, 36, bias=bias))
            out.append(make_case('mfma_tile', kern, dtype, 36, 36, bias=bias, flip=True, clamp=CLAMP[dtype] * (4 if any(bias) else 1), tag='flip-clamp'))       # (x + b is larger)
            if dtype == 'float16':
                out.append(make_case('mfma_tile', kern, dtype, 36, 36, bias=bias, sparse_g=True, tag='sparseg'))
        # exact 16-bit tile kernels (odd width)
        for kern, hw in (('u2d2', (38, 19)), ('u2d2', (70, 17)), ('u2d4', (30, 25)), ('u4d2', (17, 19))):
            out.append(make_case('tile', kern, dtype, hw=hw))
            if hw[0] != 70:
                out.append(make_case('tile', kern, dtype, hw=hw, flip=True, clamp=CLAMP[dtype], tag='flip-clamp'))
    for kern, hw in (('u2d2', (19, 21)), ('u2d4', (19, 21)), ('u4d2', (19, 21)), ('u2d2', (150, 9))):
        out.append(make_case('strip', kern, 'float32', hw=hw))
        if hw[0] != 150:
            out.append(make_case('strip', kern, 'float32', hw=hw, flip=True, clamp=CLAMP['float16'], tag='flip-clamp'))
    assert len({c['id'] for c in out}) == len(out)
    return tuple(out)


def case_by_id(cid):
    return next(c for c in cases() if c['id'] == cid)


# ------------------------------------------------------------------------------------------------- data and reference
def _draw(rng, shape, density):
    if density is None:
        return rng.integers(-1, 2, size=shape).astype(np.float64)
    return (rng.choice([-1.0, 1.0], size=shape) * (rng.random(shape) < density)).astype(np.float64)


_data_cache = {}


def data(case):
    """x, the cotangent g, bias, skip and plane factors (float64 arrays of integers / powers of two) and the two filters."""
    key = (case['id'], case['seed'])
    if key not in _data_cache:
        rng = np.random.default_rng(zlib.crc32(case['id'].encode()) + 1000 * case['seed'])
        n, c = case['n'], case['c']
        d = dict(x=_draw(rng, (n, c, case['h'], case['w']), case['density']), g=_draw(rng, (n, c, case['yh'], case['yw']), case['g_density']),
                 b=None if case['bias'] is None else np.asarray(case['bias'], dtype=np.float64), skip=None, oscale=None,
                 fu=filt(case['fu']), fd=filt(case['fd']))
        if case['epilogue']:
            d['skip'] = rng.integers(-3, 4, size=(n, c, case['yh'], case['yw'])).astype(np.float64)
            d['oscale'] = 2.0 ** rng.integers(-2, 3, size=n * c)
        _data_cache[key] = d
    return _data_cache[key]


def forward_cfg(case):
    return (case['up'], case['down'], *case['padding'], case['gain'], case['slope'], case['clamp'], case['flip'], 0, 0, 0)


def backward_cfg(case):
    import torch
    from afcm_amd.torch_utils.ops import filtered_lrelu as flr
    d = data(case)
    return flr._backward_cfg(forward_cfg(case), torch.from_numpy(d['fu']), torch.from_numpy(d['fd']), d['x'].shape, d['g'].shape, case['layout'])


_ref_cache = {}


def reference(case):
    """float64 definition of the case, computed once: u (X2 without the gain), codes, F (the op), y ((F + skip) oscale),
    dx (the sign-reading call on g with these codes), psum (its plane sums); `expected_y` / `expected_dx`: rounded once to the
    dtype."""
    key = (case['id'], case['seed'])
    if key in _ref_cache:
        return _ref_cache[key]
    d = data(case)
    xb = d['x'] if d['b'] is None else d['x'] + d['b'].reshape(1, -1, 1, 1)
    u = dnp.upfirdn2d(xb, d['fu'], up=case['up'], padding=case['padding'], gain=float(case['up'] ** 2), flip_filter=case['flip'])
    v, codes = dnp.lrelu_codes(u, case['gain'], case['slope'], None if case['clamp'] == INF else case['clamp'])
    F = dnp.upfirdn2d(v, d['fd'], down=case['down'], flip_filter=case['flip'])
    assert F.shape[2:] == (case['yh'], case['yw'])
    y = F
    if d['skip'] is not None:
        y = (F + d['skip']) * d['oscale'].reshape(case['n'], case['c'], 1, 1)
    ref = dict(u=u, v=v, codes=codes, F=F, y=y, expected_y=round_once(y, case['dtype']))
    _ref_cache[key] = ref                                       # (backward_cfg -> quantities may ask for the codes)
    dx = R.read_reference(d['g'], d['fd'], d['fu'], backward_cfg(case), codes)
    assert dx.shape == d['x'].shape
    ref.update(dx=dx, expected_dx=round_once(dx, case['dtype']), psum=dx.sum((2, 3)))
    return ref


def round_once(a, dtype):
    """float64 -> the nearest value of `dtype` (ties to even) as float64.  flrelu_read_ref.round_to passes through float32: exact
    here, which is asserted, so the 16-bit rounding is the only one."""
    a = np.asarray(a, dtype=np.float64)
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a), 'the reference must be exact in float32'
    return R.round_to(a, dtype)


def dx_representable(case):
    """Is the unrounded dx of the case a tensor of the dtype's values (then the plane sums of the kernel's fp32 accumulators and
    of its rounded outputs coincide, and both equal the float64 sums)?"""
    ref = reference(case)
    return bool(np.array_equal(ref['expected_dx'], ref['dx']))


# ------------------------------------------------------------------------------------------------- teeth
def forward_with(case, fu=None, fd=None, padding=None):
    """The rounded forward reference of `case` with another filter or padding (same data; the output must keep its shape)."""
    d = data(case)
    xb = d['x'] if d['b'] is None else d['x'] + d['b'].reshape(1, -1, 1, 1)
    y = dnp.filtered_lrelu(xb, d['fu'] if fu is None else fu, d['fd'] if fd is None else fd, None, case['up'], case['down'],
                           case['padding'] if padding is None else padding, case['gain'], case['slope'],
                           None if case['clamp'] == INF else case['clamp'], case['flip'])
    return R.round_to(y, case['dtype'])


def blocks_changed(a, b, blk=16):
    """Share of the blk x blk output blocks (edge blocks included) of every plane in which a and b differ."""
    n, c, h, w = a.shape
    hit = tot = 0
    for y0 in range(0, h, blk):
        for x0 in range(0, w, blk):
            diff = (a[:, :, y0:y0 + blk, x0:x0 + blk] != b[:, :, y0:y0 + blk, x0:x0 + blk]).reshape(n, c, -1).any(-1)
            hit, tot = hit + int(diff.sum()), tot + diff.size
    return hit / tot


def filter_variants(f):
    """[(name, filter)]: each single tap zeroed, each pair of adjacent taps swapped."""
    f = np.asarray(f)
    out = []
    for t in range(len(f)):
        g = f.copy()
        g[t] = 0
        out.append((f'tap {t} zeroed', g))
    for t in range(len(f) - 1):
        g = f.copy()
        g[t], g[t + 1] = f[t + 1], f[t]
        out.append((f'taps {t}, {t + 1} swapped', g))
    return out
