"""The statement of the per-plane normalisers (include/afcm_hip.h) restated the slow way -- sort the plane and index it; add the
strided partials one Python float at a time -- plus the planes the CPU and GPU tests share.  Nothing here imports afcm_amd: the restatement is held to
numpy's own expressions and to the golden captured from the reference's classes (tests/test_normalise_ref_cpu.py), and the package's host and device
arms are then held to it."""
import numpy as np

from intensity_ref import DTYPES, percentile, same_bits  # noqa: F401
from percentile_clip_ref import rank_percentile, signed_digit_values  # noqa: F401

EPS = 1e-10
PARTIALS = 256

# The bound on the standard deviation, relative, c n 2^-53 with n the pixels of the plane.  In the stated order a term passes through at most
# D = ceil(n / 256) + 8 additions (its partial's, then the tree's eight levels), so a sum of non-negative terms carries a relative error below
# D u (1 + O(u)), u = 2^-53.  A squared deviation carries 3 u (the subtraction, twice in the product, and the product's own rounding); the mean,
# off by at most (D + 1) u mean|m|, moves the sum of squares by n delta^2 only (the cross term vanishes at the exact mean), second order in u as
# long as the plane's variance is not below its mean square by a factor near u.  The division and the root add 2 u, the root halves the rest:
# (D + 3) / 2 + 2 <= n for every n >= 9 at D <= n / 256 + 9.  numpy's own pairwise sums obey the same form with D = n at the worst, so the
# difference of the two arms is below 2 n u: c = 2.  math.fsum, exact, checks both (tests/test_normalise_ref_cpu.py).
C_STD = 2.0


def std_bound(n):
    return C_STD * n * 2.0 ** -53


def ordered_sum(x):
    """One Python float at a time: partial t adds x[t], x[t + 256], ... in ascending order onto +0.0; the tree s[t] += s[t + o], o = 128 ... 1."""
    x = [float(v) for v in np.asarray(x, dtype=np.float64).reshape(-1)]
    part = [0.0] * PARTIALS
    for t in range(PARTIALS):
        for v in x[t::PARTIALS]:
            part[t] = part[t] + v
    off = PARTIALS // 2
    while off >= 1:
        for t in range(off):
            part[t] = part[t] + part[t + off]
        off //= 2
    return np.float64(part[0])


def record(plane, percentile_pair=None, standardize=None, eps=EPS):
    """(sub, div, stat0, stat1) of one plane: ``percentile_pair=(pmin, pmax)``, ``standardize=True`` or ``standardize=(mean, std)``."""
    v = np.asarray(plane).astype(np.float64).reshape(-1)   # the widening is exact and keeps the order
    eps = np.float64(eps)
    with np.errstate(all='ignore'):
        if percentile_pair is not None:
            lo = hi = np.float64(np.nan)
            if not np.isnan(v).any():
                s = np.sort(v) + 0.0                       # -0.0 -> +0.0
                lo, hi = percentile(s, percentile_pair[0]), percentile(s, percentile_pair[1])
            return np.array([lo, (hi - lo) + eps, lo, hi])
        if standardize is True:
            n = np.float64(v.shape[0])
            mean = ordered_sum(v) / n
            d = v - mean
            std = np.sqrt(ordered_sum(d * d) / n)
        else:
            mean, std = (np.float64(x) for x in standardize)
        return np.array([mean, eps if std < eps else std, mean, std])


def apply(plane, rec, then=None):
    """(m - sub) / div in float64, then -- ``then=(min_value, max_value)`` -- Normalize; one rounding to float32."""
    with np.errstate(all='ignore'):
        out = (np.asarray(plane).astype(np.float64) - rec[0]) / rec[1]
        if then is not None:
            out = 2.0 * ((out - np.float64(then[0])) / (np.float64(then[1]) - np.float64(then[0]))) - 1.0
            out = np.where(out < -1.0, -1.0, np.where(out > 1.0, 1.0, out))
    return out.astype(np.float32)


def item_plane(volume, pos, h, w):
    """The [h, w] item plane of slice ``pos`` of ``volume`` [D, Hs, Ws]: centred crop / zero pad; float64 zeros outside the volume."""
    d, hs, ws = volume.shape
    if not 0 <= pos <= d - 1:
        return np.zeros((h, w), dtype=np.float64)
    out = np.zeros((h, w), dtype=volume.dtype)
    oy = (hs - h) // 2 if h < hs else -((h - hs) // 2)
    ox = (ws - w) // 2 if w < ws else -((w - ws) // 2)
    for y in range(h):
        for x in range(w):
            if 0 <= y + oy < hs and 0 <= x + ox < ws:
                out[y, x] = volume[pos, y + oy, x + ox]
    return out


def positions(idx, thickness, k):
    """The slice positions of the k input planes of target ``idx``."""
    if k == 1:
        return [idx]
    own = (idx // thickness) * thickness
    return [own - thickness, own, own + thickness, own + 2 * thickness]


def plane_of(values, h, w, dtype, fill=None, seed=0):
    """An [h, w] plane of ``dtype`` that holds ``values`` at shuffled places and ``fill`` (default: the first value) everywhere else."""
    values = np.asarray(values, dtype=dtype).reshape(-1)
    assert values.shape[0] <= h * w
    flat = np.full(h * w, values[0] if fill is None else fill, dtype=dtype)
    flat[:values.shape[0]] = values
    return flat[np.random.default_rng(seed).permutation(h * w)].reshape(h, w)


def select_cases(dtype):
    """{name: (plane [h, w] of dtype, [(pmin, pmax), ...])}: the select's edge cases for one source dtype."""
    dtype = np.dtype(dtype)
    cases = {}
    rng = np.random.default_rng(dtype.itemsize)
    if dtype.kind == 'f':
        digits = signed_digit_values(dtype, 67)
    elif dtype == np.int16:                                # both bytes differ between neighbours wherever 67 values allow: steps of 257 across zero
        digits = (np.arange(67) - 33) * 257 + rng.integers(-100, 100, 67)
    else:
        digits = np.sort(rng.choice(256, 67, replace=False))
    digits = np.sort(np.asarray(digits, dtype=dtype))
    # every rank of 67 distinct keys: percentile pairs that land on rank r and on the rank from the other end, exactly (g = 0), and in between
    pairs = [(rank_percentile(r, 67), rank_percentile(66 - r, 67)) for r in range(34)] + [(rank_percentile(33, 67), rank_percentile(33, 67))]
    pairs = [(min(a, b), max(a, b)) for a, b in pairs] + [(12.3, 77.7), (0.0, 100.0)]
    cases['digits67'] = (plane_of(digits, 1, 67, dtype, seed=1), pairs)
    # neighbouring ranks across a bin boundary of each pass: keys ... 0xff | 0x00 ... at every digit, and a lerp between the two
    if dtype.kind == 'f':
        uint = np.uint32 if dtype.itemsize == 4 else np.uint64
        base = int(np.array(1.5, dtype=dtype).view(uint))
        seams = []
        for byte in range(dtype.itemsize):
            hi_bits = (base >> (8 * (byte + 1))) << (8 * (byte + 1))
            if byte == 0:
                seams += [base | 0xff, (base | 0xff) + 1]
            elif hi_bits > 0:                              # the top digit's own boundary is the one between the signs
                seams += [hi_bits - 1, hi_bits]
        seam_values = np.array(sorted(set(seams)), dtype=uint).view(dtype)
        seam_values = np.concatenate([seam_values, -seam_values])
    elif dtype == np.int16:
        seam_values = np.array([-257, -256, -1, 0, 255, 256, 511, 512, -32768, 32767], dtype=np.int16)     # the sign seam and byte seams
    else:
        seam_values = np.array([0, 1, 127, 128, 254, 255], dtype=np.uint8)
    n = seam_values.shape[0]
    cases['seams'] = (plane_of(seam_values, 1, n, dtype, seed=2),
                      [(rank_percentile(r, n), rank_percentile(r + 1, n)) for r in range(n - 1)] + [(50.0 / (n - 1), 99.0)])
    # ties: three values, long runs of each
    ties = np.repeat(np.asarray([digits[3], digits[30], digits[60]], dtype=dtype), (20, 9, 6))
    cases['ties'] = (plane_of(ties, 5, 7, dtype, seed=3), [(1.0, 99.6), (50.0, 60.0), (57.0, 83.0), (0.0, 100.0)])
    cases['all_equal'] = (np.full((5, 7), digits[40], dtype=dtype), [(1.0, 99.6), (0.0, 100.0)])
    if dtype.kind == 'f':
        tiny = np.finfo(dtype).tiny
        special = np.array([np.inf, -np.inf, -0.0, 0.0, tiny / 4, -tiny / 4, tiny, 1.0, -1.0, np.finfo(dtype).max], dtype=dtype)
        cases['specials'] = (plane_of(special, 5, 7, dtype, fill=0.5, seed=4), [(10.0, 90.0), (0.0, 100.0), (3.0, 97.0), (20.0, 40.0)])
        zeros = np.array([-0.0] * 20 + [0.0] * 10 + [-1.0, 1.0, 2.0, -2.0, 3.0], dtype=dtype)
        cases['signed_zeros'] = (plane_of(zeros, 5, 7, dtype, seed=5), [(20.0, 80.0), (30.0, 55.0)])
        for at in (0, 17, 34):
            with_nan = plane_of(digits[:35], 5, 7, dtype, seed=6).copy()
            with_nan.reshape(-1)[at] = np.nan
            cases[f'nan_at_{at}'] = (with_nan, [(1.0, 99.6)])
    return cases
