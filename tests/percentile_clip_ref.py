"""The statement of the percentile-clip normalisation (include/afcm_hip.h) restated the slow way -- sort every voxel, index -- plus the
volumes the CPU and GPU tests share.  Nothing here imports afcm_amd: the restatement is held to numpy's own percentile and clip arithmetic and to the
golden captured from the reference function (tests/test_percentile_clip_ref_cpu.py), and the package's host and device arms are then held to it."""
import numpy as np

from intensity_ref import DTYPES, percentile  # noqa: F401  (the float64 `linear` percentile of a sorted array, held to numpy's there)


def clip(volume, percentiles=(0.5, 99.5), strictly_positive=True, reference=None):
    """(uint8 volume, float64 [lo, hi, n, nan_count]) of the statement."""
    volume = np.asarray(volume)
    r = (volume if reference is None else np.asarray(reference)).reshape(-1).astype(np.float64)      # the widening is exact and keeps the order
    nans = int(np.isnan(r).sum())
    lo = hi = np.float64(np.nan)
    if nans == 0:
        s = np.sort(r)
        lo, hi = percentile(s, percentiles[0]), percentile(s, percentiles[1])
        if strictly_positive and lo < 0:
            lo = np.float64(0.0)
    with np.errstate(all='ignore'):
        v = volume.astype(np.float64)
        v = np.where(v < lo, lo, v)                        # max(v, lo), then min(.., hi); a NaN voxel stays one
        v = np.where(v > hi, hi, v)
        level = (v - lo) / (hi - lo) * np.float64(255.0)
    level[np.isnan(level)] = 0.0
    return np.trunc(level).astype(np.uint8), np.array([lo, hi, float(r.shape[0]), float(nans)])


def same_stats(a, b):
    """Two stats vectors equal numerically (so -0.0 equals +0.0), NaN matching NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def rank_percentile(r, n):
    """The percentile 100 r / (n - 1), nudged by an ulp or two where that makes q / 100 * (n - 1) land on the rank r exactly (g = 0)."""
    q = 100.0 * r / (n - 1)
    up, down = np.nextafter(q, 200.0), np.nextafter(q, -100.0)
    for cand in (q, down, up, np.nextafter(down, -100.0), np.nextafter(up, 200.0)):
        if 0.0 <= cand <= 100.0 and float(cand) / 100.0 * (n - 1) == r:
            return float(cand)
    return q


def signed_volume(shape, dtype, seed, background=0.3, negative=0.1):
    """A gamma-distributed foreground (a long bright tail), a zero background and a negative tail (uint8: none)."""
    rng = np.random.default_rng(seed)
    v = rng.gamma(2.0, 300.0, size=shape)
    u = rng.random(shape)
    v[u < background] = 0.0
    tail = u > 1.0 - negative
    v[tail] = -rng.gamma(2.0, 40.0, size=int(tail.sum()))
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return np.clip(np.rint(v / 8.0), 0, 255).astype(np.uint8)
    if dtype == np.int16:
        return np.clip(np.rint(v), -32768, 32767).astype(np.int16)
    return v.astype(dtype)


def signed_digit_values(dtype, count=67, seed=0):
    """``count`` distinct finite floats of both signs whose order-preserving keys between them differ in every 8-bit digit: one base pattern with
    each byte changed in its lowest bit and in all its bits, both signs of each, then random finite patterns."""
    dtype = np.dtype(dtype)
    nbytes, uint = dtype.itemsize, {4: np.uint32, 8: np.uint64}[dtype.itemsize]
    rng = np.random.default_rng(seed)
    top = (1 << (8 * nbytes - 1)) - 1
    finite = (0x7f800000 if nbytes == 4 else 0x7ff << 52) - 1
    base = int(rng.integers(top // 4, top // 2)) | 1
    patterns = {base}
    for byte in range(nbytes):
        patterns.add(base ^ (1 << (8 * byte)))
        patterns.add((base ^ (0xff << (8 * byte))) & top)
    patterns = {p for p in patterns if 0 < p <= finite}
    both = set()
    for p in sorted(patterns):
        both.add(p)
        both.add(p | (top + 1))                            # the negative of the same magnitude
    while len(both) < count:
        p = int(rng.integers(1, finite))
        both.add(p | ((top + 1) if rng.random() < 0.5 else 0))
    values = np.array(sorted(both)[:count], dtype=uint).view(dtype)
    assert np.isfinite(values).all() and np.unique(values).shape[0] == count and (values < 0).any() and (values > 0).any()
    return values
