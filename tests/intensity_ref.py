"""The statement of the intensity rescaling (include/afcm_hip.h) restated the slow way -- sort the foreground, index it -- plus the cases
the CPU and GPU tests share.  Nothing here imports afcm_amd: the restatement is held to numpy's own percentile and to the golden captured from the
reference function (tests/test_intensity_ref_cpu.py), and the package's host and device arms are then held to it, bit for bit."""
import numpy as np

DTYPES = (np.uint8, np.int16, np.float32, np.float64)


def percentile(sorted_values, q):
    """numpy's `linear` percentile of an ascending float64 array, q a percentile in [0, 100]; every operation a float64 one of its own."""
    s = np.asarray(sorted_values, dtype=np.float64)
    n = s.shape[0]
    vi = np.float64(q / 100.0) * np.float64(n - 1)
    i = int(np.floor(vi))
    g = vi - np.floor(vi)
    a, b = s[i], s[min(i + 1, n - 1)]
    with np.errstate(all='ignore'):
        d = b - a
        return b - d * (np.float64(1.0) - g) if g >= 0.5 else a + d * g


def rescale(volume, percentiles=(0.5, 99.5)):
    """(uint8 volume, float64 [lo, hi, n]) of the statement."""
    volume = np.asarray(volume)
    foreground = volume > 0                                # False for NaN, -inf, -0.0, 0 and negatives
    s = np.sort(volume[foreground].astype(np.float64))     # the widening is exact and keeps the order
    n = s.shape[0]
    out = np.zeros(volume.shape, dtype=np.uint8)
    if n == 0:
        return out, np.array([np.nan, np.nan, 0.0])
    lo, hi = percentile(s, percentiles[0]), percentile(s, percentiles[1])
    with np.errstate(all='ignore'):
        level = np.rint((volume[foreground].astype(np.float64) - lo) / (hi - lo) * np.float64(255.0))
    level[np.isnan(level)] = 1.0
    out[foreground] = np.clip(level, 1.0, 255.0).astype(np.uint8)
    return out, np.array([lo, hi, float(n)])


def same_bits(a, b):
    """Two float64 arrays with equal bit patterns, except that any NaN equals any NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


def skewed_volume(shape, dtype, seed, background=0.4, negatives=5):
    """A gamma-distributed foreground (a long bright tail, as MR intensities have), a zero background and a few negative voxels."""
    rng = np.random.default_rng(seed)
    v = rng.gamma(2.0, 300.0, size=shape)
    v[rng.random(shape) < background] = 0.0
    flat = v.reshape(-1)
    flat[rng.choice(flat.shape[0], size=min(negatives, flat.shape[0]), replace=False)] = -3.0
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return np.clip(np.rint(v / 8.0), -0.0, 255).astype(np.uint8)       # the negatives clip to background
    if dtype == np.int16:
        return np.clip(np.rint(v), -32768, 32767).astype(np.int16)
    return v.astype(dtype)


def digit_keys(bits, limit=None, count=67, seed=0):
    """``count`` distinct positive integer keys below ``limit`` (default 2^sum(bits)) that between them differ in every digit of the pass structure
    ``bits`` (widths, most significant first): one base key with each digit changed in turn, in its lowest bit and in all its bits, then random keys."""
    total = int(sum(bits))
    limit = 2 ** total if limit is None else int(limit)
    rng = np.random.default_rng(seed)
    high = min(limit, 2 ** 62)
    base = int(rng.integers(high // 4, high // 2)) | 1
    keys = {base}
    for p, width in enumerate(bits):                                        # every digit decides some comparison
        shift = total - int(sum(bits[:p + 1]))
        keys.add(base ^ (1 << shift))
        keys.add(base ^ (((1 << width) - 1) << shift))
    keys = {k for k in keys if 0 < k < limit}
    while len(keys) < count:
        keys.add(int(rng.integers(1, high)))
    return sorted(keys)[:count] if len(keys) > count else sorted(keys)


def keys_to_values(keys, dtype):
    """The positive values whose bit patterns are ``keys`` (floats: non-finite patterns are dropped by the caller's choice of keys)."""
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return np.array(keys, dtype=np.uint32).view(np.float32)
    if dtype == np.float64:
        return np.array(keys, dtype=np.uint64).view(np.float64)
    return np.array(keys).astype(dtype)


def rank_sweep(n):
    """Percentiles at which vi = q / 100 * (n - 1) lands on every i with g = 0, just below 0.5, at 0.5 and above, plus q = 0 and q = 100.  Each q is
    nudged by a few ulps where that makes the product hit its target exactly (so exact integers and exact halves do occur)."""
    qs = [0.0, 100.0]
    for i in range(n - 1):
        for g in (0.0, 0.5 - 2.0 ** -20, 0.5, 0.75):
            target = i + g
            q = 100.0 * target / (n - 1)
            for cand in (q, np.nextafter(q, 0.0), np.nextafter(q, 200.0), np.nextafter(np.nextafter(q, 0.0), 0.0), np.nextafter(np.nextafter(q, 200.0), 200.0)):
                if 0.0 <= cand <= 100.0 and float(cand) / 100.0 * (n - 1) == target:
                    q = float(cand)
                    break
            qs.append(q)
    return qs


def virtual_index(q, n):
    vi = np.float64(q / 100.0) * np.float64(n - 1)
    return int(np.floor(vi)), float(vi - np.floor(vi))
