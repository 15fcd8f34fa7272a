"""Float64 numpy statement of the [planes, 8] statistics table of afcm_plane_metrics (include/afcm_hip.h), for the tests.

Written from the column definitions, not from the kernel or from afcm_amd.evaluation: the window sums come from
``numpy.lib.stride_tricks.sliding_window_view`` (every valid 7 x 7 window summed on its own), not from a running or separable filter."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

WIN = 7
C1, C2 = (0.01 * 2.0) ** 2, (0.03 * 2.0) ** 2          # scikit-image's K1, K2 at data range 2


def unit_map(x):
    """train.py:93-96 in float32: add, halve, clip -- each its own rounding."""
    x = np.asarray(x, dtype=np.float32)
    return np.clip((x + np.float32(1.0)) * np.float32(0.5), np.float32(0.0), np.float32(1.0))


def ssim_map_sum(r, t):
    """Sum of the SSIM map of one plane pair (float64 [h, w]) over its (h - 6)(w - 6) valid windows."""
    win = lambda v: sliding_window_view(v, (WIN, WIN)).reshape(v.shape[0] - WIN + 1, v.shape[1] - WIN + 1, WIN * WIN)
    n = WIN * WIN
    ux, uy = win(r).sum(-1) / n, win(t).sum(-1) / n
    uxx, uyy, uxy = win(r * r).sum(-1) / n, win(t * t).sum(-1) / n, win(r * t).sum(-1) / n
    cov = n / (n - 1.0)
    vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
    s = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return float(s.sum())


def table(ref, test, map_to_unit=False):
    """[planes, h, w] arrays (any float dtype; values are taken as they are) -> float64 [planes, 8]."""
    if map_to_unit:
        ref, test = unit_map(ref), unit_map(test)
    ref, test = np.asarray(ref, dtype=np.float64), np.asarray(test, dtype=np.float64)
    assert ref.shape == test.shape and ref.ndim == 3
    out = np.empty((ref.shape[0], 8), dtype=np.float64)
    for p, (r, t) in enumerate(zip(ref, test)):
        with np.errstate(divide='ignore', invalid='ignore'):
            dn = r / r.max() - t / t.max()
        out[p] = (r.max(), r.min(), t.max(), t.min(), ((r - t) ** 2).sum(), (dn ** 2).sum(), np.abs(r - t).sum(), ssim_map_sum(r, t))
    return out


def noisy_pair(shape, seed, sigma=0.05, smooth=True):
    """A seeded target in [0, 1] and the target + N(0, sigma) clipped to [0, 1], both float32."""
    rng = np.random.default_rng(seed)
    ref = rng.random(shape)
    if smooth:                                             # a few flat regions: where the SSIM variance cancels against C2
        ref[..., : shape[-1] // 3] = np.round(ref[..., : shape[-1] // 3] * 2) / 2
    ref = ref.astype(np.float32)
    test = np.clip(ref + sigma * rng.standard_normal(shape), 0.0, 1.0).astype(np.float32)
    return ref, test
