"""Float64 numpy statement of afcm_volume_ssim's layer sums (include/afcm_hip.h), for the tests.

Written from the definition, not from the kernel or from afcm_amd.evaluation: every window sum is a direct sum of seven terms per axis taken from
``numpy.lib.stride_tricks.sliding_window_view`` -- no ``uniform_filter``, no running sums.  The order in which the three axes are summed is a
parameter, so that two orders can be held against each other."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from plane_metrics_ref import C1, C2, WIN, unit_map  # noqa: F401  (unit_map: re-exported for the tests)

NPIX = float(WIN ** 3)
# a-priori rounding bound of ONE window of a constant pair, relative: 8 x 343 x 2^-53 / c2 (the variance terms cancel to rounding against c2)
CONSTANT_WINDOW_BOUND = 8 * NPIX * 2.0 ** -53 / C2


def window_sums(v, order=(0, 1, 2)):
    """Sums of ``v`` [d, h, w] over every valid 7 x 7 x 7 window -> [d - 6, h - 6, w - 6]; seven direct terms along each axis, axes in ``order``."""
    for axis in order:
        v = sliding_window_view(v, WIN, axis=axis).sum(-1)
    return v


def ssim_map(r, t, order=(0, 1, 2)):
    """The SSIM map of one volume pair (float64 [d, h, w]) over its valid windows: data range 2, sample covariance."""
    r, t = np.asarray(r, dtype=np.float64), np.asarray(t, dtype=np.float64)
    assert r.shape == t.shape and r.ndim == 3 and min(r.shape) >= WIN
    ux, uy = window_sums(r, order) / NPIX, window_sums(t, order) / NPIX
    uxx, uyy, uxy = window_sums(r * r, order) / NPIX, window_sums(t * t, order) / NPIX, window_sums(r * t, order) / NPIX
    cov = NPIX / (NPIX - 1.0)
    vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def layer_sums(r, t, order=(0, 1, 2)):
    """[d - 6]: the map summed over the (h - 6)(w - 6) windows of every z-layer of window origins."""
    return ssim_map(r, t, order).sum(axis=(1, 2))


def noise_pair(shape, seed):
    """A seeded target in [0, 1] with flat regions and the target + N(0, 0.05) clipped, float32."""
    rng = np.random.default_rng(seed)
    ref = rng.random(shape)
    ref[..., : shape[-1] // 3] = np.round(ref[..., : shape[-1] // 3] * 2) / 2
    ref = ref.astype(np.float32)
    return ref, np.clip(ref + 0.05 * rng.standard_normal(shape), 0.0, 1.0).astype(np.float32)


def blob_pair(shape, seed):
    """MR-like: a smooth bright blob on an EXACTLY zero background (where the variance cancels against c2), and a noisy, scaled copy; float32."""
    zz, yy, xx = np.meshgrid(*(np.linspace(-1, 1, n) for n in shape), indexing='ij')
    body = np.clip(0.9 - (zz ** 2 * 0.5 + yy ** 2 + xx ** 2), 0, 1) * (0.6 + 0.4 * np.sin(7 * xx) * np.cos(5 * yy + zz))
    noise = 0.03 * np.random.default_rng(seed).standard_normal(shape) * (body > 0)
    return body.astype(np.float32), np.clip(body * 1.1 + noise, 0, 1).astype(np.float32)
