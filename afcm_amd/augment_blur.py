"""Gaussian blur as parameter rows with host-made weights: the reference's ``GaussianBlur3D`` (data/augment/transforms.py:716-726, offered for the
train phase by configs/defaults.py:80-82 with ``execution_probability`` 0.5) for the device loader.

The reference calls ``skimage.filters.gaussian(x, sigma)`` on every ``[1, h, w]`` plane the loader hands it, which by skimage's documentation is
``scipy.ndimage.gaussian_filter(x, sigma, mode='nearest', truncate=4.0)`` on a float array (skimage itself is not pinned here: parity is with that
documented scipy call).  It draws from Python's global ``random``, once per plane: ``u = random.random()``; when ``u < execution_probability``,
``sigma = random.uniform(lo, hi)`` and the plane is blurred, otherwise it is returned as it is.  The planes of an item draw in the order the
dataset transforms them: the ``slice_num`` planes of ``A`` (those outside the volume included: a plane of zeros costs its draws too), then ``B``.

``afcm_batch_assemble_blur`` (torch_utils/ops/batch_ops.py) and ``apply_host`` -- numpy, the comparison arm -- produce the same bits.  One float64
row per item is drawn on the host (``blur_rows``), ``PLANE_COLS`` = 20 doubles per plane, the planes in draw order:

    0      flag                               the plane executes the transform
    1      sigma                              finite, > 0 (recorded; the kernel evaluates no exponential)
    2      radius                             a whole number in [0, 16]: int(4 sigma + 0.5)
    3-19   w_0 ... w_16                       finite; zeros beyond the radius

Weights (``gaussian_weights``, scipy's ``_gaussian_kernel1d``): ``x = arange(-radius, radius + 1)``, ``phi = exp(-0.5 / (sigma sigma) x^2)``,
``phi / phi.sum()``, ``w_j = phi[radius + j]``: exactly symmetric.

Filter (``blur_host``, scipy's symmetric ``correlate1d``): float64, every product and every addition rounded on its own, three passes in axis
order -- depth, rows, columns.  Per output element ``i`` of a line of length ``n``:

    t = v[i] * w_0
    for j = radius, radius - 1, ..., 1:   t = t + (v[clamp(i - j, 0, n - 1)] + v[clamp(i + j, 0, n - 1)]) * w_j

The depth pass runs on a line of one element: ``t = v * w_0; t = t + (v + v) * w_j``, which is not the identity in floating point.

The stage sits after the geometric transforms and the elastic deformation and before the intensity ones (the reference lists the noise after the
blur, and a contrast clip does not commute with a filter).  The arithmetic is float64 on the float32 item; the result is rounded once to float32.
The reference filters the float64 normalised value BEFORE its float32 cast, so a blurred pixel may differ from the reference's arithmetic by one
float32 unit in the last place.
"""
import dataclasses
import math
import random

import numpy as np
import torch

R_MAX = 16
PLANE_COLS = 3 + R_MAX + 1
TRUNCATE = 4.0
# a plane that is left alone: flag 0 and a record that passes the kernel's check (sigma 1 as a placeholder, the single tap 1.0)
IDENTITY_PLANE = np.array([0.0, 1.0, 0.0, 1.0] + [0.0] * R_MAX, dtype=np.float64)


def radius_of(sigma):
    return int(TRUNCATE * float(sigma) + 0.5)


@dataclasses.dataclass(frozen=True)
class BlurConfig:
    """``GaussianBlur3D(sigma=[lo, hi], execution_probability)``.  ``sigma[1]`` must keep the radius ``int(4 sigma + 0.5)`` within ``R_MAX`` = 16
    (sigma below 4.125)."""
    sigma: tuple = (0.1, 2.0)
    execution_probability: float = 0.5

    def __post_init__(self):
        def number(v):
            return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(float(v))
        s = self.sigma
        if not isinstance(s, (tuple, list)) or len(s) != 2 or not all(number(v) for v in s):
            raise RuntimeError(f'BlurConfig: sigma must be (lo, hi), two finite numbers, got {s!r}')
        lo, hi = float(s[0]), float(s[1])
        if not lo > 0.0:
            raise RuntimeError(f'BlurConfig: sigma[0] must be positive, got {lo!r}')
        if lo > hi:
            raise RuntimeError(f'BlurConfig: sigma (lo, hi) must be ordered, got {(lo, hi)!r}')
        if radius_of(hi) > R_MAX:
            raise RuntimeError(f'BlurConfig: sigma[1] {hi!r} has a radius of {radius_of(hi)} taps, above {R_MAX} (sigma below 4.125)')
        p = self.execution_probability
        if not number(p) or not 0.0 <= float(p) <= 1.0:
            raise RuntimeError(f'BlurConfig: execution_probability must be a number in [0, 1], got {p!r}')
        object.__setattr__(self, 'sigma', (lo, hi))
        object.__setattr__(self, 'execution_probability', float(p))


def gaussian_weights(sigma):
    """``(radius, w)``: ``radius = int(4 sigma + 0.5)`` and the float64 weights ``w[0 ... radius]`` of the centre and of every pair, as
    scipy's ``_gaussian_kernel1d`` makes them."""
    sigma = float(sigma)
    if not (sigma > 0.0 and math.isfinite(sigma)):
        raise RuntimeError(f'gaussian_weights: sigma must be positive and finite, got {sigma!r}')
    radius = radius_of(sigma)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return radius, np.ascontiguousarray(phi[radius:])


def plane_record(sigma):
    """The 20 doubles of an executed plane."""
    radius, w = gaussian_weights(sigma)
    if radius > R_MAX:
        raise RuntimeError(f'plane_record: sigma {sigma!r} has a radius of {radius} taps, above {R_MAX}')
    rec = np.zeros(PLANE_COLS, dtype=np.float64)
    rec[0], rec[1], rec[2] = 1.0, float(sigma), float(radius)
    rec[3:3 + radius + 1] = w
    return rec


def identity_rows(n, slice_num):
    """``n`` rows that change nothing: every plane flag 0."""
    return np.tile(IDENTITY_PLANE, (int(n), int(slice_num) + 1))


def blur_rows(config, n, slice_num, rng):
    """float64 [n, 20 (slice_num + 1)]: the draws of ``config`` for ``n`` items from a ``random.Random`` (the reference's generator type; an int
    seeds one), item by item, per item the ``slice_num`` planes of ``A`` and then ``B``, per plane ``rng.random()`` and, when that is strictly
    below ``execution_probability``, ``rng.uniform(lo, hi)``."""
    if not isinstance(config, BlurConfig):
        raise RuntimeError(f'blur_rows: config must be a BlurConfig, got {type(config).__name__}')
    if isinstance(rng, (int, np.integer)) and not isinstance(rng, bool):
        rng = random.Random(int(rng))
    if not isinstance(rng, random.Random):
        raise RuntimeError(f'blur_rows: rng must be a random.Random or an int seed, got {type(rng).__name__}')
    n, planes = int(n), int(slice_num) + 1
    if n < 1 or planes < 2:
        raise RuntimeError(f'blur_rows: {n} rows of {planes} planes')
    rows = identity_rows(n, slice_num).reshape(n, planes, PLANE_COLS)
    for i in range(n):
        for p in range(planes):
            if rng.random() < config.execution_probability:
                rows[i, p] = plane_record(rng.uniform(*config.sigma))
    return rows.reshape(n, planes * PLANE_COLS)


def checked_rows(rows, n, slice_num, what):
    rows = np.ascontiguousarray(np.asarray(rows))
    cols = PLANE_COLS * (int(slice_num) + 1)
    if rows.ndim != 2 or rows.shape[1] != cols or rows.dtype != np.float64 or rows.shape[0] != int(n):
        raise RuntimeError(f'{what}: a blur table is float64 [{int(n)}, {cols}], one row per item, got {rows.dtype} {rows.shape}')
    return rows


def plane_is_valid(rec):
    """The kernel's own check of one plane record (a NaN fails every comparison)."""
    rec = np.asarray(rec, dtype=np.float64)
    if rec.shape != (PLANE_COLS,):
        return False
    flag, sigma, radius = rec[:3]
    return bool(flag in (0.0, 1.0) and 0.0 < sigma < math.inf and 0.0 <= radius <= R_MAX and np.floor(radius) == radius and
                np.all(np.abs(rec[3:]) < math.inf))


def row_is_valid(row):
    """The kernel's own check of one item's row: every plane record of it."""
    row = np.asarray(row, dtype=np.float64)
    if row.ndim != 1 or row.shape[0] < PLANE_COLS or row.shape[0] % PLANE_COLS:
        return False
    return all(plane_is_valid(rec) for rec in row.reshape(-1, PLANE_COLS))


def _pass(v, axis, radius, w):
    n = v.shape[axis]
    at = np.arange(n)
    t = v * w[0]
    for j in range(radius, 0, -1):                                             # outermost pair first
        t = t + (np.take(v, np.clip(at - j, 0, n - 1), axis) + np.take(v, np.clip(at + j, 0, n - 1), axis)) * w[j]
    return t


def blur_host(planes_f64, radius, w):
    """float64, the shape it was given: ``planes_f64`` [..., h, w] filtered as the module's statement says -- the depth pass on every element as
    a line of one, then along the rows' axis (-2), then along the columns' (-1)."""
    v = np.asarray(planes_f64, dtype=np.float64)
    radius, w = int(radius), np.asarray(w, dtype=np.float64)
    if v.ndim < 2 or not 0 <= radius <= R_MAX or w.ndim != 1 or w.shape[0] < radius + 1:
        raise RuntimeError(f'blur_host: planes [..., h, w], a radius in [0, {R_MAX}] and its weights, got {v.shape}, {radius}, {w.shape}')
    t = v * w[0]
    for j in range(radius, 0, -1):
        t = t + (v + v) * w[j]
    return _pass(_pass(t, -2, radius, w), -1, radius, w)


def apply_host(planes, row):
    """The host arm of the whole stage: ``row`` applied to a float32 [k, H, W] tensor or ndarray, plane ``p`` with record ``p`` of the row.  A row
    the kernel would refuse raises.  A plane with flag 0 keeps its bits.  Returns the type it was given."""
    row = np.asarray(row, dtype=np.float64)
    m = planes.numpy() if isinstance(planes, torch.Tensor) else np.asarray(planes)
    if m.ndim != 3 or m.dtype != np.float32:
        raise RuntimeError(f'apply_host: planes must be float32 [k, H, W], got {m.dtype} {tuple(m.shape)}')
    if row.shape != (PLANE_COLS * m.shape[0],) or not row_is_valid(row):
        raise RuntimeError(f'apply_host: not a valid blur row for {m.shape[0]} planes: {row.tolist()}')
    out = m.copy()
    for p, rec in enumerate(row.reshape(-1, PLANE_COLS)):
        if rec[0] == 1.0:
            with np.errstate(over='ignore', invalid='ignore'):
                out[p] = blur_host(m[p].astype(np.float64), int(rec[2]), rec[3:]).astype(np.float32)
    return torch.from_numpy(out) if isinstance(planes, torch.Tensor) else out
