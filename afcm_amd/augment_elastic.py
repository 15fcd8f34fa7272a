"""Elastic deformation as parameter rows, a folded smoothing operator and a counter-based random field: the reference's ``ElasticDeformation``
(data/augment/transforms.py:138-191, offered for the train phase by configs/defaults.py:77-79) for the device loader.

The reference draws standard normal fields as large as the patch, smooths them with ``gaussian_filter(sigma, mode='reflect')``, scales them by
``alpha`` and reads the plane at ``(y + dy, x + dx)`` with ``map_coordinates(order, mode='reflect')``.  The loader hands every ``[1, h, w]`` plane of
an item an equally seeded ``RandomState``, so all planes of an item, the target included, get one deformation, and with depth 1 the ``z``
displacement has no effect; the statement here is two-dimensional.  ``afcm_batch_assemble_elastic`` (torch_utils/ops/batch_ops.py) and
``apply_host`` -- numpy, the comparison arm -- produce the same bits.  One float64 row per item is drawn on the host (``elastic_rows``):

    0     flag                                the item executes the transform
    1     alpha                               finite, |alpha| <= 2^20
    2-3   key_lo, key_hi                      integers in [0, 2^32)

The fields ``Fy``, ``Fx`` are ``augment_intensity.normal_field`` arithmetic on Philox counters ``(x >> 2, y, 0, 1)`` and ``(x >> 2, y, 0, 2)``
(word 3 is 0 in the intensity streams).  The Gaussian is folded over its reflections into one ``[n, n]`` operator per axis by the host
(``smoothing_operator``): the kernel evaluates no exponential.  The order of every operation is stated once in include/afcm_hip.h
(afcm_batch_assemble_elastic) and followed here operation by operation: IEEE + - x / sqrt floor only.

The stage sits after the geometric transforms and before the intensity ones (``RandomContrast`` included: its clip does not commute with the
overshoot of a cubic spline).  The arithmetic is float64 on the float32 item; the result is rounded once to float32.  The reference interpolates
in float64 BEFORE its float32 cast, so a deformed pixel may differ from the reference's arithmetic by one float32 unit in the last place.
"""
import dataclasses
import math

import numpy as np
import torch

from .augment_intensity import normal_field

ROW = 4
MAX_ALPHA = 1048576.0                                     # 2^20
COORD_MAX = 1073741824.0                                  # 2^30: a coordinate beyond it reads nothing and gives NaN
SPLINE_Z = -0.2679491924311227                            # sqrt(3) - 2, the pole of the cubic B-spline
SPLINE_LAST = SPLINE_Z / (SPLINE_Z - 1.0)
SPLINE_HORIZON = 40                                       # |z|^40 = 1.3e-23
ORDERS = (0, 1, 3)
_TWO32 = 4294967296.0


@dataclasses.dataclass(frozen=True)
class ElasticConfig:
    """``ElasticDeformation(spline_order, alpha, sigma, execution_probability, apply_3d)``.  Orders 0, 1 and 3.  ``apply_3d`` is accepted for the
    signature: on the depth-1 items of the loader the ``z`` displacement it switches has no effect, and the fields here are keyed, not drawn from
    the reference's stream, so it changes nothing."""
    spline_order: int = 3
    alpha: float = 2000.0
    sigma: float = 50.0
    execution_probability: float = 0.1
    apply_3d: bool = True

    def __post_init__(self):
        if isinstance(self.spline_order, bool) or self.spline_order not in ORDERS:
            raise RuntimeError(f'ElasticConfig: spline_order must be 0, 1 or 3, got {self.spline_order!r}')
        for name, lo, hi in (('alpha', -MAX_ALPHA, MAX_ALPHA), ('sigma', 0.0, math.inf), ('execution_probability', 0.0, 1.0)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not (lo <= float(v) <= hi) or not math.isfinite(float(v)):
                raise RuntimeError(f'ElasticConfig: {name} must be a finite number in [{lo:g}, {hi:g}], got {v!r}')
            object.__setattr__(self, name, float(v))
        if not self.sigma > 0.0:
            raise RuntimeError(f'ElasticConfig: sigma must be positive, got {self.sigma!r}')
        if not isinstance(self.apply_3d, (bool, np.bool_)):
            raise RuntimeError(f'ElasticConfig: apply_3d must be a bool, got {self.apply_3d!r}')
        object.__setattr__(self, 'spline_order', int(self.spline_order))
        object.__setattr__(self, 'apply_3d', bool(self.apply_3d))


def identity_rows(n):
    """``n`` rows that change nothing: flag 0."""
    return np.zeros((int(n), ROW), dtype=np.float64)


def elastic_rows(config, n, rng):
    """float64 [n, 4]: one draw of ``config`` per item from a ``numpy.random.Generator``, in a fixed order: the decisions ``uniform(size=n)`` -- an
    item executes when its draw is strictly below ``execution_probability``, as the reference decides -- then the keys as
    ``integers(0, 2**32, (n, 2))``.  Every row carries ``config.alpha``."""
    if not isinstance(config, ElasticConfig):
        raise RuntimeError(f'elastic_rows: config must be an ElasticConfig, got {type(config).__name__}')
    if not isinstance(rng, np.random.Generator):
        raise RuntimeError(f'elastic_rows: rng must be a numpy.random.Generator, got {type(rng).__name__}')
    n = int(n)
    if n < 1:
        raise RuntimeError(f'elastic_rows: {n} rows')
    rows = identity_rows(n)
    rows[:, 0] = rng.uniform(size=n) < config.execution_probability
    rows[:, 1] = config.alpha
    rows[:, 2:4] = rng.integers(0, 2 ** 32, (n, 2))
    return rows


def checked_rows(rows, n, what):
    rows = np.ascontiguousarray(np.asarray(rows))
    if rows.ndim != 2 or rows.shape[1] != ROW or rows.dtype != np.float64 or rows.shape[0] != int(n):
        raise RuntimeError(f'{what}: an elastic table is float64 [{int(n)}, {ROW}], one row per item, got {rows.dtype} {rows.shape}')
    return rows


def row_is_valid(row):
    """The kernel's own check of one row (a NaN fails every comparison)."""
    row = np.asarray(row, dtype=np.float64)
    if row.shape != (ROW,):
        return False
    keys = all(bool(0.0 <= v <= _TWO32 - 1.0 and np.floor(v) == v) for v in row[2:4])
    return bool(row[0] in (0.0, 1.0) and abs(row[1]) <= MAX_ALPHA) and keys


def reflect(i, n):
    """scipy.ndimage's 'reflect' for integer coordinates, any number of periods: (d c b a | a b c d | d c b a)."""
    i = np.asarray(i, dtype=np.int64)
    m = np.where(i < 0, -i - 1, i) % (2 * int(n))
    return np.where(m < n, m, 2 * int(n) - 1 - m)


def smoothing_operator(sigma, n, truncate=4.0):
    """float64 [n, n]: ``gaussian_filter1d(sigma, mode='reflect', truncate=truncate)`` on a line of ``n`` as one matrix.  The radius is
    ``R = int(truncate sigma + 0.5)``, the weights ``w_j = exp(-0.5 (j - R)^2 / sigma^2)`` over their sum, and
    ``G[i][m] = sum of w_j over j = 0 ... 2R, ascending, with reflect(i + j - R, n) = m``: the filter's reflections, several periods of them
    when ``2R + 1 > n``, folded into the line."""
    sigma, n = float(sigma), int(n)
    if not (sigma > 0.0 and math.isfinite(sigma)) or n < 1:
        raise RuntimeError(f'smoothing_operator: sigma {sigma!r} on a line of {n}: sigma must be positive and finite, the line not empty')
    radius = int(float(truncate) * sigma + 0.5)
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    weights = phi / phi.sum()
    op, rows = np.zeros((n, n), dtype=np.float64), np.arange(n)
    for j in range(2 * radius + 1):
        op[rows, reflect(rows + (j - radius), n)] += weights[j]                # one column per row and j: no repeated index
    return op


def _ordered_product(a, b):
    """``out[r][c] = sum over m ascending of a[r][m] * b[m][c]``, the accumulator from +0.0, every product and addition rounded on its own.  A
    column of ``a`` that is all 0.0 is skipped: b is finite, so it would add +-0.0 to an accumulator that is never -0.0."""
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=np.float64)
    for m in range(a.shape[1]):
        column = a[:, m]
        if np.any(column != 0.0):                                             # a NaN is not 0.0
            acc = acc + column[:, None] * b[m][None, :]
    return acc


def smooth_host(field, op_h, op_w):
    """``op_h . field . op_w^T`` in the kernel's order: along y first (``T[i][x] = sum_m op_h[i][m] field[m][x]``), then along x
    (``S[y][j] = sum_m T[y][m] op_w[j][m]``)."""
    field, op_h, op_w = (np.asarray(v, dtype=np.float64) for v in (field, op_h, op_w))
    if op_h.shape != (field.shape[0],) * 2 or op_w.shape != (field.shape[1],) * 2:
        raise RuntimeError(f'smooth_host: operators {op_h.shape}, {op_w.shape} for a field {field.shape}')
    t = _ordered_product(op_h, field)
    return _ordered_product(op_w, t.T).T                                       # products commute bit for bit; the order of the sum is m ascending


def displacement_host(row, h, w, op_h, op_w, fields=None):
    """``(dy, dx)`` float64 [h, w] of one row: ``alpha * smooth_host(F)`` for ``Fy`` (counter word 3 = 1) and ``Fx`` (2).  ``fields=(Fy, Fx)``
    replaces the generated fields (the golden's recorded ones)."""
    row = np.asarray(row, dtype=np.float64)
    if not row_is_valid(row):
        raise RuntimeError(f'displacement_host: not a valid elastic row: {row.tolist()}')
    if fields is None:
        fields = tuple(normal_field(int(row[2]), int(row[3]), h, w, 0, word3) for word3 in (1, 2))
    fy, fx = (np.asarray(f, dtype=np.float64) for f in fields)
    if fy.shape != (h, w) or fx.shape != (h, w):
        raise RuntimeError(f'displacement_host: fields {fy.shape}, {fx.shape} for a plane [{h}, {w}]')
    return row[1] * smooth_host(fy, op_h, op_w), row[1] * smooth_host(fx, op_h, op_w)


def _coefficients_along_first_axis(p):
    n = p.shape[0]
    s = p[reflect(-SPLINE_HORIZON, n)]
    for k in range(SPLINE_HORIZON - 1, 0, -1):
        s = p[reflect(-k, n)] + SPLINE_Z * s
    plus = np.empty_like(p)
    plus[0] = p[0] + SPLINE_Z * s
    for k in range(1, n):
        plus[k] = p[k] + SPLINE_Z * plus[k - 1]
    c = SPLINE_LAST * plus[n - 1]
    out = np.empty_like(p)
    out[n - 1] = c * 6.0
    for k in range(n - 2, -1, -1):
        c = SPLINE_Z * (c - plus[k])
        out[k] = c * 6.0
    return out


def spline_coefficients_host(plane):
    """The cubic B-spline coefficients of a float64 [h, w] plane (or one line, 1-D) with the half-sample symmetric boundary -- the exact
    interpolating spline at every length -- along y (every column), then along x (every row).  For a line ``q[0 ... n)`` and the pole
    ``z = -0.2679491924311227`` (sqrt(3) - 2), every operation rounded on its own:

        s = q[reflect(-40)]; s = q[reflect(-k)] + z * s for k = 39 ... 1        (the causal start, 40 reflected terms out, by Horner)
        c+[0] = q[0] + z * s;  c+[k] = q[k] + z * c+[k - 1]
        c[n - 1] = (z / (z - 1)) * c+[n - 1];  c[k] = z * (c[k + 1] - c+[k]) for k = n - 2 ... 0
        the line becomes c[k] * 6
    """
    p = np.asarray(plane, dtype=np.float64)
    if p.ndim == 1:
        return _coefficients_along_first_axis(p)
    if p.ndim != 2:
        raise RuntimeError(f'spline_coefficients_host: a plane [h, w] or a line, got shape {p.shape}')
    return _coefficients_along_first_axis(_coefficients_along_first_axis(p).T).T


def cubic_weights(t):
    """The four cubic B-spline weights of ``t`` in [0, 1), in the kernel's operation order."""
    u = 1.0 - t
    return [((u * u) * u) / 6.0, (((t * t) * (t - 2.0)) * 3.0 + 4.0) / 6.0, (((u * u) * (u - 2.0)) * 3.0 + 4.0) / 6.0, ((t * t) * t) / 6.0]


def deform_host(planes, dy, dx, order):
    """float64 [C, h, w]: every plane read at ``(y + dy, x + dx)``: ``map_coordinates(order, mode='reflect')`` with exact integer index folding.
    Order 0: the pixel at ``floor(c + 0.5)``; order 1: weights ``(1 - t, t)`` at ``floor(c)`` and the next; order 3: ``cubic_weights`` at
    ``floor(c) - 1 ... + 2`` on ``spline_coefficients_host(plane)``.  The taps of a row are summed first (x ascending, from the first
    product), then the rows.  A coordinate that fails ``|c| <= 2^30`` gives NaN."""
    if order not in ORDERS:
        raise RuntimeError(f'deform_host: spline order {order!r} is not 0, 1 or 3')
    planes, dy, dx = (np.asarray(v, dtype=np.float64) for v in (planes, dy, dx))
    if planes.ndim != 3 or dy.shape != planes.shape[1:] or dx.shape != planes.shape[1:]:
        raise RuntimeError(f'deform_host: planes [C, h, w] with displacements [h, w], got {planes.shape}, {dy.shape}, {dx.shape}')
    h, w = planes.shape[1:]
    cy = np.arange(h, dtype=np.float64)[:, None] + dy
    cx = np.arange(w, dtype=np.float64)[None, :] + dx
    with np.errstate(invalid='ignore'):
        good = (np.abs(cy) <= COORD_MAX) & (np.abs(cx) <= COORD_MAX)
    cy, cx = np.where(good, cy, 0.0), np.where(good, cx, 0.0)
    out = np.empty_like(planes)
    if order == 0:
        iy, ix = reflect(np.floor(cy + 0.5).astype(np.int64), h), reflect(np.floor(cx + 0.5).astype(np.int64), w)
        for c, p in enumerate(planes):
            out[c] = p[iy, ix]
    else:
        fy, fx = np.floor(cy), np.floor(cx)
        ty, tx = cy - fy, cx - fx
        wy, wx = ([1.0 - ty, ty], [1.0 - tx, tx]) if order == 1 else (cubic_weights(ty), cubic_weights(tx))
        base = 0 if order == 1 else 1
        iy = [reflect(fy.astype(np.int64) - base + a, h) for a in range(len(wy))]
        ix = [reflect(fx.astype(np.int64) - base + l, w) for l in range(len(wx))]
        for c, p in enumerate(planes):
            src = p if order == 1 else spline_coefficients_host(p)
            acc = None
            for a in range(len(wy)):
                r = wx[0] * src[iy[a], ix[0]]
                for l in range(1, len(wx)):
                    r = r + wx[l] * src[iy[a], ix[l]]
                acc = wy[0] * r if a == 0 else acc + wy[a] * r
            out[c] = acc
    out[:, ~good] = np.nan
    return out


def apply_host(planes, row, config, ops=None, fields=None):
    """The host arm of the whole stage: ``row`` applied to a float32 [C, H, W] tensor or ndarray, all planes with one deformation.
    ``config``: the ``ElasticConfig`` (its order, and its sigma where ``ops`` is None); ``ops = (op_h, op_w)``: the smoothing operators, built
    here when None.  A row the kernel would refuse raises.  A row with flag 0 returns the planes as they are.  Returns the type it was given."""
    if not isinstance(config, ElasticConfig):
        raise RuntimeError(f'apply_host: config must be an ElasticConfig, got {type(config).__name__}')
    row = np.asarray(row, dtype=np.float64)
    if not row_is_valid(row):
        raise RuntimeError(f'apply_host: not a valid elastic row: {row.tolist()}')
    m = planes.numpy() if isinstance(planes, torch.Tensor) else np.asarray(planes)
    if m.ndim != 3 or m.dtype != np.float32:
        raise RuntimeError(f'apply_host: planes must be float32 [C, H, W], got {m.dtype} {tuple(m.shape)}')
    if row[0] == 0.0:
        return planes
    h, w = m.shape[1:]
    op_h, op_w = ops if ops is not None else (smoothing_operator(config.sigma, h), smoothing_operator(config.sigma, w))
    dy, dx = displacement_host(row, h, w, op_h, op_w, fields)
    with np.errstate(over='ignore'):
        out = deform_host(m, dy, dx, config.spline_order).astype(np.float32)
    return torch.from_numpy(out) if isinstance(planes, torch.Tensor) else out
