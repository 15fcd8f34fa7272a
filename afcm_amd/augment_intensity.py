"""Intensity training augmentation as parameter rows and a counter-based noise field: the reference's ``RandomContrast``,
``AdditiveGaussianNoise`` and ``AdditivePoissonNoise`` (data/augment/transforms.py:115-133, 619-644, offered for the train phase by
configs/defaults.py:83-88) for the device loader.

A noise field is as large as the batch, so it cannot be a host table: it is generated where it is used, from a counter-based generator
(Philox4x32-10) keyed per item, so that ``afcm_batch_assemble_noise`` (torch_utils/ops/batch_ops.py) and ``apply_host`` -- numpy, the comparison arm --
produce the same bits.  Only one float64 row per item is drawn on the host (``intensity_rows``):

    0-2   contrast flag, alpha, mean          t = mean + alpha * (t - mean), clipped to [-1, 1] (a NaN stays)
    3-4   Gaussian flag, std                  t = t + std * z
    5-6   Poisson flag, lam                   t = t + count             (lam is carried for the record; the kernel reads the table)
    7-8   key_lo, key_hi                      integers in [0, 2^32)
    9     J                                   the number of cut points, 0 ... 24
    10-33 T_0 ... T_23                        integer cut points in [0, 2^32] (``poisson_table``)
    34-35 zero

in that order on the float32 item plane widened to float64, every operation rounded on its own, one rounding to float32 at the end.  Pixel (y, x) of
plane pl takes lane ``x & 3`` of Philox(counter = (x >> 2, y, stream | P << 1, 0), key = (key_lo, key_hi)), stream 0 for the normals and 1 for the
counts, P = pl with ``independent_planes`` and 0 without (the reference hands every plane of an item a transformer of one seed: the same field).
The normals are Box-Muller on word pairs with this module's own ``log`` and ``sin`` / ``cos`` series -- IEEE + - x / sqrt floor only, no library
transcendental -- so that numpy and the kernel agree bit for bit; the counts are inversion by sequential search against integer cut points.
The reference adds its noise in float64 BEFORE its float32 cast; here the float32 item is widened back, so an item that executed a transform may
differ from the reference's arithmetic by one float32 unit in the last place.
"""
import dataclasses
import math

import numpy as np
import torch

ROW = 36
TABLE = 24                                                # cut points a row can hold
MAX_LAM = 4.0                                             # poisson_table(4.0) needs 23 cut points
_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_TWO32 = 4294967296.0
_MASK = np.uint64(0xFFFFFFFF)
SQRT_HALF, LN2, HALF_PI = 0.7071067811865476, 0.6931471805599453, 1.5707963267948966
_INV_FACT = [1.0 / math.factorial(n) for n in range(22)]  # n! is exact in a double up to 21!


def _pair(value, what, lo=None, hi=None):
    try:
        a, b = (float(v) for v in value)
    except (TypeError, ValueError):
        raise RuntimeError(f'IntensityConfig: {what} must be two numbers (lo, hi), got {value!r}') from None
    if not (math.isfinite(a) and math.isfinite(b) and a <= b) or (lo is not None and a < lo) or (hi is not None and b > hi):
        bounds = '' if lo is None else f' inside [{lo:g}, {"inf" if hi is None else format(hi, "g")}]'
        raise RuntimeError(f'IntensityConfig: {what} must be a finite range lo <= hi{bounds}, got ({a!r}, {b!r})')
    return a, b


def _prob(p, what):
    if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)) or not 0.0 <= float(p) <= 1.0:
        raise RuntimeError(f'IntensityConfig: {what} probability must be a number in [0, 1], got {p!r}')
    return float(p)


@dataclasses.dataclass(frozen=True)
class IntensityConfig:
    """``contrast``: ``(alpha_lo, alpha_hi, mean, prob)`` -- ``RandomContrast(alpha=(lo, hi), mean=mean, execution_probability=prob)``;
    ``gaussian``: ``(std_lo, std_hi, prob)`` -- ``AdditiveGaussianNoise(scale=(lo, hi), execution_probability=prob)``, 0 <= lo;
    ``poisson``: ``(lam_lo, lam_hi, prob)`` -- ``AdditivePoissonNoise(lam=(lo, hi), execution_probability=prob)``, 0 <= lo <= hi <= 4 (a row holds 24
    cut points, enough for lam 4).  None leaves a transform off.  ``independent_planes``: every plane of an item its own field instead of the one
    field the reference's equal seeds give them."""
    contrast: object = None
    gaussian: object = None
    poisson: object = None
    independent_planes: bool = False

    def __post_init__(self):
        for name, size in (('contrast', 4), ('gaussian', 3), ('poisson', 3)):
            v = getattr(self, name)
            if v is not None and (isinstance(v, (str, bytes)) or not hasattr(v, '__len__') or len(v) != size):
                raise RuntimeError(f'IntensityConfig: {name} must be None or {size} values, got {v!r}')
        if self.contrast is not None:
            lo, hi = _pair(self.contrast[:2], 'contrast alpha')
            mean = float(self.contrast[2])
            if not math.isfinite(mean):
                raise RuntimeError(f'IntensityConfig: contrast mean must be finite, got {mean!r}')
            object.__setattr__(self, 'contrast', (lo, hi, mean, _prob(self.contrast[3], 'contrast')))
        if self.gaussian is not None:
            object.__setattr__(self, 'gaussian', _pair(self.gaussian[:2], 'gaussian std', 0.0) + (_prob(self.gaussian[2], 'gaussian'),))
        if self.poisson is not None:
            object.__setattr__(self, 'poisson', _pair(self.poisson[:2], 'poisson lam', 0.0, MAX_LAM) + (_prob(self.poisson[2], 'poisson'),))
        if not isinstance(self.independent_planes, (bool, np.bool_)):
            raise RuntimeError(f'IntensityConfig: independent_planes must be a bool, got {self.independent_planes!r}')
        object.__setattr__(self, 'independent_planes', bool(self.independent_planes))


def poisson_table(lam):
    """The integer cut points of a Poisson(lam) draw from one 32-bit word: ``T_j = min(floor(F(j) 2^32), 2^32)`` with ``F`` the running float64 sum
    of ``p_0 = exp(-lam)``, ``p_j = p_{j-1} lam / j``, up to and including the first ``T_j >= 2^32 - 1``.  The count of a word is the number of
    ``T_j <= word``.  float64 [J], J <= 24."""
    lam = float(lam)
    if not 0.0 <= lam <= MAX_LAM:
        raise RuntimeError(f'poisson_table: lam must be in [0, {MAX_LAM:g}], got {lam!r}')
    p = math.exp(-lam)
    f, cuts = p, []
    for j in range(1, TABLE + 1):
        cuts.append(min(math.floor(f * _TWO32), _TWO32))
        if cuts[-1] >= _TWO32 - 1.0:
            return np.array(cuts, dtype=np.float64)
        p = p * lam / j
        f = f + p
    raise RuntimeError(f'poisson_table: lam {lam!r} needs more than {TABLE} cut points')


def identity_rows(n):
    """``n`` rows that change nothing: no flag set (alpha 1, every other column 0)."""
    rows = np.zeros((int(n), ROW), dtype=np.float64)
    rows[:, 1] = 1.0
    return rows


def make_rows(contrast=None, gaussian=None, poisson=None, keys=(0, 0), n=None):
    """Rows from given parameters, each an array of one length or a scalar broadcast against the others: ``contrast = (flag, alpha, mean)``,
    ``gaussian = (flag, std)``, ``poisson = (flag, lam)``, ``keys`` [n, 2] or one pair.  A transform whose flag is 0 leaves its columns as
    ``identity_rows`` has them."""
    parts = [np.asarray(v, dtype=np.float64) for group in (contrast, gaussian, poisson) if group is not None for v in group]
    keys = np.asarray(keys, dtype=np.float64)
    if keys.shape[-1:] != (2,) or keys.ndim > 2:
        raise RuntimeError(f'make_rows: keys must be one (key_lo, key_hi) pair or [n, 2], got shape {keys.shape}')
    n = max([int(n) if n is not None else 1] + [p.size for p in parts] + [keys.size // 2])
    rows = identity_rows(n)
    rows[:, 7:9] = keys
    if contrast is not None:
        flag, alpha, mean = (np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)) for v in contrast)
        on = flag != 0
        rows[:, 0], rows[on, 1], rows[on, 2] = flag, alpha[on], mean[on]
    if gaussian is not None:
        flag, std = (np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)) for v in gaussian)
        on = flag != 0
        rows[:, 3], rows[on, 4] = flag, std[on]
    if poisson is not None:
        flag, lam = (np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)) for v in poisson)
        rows[:, 5] = flag
        for r in np.nonzero(flag != 0)[0]:
            cuts = poisson_table(lam[r])
            rows[r, 6], rows[r, 9], rows[r, 10:10 + len(cuts)] = lam[r], len(cuts), cuts
    return rows


def intensity_rows(config, n, rng):
    """float64 [n, 36]: one draw of ``config``'s transforms per item.  The distributions are the reference's -- a transform executes when
    ``uniform() < prob``, its parameter is ``uniform(lo, hi)`` -- from a ``numpy.random.Generator`` in a fixed order: the contrast flags ([n]), the
    alphas, the Gaussian flags, the stds, the Poisson flags, the lams, then the keys as ``integers(0, 2**32, (n, 2))``.  A transform that is off
    draws nothing; the keys are always drawn.  The reference's own stream is not reproduced (it reseeds every transformer with one seed per
    subject, transforms.py:729-769)."""
    if not isinstance(config, IntensityConfig):
        raise RuntimeError(f'intensity_rows: config must be an IntensityConfig, got {type(config).__name__}')
    if not isinstance(rng, np.random.Generator):
        raise RuntimeError(f'intensity_rows: rng must be a numpy.random.Generator, got {type(rng).__name__}')
    n = int(n)
    if n < 1:
        raise RuntimeError(f'intensity_rows: {n} rows')

    def draw(spec):
        if spec is None:
            return None
        flags = rng.uniform(size=n) < spec[-1]
        return flags.astype(np.float64), rng.uniform(spec[0], spec[1], n)

    c, g, p = draw(config.contrast), draw(config.gaussian), draw(config.poisson)
    keys = rng.integers(0, 2 ** 32, (n, 2))
    return make_rows(None if c is None else (c[0], c[1], config.contrast[2]), g, p, keys, n=n)


def checked_rows(rows, n, what):
    rows = np.ascontiguousarray(np.asarray(rows))
    if rows.ndim != 2 or rows.shape[1] != ROW or rows.dtype != np.float64 or rows.shape[0] != int(n):
        raise RuntimeError(f'{what}: an intensity table is float64 [{int(n)}, {ROW}], one row per item, got {rows.dtype} {rows.shape}')
    return rows


def row_is_valid(row):
    """The kernel's own check of one row (a NaN fails every comparison)."""
    row = np.asarray(row, dtype=np.float64)

    def whole(v, hi):
        return bool(0.0 <= v <= hi and np.floor(v) == v)

    ok = row.shape == (ROW,) and all(row[c] in (0.0, 1.0) for c in (0, 3, 5)) and bool(np.isfinite(row[1]) and np.isfinite(row[2]))
    ok = ok and bool(np.isfinite(row[4]) and row[4] >= 0.0) and whole(row[7], _TWO32 - 1.0) and whole(row[8], _TWO32 - 1.0) and whole(row[9], float(TABLE))
    return ok and all(whole(row[10 + j], _TWO32) for j in range(int(row[9])))


# ---- the generator ----------------------------------------------------------------------------------------------------------------------------

def philox4x32(counter, key):
    """Philox4x32-10 (Salmon et al., 2011): ``counter`` [..., 4] and ``key`` [..., 2] of 32-bit words (broadcast against each other) -> uint32
    [..., 4].  Multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds."""
    counter, key = np.asarray(counter, dtype=np.uint64), np.asarray(key, dtype=np.uint64)
    shape = np.broadcast_shapes(counter.shape[:-1], key.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(counter[..., j], shape) for j in range(4))
    k0, k1 = (np.broadcast_to(key[..., j], shape) for j in range(2))
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2                       # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + np.uint64(_W0)) & _MASK, (k1 + np.uint64(_W1)) & _MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def field_words(key_lo, key_hi, h, w, stream, plane=0, word3=0):
    """uint32 [h, w]: the word of every pixel of one plane -- lane ``x & 3`` of Philox(counter (x >> 2, y, stream | plane << 1, word3)).
    ``word3`` is 0 for the intensity streams; the elastic deformation's fields take 1 and 2 (afcm_amd/augment_elastic.py)."""
    groups = (int(w) + 3) // 4
    counter = np.zeros((int(h), groups, 4), dtype=np.uint64)
    counter[..., 0] = np.arange(groups)[None, :]
    counter[..., 1] = np.arange(int(h))[:, None]
    counter[..., 2] = int(stream) | (int(plane) << 1)
    counter[..., 3] = int(word3)
    words = philox4x32(counter, np.array([int(key_lo), int(key_hi)], dtype=np.uint64))
    return words.reshape(int(h), groups * 4)[:, :int(w)]


def log_series(x):
    """ln(x) for positive normal doubles: ``m, e = frexp(x)`` moved to m in [sqrt(1/2), sqrt(2)), ``s = (m - 1) / (m + 1)``, the odd series
    2 s (1 + s^2 / 3 + ... + s^22 / 23) by Horner from 1/23 down, plus ``e ln 2``.  Every operation is one IEEE float64 operation."""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    low = m < SQRT_HALF
    m, e = np.where(low, m * 2.0, m), np.where(low, e - 1, e).astype(np.float64)
    s = (m - 1.0) / (m + 1.0)
    s2 = s * s
    acc = np.full_like(s, 1.0 / 23.0)
    for k in range(21, 0, -2):
        acc = acc * s2 + 1.0 / k
    return e * LN2 + 2.0 * (s * acc)


def sincos_turns(u):
    """``(sin, cos)`` of ``2 pi u`` for u in [0, 1): ``t = 4 u``, the quadrant ``q = floor(t)``, ``r = (t - q) pi / 2`` in [0, pi / 2), the Taylor
    series of sin (to r^21) and cos (to r^20) by Horner with the coefficients ``1 / n!`` (``a = 1 / n! - r^2 a``), and the quadrant's signs."""
    t = np.asarray(u, dtype=np.float64) * 4.0
    q = np.floor(t)
    r = (t - q) * HALF_PI
    r2 = r * r
    a = np.full_like(r, _INV_FACT[21])
    for n in range(19, 0, -2):
        a = _INV_FACT[n] - r2 * a
    s = r * a
    c = np.full_like(r, _INV_FACT[20])
    for n in range(18, -1, -2):
        c = _INV_FACT[n] - r2 * c
    q = q.astype(np.int64) & 3
    return np.choose(q, [s, c, -s, -c]), np.choose(q, [c, -s, -c, s])


def normals_from_words(words):
    """Box-Muller on word pairs: uint32 [..., 4 g] -> float64 [..., 4 g]; of every four words ``(w0, w1)`` give lanes 0 and 1, ``(w2, w3)`` lanes 2
    and 3: ``u1 = (w0 + 0.5) 2^-32``, ``u2 = w1 2^-32``, ``r = sqrt(-2 ln u1)``, ``r cos(2 pi u2)`` and ``r sin(2 pi u2)``."""
    words = np.asarray(words)
    pairs = words.reshape(words.shape[:-1] + (-1, 2)).astype(np.float64)
    u1, u2 = (pairs[..., 0] + 0.5) * (1.0 / _TWO32), pairs[..., 1] * (1.0 / _TWO32)
    r = np.sqrt(-2.0 * log_series(u1))
    s, c = sincos_turns(u2)
    return np.stack([r * c, r * s], axis=-1).reshape(words.shape)


def normal_field(key_lo, key_hi, h, w, plane=0, word3=0):
    """float64 [h, w]: the standard normals of one plane (stream 0)."""
    padded = field_words(key_lo, key_hi, h, 4 * ((int(w) + 3) // 4), 0, plane, word3)
    return normals_from_words(padded)[:, :int(w)]


def counts_from_words(words, cuts):
    """The number of cut points at or below each word, float64."""
    words = np.asarray(words).astype(np.float64)
    count = np.zeros(words.shape, dtype=np.float64)
    for t in np.asarray(cuts, dtype=np.float64):
        count = count + (words >= t)
    return count


def poisson_field(key_lo, key_hi, h, w, cuts, plane=0):
    """float64 [h, w]: the Poisson counts of one plane (stream 1) for the cut points ``cuts`` (``poisson_table``)."""
    return counts_from_words(field_words(key_lo, key_hi, h, w, 1, plane), cuts)


def transform(t, contrast=None, gaussian=None, poisson=None):
    """The arithmetic of the three transforms on a float64 array: ``contrast = (alpha, mean)``, ``gaussian = (std, z)`` and ``poisson = count``
    with the fields given, None for a transform that does not execute.  No rounding to float32 here."""
    t = np.asarray(t, dtype=np.float64)
    if contrast is not None:
        alpha, mean = (np.float64(v) for v in contrast)
        t = mean + alpha * (t - mean)
        t = np.where(t < -1.0, -1.0, np.where(t > 1.0, 1.0, t))                  # a NaN fails both comparisons and stays
    if gaussian is not None:
        t = t + np.float64(gaussian[0]) * np.asarray(gaussian[1], dtype=np.float64)
    if poisson is not None:
        t = t + np.asarray(poisson, dtype=np.float64)
    return t


def apply_host(planes, row, independent_planes=False, first_plane=0):
    """The host arm: ``row`` applied to a float32 [C, H, W] tensor or ndarray, plane ``c`` being plane ``first_plane + c`` of its item (an item's
    ``A`` starts at 0, its ``B`` is plane ``slice_num``; this matters with ``independent_planes`` only).  A row the kernel would refuse raises.
    A row with no flag set returns the planes as they are.  Returns the type it was given."""
    row = np.asarray(row, dtype=np.float64)
    if not row_is_valid(row):
        raise RuntimeError(f'apply_host: not a valid intensity row: {row.tolist()}')
    m = planes.numpy() if isinstance(planes, torch.Tensor) else np.asarray(planes)
    if m.ndim != 3 or m.dtype != np.float32:
        raise RuntimeError(f'apply_host: planes must be float32 [C, H, W], got {m.dtype} {tuple(m.shape)}')
    if row[0] == 0.0 and row[3] == 0.0 and row[5] == 0.0:
        return planes
    h, w = m.shape[1:]
    key_lo, key_hi, cuts = int(row[7]), int(row[8]), row[10:10 + int(row[9])]
    out, fields = np.empty_like(m), {}
    for c in range(m.shape[0]):
        plane = first_plane + c if independent_planes else 0
        if plane not in fields:
            fields[plane] = (normal_field(key_lo, key_hi, h, w, plane) if row[3] else None,
                             poisson_field(key_lo, key_hi, h, w, cuts, plane) if row[5] else None)
        z, counts = fields[plane]
        t = transform(m[c], contrast=(row[1], row[2]) if row[0] else None, gaussian=(row[4], z) if row[3] else None, poisson=counts)
        out[c] = t.astype(np.float32)
    return torch.from_numpy(out) if isinstance(planes, torch.Tensor) else out
