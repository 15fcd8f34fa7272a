"""The reference's two per-plane normalisers, ``PercentileNormalizer`` and ``Standardize`` (data/augment/transforms.py:552-601, ``channelwise``
False; the first two entries of configs/defaults.py for the train and the test phase): the statement both loaders keep, in numpy.

The plane ``m`` is the [1, H, W] item plane after the centred crop / zero pad, in the source dtype: padded zeros count in the statistics, and a
thick-slice position outside the volume is a plane of zeros.  The normalisers come before every geometric transform.

    percentile   lo, hi = np.percentile(m, pmin), np.percentile(m, pmax);  (m - lo) / (hi - lo + eps)
    standardize  (m - mean) / np.clip(std, eps, None)  with np.mean(m), np.std(m) of the plane, or two given floats

The statement kept (include/afcm_hip.h has it in full): ALL arithmetic is float64 for every source dtype, every operation rounded on its own, one
rounding to float32 at the end.  The percentiles are numpy's ``linear`` method by sort-and-index with numpy's lerp (``intensity._percentile_pair``,
pinned against ``np.percentile``), on the plane with -0.0 taken as +0.0; one NaN makes both NaN.  Mean and sum of squared deviations are taken in
ONE order, the kernel's: partial ``t`` of 256 adds pixels t, t + 256, t + 512, ... of the row-major plane in ascending order onto +0.0, then the
tree ``s[t] += s[t + o]`` for o = 128, 64, ..., 1; ``std = sqrt(ss / n)``.  The reference agrees bit for bit in percentile mode for uint8, int16
and float64 sources; numpy evaluates a float32 plane in float32 (DESIGN 8u has the measured deviation), and its own summation order differs from
the one above in the last bits of the standard deviation.

``normalise_host`` is that statement, the host arm; ``torch_utils.ops.normalise_ops`` and the ``normalise=`` keyword of ``assemble_batch`` /
``assemble_slices`` the device arm, the same bits.
"""
import numpy as np

from . import _lib
from .intensity import _percentile_pair
from .torch_utils.ops.intensity_ops import percentile_fractions

_SOURCES = tuple(np.dtype(t) for t in (np.uint8, np.int16, np.float32, np.float64))
PARTIALS = 256                                             # the workgroup's threads: the strided partials of the stated order


class NormaliseConfig:
    """Which per-plane normaliser the loaders apply.  ``percentile=(pmin, pmax)``: ``PercentileNormalizer`` with those percentages (0 <= pmin <=
    pmax <= 100; the test default (0, 100) is per-plane min-max scaling).  ``standardize=True``: ``Standardize`` with the plane's own mean and
    standard deviation; ``standardize=(mean, std)``: with those two floats.  Exactly one of the two: their composition is not an affine map of the
    raw plane's statistics and is not built.  ``eps``: the reference's 1e-10.  ``then_normalize``: the loader's ``Normalize(min_value, max_value)``
    is applied to the result, as the reference's list order does; False: the result is the normaliser's own value."""

    def __init__(self, percentile=None, standardize=None, eps=1e-10, then_normalize=False):
        if standardize is False:
            standardize = None
        if (percentile is None) == (standardize is None):
            raise RuntimeError('NormaliseConfig: give exactly one of percentile=(pmin, pmax) and standardize=True | (mean, std); the composition of '
                               'both is not an affine map of the raw plane\'s statistics and is not supported')
        if not isinstance(then_normalize, bool):
            raise RuntimeError(f'NormaliseConfig: then_normalize must be a bool, got {then_normalize!r}')
        self.eps = float(eps)
        if self.eps != self.eps:
            raise RuntimeError('NormaliseConfig: eps is a NaN')
        self.then_normalize = then_normalize
        self.percentile = self.standardize = None
        if percentile is not None:
            self.p0, self.p1 = percentile_fractions(percentile, 'NormaliseConfig: percentile')
            self.percentile = tuple(float(q) for q in percentile)
            self.mode = _lib.NORM_PERCENTILE
        elif standardize is True:
            self.standardize, self.mode, self.p0, self.p1 = True, _lib.NORM_STANDARDIZE, 0.0, 0.0
        else:
            try:
                mean, std = (float(v) for v in standardize)
            except (TypeError, ValueError):
                raise RuntimeError(f'NormaliseConfig: standardize must be True or a pair (mean, std), got {standardize!r}') from None
            self.standardize, self.mode, self.p0, self.p1 = (mean, std), _lib.NORM_FIXED, mean, std

    def __repr__(self):
        return f'NormaliseConfig(percentile={self.percentile}, standardize={self.standardize}, eps={self.eps}, then_normalize={self.then_normalize})'


def checked_config(config, what):
    """``config`` if it is a NormaliseConfig or None; RuntimeError otherwise."""
    if config is not None and not isinstance(config, NormaliseConfig):
        raise RuntimeError(f'{what}: normalise must be a NormaliseConfig or None, got {type(config).__name__}')
    return config


def refuse_with(what, **stages):
    """``normalise=`` excludes the stages that read float32 scratch planes: filtering does not commute bit for bit with the normaliser."""
    given = [name for name, value in stages.items() if value is not None]
    if given:
        raise RuntimeError(f'{what}: normalise= together with {", ".join(n + "=" for n in given)} is not supported: those stages read float32 '
                           f'scratch planes of the fixed Normalize, and their filters do not commute bit for bit with a per-plane normaliser '
                           f'(geometric augment= is supported)')


def ordered_sum(x):
    """The sum of a float64 1-D array in the stated order: 256 strided partials from +0.0, then the fixed tree."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    rounds = max(1, -(-x.shape[0] // PARTIALS))
    padded = np.zeros(rounds * PARTIALS, dtype=np.float64)                     # a partial never is -0.0, so a +0.0 past the end changes no bit
    padded[:x.shape[0]] = x
    acc = np.zeros(PARTIALS, dtype=np.float64)
    with np.errstate(all='ignore'):
        for row in padded.reshape(rounds, PARTIALS):
            acc = acc + row
        off = PARTIALS // 2
        while off >= 1:
            acc[:off] = acc[:off] + acc[off:2 * off]
            off //= 2
    return acc[0]


def plane_record(plane, config):
    """The four doubles ``(sub, div, stat0, stat1)`` of one plane (any shape, a source dtype): ``lo, hi`` or ``mean, std`` behind the two
    coefficients of ``(m - sub) / div``."""
    plane = np.asarray(plane)
    if plane.dtype not in _SOURCES:
        raise RuntimeError(f'normalise_host: source planes are uint8 / int16 / float32 / float64, got {plane.dtype}')
    if plane.size < 1:
        raise RuntimeError('normalise_host: an empty plane')
    v = plane.astype(np.float64).reshape(-1)
    n, eps = np.float64(v.shape[0]), np.float64(config.eps)
    with np.errstate(all='ignore'):
        if config.mode == _lib.NORM_PERCENTILE:
            lo = hi = np.float64(np.nan)
            if not np.isnan(v).any():                      # numpy: NaNs sort to the end, and one at the end makes every percentile NaN
                lo, hi = _percentile_pair(v + 0.0, config.p0, config.p1)       # -0.0 -> +0.0: the select's keys know one zero
            return np.array([lo, (hi - lo) + eps, lo, hi], dtype=np.float64)
        if config.mode == _lib.NORM_FIXED:
            mean, std = np.float64(config.p0), np.float64(config.p1)
        else:
            mean = ordered_sum(v) / n
            d = v - mean
            std = np.sqrt(ordered_sum(d * d) / n)
        return np.array([mean, eps if std < eps else std, mean, std], dtype=np.float64)      # numpy.clip keeps a NaN: so does the comparison


def normalise_host(plane, config, min_value=0.0, max_value=255.0):
    """``plane`` (any shape, uint8 / int16 / float32 / float64: one item plane) -> ``(float64 array of its shape, record float64 [4])``: the
    normaliser of ``config`` in float64, then -- ``config.then_normalize`` -- ``Normalize(min_value, max_value)``."""
    record = plane_record(plane, checked_config(config, 'normalise_host'))
    with np.errstate(all='ignore'):
        out = (np.asarray(plane).astype(np.float64) - record[0]) / record[1]
        if config.then_normalize:
            if not max_value > min_value:
                raise RuntimeError(f'normalise_host: max_value {max_value} is not above min_value {min_value}')
            out = np.clip(2.0 * ((out - np.float64(min_value)) / (np.float64(max_value) - np.float64(min_value))) - 1.0, -1.0, 1.0)
    return out, record
