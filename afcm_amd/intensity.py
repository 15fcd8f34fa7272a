"""Intensity rescaling, the first stage of the subject loop: the reference passes every volume it trains or tests on through ``rescale_intensity``
(data/prepare_h5.py:9-41, repeated in evaluate.py:23-40) -- the 0.5th and 99.5th percentile of the voxels above zero, the foreground mapped onto grey
levels 1..255, the background left at 0, uint8.

The statement kept here (include/afcm_hip.h has it in full): a voxel is foreground iff ``v > 0`` (NaN, -inf, -0.0 and negatives are background; +inf
and positive denormals foreground); the percentiles are numpy's ``linear`` method in float64 on the foreground widened exactly to float64; a
foreground voxel becomes ``clip(rint((v - lo) / (hi - lo) * 255), 1, 255)`` in float64, a NaN there 1.  The arithmetic is float64 for EVERY source
type.  The reference agrees bit for bit for uint8, int16 and float64 sources; numpy evaluates a float32 volume in float32, so there its grey level can
differ by one at a few voxels in 10^5.

``rescale_intensity_host`` is that statement in numpy, the host arm; ``torch_utils.ops.intensity_ops.rescale_intensity`` is the device arm, the same
bits; ``rescale_intensity`` dispatches on what it is given.

Subjects that arrive as NIfTI directories (``dataset_mode: cmsrnii``) never pass through that function: the reference normalises them with
``StandardNIIDataset.__percentile_clip`` (data/cmsrnii_dataset.py:79-114) and ``(x * 255).astype('uint8')``.  Its statement: the percentiles of EVERY
voxel (a NaN anywhere makes both NaN), the lower one raised to 0 where negative (``strictly_positive``), then
``trunc((min(max(v, lo), hi) - lo) / (hi - lo) * 255)`` in float64 with a NaN result 0.  ``percentile_clip_host`` / ``percentile_clip`` are its host
arm and its dispatcher; ``torch_utils.ops.intensity_ops.percentile_clip`` the device arm, the same bits.
"""
import numpy as np
import torch

from .torch_utils.ops import intensity_ops

_SOURCES = tuple(np.dtype(t) for t in (np.uint8, np.int16, np.float32, np.float64))


def _lerp(a, b, g):
    """numpy's _lerp for scalars: every product and sum a float64 operation of its own."""
    a, b, g = np.float64(a), np.float64(b), np.float64(g)
    d = b - a
    return b - d * (np.float64(1.0) - g) if g >= 0.5 else a + d * g


def _source_array(array, what):
    array = np.asarray(array)
    if array.ndim != 3:
        raise RuntimeError(f'{what}: expected a [D, H, W] array, got shape {array.shape}')
    if array.dtype not in _SOURCES:
        raise RuntimeError(f'{what}: source volumes are uint8 / int16 / float32 / float64, got {array.dtype}')
    return array


def _percentile_pair(values, q_lo, q_hi):
    """numpy's ``linear`` percentiles of a non-empty 1-D array at the fractions q_lo, q_hi, in float64: the four order statistics by
    ``np.partition``, widened exactly, combined with ``_lerp``."""
    n = int(values.shape[0])
    ranks, gammas = [], []
    for q in (q_lo, q_hi):
        vi = q * float(n - 1)
        i = int(np.floor(vi))
        ranks += [i, min(i + 1, n - 1)]
        gammas.append(vi - np.floor(vi))
    picked = np.partition(values, sorted(set(ranks)))[ranks].astype(np.float64)          # the four order statistics, exact
    with np.errstate(all='ignore'):
        return _lerp(picked[0], picked[1], gammas[0]), _lerp(picked[2], picked[3], gammas[1])


def rescale_intensity_host(array, percentiles=(0.5, 99.5)):
    """``array`` [D, H, W] (uint8 / int16 / float32 / float64) -> ``(uint8 [D, H, W], stats float64 [3] = lo, hi, n)``."""
    q_lo, q_hi = intensity_ops.percentile_fractions(percentiles, 'rescale_intensity_host')
    array = _source_array(array, 'rescale_intensity_host')
    foreground = array > 0
    values = array[foreground]
    n = int(values.shape[0])
    out = np.zeros(array.shape, dtype=np.uint8)
    if n == 0:
        return out, np.array([np.nan, np.nan, 0.0])
    lo, hi = _percentile_pair(values, q_lo, q_hi)
    with np.errstate(all='ignore'):
        level = np.rint((values.astype(np.float64) - lo) / (hi - lo) * np.float64(255.0))
        level = np.where(level >= 1.0, np.minimum(level, 255.0), 1.0)                    # a NaN fails the comparison: 1
    out[foreground] = level.astype(np.uint8)
    return out, np.array([lo, hi, float(n)])


def rescale_intensity(volume, percentiles=(0.5, 99.5), out=None):
    """An ndarray goes through ``rescale_intensity_host`` and comes back as arrays; a device tensor goes through the HIP kernels and comes back
    as device tensors ``(uint8 [D, H, W], stats float64 [3])`` without a host read."""
    if isinstance(volume, np.ndarray):
        if out is not None:
            raise RuntimeError('rescale_intensity: out= is for device tensors')
        return rescale_intensity_host(volume, percentiles)
    if isinstance(volume, torch.Tensor):
        return intensity_ops.rescale_intensity(volume, percentiles, out=out)
    raise RuntimeError(f'rescale_intensity: expected a numpy array or a device tensor, got {type(volume).__name__}')


def percentile_clip_host(array, percentiles=(0.5, 99.5), strictly_positive=True, reference=None):
    """``array`` [D, H, W] (uint8 / int16 / float32 / float64) -> ``(uint8 [D, H, W], stats float64 [4] = lo, hi, n, nan_count)``; the bounds come
    from ``reference`` (default: the array itself), which may have another shape and dtype."""
    q_lo, q_hi = intensity_ops.percentile_fractions(percentiles, 'percentile_clip_host')
    array = _source_array(array, 'percentile_clip_host')
    values = (array if reference is None else _source_array(reference, 'percentile_clip_host: reference')).reshape(-1)
    if values.shape[0] == 0:
        raise RuntimeError('percentile_clip_host: the reference volume is empty')
    nans = int(np.isnan(values).sum()) if values.dtype.kind == 'f' else 0
    lo = hi = np.float64(np.nan)
    if nans == 0:                                          # numpy: NaNs sort to the end, and one at the end makes every percentile NaN
        lo, hi = _percentile_pair(values, q_lo, q_hi)
        if strictly_positive and lo < 0:
            lo = np.float64(0.0)
    with np.errstate(all='ignore'):
        v = array.astype(np.float64)
        level = (np.minimum(np.maximum(v, lo), hi) - lo) / (hi - lo) * np.float64(255.0)
        level = np.where(np.isnan(level), 0.0, level)      # NaN bounds, a NaN voxel, hi == lo, inf / inf
    return level.astype(np.uint8), np.array([lo, hi, float(values.shape[0]), float(nans)])


def percentile_clip(volume, percentiles=(0.5, 99.5), strictly_positive=True, reference=None, out=None):
    """An ndarray goes through ``percentile_clip_host`` and comes back as arrays; a device tensor goes through the HIP kernels and comes back as
    device tensors ``(uint8 [D, H, W], stats float64 [4])`` without a host read."""
    if isinstance(volume, np.ndarray):
        if out is not None:
            raise RuntimeError('percentile_clip: out= is for device tensors')
        return percentile_clip_host(volume, percentiles, strictly_positive, reference)
    if isinstance(volume, torch.Tensor):
        return intensity_ops.percentile_clip(volume, percentiles, strictly_positive, reference, out)
    raise RuntimeError(f'percentile_clip: expected a numpy array or a device tensor, got {type(volume).__name__}')
