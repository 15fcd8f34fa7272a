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


def rescale_intensity_host(array, percentiles=(0.5, 99.5)):
    """``array`` [D, H, W] (uint8 / int16 / float32 / float64) -> ``(uint8 [D, H, W], stats float64 [3] = lo, hi, n)``."""
    q_lo, q_hi = intensity_ops.percentile_fractions(percentiles, 'rescale_intensity_host')
    array = np.asarray(array)
    if array.ndim != 3:
        raise RuntimeError(f'rescale_intensity_host: expected a [D, H, W] array, got shape {array.shape}')
    if array.dtype not in _SOURCES:
        raise RuntimeError(f'rescale_intensity_host: source volumes are uint8 / int16 / float32 / float64, got {array.dtype}')
    foreground = array > 0
    values = array[foreground]
    n = int(values.shape[0])
    out = np.zeros(array.shape, dtype=np.uint8)
    if n == 0:
        return out, np.array([np.nan, np.nan, 0.0])
    ranks, gammas = [], []
    for q in (q_lo, q_hi):
        vi = q * float(n - 1)
        i = int(np.floor(vi))
        ranks += [i, min(i + 1, n - 1)]
        gammas.append(vi - np.floor(vi))
    picked = np.partition(values, sorted(set(ranks)))[ranks].astype(np.float64)          # the four order statistics, exact
    with np.errstate(all='ignore'):
        lo, hi = _lerp(picked[0], picked[1], gammas[0]), _lerp(picked[2], picked[3], gammas[1])
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
