"""The reference's two intensity normalisations for a volume that lives on the device (include/afcm_hip.h; kernels in csrc/intensity.hip):
``rescale_intensity``, the rescaling of data/prepare_h5.py:9-41 (C ABI ``afcm_rescale_intensity``), and ``percentile_clip``, the
``__percentile_clip`` of data/cmsrnii_dataset.py:79-114 with its caller's uint8 cast (``afcm_percentile_bounds`` + ``afcm_clip_normalize``).

Asynchronous on the current stream, free of global atomics and of host reads, bit-identical from call to call and to
``afcm_amd.intensity.rescale_intensity_host`` / ``percentile_clip_host``.
"""
import ctypes as C

import torch

from ... import _lib

_PLAN_VALUES = 11


def percentile_fractions(percentiles, what='rescale_intensity'):
    """(q_lo / 100, q_hi / 100) of a pair of percentiles with 0 <= q_lo <= q_hi <= 100; RuntimeError otherwise."""
    try:
        q_lo, q_hi = (float(q) for q in percentiles)
    except (TypeError, ValueError):
        raise RuntimeError(f'{what}: percentiles must be a pair (q_lo, q_hi), got {percentiles!r}') from None
    if not 0.0 <= q_lo <= q_hi <= 100.0:                   # a NaN fails every comparison
        raise RuntimeError(f'{what}: percentiles ({q_lo}, {q_hi}) must satisfy 0 <= q_lo <= q_hi <= 100')
    return q_lo / 100.0, q_hi / 100.0


def _plan(entry, voxels, dtype, what):
    code = _lib.source_code(dtype, what)
    plan = (C.c_int32 * _PLAN_VALUES)()
    _lib.launched(getattr(_lib.load(), entry)(int(voxels), code, plan), what)
    return {'groups': plan[0], 'chunk': plan[1], 'passes': plan[2], 'bits': tuple(plan[3:3 + plan[2]])}


def _checked_volume(volume, what):
    """(dtype code, d, h, w) of a [D, H, W] source tensor with contiguous rows; RuntimeError otherwise."""
    if not isinstance(volume, torch.Tensor) or volume.dim() != 3:
        raise RuntimeError(f'{what}: expected a [D, H, W] tensor, got {type(volume).__name__} of shape {tuple(getattr(volume, "shape", ()))}')
    code = _lib.source_code(volume.dtype, what)
    d, h, w = (int(v) for v in volume.shape)
    if min(d, h, w) < 1 or d * h * w >= 2 ** 31:
        raise RuntimeError(f'{what}: a volume has between 1 and 2^31 - 1 voxels, got shape {(d, h, w)}')
    if volume.stride(2) != 1 or volume.stride(1) != w or volume.stride(0) < 0:
        raise RuntimeError(f'{what}: the rows of the source must be contiguous, got strides {tuple(volume.stride())}')
    return code, d, h, w


def _checked_out(out, volume, what):
    """``out=`` of an op on ``volume``: None, or a contiguous uint8 tensor of its shape on its device."""
    if out is None:
        return
    shape = tuple(volume.shape)
    if not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != torch.uint8 or not out.is_contiguous():
        raise RuntimeError(f'{what}: out must be a contiguous uint8 tensor of shape {shape}, got '
                           f'{getattr(out, "dtype", type(out).__name__)} {tuple(getattr(out, "shape", ()))}')
    if out.device != volume.device:
        raise RuntimeError(f'{what}: out is on {out.device}, the volume on {volume.device}')


def rescale_plan(voxels, dtype):
    """Where the select's seams are for a volume of ``voxels`` elements of torch ``dtype``, from the library itself (pure host, no GPU needed):
    {'groups': histogram workgroups, 'chunk': voxels of one workgroup per round of the grid, 'passes': digits, 'bits': their widths, most
    significant first}."""
    return _plan('afcm_rescale_plan', voxels, dtype, 'rescale_plan')


def rescale_intensity(volume, percentiles=(0.5, 99.5), out=None):
    """``volume`` [D, H, W] (uint8 / int16 / float32 / float64, rows contiguous, any stride in z, any offset) -> ``(out, stats)``: ``out`` uint8
    [D, H, W] with the voxels above zero mapped onto grey levels 1..255 between the two percentiles of those voxels and everything else 0, ``stats``
    float64 [3] = (lo, hi, n) on the device.  All arithmetic is float64 whatever the source type (numpy's ``linear`` percentile; the statement is in
    include/afcm_hip.h); for float32 sources the reference, which stays in float32, can differ by one grey level at a few voxels in 10^5.  No
    foreground: zeros and NaN percentiles.  ``out``: a contiguous uint8 tensor of the volume's shape on its device to write into."""
    q_lo, q_hi = percentile_fractions(percentiles)
    code, d, h, w = _checked_volume(volume, 'rescale_intensity')
    _checked_out(out, volume, 'rescale_intensity')
    _lib.require_gpu(volume)
    lib = _lib.load()
    if out is None:
        out = torch.empty((d, h, w), dtype=torch.uint8, device=volume.device)
    stats = torch.empty(3, dtype=torch.float64, device=volume.device)
    workspace = torch.empty(int(lib.afcm_rescale_workspace_bytes(d * h * w, code)) // 8 + 1, dtype=torch.int64, device=volume.device)
    rc = lib.afcm_rescale_intensity(out.data_ptr(), stats.data_ptr(), workspace.data_ptr(), volume.data_ptr(), code, d, h, w, volume.stride(0), q_lo, q_hi,
                                    _lib.stream_ptr(volume))
    _lib.launched(rc, 'rescale_intensity')
    return out, stats


def percentile_plan(voxels, dtype):
    """``rescale_plan`` for the percentile clip's select, whose keys carry a sign: every digit 8 bits -- uint8 one pass, int16 two, float32 four,
    float64 eight."""
    return _plan('afcm_percentile_plan', voxels, dtype, 'percentile_plan')


def _bounds(volume, q_lo, q_hi, strictly_positive, what):
    code, d, h, w = _checked_volume(volume, what)
    _lib.require_gpu(volume)
    lib = _lib.load()
    stats = torch.empty(4, dtype=torch.float64, device=volume.device)
    workspace = torch.empty(int(lib.afcm_percentile_workspace_bytes(d * h * w, code)) // 8 + 1, dtype=torch.int64, device=volume.device)
    rc = lib.afcm_percentile_bounds(stats.data_ptr(), workspace.data_ptr(), volume.data_ptr(), code, d, h, w, volume.stride(0), q_lo, q_hi,
                                    int(bool(strictly_positive)), _lib.stream_ptr(volume))
    _lib.launched(rc, what)
    return stats


def percentile_bounds(volume, percentiles, strictly_positive=True):
    """``stats`` float64 [4] = (lo, hi, n, nan_count) on the device: numpy's ``linear`` percentiles of EVERY voxel of ``volume`` [D, H, W] (uint8 /
    int16 / float32 / float64, rows contiguous, any stride in z, any offset) in float64, ``lo`` raised to 0 where it is negative and
    ``strictly_positive``; both NaN if the volume holds a NaN.  The statement is in include/afcm_hip.h."""
    q_lo, q_hi = percentile_fractions(percentiles, 'percentile_bounds')
    return _bounds(volume, q_lo, q_hi, strictly_positive, 'percentile_bounds')


def percentile_clip(volume, percentiles=(0.5, 99.5), strictly_positive=True, reference=None, out=None):
    """``volume`` [D, H, W] -> ``(out, stats)``: ``out`` uint8 [D, H, W] = trunc((clip(v, lo, hi) - lo) / (hi - lo) * 255) in float64, a NaN there 0,
    with ``stats`` = ``percentile_bounds(reference, ...)``; ``reference`` (default: the volume itself) may have another shape and dtype.  ``out``: a
    contiguous uint8 tensor of the volume's shape on its device to write into."""
    q_lo, q_hi = percentile_fractions(percentiles, 'percentile_clip')
    code, d, h, w = _checked_volume(volume, 'percentile_clip')
    _checked_out(out, volume, 'percentile_clip')
    if reference is None:
        reference = volume
    elif isinstance(reference, torch.Tensor) and reference.device != volume.device:
        raise RuntimeError(f'percentile_clip: reference is on {reference.device}, the volume on {volume.device}')
    stats = _bounds(reference, q_lo, q_hi, strictly_positive, 'percentile_clip')
    if out is None:
        out = torch.empty((d, h, w), dtype=torch.uint8, device=volume.device)
    rc = _lib.load().afcm_clip_normalize(out.data_ptr(), stats.data_ptr(), volume.data_ptr(), code, d, h, w, volume.stride(0), _lib.stream_ptr(volume))
    _lib.launched(rc, 'percentile_clip')
    return out, stats
