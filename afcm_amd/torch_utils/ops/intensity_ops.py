"""rescale_intensity: the reference's intensity rescaling (data/prepare_h5.py:9-41) for a volume that lives on the device (C ABI
``afcm_rescale_intensity``, include/afcm_hip.h; kernels in csrc/intensity.hip).

Asynchronous on the current stream, free of global atomics and of host reads, bit-identical from call to call and to
``afcm_amd.intensity.rescale_intensity_host``.
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


def rescale_plan(voxels, dtype):
    """Where the select's seams are for a volume of ``voxels`` elements of torch ``dtype``, from the library itself (pure host, no GPU needed):
    {'groups': histogram workgroups, 'chunk': voxels of one workgroup per round of the grid, 'passes': digits, 'bits': their widths, most
    significant first}."""
    code = _lib.source_code(dtype, 'rescale_plan')
    plan = (C.c_int32 * _PLAN_VALUES)()
    _lib.launched(_lib.load().afcm_rescale_plan(int(voxels), code, plan), 'rescale_plan')
    return {'groups': plan[0], 'chunk': plan[1], 'passes': plan[2], 'bits': tuple(plan[3:3 + plan[2]])}


def rescale_intensity(volume, percentiles=(0.5, 99.5), out=None):
    """``volume`` [D, H, W] (uint8 / int16 / float32 / float64, rows contiguous, any stride in z, any offset) -> ``(out, stats)``: ``out`` uint8
    [D, H, W] with the voxels above zero mapped onto grey levels 1..255 between the two percentiles of those voxels and everything else 0, ``stats``
    float64 [3] = (lo, hi, n) on the device.  All arithmetic is float64 whatever the source type (numpy's ``linear`` percentile; the statement is in
    include/afcm_hip.h); for float32 sources the reference, which stays in float32, can differ by one grey level at a few voxels in 10^5.  No
    foreground: zeros and NaN percentiles.  ``out``: a contiguous uint8 tensor of the volume's shape on its device to write into."""
    q_lo, q_hi = percentile_fractions(percentiles)
    if not isinstance(volume, torch.Tensor) or volume.dim() != 3:
        raise RuntimeError(f'rescale_intensity: expected a [D, H, W] tensor, got {type(volume).__name__} of shape {tuple(getattr(volume, "shape", ()))}')
    code = _lib.source_code(volume.dtype, 'rescale_intensity')
    d, h, w = (int(v) for v in volume.shape)
    if min(d, h, w) < 1 or d * h * w >= 2 ** 31:
        raise RuntimeError(f'rescale_intensity: a volume has between 1 and 2^31 - 1 voxels, got shape {(d, h, w)}')
    if volume.stride(2) != 1 or volume.stride(1) != w or volume.stride(0) < 0:
        raise RuntimeError(f'rescale_intensity: the rows of the source must be contiguous, got strides {tuple(volume.stride())}')
    if out is not None:
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != (d, h, w) or out.dtype != torch.uint8 or not out.is_contiguous():
            raise RuntimeError(f'rescale_intensity: out must be a contiguous uint8 tensor of shape {(d, h, w)}, got '
                               f'{getattr(out, "dtype", type(out).__name__)} {tuple(getattr(out, "shape", ()))}')
        if out.device != volume.device:
            raise RuntimeError(f'rescale_intensity: out is on {out.device}, the volume on {volume.device}')
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
