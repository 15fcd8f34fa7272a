"""assemble_slices / halo_accumulate: the two ends of the volume loop on the device (C ABI ``afcm_slice_assemble`` / ``afcm_halo_accumulate``,
include/afcm_hip.h; kernels in csrc/volume.hip).

``assemble_slices`` is the ``SliceDataset(phase='test')`` item for a run of consecutive target slices of a source volume that lives on the device;
``halo_accumulate`` is the body of ``SlidingWindowPredictor.accumulate`` for one batch.  Both are asynchronous on the current stream, free of
atomics and bit-identical to the host code they restate.
"""
import torch

from ... import _lib
from ...normalise import checked_config
from .normalise_ops import slice_norm_stats


def _triple(v, what):
    v = tuple(int(x) for x in v)
    if len(v) != 3:
        raise RuntimeError(f'{what}: expected three values (z, y, x), got {v}')
    return v


def assemble_slices(volume, first, count, patch_shape, thickness=None, slice_num=4, min_value=0.0, max_value=255.0, stride_shape=(1, 1, 1),
                    dtype=torch.float32, normalise=None):
    """``volume`` [D, Hs, Ws] (uint8 / int16 / float32 / float64, rows contiguous, any stride in z) -> ``A [count, slice_num, H, W]`` of ``dtype`` and
    ``slice_idx [count, 1]`` float32 for the target slices ``[first, first + count)``, with ``patch_shape = (1, H, W)``: centre crop / constant pad to
    (H, W), the thick slices at -1, 0, +1, +2 ``thickness`` around the target's own (``slice_num`` 4) or the slice itself (1), ``data.normalize``.
    Only the shipped loader geometry exists: patch depth 1, z stride 1, a ``thickness`` with ``slice_num`` 4.
    ``normalise``: a ``NormaliseConfig`` (afcm_amd/normalise.py) -- every plane goes through the reference's ``PercentileNormalizer`` or
    ``Standardize`` in place of the fixed ``Normalize`` (followed by it with ``then_normalize``), in two launches: ``afcm_slice_norm_stats`` writes the
    planes' coefficients, ``afcm_slice_assemble_norm`` applies them."""
    pd, h, w = _triple(patch_shape, 'assemble_slices: patch_shape')
    if pd != 1 or int(stride_shape[0]) != 1:
        raise RuntimeError(f'assemble_slices: patch depth {pd} with z stride {int(stride_shape[0])}: only one slice per patch and z stride 1 are supported')
    _lib.require_slice_num(slice_num, 'assemble_slices')
    if slice_num == 4 and thickness is None:
        raise RuntimeError('assemble_slices: slice number 4 needs a thickness')
    _lib.require_gpu(volume)
    if volume.dim() != 3:
        raise RuntimeError(f'assemble_slices: expected a [D, Hs, Ws] volume, got shape {tuple(volume.shape)}')
    code = _lib.source_code(volume.dtype, 'assemble_slices')
    depth, hs, ws = (int(v) for v in volume.shape)
    if volume.stride(2) != 1 or volume.stride(1) != ws:
        raise RuntimeError(f'assemble_slices: the rows of the source must be contiguous, got strides {tuple(volume.stride())}')
    _lib.require_out_dtype(dtype, 'assemble_slices')
    first, count = int(first), int(count)
    a = torch.empty([max(count, 0), slice_num, h, w], dtype=dtype, device=volume.device)
    slice_idx = torch.empty([max(count, 0), 1], dtype=torch.float32, device=volume.device)
    if checked_config(normalise, 'assemble_slices') is not None:
        coef = slice_norm_stats(volume, first, count, (h, w), thickness, slice_num, normalise)
        rc = _lib.load().afcm_slice_assemble_norm(a.data_ptr(), slice_idx.data_ptr(), volume.data_ptr(), code, _lib.dtype_code(a), depth, hs, ws,
                                                  volume.stride(0), coef.data_ptr(), int(normalise.then_normalize), first, count, slice_num,
                                                  -1 if thickness is None else int(thickness), h, w, float(min_value), float(max_value),
                                                  _lib.stream_ptr(volume))
        _lib.launched(rc, 'slice_assemble_norm')
        return a, slice_idx
    rc = _lib.load().afcm_slice_assemble(a.data_ptr(), slice_idx.data_ptr(), volume.data_ptr(), code, _lib.dtype_code(a), depth, hs, ws,
                                         volume.stride(0), first, count, slice_num, -1 if thickness is None else int(thickness), h, w,
                                         float(min_value), float(max_value), _lib.stream_ptr(volume))
    _lib.launched(rc, 'slice_assemble')
    return a, slice_idx


def halo_accumulate(prediction_map, normalization_mask, prediction, origins, first, patch_halo, prediction_channel=None, box=None):
    """Adds the batch ``prediction`` [B, C, d, h, w] (or [B, C, h, w]: d = 1; float32 / float16 / bfloat16, any strides) into
    ``prediction_map`` [Cm, D, H, W] float32 and counts the visits in ``normalization_mask`` (same shape, uint8), in place, with ``remove_halo``'s crop.
    ``origins``: DEVICE int32 [P, 3], the first voxel (z, y, x) of every patch of the volume; the batch is patches ``[first, first + B)``.
    ``box`` = ((z0, z1), (y0, y1), (x0, x1)) bounds the batch's patches (the caller knows it from its index list; None: the whole volume)."""
    _lib.require_gpu(prediction_map, normalization_mask, prediction, origins)
    if prediction.dim() == 4:
        prediction = prediction.unsqueeze(2)                 # a view: the network's [B, C, h, w] is the d = 1 case
    if prediction.dim() != 5:
        raise RuntimeError(f'halo_accumulate: expected a [B, C, d, h, w] or [B, C, h, w] prediction, got shape {tuple(prediction.shape)}')
    if prediction_map.dim() != 4 or prediction_map.dtype != torch.float32 or not prediction_map.is_contiguous():
        raise RuntimeError(f'halo_accumulate: the map must be a contiguous float32 [C, D, H, W], got {prediction_map.dtype} {tuple(prediction_map.shape)}')
    if normalization_mask.shape != prediction_map.shape or normalization_mask.dtype != torch.uint8 or not normalization_mask.is_contiguous():
        raise RuntimeError(f'halo_accumulate: the mask must be a contiguous uint8 tensor of the map\'s shape, got {normalization_mask.dtype} '
                           f'{tuple(normalization_mask.shape)}')
    if origins.dim() != 2 or origins.shape[1] != 3 or origins.dtype != torch.int32 or not origins.is_contiguous():
        raise RuntimeError(f'halo_accumulate: the origin table must be a contiguous int32 [P, 3], got {origins.dtype} {tuple(origins.shape)}')
    if len({t.device for t in (prediction_map, normalization_mask, prediction, origins)}) != 1:
        raise RuntimeError('halo_accumulate: map, mask, prediction and origin table must be on one device')
    halo = _triple(patch_halo, 'halo_accumulate: patch_halo')
    cm, D, H, W = (int(v) for v in prediction_map.shape)
    b, c, pd, ph, pw = (int(v) for v in prediction.shape)
    (z0, z1), (y0, y1), (x0, x1) = ((0, D), (0, H), (0, W)) if box is None else box
    rc = _lib.load().afcm_halo_accumulate(prediction_map.data_ptr(), normalization_mask.data_ptr(), prediction.data_ptr(), _lib.dtype_code(prediction),
                                          *prediction.stride(), c, origins.data_ptr(), int(origins.shape[0]), int(first), b, pd, ph, pw, *halo, D, H, W,
                                          cm, -1 if prediction_channel is None else int(prediction_channel), int(z0), int(z1), int(y0), int(y1), int(x0),
                                          int(x1), _lib.stream_ptr(prediction_map))
    _lib.launched(rc, 'halo_accumulate')
