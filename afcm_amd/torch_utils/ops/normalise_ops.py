"""The statistics launches of the per-plane normalisers (C ABI ``afcm_plane_norm_stats`` / ``afcm_slice_norm_stats`` / ``afcm_norm_plan``,
include/afcm_hip.h; kernels in csrc/normalise.hip): ``coef [count, planes, 4]`` float64 = ``(sub, div, stat0, stat1)`` per item plane, one
workgroup each, for the items of a device pool or for a run of slices of one volume.  ``assemble_batch(normalise=)`` and
``assemble_slices(normalise=)`` run them in front of ``afcm_batch_assemble_norm`` / ``afcm_slice_assemble_norm``.

Asynchronous on the current stream, capturable, free of global atomics and of host reads, bit-identical from call to call and to
``afcm_amd.normalise.plane_record``.
"""
import ctypes as C

import torch

from ... import _lib
from ...normalise import checked_config


def norm_plan(dtype, config):
    """How the library takes one plane of torch ``dtype`` under ``config`` (pure host, no GPU needed): {'threads': of the plane's one workgroup,
    'passes': times the plane is read (the select's digits, or the two moments), 'digit_bits', 'ranks'}."""
    if checked_config(config, 'norm_plan') is None:
        raise RuntimeError('norm_plan: a NormaliseConfig is needed')
    plan = (C.c_int32 * 4)()
    _lib.launched(_lib.load().afcm_norm_plan(_lib.source_code(dtype, 'norm_plan'), config.mode, plan), 'norm_plan')
    return {'threads': plan[0], 'passes': plan[1], 'digit_bits': plan[2], 'ranks': plan[3]}


def _checked_coef(out, shape, device, what):
    if out is None:
        return torch.empty(shape, dtype=torch.float64, device=device)
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or out.dim() != 3 or not out.is_contiguous() or out.shape[0] < shape[0] or \
            tuple(out.shape[1:]) != shape[1:]:
        got = f'{out.dtype} {tuple(out.shape)}' if isinstance(out, torch.Tensor) else type(out).__name__
        raise RuntimeError(f'{what}: the coefficients must be a contiguous torch.float64 [n >= {shape[0]}, {shape[1]}, 4], got {got}')
    if out.device != device:
        raise RuntimeError(f'{what}: the coefficients are on {out.device}, the source on {device}')
    return out


def plane_norm_stats(pool, vols, items, first, count, patch_hw, slice_num, config, cursor=None, out=None):
    """The coefficients of ``assemble_batch``'s items ``[first, first + count)`` (its ``pool``, ``vols``, ``items``, ``cursor``): float64
    ``[count, slice_num + 1, 4]``, the planes of ``A`` then ``B``.  ``out``: a contiguous float64 ``[n >= count, slice_num + 1, 4]`` to write
    the first ``count`` rows of (a captured graph needs a persistent one).  An invalid item row gives NaN and reads nothing."""
    checked_config(config, 'plane_norm_stats')
    h, w = (int(v) for v in patch_hw)
    _lib.require_slice_num(slice_num, 'plane_norm_stats')
    _lib.require_gpu(pool, vols, items, cursor)
    coef = _checked_coef(out, (int(count), slice_num + 1, 4), pool.device, 'plane_norm_stats')
    rc = _lib.load().afcm_plane_norm_stats(coef.data_ptr(), pool.data_ptr(), pool.numel(), _lib.source_code(pool.dtype, 'plane_norm_stats'),
                                           vols.data_ptr(), int(vols.shape[0]), items.data_ptr(), int(items.shape[0]), _lib.ptr(cursor), int(first),
                                           int(count), slice_num, h, w, config.mode, config.p0, config.p1, config.eps, _lib.stream_ptr(pool))
    _lib.launched(rc, 'plane_norm_stats')
    return coef


def slice_norm_stats(volume, first, count, patch_hw, thickness, slice_num, config, out=None):
    """The coefficients of ``assemble_slices``'s target slices ``[first, first + count)`` of ``volume`` [D, Hs, Ws]: float64
    ``[count, slice_num, 4]``."""
    checked_config(config, 'slice_norm_stats')
    h, w = (int(v) for v in patch_hw)
    _lib.require_slice_num(slice_num, 'slice_norm_stats')
    _lib.require_gpu(volume)
    if volume.dim() != 3 or volume.stride(2) != 1 or volume.stride(1) != volume.shape[2]:
        raise RuntimeError(f'slice_norm_stats: expected a [D, Hs, Ws] volume with contiguous rows, got shape {tuple(volume.shape)} with strides '
                           f'{tuple(volume.stride())}')
    depth, hs, ws = (int(v) for v in volume.shape)
    coef = _checked_coef(out, (max(int(count), 0), slice_num, 4), volume.device, 'slice_norm_stats')
    rc = _lib.load().afcm_slice_norm_stats(coef.data_ptr(), volume.data_ptr(), _lib.source_code(volume.dtype, 'slice_norm_stats'), depth, hs, ws,
                                           volume.stride(0), int(first), int(count), slice_num, -1 if thickness is None else int(thickness), h, w,
                                           config.mode, config.p0, config.p1, config.eps, _lib.stream_ptr(volume))
    _lib.launched(rc, 'slice_norm_stats')
    return coef
