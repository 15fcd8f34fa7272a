"""assemble_batch / advance_cursor: a training batch from a device-resident pool of volumes (C ABI ``afcm_batch_assemble`` /
``afcm_batch_assemble_aug`` / ``afcm_batch_assemble_noise`` / ``afcm_batch_assemble_elastic`` / ``afcm_batch_assemble_blur`` /
``afcm_cursor_advance``, include/afcm_hip.h; kernels in csrc/batch.hip, csrc/elastic.hip and csrc/augment_blur.hip).

``assemble_batch`` is ``SliceDataset(phase='train').__getitem__`` for ``count`` rows of a device-side item table -- ``A``, ``B`` and ``slice_idx`` in
one launch, bit-identical to the stacked host items.  The tables live on the device, so the kernel checks every row itself: an invalid row comes out
as a NaN item and reads nothing.  Both calls are asynchronous on the current stream and can be captured into a graph.
"""
import ctypes

import torch

from ... import _lib
from ...normalise import checked_config, refuse_with
from .normalise_ops import plane_norm_stats


def _table(t, what, dtype, cols):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != cols or t.dtype != dtype or not t.is_contiguous() or t.shape[0] < 1:
        got = f'{t.dtype} {tuple(t.shape)}' if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f'assemble_batch: {what} must be a contiguous {dtype} [n, {cols}] with n >= 1, got {got}')


def assemble_batch(pool, vols, items, first, count, patch_hw, slice_num=4, min_value=0., max_value=255., dtype=torch.float32, out=None, cursor=None,
                   augment=None, intensity=None, independent_planes=False, elastic=None, elastic_ops=None, workspace=None, blur=None,
                   normalise=None, norm_coef=None):
    """``pool``: 1-D DEVICE tensor (uint8 / int16 / float32 / float64) holding every volume; ``vols``: DEVICE int64 [n_vols, 4] (element offset into the
    pool, depth, hs, ws); ``items``: DEVICE int32 [n_items, 4] (vol_a, vol_b, idx, thickness; thickness -1: none, ``slice_num`` 1 only).  Sample ``i`` is
    table row ``(cursor[0] if cursor is not None else 0) + first + i``.  Returns ``A [count, slice_num, H, W]``, ``B [count, 1, H, W]`` of ``dtype``
    and ``slice_idx [count, 1]`` float32 with ``patch_hw = (H, W)``: per volume centre crop / constant pad, the thick slices at -1, 0, +1, +2
    ``thickness`` around the target's own (``slice_num`` 4) or the slice itself (1), ``data.normalize``.  ``out=(A, B, slice_idx)`` writes into existing
    tensors (a captured graph needs stable addresses); ``cursor``: DEVICE int64 scalar tensor, see ``advance_cursor``.
    ``augment``: DEVICE float64 [n_items, 8], one parameter row ``(flip_h, flip_w, k, angle, c, s, off_y, off_x)`` beside every item row
    (``afcm_amd.augment.augment_rows``): the item's planes flipped, turned by quarters and rotated as the reference's ``RandomFlip``,
    ``RandomRotate90`` and ``RandomRotate`` do (``afcm_batch_assemble_aug``); an invalid parameter row is a NaN item as an invalid item row is.
    ``intensity``: DEVICE float64 [n_items, 36], one row beside every item row (``afcm_amd.augment_intensity.intensity_rows``): contrast change,
    Gaussian and Poisson noise as the reference's ``RandomContrast``, ``AdditiveGaussianNoise`` and ``AdditivePoissonNoise`` apply them, after the
    geometric transforms, from a Philox field generated in the kernel (``afcm_batch_assemble_noise``, with or without ``augment``);
    ``independent_planes``: every plane of an item its own field.  An invalid row is a NaN item.
    ``elastic``: DEVICE float64 [n_items, 4], one row ``(flag, alpha, key_lo, key_hi)`` beside every item row
    (``afcm_amd.augment_elastic.elastic_rows``): the item's planes deformed as the reference's ``ElasticDeformation`` does, after the geometric
    transforms and before the intensity ones, in a fixed number of launches (``afcm_batch_assemble_elastic``, with or without the other two tables);
    ``elastic_ops = (op_h, op_w, order)``: the DEVICE float64 [H, H] and [W, W] smoothing operators (``augment_elastic.smoothing_operator``) and
    the spline order, 0, 1 or 3; ``workspace``: a DEVICE uint8 tensor of at least ``elastic_workspace_bytes(count, slice_num, H, W, order)`` (a
    captured graph needs a persistent one), allocated per call when None.  An invalid row is a NaN item.
    ``blur``: DEVICE float64 [n_items, 20 (slice_num + 1)], one row beside every item row, per plane ``(flag, sigma, radius, w_0 ... w_16)``
    (``afcm_amd.augment_blur.blur_rows``): every plane with flag 1 filtered as the reference's ``GaussianBlur3D`` does, after the geometric
    transforms and the elastic deformation and before the intensity ones, in a fixed number of launches (``afcm_batch_assemble_blur``, with or
    without the other three tables); ``workspace`` then holds at least ``blur_workspace_bytes(count, slice_num, H, W, order)``, ``order`` the
    spline order of the elastic table or None without one.  An invalid row is a NaN item.
    ``normalise``: a ``NormaliseConfig`` (afcm_amd/normalise.py) -- every plane of every item goes through the reference's ``PercentileNormalizer``
    or ``Standardize`` in place of the fixed ``Normalize`` (followed by it with ``then_normalize``), in two launches: ``afcm_plane_norm_stats`` writes
    the planes' coefficients, ``afcm_batch_assemble_norm`` applies them, with or without ``augment``.  ``norm_coef``: a DEVICE float64
    [n >= count, slice_num + 1, 4] the coefficients are written to (a captured graph needs a persistent one), allocated per call when None.
    ``normalise`` excludes ``intensity``, ``elastic`` and ``blur``."""
    h, w = (int(v) for v in patch_hw)
    first, count = int(first), int(count)
    _lib.require_slice_num(slice_num, 'assemble_batch')
    if not isinstance(pool, torch.Tensor) or pool.dim() != 1 or not pool.is_contiguous() or pool.numel() < 1:
        raise RuntimeError(f'assemble_batch: the pool must be a non-empty contiguous 1-D tensor, got shape {tuple(getattr(pool, "shape", ()))}')
    code = _lib.source_code(pool.dtype, 'assemble_batch')
    _table(vols, 'the volume table', torch.int64, 4)
    _table(items, 'the item table', torch.int32, 4)
    if augment is not None:
        _table(augment, 'the augment table', torch.float64, 8)
        if augment.shape[0] != items.shape[0]:
            raise RuntimeError(f'assemble_batch: the augment table has {augment.shape[0]} rows, the item table {items.shape[0]}: one parameter row per item row')
    if intensity is not None:
        _table(intensity, 'the intensity table', torch.float64, 36)
        if intensity.shape[0] != items.shape[0]:
            raise RuntimeError(f'assemble_batch: the intensity table has {intensity.shape[0]} rows, the item table {items.shape[0]}: one row per item row')
    if checked_config(normalise, 'assemble_batch') is not None:
        refuse_with('assemble_batch', intensity=intensity, elastic=elastic, blur=blur)
    elif norm_coef is not None:
        raise RuntimeError('assemble_batch: norm_coef= only with normalise=')
    if not isinstance(independent_planes, bool):
        raise RuntimeError(f'assemble_batch: independent_planes must be a bool, got {independent_planes!r}')
    if independent_planes and intensity is None:
        raise RuntimeError('assemble_batch: independent_planes without an intensity table')
    if (elastic is None) != (elastic_ops is None) or (elastic is None and blur is None and workspace is not None):
        raise RuntimeError('assemble_batch: elastic= (the table) and elastic_ops= (op_h, op_w, order) go together, workspace= only with them or blur=')
    if elastic is not None:
        _table(elastic, 'the elastic table', torch.float64, 4)
        if elastic.shape[0] != items.shape[0]:
            raise RuntimeError(f'assemble_batch: the elastic table has {elastic.shape[0]} rows, the item table {items.shape[0]}: one row per item row')
        if not isinstance(elastic_ops, (tuple, list)) or len(elastic_ops) != 3:
            raise RuntimeError(f'assemble_batch: elastic_ops must be (op_h, op_w, order), got {elastic_ops!r}')
        op_h, op_w, order = elastic_ops
        for name, op, n in (('op_h', op_h, h), ('op_w', op_w, w)):
            if not isinstance(op, torch.Tensor) or op.dtype != torch.float64 or tuple(op.shape) != (n, n) or not op.is_contiguous():
                got = f'{op.dtype} {tuple(op.shape)}' if isinstance(op, torch.Tensor) else type(op).__name__
                raise RuntimeError(f'assemble_batch: elastic_ops {name} must be a contiguous torch.float64 [{n}, {n}] for a patch of [{h}, {w}], got {got}')
        if isinstance(order, bool) or order not in (0, 1, 3):
            raise RuntimeError(f'assemble_batch: the spline order must be 0, 1 or 3, got {order!r}')
    if blur is not None:
        _table(blur, 'the blur table', torch.float64, 20 * (slice_num + 1))
        if blur.shape[0] != items.shape[0]:
            raise RuntimeError(f'assemble_batch: the blur table has {blur.shape[0]} rows, the item table {items.shape[0]}: one row per item row')
    _lib.require_out_dtype(dtype, 'assemble_batch')
    if count < 1 or first < 0 or h < 1 or w < 1:
        raise RuntimeError(f'assemble_batch: {count} items from row {first} at [{h}, {w}]: count and the patch must be positive, first not negative')
    if cursor is not None and (not isinstance(cursor, torch.Tensor) or cursor.dtype != torch.int64 or cursor.numel() != 1):
        raise RuntimeError(f'assemble_batch: the cursor must be an int64 tensor of one element, got {getattr(cursor, "dtype", type(cursor).__name__)} '
                           f'{tuple(getattr(cursor, "shape", ()))}')
    shapes = ((count, slice_num, h, w), (count, 1, h, w), (count, 1))
    if out is None:
        a = torch.empty(shapes[0], dtype=dtype, device=pool.device)
        b = torch.empty(shapes[1], dtype=dtype, device=pool.device)
        slice_idx = torch.empty(shapes[2], dtype=torch.float32, device=pool.device)
    else:
        if len(out) != 3:
            raise RuntimeError(f'assemble_batch: out must be (A, B, slice_idx), got {len(out)} values')
        a, b, slice_idx = out
        for name, t, shape, want in (('A', a, shapes[0], dtype), ('B', b, shapes[1], dtype), ('slice_idx', slice_idx, shapes[2], torch.float32)):
            if tuple(t.shape) != shape or t.dtype != want or not t.is_contiguous():
                raise RuntimeError(f'assemble_batch: out {name} must be a contiguous {want} {shape}, got {t.dtype} {tuple(t.shape)} '
                                   f'with strides {tuple(t.stride())}')
    tensors = (pool, vols, items, a, b, slice_idx) + (() if cursor is None else (cursor,)) + (() if augment is None else (augment,)) + \
        (() if intensity is None else (intensity,))
    if elastic is not None or blur is not None:
        if blur is not None:
            need = blur_workspace_bytes(count, slice_num, h, w, None if elastic is None else order)
        else:
            need = elastic_workspace_bytes(count, slice_num, h, w, order)
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=pool.device)
        elif not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous() or \
                workspace.numel() < need:
            got = f'{workspace.dtype} {tuple(workspace.shape)}' if isinstance(workspace, torch.Tensor) else type(workspace).__name__
            raise RuntimeError(f'assemble_batch: the workspace must be a contiguous 1-D uint8 tensor of at least {need} bytes, got {got}')
        tensors += (workspace,) + (() if elastic is None else (elastic, op_h, op_w)) + (() if blur is None else (blur,))
    _lib.require_gpu(*tensors)
    if len({t.device for t in tensors}) != 1:
        raise RuntimeError(f'assemble_batch: pool, tables, outputs and cursor must be on one device, got {sorted({str(t.device) for t in tensors})}')
    head = (a.data_ptr(), b.data_ptr(), slice_idx.data_ptr(), pool.data_ptr(), pool.numel(), code, vols.data_ptr(), int(vols.shape[0]), items.data_ptr(),
            int(items.shape[0]))
    tail = (_lib.ptr(cursor), first, count, slice_num, h, w, _lib.dtype_code(a), float(min_value), float(max_value), _lib.stream_ptr(pool))
    if normalise is not None:
        coef = plane_norm_stats(pool, vols, items, first, count, (h, w), slice_num, normalise, cursor=cursor, out=norm_coef)
        rc = _lib.load().afcm_batch_assemble_norm(*head, _lib.ptr(augment), coef.data_ptr(), int(normalise.then_normalize), *tail)
    elif blur is not None:
        more = (None, None, None, -1) if elastic is None else (elastic.data_ptr(), op_h.data_ptr(), op_w.data_ptr(), int(order))
        rc = _lib.load().afcm_batch_assemble_blur(*head, _lib.ptr(augment), _lib.ptr(intensity), int(independent_planes), *more, blur.data_ptr(),
                                                  workspace.data_ptr(), workspace.numel(), *tail)
    elif elastic is not None:
        rc = _lib.load().afcm_batch_assemble_elastic(*head, _lib.ptr(augment), _lib.ptr(intensity), int(independent_planes), elastic.data_ptr(),
                                                     op_h.data_ptr(), op_w.data_ptr(), int(order), workspace.data_ptr(), workspace.numel(), *tail)
    elif intensity is not None:
        rc = _lib.load().afcm_batch_assemble_noise(*head, _lib.ptr(augment), intensity.data_ptr(), int(independent_planes), *tail)
    elif augment is None:
        rc = _lib.load().afcm_batch_assemble(*head, *tail)
    else:
        rc = _lib.load().afcm_batch_assemble_aug(*head, augment.data_ptr(), *tail)
    _lib.launched(rc, 'batch_assemble')
    return a, b, slice_idx


def elastic_workspace_bytes(count, slice_num, h, w, order):
    """The bytes ``afcm_batch_assemble_elastic`` needs for ``count`` items of ``slice_num`` + 1 planes of [h, w] at spline order ``order``
    (``afcm_elastic_plan``): the float32 item, the two float64 fields and their half-smoothed copies and, at order 3, the float64 coefficients."""
    need = ctypes.c_int64(0)
    _lib.launched(_lib.load().afcm_elastic_plan(int(count), int(slice_num), int(h), int(w), int(order), ctypes.byref(need), None), 'elastic_plan')
    return int(need.value)


def blur_workspace_bytes(count, slice_num, h, w, order=None):
    """The bytes ``afcm_batch_assemble_blur`` needs for ``count`` items of ``slice_num`` + 1 planes of [h, w] (``afcm_blur_plan``): the float32 item,
    the float64 intermediate of the two passes and, with an elastic table of spline order ``order``, ``elastic_workspace_bytes`` for its launches."""
    need = ctypes.c_int64(0)
    _lib.launched(_lib.load().afcm_blur_plan(int(count), int(slice_num), int(h), int(w), -1 if order is None else int(order), ctypes.byref(need), None),
                  'blur_plan')
    return int(need.value)


def advance_cursor(cursor, by):
    """``cursor[0] += by`` on the device (one thread on the current stream): the table position a captured graph reads moves without the host."""
    if not isinstance(cursor, torch.Tensor) or cursor.dtype != torch.int64 or cursor.numel() != 1:
        raise RuntimeError(f'advance_cursor: the cursor must be an int64 tensor of one element, got {getattr(cursor, "dtype", type(cursor).__name__)} '
                           f'{tuple(getattr(cursor, "shape", ()))}')
    _lib.require_gpu(cursor)
    _lib.launched(_lib.load().afcm_cursor_advance(cursor.data_ptr(), int(by), _lib.stream_ptr(cursor)), 'cursor_advance')
