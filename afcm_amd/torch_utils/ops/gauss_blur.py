"""gauss_blur: the loss-side Gaussian blur of the `--model stylegan3` step (models/stylegan3_model.py:24-30, 97-103) with sigma read on the device
(C ABI ``afcm_gauss_blur``, include/afcm_hip.h; kernels in csrc/blur.hip).

``f = exp2(-(i / sigma)^2)`` for ``i`` in ``[-r, r]``, ``r = floor(3 sigma)``, normalised by its sum, applied along both axes with zero padding
``r``: ``upfirdn2d.filter2d(x, f / f.sum())``.  With ``schedule`` the kernels read sigma and radius from the schedule block when they run, so the
two launches captured into a graph follow the fade (afcm_amd/schedule.py).  The filter is symmetric and the padding zero: the op is self-adjoint,
and its backward is the op itself on the gradient -- called through the autograd function again, so the discriminator's R1 term can differentiate
through it twice.
"""
import math

import torch

from ... import _lib


def rmax():
    """The largest radius ``floor(3 sigma)`` the kernels are built for (at least 30: the shipped schedules start at sigma 10)."""
    return int(_lib.load().afcm_gauss_blur_rmax())


def _block_of(schedule):
    block = getattr(schedule, 'block', schedule)
    if not isinstance(block, torch.Tensor) or block.dtype != torch.float64 or tuple(block.shape) != (_lib.SCHEDULE_SLOTS,) or not block.is_contiguous():
        raise RuntimeError(f'gauss_blur: schedule must be a DeviceSchedule or its block, a contiguous float64 [{_lib.SCHEDULE_SLOTS}] tensor')
    return block


class _GaussBlur(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, sigma, block):
        ctx.sigma, ctx.block = sigma, block
        n, c, h, w = x.shape
        xf = x.to(torch.float32).contiguous()
        y = torch.empty_like(xf)
        # the row pass's output; not needed where the host knows the radius is 0 (with a block it is only known on the device)
        scratch = torch.empty_like(xf) if block is not None or math.floor(sigma * 3) > 0 else None
        _lib.launched(_lib.load().afcm_gauss_blur(y.data_ptr(), xf.data_ptr(), _lib.ptr(scratch), n * c, h, w, float(sigma), _lib.ptr(block),
                                                  _lib.stream_ptr(xf)), 'gauss_blur')
        return y if x.dtype == torch.float32 else y.to(x.dtype)

    @staticmethod
    def backward(ctx, gy):
        return _GaussBlur.apply(gy, ctx.sigma, ctx.block), None, None


def gauss_blur(x, sigma=None, schedule=None):
    """``x``: DEVICE [N, C, H, W]; fp32 runs as it is, any other floating dtype is converted up and back.  Exactly one of ``sigma`` (a host number,
    refused when its radius exceeds ``rmax()``) and ``schedule`` (a ``DeviceSchedule`` or its block: sigma and radius are slots 1 and 2 at run time).
    Radius 0 returns a copy of ``x``, bit for bit.  A block radius beyond ``rmax()`` cannot raise from the device: every output is NaN."""
    if (sigma is None) == (schedule is None):
        raise RuntimeError('gauss_blur: give sigma or schedule, not both and not neither')
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or not x.is_floating_point() or x.numel() < 1:
        raise RuntimeError(f'gauss_blur: x must be a non-empty floating-point [N, C, H, W] tensor, got {getattr(x, "dtype", type(x).__name__)} '
                           f'{tuple(getattr(x, "shape", ()))}')
    block = None if schedule is None else _block_of(schedule)
    _lib.require_gpu(x, block)
    if schedule is not None:
        if block.device != x.device:
            raise RuntimeError(f'gauss_blur: x is on {x.device}, the schedule block on {block.device}')
        sigma = 0.0
    else:
        sigma = float(sigma)
        if not (sigma >= 0.0) or math.floor(sigma * 3) > rmax():
            raise RuntimeError(f'gauss_blur: sigma {sigma} is negative, not a number, or its radius floor(3 sigma) exceeds {rmax()}')
    return _GaussBlur.apply(x, sigma, block)
