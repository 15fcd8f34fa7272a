"""Float64 restatements for the device-side schedule (tests/test_schedule_ref_cpu.py, tests/test_gpu_schedule.py): the loss-side Gaussian blur of
models/stylegan3_model.py:24-30, 97-103 and the reference's schedule expressions written out."""
import math

import numpy as np
import torch

TOTAL_ITERS = (16, 32, 50_000, 99_984, 100_000, 100_016)        # the fade of the shipped configurations: blur_init_sigma 10, blur_fade_kimg 100


def reference_taps(sigma):
    """The normalised filter as the reference forms it, in fp32 (models/stylegan3_model.py:98-103), or None when the blur is off."""
    blur_size = np.floor(sigma * 3)
    if blur_size <= 0:
        return None
    f = torch.arange(-blur_size, blur_size + 1).div(sigma).square().neg().exp2()
    return (f / f.sum()).numpy()


def blur_ref(x, sigma):
    """filter2d(x, f) with the 1-D filter ``f`` of ``reference_taps``: float64, zero padding r on each side, along x and along y; x [..., H, W]."""
    f = reference_taps(sigma)
    x = np.asarray(x, dtype=np.float64)
    if f is None:
        return x.copy()
    f = f.astype(np.float64)
    r = (len(f) - 1) // 2
    h, w = x.shape[-2:]
    pad = [(0, 0)] * (x.ndim - 2)
    xp = np.pad(x, pad + [(0, 0), (r, r)])
    y = sum(f[j] * xp[..., :, j:j + w] for j in range(2 * r + 1))
    yp = np.pad(y, pad + [(r, r), (0, 0)])
    return sum(f[j] * yp[..., j:j + h, :] for j in range(2 * r + 1))


def reference_schedule(total_iters, batch_size, blur_init_sigma, blur_fade_kimg, ema_kimgs, ramp):
    """models/stylegan3_model.py:115-116 and 98, train.py:69-73, as written there; ``total_iters`` already counts this step's batch."""
    cur_nimg = total_iters
    blur_sigma = max(1 - cur_nimg / (blur_fade_kimg * 1e3), 0) * blur_init_sigma if blur_fade_kimg > 0 else 0
    blur_size = np.floor(blur_sigma * 3)
    ema_nimg = ema_kimgs * 1000
    ema_rampup = ramp
    if ema_rampup is not None:
        ema_nimg = min(ema_nimg, total_iters * ema_rampup)
    ema_beta = 0.5 ** (batch_size / max(ema_nimg, 1e-8))
    return float(blur_sigma), float(blur_size), ema_beta


def bits(v):
    return np.float64(v).view(np.uint64)


def rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300) if a != b else 0.0


def lerp_ref(p, p_ema, beta):
    """p + beta (p_ema - p) in float64, and the per-element bound 2^-21 max(|p|, |p_ema|): the roundings of d, of w and of the fused sum are each
    at most 2^-23 of the larger magnitude (|d| <= 2 max)."""
    p, p_ema = p.double(), p_ema.double()
    return p + beta * (p_ema - p), torch.maximum(p.abs(), p_ema.abs()) * 2.0 ** -21
