"""The training loop's time-dependent scalars: the device-resident schedule block and the learning-rate policies.

A replayed graph carries the launch scalars of the step it was captured from.  Three scalars of the reference's loop change over time -- the loss-side
blur sigma (models/stylegan3_model.py:115-116), the EMA beta (train.py:67-73) and the learning rate (models/utils.py:43-69, one scheduler step per
epoch: train.py:44).  ``DeviceSchedule`` keeps them in a block of 8 doubles on the device (layout: include/afcm_hip.h), advanced by one launch per
step (``afcm_schedule_advance``, csrc/schedule.hip); the blur, the EMA and the Adam kernels read the block, so one captured graph stays right for a
whole run.  ``LRSchedule`` is the rate after the k-th ``update_learning_rate()`` call; the host writes it into the block once per epoch.
"""
import math

import torch

from . import _lib

TOTAL_ITERS, BLUR_SIGMA, BLUR_RADIUS, EMA_BETA, LR_G, LR_D = range(6)


class DeviceSchedule:
    """``blur_init_sigma`` / ``blur_fade_kimg``: the fade of the loss-side blur (0: no blur).  ``ema_kimgs`` / ``ramp``: the EMA half-life and its ramp
    (``ema_kimgs=None``: no EMA; the beta slot then holds 0 and nothing reads it).  ``total_iters``: images seen so far (a resumed run).  ``lr_G`` /
    ``lr_D`` (default: ``lr_G``): the rates the optimizers read from slots 4 and 5."""

    def __init__(self, device, blur_init_sigma=0.0, blur_fade_kimg=0.0, ema_kimgs=None, ramp=None, total_iters=0, lr_G=0.0025, lr_D=None):
        self.blur_init_sigma, self.blur_fade_kimg = float(blur_init_sigma), float(blur_fade_kimg)
        self.ema_kimgs = None if ema_kimgs is None else float(ema_kimgs)
        self.ramp = None if ramp is None else float(ramp)
        if not (self.blur_init_sigma >= 0) or (self.ramp is not None and self.ramp < 0) or (self.ema_kimgs is not None and self.ema_kimgs < 0):
            raise ValueError('DeviceSchedule: blur_init_sigma, ema_kimgs and ramp must not be negative')
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError(f'DeviceSchedule needs a ROCm device (got {device}); host_values() is the host arm')
        cap = int(_lib.load().afcm_gauss_blur_rmax())
        if self.blur_fade_kimg > 0 and math.floor(3 * self.blur_init_sigma) > cap:
            raise ValueError(f'DeviceSchedule: blur_init_sigma {self.blur_init_sigma} has radius {math.floor(3 * self.blur_init_sigma)}, the blur kernels '
                             f'are built for at most {cap}')
        self.block = torch.zeros(_lib.SCHEDULE_SLOTS, dtype=torch.float64, device=device)
        self.lr_G_dev, self.lr_D_dev = self.block[LR_G:LR_G + 1], self.block[LR_D:LR_D + 1]      # views: what FusedScrubAdam(lr_dev=...) reads
        self._set(total_iters, lr_G, lr_G if lr_D is None else lr_D)

    def _values(self, total_iters, batch_size=1):
        return self.host_values(total_iters, batch_size, self.blur_init_sigma, self.blur_fade_kimg, self.ema_kimgs, self.ramp)

    def _set(self, total_iters, lr_G, lr_D):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('DeviceSchedule: the block is written from the host between replays, never inside a capture')
        v = self._values(total_iters)
        self.lr_G, self.lr_D = float(lr_G), float(lr_D)
        # (the beta of a fresh block belongs to no step yet: advance() writes the first one that is read)
        self.block.copy_(torch.tensor([float(total_iters), v['blur_sigma'], v['blur_radius'], 0.0, self.lr_G, self.lr_D, 0.0, 0.0], dtype=torch.float64))

    @staticmethod
    def host_values(total_iters, batch_size, blur_init_sigma=0.0, blur_fade_kimg=0.0, ema_kimgs=None, ramp=None):
        """The reference's Python expressions at ``total_iters`` (already advanced by this step's batch, as train.py:50-53 passes it): the host arm,
        and what the kernel is held to.  models/stylegan3_model.py:115-116, 97-98; train.py:69-73."""
        blur_sigma = (max(1 - total_iters / (blur_fade_kimg * 1e3), 0) * blur_init_sigma) if blur_fade_kimg > 0 else 0.0
        ema_nimg = (0.0 if ema_kimgs is None else ema_kimgs) * 1000
        if ramp is not None:
            ema_nimg = min(ema_nimg, total_iters * ramp)
        ema_beta = 0.5 ** (batch_size / max(ema_nimg, 1e-8))
        return dict(total_iters=float(total_iters), blur_sigma=float(blur_sigma), blur_radius=float(math.floor(blur_sigma * 3)), ema_beta=ema_beta)

    def advance(self, batch_size):
        """``total_iters += batch_size`` and sigma, radius, beta from it: one thread on the current stream; can be captured."""
        _lib.launched(_lib.load().afcm_schedule_advance(self.block.data_ptr(), int(batch_size), self.blur_init_sigma, self.blur_fade_kimg,
                                                        0.0 if self.ema_kimgs is None else self.ema_kimgs, -1.0 if self.ramp is None else self.ramp,
                                                        _lib.stream_ptr(self.block)), 'schedule_advance')

    def set_lr(self, lr_G, lr_D=None):
        """Writes the learning-rate slots in place (a synchronising host write): between replays, never inside a capture.  ``lr_D`` defaults to
        ``lr_G``, as in the constructor and in the steps' ``set_lr``."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('DeviceSchedule.set_lr: the rates are written between replays, never inside a capture')
        self.lr_G, self.lr_D = float(lr_G), float(lr_G if lr_D is None else lr_D)
        self.block[LR_G:LR_D + 1].copy_(torch.tensor([self.lr_G, self.lr_D], dtype=torch.float64))

    def read(self):
        """The block as a dict (synchronises)."""
        v = self.block.cpu().tolist()
        return dict(total_iters=v[0], blur_sigma=v[1], blur_radius=v[2], ema_beta=v[3], lr_G=v[4], lr_D=v[5])

    def state_dict(self):
        r = self.read()
        return dict(total_iters=r['total_iters'], lr_G=r['lr_G'], lr_D=r['lr_D'])

    def load_state_dict(self, state):
        self._set(state['total_iters'], state['lr_G'], state['lr_D'])


class LRSchedule:
    """The learning rate after the k-th ``update_learning_rate()`` call (k = 1 at the top of the first epoch, train.py:44) under the reference's
    policies (models/utils.py:56-66) -- what ``scheduler.step()`` leaves in ``param_groups[0]['lr']``, without an optimizer:
      linear   lr * (1 - max(0, k + epoch_count - n_epochs) / (n_epochs_decay + 1))                       (LambdaLR)
      step     lr * 0.1 ** (k // lr_decay_iters), as the repeated product the scheduler forms             (StepLR, gamma 0.1)
      cosine   lr * (1 + cos(pi k / n_epochs)) / 2, by the scheduler's own recurrence                      (CosineAnnealingLR, T_max n_epochs, eta_min 0)
      plateau  not implemented: it steps on a metric the reference never sets."""

    def __init__(self, policy, lr, epoch_count=1, n_epochs=50, n_epochs_decay=50, lr_decay_iters=50):
        if policy == 'plateau':
            raise NotImplementedError('LRSchedule: the plateau policy needs a validation metric, which the reference never sets (models/base_model.py:121)')
        if policy not in ('linear', 'step', 'cosine'):
            raise NotImplementedError(f'learning rate policy [{policy}] is not implemented')
        self.policy, self.lr = policy, float(lr)
        self.epoch_count, self.n_epochs, self.n_epochs_decay, self.lr_decay_iters = int(epoch_count), int(n_epochs), int(n_epochs_decay), int(lr_decay_iters)
        self._cosine = [self.lr]                     # the recurrence's values, k = 0, 1, ...

    def lr_at(self, k):
        k = int(k)
        if k < 0:
            raise ValueError(f'LRSchedule.lr_at: k = {k}')
        if self.policy == 'linear':
            return self.lr * (1.0 - max(0, k + self.epoch_count - self.n_epochs) / float(self.n_epochs_decay + 1))
        if self.policy == 'step':
            lr = self.lr
            for _ in range(k // self.lr_decay_iters):
                lr = lr * 0.1
            return lr
        # CosineAnnealingLR's chainable form: near k = T_max the closed form and the recurrence differ by far more than a rounding
        t_max = self.n_epochs
        while len(self._cosine) <= k:
            e, prev = len(self._cosine), self._cosine[-1]
            if (e - 1 - t_max) % (2 * t_max) == 0:
                self._cosine.append(prev + self.lr * (1 - math.cos(math.pi / t_max)) / 2)
            else:
                self._cosine.append((1 + math.cos(math.pi * e / t_max)) / (1 + math.cos(math.pi * (e - 1) / t_max)) * prev)
        return self._cosine[k]
