"""The training log on the device: one row of doubles per training step, written inside the step, read by the host whenever it likes.

The reference's ``train.py`` reads ``get_current_losses()`` every ``print_freq`` images (models/pix2pix_model.py:75 names ``G_GAN``, ``G_L1``, ``D_real``,
``D_fake``; ``Dr1`` sits beside them).  A step replayed as a graph has no host between its launches: its loss tensors are graph buffers that every
replay overwrites, and ``FusedScrubAdam`` replaces NaN and +-inf gradients without a word.  ``DeviceTrainLog`` is a ring of ``capacity`` rows in device
memory; ``append(step)`` is what ``optimize_parameters()`` of a step built with ``log=`` ends with -- one gather of the five loss scalars and one
``afcm_trainlog_append`` launch (csrc/trainlog.hip), which also adds up the per-chunk gradient statistics the optimizers' ``afcm_grad_stats`` launches
left (``FusedScrubAdam(stats=True)``).  ``read()`` is ONE device -> host copy.  Row layout: include/afcm_hip.h.
"""
import ctypes

import numpy as np
import torch

from . import _lib

LOSSES = ('G_GAN', 'G_L1', 'D_real', 'D_fake', 'Dr1')
COLUMNS = (('serial', 'total_iters', 'blur_sigma', 'blur_radius', 'ema_beta', 'lr_G', 'lr_D', 'spare6', 'spare7', 'step_G', 'step_D') + LOSSES +
           ('G_sumsq', 'G_nan', 'G_posinf', 'G_neginf', 'D_sumsq', 'D_nan', 'D_posinf', 'D_neginf'))


def unroll(ring, head, since=None):
    """The live rows of a ring in chronological order, and how many were lost.  ``ring``: [capacity, cols], row ``s % capacity`` holding serial ``s``;
    ``head``: the number of rows ever appended.  The live serials are ``max(0, head - capacity) .. head - 1``.  ``since``: the first serial wanted
    (None: 0) -- ``rows`` are the live ones from there on, ``lost`` counts the serials in ``[since, head)`` that were overwritten before this read.  Pure
    numpy."""
    ring = np.asarray(ring)
    capacity, head = int(ring.shape[0]), int(head)
    first = 0 if since is None else int(since)
    if capacity < 1 or head < 0 or first < 0:
        raise ValueError(f'unroll: capacity {capacity}, head {head}, since {since}')
    live = max(0, head - capacity)
    start = min(max(first, live), head)
    serials = np.arange(start, head, dtype=np.int64)
    return ring[serials % capacity].copy(), max(0, live - first)


class DeviceTrainLog:
    """``capacity`` rows of ``len(COLUMNS)`` float64 on ``device`` and the int64 ``head`` (rows ever appended), in ONE allocation so that ``read`` copies
    both at once.  Give it to a step (``StyleGAN3GeneratorStep(..., log=log)`` / ``StyleGAN3Step``); a row is then appended at the end of every
    ``optimize_parameters()``, eagerly and in every replay of a graph the step was captured into."""

    def __init__(self, capacity, device='cuda'):
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError(f'DeviceTrainLog: capacity {capacity} is below 1')
        self.capacity, self.cols = capacity, len(COLUMNS)
        self._buf = torch.zeros(capacity * self.cols + 1, dtype=torch.float64, device=torch.device(device))
        self.device = self._buf.device                                                  # (with its index: what a parameter's .device is compared to)
        self.log = self._buf[:capacity * self.cols].view(capacity, self.cols)
        self.head = self._buf[capacity * self.cols:].view(torch.int64)                  # int64 0 and float64 +0.0 are the same bits
        # persistent (a captured append holds their addresses): the gathered losses, the NaN that stands for an absent one, the step counts of
        # optimizers that keep theirs on the host
        self._losses = torch.full((len(LOSSES),), float('nan'), dtype=torch.float32, device=self.device)
        self._absent = torch.full((), float('nan'), dtype=torch.float32, device=self.device)
        self._host_steps = {}

    def _step_count(self, opt):
        """The optimizer's step count as a device float: a capturable optimizer's own; otherwise a scalar of the log's, filled from the host count."""
        if opt.capturable:
            for (gi, _), t in opt._step_dev.items():
                if gi == 0:
                    return t
            return None
        t = self._host_steps.get(id(opt))
        if t is None:
            t = self._host_steps[id(opt)] = torch.zeros(1, dtype=torch.float32, device=self.device)
        t.fill_(float(opt._stats[0][2]))
        return t

    @torch.no_grad()
    def append(self, step):
        """One row for the step that has just run: ``step.loss_G_GAN`` ... ``step.loss_Dr1`` (those the step has; NaN otherwise) gathered by one
        ``torch.stack`` into the persistent 5-float tensor, then ``afcm_trainlog_append`` on the current stream.  Two launches; can be captured."""
        if self.device.type != 'cuda':
            raise RuntimeError(f'DeviceTrainLog.append needs a log on a ROCm device (this one is on {self.device})')
        lib = _lib.load()
        if lib.afcm_trainlog_cols() != self.cols:
            raise RuntimeError(f'DeviceTrainLog: the library writes rows of {lib.afcm_trainlog_cols()} columns, COLUMNS has {self.cols}')
        scalars = []
        for name in LOSSES:
            v = getattr(step, 'loss_' + name, None)
            scalars.append(self._absent if v is None else v.detach().reshape(()).to(torch.float32))
        torch.stack(scalars, out=self._losses)
        opt_G, opt_D = step.optimizer_G, getattr(step, 'optimizer_D', None)
        part_G, chunks_G = opt_G.grad_stats()
        part_D, chunks_D = (None, 0) if opt_D is None else opt_D.grad_stats()
        schedule = getattr(step, 'schedule', None)
        vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        _lib.launched(lib.afcm_trainlog_append(vp(self.log), self.capacity, vp(self.head), None if schedule is None else vp(schedule.block),
                                               vp(self._step_count(opt_G)), None if opt_D is None else vp(self._step_count(opt_D)), vp(self._losses),
                                               vp(part_G), chunks_G, vp(part_D), chunks_D, _lib.stream_ptr(self._buf)), 'trainlog_append')

    def read(self, since=None):
        """``(rows, lost)``: the live rows from serial ``since`` on (None: from serial 0) in chronological order as a float64 ndarray
        [n, len(COLUMNS)], and the number of rows from there on that the ring had already overwritten (``unroll``).  Exactly one device -> host copy,
        which synchronises with the steps enqueued so far."""
        host = self._buf.cpu().numpy()
        return unroll(host[:-1].reshape(self.capacity, self.cols), host[-1:].view(np.int64)[0], since)

    def snapshot(self):
        """A clone of rows and head, for ``restore``."""
        return self._buf.clone()

    @torch.no_grad()
    def restore(self, snapshot, head_only=False):
        """Puts a ``snapshot`` back IN PLACE (a captured append keeps pointing at the ring); ``head_only``: the head alone, the rows stay."""
        if head_only:
            self.head.copy_(snapshot[-1:].view(torch.int64))
        else:
            self._buf.copy_(snapshot)
