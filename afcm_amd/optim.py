"""Fused gradient scrub + Adam for the generator update (C ABI ``afcm_adam_multi``).

The reference's G update is ``nan_to_num`` on every gradient followed by ``torch.optim.Adam(lr, betas=(0, 0.99))``
(models/stylegan3_model.py:122-124,132-135; models/comodgan_model.py:19-20).  Run eagerly that is ~110 tiny launches plus
seven multi-tensor passes over the 234 MB of parameters; here one HIP launch reads p, g, m, v and writes p, m, v once for
every tensor.  State layout (``step``, ``exp_avg``, ``exp_avg_sq`` per parameter) and the update arithmetic are
torch.optim.Adam's, so ``state_dict()`` round-trips with it -- also for a capturable optimizer whose captured step has been
replayed: ``state_dict()`` reads the step count back from the device, ``load_state_dict()`` re-creates it from the loaded state.
"""
import ctypes
import math

import torch

from . import _lib


class FusedScrubAdam(torch.optim.Optimizer):
    """``g * grad_scale`` -> ``nan_to_num`` -> Adam, one launch per parameter group.  One step count per group (the largest in the group
    + 1; a parameter without a gradient is left alone).  ``capturable=True`` keeps that count on the device so that ``step()`` can be
    captured into a graph: replays advance the device count only, ``device_step()`` reads it, and ``state_dict()`` writes it into
    ``state[p]['step']`` of the parameters the captured step updates, so a checkpoint taken after replays resumes at the right step.
    ``stats=True`` puts one ``afcm_grad_stats`` launch in front of every Adam launch: what the scrub is about to replace and the gradients' sum of
    squares, per chunk, for ``grad_stats()`` and the training log (afcm_amd/trainlog.py)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, scrub=True, posinf=1e5, neginf=-1e5, write_grad=False, capturable=False, lr_dev=None,
                 stats=False):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1):
            raise ValueError('invalid Adam hyper-parameters')
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps))
        # stats: every step() launches afcm_grad_stats (csrc/trainlog.hip) over the group's pointer table right before the Adam launch: per chunk the
        # sum of squares of the finite scaled gradients and the counts of NaN / +inf / -inf the scrub is about to replace, into a persistent float64
        # [chunks of ALL the group's parameters, 4] tensor made here (nothing is allocated during a capture).  False: nothing is launched or allocated
        self.stats = bool(stats)
        self._stats = {}           # group index -> [partials, chunks written by the last step, that step's count]
        if self.stats:
            chunk = _lib.load().afcm_adam_chunk_elems()
            for gi, group in enumerate(self.param_groups):
                rows = sum((p.numel() + chunk - 1) // chunk for p in group['params'])
                self._stats[gi] = [torch.zeros((max(1, rows), 4), dtype=torch.float64, device=group['params'][0].device), 0, 0]
        self.scrub, self.posinf, self.neginf, self.write_grad = bool(scrub), float(posinf), float(neginf), bool(write_grad)
        self._tables = {}          # (group index, device) -> (rows, device table, pinned host copy)
        # capturable: the step count is a device scalar per group and the bias corrections are formed in the kernel (C ABI
        # afcm_adam_multi_capturable_d), so the launch can be captured into a hipGraph and replayed (bench.py --graph).  Replays advance the
        # device scalar only: `device_step()` is the count, and `state_dict()` copies it into state['step'] (see there)
        self.capturable = bool(capturable)
        self._step_dev = {}        # (group index, device) -> the count, a float32 device scalar; made at the group's first step from state['step']
        # lr_dev: the learning rate as a float64 DEVICE scalar (a view of slot 4 or 5 of a DeviceSchedule block, afcm_amd/schedule.py) that the kernel
        # reads at every launch, so that a captured step follows a learning-rate schedule; param_groups[...]['lr'] is then informational (set_lr)
        if lr_dev is not None:
            if not self.capturable:
                raise ValueError('FusedScrubAdam: lr_dev needs capturable=True')
            if not isinstance(lr_dev, torch.Tensor) or lr_dev.dtype != torch.float64 or lr_dev.numel() != 1 or lr_dev.device.type != 'cuda':
                raise ValueError('FusedScrubAdam: lr_dev must be a float64 device tensor of one element')
            if len(self.param_groups) != 1:
                raise ValueError('FusedScrubAdam: lr_dev serves one parameter group')
        self.lr_dev = lr_dev

    def set_lr(self, lr):
        """param_groups[...]['lr'] <- lr.  With ``lr_dev`` the kernel reads the device scalar, which its owner writes (``DeviceSchedule.set_lr``): this
        keeps the informational copy in step with it."""
        for group in self.param_groups:
            group['lr'] = float(lr)

    def _state(self, p):
        st = self.state[p]
        if len(st) == 0:
            st['step'] = torch.tensor(0.0, dtype=torch.float32)
            st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @torch.no_grad()
    def step(self, closure=None, grads=None, grad_scale=1.0):
        """One update.  ``grads``: optional {parameter: gradient tensor} (e.g. slices of the all-reduce buckets, so the
        reduced values are consumed in place); default ``p.grad``.  ``grad_scale`` multiplies every gradient first
        (1 / world size after a sum all-reduce)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        chunk = lib.afcm_adam_chunk_elems()
        for gi, group in enumerate(self.param_groups):
            beta1, beta2 = group['betas']
            rows = []
            touched = []
            chunks = 0
            step_t = None
            for p in group['params']:
                g = grads.get(p) if grads is not None else p.grad
                if g is None:
                    continue
                if p.dtype != torch.float32 or g.dtype != torch.float32:
                    raise RuntimeError('FusedScrubAdam updates float32 parameters with float32 gradients')
                _lib.require_gpu(p, g)
                if not p.is_contiguous():
                    raise RuntimeError('FusedScrubAdam needs contiguous parameters')
                if not g.is_contiguous():
                    g = g.contiguous()
                    if grads is None:
                        p.grad = g
                st = self._state(p)
                if step_t is None:
                    # one step count per group (bias corrections are launch scalars): the largest per-parameter count + 1.
                    # torch.optim.Adam counts per parameter; the two only differ for a parameter that skipped a step.
                    step_t = int(max(float(self._state(q)['step']) for q in group['params'])) + 1
                st['step'].fill_(step_t)
                rows.append((p.data_ptr(), g.data_ptr(), st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr(), p.numel(), chunks))
                touched.extend((p, st['exp_avg'], st['exp_avg_sq']))
                chunks += (p.numel() + chunk - 1) // chunk
            if not rows:
                continue
            dev = group['params'][0].device
            key = (gi, dev)
            ent = self._tables.get(key)
            if ent is None or ent[0] != rows:
                # the pointer table only changes when the allocator hands out different gradient blocks: steady-state steps
                # skip the upload.  A fresh pinned tensor per change: an in-flight copy never sees it rewritten.
                if self.capturable:
                    # ONE pinned buffer for the optimizer's life (nothing is allocated while a stream capture is under way): rewritten in
                    # place -- after a synchronize in eager steps (an earlier upload may not have run yet), as it is during a capture (the
                    # captured copy node reads the buffer at every replay: the captured step is then the only one that may run)
                    new = torch.tensor(rows, dtype=torch.int64).reshape(-1)
                    if ent is None:
                        host = torch.empty(6 * len(group['params']), dtype=torch.int64).pin_memory()
                        table = torch.empty(6 * len(group['params']), dtype=torch.int64, device=dev)
                    else:
                        table, host = ent[1], ent[2]
                    if not torch.cuda.is_current_stream_capturing():
                        torch.cuda.current_stream(dev).synchronize()
                    host[:new.numel()].copy_(new)
                    table[:new.numel()].copy_(host[:new.numel()], non_blocking=True)
                    self._tables[key] = ent = (rows, table, host)
                else:
                    host = torch.tensor(rows, dtype=torch.int64).reshape(-1).pin_memory()
                    table = ent[1] if (ent is not None and ent[1].numel() >= host.numel()) else torch.empty(6 * len(group['params']), dtype=torch.int64, device=dev)
                    table[:host.numel()].copy_(host, non_blocking=True)
                    self._tables[key] = ent = (rows, table, host)
            table = ent[1]
            if self.stats:
                # the same table, chunk count and scale as the Adam launch below, on the same stream, in front of it (it may write g back)
                gs = self._stats.get(gi)
                if gs is None or gs[0].device != dev or gs[0].shape[0] < chunks:
                    raise RuntimeError('FusedScrubAdam(stats=True): the statistics tensor is made at construction from the parameters the group has '
                                       'then, on their device; this group has changed since')
                _lib.launched(lib.afcm_grad_stats(ctypes.c_void_p(table.data_ptr()), len(rows), chunks, float(grad_scale), ctypes.c_void_p(gs[0].data_ptr()),
                                                  _lib.stream_ptr(table)), 'grad_stats')
                gs[1], gs[2] = chunks, step_t
            if self.capturable:
                sd = self._step_dev.get(key)
                if sd is None:
                    sd = self._step_dev[key] = torch.full([1], float(step_t - 1), dtype=torch.float32, device=dev)
                if self.lr_dev is not None:
                    _lib.launched(lib.afcm_adam_multi_capturable_lr(ctypes.c_void_p(table.data_ptr()), len(rows), chunks, ctypes.c_void_p(sd.data_ptr()),
                                                                  ctypes.c_void_p(self.lr_dev.data_ptr()), beta1, beta2, group['eps'], float(grad_scale),
                                                                  int(self.scrub), self.posinf, self.neginf, int(self.write_grad),
                                                                  _lib.stream_ptr(table)), 'adam_multi_capturable_lr')
                    torch.autograd.graph.increment_version(touched)
                    continue
                _lib.launched(lib.afcm_adam_multi_capturable_d(ctypes.c_void_p(table.data_ptr()), len(rows), chunks, ctypes.c_void_p(sd.data_ptr()), group['lr'],
                                                             beta1, beta2, group['eps'], float(grad_scale), int(self.scrub), self.posinf, self.neginf,
                                                             int(self.write_grad), _lib.stream_ptr(table)), 'adam_multi_capturable')
                torch.autograd.graph.increment_version(touched)
                continue
            # bias corrections in double on the host, as torch.optim.Adam does for non-capturable steps
            bc1 = 1.0 - beta1 ** step_t
            bc2 = 1.0 - beta2 ** step_t
            _lib.launched(lib.afcm_adam_multi(ctypes.c_void_p(table.data_ptr()), len(rows), chunks, group['lr'] / bc1, beta1, beta2,
                                              1.0 - beta1, 1.0 - beta2, math.sqrt(bc2), group['eps'], float(grad_scale), int(self.scrub), self.posinf, self.neginf,
                                              int(self.write_grad), _lib.stream_ptr(table)), 'adam_multi')
            # the kernel wrote through raw pointers: tell autograd (version counters), so that anything keyed on a parameter's version --
            # saved-tensor checks, caches of derived tensors such as packed weight images -- sees the update
            torch.autograd.graph.increment_version(touched)
        return loss


    def _pull_device_steps(self):
        """state['step'] <- the device count, for the parameters of each capturable group's current pointer table: the ones the last step
        updated, eagerly or in the capture, and so the ones every replay updates.  One synchronising read per group."""
        for key, sd in self._step_dev.items():
            ent = self._tables.get(key)
            if ent is None:
                continue
            count = float(sd.item())
            stepped = {row[0] for row in ent[0]}
            for p in self.param_groups[key[0]]['params']:
                st = self.state.get(p)
                if st and p.data_ptr() in stepped:
                    st['step'].fill_(count)

    def state_dict(self):
        """torch.optim.Adam's layout.  A capturable optimizer first brings state['step'] up to the device count, which replays of a captured
        step advance without the host: the checkpoint, and the optimizer itself from here on, carry the number of steps that ran."""
        self._pull_device_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """The next step starts from the loaded state: the device count is made anew from the loaded state['step'], the pointer tables from
        the loaded moments.  A graph captured before the load still points at the old ones: capture again."""
        super().load_state_dict(state_dict)
        self._step_dev = {}
        self._tables = {}

    def snapshot(self):
        """Clones of the moments and step counts as they stand (parameters that have not stepped yet have none): for ``restore``."""
        moments = {p: {k: v.clone() for k, v in self.state[p].items()} for group in self.param_groups for p in group['params'] if p in self.state}
        counts = {key: t.clone() for key, t in self._step_dev.items()}
        if self.stats:                                       # with stats=True a third member: the statistics of the last step, as grad_stats() gives them
            return moments, counts, {gi: [gs[0].clone(), gs[1], gs[2]] for gi, gs in self._stats.items()}
        return moments, counts

    @torch.no_grad()
    def restore(self, snapshot):
        """Puts a ``snapshot`` back IN PLACE, so that pointer tables and a captured step stay valid; state made since the snapshot starts from zero."""
        moments, counts = snapshot[:2]
        for p, st in self.state.items():
            for k, v in st.items():
                v.copy_(moments[p][k]) if p in moments else v.zero_()
        for key, t in self._step_dev.items():
            t.copy_(counts[key]) if key in counts else t.zero_()
        if self.stats and len(snapshot) > 2:
            for gi, (partials, chunks, count) in snapshot[2].items():
                self._stats[gi][0].copy_(partials)
                self._stats[gi][1:] = [chunks, count]

    def grad_stats(self, group=0):
        """``(partials, chunks)`` of the last step of a ``stats=True`` optimizer: the persistent float64 [*, 4] device tensor of per-chunk rows
        ``{sumsq, n_nan, n_posinf, n_neginf}`` (C ABI ``afcm_grad_stats``) and how many of its rows that step wrote -- the chunks of the parameters
        that had a gradient, in table order; 0 before the first step.  A replayed graph rewrites the rows of the step it captured."""
        if not self.stats:
            raise RuntimeError('FusedScrubAdam.grad_stats: this optimizer was built without stats=True')
        gs = self._stats[group]
        return gs[0], gs[1]

    def device_step(self, group=0):
        """The step count of a capturable optimizer (a device scalar; reading it synchronises)."""
        for (gi, _), t in self._step_dev.items():
            if gi == group:
                return int(t.item())
        return 0


class _WeightedL1(torch.autograd.Function):
    """weight * mean(|a - b|) for fp32 device tensors in two launches forward (partials + their sum) and one backward (C ABI afcm_l1_partials /
    afcm_l1_grad); gradient for `a` only."""

    @staticmethod
    def forward(ctx, a, b, weight):
        _lib.require_gpu(a, b)
        lib = _lib.load()
        a, b = a.contiguous(), b.contiguous()
        numel = a.numel()
        blocks = max(1, min(256, (numel + 4095) // 4096))
        partials = torch.empty([blocks], dtype=torch.float32, device=a.device)
        _lib.launched(lib.afcm_l1_partials(partials.data_ptr(), a.data_ptr(), b.data_ptr(), numel, blocks, float(weight), _lib.stream_ptr(a)), 'l1_partials')
        ctx.save_for_backward(a, b)
        ctx.weight = float(weight)
        return partials.sum()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        a, b = ctx.saved_tensors
        ga = torch.empty_like(a)
        gout = gout.to(torch.float32).contiguous()
        _lib.launched(_lib.load().afcm_l1_grad(ga.data_ptr(), a.data_ptr(), b.data_ptr(), gout.data_ptr(), a.numel(), ctx.weight, _lib.stream_ptr(a)), 'l1_grad')
        return ga, None, None


def weighted_l1(a, b, weight):
    """``torch.nn.L1Loss()(a, b) * weight`` (models/stylegan3_model.py:107); the fused form for fp32 device tensors of one shape where only `a`
    needs a gradient, the op-by-op composition otherwise."""
    if a.is_cuda and a.dtype == torch.float32 and b.dtype == torch.float32 and a.shape == b.shape and not b.requires_grad and a.numel() > 0:
        return _WeightedL1.apply(a, b, float(weight))
    return torch.nn.functional.l1_loss(a, b) * weight
