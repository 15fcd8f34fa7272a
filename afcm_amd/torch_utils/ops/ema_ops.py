"""ema_multi: the G_ema update of the reference's training loop (train.py:74-77) as ONE launch (C ABI ``afcm_ema_multi``, include/afcm_hip.h; kernel in
csrc/ema.hip): every parameter ``p_ema <- p.lerp(p_ema, beta)``, every buffer copied byte for byte, whatever its dtype.

``EmaTable`` holds the device table of one ``(net_ema, net)`` pair.  Parameters and buffers are updated in place for the life of a module, so the table
is built once, through one pinned host copy, outside any stream capture (``FusedScrubAdam``'s rules): ``update()`` allocates nothing and uploads
nothing, and can be captured.  ``update()`` checks the pointers on the host and refuses a module whose tensors have been replaced since.
"""
import torch

from ... import _lib


def ema_rows(pairs, chunk):
    """``pairs``: (dst, src, kind) tensors; the table rows (dst, src, numel, chunk0, kind) and the chunk count.  Empty tensors take no row."""
    rows, chunks = [], 0
    for dst, src, kind in pairs:
        if dst.shape != src.shape or dst.dtype != src.dtype:
            raise RuntimeError(f'ema: a tensor of the EMA copy is {dst.dtype} {tuple(dst.shape)}, its source {src.dtype} {tuple(src.shape)}')
        if not dst.is_contiguous() or not src.is_contiguous():
            raise RuntimeError('ema: the parameters and buffers of both modules must be contiguous')
        if kind == _lib.EMA_LERP and dst.dtype != torch.float32:
            raise RuntimeError(f'ema: parameters are lerped in float32, got {dst.dtype}')
        units = dst.numel() if kind == _lib.EMA_LERP else dst.numel() * dst.element_size()
        if units == 0:
            continue
        rows.append((dst.data_ptr(), src.data_ptr(), units, chunks, kind))
        chunks += (units + chunk - 1) // chunk
    return rows, chunks


class EmaTable:
    def __init__(self, net_ema, net):
        p_ema, p = list(net_ema.parameters()), list(net.parameters())
        b_ema, b = list(net_ema.buffers()), list(net.buffers())
        if len(p_ema) != len(p) or len(b_ema) != len(b):
            raise RuntimeError('EmaTable: the EMA copy and the network differ in their parameters or buffers')
        self.pairs = [(d, s, _lib.EMA_LERP) for d, s in zip(p_ema, p)] + [(d, s, _lib.EMA_COPY) for d, s in zip(b_ema, b)]
        self._build()

    @classmethod
    def from_pairs(cls, pairs):
        """A table over explicit ``(dst, src, kind)`` tensors (``_lib.EMA_LERP`` / ``_lib.EMA_COPY``)."""
        self = cls.__new__(cls)
        self.pairs = list(pairs)
        self._build()
        return self

    def _build(self):
        tensors = [t for d, s, _ in self.pairs for t in (d, s)]
        if not tensors:
            raise RuntimeError('EmaTable: nothing to update')
        _lib.require_gpu(*tensors)
        if len({t.device for t in tensors}) != 1:
            raise RuntimeError('EmaTable: every tensor must be on one device')
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('EmaTable: build the table before the capture (it allocates and uploads)')
        self.device = tensors[0].device
        self.rows, self.chunks = ema_rows(self.pairs, _lib.load().afcm_adam_chunk_elems())
        if not self.rows:
            raise RuntimeError('EmaTable: nothing to update')
        self.host = torch.tensor(self.rows, dtype=torch.int64).reshape(-1).pin_memory()
        self.table = torch.empty(self.host.numel(), dtype=torch.int64, device=self.device)
        self.table.copy_(self.host, non_blocking=True)
        self.live = [(d, s) for d, s, _ in self.pairs if d.numel()]
        self.touched = [d for d, _ in self.live]

    def current(self):
        """Whether every tensor still lives where the table points (a ``load_state_dict`` copies in place and keeps it so; ``module.to()`` does not)."""
        return all(d.data_ptr() == r[0] and s.data_ptr() == r[1] for (d, s), r in zip(self.live, self.rows))

    @torch.no_grad()
    def update(self, beta=None, schedule=None):
        """One launch on the current stream.  ``beta``: a host number in [0, 1]; ``schedule``: a ``DeviceSchedule`` or its block, beta is slot 3 when
        the kernel runs."""
        if (beta is None) == (schedule is None):
            raise RuntimeError('EmaTable.update: give beta or schedule, not both and not neither')
        if not self.current():
            raise RuntimeError('EmaTable.update: a parameter or buffer has moved since the table was built; build a new table')
        block = None
        if schedule is not None:
            block = getattr(schedule, 'block', schedule)
            if not isinstance(block, torch.Tensor) or block.dtype != torch.float64 or block.numel() != _lib.SCHEDULE_SLOTS or block.device != self.device:
                raise RuntimeError(f'EmaTable.update: schedule must be a DeviceSchedule or its float64 [{_lib.SCHEDULE_SLOTS}] block on {self.device}')
        _lib.launched(_lib.load().afcm_ema_multi(self.table.data_ptr(), len(self.rows), self.chunks, 0.0 if beta is None else float(beta), _lib.ptr(block),
                                                 _lib.stream_ptr(self.table)), 'ema_multi')
        torch.autograd.graph.increment_version(self.touched)
