"""group_expand: ``out_k[b] = in_k[groups[b]]`` over whole per-sample blocks, for several tensors in ONE launch (C ABI ``afcm_group_expand``,
include/afcm_hip.h; kernel in csrc/group.hip).  It hands the encoder state of G conditioning images to a decoder batch of B samples
(``SynthesisNetwork.decode(groups=...)``): ``groups`` is an int32 DEVICE tensor [B] that the kernel reads when it runs, nothing is read back.

A block is what lies between two samples of the tensor as allocated.  A dense tensor's block is its ``numel / G`` elements; a row-pitched view made by
``_rows.empty`` is copied with its padding (C * H * pitch elements), its output comes from ``_rows.empty`` again and has the same pitch, so the fused
layer kernels read it in place and its padding is as finite as the producer left the source's.  Any other layout is made contiguous first.
An index outside [0, G) cannot be raised from the device: every element of that sample's block, in every output, is NaN.

``GroupExpand`` is the plan for fixed sources: outputs and the device table are made once, outside any stream capture; ``run(groups)`` is the one
launch, allocates nothing and can be captured.  ``group_expand(tensors, groups)`` builds a plan and runs it.
"""
import torch

from ... import _lib
from . import _rows

_KINDS = {2: _lib.GROUP_2B, 4: _lib.GROUP_4B}


def _check_groups(groups, device, what):
    if not isinstance(groups, torch.Tensor) or groups.dtype != torch.int32 or groups.ndim != 1 or groups.numel() < 1:
        got = f'{groups.dtype} {tuple(groups.shape)}' if isinstance(groups, torch.Tensor) else type(groups).__name__
        raise RuntimeError(f'{what}: groups must be an int32 tensor [B] with B >= 1, got {got}')
    if groups.device != device:
        raise RuntimeError(f'{what}: groups are on {groups.device}, the tensors on {device}: every tensor must be on one device')
    _lib.require_gpu(groups)
    if not groups.is_contiguous():
        raise RuntimeError(f'{what}: groups must be contiguous')


def _layout(t):
    """(the tensor the kernel addresses, elements per block, pitched or not) of one source [G, ...]."""
    if t.ndim == 4 and not t.is_contiguous() and _rows.ENABLED and _rows.whole_buffer(t) is not None:
        ld = _rows.pitch_of(t)
        if ld == _rows.pitch_for(t.shape[3], t.dtype) and ld != t.shape[3] and t.dtype in (torch.bfloat16, torch.float16):
            return t, t.shape[1] * t.shape[2] * ld, True                       # the layout _rows.empty gives back
    t = t.contiguous()
    return t, t.numel() // t.shape[0], False


class GroupExpand:
    def __init__(self, tensors, batch):
        tensors = list(tensors)
        if not tensors:
            raise RuntimeError('group_expand: nothing to expand (an empty list of tensors)')
        for t in tensors:
            if not isinstance(t, torch.Tensor) or t.ndim < 1 or t.shape[0] < 1 or t.numel() < 1:
                raise RuntimeError('group_expand: every source is a non-empty tensor [G, ...]')
            _lib.dtype_code(t)
        if len({t.device for t in tensors}) != 1:
            raise RuntimeError('group_expand: every tensor must be on one device')
        _lib.require_gpu(*tensors)
        self.batch = int(batch)
        if self.batch < 1:
            raise RuntimeError(f'group_expand: batch {batch} is below 1')
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('group_expand: build the GroupExpand plan before the capture (it allocates and uploads); run() can be captured')
        self.device = tensors[0].device
        chunk = _lib.load().afcm_group_chunk_bytes()
        self.sources, self.outputs, rows, chunks = [], [], [], 0
        for t in tensors:
            src, block, pitched = _layout(t)
            if pitched:
                out = _rows.empty((self.batch,) + tuple(src.shape[1:]), src.dtype, self.device)
            else:
                out = torch.empty((self.batch,) + tuple(src.shape[1:]), dtype=src.dtype, device=self.device)
            size = src.element_size()
            rows.append((out.data_ptr(), src.data_ptr(), block * size, chunks, int(src.shape[0]) | (_KINDS[size] << 32)))
            chunks += self.batch * ((block * size + chunk - 1) // chunk)
            self.sources.append(src)                                           # (kept alive: the table points into them)
            self.outputs.append(out)
        self.host = torch.tensor(rows, dtype=torch.int64).reshape(-1).pin_memory()
        self.table = torch.empty(self.host.numel(), dtype=torch.int64, device=self.device)
        self.table.copy_(self.host, non_blocking=True)
        self.rows = len(rows)

    @torch.no_grad()
    def run(self, groups):
        """One launch on the current stream; returns the outputs (the same tensors at every call)."""
        _check_groups(groups, self.device, 'group_expand')
        if groups.numel() != self.batch:
            raise RuntimeError(f'group_expand: {groups.numel()} group indices for a plan of batch {self.batch}')
        _lib.launched(_lib.load().afcm_group_expand(self.table.data_ptr(), self.host.data_ptr(), self.rows, self.batch, groups.data_ptr(),
                                                    _lib.stream_ptr(self.table)), 'group_expand')
        return self.outputs


def group_expand(tensors, groups):
    """``[in_k[groups] for in_k in tensors]`` as new tensors in the sources' layouts, one launch.  ``tensors``: float32 / float16 / bfloat16 device
    tensors [G_k, ...]; ``groups``: int32 device tensor [B], values in [0, G_k) (a value outside gives NaN blocks)."""
    tensors = list(tensors)
    if not tensors:
        raise RuntimeError('group_expand: nothing to expand (an empty list of tensors)')
    first = tensors[0]
    _check_groups(groups, first.device if isinstance(first, torch.Tensor) else None, 'group_expand')
    return GroupExpand(tensors, groups.numel()).run(groups)
