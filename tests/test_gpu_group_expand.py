"""``afcm_group_expand`` on the GPU against its numpy restatement (tests/group_expand_ref.py), bit for bit: the raw bytes of every output as
allocated -- the padding of row-pitched tensors included -- equal the restatement's; blocks of an invalid index are compared by ``isnan``.  The
cases are those of group_expand_ref: block sizes below, at and above one 16-byte access with a tail and across a workgroup's chunk, the three
dtypes, a source off the 16-byte grid, a row-pitched tensor next to dense ones in one launch, G = 1, G > B, repeats, indices -1 and G in the
first and the last sample, and a captured launch replayed after ``groups`` was overwritten."""
import numpy as np
import pytest
import torch

import group_expand_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _raw(t):
    """The bytes of ``t`` as allocated (a row-pitched view: its whole [N, C, H, pitch] buffer), uint8 numpy [N, bytes per sample]."""
    from afcm_amd.torch_utils.ops import _rows
    buf = t if t.is_contiguous() else _rows.whole_buffer(t)
    assert buf is not None and buf.is_contiguous()
    return buf.reshape(buf.shape[0], -1).view(torch.uint8).cpu().numpy()


def _values(raw, dtype):
    t = torch.from_numpy(raw.copy())
    return t.view(dtype).float().numpy()


def _check(out, src, groups, dtype):
    size = torch.empty([], dtype=dtype).element_size()
    src_raw = _raw(src)
    want, invalid = R.expand_bytes(src_raw, src_raw.shape[1], groups, size)
    got = _raw(out)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got[~invalid], want[~invalid])
    if invalid.any():
        assert np.isnan(_values(got[invalid], dtype)).all()
    assert not np.isnan(_values(got[~invalid], dtype)).any()


def _source(G, elems, dtype, seed, offset=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    flat = torch.randn(G * elems + offset, generator=g, device='cuda').to(dtype)
    return flat[offset:].view(G, elems)


@pytest.mark.parametrize('name', sorted(R.INDEX_CASES))
@pytest.mark.parametrize('dtype', DTYPES)
def test_blocks_equal_the_restatement(name, dtype):
    from afcm_amd.torch_utils.ops.group_ops import group_expand
    G, groups = R.INDEX_CASES[name]
    gdev = torch.tensor(groups, dtype=torch.int32, device='cuda')
    size = torch.empty([], dtype=dtype).element_size()
    for k, elems in enumerate(R.BLOCK_ELEMS[size]):
        src = _source(G, elems, dtype, seed=10 + k)
        out, = group_expand([src], gdev)
        assert out.shape == (len(groups), elems) and out.dtype == dtype and out.is_contiguous()
        _check(out, src, groups, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
def test_source_off_the_16_byte_grid(dtype):
    """A view that starts one element into its allocation: no block of the source starts on a 16-byte boundary."""
    from afcm_amd.torch_utils.ops.group_ops import group_expand
    G, groups = R.INDEX_CASES['invalid_first_and_last']
    gdev = torch.tensor(groups, dtype=torch.int32, device='cuda')
    size = torch.empty([], dtype=dtype).element_size()
    for k, elems in enumerate(R.BLOCK_ELEMS[size]):
        src = _source(G, elems, dtype, seed=20 + k, offset=1)
        assert src.is_contiguous() and src.data_ptr() % 16 == size
        out, = group_expand([src], gdev)
        _check(out, src, groups, dtype)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_pitched_and_dense_tensors_in_one_launch(dtype):
    """Three tensors of different block sizes, one of them a row-pitched [G, C, H, W] view from ``_rows.empty``: its output has the same pitch and
    the same padding bytes; a strided view of another form is made contiguous."""
    from afcm_amd.torch_utils.ops import _rows
    from afcm_amd.torch_utils.ops.group_ops import group_expand
    G, groups = R.INDEX_CASES['non_monotone_repeats']
    gdev = torch.tensor(groups, dtype=torch.int32, device='cuda')
    pitched = _rows.empty([G, 3, 5, 276], dtype, 'cuda')
    assert _rows.pitch_of(pitched) == 288 and not pitched.is_contiguous()
    _rows.whole_buffer(pitched).copy_(_source(G, 3 * 5 * 288, dtype, seed=31).view(G, 3, 5, 288))      # the padding holds values of its own
    dense = _source(G, 2 * 7 * 36, dtype, seed=32).view(G, 2, 7, 36)
    vector = _source(G, 1024, torch.float32, seed=33)
    other = _source(G, 2 * 6 * 40, dtype, seed=34).view(G, 2, 6, 40)[..., ::2]           # neither dense nor row-pitched
    assert _rows.pitch_of(other) is None
    outs = group_expand([pitched, dense, vector, other], gdev)
    assert _rows.pitch_of(outs[0]) == 288 and not outs[0].is_contiguous() and outs[0].shape == (len(groups), 3, 5, 276)
    _check(outs[0], pitched, groups, dtype)
    _check(outs[1], dense, groups, dtype)
    _check(outs[2], vector, groups, torch.float32)
    assert outs[3].is_contiguous() and outs[3].shape == (len(groups), 2, 6, 20)
    _check(outs[3], other.contiguous(), groups, dtype)
    with_invalid = torch.tensor([G, 0, -1], dtype=torch.int32, device='cuda')
    outs = group_expand([pitched, vector], with_invalid)
    _check(outs[0], pitched, [G, 0, -1], dtype)                              # the padding of a NaN block is NaN too
    _check(outs[1], vector, [G, 0, -1], torch.float32)


def test_captured_launch_reads_groups_at_replay():
    from afcm_amd.torch_utils.ops.group_ops import GroupExpand, group_expand
    G, first = R.INDEX_CASES['non_monotone_repeats']
    second = [1, 1, 2, 0, 3, -1, 0, 2]
    a, b = _source(G, 8 * 1024 + 27, torch.float16, seed=41), _source(G, 21, torch.float32, seed=42)
    groups = torch.tensor(first, dtype=torch.int32, device='cuda')
    plan = GroupExpand([a, b], len(first))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan.run(groups)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = plan.run(groups)
    groups.copy_(torch.tensor(second, dtype=torch.int32, device='cuda'))      # in place: the graph holds the pointer
    for o in outs:
        o.zero_()
    graph.replay()
    eager = group_expand([a, b], torch.tensor(second, dtype=torch.int32, device='cuda'))
    for o, e, src, dtype in zip(outs, eager, (a, b), (torch.float16, torch.float32)):
        _check(o, src, second, dtype)
        assert np.array_equal(_raw(o), _raw(e))
