"""CPU checks around ``afcm_group_expand``: the numpy restatement (tests/group_expand_ref.py) against ``np.take``, the Python op's argument errors
(raised before anything is launched, so they need no GPU), and the entry point's host-side refusals."""
import os

import numpy as np
import pytest
import torch

import group_expand_ref as R


@pytest.fixture(scope='module')
def lib():
    from afcm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


@pytest.mark.parametrize('name', sorted(R.INDEX_CASES))
@pytest.mark.parametrize('dtype', [np.float32, np.float16])
def test_restatement_equals_take(name, dtype):
    G, groups = R.INDEX_CASES[name]
    size = np.dtype(dtype).itemsize
    rng = np.random.default_rng(3)
    for elems in R.BLOCK_ELEMS[size][:4]:
        src = rng.standard_normal((G, elems)).astype(dtype)
        got, invalid = R.expand_bytes(src, elems * size, groups, size)
        g = np.asarray(groups)
        assert np.array_equal(invalid, (g < 0) | (g >= G))
        want = np.take(src, np.where(invalid, 0, g), axis=0)
        values = got.view(dtype).reshape(len(groups), elems)
        assert np.array_equal(values[~invalid], want[~invalid])
        assert np.isnan(values[invalid]).all() and not np.isnan(values[~invalid]).any()


def test_nan_patterns_are_nan_in_every_16bit_type():
    assert np.isnan(np.array([R.NAN_BITS[2]]).view(np.float16)).all()
    assert torch.isnan(torch.tensor([0x7FFF], dtype=torch.int16).view(torch.bfloat16)).all()
    assert np.isnan(np.array([R.NAN_BITS[4]]).view(np.float32)).all()


def test_chunk_layout():
    firsts, total = R.chunks([4, 16384, 16386], 3, 16384)
    assert firsts == [0, 3, 6] and total == 12


def test_python_op_argument_errors(lib):
    from afcm_amd.torch_utils.ops.group_ops import GroupExpand, group_expand
    x = torch.zeros(2, 3, 4)
    g = torch.zeros(5, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='no CPU'):                        # host tensors
        group_expand([x], g)
    with pytest.raises(RuntimeError, match='no CPU'):
        GroupExpand([x], 5)
    with pytest.raises(RuntimeError, match='empty list'):
        group_expand([], g)
    with pytest.raises(RuntimeError, match='empty list'):
        GroupExpand([], 5)
    for bad in (g.to(torch.int64), g.to(torch.float32), g.reshape(5, 1), g[:0], [0, 0]):
        with pytest.raises(RuntimeError, match=r'groups must be an int32 tensor \[B\]'):
            group_expand([x], bad)
    with pytest.raises(RuntimeError, match='one device'):                    # groups somewhere else than the tensors
        group_expand([x], torch.zeros(5, dtype=torch.int32, device='meta'))
    with pytest.raises(RuntimeError, match='one device'):
        GroupExpand([x, torch.zeros(2, 3, device='meta')], 5)
    with pytest.raises(RuntimeError, match='float32/float16/bfloat16'):
        GroupExpand([x.to(torch.float64)], 5)
    with pytest.raises(RuntimeError, match='non-empty'):
        GroupExpand([torch.zeros(0, 3)], 5)


def test_entry_point_refusals(lib):
    """AFCM_E_INVALID before any launch: null pointers, an empty table, B < 1, a block size of 0 or no multiple of the element size, an unknown kind,
    a first chunk that is not the running total, more than 2^31 - 1 workgroups."""
    from afcm_amd import _lib
    chunk = lib.afcm_group_chunk_bytes()
    assert chunk == 16384

    def call(rows, n=None, batch=2, table=True, groups=True):
        t = np.array(rows, dtype=np.int64).reshape(-1)
        p = t.ctypes.data
        return lib.afcm_group_expand(p if table else None, p, len(rows) if n is None else n, batch, p if groups else None, None)

    row = lambda dst=64, src=128, bb=8, c0=0, G=2, kind=4: (dst, src, bb, c0, G | (kind << 32))
    cases = ((dict(rows=[row()], table=False), b'empty table'), (dict(rows=[row()], n=0), b'empty table'), (dict(rows=[row()], groups=False), b'null groups'),
             (dict(rows=[row()], batch=0), b'below 1'), (dict(rows=[row(dst=0)]), b'null source or destination'), (dict(rows=[row(src=0)]), b'null source'),
             (dict(rows=[row(bb=0)]), b'empty or no multiple'), (dict(rows=[row(bb=6)]), b'no multiple of 4'),
             (dict(rows=[row(bb=7, kind=2)]), b'no multiple of 2'), (dict(rows=[row(kind=3)]), b'kind 3'), (dict(rows=[row(G=0)]), b'0 groups'),
             (dict(rows=[row(), row(c0=1)]), b'starts at chunk 1'), (dict(rows=[row(bb=chunk * (1 << 30))]), b'exceed the grid'),
             (dict(rows=[row(bb=chunk * (1 << 29)), row(bb=chunk * (1 << 29), c0=1 << 30)]), b'exceed the grid'))
    for kw, word in cases:
        rc = call(**kw)
        assert rc == _lib.E_INVALID and word in lib.afcm_last_error(), (kw, rc, lib.afcm_last_error())
