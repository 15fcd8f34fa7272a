"""The re-layouts and the pointer audit of view_layouts.py, without a GPU and without the library."""
import ctypes
import types

import pytest
import torch

import view_layouts as V

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
SHAPES = [(2, 3, 4, 6), (2, 5, 3, 7), (1, 4, 2, 2), (3, 8), (5,)]


def _values(shape, dtype):
    g = torch.Generator().manual_seed(len(shape) * 100 + shape[-1])
    return torch.randint(-8, 9, shape, generator=g).to(dtype)


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_every_variant_equals_the_original_and_has_the_layout_it_claims(shape, dtype):
    t = _values(shape, dtype)
    got = dict(V.variants(t))
    want = {'aligned', 'offset1', 'offset2'} | ({'channels_last'} if len(shape) == 4 else set()) | ({'channel_slice', 'row_slice'} if len(shape) >= 2 else set())
    assert set(got) == want
    for name, v in got.items():
        assert v.shape == t.shape and v.dtype == t.dtype and torch.equal(v, t), name
        V.check_claim(name, v)
        assert v.untyped_storage().data_ptr() != t.untyped_storage().data_ptr(), f'{name} shares the original\'s storage'
    e = t.element_size()
    # the residues the kernels care about: one 16-bit element in is 2 past a dword, one fp32 element 4 past a 16-byte vector
    assert got['offset1'].data_ptr() % 4 == (2 if e == 2 else 0) and got['offset1'].data_ptr() % 16 == e
    assert got['offset2'].data_ptr() % 4 == 0 and got['offset2'].data_ptr() % 16 == 2 * e
    if len(shape) >= 2 and shape[0] > 1:
        assert not got['channel_slice'].is_contiguous() and not got['row_slice'].is_contiguous()
    assert V.variant(t, 'offset1').data_ptr() % 16 == e
    with pytest.raises(KeyError):
        V.variant(t, 'expanded')


def test_expanded_cotangent_variant():
    pc = _values((2, 3, 1, 1), torch.float16)
    t = pc.expand(2, 3, 4, 6).contiguous()
    got = dict(V.variants(t, cotangent=True))
    v = got['expanded']
    assert torch.equal(v, t) and v.stride() == (3, 1, 0, 0)
    V.check_claim('expanded', v)
    # a cotangent that is not constant on its planes has no such form
    assert 'expanded' not in dict(V.variants(_values((2, 3, 4, 6), torch.float16), cotangent=True))
    assert 'expanded' not in dict(V.variants(t))


def test_row_slice_stride_is_no_row_pitch():
    from afcm_amd.torch_utils.ops import _rows
    for w in (6, 7, 14, 64):
        t = _values((2, 3, 4, w), torch.bfloat16)
        v = V.variant(t, 'row_slice')
        assert v.stride(2) not in (w, _rows.pitch_for(w, t.dtype)) and v.stride(2) % 2 == 1
        assert _rows.pitch_of(v) is None


def _is_pointer(argtype):
    return argtype is ctypes.c_void_p or (isinstance(argtype, type) and issubclass(argtype, ctypes._Pointer))


def test_audit_table_matches_the_bindings():
    from afcm_amd import _lib
    for name, entry in V.PRECONDITIONS.items():
        assert name in _lib.SIGNATURES, name
        argtypes = _lib.SIGNATURES[name][1]
        for p in entry.ptrs:
            assert p.cite and 0 <= p.arg < len(argtypes) and _is_pointer(argtypes[p.arg]), (name, p.name)
            if p.field is None:
                assert argtypes[p.arg] is ctypes.c_void_p, (name, p.name)
            else:
                struct = argtypes[p.arg]._type_
                assert dict(struct._fields_)[p.field] is ctypes.c_void_p, (name, p.name, p.field)
            need = [p.align(c) for c in V.ESIZE] if callable(p.align) else [p.align]
            assert all(a in (2, 4, 8, 16, 32) for a in need), (name, p.name, need)
            if callable(p.align):
                arg, field = p.dt or entry.dtype
                code_type = argtypes[arg] if field is None else dict(argtypes[arg]._type_._fields_)[field]
                assert code_type is ctypes.c_int32, (name, p.name)
        if entry.count is not None:
            assert argtypes[entry.count] is ctypes.c_int32
        assert len({p.name for p in entry.ptrs}) == len(entry.ptrs)
    # the values the host code requires (AFCM_REQUIRE) or the kernels' comments state
    align = {(n, p.name): p.align for n, e in V.PRECONDITIONS.items() for p in e.ptrs}
    assert align['afcm_split16', 'x'] == 16 and align['afcm_plane_dot_parts', 'b'] == 16 and align['afcm_plane_dot', 'a'] == 16
    assert align['afcm_fc_act_fwd', 'x'] == 16 and align['afcm_fc_act_bwd', 'gy'] == 16
    for n, k in (('afcm_conv2d_ld', 'x'), ('afcm_conv2d_split', 'x_parts'), ('afcm_conv2d_stride2', 'x'), ('afcm_conv2d_wgrad_ld', 'x'),
                 ('afcm_conv2d_wgrad_ld', 'dy'), ('afcm_conv2d_wgrad_dots_ld', 'dy'), ('afcm_filtered_lrelu', 'x'), ('afcm_filtered_lrelu', 'skip')):
        assert align[n, k] == 4, (n, k)


def test_audit_refuses_before_forwarding_and_records_what_it_forwards(monkeypatch):
    seen, status = [], [-1]
    stub = types.SimpleNamespace(afcm_split16=lambda *a: seen.append(a) or 0, afcm_conv2d_ld=lambda *a: seen.append(a) or status[0])
    calls = V.audit(stub, monkeypatch, names=['afcm_split16', 'afcm_conv2d_ld'])
    ok = (0x1000, 0x2000, None, 0x3004, V.F16, 6, 24, 2, 144, None)
    assert stub.afcm_split16(*ok) == 0 and calls == ['afcm_split16'] and seen == [ok]
    with pytest.raises(AssertionError, match=r'afcm_split16: x = 0x2004 is not 16-byte aligned \(4 past\)'):
        stub.afcm_split16(0x1000, 0x2004, None, 0x3004, V.F16, 6, 24, 2, 144, None)
    with pytest.raises(AssertionError, match='afcm_split16: parts = 0x1004 is not 8-byte aligned'):
        stub.afcm_split16(ctypes.c_void_p(0x1004), 0x2000, None, None, V.F16, 6, 24, 2, 144, None)
    assert calls == ['afcm_split16'] and len(seen) == 1, 'a refused call was forwarded'
    # a 16-bit image 2 bytes past a dword; the same address is fine nowhere, whatever the dtype
    conv = [0x1000, 0x2002, 0x3000, None, None, V.BF16] + [1] * 10 + [None]
    with pytest.raises(AssertionError, match='afcm_conv2d_ld: x = 0x2002 is not 4-byte aligned'):
        stub.afcm_conv2d_ld(*conv)
    conv[1] = 0x2004
    # forwarded, but the entry point declined the shape (AFCM_E_NOKERNEL): nothing was launched, nothing is recorded
    assert stub.afcm_conv2d_ld(*conv) == -1 and len(seen) == 2 and calls == ['afcm_split16']
    status[0] = 0
    assert stub.afcm_conv2d_ld(*conv) == 0 and len(seen) == 3 and calls == ['afcm_split16', 'afcm_conv2d_ld']


def test_audit_reads_struct_fields_struct_arrays_and_per_dtype_rules(monkeypatch):
    from afcm_amd import _lib
    a = _lib.FilteredLReluArgs()
    a.dtype, a.x, a.b = V.F16, 0x1002, 0x2002
    assert V.violations('afcm_filtered_lrelu', (a, None)) == [('x', 0x1002, 4)]                 # (b: one 16-bit element at a time)
    assert V.violations('afcm_filtered_lrelu', (ctypes.byref(a), None)) == [('x', 0x1002, 4)]
    assert V.violations('afcm_filtered_lrelu', (ctypes.pointer(a), None)) == [('x', 0x1002, 4)]
    a.x, a.skip = 0x1004, 0x3006
    assert V.violations('afcm_filtered_lrelu', (a, None)) == [('skip', 0x3006, 4)]
    table = (_lib.ModulationLayer * 3)()
    table[1].t = 0x4002
    table[2].w = 0x4002                                                                          # beyond the count: not looked at
    assert V.violations('afcm_modulation_bank_fwd', (table, 2, 4, None)) == [('t[1]', 0x4002, 4)]
    # element-aligned operands: 2 bytes past a dword is fine for a 16-bit tensor and refused for an fp32 one
    assert V.violations('afcm_pool_blocks_fwd', (0x1000, 0x2002, V.BF16, 4, 8, 8, None)) == []
    assert V.violations('afcm_pool_blocks_fwd', (0x1000, 0x2002, V.F32, 4, 8, 8, None)) == [('x', 0x2002, 4)]
    # a pointer with its own dtype argument
    assert V.violations('afcm_scale_planes', (0x1002, 0x2002, None, V.F16, V.F32, 4, 16, None)) == [('y', 0x1002, 4)]
    stub = types.SimpleNamespace(afcm_filtered_lrelu=lambda *args: 0)
    calls = V.audit(stub, monkeypatch, names=['afcm_filtered_lrelu'])
    with pytest.raises(AssertionError, match='afcm_filtered_lrelu: skip = 0x3006'):
        stub.afcm_filtered_lrelu(a, None)
    assert calls == []


def test_rows_helpers_move_a_tensor_off_the_grid():
    """The rule of _rows.py on CPU tensors (it reads addresses only): a 16-bit tensor 2 bytes past a dword is copied, anything on the
    grid is handed on as it is."""
    from afcm_amd.torch_utils.ops import _rows
    for dtype in (torch.float16, torch.bfloat16):
        t = _values((2, 3, 4, 6), dtype)
        off1, off2 = V.variant(t, 'offset1'), V.variant(t, 'offset2')
        assert _rows.pitch_of(off1) is None and _rows.pitch_of(off2) == 6 and _rows.pitch_of(t) == 6
        for fn in (_rows.dense, lambda v: _rows.rows(v)[0]):
            moved = fn(off1)
            assert moved.data_ptr() % 64 == 0 and moved.is_contiguous() and torch.equal(moved, t)
            assert fn(off2) is off2 and fn(t) is t
        assert _rows.rows(off1)[1] == 6
        assert _rows.dense(off2, 16).data_ptr() % 16 == 0 and _rows.dense(off2, 16) is not off2
        for name in ('channels_last', 'channel_slice', 'row_slice'):
            moved, ld = _rows.rows(V.variant(t, name))
            assert moved.is_contiguous() and ld == 6 and moved.data_ptr() % 4 == 0 and torch.equal(moved, t)
    f = _values((2, 3, 4, 6), torch.float32)
    off1 = V.variant(f, 'offset1')
    assert _rows.dense(off1) is off1 and _rows.dense(off1, 16).data_ptr() % 16 == 0
    # a pitched view keeps its pitch on the grid and loses it off the grid
    buf = torch.zeros([2 * 3 * 4 * 32 + 8], dtype=torch.bfloat16)
    on = buf[:2 * 3 * 4 * 32].view(2, 3, 4, 32)[..., :6]
    off = buf[1:1 + 2 * 3 * 4 * 32].view(2, 3, 4, 32)[..., :6]
    assert _rows.pitch_of(on) == 32 and _rows.pitch_of(off) is None
    assert _rows.rows(off)[0].is_contiguous() and _rows.rows(off)[0].data_ptr() % 4 == 0
