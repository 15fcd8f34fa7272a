"""The per-plane passes of a fused layer's backward (afcm_amd/csrc/conv2d_planes.hip: scale_planes, axpy_planes, plane_dot -- dense, wave,
row-pitched, gated --, amax_bits, split16, unscale; modulation.hip: layer_bwd_coefs) against the restatements of tests/plane_passes_ref.py at
the edges of each kernel: rows of exactly one 16-byte vector, ragged rows, the plane where the row reciprocal needs its fix-up, every rung of the
load ladders, launches beyond their block caps, misaligned bases, NULL-pointer modes.  tests/test_plane_passes_ref_cpu.py checks the restatements
and, in integers, that each shape here hits what it is here for.  fp32-accumulated results are held to the project's bars against float64
(1e-5 of the sum of the terms' magnitudes), elementwise passes bit for bit.  The C ABI is called directly wherever the Python wrapper would copy
the case or route it to another kernel."""
import pytest
import torch

import plane_passes_ref as P

pytestmark = pytest.mark.gpu

BF16, F16, F32 = P.BF16, P.F16, P.F32
CANARY = 12288.0                   # (a bfloat16 and a float16 number)


def _lib():
    from afcm_amd import _lib
    return _lib, _lib.load(), torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _within(got, want, bar):
    assert got.dtype == F32 and got.shape == want.shape
    err = (got.double() - want).abs()
    assert bool((err <= bar).all()), (float(err.max()), float(bar.min()), got.flatten()[:4].tolist(), want.flatten()[:4].tolist())


# ---- plane_dot_rows through conv.plane_dot on pitched views ---------------------------------------------------------------------------------
def _check_rows(a, b, lda, ldb):
    from afcm_amd.torch_utils.ops import _rows
    from afcm_amd.torch_utils.ops import conv2d as conv
    pa, pb = P.pitched(a, lda), P.pitched(b, ldb)
    assert _rows.pitch_of(pa) == lda and _rows.pitch_of(pb) == ldb and not pa.is_contiguous()      # read in place by afcm_plane_dot_ld
    want, bar = P.plane_dot(a, b)
    for x, y in ((pa, pb), (pa, b), (b, pa)):
        _within(conv.plane_dot(x, y), want, bar)
    _within(conv.plane_dot(pa), *P.plane_dot(a))


@pytest.mark.parametrize('dtype, planes, h, w', P.ROW_CASES, ids=str)
def test_plane_dot_rows(dtype, planes, h, w):
    a, b = (t.cuda() for t in P.row_operands(dtype, planes, h, w))
    _check_rows(a, b, *P.row_pitches(w))


def test_plane_dot_rows_where_the_reciprocal_needs_its_fix_up():
    """One fp32 plane of 258 rows x 4092 vectors behind a pitch: the round-up reciprocal alone puts the last vector of rows 256 and 257 at
    column -4 of the next row -- the previous row's padding, NaN here.  Before the fix-up in plane_dot_rows_kernel: NaN."""
    from afcm_amd.torch_utils.ops import conv2d as conv
    dtype, planes, h, w, ld = P.ROW_BIG
    a, b = P.data((1, 1, h, w), dtype, 5).cuda(), P.data((1, 1, h, w), dtype, 6).cuda()
    pa, pb = P.pitched(a, ld), P.pitched(b, ld)
    _within(conv.plane_dot(pa, pb), *P.plane_dot(a, b))
    _within(conv.plane_dot(pa), *P.plane_dot(a))


# ---- afcm_plane_dot_gated_ld ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', P.GATED_MODES)
@pytest.mark.parametrize('dtype, h, w', P.GATED_SHAPES, ids=str)
def test_plane_dot_gated(dtype, h, w, mode):
    """8 planes in one launch, unflagged / flagged in the last of 3 slots / unflagged but cancelling, mixed within a workgroup's four waves:
    the flagged and the cancelling planes equal afcm_plane_dot_ld bit for bit, the others osc * (gz - nsc * gsk) in fp32."""
    L, lib, st = _lib()
    lda, ldb = P.row_pitches(w)
    a, b = P.data((1, 8, h, w), dtype, 41).cuda(), P.data((1, 8, h, w), dtype, 42).cuda()
    pa, pb = P.pitched(a, lda), P.pitched(b, ldb)
    host = P.gated_inputs(mode)
    real, closed = P.gate_real(host[0], *host[2:]).cuda(), P.gate_closed_form(*host[1:]).cuda()
    flags, osc, gz, nsc, gsk = (None if t is None else t.cuda() for t in host)
    code = L._DTYPES[dtype]
    plain = torch.full([8], CANARY, device='cuda')
    L.launched(lib.afcm_plane_dot_ld(plain.data_ptr(), pa.data_ptr(), pb.data_ptr(), code, 8, h, w, lda, ldb, st), 'plane_dot_ld')
    _within(plain.view(1, 8), *P.plane_dot(a, b))
    got = torch.full([8 + 4], CANARY, device='cuda')
    L.launched(lib.afcm_plane_dot_gated_ld(got.data_ptr(), pa.data_ptr(), pb.data_ptr(), code, 8, h, w, lda, ldb, flags.data_ptr(), P.GATED_SLOTS,
                                           osc.data_ptr(), gz.data_ptr(), _ptr(nsc), _ptr(gsk), st), 'plane_dot_gated_ld')
    assert real.any() and not real.all() and (got[8:] == CANARY).all()
    assert torch.equal(P.bits(got[:8][real]), P.bits(plain[real]))
    assert torch.equal(P.bits(got[:8][~real]), P.bits(closed[~real]))
    assert not torch.equal(got[:8][~real], plain[~real])                    # (the two readings of a plane differ: the test can tell them apart)


# ---- dense plane_dot --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype, hw', P.DENSE_CASES, ids=str)
def test_plane_dot_dense(dtype, hw):
    from afcm_amd.torch_utils.ops import conv2d as conv
    n, c = P.DENSE_NC
    a, b = P.data((n, c, 1, hw), dtype, 51).cuda(), P.data((n, c, 1, hw), dtype, 52).cuda()
    assert a.is_contiguous() and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0        # afcm_plane_dot on the tensors themselves
    _within(conv.plane_dot(a, b), *P.plane_dot(a, b))
    _within(conv.plane_dot(a), *P.plane_dot(a))


# ---- scale_planes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt_in, dt_out', P.SCALE_PAIRS, ids=str)
def test_scale_planes_values(dt_in, dt_out):
    """All seven dtype pairs, bit-equal to the fp32 product rounded to nearest even, NaN / inf / overflow / -0 carried through: the scalar path
    (hw in 1, 2, 3, 7), the vector path (8, 60), no scale, and a launch of 2113 workgroups' worth of work on 2048."""
    from afcm_amd.torch_utils.ops import conv2d as conv
    for shape in P.SCALE_SHAPES + [P.SCALE_BIG]:
        x = P.scale_input(shape, dt_in).cuda()
        for scale in (P.plane_scale(*shape[:2]).cuda(), None):
            got = conv.scale_planes(x, scale, dt_out)
            assert got.is_contiguous() and P.same_values(got, P.scale_planes(x, scale, dt_out)), (shape, scale is None)


@pytest.mark.parametrize('dtype', P.DTYPES, ids=str)
def test_scale_planes_pitched_view_keeps_its_pitch_and_its_values(dtype):
    from afcm_amd.torch_utils.ops import _rows
    from afcm_amd.torch_utils.ops import conv2d as conv
    x = P.scale_input((2, 3, 6, 10), dtype).cuda()
    scale = P.plane_scale(2, 3).cuda()
    px = P.pitched(x, 16)
    got = conv.scale_planes(px, scale)
    assert _rows.pitch_of(got) == 16 and not got.is_contiguous() and got.shape == x.shape
    assert P.same_values(got.contiguous(), P.scale_planes(x, scale, dtype))


@pytest.mark.parametrize('dt_in, dt_out', P.SCALE_PAIRS, ids=str)
def test_scale_planes_bases_off_the_vector_boundary(dt_in, dt_out):
    """hw % 4 == 0 with x, y or both one element past a vector boundary: the kernel takes its scalar path (it looks at the pointers), same values."""
    L, lib, st = _lib()
    n, c, h, w = 2, 3, 6, 10
    x = P.scale_input((n, c, h, w), dt_in).cuda()
    scale = P.plane_scale(n, c).cuda()
    want = P.scale_planes(x, scale, dt_out)
    from afcm_amd.torch_utils.ops import conv2d as conv
    xo = torch.empty(x.numel() + 1, dtype=dt_in, device='cuda')[1:].view(x.shape).copy_(x)
    assert xo.is_contiguous() and xo.data_ptr() % (4 * x.element_size()) == x.element_size()
    assert P.same_values(conv.scale_planes(xo, scale, dt_out), want)                       # the wrapper keeps a contiguous view where it is
    for x_off, y_off in ((0, 1), (1, 1), (1, 0), (0, 0)):
        xs = torch.empty(x.numel() + 1, dtype=dt_in, device='cuda')[x_off:x_off + x.numel()].copy_(x.view(-1))
        ybuf = torch.full([x.numel() + 2], CANARY, dtype=dt_out, device='cuda')
        y = ybuf[y_off:y_off + x.numel()]
        L.launched(lib.afcm_scale_planes(y.data_ptr(), xs.data_ptr(), scale.data_ptr(), L._DTYPES[dt_in], L._DTYPES[dt_out], n * c, h * w, st), 'scale_planes')
        assert P.same_values(y.view(x.shape), want), (x_off, y_off)
        assert (ybuf[:y_off] == CANARY).all() and (ybuf[y_off + x.numel():] == CANARY).all()


def test_scale_planes_refuses_a_pair_it_has_no_kernel_for():
    L, lib, st = _lib()
    x = torch.ones(8, dtype=BF16, device='cuda')
    y = torch.full([8], 3.0, dtype=F16, device='cuda')
    assert lib.afcm_scale_planes(y.data_ptr(), x.data_ptr(), None, L.BF16, L.F16, 2, 4, st) == L.E_INVALID
    assert 'scale_planes: unsupported dtype pair' in lib.afcm_last_error().decode()
    torch.cuda.synchronize()
    assert (y == 3.0).all()


# ---- axpy_planes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [BF16, F16], ids=str)
@pytest.mark.parametrize('planes, hw', P.AXPY_CASES, ids=str)
def test_axpy_planes(planes, hw, dtype):
    """65600 planes on grid.y's 65535 rows; a plane of three grid.x blocks.  One rounding: equal to the fp32 sum rounded, and inside the bound of
    test_skip_fork_backward_is_the_scaled_sum_of_both_arms against float64."""
    L, lib, st = _lib()
    a, b = P.data((1, planes, 1, hw), dtype, 61).cuda(), P.data((1, planes, 1, hw), dtype, 62).cuda()
    sc = P.plane_scale(1, planes).cuda()
    for scale in (sc, None):
        y = torch.full_like(a, CANARY)
        L.launched(lib.afcm_axpy_planes(y.data_ptr(), a.data_ptr(), b.data_ptr(), _ptr(scale), L._DTYPES[dtype], planes, hw, st), 'axpy_planes')
        want = a.double() + b.double() * (1.0 if scale is None else scale.double()[:, :, None, None])
        assert float((y.double() - want).abs().max()) <= float(want.abs().max()) * 2.0 ** (-7 if dtype == BF16 else -10)
        assert P.same_values(y, P.axpy_planes(a, b, scale))


@pytest.mark.parametrize('dtype', [BF16, F16], ids=str)
def test_axpy_planes_declines_what_it_has_no_vectors_for(dtype):
    L, lib, st = _lib()
    code = L._DTYPES[dtype]
    flat = [torch.full([3 * 16 + 8], 2.0, dtype=dtype, device='cuda') for _ in range(3)]
    y, a, b = flat
    assert lib.afcm_axpy_planes(y.data_ptr(), a.data_ptr(), b.data_ptr(), None, code, 4, 12, st) == L.E_NOKERNEL           # hw % 8 != 0
    for off in ((1, 0, 0), (0, 1, 0), (0, 0, 4)):                                                                            # one base off its 16 bytes
        ptrs = [t[o:].data_ptr() for t, o in zip(flat, off)]
        assert lib.afcm_axpy_planes(*ptrs, None, code, 3, 16, st) == L.E_NOKERNEL
    torch.cuda.synchronize()
    assert (y == 2.0).all()
    assert lib.afcm_axpy_planes(y.data_ptr(), a.data_ptr(), b.data_ptr(), None, code, 3, 16, st) == 0
    assert (y[:48] == 4.0).all() and (y[48:] == 2.0).all()


# ---- unscale --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bounds', P.UNSCALE_BOUNDS, ids=str)
def test_unscale(bounds):
    L, lib, st = _lib()
    words = [None if v is None else P.bound_word(v).cuda() for v in bounds]
    for numel in P.UNSCALE_NUMELS:
        x = P.data([numel], F32, numel).cuda()
        buf = torch.full([numel + 4], CANARY, device='cuda')
        buf[:numel] = x
        L.launched(lib.afcm_unscale(buf.data_ptr(), numel, _ptr(words[0]), _ptr(words[1]), st), 'unscale')
        assert torch.equal(P.bits(buf[:numel]), P.bits(P.unscale(x, *words))) and (buf[numel:] == CANARY).all(), numel


# ---- grid-stride loops behind a block cap: split16, amax_bits --------------------------------------------------------------------------------
def test_split16_past_its_block_cap():
    from afcm_amd.torch_utils.ops import conv2d as conv
    x = P.data(P.SPLIT_BIG, F32, 71).cuda()
    scale = P.plane_scale(*P.SPLIT_BIG[:2]).cuda()
    v = x * scale[:, :, None, None]                                                          # fl32(x * scale)
    parts = conv.split16(x, scale, 3, BF16)
    assert parts.shape == (3, *P.SPLIT_BIG) and torch.equal(parts.double().sum(0), v.double())      # three bfloat16 parts carry all 24 bits
    del parts
    word = conv.amax_bits(x, scale)
    assert word.view(F32).item() == float(v.abs().max())
    gs = conv.pow2_factor(word)
    parts = conv.split16(x, scale, 2, F16, word)
    assert bool(torch.isfinite(parts.float()).all())
    gv = v.double() * gs
    err = (parts.double().sum(0) - gv).abs()
    big = gv.abs() >= 2.0 ** -3
    assert float((err[big] / gv.abs()[big]).max()) <= 2.0 ** -22 and float(err[~big].max()) <= 2.0 ** -25      # (test_split16_parts_sum_back...)


def test_amax_bits_past_its_block_cap_and_on_its_scalar_path():
    from afcm_amd.torch_utils.ops import conv2d as conv
    x = P.data((1, 1, P.AMAX_BIG, P.AMAX_BIG), F32, 81).cuda()
    flat = x.view(-1)
    assert float(flat.abs().max()) < 50.0
    for at, v in ((flat.numel() - 2, -77.0), (1, 99.0)):                                     # the last 16-byte group, then the first
        flat[at] = v
        assert conv.amax_bits(x).view(F32).item() == abs(v) == float(flat.abs().max())
    # 4-byte aligned but off the 16-byte boundary (hw % 4 == 0), and hw % 4 != 0: the scalar path, with and without per-plane factors
    base = P.data([2 * 3 * 8 * 10 + 1], F32, 82).cuda()
    off = base[1:].view(2, 3, 8, 10)
    odd = P.data((3, 5, 7, 9), F32, 83).cuda()
    assert off.is_contiguous() and off.data_ptr() % 16 == 4 and odd.data_ptr() % 16 == 0
    for t in (off, odd):
        assert not P.amax_vector_path(t.shape[2] * t.shape[3], t.data_ptr() % 16)
        sc = P.plane_scale(*t.shape[:2]).cuda() * 3
        assert conv.amax_bits(t).view(F32).item() == float(t.abs().max())
        assert conv.amax_bits(t, sc).view(F32).item() == float((t * sc[:, :, None, None]).abs().max())


# ---- afcm_layer_bwd_coefs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n, o, slots', P.COEF_CASES, ids=str)
def test_layer_bwd_coefs(n, o, slots):
    """N up to 130 on 64 lanes (the loop), slot sums, the NULL-pointer modes; an output that is not asked for is not written, nor is anything
    behind one that is."""
    L, lib, st = _lib()
    psum, osc, nsc, bias, gz, dysy = (t.cuda() for t in P.coef_inputs(n, o, slots))

    def run(want_db, want_next, want_out, osc=osc, nsc=nsc, bias=bias, gz=gz, dysy=dysy):
        bufs = {'db': torch.full([o + 8], CANARY, device='cuda'), 'd_next': torch.full([n * o + 8], CANARY, device='cuda'),
                'd_out': torch.full([n * o + 8], CANARY, device='cuda')}
        asked = {'db': want_db, 'd_next': want_next, 'd_out': want_out}
        L.launched(lib.afcm_layer_bwd_coefs(*[bufs[k].data_ptr() if asked[k] else None for k in ('db', 'd_next', 'd_out')], psum.data_ptr(), slots,
                                            _ptr(osc), _ptr(nsc), _ptr(bias), _ptr(gz), _ptr(dysy), n, o, st), 'layer_bwd_coefs')
        ref = P.layer_bwd_coefs(psum, osc, nsc, bias, gz, dysy)
        for k, buf in bufs.items():
            size = o if k == 'db' else n * o
            assert (buf[size:] == CANARY).all(), k
            if asked[k]:
                _within(buf[:size].view(ref[k][0].shape), *ref[k])
            else:
                assert (buf == CANARY).all(), k
        return bufs

    run(True, True, True)
    run(True, False, False, osc=None, nsc=None, bias=None, gz=None, dysy=None)              # db alone, d = 1
    nxt = run(False, True, False, osc=None, bias=None, dysy=None)['d_next'][:n * o]
    assert (nsc == 0).any() and bool((nxt[nsc.view(-1) == 0] == 0).all())                    # exactly 0 where s_next == 0
    run(False, False, True, nsc=None, bias=None, gz=None)                                    # d_out without a bias


def test_layer_bwd_coefs_refuses_outputs_without_their_inputs():
    L, lib, st = _lib()
    psum, osc, nsc, bias, gz, dysy = (t.cuda() for t in P.coef_inputs(2, 5, 3))
    out = torch.full([10], CANARY, device='cuda')
    p = lambda t: t.data_ptr()
    for args in ((None, p(out), None, p(psum), 3, p(osc), p(nsc), p(bias), None, p(dysy)),         # d_next without <g, z>
                 (None, p(out), None, p(psum), 3, p(osc), None, p(bias), p(gz), p(dysy)),          # d_next without next_scale
                 (None, None, p(out), p(psum), 3, p(osc), p(nsc), p(bias), p(gz), None),           # d_out without <dys, y>
                 (None, None, p(out), p(psum), 3, None, p(nsc), p(bias), p(gz), p(dysy))):         # d_out without out_scale
        assert lib.afcm_layer_bwd_coefs(*args, 2, 5, st) == L.E_INVALID
        assert 'layer_bwd_coefs' in lib.afcm_last_error().decode()
    torch.cuda.synchronize()
    assert (out == CANARY).all()
