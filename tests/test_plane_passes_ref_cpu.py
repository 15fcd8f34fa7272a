"""The per-plane passes without a GPU: the float64 / exact restatements of tests/plane_passes_ref.py against hand-computed tiny cases, every
case the GPU file (tests/test_gpu_plane_passes.py) parametrises run on the restatement alone, and -- in pure integer arithmetic -- that the
chosen shapes hit what they claim: the vector counts and loop trips of the dot-product kernels, the launches beyond their block caps, the
shapes at which the row kernel's round-up reciprocal was wrong before its fix-up and is exact with it."""
import numpy as np
import pytest
import torch

import plane_passes_ref as P

BF16, F16, F32 = P.BF16, P.F16, P.F32


# ---- the restatements on hand-computed cases --------------------------------------------------------------------------------------------
def test_plane_dot_by_hand_and_over_a_pitched_buffer():
    a = torch.tensor([[[[1., 2., 3.], [4., 5., 6.]]]])
    b = torch.tensor([[[[1., -1., 2.], [0.5, 0., -2.]]]])
    want, bar = P.plane_dot(a, b)
    assert want.dtype == torch.float64 and want.tolist() == [[1 - 2 + 6 + 2 + 0 - 12]] and bar.tolist() == [[1e-5 * (1 + 2 + 6 + 2 + 0 + 12) + 1e-6]]
    assert P.plane_dot(a)[0].tolist() == [[21.]] and P.plane_dot(a)[1].tolist() == [[1e-5 * 21 + 1e-6]]
    pa, pb = P.pitched(a, 5), P.pitched(b, 8)
    assert pa.stride() == (10, 10, 5, 1) and pb.stride() == (16, 16, 8, 1) and torch.equal(pa, a)
    whole_a, whole_b = pa.as_strided((1, 1, 2, 5), (10, 10, 5, 1)), pb.as_strided((1, 1, 2, 8), (16, 16, 8, 1))
    assert whole_a[..., 3:].isnan().all() and whole_b[..., 3:].isnan().all()
    assert P.plane_dot(whole_a, whole_b[..., :5], w=3)[0].tolist() == [[-5.]]                # only [..., :w] counts
    assert P.plane_dot(whole_a, None, w=3)[0].tolist() == [[21.]]
    assert P.plane_dot(whole_a, None, w=4)[0].isnan().all()                                  # (the padding is NaN: a wrong column shows)


def test_gate_rule_by_hand():
    f = lambda *rows: torch.tensor(rows, dtype=torch.int32)
    t = lambda *v: torch.tensor(v, dtype=F32)
    flags = f([0, 0, 0], [0, 0, 7], [0, 0, 0], [0, 0, 0])
    gz, nsc, gsk, osc = t(8., 8., 8., 8.), t(2., 2., 2., 2.), t(-1., -1., 3.5, 3.), t(0.5, 0.5, 0.5, 0.5)
    # plane 2: 8 |8 - 7| = 8 < 15: cancels.  plane 3: 8 |8 - 6| = 16 > 14: does not.  plane 0: 8 * 10 = 80 > 10.
    assert P.gate_real(flags, gz, nsc, gsk).tolist() == [False, True, True, False]
    assert P.gate_real(flags, gz, None, gsk).tolist() == [False, True, False, False]        # nsc = 1: 8 |8 - 3.5| = 36 > 11.5
    assert P.gate_real(flags, gz, nsc, None).tolist() == [False, True, False, False]        # no skip sum: the cancel test is off
    assert P.gate_real(f([1, 0, 0], [0, 2, 0], [0, 0, 0], [0, 0, 0]), gz).tolist() == [True, True, False, False]     # any slot
    assert P.gate_closed_form(osc, gz, nsc, gsk).tolist() == [5., 5., 0.5, 1.]
    assert P.gate_closed_form(osc, gz, None, gsk).tolist() == [4.5, 4.5, 2.25, 2.5]
    assert P.gate_closed_form(osc, gz, nsc, None).tolist() == [4., 4., 4., 4.]
    # every operation rounds to fp32: 1 - 2^-24 * 1 is 1 - 2^-24 exactly, (1 + 2^-23) * (1 + 2^-23) loses its 2^-46
    one = t(1.0)
    k = t(1.0 + 2.0 ** -23)
    assert P.gate_closed_form(one, one, k, k).item() == 1.0 - np.float32(1.0 + 2.0 ** -22)


def test_gated_planes_stay_a_factor_of_two_from_the_threshold():
    for mode in P.GATED_MODES:
        flags, osc, gz, nsc, gsk = P.gated_inputs(mode)
        assert flags.shape == (8, 3) and (flags[:, :2] == 0).all() and [bool(v) for v in flags[:, 2]] == [k == 'flagged' for k in P.GATED_KINDS]
        assert (nsc is None) == (mode == 'no_next_scale') and (gsk is None) == (mode == 'no_gskip')
        real = P.gate_real(flags, gz, nsc, gsk).tolist()
        want = [k == 'flagged' or (k == 'cancel' and gsk is not None) for k in P.GATED_KINDS]
        assert real == want and {'plain', 'flagged', 'cancel'} == set(P.GATED_KINDS) and len(P.GATED_KINDS) == 8
        if gsk is not None:
            z, k = gz.double(), gsk.double() * (1.0 if nsc is None else nsc.double())
            ratio = 8 * (z - k).abs() / (z.abs() + k.abs())
            assert ((ratio < 0.5) | (ratio > 2.0)).all(), ratio                                # the fp32 comparison cannot flip
        closed = P.gate_closed_form(osc, gz, nsc, gsk)
        assert closed.dtype == F32 and torch.isfinite(closed).all() and (closed != 0).all()


def test_layer_bwd_coefs_by_hand():
    psum = torch.tensor([[[1., 2., 3.]], [[-1., 0.5, 0.]]])                                 # N = 2, O = 1, 3 slots: ps = 6, -0.5
    osc, nsc = torch.tensor([[2.], [0.5]]), torch.tensor([[4.], [0.]])
    bias, gz, dysy = torch.tensor([3.]), torch.tensor([[2.], [9.]]), torch.tensor([[10.], [1.]])
    out = P.layer_bwd_coefs(psum, osc, nsc, bias, gz, dysy)
    assert out['db'][0].tolist() == [6 / 2 - 0.5 / 0.5] and out['db'][1].tolist() == [1e-5 * (6 / 2 + 1.5 / 0.5)]
    assert out['d_next'][0].tolist() == [[0.5], [0.]]                                        # 0 where s_next == 0, exactly
    assert out['d_out'][0].tolist() == [[(10 - 3 * 6) / 4], [(1 + 3 * 0.5) / 0.25]]
    assert out['d_out'][1].tolist() == [[1e-5 * (10 + 3 * 6) / 4], [1e-5 * (1 + 3 * 1.5) / 0.25]]
    only_db = P.layer_bwd_coefs(psum)
    assert sorted(only_db) == ['db'] and only_db['db'][0].tolist() == [5.5]                  # d = 1
    assert P.layer_bwd_coefs(psum, osc, None, None, None, dysy)['d_out'][0].tolist() == [[2.5], [4.]]      # b = 0
    assert sorted(P.layer_bwd_coefs(psum, None, nsc, None, gz)) == ['d_next', 'db']


def test_unscale_by_hand():
    from afcm_amd.torch_utils.ops.conv2d import pow2_factor
    # 3.7 = 0.925 * 2^2: g = 2^13.  1234.5 = 0.6 * 2^11: g = 2^4.  2^-20 = 0.5 * 2^-19: g = 2^34.
    assert [pow2_factor(P.bound_word(v)) for v in (3.7, 1234.5, 2.0 ** -20)] == [2.0 ** 13, 2.0 ** 4, 2.0 ** 34]
    t = torch.tensor([1., -3., 0.1])
    assert torch.equal(P.unscale(t, P.bound_word(3.7), P.bound_word(1234.5)), t * 2.0 ** -17)
    assert torch.equal(P.unscale(t, P.bound_word(3.7)), t * 2.0 ** -13) and torch.equal(P.unscale(t, None, P.bound_word(2.0 ** -20)), t * 2.0 ** -34)
    assert torch.equal(P.unscale(t), t)
    for a, b in P.UNSCALE_BOUNDS:
        for numel in P.UNSCALE_NUMELS:
            x = P.data([numel], F32, numel)
            got = P.unscale(x, None if a is None else P.bound_word(a), None if b is None else P.bound_word(b))
            assert got.dtype == F32 and torch.equal(got.double(), x.double() * (got[0].double() / x[0].double()))     # one power of two, exact


def test_scale_and_axpy_round_once_to_nearest_even():
    x = torch.tensor([[[[1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.0, P.INF, P.NAN, 7e4]]]])
    y = P.scale_planes(x, torch.tensor([[1.0]]), BF16)
    assert y.dtype == BF16 and y.float().tolist()[0][0][0][:4] == [1.0, 1.0 + 2.0 ** -6, -0.0, P.INF] and y[0, 0, 0, 4].isnan()     # ties to even
    assert torch.signbit(y[0, 0, 0, 2]) and P.scale_planes(x, None, F16)[0, 0, 0, 5].isinf()                  # 7e4 overflows float16
    z = P.scale_planes(x, torch.tensor([[-3.0]]), F32)
    assert z[0, 0, 0, 0].item() == np.float32(-3.0) * np.float32(1.0 + 2.0 ** -8) and z[0, 0, 0, 3].item() == -P.INF and not torch.signbit(z[0, 0, 0, 2])
    # the product is formed in fp32 from the 16-bit input, then rounded once
    h = torch.tensor([[[[1.0 + 2.0 ** -7]]]]).to(BF16)
    assert P.scale_planes(h, torch.tensor([[1.0 + 2.0 ** -7]]), F32).item() == np.float32((1.0 + 2.0 ** -7) ** 2)
    assert P.scale_planes(h, torch.tensor([[1.0 + 2.0 ** -7]]), BF16).float().item() == 1.0 + 2.0 ** -6             # 1 + 2^-6 + 2^-14 rounds down
    a, b = torch.tensor([[[[1.0, 256.0]]]]).to(BF16), torch.tensor([[[[2.0 ** -8, 1.0]]]]).to(BF16)
    assert P.axpy_planes(a, b, torch.tensor([[3.0]])).float().tolist() == [[[[1.0 + 2.0 ** -6, 260.0]]]]            # 1 + 3 * 2^-8 ties up to even; 259 -> 260
    assert P.axpy_planes(a, b, None).float().tolist() == [[[[1.0, 256.0]]]]                  # 1 + 2^-8 and 257: ties, down to even
    assert P.same_values(torch.tensor([P.NAN, -0.0, 1.0]), torch.tensor([P.NAN, -0.0, 1.0]))
    assert not P.same_values(torch.tensor([0.0]), torch.tensor([-0.0])) and not P.same_values(torch.tensor([P.NAN]), torch.tensor([1.0]))


# ---- every parametrised case on the restatement alone, and what its shape claims ------------------------------------------------------------
@pytest.mark.parametrize('dtype, planes, h, w', P.ROW_CASES, ids=str)
def test_row_cases(dtype, planes, h, w):
    e = P.vec_elems(dtype)
    a, b = P.row_operands(dtype, planes, h, w)
    lda, ldb = P.row_pitches(w)
    assert lda != ldb and lda > w and P.rows_host_admits(h, w, dtype, lda, ldb) and P.rows_host_admits(h, w, dtype, lda, 0)
    assert w * P.esize(dtype) >= 16                                                          # the Python gates of plane_dot / plane_dot_gated admit it
    pa, pb = P.pitched(a, lda), P.pitched(b, ldb)
    assert a.shape == (*P.PLANE_SPLITS[planes], h, w) and (planes == 1 and h == 1 or not pa.is_contiguous())
    dense, bar = P.plane_dot(a, b)
    whole = lambda v, ld: v.as_strided((*v.shape[:3], ld), v.stride())
    got = P.plane_dot(whole(pa, lda), whole(pb, ldb)[..., :lda], w=w)[0]
    assert torch.equal(got, dense) and torch.isfinite(dense).all() and (bar > 0).all()
    want = np.einsum('nchw,nchw->nc', a.double().numpy(), b.double().numpy())
    assert np.abs(dense.numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert torch.equal(P.plane_dot(whole(pa, lda), None, w=w)[0], a.double().sum(dim=(2, 3)))
    # the integer side: exact rows with the fix-up; the old reciprocal read row 0 only wherever a row is one vector
    nvec = P.ceil_div(w, e)
    assert P.rows_first_wrong(h, w, dtype, fixed=True) is None
    assert P.rows_first_wrong(h, w, dtype, fixed=False) == (1 if (nvec == 1 and h > 1) else None)


def test_row_cases_cover_what_they_claim():
    for dtype in P.DTYPES:
        e = P.vec_elems(dtype)
        cases = [(p, h, w) for dt, p, h, w in P.ROW_CASES if dt == dtype]
        one_vec = [(p, h, w) for p, h, w in cases if w == e]
        assert {h for _, h, _ in one_vec} >= {1, 5, 70} and {P.rows_variant(h, w, dtype)[0] for _, h, w in one_vec} == {'wave', 'workgroup'}
        assert all(h * w * P.esize(dtype) > 16384 for _, h, w in one_vec if P.rows_variant(h, w, dtype)[0] == 'workgroup')
        ragged = {w for _, _, w in cases if e < w < 2 * e}
        assert ragged == ({10, 14} if e == 8 else {5, 7}) and all(w % e for w in ragged)
        assert P.rows_variant(40, 100, dtype)[0] == 'wave' and 40 * P.ceil_div(100, e) > 256 and P.rows_variant(40, 100, dtype)[1] >= 2
        assert P.rows_variant(70, 150, dtype)[0] == 'workgroup' and 70 * P.ceil_div(150, e) > 1024 and P.rows_variant(70, 150, dtype)[1] >= 2
        for shape in ((40, 100), (70, 150), (5, e)):
            assert {p for p, h, w in cases if (h, w) == shape} == {1, 5, 15}                 # 1 and 5: idle waves in the last workgroup of four
        assert {p for p, h, w in one_vec if P.rows_variant(h, w, dtype)[0] == 'workgroup'} == {1, 15}


def test_the_round_up_reciprocal_is_wrong_from_257_rows_of_4092_vectors_on_and_exact_with_the_fix_up():
    dtype, planes, h, w, ld = P.ROW_BIG
    assert (dtype, h, w) == (F32, 258, 16368) and P.rows_host_admits(h, w, dtype, ld, ld) and ld > w and planes == 1
    nvec = P.ceil_div(w, 4)
    assert nvec == 4092 == P.ceil_div(32736, 8)
    # the quotient is one over on the LAST vector of row 256: the first shape with a wrong row has 257 rows, in both element sizes
    assert P.rows_first_wrong(256, w, F32, fixed=False) is None and P.rows_first_wrong(256, 32736, BF16, fixed=False) is None
    assert P.rows_first_wrong(257, w, F32, fixed=False) == 256 * nvec + nvec - 1 == P.rows_first_wrong(257, 32736, F16, fixed=False)
    ic = np.arange(h * nvec)
    old = P.rows_quotient(ic, nvec, fixed=False)
    wrong = np.nonzero(old != ic // nvec)[0]
    assert wrong.tolist() == [256 * nvec + nvec - 1, 257 * nvec + nvec - 1] and (old[wrong] == wrong // nvec + 1).all()
    # ... which, at column (ic - row * nvec) * E = -E of the next row, is the right address only in a dense plane: with a pitch it is padding
    assert (wrong - old[wrong] * nvec).tolist() == [-1, -1] and ld - w >= 4
    assert P.rows_first_wrong(h, w, dtype, fixed=True) is None and P.rows_variant(h, w, dtype)[0] == 'workgroup'
    # no smaller vector count goes wrong within 257 rows, and the fix-up is exact over a sweep of the admitted range
    for n in range(2, 4092):
        top = np.arange(255 * n, 257 * n)
        assert (P.rows_quotient(top, n, fixed=False) == top // n).all(), n
    rng = np.random.default_rng(0)
    for n in [1, 2, 3, 5, 4091, 4092, 4093, 65535, 65537, (1 << 20) + 1, (1 << 24) - 1] + rng.integers(2, 1 << 24, 200).tolist():
        ic = np.concatenate([rng.integers(0, 1 << 27, 4000), np.arange(0, 3 * n, max(1, n // 50)), (1 << 27) - 1 - np.arange(100)])
        ic = np.concatenate([ic, (ic // n) * n, (ic // n) * n + n - 1])
        ic = ic[(ic >= 0) & (ic < (1 << 27))]
        assert (P.rows_quotient(ic, n, fixed=True) == ic // n).all(), n
        if n > 1:
            assert ((P.rows_quotient(ic, n, fixed=False) - ic // n) >> 1 == 0).all(), n      # never below, at most one above
    # the reference of the one large plane: finite, NaN as soon as a padding column is counted
    a = P.pitched(P.data((1, 1, h, w), dtype, 5), ld)
    buf = a.as_strided((1, 1, h, ld), a.stride())
    assert torch.isfinite(P.plane_dot(buf, buf, w=w)[0]).all() and P.plane_dot(buf, None, w=w + 1)[0].isnan().all()


@pytest.mark.parametrize('dtype, h, w', P.GATED_SHAPES, ids=str)
def test_gated_shapes(dtype, h, w):
    e = P.vec_elems(dtype)
    assert P.rows_variant(h, w, dtype)[0] == ('wave' if w == e else 'workgroup') and P.rows_host_admits(h, w, dtype, *P.row_pitches(w))
    assert {w == e for _, _, w in P.GATED_SHAPES} == {True, False}
    a = P.data((1, 8, h, w), dtype, 41)
    want, bar = P.plane_dot(a, a)
    assert want.shape == (1, 8) and (want > 0).all() and (bar < 1e-3 * want).all()


@pytest.mark.parametrize('dtype, hw', P.DENSE_CASES, ids=str)
def test_dense_cases(dtype, hw):
    n, c = P.DENSE_NC
    a, b = P.data((n, c, 1, hw), dtype, 51), P.data((n, c, 1, hw), dtype, 52)
    want, bar = P.plane_dot(a, b)
    ref = np.einsum('nchw,nchw->nc', a.double().numpy(), b.double().numpy())
    assert np.abs(want.numpy() - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()) and (bar >= 1e-6).all()
    assert torch.equal(P.plane_dot(a)[0], a.double().sum(dim=(2, 3)))
    splits = [P.dense_split(p, hw, dtype) for p in range(n * c)]
    assert all(head + nv * P.vec_elems(dtype) + tail == hw and 0 <= head < P.vec_elems(dtype) and 0 <= tail < P.vec_elems(dtype) for head, nv, tail in splits)
    if hw % 2 and hw > 2 * P.vec_elems(dtype):
        assert len({head for head, _, _ in splits}) == P.vec_elems(dtype)                    # an odd size: every 16-byte phase among the 15 planes


def test_dense_cases_cover_the_load_ladder():
    for dtype in P.DTYPES:
        e, es = P.vec_elems(dtype), P.esize(dtype)
        sizes = [hw for dt, hw in P.DENSE_CASES if dt == dtype]
        wave = [hw for hw in sizes if P.dense_variant(hw, dtype) == 'wave']
        group = [hw for hw in sizes if P.dense_variant(hw, dtype) == 'workgroup']
        assert {1, 2, e - 1} <= set(wave) and all(P.dense_split(0, hw, dtype)[1] == 0 for hw in (1, 2, e - 1))       # no whole vector at all
        assert max(wave) * es == 16384 and min(group) * es == 16384 + es                   # the last size of one kernel, the first of the other
        assert {P.dense_split(0, hw, dtype)[1] for hw in wave} >= {63, 64, 65, 127, 128, 129}
        # plane 0 (head 0) has exactly the vector count the size was built from; the ladder's three rungs all run, with and without b
        nvs = {P.dense_split(0, hw, dtype)[1] for hw in group}
        assert nvs >= {1024, 1025, 1279, 1280, 1281, 1535, 1536, 1537, 1791, 1792, 1793, 2047}
        trips = {nv: P.dense_trips(nv, dtype, e * nv + 3, True) for nv in nvs}
        assert trips[1024] == {'load4': 256, 'load2': 0, 'load1': 0}                       # the smallest planes of this kernel fill one 4-load trip
        assert trips[1025] == {'load4': 256, 'load2': 0, 'load1': 1} and trips[1279] == {'load4': 256, 'load2': 0, 'load1': 255}
        assert trips[1280] == {'load4': 256, 'load2': 0, 'load1': 256} and trips[1281] == {'load4': 256, 'load2': 1, 'load1': 255}
        assert trips[1535] == {'load4': 256, 'load2': 255, 'load1': 1}
        assert trips[1536] == {'load4': 256, 'load2': 256, 'load1': 0} and trips[1537] == {'load4': 256, 'load2': 256, 'load1': 1}
        assert trips[1791] == {'load4': 256, 'load2': 256, 'load1': 255}
        assert trips[1792] == {'load4': 256, 'load2': 256, 'load1': 256} and trips[1793] == {'load4': 257, 'load2': 255, 'load1': 255}
        assert trips[2047] == {'load4': 511, 'load2': 1, 'load1': 1}
        for nv, t in trips.items():                                                          # every vector is loaded exactly once
            assert 4 * t['load4'] + 2 * t['load2'] + t['load1'] == nv
            s = P.dense_trips(nv, dtype, e * nv + 3, False)                                  # the plain sum skips the 4-load loop
            assert s['load4'] == 0 and 2 * s['load2'] + s['load1'] == nv
        for nv in (63, 64, 65, 127, 128, 129):
            t = P.dense_trips(nv, dtype, e * nv + 3, True)
            assert t['load4'] == 0 and 2 * t['load2'] + t['load1'] == nv
        assert P.dense_trips(64, dtype, 64 * e + 3, True) == {'load4': 0, 'load2': 0, 'load1': 64}
        assert P.dense_trips(65, dtype, 65 * e + 3, True) == {'load4': 0, 'load2': 1, 'load1': 63}
        assert P.dense_trips(129, dtype, 129 * e + 3, True) == {'load4': 0, 'load2': 64, 'load1': 1}


@pytest.mark.parametrize('dt_in, dt_out', P.SCALE_PAIRS, ids=str)
def test_scale_cases(dt_in, dt_out):
    assert len(set(P.SCALE_PAIRS)) == 7
    assert {s[2] * s[3] for s in P.SCALE_SHAPES} == {1, 2, 3, 7, 8, 60}
    for shape in P.SCALE_SHAPES + [P.SCALE_BIG]:
        x = P.scale_input(shape, dt_in)
        assert x.isnan().any() and x.isinf().any()
        for scale in (P.plane_scale(*shape[:2]), None):
            y = P.scale_planes(x, scale, dt_out)
            assert y.dtype == dt_out and y.shape == x.shape and torch.equal(y.isnan(), x.isnan()) and (y.isinf() >= x.isinf()).all()
            v = x.double() * (1.0 if scale is None else scale.double()[:, :, None, None])
            fin = torch.isfinite(y.double()) & torch.isfinite(v)
            ulp = 2.0 ** -{F32: 24, BF16: 8, F16: 11}[dt_out]
            tiny = 2.0 ** -25 if dt_out == F16 else 0.0                                      # float16's subnormal spacing
            assert ((y.double() - v).abs()[fin] <= (v.abs() * ulp * (1 + 2.0 ** -10) + tiny)[fin]).all()
    planes, hw = P.SCALE_BIG[0] * P.SCALE_BIG[1], P.SCALE_BIG[2] * P.SCALE_BIG[3]
    want, cap = P.launch_blocks('scale_planes', planes, hw)
    assert hw % 4 == 0 and want > cap == 2048
    assert all(P.launch_blocks('scale_planes', s[0] * s[1], s[2] * s[3])[0] == 1 for s in P.SCALE_SHAPES)


def test_grid_stride_cases_exceed_their_caps():
    for planes, hw in P.AXPY_CASES:
        assert hw % 8 == 0
    assert P.launch_blocks('axpy_planes', *P.AXPY_CASES[0]) == (65600, 65535)
    assert P.ceil_div(P.AXPY_CASES[1][1] // 8, 1024) == 3                                    # grid.x: slices of 1024 vectors
    assert [P.launch_blocks('unscale', 1, n)[0] > 2048 for n in P.UNSCALE_NUMELS] == [False, False, False, True]
    assert [P.launch_blocks('unscale', 1, n)[0] for n in P.UNSCALE_NUMELS[:3]] == [1, 1, 2]
    assert set(P.UNSCALE_BOUNDS) == {(3.7, 1234.5), (3.7, None), (None, 2.0 ** -20), (None, None)}
    n, c, h, w = P.SPLIT_BIG
    assert (h * w) % 4 == 0 and n * c * h * w > 4096 * 256 * 4 and P.launch_blocks('split16', n * c, h * w) == (4114, 4096)
    numel = P.AMAX_BIG ** 2
    assert numel % 4 == 0 and numel > 2048 * 256 * 16 and P.launch_blocks('amax_bits', 1, numel) == (2054, 2048)
    assert P.amax_vector_path(numel, 0) and not P.amax_vector_path(944, 4) and not P.amax_vector_path(63, 0)
    assert sorted(set(P.COEF_CASES)) == sorted(P.COEF_CASES) and len(P.COEF_CASES) == 20
    assert {n for n, _, _ in P.COEF_CASES} == {1, 2, 64, 65, 130} and {n > 64 for n, _, _ in P.COEF_CASES} == {True, False}      # 64 lanes: the loop


@pytest.mark.parametrize('planes, hw', P.AXPY_CASES, ids=str)
def test_axpy_cases(planes, hw):
    for dtype in (BF16, F16):
        a, b = P.data((1, planes, 1, hw), dtype, 61), P.data((1, planes, 1, hw), dtype, 62)
        sc = P.plane_scale(1, planes)
        y = P.axpy_planes(a, b, sc)
        want = a.double() + sc.double()[:, :, None, None] * b.double()
        assert y.dtype == dtype and float((y.double() - want).abs().max()) <= float(want.abs().max()) * 2.0 ** (-7 if dtype == BF16 else -10)
        assert torch.equal(P.axpy_planes(a, b, None), (a.float() + b.float()).to(dtype))


@pytest.mark.parametrize('n, o, slots', P.COEF_CASES, ids=str)
def test_coef_cases(n, o, slots):
    psum, osc, nsc, bias, gz, dysy = P.coef_inputs(n, o, slots)
    out = P.layer_bwd_coefs(psum, osc, nsc, bias, gz, dysy)
    assert out['db'][0].shape == (o,) and out['d_next'][0].shape == out['d_out'][0].shape == (n, o)
    assert (nsc == 0).any() and (out['d_next'][0][nsc == 0] == 0).all() and (out['d_next'][0][nsc != 0] != 0).all()
    ps = psum.double().numpy().sum(axis=2)
    assert np.allclose(out['db'][0].numpy(), (ps / osc.double().numpy()).sum(axis=0), rtol=1e-12, atol=1e-12)
    assert np.allclose(out['d_out'][0].numpy(), (dysy.double().numpy() - bias.double().numpy() * ps) / osc.double().numpy() ** 2, rtol=1e-12, atol=1e-12)
    for name, (value, bar) in out.items():
        assert value.dtype == torch.float64 and bar.shape == value.shape and (bar >= 0).all() and (bar[value != 0] > 0).all(), name
        assert (value.abs() <= 1e5 * bar * (1 + 1e-12)).all(), name                          # a value is at most the sum of its terms' magnitudes
