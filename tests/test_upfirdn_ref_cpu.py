"""tests/upfirdn_ref.py checked without a GPU: the float64 restatement against the oracle's two independent ones and two cases worked by
hand; its transpose by <A x, r> == <x, A^T r>; the derived bound against an fp32 emulation of the definition (which must stay inside it on
every GPU case) and four deliberately wrong ones (each must leave it somewhere in every list it applies to); and which kernel each listed
case reaches."""
import numpy as np
import pytest
import torch

import upfirdn_ref as U

F32, F16, BF16 = U.F32, U.F16, U.BF16
LISTS = {'gather': U.GATHER_PARAMS, 'tile': U.TILE_PARAMS, 'rows': U.ROWS_PARAMS}
ALL_PARAMS = [(kind, name, dt) for kind, params in LISTS.items() for name, dt in params]


def _ids(v):
    return U.param_id(v)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def test_two_cases_worked_by_hand():
    # x = [1 2 3], f = [1 10 100], no padding: one output.  Convolution: f reversed meets z -> 100*1 + 10*2 + 1*3; flip: 1*1 + 10*2 + 100*3
    x, f = np.array([[[[1.0, 2.0, 3.0]]]]), np.array([[1.0, 10.0, 100.0]])
    assert U.upfirdn2d(x, f).tolist() == [[[[123.0]]]]
    assert U.upfirdn2d(x, f, flip=True).tolist() == [[[[321.0]]]]
    # up 2 along x, down 2 along y, x = [[1 2], [3 4], [5 6]], f = [[1 2], [4 8]] (flip: w = f), padding x (1, 1), y (0, 1), gain 0.5:
    # z rows (x-padded) = [0 1 0 2 0 0], [0 3 0 4 0 0], [0 5 0 6 0 0], [0 0 0 0 0 0]; outputs at z rows (0, 1) and (2, 3), columns ox .. ox + 1
    x, f = np.array([[[[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]]]), np.array([[1.0, 2.0], [4.0, 8.0]])
    y = U.upfirdn2d(x, f, up=(2, 1), down=(1, 2), padding=(1, 1, 0, 1), flip=True, gain=0.5)
    row0 = [2 * 1 + 8 * 3, 1 * 1 + 4 * 3, 2 * 2 + 8 * 4, 1 * 2 + 4 * 4, 0]
    row1 = [2 * 5, 1 * 5, 2 * 6, 1 * 6, 0]
    assert y.tolist() == [[[[0.5 * v for v in row0], [0.5 * v for v in row1]]]]
    assert U.out_size(3, 2, 2, 2, (2, 1), (1, 2), (1, 1, 0, 1)) == (2, 5)


@pytest.mark.parametrize('up, down, pad, fshape', [(1, 1, [0, 0, 0, 0], (3, 3)), (2, 1, [2, 1, 3, 0], (4, 4)), (1, 2, [1, 2, 0, 3], (4, 3)), (3, 2, [-2, 5, 4, -3], (5, 6)),
                                                   (4, 4, [9, -5, -3, 11], (8, 8)), (1, 1, [7, 6, 9, 8], (2, 3)), (2, 3, [-3, 4, -1, 2], (1, 7))])
def test_equals_the_isotropic_numpy_oracle(up, down, pad, fshape):
    from oracle import direct_np as dnp
    g = np.random.default_rng(3)
    x, f = g.standard_normal((2, 3, 7, 9)), g.standard_normal(fshape)
    for flip in (False, True):
        want = dnp.upfirdn2d(x, f, up=up, down=down, padding=pad, flip_filter=flip, gain=1.5)
        got = U.upfirdn2d(x, f, (up, up), (down, down), tuple(pad), flip, 1.5)
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize('name', [c.name for c in U.GATHER_CASES if c.up[0] != c.up[1] or c.down[0] != c.down[1]])
def test_equals_the_aten_oracle_on_per_axis_factors(name):
    from oracle import aten_ops as ops
    case = U.BY_NAME['gather'][name]
    x, f, _ = U.inputs(case, F32)
    for flip in (False, True):
        want = ops.upfirdn2d(x, f, up=case.up, down=case.down, padding=list(case.padding), flip_filter=flip, gain=case.gain).double().numpy()
        got = U.upfirdn2d(U.f64(x), U.f64(f), case.up, case.down, case.padding, flip, case.gain)
        # aten's fp32 convolution: K products and sums, each rounded -- 2 (K + 2) 2^-24 of the sum of magnitudes covers any order
        bar = 2 * (f.numel() + 2) * U.U24 * U.upfirdn2d(np.abs(U.f64(x)), np.abs(U.f64(f)), case.up, case.down, case.padding, flip, abs(case.gain))
        assert got.shape == want.shape and bool((np.abs(got - want) <= bar).all())


@pytest.mark.parametrize('kind, name, dtype', ALL_PARAMS, ids=_ids)
def test_adjoint_is_the_transpose(kind, name, dtype):
    """<A x, r> == <x, A^T r> to 1e-12 of the terms' magnitudes, and the scatter equals the forward call the op's backward makes."""
    case = U.BY_NAME[kind][name]
    x, f, r = (U.f64(t) for t in U.inputs(case, dtype))
    for flip in (False, True):
        y, _, dx, _ = U.reference(kind, name, dtype, flip)
        lhs, rhs = float((y * r).sum()), float((x * dx).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, float(np.abs(y * r).sum()), float(np.abs(x * dx).sum())), (lhs, rhs)
        gup, gdown, gpad, gflip = U.grad_call(case.xshape[2:], case.fshape, case.up, case.down, case.padding, flip)
        again = U.upfirdn2d(r, f, gup, gdown, gpad, gflip, case.gain)
        assert again.shape == dx.shape and np.abs(again - dx).max() <= 1e-12 * max(1.0, np.abs(dx).max())


def test_half_ulp_and_zero_bound():
    assert U.half_ulp(np.array([1.0, 1.99, 2.0, 0.75, 2.0 ** -20]), F16).tolist() == [2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** -12, 2.0 ** -25]
    assert U.half_ulp(np.array([1.0, 255.0, 2.0 ** -130]), BF16).tolist() == [2.0 ** -8, 2.0 ** -1, 2.0 ** -134]
    # rounding a value to the type moves it by at most that much
    v = np.random.default_rng(0).standard_normal(4096) * 37
    for dt in (F16, BF16):
        assert bool((np.abs(U.round_to(v, dt) - v) <= U.half_ulp(np.abs(v), dt)).all())
    # outputs that meet no sample: bound 0, and only +0 passes
    case = U.BY_NAME['gather']['pad_beyond_filter']
    y, bar, _, _ = U.reference('gather', case.name, BF16, False)
    assert bool((bar[..., :5] == 0).all()) and bool((bar[..., :5, :] == 0).all()) and bool((bar[..., 5:12, 5:11] > 0).all())
    assert U.mismatch(y, y, bar) is None and U.mismatch(np.where(bar == 0, -0.0, y), y, bar) is not None
    assert U.mismatch(y + 2 * bar, y, bar) is not None and U.mismatch(y + 0.99 * bar, y, bar) is None


# ---- the bound tells a wrong kernel from a right one --------------------------------------------------------------------------------------
MUTATIONS = ('drop_last_tap', 'left_edge_off_by_one', 'flip_ignored', 'c_remainder')


def emulate(x, f, up, down, padding, flip, gain, mutation=None, reverse=False):
    """The definition in fp32, as a gather: each output walks the taps that meet a sample (first tap k0 = (-U) mod up at sample (U + k0) / up,
    then steps of up taps / one sample), every product and sum rounded to fp32.  ``reverse``: the other summation order.  Mutations:
      drop_last_tap         the last tap of every filter row is never reached
      left_edge_off_by_one  column 0 of the input counts as outside the plane
      flip_ignored          the taps are reversed whether or not flip is set
      c_remainder           k0 with C's %, which is negative for positive U: the walk starts one step early, on the element BEFORE the tap row
                            in the flattened tap array (the previous row's last taps; nothing before the first row)"""
    x = np.asarray(x, dtype=np.float32)
    f = np.asarray(f, dtype=np.float32)
    taps = ((f if (flip and mutation != 'flip_ignored') else f[::-1, ::-1]) * np.float32(gain)).astype(np.float32).ravel()
    (n, c, xh, xw), (fh, fw), (ux, uy), (dx, dy), (px0, _, py0, _) = x.shape, f.shape, up, down, padding
    yh, yw = U.out_size(xh, xw, fh, fw, up, down, padding)
    Uy, Ux = np.arange(yh) * dy - py0, np.arange(yw) * dx - px0
    rem = np.fmod if mutation == 'c_remainder' else np.mod
    ky0, kx0 = rem(-Uy, uy), rem(-Ux, ux)
    iy0, ix0 = (Uy + ky0) // uy, (Ux + kx0) // ux
    steps = [(sy, sx) for sy in range((fh - 1) // uy + 2) for sx in range((fw - 1) // ux + 2)]
    acc = np.zeros((n, c, yh, yw), dtype=np.float32)
    for sy, sx in (reversed(steps) if reverse else steps):
        ky, iy, kx, ix = ky0 + sy * uy, iy0 + sy, kx0 + sx * ux, ix0 + sx
        oky = (ky < fh) & (iy >= 0) & (iy < xh)
        okx = (kx < (fw - 1 if mutation == 'drop_last_tap' else fw)) & (ix >= (1 if mutation == 'left_edge_off_by_one' else 0)) & (ix < xw)
        flat = ky[:, None] * fw + kx[None, :]
        ok = oky[:, None] & okx[None, :] & (flat >= 0)
        if not ok.any():
            continue
        t = np.where(ok, taps[np.clip(flat, 0, taps.size - 1)], np.float32(0))
        xs = x[:, :, np.clip(iy, 0, xh - 1)][:, :, :, np.clip(ix, 0, xw - 1)]
        acc = acc + t * xs
        assert acc.dtype == np.float32
    return acc


def _emulated(case, dtype, flip, grad, **kw):
    """The emulation's output in ``dtype`` (as float64) for the case's forward call, or for the call its backward makes on r."""
    x, f, r = U.inputs(case, dtype)
    if grad:
        up, down, pad, fl = U.grad_call(case.xshape[2:], case.fshape, case.up, case.down, case.padding, flip)
        acc = emulate(r.float().numpy(), f.numpy(), up, down, pad, fl, case.gain, **kw)
    else:
        acc = emulate(x.float().numpy(), f.numpy(), case.up, case.down, case.padding, flip, case.gain, **kw)
    return U.f64(torch.from_numpy(acc).to(dtype))


@pytest.mark.parametrize('kind, name, dtype', ALL_PARAMS, ids=_ids)
def test_fp32_emulation_stays_within_the_bound(kind, name, dtype):
    case = U.BY_NAME[kind][name]
    heavy = case.fshape[0] * case.fshape[1] > 1000 or case.xshape[0] > 1000
    for flip in (False, True):
        y, ybar, dx, dxbar = U.reference(kind, name, dtype, flip)
        for reverse in ((False,) if heavy else (False, True)):
            assert U.mismatch(_emulated(case, dtype, flip, False, reverse=reverse), y, ybar) is None
            assert U.mismatch(_emulated(case, dtype, flip, True, reverse=reverse), dx, dxbar) is None


@pytest.mark.parametrize('kind', sorted(LISTS))
@pytest.mark.parametrize('mutation', MUTATIONS)
def test_every_wrong_restatement_leaves_the_bound(mutation, kind):
    """In every list, in every dtype of the list, at least one element of at least one case (forward) is outside its bound."""
    for dtype in sorted({dt for _, dt in LISTS[kind]}, key=str):
        killed = []
        for name, dt in LISTS[kind]:
            case = U.BY_NAME[kind][name]
            if dt != dtype or case.fshape[0] * case.fshape[1] > 1000 or case.xshape[0] > 1000:
                continue
            for flip in (False, True):
                y, ybar, _, _ = U.reference(kind, name, dtype, flip)
                if U.mismatch(_emulated(case, dtype, flip, False, mutation=mutation), y, ybar) is not None:
                    killed.append((name, flip))
        assert killed, (mutation, kind, dtype)


# ---- every list reaches the kernel it names ------------------------------------------------------------------------------------------------
def test_case_lists_reach_their_kernels():
    assert all(U.kernel_of(U.BY_NAME['gather'][name], dt) == 'gather' for name, dt in U.GATHER_PARAMS)
    assert all(U.kernel_of(U.BY_NAME['tile'][name], dt) == 'tile' for name, dt in U.TILE_PARAMS)
    assert all(U.kernel_of(c, F32) == 'tile' for c in U.TILE_CASES)
    # the rows list: the rows kernel, except the shapes launch_rows now leaves to the tile kernel -- 2 columns wide, first group 4 to the left
    assert U.ROWS_SUSPECT in U.ROWS_LEFT_TO_TILE
    for c in U.ROWS_CASES:
        to_tile = c.xshape[3] == 2 and c.padding[0] == (3 if c.up[0] == 1 else 6)
        assert (c.name in U.ROWS_LEFT_TO_TILE) == to_tile
        for dt in (F16, BF16):
            assert U.kernel_of(c, dt) == ('tile' if to_tile else 'rows'), c
            assert U.kernel_of(c, dt, aligned=False) == 'tile'
    assert len(U.AGREE_PARAMS) >= 20 and any(min(U.BY_NAME['rows'][n].fshape) < 4 for n, _ in U.AGREE_PARAMS)
    # each kernel in each dtype it supports
    reached = {(U.kernel_of(U.BY_NAME[kind][name], dt), dt) for kind, name, dt in ALL_PARAMS}
    assert reached == {('gather', F32), ('gather', F16), ('gather', BF16), ('tile', F32), ('tile', F16), ('tile', BF16), ('rows', F16), ('rows', BF16)}
    # gradients too: the backward of each list's cases runs that list's kernel family somewhere
    for kind, dts in (('gather', U.DTYPES), ('tile', U.DTYPES), ('rows', (F16, BF16))):
        for dt in dts:
            back = set()
            for name, d in LISTS[kind]:
                c = U.BY_NAME[kind][name]
                if d == dt:
                    gup, gdown, gpad, _ = U.grad_call(c.xshape[2:], c.fshape, c.up, c.down, c.padding, False)
                    yh, yw = U.out_size(c.xshape[2], c.xshape[3], c.fshape[0], c.fshape[1], c.up, c.down, c.padding)
                    back.add(U.expected_kernel(dt, c.xshape[:2] + (yh, yw), c.fshape, gup, gdown, gpad))
            assert kind in back, (kind, dt, back)


def test_case_lists_cover_what_they_are_for():
    g = U.BY_NAME['gather']
    assert {c.up + c.down for c in U.GATHER_CASES} >= {(2, 1, 1, 1), (1, 2, 1, 1), (1, 1, 2, 1), (1, 1, 1, 2), (3, 2, 2, 3), (2, 2, 2, 2), (2, 2, 4, 4),
                                                        (4, 4, 2, 2), (4, 4, 1, 1), (1, 1, 4, 4), (3, 3, 1, 1), (1, 1, 3, 3)}
    assert {c.fshape for c in U.GATHER_CASES} >= {(4, 4), (2, 3), (1, 12), (12, 1), (5, 3), (24, 24), (1, 61), (61, 1), (64, 64)}
    outs = [U.out_size(c.xshape[2], c.xshape[3], *c.fshape, c.up, c.down, c.padding) for c in U.GATHER_CASES]
    assert {w for _, w in outs} >= {1, 63, 64, 65, 130} and {h for h, _ in outs} >= {1, 3, 4, 5, 9}
    c = g['planes_16400']
    assert c.xshape[0] * c.xshape[1] > 256 * 64 and outs[U.GATHER_CASES.index(c)] == (3, 3)            # one block per plane, more than the cap
    assert 35 <= len(U.GATHER_CASES) <= 45
    assert U.TAPS_TOO_MANY.fshape[0] * U.TAPS_TOO_MANY.fshape[1] > 4096 == g['taps_4096'].fshape[0] * g['taps_4096'].fshape[1]
    t_outs = {U.out_size(c.xshape[2], c.xshape[3], *c.fshape, c.up, c.down, c.padding) + c.up[:1] + c.down[:1] for c in U.TILE_CASES}
    assert t_outs >= {(32, 64, u, d) for u, d in ((1, 1), (1, 2), (2, 1))} | {(33, 65, u, d) for u, d in ((1, 1), (1, 2), (2, 1))}
    rows = [c for c in U.ROWS_CASES]
    assert {c.xshape[3] for c in rows} == {2, 4, 6, 8, 10, 16} and {c.padding[2] for c in rows} >= set(range(8)) and {c.xshape[1] for c in rows} == {1, 3}
    for u, d, rpt, pmax in ((1, 1, 8, 3), (1, 2, 4, 3), (2, 1, 8, 6)):
        mine = [c for c in rows if (c.up[0], c.down[0]) == (u, d)]
        assert {c.padding[0] for c in mine} == set(range(pmax + 1))
        assert {U.out_size(c.xshape[2], c.xshape[3], *c.fshape, c.up, c.down, c.padding)[0] for c in mine} >= {1, 2, 3, rpt - 1, rpt, rpt + 1}
        assert all(U.out_size(c.xshape[2], c.xshape[3], *c.fshape, c.up, c.down, c.padding)[1] % 2 == 0 for c in mine)
