"""The exact dense-layer tests' helper (dense_exact_ref.py) on a machine without a GPU: every case of every table inside the exactness
conditions (none skipped, none filtered), the float64 references against plain loops, the float32 leaky-ReLU rules against aten, and
the single-term construction of the lrelu backward cases."""
import numpy as np
import pytest
import torch

import dense_exact_ref as R


# ---- every case of every table satisfies the conditions -------------------------------------------------------------------------------------
@pytest.mark.parametrize('cin', R.FWD_CIN)
@pytest.mark.parametrize('n', R.NS)
def test_forward_op_cases_are_exact(n, cin):
    seen = set()
    for cout, act, bias in R.fwd_op_cases(n, cin):
        case = R.fc_fwd(n, cin, cout, act, bias)                     # (raises when no draw passes)
        assert case.failures() == [] and len(case.planted) == 3
        u = [float(case.u[r, c]) for r, c in case.planted]
        assert u[0] == 0.0 and u[1] < 0.0 < u[2]
        seen.add((cout, act, bias))
    assert len(seen) == len(R.FWD_COUT_OP) * 4


def test_forward_tables_put_every_value_in_every_thread_class():
    for nt in (1, 2, 4):
        ns = [n for n in R.NS if R.nt_class(n) == nt]
        assert len(ns) == 2
        assert {cin for n in ns for cin in R.FWD_CIN} == {16, 48, 144, 2032, 2048, 2064, 4608}
        assert {c[0] for n in ns for cin in R.FWD_CIN for c in R.fwd_op_cases(n, cin)} == {16, 48}
        assert {c[1] for n in ns for c in R.fwd_abi_cases(n)} == {1, 5, 18, 20, 33}
        for cases in ([c[1:] for n in ns for c in R.fwd_op_cases(n, 16)], [c[2:] for n in ns for c in R.fwd_abi_cases(n)]):
            assert set(cases) == {(a, b) for a in ('linear', 'lrelu') for b in (True, False)}


@pytest.mark.parametrize('n', R.NS)
def test_forward_abi_cases_are_exact(n):
    for cin, cout, act, bias in R.fwd_abi_cases(n):
        case = R.fc_fwd(n, cin, cout, act, bias)
        assert case.failures() == []
        assert len(case.planted) == min(3, n * cout)
        assert float(case.u[case.planted[0]]) == 0.0


@pytest.mark.parametrize('cout', R.BWD_COUT)
@pytest.mark.parametrize('n', R.NS)
def test_backward_cases_are_exact(n, cout):
    for cin in R.BWD_CIN:
        assert R.fc_linear_bwd(n, cin, cout).failures() == []
    assert R.fc_lrelu_bwd(n, cout).failures() == []


@pytest.mark.parametrize('case', R.BANK_CASES, ids=R.bank_id)
def test_affine_bank_cases_are_exact(case):
    assert R.affine_bank_case(case).failures() == []


def test_conditions_reject_what_is_not_exact():
    """The checks have teeth: an operand off the fp32 grid, and a sum past 2^24 quanta."""
    case = R.FcLinearBwd(16, 16, 16)
    case.x = case.x + 2.0 ** -30
    assert any('x is not representable' in m for m in case.failures())
    case = R.FcFwd(16, 16, 16, 'linear', True)
    case.x = case.x.clone()
    case.x[3] *= 2.0 ** 22                                           # (the other rows keep the quantum at 1)
    assert any('quanta' in m for m in case.failures())


# ---- the references against plain loops -------------------------------------------------------------------------------------------------------
def test_fc_reference_equals_the_triple_loop():
    f = R.fc_fwd(1, 16, 16, 'linear', True)
    for n in range(f.n):
        for o in range(f.cout):
            s = 0.0
            for k in range(f.cin):
                s += float(f.x[n, k]) * float(f.w[o, k])
            assert float(f.u[n, o]) == f.alpha * s + f.beta * float(f.b[o])
    c = R.fc_linear_bwd(1, 16, 16)
    for k in range(c.cin):
        assert float(c.dx[0, k]) == c.alpha * sum(float(c.gy[0, o]) * float(c.w[o, k]) for o in range(c.cout))
        for o in range(c.cout):
            assert float(c.dw[o, k]) == c.alpha * sum(float(c.gy[n, o]) * float(c.x[n, k]) for n in range(c.n))
    for o in range(c.cout):
        assert float(c.db[o]) == c.beta * sum(float(c.gy[n, o]) for n in range(c.n))
    # ... and autograd of the same float64 formula
    x, w, b = (t.clone().requires_grad_(True) for t in (c.x, c.w, c.b))
    y = c.alpha * (x @ w.t()) + c.beta * b
    dx, dw, db = torch.autograd.grad((y * c.gy).sum(), [x, w, b])
    assert torch.equal(y.detach(), c.y) and torch.equal(dx, c.dx) and torch.equal(dw, c.dw) and torch.equal(db, c.db)


def test_affine_reference_equals_the_triple_loop_and_autograd():
    b = R.affine_bank_case(R.Bank(1, 16, 0, (8, 24, 7), None, ()))
    for l, c in enumerate(b.case.couts):
        for o in range(c):
            s = 0.0
            for k in range(16):
                s += float(b.ws[0, b.idx[l], k]) * float(b.W[l][o, k])
            assert float(b.y[l][0, o]) == b.scale[l] * (b.wgain[l] * s + b.bgain[l] * float(b.b[l][o]))
    for case in (R.Bank(17, 32, 1024, (8, 24, 7), None, ()), R.BANK_CASES[-1]):
        b = R.affine_bank_case(case)
        ws, g = b.ws.clone().requires_grad_(True), b.g.clone().requires_grad_(True)
        W, bs = [t.clone().requires_grad_(True) for t in b.W], [t.clone().requires_grad_(True) for t in b.b]
        ys = [(torch.cat((ws[:, i], g), 1) @ (Wl * wg).t() + bl * bg) * sc for i, Wl, bl, wg, bg, sc in zip(b.idx, W, bs, b.wgain, b.bgain, b.scale)]
        loss = sum((y * d).sum() for y, d in zip(ys, b.dy) if d is not None)
        grads = torch.autograd.grad(loss, [ws, g] + W + bs, allow_unused=True)
        nl = len(W)
        assert all(torch.equal(a.detach(), e) for a, e in zip(ys, b.y))
        assert torch.equal(grads[0], b.dws) and torch.equal(grads[1], b.dg)
        for l in range(nl):
            for got, want in ((grads[2 + l], b.dW[l]), (grads[2 + nl + l], b.db[l])):
                assert torch.equal(torch.zeros_like(want) if got is None else got, want)
        assert all(float(b.dW[l].abs().max()) == 0.0 for l in case.drop) and len(case.drop) == (1 if case.idx else 0)


# ---- the float32 leaky-ReLU rules ---------------------------------------------------------------------------------------------------------------
def test_lrelu_rules_are_leaky_relu_times_sqrt2_to_one_ulp():
    us = [R.fc_fwd(n, cin, 48, 'lrelu', True).u for n in (1, 17, 64) for cin in (16, 144, 4608)]
    u = torch.cat([t.flatten() for t in us])
    assert bool((u == 0).any()) and bool((u < 0).any()) and bool((u > 0).any())
    got = R.lrelu32(u)
    want = torch.nn.functional.leaky_relu(u, 0.2) * np.sqrt(2)
    ulp = torch.from_numpy(np.spacing(np.abs(want.numpy()).astype(np.float32)).astype(np.float64))
    # aten's own float32 evaluation of the same expression: within 1 ulp
    want32 = (torch.nn.functional.leaky_relu(u.float(), 0.2) * np.sqrt(2)).double()
    assert bool(((got - want32).abs() <= ulp).all())
    # the float64 value: 0.2f and G each stand half an ulp off their real number and each product rounds once -- 2 ulp on the slope
    # side, 1 ulp (G and one rounding) on the other
    assert bool(((got - want).abs() <= torch.where(u > 0, ulp, 2 * ulp)).all())
    assert bool((got[u == 0] == 0).all()) and bool((torch.sign(got) == torch.sign(u)).all())
    # backward: the derivative of the same function, chosen by the sign of the OUTPUT; -0, +0 and negative outputs take the slope
    y = torch.tensor(R.Y_CLASSES, dtype=torch.float64)
    gy = torch.full_like(y, 0.5)
    gp = R.gp32(gy, y)
    slope = torch.where(y > 0, torch.tensor(np.sqrt(2)), torch.tensor(0.2 * np.sqrt(2)))
    assert bool(((gp - gy * slope).abs() <= 2 * torch.from_numpy(np.spacing((gy * slope).numpy().astype(np.float32)).astype(np.float64))).all())
    assert [float(v) for v in gp] == [0.5 * float(R.G32) if v > 0 else 0.5 * float(R.GS32) for v in R.Y_CLASSES]
    assert float(gp[2]) == float(gp[3]) == float(gp[1]) == float(gp[5]) != float(gp[0]) == float(gp[4])


# ---- the single-term construction -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cout', R.BWD_COUT)
@pytest.mark.parametrize('n', R.NS)
def test_single_term_cotangents_leave_one_term_per_sum_and_cover_every_column(n, cout):
    case = R.fc_lrelu_bwd(n, cout)
    cols, rows, classes = set(), set(), set()
    for t, v in case.launches:
        gy = case.gy(t, v)
        nz = gy != 0
        live = min(cout, n - v)
        assert int(nz.sum()) == live                                                     # one per row of the window ...
        assert nz.sum(1).tolist() == [1 if v <= r < v + cout else 0 for r in range(n)]
        assert int(nz.sum(0).max()) == 1                                                 # ... and pi injective: at most one per column
        ref = case.ref(t, v)
        hit = nz.any(0)
        assert float(ref['dw'][~hit].abs().max() if bool((~hit).any()) else 0.0) == 0.0 and float(ref['db'][~hit].abs().sum()) == 0.0
        assert bool((ref['db'][hit] != 0).all()) and bool((ref['dx'][nz.any(1)] != 0).all())
        cols |= set(hit.nonzero().flatten().tolist())
        rows |= set(nz.any(1).nonzero().flatten().tolist())
        classes |= set(case.cls[nz].tolist())
        if live >= 6:
            assert set(case.cls[nz].tolist()) == set(range(6))
    assert cols == set(range(cout)) and rows == set(range(n))
    assert classes == set(range(6))                                                      # every class of saved output meets a cotangent
    assert torch.equal(case.y.abs().unique(), torch.tensor([0.0, 2.0 ** -100, 1.0], dtype=torch.float64))
    assert int((torch.signbit(case.y) & (case.y == 0)).sum()) > 0                        # -0 is there
    assert float(case.y.abs()[case.y != 0].min()) >= float(np.finfo(np.float32).tiny)    # no subnormals
