"""The dense-layer kernels against exact arithmetic, bit for bit (operands, references, conditions and case tables: dense_exact_ref.py).

fc_act forward and backward (csrc/fc_bank.hip) and the style affine bank (csrc/affine_bank.hip) run on v_mfma_f32_16x16x4_f32; with
operands that are small integers times powers of two and power-of-two gains, every fp32 partial sum of every order is exact, so each
element has ONE right answer -- the float64 reference cast to fp32 -- and every comparison here is ``torch.equal``.  A failure names the
first differing index, both values and the lane class (index % 16, index // 16 % 4) of each of its coordinates: which lane of a 16 x 16
tile and which of the four lane groups / waves / k slots the element went through.  The shapes come from the kernels' own thresholds:
NT = 1 / 2 / 4 row tiles (n <= 16 / 32 / 64) with a dead-row tail in each, fewer K chunks than waves, the tail loop alone, the 8-deep
loop plus a tail, the 16-wave form (cin >= 2048 at n <= 32) with an idle last wave, 1 / 4 / 5 / 9 row tiles in the backward's
two-tiles-per-trip loop, 1 / 2 / 3 passes of 16 batch rows and 2 / 3 row blocks of 64 in the bank.

The mapping input stage is not exact (rsqrtf): it keeps the float64 reference and the bars of test_mapping_input_vs_float64 (1e-5
forward, 3e-5 gradients), applied per row instead of per tensor, on a batch that mixes ordinary rows with rows 1e3 and 1e-3 times as
large, an eps-dominated row, an all-zero row and a sample whose embedding is exactly zero.
"""
import types

import pytest
import torch

import dense_exact_ref as R

pytestmark = pytest.mark.gpu

F32 = torch.float32
SENTINEL = -777.25


@pytest.fixture(scope='module')
def abi():
    from afcm_amd import _lib
    return _lib, _lib.load()


def _fc():
    from afcm_amd.torch_utils.ops import fc_bank
    return fc_bank


def _dev(t, grad=False):
    return None if t is None else t.to(F32).cuda().requires_grad_(grad)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _churn(seed):
    """Unrelated allocations of odd sizes, some freed again: the next run's buffers land elsewhere."""
    keep = [torch.full([257 * (k + seed) + 3], float('nan'), device='cuda') for k in range(1, 6)]
    del keep[1::2]
    return keep


# ---- fc_act forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cin', R.FWD_CIN)
@pytest.mark.parametrize('n', R.NS)
def test_fc_act_forward(n, cin):
    fc_bank = _fc()
    for cout, act, bias in R.fwd_op_cases(n, cin):
        case = R.fc_fwd(n, cin, cout, act, bias)
        x, w, b = _dev(case.x), _dev(case.w), _dev(case.b)
        assert fc_bank.supported(x, w, act)
        y = fc_bank.fc_act(x, w, b, case.alpha, case.beta, act)
        R.assert_exact(y, case.y, f'y of n={n} cin={cin} cout={cout} {act} bias={bias} (NT={R.nt_class(n)}, {"16" if cin >= 2048 and n <= 32 else "4"} waves)')


@pytest.mark.parametrize('n', R.NS)
def test_fc_act_forward_partial_row_tiles_through_the_c_abi(n, abi):
    """cout % 16 != 0 (fc_bank.supported never lets it through, afcm_fc_act_fwd takes it): the element-wise tail (cout 1, 5, 18, 33) and
    the cout % 4 == 0 tail whose last tile stores one lane group (20).  y is dense, [n, cout], inside a buffer of sentinels: four guard
    rows in front, four and a tile behind -- the tail must write nothing in front of y or past its last row, and every element of y."""
    L, lib = abi
    for cin, cout, act, bias in R.fwd_abi_cases(n):
        case = R.fc_fwd(n, cin, cout, act, bias)
        x, w, b = _dev(case.x), _dev(case.w), _dev(case.b)
        front, back = 4 * cout, 4 * cout + 16
        buf = torch.full([front + n * cout + back], SENTINEL, device='cuda')
        y = buf[front:front + n * cout].view(n, cout)
        y.fill_(float('nan'))
        assert y.data_ptr() % 16 == 0
        rc = lib.afcm_fc_act_fwd(y.data_ptr(), x.data_ptr(), w.data_ptr(), _ptr(b), n, cin, cout, case.alpha, case.beta, 1 if act == 'lrelu' else 0, _stream())
        assert rc == 0, (rc, lib.afcm_last_error())
        what = f'n={n} cin={cin} cout={cout} {act} bias={bias}'
        R.assert_exact(y, case.y, 'y of ' + what)
        guard = torch.cat([buf[:front], buf[front + n * cout:]]).cpu()
        assert bool((guard == SENTINEL).all()), f'{what}: {int((guard != SENTINEL).sum())} guard elements overwritten, first at {int((guard != SENTINEL).nonzero()[0]) - front} from y'


def test_fc_act_forward_is_bit_identical_after_unrelated_allocations():
    fc_bank = _fc()
    case = R.fc_fwd(17, 4608, 48, 'lrelu', True)
    outs = []
    for k in range(2):
        y = fc_bank.fc_act(_dev(case.x), _dev(case.w), _dev(case.b), case.alpha, case.beta, 'lrelu')
        outs.append((y, _churn(k)))
    assert outs[0][0].data_ptr() != outs[1][0].data_ptr() and torch.equal(outs[0][0], outs[1][0])
    R.assert_exact(outs[1][0], case.y, 'second run')


# ---- fc_act backward, linear: fully exact ---------------------------------------------------------------------------------------------------
def _linear_backward(case, names):
    """y and {name: gradient} of one run that asks for the gradients in ``names`` only; the others must be absent."""
    fc_bank = _fc()
    leaves = dict(dx=_dev(case.x, 'dx' in names), dw=_dev(case.w, 'dw' in names), db=_dev(case.b, 'db' in names))
    assert fc_bank.supported(leaves['dx'], leaves['dw'], 'linear')
    y = fc_bank.fc_act(leaves['dx'], leaves['dw'], leaves['db'], case.alpha, case.beta, 'linear')
    y.backward(_dev(case.gy))
    for k, t in leaves.items():
        assert (t.grad is not None) == (k in names), f'{k} with {names}'
    return y.detach(), {k: leaves[k].grad for k in names}


@pytest.mark.parametrize('cout', R.BWD_COUT)
@pytest.mark.parametrize('n', R.NS)
def test_fc_act_backward_linear_every_gradient_subset(n, cout):
    for cin in R.BWD_CIN:
        case = R.fc_linear_bwd(n, cin, cout)
        what = f'n={n} cin={cin} cout={cout} ({cout // 16} row tiles)'
        y, full = _linear_backward(case, R.SUBSETS[0])
        R.assert_exact(y, case.y, 'y of ' + what)
        for k in R.SUBSETS[0]:
            R.assert_exact(full[k], getattr(case, k), f'{k} of {what}')
        for names in R.SUBSETS[1:]:
            _, part = _linear_backward(case, names)
            for k in names:
                R.assert_exact(part[k], getattr(case, k), f'{k} of {what}, asked {names}')
                assert torch.equal(part[k], full[k]), f'{k} of {what}: asked {names} differs from the all-three run'


def test_fc_act_backward_is_bit_identical_after_unrelated_allocations():
    case = R.fc_linear_bwd(33, 48, 144)
    runs = []
    for k in range(2):
        runs.append((_linear_backward(case, R.SUBSETS[0])[1], _churn(k)))
    for k in R.SUBSETS[0]:
        assert runs[0][0][k].data_ptr() != runs[1][0][k].data_ptr() and torch.equal(runs[0][0][k], runs[1][0][k]), k


# ---- fc_act backward, lrelu: single-term cotangents against a chosen saved output ------------------------------------------------------------
def _abi_backward(abi, case, xd, wd, gy, y, names):
    L, lib = abi
    out = dict(dx=torch.full([case.n, case.cin], float('nan'), device='cuda') if 'dx' in names else None,
               dw=torch.full([case.cout, case.cin], float('nan'), device='cuda') if 'dw' in names else None,
               db=torch.full([case.cout], float('nan'), device='cuda') if 'db' in names else None)
    rc = lib.afcm_fc_act_bwd(_ptr(out['dx']), _ptr(out['dw']), _ptr(out['db']), gy.data_ptr(), y.data_ptr(), xd.data_ptr(), wd.data_ptr(),
                             case.n, case.cin, case.cout, case.alpha, case.beta, 1, _stream())
    assert rc == 0, (rc, lib.afcm_last_error())
    return out


@pytest.mark.parametrize('cout', R.BWD_COUT)
@pytest.mark.parametrize('n', R.NS)
def test_fc_act_backward_lrelu_single_term_with_chosen_saved_output(n, cout, abi):
    """The saved output holds 1, -1, +0, -0, 2^-100 and -2^-100; each meets a non-zero cotangent.  gp = gy * G only where y > 0."""
    case = R.fc_lrelu_bwd(n, cout)
    xd, wd = _dev(case.x), _dev(case.w)
    y = _dev(case.y)
    assert bool((torch.signbit(y) & (y == 0)).any())                       # -0 arrived on the device as -0
    for i, (t, v) in enumerate(case.launches):
        gy = _dev(case.gy(t, v))
        ref = case.ref(t, v)
        full = _abi_backward(abi, case, xd, wd, gy, y, R.SUBSETS[0])
        for k in R.SUBSETS[0]:
            if not torch.equal(full[k], ref[k].to(F32).cuda()):
                R.assert_exact(full[k], ref[k], f'{k} of n={n} cout={cout}, shift {t}, rows from {v}')
        if i == 0:
            for names in R.SUBSETS[1:]:
                part = _abi_backward(abi, case, xd, wd, gy, y, names)
                for k in names:
                    assert torch.equal(part[k], full[k]), f'{k} of n={n} cout={cout}: asked {names} differs from the all-three run'


# ---- affine bank --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.BANK_CASES, ids=R.bank_id)
def test_affine_bank_every_output(case):
    from afcm_amd.torch_utils.ops import affine_bank as ab
    b = R.affine_bank_case(case)
    fcs = [types.SimpleNamespace(weight=_dev(W, True), bias=_dev(bs, True), weight_gain=wg, bias_gain=bg, activation='linear')
           for W, bs, wg, bg in zip(b.W, b.b, b.wgain, b.bgain)]
    specs = [ab.Spec(fc, i, sc) for fc, i, sc in zip(fcs, b.idx, b.scale)]
    ws, g = _dev(b.ws, True), _dev(b.g, True)
    assert ab.supported(ws, g, specs)
    ys = ab.affine_bank(ws, g, specs)
    what = R.bank_id(case)
    for l, y in enumerate(ys):
        R.assert_exact(y, b.y[l], f'styles {l} of {what}')
    used = [l for l, d in enumerate(b.dy) if d is not None]
    ins = [ws] + ([g] if g is not None else []) + [fc.weight for fc in fcs] + [fc.bias for fc in fcs]
    grads = list(torch.autograd.grad([ys[l] for l in used], ins, [_dev(b.dy[l]) for l in used], allow_unused=True))
    want = [b.dws] + ([b.dg] if g is not None else []) + b.dW + b.db
    names = ['d ws'] + (['d global_w'] if g is not None else []) + [f'dW {l}' for l in range(len(fcs))] + [f'db {l}' for l in range(len(fcs))]
    for nm, a, e in zip(names, grads, want):
        if a is None:
            assert float(e.abs().max()) == 0.0, f'{nm} of {what} is absent'
        else:
            R.assert_exact(a, e, f'{nm} of {what}')


# ---- mapping input stage: per-row bars ------------------------------------------------------------------------------------------------------
def _rows_close(got, ref, tol, what, scale=None):
    """max|err| over each row (last dimension) against ``tol`` times that row's own max|ref| (or the given per-row scale); a row whose
    reference is all zero must be exactly zero."""
    got, ref = got.detach().double().cpu(), ref.detach().double()
    assert got.shape == ref.shape, what
    err = (got - ref).abs().reshape(ref.shape[0], -1).amax(1)
    sc = ref.abs().reshape(ref.shape[0], -1).amax(1) if scale is None else scale.double()
    ratio = torch.where(sc > 0, err / sc.clamp_min(1e-300), torch.where(err > 0, torch.tensor(float('inf'), dtype=torch.float64), torch.zeros_like(err)))
    worst = int(ratio.argmax())
    print(f'{what}: worst row {worst}: {float(ratio[worst]):.3e} of its scale {float(sc[worst]):.3e} (bar {tol:.1e})')
    assert float(ratio[worst]) <= tol, f'{what}: row {worst} is off by {float(ratio[worst]):.3e} of its own scale {float(sc[worst]):.3e} (tolerance {tol:.1e})'


@pytest.mark.parametrize('zero_bias', [True, False], ids=['zero-bias', 'bias'])
@pytest.mark.parametrize('n', [1, 5])
@pytest.mark.parametrize('zdim,cdim,wdim', [(33, 7, 36), (512, 1, 512), (300, 4, 260)], ids=str)
def test_mapping_input_rows_vs_float64(zdim, cdim, wdim, n, zero_bias):
    """n = 5: sample 0 ordinary, 1 scaled by 1e3, 2 by 1e-3 (z and c), 3 with z = 1e-5 randn (eps dominates the mean square), 4 with
    z = 0 and c = 0.  n = 1: an ordinary sample, or (zero bias) sample 4 alone.  With a zero bias the embedding of the c = 0 sample is
    exactly zero: its part of x0 must be exact zeros, its ge = rsqrt(1e-8) g = 1e4 g goes into deb and nothing of it into dew."""
    from afcm_amd.networks_stylegan3 import FullyConnectedLayer
    fc_bank = _fc()
    torch.manual_seed(zdim + 3 * cdim + wdim + n)
    z, c = torch.randn(n, zdim), torch.rand(n, cdim)
    if n == 5:
        z[1] *= 1e3; c[1] *= 1e3; z[2] *= 1e-3; c[2] *= 1e-3; z[3] *= 1e-5
    zero = 4 if n == 5 else (0 if zero_bias else None)
    if zero is not None:
        z[zero] = 0.0; c[zero] = 0.0
    embed = FullyConnectedLayer(cdim, wdim).cuda()
    if not zero_bias:
        with torch.no_grad():
            embed.bias.add_(torch.randn_like(embed.bias) * 0.3)
    z, c = z.cuda(), c.cuda()
    assert fc_bank.mapping_input_supported(z, c, embed)
    x0 = fc_bank.mapping_input(z, c, embed)
    x0v = x0.detach()
    zd = z.double().cpu()
    wd, bd = embed.weight.detach().double().cpu().requires_grad_(True), embed.bias.detach().double().cpu().requires_grad_(True)
    e = c.double().cpu() @ (wd * embed.weight_gain).t() + bd * embed.bias_gain
    want = torch.cat([zd * (zd.square().mean(1, keepdim=True) + 1e-8).rsqrt(), e * (e.square().mean(1, keepdim=True) + 1e-8).rsqrt()], 1)
    r = torch.randn(want.shape).double()                                   # (an fp32 cotangent: both sides see the same numbers)
    ge, dew, deb = torch.autograd.grad((want * r).sum(), [e, wd, bd])
    what = f'z{zdim} c{cdim} w{wdim} n{n}'
    _rows_close(x0[:, :zdim], want[:, :zdim], 1e-5, 'normalised z of ' + what)
    _rows_close(x0[:, zdim:], want[:, zdim:], 1e-5, 'normalised embedding of ' + what)
    if zero is not None:
        assert float(x0v[zero, :zdim].abs().max()) == 0.0
        if zero_bias:
            assert float(x0v[zero, zdim:].abs().max()) == 0.0
            assert torch.allclose(ge[zero], 1e4 * r[zero, zdim:], rtol=1e-9, atol=0.0)                # (the reference itself)
    got_w, got_b = torch.autograd.grad((x0 * r.float().cuda()).sum(), [embed.weight, embed.bias])
    _rows_close(got_w, dew, 3e-5, 'dew of ' + what)
    _rows_close(got_b[:, None], deb[:, None], 3e-5, 'deb of ' + what, scale=embed.bias_gain * ge.abs().amax(0))
