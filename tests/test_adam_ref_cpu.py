"""CPU tests of tests/adam_ref.py: the float64 run reproduces torch.nan_to_num + torch.optim.Adam in float64, the float32 run reproduces
torch.optim.Adam in float32 to one ulp, the slice layout of the alignment cases keeps its gaps, and every case table of
tests/test_gpu_optim_edges.py has teeth -- a step count off by one, a count that replays do not advance, a missing bias_correction2, the
scrub applied before grad_scale, or posinf and neginf swapped moves the float64 reference by at least 10x the error that GPU test
allows.  The last is what makes the GPU bounds meaningful, and it needs no GPU."""
import math

import pytest
import torch

import adam_ref as R


def _torch_adam(case, dtype):
    """nan_to_num(g * grad_scale) + torch.optim.Adam, per step: lists of p, exp_avg, exp_avg_sq."""
    kw = case['kw']
    ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in case['p0s']]
    opt = torch.optim.Adam(ps, lr=kw['lr'], betas=kw['betas'], eps=kw['eps'])
    out = []
    for grads in case['sched']:
        for p, g in zip(ps, grads):
            g = g.to(dtype) * kw.get('grad_scale', 1.0)
            p.grad = torch.nan_to_num(g, nan=0.0, posinf=kw.get('posinf', 1e5), neginf=kw.get('neginf', -1e5))
        opt.step()
        out.append(([p.detach().clone() for p in ps], [opt.state[p]['exp_avg'].clone() for p in ps], [opt.state[p]['exp_avg_sq'].clone() for p in ps]))
    return out


def _dense_cases():
    """The cases in which every parameter has a gradient at every step and the scrub is on: there the group-wide count is torch's."""
    out = [('a-%s-%g' % (b[0], lr), R.case_a(b, lr)) for b, lr in R.A_CASES]
    out += [('d-%s' % b[0], R.case_d(b)) for b in R.BETAS]
    out += [('g-%s-%g-%s' % (s, sc, b[0]), R.case_g(s, sc, b)) for s, sc, b in R.G_CASES if s != 'off']
    return out


DENSE = _dense_cases()


@pytest.mark.parametrize('name,case', DENSE, ids=[n for n, _ in DENSE])
def test_float64_run_equals_torch_adam_float64(name, case):
    mine = R.adam_run(case['p0s'], case['sched'], dtype=torch.float64, **case['kw'])
    for k, (step, ref) in enumerate(zip(mine, _torch_adam(case, torch.float64))):
        for key, xs in zip(('p', 'm', 'v'), ref):
            for i, x in enumerate(xs):
                got = getattr(step, key)[i]
                assert bool(torch.isfinite(got).all())
                err = (got - x).abs().max().item()
                assert err <= 1e-13 * x.abs().max().item(), (k, key, i, err)
        assert step.count == [k + 1] * len(case['p0s'])


@pytest.mark.parametrize('name,case', DENSE, ids=[n for n, _ in DENSE])
def test_float32_run_equals_torch_adam_float32_to_one_ulp(name, case):
    mine = R.adam_run(case['p0s'], case['sched'], dtype=torch.float32, **case['kw'])
    for k, (step, ref) in enumerate(zip(mine, _torch_adam(case, torch.float32))):
        for key, xs in zip(('p', 'm', 'v'), ref):
            for i, x in enumerate(xs):
                got = getattr(step, key)[i]
                assert got.dtype == torch.float32
                # one ulp of each element: the spacing of float32 at |x| (the smallest subnormal at 0)
                ulp = torch.maximum(torch.nextafter(x.abs(), torch.full_like(x, math.inf)) - x.abs(), torch.full_like(x, 2.0 ** -149))
                assert bool(((got - x).abs() <= ulp).all()), (k, key, i, ((got - x).abs() / ulp).max().item())


def test_group_count_and_untouched_parameters():
    """One count per group, the largest + 1; a parameter without a gradient keeps its bits and its count."""
    case = R.case_f(R.BETAS[1], R.LR_TIGHT)
    run = R.adam_run(case['p0s'], case['sched'], dtype=torch.float64, **case['kw'])
    assert [s.count[R.F_SOMETIMES] for s in run] == [0, 2, 2, 4, 4]
    assert [s.count[R.F_NEVER] for s in run] == [0] * R.F_STEPS
    assert [s.count[0] for s in run] == [1, 2, 3, 4, 5]
    p0 = case['p0s'][R.F_NEVER].double()
    for k, s in enumerate(run):
        assert torch.equal(s.p[R.F_NEVER], p0) and not s.m[R.F_NEVER].any() and not s.v[R.F_NEVER].any()
        if k in (2, 4):
            for key in ('p', 'm', 'v'):
                assert torch.equal(getattr(s, key)[R.F_SOMETIMES], getattr(run[k - 1], key)[R.F_SOMETIMES])
    # the sometimes-parameter's step 2 uses the group's count 2, not a count of its own (1): one dense tensor stepped with that count
    solo = R.adam_run([case['p0s'][R.F_SOMETIMES]], [[case['sched'][1][R.F_SOMETIMES]]], dtype=torch.float64, fault='count+1', **case['kw'])
    assert torch.equal(solo[0].p[0], run[1].p[R.F_SOMETIMES])


def test_scrub_order_and_values():
    g = torch.tensor([float('nan'), float('inf'), float('-inf'), -0.0, 1e-30, 2.0], dtype=torch.float32)
    out = R.scrubbed_grad(g, 0.125, True, 7.0, -3.0, torch.float32)
    assert R.bits(out).tolist() == R.bits(torch.tensor([0.0, 7.0, -3.0, -0.0, 1.25e-31, 0.25], dtype=torch.float32)).tolist()
    assert R.scrubbed_grad(g, 0.125, True, 7.0, -3.0, torch.float32, fault='scrub_first')[1].item() == 0.875
    assert R.scrubbed_grad(g, 0.125, True, 7.0, -3.0, torch.float32, fault='inf_swapped')[1].item() == -3.0
    off = R.scrubbed_grad(g, 0.125, False, 7.0, -3.0, torch.float64)
    assert bool(off[0].isnan()) and off[1].item() == math.inf and off[2].item() == -math.inf


@pytest.mark.parametrize('offset', sorted({o for pair in R.D_OFFSETS for o in pair}))
def test_alignment_layout_keeps_its_gaps(offset):
    starts, total = R.d_layout(offset)
    edges = [0] + [x for s, n in zip(starts, R.D_SIZES) for x in (s, s + n)] + [total]
    assert all(s % 4 == offset for s in starts)
    assert all(edges[i + 1] - edges[i] >= R.D_GAP for i in range(0, len(edges), 2)), 'gaps between slices and at both ends'
    assert {(p, g) for p, g in R.D_OFFSETS} == {(0, 0), (0, 1), (3, 0), (2, 2), (1, 3)}


def test_scrub_matrix_places_every_special_value_in_the_tail():
    case = R.case_g('default', 1.0, R.BETAS[0])
    tail = []
    for grads in case['sched'][:R.G_SPECIAL_STEPS]:
        big, small = grads
        assert R.bits(big[:7]).tolist() == R.bits(small).tolist() == R.bits(big[8192:8199]).tolist()
        tail += R.bits(big[-3:]).tolist()
    assert set(tail) == set(R.bits(torch.tensor(R.G_SPECIALS, dtype=torch.float32)).tolist())
    finite = torch.cat([g[torch.isfinite(g)] for grads in case['sched'] for g in grads])
    assert finite.abs().max().item() <= 1e15


TEETH = [(name, case, frozen, fault) for name, case, frozen, faults in R.teeth_cases() for fault in faults]


def test_every_fault_is_tried_on_some_table():
    assert {f for _, _, _, f in TEETH} == set(R.FAULTS)
    assert {n.split('-')[0] for n, _, _, _ in TEETH} == set('abcdefg')


@pytest.mark.parametrize('name,case,frozen,fault', TEETH, ids=['%s-%s' % (n, f) for n, _, _, f in TEETH])
def test_case_tables_have_teeth(name, case, frozen, fault):
    """For every tensor the fault can reach, some step and one of p, m, v moves by >= 10x the bound of that tensor at that step.  The
    count faults and the missing bias correction reach every tensor that has a gradient once the count is wrong; the scrub faults
    reach the tensors with an infinite gradient (all of the scrub matrix's)."""
    run32, run64 = R.run_both(case)
    bad = R.adam_run(case['p0s'], case['sched'], dtype=torch.float64, fault='frozen:%d' % frozen if fault == 'frozen' else fault, **case['kw'])
    first_wrong = frozen if fault == 'frozen' else 0          # index of the first step whose count differs
    for i in range(len(case['p0s'])):
        if not any(grads[i] is not None for grads in case['sched'][first_wrong:]):
            continue
        best = 0.0
        for s32, s64, sb in zip(run32, run64, bad):
            for key in ('p', 'm', 'v'):
                x32, x64, xb = getattr(s32, key)[i], getattr(s64, key)[i], getattr(sb, key)[i]
                both = torch.isfinite(x64) & torch.isfinite(xb)
                move = (xb[both] - x64[both]).abs().max().item() if bool(both.any()) else 0.0
                if move > 0:
                    best = max(best, move / R.bound(x32, x64))
        assert best >= R.TEETH, 'tensor %d (%d elements): the fault moves the reference by only %.2f x the bound' % (i, case['p0s'][i].numel(), best)
