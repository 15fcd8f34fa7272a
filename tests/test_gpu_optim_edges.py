"""afcm_amd.optim (C ABI afcm_adam_multi / afcm_adam_multi_capturable, afcm_l1_partials / afcm_l1_grad) at its edges, against the float64
restatement of the update rule in tests/adam_ref.py: the graph-capturable path eagerly and replayed from a graph, the step count across
checkpoints, unaligned slices with guard words, the table search over 130 tensors in two groups, gradient sets that change between
steps, the scrub matrix, and weighted_l1 at its block-count thresholds.

Tolerance everywhere: per tensor and per step, E_k <= 2 * E_t + 2**-23 * max|x64| for x in p, m, v, where E_t is the error of the float32
run of the same rule (adam_ref.Comparison); tests/test_adam_ref_cpu.py shows that a wrong step count, a missing bias correction or a
misplaced scrub moves the reference by at least 10x that.  Every test prints its largest E_k / E_t and E_k / bound (run with -s).  One
run on an MI355X gave, as the largest E_k / E_t (largest E_k / bound) of each table; the median E_k / E_t is 1.00 everywhere, the large
ratios belong to tensors whose E_t is far below one ulp of their largest element:
    (a) capturable eager     3.00 (0.73)      (e) 130 tensors, both modes   125.89 (0.73); one tensor 1.00 (0.26)
    (b) captured step        2.85 (0.48)      (f) changing gradient sets    3.42 (0.71)
    (c) load_state_dict      1.13 (0.36)      (g) scrub matrix              1.98 (0.57)
    (d) slices and tails     3.57 (0.46)      (h) weighted_l1 relative error <= 9.6e-8
Before the fixes that came with these tests: (a) 1255 (92.4) at betas (0.9, 0.999) and 52.7 (6.2) at (0, 0.99), from 1.f - beta in the
capturable entry point; (b) state_dict() reported step 3 after 6 steps; (c) device_step() 6 instead of 3, 1834 (432); (e) 125.89 (1.85), an
unfused product in the kernel's lerp.
"""
import copy
import functools

import pytest
import torch

import adam_ref as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _ref(table, *key):
    """(case, float32 run, float64 run) of one row of a case table: computed once, shared by the tests that use it, never modified."""
    case = getattr(R, 'case_' + table)(*key)
    return (case,) + R.run_both(case)


def _params(p0s):
    return [torch.nn.Parameter(p.clone().cuda()) for p in p0s]


def _set_grads(ps, grads):
    for p, g in zip(ps, grads):
        p.grad = None if g is None else g.clone().cuda()


def _state(opt, ps):
    zeros = [torch.zeros_like(p) for p in ps]
    return dict(p=ps, m=[opt.state[p].get('exp_avg', z) for p, z in zip(ps, zeros)], v=[opt.state[p].get('exp_avg_sq', z) for p, z in zip(ps, zeros)])


def _host_steps(opt, ps):
    return [float(opt.state[p]['step']) if 'step' in opt.state[p] else 0.0 for p in ps]


# ------------------------------------------------------------------------------------------------- (a) capturable, eager
@pytest.mark.parametrize('betas,lr', R.A_CASES, ids=str)
def test_capturable_eager_steps_vs_float64(betas, lr):
    """Six eager steps of the capturable path (the count on the device, the bias corrections formed in the kernel), a fresh gradient at every
    step."""
    from afcm_amd.optim import FusedScrubAdam
    case, r32, r64 = _ref('a', betas, lr)
    ps = _params(case['p0s'])
    opt = FusedScrubAdam(ps, lr=lr, betas=betas, eps=R.EPS, capturable=True)
    cmp = R.Comparison('capturable eager %s lr %g' % (betas, lr))
    for k, grads in enumerate(case['sched']):
        _set_grads(ps, grads)
        opt.step()
        cmp.add(_state(opt, ps), r32[k], r64[k], 'step %d' % (k + 1))
    cmp.finish()
    assert opt.device_step() == R.A_STEPS
    assert _host_steps(opt, ps) == [float(R.A_STEPS)] * len(ps)


# ------------------------------------------------------------------------------------------------- (b) capturable, in a graph
@pytest.mark.parametrize('betas,lr', R.B_CASES, ids=str)
def test_captured_optimizer_step_vs_float64_and_checkpoint(betas, lr):
    """The optimizer step alone in a graph (one chain of two kernels): two eager steps on a side stream, the capture (which does not run the
    step), four replays with a different gradient copied into the static gradient tensors before each.  Every step against the float64
    run; then the checkpoint: state_dict() reports step 6 for every parameter, and a fresh non-capturable FusedScrubAdam and a
    torch.optim.Adam that load it land on the reference's 7th step."""
    from afcm_amd.optim import FusedScrubAdam
    case, r32, r64 = _ref('b', betas, lr)
    sched = case['sched']
    ps = _params(case['p0s'])
    opt = FusedScrubAdam(ps, lr=lr, betas=betas, eps=R.EPS, capturable=True)
    static = [torch.zeros_like(p) for p in ps]
    for p, g in zip(ps, static):
        p.grad = g
    cmp = R.Comparison('captured step %s lr %g' % (betas, lr))

    def load(k):
        for s, g in zip(static, sched[k]):
            s.copy_(g)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for k in range(R.B_EAGER):
            load(k)
            opt.step()
            cmp.add(_state(opt, ps), r32[k], r64[k], 'eager step %d' % (k + 1))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode='thread_local'):
        opt.step()
    assert opt.device_step() == R.B_EAGER, 'the capture records the step, it does not run it'
    for k in range(R.B_EAGER, R.B_EAGER + R.B_REPLAYS):
        load(k)
        graph.replay()
        cmp.add(_state(opt, ps), r32[k], r64[k], 'replay %d (step %d)' % (k - R.B_EAGER + 1, k + 1))
    torch.cuda.synchronize()
    total = R.B_EAGER + R.B_REPLAYS
    assert opt.device_step() == total

    sd = opt.state_dict()
    steps = [float(sd['state'][i]['step']) for i in range(len(ps))]
    print('state_dict() steps after %d eager steps + %d replays: %s' % (R.B_EAGER, R.B_REPLAYS, steps))
    assert steps == [float(total)] * len(ps), 'state_dict() of a capturable optimizer must carry the device count'
    for name, make in (('FusedScrubAdam', lambda q: FusedScrubAdam(q, lr=lr, betas=betas, eps=R.EPS)),
                       ('torch.optim.Adam', lambda q: torch.optim.Adam(q, lr=lr, betas=betas, eps=R.EPS))):
        qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
        reader = make(qs)
        loaded = copy.deepcopy(sd)
        for group in loaded['param_groups']:
            for key, value in reader.defaults.items():       # (torch.optim.Adam's own switches, which the checkpoint does not carry)
                group.setdefault(key, value)
        reader.load_state_dict(loaded)
        _set_grads(qs, sched[total])
        reader.step()
        got = dict(p=qs, m=[reader.state[q]['exp_avg'] for q in qs], v=[reader.state[q]['exp_avg_sq'] for q in qs])
        cmp.add(got, r32[total], r64[total], 'step %d by %s from the checkpoint' % (total + 1, name))
    del graph
    cmp.finish()


# ------------------------------------------------------------------------------------------------- (c) load_state_dict
@pytest.mark.parametrize('betas,lr', R.C_CASES, ids=str)
def test_load_state_dict_into_a_capturable_optimizer_that_has_stepped(betas, lr):
    """A capturable optimizer that has run 5 steps loads the state of one that ran 2 (and takes its parameter values): the next step is the
    donor's 3rd, on the device as well."""
    from afcm_amd.optim import FusedScrubAdam
    case, r32, r64 = _ref('c', betas, lr)
    recv, _, _ = _ref('c_receiver', betas, lr)
    pa = _params(recv['p0s'])
    opt_a = FusedScrubAdam(pa, lr=lr, betas=betas, eps=R.EPS, capturable=True)
    for grads in recv['sched']:
        _set_grads(pa, grads)
        opt_a.step()
    assert opt_a.device_step() == R.C_RECEIVER
    pb = _params(case['p0s'])
    opt_b = FusedScrubAdam(pb, lr=lr, betas=betas, eps=R.EPS)
    for grads in case['sched'][:R.C_DONOR]:
        _set_grads(pb, grads)
        opt_b.step()
    opt_a.load_state_dict(copy.deepcopy(opt_b.state_dict()))
    with torch.no_grad():
        for a, b in zip(pa, pb):
            a.copy_(b)
    _set_grads(pa, case['sched'][R.C_DONOR])
    opt_a.step()
    cmp = R.Comparison('load_state_dict %s lr %g' % (betas, lr))
    cmp.add(_state(opt_a, pa), r32[R.C_DONOR], r64[R.C_DONOR], 'step %d after the load' % (R.C_DONOR + 1))
    print('device_step() after the load and one step: %d' % opt_a.device_step())
    cmp.finish()
    assert opt_a.device_step() == R.C_DONOR + 1
    assert _host_steps(opt_a, pa) == [float(R.C_DONOR + 1)] * len(pa)


# ------------------------------------------------------------------------------------------------- (d) alignment and tails
@pytest.mark.parametrize('offsets,betas,write_grad', R.D_CASES, ids=str)
def test_unaligned_slices_and_tails_keep_their_guards(offsets, betas, write_grad):
    """Parameters are views of one flat buffer, gradients slices of a second one (grads=), at the given element offsets modulo 4: (0, 0) takes
    the float4 branch with its scalar tails, every other pair the scalar branch (which reads m when beta1 != 0).  The sentinel words between
    the slices and at both ends of both buffers keep their bits through every step."""
    from afcm_amd.optim import FusedScrubAdam
    case, r32, r64 = _ref('d', betas)
    (po, go) = offsets
    flats, views, masks = [], [], []
    for off in (po, go):
        starts, total = R.d_layout(off)
        flat = torch.empty(total, dtype=torch.float32, device='cuda')
        assert flat.data_ptr() % 16 == 0
        flat.view(torch.int32).fill_(R.SENTINEL)
        mask = torch.ones(total, dtype=torch.bool)
        for s, n in zip(starts, R.D_SIZES):
            mask[s:s + n] = False
        flats.append(flat)
        views.append([flat[s:s + n] for s, n in zip(starts, R.D_SIZES)])
        masks.append(mask)
    ps = [torch.nn.Parameter(v) for v in views[0]]
    with torch.no_grad():
        for p, p0 in zip(ps, case['p0s']):
            p.copy_(p0)
    assert all(p.data_ptr() // 4 % 4 == po for p in ps) and all(g.data_ptr() // 4 % 4 == go for g in views[1])
    grads = dict(zip(ps, views[1]))
    opt = FusedScrubAdam(ps, lr=case['kw']['lr'], betas=betas, eps=R.EPS, write_grad=write_grad)
    cmp = R.Comparison('slices at %s %s write_grad %s' % (offsets, betas, write_grad))
    for k in range(R.D_STEPS):
        for v, g in zip(views[1], case['sched'][k]):
            v.copy_(g)
        opt.step(grads=grads)
        cmp.add(_state(opt, ps), r32[k], r64[k], 'step %d' % (k + 1))
        for name, flat, mask in zip(('parameter', 'gradient'), flats, masks):
            guards = R.bits(flat)[mask]
            assert bool((guards == R.SENTINEL).all()), '%s buffer, step %d: %d guard words overwritten' % (name, k + 1, int((guards != R.SENTINEL).sum()))
        for i, (v, g) in enumerate(zip(views[1], case['sched'][k])):
            # (grad_scale is 1 and the values are finite: written back or not, the slice holds the gradient's bits)
            assert torch.equal(R.bits(v), R.bits(g)), 'gradient slice %d, step %d' % (i, k + 1)
        assert all(p.grad is None for p in ps)
    cmp.finish()


# ------------------------------------------------------------------------------------------------- (e) table search and groups
@pytest.mark.parametrize('capturable', [False, True], ids=['host-count', 'capturable'])
@pytest.mark.parametrize('which', list(R.E_SIZES), ids=['130-tensors', '1-tensor'])
def test_table_search_and_two_groups(which, capturable):
    """130 tensors of 1 .. 40000 elements (one to three chunks each) in two parameter groups with their own lr and betas, and one 1-element
    tensor on its own: every chunk finds its tensor, every group its hyper-parameters and its count."""
    from afcm_amd.optim import FusedScrubAdam
    refs = [_ref('e', which, g) if R.e_split(which)[g] else None for g in (0, 1)]
    groups, params = [], []
    for g, ref in enumerate(refs):
        params.append(_params(ref[0]['p0s']) if ref is not None else [])
        if ref is not None:
            groups.append(dict(params=params[g], **R.E_GROUPS[g]))
    opt = FusedScrubAdam(groups, eps=R.EPS, capturable=capturable)
    cmp = R.Comparison('%s tensors, %s' % (which, 'capturable' if capturable else 'host count'))
    for k in range(R.E_STEPS):
        for g, ref in enumerate(refs):
            if ref is not None:
                _set_grads(params[g], ref[0]['sched'][k])
        opt.step()
        for g, ref in enumerate(refs):
            if ref is not None:
                cmp.add(_state(opt, params[g]), ref[1][k], ref[2][k], 'group %d step %d' % (g, k + 1))
    cmp.finish()
    for gi, group in enumerate(opt.param_groups):
        assert _host_steps(opt, group['params']) == [float(R.E_STEPS)] * len(group['params'])
        if capturable:
            assert opt.device_step(gi) == R.E_STEPS


# ------------------------------------------------------------------------------------------------- (f) changing gradient sets
@pytest.mark.parametrize('capturable', [False, True], ids=['host-count', 'capturable'])
@pytest.mark.parametrize('betas,lr', R.F_CASES, ids=str)
def test_changing_gradient_sets(betas, lr, capturable):
    """Five parameters, five steps: one has a gradient at steps 2 and 4 only, one never (the pointer table is rebuilt at every step; in
    capturable mode it is rewritten in place).  The group-wide count applies; a parameter without a gradient keeps the bits of p, m, v."""
    from afcm_amd.optim import FusedScrubAdam
    case, r32, r64 = _ref('f', betas, lr)
    ps = _params(case['p0s'])
    opt = FusedScrubAdam(ps, lr=lr, betas=betas, eps=R.EPS, capturable=capturable)
    cmp = R.Comparison('changing gradient sets %s, %s' % (betas, 'capturable' if capturable else 'host count'))
    never0 = R.bits(ps[R.F_NEVER])
    for k, grads in enumerate(case['sched']):
        before = {key: R.bits(x[R.F_SOMETIMES]) for key, x in _state(opt, ps).items()}
        _set_grads(ps, grads)
        opt.step()
        now = _state(opt, ps)
        cmp.add(now, r32[k], r64[k], 'step %d' % (k + 1))
        if grads[R.F_SOMETIMES] is None:
            for key in ('p', 'm', 'v'):
                assert torch.equal(R.bits(now[key][R.F_SOMETIMES]), before[key]), 'step %d: %s of the skipped parameter changed' % (k + 1, key)
        assert torch.equal(R.bits(ps[R.F_NEVER]), never0)
        assert not bool(now['m'][R.F_NEVER].any()) and not bool(now['v'][R.F_NEVER].any())
        assert _host_steps(opt, ps) == [float(c) for c in r64[k].count], 'step %d' % (k + 1)
    cmp.finish()
    if capturable:
        assert opt.device_step() == R.F_STEPS


# ------------------------------------------------------------------------------------------------- (g) scrub matrix
@pytest.mark.parametrize('capturable', [False, True], ids=['host-count', 'capturable'])
@pytest.mark.parametrize('write_grad', [False, True], ids=['keep-grad', 'write-grad'])
@pytest.mark.parametrize('scrub,scale,betas', R.G_CASES, ids=str)
def test_scrub_matrix(scrub, scale, betas, write_grad, capturable):
    """nan, +inf, -inf, -0.0, 1e-30, 1e5, 1e15 at the head, in the middle and in the last three elements, scaled by grad_scale and then
    scrubbed (default bounds, custom bounds, or not at all).  Without the scrub p is NaN exactly where the float64 run is.  p.grad holds
    the float32 nan_to_num(g * scale) afterwards with write_grad, its own bits (NaN payloads included) without."""
    from afcm_amd.optim import FusedScrubAdam
    case, r32, r64 = _ref('g', scrub, scale, betas)
    kw = case['kw']
    hyper = {k: kw[k] for k in ('scrub', 'posinf', 'neginf') if k in kw}
    ps = _params(case['p0s'])
    opt = FusedScrubAdam(ps, lr=kw['lr'], betas=betas, eps=R.EPS, write_grad=write_grad, capturable=capturable, **hyper)
    cmp = R.Comparison('scrub %s scale %g %s' % (scrub, scale, betas))
    for k, grads in enumerate(case['sched']):
        _set_grads(ps, grads)
        opt.step(grad_scale=scale)
        cmp.add(_state(opt, ps), r32[k], r64[k], 'step %d' % (k + 1))
        for i, (p, g) in enumerate(zip(ps, grads)):
            nan64 = torch.isnan(r64[k].p[i])
            assert torch.equal(torch.isnan(p).cpu(), nan64) and bool(torch.isfinite(p).cpu()[~nan64].all()), 'step %d tensor %d: p is NaN elsewhere than the float64 run' % (k + 1, i)
            assert scrub == 'off' or not bool(nan64.any())
            if write_grad:
                want = R.scrubbed_grad(g, scale, dtype=torch.float32, **hyper)
                keep = ~torch.isnan(want)                # (only without the scrub: a NaN stays one, whatever its payload)
                assert torch.equal(torch.isnan(p.grad).cpu(), ~keep)
                assert torch.equal(R.bits(p.grad)[keep], R.bits(want)[keep]), 'step %d tensor %d: scrubbed gradient written back' % (k + 1, i)
            else:
                assert torch.equal(R.bits(p.grad), R.bits(g)), 'step %d tensor %d: gradient left as it was' % (k + 1, i)
    cmp.finish()


# ------------------------------------------------------------------------------------------------- (h) weighted_l1
L1_WEIGHT = 100.0
L1_SIZES = [4095, 4096, 4097, 256 * 4096, 256 * 4096 + 1]      # one block | two blocks from 4097 | 256 blocks, the cap | more elements per thread


def _l1_inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    a.view(-1)[0] = b.view(-1)[0]                              # an exact tie: gradient 0
    return a, b


def _l1_float64(a, b):
    return ((a.double() - b.double()).abs().mean() * L1_WEIGHT).item()


def _l1_grad32(a, b):
    """sign(a - b) * weight / numel in float32."""
    a, b = torch.broadcast_tensors(a, b)
    return torch.sign(a - b) * torch.tensor(L1_WEIGHT, dtype=torch.float32) / torch.tensor(float(a.numel()), dtype=torch.float32)


@pytest.mark.parametrize('numel', L1_SIZES)
def test_weighted_l1_vs_float64_at_the_block_thresholds(numel):
    """Each thread adds at most 17 terms and about 20 tree additions follow: the worst case is below 3e-6 relative, the bound stays 1e-5."""
    from afcm_amd.optim import weighted_l1
    a, b = _l1_inputs((numel,), numel)
    want = _l1_float64(a, b)
    ag = a.cuda().requires_grad_(True)
    got = weighted_l1(ag, b.cuda(), L1_WEIGHT)
    assert type(got.grad_fn).__name__ == '_WeightedL1Backward'
    ga, = torch.autograd.grad(got, [ag])
    print('weighted_l1 %d elements: relative error %.2e' % (numel, abs(got.item() - want) / want))
    assert got.shape == () and abs(got.item() - want) <= 1e-5 * abs(want)
    assert torch.equal(R.bits(ga), R.bits(_l1_grad32(a, b))) and float(ga[0]) == 0.0


@pytest.mark.parametrize('kind', ['a-non-contiguous', 'b-non-contiguous', 'b-requires-grad', 'unequal-shapes'])
def test_weighted_l1_outside_the_fused_form(kind):
    """Inputs the fused kernels do not take as they are: the result is still L1Loss()(a, b) * weight against float64, the gradients are
    sign(a - b) * weight / numel.  A gradient for b and unequal shapes go through the op-by-op composition; a non-contiguous input of the
    same shape is served by the fused kernels on a contiguous copy (weighted_l1's gate does not ask for contiguity)."""
    from afcm_amd.optim import weighted_l1
    shape = (3, 37, 70)
    a, b = _l1_inputs(shape, 5)
    if kind == 'a-non-contiguous':
        a = a.transpose(1, 2)
        b = b.transpose(1, 2).contiguous()
    elif kind == 'b-non-contiguous':
        b = b.transpose(1, 2)
        a = a.transpose(1, 2).contiguous()
    elif kind == 'unequal-shapes':
        b = b[:1]
    ad = a.cuda() if a.is_contiguous() else a.transpose(1, 2).contiguous().cuda().transpose(1, 2)
    bd = b.cuda() if b.is_contiguous() else b.transpose(1, 2).contiguous().cuda().transpose(1, 2)
    assert ad.is_contiguous() == a.is_contiguous() and bd.is_contiguous() == b.is_contiguous()
    ad.requires_grad_(True)
    bd.requires_grad_(kind == 'b-requires-grad')
    got = weighted_l1(ad, bd, L1_WEIGHT)
    want = _l1_float64(*torch.broadcast_tensors(a, b))
    assert got.shape == () and abs(got.item() - want) <= 1e-5 * abs(want)
    ref = torch.nn.L1Loss()(ad.detach(), bd.detach()) * L1_WEIGHT
    assert abs(got.item() - ref.item()) <= 1e-5 * abs(want)
    if kind in ('b-requires-grad', 'unequal-shapes'):
        assert type(got.grad_fn).__name__ != '_WeightedL1Backward', 'the op-by-op composition'
    want_ga = _l1_grad32(a, b)
    if kind == 'b-requires-grad':
        ga, gb = torch.autograd.grad(got, [ad, bd])
        assert torch.allclose(gb.cpu(), -want_ga, rtol=1e-6, atol=0)
    else:
        ga, = torch.autograd.grad(got, [ad])
    assert ga.shape == ad.shape and torch.allclose(ga.cpu(), want_ga, rtol=1e-6, atol=0)
    if type(got.grad_fn).__name__ == '_WeightedL1Backward':
        assert torch.equal(R.bits(ga), R.bits(want_ga)), 'the fused gradient is sign(a - b) * weight / numel to the bit'
