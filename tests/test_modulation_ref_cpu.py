"""The modulation kernels' suite without a GPU: the float64 restatement of tests/modulation_ref.py against a case worked by hand and against float64
autograd of the composed NET:41-57 expression; the case tables against the kernels' class and chunk decisions, recomputed here in integers; the floor
inputs' window; the refusals of the six entry points (they return before any launch); and the measurement of the bars -- the float32 eager
composition against float64 over every case and gradient set.  tests/test_gpu_modulation.py holds the kernels to the same restatement."""
import ctypes
import os

import pytest
import torch

import modulation_ref as M

F32, F64 = M.F32, M.F64


@pytest.fixture(scope='module')
def lib():
    from afcm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def test_restatement_on_a_case_worked_by_hand():
    """cout = cin = 2, k = 1, n = 2.  Row 0 of w is (3, 4): mean square 12.5, so w_hat = (3, 4) / sqrt(12.5) and wsq = (0.72, 1.28); row 1 is (1, -1):
    scale 1, wsq = (1, 1).  Styles (1, 2) and (0, 0): mean square 5 / 4, s_hat^2 = (0.8, 3.2) and (0, 0), so q = (0.8 * 0.72 + 3.2 * 1.28, 0.8 + 3.2) =
    (4.672, 4) for sample 0 and (0, 0) for sample 1.  magnitude 4: gain 1 / 2."""
    w = torch.tensor([[3.0, 4.0], [1.0, -1.0]], dtype=F64).reshape(2, 2, 1, 1)
    t = torch.tensor([[1.0, 2.0], [0.0, 0.0]], dtype=F64)
    w_hat, wsq, scale = M.weight_norm(w)
    close = lambda a, b: torch.allclose(a, torch.tensor(b, dtype=F64).reshape(a.shape), rtol=1e-14, atol=0)
    assert close(scale, [12.5 ** -0.5, 1.0]) and close(w_hat, [3 / 12.5 ** 0.5, 4 / 12.5 ** 0.5, 1.0, -1.0]) and close(wsq, [0.72, 1.28, 1.0, 1.0])
    s_eff, d, r = M.style_coefs(t, wsq, torch.tensor(4.0, dtype=F64), True)
    assert close(r, [1.25 ** -0.5]) and close(s_eff, [0.5 / 1.25 ** 0.5, 1.0 / 1.25 ** 0.5, 0.0, 0.0])
    # the epsilon sits inside the root: at q = 0 it alone decides d (outside the root, or 1e-6, or absent: 1e-8, 1e3, inf)
    assert close(d, [(4.672 + 1e-8) ** -0.5, (4.0 + 1e-8) ** -0.5, 1e4, 1e4])
    s_eff, d, r = M.style_coefs(t, None, None, False)                           # ToRGB: the styles themselves
    assert d is None and torch.equal(s_eff, t) and float(r) == 1.0
    s_eff, _, _ = M.style_coefs(t, None, torch.tensor(4.0, dtype=F64), False)
    assert torch.equal(s_eff, t * 0.5)


@pytest.mark.parametrize('name', ['cout_31', 'cout_33', 'row_114x9', 'cin_65'])
@pytest.mark.parametrize('floor', [False, True], ids=['ordinary', 'floor'])
def test_restatement_equals_the_composed_expression(name, floor):
    """The two calls chained equal NET:41-57 written out with its [N, O, I, k, k] weights -- so the factorised d equals
    ((w_hat . s_hat)^2 summed over [2, 3, 4] + 1e-8).rsqrt() -- and autograd through the chain gives the composed expression's gradients, for every
    subset of outputs in the loss, demodulating or not."""
    shape = M.SEAM_SHAPES[name]
    if floor and shape[3] < 3:
        shape = shape[:3] + (3,)                                                 # (below 3 samples the floor needs a gain on wsq: no composed form)
    w, t = (x.to(F64) for x in (M.floor_inputs(shape, 1)[:2] if floor else M.ordinary_inputs(shape, 1)))
    mag = M.magnitude(1).to(F64)
    g_hat, _, g_s, g_d = (g.to(F64) for g in M.cotangents(shape, 1))
    for demod in (True, False):
        for outputs, _, _ in M.GRAD_SETS['autograd'][::3]:
            wl, tl = w.clone().requires_grad_(True), t.clone().requires_grad_(True)
            if demod:
                w_hat, wsq, _ = M.weight_norm(wl)
            s_eff, d, _ = M.style_coefs(tl, wsq if demod else None, mag, demod)
            want = M.composed(w, t, mag, demod)
            for a, b in zip((w_hat if demod else w, s_eff, d), want):
                assert (a is None) == (b is None) and (a is None or M.forward_ratio(a, b, 1e-13) <= 1)
            gs = (g_hat if 'w' in outputs else None, g_s if 's' in outputs else None, g_d if 'd' in outputs else None)
            got = M._grads((w_hat if demod else None, s_eff, d), gs, [wl, tl])
            ref = M.composed_bwd(w, t, mag, demod, *gs)
            for a, b in zip(got, ref):
                assert M.row_ratio(a, b, 1e-11) <= 1, (demod, outputs)


def test_backward_helpers_treat_none_as_an_output_left_out():
    shape = M.SEAM_SHAPES['cout_33']
    w, t = (x.to(F64) for x in M.ordinary_inputs(shape, 2))
    g_hat, g_wsq, g_s, g_d = (g.to(F64) for g in M.cotangents(shape, 2))
    _, wsq, _ = M.weight_norm(w)
    z = torch.zeros_like
    assert not M.weight_norm_bwd(w, None, None).any()
    assert torch.allclose(M.weight_norm_bwd(w, g_hat, None) + M.weight_norm_bwd(w, None, g_wsq), M.weight_norm_bwd(w, g_hat, g_wsq), rtol=1e-12, atol=1e-12)
    assert torch.allclose(M.weight_norm_bwd(w, g_hat, None), M.weight_norm_bwd(w, g_hat, z(g_wsq)), rtol=1e-12, atol=1e-12)
    dt0, gw0 = M.style_coefs_bwd(t, wsq, None, True, None, None)
    assert not dt0.any() and not gw0.any()
    a, b, c = (M.style_coefs_bwd(t, wsq, None, True, *g) for g in ((g_s, None), (None, g_d), (g_s, g_d)))
    assert torch.allclose(a[0] + b[0], c[0], rtol=1e-12, atol=1e-12) and not a[1].any() and torch.equal(b[1], c[1])
    dt, none = M.style_coefs_bwd(t, None, None, False, g_s, None)
    assert none is None and torch.equal(dt, g_s)


# ---- the tables -----------------------------------------------------------------------------------------------------------------------------------
def test_tables_reach_every_seam():
    """From the constants in the docstrings of csrc/modulation.hip: 256 threads; PT 4 / 18 / 0; chunks of 32 channels, 8 per wave, 64 inputs, 4 waves
    over cout; the 768 / 1024 loop of the batch mean."""
    shapes = list(M.SEAM_SHAPES.values())
    assert 20 <= len(shapes) <= 30 and len(set(shapes)) == len(shapes)
    rows = {i * k * k for _, i, k, _ in shapes}
    assert {1, 255, 256, 257, 1023, 1024, 1025, 113 * 9, 114 * 9, 512 * 9, 513 * 9} <= rows
    assert {(i, k) for _, i, k, _ in shapes} >= {(1023, 1), (1024, 1), (1025, 1), (113, 3), (114, 3), (512, 3), (513, 3)}
    assert {1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 65} <= {o for o, _, _, _ in shapes}
    assert {1, 63, 64, 65, 255, 256, 257} <= {i for _, i, _, _ in shapes}
    assert {768, 769, 1023, 1024, 1025, 1792, 1793} <= {n * i for _, i, _, n in shapes}
    assert {1, 2, 17} <= {n for _, _, _, n in shapes}
    assert all(o * i * k * k <= 40000 for o, i, k, _ in shapes)                  # cout small where cin is large

    # weight rows: every PT class with k = 1 and with k = 3, both sides of each boundary, rows shorter than one pass and shorter than a wave
    assert {(M.row_class(i, k), k) for _, i, k, _ in shapes} >= {(4, 1), (18, 1), (4, 3), (18, 3), (0, 3)}
    assert M.row_class(1024, 1) == 4 and M.row_class(1025, 1) == 18 and M.row_class(512, 3) == 18 and M.row_class(513, 3) == 0
    assert M.row_class(113, 3) == 4 and M.row_class(114, 3) == 18
    assert any(i * k * k < 64 for _, i, k, _ in shapes) and any(64 < i * k * k < M.THREADS for _, i, k, _ in shapes)
    # k^2 = 9 rows whose register slots (256 elements each) are no multiple of 9: j / KK crosses slots inside one input channel
    assert all(any(k == 3 and M.row_class(i, k) == pt and i * 9 > M.THREADS for _, i, k, _ in shapes) for pt in (4, 18, 0)) and M.THREADS % 9 != 0
    # a last register slot that is partly filled, and one filled exactly
    assert any(i * k * k % M.THREADS for _, i, k, _ in shapes) and any(i * k * k % M.THREADS == 0 for _, i, k, _ in shapes)

    # style_coefs_fwd: channel chunks of 32 with 8 per wave -- full, one over, one under, a wave's worth, fewer than a wave's; the last chunk's clamped rows
    tail = {o % M.OC_CHUNK for o, _, _, _ in shapes}
    assert {0, 1, M.OC_CHUNK - 1, M.WAVE_CHANNELS, M.WAVE_CHANNELS - 1, M.WAVE_CHANNELS + 1} <= tail
    assert {1, 2, 3} <= {-(-o // M.OC_CHUNK) for o, _, _, _ in shapes}
    # the LDS row of s_hat^2: one pass of 256 threads around cin = 256; lanes of 64 around cin = 64
    assert {255, 256, 257} <= {i for _, i, _, _ in shapes} and {63, 64, 65} <= {i for _, i, _, _ in shapes}
    # the batch mean: no trip (n cin <= 768), one trip exactly and with single loads after it, two trips
    trips = lambda m: len(range(0, max(m - M.MEAN_LEAD, 0), M.MEAN_TRIP))      # of thread 0: j + 768 < m
    by_trips = {}
    for _, i, _, n in shapes:
        by_trips.setdefault(trips(n * i), set()).add(n * i)
    assert trips(768) == 0 and trips(769) == 1 and trips(1792) == 1 and trips(1793) == 2
    assert {768} <= by_trips[0] and {769, 1023, 1024, 1025, 1792} <= by_trips[1] and {1793} <= by_trips[2]
    # bwd1: input chunks of 64 (partial[n, chunk]) -- one chunk full / short, two with one element, many; cout below, at and above the 4 waves
    assert {1, 2, 5, 17} <= {-(-i // M.IC_CHUNK) for _, i, _, _ in shapes} and {0, 1, M.IC_CHUNK - 1} <= {i % M.IC_CHUNK for _, i, _, _ in shapes}
    assert set(range(1, M.O_WAVES + 2)) <= {o for o, _, _, _ in shapes}
    assert all(s in M.SEAM_SHAPES for s in M.BWD_SHAPES)
    assert {M.row_class(*M.SEAM_SHAPES[s][1:3]) for s in M.BWD_SHAPES if M.SEAM_SHAPES[s][2] == 3} == {4, 18, 0}
    o, i, k, n = M.SEAM_SHAPES[M.BWD_SHAPES[0]]
    assert o % M.OC_CHUNK and o % M.WAVE_CHANNELS and i % M.IC_CHUNK and i * k * k % M.THREADS and n > 1


def test_gradient_sets_are_complete():
    g = M.GRAD_SETS
    assert len(set(g['weight_norm_bwd'])) == 4 and len(set(g['style_coefs_bwd_demodulating'])) == 16 and len(set(g['style_coefs_bwd_plain'])) == 4
    assert len(set(g['autograd'])) == 7 * 3 and {o for o, _, _ in g['autograd']} == {'w', 's', 'd', 'ws', 'wd', 'sd', 'wsd'}
    assert not any(fw and ft for _, fw, ft in g['autograd'])


def test_bank_orders_cover_the_table_scan():
    """blk[] of the norm launches (a layer has cout workgroups if it demodulates -- backward: and its weight wants a gradient -- else none): zero-size
    layers first, last, in the middle, two adjacent, all of them; one layer; AFCM_MODULATION_MAX layers; a small layer after the one that sets the
    launch's dynamic LDS size; one layer out of the loss."""
    orders = M.BANK_ORDERS
    fwd = lambda layers: [bool(l.demodulate) for l in layers]
    bwd = lambda layers: [bool(l.demodulate and not l.frozen) for l in layers]
    seen = {'first': False, 'last': False, 'middle': False, 'adjacent': False, 'all': False}
    for n, layers in orders.values():
        assert 1 <= len(layers) <= M.BANK_MAX and n >= 1 and all(l.seam in M.SEAM_SHAPES and set(l.outputs) <= set('wsd') for l in layers)
        assert all(l.demodulate or (l.frozen and set(l.outputs) <= {'s'}) for l in layers)
        assert len(layers) == 1 or any(not l.outputs for l in layers)
        for live in (fwd(layers), bwd(layers)):
            if len(live) > 1 and any(live):
                seen['first'] |= not live[0]
                seen['last'] |= not live[-1]
                seen['middle'] |= any(not b and any(live[:j]) and any(live[j + 1:]) for j, b in enumerate(live))
                seen['adjacent'] |= any(not a and not b for a, b in zip(live, live[1:]))
            seen['all'] |= len(live) > 1 and not any(live)
    assert all(seen.values()), seen
    assert {len(layers) for _, layers in orders.values()} >= {1, M.BANK_MAX}
    assert any(len(layers) == 1 and layers[0].demodulate for _, layers in orders.values()) and any(len(layers) == 1 and not layers[0].demodulate for _, layers in orders.values())
    _, layers = orders['small_after_large']
    cin = [M.SEAM_SHAPES[l.seam][1] for l in layers]
    cout = [M.SEAM_SHAPES[l.seam][0] if l.demodulate else 0 for l in layers]
    assert cin.index(max(cin)) == 0 and min(cin[1:]) == 1 and cout.index(max(cout)) == 1 and min(c for c in cout[2:] if c) == 1
    assert any(not l.magnitude for _, layers in orders.values() for l in layers)


@pytest.mark.parametrize('name', list(M.SEAM_SHAPES))
def test_floor_inputs_meet_their_window(name):
    shape = M.SEAM_SHAPES[name]
    f = M.floor_inputs(shape, 0)                                                # (asserts the window and the zero sample itself)
    n = shape[3]
    assert f.w.dtype == F32 and f.t.dtype == F32 and f.scaled == n - 1 and (f.zero == 0) == (n > 1)
    assert (float(f.wsq_gain) == 1.0) == (n >= 3)
    q = M.floor_q(f)
    lo, hi = M.FLOOR_WINDOW
    assert bool(((q[f.scaled] >= lo) & (q[f.scaled] <= hi)).all())
    for m in range(n):                                                          # every other sample is ordinary: q of the order of cin k^2
        if m not in (f.scaled, f.zero):
            assert bool((q[m] > 1e-3).all())
    _, wsq, _ = M.weight_norm(f.w.to(F64))
    _, d, _ = M.style_coefs(f.t.to(F64), wsq * float(f.wsq_gain), None, True)
    if f.zero is not None:
        assert bool((d[f.zero] == 1e-8 ** -0.5).all()) or torch.allclose(d[f.zero], torch.full_like(d[f.zero], 1e4), rtol=1e-15, atol=0)
    # the epsilon decides this sample's d: without it, d would be off by 10 % at the least
    assert bool(((q[f.scaled].rsqrt() / d[f.scaled]) > 1.1).all())
    assert torch.equal(M.floor_inputs(shape, 0).t, f.t) and not torch.equal(M.floor_inputs(shape, 1).t, f.t)


# ---- the entry points' refusals ---------------------------------------------------------------------------------------------------------------------
def _refused(lib, rc, name):
    from afcm_amd import _lib
    return rc == _lib.E_INVALID and name in lib.afcm_last_error()


def test_per_layer_entry_points_refuse_before_any_launch(lib):
    p = [ctypes.c_void_p(64 * (j + 1)) for j in range(10)]                       # never dereferenced: every call below is refused before a launch
    for hole in range(4):                                                       # w_hat, wsq, scale, w
        a = [None if j == hole else p[j] for j in range(4)]
        assert _refused(lib, lib.afcm_weight_norm_fwd(*a, 2, 2, 1, None), b'weight_norm_fwd')
    for dims in ((0, 2, 1), (2, 0, 1), (2, 2, 0)):
        assert _refused(lib, lib.afcm_weight_norm_fwd(*p[:4], *dims, None), b'weight_norm_fwd')
    for hole in (0, 3, 4):                                                      # dw, w_hat, scale (g_hat and g_wsq may be NULL)
        a = [None if j == hole else p[j] for j in range(5)]
        assert _refused(lib, lib.afcm_weight_norm_bwd(*a, 2, 2, 1, None), b'weight_norm_bwd')
    assert _refused(lib, lib.afcm_weight_norm_bwd(*p[:5], 2, 2, 0, None), b'weight_norm_bwd')
    # style_coefs_fwd(s_eff, d, r, t, wsq, magnitude, n, cin, cout, demodulate): s_eff, r, t always; d, wsq when it demodulates
    for hole, demod in ((0, 1), (2, 1), (3, 1), (1, 1), (4, 1), (0, 0), (2, 0), (3, 0)):
        a = [None if j == hole else p[j] for j in range(6)]
        assert _refused(lib, lib.afcm_style_coefs_fwd(*a, 2, 2, 2, demod, None), b'style_coefs_fwd'), (hole, demod)
    for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):
        assert _refused(lib, lib.afcm_style_coefs_fwd(*p[:6], *dims, 1, None), b'style_coefs_fwd')
    for demod in (0, 1):
        assert _refused(lib, lib.afcm_style_coefs_fwd(*p[:6], 2, M.CHANNELS_MAX + 1, 2, demod, None), b'style_coefs_fwd') and b'16385' in lib.afcm_last_error()
    # style_coefs_bwd(dt, g_wsq, workspace, g_s, g_d, t, d, wsq, magnitude, r, n, cin, cout, demodulate): dt, workspace, t, r always; d, wsq when ...
    for hole, demod in ((0, 1), (2, 1), (5, 1), (9, 1), (6, 1), (7, 1), (0, 0), (2, 0), (5, 0), (9, 0)):
        a = [None if j == hole else p[j] for j in range(10)]
        assert _refused(lib, lib.afcm_style_coefs_bwd(*a, 2, 2, 2, demod, None), b'style_coefs_bwd'), (hole, demod)
    for dims in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):
        assert _refused(lib, lib.afcm_style_coefs_bwd(*p[:10], *dims, 1, None), b'style_coefs_bwd')
    assert _refused(lib, lib.afcm_style_coefs_bwd(*p[:10], 2, 2, M.CHANNELS_MAX + 1, 1, None), b'style_coefs_bwd') and b'16385' in lib.afcm_last_error()


def _table(count, **change):
    """A complete table of ``count`` demodulating layers (pointers never dereferenced), layer 1 -- or the only one -- changed."""
    from afcm_amd import _lib
    table = (_lib.ModulationLayer * max(count, 1))()
    for l in range(max(count, 1)):
        L = table[l]
        L.cout, L.cin, L.kk, L.demodulate = 2, 2, 1, 1
        for j, (k, _) in enumerate(_lib.ModulationLayer._fields_[4:]):
            setattr(L, k, 64 * (j + 1))
    for k, v in change.items():
        setattr(table[min(1, count - 1)], k, v)
    return table


def test_bank_entry_points_refuse_before_any_launch(lib):
    from afcm_amd import _lib
    assert _lib.MODULATION_MAX == M.BANK_MAX == 16
    for entry in (lib.afcm_modulation_bank_fwd, lib.afcm_modulation_bank_bwd):
        for count in (0, M.BANK_MAX + 1, -1):
            table = (_lib.ModulationLayer * (M.BANK_MAX + 1))()
            assert _refused(lib, entry(table, count, 2, None), b'modulation_bank') and b'1..16' in lib.afcm_last_error()
        assert _refused(lib, entry(None, 2, 2, None), b'modulation_bank') and _refused(lib, entry(_table(2), 2, 0, None), b'modulation_bank')
        for count in (1, 3):
            for field in ('w_hat', 'wsq', 'scale', 'd'):
                assert _refused(lib, entry(_table(count, **{field: None}), count, 2, None), b'demodulates'), field
            for change in ({'t': None}, {'r': None}, {'cin': 0}, {'cin': M.CHANNELS_MAX + 1}):
                assert _refused(lib, entry(_table(count, **change), count, 2, None), b'modulation_bank: layer %d' % min(1, count - 1)), change
            for change in ({'cout': 0}, {'cout': M.CHANNELS_MAX + 1}, {'kk': 0}):
                assert _refused(lib, entry(_table(count, **change), count, 2, None), b'demodulates'), change
    for field in ('dt', 'workspace'):
        assert _refused(lib, lib.afcm_modulation_bank_bwd(_table(3, **{field: None}), 3, 2, None), b'dt / workspace')
        assert _refused(lib, lib.afcm_modulation_bank_bwd(_table(3, demodulate=0, **{field: None}), 3, 2, None), b'dt / workspace')
    for change in ({'s_eff': None}, {'w': None}, {'demodulate': 0, 's_eff': None}):
        assert _refused(lib, lib.afcm_modulation_bank_fwd(_table(3, **change), 3, 2, None), b's_eff / w'), change


def test_bank_workspace_floats_is_the_header_formula(lib):
    f = lib.afcm_modulation_bank_workspace_floats
    for bad in ((0, 4, 4, 1), (-1, 4, 4, 1), (4, 0, 4, 1), (4, -3, 4, 0), (4, 4, 0, 1), (4, 4, -1, 1)):
        assert f(*bad) == -1, bad
    for n, cin, cout in ((1, 1, 1), (3, 63, 5), (3, 64, 33), (17, 65, 33), (2, 16384, 16384), (65, 16384, 16384)):
        chunks = -(-cin // M.IC_CHUNK)
        assert f(n, cin, cout, 1) == n * cin + n * cout + n * chunks + cout * cin       # G | Q | partial | g_wsq
        assert f(n, cin, cout, 0) == f(n, cin, 0, 0) == f(n, cin, -7, 0) == n * cin + n * chunks


# ---- the bars -----------------------------------------------------------------------------------------------------------------------------------
def _rel(got, want):
    return M.forward_ratio(got, want, 1.0)


def _row(got, want):
    return M.row_ratio(got, want, 1.0)


def eager_case(shape, floor, seed, sets=None):
    """Worst errors {tensor: value} of the float32 eager composition against float64 on one case, call by call (each float32 call against the float64
    call on the same float32 operands, as the kernels are tested) and -- where no gain on wsq is involved -- composed end to end."""
    worst = {}

    def note(key, v):
        if not (key == 'dw' and M.row_is_one_element(shape)):                  # (dw of a one-element row is zero by identity: modulation_ref)
            worst[key] = max(worst.get(key, 0.0), v)

    f = M.floor_inputs(shape, seed) if floor else M.Floor(*M.ordinary_inputs(shape, seed), torch.ones([]), None, None)
    w, t, mag = f.w, f.t, M.magnitude(seed)
    g_hat, g_wsq, g_s, g_d = M.cotangents(shape, seed)
    dbl = lambda x: None if x is None else x.to(F64)
    got, want = M.weight_norm(w), M.weight_norm(dbl(w))
    for k, a, b in zip(('w_hat', 'wsq', 'scale'), got, want):
        note(k, _rel(a, b))
    wsq = got[1] * f.wsq_gain                                                   # float32, the operand of both style_coefs calls
    sets = sets or {'weight_norm_bwd': [(True, True)], 'style_coefs_bwd_demodulating': [(True, True, True, True), (True, True, True, False)],
                    'style_coefs_bwd_plain': [(True, True)]}
    for hat, sq in sets['weight_norm_bwd']:
        a, b = g_hat if hat else None, g_wsq if sq else None
        note('dw', _row(M.weight_norm_bwd(w, a, b), M.weight_norm_bwd(dbl(w), dbl(a), dbl(b))))
    for demod, key in ((True, 'style_coefs_bwd_demodulating'), (False, 'style_coefs_bwd_plain')):
        for c in sets[key]:
            gs, gd, m = (c[0], c[1], c[3]) if demod else (c[0], False, c[1])
            m = mag if m else None
            got, want = M.style_coefs(t, wsq, m, demod), M.style_coefs(dbl(t), dbl(wsq), dbl(m), demod)
            for k, a, b in zip(('s_eff', 'd', 'r'), got, want):
                if b is not None:
                    note(k, _rel(a, b))
            a, b = g_s if gs else None, g_d if gd else None
            got, want = M.style_coefs_bwd(t, wsq, m, demod, a, b), M.style_coefs_bwd(dbl(t), dbl(wsq), dbl(m), demod, dbl(a), dbl(b))
            note('dt', _row(got[0], want[0]))
            if demod:
                note('g_wsq', _row(got[1], want[1]))
    if float(f.wsq_gain) == 1.0 and (not floor or M.floor_composes(shape)):
        for demod in (True, False):
            for k, a, b in zip(('w_hat', 's_eff', 'd'), M.composed(w, t, mag, demod), M.composed(dbl(w), dbl(t), dbl(mag), demod)):
                if b is not None:
                    note(k, _rel(a, b))
            for outputs, _, _ in M.GRAD_SETS['autograd'][::3]:
                if shape[1] == 1 and 'w' not in outputs:
                    continue                                                    # (dw through wsq alone is rounding residue at cin = 1: modulation_ref)
                gs = (g_hat if 'w' in outputs else None, g_s if 's' in outputs else None, g_d if 'd' in outputs else None)
                got, want = M.composed_bwd(w, t, mag, demod, *gs), M.composed_bwd(dbl(w), dbl(t), dbl(mag), demod, *(dbl(g) for g in gs))
                note('dw', _row(got[0], want[0]))
                note('dt', _row(got[1], want[1]))
    return worst


def measure_eager():
    worst = {}
    cases = [(s, fl, 0, None) for s in M.SEAM_SHAPES.values() for fl in (False, True)]
    cases += [(M.SEAM_SHAPES[s], fl, 1, M.GRAD_SETS) for s in M.BWD_SHAPES for fl in (False, True)]
    cases += [(M.SEAM_SHAPES[l.seam][:3] + (n,), M.floor_composes(M.SEAM_SHAPES[l.seam][:3] + (n,)), 2, None) for n, layers in M.BANK_ORDERS.values() for l in layers]
    for case in cases:
        for k, v in eager_case(*case).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


def test_eager_float32_sits_within_a_quarter_of_the_bars():
    """The measurement behind modulation_ref.EAGER_FWD / EAGER_GRAD (printed: run with -s)."""
    worst = measure_eager()
    print({k: '%.3g' % v for k, v in sorted(worst.items())})
    fwd = max(worst[k] for k in ('w_hat', 'wsq', 'scale', 's_eff', 'd', 'r'))
    grad = max(worst[k] for k in ('dw', 'dt', 'g_wsq'))
    assert M.BAR_FWD == 4 * M.EAGER_FWD and M.BAR_GRAD == 4 * M.EAGER_GRAD
    assert fwd <= M.EAGER_FWD and grad <= M.EAGER_GRAD, (fwd, grad)
    assert fwd >= M.EAGER_FWD / 4 and grad >= M.EAGER_GRAD / 4, (fwd, grad)     # (the constants are the measurement, not a loose guess)
