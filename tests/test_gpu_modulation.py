"""The modulation kernels (afcm_amd/csrc/modulation.hip: weight_norm_{fwd,bwd}, style_coefs_{fwd,bwd1,bwd2}, modulation_bank_*) against the float64
restatement of tests/modulation_ref.py: per element for the forward tensors, per row for the gradients, under the bars measured there (4 x the float32
eager composition's worst error); at every seam of SEAM_SHAPES, with ordinary styles and with styles that put the + 1e-8 of NET:51 to work; for every
NULL / non-NULL combination of the backward entry points' optional gradients; through the autograd ops with every subset of outputs in the loss and
frozen inputs; for every table order of BANK_ORDERS, bit for bit against the per-layer entry points.  tests/test_modulation_ref_cpu.py checks the
restatement, that the tables reach what they are here for, and the bars.  The C ABI is called directly where the Python ops cannot reach a branch
(they never pass a NULL g_hat / g_s / g_d).  Every test prints its worst error / bar per tensor (-s).

Worst error / bar seen on an MI355X over the whole file (1 would fail; BAR_FWD = 1.92e-6 per element, BAR_GRAD = 2.08e-5 of the row's largest):
w_hat 0.087, wsq 0.192 (cout_31 ordinary), scale 0.065, s_eff 0.100, d 0.086, r 0.049; dw 0.034, g_wsq 0.052 (row_9 ordinary), dt 0.197 (bank order
full_16, a cin = 1 layer); dw of one-element rows 0.009 of their cancelling terms."""
import pytest
import torch

import modulation_ref as M

pytestmark = pytest.mark.gpu

F32, F64 = M.F32, M.F64
SENTINEL = 12288.0


def _lib():
    from afcm_amd import _lib
    return _lib, _lib.load(), torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _nan(*shape):
    return torch.full(shape, float('nan'), dtype=F32, device='cuda')


def _dev(x):
    return None if x is None else x.to(F32).cuda().contiguous()


def _dbl(x):
    return None if x is None else x.detach().to(F64).cpu()


class Worst(dict):
    """tensor name -> worst error / bar of one test."""

    def fwd(self, key, got, want):
        self[key] = max(self.get(key, 0.0), M.forward_ratio(got, want, M.BAR_FWD))

    def row(self, key, got, want):
        self[key] = max(self.get(key, 0.0), M.row_ratio(got, want, M.BAR_GRAD))

    def dw(self, shape, got, want, scale, g_hat, g_wsq):
        """dw under the per-row bar; a one-element row (zero by identity) under the bar of its cancelling terms (modulation_ref.row_is_one_element)."""
        if not M.row_is_one_element(shape):
            return self.row('dw', got, want)
        terms = (0 if g_hat is None else _dbl(g_hat).abs().flatten(1)) + (0 if g_wsq is None else 2 * _dbl(g_wsq).abs())
        if not torch.is_tensor(terms):
            terms = torch.zeros(shape[0], 1, dtype=F64)
        lim = M.BAR_GRAD * _dbl(scale)[:, None] * terms
        err = _dbl(got).flatten(1).abs()
        assert bool(torch.isfinite(err).all()) and float(_dbl(want).abs().max()) <= 1e-12
        self['dw_one'] = max(self.get('dw_one', 0.0), float(torch.where(err == 0, err, err / lim).max()))

    def done(self, what):
        print(what, {k: '%.3f' % v for k, v in sorted(self.items())})
        bad = {k: v for k, v in self.items() if not v <= 1}
        assert not bad, (what, bad)


def _inputs(shape, floor, seed):
    """(w, t, wsq gain, scaled sample, zero sample) on the host: floor inputs or ordinary ones."""
    return M.floor_inputs(shape, seed) if floor else M.Floor(*M.ordinary_inputs(shape, seed), torch.ones([]), None, None)


# ---- the per-layer entry points ------------------------------------------------------------------------------------------------------------------
def weight_norm_fwd(w):
    L, lib, st = _lib()
    o, i, kh, kw = w.shape
    w_hat, wsq, scale = _nan(o, i, kh, kw), _nan(o, i), _nan(o)
    L.launched(lib.afcm_weight_norm_fwd(w_hat.data_ptr(), wsq.data_ptr(), scale.data_ptr(), w.data_ptr(), o, i, kh * kw, st), 'weight_norm_fwd')
    return w_hat, wsq, scale


def weight_norm_bwd(w_hat, scale, g_hat, g_wsq):
    L, lib, st = _lib()
    o, i, kh, kw = w_hat.shape
    dw = _nan(o, i, kh, kw)
    L.launched(lib.afcm_weight_norm_bwd(dw.data_ptr(), _ptr(g_hat), _ptr(g_wsq), w_hat.data_ptr(), scale.data_ptr(), o, i, kh * kw, st), 'weight_norm_bwd')
    return dw


def style_coefs_fwd(t, wsq, mag, demod):
    L, lib, st = _lib()
    n, i = t.shape
    o = int(wsq.shape[0]) if demod else 0
    s_eff, d, r = _nan(n, i), (_nan(n, o) if demod else None), _nan(1)
    L.launched(lib.afcm_style_coefs_fwd(s_eff.data_ptr(), _ptr(d), r.data_ptr(), t.data_ptr(), _ptr(wsq) if demod else None, _ptr(mag), n, i, o, int(demod), st),
               'style_coefs_fwd')
    return s_eff, d, r


def style_coefs_bwd(t, d, wsq, mag, r, g_s, g_d, want_wsq, demod):
    """(dt, the caller's g_wsq buffer -- pre-filled with SENTINEL, handed over only if ``want_wsq``)."""
    L, lib, st = _lib()
    n, i = t.shape
    o = int(wsq.shape[0]) if demod else 0
    dt = _nan(n, i)
    g_wsq = torch.full([o, i], SENTINEL, dtype=F32, device='cuda') if demod else None
    ws = _nan(n * i + n * o + n * ((i + 63) // 64))
    L.launched(lib.afcm_style_coefs_bwd(dt.data_ptr(), _ptr(g_wsq) if want_wsq else None, ws.data_ptr(), _ptr(g_s), _ptr(g_d), t.data_ptr(), _ptr(d),
                                        _ptr(wsq) if demod else None, _ptr(mag), r.data_ptr(), n, i, o, int(demod), st), 'style_coefs_bwd')
    return dt, g_wsq


@pytest.mark.parametrize('floor', [False, True], ids=['ordinary', 'floor'])
@pytest.mark.parametrize('name', list(M.SEAM_SHAPES))
def test_forward_and_backward_at_every_seam(name, floor):
    """afcm_weight_norm_{fwd,bwd} and afcm_style_coefs_{fwd,bwd}, demodulating or not, magnitude NULL or set, all gradients present: every output per
    element / per row against float64.  Floor inputs: the zero sample's d is rsqrt(1e-8) and its s_eff exactly 0; the scaled sample's d is decided by
    the epsilon (a kernel without it, or with it outside the root, is off by 10 % or more there)."""
    shape = M.SEAM_SHAPES[name]
    f = _inputs(shape, floor, 0)
    g_hat, g_wsq, g_s, g_d = (_dev(g) for g in M.cotangents(shape, 0))
    w, t, mag = _dev(f.w), _dev(f.t), _dev(M.magnitude(0))
    worst = Worst()
    w_hat, wsq, scale = weight_norm_fwd(w)
    for k, a, b in zip(('w_hat', 'wsq', 'scale'), (w_hat, wsq, scale), M.weight_norm(_dbl(w))):
        worst.fwd(k, a, b)
    worst.dw(shape, weight_norm_bwd(w_hat, scale, g_hat, g_wsq), M.weight_norm_bwd(_dbl(w), _dbl(g_hat), _dbl(g_wsq)), scale, g_hat, g_wsq)
    wsq_in = (wsq * f.wsq_gain.cuda()).contiguous()                             # (the gain is 1 unless the floor needs it: modulation_ref.floor_inputs)
    for demod in (True, False):
        for m in (mag, None):
            s_eff, d, r = style_coefs_fwd(t, wsq_in, m, demod)
            want = M.style_coefs(_dbl(t), _dbl(wsq_in), _dbl(m), demod)
            for k, a, b in zip(('s_eff', 'd', 'r'), (s_eff, d, r), want):
                assert (a is None) == (b is None)
                if a is not None:
                    worst.fwd(k, a, b)
            if not demod:
                assert float(r) == 1.0
            if floor and demod:
                if f.zero is not None:
                    assert not s_eff[f.zero].any()
                    assert M.forward_ratio(d[f.zero], torch.full([shape[0]], 1e4, dtype=F64), M.BAR_FWD) <= 1
                assert bool((d[f.scaled].double().cpu() * (M.floor_q(f)[f.scaled]).sqrt() < 1 / 1.1).all())
            dt, gw = style_coefs_bwd(t, d, wsq_in, m, r, g_s, g_d if demod else None, demod, demod)
            want = M.style_coefs_bwd(_dbl(t), _dbl(wsq_in), _dbl(m), demod, _dbl(g_s), _dbl(g_d) if demod else None)
            worst.row('dt', dt, want[0])
            if demod:
                worst.row('g_wsq', gw, want[1])
    worst.done('%s %s' % (name, 'floor' if floor else 'ordinary'))


@pytest.mark.parametrize('floor', [False, True], ids=['ordinary', 'floor'])
@pytest.mark.parametrize('name', M.BWD_SHAPES)
def test_backward_for_every_set_of_null_gradients(name, floor):
    """Every NULL / non-NULL combination of g_hat, g_wsq (afcm_weight_norm_bwd) and of g_s, g_d, the g_wsq buffer, magnitude (afcm_style_coefs_bwd,
    demodulating or not): a NULL gradient is an output left out of the loss.  All NULL: exact zeros.  A g_wsq buffer not handed over stays as it was."""
    shape = M.SEAM_SHAPES[name]
    f = _inputs(shape, floor, 1)
    g_hat, g_wsq, g_s, g_d = (_dev(g) for g in M.cotangents(shape, 1))
    w, t, mag = _dev(f.w), _dev(f.t), _dev(M.magnitude(1))
    worst = Worst()
    w_hat, wsq, scale = weight_norm_fwd(w)
    for hat, sq in M.GRAD_SETS['weight_norm_bwd']:
        a, b = g_hat if hat else None, g_wsq if sq else None
        dw = weight_norm_bwd(w_hat, scale, a, b)
        worst.dw(shape, dw, M.weight_norm_bwd(_dbl(w), _dbl(a), _dbl(b)), scale, a, b)
        if not hat and not sq:
            assert not dw.any()
    wsq_in = (wsq * f.wsq_gain.cuda()).contiguous()
    for demod, key in ((True, 'style_coefs_bwd_demodulating'), (False, 'style_coefs_bwd_plain')):
        for c in M.GRAD_SETS[key]:
            gs, gd, want_wsq, m = (c[0], c[1], c[2], c[3]) if demod else (c[0], False, False, c[1])
            m, a, b = (mag if m else None), (g_s if gs else None), (g_d if gd else None)
            _, d, r = style_coefs_fwd(t, wsq_in, m, demod)
            dt, gw = style_coefs_bwd(t, d, wsq_in, m, r, a, b, want_wsq, demod)
            want = M.style_coefs_bwd(_dbl(t), _dbl(wsq_in), _dbl(m), demod, _dbl(a), _dbl(b))
            worst.row('dt', dt, want[0])
            if not gs and not gd:
                assert not dt.any()
            if demod and want_wsq:
                worst.row('g_wsq', gw, want[1])
                assert gd or not gw.any()
            elif demod:
                assert bool((gw == SENTINEL).all())
    worst.done('%s %s' % (name, 'floor' if floor else 'ordinary'))


# ---- the bank through the C ABI --------------------------------------------------------------------------------------------------------------------
def _layer_operands(n, layers, seed=2):
    """Per layer: dict of the device operands -- w, t, magnitude, the gradients its ``outputs`` name (the others None) -- and the host shape."""
    ops = []
    for l in layers:
        shape = M.SEAM_SHAPES[l.seam][:3] + (n,)
        f = _inputs(shape, M.floor_composes(shape), seed)
        g_hat, _, g_s, g_d = (_dev(g) for g in M.cotangents(shape, seed))
        ops.append(dict(shape=shape, layer=l, w=_dev(f.w), t=_dev(f.t), mag=_dev(M.magnitude(seed)) if l.magnitude else None,
                        g_hat=g_hat if 'w' in l.outputs and l.demodulate else None, g_s=g_s if 's' in l.outputs else None,
                        g_d=g_d if 'd' in l.outputs and l.demodulate else None))
    return ops


def bank_abi(n, ops):
    """afcm_modulation_bank_fwd, then _bwd: per layer a dict of every output (None where the layer has none)."""
    L, lib, st = _lib()
    table = (L.ModulationLayer * len(ops))()
    outs = []
    for T, op in zip(table, ops):
        o, i, k, _ = op['shape']
        l = op['layer']
        out = dict(s_eff=_nan(n, i), r=_nan(1), dt=_nan(n, i), w_hat=None, wsq=None, scale=None, d=None, dw=None)
        T.cin, T.demodulate, T.t, T.magnitude = i, int(l.demodulate), op['t'].data_ptr(), _ptr(op['mag'])
        if l.demodulate:
            out.update(w_hat=_nan(o, i, k, k), wsq=_nan(o, i), scale=_nan(o), d=_nan(n, o), dw=None if l.frozen else _nan(o, i, k, k))
            T.cout, T.kk, T.w = o, k * k, op['w'].data_ptr()
        out['workspace'] = _nan(int(lib.afcm_modulation_bank_workspace_floats(n, i, o if l.demodulate else 0, int(l.demodulate))))
        for key in ('w_hat', 'wsq', 'scale', 's_eff', 'd', 'r', 'dw', 'dt', 'workspace'):
            setattr(T, key, _ptr(out[key]))
        for key in ('g_hat', 'g_s', 'g_d'):
            setattr(T, key, _ptr(op[key]))
        outs.append(out)
    L.launched(lib.afcm_modulation_bank_fwd(table, len(ops), n, st), 'modulation_bank_fwd')
    L.launched(lib.afcm_modulation_bank_bwd(table, len(ops), n, st), 'modulation_bank_bwd')
    torch.cuda.synchronize()
    return outs


def layers_abi(ops):
    """The same layers one by one through afcm_weight_norm_* and afcm_style_coefs_*."""
    outs = []
    for op in ops:
        l = op['layer']
        out = dict(w_hat=None, wsq=None, scale=None, d=None, dw=None, g_wsq=None)
        if l.demodulate:
            out['w_hat'], out['wsq'], out['scale'] = weight_norm_fwd(op['w'])
        out['s_eff'], out['d'], out['r'] = style_coefs_fwd(op['t'], out['wsq'], op['mag'], l.demodulate)
        out['dt'], gw = style_coefs_bwd(op['t'], out['d'], out['wsq'], op['mag'], out['r'], op['g_s'], op['g_d'], l.demodulate and not l.frozen, l.demodulate)
        if l.demodulate and not l.frozen:
            out['g_wsq'] = gw
            out['dw'] = weight_norm_bwd(out['w_hat'], out['scale'], op['g_hat'], gw)
        outs.append(out)
    return outs


OUT_KEYS = ('w_hat', 'wsq', 'scale', 's_eff', 'd', 'r', 'dw', 'dt')


@pytest.mark.parametrize('order', list(M.BANK_ORDERS))
def test_bank_orders(order):
    """afcm_modulation_bank_{fwd,bwd} over one table order: every output and gradient of every layer against float64 under the bars, and equal bit for
    bit to the per-layer entry points, as include/afcm_hip.h promises.  Gradients a layer's ``outputs`` leave out are NULL in the table, a frozen
    layer's dw is NULL; the layer left out of the loss must come back with exact zeros."""
    n, layers = M.BANK_ORDERS[order]
    ops = _layer_operands(n, layers)
    got, one = bank_abi(n, ops), layers_abi(ops)
    worst = Worst()
    for j, (op, a, b) in enumerate(zip(ops, got, one)):
        l = op['layer']
        for k in OUT_KEYS:
            assert (a[k] is None) == (b[k] is None), (j, k)
            assert a[k] is None or torch.equal(a[k], b[k]), (j, k, float((a[k] - b[k]).abs().max()))
        w, t, mag = _dbl(op['w']), _dbl(op['t']), _dbl(op['mag'])
        if l.demodulate:
            for k, x in zip(('w_hat', 'wsq', 'scale'), M.weight_norm(w)):
                worst.fwd(k, a[k], x)
        for k, x in zip(('s_eff', 'd', 'r'), M.style_coefs(t, _dbl(a['wsq']), mag, l.demodulate)):
            assert (a[k] is None) == (x is None), (j, k)
            if x is not None:
                worst.fwd(k, a[k], x)
        dw, dt = M.composed_bwd(w, t, mag, l.demodulate, _dbl(op['g_hat']), _dbl(op['g_s']), _dbl(op['g_d']))
        worst.row('dt', a['dt'], dt)
        if a['dw'] is not None:
            worst.dw(op['shape'], a['dw'], dw, a['scale'], op['g_hat'], b['g_wsq'])
        if not l.outputs:
            assert not a['dt'].any() and (a['dw'] is None or not a['dw'].any()), j
    worst.done(order)


def test_bank_of_seventeen_layers_is_declined():
    from afcm_amd.torch_utils.ops import modulation_bank as mb
    w, t = torch.randn(2, 3, 1, 1, device='cuda'), torch.randn(2, 3, device='cuda')
    assert mb.supported([mb.Item(w, t, None, True)] * M.BANK_MAX) and not mb.supported([mb.Item(w, t, None, True)] * (M.BANK_MAX + 1))
    assert not mb.supported([])


def test_bank_is_reproducible():
    """Two runs of one mixed bank, forward and backward, with unrelated allocations (and so other addresses) in between: equal bits.  The family uses
    no atomics; every sum has one fixed order."""
    n, layers = M.BANK_ORDERS['small_after_large']
    ops = _layer_operands(n, layers)
    first = bank_abi(n, ops)
    junk = [torch.randn(1000 + 37 * j, device='cuda') for j in range(5)]
    ops = _layer_operands(n, layers)                                            # (fresh operand tensors too)
    again = bank_abi(n, ops)
    for a, b in zip(first, again):
        for k in OUT_KEYS:
            assert a[k] is None or (a[k].data_ptr() != b[k].data_ptr() and torch.equal(a[k], b[k])), k
    del junk


# ---- the autograd ops --------------------------------------------------------------------------------------------------------------------------------
def _autograd_run(via, n, layers, outputs, frozen_w, frozen_t):
    from afcm_amd.torch_utils.ops import modulation_bank as mb
    from afcm_amd.torch_utils.ops.conv2d import modulation_coefficients_fused
    ops = _layer_operands(n, layers)
    ws = [op['w'].requires_grad_(not frozen_w) for op in ops]
    ts = [op['t'].requires_grad_(not frozen_t) for op in ops]
    if via == 'bank':
        items = [mb.Item(w, t, op['mag'], op['layer'].demodulate) for w, t, op in zip(ws, ts, ops)]
        assert mb.supported(items)
        res = mb.modulation_bank(items)
    else:
        res = [modulation_coefficients_fused(w, t, demodulate=op['layer'].demodulate, magnitude=op['mag']) for w, t, op in zip(ws, ts, ops)]
    loss, cots = 0, []
    for op, (w_hat, s_eff, d) in zip(ops, res):
        g_hat, _, g_s, g_d = (_dev(g) for g in M.cotangents(op['shape'], 2))
        demod = op['layer'].demodulate
        assert (d is None) == (not demod)
        cot = (g_hat if 'w' in outputs and demod else None, g_s if 's' in outputs else None, g_d if 'd' in outputs and demod else None)
        cots.append(cot)
        loss = loss + sum((x * g).sum() for x, g in zip((w_hat, s_eff, d), cot) if g is not None)
    if torch.is_tensor(loss) and loss.requires_grad:
        loss.backward()
    return ops, cots, [w.grad for w in ws], [t.grad for t in ts]


@pytest.mark.parametrize('via', ['fused', 'bank'])
@pytest.mark.parametrize('order', ['one_demodulating', 'plain_middle'])
def test_autograd_output_subsets_and_frozen_inputs(order, via):
    """modulation_coefficients_fused layer by layer and modulation_bank (one layer; a mixed list) with every non-empty subset of {w_hat, s_eff, d} in
    the loss: gradients against float64 under the bars; with the weights or the styles frozen that input's gradient is None and the other's is equal,
    bit for bit, to the unfrozen run's."""
    n, layers = M.BANK_ORDERS[order]
    worst = Worst()
    base = {}
    for outputs, frozen_w, frozen_t in M.GRAD_SETS['autograd']:
        ops, cots, dws, dts = _autograd_run(via, n, layers, outputs, frozen_w, frozen_t)
        if not frozen_w and not frozen_t:
            base[outputs] = (dws, dts)
            for op, cot, dw, dt in zip(ops, cots, dws, dts):
                want = M.composed_bwd(_dbl(op['w']), _dbl(op['t']), _dbl(op['mag']), op['layer'].demodulate, *(_dbl(g) for g in cot))
                if dw is not None and op['layer'].demodulate:
                    worst.row('dw', dw, want[0])
                if dt is not None:
                    worst.row('dt', dt, want[1])
                assert dt is not None or not want[1].any()
                assert dw is not None or not want[0].any()
            continue
        for mine, ref, frozen in ((dws, base[outputs][0], frozen_w), (dts, base[outputs][1], frozen_t)):
            for a, b in zip(mine, ref):
                if frozen:
                    assert a is None, (outputs, frozen_w, frozen_t)
                elif a is None or b is None:                                     # (no path from the loss: no gradient either way, or zeros)
                    assert (a is None or not a.any()) and (b is None or not b.any()), (outputs, frozen_w, frozen_t)
                else:
                    assert torch.equal(a, b), (outputs, frozen_w, frozen_t, float((a - b).abs().max()))
    worst.done('%s %s' % (order, via))
