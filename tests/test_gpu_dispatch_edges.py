"""The generator's one-launch small kernels -- affine bank, dense layers, mapping input stage, modulation coefficients, 4x4 pooling -- against
float64 aten on both sides of every dispatch threshold.  Where the Python gate says yes the op is called directly (a launch the C entry point
declines raises, _lib.launched); where it says no, either the op itself must refuse the shape (the C gate agrees) or the module's fallback
runs and is held to the same bar.  Thresholds, from the code:
  affine_bank   K = kw + kg <= 1536, K % 16, kw % 4, kg % 4, 16-byte aligned rows (csrc/affine_bank.hip bank_supported); 16 batch rows
                per pass (kNB), later passes accumulate dW
  fc_act        n <= 64, cin % 16, cout % 16 backward, 16-byte aligned x and weight; NT = 1 / 2 / 4 at n <= 16 / 32 / 64; 1024-thread form at cin >= 2048, n <= 32
                (csrc/fc_bank.hip afcm_fc_act_fwd / _bwd)
  mapping_input one workgroup per sample, the last one (a ticket) reduces and re-arms the ticket (csrc/fc_bank.hip mapping_input_bwd_kernel)
  modulation    weight rows cin k^2 <= 1024 / <= 4608 / longer; style rows of at most 16384 channels (csrc/modulation.hip)
  pool_blocks   H % 4 == W % 4 == 0, four planes per workgroup (csrc/bias_act.hip afcm_pool_blocks_fwd / _bwd)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _close(a, b, tol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    scale = max(float(b.abs().max()), 1e-30)
    err = float((a - b).abs().max()) / scale
    assert err <= tol, f'{what}: {err:.3e} of scale {scale:.3e} (tolerance {tol:.1e})'


# ---- affine bank ------------------------------------------------------------------------------------------------------------------------------
def _affine_case(n, kw, kg, couts, idx=None, seed=0):
    from afcm_amd.networks_stylegan3 import FullyConnectedLayer
    from afcm_amd.torch_utils.ops import affine_bank as ab
    torch.manual_seed(seed)
    fcs = [FullyConnectedLayer(kw + kg, c, bias_init=1).cuda() for c in couts]
    for fc in fcs:
        with torch.no_grad():
            fc.bias.add_(torch.randn_like(fc.bias) * 0.1)
    idx = list(range(1, 1 + len(couts))) if idx is None else idx
    ws = torch.randn(n, max(idx) + 2, kw, device='cuda')
    g = torch.randn(n, kg, device='cuda') if kg else None
    scales = [1.0] * (len(couts) - 1) + [0.125]
    specs = [ab.Spec(fc, i, sc) for fc, i, sc in zip(fcs, idx, scales)]
    return ab, fcs, ws, g, specs


def _affine_vs_float64(ab, fcs, ws, g, specs, drop=()):
    """Forward at 1e-5 and every gradient at 1e-4 of scale (the bars of test_affine_bank_matches_the_layers_one_by_one) against float64;
    layers in `drop` receive no gradient."""
    ws = ws.clone().requires_grad_(True)
    g = None if g is None else g.clone().requires_grad_(True)
    params = [p for fc in fcs for p in (fc.weight, fc.bias)]
    got = ab.affine_bank(ws, g, specs)
    wsd = ws.detach().double().cpu().requires_grad_(True)
    gd = None if g is None else g.detach().double().cpu().requires_grad_(True)
    pd = [p.detach().double().cpu().requires_grad_(True) for p in params]
    want = []
    for l, sp in enumerate(specs):
        x = wsd[:, sp.w_index] if gd is None else torch.cat((wsd[:, sp.w_index], gd), 1)
        want.append((x @ (pd[2 * l] * sp.fc.weight_gain).t() + pd[2 * l + 1] * sp.fc.bias_gain) * sp.scale)
    for l, (a, b) in enumerate(zip(got, want)):
        _close(a, b, 1e-5, f'styles {l}')
    gen = torch.Generator().manual_seed(1)
    rs = [None if l in drop else torch.randn(b.shape, generator=gen, dtype=torch.float64) for l, b in enumerate(want)]
    ins_g = [ws] + ([g] if g is not None else []) + params
    ins_d = [wsd] + ([gd] if gd is not None else []) + pd
    gg = torch.autograd.grad(sum((a * r.float().cuda()).sum() for a, r in zip(got, rs) if r is not None), ins_g, allow_unused=True)
    gw = torch.autograd.grad(sum((b * r).sum() for b, r in zip(want, rs) if r is not None), ins_d, allow_unused=True)
    for i, (a, b) in enumerate(zip(gg, gw)):
        if b is None:
            assert a is None or float(a.abs().max()) == 0.0, i
        else:
            _close(a, b, 1e-4, f'gradient {i}')


@pytest.mark.parametrize('n', [1, 15, 16, 17, 33, 70])
def test_affine_bank_batch_passes_vs_float64(n):
    """K = 32 + 1024 = 1056 (the tiny generators' shape): one 16-row pass, exactly one, one plus a row, three and five passes."""
    ab, fcs, ws, g, specs = _affine_case(n, 32, 1024, [8, 24, 7], seed=n)
    assert ab.supported(ws, g, specs)
    _affine_vs_float64(ab, fcs, ws, g, specs)


@pytest.mark.parametrize('n,kw,kg,couts', [(17, 512, 1024, [64, 3]), (16, 48, 0, [16, 5]), (3, 16, 0, [9])], ids=str)
def test_affine_bank_k_edges_vs_float64(n, kw, kg, couts):
    """K = 1536 (the limit), no global vector (kg = 0, K = 48 and 16)."""
    ab, fcs, ws, g, specs = _affine_case(n, kw, kg, couts)
    assert ab.supported(ws, g, specs)
    _affine_vs_float64(ab, fcs, ws, g, specs)


def test_affine_bank_unused_layer_and_shared_latents_vs_float64():
    """A layer whose styles get no gradient (zeros for its weights), and latents that are neither consecutive nor distinct: the input
    gradient goes back through _AffineBank.backward's index_add_ branch."""
    ab, fcs, ws, g, specs = _affine_case(19, 32, 1024, [8, 8, 16, 4], idx=[3, 0, 3, 1])
    assert ab.supported(ws, g, specs)
    _affine_vs_float64(ab, fcs, ws, g, specs, drop=(1,))


@pytest.mark.parametrize('kw,kg', [(36, 1024), (40, 1024), (516, 1024), (36, 0), (520, 1024)], ids=str)
def test_affine_bank_gate_agrees_with_the_kernels(kw, kg):
    """K = 1060, 1064 (multiples of 4, not of 16), 1540 (over the limit), 36 without a global vector, 1544: the gate says no, and so does
    the C entry point -- the op raises instead of handing back unwritten styles."""
    ab, fcs, ws, g, specs = _affine_case(4, kw, kg, [8])
    assert not ab.supported(ws, g, specs)
    with pytest.raises(RuntimeError, match='affine_bank'):
        ab.affine_bank(ws, g, specs)


def test_affine_bank_gate_rejects_misaligned_rows():
    """ws whose storage starts 4 bytes past a 16-byte boundary (strides still multiples of 4): the kernels' 16-byte loads cannot take it."""
    ab, fcs, ws, g, specs = _affine_case(4, 32, 1024, [8])
    buf = torch.empty(ws.numel() + 1, device='cuda')
    wso = buf[1:].view(ws.shape)
    wso.copy_(ws)
    assert wso.data_ptr() % 16 != 0 and ab.supported(ws, g, specs)
    assert not ab.supported(wso, g, specs)


# ---- dense layers -----------------------------------------------------------------------------------------------------------------------------
def _fc_vs_float64(n, cin, cout, act, expect_kernel, monkeypatch):
    """FullyConnectedLayer.forward: the one-launch kernel where fc_bank's gate says yes, the GEMM composition where it says no; both held
    to the kernel's bar (test_fc_act_forward_backward_vs_float64: 2e-6 forward, 3e-6 gradients, of scale)."""
    from afcm_amd.networks_stylegan3 import FullyConnectedLayer
    from afcm_amd.torch_utils.ops import fc_bank
    torch.manual_seed(n * 7 + cin + cout)
    fc = FullyConnectedLayer(cin, cout, activation=act, lr_multiplier=0.37, bias_init=0.5).cuda()
    x = torch.randn(n, cin, device='cuda', requires_grad=True)
    r = torch.randn(n, cout, device='cuda')
    calls = []
    real = fc_bank.fc_act
    monkeypatch.setattr(fc_bank, 'fc_act', lambda *a, **k: calls.append(1) or real(*a, **k))
    assert fc_bank.supported(x, fc.weight, act) == expect_kernel
    y = fc(x)
    got = torch.autograd.grad((y * r).sum(), [x, fc.weight, fc.bias])
    assert len(calls) == (1 if expect_kernel else 0)
    xd, wd, bd = (t.detach().double().cpu().requires_grad_(True) for t in (x, fc.weight, fc.bias))
    yd = xd @ (wd * fc.weight_gain).t() + bd * fc.bias_gain
    if act == 'lrelu':
        yd = torch.nn.functional.leaky_relu(yd, 0.2) * np.sqrt(2)
    ref = torch.autograd.grad((yd * r.double().cpu()).sum(), [xd, wd, bd])
    _close(y, yd, 2e-6, 'y')
    for nm, a, b in zip(('dx', 'dw', 'db'), got, ref):
        _close(a, b, 3e-6, nm)


@pytest.mark.parametrize('n', [16, 17, 24, 32, 33, 64])
@pytest.mark.parametrize('cin', [2032, 2048, 4608])
def test_fc_act_thread_classes_vs_float64(n, cin, monkeypatch):
    """NT = 1 / 2 / 4 (n <= 16 / 32 / 64) crossed with the 256-thread form (cin 2032) and the 1024-thread wide form (cin >= 2048 at n <= 32;
    n = 33 and 64 leave it)."""
    _fc_vs_float64(n, cin, 48, 'lrelu', True, monkeypatch)


@pytest.mark.parametrize('n,cin,cout,act', [(8, 64, 40, 'lrelu'), (65, 512, 64, 'lrelu'), (65, 48, 24, 'linear'), (3, 40, 16, 'linear')], ids=str)
def test_fc_fallback_outside_the_gate_vs_float64(n, cin, cout, act, monkeypatch):
    """cout % 16, more than 64 rows, cin % 16: the gate says no and the GEMM composition holds the same bar."""
    _fc_vs_float64(n, cin, cout, act, False, monkeypatch)


@pytest.mark.parametrize('n,cin,cout,act', [(8, 64, 48, 'lrelu'), (16, 32, 16, 'linear')], ids=str)
def test_fc_fallback_for_a_view_off_the_16_byte_grid_vs_float64(n, cin, cout, act, monkeypatch):
    """x = buf[1:].view(n, cin): contiguous, so .contiguous() leaves it where it is, 4 bytes past a 16-byte boundary.  The kernel's
    16-byte loads cannot take it (afcm_fc_act_fwd refuses the pointers), so the gate must say no and the GEMM composition run, held to
    the kernel's bars.  The same input on the 16-byte grid takes the kernel; there a cotangent off the grid is copied, not refused."""
    from afcm_amd.networks_stylegan3 import FullyConnectedLayer
    from afcm_amd.torch_utils.ops import fc_bank
    torch.manual_seed(n + cin + cout)
    fc = FullyConnectedLayer(cin, cout, activation=act, lr_multiplier=0.37, bias_init=0.5).cuda()
    xa = torch.randn(n, cin, device='cuda')
    x = torch.empty(n * cin + 1, device='cuda')[1:].view(n, cin).copy_(xa).requires_grad_(True)
    r = torch.empty(n * cout + 1, device='cuda')[1:].view(n, cout).copy_(torch.randn(n, cout, device='cuda'))
    assert x.is_contiguous() and x.data_ptr() % 16 == 4 and x.contiguous().data_ptr() == x.data_ptr() and r.data_ptr() % 16 == 4
    calls = []
    real = fc_bank.fc_act
    monkeypatch.setattr(fc_bank, 'fc_act', lambda *a, **k: calls.append(1) or real(*a, **k))
    y = fc(x)                                                                      # (raised before the gate looked at addresses)
    got = torch.autograd.grad(y, [x, fc.weight, fc.bias], r)
    assert len(calls) == 0
    assert fc_bank.supported(xa, fc.weight, act) and not fc_bank.supported(x, fc.weight, act)
    xa.requires_grad_(True)
    ya = fc(xa)
    gota = torch.autograd.grad(ya, [xa, fc.weight, fc.bias], r)                    # the kernel, its cotangent off the grid
    assert len(calls) == 1
    xd, wd, bd = (t.detach().double().cpu().requires_grad_(True) for t in (x, fc.weight, fc.bias))
    yd = xd @ (wd * fc.weight_gain).t() + bd * fc.bias_gain
    if act == 'lrelu':
        yd = torch.nn.functional.leaky_relu(yd, 0.2) * np.sqrt(2)
    ref = torch.autograd.grad(yd, [xd, wd, bd], r.double().cpu())
    for route, yy, gg in (('fallback', y, got), ('kernel', ya, gota)):
        _close(yy, yd, 2e-6, f'y ({route})')
        for nm, a, b in zip(('dx', 'dw', 'db'), gg, ref):
            _close(a, b, 3e-6, f'{nm} ({route})')


# ---- mapping input stage ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 64, 257])
@pytest.mark.parametrize('zdim,cdim,wdim', [(1, 1, 36), (33, 7, 512), (512, 0, 36), (512, 1, 512), (33, 1, 36)], ids=str)
def test_mapping_input_vs_float64(n, zdim, cdim, wdim):
    """cat(normalize(z), normalize(embed(c))) (NET:143-150) and the embedding's gradients against float64 (forward 1e-5, gradients 3e-5:
    the bars of test_mapping_network_matches_the_op_by_op_composition); a second backward of the same graph must be bit-identical to the
    first -- the last workgroup re-arms the ticket the cached workspace depends on."""
    from afcm_amd.networks_stylegan3 import FullyConnectedLayer
    from afcm_amd.torch_utils.ops import fc_bank
    torch.manual_seed(n + zdim + cdim + wdim)
    z = torch.randn(n, zdim, device='cuda')
    c = torch.rand(n, cdim, device='cuda') if cdim else None
    embed = FullyConnectedLayer(cdim, wdim).cuda() if cdim else None
    if embed is not None:
        with torch.no_grad():
            embed.bias.add_(torch.randn_like(embed.bias) * 0.3)
    assert fc_bank.mapping_input_supported(z, c, embed)
    x0 = fc_bank.mapping_input(z, c, embed)
    zd = z.double().cpu()
    want = zd * (zd.square().mean(1, keepdim=True) + 1e-8).rsqrt()
    if cdim:
        wd, bd = embed.weight.detach().double().cpu().requires_grad_(True), embed.bias.detach().double().cpu().requires_grad_(True)
        e = c.double().cpu() @ (wd * embed.weight_gain).t() + bd * embed.bias_gain
        want = torch.cat([want, e * (e.square().mean(1, keepdim=True) + 1e-8).rsqrt()], 1)
    _close(x0, want, 1e-5, 'x0')
    if not cdim:
        return
    r = torch.randn(want.shape, dtype=torch.float64)
    ref = torch.autograd.grad((want * r).sum(), [wd, bd])
    got = torch.autograd.grad((x0 * r.float().cuda()).sum(), [embed.weight, embed.bias], retain_graph=True)
    again = torch.autograd.grad((x0 * r.float().cuda()).sum(), [embed.weight, embed.bias])
    for nm, a, b, a2 in zip(('dW', 'db'), got, ref, again):
        _close(a, b, 3e-5, nm)
        assert torch.equal(a, a2), nm


# ---- modulation coefficients ------------------------------------------------------------------------------------------------------------------
def _modulation_float64(w, t, demodulate, magnitude):
    """NET:41-57 with input_gain = magnitude.rsqrt() (NET:346), float64: (w_hat, in_scale, out_scale or None)."""
    d = None
    if demodulate:
        w = w * w.square().mean([1, 2, 3], keepdim=True).rsqrt()
        t = t * t.square().mean().rsqrt()
        d = ((w.unsqueeze(0) * t[:, None, :, None, None]).square().sum([2, 3, 4]) + 1e-8).rsqrt()
    if magnitude is not None:
        t = t * magnitude.rsqrt()
    return w, t, d


MOD_SHAPES = [(8, 1024, 1, True), (8, 1025, 1, True), (4, 512, 3, True), (3, 4609, 1, True), (24, 16, 1, True), (5, 113, 3, True),
              (3, 1025, 1, False), (2, 16384, 1, True)]


@pytest.mark.parametrize('n', [1, 17, 65])
@pytest.mark.parametrize('bank', [True, False], ids=['bank', 'per_layer'])
def test_modulation_vs_float64(n, bank):
    """Weight rows of cin k^2 = 1024 / 1025, 4608 / 4609 (the row-length classes of weight_norm), 1x1 layers that demodulate, a ToRGB-like
    layer that does not, 16384 input channels (the style kernels' limit): the bank (afcm_modulation_bank_*) and the per-layer kernels
    (afcm_weight_norm_* + afcm_style_coefs_*) against float64, forward 1e-5 and gradients 1e-4 of scale (fp32 reductions, the affine bank's
    bars)."""
    from afcm_amd.torch_utils.ops import modulation_bank as mb
    from afcm_amd.torch_utils.ops.conv2d import modulation_coefficients_fused
    torch.manual_seed(n)
    ws = [torch.randn(o, i, k, k, device='cuda', requires_grad=True) for o, i, k, _ in MOD_SHAPES]
    ts = [(torch.randn(n, i, device='cuda') + 1.0).requires_grad_(True) for _, i, _, _ in MOD_SHAPES]
    mags = [None if l == 2 else torch.rand([], device='cuda') + 0.5 for l in range(len(MOD_SHAPES))]
    dms = [dm for _, _, _, dm in MOD_SHAPES]
    if bank:
        items = [mb.Item(w, t, m, dm) for w, t, m, dm in zip(ws, ts, mags, dms)]
        assert mb.supported(items)
        got = mb.modulation_bank(items)
    else:
        got = [modulation_coefficients_fused(w, t, demodulate=dm, magnitude=m) for w, t, m, dm in zip(ws, ts, mags, dms)]
    wd = [w.detach().double().cpu().requires_grad_(True) for w in ws]
    td = [t.detach().double().cpu().requires_grad_(True) for t in ts]
    want = [_modulation_float64(w, t, dm, None if m is None else m.double().cpu()) for w, t, m, dm in zip(wd, td, mags, dms)]
    gen = torch.Generator().manual_seed(2)
    lg, lw = 0, 0
    for l, (a, b) in enumerate(zip(got, want)):
        for j, (x, y) in enumerate(zip(a, b)):
            assert (x is None) == (y is None), (l, j)
            if y is None:
                continue
            if j == 0 and not dms[l]:
                assert torch.equal(x.cpu().double(), y.detach())
                continue
            _close(x, y, 1e-5, f'layer {l} output {j}')
            r = torch.randn(y.shape, generator=gen, dtype=torch.float64)
            lg, lw = lg + (x * r.float().cuda()).sum(), lw + (y * r).sum()
    gg = torch.autograd.grad(lg, ws + ts, allow_unused=True)
    gw = torch.autograd.grad(lw, wd + td, allow_unused=True)
    for i, (a, b) in enumerate(zip(gg, gw)):
        if b is None:                                   # the weight of the layer that does not demodulate (its w_hat is not in the loss)
            assert a is None or float(a.abs().max()) == 0.0, i
        else:
            _close(a, b, 1e-4, f'gradient {i}')


def test_modulation_over_the_channel_limit_raises():
    """16385 input channels: the bank's gate says no, and the per-layer path refuses the shape up front with a clear error (no eager
    fallback: a missing kernel is an error)."""
    from afcm_amd.torch_utils.ops import modulation_bank as mb
    from afcm_amd.torch_utils.ops.conv2d import modulation_coefficients_fused
    for o, i, dm in ((2, 16385, True), (2, 16385, False), (16385, 2, True)):
        w = torch.randn(o, i, 1, 1, device='cuda')
        t = torch.randn(3, i, device='cuda')
        assert not mb.supported([mb.Item(w, t, None, dm)])
        with pytest.raises(RuntimeError, match='16384'):
            modulation_coefficients_fused(w, t, demodulate=dm)


# ---- 4x4 pooling ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('planes', [1, 3, 4, 5])
@pytest.mark.parametrize('hw', [(4, 4), (12, 20), (36, 36), (38, 38)], ids=str)
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_pool4_vs_float64(planes, hw, dtype, monkeypatch):
    """SynthesisNetwork._pool4 (NET:636,683): the block-mean kernel for H % 4 == W % 4 == 0 with one, less than, exactly and more than one
    workgroup's four planes; 38 x 38 (margin_size 11) takes AdaptiveAvgPool2d with its uneven, overlapping bins.  Both against float64
    adaptive_avg_pool2d of the same (rounded) values, at the block kernel's bars (test_pool_blocks_matches_adaptive_avg_pool)."""
    from afcm_amd import networks_stylegan3 as net
    h, w = hw
    sn = net.SynthesisNetwork.__new__(net.SynthesisNetwork)
    torch.nn.Module.__init__(sn)
    sn.pool = torch.nn.AdaptiveAvgPool2d((4, 4))
    calls = []
    real = net._PoolBlocks.apply
    monkeypatch.setattr(net._PoolBlocks, 'apply', lambda x: calls.append(1) or real(x))
    g = torch.Generator().manual_seed(planes * 100 + h)
    x = torch.randn([1, planes, h, w], generator=g).to(dtype)
    r = torch.randn([1, planes, 4, 4], generator=g, dtype=torch.float64)
    xg = x.cuda().requires_grad_(True)
    got = sn._pool4(xg)
    ggot, = torch.autograd.grad((got * r.float().cuda()).sum(), [xg])
    assert len(calls) == (1 if h % 4 == 0 and w % 4 == 0 else 0)
    xd = x.double().requires_grad_(True)
    ref = torch.nn.functional.adaptive_avg_pool2d(xd, (4, 4))
    gref, = torch.autograd.grad((ref * r).sum(), [xd])
    assert got.dtype == torch.float32 and ggot.dtype == dtype
    _close(got, ref, 1e-6, 'y')
    _close(ggot, gref, {torch.bfloat16: 2.0 ** -8, torch.float32: 1e-6}[dtype], 'dx')
