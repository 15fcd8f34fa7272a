"""Radial (StyleGAN3-R) filtered_lrelu on the fused tile kernels (run with `-m gpu` on an MI355X).

A radial layer's down filter is a 12 x 12 2-D filter.  Its forward runs the SUFD form (separable up, 2-D down), its backward the FUSD
form (2-D up, separable down); csrc/filtered_lrelu_tile.hip flrelu_radial_kernel.  Bars: fp32 2e-5 x scale against the float64 oracle or
the reference's golden vectors (test_gpu_ops.py), 16-bit I/O 4e-3 (f16) / 3e-2 (bf16) as test_filtered_lrelu_16bit_io.
"""
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

TOL = 2e-5
TOL16 = {torch.float16: 4e-3, torch.bfloat16: 3e-2}
TINY = dict(channel_base=256, channel_max=8, num_layers=14, num_critical=2, margin_size=10, output_scale=0.25, skip_resolution=128,
            conv_kernel=3, filter_size=6, lrelu_upsampling=2, use_radial_filters=True, conv_clamp=256,
            magnitude_ema_beta=0.5 ** (16 / 20e3), cond_mod=True)


def _dev(a, grad=False, dtype=None):
    if a is None:
        return None
    t = torch.as_tensor(np.array(a) if isinstance(a, np.ndarray) else a).cuda()
    if dtype is not None:
        t = t.to(dtype)
    return t.requires_grad_(True) if grad else t


def _close(a, b, tol=TOL, what=''):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    assert err <= tol * scale, f'{what}: max-abs err {err:.3e} (scale {scale:.3g}, tol {tol:g})'
    return err


def _golden_args(g):
    up, down, *pad = [int(v) for v in g['meta']]
    gain, slope, clamp, flip = g['fmeta']
    return dict(up=up, down=down, padding=pad, gain=float(gain), slope=float(slope), clamp=None if clamp < 0 else float(clamp),
                flip_filter=bool(flip))


def _cfg(kw):
    pad = kw['padding']
    return (kw['up'], kw['down'], *pad, kw['gain'], kw['slope'], float('inf') if kw['clamp'] is None else kw['clamp'],
            kw['flip_filter'], 0, 0, 0)


def _oracle(x, fu, fd, b, r, kw):
    """float64 CPU oracle: y and (with r) dx, db of sum(y * r)."""
    from oracle import aten_ops as ops
    xs = torch.as_tensor(x).detach().double().cpu().requires_grad_(True)
    bs = None if b is None else torch.as_tensor(b).detach().double().cpu().requires_grad_(True)
    y = ops.filtered_lrelu(xs, fu=torch.as_tensor(fu).double().cpu(), fd=torch.as_tensor(fd).double().cpu(), b=bs, **kw)
    if r is None:
        return y.detach(), None, None
    gs = torch.autograd.grad((y * torch.as_tensor(r).double().cpu()).sum(), [xs] + ([bs] if bs is not None else []))
    return y.detach(), gs[0], (gs[1] if bs is not None else None)


def _radial_layers():
    from afcm_amd import layer_schedule
    pl = layer_schedule.plan(256, 4, 1, {'use_radial_filters': True})
    return [L for L in pl['enc'] + pl['dec'] if L['fd'] is not None and L['fd'].ndim == 2]


RADIAL = _radial_layers()


# ------------------------------------------------------------------------------------------------- 1: golden vectors
@pytest.mark.parametrize('name', ['F8_radial2d', 'R1_ups4_radial_down', 'R2_asym2d_up_flip', 'R2b_asym2d_up_noflip'])
def test_radial_golden_on_the_fused_kernels(name):
    from afcm_amd.torch_utils.ops import filtered_lrelu as flr
    g = load_golden(name)
    kw = _golden_args(g)
    x, b = _dev(g['x'], True), _dev(g['b'], True)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)      # no generic fallback, forward or backward
        y = flr.filtered_lrelu(x, fu=_dev(g['fu']), fd=_dev(g['fd']), b=b, **kw)
        _close(y, g['y'], what=name + ' y')
        dx, db = torch.autograd.grad((y * _dev(g['r'])).sum(), [x, b])
    _close(dx, g['dx'], what=name + ' dx')
    _close(db, g['db'], what=name + ' db', tol=1e-4)


# ------------------------------------------------------------------------------------------------- 2: every radial layer geometry
@pytest.mark.parametrize('li', range(len(RADIAL)), ids=[L['name'] for L in RADIAL])
def test_radial_layer_geometry_fp32_and_16bit(li):
    from afcm_amd.torch_utils.ops import filtered_lrelu as flr
    L = RADIAL[li]
    h = L['in_size'] + L['k'] - 1
    torch.manual_seed(li)
    x = torch.randn(1, 2, h, h)
    b = torch.randn(2) * 0.2
    kw = dict(up=L['up'], down=L['down'], padding=L['padding'], gain=float(np.sqrt(2)), slope=0.2, clamp=256.0, flip_filter=False)
    cfg = _cfg(kw)
    fu, fd = L['fu'].cuda(), L['fd'].cuda()
    # the forward and its transposed call both have fused kernels
    y, so, layout, _ = flr._run(x.cuda(), fu, fd, b.cuda(), None, cfg, True, no_fallback=True)
    assert layout == 0 and so is not None
    bcfg = flr._backward_cfg(cfg, fu, fd, x.shape, y.shape, layout)
    r = torch.randn(y.shape)
    dx, _, _, _ = flr._run(r.cuda(), fd, fu, None, so, bcfg, False, no_fallback=True)
    want, gx, gb = _oracle(x, L['fu'], L['fd'], b, r, kw)
    _close(y, want, what=L['name'] + ' y')
    _close(dx, gx, what=L['name'] + ' dx')
    # the same through autograd (db from the fused backward's dx)
    xg, bg = x.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        yg = flr.filtered_lrelu(xg, fu=fu, fd=fd, b=bg, **kw)
        dxg, dbg = torch.autograd.grad((yg * r.cuda()).sum(), [xg, bg])
    _close(dbg, gb, what=L['name'] + ' db', tol=1e-4)
    _close(dxg, gx, what=L['name'] + ' dx (autograd)')
    for dtype, tol in TOL16.items():
        x16, b16 = x.to(dtype), b.to(dtype)
        with warnings.catch_warnings():
            warnings.simplefilter('error', RuntimeWarning)
            y16 = flr.filtered_lrelu(x16.cuda(), fu=fu, fd=fd, b=b16.cuda(), **kw)
        assert y16.dtype == dtype
        ref, _, _ = _oracle(x16.double(), L['fu'], L['fd'], b16.double(), None, kw)
        _close(y16, ref, tol=tol, what=f'{L["name"]} {dtype}')


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('lname', ['encoder_12', 'L3_52_512', 'L9_148_181'])
def test_radial_16bit_backward_vs_float64(lname, dtype):
    """16-bit data through both directions: the fused forward writes the codes, the FUSD sign-read kernel (the backward of a radial layer;
    down 4 after the up-4 layer L3, down 2 otherwise) reads them.  y, dx and db against the float64 oracle on the same 16-bit-rounded
    x, b and cotangent, at the 16-bit I/O bar (the kernels compute in fp32; the error is the rounding of their 16-bit outputs)."""
    from afcm_amd.torch_utils.ops import filtered_lrelu as flr
    L = next(L for L in RADIAL if L['name'] == lname)
    tol = TOL16[dtype]
    h = L['in_size'] + L['k'] - 1
    torch.manual_seed(11)
    x = torch.randn(1, 2, h, h).to(dtype)
    b = (torch.randn(2) * 0.2).to(dtype)
    kw = dict(up=L['up'], down=L['down'], padding=L['padding'], gain=float(np.sqrt(2)), slope=0.2, clamp=256.0, flip_filter=False)
    cfg = _cfg(kw)
    fu, fd = L['fu'].cuda(), L['fd'].cuda()
    y, so, layout, _ = flr._run(x.cuda(), fu, fd, b.cuda(), None, cfg, True, no_fallback=True)
    assert layout == 0 and y.dtype == dtype
    r = torch.randn(y.shape).to(dtype)
    bcfg = flr._backward_cfg(cfg, fu, fd, x.shape, y.shape, layout)
    dx, _, _, _ = flr._run(r.cuda(), fd, fu, None, so, bcfg, False, no_fallback=True)
    assert dx.dtype == dtype
    want, gx, gb = _oracle(x.double(), L['fu'], L['fd'], b.double(), r.double(), kw)
    _close(y, want, tol=tol, what=f'{lname} {dtype} y')
    _close(dx, gx, tol=tol, what=f'{lname} {dtype} dx (_run)')
    xg, bg = x.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        yg = flr.filtered_lrelu(xg, fu=fu, fd=fd, b=bg, **kw)
        dxg, dbg = torch.autograd.grad((yg * r.cuda()).sum(), [xg, bg])
    assert dxg.dtype == dtype and dbg.dtype == dtype
    _close(dxg, gx, tol=tol, what=f'{lname} {dtype} dx')
    _close(dbg, gb, tol=tol, what=f'{lname} {dtype} db')


def _edge_cases():
    from afcm_amd import layer_schedule
    fr = layer_schedule.design_lowpass_filter(12, 56.0, 2 * (160.0 - 56.0), 512, radial=True)
    fu12 = layer_schedule.design_lowpass_filter(12, 64.0, 2 * (181.02 - 64.0), 512)
    fu24 = layer_schedule.design_lowpass_filter(24, 20.0, 2 * (64.0 - 20.0), 512)
    fd24 = fu24
    cases = []
    # SUFD up 2 / down 2: odd widths, a plane narrower than one tile, crop padding, clamp on / off, no bias
    cases.append(('sufd22_odd', [2, 3, 21, 37], fu12, fr, 2, 2, [9, 8, 7, 10], 256.0, True))
    cases.append(('sufd22_narrow', [1, 2, 9, 13], fu12, fr, 2, 2, [9, 8, 9, 8], None, False))
    cases.append(('sufd22_crop_clamp', [1, 2, 90, 71], fu12, fr, 2, 2, [-11, -12, -5, -4], 0.5, True))
    cases.append(('sufd22_multitile', [1, 1, 150, 133], fu12, fr, 2, 2, [9, 8, 9, 8], 256.0, True))
    # SUFD up 4 / down 2
    cases.append(('sufd42_crop', [1, 2, 38, 38], fu24, fr, 4, 2, [-6, -9, -6, -9], 256.0, True))
    cases.append(('sufd42_odd_noclamp', [1, 2, 45, 27], fu24, fr, 4, 2, [-6, -9, -7, -8], None, False))
    # FUSD (a forward with a 2-D up filter writes the codes of the tile family): up 2 / down 2 and up 2 / down 4
    cases.append(('fusd22_odd', [2, 2, 23, 19], fr, fu12, 2, 2, [9, 8, 10, 7], 256.0, True))
    cases.append(('fusd22_narrow_clamp', [1, 2, 11, 8], fr, fu12, 2, 2, [9, 8, 9, 8], 0.5, False))
    cases.append(('fusd22_multitile_crop', [1, 1, 140, 90], fr, fu12, 2, 2, [-3, -4, -9, -2], 256.0, True))
    cases.append(('fusd24', [1, 2, 38, 38], fr, fd24, 2, 4, [34, 33, 34, 33], 256.0, True))
    cases.append(('fusd24_odd_noclamp', [1, 2, 57, 41], fr, fd24, 2, 4, [33, 35, 31, 34], None, False))
    return cases


EDGE = _edge_cases()


@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('ci', range(len(EDGE)), ids=[c[0] for c in EDGE])
def test_radial_edges_fp32_vs_float64(ci, flip):
    from afcm_amd.torch_utils.ops import filtered_lrelu as flr
    name, shape, fu, fd, up, down, pad, clamp, bias = EDGE[ci]
    torch.manual_seed(ci)
    x = torch.randn(shape) * (3.0 if clamp == 0.5 else 1.0)
    b = torch.randn(shape[1]) * 0.3 if bias else None
    kw = dict(up=up, down=down, padding=pad, gain=float(np.sqrt(2)), slope=0.2, clamp=clamp, flip_filter=flip)
    cfg = _cfg(kw)
    y, so, layout, _ = flr._run(x.cuda(), fu.cuda(), fd.cuda(), _dev(b), None, cfg, True, no_fallback=True)
    bcfg = flr._backward_cfg(cfg, fu, fd, x.shape, y.shape, layout)
    flr._run(torch.ones_like(y), fd.cuda(), fu.cuda(), None, so, bcfg, False, no_fallback=True)
    r = torch.randn(y.shape)
    xg = x.cuda().requires_grad_(True)
    bg = None if b is None else b.cuda().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        yg = flr.filtered_lrelu(xg, fu=fu.cuda(), fd=fd.cuda(), b=bg, **kw)
        gs = torch.autograd.grad((yg * r.cuda()).sum(), [xg] + ([bg] if bg is not None else []))
    want, gx, gb = _oracle(x, fu, fd, b, r, kw)
    _close(y, want, what=name + ' y (_run)')
    _close(yg, want, what=name + ' y')
    _close(gs[0], gx, what=name + ' dx')
    if b is not None:
        _close(gs[1], gb, what=name + ' db', tol=1e-4)
    for dtype, tol in TOL16.items():
        with warnings.catch_warnings():
            warnings.simplefilter('error', RuntimeWarning)
            y16 = flr.filtered_lrelu(x.to(dtype).cuda(), fu=fu.cuda(), fd=fd.cuda(), b=None if b is None else b.to(dtype).cuda(), **kw)
        ref, _, _ = _oracle(x.to(dtype).double(), fu, fd, None if b is None else b.to(dtype).double(), None, kw)
        _close(y16, ref, tol=tol, what=f'{name} {dtype}')


# ------------------------------------------------------------------------------------------------- 3: sign codes
@pytest.mark.parametrize('name', ['F8_radial2d', 'R1_ups4_radial_down', 'R2_asym2d_up_flip', 'R2b_asym2d_up_noflip'])
def test_radial_sign_codes_bit_exact(name):
    """The layout-0 codes the radial kernels write equal the definition-level restatement wherever the pre-activation is not within
    rounding distance of 0 or of the clamp (method of test_filtered_lrelu_sign_codes_bit_exact)."""
    from afcm_amd.torch_utils.ops.filtered_lrelu import _FilteredLRelu
    from oracle import direct_np as dnp
    g = load_golden(name)
    kw = _golden_args(g)
    up, pad = kw['up'], kw['padding']
    x = _dev(g['x'], True)
    y = _FilteredLRelu.apply(x, _dev(g['fu']), _dev(g['fd']), _dev(g['b']), None, _cfg(kw))
    assert y.grad_fn.sign_layout == 0
    signs = y.grad_fn.saved_tensors[2].cpu().numpy()
    xb = g['x'].astype(np.float64) + g['b'].astype(np.float64).reshape(1, -1, 1, 1)
    u = dnp.upfirdn2d(xb, g['fu'], up=up, padding=pad, gain=float(up * up), flip_filter=kw['flip_filter'])
    _, codes = dnp.lrelu_codes(u, kw['gain'], kw['slope'], kw['clamp'])
    sh, sw = signs.shape[2], signs.shape[3] * 4
    assert sh <= codes.shape[2] and codes.shape[3] <= sw
    got = np.stack([(signs >> (2 * k)) & 3 for k in range(4)], axis=-1).reshape(*signs.shape[:3], sw)
    w = codes.shape[3]
    margin = 1e-4 * max(1.0, np.abs(u).max())
    safe = (np.abs(u[:, :, :sh]) > margin) | (u[:, :, :sh] == 0)
    if kw['clamp'] is not None:
        safe &= np.abs(np.abs(u[:, :, :sh] * kw['gain'] * np.where(u[:, :, :sh] < 0, kw['slope'], 1.0)) - kw['clamp']) > 1e-3
    assert safe.mean() > 0.95
    assert np.array_equal(got[..., :w][safe], codes[:, :, :sh, :][safe])


# ------------------------------------------------------------------------------------------------- 4: asymmetric 2-D filters
@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('mode', ['sufd22', 'sufd42', 'fusd22', 'fusd24'])
def test_asymmetric_2d_filters(mode, flip):
    from afcm_amd import layer_schedule
    from afcm_amd.torch_utils.ops import filtered_lrelu as flr
    gen = torch.Generator().manual_seed(7)
    f2 = torch.randn(12, 12, generator=gen)
    f2 = f2 / f2.abs().sum() * 4
    f12 = layer_schedule.design_lowpass_filter(12, 64.0, 2 * (181.02 - 64.0), 512)
    f24 = layer_schedule.design_lowpass_filter(24, 20.0, 2 * (64.0 - 20.0), 512)
    fu, fd, up, down, pad = {'sufd22': (f12, f2, 2, 2, [9, 8, 10, 7]), 'sufd42': (f24, f2, 4, 2, [-6, -9, -5, -8]),
                             'fusd22': (f2, f12, 2, 2, [8, 9, 10, 7]), 'fusd24': (f2, f24, 2, 4, [33, 35, 31, 34])}[mode]
    x = torch.randn(1, 2, 30, 35, generator=gen)
    b = torch.randn(2, generator=gen) * 0.3
    kw = dict(up=up, down=down, padding=pad, gain=float(np.sqrt(2)), slope=0.2, clamp=256.0, flip_filter=flip)
    xg, bg = x.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        y = flr.filtered_lrelu(xg, fu=fu.cuda(), fd=fd.cuda(), b=bg, **kw)
        r = torch.randn(y.shape, generator=gen)
        dx, db = torch.autograd.grad((y * r.cuda()).sum(), [xg, bg])
    want, gx, gb = _oracle(x, fu, fd, b, r, kw)
    _close(y, want, what=f'{mode} flip={flip} y')
    _close(dx, gx, what=f'{mode} flip={flip} dx')
    _close(db, gb, what=f'{mode} flip={flip} db', tol=1e-4)


# ------------------------------------------------------------------------------------------------- 5: second order
@pytest.mark.parametrize('name', ['F8_radial2d', 'R1_ups4_radial_down'])
def test_radial_second_order(name):
    """create_graph=True: dx is itself differentiable in dy (the recorded transposed call's backward is the forward op again, in
    sign-read mode).  dx is linear in dy for fixed codes, so d<dx, v>/d(dy) is the forward op applied to v on the codes of x."""
    from afcm_amd.torch_utils.ops import filtered_lrelu as flr
    from oracle import aten_ops as ops
    g = load_golden(name)
    kw = _golden_args(g)
    x = _dev(g['x'], True)
    v = torch.randn(g['x'].shape, generator=torch.Generator().manual_seed(3))
    xs = torch.from_numpy(g['x']).double().requires_grad_(True)
    # the recorded backward call runs forward again on the transposed op: its own gradient w.r.t. dy
    dy = _dev(g['r'], True)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        y = flr.filtered_lrelu(x, fu=_dev(g['fu']), fd=_dev(g['fd']), b=_dev(g['b']), **kw)
        dx, = torch.autograd.grad(y, [x], dy, create_graph=True)
        ddy, = torch.autograd.grad((dx * v.cuda()).sum(), [dy])
    ysv = ops.filtered_lrelu(xs, fu=torch.from_numpy(g['fu']).double(), fd=torch.from_numpy(g['fd']).double(),
                             b=torch.from_numpy(g['b']).double(), **kw)
    dys = torch.from_numpy(g['r']).double().requires_grad_(True)
    gx2, = torch.autograd.grad(ysv, [xs], dys, create_graph=True)
    ref2, = torch.autograd.grad((gx2 * v.double()).sum(), [dys])
    _close(dx, gx2, what=name + ' dx (create_graph)')
    _close(ddy, ref2, what=name + ' d(dx)/d(dy)')


# ------------------------------------------------------------------------------------------------- 6: plugin / operator surfaces
def _plugin_pair(call, g):
    kw = _golden_args(g)
    up, down, (px0, px1, py0, py1) = kw['up'], kw['down'], kw['padding']
    gain, slope, flip = kw['gain'], kw['slope'], kw['flip_filter']
    clamp = float('inf') if kw['clamp'] is None else kw['clamp']
    x, fu, fd, r, b = _dev(g['x']), _dev(g['fu']), _dev(g['fd']), _dev(g['r']), _dev(g['b'])
    empty = torch.empty([0], dtype=torch.uint8, device='cuda')
    y, so, rc = call(x, fu, fd, b, empty, up, down, px0, px1, py0, py1, 0, 0, gain, slope, clamp, flip, True)
    assert rc == 0 and so.dtype == torch.uint8 and so.ndim == 4
    fuw, fdw = fu.shape[-1], fd.shape[-1]
    fuh, fdh = fu.shape[0] if fu.ndim == 2 else fuw, fd.shape[0] if fd.ndim == 2 else fdw
    pp = [(fuw - 1) + (fdw - 1) - px0, x.shape[3] * up - y.shape[3] * down + px0 - (up - 1),
          (fuh - 1) + (fdh - 1) - py0, x.shape[2] * up - y.shape[2] * down + py0 - (up - 1)]
    dx, so2, rc2 = call(r.contiguous(), fd, fu, torch.zeros_like(b), so, down, up, *pp, px0 - (fuw - 1), py0 - (fuh - 1),
                        gain * (up ** 2) / (down ** 2), slope, float('inf'), not flip, False)
    assert rc2 == 0 and so2.numel() == 0
    return y, dx


@pytest.mark.parametrize('name', ['F8_radial2d', 'R1_ups4_radial_down', 'R2_asym2d_up_flip'])
def test_plugin_and_registered_op_run_radial_calls(name):
    import afcm_amd  # noqa: F401  (registers the operator library)
    from afcm_amd.torch_utils import custom_ops
    plugin = custom_ops.get_plugin(module_name='filtered_lrelu_plugin', sources=[], headers=[], source_dir='.')
    g = load_golden(name)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        for what, call in (('plugin', plugin.filtered_lrelu), ('torch.ops.afcm', torch.ops.afcm.filtered_lrelu)):
            y, dx = _plugin_pair(call, g)
            _close(y, g['y'], what=f'{name} y ({what})')
            _close(dx, g['dx'], what=f'{name} dx ({what})')


def test_2d_argument_sets_outside_the_radial_cases_still_fall_back():
    from afcm_amd.torch_utils import custom_ops
    from afcm_amd.torch_utils.ops import filtered_lrelu as flr
    plugin = custom_ops.get_plugin('filtered_lrelu_plugin')
    torch.manual_seed(5)
    f2 = torch.randn(12, 12, device='cuda') / 30
    f1 = torch.randn(12, device='cuda') / 5
    x = torch.randn(1, 2, 20, 20, device='cuda')
    e = torch.empty([0], dtype=torch.uint8, device='cuda')
    z = torch.zeros(2, device='cuda')
    for fu, fd, up, down in ((f2, f2, 2, 2), (f1, f2, 2, 4), (f2, f1, 4, 2), (f2[:, :10].contiguous(), f1, 2, 2)):
        y, so, rc = plugin.filtered_lrelu(x, fu, fd, z, e, up, down, 9, 8, 9, 8, 0, 0, 1.0, 0.2, float('inf'), False, True)
        assert rc == -1 and y.numel() == 0 and so.numel() == 0, (tuple(fu.shape), tuple(fd.shape), up, down)
    with pytest.warns(RuntimeWarning):
        flr.filtered_lrelu(x, fu=f2, fd=f2, up=2, down=2, padding=[9, 8, 9, 8])


# ------------------------------------------------------------------------------------------------- 7: memory
def test_radial_forward_keeps_the_upsampled_intermediate_on_chip():
    from afcm_amd.torch_utils.ops import filtered_lrelu as flr
    L = next(L for L in RADIAL if L['out_size'] == 276 and L['in_size'] == 276)
    h = L['in_size'] + L['k'] - 1
    torch.manual_seed(0)
    x = torch.randn(2, 64, h, h, device='cuda', requires_grad=True)
    b = torch.randn(64, device='cuda') * 0.1
    fu, fd = L['fu'].cuda(), L['fd'].cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        y = flr.filtered_lrelu(x, fu=fu, fd=fd, b=b, up=L['up'], down=L['down'], padding=L['padding'], gain=float(np.sqrt(2)),
                               slope=0.2, clamp=256.0)
    torch.cuda.synchronize()
    signs = y.grad_fn.saved_tensors[2]
    out = y.numel() * y.element_size() + signs.numel()
    assert y.numel() * y.element_size() >= 30e6
    grew = torch.cuda.max_memory_allocated() - before
    assert grew < 1.25 * out, f'peak grew by {grew / 1e6:.1f} MB for {out / 1e6:.1f} MB of y + signs'


# ------------------------------------------------------------------------------------------------- 8-10: the radial generator
def _tiny_radial(dtype):
    from afcm_amd.networks_stylegan3 import Stylegan3Generator
    return Stylegan3Generator(z_dim=32, c_dim=1, w_dim=32, img_resolution=128, img_channels_in=4, img_channels_out=1,
                              mapping_kwargs=dict(num_layers=2), synthesis_kwargs=dict(TINY, compute_dtype=dtype))


def test_radial_generator_matches_reference_golden():
    """Bars of test_generator_matches_reference_golden on the R3 fixture (the G1 recipe with use_radial_filters=True)."""
    g = load_golden('R3_tiny128_radial')
    G = _tiny_radial(torch.float32).eval()
    G.load_state_dict({k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith('sd/')}, strict=True)
    G = G.cuda()
    feats = {}
    for lname, mod in G.synthesis.named_children():
        if hasattr(mod, 'up_factor'):
            mod.register_forward_hook(lambda m, i, o, lname=lname: feats.__setitem__(lname, o.detach()))
    z, c, x = (torch.from_numpy(g[k]).cuda() for k in ('z', 'c', 'x'))
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        y = G(z, c, x)
        err = (y.cpu() - torch.from_numpy(g['y'])).abs().max().item()
        assert err <= 5e-5 * max(1.0, float(np.abs(g['y']).max())), f'forward max-abs {err:.3e}'
        assert [str(n) for n in g['layer_names']] == list(feats.keys())
        for lname, t in feats.items():
            st = g['stat/' + lname]
            got = np.array([t.float().mean().item(), t.float().std().item(), t.float().abs().max().item()])
            assert np.allclose(got, st, rtol=1e-3, atol=1e-5), (lname, got, st)
        want = {k[5:]: v for k, v in g.items() if k.startswith('grad/')}
        params = dict(G.named_parameters())
        grads = torch.autograd.grad((y * torch.from_numpy(g['r']).cuda()).sum(), [params[k] for k in want])
    for k, gr in zip(want, grads):
        w = want[k]
        d = gr.cpu().numpy().astype(np.float64) - w
        rel_l2 = float(np.sqrt((d ** 2).sum()) / max(1e-30, np.sqrt((w.astype(np.float64) ** 2).sum())))
        assert rel_l2 <= 1e-2, f'grad {k}: relative L2 error {rel_l2:.3e}'


def _psnr_vs_float64(radial):
    """(bf16, f16) PSNR of the tiny generator against the float64 oracle on a random state dict; for the radial configuration
    the oracle's plain-data plan gets the radial down filters of the layer schedule."""
    from afcm_amd import layer_schedule
    from afcm_amd.networks_stylegan3 import Stylegan3Generator
    from oracle import generator as ogen
    skw = dict(TINY, use_radial_filters=radial)
    pl = ogen.plan(128, 4, 1, {k: v for k, v in skw.items() if k not in ('use_radial_filters', 'magnitude_ema_beta')})
    if radial:
        sched = layer_schedule.plan(128, 4, 1, skw)
        fds = {L['name']: L['fd'] for L in sched['enc'] + sched['dec'] if L['fd'] is not None and L['fd'].ndim == 2}
        n = 0
        for L in pl['enc'] + pl['dec']:
            if L['name'] in fds:
                L['fd'] = fds[L['name']]
                n += 1
        assert n == len(fds) == 14
    sd = ogen.random_state_dict(pl, 32, 1, 32, 2, seed=0)
    gen = torch.Generator().manual_seed(1)
    z, c = torch.randn(2, 32, generator=gen), torch.rand(2, 1, generator=gen)
    x = torch.randn(2, 4, 128, 128, generator=gen)
    want = ogen.generator({k: v.double() for k, v in sd.items()}, pl, z.double(), c.double(), x.double(), mapping_layers=2)
    out = []
    for dtype in (torch.bfloat16, torch.float16):
        G = Stylegan3Generator(z_dim=32, c_dim=1, w_dim=32, img_resolution=128, img_channels_in=4, img_channels_out=1,
                               mapping_kwargs=dict(num_layers=2), synthesis_kwargs=dict(skw, compute_dtype=dtype)).eval()
        missing, unexpected = G.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.endswith('_filter') for k in missing)
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter('error', RuntimeWarning)
            y = G.cuda()(z.cuda(), c.cuda(), x.cuda()).double().cpu()
        assert torch.isfinite(y).all()
        out.append(10 * np.log10(float((want.max() - want.min()) ** 2) / max(1e-30, float(((y - want) ** 2).mean()))))
    return out


def test_16bit_radial_generator_vs_float64_oracle():
    base = _psnr_vs_float64(False)
    got = _psnr_vs_float64(True)
    print(f'radial: bf16 {got[0]:.1f} dB, f16 {got[1]:.1f} dB; default: bf16 {base[0]:.1f} dB, f16 {base[1]:.1f} dB')
    for dtype, p, p0 in zip(('bf16', 'f16'), got, base):
        assert p >= p0 - 7.0, f'{dtype}: {p:.1f} dB vs the oracle, the default tiny configuration {p0:.1f} dB'


def test_bf16_radial_generator_training_step():
    from afcm_amd import synthetic
    from afcm_amd.stylegan3_model import StyleGAN3GeneratorStep
    torch.manual_seed(0)
    G = _tiny_radial(torch.bfloat16).cuda()
    step = StyleGAN3GeneratorStep(G, lambda_L1=100.0)
    a, b, z, c = synthetic.generator_inputs(2, size=128, z_dim=32, seed=3, device='cuda')
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        step.set_input(a, b, z, c)
        step.optimize_parameters()
    loss = float(step.loss_G)
    assert np.isfinite(loss), loss
