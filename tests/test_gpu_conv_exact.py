"""Every conv2d kernel against exact integer arithmetic, bit for bit (helper, conditions and case tables: conv_exact_ref.py).

The operands are small integers times powers of two, for which every fp32 partial sum of every summation order is exact: forward,
data gradient, weight gradient and scale gradients have ONE right answer per element -- the float64 reference cast to the output type --
and every comparison here is ``torch.equal``.  Which kernel a case reaches is asserted through the library's plan queries
(afcm_conv2d_plan, afcm_conv2d_wgrad_plan); the second-round cases take their batch from the plan on this device and assert
items > grid, so they cannot pass without the persistent loop having gone round.  A failure names the count and the first wrong indices
next to the plan (tile, block rows, items, grid): element (n, o, p, q) lies in tile (p // th, q // tw), row block o // rows.

Not covered: tensors above 2 GB (the per-piece descriptor form of the granule weight-gradient kernel).
"""
import pytest
import torch

import conv_exact_ref as R

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
HALVES = [BF16, F16]
_ids = R.case_id


@pytest.fixture(scope='module')
def lib():
    from afcm_amd import _lib
    return _lib.load()


def _conv():
    from afcm_amd.torch_utils.ops import conv2d as conv
    return conv


def _dev(t, dtype):
    return None if t is None else t.to(dtype).cuda()


def _pitched(t, fill=float('nan')):
    """A row-pitched copy of t whose padding columns hold ``fill``."""
    from afcm_amd.torch_utils.ops import _rows
    n, c, h, w = t.shape
    ld = (w + 31) // 32 * 32 + 32
    buf = torch.full([n, c, h, ld], fill, dtype=t.dtype, device=t.device)
    buf[..., :w] = t
    v = buf[..., :w]
    assert _rows.pitch_of(v) == ld and not v.is_contiguous()
    return v


def _forward_variants(node, dtype, ks, what, **kw):
    """_conv_raw with every combination of the per-plane output scale and the bias, each held to the reference."""
    conv = _conv()
    cout = node.w.shape[0]
    x = kw.pop('x', None)
    x = _dev(node.x, dtype) if x is None else x
    wp, rows_pad = conv.pack_weights(node.w.float().cuda(), dtype, 0)
    out = {}
    for (sc, bi), ref in node.forward_variants().items():
        y = conv._conv_raw(x, wp, rows_pad, _dev(node.d, F32) if sc else None, cout, ks, node.pad, obias=_dev(node.b, F32) if bi else None, **kw)
        assert y.dtype == dtype
        R.assert_exact(y, ref, f'{what} scale={sc} bias={bi}')
        out[(sc, bi)] = y
    return out


# ---- forward = data-gradient kernel, 16-bit 3x3 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', HALVES, ids=_ids)
@pytest.mark.parametrize('case', R.FWD16, ids=_ids)
def test_forward_3x3(case, dtype, lib):
    shape = R.with_batch(lib, case, dtype)
    pl = R.conv_plan(lib, dtype, *shape[:5], 3, shape[5])
    assert (pl.family, pl.fast) == (case.family, case.fast), pl
    if case.shape[0] is None:
        assert pl.items > pl.grid and pl.items % pl.grid != 0, pl          # a second round, its last one ragged
    node = R.forward_node(shape, case, dtype)
    node.check(dtype, ('y',))
    _forward_variants(node, dtype, 3, f'{shape} {pl}')


@pytest.mark.parametrize('dtype', HALVES, ids=_ids)
@pytest.mark.parametrize('case', R.PITCHED16, ids=_ids)
def test_forward_3x3_row_pitched(case, dtype, lib, monkeypatch):
    """NaN in the input's padding columns, NaN under the whole output buffer: the result is the reference, the output's padding is finite
    up to the next multiple of 8 columns (the contract of afcm_conv2d_ld), and the dense run of the same case is the reference too."""
    from afcm_amd.torch_utils.ops import _rows
    monkeypatch.setattr(_rows, 'MAX_OVERHEAD', 10.0)
    empty = _rows.empty

    def nan_empty(shape, dtype_, device, pitched=True):
        t = empty(shape, dtype_, device, pitched)
        (_rows.whole_buffer(t) if not t.is_contiguous() else t).fill_(float('nan'))
        return t
    monkeypatch.setattr(_rows, 'empty', nan_empty)
    shape = case.shape
    node = R.forward_node(shape, case, dtype)
    node.check(dtype, ('y',))
    q = node.y.shape[3]
    ldy = _rows.pitch_for(q, dtype)
    assert ldy != q
    pl = R.conv_plan(lib, dtype, *shape[:5], 3, shape[5], y_pitch=ldy)
    assert (pl.family, pl.fast) == (case.family, case.fast), pl
    xp = _pitched(_dev(node.x, dtype))
    for y in _forward_variants(node, dtype, 3, f'pitched {shape} {pl}', x=xp, pitched_out=True).values():
        assert _rows.pitch_of(y) == ldy and not y.is_contiguous()
        pad = _rows.whole_buffer(y)[..., q:(q + 7) // 8 * 8]
        assert torch.isfinite(pad.float()).all()
    _forward_variants(node, dtype, 3, f'pitched in, dense out {shape}', x=xp)
    _forward_variants(node, dtype, 3, f'dense {shape}')


# ---- 1x1 16-bit forward and data gradient ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', HALVES, ids=_ids)
@pytest.mark.parametrize('case', R.FWD16_1X1, ids=_ids)
def test_forward_and_data_gradient_1x1(case, dtype, lib):
    conv = _conv()
    n, cin, cout, h, w, _ = case.shape
    pl = R.conv_plan(lib, dtype, n, cin, cout, h, w, 1, 0)
    assert (pl.family, pl.kernel) == (case.family, R.K_GENERAL16), pl
    node = R.onebyone_node(case, dtype)
    node.check(dtype, ('y', 'dx'))
    _forward_variants(node, dtype, 1, f'{case.shape} {pl}')
    wpt, rows_pad = conv.pack_weights(node.w.float().cuda(), dtype, 1)
    dx = conv._conv_raw(_dev(node.dys, dtype), wpt, rows_pad, None, cin, 1, 0)
    R.assert_exact(dx, node.dx, f'{case.shape} dx {R.conv_plan(lib, dtype, n, cout, cin, h, w, 1, 0)}')


# ---- fp32: the split route at three settings, the native kernels --------------------------------------------------------------------------
@pytest.mark.parametrize('split', [None, (BF16, 6, 6, 6), (BF16, 3, 3, 3)], ids=_ids)
@pytest.mark.parametrize('case', R.FWD32_SPLIT, ids=_ids)
def test_forward_fp32_split_route(case, split, lib, monkeypatch):
    conv = _conv()
    if split is not None:
        monkeypatch.setattr(conv, 'FP32_SPLIT', split)
    assert conv.FP32_SPLIT is not None and (split is not None or conv.FP32_SPLIT[0] == F16)
    part = conv.FP32_SPLIT[0]
    shape = R.with_batch(lib, case, part, split=True)
    pl = R.conv_plan(lib, part, *shape[:5], 3, shape[5], split=True)
    assert (pl.family, pl.kernel) == (case.family, R.K_SPLIT), pl
    if case.shape[0] is None:
        assert pl.items > pl.grid and pl.items % pl.grid != 0, pl
    node = R.forward_node(shape, case, F32, in_scale=True, bias=False)
    node.check(F32, ('y',))
    x = _dev(node.x, F32)
    assert conv._split_plan(x, 3, shape[2], shape[5]) is not None
    y = conv.scaled_conv2d(x, _dev(node.w, F32), _dev(node.s, F32), _dev(node.d, F32), shape[5])
    assert y.dtype == F32
    R.assert_exact(y, node.y, f'{shape} {conv.FP32_SPLIT} {pl}')


@pytest.mark.parametrize('split_off', [True, False], ids=['FP32_SPLIT=None', 'default'])
@pytest.mark.parametrize('case,ks', [(c, 3) for c in R.FWD32_NATIVE] + [(c, 1) for c in R.FWD32_NATIVE_1X1], ids=_ids)
def test_forward_fp32_native_kernels(case, ks, split_off, lib, monkeypatch):
    """conv2d_fwd_kernel<float, 64 | 128, 3 | 1>: what FP32_SPLIT = None selects, and what odd widths (and 1x1) get under the default."""
    conv = _conv()
    if split_off:
        monkeypatch.setattr(conv, 'FP32_SPLIT', None)
    shape = case.shape
    pl = R.conv_plan(lib, F32, *shape[:5], ks, shape[5])
    assert (pl.family, pl.kernel) == (case.family, R.K_F32), pl
    node = R.forward_node(shape, case, F32, ks=ks, in_scale=True, bias=False)
    node.check(F32, ('y',))
    x = _dev(node.x, F32)
    assert conv._split_plan(x, ks, shape[2], shape[5]) is None           # odd width, 1x1 or switched off: the native kernels
    y = conv.scaled_conv2d(x, _dev(node.w, F32), _dev(node.s, F32), _dev(node.d, F32), shape[5])
    R.assert_exact(y, node.y, f'{shape} {pl}')
    # the same kernel with a bias, through the raw entry point
    _forward_variants(R.forward_node(shape, case, F32, ks=ks), F32, ks, f'raw {shape} {pl}')


# ---- stride 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', HALVES, ids=_ids)
@pytest.mark.parametrize('shape,kind', R.STRIDE2, ids=_ids)
def test_stride2_forward_and_gradients(shape, kind, dtype):
    conv = _conv()
    node = R.stride2_node(shape, kind, dtype)
    node.check(dtype, ('y', 'dx', 'dw'))
    x, w = _dev(node.x, dtype).requires_grad_(True), _dev(node.w, F32).requires_grad_(True)
    assert conv.strided_conv2d_supported(x, w, shape[5])
    y = conv.strided_conv2d(x, w, shape[5])
    R.assert_exact(y, node.y, f'{shape} y')
    dx, dw = torch.autograd.grad(y, [x, w], grad_outputs=_dev(node.dy, dtype))
    R.assert_exact(dx, node.dx, f'{shape} dx')
    R.assert_exact(dw, node.dw, f'{shape} dw')


# ---- weight gradient ----------------------------------------------------------------------------------------------------------------------
def _wgrad(node, dtype, case):
    n, cin, cout, h, w, pad = case.shape
    return _conv()._wgrad_raw(_dev(node.dy, dtype), _dev(node.x, dtype), cout, cin, case.ks, pad)


@pytest.mark.parametrize('dtype', HALVES, ids=_ids)
@pytest.mark.parametrize('case', R.WGRAD16_GRANULE, ids=_ids)
def test_wgrad_granule_kernel(case, dtype, lib):
    pl = R.wgrad_plan(lib, dtype, *case.shape[:5], case.ks, case.shape[5])
    assert (pl.kernel, pl.x16, pl.small) == (R.WG_GRANULE, case.x16, 1), pl
    node = R.wgrad_node(case, dtype)
    node.check(dtype, ('dw',))
    dw = _wgrad(node, dtype, case)
    assert dw.dtype == F32
    R.assert_exact(dw, node.dw, f'{case.shape} {pl}')


@pytest.mark.parametrize('dtype', HALVES, ids=_ids)
@pytest.mark.parametrize('case', R.WGRAD16_DWORD, ids=_ids)
def test_wgrad_dword_kernel(case, dtype, lib, monkeypatch):
    """conv2d_wgrad16_kernel<T, 3, 0 | 1>: pad 0 as it is dispatched; pad 1 with the framing threshold at 0 (the production path of
    the discriminator's large planes) and, at the default threshold, the framed pad-2 route on the same inputs."""
    conv = _conv()
    pad = case.shape[5]
    pl = R.wgrad_plan(lib, dtype, *case.shape[:5], 3, pad)
    assert (pl.kernel, pl.pad_odd) == (R.WG_DWORD, pad), pl
    node = R.wgrad_node(case, dtype)
    node.check(dtype, ('dw',))
    if pad == 1:
        dy = _dev(node.dy, dtype)
        assert conv._frame_dy(dy, 3, 1)[1] == 2
        R.assert_exact(_wgrad(node, dtype, case), node.dw, f'{case.shape} framed')
        monkeypatch.setattr(conv, '_FRAME_WGRAD_MAX', 0)
        assert conv._frame_dy(dy, 3, 1)[1] == 1
    R.assert_exact(_wgrad(node, dtype, case), node.dw, f'{case.shape} {pl}')


@pytest.mark.parametrize('case', R.WGRAD32, ids=_ids)
def test_wgrad_fp32_native_kernels(case, lib):
    pl = R.wgrad_plan(lib, F32, *case.shape[:5], case.ks, case.shape[5])
    assert (pl.kernel, pl.pad_odd) == (R.WG_F32, case.shape[5] & 1 if case.ks == 3 else 0), pl
    node = R.wgrad_node(case, F32)
    node.check(F32, ('dw',))
    R.assert_exact(_wgrad(node, F32, case), node.dw, f'{case.shape} {pl}')


@pytest.mark.parametrize('dtype', HALVES, ids=_ids)
@pytest.mark.parametrize('shape', R.WGRAD_DOTS + [R.WGRAD_DOTS_NONE], ids=_ids)
def test_wgrad_image_aligned_slabs(shape, dtype, lib):
    conv = _conv()
    n, cin, cout, h, w, pad = shape
    node = R.dots_node(shape, dtype)
    node.check(dtype, ('dx', 'dw'))
    pl = R.wgrad_plan(lib, dtype, n, cin, cout, h, w, 3, pad, dots=True)
    dw, dots = conv._wgrad_raw(_dev(node.dy, dtype), _dev(node.x, dtype), cout, cin, 3, pad, dots_with=_dev(node.w, F32))
    R.assert_exact(dw, node.dw, f'{shape} dw {pl}')
    if shape == R.WGRAD_DOTS_NONE:
        assert pl is None and dots is None
        return
    assert pl.reduce == R.RED_DOTS and pl.splits_img * n == pl.splits, pl
    R.assert_exact(dots, node.dots, f'{shape} dots {pl}')


# ---- the autograd nodes end to end --------------------------------------------------------------------------------------------------------
ROUTES = [('bfloat16', BF16, False), ('float16', F16, False), ('fp32-split', F32, False), ('fp32-native', F32, True)]


@pytest.mark.parametrize('route,dtype,split_off', ROUTES, ids=[r[0] for r in ROUTES])
@pytest.mark.parametrize('shape', R.NODES, ids=_ids)
def test_scaled_conv2d_node(shape, route, dtype, split_off, monkeypatch):
    """y, dx, dw, d in_scale, d out_scale of scaled_conv2d, all five exact."""
    conv = _conv()
    if split_off:
        monkeypatch.setattr(conv, 'FP32_SPLIT', None)
    node = R.full_node(shape, dtype)
    node.check(dtype)
    x, w = _dev(node.x, dtype).requires_grad_(True), _dev(node.w, F32).requires_grad_(True)
    s, d = _dev(node.s, F32).requires_grad_(True), _dev(node.d, F32).requires_grad_(True)
    assert (conv._split_plan(x, 3, shape[2], shape[5]) is not None) == (route == 'fp32-split')
    y = conv.scaled_conv2d(x, w, s, d, shape[5])
    assert y.dtype == dtype
    R.assert_exact(y, node.y, f'{shape} {route} y')
    got = torch.autograd.grad(y, [x, w, s, d], grad_outputs=_dev(node.dy, dtype))
    for g, ref, name in zip(got, (node.dx, node.dw, node.ds, node.dd), ('dx', 'dw', 'd in_scale', 'd out_scale')):
        R.assert_exact(g, ref, f'{shape} {route} {name}')


@pytest.mark.parametrize('route,dtype,split_off', ROUTES, ids=[r[0] for r in ROUTES])
def test_scaled_conv2d_node_prescaled(route, dtype, split_off, monkeypatch):
    """prescaled=True: the input already carries in_scale; the gradient is taken with respect to that product."""
    conv = _conv()
    if split_off:
        monkeypatch.setattr(conv, 'FP32_SPLIT', None)
    shape = R.NODES[0]
    node = R.full_node(shape, dtype)
    xs, w = _dev(node.xs, dtype).requires_grad_(True), _dev(node.w, F32).requires_grad_(True)
    s, d = _dev(node.s, F32), _dev(node.d, F32).requires_grad_(True)
    y = conv.scaled_conv2d(xs, w, s, d, shape[5], prescaled=True)
    R.assert_exact(y, node.y, f'{route} y')
    got = torch.autograd.grad(y, [xs, w, d], grad_outputs=_dev(node.dy, dtype))
    for g, ref, name in zip(got, (node.dxs, node.dw, node.dd), ('d (s x)', 'dw', 'd out_scale')):
        R.assert_exact(g, ref, f'{route} prescaled {name}')


@pytest.mark.parametrize('dtype', [F16, F32], ids=_ids)
def test_r1_double_backward(dtype):
    """Gradient of |dL/dx|^2 with respect to w of the unscaled conv: through _ConvWgrad and the transposed conv."""
    conv = _conv()
    n, cin, cout, h, w_, pad = R.R1_CASE
    g = R.gen(11)
    x, wt = R.pick([n, cin, h, w_], (-2, -1, 1, 2), g), R.pick([cout, cin, 3, 3], (-1, 1), g)
    dy = R.pm1([n, cout, h + 2 * pad - 2, w_ + 2 * pad - 2], g)
    dx_ref, gw_ref = R.r1_ref(x, wt, dy, pad)
    # conditions on the inputs: dx and 2 dx are stored in `dtype`, the second weight gradient sums n * h * w products of 2 dx and dy
    assert R.representable(dx_ref, dtype) and R.representable(2 * dx_ref, dtype)
    assert R.dot_units(2 * dx_ref, dy, n * h * w_) < R.LIMIT and R.dot_units(dy, wt, cout * 9) < R.LIMIT
    xg, wg = _dev(x, dtype).requires_grad_(True), _dev(wt, F32).requires_grad_(True)
    y = conv.scaled_conv2d(xg, wg, None, None, pad)
    dx, = torch.autograd.grad(y, xg, grad_outputs=_dev(dy, dtype), create_graph=True)
    R.assert_exact(dx, dx_ref, 'dx')
    gw, = torch.autograd.grad(dx.float().square().sum(), wg)
    R.assert_exact(gw, gw_ref, 'd |dx|^2 / dw')
