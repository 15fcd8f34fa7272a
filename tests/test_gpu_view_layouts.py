"""Every op on offset and strided views of its operands: the bits of the same call on fresh dense tensors (helper: view_layouts.py).

One operand at a time is handed over in each layout of ``view_layouts.variants`` -- contiguous one and two elements into its buffer,
channels_last, a channel slice, a row slice, an expanded per-plane cotangent -- plus one run with every operand one element in; outputs
AND every gradient must be ``torch.equal`` to the run on fresh contiguous tensors.  The kernels' arithmetic does not depend on addresses,
so no comparison between two layouts has a tolerance.  Where the project has an exact float64 reference (conv_exact_ref, flrelu_exact_ref)
the operands come from it and the baseline is held to it bit for bit as well, so a wrong baseline cannot hide behind an equally wrong
variant; the other ops' baselines -- every output and gradient of the radial op and of the fused layer included -- are held to float64
at the bar their own tests use, cited at the assertion, or at a bound derived next to it.

Every test runs under ``view_layouts.audit``: each listed C entry point checks its base pointers against the audit table BEFORE the call is
forwarded, so a Python call site that lets a tensor through off the kernels' grid fails with an AssertionError that names the entry point
and the argument, and nothing is launched.  Each test ends by asserting that the entry points it is meant to reach were reached.

Left out, each for its reason:
* ``expanded`` for operands that are not cotangents: a stride-0 activation or weight is not a layout these ops are given.
* ``expanded`` for the 2-D cotangents of mapping_input and modulation_bank: the variant is defined for [N, C, 1, 1] planes; their cotangents
  take the other layouts (mapping_input) or stay fresh (modulation_bank, whose operands under test are the weights and styles).
* weighted_l1 has no tensor cotangent (its output is a scalar).
* modulated_conv2d: the weight and the styles (see its docstring).
* the sign tensor of filtered_lrelu, which the op documents as contiguous-only: its refusal is tested instead, next to a contiguous one at
  an odd byte offset.
* 16-bit second-order results of the radial op and nothing else are held to a bar reasoned here rather than one an existing test uses
  (test_filtered_lrelu_radial_first_and_second_order).
"""
import math

import numpy as np
import pytest
import torch

import conv_exact_ref as R
import flrelu_exact_ref as E
import upfirdn_ref as U
import view_layouts as V

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
HALVES = [BF16, F16]
_ids = R.case_id
DEVICE_ALIGN = 512                    # the caching allocator's block alignment


@pytest.fixture
def calls(monkeypatch):
    """The audit, active: the list of entry points forwarded so far."""
    from afcm_amd import _lib
    return V.audit(_lib.load(), monkeypatch)


@pytest.fixture(scope='module')
def lib():
    from afcm_amd import _lib
    return _lib.load()


def _conv():
    from afcm_amd.torch_utils.ops import conv2d as conv
    return conv


def _dev(t, dtype):
    return None if t is None else t.to(dtype).cuda()


def _leaf(t):
    """``t`` (in whatever layout) as a leaf that wants a gradient."""
    return t.detach().requires_grad_(True)


def _differs(got, want):
    if want is None or got is None:
        return None if got is want else 'one of the two is absent'
    got, want = got.detach(), want.detach()
    if got.shape != want.shape or got.dtype != want.dtype:
        return f'{tuple(got.shape)} {got.dtype} instead of {tuple(want.shape)} {want.dtype}'
    if torch.equal(got, want):
        return None
    bad = (got != want) | (got != got)
    i = tuple(bad.nonzero()[0].tolist())
    return f'{int(bad.sum())} of {bad.numel()} elements differ, first at {i}: {got[i].item()!r} != {want[i].item()!r}'


def _same(got, base, what):
    assert set(got) == set(base), what
    for k in base:
        msg = _differs(got[k], base[k])
        assert msg is None, f'{what}: {k}: {msg}'


def _layouts(t, more=()):
    """(name, tensor) for every re-layout of ``t`` but the baseline, each checked for the layout it claims."""
    for name, v in V.variants(t):
        if name != 'aligned':
            V.check_claim(name, v, DEVICE_ALIGN)
            assert torch.equal(v, t)
            yield name, v
    for name, v in more:
        assert torch.equal(v, t)
        yield name, v


def _param_slice(w):
    """A weight as rows [1, 1 + O) of a larger parameter: contiguous, somewhere inside its storage."""
    v = V.slice_of(w, 0, 1, 2)
    assert v.is_contiguous() and v.data_ptr() != v.untyped_storage().data_ptr()
    return v


def sweep(run, operands, what, weights=(), cotangent=None):
    """``run({name: tensor}) -> {name: result}`` on fresh contiguous operands, then with each operand in each layout (the others fresh), then
    with all of them one element in; every result equal to the first run's.  ``weights``: operands that are also tried as a slice of a larger
    parameter.  ``cotangent``: (name, per-plane constants [N, C, 1, 1]) -- that operand once more as a stride-0 expansion, against the dense
    tensor of the same values.  Returns the baseline."""
    fresh = lambda: {k: V.variant(t, 'aligned') for k, t in operands.items()}
    base = run(fresh())
    _same(run(fresh()), base, f'{what}: the baseline is not reproducible')
    for k, t in operands.items():
        for name, v in _layouts(t, [('param_slice', _param_slice(t))] if k in weights else []):
            ops = fresh()
            ops[k] = v
            _same(run(ops), base, f'{what}: {k} as {name}')
    _same(run({k: V.variant(t, 'offset1') for k, t in operands.items()}), base, f'{what}: every operand one element in')
    if cotangent is not None:
        k, pc = cotangent
        dense = pc.expand(operands[k].shape).contiguous()
        ops = fresh()
        ops[k] = dense
        want = run(ops)
        ops = fresh()
        ops[k] = V.variant(dense, 'expanded', cotangent=True)
        V.check_claim('expanded', ops[k], DEVICE_ALIGN)
        _same(run(ops), want, f'{what}: {k} expanded from per-plane constants')
    return {k: None if v is None else v.detach() for k, v in base.items()}


def _per_plane(shape, dtype, seed=5):
    return R.pm1([shape[0], shape[1], 1, 1], R.gen(seed)).to(dtype).cuda()


def _reached(calls, *groups):
    """Each group: entry points of which at least one must have been forwarded."""
    seen = set(calls)
    for g in groups:
        g = (g,) if isinstance(g, str) else g
        assert seen & set(g), f'none of {g} was reached; reached: {sorted(seen)}'


# ---- conv2d -----------------------------------------------------------------------------------------------------------------------------
# (n, cin, cout, h, w, pad), kernel size, forward (family, kernel), weight gradient (kernel, pad_odd) as dispatched
CONV16 = [
    ('3x3-pad0', (2, 8, 20, 12, 14, 0), 3, (R.ROWS64, R.K_X16), (R.WG_DWORD, 0)),
    ('3x3-pad1', (2, 20, 70, 12, 14, 1), 3, (R.ROWS96, R.K_X16), (R.WG_GRANULE, 0)),        # (dy framed by a ring of zeros: a pad-2 weight gradient)
    ('3x3-pad2', (2, 70, 8, 12, 14, 2), 3, (R.ROWS64, R.K_X16), (R.WG_GRANULE, 0)),
    ('1x1', (2, 20, 70, 12, 14, 0), 1, (R.ROWS128, R.K_GENERAL16), (R.WG_GRANULE, 0)),
    ('direct', (2, 3, 20, 12, 14, 2), 3, (R.DIRECT, R.K_DIRECT), (R.WG_GRANULE, 0)),
]
FP32_CASE = (2, 8, 20, 12, 14, 1)
FP32_ROUTES = [('split-float16', (F16, 3, 3, 3), F16), ('split-bfloat16', (BF16, 6, 6, 6), BF16), ('native', None, None)]
STRIDE2_CASE = (2, 8, 20, 12, 16, 1)


def _assert_routes(lib, dtype, shape, ks, fwd, wg):
    conv = _conv()
    n, cin, cout, h, w, pad = shape
    pl = R.conv_plan(lib, dtype, n, cin, cout, h, w, ks, pad)
    assert (pl.family, pl.kernel) == fwd, pl
    p, q = h + 2 * pad - ks + 1, w + 2 * pad - ks + 1
    wpad = conv._frame_dy(torch.empty([n, cout, p, q], dtype=dtype, device='cuda'), ks, pad)[1]
    wpl = R.wgrad_plan(lib, dtype, n, cin, cout, h, w, ks, wpad)
    assert (wpl.kernel, wpl.pad_odd) == wg, wpl


def _node_operands(node, dtype):
    return dict(x=_dev(node.x, dtype), w=_dev(node.w, F32), dy=_dev(node.dy, dtype))


def _scaled_run(node, pad, scaled):
    conv = _conv()
    s, d = (_dev(node.s, F32), _dev(node.d, F32)) if scaled else (None, None)

    def run(o):
        x, w = _leaf(o['x']), _leaf(o['w'])
        sl, dl = (_leaf(s), _leaf(d)) if scaled else (None, None)
        y = conv.scaled_conv2d(x, w, sl, dl, pad)
        grads = torch.autograd.grad(y, [x, w] + ([sl, dl] if scaled else []), grad_outputs=o['dy'])
        return dict(zip(('y', 'dx', 'dw', 'ds', 'dd'), (y,) + grads))
    return run


def _hold_to_node(base, node, what):
    for k in base:
        R.assert_exact(base[k], getattr(node, k), f'{what} {k} against float64')


@pytest.mark.parametrize('dtype', HALVES, ids=_ids)
@pytest.mark.parametrize('name,shape,ks,fwd,wg', CONV16, ids=[c[0] for c in CONV16])
def test_scaled_conv2d_16bit(name, shape, ks, fwd, wg, dtype, lib, calls):
    """scaled_conv2d with both scales: y, dx, dw, d in_scale, d out_scale."""
    _assert_routes(lib, dtype, shape, ks, fwd, wg)
    node = R.make_node(shape, 'small', dtype, bias=False, ks=ks)
    node.check(dtype)
    ops = _node_operands(node, dtype)
    base = sweep(_scaled_run(node, shape[5], True), ops, f'{name} {dtype}', weights=('w',), cotangent=('dy', _per_plane(ops['dy'].shape, dtype)))
    _hold_to_node(base, node, f'{name} {dtype}')
    _reached(calls, 'afcm_conv2d_ld', 'afcm_conv2d_wgrad_ld', 'afcm_scale_planes', ('afcm_plane_dot', 'afcm_plane_dot_ld'))


@pytest.mark.parametrize('dtype', HALVES, ids=_ids)
@pytest.mark.parametrize('name,shape,ks,fwd,wg', CONV16, ids=[c[0] for c in CONV16])
def test_conv2d_gradfix_16bit(name, shape, ks, fwd, wg, dtype, lib, calls):
    """conv2d_gradfix.conv2d (no scales, no bias): y, dx, dw."""
    from afcm_amd.torch_utils.ops import conv2d_gradfix
    _assert_routes(lib, dtype, shape, ks, fwd, wg)
    node = R.make_node(shape, 'small', dtype, need=('y', 'dx', 'dw'), scales=False, bias=False, ks=ks)
    node.check(dtype, ('y', 'dx', 'dw'))

    def run(o):
        x, w = _leaf(o['x']), _leaf(o['w'])
        y = conv2d_gradfix.conv2d(x, w, padding=shape[5])
        return dict(zip(('y', 'dx', 'dw'), (y,) + torch.autograd.grad(y, [x, w], grad_outputs=o['dy'])))
    ops = _node_operands(node, dtype)
    base = sweep(run, ops, f'{name} {dtype}', weights=('w',), cotangent=('dy', _per_plane(ops['dy'].shape, dtype)))
    _hold_to_node(base, node, f'{name} {dtype}')
    _reached(calls, 'afcm_conv2d_ld', 'afcm_conv2d_wgrad_ld')


@pytest.mark.parametrize('scaled', [True, False], ids=['scales', 'plain'])
@pytest.mark.parametrize('route,split,part', FP32_ROUTES, ids=[r[0] for r in FP32_ROUTES])
def test_scaled_conv2d_fp32_routes(route, split, part, scaled, lib, calls, monkeypatch):
    """The fp32 3x3 conv on the split route (float16 parts: the default; bfloat16 parts) and on the native fp32 kernels."""
    conv = _conv()
    monkeypatch.setattr(conv, 'FP32_SPLIT', split)
    n, cin, cout, h, w, pad = shape = FP32_CASE
    if part is not None:
        pl = R.conv_plan(lib, part, n, cin, cout, h, w, 3, pad, split=True)
        assert (pl.family, pl.kernel) == (R.ROWS64, R.K_SPLIT), pl
    else:
        pl = R.conv_plan(lib, F32, n, cin, cout, h, w, 3, pad)
        assert (pl.family, pl.kernel) == (R.ROWS64, R.K_F32), pl
        assert R.wgrad_plan(lib, F32, n, cin, cout, h, w, 3, pad).kernel == R.WG_F32
    need = ('y', 'dx', 'dw', 'ds', 'dd') if scaled else ('y', 'dx', 'dw')
    node = R.make_node(shape, 'small', F32, need=need, scales=scaled, bias=False)
    node.check(F32, need)
    ops = _node_operands(node, F32)
    assert (conv._split_plan(ops['x'], 3, cout, pad) is not None) == (part is not None)
    base = sweep(_scaled_run(node, pad, scaled), ops, f'fp32 {route}', weights=('w',), cotangent=('dy', _per_plane(ops['dy'].shape, F32)))
    _hold_to_node(base, node, f'fp32 {route}')
    if part is None:
        _reached(calls, 'afcm_conv2d_ld', 'afcm_conv2d_wgrad_ld')
        assert 'afcm_conv2d_split' not in calls
    else:
        _reached(calls, 'afcm_conv2d_split', 'afcm_split16', 'afcm_conv2d_wgrad_ld', 'afcm_conv2d_pack_split')
        if scaled:
            _reached(calls, 'afcm_plane_dot_parts')
        assert ('afcm_amax_bits' in calls) == (part == F16)


def test_fp32_conv_on_offset_x_and_cotangent_returns_the_aligned_bits(calls):
    """An fp32 3x3 conv (the split route, the default) on an x and a cotangent 4 bytes past a 16-byte boundary raised
    'split16: x must be 16-byte ... aligned' from afcm_split16: _split_operand handed it the tensor where .contiguous() had left it.
    That refusal (AFCM_REQUIRE, csrc/conv2d_planes.hip:444) was established by reading the code, not by running it: under the audit
    of this file a split16 without its copy fails one step earlier, with the audit's AssertionError naming afcm_split16 and x."""
    conv = _conv()
    assert conv.FP32_SPLIT is not None
    node = R.make_node(FP32_CASE, 'small', F32, need=('y', 'dx', 'dw'), scales=False, bias=False)
    run = _scaled_run(node, FP32_CASE[5], False)
    ops = _node_operands(node, F32)
    base = run({k: V.variant(t, 'aligned') for k, t in ops.items()})
    off = {k: V.variant(t, 'offset1') for k, t in ops.items()}
    off['w'] = V.variant(ops['w'], 'aligned')
    assert off['x'].data_ptr() % 16 == 4 and off['dy'].data_ptr() % 16 == 4 and off['x'].is_contiguous() and off['dy'].is_contiguous()
    _same(run(off), base, 'offset1 x and cotangent')
    _hold_to_node(base, node, 'fp32 split')
    _reached(calls, 'afcm_split16', 'afcm_conv2d_split')


def test_split_conv_style_gradient_with_an_offset_cotangent_returns_the_aligned_bits(calls):
    """The style gradient of a split conv is plane_dot_parts(kept parts of s x, dx): called directly with a ``b`` 4 bytes past a 16-byte
    boundary it raised 'plane_dot_parts: parts must be 8-byte, b 16-byte aligned' (AFCM_REQUIRE, csrc/conv2d_planes.hip:471: established by
    reading; under the audit the failure is the audit's AssertionError naming afcm_plane_dot_parts and b); through the node, with the
    cotangent at that offset."""
    conv = _conv()
    assert conv.FP32_SPLIT is not None
    node = R.full_node(FP32_CASE, F32)
    run = _scaled_run(node, FP32_CASE[5], True)
    ops = _node_operands(node, F32)
    base = run({k: V.variant(t, 'aligned') for k, t in ops.items()})
    off = {k: V.variant(t, 'aligned') for k, t in ops.items()}
    off['dy'] = V.variant(ops['dy'], 'offset1')
    assert off['dy'].data_ptr() % 16 == 4
    got = run(off)
    _same(got, base, 'offset1 cotangent')
    R.assert_exact(got['ds'], node.ds, 'd in_scale')
    # the op itself, on the parts the node keeps
    x, s, dx = ops['x'], _dev(node.s, F32), _dev(node.dx, F32)
    bound = conv.amax_bits(x, s)
    parts = conv.split16(x, s, 2, F16, bound)
    want = conv.plane_dot_parts(parts, V.variant(dx, 'aligned'), bound)
    for name, v in _layouts(dx):
        assert torch.equal(conv.plane_dot_parts(parts, v, bound), want), name
    R.assert_exact(want, (node.xs * node.dx).sum([2, 3]), '<s x, dx>')
    _reached(calls, 'afcm_plane_dot_parts', 'afcm_split16', 'afcm_amax_bits')


@pytest.mark.parametrize('dtype', HALVES + [F32], ids=_ids)
def test_modulated_conv2d(dtype, lib, calls):
    """modulated_conv2d(x, w, styles): the conv is scaled_conv2d with both scales.  x and the cotangent are re-laid-out; the weight and
    the styles go through framework arithmetic first (normalisation, the demodulation matmul), whose summation order may follow its
    input's strides and which hands the kernels fresh tensors in any case, so they stay as they are."""
    conv = _conv()
    shape = CONV16[1][1]
    n, cin, cout, h, w, pad = shape
    node = R.full_node(shape, dtype)
    ops = _node_operands(node, dtype)
    w0, s0 = ops.pop('w'), _dev(node.s, F32)

    def run(o):
        x, wt, st = _leaf(o['x']), _leaf(w0), _leaf(s0)
        y = conv.modulated_conv2d(x, wt, st, demodulate=True, padding=pad)
        return dict(zip(('y', 'dx', 'dw', 'ds'), (y,) + torch.autograd.grad(y, [x, wt, st], grad_outputs=o['dy'])))
    base = sweep(run, ops, f'modulated {dtype}', cotangent=('dy', _per_plane(ops['dy'].shape, dtype)))
    # against the definition in float64 (per-sample weights), every element within its own bound: the two operands of each product are
    # rounded once (s x and w_hat into the 16-bit type, unit roundoff u; fp32: the 22 bits of a two-part float16 split), the K = cin * 9
    # products are accumulated in fp32, the coefficients are a few fp32 operations, and y is rounded once into its type
    xr, wr, sr = (t.double().cpu() for t in (ops['x'], w0, s0))
    wn = wr * wr.square().mean([1, 2, 3], keepdim=True).rsqrt()
    sn = sr * sr.square().mean().rsqrt()
    ww = wn[None] * sn[:, None, :, None, None]
    ww = ww * (ww.square().sum([2, 3, 4], keepdim=True) + 1e-8).rsqrt()
    yr = torch.cat([torch.nn.functional.conv2d(xr[i:i + 1], ww[i], padding=pad) for i in range(n)]).detach()
    mass = torch.cat([torch.nn.functional.conv2d(xr[i:i + 1].abs(), ww[i].abs(), padding=pad) for i in range(n)]).detach()
    u = {F32: 2.0 ** -22, F16: 2.0 ** -11, BF16: 2.0 ** -8}[dtype]
    out_u = {F32: 2.0 ** -24, F16: 2.0 ** -11, BF16: 2.0 ** -8}[dtype]
    bound = (2 * u + (cin * 9 + 16) * 2.0 ** -24) * mass + out_u * yr.abs()
    err = (base['y'].double().cpu() - yr).abs()
    worst = float((err / bound).max())
    print(f'modulated_conv2d {dtype}: worst error {worst:.3f} of its bound')
    assert worst <= 1.0, worst
    _reached(calls, ('afcm_conv2d_ld', 'afcm_conv2d_split'), 'afcm_conv2d_wgrad_ld')


@pytest.mark.parametrize('dtype', HALVES, ids=_ids)
def test_strided_conv2d(dtype, calls):
    conv = _conv()
    shape = STRIDE2_CASE
    node = R.stride2_node(shape, 'small', dtype)
    node.check(dtype, ('y', 'dx', 'dw'))

    def run(o):
        x, w = _leaf(o['x']), _leaf(o['w'])
        assert conv.strided_conv2d_supported(x, w, shape[5])
        y = conv.strided_conv2d(x, w, shape[5])
        return dict(zip(('y', 'dx', 'dw'), (y,) + torch.autograd.grad(y, [x, w], grad_outputs=o['dy'])))
    ops = _node_operands(node, dtype)
    base = sweep(run, ops, f'stride 2 {dtype}', weights=('w',), cotangent=('dy', _per_plane(ops['dy'].shape, dtype)))
    _hold_to_node(base, node, f'stride 2 {dtype}')
    _reached(calls, 'afcm_conv2d_stride2', 'afcm_conv2d_ld', 'afcm_conv2d_wgrad_ld', 'afcm_upfirdn2d')


@pytest.mark.parametrize('dtype', HALVES, ids=_ids)
def test_weight_gradient_with_plane_dots(dtype, lib, calls):
    """The image-aligned weight gradient that also returns <x, conv^T(w, dy)> per plane (afcm_conv2d_wgrad_dots_ld)."""
    conv = _conv()
    shape = R.WGRAD_DOTS[0]
    n, cin, cout, h, w, pad = shape
    pl = R.wgrad_plan(lib, dtype, n, cin, cout, h, w, 3, pad, dots=True)
    assert pl is not None and pl.kernel == R.WG_GRANULE and pl.reduce == R.RED_DOTS, pl
    node = R.dots_node(shape, dtype)
    node.check(dtype, ('dx', 'dw'))

    def run(o):
        dw, dots = conv._wgrad_raw(o['dy'], o['x'], cout, cin, 3, pad, dots_with=o['w'])
        return dict(dw=dw, dots=dots)
    ops = _node_operands(node, dtype)
    base = sweep(run, ops, f'dots {dtype}', weights=('w',), cotangent=('dy', _per_plane(ops['dy'].shape, dtype)))
    _hold_to_node(base, node, f'dots {dtype}')
    _reached(calls, 'afcm_conv2d_wgrad_dots_ld')
    assert 'afcm_conv2d_wgrad_ld' not in calls


@pytest.mark.parametrize('dtype', [F16, F32], ids=_ids)
def test_r1_double_backward(dtype, calls):
    """The R1 penalty's graph through conv2d_gradfix.conv2d: dx with create_graph, then the gradient of |dx|^2 with respect to w."""
    from afcm_amd.torch_utils.ops import conv2d_gradfix
    n, cin, cout, h, w_, pad = R.R1_CASE
    g = R.gen(11)
    x, wt = R.pick([n, cin, h, w_], (-2, -1, 1, 2), g), R.pick([cout, cin, 3, 3], (-1, 1), g)
    dy = R.pm1([n, cout, h + 2 * pad - 2, w_ + 2 * pad - 2], g)
    dx_ref, gw_ref = R.r1_ref(x, wt, dy, pad)
    assert R.representable(dx_ref, dtype) and R.representable(2 * dx_ref, dtype)
    assert R.dot_units(2 * dx_ref, dy, n * h * w_) < R.LIMIT and R.dot_units(dy, wt, cout * 9) < R.LIMIT

    def run(o):
        xg, wg = _leaf(o['x']), _leaf(o['w'])
        y = conv2d_gradfix.conv2d(xg, wg, padding=pad)
        dx, = torch.autograd.grad(y, xg, grad_outputs=o['dy'], create_graph=True)
        gw, = torch.autograd.grad(dx.float().square().sum(), wg)
        return dict(y=y, dx=dx, gw=gw)
    base = sweep(run, dict(x=_dev(x, dtype), w=_dev(wt, F32), dy=_dev(dy, dtype)), f'R1 {dtype}', weights=('w',),
                 cotangent=('dy', _per_plane(dy.shape, dtype)))
    R.assert_exact(base['dx'], dx_ref, 'dx')
    R.assert_exact(base['gw'], gw_ref, 'd |dx|^2 / dw')
    _reached(calls, ('afcm_conv2d_ld', 'afcm_conv2d_split'), 'afcm_conv2d_wgrad_ld')


# ---- filtered_lrelu ---------------------------------------------------------------------------------------------------------------------
def _smallest(family, dtype, tag=None):
    pool = [c for c in E.cases() if c['family'] == family and c['dtype'] == dtype and (c['id'].endswith('-' + tag) if tag else c['id'].count('-') == 3)]
    return min(pool, key=lambda c: c['h'] * c['w'])


FLRELU_CASES = ([_smallest(f, dt) for dt in ('float16', 'bfloat16') for f in ('wave', 'mfma_tile', 'tile')]
                + [_smallest('wave', dt, 'skip') for dt in ('float16', 'bfloat16')] + [_smallest('strip', 'float32')])


def _arr(a, dtype):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(getattr(torch, dtype)).cuda()
    assert torch.equal(t.double().cpu(), torch.from_numpy(np.ascontiguousarray(a)))
    return t


def _equals_array(got, want, what):
    got = got.double().cpu().numpy()
    assert got.shape == want.shape and not (got != want).any(), f'{what}: {int((got != want).sum())} elements differ from the float64 reference'


@pytest.mark.parametrize('case', FLRELU_CASES, ids=[c['id'] for c in FLRELU_CASES])
def test_filtered_lrelu_families(case, calls):
    """The smallest exact case of each kernel family: the sign-writing forward (x, b, skip re-laid-out) and the transposed call that reads
    its codes (the cotangent re-laid-out); outputs, the written sign tensor, dx and the plane sums."""
    from afcm_amd.torch_utils.ops import filtered_lrelu as flr
    d, ref, dtype = E.data(case), E.reference(case), case['dtype']
    fu, fd = torch.from_numpy(d['fu']).cuda(), torch.from_numpy(d['fd']).cuda()
    osc = None if d['oscale'] is None else torch.from_numpy(d['oscale']).float().cuda()
    cfg, bcfg = E.forward_cfg(case), E.backward_cfg(case)
    ops = dict(x=_arr(d['x'], dtype), g=_arr(d['g'], dtype))
    if d['b'] is not None:
        ops['b'] = _arr(d['b'], dtype)
    if d['skip'] is not None:
        ops['skip'] = _arr(d['skip'], dtype)

    def run(o):
        y, s, lay, _ = flr._run(o['x'], fu, fd, o.get('b'), None, cfg, True, oscale=osc, skip=o.get('skip'), no_fallback=True)
        assert lay == case['layout'], f'expected the {case["family"]} kernels'
        dx, _, _, psum = flr._run(o['g'], fd, fu, None, s, bcfg, False, want_plane_sum=True, no_fallback=True)
        return dict(y=y, signs=s, dx=dx, psum=psum)
    base = sweep(run, ops, case['id'], cotangent=('g', _per_plane(ops['g'].shape, getattr(torch, dtype))))
    _equals_array(base['y'], ref['expected_y'], 'y')
    _equals_array(base['dx'], ref['expected_dx'], 'dx')
    # the sign tensor: contiguous at an odd byte offset is read where it is or copied, never misread; any other layout is refused
    s = base['signs']
    s1 = V.variant(s, 'offset1')
    assert s1.data_ptr() % 4 == 1 and s1.is_contiguous()
    dx1 = flr._run(V.variant(ops['g'], 'aligned'), fd, fu, None, s1, bcfg, False, no_fallback=True)[0]
    assert torch.equal(dx1, base['dx']), 'codes one byte into their buffer'
    wide = torch.zeros(list(s.shape[:3]) + [s.shape[3] + 4], dtype=torch.uint8, device='cuda')[..., :s.shape[3]]
    wide.copy_(s)
    with pytest.raises(RuntimeError, match='signs must be a contiguous uint8 tensor'):
        flr._run(V.variant(ops['g'], 'aligned'), fd, fu, None, wide, bcfg, False, no_fallback=True)
    _reached(calls, 'afcm_filtered_lrelu')


def _radial_layer():
    from afcm_amd import layer_schedule
    pl = layer_schedule.plan(256, 4, 1, {'use_radial_filters': True})
    return min((L for L in pl['enc'] + pl['dec'] if L['fd'] is not None and L['fd'].ndim == 2), key=lambda L: L['in_size'])


@pytest.mark.parametrize('dtype', [F32, F16, BF16], ids=_ids)
def test_filtered_lrelu_radial_first_and_second_order(dtype, calls):
    """The smallest radial layer geometry (a 2-D down filter: the exact LDS-tile kernels in every dtype) through the public op: y, dx, db,
    and the second-order d<dx, v>/d(cotangent), which runs the forward kernels again on the written codes."""
    from afcm_amd.torch_utils.ops import filtered_lrelu as flr
    L = _radial_layer()
    h = L['in_size'] + L['k'] - 1
    g = torch.Generator().manual_seed(7)
    x, b = torch.randn(1, 2, h, h, generator=g).to(dtype).cuda(), (torch.randn(2, generator=g) * 0.2).to(dtype).cuda()
    fu, fd = L['fu'].cuda(), L['fd'].cuda()
    kw = dict(up=L['up'], down=L['down'], padding=L['padding'], gain=math.sqrt(2), slope=0.2, clamp=256.0)
    with torch.no_grad():
        shape = flr.filtered_lrelu(x, fu=fu, fd=fd, b=b, **kw).shape
    r = torch.randn(shape, generator=g).to(dtype).cuda()
    v = torch.randn(x.shape, generator=g).to(dtype).cuda()

    def run(o):
        xg, bg, dy = _leaf(o['x']), _leaf(o['b']), _leaf(o['dy'])
        y = flr.filtered_lrelu(xg, fu=fu, fd=fd, b=bg, **kw)
        dx, db = torch.autograd.grad(y, [xg, bg], dy, create_graph=True)
        ddy, = torch.autograd.grad((dx * o['v']).sum(), [dy])
        return dict(y=y, dx=dx, db=db, ddy=ddy)
    base = sweep(run, dict(x=x, b=b, dy=r, v=v), f'radial {L["name"]} {dtype}', cotangent=('dy', _per_plane(r.shape, dtype)))
    # against the float64 oracle on the same (rounded) operands, max |error| against tol * max(1, |reference|max) as _close of
    # test_gpu_flrelu_radial.py does: fp32 TOL = 2e-5 (its line 17; y, dx: lines 112-113, second order: 309-310) and 1e-4 for db (line 120);
    # 16-bit TOL16 (line 18) for y, dx and db (lines 155-164).  The 16-bit second-order result has no test of its own there: it is the
    # forward op applied to v on the written codes, computed in fp32 and rounded once into the 16-bit output like y, hence the same bar.
    from oracle import aten_ops as ops
    xs, bs, dys = (t.double().cpu().requires_grad_(True) for t in (x, b, r))
    ys = ops.filtered_lrelu(xs, fu=L['fu'].double(), fd=L['fd'].double(), b=bs, flip_filter=False, **kw)
    gx, gb = torch.autograd.grad(ys, [xs, bs], dys, create_graph=True)
    gdy, = torch.autograd.grad((gx * v.double().cpu()).sum(), [dys])
    tol = {F32: 2e-5, F16: 4e-3, BF16: 3e-2}[dtype]
    for name, ref, bar in (('y', ys, tol), ('dx', gx, tol), ('db', gb, 1e-4 if dtype == F32 else tol), ('ddy', gdy, tol)):
        ref = ref.detach()
        err = float((base[name].double().cpu() - ref).abs().max())
        print(f'radial {dtype} {name}: max |error| {err:.3e}, bar {bar * max(1.0, float(ref.abs().max())):.3e}')
        assert err <= bar * max(1.0, float(ref.abs().max())), (name, err, bar)
    _reached(calls, 'afcm_filtered_lrelu')


@pytest.mark.parametrize('dtype', HALVES, ids=_ids)
def test_fused_conv_filtered_lrelu_layer(dtype, calls):
    """fused_layer.conv_filtered_lrelu: conv -> filtered_lrelu (+ skip, x next styles) as one node; x, w, skip and the cotangent re-laid-out."""
    from afcm_amd.torch_utils.ops import fused_layer
    from oracle import generator as ogen
    L = [l for l in ogen.plan(256, 4, 1, {})['dec'] if l['name'] == 'L12_276_64'][0]
    g = torch.Generator().manual_seed(3)
    n, cin, cout, h = 2, 8, 20, 36
    act = dict(up=2, down=2, padding=L['padding'], gain=math.sqrt(2), slope=0.2, clamp=256.0)
    fu, fd = L['fu'].cuda(), L['fd'].cuda()
    x = torch.randn(n, cin, h, h, generator=g).to(dtype).cuda()
    w = (torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)).cuda()
    s, d, nx = (torch.rand(n, c, generator=g).cuda() + 0.5 for c in (cin, cout, cout))
    b = (torch.randn(cout, generator=g) * 0.1).cuda()
    assert fused_layer.available(x, w, fu, fd, conv_pad=2, **act)
    with torch.no_grad():
        zshape = fused_layer.conv_filtered_lrelu(x, w, s, d, b, fu, fd, conv_pad=2, next_scale=nx, **act).shape
    skip = torch.randn(zshape, generator=g).to(dtype).cuda()
    r = torch.randn(zshape, generator=g).to(dtype).cuda()

    def run(o):
        lv = [_leaf(t) for t in (o['x'], o['w'], s, d, b, o['skip'], nx)]
        z = fused_layer.conv_filtered_lrelu(lv[0], lv[1], lv[2], lv[3], lv[4], fu, fd, conv_pad=2, skip=lv[5], next_scale=lv[6], **act)
        grads = torch.autograd.grad(z, lv, grad_outputs=o['g'])
        return dict(zip(('z', 'dx', 'dw', 'ds', 'dd', 'db', 'dskip', 'dnext'), (z,) + grads))
    base = sweep(run, dict(x=x, w=w, skip=skip, g=r), f'fused layer {dtype}', weights=('w',), cotangent=('g', _per_plane(zshape, dtype)))
    # against the layer composed op by op in float64 on the same (rounded) operands, at the bars of
    # test_gpu_conv.py::test_fused_layer_node_matches_op_by_op: relative L2 error 4e-2 (bfloat16) / 8e-3 (float16) for z (its lines 149, 200),
    # three times that for every gradient (line 204)
    from oracle import aten_ops as ops
    lv = [t.double().cpu().requires_grad_(True) for t in (x, w, s, d, b, skip, nx)]
    y = torch.nn.functional.conv2d(lv[0] * lv[2][:, :, None, None], lv[1], padding=2) * lv[3][:, :, None, None]
    z = (ops.filtered_lrelu(y, fu=L['fu'].double(), fd=L['fd'].double(), b=lv[4], **act) + lv[5]) * lv[6][:, :, None, None]
    refs = (z,) + torch.autograd.grad(z, lv, grad_outputs=r.double().cpu())
    tol = {BF16: 4e-2, F16: 8e-3}[dtype]
    for name, ref in zip(('z', 'dx', 'dw', 'ds', 'dd', 'db', 'dskip', 'dnext'), refs):
        ref = ref.detach()
        rel = float((base[name].double().cpu() - ref).norm() / ref.norm().clamp_min(1e-20))
        print(f'fused layer {dtype} {name}: relative L2 error {rel:.3e}')
        assert rel <= (tol if name == 'z' else 3 * tol), (name, rel, tol)
    _reached(calls, 'afcm_conv2d_ld', 'afcm_filtered_lrelu', ('afcm_conv2d_wgrad_ld', 'afcm_conv2d_wgrad_dots_ld'), 'afcm_layer_bwd_coefs')


# ---- upfirdn2d --------------------------------------------------------------------------------------------------------------------------
def _first(params, kind, ok=lambda case, dt: True):
    out = {}
    for name, dt in params:
        case = U.BY_NAME[kind][name]
        if dt not in out and ok(case, dt):
            out[dt] = case
    return [(kind, case, dt) for dt, case in out.items()]


UPFIRDN_CASES = (_first(U.TILE_PARAMS, 'tile', lambda c, dt: c.fshape == (4, 4) and c.xshape[2] * c.xshape[3] >= 6)
                 + _first(U.AGREE_PARAMS, 'rows', lambda c, dt: c.xshape[1] == 3 and c.xshape[3] >= 6)
                 + _first(U.GATHER_PARAMS, 'gather', lambda c, dt: c.name == 'pad_uneven_f5x3'))


@pytest.mark.parametrize('kind,case,dtype', UPFIRDN_CASES, ids=[f'{k}-{c.name}-{_ids(dt)}' for k, c, dt in UPFIRDN_CASES])
def test_upfirdn2d(kind, case, dtype, calls):
    """x, f and the cotangent; y and dx.  (A 16-bit x two bytes past a dword leaves the rows kernel to the tile kernel inside the entry
    point: the two meet the taps in the same order, test_gpu_upfirdn2d.py::test_rows_and_tile_kernels_agree_bit_for_bit.)"""
    from afcm_amd.torch_utils.ops import upfirdn2d as ufd
    assert U.kernel_of(case, dtype) == kind
    x, f, r = (t.cuda() for t in U.inputs(case, dtype))

    def run(o):
        xg = _leaf(o['x'])
        y = ufd.upfirdn2d(xg, o['f'], up=list(case.up), down=list(case.down), padding=list(case.padding), gain=case.gain)
        dx, = torch.autograd.grad(y, xg, o['r'])
        return dict(y=y, dx=dx)
    base = sweep(run, dict(x=x, f=f, r=r), f'{kind} {case.name} {dtype}', cotangent=('r', _per_plane(r.shape, dtype)))
    y, ybar, dx, dxbar = U.reference(kind, case.name, dtype, False)
    assert U.mismatch(U.f64(base['y'].cpu()), y, ybar) is None and U.mismatch(U.f64(base['dx'].cpu()), dx, dxbar) is None
    _reached(calls, 'afcm_upfirdn2d')


# ---- dense and small ops ----------------------------------------------------------------------------------------------------------------
def _flat_slices(tensors):
    """Every tensor as a contiguous slice of ONE flat buffer, each starting an odd number of elements in."""
    total = sum(t.numel() + 1 for t in tensors)
    flat = torch.full([total + 1], float('nan'), dtype=tensors[0].dtype, device=tensors[0].device)
    out, at = [], 1
    for t in tensors:
        v = flat[at:at + t.numel()].view(t.shape)
        v.copy_(t)
        out.append(v)
        at += t.numel() + 1
    return out


def test_modulation_bank(calls):
    """Three layers (two demodulating) as one op: weights as slices of one flat buffer, styles one element into theirs, and each operand in
    every other layout; w_hat, s_eff, d and the gradients of weights and styles.  fp32 inputs: also against float64 at the bars of
    modulation_ref.py (BAR_FWD, BAR_GRAD: lines 35-36), per row."""
    import modulation_ref as M
    from afcm_amd.torch_utils.ops import modulation_bank as mb
    g = torch.Generator().manual_seed(9)
    n = 3
    dims = [(20, 8, 3, True), (8, 20, 3, True), (5, 8, 1, False)]
    ws = [torch.randn(o, i, k, k, generator=g).cuda() for o, i, k, _ in dims]
    ts = [(torch.randn(n, i, generator=g) + 1.5).cuda() for _, i, _, _ in dims]
    mags = [(torch.rand([], generator=g) + 0.5).cuda() for _ in dims]
    cots = [[torch.randn(w.shape, generator=g).cuda() for w in ws], [torch.randn(t.shape, generator=g).cuda() for t in ts],
            [torch.randn(n, o, generator=g).cuda() for o, _, _, _ in dims]]
    names = [f'w{l}' for l in range(3)] + [f't{l}' for l in range(3)]

    def run(o):
        wl, tl = [_leaf(o[f'w{l}']) for l in range(3)], [_leaf(o[f't{l}']) for l in range(3)]
        items = [mb.Item(w, t, m, dm[3]) for w, t, m, dm in zip(wl, tl, mags, dims)]
        assert mb.supported(items)
        res = mb.modulation_bank(items)
        outs, gos = [], []
        for l, (w_hat, s_eff, dd) in enumerate(res):
            if dims[l][3]:
                outs += [w_hat, s_eff, dd]
                gos += [cots[0][l], cots[1][l], cots[2][l]]
            else:
                outs += [s_eff]
                gos += [cots[1][l]]
        grads = torch.autograd.grad(outs, wl[:2] + tl, gos)
        out = {f'out{k}': t for k, t in enumerate(outs)}
        out.update({f'd{nm}': gr for nm, gr in zip(names[:2] + names[3:], grads)})
        return out
    ops = dict(zip(names, ws + ts))
    base = sweep(run, ops, 'modulation bank', weights=('w0', 'w1', 'w2'))
    flat = dict(zip(names, _flat_slices(ws) + [V.variant(t, 'offset1') for t in ts]))
    assert all(flat[f'w{l}'].untyped_storage().data_ptr() == flat['w0'].untyped_storage().data_ptr() for l in range(3))
    _same(run(flat), base, 'weights in one flat buffer, styles one element in')
    for l in (0, 1):
        w64, t64, m64 = ws[l].double().cpu(), ts[l].double().cpu(), mags[l].double().cpu()
        w_hat, s_eff, dd = M.composed(w64, t64, m64, True)
        k = 3 * l
        assert M.row_ratio(base[f'out{k}'], w_hat, M.BAR_FWD) <= 1 and M.row_ratio(base[f'out{k + 1}'], s_eff, M.BAR_FWD) <= 1
        assert M.row_ratio(base[f'out{k + 2}'], dd, M.BAR_FWD) <= 1
        dw, dt = M.composed_bwd(w64, t64, m64, True, cots[0][l].double().cpu(), cots[1][l].double().cpu(), cots[2][l].double().cpu())
        assert M.row_ratio(base[f'dw{l}'], dw, M.BAR_GRAD) <= 1 and M.row_ratio(base[f'dt{l}'], dt, M.BAR_GRAD) <= 1
    _reached(calls, 'afcm_modulation_bank_fwd', 'afcm_modulation_bank_bwd')


def test_mapping_input(calls):
    """cat(normalize(z), normalize(embed(c))): z, c, the embedding's weight and bias and the cotangent; against float64 at the bars of
    test_gpu_dense_exact.py::test_mapping_input_rows_vs_float64 (1e-5 forward, 3e-5 gradients: lines 249-258)."""
    import types
    from afcm_amd.torch_utils.ops import fc_bank
    g = torch.Generator().manual_seed(4)
    n, zdim, cdim, wdim = 5, 33, 7, 36
    z, c = torch.randn(n, zdim, generator=g).cuda(), torch.rand(n, cdim, generator=g).cuda()
    ew, eb = torch.randn(wdim, cdim, generator=g).cuda(), (torch.randn(wdim, generator=g) * 0.3).cuda()
    r = torch.randn(n, zdim + wdim, generator=g).cuda()
    gains = dict(weight_gain=1.0 / math.sqrt(cdim), bias_gain=1.0, activation='linear')

    def run(o):
        embed = types.SimpleNamespace(weight=_leaf(o['ew']), bias=_leaf(o['eb']), **gains)
        assert fc_bank.mapping_input_supported(o['z'], o['c'], embed)
        x0 = fc_bank.mapping_input(o['z'], o['c'], embed)
        dew, deb = torch.autograd.grad(x0, [embed.weight, embed.bias], o['r'])
        return dict(x0=x0, dew=dew, deb=deb)
    base = sweep(run, dict(z=z, c=c, ew=ew, eb=eb, r=r), 'mapping input')
    zd, wd, bd = z.double().cpu(), ew.double().cpu().requires_grad_(True), eb.double().cpu().requires_grad_(True)
    e = c.double().cpu() @ (wd * gains['weight_gain']).t() + bd
    want = torch.cat([zd * (zd.square().mean(1, keepdim=True) + 1e-8).rsqrt(), e * (e.square().mean(1, keepdim=True) + 1e-8).rsqrt()], 1)
    ge, dew, deb = torch.autograd.grad((want * r.double().cpu()).sum(), [e, wd, bd])
    want = want.detach()
    for got, ref, tol, scale in ((base['x0'][:, :zdim], want[:, :zdim], 1e-5, None), (base['x0'][:, zdim:], want[:, zdim:], 1e-5, None),
                                 (base['dew'], dew, 3e-5, None), (base['deb'][:, None], deb[:, None], 3e-5, ge.abs().amax(0))):
        err = (got.double().cpu() - ref).abs().amax(1)                       # per row, against that row's own scale
        assert bool((err <= tol * (ref.abs().amax(1) if scale is None else scale)).all()), (float(err.max()), tol)
    _reached(calls, 'afcm_mapping_input_fwd', 'afcm_mapping_input_bwd')


@pytest.mark.parametrize('dtype', [F32, F16, BF16], ids=_ids)
def test_pool_blocks(dtype, calls):
    """pool4: [N, C, H, W] -> fp32 [N, C, 4, 4] block means (afcm_pool_blocks_fwd / _bwd).  Blocks of 3 x 5 integers: the sums are exact,
    so fp32 and 16-bit inputs alike are held to float64 up to the one division."""
    from afcm_amd.networks_stylegan3 import _PoolBlocks
    g = torch.Generator().manual_seed(2)
    x = torch.randint(-8, 9, (2, 3, 12, 20), generator=g).to(dtype).cuda()
    r = torch.randint(-4, 5, (2, 3, 4, 4), generator=g).float().cuda()

    def run(o):
        xg = _leaf(o['x'])
        y = _PoolBlocks.apply(xg)
        dx, = torch.autograd.grad(y, xg, o['r'])
        return dict(y=y, dx=dx)
    base = sweep(run, dict(x=x, r=r), f'pool4 {dtype}', cotangent=('r', _per_plane(r.shape, F32)))
    want = x.double().cpu().reshape(2, 3, 4, 3, 4, 5).sum((3, 5))
    assert torch.equal(base['y'].cpu(), (want.float() / 15.0)), 'block means'
    dx = (r.double().cpu() * (1.0 / 15.0))[:, :, :, None, :, None].expand(2, 3, 4, 3, 4, 5).reshape(2, 3, 12, 20)
    # gy * fl(1 / 15): two fp32 roundings, then one into x's type
    u = 2.0 ** -22 + {F32: 0.0, F16: 2.0 ** -11, BF16: 2.0 ** -8}[dtype]
    assert bool(((base['dx'].double().cpu() - dx).abs() <= u * dx.abs()).all())
    _reached(calls, 'afcm_pool_blocks_fwd', 'afcm_pool_blocks_bwd')


def test_weighted_l1(calls):
    """weight * mean |a - b| and its gradient for a (afcm_l1_partials / afcm_l1_grad): integer operands, 2^13 elements in two
    workgroup partials -- every sum and the factor weight / numel are exact, so there is one right answer."""
    from afcm_amd.optim import weighted_l1
    g = torch.Generator().manual_seed(6)
    a = torch.randint(-8, 9, (2, 4, 32, 32), generator=g).float().cuda()
    b = torch.randint(-8, 9, (2, 4, 32, 32), generator=g).float().cuda()

    def run(o):
        ag = _leaf(o['a'])
        loss = weighted_l1(ag, o['b'], 8.0)
        ga, = torch.autograd.grad(loss, ag)
        return dict(loss=loss, ga=ga)
    base = sweep(run, dict(a=a, b=b), 'weighted L1')
    d = (a - b).double().cpu()
    assert float(base['loss']) == float(d.abs().mean() * 8.0)
    assert torch.equal(base['ga'].double().cpu(), d.sign() * 8.0 / d.numel())
    _reached(calls, 'afcm_l1_partials', 'afcm_l1_grad')


def test_gauss_blur(calls):
    """The loss-side blur (afcm_gauss_blur), its own adjoint: x and the cotangent; against the float64 definition.  The bound: the
    K = 2 r + 1 normalised taps are fp32 (exp2f, a sum, a division: within 4 units of 2^-24 each), each pass adds K fused multiply-adds,
    and the taps sum to one, so an output is within 2 (K + 4) 2^-24 of the largest input magnitude."""
    from afcm_amd.torch_utils.ops.gauss_blur import gauss_blur
    g = torch.Generator().manual_seed(8)
    x, r = torch.randn(2, 3, 12, 70, generator=g).cuda(), torch.randn(2, 3, 12, 70, generator=g).cuda()
    sigma = 1.5

    def run(o):
        xg = _leaf(o['x'])
        y = gauss_blur(xg, sigma=sigma)
        dx, = torch.autograd.grad(y, xg, o['r'])
        return dict(y=y, dx=dx)
    base = sweep(run, dict(x=x, r=r), 'gauss blur', cotangent=('r', _per_plane(r.shape, F32)))
    rad = int(math.floor(3 * sigma))
    f = torch.exp2(-(torch.arange(-rad, rad + 1).double() / sigma).square())
    f = f / f.sum()
    pad = torch.nn.functional.pad
    def blur(t):
        t = t.double().cpu().reshape(6, 1, 12, 70)
        t = torch.nn.functional.conv2d(pad(t, [rad, rad, 0, 0]), f.reshape(1, 1, 1, -1))
        return torch.nn.functional.conv2d(pad(t, [0, 0, rad, rad]), f.reshape(1, 1, -1, 1)).reshape(2, 3, 12, 70)
    for got, src in ((base['y'], x), (base['dx'], r)):
        assert float((got.double().cpu() - blur(src)).abs().max()) <= 2 * (2 * rad + 1 + 4) * 2.0 ** -24 * float(src.abs().max())
    _reached(calls, 'afcm_gauss_blur')


def test_split16_amax_bits_and_scale_planes_directly(calls):
    """The fp32 split's passes called as ops: amax_bits (documented contiguous-only: a strided x is refused), split16 and scale_planes."""
    conv = _conv()
    node = R.full_node(FP32_CASE, F32)
    x, s = _dev(node.x, F32), _dev(node.s, F32)
    want_bits = conv.amax_bits(V.variant(x, 'aligned'), s).clone()
    assert float(want_bits.view(F32)) == float((node.x * node.s[:, :, None, None]).abs().max())
    want_parts = conv.split16(V.variant(x, 'aligned'), s, 2, F16, want_bits)
    g = conv.pow2_factor(want_bits)
    assert torch.equal(want_parts.double().sum(0).cpu(), node.xs * g), 'the parts add up to g s x'
    want_scaled = conv.scale_planes(V.variant(x, 'aligned'), s)
    R.assert_exact(want_scaled, node.xs, 'scale_planes')
    for name, v in _layouts(x):
        if v.is_contiguous():
            assert torch.equal(conv.amax_bits(v, s), want_bits), name
        else:
            with pytest.raises(AssertionError):
                conv.amax_bits(v, s)
        assert torch.equal(conv.split16(v, s, 2, F16, want_bits), want_parts), name
        assert torch.equal(conv.scale_planes(v, s), want_scaled), name
    for name, v in _layouts(s):
        assert torch.equal(conv.amax_bits(V.variant(x, 'aligned'), v), want_bits), name
        assert torch.equal(conv.split16(V.variant(x, 'aligned'), v, 2, F16, want_bits), want_parts), name
    _reached(calls, 'afcm_amax_bits', 'afcm_split16', 'afcm_scale_planes')
