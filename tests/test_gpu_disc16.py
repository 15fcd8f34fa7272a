"""The discriminator's 16-bit path -- MFMA convs incl. the stride-2 kernel, bias_act, upfirdn2d, and the R1 double backward through
all of them -- op by op, block by block and as a network against float64 references of the same mathematics (tests/disc16_ref.py):
one on the operands the kernels multiply ("pure"), one with a rounding node wherever the product stores a 16-bit tensor
("emulated").  Bars: the project's own for single launches from exact operands (1.05 ulp; 1e-4 / 2e-4 of an fp32 sum), and for
everything downstream of a stored 16-bit tensor  relL2(kernel - emulated) <= E / 4 + fp32 floor  with  E = relL2(emulated - pure)
computed in the test.  Every case asserts the route it means to test (launch names seen by ``_lib.launched``, upfirdn2d launches).
Every figure is printed before it is asserted (``pytest -s`` / ``-rP``)."""
import collections

import numpy as np
import pytest
import torch

import disc16_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture
def calls(monkeypatch):
    """Counter of kernel launches by name: everything that goes through ``_lib.launched``, plus 'upfirdn2d' / 'upfirdn2d_stuff'
    (the one-tap up=2 zero-stuffing) for the op that checks its status itself."""
    from afcm_amd import _lib
    from afcm_amd.torch_utils.ops import upfirdn2d as U
    seen = collections.Counter()
    launched, launch = _lib.launched, U._launch

    def spy(rc, what):
        seen[what] += 1
        return launched(rc, what)

    def spy_upfirdn(x, f2d, upx, upy, *rest):
        seen['upfirdn2d_stuff' if (upx == 2 and tuple(f2d.shape) == (1, 1)) else 'upfirdn2d'] += 1
        return launch(x, f2d, upx, upy, *rest)
    monkeypatch.setattr(_lib, 'launched', spy)
    monkeypatch.setattr(U, '_launch', spy_upfirdn)
    return seen


def _gpu(t, dtype=None):
    t = t.to(torch.float32).cuda()
    return (t if dtype is None else t.to(dtype)).requires_grad_(True)


def _compare(kq, p, e, rules, dtype, what, floor_norms=None, factor=R.E_FACTOR):
    assert set(rules) <= set(kq) and set(rules) <= set(p), (sorted(rules), sorted(kq))
    recs = []
    for name, rule in rules.items():
        k = kq[name]
        if rule != 'zero':
            assert k is not None and k.shape == p[name].shape, (what, name)
            assert bool(torch.isfinite(k).all()), (what, name)
        recs.append(R.judge(rule, name, k, p[name], e[name], dtype, factor=factor, floor_norm=(floor_norms or {}).get(name)))
    R.check(recs, f'DISC16 {what} {str(dtype)[6:]}')
    return recs


def _run(what, dtype, ref_fn, gpu_fn, leaves64, leaf_dtypes, xname, others, rules, calls, seed, x_second=False):
    """The R1 quantities of one op-level case on the GPU and in both references, compared by ``rules``; returns the launch counters
    after the forward pass and at the end."""
    with torch.no_grad():
        shape = ref_fn(leaves64, R.Lowp(dtype, False)).shape
    r, q = R.cotangents(dtype, seed, shape, leaves64[xname].shape)
    p, e, _ = R.both_references(ref_fn, lambda: leaves64, xname, others, r, q, dtype, x_second=x_second)
    lv = {k: _gpu(v, dtype if leaf_dtypes[k] else None) for k, v in leaves64.items()}
    snap = {}

    def fwd(leaves):
        calls.clear()
        y = gpu_fn(leaves)
        snap['fwd'] = collections.Counter(calls)
        assert y.dtype == dtype and tuple(y.shape) == tuple(shape), (what, y.dtype, y.shape, shape)
        return y
    kq = R.r1_quantities(fwd, lv, xname, others, _gpu(r), q.float().cuda(), f32=lambda t: t.float(), x_second=x_second)
    _compare(kq, p, e, rules, dtype, what)
    return snap['fwd'], collections.Counter(calls)


# ------------------------------------------------------------------------------------------------------- a. convolutions
def _conv_gpu(mode, pad=0):
    from afcm_amd.torch_utils.ops import conv2d as C
    from afcm_amd.torch_utils.ops import conv2d_resample, upfirdn2d
    if mode == 's2':
        def fn(lv):
            assert C.strided_conv2d_supported(lv['x'], lv['w'], pad)
            return C.strided_conv2d(lv['x'], lv['w'], pad)
        return fn
    ks = 1 if mode.endswith('1') else 3
    down = 2 if mode.startswith('down') else 1
    filt = upfirdn2d.setup_filter(R.FILT).cuda()          # what Conv2dLayer registers: the 4 x 4 outer product
    return lambda lv: conv2d_resample.conv2d_resample(x=lv['x'], w=lv['w'], f=filt, down=down, padding=ks // 2)


def _conv_case(mode, dims, dtype, calls, what, seed, pad=0):
    n, cin, cout, h, w = dims
    ks = 1 if mode.endswith('1') else 3
    leaves = R.conv_inputs(dtype, seed, n, cin, cout, h, w, ks)
    return _run(what, dtype, R.conv_reference(mode, pad), _conv_gpu(mode, pad), leaves, dict(x=True, w=False), 'x', ['w'],
                R.conv_rules(mode), calls, seed)


@pytest.mark.parametrize('dtype', R.DTYPES, ids=str)
@pytest.mark.parametrize('case', R.DOWN3, ids=lambda c: c[0])
def test_down_conv_layer_vs_float64(case, dtype, calls):
    """3x3, down 2, [1, 3, 3, 1], padding 1 as Conv2dLayer calls conv2d_resample: the blur, then _StridedConv2d on
    conv2d_fwd16s2_kernel; gradients and the R1 pattern through _StridedConv2d.backward (zero-stuffing, _ScaledConv2d with the
    transposed flipped weights at pad 2, _ConvWgrad at pad 0) and upfirdn2d re-entering itself.  Production planes at N = 1 and the
    tile shapes of choose_tile_s2 (tests/disc16_ref.py DOWN3)."""
    cid, n, cin, cout, h, w, _ = case
    fwd, total = _conv_case('down3', (n, cin, cout, h, w), dtype, calls, f'down3/{cid}', 20 + R.DOWN3.index(case))
    assert fwd['conv2d_stride2'] == 1 and fwd['conv2d'] == 0 and fwd['upfirdn2d'] == 1, fwd
    assert total['conv2d'] >= 2 and total['conv2d_wgrad'] >= 2 and total['conv2d_stride2'] == 1, total
    # the backward's zero-stuffing route: the blurred width is even, so the one-tap upfirdn2d runs exactly when the output width is even
    assert (total['upfirdn2d_stuff'] > 0) == (R.down_out(w) % 2 == 0), (cid, R.down_out(w), total)


@pytest.mark.parametrize('dtype', R.DTYPES, ids=str)
@pytest.mark.parametrize('case', R.S2, ids=lambda c: c[0])
def test_strided_conv_backward_routes_vs_float64(case, dtype, calls):
    """strided_conv2d called directly at pads 0 / 1 / 2: the backward's two zero-stuffing routes -- the one-tap up=2 upfirdn2d (with
    the crop an odd-height plane asks of its trailing padding) and the slice assignment."""
    cid, n, cin, cout, h, w, pad, one_tap = case
    fwd, total = _conv_case('s2', (n, cin, cout, h, w), dtype, calls, f's2/{cid}', 40 + R.S2.index(case), pad)
    assert fwd['conv2d_stride2'] == 1 and fwd['conv2d'] == 0, fwd
    assert (total['upfirdn2d_stuff'] > 0) == one_tap, (cid, total)
    assert total['conv2d'] >= 2 and total['conv2d_wgrad'] >= 2, total


@pytest.mark.parametrize('dtype', R.DTYPES, ids=str)
@pytest.mark.parametrize('case', R.PLAIN, ids=lambda c: c[0])
def test_plain_and_skip_conv_layers_vs_float64(case, dtype, calls):
    """conv0 (3x3 pad 1), fromrgb (1x1, 5 channels) and the skip layer (1x1 + down 2: upfirdn2d first) on _ScaledConv2d; the R1
    pattern puts the transposed, flipped weights at pad k - 1 - pad with Cin and Cout swapped (tails on both sides)."""
    cid, mode, n, cin, cout, h, w = case
    fwd, total = _conv_case(mode, (n, cin, cout, h, w), dtype, calls, f'{mode}/{cid}', 60 + R.PLAIN.index(case))
    assert fwd['conv2d'] == 1 and fwd['conv2d_stride2'] == 0 and fwd['upfirdn2d'] == (1 if mode == 'down1' else 0), fwd
    assert total['conv2d'] >= 3 and total['conv2d_wgrad'] >= 2, total


@pytest.mark.parametrize('dtype', R.DTYPES, ids=str)
@pytest.mark.parametrize('case', R.GATE, ids=lambda c: c[0])
def test_odd_widths_take_the_framework_conv_and_match(case, dtype, calls):
    """The gate of _conv2d_wrapper: an odd width in 16 bit is the framework convolution's -- no MFMA launch -- and still the
    reference's operation.  The framework's 16-bit convolution is not held to one rounding of an fp32 sum (measured here: up to
    1.8 ulp for float16), so the bar is the larger of the single-launch bar and the error the framework convolution itself makes
    against float64 when called directly on the same tensors: the route may add nothing to it.  The route behind the gate IS that
    framework convolution, so the value comparison is deliberately weak (close to a self-comparison: it catches a wrong padding,
    stride or flip in the wrapper, not the framework's arithmetic); the assertion that carries the case is "no conv2d* launch"."""
    import torch.nn.functional as F
    cid, mode, n, cin, cout, h, w = case
    ks = 1 if mode.endswith('1') else 3
    seed = 80 + R.GATE.index(case)
    leaves = R.conv_inputs(dtype, seed, n, cin, cout, h, w, ks)
    ref_fn = R.conv_reference(mode)
    with torch.no_grad():
        shape = ref_fn(leaves, R.Lowp(dtype, False)).shape
    r, q = R.cotangents(dtype, seed, shape, leaves['x'].shape)
    p, _, _ = R.both_references(ref_fn, lambda: leaves, 'x', ['w'], r, q, dtype)
    got = {}
    for who, fn in (('route', _conv_gpu(mode)), ('framework', lambda lv: F.conv2d(lv['x'], lv['w'].to(dtype), padding=ks // 2))):
        calls.clear()
        lv = dict(x=_gpu(leaves['x'], dtype), w=_gpu(leaves['w']))
        got[who] = R.r1_quantities(fn, lv, 'x', ['w'], _gpu(r), q.float().cuda(), f32=lambda t: t.float())
        assert not any(k.startswith('conv2d') for k in calls), (who, calls)
    for name in ('y', 'dx', 'dw'):
        scale = float(p[name].abs().max())
        err, own = (float((got[who][name] - p[name]).abs().max()) for who in ('route', 'framework'))
        bar = max(R.ONE_ROUNDING * R.ULP[dtype] * scale, own)
        print(f'DISC16 gate/{cid} {str(dtype)[6:]} {name}: err {err:.3e}, the framework conv alone {own:.3e}, one rounding {R.ULP[dtype] * scale:.3e}')
        assert got['route'][name].shape == p[name].shape and err <= bar, (cid, name, err, bar)


# ------------------------------------------------------------------------------------------------------- b. _ConvWgrad
@pytest.mark.parametrize('dtype', R.DTYPES, ids=str)
@pytest.mark.parametrize('case', R.WGRAD, ids=lambda c: c[0])
def test_conv_wgrad_node_vs_float64(case, dtype, calls):
    """_ConvWgrad: the fp32 weight gradient from 16-bit dy and x, and its own gradients -- a forward convolution of x with the
    incoming (representable) cotangent in the weight slot, and a data-gradient convolution of dy with it transposed and flipped."""
    from afcm_amd.torch_utils.ops import conv2d as C
    cid, n, cin, cout, ks, h, w, pad = case
    seed = 90 + R.WGRAD.index(case)
    x = R.randn16([n, cin, h, w], dtype, seed)
    dy = R.randn16([n, cout, h + 2 * pad - ks + 1, w + 2 * pad - ks + 1], dtype, seed + 1)
    g = R.randn16([cout, cin, ks, ks], dtype, seed + 2)
    dyr, xr = dy.clone().requires_grad_(True), x.clone().requires_grad_(True)
    dw = R.wgrad_reference(ks, pad)(dyr, xr)
    p = dict(zip(('g_dy', 'g_x'), map(R.f64, torch.autograd.grad((dw * g).sum(), [dyr, xr]))), dw=R.f64(dw))
    dyg, xg = _gpu(dy, dtype), _gpu(x, dtype)
    calls.clear()
    got = C._ConvWgrad.apply(dyg, xg, ks, pad)
    assert got.dtype == torch.float32 and calls['conv2d_wgrad'] == 1, calls
    kq = dict(zip(('g_dy', 'g_x'), map(R.f64, torch.autograd.grad((got * g.float().cuda()).sum(), [dyg, xg]))), dw=R.f64(got))
    assert calls['conv2d'] == 2, calls
    _compare(kq, p, p, {'dw': 'fp32', 'g_dy': 'ulp', 'g_x': 'ulp'}, dtype, f'wgrad/{cid}')


# ------------------------------------------------------------------------------------------------------- c. bias_act
@pytest.mark.parametrize('dtype', R.DTYPES, ids=str)
@pytest.mark.parametrize('case', R.BIAS_ACT, ids=lambda c: c[0])
def test_bias_act_orders_0_1_2_vs_float64(case, dtype, calls):
    """bias_act in 16 bit, forward / grad = 1 / grad = 2 modes with gain and clamp, vector and element paths, gradients w.r.t. x, b
    and dy.  The inputs keep 4 ulp away from the leaky-ReLU kink and from the clamp (asserted before the GPU is touched), so
    max-abs bars apply; second derivatives that are identically zero must come back None or exactly zero."""
    from afcm_amd.torch_utils.ops import bias_act as B
    cid, shape, act, gain, clamp, with_b = case
    x, b = R.bias_act_inputs(case, dtype)
    kink, edge = R.bias_act_margins(x, b, act, gain, clamp, dtype)
    assert not bool(kink.any()) and not bool(edge.any()), cid
    leaves = dict(x=x, b=b) if with_b else dict(x=x)
    gpu_fn = lambda lv: B.bias_act(lv['x'], lv.get('b'), act=act, gain=gain, clamp=clamp)
    fwd, total = _run(f'bias_act/{cid}', dtype, R.bias_act_reference(case), gpu_fn, leaves, dict(x=True, b=True), 'x', ['b'] if with_b else [],
                      R.bias_act_rules(case), calls, 100 + R.BIAS_ACT.index(case), x_second=True)
    assert fwd['bias_act'] == 1, fwd
    # forward, grad = 1 once, its double backward w.r.t. dy twice; a smooth activation adds the grad = 2 launch twice
    assert total['bias_act'] >= 1 + 1 + 2 + (2 if act == 'swish' else 0), total
    if with_b and len(shape) == 4:
        assert total['plane_dot'] >= (3 if act == 'swish' else 1), total      # _SumPlanes: db, and the second-order d_b of a smooth activation


# ------------------------------------------------------------------------------------------------------- d. upfirdn2d
@pytest.mark.parametrize('dtype', R.DTYPES, ids=str)
@pytest.mark.parametrize('case', R.UPFIRDN, ids=lambda c: c[0])
def test_upfirdn2d_second_order_at_the_discriminators_calls(case, dtype, calls):
    """upfirdn2d in 16 bit as the discriminator calls it.  The op is linear: the gradient of <its gradient, q> w.r.t. dy is the
    forward op on q, and must equal it on the float64 side to one rounding."""
    from afcm_amd.torch_utils.ops import upfirdn2d as U
    cid, shape, up, down, padding, one_tap = case
    seed = 120 + R.UPFIRDN.index(case)
    f = R.upfirdn_filter(one_tap).cuda()
    gpu_fn = lambda lv: U.upfirdn2d(lv['x'], f, up=up, down=down, padding=padding)
    fwd, total = _run(f'upfirdn2d/{cid}', dtype, R.upfirdn_reference(case), gpu_fn, dict(x=R.randn16(shape, dtype, seed)), dict(x=True), 'x', [],
                      R.upfirdn_rules(case), calls, seed)
    key = 'upfirdn2d_stuff' if one_tap else 'upfirdn2d'
    assert fwd[key] == 1 and sum(fwd.values()) == 1, fwd
    assert total['upfirdn2d'] + total['upfirdn2d_stuff'] == 4, total           # forward, its gradient, and the gradient of that for sq and q


# ------------------------------------------------------------------------------------------------------- blocks
def _hook_layers(module, names, sink):
    for name in names:
        layer = module.get_submodule(name) if name else module
        layer.register_forward_hook(lambda m, i, o, name=name: sink.setdefault(name, []).append(o.detach()))


@pytest.mark.parametrize('dtype', R.DTYPES, ids=str)
@pytest.mark.parametrize('case', R.BLOCKS, ids=lambda c: c[0])
def test_discriminator_block_vs_float64(case, dtype, calls):
    """DiscriminatorBlock ('resnet', use_fp16, conv_clamp 256) against oracle.discriminator.discriminator_block in float64: output,
    R1 image gradient, first-order gradients and the gradients of sum g^2 and <g, q> w.r.t. EVERY parameter, all by the E rule; the
    leaky-ReLU branch decisions at each activation's output by the share rule."""
    from afcm_amd.networks_discriminator import DiscriminatorBlock
    cid, n, cin, tmp, cout, res = case
    first = cin == 0
    sd, x = R.block_state(case), R.block_input(case, dtype)
    ref_fn = R.block_reference(case)
    leaves64 = dict(sd, x=x)
    with torch.no_grad():
        shape = ref_fn(leaves64, R.Lowp(dtype, False)).shape
    seed = 200 + R.BLOCKS.index(case)
    r, q = R.cotangents(dtype, seed, shape, x.shape)
    p, e, (lp, le) = R.both_references(ref_fn, lambda: leaves64, 'x', list(sd), r, q, dtype)
    blk = DiscriminatorBlock(cin, tmp, cout, resolution=res, img_channels=5, first_layer_idx=0, architecture='resnet', conv_clamp=R.BLOCK_CLAMP,
                             use_fp16=True, fp16_dtype=dtype)
    missing = blk.load_state_dict({k: v.float() for k, v in sd.items()}, strict=False)
    assert not missing.unexpected_keys and all(k.endswith('resample_filter') for k in missing.missing_keys), missing
    blk = blk.cuda()
    acts = {}
    layers = [k for k in R.BLOCK_LAYERS if first or k != 'fromrgb']
    _hook_layers(blk, layers, acts)
    lv = dict(blk.named_parameters())
    assert set(lv) == set(sd)
    lv['x'] = _gpu(x, None if first else dtype)        # the first block casts the fp32 image itself
    snap = {}

    def fwd(leaves):
        calls.clear()
        y = blk(None, leaves['x'])[0] if first else blk(leaves['x'], None)[0]
        snap['fwd'] = collections.Counter(calls)
        return y
    kq = R.r1_quantities(fwd, lv, 'x', list(sd), _gpu(r), q.float().cuda(), f32=lambda t: t.float())
    assert kq['y'].shape == tuple(shape)
    # conv1 on the stride-2 kernel, conv0 / skip (/ fromrgb) on the stride-1 MFMA kernel, two upfirdn2d (blur, skip decimation)
    assert snap['fwd']['conv2d_stride2'] == 1 and snap['fwd']['conv2d'] == (3 if first else 2) and snap['fwd']['upfirdn2d'] == 2, snap['fwd']
    assert snap['fwd']['bias_act'] == (4 if first else 3), snap['fwd']
    rules = {k: R.chain_rule(p, e, k) for k in p}
    assert sorted(k for k, v in rules.items() if v == 'zero') == sorted(f'{t}/d{k}' for t in ('sq', 'q') for k in sd if k.endswith('bias'))
    _compare(kq, p, e, rules, dtype, f'block/{cid}')
    for k in layers:
        assert len(acts[k]) == 1
        R.check_signs(R.f64(acts[k][0]), lp.trace[f'b.{k}.'], le.trace[f'b.{k}.'], f'DISC16 block/{cid} {str(dtype)[6:]} {k}')


# ------------------------------------------------------------------------------------------------------- network
def build_network(g, dtype):
    from afcm_amd.networks_discriminator import CoModDiscriminator
    res, n, cb, cm, group, clamp = [int(v) for v in g['meta']]
    D = CoModDiscriminator(c_dim=0, img_resolution=res, img_channels=5, channel_base=cb, channel_max=cm, conv_clamp=clamp,
                           num_fp16_res=R.NETWORK_FP16_RES, block_kwargs=dict(fp16_dtype=dtype), epilogue_kwargs=dict(mbstd_group_size=group))
    D.load_state_dict({k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith('sd/')}, strict=True)
    return D.cuda()


def network_rules_and_floors(p, e):
    rules = {k: R.chain_rule(p, e, k) for k in p}
    floors = {}
    for prefix in ('gr1/', 'greal/', 'gfake/'):
        floors.update(R.group_norms(e, prefix))
    return rules, floors


@pytest.mark.parametrize('dtype', R.DTYPES, ids=str)
def test_discriminator_network_16bit_vs_emulated_float64(dtype, calls):
    """The D2_tiny128_clamp golden network with its three highest-resolution blocks in 16 bit against the float64 oracle with the
    same blocks' storage emulated: logits, R1 image gradient, and per parameter tensor the gradients of the R1 term, the real term
    and the fake term, and the image gradient of the G term, each by the E rule (floors at the scale of the group's largest tensor).

    Leaky-ReLU branch decisions are compared at every activation of the network, fp32 blocks included, in all three passes: the
    kernels may disagree with the emulated reference on no larger a share than the two references with each other -- never more
    than 1e-3, which the bfloat16 references alone exceed at nine layers (disc16_ref.NETWORK_WIDE) -- plus two elements.  The
    factor of the E rule is 1 / 4, except for the gradients whose cotangent passes through an activation where a decision
    differs: those get 1, the ceiling, for the cause named and measured at disc16_ref.BRANCH_FLIP_FACTOR (in this tiny network
    one flipped element of a 6144-output layer moves the gradients by more than rounding does).  Logits, the gradients of
    layers behind the flipped activation, and a run without flips stay at 1 / 4.  Measured on an MI355X: bfloat16 no flip, at
    most 0.36 E (R1 image gradient 0.008 E); float16 two flips at b16.conv0 in the real pass and one at b32.conv0 in the two
    fake passes, R1 image gradient 0.65 E, G-term image gradient 0.42 E, parameter gradients at most 1.17 E (gr1/b4.out.weight,
    12 elements, at 0.94 of its bar with the floor)."""
    g = load_golden(R.NETWORK)
    p, e, (lp, le) = R.network_references(g, dtype)
    D = build_network(g, dtype)
    acts = {}
    layers = [k for k in lp.passes[0] if not k.endswith('skip.')]
    assert len(layers) == 12
    _hook_layers(D, [k[:-1] for k in layers], acts)
    names = [str(k) for k in g['names']]
    params = dict(D.named_parameters())
    seen = []

    def net(img):
        calls.clear()
        y = D(img, None)
        seen.append(collections.Counter(calls))
        return y
    kq = R.network_quantities(net, {k: params[k] for k in names}, torch.from_numpy(g['fake']).cuda(), torch.from_numpy(g['real']).cuda())
    for fwd in seen:           # each pass: three 16-bit blocks on the MFMA kernels (fromrgb + 3 x (conv0, skip)), the rest on the framework conv
        assert fwd['conv2d_stride2'] == R.NETWORK_FP16_RES and fwd['conv2d'] == 1 + 2 * R.NETWORK_FP16_RES, fwd
    flipped = {n_pass: [] for n_pass in range(3)}
    for n_pass in range(3):
        for k in layers:
            n = R.check_signs(R.f64(acts[k[:-1]][n_pass]), lp.passes[n_pass][k], le.passes[n_pass][k],
                              f'DISC16 network {str(dtype)[6:]} pass {n_pass} {k}', sharp=(n_pass, k) not in R.NETWORK_WIDE[dtype])
            if n:
                flipped[n_pass].append(k)
    print(f'DISC16 network {str(dtype)[6:]}: branch decisions differ from the emulated reference at {flipped}')
    rules, floors = network_rules_and_floors(p, e)
    assert all(k.startswith('gr1/') and k.endswith('bias') for k, v in rules.items() if v == 'zero')
    recs = []
    for factor in (R.E_FACTOR, R.BRANCH_FLIP_FACTOR):
        group = {k: v for k, v in rules.items() if R.network_factor(k, flipped) == factor}
        if group:
            recs.append((factor, group))
    assert sum(len(gr) for _, gr in recs) == len(rules) and all(R.network_factor(k, flipped) == R.E_FACTOR for k in ('gen_logits', 'real_logits'))
    failures = []
    for factor, group in recs:
        try:
            _compare(kq, p, e, group, dtype, f'network[factor {factor}]', floor_norms=floors, factor=factor)
        except AssertionError as err:
            failures.append(str(err))
    assert not failures, failures
