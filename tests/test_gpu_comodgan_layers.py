"""The CoModGAN generator's wiring (afcm_amd/networks_comodgan.py) on the GPU against the float64 oracle (oracle/comodgan.py), layer by layer
and end to end: ``SynthesisLayer`` and ``ToRGBLayer``, ``SynthesisBlock``, and two tiny generators -- the output and the gradient with
respect to EVERY parameter and input, under ``IMPL='fused'`` and ``IMPL='unfused'``, each against the oracle and not against each other.
Cases and criterion: tests/comodgan_ref.py (``err <= MARGIN * max(Y, median Y)``, Y the float32 oracle's own error);
tests/test_comodgan_oracle_cpu.py proves on the CPU that each planted wiring fault misses that criterion by 4x.

Forward, per element (layers): |y - ref| <= max(4, 4.3 sqrt((K + 8) / 12)) ulps of the tensor's largest magnitude, ulp = np.spacing(float32(max|ref|)),
K = 9 * in_channels the length of the convolution's sums.  4 ulps are too tight for every K here: each of the K roundings of a float32 sum, and
of about 8 more steps around it (style product, the fold or the FIR, demodulation, noise, bias, gain), errs uniformly within half an ulp of a
running value in the binade of the tensor's largest magnitude, so an element's error has sigma = sqrt((K + 8) / 12) ulps, and the largest of
the up to 10^4 elements of a case is expected at 4.3 sigma: 7.3 ulps at K = 27, 13.4 at K = 108, 30 at K = 576.  (A first form of this bound,
2 sigma on the argument that partial sums lie well below the tensor's largest element, was wrong where a clamp caps that largest element at
the size of a typical one: both arms, the framework's own convolution included, ran to 7.8 ulps at K = 108.)  A lost or mis-scaled term is
10^5 ulps and more.

Paths.  ``modconv_epilogue`` and ``conv2d._split_plan`` are wrapped as observers: a fused case ran the epilogue once on the tensor its name says
(4 O channels under the fold) and its convolution took the route its name says (the float16 split, or the native fp32 kernels at odd widths); an
unfused case ran neither.  Which of the epilogue's two access paths (vector / element) a plane width takes is decided inside the kernel's entry
point; tests/test_gpu_modconv_epilogue.py holds both per element.

Random noise: the layer runs after ``torch.manual_seed(s)``; reseeding and drawing ``torch.randn([N, 1, R, R])`` once gives the oracle the same
planes, and the generator state afterwards equal to the state after the layer shows the layer drew exactly that one tensor.  Dropout likewise.

Not tested: a style of exactly 0 or below about 1e-15 -- the convolution's backward recovers d styles as <s x, dx> / s^2, which cannot give that
gradient back (an inherited design limit); inputs beyond the float16 split route's documented 2^18 window; 16-bit blocks and shared-encoder
inference (refused, and the refusals are tested).

Measured on the MI355X (err / max(Y, median Y), worst over the cases of each group; printed by every test before it asserts):
    group (worst output ratio / worst gradient ratio and its gradient, per arm; the layer groups include the dynamic-range and non-foldable cases)
    SynthesisBlock                           fused 0.93 / 1.80 (torgb.bias)    unfused 1.21 / 2.14 (torgb.affine.bias)
    SynthesisLayer 12to20up                  fused 0.87 / 1.40 (w)    unfused 1.06 / 1.97 (affine.weight)
    SynthesisLayer 16to16up                  fused 0.68 / 1.17 (affine.bias)    unfused 0.95 / 2.28 (affine.bias)
    SynthesisLayer 3to130up                  fused 1.22 / 2.29 (w)    unfused 0.79 / 1.58 (x)
    SynthesisLayer 5to3                      fused 1.15 / 3.17 (affine.weight)    unfused 0.84 / 1.58 (weight)
    SynthesisLayer 64to64                    fused 0.86 / 1.24 (w)    unfused 1.39 / 3.04 (noise_strength)
    SynthesisLayer 6to4up5                   fused 0.95 / 1.72 (affine.weight)    unfused 1.06 / 1.77 (noise_strength)
    SynthesisLayer 7to5odd                   fused 1.07 / 0.99 (affine.weight)    unfused 1.10 / 1.23 (noise_strength)
    ToRGBLayer                               1.19 / 1.28 (x)
    generator net16 eval                     fused 0.83 / 1.24 (mapping.fc1.weight)    unfused 0.88 / 1.87 (synthesis.e_fromrgb.con_layer.weight)
    generator net16 train                    fused 0.83 / 1.24 (mapping.fc1.weight)    unfused 0.88 / 1.95 (synthesis.e_fromrgb.con_layer.weight)
    generator net16 train, dropout 0.5       fused 0.90 / 0.94 (synthesis.b8.conv1.affine.weight)    unfused 1.07 / 2.03 (synthesis.b8.conv0.noise_strength)
    generator net32 eval                     fused 0.85 / 1.98 (synthesis.b8.conv0.affine.bias)    unfused 1.17 / 2.10 (synthesis.b8.torgb.weight)
    generator net32 train                    fused 0.85 / 1.98 (synthesis.b8.conv0.affine.bias)    unfused 1.17 / 2.10 (synthesis.b8.torgb.weight)
    generator net32 train, dropout 0.5       fused 0.91 / 2.82 (synthesis.b8.torgb.bias)    unfused 1.36 / 3.29 (synthesis.b32.conv0.noise_strength)
    worst of all: 3.29 (generator net32, batch 2, train, dropout 0.5, unfused arm, synthesis.b32.conv0.noise_strength); 2 x 3.29 = 6.58, so
    MARGIN = 8.  Each planted fault of tests/test_comodgan_oracle_cpu.py stands at 3e5 x the bound or more: 8 satisfies both conditions.
    Forward, per element, worst error / bound in ulps: 5.44 / 7.3 (3 -> 130 up-2, fused), 7.77 / 13.4 (12 -> 20 up-2, unfused), 11.93 / 30.0 (64 -> 64).
    Dynamic range (styles 2^-6 .. 2^6, sample 2 at 2^-8), ratios per sample / worst d weight per input channel:
      12 -> 20 up-2   fused 0.66 0.59 0.60 / 0.79     unfused 0.71 0.73 0.99 / 0.64
      64 -> 64        fused 0.79 0.78 0.63 / 0.76     unfused 1.18 1.32 1.00 / 0.92
    -- the float16 split route is as good as float32 per sample and per input channel inside its window; no route is changed.
    Fused against unfused on the goldens (tests/test_gpu_comodgan.py): worst gradient ratio 3.96 (K1), 2.76 (K2), 1.50 (K3).
    The whole file: 125 tests in 10.8 s.
"""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import comodgan_ref as R

pytestmark = pytest.mark.gpu

SEED = 1234
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


@pytest.fixture
def paths(monkeypatch):
    """Observers on the fused arm's two ops: what ran, on what."""
    from afcm_amd.torch_utils.ops import conv2d as conv
    from afcm_amd.torch_utils.ops import modconv_epilogue as epi
    seen = {'epilogue': [], 'split': []}
    real_epi, real_plan = epi.modconv_epilogue, conv._split_plan

    def recording_epilogue(t, *a, **k):
        seen['epilogue'].append((tuple(t.shape), k.get('up')))
        return real_epi(t, *a, **k)

    def recording_plan(x, ks, *a, **k):
        plan = real_plan(x, ks, *a, **k)
        seen['split'].append((tuple(x.shape), ks, plan is not None))
        return plan

    monkeypatch.setattr(epi, 'modconv_epilogue', recording_epilogue)
    monkeypatch.setattr(conv, '_split_plan', recording_plan)
    return seen


def _assert_paths(seen, impl, case, fused_arm=True):
    i, o, res, up, n = case.info['shape']
    if impl == 'fused' and fused_arm:
        h = res // up
        assert seen['epilogue'] == [((n, up * up * o, h, h), up)], seen
        assert seen['split'] == [((n, i, h, h), 3, h % 2 == 0)], seen          # even width: the float16 split; odd: the native fp32 kernels
    else:
        assert seen['epilogue'] == [] and seen['split'] == [], seen            # the unfused arm: the framework's convolution, bias_act


def _forward_ulps(case, got):
    ref = case.reference()['y'][0]
    i = case.info['shape'][0]
    ks = int(case.module.weight.shape[2])
    bound = max(4.0, 4.3 * math.sqrt((i * ks * ks + 8) / 12.0))
    ulp = float(np.spacing(np.float32(ref.abs().max().item())))
    e = float((got['y'][0].double().cpu() - ref).abs().max()) / ulp
    return e, bound


def _layer_call(case):
    i, o, res, up, n = case.info['shape']
    mode, gain = case.info['mode'], case.info['gain']

    def call(layer, inp):
        if mode != 'random':
            return {'y': layer(inp['x'], inp['w'], noise_mode=mode, gain=gain)}
        torch.manual_seed(SEED)
        start = torch.cuda.get_rng_state()
        y = layer(inp['x'], inp['w'], noise_mode='random', gain=gain)
        after = torch.cuda.get_rng_state()
        torch.manual_seed(SEED)
        if not case.info['use_noise']:
            assert torch.equal(after, start), 'a layer without noise drew from the generator'
            return {'y': y}
        planes = torch.randn([n, 1, res, res], device='cuda')
        assert torch.equal(torch.cuda.get_rng_state(), after) and not torch.equal(after, start), 'the layer did not draw exactly one [N, 1, R, R] tensor'
        if 'planes' in case.consts:
            assert torch.equal(case.consts['planes'], planes.cpu())
        else:
            case.consts['planes'] = planes.cpu()
        return {'y': y}
    return call


def _run_layer(case, impl, paths, monkeypatch, fused_arm=True):
    from afcm_amd import networks_comodgan as nc
    monkeypatch.setattr(nc, 'IMPL', impl)
    got = case.run_module('cuda', _layer_call(case))
    _assert_paths(paths, impl, case, fused_arm)
    if case.info['clamp'] is not None:
        share = R.clamped_share(case)
        print(f'COMOD {case.name}: the float64 oracle clamps {100 * share:.2f} % of the outputs')
        assert 0.01 <= share <= 0.30
    e, bound = _forward_ulps(case, got)
    print(f'COMOD {case.name} {impl}: forward max error {e:.2f} ulps of the largest magnitude (bound {bound:.1f})')
    R.check(case, got, f'{case.name} {impl}')
    assert e <= bound
    return got


LAYER_PARAMS = [(s, v) for s in R.LAYER_SHAPES for v in R.layer_variants(s)]


def test_every_variant_runs():
    assert {v for _, v in LAYER_PARAMS} == set(range(len(R.LAYER_VARIANTS)))
    for v in range(len(R.LAYER_VARIANTS)):
        assert sum(1 for _, u in LAYER_PARAMS if u == v) >= 2


@pytest.mark.parametrize('impl', ['fused', 'unfused'])
@pytest.mark.parametrize('shape,variant', LAYER_PARAMS, ids=[f'{s}-v{v}' for s, v in LAYER_PARAMS])
def test_synthesis_layer(shape, variant, impl, paths, monkeypatch):
    case = _cached(('layer', shape, variant), lambda: R.layer_case(shape, variant))
    _run_layer(case, impl, paths, monkeypatch)


@pytest.mark.parametrize('what', ['linear3x3', 'lrelu1x1'])
def test_non_foldable_layer_takes_the_unfused_arm_under_fused(what, paths, monkeypatch):
    kw = dict(activation='linear') if what == 'linear3x3' else dict(kernel_size=1)
    case = R.layer_case('5to3', R.LAYER_VARIANTS.index(('const', True, 1.0, True)), seed=90, batch=2, **kw)
    assert not case.module.foldable
    _run_layer(case, 'fused', paths, monkeypatch, fused_arm=False)


@pytest.mark.parametrize('impl', ['fused', 'unfused'])
@pytest.mark.parametrize('shape', ['12to20up', '64to64'])
def test_synthesis_layer_dynamic_range(shape, impl, paths, monkeypatch):
    """Styles spread log-uniformly over 2^-6 .. 2^6 across the input channels, sample 2 scaled by 2^-8: y graded per sample against that sample's
    own norm, d weight per input channel -- inside the float16 split route's documented 2^18 window."""
    case = _cached(('dynamic', shape), lambda: R.layer_case(shape, R.LAYER_VARIANTS.index(('const', False, 1.0, True)), seed=77, batch=3, dynamic=True))
    got = _run_layer(case, impl, paths, monkeypatch)
    r = case.ratios(got)
    print(f'COMOD {case.name} dynamic {impl}: per sample', {k: round(v, 3) for k, v in r.items() if k.startswith('y[')})
    print(f'COMOD {case.name} dynamic {impl}: d weight per input channel', [round(v, 2) for k, v in r.items() if k.startswith('weight[')])


@pytest.mark.parametrize('name', sorted(R.TORGB_CASES))
def test_torgb_layer(name, paths):
    case = R.torgb_case(name)
    got = case.run_module('cuda', lambda layer, inp: {'y': layer(inp['x'], inp['w'])})
    assert paths['epilogue'] == []
    if case.info['clamp'] is not None:
        share = R.clamped_share(case)
        print(f'COMOD {case.name}: the float64 oracle clamps {100 * share:.2f} % of the outputs')
        assert 0.01 <= share <= 0.30
    R.check(case, got, case.name)


BLOCK_PARAMS = [(False, cm, sk, im) for cm in (False, True) for sk in R.BLOCK_SKIPS for im in (False, True)] + [(True, False, 'no-features', False),
                                                                                                                  (True, True, 'no-features', False)]


@pytest.mark.parametrize('impl', ['fused', 'unfused'])
@pytest.mark.parametrize('early,cond_mod,skip,with_img', BLOCK_PARAMS)
def test_synthesis_block(early, cond_mod, skip, with_img, impl, paths, monkeypatch):
    from afcm_amd import networks_comodgan as nc
    case = _cached(('block', early, cond_mod, skip, with_img), lambda: R.block_case(early, cond_mod, skip, with_img))
    monkeypatch.setattr(nc, 'IMPL', impl)
    got = case.run_module('cuda', case.info['call'])
    assert len(paths['epilogue']) == ((1 if early else 2) if impl == 'fused' else 0)
    assert all(route for _, _, route in paths['split']) and len(paths['split']) == len(paths['epilogue'])
    R.check(case, got, f'{case.name} {impl}')


def _net_call(case):
    inner = case.info['call']

    def call(G, inp):
        if case.info['mode'] != 'train-dropout':
            return inner(G, inp)
        assert G.training and G.synthesis.dropout.p == 0.5
        torch.manual_seed(SEED)
        out = inner(G, inp)                              # noise_mode='const': the dropout draw is the only one
        after = torch.cuda.get_rng_state()
        torch.manual_seed(SEED)
        n = inp['cond_img'].shape[0]
        mask = F.dropout(torch.ones([n, G.synthesis.fc_in.weight.shape[0]], device='cuda'), p=0.5, training=True)
        assert torch.equal(torch.cuda.get_rng_state(), after), 'the generator drew something besides the dropout mask'
        kept = float((mask != 0).float().mean())
        assert 0.0 < kept < 1.0
        if 'mask' in case.consts:
            assert torch.equal(case.consts['mask'], mask.cpu())
        else:
            case.consts['mask'] = mask.cpu()
        return out
    return call


@pytest.mark.parametrize('impl', ['fused', 'unfused'])
@pytest.mark.parametrize('mode', R.NET_MODES)
@pytest.mark.parametrize('net,batch', R.NET_RUNS)
def test_generator(net, batch, mode, impl, paths, monkeypatch):
    from afcm_amd import networks_comodgan as nc
    case = _cached(('net', net, batch, mode), lambda: R.net_case(net, batch, mode))
    monkeypatch.setattr(nc, 'IMPL', impl)
    got = case.run_module('cuda', _net_call(case))
    layers = sum(1 for m in case.module.modules() if isinstance(m, nc.SynthesisLayer))
    assert len(paths['epilogue']) == (layers if impl == 'fused' else 0), paths
    R.check(case, got, f'{case.name} {impl}')


@pytest.mark.parametrize('skip_resolution', [4, 0])
def test_generator_forward_other_skip_resolutions(skip_resolution):
    case = R.net_case('net16', 3, 'eval', skip_resolution=skip_resolution)
    G = copy.deepcopy(case.module).cuda()
    with torch.no_grad():
        y = G(case.inputs['z'].cuda(), None, case.inputs['cond_img'].cuda(), noise_mode='const')
    ref, _, bound = case.reference()['y']
    e = R.err(y, ref)
    print(f'COMOD {case.name}: forward err {e:.3e}, float32 oracle {bound:.3e}, ratio {e / bound:.3f}')
    assert e <= R.MARGIN * bound
