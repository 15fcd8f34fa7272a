"""oracle/comodgan.py, the float64 restatement of the CoModGAN generator, pinned to the reference's own outputs (tests/golden/K1, K2, K3:
tools/gen_golden_comodgan.py), and the criterion of tests/comodgan_ref.py proven to have teeth.  CPU only.

Pin.  The goldens are the reference in float32, so float64 oracle - golden is the reference's own rounding.  First the bounds
tests/test_gpu_comodgan.py applies to the device (a floor), then 8x what this comparison measures on the CPU, where it is deterministic:

    golden        eval forward max-abs / scale    train forward max-abs / scale    worst gradient relative L2
    K1_comod64    7.589e-07                        8.390e-07                        9.262e-06 (synthesis.b16.conv0.noise_strength)
    K2_comod128   1.119e-06                        1.068e-06                        2.800e-06 (synthesis.b128.conv0.affine.weight)
    K3_comod32    8.551e-07                        1.007e-06                        3.313e-06 (synthesis.e_b4.conv_layer1.weight)
    (scale = max(1, max|y|)); worst over the three: forward 1.119e-06, gradient 9.262e-06 -- asserted: 8x each, FWD_BOUND and GRAD_BOUND.

Teeth.  The oracle in float32 with ONE planted wiring fault (oracle.comodgan.FAULTS) must miss the criterion by 4x at least on one graded
quantity: err >= 4 * MARGIN * bound.  Cases: the 12 -> 20 up-2 layer (noise_mode='const', clamp, gain sqrt(0.5)), the 32^2 network of the
device tests in train() at batch 2, and -- for the fault that reads another row of ``ws``, which through the mapping network (every row the
same vector) is no fault at all -- that network's synthesis half on a ``ws`` whose rows differ.  The unplanted float32 oracle passes at
ratio 1 by construction."""
import numpy as np
import pytest
import torch

import comodgan_ref as R
from conftest import load_golden
from oracle import comodgan as O
from test_comodgan_fold_cpu import GOLDEN_CONFIGS

FWD_BOUND = 8 * 1.119e-6         # 8 x the worst measured forward max-abs / scale (docstring)
GRAD_BOUND = 8 * 9.262e-6        # 8 x the worst measured gradient relative L2


@pytest.mark.parametrize('name', sorted(GOLDEN_CONFIGS))
def test_float64_oracle_reproduces_the_reference_golden(name):
    g = load_golden(name)
    cfg = GOLDEN_CONFIGS[name]
    skw = cfg['synthesis_kwargs']
    sd = {k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith('sd/')}
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    names = [str(n) for n in g['names']]
    for k in names:
        sd[k].requires_grad_(True)
    z, x, r = (torch.from_numpy(g[k].astype(np.float64)) for k in ('z', 'cond_img', 'r'))
    c = torch.from_numpy(g['c'].astype(np.float64)) if 'c' in g else None
    y = O.generator(sd, z, c, x, cfg['img_resolution'], mapping_layers=2, skip_resolution=skw['skip_resolution'], cond_mod=skw.get('cond_mod', False),
                    conv_clamp=skw.get('conv_clamp'), noise='const')
    grads = dict(zip(names, torch.autograd.grad((y * r).sum(), [sd[k] for k in names])))
    y = y.detach().numpy()
    fwd = {}
    for which in ('y_eval', 'y_train'):             # the oracle has one arithmetic; the reference's eval() is its grouped-conv form
        scale = max(1.0, float(np.abs(g[which]).max()))
        e = float(np.abs(y - g[which]).max())
        fwd[which] = e / scale
        print(f'{name}: float64 oracle vs {which}: max-abs {e:.3e}, scale {scale:.3f}, ratio {e / scale:.3e}')
        assert e <= 1e-3 and e <= 5e-5 * scale                                           # the floor: what the device test asks
    worst = (0.0, '')
    for k in names:
        w = g['g/' + k].astype(np.float64)
        d = grads[k].numpy() - w
        nw, ng = float(np.sqrt((w ** 2).sum())), float(np.sqrt((grads[k].numpy() ** 2).sum()))
        rel = float(np.sqrt((d ** 2).sum()) / max(1e-30, nw))
        worst = max(worst, (rel, k))
        assert rel <= 1e-2 and float(np.abs(d).max()) <= 2e-2 * max(1.0, float(np.abs(w).max())) and abs(ng - nw) <= 5e-3 * max(1.0, nw), (k, rel)
    print(f'{name}: worst gradient relative L2 {worst[0]:.3e} ({worst[1]})')
    assert max(fwd.values()) <= FWD_BOUND, fwd
    assert worst[0] <= GRAD_BOUND, worst


def _teeth_cases():
    layer = R.layer_case('12to20up', R.LAYER_VARIANTS.index(('const', True, float(np.sqrt(0.5)), True)))
    return {'layer': layer, 'net': R.net_case('net32', 2, 'train'), 'net-ws': R.net_case('net32', 2, 'train', distinct_ws=True)}


TEETH = [('torgb_no_weight_gain', 'net'), ('phase_order', 'layer'), ('phase_order', 'net'), ('no_d_noise_strength', 'layer'), ('no_d_noise_strength', 'net'),
         ('skip_before_act', 'net'), ('no_dcoefs_dweight', 'layer'), ('no_dcoefs_dweight', 'net'), ('no_dcoefs_dstyles', 'layer'),
         ('no_dcoefs_dstyles', 'net'), ('clamp_no_gain', 'layer'), ('conv1_next_w', 'net-ws')]
_CASES = {}


def _case(which):
    if not _CASES:
        _CASES.update(_teeth_cases())
    return _CASES[which]


def test_every_fault_has_a_tooth():
    assert sorted({f for f, _ in TEETH}) == sorted(O.FAULTS)


@pytest.mark.parametrize('which', ['layer', 'net', 'net-ws'])
def test_unplanted_float32_oracle_passes(which):
    case = _case(which)
    assert R.check(case, case.run_oracle(torch.float32), f'{case.name} float32 oracle') <= 1.0


@pytest.mark.parametrize('fault,which', TEETH)
def test_planted_fault_misses_the_criterion_by_4x(fault, which):
    case = _case(which)
    r = case.ratios(case.run_oracle(torch.float32, fault=fault))
    worst = max((v, k) for k, v in r.items())
    print(f'COMOD teeth {fault} on {case.name}: worst err / bound {worst[0]:.3e} ({worst[1]}); needed {4 * R.MARGIN}')
    assert worst[0] >= 4 * R.MARGIN
