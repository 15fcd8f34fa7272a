"""Radial (StyleGAN3-R) filters on the CPU: the oracle against the reference's radial fixtures (tools/gen_golden_radial.py), and
the layer schedule / modules against the reference's radial down filters of the full-width 256^2 generator."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import aten_ops as ops
from oracle import direct_np as dnp

TOL = 1e-5
RADIAL_CASES = ['R1_ups4_radial_down', 'R2_asym2d_up_flip', 'R2b_asym2d_up_noflip']


def _close(a, b, tol=TOL, what=''):
    a = a.detach().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    assert err <= tol * scale, f'{what}: max-abs err {err:.3e} (scale {scale:.3g})'


@pytest.mark.parametrize('name', RADIAL_CASES)
def test_oracle_reproduces_radial_fixture(name):
    g = load_golden(name)
    up, down, *pad = [int(v) for v in g['meta']]
    gain, slope, clamp, flip = g['fmeta']
    clamp = None if clamp < 0 else float(clamp)
    assert (g['fu'].ndim == 2) != (g['fd'].ndim == 2)            # one 2-D filter, one separable
    x = torch.from_numpy(g['x']).requires_grad_(True)
    b = torch.from_numpy(g['b']).requires_grad_(True)
    y = ops.filtered_lrelu(x, fu=torch.from_numpy(g['fu']), fd=torch.from_numpy(g['fd']), b=b, up=up, down=down, padding=pad,
                           gain=float(gain), slope=float(slope), clamp=clamp, flip_filter=bool(flip))
    _close(y, g['y'], what=name + ' y')
    dx, db = torch.autograd.grad((y * torch.from_numpy(g['r'])).sum(), [x, b])
    _close(dx, g['dx'], what=name + ' dx')
    _close(db, g['db'], what=name + ' db', tol=1e-4)
    y2 = dnp.filtered_lrelu(g['x'], g['fu'], g['fd'], g['b'], up, down, pad, float(gain), float(slope), clamp, bool(flip))
    _close(y2, g['y'], what=name + ' y(direct)', tol=2e-5)


def test_flip_fixtures_differ():
    """R2 and R2b share every input but flip_filter: with an asymmetric 2-D up filter the outputs must differ."""
    a, b = load_golden('R2_asym2d_up_flip'), load_golden('R2b_asym2d_up_noflip')
    assert np.array_equal(a['x'], b['x']) and np.array_equal(a['fu'], b['fu'])
    assert np.abs(a['y'] - b['y']).max() > 1e-2


def _radial_plan():
    from afcm_amd import layer_schedule
    return layer_schedule.plan(256, 4, 1, {'use_radial_filters': True})


def test_plan_honours_use_radial_filters():
    g = load_golden('R4_radial_filters256')
    pl = _radial_plan()
    got = {L['name']: L['fd'] for L in pl['enc'] + pl['dec'] if L['fd'] is not None and L['fd'].ndim == 2}
    assert sorted(got) == sorted(str(n) for n in g['names']) and len(got) == 14
    for name, f in zip(g['names'], g['filters']):
        assert got[str(name)].dtype == torch.float32
        assert np.array_equal(got[str(name)].numpy(), f), name
    # every other layer keeps its separable filter, unchanged from the default schedule
    from afcm_amd import layer_schedule
    base = layer_schedule.plan(256, 4, 1, {})
    for L, B in zip(pl['enc'] + pl['dec'], base['enc'] + base['dec']):
        if L['name'] not in got:
            assert (L['fd'] is None and B['fd'] is None) or torch.equal(L['fd'], B['fd']), L['name']
        assert (L['fu'] is None and B['fu'] is None) or torch.equal(L['fu'], B['fu']), L['name']
        assert L['padding'] == B['padding'] and L['up'] == B['up'] and L['down'] == B['down']


def test_algorithmic_work_counts_radial_layers_like_separable_ones():
    """A 12 x 12 radial down filter has the same sign grid as the 12-tap separable one it replaces."""
    from afcm_amd import layer_schedule
    a = layer_schedule.algorithmic_work(_radial_plan(), 16, 2)
    b = layer_schedule.algorithmic_work(layer_schedule.plan(256, 4, 1, {}), 16, 2)
    assert a == b


def test_module_down_filters_match_the_reference():
    from afcm_amd.networks_stylegan3 import Stylegan3Generator
    from afcm_amd.layer_schedule import DEFAULT_SYNTHESIS_KWARGS
    g = load_golden('R4_radial_filters256')
    torch.manual_seed(0)
    G = Stylegan3Generator(z_dim=512, c_dim=1, w_dim=512, img_resolution=256, img_channels_in=4, img_channels_out=1,
                           mapping_kwargs=dict(num_layers=8),
                           synthesis_kwargs=dict(DEFAULT_SYNTHESIS_KWARGS, use_radial_filters=True))
    got = {n: m.down_filter for n, m in G.synthesis.named_children()
           if getattr(m, 'down_filter', None) is not None and m.down_filter.ndim == 2}
    assert sorted(got) == sorted(str(n) for n in g['names'])
    for name, f in zip(g['names'], g['filters']):
        assert np.array_equal(got[str(name)].numpy(), f), name
