"""CoModGAN generator, CPU side: the fold of the up-2 layer into four 3x3 phase kernels against the composition it replaces
(transposed stride-2 convolution, pad, 4x4 FIR with gain 4 -- ``conv2d_resample(up=2, padding=1, flip_weight=False)``) in float64;
the state-dict keys of the golden fixtures; the refusals."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from afcm_amd import networks_comodgan as nc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _up2_composition(x, w):
    """conv2d_resample.py:127-143 of the reference for up=2, a 3x3 kernel, f=[1,3,3,1], padding=1, flip_weight=False."""
    o = w.shape[0]
    y = F.conv_transpose2d(x, w.transpose(0, 1), stride=2)                   # [N, O, 2H + 1, 2W + 1]
    y = F.pad(y, [1, 1, 1, 1])
    f = torch.tensor([1, 3, 3, 1], dtype=x.dtype)
    f2 = torch.outer(f, f) / 64 * 4                                           # normalised, gain up^2 (symmetric: the flip is the identity)
    return F.conv2d(y, f2.expand(o, 1, 4, 4).contiguous(), groups=o)          # [N, O, 2H, 2W]


def _folded(x, w):
    return nc.unfold_phases(F.conv2d(x, nc.fold_up2_weights(w), padding=1))


@pytest.mark.parametrize('plane', [(1, 1), (2, 2), (3, 5), (7, 7)])
@pytest.mark.parametrize('io', [(1, 1), (5, 3)])
def test_fold_equals_transposed_conv_then_fir(plane, io):
    g = torch.Generator().manual_seed(1000 * plane[0] + 10 * plane[1] + io[0])
    x = torch.randn(2, io[0], *plane, dtype=torch.float64, generator=g)
    w = torch.randn(io[1], io[0], 3, 3, dtype=torch.float64, generator=g)
    want, got = _up2_composition(x, w), _folded(x, w)
    assert got.shape == want.shape == (2, io[1], 2 * plane[0], 2 * plane[1])
    err = (got - want).abs().max().item()
    print(f'plane {plane} (I, O) {io}: max-abs {err:.3e}, scale {want.abs().max().item():.3e}')
    assert err <= 1e-12 * want.abs().max().item()


def test_fold_gradcheck_wrt_weight():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 3, 5, dtype=torch.float64, generator=g)
    w = torch.randn(2, 3, 3, 3, dtype=torch.float64, generator=g).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: _folded(x, v), (w,))
    # and the same gradient as through the composition
    r = torch.randn(2, 2, 6, 10, dtype=torch.float64, generator=g)
    ga, = torch.autograd.grad((_folded(x, w) * r).sum(), w)
    gb, = torch.autograd.grad((_up2_composition(x, w) * r).sum(), w)
    assert (ga - gb).abs().max().item() <= 1e-12 * gb.abs().max().item()


GOLDEN_CONFIGS = {
    'K1_comod64': dict(z_dim=32, c_dim=0, w_dim=32, img_resolution=64, img_channels_in=1, img_channels_out=1, mapping_kwargs=dict(num_layers=2),
                       synthesis_kwargs=dict(channel_base=512, channel_max=16, cond_mod=True, skip_resolution=64)),
    'K2_comod128': dict(z_dim=32, c_dim=1, w_dim=32, img_resolution=128, img_channels_in=4, img_channels_out=1, mapping_kwargs=dict(num_layers=2),
                        synthesis_kwargs=dict(channel_base=1024, channel_max=12, conv_clamp=256, skip_resolution=32)),
    'K3_comod32': dict(z_dim=32, c_dim=2, w_dim=32, img_resolution=32, img_channels_in=2, img_channels_out=1, mapping_kwargs=dict(num_layers=2),
                       synthesis_kwargs=dict(channel_base=256, channel_max=8, cond_mod=False, conv_clamp=2, skip_resolution=8)),
}


@pytest.mark.parametrize('name', sorted(GOLDEN_CONFIGS))
def test_state_dict_keys_are_the_reference_s(name):
    g = np.load(os.path.join(GOLDEN, name + '.npz'))
    G = nc.CoModGenerator(**GOLDEN_CONFIGS[name])
    keys = list(G.state_dict().keys())
    assert keys == [str(k) for k in g['keys']]
    for k, v in G.state_dict().items():
        assert tuple(v.shape) == g['sd/' + k].shape, k
    assert any(k.endswith('noise_const') for k in keys) and any(k.endswith('noise_strength') for k in keys) and any(k.endswith('resample_filter') for k in keys)
    G.load_state_dict({k: torch.from_numpy(np.array(g['sd/' + k])) for k in keys}, strict=True)


def _gen(**over):
    kw = dict(GOLDEN_CONFIGS['K1_comod64'])
    kw['synthesis_kwargs'] = dict(kw['synthesis_kwargs'])
    kw['mapping_kwargs'] = dict(kw['mapping_kwargs'])
    for k, v in over.items():
        where, key = k.split('__')
        kw[where + '_kwargs'][key] = v
    return nc.CoModGenerator(**kw)


@pytest.mark.parametrize('over', [dict(synthesis__num_fp16_res=1), dict(synthesis__channel_attention=True), dict(synthesis__architecture='orig'),
                                  dict(synthesis__architecture='resnet'), dict(mapping__name='RefMappingNetwork'),
                                  dict(synthesis__name='CASynthesisNetwork')])
def test_refusals_at_construction(over):
    with pytest.raises(NotImplementedError):
        _gen(**over)


def test_names_of_the_supported_classes_are_accepted_and_shared_encoder_is_refused():
    G = _gen(mapping__name='MappingNetwork', synthesis__name='SynthesisNetwork')
    assert G.synthesis.compute_dtype == torch.float32
    z, x = torch.zeros(2, 32), torch.zeros(2, 1, 64, 64)
    with pytest.raises(NotImplementedError, match='cond_groups'):
        G(z, None, x, cond_groups=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match='encode'):
        G.synthesis.encode(x)
    with pytest.raises(NotImplementedError, match='decode'):
        G.synthesis.decode(None, None)
