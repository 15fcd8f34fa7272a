#!/usr/bin/env python3
"""Golden vectors for the CoModGAN generator (afcm_amd/networks_comodgan.py), captured on the CPU from the *actual* reference
``CoModGenerator`` (models/networks/CoModGAN/generator.py:545-572 with the layers of layers.py:214-450).

Run ONLY where the reference checkout is mounted:   python tools/gen_golden_comodgan.py [K1_comod64 | K2_comod128 | K3_comod32]
Same import recipe as tools/gen_golden_disc.py.  Fixtures are data only: the state dict and its ordered key list, the inputs, the
``eval()`` forward with noise_mode='const' (the reference's grouped-conv arithmetic), and a ``train()`` forward (its unfused arithmetic;
dropout_rate=0, noise_mode='const') with every parameter gradient of (y * r).sum().  Inputs are drawn, rounded to multiples of 1/16 and stored
as float16 (exact; they compress to about a byte each): each file stays below 1 MiB.

K3 (conv_clamp=2, batch 3, skips at 4^2 and 8^2 only) is the configuration whose clamps bite: the script prints the share of each
SynthesisLayer's outputs that sit on the clamp in the ``train()`` forward.  As generated: block_early.conv1 0.52 %, b8.conv0 0.07 %,
b8.conv1 10.29 %, b16.conv0 4.04 %, b16.conv1 3.52 %, b32.conv0 4.15 %, b32.conv1 7.43 % -- five layers between 1 % and 30 %.
"""
import os
import sys
import types

import numpy as np

REF = '/root/reference'
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden')

CONFIGS = [
    # (name, resolution, c_dim, img_channels_in, batch, synthesis kwargs)
    ('K1_comod64', 64, 0, 1, 2, dict(channel_base=512, channel_max=16, cond_mod=True, skip_resolution=64)),
    ('K2_comod128', 128, 1, 4, 2, dict(channel_base=1024, channel_max=12, conv_clamp=256, skip_resolution=32)),
    ('K3_comod32', 32, 2, 2, 3, dict(channel_base=256, channel_max=8, cond_mod=False, conv_clamp=2, skip_resolution=8)),
]


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    pkg = types.ModuleType('models')
    pkg.__path__ = [os.path.join(REF, 'models')]
    sys.modules['models'] = pkg
    import torch
    from models.networks.CoModGAN.generator import CoModGenerator

    only = sys.argv[1:]
    from models.networks.CoModGAN.layers import SynthesisLayer
    for name, res, c_dim, ch_in, n, skw in CONFIGS:
        if only and name not in only:
            continue
        torch.manual_seed(78)
        G = CoModGenerator(z_dim=32, c_dim=c_dim, w_dim=32, img_resolution=res, img_channels_in=ch_in, img_channels_out=1,
                           mapping_kwargs=dict(name='MappingNetwork', num_layers=2),
                           synthesis_kwargs=dict(name='SynthesisNetwork', dropout_rate=0, **skw))
        with torch.no_grad():
            for k, p in G.named_parameters():              # biases and noise strengths start at 0: make every term of the arithmetic count
                if p.ndim == 1 or k.endswith('noise_strength'):
                    p.add_(torch.randn_like(p) * 0.1)
        half = lambda t: ((t * 16).round() / 16).to(torch.float16)      # noqa: E731  (multiples of 1/16: exact in float16, and they compress)
        z = half(torch.randn(n, 32))
        c = half(torch.rand(n, c_dim)) if c_dim > 0 else None
        x = half(torch.randn(n, ch_in, res, res))
        r = half(torch.randn(n, 1, res, res))
        out = {'sd/' + k: v.detach().numpy() for k, v in G.state_dict().items()}
        out['keys'] = np.array(list(G.state_dict().keys()))
        out['z'], out['cond_img'], out['r'] = z.numpy(), x.numpy(), r.numpy()
        if c is not None:
            out['c'] = c.numpy()
        cf = None if c is None else c.float()
        G.eval()
        with torch.no_grad():
            out['y_eval'] = G(z.float(), cf, x.float(), noise_mode='const').numpy()
        G.train()
        shares = {}
        hooks = []
        if skw.get('conv_clamp') is not None:              # the share of each SynthesisLayer's outputs that sit on the clamp (gain 1 in this architecture)
            for lname, mod in G.named_modules():
                if isinstance(mod, SynthesisLayer):
                    hooks.append(mod.register_forward_hook(
                        lambda m, i, o, lname=lname: shares.__setitem__(lname, float((o.detach().abs() >= m.conv_clamp).float().mean()))))
        y = G(z.float(), cf, x.float(), noise_mode='const')
        for h in hooks:
            h.remove()
        for lname, share in shares.items():
            print(f'{name}: clamped share {lname}: {100 * share:.2f} %')
        if shares:
            print(f'{name}: SynthesisLayers with a clamped share between 1 % and 30 %:', sum(0.01 <= v <= 0.30 for v in shares.values()))
        params = dict(G.named_parameters())
        names = sorted(params)
        grads = torch.autograd.grad((y * r.float()).sum(), [params[k] for k in names])
        out['y_train'] = y.detach().numpy()
        for k, g in zip(names, grads):
            out['g/' + k] = g.numpy()
        out['names'] = np.array(names)
        out['meta'] = np.array([res, n, c_dim, ch_in, skw['channel_base'], skw['channel_max'], int(skw.get('conv_clamp') or -1),
                                skw['skip_resolution'], int(bool(skw.get('cond_mod', False)))], dtype=np.int64)
        path = os.path.join(OUT, name + '.npz')
        np.savez_compressed(path, **out)
        print(name, os.path.getsize(path) // 1024, 'KiB', 'params', sum(p.numel() for p in G.parameters()),
              'eval-vs-train max-abs', float(np.abs(out['y_eval'] - out['y_train']).max()), '|y|max', float(np.abs(out['y_train']).max()))


if __name__ == '__main__':
    main()
