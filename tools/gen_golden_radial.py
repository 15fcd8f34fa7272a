#!/usr/bin/env python3
"""Generate the radial-filter (StyleGAN3-R) golden vectors R1..R4 from the *actual* reference.

Run ONLY where the reference is available (see tools/gen_golden.py for the import route):

    python tools/gen_golden_radial.py     # writes tests/golden/R*.npz

The prefix R keeps these fixtures out of the tests that collect every F / U / B / M fixture.  Data only: inputs, filters,
outputs and gradients of ``sum(y * r)`` for a fixed random ``r``; every case seeds its own generator, so a rerun reproduces the
committed arrays exactly.

  R1                  6t-ups4-downf2: up 4 (24 taps), radial 12 x 12 down filter, down 2, the F3 plane and crop padding
  R2 / R2b            an asymmetric random 12 x 12 up filter, up 2, separable 24-tap down filter, down 4, asymmetric padding;
                      flip_filter True / False (pins the orientation and the once-only gain of a 2-D up filter)
  R3_tiny128_radial   the G1 generator recipe (tools/gen_golden.py) with use_radial_filters=True
  R4_radial_filters256  the down filters of the radial layers of the full-width 256^2 generator, with the layer names
"""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import _import_reference, _np, save  # noqa: E402

TINY = dict(channel_base=256, channel_max=8, num_layers=14, num_critical=2, first_cutoff=2, first_stopband=2 ** 2.1,
            last_stopband_rel=2 ** 0.3, margin_size=10, output_scale=0.25, skip_resolution=128, conv_kernel=3, filter_size=6,
            lrelu_upsampling=2, use_radial_filters=True, conv_clamp=256, magnitude_ema_beta=0.5 ** (16 / 20e3), cond_mod=True)


def main():
    import torch
    net, flr, _, _, _ = _import_reference()
    design = net.SynthesisLayer.design_lowpass_filter

    def flrelu_case(name, seed, xshape, fu, fd, up, down, padding, gain=float(np.sqrt(2)), slope=0.2, clamp=256.0,
                    flip_filter=False):
        torch.manual_seed(seed)
        x = torch.randn(xshape).requires_grad_(True)
        b = (torch.randn(xshape[1]) * 0.5).requires_grad_(True)
        y = flr.filtered_lrelu(x, fu=fu, fd=fd, b=b, up=up, down=down, padding=padding, gain=gain, slope=slope,
                               clamp=clamp, flip_filter=flip_filter, impl='ref')
        r = torch.randn_like(y)
        dx, db = torch.autograd.grad((y * r).sum(), [x, b])
        save(name, x=_np(x), b=_np(b), fu=_np(fu), fd=_np(fd), y=_np(y), r=_np(r), dx=_np(dx), db=_np(db),
             meta=np.array([up, down] + list(padding), dtype=np.int64),
             fmeta=np.array([gain, slope, -1.0 if clamp is None else clamp, float(flip_filter)], dtype=np.float64))

    fu24 = design(numtaps=24, cutoff=20.0, width=2 * (64.0 - 20.0), fs=512)
    fd24 = design(numtaps=24, cutoff=20.0, width=2 * (64.0 - 20.0), fs=512)
    fr = design(numtaps=12, cutoff=56.0, width=2 * (160.0 - 56.0), fs=512, radial=True)
    flrelu_case('R1_ups4_radial_down', 101, [1, 2, 38, 38], fu24, fr, 4, 2, [-6, -9, -6, -9])
    torch.manual_seed(102)
    fa = torch.randn(12, 12)
    fa = fa / fa.abs().sum() * 4.0
    flrelu_case('R2_asym2d_up_flip', 103, [1, 2, 37, 41], fa, fd24, 2, 4, [33, 35, 31, 34], flip_filter=True)
    flrelu_case('R2b_asym2d_up_noflip', 103, [1, 2, 37, 41], fa, fd24, 2, 4, [33, 35, 31, 34], flip_filter=False)

    # ---------------------------------------------------------------- tiny radial generator (G1 recipe)
    torch.manual_seed(128)
    G = net.Stylegan3Generator(z_dim=32, c_dim=1, w_dim=32, img_resolution=128, img_channels_in=4, img_channels_out=1,
                               mapping_kwargs=dict(num_layers=2), synthesis_kwargs=dict(TINY)).eval()
    # Deviations from the G1 recipe, to keep the file under 1 MiB: G1 does not round its parameters, here they are rounded to
    # bfloat16-representable values (still stored as float32; they compress to about half), and the input / cotangent are stored in
    # the 8-bit encodings of conftest.load_golden (x_u8, r_i8).  Everything else is G1's recipe with use_radial_filters=True.
    with torch.no_grad():
        for n, p in G.named_parameters():
            if n.endswith('.bias') and 'affine' not in n:
                p.add_(torch.randn_like(p) * 0.1)
            p.copy_(p.bfloat16().float())
    batch = 2
    z = torch.randn(batch, 32); c = torch.rand(batch, 1)
    x_u8 = ((torch.randn(batch, 4, 128, 128).clamp(-1, 1) + 1) * 127.5).round().to(torch.uint8)
    xin = x_u8.float() * np.float32(2.0 / 255.0) - np.float32(1.0)
    feats, hooks = {}, []
    for lname, mod in G.synthesis.named_children():
        if hasattr(mod, 'up_factor'):
            hooks.append(mod.register_forward_hook(lambda m, i, o, lname=lname: feats.__setitem__(lname, o.detach())))
    y = G(z, c, xin)
    for h in hooks:
        h.remove()
    r_i8 = torch.randint(-3, 4, y.shape, dtype=torch.int8)
    r = r_i8.float()
    pnames = [n for n, _ in G.named_parameters()]
    allg = torch.autograd.grad((y * r).sum(), list(G.parameters()), allow_unused=True)
    gd = {n: g for n, g in zip(pnames, allg) if g is not None}
    arrays = {'sd/' + k: _np(v) for k, v in G.state_dict().items()}
    arrays.update(z=_np(z), c=_np(c), x_u8=_np(x_u8), y=_np(y), r_i8=_np(r_i8))
    arrays.update({'stat/' + k: np.array([v.mean().item(), v.std().item(), v.abs().max().item()]) for k, v in feats.items()})
    for pat in [r'synthesis\.encoder_0\.weight', r'synthesis\.encoder_12\.bias', r'synthesis\.L3_52_8\.weight',
                r'synthesis\.L13_128_2\.bias', r'mapping\.fc0\.weight']:
        for k in gd:
            if re.fullmatch(pat, k):
                arrays['grad/' + k] = _np(gd[k])
    arrays['gradnorm_names'] = np.array(sorted(gd.keys()))
    arrays['gradnorm'] = np.array([gd[k].norm().item() for k in sorted(gd.keys())])
    arrays['layer_names'] = np.array(list(feats.keys()))
    save('R3_tiny128_radial', **arrays)

    # ---------------------------------------------------------------- radial down filters of the full-width 256^2 generator
    torch.manual_seed(0)
    full = dict(TINY, channel_base=16384, channel_max=512)
    Gfull = net.Stylegan3Generator(z_dim=512, c_dim=1, w_dim=512, img_resolution=256, img_channels_in=4, img_channels_out=1,
                                   mapping_kwargs=dict(num_layers=8), synthesis_kwargs=full)
    names, filters = [], []
    for lname, mod in Gfull.synthesis.named_children():
        f = getattr(mod, 'down_filter', None)
        if f is not None and f.ndim == 2:
            names.append(lname)
            filters.append(_np(f))
    save('R4_radial_filters256', names=np.array(names), filters=np.stack(filters))


if __name__ == '__main__':
    main()
