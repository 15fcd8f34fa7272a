"""Generators with other hyperparameters than the shipped ones, against the CPU oracle run in float64 on the same random state dict
(oracle.generator.random_state_dict).  Each configuration moves at least one dispatch gate of the generator's small kernels:

  w_dim 36         K = 36 + 1024 = 1060, no multiple of 16: the style FCs run per layer (affine_bank.supported), and the mapping FCs
                   (cout 36) take the GEMM composition (fc_bank.supported)
  w_dim 48, c 0    no embedding: mapping_input without labels
  w_dim 528        K = 1552 > 1536: the style FCs run per layer
  z_dim 20         the first mapping FC has cin = 52: GEMM composition
  cond_mod False   no global vector: every layer modulates on its own latent (the per-layer modulation path)
  margin_size 11   the 16^2 stage's planes are 38 wide: _pool4 takes AdaptiveAvgPool2d, filtered_lrelu runs off its 16m + 4 widths
  channel_max 24   conv Cout and fc_in's cin = 384 no multiples of 64

fp32: forward within 5e-5 of the output scale (the golden generators' tight bar), every parameter gradient within relative L2 1e-2 (the
end-to-end bar, against the oracle on the kernels' branch decisions).  bf16 / f16 on the same weights: PSNR against the float64 oracle at
least that of the default tiny configuration in the same session, minus 7 dB.  Measured on the MI355X (dB, bf16 / f16), default tiny
configuration first:
  default 58.0 / 75.3   w36 53.3 / 71.5   w48_c0 55.2 / 77.2   w528 53.8 / 72.3   z20 58.4 / 74.8   nocond 56.4 / 78.1
  margin11 58.0 / 75.3   cmax24 52.7 / 69.3
The spread is that of the random draws, not of the kernels: w36 and the default differ only in the width of the style FCs' input (the
modulation kernels are bit-identical on both paths, test_modulation_bank_is_bit_identical_to_the_layers_one_by_one), yet 4.7 dB apart
in bf16; cmax24 accumulates three times the channels.  Hence 7 dB, not the 3 dB first proposed, which the default's own neighbours miss."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TINY = dict(channel_base=256, channel_max=8, num_layers=14, num_critical=2, margin_size=10, output_scale=0.25, skip_resolution=128,
            conv_kernel=3, filter_size=6, lrelu_upsampling=2, use_radial_filters=False, conv_clamp=256,
            magnitude_ema_beta=0.5 ** (16 / 20e3), cond_mod=True)

# name: (z_dim, c_dim, w_dim, synthesis overrides)
CONFIGS = {
    'default': (32, 1, 32, {}),
    'w36': (32, 1, 36, {}),
    'w48_c0': (32, 0, 48, {}),
    'w528': (32, 1, 528, {}),
    'z20': (20, 1, 32, {}),
    'nocond': (32, 1, 32, dict(cond_mod=False)),
    'margin11': (32, 1, 32, dict(margin_size=11)),
    'cmax24': (32, 1, 32, dict(channel_max=24)),
}


def _setup(name, batch, seed=0):
    from afcm_amd.networks_stylegan3 import Stylegan3Generator
    from oracle import generator as ogen
    z_dim, c_dim, w_dim, over = CONFIGS[name]
    skw = dict(TINY, **over)
    pl = ogen.plan(128, 4, 1, {k: v for k, v in skw.items() if k not in ('use_radial_filters', 'magnitude_ema_beta')})
    sd = ogen.random_state_dict(pl, z_dim, c_dim, w_dim, 2, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    z = torch.randn(batch, z_dim, generator=g)
    c = torch.rand(batch, c_dim, generator=g) if c_dim else None
    x = torch.randn(batch, 4, 128, 128, generator=g)
    r = torch.randn(batch, 1, 128, 128, generator=g)

    def make(dtype):
        G = Stylegan3Generator(z_dim=z_dim, c_dim=c_dim, w_dim=w_dim, img_resolution=128, img_channels_in=4, img_channels_out=1,
                               mapping_kwargs=dict(num_layers=2), synthesis_kwargs=dict(skw, compute_dtype=dtype)).eval()
        missing, unexpected = G.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.endswith('_filter') for k in missing), (missing, unexpected)   # (the resampling filters are the module's own)
        return G.cuda()
    return pl, sd, (z, c, x, r), make


def _oracle(pl, sd, inputs, names, grads=True, codes=None):
    from oracle import generator as ogen
    z, c, x, r = inputs
    osd = {k: v.double() for k, v in sd.items()}
    for k in names:
        osd[k].requires_grad_(grads)
    y = ogen.generator(osd, pl, z.double(), None if c is None else c.double(), x.double(), mapping_layers=2, codes=codes)
    if not grads:
        return y.detach(), None
    return y.detach(), torch.autograd.grad((y * r.double()).sum(), [osd[k] for k in names], allow_unused=True)


def _psnr(y, ref):
    y, ref = y.double().cpu(), ref.double().cpu()
    return 10 * np.log10(float((ref.max() - ref.min()) ** 2) / max(1e-30, float(((y - ref) ** 2).mean())))


_SESSION = {}


def _psnr_16bit(name, batch=2):
    """(bf16 PSNR, f16 PSNR) of configuration `name` against its float64 oracle; cached for the session (the default is the yardstick)."""
    key = (name, batch)
    if key not in _SESSION:
        pl, sd, inputs, make = _setup(name, batch)
        want, _ = _oracle(pl, sd, inputs, [], grads=False)
        z, c, x, _ = inputs
        out = []
        for dtype in (torch.bfloat16, torch.float16):
            with torch.no_grad():
                y = make(dtype)(z.cuda(), None if c is None else c.cuda(), x.cuda()).float()
            assert torch.isfinite(y).all(), (name, dtype)
            out.append(_psnr(y, want))
        _SESSION[key] = tuple(out)
        print(f'{name}: bf16 {out[0]:.1f} dB, f16 {out[1]:.1f} dB vs the float64 oracle')
    return _SESSION[key]


@pytest.mark.parametrize('name,batch', [('w36', 2), ('w36', 1), ('w36', 17), ('w48_c0', 2), ('w528', 2), ('z20', 2), ('nocond', 2),
                                        ('margin11', 2), ('cmax24', 2)])
def test_fp32_generator_config_vs_float64_oracle(name, batch, monkeypatch):
    """The gradients are compared with the oracle run on the kernels' own leaky-ReLU branch decisions (as in
    test_generator_gradients_with_the_kernels_branch_decisions_imposed): without that, a pre-activation within rounding distance of the
    kink takes the other branch, and the bias gradient of encoder_0 -- a sum over whole planes of a random cotangent, mostly cancelling --
    moves by 1-5 % relative L2 (measured) on one such flip."""
    from afcm_amd.torch_utils.ops import filtered_lrelu as flr
    pl, sd, inputs, make = _setup(name, batch)
    G = make(torch.float32)
    names = [k for k, _ in G.named_parameters()]
    written = []
    run = flr._run

    def recording_run(x, fu, fd, b, si, cfg, write_signs, *a, **k):
        out = run(x, fu, fd, b, si, cfg, write_signs, *a, **k)
        if write_signs:
            assert out[2] == 0                                     # fp32: the reference's row-major 2-bit packing
            written.append(out[1])
        return out
    monkeypatch.setattr(flr, '_run', recording_run)
    z, c, x, r = inputs
    y = G(z.cuda(), None if c is None else c.cuda(), x.cuda())
    ggot = torch.autograd.grad((y * r.cuda()).sum(), list(G.parameters()), allow_unused=True)
    layers = [L['name'] for L in pl['enc'] + pl['dec']]
    assert len(written) == len(layers)
    codes = {}
    for lname, sg in zip(layers, written):
        sg = sg.cpu().numpy()
        codes[lname] = torch.from_numpy(np.stack([(sg >> (2 * k)) & 3 for k in range(4)], axis=-1).reshape(*sg.shape[:3], sg.shape[3] * 4))
    want, gref = _oracle(pl, sd, inputs, names, codes=codes)
    err = float((y.detach().cpu().double() - want).abs().max())
    scale = float(want.abs().max())
    print(f'{name} batch {batch}: fp32 forward max-abs {err:.2e} (output scale {scale:.3g})')
    assert err <= 5e-5 * max(1.0, scale), f'{name}: forward max-abs {err:.3e}'
    for k, a, b in zip(names, ggot, gref):
        assert (a is None) == (b is None), k
        if b is None:
            continue
        d = a.cpu().double() - b
        # (floor: a gradient that is analytically zero -- the styles of a demodulated one-input-channel layer -- is rounding noise here)
        ref = max(float(b.norm()), 1e-6 * float(np.sqrt(b.numel())))
        assert float(d.norm()) <= 1e-2 * ref, f'{name} grad {k}: relative L2 {float(d.norm()) / ref:.3e}'


@pytest.mark.parametrize('name', ['w36', 'w48_c0', 'w528', 'z20', 'nocond', 'margin11', 'cmax24'])
def test_16bit_generator_config_vs_float64_oracle(name):
    base = _psnr_16bit('default')
    got = _psnr_16bit(name)
    for dtype, p, p0 in zip(('bf16', 'f16'), got, base):
        assert p >= p0 - 7.0, f'{name} {dtype}: {p:.1f} dB vs the oracle, the default tiny configuration {p0:.1f} dB'


def test_second_backward_is_identical_or_refused():
    """Two backward passes over one bf16 generator graph (retain_graph): the second gives the first's parameter gradients or raises
    RuntimeError -- never different gradients.  (The encoder's skip fork hands a style factor from the decoder's forward to its own
    backward once: fused_layer._SkipFork.)"""
    pl, sd, inputs, make = _setup('default', 2)
    G = make(torch.bfloat16)
    z, c, x, r = inputs
    y = G(z.cuda(), c.cuda(), x.cuda())
    loss = (y.float() * r.cuda()).sum()
    params = list(G.parameters())
    first = torch.autograd.grad(loss, params, retain_graph=True, allow_unused=True)
    try:
        second = torch.autograd.grad(loss, params, allow_unused=True)
    except RuntimeError as e:
        assert 'backward' in str(e), e
        return
    for (k, _), a, b in zip(G.named_parameters(), first, second):
        assert (a is None) == (b is None), k
        assert a is None or torch.equal(a, b), f'{k}: second backward differs by {float((a - b).abs().max()):.3e}'
