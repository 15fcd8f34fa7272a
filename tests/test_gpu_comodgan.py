"""The CoModGAN generator (afcm_amd/networks_comodgan.py) on the GPU: against the reference's own outputs and gradients (tests/golden/K1, K2:
tools/gen_golden_comodgan.py) under the bounds tests/test_gpu_generator.py applies to the fp32 stylegan3 generator, the fused arm against the
unfused one (also under the float64-oracle criterion of tests/comodgan_ref.py), the noise modes, and the generator inside the package's training step, captured graph, validation and volume loops.

Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

CONFIGS = {
    'K1_comod64': dict(z_dim=32, c_dim=0, w_dim=32, img_resolution=64, img_channels_in=1, img_channels_out=1, mapping_kwargs=dict(num_layers=2),
                       synthesis_kwargs=dict(channel_base=512, channel_max=16, cond_mod=True, skip_resolution=64, dropout_rate=0)),
    'K2_comod128': dict(z_dim=32, c_dim=1, w_dim=32, img_resolution=128, img_channels_in=4, img_channels_out=1, mapping_kwargs=dict(num_layers=2),
                        synthesis_kwargs=dict(channel_base=1024, channel_max=12, conv_clamp=256, skip_resolution=32, dropout_rate=0)),
    'K3_comod32': dict(z_dim=32, c_dim=2, w_dim=32, img_resolution=32, img_channels_in=2, img_channels_out=1, mapping_kwargs=dict(num_layers=2),
                       synthesis_kwargs=dict(channel_base=256, channel_max=8, cond_mod=False, conv_clamp=2, skip_resolution=8, dropout_rate=0)),
}
_CACHE = {}


def _golden(name):
    if name not in _CACHE:
        g = load_golden(name)
        sd = {k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith('sd/')}
        ins = {k: torch.from_numpy(g[k].astype(np.float32)).cuda() for k in ('z', 'cond_img', 'r')}
        ins['c'] = torch.from_numpy(g['c'].astype(np.float32)).cuda() if 'c' in g else None
        _CACHE[name] = (g, sd, ins)
    return _CACHE[name]


def _build(name, **over):
    from afcm_amd.networks_comodgan import CoModGenerator
    kw = dict(CONFIGS[name])
    kw['synthesis_kwargs'] = dict(kw['synthesis_kwargs'], **over)
    G = CoModGenerator(**kw)
    own = G.state_dict()
    G.load_state_dict({k: v for k, v in _golden(name)[1].items() if k in own or not over}, strict=True)      # (use_noise=False has no noise entries)
    return G.cuda()


def _forward_backward(G, ins, **kw):
    y = G(ins['z'], ins['c'], ins['cond_img'], noise_mode='const', **kw)
    params = dict(G.named_parameters())
    names = sorted(params)
    grads = torch.autograd.grad((y * ins['r']).sum(), [params[k] for k in names])
    return y.detach(), dict(zip(names, grads))


def _grad_bounds(name, got, want):
    worst = [0.0, 0.0, 0.0, '']
    for k, w in want.items():
        w = np.asarray(w, dtype=np.float64)
        d = got[k].detach().cpu().numpy().astype(np.float64) - w
        rel_l2 = float(np.sqrt((d ** 2).sum()) / max(1e-30, np.sqrt((w ** 2).sum())))
        e = float(np.abs(d).max())
        nw, ng = float(np.sqrt((w ** 2).sum())), float(np.sqrt((got[k].detach().cpu().numpy().astype(np.float64) ** 2).sum()))
        if rel_l2 > worst[0]:
            worst = [rel_l2, e, abs(ng - nw), k]
        assert rel_l2 <= 1e-2, f'{name} grad {k}: relative L2 error {rel_l2:.3e}'
        assert e <= 2e-2 * max(1.0, float(np.abs(w).max())), f'{name} grad {k}: max-abs {e:.3e}'
        assert abs(ng - nw) <= 5e-3 * max(1.0, nw), f'{name} grad {k}: norm {ng} vs {nw}'
    print(f'{name}: worst gradient {worst[3]}: relative L2 {worst[0]:.3e}, max-abs {worst[1]:.3e}, norm difference {worst[2]:.3e}')


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_matches_reference_golden(name):
    g, _, ins = _golden(name)
    G = _build(name).eval()
    with torch.no_grad():
        y = G(ins['z'], ins['c'], ins['cond_img'], noise_mode='const')
    scale = max(1.0, float(np.abs(g['y_eval']).max()))
    err = (y.cpu() - torch.from_numpy(g['y_eval'])).abs().max().item()
    print(f'{name}: eval forward max-abs {err:.3e} (scale {scale:.3f})')
    assert err <= 1e-3 and err <= 5e-5 * scale
    G.train()
    y, grads = _forward_backward(G, ins)
    err = (y.cpu() - torch.from_numpy(g['y_train'])).abs().max().item()
    print(f'{name}: train forward max-abs {err:.3e}')
    assert err <= 1e-3 and err <= 5e-5 * max(1.0, float(np.abs(g['y_train']).max()))
    assert sorted(grads) == [str(n) for n in g['names']]
    _grad_bounds(name, grads, {k: g['g/' + k] for k in grads})


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_fused_arm_equals_unfused_arm(name, monkeypatch):
    from afcm_amd import networks_comodgan as nc
    _, _, ins = _golden(name)
    G = _build(name).train()
    out = {}
    for impl in ('unfused', 'fused'):
        monkeypatch.setattr(nc, 'IMPL', impl)
        out[impl] = _forward_backward(G, ins)
    (yu, gu), (yf, gf) = out['unfused'], out['fused']
    scale = max(1.0, float(yu.abs().max()))
    err = float((yf - yu).abs().max())
    print(f'{name}: fused vs unfused forward max-abs {err:.3e} (scale {scale:.3f})')
    assert err <= 1e-5 * scale
    worst = max((float((gf[k] - gu[k]).double().norm() / gu[k].double().norm().clamp_min(1e-30)), k) for k in gu)
    print(f'{name}: fused vs unfused worst gradient relative L2 {worst[0]:.3e} ({worst[1]})')
    assert worst[0] <= 1e-2
    # the criterion of tests/comodgan_ref.py between the two arms: each arm's gradient against the other's, the yardstick Y from the float64
    # and float32 oracle on the golden's own state and inputs (nothing in it comes from either arm)
    import comodgan_ref as R
    bounds = R.golden_bounds(_golden(name)[0], CONFIGS[name])
    ratios = {k: max(R.err(gf[k], gu[k]), R.err(gu[k], gf[k])) / bounds[k] for k in gu}
    worst = max((v, k) for k, v in ratios.items())
    print(f'{name}: fused vs unfused worst gradient err / max(Y, median Y) {worst[0]:.3f} ({worst[1]}), MARGIN {R.MARGIN}')
    bad = {k: round(v, 3) for k, v in ratios.items() if not v <= R.MARGIN}
    assert not bad, bad


def test_noise_modes():
    _, _, ins = _golden('K1_comod64')
    G = _build('K1_comod64').eval()
    with torch.no_grad():
        none = G(ins['z'], ins['c'], ins['cond_img'], noise_mode='none')
        rand = G(ins['z'], ins['c'], ins['cond_img'], noise_mode='random')
        rand2 = G(ins['z'], ins['c'], ins['cond_img'], noise_mode='random')
        assert bool(torch.isfinite(none).all()) and bool(torch.isfinite(rand).all())
        assert not torch.equal(rand, rand2) and not torch.equal(rand, none)
        for k, p in G.named_parameters():
            if k.endswith('noise_strength'):
                p.zero_()
        assert torch.equal(G(ins['z'], ins['c'], ins['cond_img'], noise_mode='random'), none), 'random noise at strength 0 is no noise'
    G = _build('K1_comod64', use_noise=False).eval()
    with torch.no_grad():
        assert torch.equal(G(ins['z'], ins['c'], ins['cond_img'], noise_mode='random'), none)


def _step_nets(seed=0, **skw):
    from afcm_amd.networks_comodgan import CoModGenerator
    from afcm_amd.networks_discriminator import CoModDiscriminator
    torch.manual_seed(seed)
    G = CoModGenerator(z_dim=32, c_dim=0, w_dim=32, img_resolution=64, img_channels_in=1, img_channels_out=1, mapping_kwargs=dict(num_layers=2),
                       synthesis_kwargs=dict(channel_base=512, channel_max=16, cond_mod=True, skip_resolution=64, **skw)).cuda()
    D = CoModDiscriminator(c_dim=0, img_resolution=64, img_channels=2, channel_base=512, channel_max=16, epilogue_kwargs=dict(mbstd_group_size=2)).cuda()
    return G, D


def _step_inputs():
    gen = torch.Generator().manual_seed(4)
    real_A = torch.randn(2, 1, 64, 64, generator=gen).cuda()
    real_B = torch.tanh(torch.randn(2, 1, 64, 64, generator=gen)).cuda()
    return real_A, real_B, torch.randn(2, 32, generator=gen).cuda(), torch.zeros(2, 0).cuda()


def test_two_training_iterations_move_every_parameter():
    from afcm_amd.stylegan3_model import StyleGAN3Step
    G, D = _step_nets()
    step = StyleGAN3Step(netG=G, netD=D, blur_init_sigma=0)
    before = {k: p.detach().clone() for net in (G, D) for k, p in net.named_parameters()}
    for _ in range(2):
        step.set_input(*_step_inputs())
        step.optimize_parameters()
    for net in (G, D):
        for k, p in net.named_parameters():
            assert bool(torch.isfinite(p).all()) and not torch.equal(p, before[k]), k
    losses = {k: float(getattr(step, k).detach()) for k in ('loss_D_fake', 'loss_D_real', 'loss_Dr1', 'loss_G_GAN', 'loss_G_L1')}
    print(losses)
    assert all(np.isfinite(v) for v in losses.values())


def test_captured_step_replays_equal_eager_steps():
    """dropout_rate=0, use_noise=False, capturable=True: three warm-up steps and three replays of ``capture_step`` against six eager steps (a
    capture records the step without running it; tests/test_gpu_optim.py counts the same way).

    Under ``torch.backends.cudnn.deterministic = True``: the encoder's and the fp32 discriminator's convolutions are the framework's, whose default
    fp32 weight gradient adds with atomics -- measured on the MI355X without the flag, two EAGER runs of this step already differ from each other
    (34 of 112 parameters after one step, 88 after six, up to 2.4e-7; replays differ from eager by the same order, fused and unfused arm alike), so
    equal bits say nothing about the capture there.  With the flag eager equals eager and the replays equal eager, 0 of 112 parameters apart."""
    from afcm_amd.stylegan3_model import StyleGAN3Step, capture_step
    inputs = _step_inputs()
    finals = []
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        _captured_and_eager(StyleGAN3Step, capture_step, inputs, finals)
    finally:
        torch.backends.cudnn.deterministic = was
    differ = [(k, float((a - b).abs().max())) for (k, a), (_, b) in zip(*finals) if not torch.equal(a, b)]
    print(f'{len(differ)} of {len(finals[0])} parameters differ between replays and eager steps; largest difference '
          f'{max([d for _, d in differ], default=0.0):.3e}')
    assert not differ
    assert all(bool(torch.isfinite(p).all()) for _, p in finals[1])


def _captured_and_eager(StyleGAN3Step, capture_step, inputs, finals):
    for mode in ('eager', 'graph'):
        G, D = _step_nets(dropout_rate=0, use_noise=False)
        step = StyleGAN3Step(netG=G, netD=D, blur_init_sigma=0, capturable=True)
        if mode == 'eager':
            for _ in range(3 + 3):
                step.set_input(*inputs)
                step.optimize_parameters()
        else:
            graph = capture_step(step, inputs, warmup=3)
            for _ in range(3):
                graph.replay()
            torch.cuda.synchronize()
        assert step.optimizer_G.device_step() == 6
        finals.append([(k, p.detach().clone()) for net in (G, D) for k, p in net.named_parameters()])


def test_ema_copy_runs_the_evaluation_forward():
    from afcm_amd.stylegan3_model import StyleGAN3Step
    G, D = _step_nets()
    step = StyleGAN3Step(netG=G, netD=D, blur_init_sigma=0, ema=True)
    real_A, real_B, z, c = _step_inputs()
    step.set_input(real_A, real_B, z, c)
    with torch.no_grad():
        for p in G.parameters():                       # the live generator is no longer the EMA copy
            p.mul_(0.5)
    step.test()
    with torch.no_grad():
        want = step.netG_ema(z, c, real_A, noise_mode='const')
        other = G.eval()(z, c, real_A, noise_mode='const')
    assert step.fake_B.shape == (2, 1, 64, 64) and torch.equal(step.fake_B, want) and not torch.equal(step.fake_B, other)
    assert not step.netG_ema.training


def test_validation_and_volume_loops():
    from afcm_amd.networks_comodgan import CoModGenerator
    from afcm_amd.stylegan3_model import StyleGAN3GeneratorStep
    from afcm_amd.validation import validate
    from afcm_amd.volume import predict_volume
    G, _ = _step_nets()
    step = StyleGAN3GeneratorStep(G, ema=True)
    gen = torch.Generator().manual_seed(6)
    batches = [(torch.randn(2, 1, 64, 64, generator=gen), torch.rand(2, 1, 64, 64, generator=gen) * 2 - 1) for _ in range(2)]
    out = validate(step, batches, metrics='device')
    print(out)
    assert out['batches'] == 2 and np.isfinite(out['psnr']) and np.isfinite(out['ssim']) and np.isfinite(out['mae'])
    # one (5, 60, 68) uint8 subject: pad in y, crop in x; single-slice inputs, batches of 2, the last one of 1
    zz, yy, xx = np.meshgrid(np.linspace(-1, 1, 5), np.linspace(-1, 1, 60), np.linspace(-1, 1, 68), indexing='ij')
    src = np.round(np.clip(1.2 - (zz ** 2 * 0.3 + yy ** 2 + xx ** 2), 0, 1) * (0.6 + 0.4 * np.sin(7 * xx)) * 255).astype(np.uint8)
    kw = dict(raw_internal_path_in='raw', patch_hw=(64, 64), batch_size=2, patch_halo=(0, 8, 8))
    pred = predict_volume(step, {'raw': src}, thickness=None, slice_num=1, **kw)['prediction']
    assert pred.is_cuda and pred.shape == (1, 5, 64, 64) and bool(torch.isfinite(pred).all())
    # four-slice inputs with a label: the unshared loop runs, the shared-encoder loop is refused by the generator
    torch.manual_seed(1)
    G4 = CoModGenerator(z_dim=32, c_dim=1, w_dim=32, img_resolution=64, img_channels_in=4, img_channels_out=1, mapping_kwargs=dict(num_layers=2),
                        synthesis_kwargs=dict(channel_base=512, channel_max=16, skip_resolution=64)).cuda()
    step4 = StyleGAN3GeneratorStep(G4, ema=True)
    pred = predict_volume(step4, {'raw': src}, thickness=2, slice_num=4, **kw)['prediction']
    assert pred.shape == (1, 5, 64, 64) and bool(torch.isfinite(pred).all())
    with pytest.raises(NotImplementedError, match='cond_groups'):
        predict_volume(step4, {'raw': src}, thickness=2, slice_num=4, share_encoder=True, **kw)
