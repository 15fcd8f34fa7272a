"""afcm_amd.validation.validate on the GPU: the device arm (statistics kernel per batch, one copy at the end) against the host arm (the
reference's way: copy, ``to_unit_range``, ``evaluation.evaluate_2D``), on a stub step and once on the tiny 128^2 EMA generator.

Tolerances are those of tests/test_plane_metrics_cpu.py: 1e-9 dB PSNR, 1e-10 SSIM, 2e-6 relative MAE.  The host arm divides by the maxima
in float32 (psnr_2D on float32 arrays: numpy keeps the dtype) where the table divides in float64 -- one rounding of 2^-24 per element that only
a maximum equal to a power of two avoids.  Figures are printed before they are asserted.  Measured on an MI355X: stub step (targets saturate at 1,
predictions clip to 1: exact quotients) PSNR 0.0 dB / SSIM 4.4e-16 / MAE 8.4e-9 relative apart; tiny generator (prediction maximum below 1) PSNR
5.6e-10 dB / SSIM 1.2e-15 / MAE 4.5e-8 apart.  At the full-width 256^2 generator the same difference is 2.2e-9 dB, above the 1e-9 dB asked of the
loop (tools/bench_validation.py, DESIGN section 8f: the host arm on float64 copies reproduces the device arm's PSNR to the last bit)."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

TOL_PSNR_DB, TOL_SSIM, TOL_MAE_REL = 1e-9, 1e-10, 2e-6


def _agree(dev, host):
    print('device', dev)
    print('host  ', host)
    print(f"differences: psnr {abs(dev['psnr'] - host['psnr']):.3e} dB, ssim {abs(dev['ssim'] - host['ssim']):.3e}, "
          f"mae {abs(dev['mae'] - host['mae']) / host['mae']:.3e} relative")
    assert dev['batches'] == host['batches'] and dev['batches_counted'] == host['batches_counted']
    assert abs(dev['psnr'] - host['psnr']) <= TOL_PSNR_DB
    assert abs(dev['ssim'] - host['ssim']) <= TOL_SSIM
    assert abs(dev['mae'] - host['mae']) <= TOL_MAE_REL * host['mae']


class StubStep:
    """``test()`` writes a seeded prediction in network range: the target + N(0, 0.1), unclipped (the metrics clip)."""

    def set_input(self, real_A, real_B):
        self.real_A, self.real_B = real_A.cuda(), real_B.cuda()
        self.fake_B = None

    def test(self):
        gen = torch.Generator(device='cuda').manual_seed(int(self.real_A.flatten()[0].item()))
        self.fake_B = self.real_B + 0.1 * torch.randn(self.real_B.shape, generator=gen, device='cuda')


def _stub_batches():
    gen = torch.Generator().manual_seed(5)
    batches = []
    for b in range(3):
        real_B = (torch.rand(4, 1, 32, 48, generator=gen) * 2.4 - 1.2).clamp(-1, 1)     # saturates at both ends, as normalised slices do
        if b == 1:
            real_B[:] = -1.0                               # an all-empty batch: maps to 0 everywhere
        if b == 2:
            real_B[1] = -1.0                               # one empty slice inside a counted batch
        batches.append((torch.full((4, 1, 32, 48), float(b + 1)), real_B))
    return batches


def test_device_arm_equals_host_arm_on_a_stub_step():
    from afcm_amd.validation import validate
    batches = _stub_batches()
    host = validate(StubStep(), batches, metrics='host')
    dev = validate(StubStep(), batches, metrics='device')
    assert dev['batches'] == 3 and dev['batches_counted'] == 2
    _agree(dev, host)


def test_device_arm_copies_to_the_host_once(monkeypatch):
    from afcm_amd.validation import validate
    batches = [(a.cuda(), b.cuda()) for a, b in _stub_batches()]
    copies = []
    cpu, to, numpy, item, tolist = torch.Tensor.cpu, torch.Tensor.to, torch.Tensor.numpy, torch.Tensor.item, torch.Tensor.tolist

    def counted_cpu(self, *a, **k):
        if self.is_cuda:
            copies.append(('cpu', tuple(self.shape)))
        return cpu(self, *a, **k)

    def counted_to(self, *a, **k):
        out = to(self, *a, **k)
        if self.is_cuda and not out.is_cuda:
            copies.append(('to', tuple(self.shape)))
        return out

    def no_scalar_reads(name, fn):
        def wrapped(self, *a, **k):
            if self.is_cuda:
                copies.append((name, tuple(self.shape)))
            return fn(self, *a, **k)
        return wrapped

    class QuietStub(StubStep):
        def test(self):                                    # (the stub's own seed read is not the loop's)
            self.fake_B = self.real_B * 0.9
    monkeypatch.setattr(torch.Tensor, 'cpu', counted_cpu)
    monkeypatch.setattr(torch.Tensor, 'to', counted_to)
    monkeypatch.setattr(torch.Tensor, 'item', no_scalar_reads('item', item))
    monkeypatch.setattr(torch.Tensor, 'tolist', no_scalar_reads('tolist', tolist))
    out = validate(QuietStub(), batches, metrics='device')
    monkeypatch.undo()
    assert out['batches'] == 3 and out['batches_counted'] == 2
    assert copies == [('cpu', (12, 8))], copies           # the three batches' tables, together, once
    copies.clear()
    monkeypatch.setattr(torch.Tensor, 'cpu', counted_cpu)
    validate(QuietStub(), batches, metrics='host')
    monkeypatch.undo()
    assert len(copies) == 6, copies                       # the comparison arm: two images per batch


def test_arms_agree_on_the_tiny_ema_generator():
    """The 128^2 generator of tests/golden/G1_tiny128.npz as ``smoke()`` builds it, as the EMA copy of a step; two batches of 2."""
    from afcm_amd.networks_stylegan3 import Stylegan3Generator
    from afcm_amd.stylegan3_model import StyleGAN3GeneratorStep
    from afcm_amd.validation import validate
    tiny = dict(channel_base=256, channel_max=8, num_layers=14, num_critical=2, margin_size=10, output_scale=0.25, skip_resolution=128,
                conv_kernel=3, filter_size=6, lrelu_upsampling=2, use_radial_filters=False, conv_clamp=256,
                magnitude_ema_beta=0.5 ** (16 / 20e3), cond_mod=True)
    g = load_golden('G1_tiny128')
    G = Stylegan3Generator(z_dim=32, c_dim=1, w_dim=32, img_resolution=128, img_channels_in=4, img_channels_out=1,
                           mapping_kwargs=dict(num_layers=2), synthesis_kwargs=dict(tiny, compute_dtype=torch.float32)).eval()
    G.load_state_dict({k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith('sd/')}, strict=True)
    step = StyleGAN3GeneratorStep(G.cuda(), ema=True)
    x, y = torch.from_numpy(g['x']), torch.from_numpy(g['y'])
    gen = torch.Generator().manual_seed(9)
    # targets: the golden output pushed to the full network range, and a second batch made of the flipped slices
    target = (y / y.abs().max() * 1.1 + 0.05 * torch.randn(y.shape, generator=gen)).clamp(-1, 1)
    batches = [(x, target), (x.flip(0), target.flip(0).flip(-1))]
    torch.manual_seed(3)                                   # set_input draws gen_z: the same draws for both arms
    host = validate(step, batches, metrics='host')
    torch.manual_seed(3)
    dev = validate(step, batches, metrics='device')
    assert dev['batches'] == dev['batches_counted'] == 2
    assert step.fake_B.shape == (2, 1, 128, 128)
    _agree(dev, host)
