"""Whole-volume inference on the GPU: ``afcm_halo_accumulate`` against ``SlidingWindowPredictor`` on seeded random predictions, ``afcm_slice_assemble``
against stacked ``SliceDataset(phase='test')`` items, argument errors, and ``predict_volume`` / ``evaluate_volume`` with a stub step and with the tiny
128^2 EMA generator.  Equality is exact (``array_equal`` with ``equal_nan`` / equal bit patterns) everywhere except the metric values of the last test,
which carry the tolerances of tests/test_gpu_validation.py (1e-9 dB PSNR, 1e-10 SSIM, 2e-6 relative MAE, host functions on float64 copies as in
tests/test_gpu_plane_metrics.py).  The cases are those of tests/volume_ref.py, where the numpy restatement of the kernels is held to the same host code."""
import warnings

import numpy as np
import pytest
import torch

import volume_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

TOL_PSNR_DB, TOL_SSIM, TOL_MAE_REL = 1e-9, 1e-10, 2e-6


def _host_predict(volume_shape, idx, halo, batch, predictions, prediction_channel):
    from afcm_amd.predictor import SlidingWindowPredictor
    p = SlidingWindowPredictor(out_channels=predictions.shape[1], patch_halo=halo, prediction_channel=prediction_channel)
    prediction_map, mask = p.allocate(volume_shape)
    for i in range(0, len(idx), batch):
        p.accumulate(prediction_map, mask, predictions[i:i + batch], idx[i:i + batch], volume_shape)
    with warnings.catch_warnings(), np.errstate(divide='ignore', invalid='ignore'):
        warnings.simplefilter('ignore', RuntimeWarning)              # case (e): numpy's divide warning where the mask wrapped to 0
        return prediction_map / mask, prediction_map, mask


def _device_predict(volume_shape, patch_shape, stride_shape, halo, batch, batches, out_channels, prediction_channel):
    """``batches(first, count)`` -> the device tensor of that batch, in whatever form the test is about."""
    from afcm_amd.volume import DevicePredictor
    p = DevicePredictor(out_channels=out_channels, patch_halo=halo, prediction_channel=prediction_channel)
    p.allocate(volume_shape, 'cuda')
    plan = p.plan(patch_shape, stride_shape)
    for first in range(0, len(plan), batch):
        p.accumulate(batches(first, min(batch, len(plan) - first)), plan, first)
    return p.finish().cpu().numpy(), p.prediction_map.cpu().numpy(), p.normalization_mask.cpu().numpy()


@pytest.fixture(scope='module')
def host_cases():
    """{name: (predictions float32 numpy, (quotient, map, mask) of the host predictor)}, computed once."""
    from afcm_amd.predictor import patch_indices
    out = {}
    for name, (volume_shape, patch_shape, stride_shape, halo, batch, channels, pc) in R.ACCUMULATOR_CASES.items():
        idx = patch_indices(volume_shape, patch_shape, stride_shape)
        predictions = R.random_predictions(len(idx), channels, patch_shape, seed=11)
        out[name] = (predictions, _host_predict(volume_shape, idx, halo, batch, predictions, pc))
    return out


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert np.array_equal(g, w, equal_nan=True)


@pytest.mark.parametrize('name', sorted(R.ACCUMULATOR_CASES))
def test_accumulator_equals_the_host_predictor(name, host_cases):
    volume_shape, patch_shape, stride_shape, halo, batch, channels, pc = R.ACCUMULATOR_CASES[name]
    predictions, want = host_cases[name]
    dev = torch.from_numpy(predictions).cuda()
    got = _device_predict(volume_shape, patch_shape, stride_shape, halo, batch, lambda first, count: dev[first:first + count], channels, pc)
    _same(got, want)
    if name == 'a_ragged_d1':
        assert len(predictions) == 100 and set(np.unique(got[2])) == {1, 2}
    if name == 'c_broadcast_quirk':                       # the host's broadcast of patch[..., :1] is reproduced, and it is not the (2, 4, 4) volume
        assert not np.array_equal(got[0], host_cases['b_deep'][1][0], equal_nan=True)
    if name == 'e_mask_wraps':
        assert len(predictions) == 289 and int((got[2] == 0).sum()) == 4 and np.isinf(got[0][got[2] == 0]).all()
    again = _device_predict(volume_shape, patch_shape, stride_shape, halo, batch, lambda first, count: dev[first:first + count], channels, pc)
    _same(again, got)                                     # no atomics: the same bits from run to run


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_accumulator_reads_16bit_predictions(dtype):
    from afcm_amd.predictor import patch_indices
    volume_shape, patch_shape, stride_shape, halo, batch, channels, pc = R.ACCUMULATOR_CASES['b_deep']
    idx = patch_indices(volume_shape, patch_shape, stride_shape)
    low = torch.from_numpy(R.random_predictions(len(idx), channels, patch_shape, seed=12)).to(dtype)
    host = low.numpy() if dtype == torch.float16 else low.float().numpy()            # numpy has no bfloat16: the host adds the exact widening
    want = _host_predict(volume_shape, idx, halo, batch, host, pc)
    dev = low.cuda()
    _same(_device_predict(volume_shape, patch_shape, stride_shape, halo, batch, lambda first, count: dev[first:first + count], channels, pc), want)


def test_accumulator_reads_strided_four_dimensional_views(host_cases):
    """Case (a) with every batch handed over as the network hands it over: [B, C, h, w] (d = 1), here a channel slice and a window of a wider tensor."""
    volume_shape, patch_shape, stride_shape, halo, batch, channels, pc = R.ACCUMULATOR_CASES['a_ragged_d1']
    predictions, want = host_cases['a_ragged_d1']
    wide = torch.full((len(predictions), 3, patch_shape[1] + 3, patch_shape[2] + 5), float('nan'), device='cuda')
    wide[:, 1, 2:2 + patch_shape[1], 4:4 + patch_shape[2]] = torch.from_numpy(predictions[:, 0, 0]).cuda()

    def view(first, count):
        v = wide[first:first + count, 1:2, 2:2 + patch_shape[1], 4:4 + patch_shape[2]]
        assert v.dim() == 4 and not v.is_contiguous() and v.data_ptr() != wide.data_ptr()
        return v
    _same(_device_predict(volume_shape, patch_shape, stride_shape, halo, batch, view, channels, pc), want)


def _dataset_items(src, hw, thickness, slice_num, lo, hi):
    from afcm_amd.data import SliceDataset
    ds = SliceDataset({'raw': src}, phase='test', patch_shape=(1,) + hw, stride_shape=(1, 8, 8), thickness=[] if thickness is None else [thickness],
                      slice_num=slice_num, min_value=lo, max_value=hi)
    items = [ds[i] for i in range(len(ds))]
    return torch.stack([it[0] for it in items]), torch.stack([it[1] for it in items])


def _same_bits(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    bits = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}[want.dtype]
    assert torch.equal(got.cpu().view(bits), want.view(bits))


@pytest.mark.parametrize('name', sorted(R.ASSEMBLY_CASES))
def test_assembly_equals_stacked_dataset_items(name):
    from afcm_amd.torch_utils.ops.volume_ops import assemble_slices
    shape, dtype, hw, thickness, slice_num, (lo, hi) = R.ASSEMBLY_CASES[name]
    src = R.source(shape, dtype)
    want_a, want_idx = _dataset_items(src, hw, thickness, slice_num, lo, hi)
    vol = torch.from_numpy(src).cuda()
    kw = dict(thickness=thickness, slice_num=slice_num, min_value=lo, max_value=hi)
    a, idx = assemble_slices(vol, 0, shape[0], (1,) + hw, **kw)
    assert a.shape == (shape[0], slice_num) + hw and idx.shape == (shape[0], 1)
    _same_bits(a, want_a)
    _same_bits(idx, want_idx)
    if slice_num == 4:                                    # zero planes at both ends (depth 23, thickness 5: targets 0-4 and 15-22), at the value
        before, after = R.zero_plane_targets(shape[0], thickness)                  # a zero normalises to
        pad_value = np.float32(np.clip(2 * ((0.0 - lo) / (hi - lo)) - 1, -1, 1))
        assert (a[before, 0] == float(pad_value)).all() and (a[after, 3] == float(pad_value)).all()
        assert (pad_value == -1) == (lo == 0.0)
    for first, count in ((shape[0] // 3, 4), (shape[0] - 3, 3)):      # a run in the middle; a batch that ends at the last slice
        part_a, part_idx = assemble_slices(vol, first, count, (1,) + hw, **kw)
        _same_bits(part_a, want_a[first:first + count])
        _same_bits(part_idx, want_idx[first:first + count])
    for out_dtype in (torch.float16, torch.bfloat16):     # one more rounding of the float32 result
        low, low_idx = assemble_slices(vol, 0, shape[0], (1,) + hw, dtype=out_dtype, **kw)
        _same_bits(low, want_a.to(out_dtype))
        _same_bits(low_idx, want_idx)


@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
def test_assembly_reads_a_z_strided_view(dtype):
    from afcm_amd.torch_utils.ops.volume_ops import assemble_slices
    big = R.source((46, 28, 36), dtype, seed=5)
    lo, hi = (0., 255.) if dtype == np.uint8 else (-100., 900.)
    want_a, want_idx = _dataset_items(np.ascontiguousarray(big[::2]), (32, 32), 5, 4, lo, hi)
    view = torch.from_numpy(big).cuda()[::2]
    assert not view.is_contiguous() and view.stride(0) == 2 * 28 * 36
    a, idx = assemble_slices(view, 0, 23, (1, 32, 32), thickness=5, slice_num=4, min_value=lo, max_value=hi)
    _same_bits(a, want_a)
    _same_bits(idx, want_idx)


def test_argument_errors_raise_before_any_launch():
    from afcm_amd.torch_utils.ops.volume_ops import assemble_slices, halo_accumulate
    from afcm_amd.volume import DevicePredictor, PatchPlan
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device='cuda')
    pmap, mask, table = z(1, 4, 8, 8), z(1, 4, 8, 8, dtype=torch.uint8), z(4, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='larger than the volume'):        # patch outside the volume
        halo_accumulate(pmap, mask, z(1, 1, 5, 8, 8), table, 0, (0, 0, 0))
    with pytest.raises(RuntimeError, match='not inside the volume'):
        PatchPlan((4, 8, 8), [(slice(2, 6), slice(0, 8), slice(0, 8))])
    with pytest.raises(RuntimeError, match='negative halo'):
        halo_accumulate(pmap, mask, z(1, 1, 1, 8, 8), table, 0, (0, -1, 0))
    with pytest.raises(RuntimeError, match='non-negative'):
        DevicePredictor(patch_halo=(0, -1, 0))
    p = DevicePredictor(patch_halo=(2, 4, 4))
    p.allocate((12, 40, 44), 'cuda')
    with pytest.raises(AssertionError, match='Not enough patch overlap'):    # overlap smaller than the halo, via validate_halo
        p.plan((8, 16, 16), (7, 8, 8))
    with pytest.raises(RuntimeError, match='not inside a table'):
        halo_accumulate(pmap, mask, z(2, 1, 1, 8, 8), table, 3, (0, 0, 0))
    with pytest.raises(RuntimeError, match='outside the volume'):
        halo_accumulate(pmap, mask, z(1, 1, 1, 8, 8), table, 0, (0, 0, 0), box=((0, 5), (0, 8), (0, 8)))
    with pytest.raises(RuntimeError, match='prediction channel 2 of 2'):
        halo_accumulate(pmap, mask, z(1, 2, 1, 8, 8), table, 0, (0, 0, 0), prediction_channel=2)
    with pytest.raises(RuntimeError, match='a map of 1 channels for a prediction of 2'):
        halo_accumulate(pmap, mask, z(1, 2, 1, 8, 8), table, 0, (0, 0, 0))
    with pytest.raises(RuntimeError, match='no CPU'):                        # tensors on the CPU
        halo_accumulate(pmap, mask, torch.zeros(1, 1, 1, 8, 8), table, 0, (0, 0, 0))
    with pytest.raises(RuntimeError, match='no CPU'):
        halo_accumulate(pmap, mask, z(1, 1, 1, 8, 8), table.cpu(), 0, (0, 0, 0))
    with pytest.raises(RuntimeError, match='no CPU'):
        assemble_slices(torch.zeros(4, 8, 8, dtype=torch.uint8), 0, 2, (1, 8, 8), thickness=2)
    vol = z(4, 8, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='patch depth 2'):                 # patch depth != 1
        assemble_slices(vol, 0, 2, (2, 8, 8), thickness=2)
    with pytest.raises(RuntimeError, match='are not inside a volume of 4'):
        assemble_slices(vol, 3, 2, (1, 8, 8), thickness=2)
    with pytest.raises(RuntimeError, match='is not above min_value'):
        assemble_slices(vol, 0, 2, (1, 8, 8), thickness=2, min_value=1.0, max_value=1.0)
    with pytest.raises(RuntimeError, match='rows of the source must be contiguous'):
        assemble_slices(vol[:, :, ::2], 0, 2, (1, 8, 8), thickness=2)
    assert not pmap.any() and not mask.any()                                # nothing was launched


class StubStep:
    """``fake_B`` is a fixed function of ``real_A`` and ``gen_c`` (two channels of the input and the label); no host read."""

    def set_test_input(self, real_A, slice_idx):
        self.real_A, self.gen_c = real_A.cuda(), slice_idx.cuda()
        self.gen_z = torch.randn([real_A.shape[0], 8], device='cuda')

    def test(self):
        self.fake_B = self.real_A[:, 0:1] * 0.5 - self.real_A[:, 2:3] * 0.25 + self.gen_c[:, :, None, None]


def _counting(monkeypatch, copies):
    """Counts device -> host copies and scalar reads the way tests/test_gpu_validation.py::test_device_arm_copies_to_the_host_once does."""
    cpu, to, item, tolist = torch.Tensor.cpu, torch.Tensor.to, torch.Tensor.item, torch.Tensor.tolist

    def counted_cpu(self, *a, **k):
        if self.is_cuda:
            copies.append(('cpu', tuple(self.shape)))
        return cpu(self, *a, **k)

    def counted_to(self, *a, **k):
        out = to(self, *a, **k)
        if self.is_cuda and not out.is_cuda:
            copies.append(('to', tuple(self.shape)))
        return out

    def scalar_read(name, fn):
        def wrapped(self, *a, **k):
            if self.is_cuda:
                copies.append((name, tuple(self.shape)))
            return fn(self, *a, **k)
        return wrapped
    monkeypatch.setattr(torch.Tensor, 'cpu', counted_cpu)
    monkeypatch.setattr(torch.Tensor, 'to', counted_to)
    monkeypatch.setattr(torch.Tensor, 'item', scalar_read('item', item))
    monkeypatch.setattr(torch.Tensor, 'tolist', scalar_read('tolist', tolist))


def test_loop_with_a_stub_step(monkeypatch):
    from afcm_amd.volume import evaluate_volume, predict_volume
    src = R.source((11, 30, 40), np.uint8, seed=8)                          # pad in y, crop in x; three batches of 4, the last one ragged
    kw = dict(raw_internal_path_in='raw', thickness=5, patch_hw=(32, 32), batch_size=4, patch_halo=(0, 4, 4))
    host = predict_volume(StubStep(), {'raw': src}, where='host', heads=('prediction', 'input'), **kw)
    dev = predict_volume(StubStep(), {'raw': src}, where='device', heads=('prediction', 'input'), **kw)
    for head in ('prediction', 'input'):
        assert dev[head].is_cuda and not host[head].is_cuda and dev[head].shape == host[head].shape == (1, 11, 32, 32)
        assert np.array_equal(dev[head].cpu().numpy(), host[head].numpy(), equal_nan=True)
    assert np.array_equal(host['input'].numpy()[0], R.assemble(src, 0, 11, 4, 5, 32, 32)[0][:, 1])

    target = torch.from_numpy(R.assemble(R.source((11, 30, 40), np.uint8, seed=9), 0, 11, 1, None, 32, 32)[0][:, 0]).cuda()
    copies = []
    _counting(monkeypatch, copies)
    predict_volume(StubStep(), {'raw': src}, where='device', heads=('prediction', 'input'), **kw)
    assert copies == [], copies                                             # no device -> host copy, no scalar read
    out = evaluate_volume(StubStep(), {'raw': src}, target, **kw)
    assert copies == [('cpu', (11 + 32 + 32, 8))], copies                    # the three axes' tables, together, once
    copies.clear()
    predict_volume(StubStep(), {'raw': src}, where='host', heads=('prediction', 'input'), **kw)
    monkeypatch.undo()
    assert len(copies) == 3 * 2 and all(c[0] == 'cpu' for c in copies), copies     # the comparison arm: one copy per batch and head
    assert torch.equal(out['prediction'], dev['prediction'])
    assert all(np.isfinite(v) for v in out['slice'] + out['one'])


def _agree(name, got, want):
    print(f'{name}: device {got}')
    print(f'{name}: host   {want}')
    print(f'{name}: differences psnr {abs(got[0] - want[0]):.3e} dB, ssim {abs(got[1] - want[1]):.3e}, mae {abs(got[2] - want[2]) / want[2]:.3e} relative')
    assert abs(got[0] - want[0]) <= TOL_PSNR_DB
    assert abs(got[1] - want[1]) <= TOL_SSIM
    assert abs(got[2] - want[2]) <= TOL_MAE_REL * want[2]


def test_loop_with_the_tiny_ema_generator():
    """The 128^2 generator of tests/golden/G1_tiny128.npz as the EMA copy of a step (built as tests/test_gpu_validation.py builds it); one
    (11, 120, 136) uint8 subject: pad in y, crop in x, thickness 5, batch 4 -> three batches, the last one of 3."""
    from afcm_amd import evaluation
    from afcm_amd.networks_stylegan3 import Stylegan3Generator
    from afcm_amd.stylegan3_model import StyleGAN3GeneratorStep
    from afcm_amd.volume import evaluate_volume, predict_volume
    tiny = dict(channel_base=256, channel_max=8, num_layers=14, num_critical=2, margin_size=10, output_scale=0.25, skip_resolution=128,
                conv_kernel=3, filter_size=6, lrelu_upsampling=2, use_radial_filters=False, conv_clamp=256,
                magnitude_ema_beta=0.5 ** (16 / 20e3), cond_mod=True)
    g = load_golden('G1_tiny128')
    G = Stylegan3Generator(z_dim=32, c_dim=1, w_dim=32, img_resolution=128, img_channels_in=4, img_channels_out=1,
                           mapping_kwargs=dict(num_layers=2), synthesis_kwargs=dict(tiny, compute_dtype=torch.float32)).eval()
    G.load_state_dict({k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith('sd/')}, strict=True)
    step = StyleGAN3GeneratorStep(G.cuda(), ema=True)
    # an MR-like subject: a smooth bright blob on an exactly-zero background, so that slices are neither empty nor flat
    zz, yy, xx = np.meshgrid(np.linspace(-1, 1, 11), np.linspace(-1, 1, 120), np.linspace(-1, 1, 136), indexing='ij')
    body = np.clip(1.2 - (zz ** 2 * 0.3 + yy ** 2 + xx ** 2), 0, 1) * (0.6 + 0.4 * np.sin(7 * xx) * np.cos(5 * yy + zz))
    src = np.round(body * 255).astype(np.uint8)
    kw = dict(raw_internal_path_in='raw', thickness=5, patch_hw=(128, 128), batch_size=4, patch_halo=(0, 8, 8))

    def arm(where):
        torch.manual_seed(3)                                # set_test_input draws gen_z: the same draws for both arms
        return predict_volume(step, {'raw': src}, where=where, **kw)['prediction']
    host, dev = arm('host'), arm('device')
    assert dev.is_cuda and dev.shape == host.shape == (1, 11, 128, 128) and dev.dtype == host.dtype == torch.float32
    equal = torch.equal(dev.cpu(), host)
    if not equal:                                          # is the forward itself bit-reproducible?  (reported, the assertion below stands)
        print('host arm twice equal:', torch.equal(arm('host'), host), '; max |device - host| =', float((dev.cpu() - host).abs().max()))
    assert equal

    target_src = np.round(np.clip(body * 1.1 + 0.03 * np.random.default_rng(2).standard_normal(body.shape), 0, 1) * 255).astype(np.uint8)
    target = torch.from_numpy(R.assemble(target_src, 0, 11, 1, None, 128, 128)[0][:, 0])       # normalised as the loader normalises
    torch.manual_seed(3)
    out = evaluate_volume(step, {'raw': src}, target.cuda(), **kw)
    assert torch.equal(out['prediction'], dev)
    pred64 = evaluation.to_unit_range(host[0].numpy()).astype(np.float64)
    target64 = evaluation.to_unit_range(target.numpy()).astype(np.float64)
    _agree('evaluate_slice', out['slice'], evaluation.evaluate_slice(pred64, target64))
    _agree('evaluate_one', out['one'], evaluation.evaluate_one(pred64, target64))
