"""Percentile-clip normalisation on the GPU: ``afcm_percentile_bounds`` + ``afcm_clip_normalize`` (csrc/intensity.hip) against
``afcm_amd.intensity.percentile_clip_host``, which tests/test_percentile_clip_ref_cpu.py holds to the sort-and-index restatement, to numpy and to the
golden captured from the reference function.  The output volume is compared with ``torch.equal``; ``stats`` numerically, NaN matching NaN (which
zero a bound carries is not pinned).  The shapes come from ``afcm_percentile_plan`` where the kernels have seams."""
import numpy as np
import pytest
import torch

import percentile_clip_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

TORCH = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int16): torch.int16, np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
IDS = [np.dtype(t).name for t in R.DTYPES]
FLOATS = [np.float32, np.float64]


def _check(view, host, percentiles=(0.5, 99.5), positive=True, reference=None, **kw):
    """``view``: the device tensor as handed to the op; ``host``: the same values as an array; ``reference``: (device tensor, array) or None."""
    from afcm_amd.intensity import percentile_clip_host
    from afcm_amd.torch_utils.ops.intensity_ops import percentile_clip
    out, stats = percentile_clip(view, percentiles, positive, None if reference is None else reference[0], **kw)
    want, want_stats = percentile_clip_host(host, percentiles, positive, None if reference is None else reference[1])
    assert out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == host.shape
    assert stats.dtype == torch.float64 and tuple(stats.shape) == (4,)
    got_stats = stats.cpu().numpy()
    assert R.same_stats(got_stats, want_stats), (got_stats, want_stats)
    assert torch.equal(out.cpu(), torch.from_numpy(want)), f'{int((out.cpu().numpy() != want).sum())} of {want.size} voxels differ'
    return out.cpu().numpy(), got_stats


def _every_rank(values, shape, seed):
    """Every rank of ``values`` (all distinct) as the low and as the high percentile, for both ``strictly_positive`` values: one host copy."""
    from afcm_amd.intensity import percentile_clip_host
    from afcm_amd.torch_utils.ops.intensity_ops import percentile_clip
    n = values.shape[0]
    v = np.random.default_rng(seed).permutation(values).reshape(shape)
    dev = torch.from_numpy(v).cuda()
    qs = [R.rank_percentile(r, n) for r in range(n)]                        # q = 100 r / (n - 1)
    pairs = [(min(a, b), max(a, b), positive) for a, b in zip(qs, reversed(qs)) for positive in (True, False)]
    got = [percentile_clip(dev, (a, b), positive) for a, b, positive in pairs]
    outs, stats = torch.stack([g[0] for g in got]).cpu(), torch.stack([g[1] for g in got]).cpu().numpy()
    reached = set()
    for k, (a, b, positive) in enumerate(pairs):
        want, want_stats = percentile_clip_host(v, (a, b), positive)
        assert R.same_stats(stats[k], want_stats), ((a, b, positive), stats[k], want_stats)
        assert torch.equal(outs[k], torch.from_numpy(want)), (a, b, positive)
        for q in (a, b):                                                    # the order statistics this call selected
            i = int(np.floor(np.float64(q / 100.0) * np.float64(n - 1)))
            reached |= {i, min(i + 1, n - 1)}
    assert reached == set(range(n))


@pytest.mark.parametrize('dtype', FLOATS, ids=['float32', 'float64'])
def test_every_rank_of_signed_keys_that_differ_in_every_digit(dtype):
    from afcm_amd.torch_utils.ops.intensity_ops import percentile_plan
    values = R.signed_digit_values(dtype)
    plan = percentile_plan(67, TORCH[np.dtype(dtype)])
    assert plan['bits'] == (8,) * np.dtype(dtype).itemsize and values.shape == (67,)
    bits = values.view({4: np.uint32, 8: np.uint64}[values.itemsize])
    for byte in range(values.itemsize):                                     # some pair of values differs in every digit
        assert len({(int(b) >> (8 * byte)) & 0xff for b in bits}) > 1
    _every_rank(values, (1, 1, 67), 6)


@pytest.mark.parametrize('dtype', FLOATS, ids=['float32', 'float64'])
def test_neighbours_across_zero_and_infinities(dtype):
    info = np.finfo(dtype)
    d = np.array(info.smallest_subnormal, dtype=dtype)
    v = np.array([-d, -0.0, 0.0, d, -1.5, 2.5, -info.max, info.max, info.tiny, -info.tiny, 3.0, -3.0], dtype=dtype).reshape(1, 3, 4)
    dev = torch.from_numpy(v).cuda()
    n = v.size
    for r in range(n - 1):                                                  # ranks r and r + 1 as the two bounds, and the point halfway
        for pair in ((R.rank_percentile(r, n), R.rank_percentile(r + 1, n)), (100.0 * (r + 0.5) / (n - 1),) * 2):
            for positive in (True, False):
                _check(dev, v, pair, positive)
    _, stats = _check(dev, v, (R.rank_percentile(4, n), R.rank_percentile(7, n)), False)
    assert stats[0] == -float(d) and stats[1] == float(d)                   # ... -tiny, -d, -0, +0, d, tiny ...: ranks 4 and 7 are the denormals
    w = v.copy()
    w[0, 2, 2:] = [-np.inf, np.inf]                                         # replaces 3.0 and -3.0
    dev = torch.from_numpy(w).cuda()
    for pair in ((0.0, 100.0), (5.0, 95.0), (R.rank_percentile(1, n), R.rank_percentile(10, n)), (30.0, 60.0)):
        for positive in (True, False):
            _check(dev, w, pair, positive)
    _, stats = _check(dev, w, (5.0, 95.0), False)                           # between -inf and -max, and between max and +inf: a + inf * g
    assert stats[0] == -np.inf and stats[1] == np.inf and stats[3] == 0.0


def test_int16_seams_of_the_high_byte_and_of_the_sign():
    from afcm_amd.torch_utils.ops.intensity_ops import percentile_plan
    assert percentile_plan(10, torch.int16)['bits'] == (8, 8)
    seams = np.array([-32768, -257, -256, -255, -1, 0, 1, 255, 256, 32767], dtype=np.int16)
    _every_rank(seams, (1, 2, 5), 7)
    spread = np.array([-300, -257, -256, -255, -2, -1, 0, 1, 2, 254, 255, 256, 257, 300, -32768 + 32767, 77, -77], dtype=np.int16)
    _every_rank(np.unique(spread), (1, 1, np.unique(spread).shape[0]), 8)


BOUNDARIES = [
    ('int16_sign_and_high_byte', np.int16, -1, 0),
    ('int16_high_byte_255_256', np.int16, 255, 256),
    ('int16_high_byte_negative', np.int16, -257, -256),
    ('int16_low_byte_0_1', np.int16, 0, 1),
    ('int16_low_byte_negative', np.int16, -3, -2),
    ('int16_lowest_and_minus_one', np.int16, -32768, -1),                   # 32767 apart: the most that numpy's int16 subtraction of neighbours holds
    ('int16_zero_and_highest', np.int16, 0, 32767),
    ('uint8_127_128', np.uint8, 127, 128),
    ('uint8_0_255', np.uint8, 0, 255),
    ('float32_sign', np.float32, -np.float32(1e-3), np.float32(1e-3)),
    ('float32_lowest_digit', np.float32, np.float32(1), np.nextafter(np.float32(1), np.float32(2))),
    ('float32_top_digit_negative', np.float32, np.float32(-2), np.nextafter(np.float32(-2), np.float32(0))),
    ('float64_sign', np.float64, -1e-3, 1e-3),
    ('float64_middle_digit', np.float64, np.nextafter(1.0 + 2.0 ** -21, 0.0), 1.0 + 2.0 ** -21),
    ('float64_lowest_digit_negative', np.float64, np.nextafter(-1.0, -2.0), -1.0),
]


@pytest.mark.parametrize('name,dtype,a,b', BOUNDARIES, ids=[c[0] for c in BOUNDARIES])
def test_neighbouring_ranks_across_a_bin_boundary(name, dtype, a, b):
    """Ranks i and i + 1 fall into different bins of the digit named: 60 voxels of ``a`` and 60 of ``b``, the median between them."""
    v = np.empty(120, dtype=dtype)
    v[:60], v[60:] = a, b
    v = np.random.default_rng(7).permutation(v).reshape(2, 6, 10)
    dev = torch.from_numpy(v).cuda()
    for pair in ((50.0, 100.0), (0.0, 50.0), (49.0, 51.0), (50.0, 50.0)):
        for positive in (True, False):
            _check(dev, v, pair, positive)
    _, stats = _check(dev, v, (0.0, 100.0), False)
    assert stats[0] == float(a) and stats[1] == float(b)


def test_uint8_full_range():
    v = np.random.default_rng(9).permutation(np.arange(256, dtype=np.uint8)).reshape(4, 8, 8)
    dev = torch.from_numpy(v).cuda()
    got, stats = _check(dev, v, (0.0, 100.0))
    assert stats.tolist() == [0.0, 255.0, 256.0, 0.0] and got.min() == 0 and got.max() == 255
    _every_rank(np.arange(256, dtype=np.uint8)[::4], (1, 8, 8), 10)
    _check(dev, v)


@pytest.mark.parametrize('dtype', R.DTYPES, ids=IDS)
def test_ties_and_single_voxels(dtype):
    value = {'uint8': 200}.get(np.dtype(dtype).name, -300)
    constant = np.full((2, 5, 9), value, dtype=dtype)
    got, stats = _check(torch.from_numpy(constant).cuda(), constant, positive=False)
    assert stats.tolist() == [float(value), float(value), 90.0, 0.0] and not got.any()          # hi == lo: 0 / 0 -> 0
    _check(torch.from_numpy(constant).cuda(), constant, positive=True)                          # negative: lo = 0 above hi, everything 255
    two = constant.copy()
    two[0] = 3
    for pair in ((0.5, 99.5), (0.0, 100.0), (50.0, 50.0), (37.5, 37.5)):                        # the minimum and the maximum; equal percentiles
        for positive in (True, False):
            _check(torch.from_numpy(two).cuda(), two, pair, positive)
    _, stats = _check(torch.from_numpy(two).cuda(), two, (0.0, 100.0), False)
    assert stats[:2].tolist() == [float(min(3, value)), float(max(3, value))]
    one = np.full((1, 1, 1), value, dtype=dtype)
    got, stats = _check(torch.from_numpy(one).cuda(), one, positive=False)
    assert got.item() == 0 and stats.tolist() == [float(value), float(value), 1.0, 0.0]
    for shape, seed in (((3, 5, 7), 1), ((2, 33, 65), 2)):
        v = R.signed_volume(shape, dtype, seed)
        for positive in (True, False):
            _check(torch.from_numpy(v).cuda(), v, positive=positive)


@pytest.mark.parametrize('dtype', FLOATS, ids=['float32', 'float64'])
def test_one_nan_anywhere(dtype):
    base = R.signed_volume((3, 9, 13), dtype, 11)
    for at, nan in ((0, np.nan), (base.size - 1, np.nan), (base.size // 2, -np.nan)):
        v = base.copy()
        v.reshape(-1)[at] = nan
        assert np.signbit(v.reshape(-1)[at]) == np.signbit(nan)
        for positive in (True, False):
            got, stats = _check(torch.from_numpy(v).cuda(), v, positive=positive)
            assert not got.any() and np.isnan(stats[:2]).all() and stats[2:].tolist() == [float(v.size), 1.0]
    v = base.copy()
    v.reshape(-1)[[3, 77, 200]] = [np.nan, -np.nan, np.nan]
    _, stats = _check(torch.from_numpy(v).cuda(), v)
    assert stats[2:].tolist() == [float(v.size), 3.0]
    nothing = np.full((1, 2, 3), np.nan, dtype=dtype)                       # no voxel has a key
    _, stats = _check(torch.from_numpy(nothing).cuda(), nothing)
    assert stats[2:].tolist() == [6.0, 6.0]


def test_more_than_two_rounds_of_the_grid_uint8():
    """A little over two rounds of the full grid plus a ragged tail: the grid-stride loop runs three times in some workgroups and twice in others,
    the last chunk is partial, and the scan adds every slot."""
    from afcm_amd.torch_utils.ops.intensity_ops import percentile_plan
    plan = percentile_plan(2 ** 31 - 1, torch.uint8)
    voxels = (2 * plan['groups'] + 1) * plan['chunk'] + 37
    h = -(-voxels // (3 * 101))
    here = percentile_plan(3 * h * 101, torch.uint8)
    assert here['groups'] == plan['groups'] and 2 * here['groups'] * here['chunk'] < 3 * h * 101 < 3 * here['groups'] * here['chunk']
    assert (3 * h * 101) % here['chunk'] != 0
    v = R.signed_volume((3, h, 101), np.uint8, 5)
    _check(torch.from_numpy(v).cuda(), v)


@pytest.mark.parametrize('dtype', [np.int16, np.float32], ids=['int16', 'float32'])
def test_one_voxel_past_a_full_round_of_the_grid(dtype):
    from afcm_amd.torch_utils.ops.intensity_ops import percentile_plan
    plan = percentile_plan(2 ** 31 - 1, TORCH[np.dtype(dtype)])
    voxels = plan['groups'] * plan['chunk'] + 1
    v = R.signed_volume((1, 1, voxels), dtype, 12)
    v[0, 0, -1] = -12345                                                    # the one voxel of the second round is the minimum
    _, stats = _check(torch.from_numpy(v).cuda(), v, (0.0, 100.0), False)
    assert stats[0] == -12345.0 and stats[2] == voxels


@pytest.mark.parametrize('dtype', R.DTYPES, ids=IDS)
def test_views(dtype):
    v = R.signed_volume((6, 9, 20), dtype, 3)                               # every second slice: a z stride of two slices
    view = torch.from_numpy(v).cuda()[::2]
    assert not view.is_contiguous()
    _check(view, v[::2], positive=False)
    # a volume that starts at an odd element of a larger buffer, odd width: the map's rows start on every alignment, its head and tail run
    v = R.signed_volume((3, 7, 37), dtype, 4)
    buffer = torch.zeros(v.size + 5, dtype=TORCH[np.dtype(dtype)], device='cuda')
    buffer[3:3 + v.size] = torch.from_numpy(v).cuda().reshape(-1)
    view = buffer[3:3 + v.size].view(v.shape)
    assert view.storage_offset() == 3
    _check(view, v)
    plane = torch.full((v.size + 40,), 99, dtype=torch.uint8, device='cuda')
    for at in (0, 5, 16):                                                   # an aligned output, one that starts 5 bytes in, and one a whole run in
        plane.fill_(99)
        out = plane[at:at + v.size].view(v.shape)
        _check(view, v, positive=False, out=out)
        host = plane.cpu().numpy()
        assert (host[:at] == 99).all() and (host[at + v.size:] == 99).all()


def test_reference_of_another_shape_and_dtype():
    from afcm_amd.torch_utils.ops.intensity_ops import percentile_bounds, percentile_clip
    v = R.signed_volume((3, 7, 37), np.float32, 13)
    r = R.signed_volume((5, 11, 6), np.int16, 14)
    dev, ref = torch.from_numpy(v).cuda(), torch.from_numpy(r).cuda()
    for positive in (True, False):
        _, stats = _check(dev, v, (2.0, 90.0), positive, reference=(ref, r))
        assert stats[2] == r.size
    dirty = v.copy()
    dirty[1, 2, 3] = np.nan                                                 # a NaN voxel under the finite bounds of a clean reference: 0
    got, stats = _check(torch.from_numpy(dirty).cuda(), dirty, (2.0, 90.0), True, reference=(ref, r))
    assert got[1, 2, 3] == 0 and stats[3] == 0.0 and got.any()
    # percentile_bounds alone: the stats of the whole op, and twice the same bits
    out, stats = percentile_clip(dev, (2.0, 90.0), False, ref)
    alone = percentile_bounds(ref, (2.0, 90.0), False)
    assert torch.equal(alone.view(torch.int64), stats.view(torch.int64))
    again, stats2 = percentile_clip(dev, (2.0, 90.0), False, ref)
    assert torch.equal(again, out) and torch.equal(stats2.view(torch.int64), stats.view(torch.int64))


def test_workspace_reused_after_a_nan_call_and_the_refusals():
    """Through the C ABI with one caller-owned workspace, poisoned first: a NaN call leaves nothing behind that the next call reads."""
    from afcm_amd import _lib
    from afcm_amd.intensity import percentile_clip_host
    lib = _lib.load()
    v = R.signed_volume((3, 10, 12), np.float32, 9)
    bad = v.copy()
    bad[0, 0, :5] = np.nan
    dev, dev_bad = torch.from_numpy(v).cuda(), torch.from_numpy(bad).cuda()
    nbytes = lib.afcm_percentile_workspace_bytes(v.size, _lib.SRC_F32)
    assert nbytes > 0
    workspace = torch.full((nbytes // 8 + 1,), -1, dtype=torch.int64, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream

    def run(t):
        out = torch.full(tuple(t.shape), 77, dtype=torch.uint8, device='cuda')
        stats = torch.full((4,), 5.0, dtype=torch.float64, device='cuda')
        assert lib.afcm_percentile_bounds(stats.data_ptr(), workspace.data_ptr(), t.data_ptr(), _lib.SRC_F32, *t.shape, t.stride(0), 0.005, 0.995, 0,
                                          stream) == 0
        assert lib.afcm_clip_normalize(out.data_ptr(), stats.data_ptr(), t.data_ptr(), _lib.SRC_F32, *t.shape, t.stride(0), stream) == 0
        return out.cpu().numpy(), stats.cpu().numpy()
    want, want_stats = percentile_clip_host(v, (0.5, 99.5), False)
    for t, nans in ((dev_bad, 5), (dev, 0), (dev, 0), (dev_bad, 5), (dev, 0)):
        out, stats = run(t)
        if nans:
            assert not out.any() and np.isnan(stats[:2]).all() and stats[2:].tolist() == [float(v.size), 5.0]
        else:
            assert np.array_equal(out, want) and R.same_stats(stats, want_stats)
    # refusals leave the outputs alone
    out = torch.full(tuple(dev.shape), 77, dtype=torch.uint8, device='cuda')
    stats = torch.full((4,), 5.0, dtype=torch.float64, device='cuda')
    d, h, w = dev.shape
    for args in ((stats.data_ptr(), workspace.data_ptr(), dev.data_ptr(), 4, d, h, w, h * w, 0.005, 0.995, 1, stream),
                 (stats.data_ptr(), workspace.data_ptr(), dev.data_ptr(), _lib.SRC_F32, d, h, w, -1, 0.005, 0.995, 1, stream),
                 (stats.data_ptr(), workspace.data_ptr(), dev.data_ptr(), _lib.SRC_F32, d, h, w, h * w, 0.7, 0.2, 1, stream),
                 (stats.data_ptr(), workspace.data_ptr() + 4, dev.data_ptr(), _lib.SRC_F32, d, h, w, h * w, 0.005, 0.995, 1, stream),
                 (None, workspace.data_ptr(), dev.data_ptr(), _lib.SRC_F32, d, h, w, h * w, 0.005, 0.995, 1, stream)):
        assert lib.afcm_percentile_bounds(*args) == _lib.E_INVALID
    for args in ((out.data_ptr(), stats.data_ptr(), dev.data_ptr(), -1, d, h, w, h * w, stream), (out.data_ptr(), stats.data_ptr(), dev.data_ptr(), _lib.SRC_F32, d, 0, w, h * w, stream),
                 (out.data_ptr(), None, dev.data_ptr(), _lib.SRC_F32, d, h, w, h * w, stream), (out.data_ptr(), stats.data_ptr() + 4, dev.data_ptr(), _lib.SRC_F32, d, h, w, h * w, stream)):
        assert lib.afcm_clip_normalize(*args) == _lib.E_INVALID
    assert (out == 77).all() and (stats == 5.0).all()


def test_golden_through_the_device_op():
    from afcm_amd.torch_utils.ops.intensity_ops import percentile_clip
    g = load_golden('I2_percentile_clip')
    pair = tuple(g['percentiles'].tolist())
    for name in IDS:
        dev = torch.from_numpy(g[f'volume_{name}']).cuda()
        for positive, tag in ((True, f'{name}_positive'), (False, f'{name}_signed')):
            assert float(g[f'differing_share_{tag}']) == 0.0
            out, stats = percentile_clip(dev, pair, positive)
            assert np.array_equal(out.cpu().numpy(), g[f'clipped_{tag}']), tag
            assert R.same_stats(stats.cpu().numpy()[:2], g[f'bounds_{tag}']), tag


class StubStep:
    """``fake_B`` is a fixed function of ``real_A`` and the label; no host read (the stub of tests/test_gpu_volume.py)."""

    def set_test_input(self, real_A, slice_idx):
        self.real_A, self.gen_c = real_A.cuda(), slice_idx.cuda()

    def test(self):
        self.fake_B = self.real_A[:, 0:1] * 0.5 - self.real_A[:, 2:3] * 0.25 + self.gen_c[:, :, None, None]


def _counting(monkeypatch, copies):
    cpu, to, item, tolist = torch.Tensor.cpu, torch.Tensor.to, torch.Tensor.item, torch.Tensor.tolist

    def counted_to(self, *a, **k):
        out = to(self, *a, **k)
        if self.is_cuda and not out.is_cuda:
            copies.append(('to', tuple(self.shape)))
        return out

    def reads(name, fn):
        def wrapped(self, *a, **k):
            if self.is_cuda:
                copies.append((name, tuple(self.shape)))
            return fn(self, *a, **k)
        return wrapped
    monkeypatch.setattr(torch.Tensor, 'cpu', reads('cpu', cpu))
    monkeypatch.setattr(torch.Tensor, 'to', counted_to)
    monkeypatch.setattr(torch.Tensor, 'item', reads('item', item))
    monkeypatch.setattr(torch.Tensor, 'tolist', reads('tolist', tolist))


def test_predict_volume_clips_a_raw_source(monkeypatch):
    from afcm_amd.intensity import percentile_clip_host
    from afcm_amd.volume import predict_volume
    raw = R.signed_volume((11, 30, 40), np.int16, 11)
    kw = dict(raw_internal_path_in='raw', thickness=5, patch_hw=(32, 32), batch_size=4, patch_halo=(0, 4, 4), heads=('prediction', 'input'))
    host = predict_volume(StubStep(), {'raw': raw}, where='host', clip=(0.5, 99.5), **kw)
    copies = []
    _counting(monkeypatch, copies)
    dev = predict_volume(StubStep(), {'raw': raw}, where='device', clip=(0.5, 99.5), **kw)
    monkeypatch.undo()
    assert copies == [], copies                                             # no device -> host copy, no scalar read
    for head in kw['heads']:
        assert dev[head].is_cuda and torch.equal(dev[head].cpu(), host[head])
    # the loop saw the clipped volume: the same as clipping on the host first and passing clip=None; rescale= is another normalisation
    pre = predict_volume(StubStep(), {'raw': percentile_clip_host(raw)[0]}, where='device', **kw)
    other = predict_volume(StubStep(), {'raw': raw}, where='device', rescale=(0.5, 99.5), **kw)
    assert torch.equal(pre['prediction'], dev['prediction']) and not torch.equal(other['prediction'], dev['prediction'])
    with pytest.raises(ValueError, match='rescale= and clip='):
        predict_volume(StubStep(), {'raw': raw}, where='device', rescale=(0.5, 99.5), clip=(0.5, 99.5), **kw)


def test_predict_and_evaluate_volume_clip_with_the_tiny_ema_generator():
    """The 128^2 generator of tests/golden/G1_tiny128.npz as the EMA copy of a step (built as tests/test_gpu_volume.py builds it); one (7, 120, 136)
    float32 subject with a negative tail: device arm against host arm, and ``evaluate_volume`` following through its keywords."""
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
    raw = R.signed_volume((7, 120, 136), np.float32, 15)                    # depth 7: the metrics' SSIM window
    kw = dict(raw_internal_path_in='raw', thickness=3, patch_hw=(128, 128), batch_size=4, patch_halo=(0, 8, 8), clip=(1.0, 99.0))

    def arm(where):
        torch.manual_seed(3)                                # set_test_input draws gen_z: the same draws for both arms
        return predict_volume(step, {'raw': raw}, where=where, **kw)['prediction']
    host, dev = arm('host'), arm('device')
    assert dev.is_cuda and dev.shape == host.shape == (1, 7, 128, 128) and torch.equal(dev.cpu(), host)
    torch.manual_seed(3)
    out = evaluate_volume(step, {'raw': raw}, torch.zeros(7, 128, 128, device='cuda'), **kw)
    assert torch.equal(out['prediction'], dev)


def test_slice_set_clips_into_a_uint8_pool():
    from afcm_amd.data import SliceDataset
    from afcm_amd.intensity import percentile_clip_host
    from afcm_amd.training import DeviceSliceSet
    sources = [{'raw': R.signed_volume(shape, dtype, seed)} for shape, dtype, seed in
               (((5, 20, 24), np.int16, 12), ((4, 33, 17), np.float32, 13), ((6, 16, 16), np.float64, 14))]
    ds = DeviceSliceSet(sources, phase='train', patch_shape=(1, 24, 24), thickness=[2, 3], clip=(0.5, 99.5))
    assert ds.pool.dtype == torch.uint8 and ds.source_dtype == np.uint8
    want = [percentile_clip_host(s['raw'])[0] for s in sources]
    assert torch.equal(ds.pool.cpu(), torch.from_numpy(np.concatenate([w.reshape(-1) for w in want])))
    items = ds.epoch_items(3)
    ds.load_epoch(items)
    got = ds.batch(0, len(ds))
    for g, w in zip(got, ds.host_batch(items, 0, len(ds), device='cpu')):
        assert torch.equal(g.cpu(), w)
    # ... and the host arm is SliceDataset on the host-clipped volumes
    for row in (0, 7, 14):
        vol_a, vol_b, idx, t = items[row].tolist()
        item = SliceDataset({'raw': want[vol_b]}, phase='train', patch_shape=(1, 24, 24), stride_shape=(1, 1, 1), thickness=[t])[idx]
        assert torch.equal(got[0][row].cpu(), item['A']) and torch.equal(got[1][row].cpu(), item['B'])
    # a set built with neither keyword pools the volumes as they are and gives the plain batches
    plain = DeviceSliceSet(sources[:1], phase='train', patch_shape=(1, 24, 24), thickness=[2, 3])
    assert plain.pool.dtype == torch.int16 and torch.equal(plain.pool.cpu(), torch.from_numpy(sources[0]['raw'].reshape(-1)))
    items = plain.epoch_items(3)
    plain.load_epoch(items)
    for g, w in zip(plain.batch(0, len(plain)), plain.host_batch(items, 0, len(plain), device='cpu')):
        assert torch.equal(g.cpu(), w)
    with pytest.raises(RuntimeError, match='mixed source dtypes'):
        DeviceSliceSet(sources, phase='train', patch_shape=(1, 24, 24), thickness=[2, 3])
