"""Intensity rescaling on the GPU: ``afcm_rescale_intensity`` (csrc/intensity.hip) against the sort-and-index restatement of tests/intensity_ref.py.
Output volume and ``stats`` are compared bit for bit (any NaN equals any NaN) everywhere; the only condition is the float32 golden case, where the
reference computes in float32 (see its test).  The shapes come from ``afcm_rescale_plan`` where the kernels have seams."""
import numpy as np
import pytest
import torch

import intensity_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

TORCH = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int16): torch.int16, np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
IDS = [np.dtype(t).name for t in R.DTYPES]


def _check(view, host, percentiles=(0.5, 99.5)):
    """``view``: the device tensor as handed to the op; ``host``: the same values as an array."""
    from afcm_amd.torch_utils.ops.intensity_ops import rescale_intensity
    out, stats = rescale_intensity(view, percentiles)
    want, want_stats = R.rescale(host, percentiles)
    assert out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == host.shape
    assert stats.dtype == torch.float64 and tuple(stats.shape) == (3,)
    got, got_stats = out.cpu().numpy(), stats.cpu().numpy()
    assert R.same_bits(got_stats, want_stats), (got_stats, want_stats)
    assert np.array_equal(got, want), f'{int((got != want).sum())} of {got.size} voxels differ'
    return got, got_stats


def _plan(dtype, voxels=2 ** 31 - 1):
    from afcm_amd.torch_utils.ops.intensity_ops import rescale_plan
    return rescale_plan(voxels, TORCH[np.dtype(dtype)])


@pytest.mark.parametrize('dtype', R.DTYPES, ids=IDS)
def test_small_shapes_and_views(dtype):
    one = np.full((1, 1, 1), 7, dtype=dtype)
    got, stats = _check(torch.from_numpy(one).cuda(), one)
    assert got.item() == 1 and stats.tolist() == [7.0, 7.0, 1.0]           # hi == lo, v == lo: 0 / 0 -> 1
    zero = np.zeros((1, 1, 1), dtype=dtype)
    got, stats = _check(torch.from_numpy(zero).cuda(), zero)
    assert got.item() == 0 and np.isnan(stats[:2]).all() and stats[2] == 0.0
    for shape, seed in (((3, 5, 7), 1), ((2, 33, 65), 2)):
        v = R.skewed_volume(shape, dtype, seed)
        _check(torch.from_numpy(v).cuda(), v)
    v = R.skewed_volume((6, 9, 20), dtype, 3)                              # every second slice: a z stride of two slices
    view = torch.from_numpy(v).cuda()[::2]
    assert not view.is_contiguous()
    _check(view, v[::2])
    # a volume that starts at an odd element of a larger buffer, odd width: the map's rows start on every alignment, its head and tail run
    v = R.skewed_volume((3, 7, 37), dtype, 4)
    buffer = torch.zeros(v.size + 5, dtype=TORCH[np.dtype(dtype)], device='cuda')
    buffer[3:3 + v.size] = torch.from_numpy(v).cuda().reshape(-1)
    view = buffer[3:3 + v.size].view(v.shape)
    assert view.storage_offset() == 3
    _check(view, v)


@pytest.mark.parametrize('dtype', R.DTYPES, ids=IDS)
def test_more_than_two_rounds_of_the_grid(dtype):
    """A little over two rounds of the full grid plus a ragged tail: the grid-stride loop runs three times in some workgroups and twice in others,
    the last chunk is partial, and the scan adds every slot."""
    plan = _plan(dtype)
    voxels = (2 * plan['groups'] + 1) * plan['chunk'] + 37
    h = -(-voxels // (3 * 101))
    shape = (3, h, 101)
    here = _plan(dtype, 3 * h * 101)
    assert here['groups'] == plan['groups'] and 2 * here['groups'] * here['chunk'] < 3 * h * 101 < 3 * here['groups'] * here['chunk']
    assert (3 * h * 101) % here['chunk'] != 0
    v = R.skewed_volume(shape, dtype, 5)
    _check(torch.from_numpy(v).cuda(), v)


@pytest.mark.parametrize('dtype', R.DTYPES, ids=IDS)
def test_every_rank_of_keys_that_differ_in_every_digit(dtype):
    from afcm_amd.torch_utils.ops.intensity_ops import rescale_intensity
    plan = _plan(dtype, 77)
    limit = {np.dtype(np.float32): 0x7f800000, np.dtype(np.float64): 0x7ff << 52}.get(np.dtype(dtype))
    keys = R.digit_keys(plan['bits'], limit)
    assert len(keys) == 67 and sum(plan['bits']) == {'uint8': 8, 'int16': 15, 'float32': 31, 'float64': 63}[np.dtype(dtype).name]
    total = sum(plan['bits'])
    for p, width in enumerate(plan['bits']):                               # some pair of keys differs in digit p
        shift = total - sum(plan['bits'][:p + 1])
        assert len({(k >> shift) & ((1 << width) - 1) for k in keys}) > 1
    values = np.zeros(77, dtype=dtype)
    values[:67] = R.keys_to_values(keys, dtype)
    v = np.random.default_rng(6).permutation(values).reshape(1, 7, 11)
    dev = torch.from_numpy(v).cuda()
    qs = R.rank_sweep(67)
    index = [R.virtual_index(q, 67) for q in qs]
    assert {i for i, _ in index} == set(range(67))
    assert sum(1 for i, g in index if g == 0.0 and i > 0) >= 10 and sum(1 for _, g in index if g == 0.5) >= 10
    assert any(0.49 < g < 0.5 for _, g in index) and index[1] == (66, 0.0)
    pairs = [(min(a, b), max(a, b)) for a, b in zip(qs, reversed(qs))]
    got = [rescale_intensity(dev, pair) for pair in pairs]
    outs, stats = torch.stack([g[0] for g in got]).cpu().numpy(), torch.stack([g[1] for g in got]).cpu().numpy()
    for k, pair in enumerate(pairs):
        want, want_stats = R.rescale(v, pair)
        assert R.same_bits(stats[k], want_stats), (pair, stats[k], want_stats)
        assert np.array_equal(outs[k], want), pair


BOUNDARIES = [
    ('float32_top_digit', np.float32, np.nextafter(np.float32(2), np.float32(0)), np.float32(2)),
    ('float64_top_digit', np.float64, np.nextafter(2.0, 0.0), 2.0),
    ('float32_lowest_digit', np.float32, np.float32(1), np.nextafter(np.float32(1), np.float32(2))),
    ('float64_lowest_digit', np.float64, 1.0, np.nextafter(1.0, 2.0)),
    ('float32_second_digit', np.float32, np.float32(1.4999999), np.float32(1.5)),
    ('float64_middle_digit', np.float64, np.nextafter(1.0 + 2.0 ** -21, 0.0), 1.0 + 2.0 ** -21),
    ('int16_255_256', np.int16, 255, 256),
    ('int16_32766_32767', np.int16, 32766, 32767),
    ('int16_1_32767', np.int16, 1, 32767),
    ('uint8_127_128', np.uint8, 127, 128),
    ('uint8_254_255', np.uint8, 254, 255),
]


@pytest.mark.parametrize('name,dtype,a,b', BOUNDARIES, ids=[c[0] for c in BOUNDARIES])
def test_neighbouring_ranks_across_a_bin_boundary(name, dtype, a, b):
    """Ranks i and i + 1 fall into different bins of the digit named: 50 voxels of ``a`` and 50 of ``b``, the median between them."""
    v = np.zeros((2, 6, 10), dtype=dtype).reshape(-1)
    v[:50], v[50:100] = a, b
    v = np.random.default_rng(7).permutation(v).reshape(2, 6, 10)
    dev = torch.from_numpy(v).cuda()
    for pair in ((50.0, 100.0), (0.0, 50.0), (49.0, 51.0), (50.0, 50.0)):
        _, stats = _check(dev, v, pair)
    assert stats[0] == stats[1] == (float(a) + float(b)) / 2 or name.endswith('lowest_digit')      # the median proper, where a double holds it


@pytest.mark.parametrize('dtype', R.DTYPES, ids=IDS)
def test_ties(dtype):
    top = {'uint8': 255, 'int16': 32767}.get(np.dtype(dtype).name, 1000.5)
    constant = np.zeros((2, 5, 9), dtype=dtype)
    constant[:, 1:4] = top
    got, stats = _check(torch.from_numpy(constant).cuda(), constant)
    assert stats.tolist() == [float(top), float(top), 54.0] and set(np.unique(got)) == {0, 1}   # hi == lo: everything equal maps to 1
    full = np.full((2, 5, 9), top, dtype=dtype)                                                 # no background at all (uint8: all 255)
    got, _ = _check(torch.from_numpy(full).cuda(), full)
    assert (got == 1).all()
    two = constant.copy()
    two[0, 1:4] = 3
    _check(torch.from_numpy(two).cuda(), two)
    _check(torch.from_numpy(two).cuda(), two, (0.0, 100.0))
    single = np.zeros((2, 5, 9), dtype=dtype)
    single[1, 2, 3] = 9
    got, stats = _check(torch.from_numpy(single).cuda(), single)
    assert stats.tolist() == [9.0, 9.0, 1.0] and got[1, 2, 3] == 1 and got.sum() == 1


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_non_finite_values_and_signs(dtype):
    info = np.finfo(dtype)
    denormal = np.array(info.smallest_subnormal, dtype=dtype)
    rng = np.random.default_rng(8)
    v = rng.gamma(2.0, 50.0, size=(4, 9, 13)).astype(dtype)
    flat = v.reshape(-1)
    flat[:12] = [np.nan, -np.inf, np.inf, -0.0, denormal, -denormal, -1.5, 0.0, -np.nan, info.max, info.tiny, -info.max]
    v = rng.permutation(flat).reshape(4, 9, 13)
    dev = torch.from_numpy(v).cuda()
    got, stats = _check(dev, v, (10.0, 50.0))                              # the +inf is foreground but on no rank
    assert stats[2] == v.size - 8 and np.isfinite(stats[:2]).all()         # background: NaN, -inf, -0.0, -denormal, -1.5, 0.0, -NaN, -max
    background = ~(v > 0)
    assert background.sum() == 8 and (got[background] == 0).all() and (got[~background] >= 1).all()
    assert got[v == denormal] == 1 and got[np.isposinf(v)] == 255
    got, stats = _check(dev, v, (0.0, 100.0))                              # lo = the denormal; a = b = +inf: d = inf - inf, hi NaN, every level NaN -> 1
    assert stats[0] == float(denormal) and np.isnan(stats[1]) and (got[~background] == 1).all()
    few = np.array([np.inf, np.inf, 3.0, np.nan, -np.inf, 1.0], dtype=dtype).reshape(1, 2, 3)
    _, stats = _check(torch.from_numpy(few).cuda(), few, (50.0, 90.0))      # ranks between 3 and inf, and between inf and inf: inf - inf is NaN
    assert stats[2] == 4.0 and np.isnan(stats[1])


def test_empty_foreground_then_reuse_of_the_workspace():
    """Through the C ABI with one caller-owned workspace, poisoned first: n == 0 gives zeros and NaN, and the next call on that workspace is right."""
    from afcm_amd import _lib
    lib = _lib.load()
    empty = torch.from_numpy(np.array([0.0, -1.0, np.nan, -0.0, -np.inf, 0.0], dtype=np.float32).reshape(1, 2, 3)).cuda()
    v = R.skewed_volume((3, 10, 12), np.float32, 9)
    dev = torch.from_numpy(v).cuda()
    nbytes = max(lib.afcm_rescale_workspace_bytes(6, _lib.SRC_F32), lib.afcm_rescale_workspace_bytes(v.size, _lib.SRC_F32))
    assert nbytes > 0
    workspace = torch.full((nbytes // 8 + 1,), -1, dtype=torch.int64, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream

    def run(t):
        out = torch.full(tuple(t.shape), 77, dtype=torch.uint8, device='cuda')
        stats = torch.full((3,), 5.0, dtype=torch.float64, device='cuda')
        rc = lib.afcm_rescale_intensity(out.data_ptr(), stats.data_ptr(), workspace.data_ptr(), t.data_ptr(), _lib.SRC_F32, *t.shape, t.stride(0), 0.005,
                                        0.995, stream)
        assert rc == 0
        return out.cpu().numpy(), stats.cpu().numpy()
    out, stats = run(empty)
    assert not out.any() and np.isnan(stats[:2]).all() and stats[2] == 0.0
    want, want_stats = R.rescale(v)
    for _ in range(2):                                                      # after the empty volume, and again: equal bits
        out, stats = run(dev)
        assert np.array_equal(out, want) and R.same_bits(stats, want_stats)
    out, stats = run(empty)
    assert not out.any() and np.isnan(stats[:2]).all() and stats[2] == 0.0


def test_out_is_honoured_and_nothing_else_is_written():
    from afcm_amd.intensity import rescale_intensity
    v = R.skewed_volume((3, 7, 37), np.int16, 10)
    dev = torch.from_numpy(v).cuda()
    buffer = torch.full((v.size + 40,), 99, dtype=torch.uint8, device='cuda')
    for at in (0, 5, 16):                                                   # an aligned output, one that starts 5 bytes in, and one a whole run in
        buffer.fill_(99)
        out = buffer[at:at + v.size].view(v.shape)
        got, stats = rescale_intensity(dev, (0.5, 99.5), out=out)
        assert got is out
        host = buffer.cpu().numpy()
        assert (host[:at] == 99).all() and (host[at + v.size:] == 99).all()
        want, want_stats = R.rescale(v)
        assert np.array_equal(host[at:at + v.size].reshape(v.shape), want) and R.same_bits(stats.cpu().numpy(), want_stats)
    again, _ = rescale_intensity(dev, (0.5, 99.5))
    assert torch.equal(again, out)


def test_golden_through_the_device_op():
    g = load_golden('I1_rescale_intensity')
    pair = tuple(g['percentiles'].tolist())
    from afcm_amd.torch_utils.ops.intensity_ops import rescale_intensity
    for dtype in R.DTYPES:
        name = np.dtype(dtype).name
        got = rescale_intensity(torch.from_numpy(g[f'volume_{name}']).cuda(), pair)[0].cpu().numpy()
        want = g[f'rescaled_{name}']
        if name != 'float32':
            assert np.array_equal(got, want), name
        else:                                                               # the reference stays in float32 there: one grey level at most, rarely
            diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
            share = float((diff > 0).mean())
            print(f'float32 golden: {int((diff > 0).sum())} of {diff.size} voxels differ from the reference')
            assert diff.max() <= 1 and share <= 1e-3 and share == float(g['float32_differing_share'])


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


def test_predict_volume_rescales_a_raw_source(monkeypatch):
    from afcm_amd.volume import predict_volume
    raw = R.skewed_volume((11, 30, 40), np.int16, 11)
    kw = dict(raw_internal_path_in='raw', thickness=5, patch_hw=(32, 32), batch_size=4, patch_halo=(0, 4, 4), heads=('prediction', 'input'))
    host = predict_volume(StubStep(), {'raw': raw}, where='host', rescale=(0.5, 99.5), **kw)
    copies = []
    _counting(monkeypatch, copies)
    dev = predict_volume(StubStep(), {'raw': raw}, where='device', rescale=(0.5, 99.5), **kw)
    monkeypatch.undo()
    assert copies == [], copies                                             # no device -> host copy, no scalar read
    for head in kw['heads']:
        assert dev[head].is_cuda and torch.equal(dev[head].cpu(), host[head])
    # the loop saw the rescaled volume: the same as rescaling on the host first and passing rescale=None
    pre = predict_volume(StubStep(), {'raw': R.rescale(raw)[0]}, where='device', **kw)
    plain = predict_volume(StubStep(), {'raw': raw}, where='device', **kw)
    assert torch.equal(pre['prediction'], dev['prediction']) and not torch.equal(plain['prediction'], dev['prediction'])


def test_slice_set_rescales_into_a_uint8_pool():
    from afcm_amd.data import SliceDataset
    from afcm_amd.training import DeviceSliceSet
    sources = [{'raw': R.skewed_volume(shape, dtype, seed)} for shape, dtype, seed in
               (((5, 20, 24), np.int16, 12), ((4, 33, 17), np.float32, 13), ((6, 16, 16), np.int16, 14))]
    ds = DeviceSliceSet(sources, phase='train', patch_shape=(1, 24, 24), thickness=[2, 3], rescale=(0.5, 99.5))
    assert ds.pool.dtype == torch.uint8 and ds.source_dtype == np.uint8
    want = [R.rescale(s['raw'])[0] for s in sources]
    assert np.array_equal(ds.pool.cpu().numpy(), np.concatenate([w.reshape(-1) for w in want]))
    items = ds.epoch_items(3)
    ds.load_epoch(items)
    got = ds.batch(0, len(ds))
    for g, w in zip(got, ds.host_batch(items, 0, len(ds), device='cpu')):
        assert torch.equal(g.cpu(), w)
    # ... and the host arm is SliceDataset on the rescaled volumes
    vol_a, vol_b, idx, t = items[0].tolist()
    item = SliceDataset({'raw': want[vol_b]}, phase='train', patch_shape=(1, 24, 24), stride_shape=(1, 1, 1), thickness=[t])[idx]
    assert torch.equal(got[0][0].cpu(), item['A']) and torch.equal(got[1][0].cpu(), item['B'])
    with pytest.raises(RuntimeError, match='mixed source dtypes'):
        DeviceSliceSet(sources, phase='train', patch_shape=(1, 24, 24), thickness=[2, 3])
