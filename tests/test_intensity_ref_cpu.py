"""The intensity rescaling without a GPU: the restatement of tests/intensity_ref.py against numpy's own percentile and against the golden captured
from the reference function; the package's host arm against the restatement; the rules for an empty foreground, ties and non-finite values; the
host-side argument checks of the device op; the select's plan; ``DeviceSliceSet(device=None, rescale=...)``."""
import numpy as np
import pytest
import torch

import intensity_ref as R
from conftest import load_golden


@pytest.mark.parametrize('dtype', [np.int16, np.uint8, np.float64], ids=['int16', 'uint8', 'float64'])
def test_restated_percentile_is_numpys_bit_for_bit(dtype):
    rng = np.random.default_rng(1)
    for trial in range(300):
        n = int(rng.integers(1, 400))
        a = (rng.gamma(2.0, 40.0, n) + 1).astype(dtype) if dtype != np.float64 else rng.gamma(2.0, 40.0, n) + 1e-3
        a = np.maximum(a, 1).astype(dtype) if dtype != np.float64 else a
        s = np.sort(a.astype(np.float64))
        for q in (0.5, 99.5, float(rng.uniform(0, 100)), 0.0, 100.0, 50.0):
            want = np.percentile(a, q)
            assert R.same_bits(R.percentile(s, q), np.float64(want)), (trial, n, q)


def test_restatement_equals_the_reference_golden():
    g = load_golden('I1_rescale_intensity')
    pair = tuple(g['percentiles'].tolist())
    assert pair == (0.5, 99.5)
    for name in ('uint8', 'int16', 'float64'):
        volume = g[f'volume_{name}']
        assert volume.shape == (8, 40, 40) and 0.3 < np.mean(volume <= 0) < 0.5
        assert np.array_equal(R.rescale(volume, pair)[0], g[f'rescaled_{name}']), name
    assert (g['volume_int16'] < 0).sum() > 0 and (g['volume_float32'] < 0).sum() > 0
    # float32: the reference stays in float32 (numpy keeps the array's type), the statement is float64: one grey level at most, at a small share
    got, want = R.rescale(g['volume_float32'], pair)[0], g['rescaled_float32']
    diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
    share = float((diff > 0).mean())
    assert diff.max() <= 1 and share <= 1e-3
    assert share == float(g['float32_differing_share']) and int(diff.max()) == int(g['float32_largest_difference'])


@pytest.mark.parametrize('dtype', R.DTYPES, ids=[np.dtype(t).name for t in R.DTYPES])
def test_host_arm_equals_the_restatement(dtype):
    from afcm_amd.intensity import rescale_intensity, rescale_intensity_host
    for shape, seed, pair in (((3, 5, 7), 1, (0.5, 99.5)), ((2, 33, 65), 2, (0.5, 99.5)), ((4, 9, 11), 3, (0.0, 100.0)), ((4, 9, 11), 4, (37.5, 37.5)),
                              ((1, 1, 1), 5, (0.5, 99.5))):
        v = R.skewed_volume(shape, dtype, seed)
        got, stats = rescale_intensity_host(v, pair)
        want, want_stats = R.rescale(v, pair)
        assert got.dtype == np.uint8 and np.array_equal(got, want) and R.same_bits(stats, want_stats)
    again, _ = rescale_intensity(v, pair)                                   # the dispatcher: an array goes to the host arm
    assert np.array_equal(again, got)
    values = np.zeros(77, dtype=dtype)
    values[:67] = R.keys_to_values(R.digit_keys((8,) if dtype == np.uint8 else (15,)), dtype)
    v = values.reshape(1, 7, 11)
    for q in R.rank_sweep(67)[::7]:
        got, stats = rescale_intensity_host(v, (min(q, 100 - q), max(q, 100 - q)))
        want, want_stats = R.rescale(v, (min(q, 100 - q), max(q, 100 - q)))
        assert np.array_equal(got, want) and R.same_bits(stats, want_stats)


def test_empty_foreground_ties_and_non_finite_values():
    from afcm_amd.intensity import rescale_intensity_host
    for fn in (R.rescale, rescale_intensity_host):
        out, stats = fn(np.array([0.0, -1.0, np.nan, -0.0, -np.inf], dtype=np.float32).reshape(1, 1, 5))
        assert not out.any() and np.isnan(stats[:2]).all() and stats[2] == 0.0                  # n == 0: zeros, NaN, nothing raised
        constant = np.zeros((2, 3, 4), dtype=np.int16)
        constant[0] = 300
        out, stats = fn(constant)
        assert stats.tolist() == [300.0, 300.0, 12.0] and (out[0] == 1).all() and not out[1].any()   # hi == lo: 0 / 0 -> 1
        full = np.full((1, 2, 3), 255, dtype=np.uint8)
        assert (fn(full)[0] == 1).all()
        denormal = np.float64(5e-324)
        v = np.array([np.nan, -np.inf, np.inf, -0.0, denormal, -2.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0]).reshape(1, 3, 4)
        out, stats = fn(v, (0.0, 50.0))
        assert stats[2] == 8.0 and stats[0] == denormal and stats[1] == 3.5
        assert out.reshape(-1).tolist() == [0, 0, 255, 0, 1, 0, 73, 146, 219, 255, 255, 255]
        out, stats = fn(v, (0.0, 100.0))                                   # a = b = +inf: d = inf - inf, so hi is NaN and every level NaN -> 1
        assert np.isnan(stats[1]) and out.reshape(-1).tolist() == [0, 0, 1, 0, 1, 0, 1, 1, 1, 1, 1, 1]
        few = np.array([np.inf, np.inf, 3.0, 1.0], dtype=np.float32).reshape(1, 2, 2)
        out, stats = fn(few, (50.0, 90.0))                                 # inf - inf inside the interpolation: NaN, by IEEE, no special case
        assert np.isnan(stats[:2]).all() and (out == 1).all()
    for v, pair in ((np.array([np.inf, 2.0, 1.0, np.nan, 7.0, -1.0], dtype=np.float32).reshape(1, 2, 3), (25.0, 60.0)),):
        a, b = R.rescale(v, pair), rescale_intensity_host(v, pair)
        assert np.array_equal(a[0], b[0]) and R.same_bits(a[1], b[1])


def test_host_side_argument_checks():
    from afcm_amd.intensity import rescale_intensity, rescale_intensity_host
    from afcm_amd.torch_utils.ops import intensity_ops
    ok = torch.zeros(2, 3, 4, dtype=torch.int16)
    for bad, match in ((torch.zeros(2, 3, 4, dtype=torch.int32), 'uint8 / int16 / float32 / float64'), (torch.zeros(3, 4, dtype=torch.uint8), r'\[D, H, W\]'),
                       (torch.zeros(2, 3, 8, dtype=torch.float32)[:, :, ::2], 'rows of the source must be contiguous'),
                       (torch.zeros(2, 6, 4, dtype=torch.float32)[:, ::2], 'rows of the source must be contiguous'),
                       (torch.zeros(0, 3, 4, dtype=torch.uint8), 'between 1 and')):
        with pytest.raises(RuntimeError, match=match):
            intensity_ops.rescale_intensity(bad)
    for pair in ((-1.0, 50.0), (60.0, 50.0), (0.0, 100.5), (float('nan'), 50.0), (1.0,), 5.0):
        with pytest.raises(RuntimeError, match='percentiles'):
            intensity_ops.rescale_intensity(ok, pair)
        with pytest.raises(RuntimeError, match='percentiles'):
            rescale_intensity_host(ok.numpy(), pair)
    for out, match in ((torch.zeros(2, 3, 5, dtype=torch.uint8), 'out must be'), (torch.zeros(2, 3, 4, dtype=torch.int16), 'out must be'),
                       (torch.zeros(2, 3, 8, dtype=torch.uint8)[:, :, ::2], 'out must be'), (torch.zeros(2, 3, 4, dtype=torch.uint8, device='meta'), 'out is on')):
        with pytest.raises(RuntimeError, match=match):
            intensity_ops.rescale_intensity(ok, out=out)
    with pytest.raises(RuntimeError, match='no CPU'):                       # every argument in order, but a host tensor
        intensity_ops.rescale_intensity(ok, out=torch.zeros(2, 3, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='no CPU'):
        rescale_intensity(ok)
    with pytest.raises(RuntimeError, match='numpy array or a device tensor'):
        rescale_intensity([[1, 2]])
    with pytest.raises(RuntimeError, match=r'\[D, H, W\]'):
        rescale_intensity_host(np.zeros((3, 4)))
    with pytest.raises(RuntimeError, match='uint8 / int16'):
        rescale_intensity_host(np.zeros((2, 3, 4), dtype=np.uint16))


def test_plan_and_c_level_checks():
    """Pure host calls into the library: the plan, the workspace size, and the argument checks that return before any launch."""
    from afcm_amd import _lib
    from afcm_amd.torch_utils.ops.intensity_ops import rescale_plan
    lib = _lib.load()
    want_bits = {torch.uint8: (8,), torch.int16: (15,), torch.float32: 31, torch.float64: 63}
    for dtype, bits in want_bits.items():
        small, large = rescale_plan(1, dtype), rescale_plan(2 ** 31 - 1, dtype)
        assert small['groups'] == 1 and large['groups'] >= 2 and small['chunk'] == large['chunk'] >= 64
        assert small['passes'] == len(small['bits']) == large['passes'] and sum(small['bits']) == (bits if isinstance(bits, int) else sum(bits))
        assert (small['passes'] == 1) == (dtype in (torch.uint8, torch.int16))                  # 8- and 16-bit sources: one histogram pass
        assert rescale_plan(large['chunk'] + 1, dtype)['groups'] == 2
        code = {torch.uint8: _lib.SRC_U8, torch.int16: _lib.SRC_I16, torch.float32: _lib.SRC_F32, torch.float64: _lib.SRC_F64}[dtype]
        assert 0 < lib.afcm_rescale_workspace_bytes(1, code) <= lib.afcm_rescale_workspace_bytes(2 ** 31 - 1, code) < 64 << 20
    assert lib.afcm_rescale_workspace_bytes(2 ** 31, _lib.SRC_U8) == 0 and lib.afcm_rescale_workspace_bytes(8, 7) == 0
    with pytest.raises(RuntimeError, match='2\\^31'):
        rescale_plan(2 ** 31, torch.uint8)
    p = 4096                                                               # a non-null stand-in: these calls return before touching any pointer
    for args, text in (((0, p, p, p, _lib.SRC_U8, 2, 3, 4, 12, 0.005, 0.995, None), b'null'), ((p, p, p, p, 9, 2, 3, 4, 12, 0.005, 0.995, None), b'dtype'),
                       ((p, p, p, p, _lib.SRC_U8, 2, 0, 4, 12, 0.005, 0.995, None), b'positive'),
                       ((p, p, p, p, _lib.SRC_U8, 2048, 1024, 1024, 1 << 20, 0.005, 0.995, None), b'2^31'),
                       ((p, p, p, p, _lib.SRC_U8, 2, 3, 4, -12, 0.005, 0.995, None), b'negative'),
                       ((p, p, p, p, _lib.SRC_U8, 2, 3, 4, 12, 0.6, 0.5, None), b'fractions'), ((p, p, p, p, _lib.SRC_U8, 2, 3, 4, 12, 0.5, 1.5, None), b'fractions'),
                       ((p, p, p, p, _lib.SRC_U8, 2, 3, 4, 12, float('nan'), 0.5, None), b'fractions'),
                       ((p, p, p + 4, p, _lib.SRC_U8, 2, 3, 4, 12, 0.005, 0.995, None), b'aligned')):
        assert lib.afcm_rescale_intensity(*args) == _lib.E_INVALID and text in lib.afcm_last_error(), args


def test_slice_set_tables_with_rescale():
    from afcm_amd.data import SliceDataset
    from afcm_amd.training import DeviceSliceSet
    sources = [{'raw': R.skewed_volume(shape, dtype, seed)} for shape, dtype, seed in
               (((5, 20, 24), np.int16, 12), ((4, 33, 17), np.float32, 13), ((6, 16, 16), np.int16, 14))]
    with pytest.raises(RuntimeError, match='mixed source dtypes'):
        DeviceSliceSet(sources, phase='train', patch_shape=(1, 24, 24), thickness=[2, 3], device=None)
    with pytest.raises(RuntimeError, match='percentiles'):
        DeviceSliceSet(sources, phase='train', patch_shape=(1, 24, 24), thickness=[2, 3], device=None, rescale=(70.0, 30.0))
    ds = DeviceSliceSet(sources, phase='train', patch_shape=(1, 24, 24), thickness=[2, 3], device=None, rescale=(0.5, 99.5))
    assert ds.source_dtype == np.uint8 and len(ds) == 15 and ds.pool is None
    assert ds.vols_host.tolist() == [[0, 5, 20, 24], [2400, 4, 33, 17], [2400 + 2244, 6, 16, 16]]
    items = ds.epoch_items(3)
    a, b, c = ds.host_batch(items, 0, 15)
    for row, (vol_a, vol_b, idx, t) in enumerate(items.tolist()):
        item = SliceDataset({'raw': R.rescale(sources[vol_b]['raw'])[0]}, phase='train', patch_shape=(1, 24, 24), stride_shape=(1, 1, 1), thickness=[t])[idx]
        assert torch.equal(a[row], item['A']) and torch.equal(b[row], item['B']) and c[row].item() == item['slice_idx'][0]
    plain = DeviceSliceSet(sources[:1], phase='train', patch_shape=(1, 24, 24), thickness=[2, 3], device=None)      # rescale=None: as before
    assert plain.source_dtype == np.int16 and plain.rescale is None
