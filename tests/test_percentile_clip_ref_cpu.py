"""The percentile-clip normalisation without a GPU: the restatement of tests/percentile_clip_ref.py against numpy's own percentile and clip arithmetic
and against the golden captured from the reference function; the package's host arm against the restatement, bit for bit; the select's plan from the
library; the host-side argument checks of the device op; ``DeviceSliceSet(device=None, clip=...)``."""
import numpy as np
import pytest
import torch

import percentile_clip_ref as R
from conftest import load_golden

IDS = [np.dtype(t).name for t in R.DTYPES]


def _numpy_way(volume, pair, positive):
    """The reference's expression: numpy's percentile, clip, the division, the cast.  numpy forms b - a of two neighbouring order statistics in the
    array's own type before it widens, so a float32 volume is widened first (exactly), as the statement has it; the int16 volumes here stay as they
    are, since no two neighbours lie more than 32767 apart."""
    v_min, v_max = np.percentile(volume.astype(np.float64) if volume.dtype == np.float32 else volume, list(pair))
    if v_min < 0 and positive:
        v_min = 0
    with np.errstate(all='ignore'):
        x = (np.clip(volume, v_min, v_max) - v_min) / (v_max - v_min)
        x = x * 255
    return np.where(np.isnan(x), 0, x).astype(np.uint8), np.array([v_min, v_max], dtype=np.float64)


@pytest.mark.parametrize('dtype', R.DTYPES, ids=IDS)
def test_restatement_is_numpys_percentile_and_clip(dtype):
    rng = np.random.default_rng(1)
    for trial in range(60):
        shape = tuple(int(n) for n in rng.integers(1, 9, size=3))
        v = R.signed_volume(shape, dtype, 100 + trial)
        for pair in ((0.5, 99.5), (0.0, 100.0), tuple(sorted(rng.uniform(0, 100, size=2).tolist())), (50.0, 50.0)):
            for positive in (True, False):
                want, bounds = _numpy_way(v, pair, positive)
                got, stats = R.clip(v, pair, positive)
                assert R.same_stats(stats[:2], bounds) and stats[2] == v.size and stats[3] == 0.0, (trial, pair, positive)
                assert np.array_equal(got, want), (trial, pair, positive)


def test_restatement_equals_the_reference_golden():
    g = load_golden('I2_percentile_clip')
    pair = tuple(g['percentiles'].tolist())
    assert pair == (0.5, 99.5)
    for name in IDS:
        volume = g[f'volume_{name}']
        assert volume.shape == (8, 40, 40) and (volume == 0).mean() > 0.2
        assert name == 'uint8' or (volume < 0).mean() > 0.05
        for positive, tag in ((True, f'{name}_positive'), (False, f'{name}_signed')):
            got, stats = R.clip(volume, pair, positive)
            want = g[f'clipped_{tag}']
            assert R.same_stats(stats[:2], g[f'bounds_{tag}']), tag
            assert name == 'uint8' or positive or stats[0] < 0
            share = float(g[f'differing_share_{tag}'])
            diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
            if share == 0.0:
                assert np.array_equal(got, want), tag
            else:                                           # another numpy kept float32 when the golden was captured: the recorded share, one level
                assert float((diff > 0).mean()) <= share and diff.max() <= 1, tag
    assert all(float(g[f'differing_share_{name}_{kind}']) == 0.0 for name in IDS for kind in ('positive', 'signed'))


@pytest.mark.parametrize('dtype', R.DTYPES, ids=IDS)
def test_host_arm_equals_the_restatement(dtype):
    from afcm_amd.intensity import percentile_clip, percentile_clip_host
    for shape, seed, pair in (((3, 5, 7), 1, (0.5, 99.5)), ((2, 33, 65), 2, (0.5, 99.5)), ((4, 9, 11), 3, (0.0, 100.0)), ((4, 9, 11), 4, (37.5, 37.5)),
                              ((1, 1, 1), 5, (0.5, 99.5)), ((2, 7, 9), 6, (0.0, 30.0))):
        v = R.signed_volume(shape, dtype, seed)
        for positive in (True, False):
            got, stats = percentile_clip_host(v, pair, positive)
            want, want_stats = R.clip(v, pair, positive)
            assert got.dtype == np.uint8 and got.shape == v.shape and np.array_equal(got, want) and R.same_stats(stats, want_stats)
    again, _ = percentile_clip(v, pair, False)                              # the dispatcher: an array goes to the host arm
    assert np.array_equal(again, got)
    other = R.signed_volume((3, 4, 5), np.int16, 7)                         # the bounds of another volume, of another shape and dtype
    got, stats = percentile_clip_host(v, (10.0, 90.0), True, reference=other)
    want, want_stats = R.clip(v, (10.0, 90.0), True, reference=other)
    assert np.array_equal(got, want) and R.same_stats(stats, want_stats) and stats[2] == other.size


def test_nan_zeros_ties_and_non_finite_values():
    from afcm_amd.intensity import percentile_clip_host
    for fn in (R.clip, percentile_clip_host):
        for at, nan in ((0, np.nan), (11, np.nan), (5, -np.nan)):
            v = np.arange(12, dtype=np.float32).reshape(1, 3, 4) - 4
            v.reshape(-1)[at] = nan
            out, stats = fn(v)
            assert not out.any() and np.isnan(stats[:2]).all() and stats[2:].tolist() == [12.0, 1.0]
        constant = np.full((2, 3, 4), -7, dtype=np.int16)
        out, stats = fn(constant, (0.5, 99.5), False)
        assert stats.tolist() == [-7.0, -7.0, 24.0, 0.0] and not out.any()      # hi == lo: 0 / 0 -> 0
        out, stats = fn(constant)                                               # lo raised to 0 above hi = -7: min(max(v, 0), -7) = -7, (-7 - 0) / (-7 - 0) = 1
        assert stats.tolist() == [0.0, -7.0, 24.0, 0.0] and (out == 255).all()
        denormal = np.float64(5e-324)
        v = np.array([-np.inf, np.inf, -0.0, 0.0, denormal, -denormal, 1.0, 2.0, 3.0, 4.0, 6.0]).reshape(1, 1, 11)
        out, stats = fn(v, (0.0, 100.0), False)                                 # a = -inf, d = b - a = inf, a + d * 0 = NaN: by IEEE, no special case
        assert np.isnan(stats[:2]).all() and stats[3] == 0.0 and not out.any()
        out, stats = fn(np.array([-4.0, 1.0, 2.0, 5.0, np.inf]).reshape(1, 1, 5), (25.0, 80.0), False)
        assert stats[:2].tolist() == [1.0, np.inf] and not out.any()            # hi = 5 + inf * 0.2; finite / inf = 0, inf / inf = NaN -> 0
        out, stats = fn(v, (45.0, 80.0), True)                                  # ranks 4.5 and 8: halfway from the denormal to 1, and 4
        assert stats[:2].tolist() == [0.5, 4.0] and out.reshape(-1).tolist() == [0, 255, 0, 0, 0, 0, 36, 109, 182, 255, 255]
        out, stats = fn(v, (20.0, 20.0), False)                                 # rank 2: a zero, whichever sign it carries
        assert stats[0] == 0.0 and stats[1] == 0.0 and not out.any()
        out, stats = fn(v, (10.0, 40.0), True)                                  # -denormal < 0 is raised to 0; hi is the denormal
        assert stats[:2].tolist() == [0.0, float(denormal)] and out.reshape(-1).tolist() == [0, 255, 0, 0, 255, 0, 255, 255, 255, 255, 255]
    v = np.array([np.inf, 2.0, 1.0, -3.0, 7.0, -1.0], dtype=np.float32).reshape(1, 2, 3)
    a, b = R.clip(v, (25.0, 60.0)), percentile_clip_host(v, (25.0, 60.0))
    assert np.array_equal(a[0], b[0]) and R.same_stats(a[1], b[1])
    clean = np.array([1.0, 2.0, 3.0, 4.0], dtype=np.float32).reshape(1, 2, 2)   # a NaN voxel under finite bounds (the reference is another volume): 0
    v = np.array([np.nan, 0.0, 2.5, 9.0], dtype=np.float32).reshape(1, 2, 2)
    for fn in (R.clip, percentile_clip_host):
        out, stats = fn(v, (0.0, 100.0), True, reference=clean)
        assert stats.tolist() == [1.0, 4.0, 4.0, 0.0] and out.reshape(-1).tolist() == [0, 0, 127, 255]


def test_plan_from_the_library():
    """Pure host calls into the library: the plan, the workspace size, and the argument checks that return before any launch."""
    from afcm_amd import _lib
    from afcm_amd.torch_utils.ops.intensity_ops import percentile_plan, rescale_plan
    lib = _lib.load()
    codes = {torch.uint8: _lib.SRC_U8, torch.int16: _lib.SRC_I16, torch.float32: _lib.SRC_F32, torch.float64: _lib.SRC_F64}
    for dtype, passes in ((torch.uint8, 1), (torch.int16, 2), (torch.float32, 4), (torch.float64, 8)):
        small, large = percentile_plan(1, dtype), percentile_plan(2 ** 31 - 1, dtype)
        assert small['bits'] == large['bits'] == (8,) * passes and small['passes'] == passes       # int16: two 8-bit digits; float64: eight
        assert small['groups'] == 1 and large['groups'] >= 2 and small['chunk'] == large['chunk'] == rescale_plan(1, dtype)['chunk']
        assert percentile_plan(large['chunk'] + 1, dtype)['groups'] == 2
        assert 0 < lib.afcm_percentile_workspace_bytes(1, codes[dtype]) <= lib.afcm_percentile_workspace_bytes(2 ** 31 - 1, codes[dtype]) < 64 << 20
    assert rescale_plan(77, torch.int16)['bits'] == (15,)                                          # the foreground select keeps its plan
    assert lib.afcm_percentile_workspace_bytes(2 ** 31, _lib.SRC_U8) == 0 and lib.afcm_percentile_workspace_bytes(8, 7) == 0
    assert lib.afcm_percentile_workspace_bytes(0, _lib.SRC_F32) == 0 and lib.afcm_percentile_workspace_bytes(8, -1) == 0
    with pytest.raises(RuntimeError, match='2\\^31'):
        percentile_plan(2 ** 31, torch.uint8)
    with pytest.raises(RuntimeError, match='uint8 / int16'):
        percentile_plan(8, torch.int32)
    p, u8 = 4096, _lib.SRC_U8                                              # a non-null stand-in: these calls return before touching any pointer
    for args, text in (((0, p, p, u8, 2, 3, 4, 12, 0.005, 0.995, 1, None), b'null'), ((p, 0, p, u8, 2, 3, 4, 12, 0.005, 0.995, 1, None), b'null'),
                       ((p, p, 0, u8, 2, 3, 4, 12, 0.005, 0.995, 1, None), b'null'), ((p, p, p, 9, 2, 3, 4, 12, 0.005, 0.995, 1, None), b'dtype'),
                       ((p, p, p, u8, 2, 0, 4, 12, 0.005, 0.995, 1, None), b'positive'),
                       ((p, p, p, u8, 2048, 1024, 1024, 1 << 20, 0.005, 0.995, 1, None), b'2^31'),
                       ((p, p, p, u8, 2, 3, 4, -12, 0.005, 0.995, 1, None), b'negative'), ((p, p, p, u8, 2, 3, 4, 12, 0.6, 0.5, 1, None), b'fractions'),
                       ((p, p, p, u8, 2, 3, 4, 12, 0.5, 1.5, 0, None), b'fractions'), ((p, p, p, u8, 2, 3, 4, 12, float('nan'), 0.5, 1, None), b'fractions'),
                       ((p + 4, p, p, u8, 2, 3, 4, 12, 0.005, 0.995, 1, None), b'aligned'), ((p, p + 4, p, u8, 2, 3, 4, 12, 0.005, 0.995, 1, None), b'aligned')):
        assert lib.afcm_percentile_bounds(*args) == _lib.E_INVALID and text in lib.afcm_last_error() and b'percentile_bounds' in lib.afcm_last_error(), args
    for args, text in (((0, p, p, u8, 2, 3, 4, 12, None), b'null'), ((p, 0, p, u8, 2, 3, 4, 12, None), b'null'), ((p, p, 0, u8, 2, 3, 4, 12, None), b'null'),
                       ((p, p, p, -1, 2, 3, 4, 12, None), b'dtype'), ((p, p, p, u8, 2, 3, 0, 12, None), b'positive'),
                       ((p, p, p, u8, 2048, 1024, 1024, 1 << 20, None), b'2^31'), ((p, p, p, u8, 2, 3, 4, -1, None), b'negative'),
                       ((p, p + 4, p, u8, 2, 3, 4, 12, None), b'aligned')):
        assert lib.afcm_clip_normalize(*args) == _lib.E_INVALID and text in lib.afcm_last_error() and b'clip_normalize' in lib.afcm_last_error(), args


def test_host_side_argument_checks():
    from afcm_amd.intensity import percentile_clip, percentile_clip_host
    from afcm_amd.torch_utils.ops import intensity_ops
    ok = torch.zeros(2, 3, 4, dtype=torch.int16)
    for bad, match in ((torch.zeros(2, 3, 4, dtype=torch.int32), 'uint8 / int16 / float32 / float64'), (torch.zeros(3, 4, dtype=torch.uint8), r'\[D, H, W\]'),
                       (torch.zeros(2, 3, 8, dtype=torch.float32)[:, :, ::2], 'rows of the source must be contiguous'),
                       (torch.zeros(2, 6, 4, dtype=torch.float32)[:, ::2], 'rows of the source must be contiguous'),
                       (torch.zeros(0, 3, 4, dtype=torch.uint8), 'between 1 and')):
        with pytest.raises(RuntimeError, match=match):
            intensity_ops.percentile_clip(bad)
        with pytest.raises(RuntimeError, match=match):
            intensity_ops.percentile_bounds(bad, (0.5, 99.5))
        with pytest.raises(RuntimeError, match=match):
            intensity_ops.percentile_clip(ok, reference=bad)
    for pair in ((-1.0, 50.0), (60.0, 50.0), (0.0, 100.5), (float('nan'), 50.0), (1.0,), 5.0):
        with pytest.raises(RuntimeError, match='percentiles'):
            intensity_ops.percentile_clip(ok, pair)
        with pytest.raises(RuntimeError, match='percentiles'):
            intensity_ops.percentile_bounds(ok, pair)
        with pytest.raises(RuntimeError, match='percentiles'):
            percentile_clip_host(ok.numpy(), pair)
    for out, match in ((torch.zeros(2, 3, 5, dtype=torch.uint8), 'out must be'), (torch.zeros(2, 3, 4, dtype=torch.int16), 'out must be'),
                       (torch.zeros(2, 3, 8, dtype=torch.uint8)[:, :, ::2], 'out must be'), (torch.zeros(2, 3, 4, dtype=torch.uint8, device='meta'), 'out is on')):
        with pytest.raises(RuntimeError, match=match):
            intensity_ops.percentile_clip(ok, out=out)
    with pytest.raises(RuntimeError, match='reference is on'):
        intensity_ops.percentile_clip(ok, reference=torch.zeros(2, 3, 4, dtype=torch.int16, device='meta'))
    with pytest.raises(RuntimeError, match='no CPU'):                       # every argument in order, but a host tensor
        intensity_ops.percentile_clip(ok, out=torch.zeros(2, 3, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='no CPU'):
        intensity_ops.percentile_bounds(ok, (0.5, 99.5))
    with pytest.raises(RuntimeError, match='no CPU'):
        percentile_clip(ok)
    with pytest.raises(RuntimeError, match='numpy array or a device tensor'):
        percentile_clip([[1, 2]])
    with pytest.raises(RuntimeError, match='out= is for device tensors'):
        percentile_clip(ok.numpy(), out=torch.zeros(2, 3, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match=r'\[D, H, W\]'):
        percentile_clip_host(np.zeros((3, 4)))
    with pytest.raises(RuntimeError, match='uint8 / int16'):
        percentile_clip_host(np.zeros((2, 3, 4), dtype=np.uint16))
    with pytest.raises(RuntimeError, match='reference'):
        percentile_clip_host(np.zeros((2, 3, 4)), reference=np.zeros((3, 4)))


def test_clip_and_rescale_exclude_each_other():
    from afcm_amd.training import DeviceSliceSet
    from afcm_amd.volume import predict_volume
    raw = R.signed_volume((5, 20, 24), np.int16, 12)
    with pytest.raises(ValueError, match='rescale= and clip='):
        predict_volume(None, {'raw': raw}, raw_internal_path_in='raw', thickness=2, patch_hw=(24, 24), batch_size=2, where='host', rescale=(0.5, 99.5),
                       clip=(0.5, 99.5))
    with pytest.raises(RuntimeError, match='percentiles'):
        predict_volume(None, {'raw': raw}, raw_internal_path_in='raw', thickness=2, patch_hw=(24, 24), batch_size=2, where='host', clip=(70.0, 30.0))
    with pytest.raises(RuntimeError, match='rescale= and clip='):
        DeviceSliceSet([{'raw': raw}], phase='train', patch_shape=(1, 24, 24), thickness=[2], device=None, rescale=(0.5, 99.5), clip=(0.5, 99.5))


def test_slice_set_tables_with_clip():
    from afcm_amd.data import SliceDataset
    from afcm_amd.training import DeviceSliceSet
    sources = [{'raw': R.signed_volume(shape, dtype, seed)} for shape, dtype, seed in
               (((5, 20, 24), np.int16, 12), ((4, 33, 17), np.float32, 13), ((6, 16, 16), np.float64, 14))]
    with pytest.raises(RuntimeError, match='mixed source dtypes'):
        DeviceSliceSet(sources, phase='train', patch_shape=(1, 24, 24), thickness=[2, 3], device=None)
    with pytest.raises(RuntimeError, match='percentiles'):
        DeviceSliceSet(sources, phase='train', patch_shape=(1, 24, 24), thickness=[2, 3], device=None, clip=(70.0, 30.0))
    ds = DeviceSliceSet(sources, phase='train', patch_shape=(1, 24, 24), thickness=[2, 3], device=None, clip=(0.5, 99.5))
    assert ds.source_dtype == np.uint8 and len(ds) == 15 and ds.pool is None and ds.clip == (0.5, 99.5) and ds.rescale is None
    items = ds.epoch_items(3)
    a, b, c = ds.host_batch(items, 0, 15)
    for row, (vol_a, vol_b, idx, t) in enumerate(items.tolist()):
        item = SliceDataset({'raw': R.clip(sources[vol_b]['raw'])[0]}, phase='train', patch_shape=(1, 24, 24), stride_shape=(1, 1, 1), thickness=[t])[idx]
        assert torch.equal(a[row], item['A']) and torch.equal(b[row], item['B']) and c[row].item() == item['slice_idx'][0]
    plain = DeviceSliceSet(sources[:1], phase='train', patch_shape=(1, 24, 24), thickness=[2, 3], device=None)      # neither: as before
    assert plain.source_dtype == np.int16 and plain.rescale is None and plain.clip is None
