"""The per-plane normalisers on the GPU (csrc/normalise.hip): the coefficients of ``afcm_slice_norm_stats`` / ``afcm_plane_norm_stats`` against
``afcm_amd.normalise.plane_record`` on the same planes, bit for bit (a NaN matching a NaN), and the launches that apply them against the host arm
-- ``DeviceSliceSet.host_batch(normalise=)``, ``SliceDataset(normalise=)``, ``predict_volume(where='host')`` -- with ``torch.equal``.  The shapes
are the smallest at which the kernels can go wrong: planes of fewer pixels than the workgroup has threads, ragged strided partials, sources that
are padded in one axis and cropped in the other, thick-slice planes outside the volume at both ends, 256 r + 1 pixels for the seams of the
summation order, and the select's edge cases of tests/normalise_ref.py."""
import numpy as np
import pytest
import torch

import normalise_ref as N
import train_batch_ref as T
import volume_ref as R
from afcm_amd import augment as A
from afcm_amd.data import SliceDataset, crop_to_fixed
from afcm_amd.normalise import NormaliseConfig, plane_record

pytestmark = pytest.mark.gpu

PERCENTILE = NormaliseConfig(percentile=(1, 99.6))
MINMAX = NormaliseConfig(percentile=(0, 100))
STANDARD = NormaliseConfig(standardize=True)
FIXED = NormaliseConfig(standardize=(100.0, 40.0))
MODES = {'percentile': PERCENTILE, 'minmax': MINMAX, 'standardize': STANDARD, 'fixed': FIXED}
# (patch, source [Hs, Ws]): cropped in both axes; padded in y and cropped in x; padded in both (zeros in the statistics); padded in y, cropped in x
GEOMETRIES = (((5, 7), (13, 20)), ((16, 16), (13, 20)), ((33, 47), (20, 13)), ((64, 64), (40, 70)))


def _slice_stats(volume, first, count, hw, thickness, k, config):
    from afcm_amd.torch_utils.ops.normalise_ops import slice_norm_stats
    return slice_norm_stats(volume, first, count, hw, thickness, k, config)


def _plane_coef(plane, config):
    """The device's coefficients of one [h, w] plane: a volume of depth 1, one slice, k = 1."""
    h, w = plane.shape
    return _slice_stats(torch.from_numpy(np.ascontiguousarray(plane[None])).cuda(), 0, 1, (h, w), None, 1, config)[0, 0]


def _item_planes(volume, idx, thickness, k, hw):
    """The k item planes of target ``idx``: the centred crop / zero pad of the source slice, float64 zeros outside the volume."""
    cropped = crop_to_fixed(volume, hw)
    return [cropped[pos] if 0 <= pos <= volume.shape[0] - 1 else np.zeros(hw) for pos in N.positions(idx, thickness, k)]


def _want_slices(volume, first, count, thickness, k, hw, config):
    return np.array([[plane_record(p, config) for p in _item_planes(volume, first + i, thickness, k, hw)] for i in range(count)])


@pytest.mark.parametrize('dtype', N.DTYPES)
def test_select_edge_cases(dtype):
    """Every rank of 67 keys that differ in every digit, neighbouring ranks across a bin boundary of each pass, ties, an all-equal plane, pmin 0 /
    pmax 100, +-inf, -0.0 and denormals, one NaN anywhere, the int16 sign seam: all four doubles of every case, against the host arm and against
    the slow restatement."""
    got, want, names = [], [], []
    for name, (plane, pairs) in N.select_cases(dtype).items():
        for pair in pairs:
            config = NormaliseConfig(percentile=pair)
            got.append(_plane_coef(plane, config))
            want.append(plane_record(plane, config))
            assert N.same_bits(want[-1], N.record(plane, percentile_pair=pair))
            names.append((name, pair))
    got = torch.stack(got).cpu().numpy()
    assert len(names) > 40
    for g, w, name in zip(got, want, names):
        assert N.same_bits(g, w), (name, g, w)
    nan_cases = [i for i, (name, _) in enumerate(names) if name.startswith('nan_at')]
    assert (len(nan_cases) == 3 and all(np.isnan(got[i]).all() for i in nan_cases)) if np.dtype(dtype).kind == 'f' else not nan_cases


@pytest.mark.parametrize('k', [4, 1])
@pytest.mark.parametrize('dtype', N.DTYPES)
def test_slice_coefficients_over_shapes_crops_pads_and_zero_planes(dtype, k):
    """A run of 7 target slices with thickness 2: with k = 4 the planes at idx_a - 2 (targets 0, 1) and idx_a + 2, idx_a + 4 (targets 4 ... 6) lie
    outside the volume.  Every mode, every geometry, coefficients with torch.equal where no NaN is involved; a second launch gives the same bits."""
    for hw, source_hw in GEOMETRIES:
        src = R.source((7,) + source_hw, dtype, seed=hw[0] + k)
        volume = torch.from_numpy(src).cuda()
        for name, config in MODES.items():
            got = _slice_stats(volume, 0, 7, hw, 2 if k == 4 else None, k, config)
            want = torch.from_numpy(_want_slices(src, 0, 7, 2, k, hw, config))
            assert got.shape == (7, k, 4) and torch.equal(got.cpu(), want), (hw, name)
            assert torch.equal(_slice_stats(volume, 0, 7, hw, 2 if k == 4 else None, k, config), got)
            part = _slice_stats(volume, 3, 2, hw, 2 if k == 4 else None, k, config)              # a run that starts inside the volume
            assert torch.equal(part, got[3:5])
        if k == 4:                                                                                # a plane of zeros: sub 0 or the mean, div from eps
            eps = 1e-10
            zero = _slice_stats(volume, 0, 7, hw, 2, 4, PERCENTILE).cpu()
            assert torch.equal(zero[0, 0], torch.tensor([0.0, eps, 0.0, 0.0], dtype=torch.float64)) and torch.equal(zero[6, 3], zero[0, 0])
            zero = _slice_stats(volume, 0, 7, hw, 2, 4, STANDARD).cpu()
            assert torch.equal(zero[6, 2], torch.tensor([0.0, eps, 0.0, 0.0], dtype=torch.float64))


def test_standardize_seams_given_moments_and_small_std():
    """Planes of 256 r + 1 pixels: one strided partial is a term longer than the other 255.  Then two given floats, and a std below eps."""
    rng = np.random.default_rng(5)
    for h, w in ((1, 257), (27, 19), (25, 41), (1, 255), (16, 16)):
        for dtype in (np.float64, np.float32, np.int16):
            plane = (rng.standard_normal((h, w)) * 300 + 100).astype(dtype)
            got = _plane_coef(plane, STANDARD).cpu().numpy()
            assert N.same_bits(got, plane_record(plane, STANDARD)) and N.same_bits(got, N.record(plane, standardize=True)), (h, w, dtype)
    plane = np.full((5, 7), 3.0)
    plane[0, 0] = 3.0 + 1e-11                                                                     # a standard deviation of 1.7e-12: below eps
    got = _plane_coef(plane, STANDARD).cpu().numpy()
    assert N.same_bits(got, plane_record(plane, STANDARD)) and 0.0 < got[3] < 1e-10 and got[1] == 1e-10
    for config in (FIXED, NormaliseConfig(standardize=(3.0, 1e-12)), NormaliseConfig(standardize=(0.5, 2.0), eps=4.0)):
        assert N.same_bits(_plane_coef(plane, config).cpu().numpy(), plane_record(plane, config))
    holed = plane.copy()
    holed[2, 3] = np.nan
    assert np.isnan(_plane_coef(holed, STANDARD).cpu().numpy()).all()


def _set(dtype, hw, k, config, augment=None, then_range=False, **kw):
    from afcm_amd.training import DeviceSliceSet
    lo, hi = (0.0, 1.0) if then_range else T.value_range(dtype)
    return DeviceSliceSet(T.subjects(dtype), patch_shape=(1,) + hw, raw_internal_path_in=['t1'], raw_internal_path_out=['t2'], thickness=T.THICKNESSES,
                          slice_num=k, min_value=lo, max_value=hi, device='cuda', normalise=config, augment=augment, **kw)


def _want_pool(ds, items, k, hw, config):
    """[count, k + 1, 4]: the planes of A from the input volume, then B's from the target volume."""
    rows = []
    for va, vb, idx, t in items.tolist():
        subject = ds.volumes[va // 2]
        rows.append([plane_record(p, config) for p in _item_planes(subject['t1'], idx, t, k, hw)] +
                    [plane_record(_item_planes(subject['t2'], idx, t, 1, hw)[0], config)])
    return torch.from_numpy(np.array(rows))


@pytest.mark.parametrize('k', [4, 1])
@pytest.mark.parametrize('dtype', T.DTYPES)
def test_pool_coefficients_and_invalid_rows(dtype, k):
    from afcm_amd.torch_utils.ops.normalise_ops import plane_norm_stats
    hw = (12, 10)
    ds = _set(dtype, hw, k, PERCENTILE)
    items = T.shuffled_items(k)
    table = torch.from_numpy(items).cuda()
    for name, config in MODES.items():
        got = plane_norm_stats(ds.pool, ds.vols, table, 0, 23, hw, k, config)
        assert got.shape == (23, k + 1, 4) and torch.equal(got.cpu(), _want_pool(ds, items, k, hw, config)), name
        assert torch.equal(plane_norm_stats(ds.pool, ds.vols, table, 0, 23, hw, k, config), got)
    # one invalid row of each kind between two good ones: four NaNs for every plane of the row, the neighbours untouched; the batch likewise
    from afcm_amd.torch_utils.ops.batch_ops import assemble_batch
    bad = {kind: row for kind, row in T.invalid_rows(ds.vols_host).items() if not (k == 1 and kind == 'thickness_negative_k4')}
    mixed = np.array([r for row in bad.values() for r in (items[0], row, items[1])], dtype=np.int32)
    got = plane_norm_stats(ds.pool, ds.vols, torch.from_numpy(mixed).cuda(), 0, len(mixed), hw, k, STANDARD).cpu()
    good = _want_pool(ds, items[:2], k, hw, STANDARD)
    a, b, c = assemble_batch(ds.pool, ds.vols, torch.from_numpy(mixed).cuda(), 0, len(mixed), hw, slice_num=k, normalise=STANDARD)
    want = ds.host_batch(items, 0, 2, normalise=STANDARD)
    for j in range(len(bad)):
        assert torch.equal(got[3 * j], good[0]) and torch.equal(got[3 * j + 2], good[1]) and bool(got[3 * j + 1].isnan().all()), list(bad)[j]
        assert all(bool(t[3 * j + 1].isnan().all()) for t in (a, b, c))
        assert torch.equal(a[3 * j], want[0][0]) and torch.equal(b[3 * j + 2], want[1][1]) and torch.equal(c[3 * j + 2], want[2][1])
    past = plane_norm_stats(ds.pool, ds.vols, table, 20, 5, hw, k, STANDARD).cpu()                # rows 23, 24 lie past the table
    assert not bool(past[:3].isnan().any()) and bool(past[3:].isnan().all())


def _same_batches(got, want, dtype=torch.float32):
    assert torch.equal(got[0], want[0].to(dtype)) and torch.equal(got[1], want[1].to(dtype)) and torch.equal(got[2], want[2])


@pytest.mark.parametrize('mode', ['percentile', 'standardize'])
@pytest.mark.parametrize('dtype', T.DTYPES)
def test_batches_equal_the_host_arm(dtype, mode):
    """23 shuffled rows of three subjects into 12 x 10 (w a multiple of neither 4 nor 8), float32 and 16-bit outputs, then_normalize both ways,
    batches of 5 with a ragged last one, ``out=``, and the device cursor."""
    hw, base = (12, 10), MODES[mode]
    items = T.shuffled_items(4)
    for then in (False, True):
        config = NormaliseConfig(percentile=base.percentile, standardize=base.standardize, then_normalize=then)
        ds = _set(dtype, hw, 4, config, then_range=then)
        want = ds.host_batch(items, 0, 23, normalise=config)
        assert all(bool(torch.isfinite(t).all()) for t in want) and not torch.equal(want[0], ds.host_batch(items, 0, 23)[0])
        if then:
            assert float(want[0].min()) == -1.0 and float(want[0].max()) <= 1.0
        ds.load_epoch(items)
        batches = list(ds.batches(T.BATCH))
        assert [int(b[0].shape[0]) for b in batches] == [5, 5, 5, 5, 3]
        _same_batches([torch.cat([b[j] for b in batches]) for j in range(3)], want)
        for out_dtype in (torch.float16, torch.bfloat16):
            _same_batches(ds.batch(0, 23, dtype=out_dtype), want, out_dtype)
    out = (torch.full((5, 4) + hw, 7., device='cuda'), torch.full((5, 1) + hw, 7., device='cuda'), torch.full((5, 1), 7., device='cuda'))
    got = ds.batch(5, 5, out=out)
    assert all(g is o for g, o in zip(got, out))
    _same_batches(out, [t[5:10] for t in want])
    coef = ds.norm_coef
    assert coef.shape == (23, 5, 4) and ds.batch(10, 5)[0] is not None and ds.norm_coef is coef   # persistent: a smaller batch reuses it
    ds.cursor.fill_(10)
    _same_batches(ds.batch(3, 5, use_cursor=True), [t[13:18] for t in want])
    assert torch.equal(ds.norm_coef[:5].cpu(), _want_pool(ds, items[13:18], 4, hw, config))


@pytest.mark.parametrize('k', [4, 1])
def test_batches_with_geometric_augmentation(k):
    """Every flip, every quarter turn on the square patch, and a rotation: coefficients of the un-augmented plane, then the gather -- the
    reference's order of operations bit for bit, because a nearest-neighbour gather commutes with a pointwise map."""
    hw = (16, 16)
    full = A.AugmentConfig(flip_axes=(1, 2), rotate90=True, angle_spectrum=45)
    for config in (PERCENTILE, NormaliseConfig(standardize=True, then_normalize=True)):
        ds = _set(np.int16, hw, k, config, augment=full, then_range=config.then_normalize)
        items = T.shuffled_items(k)
        fh, fw, q = np.arange(23) % 2, np.arange(23) // 2 % 2, np.arange(23) % 4
        angle = np.where(np.arange(23) < 8, 0, np.where(np.arange(23) < 16, 37, -12))
        rows = A.make_rows(fh, fw, q, angle, hw)
        want = ds.host_batch(items, 0, 23, augment=rows, normalise=config)
        plain = ds.host_batch(items, 0, 23, normalise=config)
        assert not torch.equal(want[0], plain[0])
        ds.load_epoch(items, rows)
        _same_batches(ds.batch(0, 23), want)
        _same_batches(ds.batch(0, 23, dtype=torch.bfloat16), want, torch.bfloat16)
        ds.load_epoch(items)                                                                      # identity rows: the launch without a table
        _same_batches(ds.batch(0, 23), plain)


@pytest.mark.parametrize('name', ['crop_and_pad_u8', 'pad_i16', 'crop_f32', 'tail_f32', 'tail_i16_k1', 'narrow_f64', 'single_slice_no_thickness'])
def test_slices_equal_stacked_dataset_items(name):
    from afcm_amd.torch_utils.ops.volume_ops import assemble_slices
    shape, dtype, hw, thickness, k, (lo, hi) = R.ASSEMBLY_CASES[name]
    src = R.source(shape, dtype, seed=7)
    volume = torch.from_numpy(src).cuda()
    for config in (PERCENTILE, MINMAX, STANDARD, NormaliseConfig(standardize=True, then_normalize=True), NormaliseConfig(percentile=(2, 98), then_normalize=True)):
        lo_, hi_ = (0.0, 1.0) if config.then_normalize else (lo, hi)
        ds = SliceDataset({'raw': src}, phase='test', patch_shape=(1,) + hw, stride_shape=(1, 1, 1), thickness=[] if thickness is None else [thickness],
                          slice_num=k, min_value=lo_, max_value=hi_, normalise=config)
        items = [ds[i] for i in range(len(ds))]
        want_a, want_c = torch.stack([it[0] for it in items]), torch.stack([it[1] for it in items])
        a, c = assemble_slices(volume, 0, shape[0], (1,) + hw, thickness=thickness, slice_num=k, min_value=lo_, max_value=hi_, normalise=config)
        assert torch.equal(a.cpu(), want_a) and torch.equal(c.cpu(), want_c), config
        for out_dtype in (torch.float16, torch.bfloat16):
            a16, _ = assemble_slices(volume, 2, 3, (1,) + hw, thickness=thickness, slice_num=k, min_value=lo_, max_value=hi_, dtype=out_dtype,
                                     normalise=config)
            assert torch.equal(a16.cpu(), want_a[2:5].to(out_dtype))
    plain, _ = assemble_slices(volume, 0, shape[0], (1,) + hw, thickness=thickness, slice_num=k, min_value=lo, max_value=hi)
    again, _ = assemble_slices(volume, 0, shape[0], (1,) + hw, thickness=thickness, slice_num=k, min_value=lo, max_value=hi, normalise=None)
    assert torch.equal(plain, again) and not torch.equal(plain, a)


def test_predict_volume_device_and_host_arms(monkeypatch):
    from afcm_amd.volume import evaluate_volume, predict_volume
    from test_gpu_volume import StubStep, _counting
    src = R.source((11, 30, 40), np.int16, seed=8)                                                # pad in y, crop in x; three batches of 4, one ragged
    kw = dict(raw_internal_path_in='raw', thickness=5, patch_hw=(32, 32), batch_size=4, patch_halo=(0, 4, 4))
    plain = predict_volume(StubStep(), {'raw': src}, where='device', heads=('input',), **kw)
    for config in (PERCENTILE, NormaliseConfig(standardize=True, then_normalize=True)):
        more = dict(kw, normalise=config, min_value=0.0, max_value=1.0)
        host = predict_volume(StubStep(), {'raw': src}, where='host', heads=('prediction', 'input'), **more)
        copies = []
        _counting(monkeypatch, copies)
        dev = predict_volume(StubStep(), {'raw': src}, where='device', heads=('prediction', 'input'), **more)
        assert copies == [], copies                                                               # no device -> host copy, no scalar read
        target = dev['input'][0].clone()
        out = evaluate_volume(StubStep(), {'raw': src}, target, from_network_range=False, **more)
        monkeypatch.undo()
        assert copies == [('cpu', (11 + 32 + 32, 8))], copies                                     # the three axes' tables, together, once
        for head in ('prediction', 'input'):
            assert dev[head].is_cuda and dev[head].shape == host[head].shape == (1, 11, 32, 32)
            assert torch.equal(dev[head].cpu(), host[head])
        assert torch.equal(out['prediction'], dev['prediction']) and not torch.equal(dev['input'], plain['input'])


def test_a_set_without_normalise_launches_what_it_launched_before():
    from afcm_amd.torch_utils.ops.batch_ops import assemble_batch
    hw = (12, 10)
    ds = _set(np.uint8, hw, 4, None)
    items = T.shuffled_items(4)
    ds.load_epoch(items)
    assert ds.normalise is None and ds.norm_coef is None
    got = ds.batch(0, 23)
    want = assemble_batch(ds.pool, ds.vols, torch.from_numpy(items).cuda(), 0, 23, hw, slice_num=4, min_value=ds.min_value, max_value=ds.max_value)
    host = ds.host_batch(items, 0, 23)
    for g, w, h in zip(got, want, host):
        assert torch.equal(g, w) and torch.equal(g.cpu(), h.cpu())
    assert ds.norm_coef is None


def _tiny_normalised_set(config):
    from afcm_amd.training import DeviceSliceSet
    from test_gpu_train_batch import _tiny_set
    plain, items = _tiny_set()
    ds = DeviceSliceSet(plain.volumes, patch_shape=(1, 128, 128), raw_internal_path_in=['t1'], raw_internal_path_out=['t2'], thickness=[5], device='cuda',
                        min_value=0.0, max_value=1.0, normalise=config)
    return ds, items


def test_train_epoch_arms_and_training_graph_on_the_tiny_generator():
    """``train_epoch``'s two arms leave the same parameters; three warm-up steps and three replays of a ``TrainingGraph`` equal six eager steps
    (bfloat16 compute, as tests/test_gpu_train_batch.py explains), and the graph's batch is the set's own."""
    from afcm_amd.training import TrainingGraph, train_epoch
    from test_gpu_train_batch import _state, _tiny_step
    config = NormaliseConfig(percentile=(1, 99.6), then_normalize=True)
    ds, items = _tiny_normalised_set(config)
    finals = {}
    for where in ('device', 'host'):
        step = _tiny_step(ema=True)
        torch.manual_seed(3)
        assert train_epoch(step, ds, 4, items[:8], total_iters=100, ema_kimgs=10.0, ramp=0.05, where=where) == 108
        finals[where] = _state(step)
        assert all(bool(torch.isfinite(t).all()) for t in finals[where])
    assert all(torch.equal(a, b) for a, b in zip(finals['device'], finals['host']))

    items = items[:12]
    z = torch.randn(4, 32, generator=torch.Generator().manual_seed(9)).cuda()
    eager = _tiny_step(compute_dtype=torch.bfloat16, capturable=True)
    for _ in range(2):
        train_epoch(eager, ds, 4, items, gen_z=z)
    want = [p.detach().clone() for p in eager.netG.parameters()]
    step = _tiny_step(compute_dtype=torch.bfloat16, capturable=True)
    ds.load_epoch(items)
    graph = TrainingGraph(step, ds, 4, warmup=3, fixed_z=True, gen_z=z)
    assert graph.norm_coef is ds.norm_coef and graph.norm_coef.shape == (4, 5, 4)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(ds.cursor.cpu()) == 12
    for a, b in zip(step.netG.parameters(), want):
        assert torch.equal(a.detach(), b)
    last = ds.host_batch(items, 8, 4, normalise=config)
    assert torch.equal(graph.real_A.cpu(), last[0].cpu()) and torch.equal(graph.real_B.cpu(), last[1].cpu())
