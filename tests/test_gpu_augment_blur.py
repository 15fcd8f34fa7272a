"""Training batches with a per-plane Gaussian blur on the GPU: ``afcm_batch_assemble_blur`` against ``DeviceSliceSet.host_batch(..., blur=...)`` --
stacked ``SliceDataset(phase='train')`` items through ``afcm_amd.augment_blur.apply_host``, the numpy arm that tests/test_augment_blur_ref_cpu.py
holds to scipy and to the golden captured from the reference's class.  Every comparison is ``torch.equal`` / of bit patterns.
The shapes are the smallest at which the kernels can go wrong: 24 x 32 and a plane shorter than the largest radius (5 x 7 at radius 16: every
tap but the centre is clamped), widths that are no multiple of the 4-pixel run (30, 33), one plane a tile plus one in each direction of either
pass (the extents come from ``afcm_blur_tiles``), more than one workgroup per launch, the first and the last slice of a 7-deep volume (thick-slice
planes outside it are blurred constants)."""
import ctypes

import numpy as np
import pytest
import torch

import augment_blur_ref as R
import train_batch_ref as T
from afcm_amd import augment as A
from afcm_amd import augment_blur as B
from afcm_amd import augment_elastic as E
from afcm_amd import augment_intensity as I

pytestmark = pytest.mark.gpu

_BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
GEO = A.AugmentConfig(flip_axes=(1, 2), angle_spectrum=45)
NOISE = I.IntensityConfig(contrast=(0.5, 1.5, 0.0, 0.6), gaussian=(0.0, 1.0, 0.6), poisson=(0.0, 1.0, 0.6))
OFTEN = B.BlurConfig(sigma=(0.1, 4.1), execution_probability=0.6)
# sigma -> radius: 0, 1, 8, 16
RADII = {0.1: 0, 0.3: 1, 2.0: 8, 4.1: 16}
# three items: the first slice of subject 0 (planes at -2 outside), the last of subject 1 (planes at +2, +4 outside), one inside
THREE = np.array([(0, 1, 0, 2), (2, 3, 6, 2), (0, 1, 3, 2)], dtype=np.int32)
PLAIN = np.array([(0, 1, 1, -1), (2, 3, 2, -1)], dtype=np.int32)                 # slice_num 1, no thickness


def _same_bits(got, want):
    got, want = got.cpu(), torch.as_tensor(want).cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    assert not bool(torch.isnan(want).any())
    differing = int((got.view(_BITS[want.dtype]) != want.view(_BITS[want.dtype])).sum())
    assert differing == 0, f'{differing} of {want.numel()} elements differ'


def _sources(hw, depth=7, dtype=np.uint8):
    """Two subjects whose planes are a little larger and a little smaller than the patch: a crop and a pad in each."""
    from volume_ref import source
    shapes = ((depth, hw[0] + 2, max(hw[1] - 2, 1)), (depth, max(hw[0] - 2, 1), hw[1] + 5))
    return [{m: source(shape, dtype, seed=90 + 2 * s + j) for j, m in enumerate(('t1', 't2'))} for s, shape in enumerate(shapes)]


def _set(hw, k, blur=OFTEN, sources=None, augment=None, intensity=None, elastic=None, dtype=np.uint8, thickness=(2,)):
    from afcm_amd.training import DeviceSliceSet
    lo, hi = T.value_range(dtype)
    return DeviceSliceSet(_sources(hw) if sources is None else sources, patch_shape=(1,) + tuple(hw), raw_internal_path_in=['t1'],
                          raw_internal_path_out=['t2'], thickness=thickness if k == 4 else (), slice_num=k, min_value=lo, max_value=hi, device='cuda',
                          augment=augment, intensity=intensity, elastic=elastic, blur=blur)


def _launch(ds, items, rows, geo=None, noise=None, warp=None, first=0, count=None, independent=False, **kw):
    """The op on tables of the test's own (any number of rows): what ``ds.batch`` launches on the set's persistent ones."""
    from afcm_amd.torch_utils.ops.batch_ops import assemble_batch
    count = len(items) - first if count is None else count
    more = {} if rows is None else dict(blur=torch.from_numpy(rows).cuda())
    if warp is not None:
        more.update(elastic=torch.from_numpy(warp).cuda(), elastic_ops=ds.elastic_ops)
    return assemble_batch(ds.pool, ds.vols, torch.from_numpy(items).cuda(), first, count, ds.patch_shape[1:], slice_num=ds.slice_num, min_value=ds.min_value,
                          max_value=ds.max_value, augment=None if geo is None else torch.from_numpy(geo).cuda(),
                          intensity=None if noise is None else torch.from_numpy(noise).cuda(), independent_planes=independent, **more, **kw)


def _rows(sigmas, k):
    """One row per item from a list of per-plane sigmas, None for a plane left alone."""
    rows = B.identity_rows(len(sigmas), k).reshape(len(sigmas), k + 1, B.PLANE_COLS)
    for i, item in enumerate(sigmas):
        assert len(item) == k + 1
        for p, sigma in enumerate(item):
            if sigma is not None:
                rows[i, p] = B.plane_record(sigma)
    return rows.reshape(len(sigmas), -1)


def _tiles():
    from afcm_amd import _lib
    v = [ctypes.c_int32(0) for _ in range(4)]
    _lib.load().afcm_blur_tiles(*[ctypes.byref(x) for x in v])
    return [x.value for x in v]


@pytest.mark.parametrize('hw', [(24, 32), (5, 7)])
def test_radii_0_1_8_16_and_lines_shorter_than_the_radius(hw):
    assert [B.gaussian_weights(s)[0] for s in RADII] == list(RADII.values())
    ds = _set(hw, 4)
    rows = _rows([[0.1, 0.3, 2.0, 4.1, 4.1], [4.1, 2.0, 0.3, 0.1, 2.0], [0.3, 4.1, 0.1, 2.0, 0.3]], 4)
    want = ds.host_batch(THREE, 0, 3, blur=rows)
    plain = ds.host_batch(THREE, 0, 3)
    assert not torch.equal(want[0][:, 1:], plain[0][:, 1:]) and torch.equal(want[2], plain[2])
    if hw == (24, 32):                                                            # a constant plane outside the volume stays that constant, to rounding
        assert bool((plain[0][0, 0] == -1.0).all()) and float((want[0][0, 0] + 1.0).abs().max()) < 1e-6
    for dtype in (torch.float32, torch.bfloat16):
        got = _launch(ds, THREE, rows, dtype=dtype)
        _same_bits(got[0], want[0].to(dtype))
        _same_bits(got[1], want[1].to(dtype))
        _same_bits(got[2], want[2])


def test_widths_off_the_run_and_a_tile_plus_one_of_either_pass():
    rows_h, rows_w, cols_h, cols_w = _tiles()
    assert rows_w % 4 == 0 and cols_w % 4 == 0
    for hw in [(24, 30), (21, 33), (rows_h + 1, rows_w + 1), (cols_h + 1, cols_w + 1)]:
        ds = _set(hw, 1, sources=_sources(hw, depth=3))
        rows = _rows([[4.1, 2.0], [0.3, 4.1]], 1)
        want = ds.host_batch(PLAIN, 0, 2, blur=rows)
        for g, w in zip(_launch(ds, PLAIN, rows), want):
            _same_bits(g, w)


def test_every_plane_its_own_flag_and_a_batch_that_executes_nothing():
    hw = (24, 32)
    ds = _set(hw, 4)
    rows = _rows([[None, 1.37, None, 0.9, None], [2.0, None, None, None, 3.3], [None] * 5], 4)
    want = ds.host_batch(THREE, 0, 3, blur=rows)
    plain = ds.host_batch(THREE, 0, 3)
    for i, item in enumerate(rows.reshape(3, 5, 20)[:, :, 0]):                    # the flag decides, plane by plane
        for p, flag in enumerate(item):
            a, b = (want[0][i, p], plain[0][i, p]) if p < 4 else (want[1][i, 0], plain[1][i, 0])
            assert torch.equal(a, b) == (flag == 0.0 or bool((b == b[0, 0]).all()))
    for g, w in zip(_launch(ds, THREE, rows), want):
        _same_bits(g, w)
    # no executed plane: the launch without the table, whatever the records of the idle planes say
    quiet = _rows([[4.1] * 5] * 3, 4)
    quiet[:, ::20] = 0.0
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        for g, w in zip(_launch(ds, THREE, quiet, dtype=dtype), _launch(ds, THREE, None, dtype=dtype)):
            assert torch.equal(g, w)
    for g, w in zip(_launch(ds, THREE, B.identity_rows(3, 4)), plain):
        _same_bits(g, w)


@pytest.mark.parametrize('case', ['augment', 'intensity', 'intensity independent', 'elastic 1', 'elastic 3', 'all four'])
def test_with_the_other_tables(case):
    hw = (21, 37)
    order = 1 if case == 'elastic 1' else 3
    warp_config = E.ElasticConfig(spline_order=order, alpha=30.0, sigma=2.0, execution_probability=0.5) if case.startswith('elastic') or case == 'all four' else None
    with_geo, with_noise = case in ('augment', 'all four'), case.startswith('intensity') or case == 'all four'
    independent = case == 'intensity independent'
    noise_config = None if not with_noise else (I.IntensityConfig(contrast=(0.5, 1.5, 0.0, 0.6), gaussian=(0.0, 1.0, 0.6), poisson=(0.0, 1.0, 0.6),
                                                                  independent_planes=True) if independent else NOISE)
    ds = _set(hw, 4, augment=GEO if with_geo else None, intensity=noise_config, elastic=warp_config)
    items = np.concatenate([THREE, THREE])
    rows = ds.epoch_blur(7, rows=6)
    assert 10 <= rows[:, ::20].sum() <= 26
    geo = ds.epoch_augment(5, rows=6) if with_geo else None
    noise = ds.epoch_intensity(12, rows=6) if with_noise else None
    warp = None
    if warp_config is not None:
        warp = ds.epoch_elastic(4, rows=6)
        warp[:, 0] = [1, 0, 1, 0, 1, 1]
    want = ds.host_batch(items, 0, 6, augment=geo, intensity=noise, elastic=warp, blur=rows)
    if case == 'all four':                                                        # the chain, said once more: rotate, deform, blur, then noise
        before = ds.host_batch(items, 0, 6, augment=geo)
        for j in (0, 1):
            x = E.apply_host(torch.cat([before[0][j], before[1][j]]).cpu(), warp[j], ds.elastic, ds.elastic_ops_host)
            x = B.apply_host(x, rows[j])
            x = torch.cat([I.apply_host(x[:4], noise[j], False, 0), I.apply_host(x[4:], noise[j], False, 4)])
            assert torch.equal(want[0][j].cpu(), x[:4]) and torch.equal(want[1][j].cpu(), x[4:])
    for dtype in (torch.float32, torch.float16):
        got = _launch(ds, items, rows, geo, noise, warp, independent=independent, dtype=dtype)
        _same_bits(got[0], want[0].to(dtype))
        _same_bits(got[1], want[1].to(dtype))
        _same_bits(got[2], want[2])
    # a table that executes nothing gives the launch without it
    for g, w in zip(_launch(ds, items, B.identity_rows(6, 4), geo, noise, warp, independent=independent),
                    _launch(ds, items, None, geo, noise, warp, independent=independent)):
        assert torch.equal(g, w)


@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
def test_the_sets_own_tables_a_ragged_last_batch_out_and_the_cursor(dtype):
    from afcm_amd.torch_utils.ops.batch_ops import advance_cursor
    hw = (24, 30)
    ds = _set(hw, 4, sources=T.subjects(dtype), dtype=dtype, thickness=T.THICKNESSES, augment=GEO)
    items, geo, rows = T.shuffled_items(4), ds.epoch_augment(3), ds.epoch_blur(4)
    assert rows.shape == (23, 100) and 40 <= rows[:, ::20].sum() <= 100
    want = ds.host_batch(items, 0, 23, augment=geo, blur=rows)
    ds.load_epoch(items, geo, None, None, rows)
    assert torch.equal(ds.blur_table.cpu(), torch.from_numpy(rows))
    batches = list(ds.batches(T.BATCH))
    assert [int(b[0].shape[0]) for b in batches] == [5, 5, 5, 5, 3]
    for j in range(3):
        _same_bits(torch.cat([b[j] for b in batches]), want[j])
    out = (torch.full((5, 4) + hw, 7., device='cuda'), torch.full((5, 1) + hw, 7., device='cuda'), torch.full((5, 1), 7., device='cuda'))
    got = []
    for _ in range(2):
        assert all(g is o for g, o in zip(ds.batch(0, 5, out=out, use_cursor=True), out))
        got.append([t.clone() for t in out])
        advance_cursor(ds.cursor, 5)
    assert int(ds.cursor.cpu()) == 10
    for j in range(3):
        _same_bits(torch.cat([g[j] for g in got]), want[j][:10])
    past = ds.batch(10, 5, use_cursor=True)                                       # rows 20 ... 24: two past the table
    assert all(bool(torch.isnan(t[3:]).all()) for t in past)
    for t, w in zip(past, want):
        _same_bits(t[:3], w[20:23])
    # a set that is given no rows loads identity rows; rows past a short epoch are identity rows again
    ds.load_epoch(items[:10], geo[:10])
    assert torch.equal(ds.blur_table.cpu(), torch.from_numpy(B.identity_rows(23, 4)))
    for g, w in zip(ds.batch(0, 10), ds.host_batch(items, 0, 10, augment=geo)):
        _same_bits(g, w)


def test_slice_num_1_a_callers_workspace_and_two_launches():
    from afcm_amd import _lib
    from afcm_amd.torch_utils.ops.batch_ops import blur_workspace_bytes, elastic_workspace_bytes
    hw = (24, 30)
    ds = _set(hw, 1, sources=_sources(hw, depth=3))
    rows = _rows([[1.37, None], [None, 4.1]], 1)
    want = ds.host_batch(PLAIN, 0, 2, blur=rows)
    need = blur_workspace_bytes(2, 1, 24, 30)
    assert need >= 2 * 24 * 30 * 2 * (4 + 8) and blur_workspace_bytes(2, 1, 24, 30, 3) >= need + elastic_workspace_bytes(2, 1, 24, 30, 3)
    launches, bytes_ = ctypes.c_int32(0), ctypes.c_int64(0)
    lib = _lib.load()
    assert lib.afcm_blur_plan(2, 1, 24, 30, -1, ctypes.byref(bytes_), ctypes.byref(launches)) == 0 and launches.value == 4 and bytes_.value == need
    assert lib.afcm_blur_plan(2, 1, 24, 30, 3, ctypes.byref(bytes_), ctypes.byref(launches)) == 0 and launches.value == 11
    assert lib.afcm_blur_plan(2, 1, 24, 30, 1, ctypes.byref(bytes_), ctypes.byref(launches)) == 0 and launches.value == 9
    for bad, message in [((2, 1, 24, 30, 2), 'spline order 2'), ((0, 1, 24, 30, -1), '1 to 32767 items'), ((2, 2, 24, 30, -1), 'slice number 2'),
                         ((2, 4, 24, 32769, -1), 'extents 1 to 32768')]:
        assert lib.afcm_blur_plan(*bad, ctypes.byref(bytes_), None) == _lib.E_INVALID and message in lib.afcm_last_error().decode(), bad
    work = torch.empty(need, dtype=torch.uint8, device='cuda')
    first = _launch(ds, PLAIN, rows, workspace=work)
    for g, w in zip(first, want):
        _same_bits(g, w)
    work.fill_(255)                                                               # nothing is kept between calls, and the same bits come out again
    for g, f in zip(_launch(ds, PLAIN, rows, workspace=work), first):
        assert torch.equal(g, f)
    with pytest.raises(RuntimeError, match=f'workspace must be a contiguous 1-D uint8 tensor of at least {need} bytes'):
        _launch(ds, PLAIN, rows, workspace=torch.empty(need - 1, dtype=torch.uint8, device='cuda'))
    with pytest.raises(RuntimeError, match=r'blur table must be a contiguous torch.float64 \[n, 40\]'):
        _launch(ds, PLAIN, rows[:, :20].copy())
    with pytest.raises(RuntimeError, match='has 1 rows, the item table 2'):
        _launch(ds, PLAIN, rows[:1])


def test_invalid_rows_are_nan_items_and_their_neighbours_are_untouched():
    hw = (21, 37)
    ds = _set(hw, 4, intensity=NOISE)
    kinds = ['flag 2', 'sigma nan', 'radius 17', 'radius 0.5', 'weight inf', 'flag nan', 'sigma 0', 'radius -1', 'weight nan']
    n = len(kinds) + 4
    items = THREE[np.arange(n) % 3]
    good = ds.epoch_blur(31, rows=n)
    plain = ds.host_batch(items, 0, n)
    at, keep = list(range(2, 2 + len(kinds))), [0, 1, n - 2, n - 1]
    table = good.copy()
    for row, kind in zip(at, kinds):
        col, value = R.INVALID[kind]
        table[row, 20 * (row % 5) + col] = value                                  # a different plane's record from row to row, the target's among them
        assert not B.row_is_valid(table[row])
    got = _launch(ds, items, table)
    for j, g in enumerate(got):
        nan_items = torch.isnan(g).reshape(n, -1).cpu()
        assert bool(nan_items[at].all()), [kind for kind, row in zip(kinds, at) if not bool(nan_items[row].all())]
        assert not bool(nan_items[keep].any())
        if j < 2:                                                                 # the numpy restatement of the stage on the items without the table
            for i in keep:
                planes = torch.cat([plain[0][i], plain[1][i]]).cpu().numpy()
                want = R.numpy_blur_item(planes, good[i])
                assert np.array_equal(g[i].cpu().numpy(), want[:4] if j == 0 else want[4:])
    # with the intensity table: an invalid blur row beside valid intensity rows, and the other way round
    noise = ds.epoch_intensity(9, rows=n)
    want = ds.host_batch(items, 0, n, intensity=noise, blur=good)
    bad_noise = noise.copy()
    bad_noise[1, 9] = np.nan
    for g, w in zip(_launch(ds, items, table, None, bad_noise), want):
        nan_items = torch.isnan(g).reshape(n, -1).cpu()
        assert bool(nan_items[at + [1]].all()) and int(nan_items.any(dim=1).sum()) == len(at) + 1
        _same_bits(g.cpu()[[0, n - 2, n - 1]], w[[0, n - 2, n - 1]])
    # a row index outside the table: the cursor sends the last two items past it
    cursor = torch.tensor([n - 2], dtype=torch.int64, device='cuda')
    for g, w in zip(_launch(ds, items, good, None, noise, first=0, count=4, cursor=cursor), want):
        assert bool(torch.isnan(g[2:]).all())
        _same_bits(g[:2], w[n - 2:])


# ---- the set and the training loops on the tiny 128^2 generator of test_gpu_train_batch.py ---------------------------------------------------------

def _tiny_blur_set(**kw):
    from afcm_amd.training import DeviceSliceSet
    from test_gpu_train_batch import _tiny_set
    plain, items = _tiny_set()
    ds = DeviceSliceSet(plain.volumes, patch_shape=(1, 128, 128), raw_internal_path_in=['t1'], raw_internal_path_out=['t2'], thickness=[5], device='cuda',
                        blur=B.BlurConfig(), **kw)
    assert np.array_equal(ds.epoch_items(11), items)                              # the item draw does not know about the augmentation
    return ds, items, ds.epoch_blur(21)


def test_a_set_without_blur_is_what_it_was():
    from afcm_amd.training import DeviceSliceSet
    hw = (24, 30)
    with_blur = _set(hw, 4, augment=GEO, intensity=NOISE)
    without = _set(hw, 4, blur=None, augment=GEO, intensity=NOISE)
    assert without.blur is None and without.blur_table is None and without.elastic_workspace is None
    for name in ('epoch_items', 'epoch_augment', 'epoch_intensity'):
        assert np.array_equal(getattr(with_blur, name)(3), getattr(without, name)(3))
    items, geo, noise = without.epoch_items(3), without.epoch_augment(4), without.epoch_intensity(5)
    without.load_epoch(items, geo, noise)
    with_blur.load_epoch(items, geo, noise)                                       # no rows given: identity rows
    for g, p, w in zip(with_blur.batch(0, 5), without.batch(0, 5), without.host_batch(items, 0, 5, augment=geo, intensity=noise)):
        assert torch.equal(g, p)
        _same_bits(p, w)
    assert without.elastic_workspace is None and with_blur.elastic_workspace is not None
    with pytest.raises(RuntimeError, match='built without blur'):
        without.load_epoch(items, geo, noise, None, B.identity_rows(len(items), 4))
    with pytest.raises(RuntimeError, match='built without blur'):
        without.epoch_blur(1)
    with pytest.raises(RuntimeError, match=r'float64 \[14, 100\]'):
        with_blur.load_epoch(items, geo, noise, None, B.identity_rows(13, 4))
    with pytest.raises(RuntimeError, match='BlurConfig or None'):
        DeviceSliceSet(_sources(hw), patch_shape=(1,) + hw, raw_internal_path_in=['t1'], raw_internal_path_out=['t2'], thickness=(2,), device=None, blur=0.5)
    with pytest.raises(RuntimeError, match="'train' phase"):
        DeviceSliceSet(_sources(hw), phase='val', patch_shape=(1,) + hw, raw_internal_path_in=['t1'], raw_internal_path_out=['t2'], thickness=(2,),
                       device=None, blur=B.BlurConfig())


def test_train_epoch_device_and_host_arms_leave_the_same_bits():
    from afcm_amd.training import train_epoch
    from test_gpu_train_batch import _state, _tiny_step
    ds, items, rows = _tiny_blur_set()
    assert 15 <= rows[:8, ::20].sum() <= 25
    finals = {}
    for arm, blur in (('device', rows), ('host', rows), ('plain', None)):
        step = _tiny_step(ema=True)
        torch.manual_seed(3)                                                      # set_input draws gen_z: the same draws for every arm
        total = train_epoch(step, ds, 4, items[:8], total_iters=100, ema_kimgs=10.0, ramp=0.05, where='host' if arm == 'host' else 'device',
                            blur=None if blur is None else blur[:8])
        assert total == 108
        finals[arm] = _state(step)
        assert all(bool(torch.isfinite(t).all()) for t in finals[arm])
    assert all(torch.equal(a, b) for a, b in zip(finals['device'], finals['host']))
    assert any(not torch.equal(a, b) for a, b in zip(finals['device'], finals['plain']))       # the blur did reach the step


def test_train_epochs_with_and_without_the_graph():
    """The outer loop on the bfloat16 generator step with a schedule and an EMA copy: two epochs of 18 rows in batches of 2, each with its own draw
    of items, parameter rows, intensity rows and blur rows -- the last from a ``random.Random`` seeded by one more draw of the generator; ONE
    captured graph against eager steps."""
    import random
    from afcm_amd.schedule import LRSchedule
    from afcm_amd.training import train_epochs
    from test_gpu_schedule import _schedule
    from test_gpu_train_batch import _state, _tiny_step
    ds, _, _ = _tiny_blur_set(augment=A.AugmentConfig(flip_axes=(1, 2), rotate90=True, angle_spectrum=45), intensity=NOISE)
    z = torch.randn(2, 32, generator=torch.Generator().manual_seed(10)).cuda()
    lrs = LRSchedule('linear', 0.0002, epoch_count=1, n_epochs=2, n_epochs_decay=2)
    rng = np.random.default_rng(5)
    for _ in range(2):
        last = ds.epoch_items(rng), ds.epoch_augment(rng), ds.epoch_intensity(rng)
        last += (ds.epoch_blur(random.Random(int(rng.integers(0, 2 ** 63)))),)
    assert 20 < last[3][:, ::20].sum() < 70
    finals = {}
    for graph in (True, False):
        step = _tiny_step(compute_dtype=torch.bfloat16, capturable=True, ema=True, schedule=_schedule(ema_kimgs=10.0, ramp=0.05))
        before = _state(step)
        assert train_epochs(step, ds, 2, range(1, 3), lrs, 5, graph=graph, gen_z=z) == 18
        for table, rows in zip((ds.items, ds.augment_table, ds.intensity_table, ds.blur_table), last):
            assert torch.equal(table.cpu(), torch.from_numpy(rows))
        assert step.schedule.read()['total_iters'] == 36.0 and step.optimizer_G.device_step() == 18
        finals[graph] = _state(step)
        assert any(not torch.equal(p, q) for p, q in zip(finals[graph], before))
    assert len(finals[True]) == len(finals[False]) and all(torch.equal(p, q) for p, q in zip(finals[True], finals[False]))
    assert all(bool(torch.isfinite(p).all()) for p in finals[True])


def test_training_graph_reads_the_last_batch_of_redrawn_rows():
    from afcm_amd.training import TrainingGraph
    from test_gpu_train_batch import _tiny_step
    ds, items, rows = _tiny_blur_set()
    items, rows = items[:8], rows[:8]
    ds.load_epoch(items, None, None, None, rows)
    for g, w in zip(ds.batch(0, 4), ds.host_batch(items, 0, 4, blur=rows)):       # `batch` against `host_batch` at 128 x 128: four tiles of the y pass
        assert torch.equal(g, w)
    z = torch.randn(4, 32, generator=torch.Generator().manual_seed(9)).cuda()
    step = _tiny_step(compute_dtype=torch.bfloat16, capturable=True)
    graph = TrainingGraph(step, ds, 4, warmup=2, fixed_z=True, gen_z=z)
    assert int(ds.cursor.cpu()) == 0 and graph.elastic_workspace is ds.elastic_workspace
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    fresh = ds.host_batch(items, 4, 4, blur=rows)
    assert int(ds.cursor.cpu()) == 8 and torch.equal(graph.real_A, fresh[0]) and torch.equal(graph.real_B, fresh[1]) and torch.equal(graph.slice_idx, fresh[2])
    other = ds.epoch_blur(23, rows=8)                                             # refreshed in place: the graph reads the new rows
    assert not np.array_equal(other[:4, ::20], rows[:4, ::20])
    graph.load_epoch(items, None, None, None, other)
    graph.replay()
    torch.cuda.synchronize()
    fresh = ds.host_batch(items, 0, 4, blur=other)
    assert int(ds.cursor.cpu()) == 4 and torch.equal(graph.real_A, fresh[0]) and torch.equal(graph.real_B, fresh[1])
