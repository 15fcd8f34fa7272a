"""Training batches with an elastic deformation on the GPU: ``afcm_batch_assemble_elastic`` against ``DeviceSliceSet.host_batch(..., elastic=...)`` --
stacked ``SliceDataset(phase='train')`` items through ``afcm_amd.augment_elastic.apply_host``, the numpy arm that
tests/test_augment_elastic_ref_cpu.py holds to scipy and to the golden captured from the reference's class.  Every comparison is of bit patterns.
The shapes are the smallest at which the kernels can go wrong: 24 x 40 and 21 x 37 (no multiple of the 4-pixel run, of the 16 x 64 smoothing tile
or of the 64-line prefilter block; h != w), cut from 26 x 38 and 22 x 45 sources (a crop and a pad in each), more than one workgroup per launch,
the first and the last slice of a 7-deep volume (thick-slice planes outside it are deformed constants).  One further case runs 70 x 130, where the
smoothing sum and the prefilter's LDS transpose take more than one 64-wide block."""
import ctypes

import numpy as np
import pytest
import torch

import augment_elastic_ref as R
import train_batch_ref as T
from afcm_amd import augment as A
from afcm_amd import augment_elastic as E
from afcm_amd import augment_intensity as I

pytestmark = pytest.mark.gpu

_BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
GEO = A.AugmentConfig(flip_axes=(1, 2), angle_spectrum=45)
NOISE = I.IntensityConfig(contrast=(0.5, 1.5, 0.0, 0.6), gaussian=(0.0, 1.0, 0.6), poisson=(0.0, 1.0, 0.6))
SHAPES = [(24, 40), (21, 37)]
# three items: the first slice of subject 0 (planes at -2 outside), the last of subject 1 (planes at +2, +4 outside), one inside
THREE = np.array([(0, 1, 0, 2), (2, 3, 6, 2), (0, 1, 3, 2)], dtype=np.int32)


def _config(order=3, sigma=2.0, alpha=30.0, p=0.5):
    return E.ElasticConfig(spline_order=order, alpha=alpha, sigma=sigma, execution_probability=p)


def _same_bits(got, want):
    got, want = got.cpu(), torch.as_tensor(want).cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    assert not bool(torch.isnan(want).any())
    differing = int((got.view(_BITS[want.dtype]) != want.view(_BITS[want.dtype])).sum())
    assert differing == 0, f'{differing} of {want.numel()} elements differ'


def _sources(shapes=((7, 26, 38), (7, 22, 45)), dtype=np.uint8):
    from volume_ref import source
    return [{m: source(shape, dtype, seed=80 + 2 * s + j) for j, m in enumerate(('t1', 't2'))} for s, shape in enumerate(shapes)]


def _set(hw, k, elastic, sources=None, augment=None, intensity=None, dtype=np.uint8, thickness=(2,)):
    from afcm_amd.training import DeviceSliceSet
    lo, hi = T.value_range(dtype)
    return DeviceSliceSet(_sources() if sources is None else sources, patch_shape=(1,) + hw, raw_internal_path_in=['t1'], raw_internal_path_out=['t2'],
                          thickness=thickness, slice_num=k, min_value=lo, max_value=hi, device='cuda', augment=augment, intensity=intensity, elastic=elastic)


def _launch(ds, items, rows, geo=None, noise=None, first=0, count=None, ops=None, **kw):
    """The op on tables of the test's own (any number of rows): what ``ds.batch`` launches on the set's persistent ones."""
    from afcm_amd.torch_utils.ops.batch_ops import assemble_batch
    count = len(items) - first if count is None else count
    more = {} if rows is None else dict(elastic=torch.from_numpy(rows).cuda(), elastic_ops=ds.elastic_ops if ops is None else ops)
    return assemble_batch(ds.pool, ds.vols, torch.from_numpy(items).cuda(), first, count, ds.patch_shape[1:], slice_num=ds.slice_num, min_value=ds.min_value,
                          max_value=ds.max_value, augment=None if geo is None else torch.from_numpy(geo).cuda(),
                          intensity=None if noise is None else torch.from_numpy(noise).cuda(), **more, **kw)


def _rows(flags, alpha, seed=1):
    rows = E.identity_rows(len(flags))
    rows[:, 0], rows[:, 1] = flags, alpha
    rows[:, 2:] = np.random.default_rng(seed).integers(0, 2 ** 32, (len(flags), 2))
    return rows


@pytest.mark.parametrize('k', [4, 1])
@pytest.mark.parametrize('order', [0, 1, 3])
@pytest.mark.parametrize('hw', SHAPES)
def test_orders_shapes_and_slice_counts(hw, order, k):
    """A flag-0 item between two flag-1 items, twice; float32, both 16-bit outputs and ``out=``."""
    ds = _set(hw, k, _config(order))
    items = np.concatenate([THREE, THREE[::-1]])
    rows = _rows([1, 0, 1, 1, 0, 1], 30.0)
    want = ds.host_batch(items, 0, 6, elastic=rows)
    plain = ds.host_batch(items, 0, 6)
    for j in range(6):                                                            # the flag decides, and the label is never touched
        assert torch.equal(want[0][j], plain[0][j]) == (rows[j, 0] == 0) and torch.equal(want[1][j], plain[1][j]) == (rows[j, 0] == 0)
    assert torch.equal(want[2], plain[2])
    if order == 3:
        assert float(want[1].abs().max()) > 1.0                                   # cubic overshoot past the normalised range: no clip
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        got = _launch(ds, items, rows, dtype=dtype)
        _same_bits(got[0], want[0].to(dtype))
        _same_bits(got[1], want[1].to(dtype))
        _same_bits(got[2], want[2])
    out = (torch.full((6, k) + hw, 7., device='cuda'), torch.full((6, 1) + hw, 7., device='cuda'), torch.full((6, 1), 7., device='cuda'))
    got = _launch(ds, items, rows, out=out)
    assert all(g is o for g, o in zip(got, out))
    for g, w in zip(out, want):
        _same_bits(g, w)
    if k == 4:                                                                    # a constant plane outside the volume stays that constant, to rounding
        assert bool((plain[0][0, 0] == -1.0).all()) and float((want[0][0, 0] + 1.0).abs().max()) < 1e-6


@pytest.mark.parametrize('order', [1, 3])
@pytest.mark.parametrize('hw', SHAPES)
def test_sigma_50_and_displacements_of_several_periods(hw, order):
    """The reference's sigma on a small plane: 401 taps folded over 21 to 40 pixels; ten times its alpha, so that the coordinates wrap several
    periods (2n) of the plane; and |alpha| at its bound."""
    ds = _set(hw, 4, _config(order, sigma=50.0, alpha=20000.0))
    assert bool((ds.elastic_ops[0] > 0).all())                                    # a full operator, where sigma 2 gives a banded one
    items = THREE
    rows = _rows([1, 1, 1], 20000.0, seed=4)
    rows[2, 1] = -2.0 ** 20
    dy, dx = E.displacement_host(rows[0], *hw, *ds.elastic_ops_host)
    assert max(np.abs(dy).max(), np.abs(dx).max()) > 4 * max(hw)                  # more than two periods of the longer axis
    want = ds.host_batch(items, 0, 3, elastic=rows)
    for g, w in zip(_launch(ds, items, rows), want):
        _same_bits(g, w)


def test_blocks_of_the_smoothing_sum_and_of_the_transpose():
    """70 x 130: the smoothing sums run over two and three 64-blocks of m, the prefilter's rows pass through LDS in three column blocks and two
    row blocks, every one with a partial last block."""
    hw = (70, 130)
    ds = _set(hw, 1, _config(3, sigma=6.0, alpha=300.0), sources=_sources(((3, 75, 120), (3, 66, 140))), thickness=())
    items = np.array([(0, 1, 1, -1), (2, 3, 2, -1)], dtype=np.int32)
    rows = _rows([1, 1], 300.0, seed=6)
    want = ds.host_batch(items, 0, 2, elastic=rows)
    for g, w in zip(_launch(ds, items, rows), want):
        _same_bits(g, w)


@pytest.mark.parametrize('with_geo', [False, True])
@pytest.mark.parametrize('with_noise', [False, True])
def test_between_the_geometric_and_the_intensity_stage(with_geo, with_noise):
    hw = (21, 37)
    ds = _set(hw, 4, _config(3), augment=GEO if with_geo else None, intensity=NOISE if with_noise else None)
    items = np.concatenate([THREE, THREE])
    rows = _rows([1, 0, 1, 0, 1, 1], 30.0, seed=2)
    geo = ds.epoch_augment(5, rows=6) if with_geo else None
    noise = ds.epoch_intensity(12, rows=6) if with_noise else None
    assert noise is None or noise[:, [0, 3, 5]].sum() >= 4
    want = ds.host_batch(items, 0, 6, augment=geo, intensity=noise, elastic=rows)
    before = ds.host_batch(items, 0, 6, augment=geo)
    for j in (0, 2):                                                              # the composition, said once more: rotate, deform, then noise
        a = E.apply_host(torch.cat([before[0][j], before[1][j]]).cpu(), rows[j], ds.elastic, ds.elastic_ops_host)
        if with_noise:
            a = torch.cat([I.apply_host(a[:4], noise[j], False, 0), I.apply_host(a[4:], noise[j], False, 4)])
        assert torch.equal(want[0][j].cpu(), a[:4]) and torch.equal(want[1][j].cpu(), a[4:])
    for dtype in (torch.float32, torch.float16):
        got = _launch(ds, items, rows, geo, noise, dtype=dtype)
        _same_bits(got[0], want[0].to(dtype))
        _same_bits(got[1], want[1].to(dtype))
        _same_bits(got[2], want[2])
    # a table whose flags are all 0 gives the launch without it, whatever alpha and the keys say
    quiet = _rows([0] * 6, 55.0, seed=3)
    for g, w in zip(_launch(ds, items, quiet, geo, noise), _launch(ds, items, None, geo, noise)):
        _same_bits(g, w)


@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
def test_the_sets_own_tables_a_ragged_last_batch_and_the_cursor(dtype):
    from afcm_amd.torch_utils.ops.batch_ops import advance_cursor
    hw = (24, 40)
    ds = _set(hw, 4, _config(3, p=0.6), sources=T.subjects(dtype), dtype=dtype, thickness=T.THICKNESSES, augment=GEO)
    items, geo, rows = T.shuffled_items(4), ds.epoch_augment(3), ds.epoch_elastic(4)
    assert rows.shape == (23, 4) and 6 <= rows[:, 0].sum() <= 20
    want = ds.host_batch(items, 0, 23, augment=geo, elastic=rows)
    ds.load_epoch(items, geo, None, rows)
    assert torch.equal(ds.elastic_table.cpu(), torch.from_numpy(rows))
    batches = list(ds.batches(T.BATCH))
    assert [int(b[0].shape[0]) for b in batches] == [5, 5, 5, 5, 3]
    for j in range(3):
        _same_bits(torch.cat([b[j] for b in batches]), want[j])
    got = []
    for _ in range(2):
        got.append(ds.batch(0, 5, use_cursor=True))
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
    assert torch.equal(ds.elastic_table.cpu(), torch.from_numpy(E.identity_rows(23)))
    for g, w in zip(ds.batch(0, 10), ds.host_batch(items, 0, 10, augment=geo)):
        _same_bits(g, w)


def test_invalid_rows_are_nan_items_and_their_neighbours_are_untouched():
    hw = (21, 37)
    ds = _set(hw, 4, _config(3), intensity=NOISE)
    n = len(R.INVALID) + 4
    items = THREE[np.arange(n) % 3]
    good = _rows([1, 0] * (n // 2), 30.0, seed=7)
    good[:, 1], good[0, 2], good[1, 3] = -2.0 ** 20, 2.0 ** 32 - 1, 2.0 ** 32 - 1    # the boundary of validity is valid
    noise = ds.epoch_intensity(9, rows=n)
    want = ds.host_batch(items, 0, n, intensity=noise, elastic=good)
    at, keep = list(range(2, 2 + len(R.INVALID))), [0, 1, n - 2, n - 1]
    table = good.copy()
    for row, (col, value) in zip(at, R.INVALID.values()):
        table[row, col] = value
        assert not E.row_is_valid(table[row])
    for with_noise in (noise, None):
        got = _launch(ds, items, table, None, with_noise)
        for g, w in zip(got, want if with_noise is not None else ds.host_batch(items, 0, n, elastic=good)):
            nan_items = torch.isnan(g).reshape(n, -1).cpu()
            assert bool(nan_items[at].all()), [name for name, row in zip(R.INVALID, at) if not bool(nan_items[row].all())]
            assert not bool(nan_items[keep].any())
            _same_bits(g.cpu()[keep], w[keep])
    # an invalid item row or intensity row beside valid elastic rows: NaN items, label included, and only those
    bad_items, bad_noise = items.copy(), noise.copy()
    bad_items[3, 0], bad_noise[5, 9] = 99, np.nan
    for g, w in zip(_launch(ds, bad_items, good, None, bad_noise), want):
        nan_items = torch.isnan(g).reshape(n, -1).cpu()
        assert bool(nan_items[[3, 5]].all()) and int(nan_items.any(dim=1).sum()) == 2
        rest = sorted(set(range(n)) - {3, 5})
        _same_bits(g.cpu()[rest], w[rest])


@pytest.mark.parametrize('order', [0, 1, 3])
def test_a_nan_in_the_operator_is_nan_pixels_in_the_executing_items_only(order):
    hw = (24, 40)
    ds = _set(hw, 4, _config(order))
    items = np.concatenate([THREE, THREE])
    rows = _rows([1, 0, 1, 0, 0, 1], 30.0, seed=8)
    clean = _launch(ds, items, rows)
    for which, at in ((0, (5, 7)), (1, (30, 31))):                                # one NaN in op_h, then one in op_w
        ops = [ds.elastic_ops[0].clone(), ds.elastic_ops[1].clone(), order]
        ops[which][at] = float('nan')
        got = _launch(ds, items, rows, ops=tuple(ops))
        for g, c in zip(got[:2], clean[:2]):
            nan = torch.isnan(g).reshape(6, -1).cpu()
            assert bool(nan[[0, 2, 5]].any(dim=1).all()) and not bool(nan[[1, 3, 4]].any())
            assert bool(torch.isfinite(g[[1, 3, 4]]).all())
            _same_bits(g[[1, 3, 4]], c[[1, 3, 4]].cpu())
        _same_bits(got[2], clean[2].cpu())                                        # the rows are valid: the labels stay
    # an operator that sends every coordinate past 2^30: the guard, not an index, decides
    ops = (ds.elastic_ops[0] * 1e15, ds.elastic_ops[1], order)
    got = _launch(ds, items, rows, ops=ops)
    assert bool(torch.isnan(got[0][[0, 2, 5]]).all()) and bool(torch.isfinite(got[0][[1, 3, 4]]).all())


def test_host_checks_and_the_entry_points_refusals():
    from afcm_amd import _lib
    from afcm_amd.torch_utils.ops.batch_ops import assemble_batch, elastic_workspace_bytes
    hw = (24, 40)
    ds = _set(hw, 4, _config(3), sources=T.subjects(np.uint8), thickness=T.THICKNESSES, augment=GEO, intensity=NOISE)
    items = torch.from_numpy(T.shuffled_items(4)).cuda()
    rows = torch.from_numpy(E.identity_rows(23)).cuda()
    out = (torch.full((2, 4) + hw, 7., device='cuda'), torch.full((2, 1) + hw, 7., device='cuda'), torch.full((2, 1), 7., device='cuda'))
    op_h, op_w, order = ds.elastic_ops

    def call(**kw):
        args = dict(elastic=rows, elastic_ops=ds.elastic_ops)
        args.update(kw)
        return assemble_batch(ds.pool, ds.vols, items, 0, 2, hw, out=out, **args)

    for kw, message in [(dict(elastic=rows.float()), 'elastic table must be a contiguous torch.float64'), (dict(elastic=rows[:, :3]), 'elastic table must be'),
                        (dict(elastic=rows[:22]), 'has 22 rows, the item table 23'), (dict(elastic=rows.cpu()), 'no CPU'),
                        (dict(elastic_ops=None), 'go together'), (dict(elastic=None), 'go together'), (dict(elastic_ops=(op_h, op_w)), r'must be \(op_h, op_w, order\)'),
                        (dict(elastic_ops=(op_w, op_w, 3)), r'op_h must be a contiguous torch.float64 \[24, 24\]'),
                        (dict(elastic_ops=(op_h, op_w.float(), 3)), 'op_w must be'), (dict(elastic_ops=(op_h, op_w, 2)), 'spline order must be 0, 1 or 3'),
                        (dict(workspace=torch.empty(64, dtype=torch.uint8, device='cuda')), 'workspace must be a contiguous 1-D uint8 tensor of at least'),
                        (dict(workspace=torch.empty(1 << 20, dtype=torch.float32, device='cuda')), 'workspace must be')]:
        with pytest.raises(RuntimeError, match=message):
            call(**kw)
    with pytest.raises(RuntimeError, match='workspace= only with them'):
        assemble_batch(ds.pool, ds.vols, items, 0, 2, hw, out=out, workspace=torch.empty(64, dtype=torch.uint8, device='cuda'))
    with pytest.raises(RuntimeError, match=r'float64 \[23, 4\]'):
        ds.load_epoch(T.shuffled_items(4), None, None, E.identity_rows(22))
    plain = _set(hw, 4, None, sources=T.subjects(np.uint8), thickness=T.THICKNESSES)
    assert plain.elastic_table is None and plain.elastic_ops is None and plain.elastic_workspace is None
    with pytest.raises(RuntimeError, match='built without elastic'):
        plain.load_epoch(T.shuffled_items(4), None, None, E.identity_rows(23))
    with pytest.raises(RuntimeError, match='built without elastic'):
        plain.epoch_elastic(1)

    lib = _lib.load()
    need, launches = ctypes.c_int64(0), ctypes.c_int32(0)
    assert lib.afcm_elastic_plan(2, 4, 24, 40, 3, ctypes.byref(need), ctypes.byref(launches)) == 0 and launches.value == 8
    assert need.value == elastic_workspace_bytes(2, 4, 24, 40, 3) and need.value >= 2 * 24 * 40 * (5 * 4 + 4 * 8 + 5 * 8)
    less = ctypes.c_int64(0)
    assert lib.afcm_elastic_plan(2, 4, 24, 40, 1, ctypes.byref(less), ctypes.byref(launches)) == 0 and launches.value == 6 and less.value < need.value
    for bad, message in [((2, 4, 24, 40, 2), 'spline order 2'), ((0, 4, 24, 40, 3), '1 to 32767 items'), ((2, 2, 24, 40, 3), 'slice number 2'),
                         ((2, 4, 0, 40, 3), 'extents 1 to 32768'), ((2, 4, 24, 32769, 3), 'extents 1 to 32768')]:
        assert lib.afcm_elastic_plan(*bad, ctypes.byref(less), None) == _lib.E_INVALID and message in lib.afcm_last_error().decode(), bad
    assert lib.afcm_elastic_plan(2, 4, 24, 40, 3, None, None) == _lib.E_INVALID

    work = torch.empty(need.value, dtype=torch.uint8, device='cuda')
    geo_rows, noise_rows = torch.from_numpy(A.identity_rows(23)).cuda(), torch.from_numpy(I.identity_rows(23)).cuda()
    args = dict(a=out[0].data_ptr(), b=out[1].data_ptr(), slice_idx=out[2].data_ptr(), pool=ds.pool.data_ptr(), pool_elems=ds.pool.numel(),
                src_dtype=_lib.SRC_U8, vols=ds.vols.data_ptr(), n_vols=6, items=items.data_ptr(), n_items=23, augment=geo_rows.data_ptr(),
                intensity=noise_rows.data_ptr(), independent_planes=0, elastic=rows.data_ptr(), smooth_h=op_h.data_ptr(), smooth_w=op_w.data_ptr(),
                spline_order=3, workspace=work.data_ptr(), workspace_bytes=need.value, cursor=None, first=0, count=2, k=4, h=24, w=40,
                out_dtype=_lib.F32, min_value=0., max_value=255., stream=_lib.stream_ptr(ds.pool))
    for edit, message in [(dict(elastic=None), 'null elastic table, smoothing operator or workspace'), (dict(smooth_h=None), 'null elastic table'),
                          (dict(smooth_w=None), 'null elastic table'), (dict(workspace=None), 'null elastic table'),
                          (dict(workspace_bytes=need.value - 1), f'afcm_elastic_plan asks for {need.value}'), (dict(workspace_bytes=0), 'afcm_elastic_plan asks'),
                          (dict(workspace=work.data_ptr() + 8), 'multiple of 256 bytes'), (dict(spline_order=2), 'spline order 2 is not 0, 1 or 3'),
                          (dict(spline_order=-1), 'spline order -1'), (dict(independent_planes=2), 'independent_planes 2 is not 0 or 1'),
                          (dict(items=None), 'null output'), (dict(a=None), 'null output'), (dict(k=2), 'slice number 2 is not 1 or 4'),
                          (dict(src_dtype=4), 'source dtype 4'), (dict(out_dtype=3), 'output dtype 3'), (dict(count=0), '1 to 32767 items'),
                          (dict(first=-1), 'first row -1'), (dict(max_value=0.), 'is not above min_value')]:
        rc = lib.afcm_batch_assemble_elastic(*dict(args, **edit).values())
        assert rc == _lib.E_INVALID and message in lib.afcm_last_error().decode(), (edit, rc, lib.afcm_last_error())
    torch.cuda.synchronize()
    assert all(bool((t == 7.).all()) for t in out)                                # nothing was launched
    assert lib.afcm_batch_assemble_elastic(*args.values()) == 0                   # the unedited call is a good one,
    assert lib.afcm_batch_assemble_elastic(*dict(args, augment=None, intensity=None, independent_planes=1, spline_order=0).values()) == 0    # and so is one without the other tables
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out[0]).any()) and float(out[0].abs().max()) <= 1.


# ---- the training loops on the tiny 128^2 generator of test_gpu_train_batch.py ---------------------------------------------------------------

OFTEN = E.ElasticConfig(spline_order=3, alpha=100.0, sigma=8.0, execution_probability=0.5)


def _tiny_elastic_set(augment=None, intensity=None):
    from afcm_amd.training import DeviceSliceSet
    from test_gpu_train_batch import _tiny_set
    plain, items = _tiny_set()
    ds = DeviceSliceSet(plain.volumes, patch_shape=(1, 128, 128), raw_internal_path_in=['t1'], raw_internal_path_out=['t2'], thickness=[5], device='cuda',
                        augment=augment, intensity=intensity, elastic=OFTEN)
    assert np.array_equal(ds.epoch_items(11), items)                              # the item draw does not know about the augmentation
    return ds, items, ds.epoch_elastic(21)


def test_train_epoch_device_and_host_arms_leave_the_same_bits():
    from afcm_amd.training import train_epoch
    from test_gpu_train_batch import _state, _tiny_step
    ds, items, rows = _tiny_elastic_set()
    assert 3 <= rows[:12, 0].sum() <= 9
    finals = {}
    for arm, elastic in (('device', rows), ('host', rows), ('plain', None)):
        step = _tiny_step(ema=True)
        torch.manual_seed(3)                                                      # set_input draws gen_z: the same draws for every arm
        total = train_epoch(step, ds, 4, items[:12], total_iters=100, ema_kimgs=10.0, ramp=0.05, where='host' if arm == 'host' else 'device',
                            elastic=None if elastic is None else elastic[:12])
        assert total == 112
        finals[arm] = _state(step)
        assert all(bool(torch.isfinite(t).all()) for t in finals[arm])
    assert all(torch.equal(a, b) for a, b in zip(finals['device'], finals['host']))
    assert any(not torch.equal(a, b) for a, b in zip(finals['device'], finals['plain']))       # the deformation did reach the step


def test_train_epochs_with_and_without_the_graph():
    """The outer loop on the bfloat16 generator step with a schedule and an EMA copy: two epochs of 18 rows in batches of 2, each with its own draw
    of items, parameter rows, intensity rows and elastic rows, in that order on one generator; ONE captured graph against eager steps."""
    from afcm_amd.schedule import LRSchedule
    from afcm_amd.training import train_epochs
    from test_gpu_schedule import _schedule
    from test_gpu_train_batch import _state, _tiny_step
    ds, _, _ = _tiny_elastic_set(augment=A.AugmentConfig(flip_axes=(1, 2), rotate90=True, angle_spectrum=45), intensity=NOISE)
    z = torch.randn(2, 32, generator=torch.Generator().manual_seed(10)).cuda()
    lrs = LRSchedule('linear', 0.0002, epoch_count=1, n_epochs=2, n_epochs_decay=2)
    rng = np.random.default_rng(5)
    for _ in range(2):
        last = ds.epoch_items(rng), ds.epoch_augment(rng), ds.epoch_intensity(rng), ds.epoch_elastic(rng)
    assert 0 < last[3][:, 0].sum() < 18
    finals = {}
    for graph in (True, False):
        step = _tiny_step(compute_dtype=torch.bfloat16, capturable=True, ema=True, schedule=_schedule(ema_kimgs=10.0, ramp=0.05))
        before = _state(step)
        assert train_epochs(step, ds, 2, range(1, 3), lrs, 5, graph=graph, gen_z=z) == 18
        for table, rows in zip((ds.items, ds.augment_table, ds.intensity_table, ds.elastic_table), last):
            assert torch.equal(table.cpu(), torch.from_numpy(rows))
        assert step.schedule.read()['total_iters'] == 36.0 and step.optimizer_G.device_step() == 18
        finals[graph] = _state(step)
        assert any(not torch.equal(p, q) for p, q in zip(finals[graph], before))
    assert len(finals[True]) == len(finals[False]) and all(torch.equal(p, q) for p, q in zip(finals[True], finals[False]))
    assert all(bool(torch.isfinite(p).all()) for p in finals[True])


def test_training_graph_reads_the_last_batch_of_redrawn_rows():
    from afcm_amd.training import TrainingGraph
    from test_gpu_train_batch import _tiny_step
    ds, items, rows = _tiny_elastic_set()
    items, rows = items[:8], rows[:8]
    z = torch.randn(4, 32, generator=torch.Generator().manual_seed(9)).cuda()
    step = _tiny_step(compute_dtype=torch.bfloat16, capturable=True)
    ds.load_epoch(items, None, None, rows)
    graph = TrainingGraph(step, ds, 4, warmup=2, fixed_z=True, gen_z=z)
    assert int(ds.cursor.cpu()) == 0 and graph.elastic_workspace is ds.elastic_workspace
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    fresh = ds.host_batch(items, 4, 4, elastic=rows)
    assert int(ds.cursor.cpu()) == 8 and torch.equal(graph.real_A, fresh[0]) and torch.equal(graph.real_B, fresh[1]) and torch.equal(graph.slice_idx, fresh[2])
    other = ds.epoch_elastic(23, rows=8)                                          # refreshed in place: the graph reads the new rows
    assert not np.array_equal(other[:4, 0], rows[:4, 0])
    graph.load_epoch(items, None, None, other)
    graph.replay()
    torch.cuda.synchronize()
    fresh = ds.host_batch(items, 0, 4, elastic=other)
    assert int(ds.cursor.cpu()) == 4 and torch.equal(graph.real_A, fresh[0]) and torch.equal(graph.real_B, fresh[1])
