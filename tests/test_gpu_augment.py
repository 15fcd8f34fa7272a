"""Augmented training batches on the GPU: ``afcm_batch_assemble_aug`` against ``DeviceSliceSet.host_batch(..., augment=...)`` -- stacked
``SliceDataset`` items through ``np.flip`` / ``np.rot90`` / ``scipy.ndimage.rotate`` as the reference's classes call them (afcm_amd/augment.py, held to
the reference's golden and to the numpy restatement by tests/test_augment_ref_cpu.py).  Every comparison is of bit patterns.  The shapes are the
smallest at which the kernel can go wrong: patches of at most 40 pixels a side that are padded in one axis and cropped in the other, widths that are
no multiple of the run of 4 (fp32) or 8 (16-bit) pixels, more than one workgroup, zero planes at both ends of a volume."""
import numpy as np
import pytest
import torch

import train_batch_ref as T
from afcm_amd import augment as A

pytestmark = pytest.mark.gpu

_BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
FULL = A.AugmentConfig(flip_axes=(1, 2), rotate90=True, angle_spectrum=45)
OBLONG = A.AugmentConfig(flip_axes=(1, 2), angle_spectrum=45)


def _same_bits(got, want):
    got, want = got.cpu(), torch.as_tensor(want).cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    assert not bool(torch.isnan(want).any())
    differing = int((got.view(_BITS[want.dtype]) != want.view(_BITS[want.dtype])).sum())
    assert differing == 0, f'{differing} of {want.numel()} elements differ'


def _set(sources, hw, k, config, dtype=np.uint8, thickness=(2,)):
    from afcm_amd.training import DeviceSliceSet
    lo, hi = T.value_range(dtype)
    return DeviceSliceSet(sources, patch_shape=(1,) + hw, raw_internal_path_in=['t1'], raw_internal_path_out=['t2'], thickness=thickness, slice_num=k,
                          min_value=lo, max_value=hi, device='cuda', augment=config)


def _launch(ds, items, rows, first=0, count=None, **kw):
    """The op on tables of the test's own (any number of rows): what ``ds.batch`` launches on the set's persistent ones."""
    from afcm_amd.torch_utils.ops.batch_ops import assemble_batch
    count = len(items) - first if count is None else count
    return assemble_batch(ds.pool, ds.vols, torch.from_numpy(items).cuda(), first, count, ds.patch_shape[1:], slice_num=ds.slice_num, min_value=ds.min_value,
                          max_value=ds.max_value, augment=None if rows is None else torch.from_numpy(rows).cuda(), **kw)


def _two_subjects():
    """7-deep uint8 volumes of 13 x 20 and 20 x 13: into 16 x 16 one is padded in H and cropped in W, the other the reverse."""
    from volume_ref import source
    return [{m: source(shape, np.uint8, seed=40 + 2 * s + j) for j, m in enumerate(('t1', 't2'))} for s, shape in enumerate(((7, 13, 20), (7, 20, 13)))]


@pytest.mark.parametrize('k', [4, 1])
def test_every_flip_and_quarter_turn_at_37_degrees(k):
    ds = _set(_two_subjects(), (16, 16), k, FULL)
    combos = [(fh, fw, q) for fh in (0, 1) for fw in (0, 1) for q in range(4)]
    # the first and the last slice of each subject: with thickness 2 the planes at idx_a - 2 and idx_a + 2, + 4 lie outside the volume
    items = np.array([(2 * s, 2 * s + 1, idx, 2) for s in (0, 1) for idx in (0, 6) for _ in combos], dtype=np.int32)
    fh, fw, q = (np.tile(np.array(c), 4) for c in zip(*combos))
    rows = A.make_rows(fh, fw, q, 37, (16, 16))
    assert len(items) == len(rows) == 64
    want = ds.host_batch(items, 0, 64, augment=rows)
    got = _launch(ds, items, rows)
    for g, w in zip(got, want):
        _same_bits(g, w)
    plain = ds.host_batch(items, 0, 64)
    assert not torch.equal(want[0], plain[0]) and torch.equal(want[2], plain[2])
    if k == 4:                                                                    # the zero planes are there, and constant after the gather
        background = float(np.float32(-1.0))
        assert bool((got[0][0, 0] == background).all()) and bool((got[0][16, 3] == background).all()) and not bool((got[0][0, 1] == background).all())


def test_oblong_patch_at_every_angle_of_the_spectrum():
    """12 x 18: not square, 18 a multiple of neither 4 nor 8, so every row ends in the element-by-element tail; every integer angle -45 ... 44 under
    each of the four flips, over the 23 shuffled rows of the shared subjects (crops of different parities)."""
    ds = _set(T.subjects(np.uint8), (12, 18), 4, OBLONG, thickness=T.THICKNESSES)
    base = T.shuffled_items(4)
    angles = np.tile(np.arange(-45, 45), 4)
    flips = np.repeat(np.arange(4), 90)
    items = base[np.arange(360) % 23]
    rows = A.make_rows(flips // 2, flips % 2, 0, angles, (12, 18))
    want = ds.host_batch(items, 0, 360, augment=rows)
    for dtype in (torch.float32, torch.bfloat16):
        got = _launch(ds, items, rows, dtype=dtype)
        _same_bits(got[0], want[0].to(dtype))
        _same_bits(got[1], want[1].to(dtype))
        _same_bits(got[2], want[2])


def test_many_reflect_periods():
    """2 x 40 at 90 degrees: a row of the output walks 40 pixels along an axis of 2, ten periods of the reflection; 37 degrees: both axes leave."""
    ds = _set(T.subjects(np.uint8), (2, 40), 4, OBLONG, thickness=T.THICKNESSES)
    items = T.shuffled_items(4)[:16]
    rows = A.make_rows(np.arange(16) % 2, np.arange(16) // 2 % 2, 0, np.where(np.arange(16) < 8, 90, 37), (2, 40))
    want = ds.host_batch(items, 0, 16, augment=rows)
    for g, w in zip(_launch(ds, items, rows), want):
        _same_bits(g, w)


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_source_dtypes_and_16bit_outputs(dtype):
    ds = _set(T.subjects(dtype), (16, 16), 4, FULL, dtype=dtype, thickness=T.THICKNESSES)
    items = T.shuffled_items(4)
    rows = ds.epoch_augment(12)
    assert len({tuple(r[:3]) for r in rows}) > 8 and len(set(rows[:, 3])) > 12
    want = ds.host_batch(items, 0, 23, augment=rows)
    ds.load_epoch(items, rows)
    batches = list(ds.batches(T.BATCH))                                           # the set's own tables, batch by batch, the ragged last one included
    assert [int(b[0].shape[0]) for b in batches] == [5, 5, 5, 5, 3]
    for j in range(3):
        _same_bits(torch.cat([b[j] for b in batches]), want[j])
    for out_dtype in (torch.float16, torch.bfloat16):                             # one more rounding of the fp32 result
        a, b, c = ds.batch(0, 23, dtype=out_dtype)
        _same_bits(a, want[0].to(out_dtype))
        _same_bits(b, want[1].to(out_dtype))
        _same_bits(c, want[2])


@pytest.mark.parametrize('hw', [(16, 16), (12, 10)])
def test_identity_rows_give_the_plain_launch_bit_for_bit(hw):
    ds = _set(T.subjects(np.int16), hw, 4, OBLONG, dtype=np.int16, thickness=T.THICKNESSES)
    items = T.shuffled_items(4)
    for dtype in (torch.float32, torch.float16):
        plain = _launch(ds, items, None, dtype=dtype)
        got = _launch(ds, items, A.identity_rows(23), dtype=dtype)
        for g, w in zip(got, plain):
            _same_bits(g, w)
    ds.load_epoch(items)                                                          # a configured set that is given no rows loads identity rows
    assert torch.equal(ds.augment_table.cpu(), torch.from_numpy(A.identity_rows(23)))
    plain = _launch(ds, items, None, first=5, count=5)
    out = (torch.full((5, 4) + hw, 7., device='cuda'), torch.full((5, 1) + hw, 7., device='cuda'), torch.full((5, 1), 7., device='cuda'))
    got = ds.batch(5, 5, out=out)
    assert all(g is o for g, o in zip(got, out))
    for g, w in zip(out, plain):
        _same_bits(g, w)
    # rows past a short epoch are identity rows again, whatever the table held
    ds.load_epoch(items, ds.epoch_augment(1))
    ds.load_epoch(items[:10], ds.epoch_augment(2, rows=10))
    assert torch.equal(ds.augment_table[10:].cpu(), torch.from_numpy(A.identity_rows(13))) and bool((ds.items[10:] == -1).all())


def test_cursor_moves_through_both_tables():
    from afcm_amd.torch_utils.ops.batch_ops import advance_cursor
    ds = _set(T.subjects(np.uint8), (16, 16), 4, FULL, thickness=T.THICKNESSES)
    items, rows = T.shuffled_items(4), ds.epoch_augment(3)
    want = ds.host_batch(items, 0, 23, augment=rows)
    ds.load_epoch(items, rows)
    got = []
    for _ in range(2):
        got.append(ds.batch(0, 5, use_cursor=True))
        advance_cursor(ds.cursor, 5)
    assert int(ds.cursor.cpu()) == 10
    for j in range(3):
        _same_bits(torch.cat([g[j] for g in got]), want[j][:10])
    tail = ds.batch(8, 5, use_cursor=True)                                        # first counts from the cursor: rows 18 ... 22
    for t, w in zip(tail, want):
        _same_bits(t, w[18:23])
    past = ds.batch(10, 5, use_cursor=True)                                       # rows 20 ... 24: two past the table
    assert all(bool(torch.isnan(t[3:]).all()) for t in past)
    for t, w in zip(past, want):
        _same_bits(t[:3], w[20:23])


def test_invalid_parameter_rows_are_nan_items_and_their_neighbours_are_untouched():
    ds = _set(T.subjects(np.uint8), (16, 16), 4, FULL, thickness=T.THICKNESSES)
    items, rows = T.shuffled_items(4), ds.epoch_augment(4)
    clean = _launch(ds, items, rows)
    assert not any(bool(torch.isnan(c).any()) for c in clean)
    bad = {'flip_h of 2': (0, 2.0), 'flip_w of 2': (1, 2.0), 'flip of one half': (0, 0.5), 'k of 4': (2, 4.0), 'k negative': (2, -1.0), 'k of 1.5': (2, 1.5),
           'c not a number': (4, np.nan), 'c of 2': (4, 2.0), 's of -1.5': (5, -1.5), 's infinite': (5, np.inf), 'off_y of h + w + 1': (6, 33.0),
           'off_x of -(h + w + 1)': (7, -33.0), 'off_x not a number': (7, np.nan)}
    table = rows.copy()
    at = [1 + j + (j >= 6) * 3 for j in range(len(bad))]                          # rows 1 ... 6 and 10 ... 16: valid rows before, between and after
    keep = sorted(set(range(23)) - set(at))
    for row, (col, value) in zip(at, bad.values()):
        table[row, col] = value
    edge = table.copy()
    edge[keep, 6:] = [32.0, -32.0]                                                # |off| = h + w itself is valid
    for k in (4, 1):
        ds.slice_num = k                                                          # the same pool and tables as one-plane items
        reference = _launch(ds, items, rows)
        got = _launch(ds, items, table)
        for g, c in zip(got, reference):
            nan_items = torch.isnan(g).reshape(23, -1).cpu()
            assert bool(nan_items[at].all()), [name for name, row in zip(bad, at) if not bool(nan_items[row].all())]
            assert not bool(nan_items[keep].any())
            _same_bits(g.cpu()[keep], c.cpu()[keep])
        assert not bool(torch.isnan(_launch(ds, items, edge)[0].cpu()[keep]).any())
    ds.slice_num = 4
    # an invalid ITEM row with a valid parameter row: the same NaN item
    broken = items.copy()
    for j, row in enumerate(sorted(T.invalid_rows(ds.vols_host).values())):
        broken[1 + 2 * j] = row
    got = _launch(ds, broken, rows)
    want = T.assemble_batch(*T.pool_and_table(ds.volumes, ('t1', 't2')), broken, 0, 23, 4, 16, 16)
    for g, w, c in zip(got, want, clean):
        nan = torch.from_numpy(np.isnan(w))
        assert bool(nan.any()) and torch.equal(torch.isnan(g).cpu(), nan)
        assert torch.equal(g.cpu()[~nan].view(torch.int32), c.cpu()[~nan].view(torch.int32))
    # an odd number of quarter turns on an oblong patch
    ob = _set(T.subjects(np.uint8), (12, 18), 4, OBLONG, thickness=T.THICKNESSES)
    turned = A.identity_rows(23)
    turned[3, 2], turned[7, 2], turned[9, 2] = 1.0, 3.0, 2.0
    got = _launch(ob, items, turned)
    plain = _launch(ob, items, None)
    for g, c in zip(got, plain):
        nan_items = torch.isnan(g).reshape(23, -1).cpu()
        assert bool(nan_items[[3, 7]].all()) and int(nan_items.any(dim=1).sum()) == 2
        rest = sorted(set(range(23)) - {3, 7, 9})
        _same_bits(g.cpu()[rest], c.cpu()[rest])
    _same_bits(got[0][9], torch.flip(plain[0][9], (1, 2)))                        # two quarter turns: valid on any patch


def test_host_checks_raise_before_any_launch():
    from afcm_amd import _lib
    from afcm_amd.torch_utils.ops.batch_ops import assemble_batch
    ds = _set(T.subjects(np.uint8), (16, 16), 4, FULL, thickness=T.THICKNESSES)
    items = torch.from_numpy(T.shuffled_items(4)).cuda()
    rows = torch.from_numpy(A.identity_rows(23)).cuda()
    out = (torch.full((2, 4, 16, 16), 7., device='cuda'), torch.full((2, 1, 16, 16), 7., device='cuda'), torch.full((2, 1), 7., device='cuda'))
    for bad, message in [(rows.float(), 'augment table must be a contiguous torch.float64'), (rows[:, :7], 'augment table must be a contiguous torch.float64'),
                         (rows.t().contiguous().t(), 'augment table must be a contiguous'), (rows.reshape(-1), 'augment table must be a contiguous'),
                         (rows.cpu().numpy(), 'augment table must be a contiguous'), (rows[:22], 'has 22 rows, the item table 23'),
                         (torch.cat([rows, rows]), 'has 46 rows, the item table 23'), (rows.cpu(), 'no CPU')]:
        with pytest.raises(RuntimeError, match=message):
            assemble_batch(ds.pool, ds.vols, items, 0, 2, (16, 16), out=out, augment=bad)
    with pytest.raises(RuntimeError, match=r'float64 \[23, 8\]'):
        ds.load_epoch(T.shuffled_items(4), A.identity_rows(22))
    with pytest.raises(RuntimeError, match=r'float64 \[10, 8\]'):
        ds.load_epoch(T.shuffled_items(4)[:10], A.identity_rows(23))
    plain = _set(T.subjects(np.uint8), (16, 16), 4, None, thickness=T.THICKNESSES)
    assert plain.augment_table is None
    with pytest.raises(RuntimeError, match='built without augment'):
        plain.load_epoch(T.shuffled_items(4), A.identity_rows(23))

    lib = _lib.load()
    args = dict(a=out[0].data_ptr(), b=out[1].data_ptr(), slice_idx=out[2].data_ptr(), pool=ds.pool.data_ptr(), pool_elems=ds.pool.numel(),
                src_dtype=_lib.SRC_U8, vols=ds.vols.data_ptr(), n_vols=6, items=items.data_ptr(), n_items=23, augment=rows.data_ptr(), cursor=None, first=0,
                count=2, k=4, h=16, w=16, out_dtype=_lib.F32, min_value=0., max_value=255., stream=_lib.stream_ptr(ds.pool))
    for edit, message in [(dict(augment=None), 'null augment table'), (dict(items=None), 'null output'), (dict(k=2), 'slice number 2 is not 1 or 4'),
                          (dict(src_dtype=4), 'source dtype 4'), (dict(count=0), 'every extent must be positive'),
                          (dict(h=1 << 27, w=(1 << 27) + 1), 'h + w above 2^28')]:
        rc = lib.afcm_batch_assemble_aug(*dict(args, **edit).values())
        assert rc == _lib.E_INVALID and message in lib.afcm_last_error().decode(), (edit, rc, lib.afcm_last_error())
    torch.cuda.synchronize()
    assert all(bool((t == 7.).all()) for t in out)                                # nothing was launched
    assert lib.afcm_batch_assemble_aug(*args.values()) == 0                       # the unedited call is a good one
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out[0]).any()) and float(out[0].abs().max()) <= 1.


# ---- the training loops on the tiny 128^2 generator of test_gpu_train_batch.py ---------------------------------------------------------------

def _tiny_augmented_set():
    from afcm_amd.training import DeviceSliceSet
    from test_gpu_train_batch import _tiny_set
    plain, items = _tiny_set()
    ds = DeviceSliceSet(plain.volumes, patch_shape=(1, 128, 128), raw_internal_path_in=['t1'], raw_internal_path_out=['t2'], thickness=[5], device='cuda',
                        augment=FULL)
    assert np.array_equal(ds.epoch_items(11), items)                              # the item draw does not know about the augmentation
    return ds, items, ds.epoch_augment(21)


def test_train_epoch_device_and_host_arms_leave_the_same_bits():
    from afcm_amd.training import train_epoch
    from test_gpu_train_batch import _state, _tiny_step
    ds, items, rows = _tiny_augmented_set()
    finals = {}
    for arm, augment in (('device', rows), ('host', rows), ('plain', None)):
        step = _tiny_step(ema=True)
        torch.manual_seed(3)                                                      # set_input draws gen_z: the same draws for every arm
        total = train_epoch(step, ds, 4, items[:12], total_iters=100, ema_kimgs=10.0, ramp=0.05, where='host' if arm == 'host' else 'device',
                            augment=None if augment is None else augment[:12])
        assert total == 112
        finals[arm] = _state(step)
        assert all(bool(torch.isfinite(t).all()) for t in finals[arm])
    assert all(torch.equal(a, b) for a, b in zip(finals['device'], finals['host']))
    assert any(not torch.equal(a, b) for a, b in zip(finals['device'], finals['plain']))       # the augmentation did reach the step


def test_training_graph_replays_equal_eager_steps():
    """As tests/test_gpu_train_batch.py's test of the same name (bfloat16 compute, three warm-up steps and three replays against six eager steps),
    with the augmented launch inside the graph."""
    from afcm_amd.training import TrainingGraph, train_epoch
    from test_gpu_train_batch import _tiny_step
    ds, items, rows = _tiny_augmented_set()
    items, rows = items[:12], rows[:12]
    z = torch.randn(4, 32, generator=torch.Generator().manual_seed(9)).cuda()
    eager = _tiny_step(compute_dtype=torch.bfloat16, capturable=True)
    for _ in range(2):
        train_epoch(eager, ds, 4, items, gen_z=z, augment=rows)
    want = [p.detach().clone() for p in eager.netG.parameters()]

    step = _tiny_step(compute_dtype=torch.bfloat16, capturable=True)
    ds.load_epoch(items, rows)
    graph = TrainingGraph(step, ds, 4, warmup=3, fixed_z=True, gen_z=z)
    assert int(ds.cursor.cpu()) == 0 and ds.position == 0
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(ds.cursor.cpu()) == 12 and step.optimizer_G.device_step() == 6
    for a, b in zip(step.netG.parameters(), want):
        assert torch.equal(a.detach(), b)
    fresh = ds.host_batch(items, 8, 4, augment=rows)                              # the last replay's batch: rows 8 ... 11 of both tables
    assert torch.equal(graph.real_A, fresh[0]) and torch.equal(graph.real_B, fresh[1]) and torch.equal(graph.slice_idx, fresh[2])
    other = ds.epoch_augment(22, rows=12)                                         # refreshed in place: the graph reads the new rows
    graph.load_epoch(items, other)
    graph.replay()
    torch.cuda.synchronize()
    fresh = ds.host_batch(items, 0, 4, augment=other)
    assert int(ds.cursor.cpu()) == 4 and torch.equal(graph.real_A, fresh[0]) and torch.equal(graph.real_B, fresh[1])


def test_train_epochs_with_and_without_the_graph():
    """The outer loop on the bfloat16 generator step with a schedule and an EMA copy (the step whose replays equal eager steps bit for bit, as in
    ``test_training_graph_replays_equal_eager_steps``): two epochs of 18 rows in batches of 2, each with its own draw of items and parameter rows."""
    from afcm_amd.schedule import LRSchedule
    from afcm_amd.training import train_epochs
    from test_gpu_schedule import _schedule
    from test_gpu_train_batch import _state, _tiny_step
    ds, _, _ = _tiny_augmented_set()
    z = torch.randn(2, 32, generator=torch.Generator().manual_seed(10)).cuda()
    lrs = LRSchedule('linear', 0.0002, epoch_count=1, n_epochs=2, n_epochs_decay=2)
    rng = np.random.default_rng(5)                                                # per epoch: the items, then the parameter rows, on one generator
    for _ in range(2):
        last_items, last_rows = ds.epoch_items(rng), ds.epoch_augment(rng)
    finals = {}
    for graph in (True, False):
        step = _tiny_step(compute_dtype=torch.bfloat16, capturable=True, ema=True, schedule=_schedule(ema_kimgs=10.0, ramp=0.05))
        before = _state(step)
        assert train_epochs(step, ds, 2, range(1, 3), lrs, 5, graph=graph, gen_z=z) == 18
        assert torch.equal(ds.items.cpu(), torch.from_numpy(last_items)) and torch.equal(ds.augment_table.cpu(), torch.from_numpy(last_rows))
        assert step.schedule.read()['total_iters'] == 36.0 and step.optimizer_G.device_step() == 18
        finals[graph] = _state(step)
        assert any(not torch.equal(p, q) for p, q in zip(finals[graph], before))
    assert len(finals[True]) == len(finals[False]) and all(torch.equal(p, q) for p, q in zip(finals[True], finals[False]))
    assert all(bool(torch.isfinite(p).all()) for p in finals[True])
