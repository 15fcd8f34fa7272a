"""Training batches with intensity augmentation on the GPU: ``afcm_batch_assemble_noise`` against ``DeviceSliceSet.host_batch(..., intensity=...)`` --
stacked ``SliceDataset`` items through ``afcm_amd.augment_intensity.apply_host``, the numpy arm that tests/test_augment_intensity_ref_cpu.py holds to the
generator's known answers, to ``math`` Box-Muller and to the golden captured from the reference's classes.  Every comparison is of bit patterns.
The shapes are the smallest at which the kernel can go wrong: 12 x 18 patches (18 is a multiple of neither run, 4 pixels fp32 and 8 pixels 16-bit,
so every row ends in a partly used Philox call) cut from 13 x 20 and 20 x 13 sources, 16 x 16, more than one workgroup, the first and the last slice of
a 7-deep volume (the zero planes outside it receive noise as every plane does).
Left out: the ends of u1 (a word pair whose first word is 0 or 2^32 - 1).  Finding a key that puts one into a 12 x 18 field is a 2^-32 event per word,
no cheap search; the series are checked at those arguments on the CPU (test_series_accuracy_against_the_library)."""
import numpy as np
import pytest
import torch

import augment_intensity_ref as R
import train_batch_ref as T
from afcm_amd import augment as A
from afcm_amd import augment_intensity as I

pytestmark = pytest.mark.gpu

_BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
GEO = A.AugmentConfig(flip_axes=(1, 2), angle_spectrum=45)
GEO_SQUARE = A.AugmentConfig(flip_axes=(1, 2), rotate90=True, angle_spectrum=45)
OFTEN = I.IntensityConfig(contrast=(0.5, 1.5, 0.0, 0.6), gaussian=(0.0, 1.0, 0.6), poisson=(0.0, 1.0, 0.6))


def _same_bits(got, want):
    got, want = got.cpu(), torch.as_tensor(want).cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    assert not bool(torch.isnan(want).any())
    differing = int((got.view(_BITS[want.dtype]) != want.view(_BITS[want.dtype])).sum())
    assert differing == 0, f'{differing} of {want.numel()} elements differ'


def _set(sources, hw, k, intensity=OFTEN, augment=None, dtype=np.uint8, thickness=(2,)):
    from afcm_amd.training import DeviceSliceSet
    lo, hi = T.value_range(dtype)
    return DeviceSliceSet(sources, patch_shape=(1,) + hw, raw_internal_path_in=['t1'], raw_internal_path_out=['t2'], thickness=thickness, slice_num=k,
                          min_value=lo, max_value=hi, device='cuda', augment=augment, intensity=intensity)


def _launch(ds, items, rows, geo=None, first=0, count=None, **kw):
    """The op on tables of the test's own (any number of rows): what ``ds.batch`` launches on the set's persistent ones."""
    from afcm_amd.torch_utils.ops.batch_ops import assemble_batch
    count = len(items) - first if count is None else count
    return assemble_batch(ds.pool, ds.vols, torch.from_numpy(items).cuda(), first, count, ds.patch_shape[1:], slice_num=ds.slice_num, min_value=ds.min_value,
                          max_value=ds.max_value, augment=None if geo is None else torch.from_numpy(geo).cuda(),
                          intensity=None if rows is None else torch.from_numpy(rows).cuda(), **kw)


def _two_subjects():
    """7-deep uint8 volumes of 13 x 20 and 20 x 13: into 12 x 18 both are cropped, into 16 x 16 each is padded in one axis and cropped in the other."""
    from volume_ref import source
    return [{m: source(shape, np.uint8, seed=60 + 2 * s + j) for j, m in enumerate(('t1', 't2'))} for s, shape in enumerate(((7, 13, 20), (7, 20, 13)))]


# three items: the first slice of subject 0 (planes at -2 outside), the last of subject 1 (planes at +2, +4 outside), one inside
THREE = np.array([(0, 1, 0, 2), (2, 3, 6, 2), (0, 1, 3, 2)], dtype=np.int32)
# each transform alone, then all three
COMBOS = [dict(contrast=(1, 1.4, 0.1)), dict(gaussian=(1, 0.35)), dict(poisson=(1, 0.8)), dict(contrast=(1, 0.7, -0.2), gaussian=(1, 0.9), poisson=(1, 0.3))]


def _combo_tables(seed=1):
    items = np.repeat(THREE, len(COMBOS), axis=0)
    keys = np.random.default_rng(seed).integers(0, 2 ** 32, (len(items), 2))
    rows = np.concatenate([I.make_rows(keys=keys[j:j + 1], **COMBOS[j % len(COMBOS)]) for j in range(len(items))])
    return items, rows


@pytest.mark.parametrize('k', [4, 1])
@pytest.mark.parametrize('hw', [(12, 18), (16, 16)])
def test_each_transform_alone_and_all_three(hw, k):
    ds = _set(_two_subjects(), hw, k)
    items, rows = _combo_tables()
    want = ds.host_batch(items, 0, len(items), intensity=rows)
    plain = ds.host_batch(items, 0, len(items))
    assert not torch.equal(want[0], plain[0]) and not torch.equal(want[1], plain[1]) and torch.equal(want[2], plain[2])
    assert float(want[0].abs().max()) > 1.0                                       # no clip after the noise
    for dtype in (torch.float32, torch.bfloat16):
        got = _launch(ds, items, rows, dtype=dtype)
        _same_bits(got[0], want[0].to(dtype))
        _same_bits(got[1], want[1].to(dtype))
        _same_bits(got[2], want[2])
    if k == 4:                                                                    # a zero plane outside the volume received the item's noise
        a = got[0].float().cpu()
        assert bool((plain[0][1, 0] == -1.0).all()) and float(a[1, 0].std()) > 0.1 and float(a[5, 3].std()) > 0.1
        # one field for all planes of an item: plane 0 (a constant -1 before) and B carry the same noise up to the rounding
        noise = want[1][1, 0].double() - plain[1][1, 0].double()
        assert float((want[0][1, 0].double() + 1.0 - noise).abs().max()) < 1e-6


@pytest.mark.parametrize('dtype', T.DTYPES)
def test_source_dtypes_and_16bit_outputs(dtype):
    ds = _set(T.subjects(dtype), (12, 18), 4, dtype=dtype, thickness=T.THICKNESSES)
    items = T.shuffled_items(4)
    rows = ds.epoch_intensity(12)
    assert len({tuple(r) for r in rows[:, [0, 3, 5]]}) >= 6
    want = ds.host_batch(items, 0, 23, intensity=rows)
    ds.load_epoch(items, intensity=rows)
    batches = list(ds.batches(T.BATCH))                                           # the set's own tables, batch by batch, the ragged last one included
    assert [int(b[0].shape[0]) for b in batches] == [5, 5, 5, 5, 3]
    for j in range(3):
        _same_bits(torch.cat([b[j] for b in batches]), want[j])
    for out_dtype in (torch.float16, torch.bfloat16):                             # one more rounding of the fp32 result
        a, b, c = ds.batch(0, 23, dtype=out_dtype)
        _same_bits(a, want[0].to(out_dtype))
        _same_bits(b, want[1].to(out_dtype))
        _same_bits(c, want[2])


@pytest.mark.parametrize('independent', [False, True])
@pytest.mark.parametrize('hw,geo', [((12, 18), GEO), ((16, 16), GEO_SQUARE)])
def test_rotated_item_plus_noise_equals_host_rotate_then_noise(hw, geo, independent):
    cfg = I.IntensityConfig(contrast=OFTEN.contrast, gaussian=OFTEN.gaussian, poisson=OFTEN.poisson, independent_planes=independent)
    ds = _set(_two_subjects(), hw, 4, intensity=cfg, augment=geo)
    items, rows = _combo_tables(seed=2)
    geo_rows = ds.epoch_augment(5, rows=len(items))
    assert len(set(geo_rows[:, 3])) > 6
    want = ds.host_batch(items, 0, len(items), augment=geo_rows, intensity=rows)
    turned = ds.host_batch(items, 0, len(items), augment=geo_rows)
    for j in (1, 7):                                                              # the composition, said once more: rotate, then noise
        assert torch.equal(want[0][j].cpu(), I.apply_host(turned[0][j].cpu(), rows[j], independent, 0))
        assert torch.equal(want[1][j].cpu(), I.apply_host(turned[1][j].cpu(), rows[j], independent, 4))
    ds.load_epoch(items, geo_rows, rows)
    for dtype in (torch.float32, torch.float16):
        got = ds.batch(0, len(items), dtype=dtype)
        _same_bits(got[0], want[0].to(dtype))
        _same_bits(got[1], want[1].to(dtype))
        _same_bits(got[2], want[2])
    # without the augment table the same set's launch leaves the rotation out
    flat = _launch(ds, items, rows, independent_planes=independent)
    for g, w in zip(flat, _set(_two_subjects(), hw, 4, intensity=cfg).host_batch(items, 0, len(items), intensity=rows)):
        _same_bits(g, w)
    if independent:                                                               # every plane its own field: the shared-field result differs
        shared = [t.cpu() for t in _launch(ds, items, rows, geo_rows)]
        assert not torch.equal(shared[0][:, 1:], want[0][:, 1:].cpu()) and not torch.equal(shared[1], want[1].cpu())
        assert torch.equal(shared[0][:, 0], want[0][:, 0].cpu())                     # plane 0 is field 0 either way


def test_parameter_edges():
    """std = 0, a lam so small that one or two cut points hold it, lam = 4 (23 cut points), lam = 0, the key's ends, an alpha that clips everything."""
    ds = _set(_two_subjects(), (12, 18), 4)
    specs = [dict(gaussian=(1, 0.0)), dict(poisson=(1, 1e-12)), dict(poisson=(1, 1e-6)), dict(poisson=(1, 4.0)), dict(poisson=(1, 0.0)),
             dict(gaussian=(1, 1.0), poisson=(1, 4.0), keys=(2 ** 32 - 1, 2 ** 32 - 1)), dict(gaussian=(1, 1.0), keys=(0, 0)), dict(contrast=(1, 1e6, 0.0)),
             dict(contrast=(1, -3.0, 0.5), gaussian=(1, 1e-3)), dict(gaussian=(1, 1e300))]
    rows = np.concatenate([I.make_rows(**dict(dict(keys=(17 + j, 4)), **s)) for j, s in enumerate(specs)])
    assert rows[1:6, 9].tolist() == [1, 2, 23, 1, 23]
    items = THREE[np.arange(len(specs)) % 3]
    with np.errstate(over='ignore'):
        want = ds.host_batch(items, 0, len(specs), intensity=rows)
    plain = ds.host_batch(items, 0, len(specs))
    for j in (0, 1, 4):                                                           # nothing to add: the item's own bits (lam 1e-12: no word reaches 2^32 - 1)
        assert torch.equal(want[0][j], plain[0][j])
    assert float((want[0][3] - plain[0][3]).mean()) > 3.0 and bool(want[0][7].abs().eq(1.0).all())
    assert bool(torch.isinf(want[0][9]).any())                                    # float64 noise past the float32 range rounds to infinity on both arms
    for dtype in (torch.float32, torch.bfloat16):
        got = _launch(ds, items, rows, dtype=dtype)
        for g, w in zip(got, want):
            _same_bits(g, w if w.shape[-1] == 1 else w.to(dtype))


@pytest.mark.parametrize('hw', [(16, 16), (12, 18)])
def test_identity_rows_give_the_plain_and_the_augmented_launch_bit_for_bit(hw):
    ds = _set(T.subjects(np.int16), hw, 4, dtype=np.int16, augment=GEO, thickness=T.THICKNESSES)
    items = T.shuffled_items(4)
    geo_rows = ds.epoch_augment(2)
    for dtype in (torch.float32, torch.float16):
        for geo in (None, geo_rows):
            base = _launch(ds, items, None, geo, dtype=dtype)
            got = _launch(ds, items, I.identity_rows(23), geo, dtype=dtype)
            for g, w in zip(got, base):
                _same_bits(g, w)
    ds.load_epoch(items, geo_rows)                                                # a configured set that is given no rows loads identity rows
    assert torch.equal(ds.intensity_table.cpu(), torch.from_numpy(I.identity_rows(23)))
    base = _launch(ds, items, None, geo_rows, first=5, count=5)
    out = (torch.full((5, 4) + hw, 7., device='cuda'), torch.full((5, 1) + hw, 7., device='cuda'), torch.full((5, 1), 7., device='cuda'))
    got = ds.batch(5, 5, out=out)
    assert all(g is o for g, o in zip(got, out))
    for g, w in zip(out, base):
        _same_bits(g, w)
    for g, w in zip(ds.batch(5, 5), base):                                        # and without out=
        _same_bits(g, w)
    # rows past a short epoch are identity rows again, whatever the table held
    ds.load_epoch(items, geo_rows, ds.epoch_intensity(1))
    ds.load_epoch(items[:10], None, ds.epoch_intensity(2, rows=10))
    assert torch.equal(ds.intensity_table[10:].cpu(), torch.from_numpy(I.identity_rows(13))) and bool((ds.items[10:] == -1).all())
    assert not torch.equal(ds.intensity_table[:10].cpu(), torch.from_numpy(I.identity_rows(10)))
    # a row whose flags are 0 is an identity row whatever its parameters say
    quiet = I.make_rows(contrast=(1, 1.3, 0.2), gaussian=(1, 0.5), poisson=(1, 2.0), keys=(5, 6), n=23)
    quiet[:, [0, 3, 5]] = 0.0
    for g, w in zip(_launch(ds, items, quiet), _launch(ds, items, None)):
        _same_bits(g, w)


def test_cursor_moves_through_all_three_tables():
    from afcm_amd.torch_utils.ops.batch_ops import advance_cursor
    ds = _set(T.subjects(np.uint8), (12, 18), 4, augment=GEO, thickness=T.THICKNESSES)
    items, geo_rows, rows = T.shuffled_items(4), ds.epoch_augment(3), ds.epoch_intensity(4)
    want = ds.host_batch(items, 0, 23, augment=geo_rows, intensity=rows)
    ds.load_epoch(items, geo_rows, rows)
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


def test_invalid_rows_are_nan_items_and_their_neighbours_are_untouched():
    ds = _set(T.subjects(np.uint8), (12, 18), 4, augment=GEO, thickness=T.THICKNESSES)
    items = T.shuffled_items(4)[np.arange(30) % 23]
    geo_rows = ds.epoch_augment(6, rows=30)
    # every row at the boundary of validity: J = 24 with T_23 = 2^32, key 2^32 - 1, all three transforms on
    edge = I.make_rows(contrast=(1, 1.2, 0.0), gaussian=(1, 0.5), poisson=(1, 4.0), keys=(2 ** 32 - 1, 2 ** 32 - 1), n=30)
    edge[:, 9], edge[:, 33] = 24, 2.0 ** 32
    want = ds.host_batch(items, 0, 30, augment=geo_rows, intensity=edge)          # the host arm takes the boundary values too
    assert len(R.INVALID) == 23
    at = list(range(1, 24))                                                       # valid rows before and after
    keep = [0] + list(range(24, 30))
    table = edge.copy()
    for row, (col, value) in zip(at, R.INVALID.values()):
        table[row, col] = value
    for k in (4, 1):
        ds.slice_num = k                                                          # the same pool and tables as one-plane items
        for geo in (geo_rows, None):
            clean = _launch(ds, items, edge, geo)
            assert not any(bool(torch.isnan(c).any()) for c in clean)
            if k == 4 and geo is not None:
                for c, w in zip(clean, want):
                    _same_bits(c, w)
            got = _launch(ds, items, table, geo)
            for g, c in zip(got, clean):
                nan_items = torch.isnan(g).reshape(30, -1).cpu()
                assert bool(nan_items[at].all()), [name for name, row in zip(R.INVALID, at) if not bool(nan_items[row].all())]
                assert not bool(nan_items[keep].any())
                _same_bits(g.cpu()[keep], c.cpu()[keep])
    ds.slice_num = 4
    # an invalid row with no flag set is a NaN item all the same; an invalid augment or item row beside a valid intensity row likewise
    off = I.identity_rows(30)
    off[2, 7], off[4, 9] = -1.0, np.nan
    nan_items = torch.isnan(_launch(ds, items, off)[0]).reshape(30, -1).cpu()
    assert bool(nan_items[[2, 4]].all()) and int(nan_items.any(dim=1).sum()) == 2
    bad_geo, bad_items = geo_rows.copy(), items.copy()
    bad_geo[3, 4], bad_items[5, 0] = 2.0, 99
    got = _launch(ds, bad_items, edge, bad_geo)
    for g, w in zip(got, want):
        nan_items = torch.isnan(g).reshape(30, -1).cpu()
        assert bool(nan_items[[3, 5]].all()) and int(nan_items.any(dim=1).sum()) == 2
        rest = sorted(set(range(30)) - {3, 5})
        _same_bits(g.cpu()[rest], w[rest])


def test_host_checks_raise_before_any_launch():
    from afcm_amd import _lib
    from afcm_amd.torch_utils.ops.batch_ops import assemble_batch
    ds = _set(T.subjects(np.uint8), (16, 16), 4, augment=GEO, thickness=T.THICKNESSES)
    items = torch.from_numpy(T.shuffled_items(4)).cuda()
    rows, geo_rows = torch.from_numpy(I.identity_rows(23)).cuda(), torch.from_numpy(A.identity_rows(23)).cuda()
    out = (torch.full((2, 4, 16, 16), 7., device='cuda'), torch.full((2, 1, 16, 16), 7., device='cuda'), torch.full((2, 1), 7., device='cuda'))
    for bad, message in [(rows.float(), 'intensity table must be a contiguous torch.float64'), (rows[:, :35], 'intensity table must be a contiguous torch.float64'),
                         (rows.t().contiguous().t(), 'intensity table must be a contiguous'), (rows.reshape(-1), 'intensity table must be a contiguous'),
                         (rows.cpu().numpy(), 'intensity table must be a contiguous'), (rows[:22], 'has 22 rows, the item table 23'),
                         (torch.cat([rows, rows]), 'has 46 rows, the item table 23'), (rows.cpu(), 'no CPU')]:
        with pytest.raises(RuntimeError, match=message):
            assemble_batch(ds.pool, ds.vols, items, 0, 2, (16, 16), out=out, augment=geo_rows, intensity=bad)
    with pytest.raises(RuntimeError, match='independent_planes must be a bool'):
        assemble_batch(ds.pool, ds.vols, items, 0, 2, (16, 16), out=out, intensity=rows, independent_planes=2)
    with pytest.raises(RuntimeError, match=r'float64 \[23, 36\]'):
        ds.load_epoch(T.shuffled_items(4), None, I.identity_rows(22))
    with pytest.raises(RuntimeError, match=r'float64 \[10, 36\]'):
        ds.load_epoch(T.shuffled_items(4)[:10], None, I.identity_rows(23))
    plain = _set(T.subjects(np.uint8), (16, 16), 4, intensity=None, thickness=T.THICKNESSES)
    assert plain.intensity_table is None and plain.augment_table is None
    with pytest.raises(RuntimeError, match='built without intensity'):
        plain.load_epoch(T.shuffled_items(4), None, I.identity_rows(23))

    lib = _lib.load()
    args = dict(a=out[0].data_ptr(), b=out[1].data_ptr(), slice_idx=out[2].data_ptr(), pool=ds.pool.data_ptr(), pool_elems=ds.pool.numel(),
                src_dtype=_lib.SRC_U8, vols=ds.vols.data_ptr(), n_vols=6, items=items.data_ptr(), n_items=23, augment=geo_rows.data_ptr(),
                intensity=rows.data_ptr(), independent_planes=0, cursor=None, first=0, count=2, k=4, h=16, w=16, out_dtype=_lib.F32, min_value=0.,
                max_value=255., stream=_lib.stream_ptr(ds.pool))
    for edit, message in [(dict(intensity=None), 'null intensity table'), (dict(independent_planes=2), 'independent_planes 2 is not 0 or 1'),
                          (dict(independent_planes=-1), 'independent_planes -1'), (dict(items=None), 'null output'), (dict(k=2), 'slice number 2 is not 1 or 4'),
                          (dict(src_dtype=4), 'source dtype 4'), (dict(out_dtype=3), 'output dtype 3'), (dict(count=0), 'every extent must be positive'),
                          (dict(first=-1), 'first row -1'), (dict(max_value=0.), 'is not above min_value'),
                          (dict(h=1 << 27, w=(1 << 27) + 1), 'h + w above 2^28')]:
        rc = lib.afcm_batch_assemble_noise(*dict(args, **edit).values())
        assert rc == _lib.E_INVALID and message in lib.afcm_last_error().decode(), (edit, rc, lib.afcm_last_error())
    torch.cuda.synchronize()
    assert all(bool((t == 7.).all()) for t in out)                                # nothing was launched
    assert lib.afcm_batch_assemble_noise(*args.values()) == 0                     # the unedited call is a good one,
    assert lib.afcm_batch_assemble_noise(*dict(args, augment=None, independent_planes=1).values()) == 0      # and so is one without an augment table
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out[0]).any()) and float(out[0].abs().max()) <= 1.


# ---- the training loops on the tiny 128^2 generator of test_gpu_train_batch.py ---------------------------------------------------------------

def _tiny_noisy_set(augment=None):
    from afcm_amd.training import DeviceSliceSet
    from test_gpu_train_batch import _tiny_set
    plain, items = _tiny_set()
    ds = DeviceSliceSet(plain.volumes, patch_shape=(1, 128, 128), raw_internal_path_in=['t1'], raw_internal_path_out=['t2'], thickness=[5], device='cuda',
                        augment=augment, intensity=OFTEN)
    assert np.array_equal(ds.epoch_items(11), items)                              # the item draw does not know about the augmentation
    return ds, items, ds.epoch_intensity(21)


def test_train_epoch_device_and_host_arms_leave_the_same_bits():
    from afcm_amd.training import train_epoch
    from test_gpu_train_batch import _state, _tiny_step
    ds, items, rows = _tiny_noisy_set()
    assert rows[:12, [0, 3, 5]].sum(0).min() >= 2
    finals = {}
    for arm, intensity in (('device', rows), ('host', rows), ('plain', None)):
        step = _tiny_step(ema=True)
        torch.manual_seed(3)                                                      # set_input draws gen_z: the same draws for every arm
        total = train_epoch(step, ds, 4, items[:12], total_iters=100, ema_kimgs=10.0, ramp=0.05, where='host' if arm == 'host' else 'device',
                            intensity=None if intensity is None else intensity[:12])
        assert total == 112
        finals[arm] = _state(step)
        assert all(bool(torch.isfinite(t).all()) for t in finals[arm])
    assert all(torch.equal(a, b) for a, b in zip(finals['device'], finals['host']))
    assert any(not torch.equal(a, b) for a, b in zip(finals['device'], finals['plain']))       # the noise did reach the step


def test_training_graph_replays_equal_eager_steps():
    """As tests/test_gpu_augment.py's test of the same name (bfloat16 compute, three warm-up steps and three replays against six eager steps), with
    the noise launch -- and an augment table beside the intensity table -- inside the graph."""
    from afcm_amd.training import TrainingGraph, train_epoch
    from test_gpu_train_batch import _tiny_step
    ds, items, rows = _tiny_noisy_set(augment=GEO_SQUARE)
    items, rows, geo_rows = items[:12], rows[:12], ds.epoch_augment(22, rows=12)
    z = torch.randn(4, 32, generator=torch.Generator().manual_seed(9)).cuda()
    eager = _tiny_step(compute_dtype=torch.bfloat16, capturable=True)
    for _ in range(2):
        train_epoch(eager, ds, 4, items, gen_z=z, augment=geo_rows, intensity=rows)
    want = [p.detach().clone() for p in eager.netG.parameters()]

    step = _tiny_step(compute_dtype=torch.bfloat16, capturable=True)
    ds.load_epoch(items, geo_rows, rows)
    graph = TrainingGraph(step, ds, 4, warmup=3, fixed_z=True, gen_z=z)
    assert int(ds.cursor.cpu()) == 0 and ds.position == 0
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(ds.cursor.cpu()) == 12 and step.optimizer_G.device_step() == 6
    for a, b in zip(step.netG.parameters(), want):
        assert torch.equal(a.detach(), b)
    fresh = ds.host_batch(items, 8, 4, augment=geo_rows, intensity=rows)          # the last replay's batch: rows 8 ... 11 of all three tables
    assert torch.equal(graph.real_A, fresh[0]) and torch.equal(graph.real_B, fresh[1]) and torch.equal(graph.slice_idx, fresh[2])
    other = ds.epoch_intensity(23, rows=12)                                       # refreshed in place: the graph reads the new rows
    graph.load_epoch(items, geo_rows, other)
    graph.replay()
    torch.cuda.synchronize()
    fresh = ds.host_batch(items, 0, 4, augment=geo_rows, intensity=other)
    assert int(ds.cursor.cpu()) == 4 and torch.equal(graph.real_A, fresh[0]) and torch.equal(graph.real_B, fresh[1])


def test_train_epochs_with_and_without_the_graph():
    """The outer loop on the bfloat16 generator step with a schedule and an EMA copy: two epochs of 18 rows in batches of 2, each with its own draw
    of items, parameter rows and intensity rows, in that order on one generator."""
    from afcm_amd.schedule import LRSchedule
    from afcm_amd.training import train_epochs
    from test_gpu_schedule import _schedule
    from test_gpu_train_batch import _state, _tiny_step
    ds, _, _ = _tiny_noisy_set(augment=GEO_SQUARE)
    z = torch.randn(2, 32, generator=torch.Generator().manual_seed(10)).cuda()
    lrs = LRSchedule('linear', 0.0002, epoch_count=1, n_epochs=2, n_epochs_decay=2)
    rng = np.random.default_rng(5)
    for _ in range(2):
        last_items, last_geo, last_rows = ds.epoch_items(rng), ds.epoch_augment(rng), ds.epoch_intensity(rng)
    finals = {}
    for graph in (True, False):
        step = _tiny_step(compute_dtype=torch.bfloat16, capturable=True, ema=True, schedule=_schedule(ema_kimgs=10.0, ramp=0.05))
        before = _state(step)
        assert train_epochs(step, ds, 2, range(1, 3), lrs, 5, graph=graph, gen_z=z) == 18
        assert torch.equal(ds.items.cpu(), torch.from_numpy(last_items)) and torch.equal(ds.augment_table.cpu(), torch.from_numpy(last_geo))
        assert torch.equal(ds.intensity_table.cpu(), torch.from_numpy(last_rows))
        assert step.schedule.read()['total_iters'] == 36.0 and step.optimizer_G.device_step() == 18
        finals[graph] = _state(step)
        assert any(not torch.equal(p, q) for p, q in zip(finals[graph], before))
    assert len(finals[True]) == len(finals[False]) and all(torch.equal(p, q) for p, q in zip(finals[True], finals[False]))
    assert all(bool(torch.isfinite(p).all()) for p in finals[True])
