"""Intensity augmentation without a GPU: the numpy host arm (afcm_amd/augment_intensity.py) against the generator's known answers and an
independent pure-Python Philox, against ``math`` Box-Muller and the normal and Poisson distributions, against the golden captured from the
reference's RandomContrast / AdditiveGaussianNoise / AdditivePoissonNoise classes (tests/golden/A2_augment_intensity.npz,
tools/gen_golden_augment_intensity.py); ``intensity_rows``, ``IntensityConfig``, the host side of ``DeviceSliceSet(intensity=...)``, the binding
table and the built kernels' resources.  tests/test_gpu_augment_intensity.py holds the kernel to ``host_batch(..., intensity=...)``."""
import numpy as np
import pytest
import torch
from scipy import special, stats

import augment_intensity_ref as R
import train_batch_ref as T
from afcm_amd import augment_intensity as I
from conftest import load_golden

KEYS = ((0x12345678, 0x9abcdef0), (7, 11))                  # fixed keys of the distribution tests (chosen once; both pass the bounds below)
SIDE = 512                                                  # 2^18 pixels


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ---- the generator -----------------------------------------------------------------------------------------------------------------------------

def test_philox_known_answers_and_the_scalar_restatement():
    for counter, key, want in R.KNOWN_ANSWERS:
        assert R.philox4x32(counter, key) == want
        assert tuple(int(v) for v in I.philox4x32(counter, key)) == want
    rng = np.random.default_rng(0)
    counters, keys = rng.integers(0, 2 ** 32, (200, 4)), rng.integers(0, 2 ** 32, (200, 2))
    got = I.philox4x32(counters, keys)
    assert got.dtype == np.uint32 and got.shape == (200, 4)
    for c, k, g in zip(counters.tolist(), keys.tolist(), got.tolist()):
        assert R.philox4x32(c, k) == tuple(g)
    # one key against many counters (the field's use), and the field's counter layout: lane x & 3 of counter (x >> 2, y, stream | plane << 1, 0)
    assert np.array_equal(I.philox4x32(counters, keys[0]), np.array([R.philox4x32(c, keys[0].tolist()) for c in counters.tolist()], dtype=np.uint32))
    for stream, plane in ((0, 0), (1, 0), (0, 3), (1, 4)):
        words = I.field_words(5, 6, 3, 18, stream, plane)
        assert words.shape == (3, 18)
        assert all(int(words[y, x]) == R.pixel_word((5, 6), y, x, stream, plane) for y in range(3) for x in range(18))


# ---- normals -----------------------------------------------------------------------------------------------------------------------------------

def test_series_accuracy_against_the_library():
    """Reported, with loose bars: what the tests hold is that the two arms agree bit for bit."""
    x = np.exp(np.random.default_rng(0).uniform(np.log(2.0 ** -33), 0.0, 1 << 18))
    err = np.abs(I.log_series(x) - np.log(x))
    u = np.random.default_rng(1).uniform(0.0, 1.0, 1 << 18)
    s, c = I.sincos_turns(u)
    es, ec = np.abs(s - np.sin(2 * np.pi * u)).max(), np.abs(c - np.cos(2 * np.pi * u)).max()
    print(f'log_series: max abs {err.max():.2e}, max rel {(err / np.abs(np.log(x))).max():.2e}; sin {es:.2e}, cos {ec:.2e}')
    assert err.max() < 8e-15 and es < 4e-15 and ec < 4e-15
    # the ends of u1 = (w + 0.5) 2^-32 and the quadrant boundaries of u2 = w 2^-32
    ends = (np.array([0.0, 1.0, 2.0 ** 32 - 1]) + 0.5) * 2.0 ** -32
    assert np.all(I.log_series(ends) < 0) and np.abs(I.log_series(ends) - np.log(ends)).max() < 8e-15
    quarter = np.array([0.0, 0.25, 0.5, 0.75])
    s, c = I.sincos_turns(quarter)
    assert np.array_equal(s, [0.0, 1.0, -0.0, -1.0]) and np.array_equal(c, [1.0, -0.0, -1.0, 0.0])
    below = np.nextafter(quarter[1:], 0)
    s, c = I.sincos_turns(below)
    assert np.abs(s - np.sin(2 * np.pi * below)).max() < 4e-15 and np.abs(c - np.cos(2 * np.pi * below)).max() < 4e-15


def test_normals_equal_math_box_muller_on_the_same_words():
    z = I.normal_field(*KEYS[0], 9, 18)
    want = np.array([[R.normal_math(KEYS[0], y, x) for x in range(18)] for y in range(9)])
    assert np.abs(z - want).max() < 1e-13
    z3 = I.normal_field(*KEYS[0], 9, 18, plane=3)
    assert np.abs(z3 - np.array([[R.normal_math(KEYS[0], y, x, plane=3) for x in range(18)] for y in range(9)])).max() < 1e-13
    assert not np.array_equal(z, z3)
    assert np.array_equal(I.normal_field(*KEYS[0], 9, 17), z[:, :17])              # a width that is no multiple of 4: the same field, cut


@pytest.mark.parametrize('key', KEYS)
def test_normal_field_distribution(key):
    z = I.normal_field(*key, SIDE, SIDE).reshape(-1)
    n = z.size
    assert n == 1 << 18 and np.isfinite(z).all()
    assert abs(z.mean()) < 4 / np.sqrt(n) and abs(z.std() - 1.0) < 4 / np.sqrt(2 * n)
    z = np.sort(z)
    cdf = special.ndtr(z)
    ks = max((np.arange(1, n + 1) / n - cdf).max(), (cdf - np.arange(n) / n).max())
    assert ks < 1.95 / np.sqrt(n), ks


# ---- Poisson -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('lam', [0.01, 0.5, 1.0, 4.0])
def test_poisson_table_and_field(lam):
    cuts = I.poisson_table(lam)
    assert 1 <= len(cuts) <= 23 and np.array_equal(cuts, np.floor(cuts)) and np.all(np.diff(cuts) >= 0)
    assert cuts[-1] >= 2.0 ** 32 - 1 and np.all(cuts[:-1] < 2.0 ** 32 - 1) and cuts.max() <= 2.0 ** 32
    cdf = stats.poisson.cdf(np.arange(len(cuts)), lam)
    assert np.abs(cuts - cdf * 2.0 ** 32).max() <= 2.0
    counts = I.poisson_field(*KEYS[0], SIDE, SIDE, cuts)
    n = counts.size
    assert abs(counts.mean() - lam) < 4 * np.sqrt(lam / n)
    words = I.field_words(*KEYS[0], 4, 18, 1)
    got = I.poisson_field(*KEYS[0], 4, 18, cuts)
    assert all(got[y, x] == R.count(int(words[y, x]), cuts.tolist()) for y in range(4) for x in range(18))


def test_poisson_table_edges():
    assert np.array_equal(I.poisson_table(0.0), [2.0 ** 32])                      # never a count
    assert len(I.poisson_table(1e-12)) == 1 and I.poisson_table(1e-12)[0] == 2.0 ** 32 - 1
    assert len(I.poisson_table(1e-6)) == 2
    assert len(I.poisson_table(4.0)) == 23
    assert R.count(0xFFFFFFFF, [2.0 ** 32]) == 0 and R.count(0xFFFFFFFF, [2.0 ** 32 - 1]) == 1
    for bad in (-0.1, 4.5, float('nan'), float('inf')):
        with pytest.raises(RuntimeError, match='lam must be in'):
            I.poisson_table(bad)


# ---- the golden: the reference's classes -----------------------------------------------------------------------------------------------------

def test_restatement_equals_the_reference_classes():
    g = load_golden('A2_augment_intensity')
    x, cases, zs, counts, want, prob = g['x'], g['cases'], g['z'], g['counts'], g['out'], float(g['prob'])
    assert x.dtype == np.float64 and np.array_equal(x, x.astype(np.float32).astype(np.float64)) and x.shape == (2, 12, 18)
    executed = set()
    for case, z, k, w in zip(cases, zs, counts, want):
        dc, dg, dp, alpha, mean, std, lam, which = case.tolist()
        ran = (dc < prob, dg < prob, dp < prob)                                    # the reference executes when uniform() < probability
        executed.add(ran)
        p = x[int(which)]
        got = I.transform(p, contrast=(alpha, mean) if ran[0] else None, gaussian=(std, z) if ran[1] else None, poisson=k if ran[2] else None)
        assert got.dtype == np.float64 and np.array_equal(got, w), case
        scalar = [[R.transform_pixel(p[y, xx], (alpha, mean) if ran[0] else None, (std, z[y, xx]) if ran[1] else None, int(k[y, xx]) if ran[2] else None)
                   for xx in range(18)] for y in range(12)]
        assert np.array_equal(np.array(scalar), w), case
        if not any(ran):
            assert np.array_equal(w, p)
    assert len(executed) == 8                                                      # every combination of executed / not
    # draws equal to, below and above the probability
    assert (cases[8, :3] == prob).all() and np.array_equal(want[8], x[0])          # equal: not executed
    assert cases[9, 0] < prob and cases[9, 0] == np.nextafter(prob, 0) and not np.array_equal(want[9], x[1])
    assert (cases[:8, :3] != prob).all()
    # the contrast clip did act somewhere and the noise did leave [-1, 1]: no clip after it
    assert any((np.abs(w) == 1.0).sum() > (np.abs(x[int(c[7])]) == 1.0).sum() for c, w in zip(cases, want) if c[0] < prob and not c[1] < prob and not c[2] < prob)
    assert np.abs(want).max() > 1.0


# ---- rows ------------------------------------------------------------------------------------------------------------------------------------

def test_intensity_rows_draw_order_and_off_transforms():
    cfg = I.IntensityConfig(contrast=(0.5, 1.5, 0.25, 0.5), gaussian=(0.0, 1.0, 0.5), poisson=(0.0, 1.0, 0.5))
    n = 40
    rows = I.intensity_rows(cfg, n, np.random.default_rng(9))
    ref = np.random.default_rng(9)
    fc, alpha = ref.uniform(size=n) < 0.5, ref.uniform(0.5, 1.5, n)
    fg, std = ref.uniform(size=n) < 0.5, ref.uniform(0.0, 1.0, n)
    fp, lam = ref.uniform(size=n) < 0.5, ref.uniform(0.0, 1.0, n)
    keys = ref.integers(0, 2 ** 32, (n, 2))
    assert rows.shape == (n, 36) and rows.dtype == np.float64 and all(I.row_is_valid(r) for r in rows)
    assert np.array_equal(rows[:, 0], fc) and np.array_equal(rows[:, 3], fg) and np.array_equal(rows[:, 5], fp) and np.array_equal(rows[:, 7:9], keys)
    assert np.array_equal(rows[fc, 1], alpha[fc]) and (rows[fc, 2] == 0.25).all() and (rows[~fc, 1] == 1.0).all() and (rows[~fc, 2] == 0.0).all()
    assert np.array_equal(rows[fg, 4], std[fg]) and (rows[~fg, 4] == 0.0).all()
    assert np.array_equal(rows[fp, 6], lam[fp]) and (rows[~fp, 6] == 0.0).all() and (rows[~fp, 9:] == 0.0).all() and (rows[:, 34:] == 0.0).all()
    for r in np.nonzero(fp)[0]:
        cuts = I.poisson_table(lam[r])
        assert rows[r, 9] == len(cuts) and np.array_equal(rows[r, 10:10 + len(cuts)], cuts) and (rows[r, 10 + len(cuts):] == 0).all()
    assert 5 < fc.sum() < 35 and 5 < fg.sum() < 35 and 5 < fp.sum() < 35
    # a transform that is off draws nothing: the generator is where the remaining draws leave it
    only = I.intensity_rows(I.IntensityConfig(gaussian=(0.25, 0.5, 1.0)), n, np.random.default_rng(9))
    ref = np.random.default_rng(9)
    flags, std = ref.uniform(size=n) < 1.0, ref.uniform(0.25, 0.5, n)
    assert flags.all() and np.array_equal(only[:, 4], std) and np.array_equal(only[:, 7:9], ref.integers(0, 2 ** 32, (n, 2)))
    assert (only[:, 0] == 0).all() and (only[:, 5] == 0).all() and (only[:, 3] == 1).all()
    none = I.intensity_rows(I.IntensityConfig(), 3, np.random.default_rng(9))
    assert np.array_equal(none[:, :7], I.identity_rows(3)[:, :7]) and np.array_equal(none[:, 7:9], np.random.default_rng(9).integers(0, 2 ** 32, (3, 2)))
    never = I.intensity_rows(I.IntensityConfig(poisson=(1.0, 2.0, 0.0)), 5, np.random.default_rng(1))   # probability 0: uniform() < 0 never holds
    assert (never[:, 5] == 0).all() and (never[:, 9] == 0).all()
    assert np.array_equal(I.identity_rows(2), I.make_rows(n=2)) and not I.identity_rows(2)[:, [0, 3, 5]].any()


def test_refusals():
    for kw, message in [(dict(contrast=(0.5, 1.5, 0.0)), 'contrast must be None or 4 values'), (dict(contrast=(1.5, 0.5, 0.0, 0.1)), 'contrast alpha must be a finite range'),
                        (dict(contrast=(0.5, 1.5, float('nan'), 0.1)), 'contrast mean must be finite'), (dict(contrast=(0.5, 1.5, 0.0, 1.5)), 'contrast probability'),
                        (dict(gaussian=(-0.1, 1.0, 0.1)), 'gaussian std must be a finite range'), (dict(gaussian=(0.0, float('inf'), 0.1)), 'gaussian std'),
                        (dict(gaussian=(0.0, 1.0, -0.1)), 'gaussian probability'), (dict(gaussian='abc'), 'gaussian must be None or 3 values'),
                        (dict(poisson=(0.0, 4.5, 0.1)), r'poisson lam must be a finite range lo <= hi inside \[0, 4\]'), (dict(poisson=(-1.0, 1.0, 0.1)), 'poisson lam'),
                        (dict(poisson=(0.0, 1.0, True)), 'poisson probability'), (dict(independent_planes=1), 'independent_planes must be a bool')]:
        with pytest.raises(RuntimeError, match=message):
            I.IntensityConfig(**kw)
    assert I.IntensityConfig(poisson=(0, 4, 1)).poisson == (0.0, 4.0, 1.0)
    cfg = I.IntensityConfig(gaussian=(0.0, 1.0, 0.2))
    with pytest.raises(RuntimeError, match='must be an IntensityConfig'):
        I.intensity_rows(dict(), 3, np.random.default_rng(0))
    with pytest.raises(RuntimeError, match='numpy.random.Generator'):
        I.intensity_rows(cfg, 3, np.random.RandomState(0))
    with pytest.raises(RuntimeError, match='0 rows'):
        I.intensity_rows(cfg, 0, np.random.default_rng(0))
    with pytest.raises(RuntimeError, match=r'float64 \[3, 36\]'):
        I.checked_rows(I.identity_rows(4), 3, 'here')
    with pytest.raises(RuntimeError, match=r'float64 \[3, 36\]'):
        I.checked_rows(I.identity_rows(3).astype(np.float32), 3, 'here')
    planes = np.zeros((2, 4, 6), dtype=np.float32)
    good = I.make_rows(gaussian=(1, 0.5), poisson=(1, 4.0), keys=(2 ** 32 - 1, 0))[0]
    assert I.row_is_valid(good) and good[9] == 23
    edge = good.copy()
    edge[9], edge[33] = 24, 2.0 ** 32                                              # the boundary values are valid
    assert I.row_is_valid(edge)
    for col, value in R.INVALID.values():
        bad = edge.copy()
        bad[col] = value
        assert not I.row_is_valid(bad), (col, value)
        with pytest.raises(RuntimeError, match='not a valid intensity row'):
            I.apply_host(planes, bad)
    with pytest.raises(RuntimeError, match=r'float32 \[C, H, W\]'):
        I.apply_host(planes.astype(np.float64), good)
    with pytest.raises(RuntimeError, match=r'float32 \[C, H, W\]'):
        I.apply_host(planes[0], good)


def test_apply_host_fields_and_independent_planes():
    planes = np.random.default_rng(3).uniform(-1, 1, (5, 12, 18)).astype(np.float32)
    planes[0, 0, 0] = np.nan
    row = I.make_rows(contrast=(1, 1.4, 0.1), gaussian=(1, 0.3), poisson=(1, 0.8), keys=KEYS[0])[0]
    shared, own = I.apply_host(planes, row), I.apply_host(planes, row, independent_planes=True)
    assert shared.dtype == np.float32 and shared.shape == planes.shape and np.isnan(shared[0, 0, 0]) and np.isnan(shared).sum() == 1
    z, k = I.normal_field(*KEYS[0], 12, 18), I.poisson_field(*KEYS[0], 12, 18, I.poisson_table(0.8))
    for c in range(5):                                                             # the statement, written out once more
        t = planes[c].astype(np.float64)
        t = 0.1 + 1.4 * (t - 0.1)
        t = np.where(t < -1, -1.0, np.where(t > 1, 1.0, t))
        t = (t + 0.3 * z) + k
        assert np.array_equal(_bits(shared[c]), _bits(t.astype(np.float32)))
    noise = lambda out: out.astype(np.float64) - np.clip(0.1 + 1.4 * (planes.astype(np.float64) - 0.1), -1, 1)
    ns, no = noise(shared)[:, 1:], noise(own)[:, 1:]
    assert np.abs(ns - ns[0]).max() < 1e-6                                         # one field for every plane (up to the float32 rounding)
    assert np.array_equal(_bits(shared[0]), _bits(own[0])) and all(np.abs(no[c] - no[0]).max() > 0.5 for c in range(1, 5))
    # B of a 4-plane item is plane 4
    assert np.array_equal(_bits(I.apply_host(planes[4:], row, True, first_plane=4)), _bits(own[4:]))
    assert np.array_equal(_bits(I.apply_host(planes[4:], row, False, first_plane=4)), _bits(shared[4:]))
    # no flag: the planes themselves; tensors come back as tensors
    assert I.apply_host(planes, I.identity_rows(1)[0]) is planes
    t = I.apply_host(torch.from_numpy(planes), row)
    assert isinstance(t, torch.Tensor) and np.array_equal(_bits(t.numpy()), _bits(shared))
    # std = 0 and a lam whose counts are all zero leave only the contrast
    still = I.apply_host(planes, I.make_rows(gaussian=(1, 0.0), poisson=(1, 0.0), keys=KEYS[1])[0])
    assert np.array_equal(_bits(still), _bits(planes))


# ---- DeviceSliceSet, host side; the binding; the kernels' resources -----------------------------------------------------------------------------

def _host_set(**kw):
    from afcm_amd.training import DeviceSliceSet
    kw.setdefault('patch_shape', (1, 12, 18))
    return DeviceSliceSet(T.subjects(np.uint8), raw_internal_path_in=['t1'], raw_internal_path_out=['t2'], thickness=T.THICKNESSES, device=None, **kw)


def test_device_slice_set_host_side():
    from afcm_amd.augment import AugmentConfig, augment_rows
    cfg = I.IntensityConfig(contrast=(0.5, 1.5, 0.0, 0.5), gaussian=(0.0, 1.0, 0.5), poisson=(0.0, 1.0, 0.5))
    geo = AugmentConfig(flip_axes=(1, 2), angle_spectrum=45)
    plain, ds, both = _host_set(), _host_set(intensity=cfg), _host_set(intensity=cfg, augment=geo)
    # the draws before it are what they were; the intensity rows come after them on the same generator
    rng, ref = np.random.default_rng(3), np.random.default_rng(3)
    items, geo_rows, rows = both.epoch_items(rng), both.epoch_augment(rng), both.epoch_intensity(rng)
    assert np.array_equal(items, plain.epoch_items(ref)) and np.array_equal(geo_rows, augment_rows(geo, 23, (12, 18), ref))
    assert rows.shape == (23, 36) and np.array_equal(rows, I.intensity_rows(cfg, 23, ref))
    assert np.array_equal(ds.epoch_items(3), items) and ds.epoch_intensity(5, rows=7).shape == (7, 36)
    base = ds.host_batch(items, 5, 4)
    got = ds.host_batch(items, 5, 4, intensity=rows)
    assert rows[5:9, [0, 3, 5]].any()
    for j in range(4):
        assert np.array_equal(_bits(got[0][j].numpy()), _bits(I.apply_host(base[0][j].numpy(), rows[5 + j])))
        assert np.array_equal(_bits(got[1][j].numpy()), _bits(I.apply_host(base[1][j].numpy(), rows[5 + j], False, 4)))
    assert torch.equal(got[2], base[2]) and not torch.equal(got[0], base[0])
    assert all(torch.equal(a, b) for a, b in zip(ds.host_batch(items, 5, 4, intensity=I.identity_rows(23)), base))
    # with both tables: rotate, then noise
    turned = both.host_batch(items, 5, 4, augment=geo_rows)
    full = both.host_batch(items, 5, 4, augment=geo_rows, intensity=rows)
    for j in range(4):
        assert np.array_equal(_bits(full[0][j].numpy()), _bits(I.apply_host(turned[0][j].numpy(), rows[5 + j])))
    own = _host_set(intensity=I.IntensityConfig(gaussian=(0.5, 0.5, 1.0), independent_planes=True))
    a, b, _ = own.host_batch(items, 0, 1, intensity=own.epoch_intensity(1))
    a0, b0, _ = own.host_batch(items, 0, 1)
    assert np.array_equal(_bits(b[0].numpy()), _bits(I.apply_host(b0[0].numpy(), own.epoch_intensity(1)[0], True, 4)))
    assert not np.array_equal(_bits(b[0].numpy()), _bits(I.apply_host(b0[0].numpy(), own.epoch_intensity(1)[0], True, 0)))
    for call, message in [(lambda: ds.host_batch(items, 5, 4, intensity=rows[:22]), r'float64 \[23, 36\]'),
                          (lambda: plain.host_batch(items, 5, 4, intensity=rows), 'built without intensity'),
                          (lambda: plain.epoch_intensity(3), 'built without intensity'),
                          (lambda: _host_set(intensity=cfg, phase='val'), "belongs to the 'train' phase"),
                          (lambda: _host_set(intensity=dict(gaussian=(0, 1, 0.2))), 'must be an IntensityConfig'),
                          (lambda: ds.load_epoch(items, None, rows), 'device=None')]:
        with pytest.raises(RuntimeError, match=message):
            call()


def test_binding_and_host_checks_of_the_launch():
    from afcm_amd import _lib
    from afcm_amd.torch_utils.ops.batch_ops import assemble_batch
    res, args = _lib.SIGNATURES['afcm_batch_assemble_noise']
    aug = _lib.SIGNATURES['afcm_batch_assemble_aug'][1]
    assert len(args) == 23 and args[:11] == aug[:11] and args[11:13] == [_lib._vp, _lib._i32] and args[13:] == aug[11:]
    assert hasattr(_lib.load(), 'afcm_batch_assemble_noise') and _lib.load().afcm_abi_version() == 13
    pool, vols = torch.zeros(64, dtype=torch.uint8), torch.tensor([[0, 1, 8, 8]], dtype=torch.int64)
    items, rows = torch.tensor([[0, 0, 0, 1]] * 3, dtype=torch.int32), torch.from_numpy(I.identity_rows(3))
    for bad, message in [(rows.float(), 'intensity table must be a contiguous torch.float64'), (rows[:, :35], 'intensity table must be a contiguous'),
                         (rows.numpy(), 'intensity table must be a contiguous'), (rows.t().contiguous().t(), 'intensity table must be a contiguous'),
                         (rows[:2], 'has 2 rows, the item table 3'), (rows, 'no CPU')]:
        with pytest.raises(RuntimeError, match=message):
            assemble_batch(pool, vols, items, 0, 2, (4, 4), intensity=bad)
    with pytest.raises(RuntimeError, match='independent_planes must be a bool'):
        assemble_batch(pool, vols, items, 0, 2, (4, 4), intensity=rows, independent_planes=1)
    with pytest.raises(RuntimeError, match='independent_planes without an intensity table'):
        assemble_batch(pool, vols, items, 0, 2, (4, 4), independent_planes=True)


def test_intensity_kernels_use_no_scratch_and_no_lds():
    """Code-object metadata of the built batch.o, as tests/test_augment_ref_cpu.py reads it: every (source, output) instance of the noise kernel,
    without scratch, spills or LDS (DESIGN section 8p quotes the registers), and the two earlier kernels' twelve each beside them."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, 'afcm_amd', 'csrc')
    if not os.path.exists(os.path.join(csrc, 'batch.o')):
        subprocess.check_call(['make', '-C', csrc, 'batch.o'])
    sys.path.insert(0, os.path.join(root, 'tools'))
    from kernel_resources import kernel_resources
    found = kernel_resources(os.path.join(csrc, 'batch.o'))
    kernels = [k for k in found if 'batch_intensity_kernel' in k['name']]
    assert len(kernels) == 4 * 3 and len(found) == 3 * 4 * 3 + 1, [k['name'] for k in found]
    for k in kernels:
        assert k.get('scratch', 0) == 0 and k.get('vgpr_spill', 0) == 0 and k.get('sgpr_spill', 0) == 0 and k.get('lds', 0) == 0, k
        assert k.get('vgpr', 0) <= 128, k                                          # at least four waves per SIMD
