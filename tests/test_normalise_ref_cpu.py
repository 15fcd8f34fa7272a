"""The per-plane normalisers without a GPU: the slow restatement (tests/normalise_ref.py) and the package's host arm
(``afcm_amd.normalise.normalise_host``) against the reference's own expressions and against the N1 golden captured from its two classes
(tools/gen_golden_normalise.py); the stated summation order against ``math.fsum``; the host-side logic of the ``normalise=`` keyword."""
import math

import numpy as np
import pytest
import torch

import normalise_ref as N
from conftest import load_golden
from afcm_amd.normalise import NormaliseConfig, normalise_host, ordered_sum, plane_record

SHAPES = ((5, 7), (16, 16), (33, 47))
U = 2.0 ** -53


@pytest.fixture(scope='module')
def n1():
    return load_golden('N1_normalise')


def _planes(n1, dtypes):
    for dtype in dtypes:
        for h, w in SHAPES:
            name = f'{np.dtype(dtype).name}_{h}x{w}'
            yield name, n1[f'{name}_x']


def test_percentile_mode_equals_the_reference_for_exact_sources(n1):
    """uint8 / int16 / float64 planes: numpy evaluates the reference's expression in float64, and so does the statement -- equal arrays."""
    pairs = [tuple(p) for p in n1['percentiles']]
    assert pairs == [(1.0, 99.6), (0.0, 100.0)]
    for name, x in _planes(n1, (np.uint8, np.int16, np.float64)):
        for j, pair in enumerate(pairs):
            config = NormaliseConfig(percentile=pair)
            out, rec = normalise_host(x, config)
            assert out.dtype == np.float64 and out.shape == x.shape
            assert np.array_equal(rec[2:], n1[f'{name}_p{j}_bounds']), name                   # np.percentile's own two values
            assert np.array_equal(out, n1[f'{name}_p{j}']), name                              # the class's output
            lo, hi = np.percentile(x, pair[0]), np.percentile(x, pair[1])                     # and the expression, evaluated here
            assert np.array_equal(out, (x - lo) / (hi - lo + 1e-10))
            assert N.same_bits(rec, N.record(x, percentile_pair=pair)), name                  # the slow restatement: the same record
            assert np.array_equal(N.apply(x, rec), out.astype(np.float32))


def test_percentile_mode_on_float32_sources_is_measured(n1):
    """numpy keeps a float32 plane in float32: its percentiles are rounded to float32 and so is every operation after them; the statement works
    in float64 and rounds once.  The share of pixels that differ after the float32 rounding and the largest difference in units of the last
    place are printed (DESIGN 8u records them).  What is asserted is what float32 arithmetic allows.  numpy's float32 lerp holds the virtual
    index q (n - 1) in float32, so its fractional part is off by up to n 2^-24 and the bound by that times the gap d <= 2 M between the two
    order statistics (M = max|m|), plus four roundings of values below 2 M: E = (2 n + 8) M 2^-24 on either bound.  A pixel then differs by at
    most E (1 + 2 |out|) / (hi - lo) from the bounds and 4 |out| 2^-24 from the expression's own float32 roundings."""
    pairs = [tuple(p) for p in n1['percentiles']]
    for name, x in _planes(n1, (np.float32,)):
        for j, pair in enumerate(pairs):
            out, rec = normalise_host(x, NormaliseConfig(percentile=pair))
            want = n1[f'{name}_p{j}']
            assert want.dtype == np.float32
            got = out.astype(np.float32)
            differ = got != want
            units = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
            print(f'{name} p{pair}: {int(differ.sum())} of {differ.size} pixels differ ({100.0 * differ.mean():.2f} %), at most {int(units.max())} units')
            bounds = n1[f'{name}_p{j}_bounds']
            e = (2.0 * x.size + 8.0) * float(np.abs(x).max()) * 2.0 ** -24
            assert np.all(np.abs(bounds - rec[2:]) <= e), name
            allowed = e * (1.0 + 2.0 * np.abs(out)) / float(rec[3] - rec[2]) + 4.0 * np.abs(out) * 2.0 ** -24
            assert np.all(np.abs(want.astype(np.float64) - out) <= allowed), name


def test_ordered_sum_is_the_stated_order():
    rng = np.random.default_rng(0)
    for n in (1, 35, 255, 256, 257, 513, 1025, 1551, 4096):                                  # 256 r + 1: one partial a term longer than the rest
        x = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
        assert ordered_sum(x) == N.ordered_sum(x), n
        assert abs(ordered_sum(x) - math.fsum(x)) <= (n / 256 + 9) * U * math.fsum(np.abs(x)), n
    assert ordered_sum(np.array([-0.0, -0.0])) == 0.0 and not np.signbit(ordered_sum(np.array([-0.0, -0.0])))


def test_standardize_mode_against_the_reference_expressions(n1):
    for name, x in _planes(n1, N.DTYPES):
        n = x.size
        out, rec = normalise_host(x, NormaliseConfig(standardize=True))
        assert N.same_bits(rec, N.record(x, standardize=True)), name
        moments = n1[f'{name}_s_moments'].astype(np.float64)
        v = x.astype(np.float64).reshape(-1)
        if x.dtype.kind in 'iu':
            assert rec[2] == moments[0] == np.mean(x), name                                  # an integer sum is exact in any order
        if x.dtype != np.float32:                                                             # numpy's float32 moments are float32: not the statement
            assert abs(rec[3] - moments[1]) <= N.std_bound(n) * moments[1], name
        # math.fsum: the exactly rounded sum; its mean is one rounding off, every squared deviation three
        mean = math.fsum(v) / n
        std = math.sqrt(math.fsum((t - mean) ** 2 for t in v) / n)
        assert abs(rec[2] - mean) <= (n / 256 + 10) * U * math.fsum(np.abs(v)) / n, name
        assert abs(rec[3] - std) <= N.std_bound(n) * std, name
        assert rec[1] == rec[3] and rec[0] == rec[2]
        if x.dtype != np.float32:
            want = n1[f'{name}_s'].astype(np.float64)
            slack = (N.std_bound(n) + 2 * U) * np.abs(want) + abs(rec[2] - moments[0]) / moments[1] * (1 + 4 * U)
            assert np.all(np.abs(out - want) <= slack), name
        # two given floats: no statistic is taken, and the expression is numpy's own for the exact sources
        fixed = tuple(n1['fixed'])
        out, rec = normalise_host(x, NormaliseConfig(standardize=fixed))
        assert N.same_bits(rec, np.array([fixed[0], fixed[1], fixed[0], fixed[1]]))
        if x.dtype != np.float32:
            assert np.array_equal(out, n1[f'{name}_f']), name


def test_special_planes():
    eps = 1e-10
    flat = np.full((5, 7), 37, dtype=np.int16)
    assert N.same_bits(plane_record(flat, NormaliseConfig(percentile=(1, 99.6))), [37.0, eps, 37.0, 37.0])
    assert N.same_bits(plane_record(flat, NormaliseConfig(standardize=True)), [37.0, eps, 37.0, 0.0])
    assert N.same_bits(plane_record(flat, NormaliseConfig(standardize=True, eps=-1.0)), [37.0, 0.0, 37.0, 0.0])          # div = max(0, eps)
    zeros = np.zeros((1, 5, 7))
    assert N.same_bits(plane_record(zeros, NormaliseConfig(percentile=(0, 100))), [0.0, eps, 0.0, 0.0])
    assert N.same_bits(plane_record(zeros, NormaliseConfig(standardize=(3.0, 1e-12))), [3.0, eps, 3.0, 1e-12])           # a std below eps
    holed = np.arange(35, dtype=np.float32).reshape(5, 7)
    holed[2, 3] = np.nan
    for config in (NormaliseConfig(percentile=(1, 99.6)), NormaliseConfig(standardize=True)):
        out, rec = normalise_host(holed, config)
        assert np.isnan(rec).all() and np.isnan(out).all()
    out, rec = normalise_host(flat, NormaliseConfig(percentile=(0, 100), then_normalize=True), 0.0, 1.0)
    assert np.array_equal(out, np.full((5, 7), -1.0))                                         # (37 - 37) / eps = 0 -> Normalize(0, 1) -> -1
    for dtype in N.DTYPES:                                                                    # the shared select cases: host arm = slow restatement
        for name, (plane, pairs) in N.select_cases(dtype).items():
            for pair in pairs:
                assert N.same_bits(plane_record(plane, NormaliseConfig(percentile=pair)), N.record(plane, percentile_pair=pair)), (dtype, name, pair)


def test_config_refusals():
    for kw in (dict(), dict(percentile=(1, 99), standardize=True), dict(percentile=(1, 99), standardize=(0.0, 1.0))):
        with pytest.raises(RuntimeError, match='exactly one'):
            NormaliseConfig(**kw)
    for bad in ((99, 1), (-1, 50), (0, 101), (float('nan'), 50), 5):
        with pytest.raises(RuntimeError, match='percentile'):
            NormaliseConfig(percentile=bad)
    with pytest.raises(RuntimeError, match='pair'):
        NormaliseConfig(standardize=(1.0,))
    with pytest.raises(RuntimeError, match='then_normalize'):
        NormaliseConfig(standardize=True, then_normalize=1)
    with pytest.raises(RuntimeError, match='NaN'):
        NormaliseConfig(standardize=True, eps=float('nan'))
    with pytest.raises(RuntimeError, match='uint8 / int16 / float32 / float64'):
        normalise_host(np.zeros((2, 2), dtype=np.int32), NormaliseConfig(standardize=True))
    with pytest.raises(RuntimeError, match='NormaliseConfig or None'):
        normalise_host(np.zeros((2, 2)), dict(percentile=(0, 100)))


def _subjects():
    from volume_ref import source
    return [{m: source(shape, np.int16, seed=60 + 2 * s + j) for j, m in enumerate(('t1', 't2'))} for s, shape in enumerate(((7, 13, 20), (6, 20, 13)))]


def test_unsupported_combinations_are_refused_with_a_reason():
    from afcm_amd import augment_blur, augment_elastic, augment_intensity
    from afcm_amd.torch_utils.ops.batch_ops import assemble_batch
    from afcm_amd.training import DeviceSliceSet
    config = NormaliseConfig(percentile=(1, 99.6))
    stages = dict(intensity=augment_intensity.IntensityConfig(gaussian=(0.0, 0.1, 1.0)), elastic=augment_elastic.ElasticConfig(),
                  blur=augment_blur.BlurConfig())
    kw = dict(patch_shape=(1, 16, 16), raw_internal_path_in=['t1'], raw_internal_path_out=['t2'], thickness=[2], device=None)
    for name, stage in stages.items():
        with pytest.raises(RuntimeError, match=f'normalise= together with {name}=.*float32 scratch planes'):
            DeviceSliceSet(_subjects(), normalise=config, **{name: stage}, **kw)
    with pytest.raises(RuntimeError, match='NormaliseConfig or None'):
        DeviceSliceSet(_subjects(), normalise=(1, 99.6), **kw)
    ds = DeviceSliceSet(_subjects(), normalise=config, **kw)
    items = ds.epoch_items(0)
    with pytest.raises(RuntimeError, match='normalise= together with blur='):
        ds.host_batch(items, 0, 2, normalise=config, blur=np.zeros((len(items), 100)))
    pool, vols, table = torch.zeros(64, dtype=torch.uint8), torch.tensor([[0, 1, 8, 8]]), torch.zeros((1, 4), dtype=torch.int32)
    with pytest.raises(RuntimeError, match='normalise= together with intensity='):
        assemble_batch(pool, vols, table, 0, 1, (8, 8), normalise=config, intensity=torch.zeros((1, 36), dtype=torch.float64))
    with pytest.raises(RuntimeError, match='norm_coef= only with normalise='):
        assemble_batch(pool, vols, table, 0, 1, (8, 8), norm_coef=torch.zeros((1, 5, 4), dtype=torch.float64))
    with pytest.raises(RuntimeError, match='no CPU'):                                         # past the refusals: only the device is missing
        assemble_batch(pool, vols, table, 0, 1, (8, 8), normalise=config)


@pytest.mark.parametrize('k', [4, 1])
def test_slice_dataset_items_equal_the_restatement_on_stacked_planes(k):
    from afcm_amd.data import SliceDataset
    from afcm_amd.training import DeviceSliceSet
    volumes = _subjects()[0]
    h, w = 16, 16                                                                             # 13 x 20: padded in y, cropped in x
    for config, kind in ((NormaliseConfig(percentile=(1, 99.6)), dict(percentile_pair=(1, 99.6))),
                         (NormaliseConfig(standardize=True, then_normalize=True), dict(standardize=True))):
        then = (-100.0, 900.0) if config.then_normalize else None
        ds = SliceDataset(volumes, phase='test', patch_shape=(1, h, w), stride_shape=(1, 1, 1), raw_internal_path_in=['t1'], raw_internal_path_out=['t2'],
                          thickness=[2] if k == 4 else [], slice_num=k, min_value=-100.0, max_value=900.0, normalise=config)
        plain = SliceDataset(volumes, phase='test', patch_shape=(1, h, w), stride_shape=(1, 1, 1), raw_internal_path_in=['t1'],
                             raw_internal_path_out=['t2'], thickness=[2] if k == 4 else [], slice_num=k, min_value=-100.0, max_value=900.0)
        assert len(ds) == 7
        for idx in range(7):
            a, label, where = ds[idx]
            planes = [N.item_plane(volumes['t1'], pos, h, w) for pos in N.positions(idx, 2, k)]
            want = np.stack([N.apply(p, N.record(p, **kind), then) for p in planes])
            assert a.dtype == torch.float32 and np.array_equal(a.numpy(), want), (idx, k)
            assert torch.equal(label, plain[idx][1]) and where == plain[idx][2]
            assert not torch.equal(a, plain[idx][0])
    # the training arm: host_batch hands the configuration on to its datasets, target plane included
    sets = DeviceSliceSet(_subjects(), patch_shape=(1, h, w), raw_internal_path_in=['t1'], raw_internal_path_out=['t2'], thickness=[2] if k == 4 else [],
                          slice_num=k, min_value=-100.0, max_value=900.0, device=None, normalise=config)
    items = sets.epoch_items(3)
    a, b, c = sets.host_batch(items, 0, 4, normalise=config)
    for j, (va, vb, idx, t) in enumerate(items[:4].tolist()):
        subject = _subjects()[vb // 2]
        target = N.item_plane(subject['t2'], idx, h, w)
        assert np.array_equal(b[j, 0].numpy(), N.apply(target, N.record(target, **kind), then))
        first = N.item_plane(subject['t1'], N.positions(idx, 2, k)[0], h, w)
        assert np.array_equal(a[j, 0].numpy(), N.apply(first, N.record(first, **kind), then))
    assert not torch.equal(a, sets.host_batch(items, 0, 4)[0])


def test_library_exports_the_plan():
    from afcm_amd.torch_utils.ops.normalise_ops import norm_plan
    passes = {torch.uint8: 1, torch.int16: 2, torch.float32: 4, torch.float64: 8}
    for dtype, want in passes.items():
        assert norm_plan(dtype, NormaliseConfig(percentile=(0, 100))) == {'threads': 256, 'passes': want, 'digit_bits': 8, 'ranks': 4}
        assert norm_plan(dtype, NormaliseConfig(standardize=True))['passes'] == 2
        assert norm_plan(dtype, NormaliseConfig(standardize=(0.0, 1.0)))['passes'] == 0
