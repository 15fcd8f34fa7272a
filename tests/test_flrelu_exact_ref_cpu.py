"""The exact filtered_lrelu cases (tests/flrelu_exact_ref.py) without a GPU: every quantity a kernel rounds is representable -- a
condition, not a measurement --, the float64 reference is the oracle's, and the cases have teeth: outputs that are not zero, a
reference that moves in every 16 x 16 output block when one tap is dropped, two neighbours are swapped or the padding moves by one,
a clamp that is met exactly, exceeded and not reached, pre-activations that are exactly 0."""
import numpy as np
import pytest
import torch

import flrelu_exact_ref as E
import flrelu_read_ref as R

CASES = E.cases()
IDS = [c['id'] for c in CASES]
GROUPS = sorted({(c['family'], c['kern']) for c in CASES})


def test_filters_are_integer_irregular_and_asymmetric():
    for name, taps in E.FILTERS.items():
        f = np.asarray(taps)
        assert len(f) == len(R.filters()[name]), 'tap counts of the kernels'
        assert set(np.abs(f)) == {1, 2} and (np.abs(f) == 2).sum() <= len(f) // 3, 'taps +-1 with a few +-2, none zero'
        assert (f[1:] != f[:-1]).all(), 'a swap of two neighbours must change the filter'
        assert all((f[s:] != f[:-s]).any() for s in range(1, len(f))), 'no shift maps the filter onto itself'
        assert (f != f[::-1]).any() and (f != -f[::-1]).any(), 'not symmetric: flip_filter must matter'


def test_fits_knows_the_significands():
    q = np.array([0, 1, 255, 256, 257, 258, 2047, 2048, 2049, 4094, 4098, 3 << 20])
    assert E.fits(q, 0, 'bfloat16').tolist() == [True, True, True, True, False, True, False, True, False, False, False, True]
    assert E.fits(q, 0, 'float16').tolist() == [True, True, True, True, True, True, True, True, False, True, False, False]      # 3 * 2^20 > 65504
    assert E.fits(np.array([1, 3]), -14, 'float16').tolist() == [True, True] and not E.fits(np.array([1]), -16, 'float16')[0]      # no subnormals
    # against the conversion itself
    rng = np.random.default_rng(0)
    q = rng.integers(-5000, 5000, size=4000)
    for dtype in ('float16', 'bfloat16'):
        for lg in (0, -8):
            v = q * 2.0 ** lg
            assert np.array_equal(E.fits(q, lg, dtype), R.round_to(v, dtype) == v)
    assert E.width(np.array([0, 12, -40, 7 * 64])) == 3


def test_case_table_covers_the_families():
    by = {}
    for c in CASES:
        by.setdefault((c['family'], c['dtype']), []).append(c)
    for dtype in ('float16', 'bfloat16'):
        for kern in R.KERNELS:
            wave = [c for c in by[('wave', dtype)] if c['kern'] == kern]
            assert {(c['yh'], c['yw']) for c in wave} == {(4, 20), (36, 36), (70, 52)}
            assert any(c['flip'] for c in wave) and any(c['epilogue'] for c in wave) and any(c['clamp'] != E.INF for c in wave)
            tile = [c for c in by[('mfma_tile', dtype)] if c['kern'] == kern]
            assert {(c['yh'], c['yw']) for c in tile} == {(36, 36), (70, 36)} and any(c['clamp'] != E.INF and c['flip'] for c in tile)
            assert all(c['bias'] is not None and (any(c['bias']) == (dtype == 'float16')) for c in tile)
        assert [(c['kern'], c['h'], c['w']) for c in by[('tile', dtype)] if not c['flip']] == [('u2d2', 38, 19), ('u2d2', 70, 17), ('u2d4', 30, 25), ('u4d2', 17, 19)]
        assert all(c['yw'] % 2 == 1 for c in by[('tile', dtype)]), 'an even width would run the matrix-core kernels'
    assert {(c['h'], c['w']) for c in by[('strip', 'float32')]} == {(19, 21), (150, 9)}
    for c in CASES:
        assert c['layout'] == 0 or (c['yw'] % 2 == 0 and c['w'] % 2 == 0), 'matrix-core kernels: even widths, both directions'
        assert c['slope'] in (0.25, 0.5) and c['gain'] == 1.0
        d = E.data(c)
        assert set(np.unique(d['x'])) <= {-1, 0, 1} and set(np.unique(d['g'])) <= {-1, 0, 1}
        if c['density'] is not None:
            assert 0.5 * c['density'] <= (d['x'] != 0).mean() <= 1.5 * c['density']


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_every_rounded_quantity_is_representable(case):
    assert E.representable(case) == 1.0, {k: v for k, v in E.widths(case).items() if v > E.SIG_BITS[case['dtype']]}
    assert E.accumulation_units(case) < 2.0 ** 24, 'an fp32 partial sum could round'


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_reference_is_the_oracle_in_float64(case):
    from oracle import aten_ops as ops
    d, ref = E.data(case), E.reference(case)
    want = ops.filtered_lrelu(torch.from_numpy(d['x']), fu=torch.from_numpy(d['fu']), fd=torch.from_numpy(d['fd']),
                              b=None if d['b'] is None else torch.from_numpy(d['b']), up=case['up'], down=case['down'], padding=case['padding'],
                              gain=case['gain'], slope=case['slope'], clamp=None if case['clamp'] == E.INF else case['clamp'], flip_filter=case['flip'])
    assert want.dtype == torch.float64 and np.array_equal(want.numpy(), ref['F'])
    # ... and the int64 chain behind `representable` is that same function
    q = dict((n, (a, lg)) for n, a, lg in E.quantities(case, 'forward'))
    assert np.array_equal(q['y (fp32 accumulator)'][0] * 2.0 ** -16, ref['F'])
    assert np.array_equal(q['X2'][0] * 2.0 ** -8, ref['u'] * case['gain'])
    qb = dict((n, (a, lg)) for n, a, lg in E.quantities(case, 'backward'))
    assert np.array_equal(qb['y (fp32 accumulator)'][0] * 2.0 ** -16, ref['dx'])
    # one rounding: the rounded reference is a fixed point, and where the epilogue applies it is round((F + skip) oscale)
    assert np.array_equal(R.round_to(ref['expected_y'], case['dtype']), ref['expected_y'])
    if case['epilogue']:
        assert not np.array_equal(ref['y'], ref['F'])
        assert np.array_equal(ref['y'], (ref['F'] + d['skip']) * d['oscale'].reshape(case['n'], case['c'], 1, 1))
        assert set(np.unique(np.log2(d['oscale']))) <= {-2.0, -1.0, 0.0, 1.0, 2.0}


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_outputs_are_not_zero(case):
    ref = E.reference(case)
    assert (ref['expected_y'] != 0).mean() >= 0.9
    assert (ref['expected_dx'] != 0).mean() >= 0.5          # (a clamped element passes no gradient)
    assert (ref['expected_dx'] != 0).reshape(case['n'] * case['c'], -1).any(1).all()


@pytest.mark.parametrize('family,kern', GROUPS, ids=[f'{f}-{k}' for f, k in GROUPS])
def test_one_case_per_kernel_feels_every_tap_and_the_padding(family, kern):
    """In at least one case of each kernel and family, zeroing any single tap of fu or fd, swapping any two adjacent taps, or moving
    the padding by one column or row changes the ROUNDED reference in every 16 x 16 output block of every plane."""
    for case in (c for c in CASES if (c['family'], c['kern']) == (family, kern)):
        d = E.data(case)
        base = E.forward_with(case)
        px0, px1, py0, py1 = case['padding']
        moved = [E.forward_with(case, padding=[px0 + 1, px1 - 1, py0, py1]), E.forward_with(case, padding=[px0, px1, py0 + 1, py1 - 1])]
        if any(m.shape != base.shape or E.blocks_changed(base, m) < 1.0 for m in moved):
            continue
        if all(E.blocks_changed(base, E.forward_with(case, **{which: f})) == 1.0 for which in ('fu', 'fd') for _, f in E.filter_variants(d[which])):
            return
    raise AssertionError(f'no case of {family} {kern} in which every tap and the padding reach every output block')


@pytest.mark.parametrize('case', [c for c in CASES if c['clamp'] != E.INF], ids=[c['id'] for c in CASES if c['clamp'] != E.INF])
def test_clamp_cases_meet_the_clamp_exactly(case):
    ref = E.reference(case)
    assert set(np.unique(ref['codes'])) == {0, 1, 2}
    v = ref['u'] * case['gain']
    v = np.abs(np.where(v < 0, v * case['slope'], v))
    at, over, zero = v == case['clamp'], v > case['clamp'], ref['u'] == 0
    assert at.sum() >= 50 and over.sum() >= 50 and zero.sum() >= 50
    assert (ref['codes'][at] != 2).all() and (ref['codes'][over] == 2).all() and (ref['codes'][zero] == 0).all()
    assert (at & (ref['u'] < 0)).any() and (at & (ref['u'] > 0)).any(), 'the clamp is met exactly on both branches'
    assert not np.signbit(ref['u'][zero]).any()
    # every plane and both halves of the clamp's reach: a clamped element in most 16 x 16 blocks of the upsampled grid
    assert 0.02 <= over.mean() <= 0.6


def test_plane_sum_cases():
    """Each family that returns plane sums has a case per kernel whose UNROUNDED dx is a tensor of the dtype's values."""
    for family in ('wave', 'mfma_tile'):
        for kern in R.KERNELS:
            assert any(E.dx_representable(c) for c in CASES if (c['family'], c['kern']) == (family, kern)), (family, kern)
    assert all(E.dx_representable(c) for c in CASES if c['dtype'] == 'float32')
