"""afcm_amd/augment_elastic.py -- the numpy arm the GPU tests compare the kernels with, bit for bit -- against scipy (tests/augment_elastic_ref.py:
``gaussian_filter`` and ``map_coordinates`` on ``[1, h, w]``, as the reference's class calls them) and against the golden captured from the
reference's own ``ElasticDeformation`` (tools/gen_golden_augment_elastic.py).  Every plane compared with scipy is at least 20 in both extents:
scipy's 'reflect' prefilter is not the exact interpolating spline below about 16 (augment_elastic_ref.py); the short lines are held to the
project's own statement, reconstruction of the samples.

The bounds are 16 x the largest difference measured over these cases with numpy 2.2.6 and scipy 1.15.3 (the margin covers other summation orders
in other builds), relative to ``alpha max|field|`` for displacements and absolute for pixel values in [-1, 1]:

    displacements vs gaussian_filter (sigma 50 and 2; 24 x 32 and 256 x 256)   6.83e-17 relative    bound 1.10e-15
    coefficients vs spline_filter (20 x 20, 24 x 32, 256 x 256)                 1.78e-15             bound 2.85e-14
    deform vs map_coordinates, the same displacement arrays: order 0            exact                exact
                                                             order 1            2.23e-16             bound 3.57e-15
                                                             order 3            8.89e-16             bound 1.43e-14
    the whole stage vs the E1 golden (orders 1 and 3; order 0 exact)            7.54e-14             bound 1.21e-12
    reconstruction of the samples at lengths 1, 2, 3, 7, 16                     5.56e-16             bound 8.90e-15

The golden's figure is the largest: there each side reads the plane at its own displacements, which differ by 1e-13 pixels at alpha 2000.
"""
import os

import numpy as np
import pytest

import augment_elastic_ref as R
from afcm_amd import augment_elastic as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'E1_augment_elastic.npz')

# 16 x the measured figures of the docstring
BOUND_DISPLACEMENT = 16 * 6.83e-17
BOUND_COEFFICIENTS = 16 * 1.78e-15
BOUND_DEFORM = {1: 16 * 2.23e-16, 3: 16 * 8.89e-16}
BOUND_GOLDEN = 16 * 7.54e-14
BOUND_RECONSTRUCTION = 16 * 5.56e-16


def _plane(h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    raw = np.clip(128 + 90 * np.sin(0.5 * y + 0.3 * x + seed) + rng.integers(-30, 31, (h, w)), 0, 255)
    return (2.0 * (raw / 255.0) - 1.0).astype(np.float32).astype(np.float64)


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize('hw', [(24, 32), (256, 256)])
@pytest.mark.parametrize('sigma', [50.0, 2.0])
def test_folded_operator_against_gaussian_filter(hw, sigma):
    h, w = hw
    alpha = 2000.0
    fy, fx = np.random.default_rng(3).standard_normal((2, h, w))
    op_h, op_w = E.smoothing_operator(sigma, h), E.smoothing_operator(sigma, w)
    assert op_h.shape == (h, h) and np.allclose(op_h.sum(1), 1.0, rtol=0, atol=1e-12)
    if sigma == 2.0:                                                              # banded: radius 8
        i, m = np.mgrid[0:h, 0:h]
        assert not op_h[np.abs(i - m) > 8].any() and (op_h[np.abs(i - m) <= 8] > 0).all()
    else:
        assert (op_h > 0).all() or h > 200                                        # 401 taps folded over the whole of a short line
    dy, dx = E.displacement_host(np.array([1.0, alpha, 0.0, 0.0]), h, w, op_h, op_w, fields=(fy, fx))
    scale = alpha * max(np.abs(fy).max(), np.abs(fx).max())
    err = max(np.abs(dy - R.displacement(fy, sigma, alpha)).max(), np.abs(dx - R.displacement(fx, sigma, alpha)).max()) / scale
    print(f'displacement {hw} sigma {sigma}: {err:.3e} relative')
    assert err <= BOUND_DISPLACEMENT


def test_generated_fields_are_the_intensity_normals_on_their_own_counters():
    from afcm_amd import augment_intensity as I
    row = np.array([1.0, 3.0, 17.0, 4.0])
    h, w = 21, 37
    op_h, op_w = np.eye(h), np.eye(w)                                             # no smoothing: the displacement is alpha times the field
    dy, dx = E.displacement_host(row, h, w, op_h, op_w)
    fy, fx = I.normal_field(17, 4, h, w, 0, 1), I.normal_field(17, 4, h, w, 0, 2)
    assert np.array_equal(dy, 3.0 * fy) and np.array_equal(dx, 3.0 * fx)
    noise = I.normal_field(17, 4, h, w)                                           # the Gaussian noise of the same key: another counter
    assert not np.array_equal(fy, noise) and not np.array_equal(fx, noise) and not np.array_equal(fy, fx)
    both = np.concatenate([fy.ravel(), fx.ravel()])
    assert abs(both.mean()) < 0.1 and abs(both.std() - 1.0) < 0.1


@pytest.mark.parametrize('hw', [(24, 32), (20, 20), (256, 256)])
def test_spline_coefficients_against_spline_filter(hw):
    p = _plane(*hw, seed=5)
    err = np.abs(E.spline_coefficients_host(p) - R.coefficients(p)).max()
    print(f'coefficients {hw}: {err:.3e}')
    assert err <= BOUND_COEFFICIENTS


def _reconstruct(c):
    """sum c beta^3 at the samples of a line: (c[k - 1] + 4 c[k] + c[k + 1]) / 6 with the half-sample symmetric boundary."""
    n = c.shape[0]
    k = np.arange(n)
    return (c[E.reflect(k - 1, n)] + 4.0 * c + c[E.reflect(k + 1, n)]) / 6.0


@pytest.mark.parametrize('n', [1, 2, 3, 7, 16])
def test_spline_coefficients_reconstruct_their_input_at_every_length(n):
    """scipy's prefilter does not at these lengths (its residual is 2e-4 at n = 2)."""
    rng = np.random.default_rng(n)
    line = rng.uniform(-1, 1, n)
    err = np.abs(_reconstruct(E.spline_coefficients_host(line)) - line).max()
    plane = rng.uniform(-1, 1, (n, n + 2))
    c = E.spline_coefficients_host(plane)
    rows = np.stack([_reconstruct(r) for r in c])                                 # along x, then along y
    err = max(err, np.abs(np.stack([_reconstruct(col) for col in rows.T]).T - plane).max())
    print(f'reconstruction n = {n}: {err:.3e}')
    assert err <= BOUND_RECONSTRUCTION


@pytest.mark.parametrize('order', [0, 1, 3])
def test_deform_against_map_coordinates(order):
    """The same displacement arrays on both sides: small ones, and ones beyond one period of the plane in both directions."""
    h, w = 24, 32
    p = np.stack([_plane(h, w, seed=s) for s in (1, 2)])
    rng = np.random.default_rng(9)
    worst = 0.0
    for reach in (1.5, 7.0, 90.0, 1000.0):
        dy, dx = rng.uniform(-reach, reach, (2, h, w))
        got = E.deform_host(p, dy, dx, order)
        want = np.stack([R.deform(q, dy, dx, order) for q in p])
        if order == 0:
            assert np.array_equal(got, want)
        worst = max(worst, np.abs(got - want).max())
    print(f'deform order {order}: {worst:.3e}')
    if order != 0:
        assert worst <= BOUND_DEFORM[order]


def test_deform_guards_wild_coordinates():
    p = _plane(24, 32, seed=1)[None]
    dy, dx = np.zeros((24, 32)), np.zeros((24, 32))
    dy[3, 4], dx[5, 6], dy[7, 8], dx[9, 10], dy[11, 12] = np.nan, np.inf, -1e300, 2.0 ** 30 + 1, 2.0 ** 30 - 12
    for order in E.ORDERS:
        out = E.deform_host(p, dy, dx, order)[0]
        assert np.isnan(out[[3, 5, 7, 9], [4, 6, 8, 10]]).all() and int(np.isnan(out).sum()) == 4      # 2^30 - 1 itself is inside the guard
    with pytest.raises(RuntimeError, match='spline order'):
        E.deform_host(p, dy, dx, 2)


def test_whole_stage_against_the_reference_golden(golden):
    x, cases, fields, out = golden['x'], golden['cases'], golden['fields'], golden['out']
    assert x.shape[1:] == (24, 32) and float(golden['prob']) == 0.1
    seen, worst = set(), 0.0
    for (draw, order, apply_3d, sigma, alpha, which), f, want in zip(cases, fields, out):
        p, order = x[int(which)], int(order)
        executed = draw < 0.1
        seen.add((order, bool(apply_3d), bool(executed), sigma))
        # the golden is what this test file's scipy restatement says too (apply_3d: the z displacement of a depth-1 plane changes nothing)
        again = R.elastic(p, draw, f, order, alpha, sigma, 0.1, bool(apply_3d))
        assert np.abs(again - want).max() <= 1e-13
        if not executed:
            assert np.array_equal(want, p)
            continue
        config = E.ElasticConfig(spline_order=order, alpha=alpha, sigma=sigma, execution_probability=0.1, apply_3d=bool(apply_3d))
        ops = E.smoothing_operator(sigma, 24), E.smoothing_operator(sigma, 32)
        dy, dx = E.displacement_host(np.array([1.0, alpha, 0.0, 0.0]), 24, 32, *ops, fields=(f[1], f[2]))
        got = E.deform_host(p[None], dy, dx, config.spline_order)[0]
        if order == 0:                                                            # no coordinate of the golden lies within 1e-9 of a tie
            assert np.array_equal(got, want)
        else:
            worst = max(worst, np.abs(got - want).max())
        # apply_host: the same on the float32 plane, one rounding to float32
        host = E.apply_host(p[None].astype(np.float32), np.array([1.0, alpha, 0.0, 0.0]), config, ops, fields=(f[1], f[2]))
        assert host.dtype == np.float32 and np.array_equal(host[0], got.astype(np.float32))
    assert {s[0] for s in seen} == {0, 1, 3} and {s[1] for s in seen} == {True, False} and {s[2] for s in seen} == {True, False}
    assert {s[3] for s in seen} == {2.0, 50.0}
    equal = cases[(cases[:, 0] == 0.1)]
    assert len(equal) == 1                                                        # a draw equal to the probability is in the golden, not executed
    print(f'golden: {worst:.3e}')
    assert worst <= BOUND_GOLDEN


def test_rows_draw_order_strictness_and_validity():
    config = E.ElasticConfig(execution_probability=0.4, alpha=123.0, sigma=3.0)
    rows = E.elastic_rows(config, 50, np.random.default_rng(8))
    rng = np.random.default_rng(8)                                                # the decisions first, then the keys
    flags, keys = rng.uniform(size=50) < 0.4, rng.integers(0, 2 ** 32, (50, 2))
    assert rows.shape == (50, 4) and rows.dtype == np.float64
    assert np.array_equal(rows[:, 0], flags.astype(np.float64)) and 10 < flags.sum() < 35
    assert np.array_equal(rows[:, 1], np.full(50, 123.0)) and np.array_equal(rows[:, 2:], keys.astype(np.float64))
    assert all(E.row_is_valid(r) for r in rows)

    class Fixed(np.random.Generator):                                             # a generator whose decision draws are the listed ones
        def __init__(self, draws):
            super().__init__(np.random.PCG64(0))
            self.draws = np.asarray(draws)

        def uniform(self, *args, size=None, **kw):
            return self.draws[:size]

    p = 0.1
    rows = E.elastic_rows(E.ElasticConfig(execution_probability=p), 3, Fixed([np.nextafter(p, 0), p, np.nextafter(p, 1)]))
    assert rows[:, 0].tolist() == [1.0, 0.0, 0.0]                                 # strict: a draw equal to the probability does not execute
    assert E.elastic_rows(E.ElasticConfig(execution_probability=0.0), 20, np.random.default_rng(1))[:, 0].sum() == 0
    assert E.elastic_rows(E.ElasticConfig(execution_probability=1.0), 20, np.random.default_rng(1))[:, 0].sum() == 20

    assert np.array_equal(E.identity_rows(3), np.zeros((3, 4))) and all(E.row_is_valid(r) for r in E.identity_rows(3))
    good = np.array([1.0, -2.0 ** 20, 2.0 ** 32 - 1, 0.0])
    assert E.row_is_valid(good) and not E.row_is_valid(good[:3])
    for name, (col, value) in R.INVALID.items():
        bad = good.copy()
        bad[col] = value
        assert not E.row_is_valid(bad), name
        with pytest.raises(RuntimeError, match='not a valid elastic row'):
            E.apply_host(np.zeros((1, 20, 20), np.float32), bad, config)
    with pytest.raises(RuntimeError, match=r'float64 \[5, 4\]'):
        E.checked_rows(np.zeros((4, 4)), 5, 'here')
    with pytest.raises(RuntimeError, match=r'float64 \[4, 4\]'):
        E.checked_rows(np.zeros((4, 4), np.float32), 4, 'here')
    assert E.checked_rows(np.zeros((4, 4)), 4, 'here').shape == (4, 4)
    for bad in (dict(spline_order=2), dict(spline_order=True), dict(alpha=np.inf), dict(alpha=2.0 ** 21), dict(sigma=0.0), dict(sigma=-1.0),
                dict(execution_probability=1.5), dict(apply_3d=1)):
        with pytest.raises(RuntimeError, match='ElasticConfig'):
            E.ElasticConfig(**bad)
    planes = np.zeros((2, 20, 20), np.float32)
    assert E.apply_host(planes, E.identity_rows(1)[0], config) is planes          # flag 0: the planes as they are
