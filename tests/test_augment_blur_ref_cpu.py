"""afcm_amd/augment_blur.py -- the numpy arm the GPU tests compare the kernels with, bit for bit -- against scipy (tests/augment_blur_ref.py:
``gaussian_filter(mode='nearest', truncate=4.0)`` on ``[1, h, w]``, the call skimage's ``gaussian`` documents) and against the golden captured from
the reference's own ``GaussianBlur3D`` (tools/gen_golden_augment_blur.py).  Every comparison with scipy is ``np.array_equal``: scipy's symmetric
``correlate1d`` has one order of operations and ``blur_host`` restates it."""
import os
import random

import numpy as np
import pytest
import torch

import augment_blur_ref as R
from afcm_amd import augment_blur as B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'A3_augment_blur.npz')


@pytest.mark.parametrize('float32_valued', [False, True])
@pytest.mark.parametrize('shape', R.SHAPES)
def test_blur_host_is_scipys_gaussian_filter_bit_for_bit(shape, float32_valued):
    v = R.volume(shape, seed=shape[1] * 7 + shape[2], float32_valued=float32_valued)
    for sigma in R.SIGMAS:
        radius, w = B.gaussian_weights(sigma)
        assert radius == int(4.0 * sigma + 0.5) <= B.R_MAX
        got = B.blur_host(v, radius, w)
        assert got.dtype == np.float64 and got.shape == v.shape
        assert np.array_equal(got, R.blur(v, sigma)), (shape, sigma)
    assert 2 * B.gaussian_weights(4.1)[0] + 1 > shape[1] or shape[1] >= 64        # planes narrower than the filter are in the grid


def test_the_golden_from_the_references_class():
    g = np.load(GOLDEN)
    x, draws, which = g['x'], g['draws'], g['which']
    assert x.shape == (3, 1, 24, 32) and np.array_equal(x, x.astype(np.float32).astype(np.float64)) and not x[2].any()
    executed = ~np.isnan(draws[:, 1])
    assert len(which) >= 12 and executed.any() and (~executed).any() and np.array_equal(executed, draws[:, 0] < float(g['prob']))
    for n, (plane, (u, sigma)) in enumerate(zip(which, draws)):
        want = g['out'][n]
        if executed[n]:
            radius, w = B.gaussian_weights(sigma)
            assert np.array_equal(B.blur_host(x[plane], radius, w), want), n
            assert np.array_equal(R.blur(x[plane], sigma), want)
        else:
            assert np.array_equal(x[plane], want)
    # blur_rows with the golden's seed: the same decisions and sigmas in the same order, the planes of zeros included.  The stream is consumed
    # plane after plane whatever the grouping: six items of 1 + 1 planes, and two of 4 + 1 (the first ten draws)
    config = B.BlurConfig(sigma=tuple(g['sigma']), execution_probability=float(g['prob']))
    for n_items, k in ((len(which) // 2, 1), (len(which) // 5, 4)):
        rows = B.blur_rows(config, n_items, k, int(g['seed'])).reshape(-1, B.PLANE_COLS)
        for rec, (u, sigma), ran in zip(rows, draws, executed):
            assert rec[0] == float(ran)
            if ran:
                assert rec[1] == sigma and np.array_equal(rec, B.plane_record(sigma))
            else:
                assert np.array_equal(rec, B.IDENTITY_PLANE)


def test_gaussian_weights():
    for sigma, radius in [(0.1, 0), (0.124, 0), (0.125, 1), (0.374, 1), (0.375, 2), (0.376, 2), (1.0, 4), (2.0, 8), (4.1, 16), (4.124, 16)]:
        r, w = B.gaussian_weights(sigma)
        assert r == radius and w.shape == (radius + 1,) and w.dtype == np.float64
        x = np.arange(-r, r + 1)
        phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
        phi = phi / phi.sum()
        assert np.array_equal(phi[::-1], phi) and np.array_equal(phi[r:], w)      # exactly symmetric: one weight per pair
        assert abs((w[0] + 2 * w[1:].sum()) - 1.0) < 1e-15 and bool((np.diff(w) < 0).all())
    assert np.array_equal(B.gaussian_weights(0.1)[1], [1.0])                       # the single tap
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(RuntimeError, match='positive and finite'):
            B.gaussian_weights(bad)
    with pytest.raises(RuntimeError, match='above 16'):
        B.plane_record(4.125)


def test_config_refusals():
    c = B.BlurConfig()
    assert c.sigma == (0.1, 2.0) and c.execution_probability == 0.5
    assert B.BlurConfig(sigma=[0.5, 0.5], execution_probability=1).sigma == (0.5, 0.5)
    assert B.BlurConfig(sigma=(0.1, 4.124)).sigma[1] == 4.124
    for kw, message in [(dict(sigma=(0.0, 2.0)), 'must be positive'), (dict(sigma=(-0.1, 2.0)), 'must be positive'), (dict(sigma=(2.0, 1.0)), 'must be ordered'),
                        (dict(sigma=(0.1, 4.125)), 'above 16'), (dict(sigma=(0.1, 9.0)), 'above 16'), (dict(sigma=(0.1, np.nan)), 'two finite numbers'),
                        (dict(sigma=0.5), 'two finite numbers'), (dict(sigma=(0.1, 1.0, 2.0)), 'two finite numbers'),
                        (dict(execution_probability=-0.01), r'in \[0, 1\]'), (dict(execution_probability=1.01), r'in \[0, 1\]'),
                        (dict(execution_probability=np.nan), r'in \[0, 1\]'), (dict(execution_probability=True), r'in \[0, 1\]')]:
        with pytest.raises(RuntimeError, match=message):
            B.BlurConfig(**kw)


def test_rows_their_layout_and_the_check():
    assert B.R_MAX == 16 and B.PLANE_COLS == 20
    assert B.identity_rows(3, 4).shape == (3, 100) and B.identity_rows(3, 1).shape == (3, 40)
    assert all(B.row_is_valid(r) for r in B.identity_rows(2, 4)) and not B.identity_rows(2, 4)[:, ::20].any()
    rows = B.blur_rows(B.BlurConfig(execution_probability=1.0), 3, 4, 5)
    assert rows.shape == (3, 100) and rows.dtype == np.float64 and all(B.row_is_valid(r) for r in rows)
    for rec in rows.reshape(-1, 20):
        radius, w = B.gaussian_weights(rec[1])
        assert rec[0] == 1.0 and rec[2] == radius and np.array_equal(rec[3:4 + radius], w) and not rec[4 + radius:].any()
    for name, (col, value) in R.INVALID.items():
        for plane in (0, 4):
            bad = rows[1].copy()
            bad[plane * 20 + col] = value
            assert not B.row_is_valid(bad), name
    assert B.row_is_valid(rows[0][:20]) and not B.row_is_valid(rows[0][:30]) and not B.row_is_valid(rows[:2])
    assert B.checked_rows(rows, 3, 4, 'here') is not None
    for bad in (rows[:2], rows[:, :40], rows.astype(np.float32)):
        with pytest.raises(RuntimeError, match=r'float64 \[3, 100\]'):
            B.checked_rows(bad, 3, 4, 'here')
    with pytest.raises(RuntimeError, match='BlurConfig'):
        B.blur_rows(None, 3, 4, 5)
    with pytest.raises(RuntimeError, match='random.Random'):
        B.blur_rows(B.BlurConfig(), 3, 4, np.random.default_rng(1))


class _Counting(random.Random):
    def __init__(self, seed):
        super().__init__(seed)
        self.calls = []

    def random(self):
        self.calls.append('random')
        return super().random()

    def uniform(self, a, b):
        self.calls.append('uniform')
        before = len(self.calls)
        value = super().uniform(a, b)                                             # CPython's uniform calls self.random() once
        del self.calls[before:]
        return value


def test_blur_rows_draws_once_for_a_plane_left_alone_and_twice_for_a_blurred_one():
    config = B.BlurConfig()
    rng = _Counting(3)
    rows = B.blur_rows(config, 6, 4, rng).reshape(-1, 20)
    executed = int(rows[:, 0].sum())
    assert 5 <= executed <= 25 and rng.calls.count('random') == 30 and rng.calls.count('uniform') == executed
    plain = random.Random(3)                                             # the stream itself: one value per call, in order
    for rec in rows:
        u = plain.random()
        assert (u < 0.5) == (rec[0] == 1.0)
        if rec[0] == 1.0:
            assert rec[1] == 0.1 + (2.0 - 0.1) * plain.random()
    # the same seed as an int, and probabilities 0 and 1
    assert np.array_equal(B.blur_rows(config, 6, 4, 3).reshape(-1, 20), rows)
    assert np.array_equal(B.blur_rows(B.BlurConfig(execution_probability=0.0), 2, 1, 1), B.identity_rows(2, 1))


def test_apply_host():
    x = torch.from_numpy(R.volume((5, 24, 32), 9, True).astype(np.float32))
    x[3, 2, 2] = -0.0
    row = B.identity_rows(1, 4)[0].reshape(5, 20)
    row[1], row[4] = B.plane_record(1.37), B.plane_record(0.1)
    got = B.apply_host(x, row.reshape(-1))
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and got.shape == x.shape
    for p in (0, 2, 3):                                                           # a flag-0 plane keeps its bits
        assert torch.equal(got[p].view(torch.int32), x[p].view(torch.int32))
    want = R.blur(x[1:2].numpy().astype(np.float64), 1.37).astype(np.float32)[0]
    assert np.array_equal(got[1].numpy(), want) and not torch.equal(got[1], x[1])
    assert torch.equal(got[4], x[4])                                              # sigma 0.1: the single tap 1.0, x * 1.0 three times
    assert np.array_equal(R.numpy_blur_item(x.numpy(), row.reshape(-1)), got.numpy())
    assert isinstance(B.apply_host(x.numpy(), row.reshape(-1)), np.ndarray)
    one = B.apply_host(x[1:2], row[1])                                            # a single plane with its own record
    assert torch.equal(one[0], got[1])
    bad = row.copy()
    bad[2, 2] = 17.0
    for args in ((x, bad.reshape(-1)), (x, row.reshape(-1)[:80]), (x.double(), row.reshape(-1)), (x[0], row.reshape(-1))):
        with pytest.raises(RuntimeError, match='apply_host'):
            B.apply_host(*args)
