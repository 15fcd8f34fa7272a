"""The training log without a device: the restatement of the two kernels (tests/trainlog_ref.py) against math.fsum, the ring unrolling, the column
table against the built library, and the refusals the host makes before anything is launched."""
import math

import numpy as np
import pytest
import torch

import trainlog_ref as R

CHUNK = 16384


def _gradient(n, seed):
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n)).astype(np.float32)
    planted = dict(nan=[0, n // 3], pos=[n - 1], neg=[n // 2, min(n - 1, CHUNK)]) if n >= 8 else dict(nan=[0], pos=[], neg=[])
    for i in planted['nan']:
        g[i] = np.nan
    for i in planted['pos']:
        g[i] = np.inf
    for i in planted['neg']:
        g[i] = -np.inf
    if n >= 8:
        g[1], g[2], g[3] = -0.0, 1e-40, -3e-44                                           # a signed zero and two denormals
    return g


@pytest.mark.parametrize('aligned', [True, False])
@pytest.mark.parametrize('scale', [1.0, 0.5, 1.0 / 3.0])
@pytest.mark.parametrize('n', [1, 5, 1023, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 5])
def test_restated_sumsq_is_within_the_bound_of_any_order_summation(n, scale, aligned):
    """n non-negative float64 terms added in ANY order are within n * 2^-53 relative of the exact sum (each of the at most n - 1 roundings that a
    term passes through is relative 2^-53 of a partial sum that never exceeds the total).  The squares themselves are exact."""
    g = _gradient(n, n)
    part = R.tensor_partials(g, scale, aligned, CHUNK)
    assert part.shape == ((n + CHUNK - 1) // CHUNK, 4)
    gr = R.scaled(g, scale)
    finite = gr[np.isfinite(gr)]
    exact = math.fsum(float(v) * float(v) for v in finite)
    got = float(R.reduce_partials(part)[0])
    assert abs(got - exact) <= n * 2.0 ** -53 * exact, (got, exact)
    assert exact > 0 or n == 1
    counts = R.reduce_partials(part)[1:]
    assert counts.tolist() == [int(np.isnan(gr).sum()), int((gr == np.inf).sum()), int((gr == -np.inf).sum())]
    # per chunk as well, against a plain slice
    for c in range(part.shape[0]):
        piece = gr[c * CHUNK:(c + 1) * CHUNK]
        assert part[c, 1:].tolist() == [int(np.isnan(piece).sum()), int((piece == np.inf).sum()), int((piece == -np.inf).sum())]
        ok = piece[np.isfinite(piece)]
        want = math.fsum(float(v) * float(v) for v in ok)
        assert abs(part[c, 0] - want) <= max(1, ok.size) * 2.0 ** -53 * want


def test_a_finite_gradient_that_overflows_under_the_scale_counts_as_infinite():
    g = np.array([3e38, -3e38, 1.0, np.nan], dtype=np.float32)
    assert R.tensor_partials(g, 1.0, True, CHUNK)[0].tolist() == [float(np.float32(3e38)) ** 2 * 2 + 1.0, 1.0, 0.0, 0.0]
    assert R.tensor_partials(g, 2.0, True, CHUNK)[0].tolist() == [4.0, 1.0, 1.0, 1.0]


def test_the_two_paths_are_two_orders():
    """The aligned and the unaligned order give the same counts and, on most data, sums that differ in the last bits: the flag matters."""
    g = _gradient(CHUNK, 99)
    a, b = R.tensor_partials(g, 1.0, True, CHUNK), R.tensor_partials(g, 1.0, False, CHUNK)
    assert a[0, 1:].tolist() == b[0, 1:].tolist()
    assert abs(a[0, 0] - b[0, 0]) <= CHUNK * 2.0 ** -53 * a[0, 0]


@pytest.mark.parametrize('rows', [1, 255, 256, 257, 600])
def test_restated_append_reduction(rows):
    rng = np.random.default_rng(rows)
    p = np.stack([rng.uniform(0, 1e6, rows), rng.integers(0, CHUNK, rows), rng.integers(0, 9, rows), rng.integers(0, 3, rows)], axis=1).astype(np.float64)
    got = R.reduce_partials(p)
    want = math.fsum(p[:, 0])
    assert abs(got[0] - want) <= rows * 2.0 ** -53 * want
    assert got[1:].tolist() == p[:, 1:].sum(0).tolist()
    row = R.append_row(7, None, 3.0, None, [1.5, np.nan, 0.25, 2.0, np.nan], p, None)
    assert row[0] == 7.0 and np.isnan(row[1:9]).all() and row[9] == 3.0 and np.isnan(row[10]) and np.isnan(row[20:]).all()
    assert R.same_bits(row[16:20], got) and np.array_equal(row[11:16], [1.5, np.nan, 0.25, 2.0, np.nan], equal_nan=True)


@pytest.mark.parametrize('capacity', [1, 4])
def test_ring_unrolling(capacity):
    from afcm_amd.trainlog import unroll
    cols = 3
    for head in (0, capacity - 1, capacity, 2 * capacity + 3):
        if head < 0:
            continue
        ring = np.full((capacity, cols), -1.0)
        for s in range(head):                                                            # what `head` appends leave behind
            ring[s % capacity] = [s, 10.0 * s, -s]
        live = max(0, head - capacity)
        for since in (None, 0, live, live + 1, max(0, live - 1), head, head + 5):
            rows, lost = unroll(ring, head, since)
            want, want_lost = R.unroll(ring, head, since)
            first = 0 if since is None else since
            assert rows.dtype == np.float64 and rows.shape == want.shape and np.array_equal(rows, want) and lost == want_lost
            assert rows[:, 0].tolist() == [float(s) for s in range(min(max(first, live), head), head)]
            assert lost == max(0, live - first)
            assert len(rows) + lost == max(0, head - first)
    with pytest.raises(ValueError):
        unroll(np.zeros((capacity, cols)), -1)
    with pytest.raises(ValueError):
        unroll(np.zeros((capacity, cols)), 3, since=-2)


def test_columns_match_the_library():
    from afcm_amd import _lib
    from afcm_amd.trainlog import COLUMNS, LOSSES
    lib = _lib.load()
    for name in ('afcm_grad_stats', 'afcm_trainlog_append', 'afcm_trainlog_cols'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert len(COLUMNS) == lib.afcm_trainlog_cols() == R.COLS and len(set(COLUMNS)) == len(COLUMNS)
    assert COLUMNS[0] == 'serial' and COLUMNS[1] == 'total_iters' and COLUMNS[5:7] == ('lr_G', 'lr_D') and COLUMNS[9:11] == ('step_G', 'step_D')
    assert COLUMNS[11:16] == LOSSES == ('G_GAN', 'G_L1', 'D_real', 'D_fake', 'Dr1')
    assert COLUMNS[16:20] == ('G_sumsq', 'G_nan', 'G_posinf', 'G_neginf') and COLUMNS[20:24] == ('D_sumsq', 'D_nan', 'D_posinf', 'D_neginf')
    assert lib.afcm_abi_version() == 13


def test_host_refusals_and_a_host_side_ring():
    from afcm_amd.optim import FusedScrubAdam
    from afcm_amd.stylegan3_model import StyleGAN3GeneratorStep
    from afcm_amd.trainlog import COLUMNS, DeviceTrainLog
    for capacity in (0, -3):
        with pytest.raises(ValueError, match='capacity'):
            DeviceTrainLog(capacity, 'cpu')
    log = DeviceTrainLog(4, 'cpu')                                                       # the storage may live anywhere; appending needs the device
    assert log.log.shape == (4, len(COLUMNS)) and log.log.dtype == torch.float64 and log.head.dtype == torch.int64 and int(log.head) == 0
    rows, lost = log.read()
    assert rows.shape == (0, len(COLUMNS)) and rows.dtype == np.float64 and lost == 0
    for s in range(6):                                                                   # what six appends would leave
        log.log[s % 4] = float(s)
    log.head.fill_(6)
    rows, lost = log.read()
    assert rows[:, 0].tolist() == [2.0, 3.0, 4.0, 5.0] and lost == 2
    rows, lost = log.read(since=4)
    assert rows[:, 0].tolist() == [4.0, 5.0] and lost == 0
    saved = log.snapshot()
    log.log.fill_(-1.0), log.head.fill_(9)
    log.restore(saved, head_only=True)
    assert int(log.head) == 6 and float(log.log[0, 0]) == -1.0
    log.restore(saved)
    assert log.read()[0][:, 0].tolist() == [2.0, 3.0, 4.0, 5.0]

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.mapping = torch.nn.Linear(2, 2, device='meta')
            self.synthesis = torch.nn.Linear(2, 2, device='meta')
    with pytest.raises(RuntimeError, match='own device'):
        StyleGAN3GeneratorStep(Net(), log=log)
    with pytest.raises(RuntimeError, match='ROCm device'):
        log.append(object())
    with pytest.raises(RuntimeError, match='stats=True'):
        FusedScrubAdam([torch.nn.Parameter(torch.zeros(3))]).grad_stats()
    opt = FusedScrubAdam([torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(CHUNK + 1))], stats=True)
    partials, chunks = opt.grad_stats()
    assert partials.shape == (3, 4) and partials.dtype == torch.float64 and chunks == 0   # sized from every parameter of the group, at construction
    assert len(opt.snapshot()) == 3 and len(FusedScrubAdam([torch.nn.Parameter(torch.zeros(3))]).snapshot()) == 2
