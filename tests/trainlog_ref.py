"""Numpy restatement of csrc/trainlog.hip in the orders the kernels state, and of the ring unrolling.  No torch, no device: the CPU tests hold it to
math.fsum, the GPU tests hold the kernels to it bit for bit.

grad_stats_kernel, one chunk of `chunk` elements of one tensor, 256 threads:
  gr = g * grad_scale in float32; counts of gr NaN / +inf / -inf; every FINITE gr contributes (double)gr * (double)gr (exact: 48 bits).
  thread t adds its contributions in ascending element index from +0.0 -- elements 4 t + 1024 k + {0, 1, 2, 3} of the chunk where g is 16-byte aligned,
  t + 256 k where it is not; then the tree s[t] += s[t + o], o = 128, 64, ..., 1.
trainlog_append_kernel, per column of a [rows, 4] table: thread t adds rows t, t + 256, ... in ascending order from +0.0; then the same tree.
A missing element or row contributes +0.0, which changes no sum of non-negative terms: the restatement pads with zeros.
"""
import numpy as np

COLS = 24
THREADS = 256


def scaled(g, grad_scale):
    """g * grad_scale as the kernels form it: one float32 product."""
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        return (np.asarray(g, dtype=np.float32) * np.float32(grad_scale)).astype(np.float32)


def tree(a):
    """[..., 256] -> [...]: s[t] += s[t + o] for o = 128 ... 1."""
    n = THREADS
    assert a.shape[-1] == n
    while n > 1:
        n //= 2
        a = a[..., :n] + a[..., n:2 * n]
    return a[..., 0]


def _sequential(seq):
    """[..., 256, k] -> [..., 256]: every thread's terms added one after the other, from +0.0."""
    acc = np.zeros(seq.shape[:-1], dtype=np.float64)
    for k in range(seq.shape[-1]):
        acc = acc + seq[..., k]
    return acc


def tensor_partials(g, grad_scale, aligned, chunk):
    """The rows {sumsq, n_nan, n_posinf, n_neginf} of one tensor's chunks: float64 [ceil(numel / chunk), 4]."""
    gr = scaled(np.asarray(g).reshape(-1), grad_scale)
    rows = (gr.size + chunk - 1) // chunk
    padded = np.zeros(rows * chunk, dtype=np.float32)
    padded[:gr.size] = gr
    per_chunk = padded.reshape(rows, chunk)
    finite = np.isfinite(per_chunk)
    d = np.where(finite, per_chunk, np.float32(0)).astype(np.float64)
    sq = d * d
    if aligned:
        seq = sq.reshape(rows, chunk // (4 * THREADS), THREADS, 4).transpose(0, 2, 1, 3).reshape(rows, THREADS, -1)
    else:
        seq = sq.reshape(rows, chunk // THREADS, THREADS).transpose(0, 2, 1)
    out = np.empty((rows, 4), dtype=np.float64)
    out[:, 0] = tree(_sequential(seq))
    out[:, 1] = np.isnan(per_chunk).sum(1)
    out[:, 2] = (per_chunk == np.inf).sum(1)
    out[:, 3] = (per_chunk == -np.inf).sum(1)
    return out


def table_partials(tensors, grad_scale, chunk):
    """``tensors``: [(gradient array, its pointer is 16-byte aligned)] in table order -> the partials the launch writes."""
    return np.concatenate([tensor_partials(g, grad_scale, aligned, chunk) for g, aligned in tensors], axis=0)


def reduce_partials(partials):
    """[rows, 4] -> [4] in the append kernel's order."""
    p = np.asarray(partials, dtype=np.float64).reshape(-1, 4)
    k = max(1, (p.shape[0] + THREADS - 1) // THREADS)
    padded = np.zeros((k * THREADS, 4), dtype=np.float64)
    padded[:p.shape[0]] = p
    return tree(_sequential(padded.reshape(k, THREADS, 4).transpose(2, 1, 0)))


def append_row(serial, block=None, step_G=None, step_D=None, losses=None, partials_G=None, partials_D=None):
    """The row afcm_trainlog_append writes; None is a NULL pointer."""
    row = np.full(COLS, np.nan, dtype=np.float64)
    row[0] = float(serial)
    if block is not None:
        row[1:9] = np.asarray(block, dtype=np.float64)
    if step_G is not None:
        row[9] = float(np.float32(step_G))
    if step_D is not None:
        row[10] = float(np.float32(step_D))
    if losses is not None:
        row[11:16] = np.asarray(losses, dtype=np.float32).astype(np.float64)
    if partials_G is not None:
        row[16:20] = reduce_partials(partials_G)
    if partials_D is not None:
        row[20:24] = reduce_partials(partials_D)
    return row


def unroll(ring, head, since=None):
    """Serial by serial: row s lives at s % capacity while s >= head - capacity."""
    ring = np.asarray(ring)
    capacity = ring.shape[0]
    rows, lost = [], 0
    for s in range(0 if since is None else since, head):
        if s < head - capacity:
            lost += 1
        else:
            rows.append(ring[s % capacity])
    return np.array(rows, dtype=ring.dtype).reshape(len(rows), ring.shape[1]), lost


def same_bits(a, b):
    """Equal as bit patterns (so NaN equals NaN, and +0.0 differs from -0.0)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))
