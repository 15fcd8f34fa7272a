"""numpy restatement of batch_assemble_kernel (afcm_amd/csrc/batch.hip) AS THE KERNEL COMPUTES, guards included: every item is decoded from its table
row, checked against the volume table and the pool before anything is read, and gathered with ``volume_ref.assemble`` from its own two volumes.
tests/test_train_batch_ref_cpu.py holds it to ``SliceDataset(phase='train')``; tests/test_gpu_train_batch.py holds the kernel to the same items and,
for invalid rows, to this file.  Also the cases both test files share."""
import numpy as np

import volume_ref as R

SUBJECT_SHAPES = ((7, 13, 18), (11, 20, 16), (5, 16, 23))     # into 16 x 16: a pad in y and odd / zero crop offsets in x; t = depth for subject 2
THICKNESSES = (2, 3, 5)
PATCHES = ((16, 16), (12, 10))                                # (12, 10): w a multiple of neither 4 nor 8, every row ends in the scalar tail
DTYPES = (np.uint8, np.int16, np.float32, np.float64)
BATCH = 5                                                     # 23 rows: four batches of 5 and a ragged one of 3


def value_range(dtype):
    return (0., 255.) if dtype == np.uint8 else (-100., 900.)


def subjects(dtype, modalities=('t1', 't2')):
    """One mapping {modality: volume} per subject; the modalities are independent draws."""
    return [{m: R.source(shape, dtype, seed=20 + 7 * s + j) for j, m in enumerate(modalities)} for s, shape in enumerate(SUBJECT_SHAPES)]


def pool_and_table(volumes, paths):
    """The pool (1-D, subject by subject, modality by modality) and the int64 [n, 4] table (offset, depth, hs, ws)."""
    rows, parts, offset = [], [], 0
    for subject in volumes:
        for p in paths:
            v = subject[p]
            rows.append((offset,) + v.shape)
            parts.append(v.reshape(-1))
            offset += v.size
    return np.concatenate(parts), np.array(rows, dtype=np.int64)


def shuffled_items(k, seed=5, thickness=True):
    """All 23 (subject, idx) of SUBJECT_SHAPES, shuffled, input modality 0 and target modality 1, a thickness from THICKNESSES per row
    (``thickness`` False: -1, the loader's "no thickness", k = 1 only)."""
    rng = np.random.default_rng(seed)
    rows = [(s, i) for s, shape in enumerate(SUBJECT_SHAPES) for i in range(shape[0])]
    rows = [rows[j] for j in rng.permutation(len(rows))]
    t = rng.choice(THICKNESSES, len(rows)) if thickness else np.full(len(rows), -1)
    assert thickness or k == 1
    return np.array([(2 * s, 2 * s + 1, i, tt) for (s, i), tt in zip(rows, t)], dtype=np.int32)


def _descriptor_ok(d, pool_elems):
    off, depth, hs, ws = (int(v) for v in d)
    return depth > 0 and hs > 0 and ws > 0 and off >= 0 and off + depth * hs * ws <= pool_elems


def item_valid(pool_elems, vols, items, row, k):
    if not 0 <= row < len(items):
        return False
    va, vb, idx, t = (int(v) for v in items[row])
    if not (0 <= va < len(vols) and 0 <= vb < len(vols)):
        return False
    if not (_descriptor_ok(vols[va], pool_elems) and _descriptor_ok(vols[vb], pool_elems)) or tuple(vols[va][1:]) != tuple(vols[vb][1:]):
        return False
    return 0 <= idx < int(vols[va][1]) and t != 0 and (k == 1 or t >= 1)


def assemble_batch(pool, vols, items, first, count, k, h, w, lo=0.0, hi=255.0, cursor=0):
    """A [count, k, h, w], B [count, 1, h, w], slice_idx [count, 1], float32; an invalid item is NaN throughout and reads nothing."""
    a = np.full((count, k, h, w), np.nan, dtype=np.float32)
    b = np.full((count, 1, h, w), np.nan, dtype=np.float32)
    slice_idx = np.full((count, 1), np.nan, dtype=np.float32)
    for i in range(count):
        row = cursor + first + i
        if not (0 <= cursor < len(items)) or not item_valid(pool.size, vols, items, row, k):
            continue
        va, vb, idx, t = (int(v) for v in items[row])
        (off_a, depth, hs, ws), off_b = (int(v) for v in vols[va]), int(vols[vb][0])
        src_a = pool[off_a:off_a + depth * hs * ws].reshape(depth, hs, ws)
        src_b = pool[off_b:off_b + depth * hs * ws].reshape(depth, hs, ws)
        a[i:i + 1], slice_idx[i:i + 1] = R.assemble(src_a, idx, 1, k, None if t == -1 else t, h, w, lo, hi)
        b[i:i + 1] = R.assemble(src_b, idx, 1, 1, None, h, w, lo, hi)[0]
    return a, b, slice_idx


def invalid_rows(vols):
    """{kind: table row} -- one invalid row of each kind, every one of them placed in the MIDDLE
    subject of the pool (volumes 2 and 3), so that a missing guard reads other volumes' voxels, not memory outside the pool."""
    depth = int(vols[2][1])
    return {
        'vol_a_negative': (-1, 3, 4, 2),
        'vol_a_past_the_table': (len(vols), 3, 4, 2),
        'vol_b_negative': (2, -1, 4, 2),
        'vol_b_past_the_table': (2, len(vols), 4, 2),
        'shapes_differ': (2, 1, 4, 2),                      # subject 1's input with subject 0's target
        'idx_negative': (2, 3, -1, 2),
        'idx_at_depth': (2, 3, depth, 2),
        'thickness_zero': (2, 3, 4, 0),
        'thickness_negative_k4': (2, 3, 4, -1),             # valid with k = 1
    }


def bad_descriptors(vols, pool_elems):
    """{kind: edited copy of the volume table}: volume 3 (the middle subject's target) made unusable; every item that names it turns NaN."""
    out = {}
    for kind, (col, value) in {'depth_zero': (1, 0), 'hs_negative': (2, -4), 'ws_zero': (3, 0), 'offset_negative': (0, -1),
                               'runs_past_the_pool': (0, pool_elems - int(np.prod(vols[3][1:])) + 1)}.items():
        v = vols.copy()
        v[3, col] = value
        out[kind] = v
    return out
