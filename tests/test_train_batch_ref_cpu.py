"""Training batches without a GPU: the numpy restatement of the batch kernel (tests/train_batch_ref.py) against stacked
``SliceDataset(phase='train', thickness=[t])`` items, bit for bit; its guards; the host side of ``DeviceSliceSet`` (epoch tables, refusals,
``host_batch``); the code-object resources of the built kernels.  tests/test_gpu_train_batch.py holds the kernel to the same items on the same cases."""
import numpy as np
import pytest
import torch

import train_batch_ref as T
from afcm_amd.data import SliceDataset


def dataset_items(volumes, items, hw, k, lo, hi):
    """The rows of ``items`` as the training loader builds them, stacked: (A, B, slice_idx [n, 1]) float32 numpy."""
    a, b, c = [], [], []
    for va, vb, idx, t in items.tolist():
        assert va // 2 == vb // 2
        ds = SliceDataset(volumes[va // 2], phase='train', patch_shape=(1,) + hw, stride_shape=(1, 1, 1), raw_internal_path_in=['t1'],
                          raw_internal_path_out=['t2'], thickness=[] if t == -1 else [t], slice_num=k, min_value=lo, max_value=hi)
        item = ds[idx]
        a.append(item['A'].numpy()), b.append(item['B'].numpy()), c.append(item['slice_idx'])
    return np.stack(a), np.stack(b), np.stack(c)


def _bits(x):
    return x.view(np.uint32)


@pytest.mark.parametrize('k, thickness', [(4, True), (1, True), (1, False)])
@pytest.mark.parametrize('hw', T.PATCHES)
@pytest.mark.parametrize('dtype', T.DTYPES)
def test_restatement_equals_the_training_loader(dtype, hw, k, thickness):
    lo, hi = T.value_range(dtype)
    volumes = T.subjects(dtype)
    pool, vols = T.pool_and_table(volumes, ('t1', 't2'))
    items = T.shuffled_items(k, thickness=thickness)
    assert len(items) == 23 and sorted(map(tuple, items[:, [0, 2]].tolist())) == [(2 * s, i) for s, sh in enumerate(T.SUBJECT_SHAPES) for i in range(sh[0])]
    want = dataset_items(volumes, items, hw, k, lo, hi)
    got = [np.concatenate(parts) for parts in zip(*(T.assemble_batch(pool, vols, items, first, min(T.BATCH, 23 - first), k, hw[0], hw[1], lo, hi)
                                                    for first in range(0, 23, T.BATCH)))]
    for g, w in zip(got, want):
        assert g.dtype == w.dtype == np.float32 and g.shape == w.shape
        assert np.array_equal(_bits(g), _bits(w))                                        # bit for bit, the sign of a zero included
    assert got[0].shape == (23, k) + hw and got[1].shape == (23, 1) + hw and got[2].shape == (23, 1)
    if k == 4 and hw == (16, 16):                          # out-of-volume planes at both ends (a third of the 92), and a thickness that spans a whole subject
        background = np.float32(np.clip(2 * ((0.0 - lo) / (hi - lo)) - 1, -1, 1))
        flat = (got[0] == background).all(axis=(2, 3))
        outside = np.array([[not 0 <= (i // t) * t + (p - 1) * t <= T.SUBJECT_SHAPES[va // 2][0] - 1 for p in range(4)] for va, _, i, t in items.tolist()])
        assert np.array_equal(flat, outside) and flat[:, 0].any() and flat[:, 3].any() and not flat[:, 1].any() and int(flat.sum()) > 20
        assert any(t >= T.SUBJECT_SHAPES[va // 2][0] for va, _, _, t in items.tolist())
    if not thickness:
        assert np.signbit(got[2]).all() and (got[2] == 0).all()                        # 0 / -1: the loader's -0.0
    # the cursor is an offset into the table
    part = T.assemble_batch(pool, vols, items, 2, 4, k, hw[0], hw[1], lo, hi, cursor=9)
    assert all(np.array_equal(_bits(p), _bits(w[11:15])) for p, w in zip(part, want))


def _poisoned(k):
    volumes = T.subjects(np.uint8)
    pool, vols = T.pool_and_table(volumes, ('t1', 't2'))
    items = T.shuffled_items(k)
    return pool, vols, items


def test_every_kind_of_invalid_row_is_a_nan_item_and_nothing_else_changes():
    pool, vols, items = _poisoned(4)
    clean = T.assemble_batch(pool, vols, items, 0, 23, 4, 16, 16)
    assert not any(np.isnan(c).any() for c in clean)
    kinds = T.invalid_rows(vols)
    table = items.copy()
    at = {kind: 1 + 2 * j for j, kind in enumerate(sorted(kinds))}                      # rows 1, 3, ..., 17: valid neighbours on both sides
    for kind, row in at.items():
        table[row] = kinds[kind]
    got = T.assemble_batch(pool, vols, table, 0, 23, 4, 16, 16)
    bad = sorted(at.values())
    for g, c in zip(got, clean):
        nan_items = np.isnan(g).reshape(23, -1)
        assert nan_items[bad].all() and not np.delete(nan_items, bad, axis=0).any()
        keep = np.setdiff1d(np.arange(23), bad)
        assert np.array_equal(_bits(g[keep]), _bits(c[keep]))
    # a negative thickness is the "no thickness" of k = 1, and valid there
    one = T.assemble_batch(pool, vols, table, 0, 23, 1, 16, 16)
    assert not np.isnan(one[0][at['thickness_negative_k4']]).any() and np.isnan(one[0][at['thickness_zero']]).all()
    # rows past the table, before it, and a cursor outside it
    tail = T.assemble_batch(pool, vols, items, 20, 5, 4, 16, 16)
    assert all(np.array_equal(_bits(t[:3]), _bits(c[20:])) and np.isnan(t[3:]).all() for t, c in zip(tail, clean))
    for cursor in (-1, 23, 1 << 40):
        assert all(np.isnan(t).all() for t in T.assemble_batch(pool, vols, items, 0, 2, 4, 16, 16, cursor=cursor))
    # an unusable descriptor takes out exactly the items that name it
    uses = (items[:, 0] == 3) | (items[:, 1] == 3)
    assert 0 < uses.sum() < 23
    for kind, edited in T.bad_descriptors(vols, pool.size).items():
        got = T.assemble_batch(pool, edited, items, 0, 23, 4, 16, 16)
        for g, c in zip(got, clean):
            assert np.isnan(g[uses]).all() and np.array_equal(_bits(g[~uses]), _bits(c[~uses])), kind


def _host_set(**kw):
    from afcm_amd.training import DeviceSliceSet
    kw.setdefault('raw_internal_path_in', ['t1'])
    kw.setdefault('raw_internal_path_out', ['t2'])
    kw.setdefault('patch_shape', (1, 16, 16))
    return DeviceSliceSet(kw.pop('sources', T.subjects(np.uint8)), device=None, **kw)


def test_epoch_items_train():
    ds = _host_set(thickness=T.THICKNESSES)
    assert len(ds) == 23 and ds.vols_host.dtype == np.int64
    pool, vols = T.pool_and_table(ds.volumes, ('t1', 't2'))
    assert np.array_equal(ds.vols_host, vols) and ds.pool_elems == pool.size
    items = ds.epoch_items(3)
    assert items.dtype == np.int32 and items.shape == (23, 4)
    serial = [(2 * s, 2 * s + 1, i) for s, sh in enumerate(T.SUBJECT_SHAPES) for i in range(sh[0])]
    assert sorted(map(tuple, items[:, :3].tolist())) == serial and list(map(tuple, items[:, :3].tolist())) != serial     # a permutation, shuffled
    assert set(items[:, 3].tolist()) <= set(T.THICKNESSES) and len(set(items[:, 3].tolist())) > 1
    assert np.array_equal(items, ds.epoch_items(3)) and np.array_equal(items, ds.epoch_items(np.random.default_rng(3)))
    assert not np.array_equal(items, ds.epoch_items(4))
    assert list(map(tuple, ds.epoch_items(3, shuffle=False)[:, :3].tolist())) == serial
    assert (_host_set(slice_num=1).epoch_items(0)[:, 3] == -1).all()                    # no thickness list: the loader's -1


def test_epoch_items_val_is_serial_and_rand_output_draws_output_modalities_only():
    ds = _host_set(phase='val', thickness=(5, 2), rand_output=True)
    items = ds.epoch_items(7)
    assert list(map(tuple, items.tolist())) == [(2 * s, 2 * s + 1, i, 5) for s, sh in enumerate(T.SUBJECT_SHAPES) for i in range(sh[0])]
    three = T.subjects(np.uint8, modalities=('t1', 't2', 'pd'))
    ds = _host_set(sources=three, thickness=(2,), rand_output=True, raw_internal_path_out=['t2', 'pd'])
    items = np.concatenate([ds.epoch_items(seed) for seed in range(4)])
    assert (items[:, 0] % 3 == 0).all() and set((items[:, 1] % 3).tolist()) == {1, 2} and (items[:, 0] // 3 == items[:, 1] // 3).all()
    fixed = _host_set(sources=three, thickness=(2,), raw_internal_path_out=['t2', 'pd']).epoch_items(0)
    assert (fixed[:, 1] % 3 == 2).all()                                                # without rand_output: the last output modality


def test_host_batch_is_the_stacked_loader_items():
    ds = _host_set(thickness=T.THICKNESSES)
    items = T.shuffled_items(4)
    want = dataset_items(ds.volumes, items[5:10], (16, 16), 4, 0., 255.)
    got = ds.host_batch(items, 5, 5)
    assert [tuple(g.shape) for g in got] == [(5, 4, 16, 16), (5, 1, 16, 16), (5, 1)]
    assert all(np.array_equal(_bits(g.numpy()), _bits(w)) for g, w in zip(got, want))
    with pytest.raises(RuntimeError, match='does not pair'):
        ds.host_batch(np.array([[2, 1, 0, 2]], dtype=np.int32), 0, 1)


def test_constructor_refusals():
    from afcm_amd.training import DeviceSliceSet
    mixed = T.subjects(np.uint8)
    mixed[1] = {m: v.astype(np.int16) for m, v in mixed[1].items()}
    with pytest.raises(RuntimeError, match='mixed source dtypes'):
        _host_set(sources=mixed, thickness=(2,))
    with pytest.raises(RuntimeError, match='no shipped configuration uses it'):
        _host_set(thickness=(2,), cat_inputs=True)
    crooked = T.subjects(np.uint8)
    crooked[2]['t2'] = crooked[2]['t2'][:, :-1]
    with pytest.raises(RuntimeError, match='subject 2: the input and output volumes must have one'):
        _host_set(sources=crooked, thickness=(2,))
    with pytest.raises(RuntimeError, match='slice number 4 needs one'):
        _host_set()
    with pytest.raises(RuntimeError, match=r'patch_shape must be \(1, H, W\)'):
        _host_set(thickness=(2,), patch_shape=(2, 16, 16))
    with pytest.raises(RuntimeError, match='uint8 / int16 / float32 / float64'):
        _host_set(sources=[{m: v.astype(np.int32) for m, v in s.items()} for s in T.subjects(np.uint8)], thickness=(2,))
    with pytest.raises(RuntimeError, match='ROCm device'):
        DeviceSliceSet(T.subjects(np.uint8), raw_internal_path_in=['t1'], raw_internal_path_out=['t2'], thickness=(2,), device='cpu')
    with pytest.raises(RuntimeError, match='device=None'):
        _host_set(thickness=(2,)).load_epoch(T.shuffled_items(4))


def test_ops_refuse_bad_arguments_before_any_launch():
    from afcm_amd.torch_utils.ops.batch_ops import advance_cursor, assemble_batch
    pool, vols, items = torch.zeros(64, dtype=torch.uint8), torch.zeros(1, 4, dtype=torch.int64), torch.zeros(2, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='no CPU'):
        assemble_batch(pool, vols, items, 0, 2, (4, 4))
    with pytest.raises(RuntimeError, match='slice number 3'):
        assemble_batch(pool, vols, items, 0, 2, (4, 4), slice_num=3)
    with pytest.raises(RuntimeError, match='volume table must be a contiguous torch.int64'):
        assemble_batch(pool, vols.int(), items, 0, 2, (4, 4))
    with pytest.raises(RuntimeError, match='item table must be a contiguous torch.int32'):
        assemble_batch(pool, vols, items[:, :3], 0, 2, (4, 4))
    with pytest.raises(RuntimeError, match='non-empty contiguous 1-D'):
        assemble_batch(pool.reshape(8, 8), vols, items, 0, 2, (4, 4))
    with pytest.raises(RuntimeError, match='source volumes are uint8'):
        assemble_batch(pool.int(), vols, items, 0, 2, (4, 4))
    with pytest.raises(RuntimeError, match='output dtype'):
        assemble_batch(pool, vols, items, 0, 2, (4, 4), dtype=torch.float64)
    with pytest.raises(RuntimeError, match='0 items from row 0'):
        assemble_batch(pool, vols, items, 0, 0, (4, 4))
    with pytest.raises(RuntimeError, match='2 items from row -1'):
        assemble_batch(pool, vols, items, -1, 2, (4, 4))
    with pytest.raises(RuntimeError, match='cursor must be an int64 tensor of one element'):
        assemble_batch(pool, vols, items, 0, 2, (4, 4), cursor=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match=r'out A must be a contiguous torch.float32 \(2, 4, 4, 4\)'):
        assemble_batch(pool, vols, items, 0, 2, (4, 4), out=(torch.zeros(2, 4, 4, 5), torch.zeros(2, 1, 4, 4), torch.zeros(2, 1)))
    with pytest.raises(RuntimeError, match='out B must be'):
        assemble_batch(pool, vols, items, 0, 2, (4, 4), out=(torch.zeros(2, 4, 4, 4), torch.zeros(2, 1, 4, 8)[..., ::2], torch.zeros(2, 1)))
    with pytest.raises(RuntimeError, match='out slice_idx must be'):
        assemble_batch(pool, vols, items, 0, 2, (4, 4), out=(torch.zeros(2, 4, 4, 4), torch.zeros(2, 1, 4, 4), torch.zeros(2, 1, dtype=torch.float64)))
    with pytest.raises(RuntimeError, match='cursor must be an int64'):
        advance_cursor(torch.zeros(2, dtype=torch.int64), 1)
    with pytest.raises(RuntimeError, match='no CPU'):
        advance_cursor(torch.zeros(1, dtype=torch.int64), 1)


def test_batch_kernels_use_no_scratch_and_no_lds():
    """Code-object metadata of the built batch.o: every (source, output) instance of the batch kernel and the cursor kernel, without scratch,
    spills or LDS (DESIGN section 8i quotes the registers).  The object is a build product; a tree that has the library but not the object compiles
    this one file."""
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
    kernels = [k for k in found if 'batch_assemble_kernel' in k['name'] or 'cursor_advance_kernel' in k['name']]
    assert len(kernels) == 4 * 3 + 1, [k['name'] for k in found]
    for k in kernels:
        assert k.get('scratch', 0) == 0 and k.get('vgpr_spill', 0) == 0 and k.get('sgpr_spill', 0) == 0 and k.get('lds', 0) == 0, k
        assert k.get('vgpr', 0) <= 64, k
