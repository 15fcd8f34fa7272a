"""Geometric augmentation without a GPU, exact equality throughout: the numpy restatement of the augmenting gather (tests/augment_ref.py) against the
golden captured from the reference's RandomFlip / RandomRotate90 / RandomRotate classes (tests/golden/A1_augment.npz, tools/gen_golden_augment.py),
against ``scipy.ndimage.rotate``, ``np.flip`` and ``np.rot90``; ``afcm_amd.augment`` (``apply_host``, ``augment_rows``, ``AugmentConfig``) and the
host side of ``DeviceSliceSet(augment=...)``.  tests/test_gpu_augment.py holds the kernel to ``host_batch(..., augment=...)``."""
import numpy as np
import pytest
import torch
from scipy import ndimage

import augment_ref as R
import train_batch_ref as T
from afcm_amd import augment as A
from conftest import load_golden


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _plane(h, w, seed=0, c=1):
    return np.random.default_rng(seed).standard_normal((c, h, w)).astype(np.float32)


def test_restatement_equals_the_reference_classes():
    g = load_golden('A1_augment')
    for name, hw in (('sq', (16, 16)), ('ob', (12, 20))):
        x, params, want = g[f'{name}_x'], g[f'{name}_params'], g[f'{name}_out']
        assert x.shape == (1,) + hw and want.shape == (len(params), 1) + hw and len(params) >= 25
        assert {tuple(p[:3]) for p in params.tolist()} >= {(fh, fw, k) for fh in (0, 1) for fw in (0, 1) for k in ((0, 1, 2, 3) if name == 'sq' else (0, 2))}
        assert params[:, 3].min() == -45 and params[:, 3].max() == 44 and (params[:, 3] == 0).any()
        for (fh, fw, k, angle), w in zip(params.tolist(), want):
            row = A.make_rows(fh, fw, k, angle, hw)[0]
            assert np.array_equal(_bits(R.augment_planes(x, row)), _bits(w)), (name, fh, fw, k, angle)
            assert np.array_equal(_bits(A.apply_host(x, row)), _bits(w)), (name, fh, fw, k, angle)


@pytest.mark.parametrize('hw', [(16, 16), (5, 7), (37, 53), (2, 40)])
def test_rotation_equals_scipy_at_every_angle_of_the_spectrum(hw):
    x = _plane(*hw, seed=hw[0])
    differing = 0
    for angle in list(range(-45, 45)) + ([90] if hw == (2, 40) else []):       # 2 x 40 at 90 degrees reflects through ten periods
        want = ndimage.rotate(x, angle, axes=(2, 1), reshape=False, order=0, mode='reflect', cval=-1)
        row = A.make_rows(0, 0, 0, angle, hw)[0]
        assert R.row_valid(row, *hw)
        got = R.augment_planes(x, row)
        differing += int((_bits(got) != _bits(want)).sum())
    assert differing == 0
    if hw == (2, 40):
        sy, _ = R.source_index(A.make_rows(0, 0, 0, 90, hw)[0], *hw)
        raw = np.floor((np.arange(40) * 1.0) + A.rotation(90, hw)[2] + 0.5)    # iy along a row at 90 degrees: x + off_y
        assert raw.min() <= -19 and raw.max() >= 20 and set(np.unique(sy)) == {0, 1}


def test_angle_zero_is_the_identity_exactly():
    assert A.rotation(0, (12, 18)) == (1.0, 0.0, 0.0, 0.0)
    assert np.array_equal(A.make_rows(0, 0, 0, 0, (12, 18)), A.identity_rows(1))
    sy, sx = R.source_index(A.identity_rows(1)[0], 12, 18)
    yy, xx = np.meshgrid(np.arange(12), np.arange(18), indexing='ij')
    assert np.array_equal(sy, yy) and np.array_equal(sx, xx)


def test_flips_and_quarter_turns_equal_numpy():
    x = _plane(16, 16, seed=4, c=3)
    for fh in (0, 1):
        for fw in (0, 1):
            for k in range(4):
                want = x
                if fh:
                    want = np.flip(want, 1)
                if fw:
                    want = np.flip(want, 2)
                want = np.rot90(want, k, (1, 2))
                got = R.augment_planes(x, A.make_rows(fh, fw, k, 0, (16, 16))[0])
                assert np.array_equal(_bits(got), _bits(want)), (fh, fw, k)
    ob = _plane(12, 18, seed=5)
    assert np.array_equal(R.augment_planes(ob, A.make_rows(1, 1, 2, 0, (12, 18))[0]), np.rot90(np.flip(np.flip(ob, 1), 2), 2, (1, 2)))
    assert not R.row_valid(A.make_rows(0, 0, 1, 0, (12, 18))[0], 12, 18) and R.row_valid(A.make_rows(0, 0, 1, 0, (12, 12))[0], 12, 12)


def test_apply_host_equals_the_chained_restatement():
    rng = np.random.default_rng(8)
    for hw, ks in (((16, 16), (0, 1, 2, 3)), ((12, 18), (0, 2)), ((2, 40), (0, 2))):
        x = _plane(*hw, seed=9, c=4)
        for _ in range(24):
            row = A.make_rows(rng.integers(0, 2), rng.integers(0, 2), rng.choice(ks), rng.integers(-45, 45), hw)[0]
            want = R.augment_planes(x, row)
            got = A.apply_host(x, row)
            assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.flags.c_contiguous
            assert np.array_equal(_bits(got), _bits(want)), row
            t = A.apply_host(torch.from_numpy(x), row)
            assert isinstance(t, torch.Tensor) and np.array_equal(_bits(t.numpy()), _bits(want))
    x = _plane(16, 16)
    with pytest.raises(RuntimeError, match='must be \\[C, H, W\\]'):
        A.apply_host(x[0], A.identity_rows(1)[0])
    with pytest.raises(RuntimeError, match='flips are 0 or 1'):
        A.apply_host(x, np.array([2., 0, 0, 0, 1, 0, 0, 0]))
    with pytest.raises(RuntimeError, match='needs square planes'):
        A.apply_host(_plane(12, 18), A.make_rows(0, 0, 1, 0, (12, 12))[0])
    with pytest.raises(RuntimeError, match='are not those of angle 10'):
        A.apply_host(x, np.array([0., 0, 0, 10, 1, 0, 0, 0]))


def test_augment_rows_ranges_and_draw_order():
    cfg = A.AugmentConfig(flip_axes=(1, 2), rotate90=True, angle_spectrum=45)
    rows = A.augment_rows(cfg, 4000, (16, 16), np.random.default_rng(1))
    assert rows.dtype == np.float64 and rows.shape == (4000, 8)
    assert set(rows[:, 0]) == {0., 1.} and set(rows[:, 1]) == {0., 1.} and set(rows[:, 2]) == {0., 1., 2., 3.}
    assert set(rows[:, 3]) == set(float(a) for a in range(-45, 45))                        # -S inclusive, S exclusive: RandomState.randint(-S, S)
    assert 0.45 < rows[:, 0].mean() < 0.55 and 0.45 < rows[:, 1].mean() < 0.55
    assert all(R.row_valid(r, 16, 16) for r in rows[:200])
    for r in rows[:50]:
        assert tuple(r[4:]) == A.rotation(int(r[3]), (16, 16))
    zero = rows[rows[:, 3] == 0]
    assert len(zero) and (zero[:, 4:] == [1., 0., 0., 0.]).all()
    # the fixed order: the flips ([n, axes] in one draw), then the ks, then the angles
    rng = np.random.default_rng(1)
    flips, k, angle = rng.uniform(size=(4000, 2)) > 0.5, rng.integers(0, 4, 4000), rng.integers(-45, 45, 4000)
    assert np.array_equal(rows[:, 0], flips[:, 0]) and np.array_equal(rows[:, 1], flips[:, 1])
    assert np.array_equal(rows[:, 2], k) and np.array_equal(rows[:, 3], angle)
    # a transform that is off draws nothing and leaves its columns at the identity
    rng = np.random.default_rng(2)
    only_w = A.augment_rows(A.AugmentConfig(flip_axes=(2,)), 64, (12, 18), rng)
    again = np.random.default_rng(2)
    assert np.array_equal(only_w[:, 1], again.uniform(size=(64, 1))[:, 0] > 0.5) and rng.integers(1 << 30) == again.integers(1 << 30)
    assert not only_w[:, 0].any() and not only_w[:, 2:4].any() and (only_w[:, 4:] == [1., 0., 0., 0.]).all()
    nothing = A.augment_rows(A.AugmentConfig(), 5, (12, 18), np.random.default_rng(0))
    assert np.array_equal(nothing, A.identity_rows(5))
    with pytest.raises(RuntimeError, match='rotate90 needs a square patch'):
        A.augment_rows(cfg, 4, (12, 18), np.random.default_rng(0))
    with pytest.raises(RuntimeError, match='numpy.random.Generator'):
        A.augment_rows(cfg, 4, (16, 16), 3)


def test_config_refusals():
    for bad in ((0,), (1, 1), (3,), ('1',), (True,)):
        with pytest.raises(RuntimeError, match='flip_axes must be'):
            A.AugmentConfig(flip_axes=bad)
    for bad in (0, -5, 4.5, True):
        with pytest.raises(RuntimeError, match='angle_spectrum must be'):
            A.AugmentConfig(angle_spectrum=bad)
    with pytest.raises(RuntimeError, match='rotate90 must be a bool'):
        A.AugmentConfig(rotate90=1)
    assert A.AugmentConfig(flip_axes=[2, 1], angle_spectrum=np.int64(30)) == A.AugmentConfig(flip_axes=(2, 1), angle_spectrum=30)


def _host_set(**kw):
    from afcm_amd.training import DeviceSliceSet
    kw.setdefault('patch_shape', (1, 16, 16))
    return DeviceSliceSet(T.subjects(np.uint8), raw_internal_path_in=['t1'], raw_internal_path_out=['t2'], thickness=T.THICKNESSES, device=None, **kw)


def test_device_slice_set_host_side():
    cfg = A.AugmentConfig(flip_axes=(1, 2), rotate90=True, angle_spectrum=45)
    plain, ds = _host_set(), _host_set(augment=cfg)
    # a set with augmentation draws the item table it drew before, and the parameter rows after it on the same generator
    assert np.array_equal(ds.epoch_items(3), plain.epoch_items(3)) and np.array_equal(plain.epoch_items(3), T_EPOCH_3)
    rng, ref = np.random.default_rng(3), np.random.default_rng(3)
    items, rows = ds.epoch_items(rng), ds.epoch_augment(rng)
    plain.epoch_items(ref)
    assert rows.shape == (23, 8) and np.array_equal(rows, A.augment_rows(cfg, 23, (16, 16), ref))
    assert ds.epoch_augment(5, rows=7).shape == (7, 8)
    # host_batch applies row first + j to A and B of item first + j
    base = ds.host_batch(items, 5, 4)
    got = ds.host_batch(items, 5, 4, augment=rows)
    for j in range(4):
        assert np.array_equal(_bits(got[0][j].numpy()), _bits(R.augment_planes(base[0][j].numpy(), rows[5 + j])))
        assert np.array_equal(_bits(got[1][j].numpy()), _bits(R.augment_planes(base[1][j].numpy(), rows[5 + j])))
    assert torch.equal(got[2], base[2]) and not torch.equal(got[0], base[0])
    same = ds.host_batch(items, 5, 4, augment=A.identity_rows(23))
    assert all(torch.equal(a, b) for a, b in zip(same, base))
    with pytest.raises(RuntimeError, match=r'float64 \[23, 8\]'):
        ds.host_batch(items, 5, 4, augment=rows[:22])
    with pytest.raises(RuntimeError, match=r'float64 \[23, 8\]'):
        ds.host_batch(items, 5, 4, augment=rows.astype(np.float32))
    with pytest.raises(RuntimeError, match='built without augment'):
        plain.host_batch(items, 5, 4, augment=rows)
    with pytest.raises(RuntimeError, match='built without augment'):
        plain.epoch_augment(3)
    with pytest.raises(RuntimeError, match="belongs to the 'train' phase"):
        _host_set(augment=cfg, phase='val')
    with pytest.raises(RuntimeError, match='rotate90 needs a square patch'):
        _host_set(augment=cfg, patch_shape=(1, 12, 18))
    with pytest.raises(RuntimeError, match='must be an AugmentConfig'):
        _host_set(augment=dict(rotate90=True))
    with pytest.raises(RuntimeError, match='device=None'):
        ds.load_epoch(items, rows)
    assert _host_set(augment=A.AugmentConfig(flip_axes=(1,), angle_spectrum=45), patch_shape=(1, 12, 18)).epoch_augment(0).shape == (23, 8)


def test_augment_kernels_use_no_scratch_and_no_lds():
    """Code-object metadata of the built batch.o, as tests/test_train_batch_ref_cpu.py reads it for the plain kernel: every (source, output) instance
    of the augmenting kernel, without scratch, spills or LDS, and the plain kernel's twelve beside them."""
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
    kernels = [k for k in found if 'batch_augment_kernel' in k['name']]
    assert len(kernels) == 4 * 3 and len([k for k in found if 'batch_assemble_kernel' in k['name']]) == 4 * 3, [k['name'] for k in found]
    for k in kernels:
        assert k.get('scratch', 0) == 0 and k.get('vgpr_spill', 0) == 0 and k.get('sgpr_spill', 0) == 0 and k.get('lds', 0) == 0, k
        assert k.get('vgpr', 0) <= 64, k


# DeviceSliceSet.epoch_items(3) of the 23 slices of train_batch_ref's subjects with its thicknesses, as the code before augmentation returned it
T_EPOCH_3 = np.array([
    (2, 3, 2, 3), (2, 3, 10, 2), (2, 3, 5, 5), (4, 5, 0, 5), (0, 1, 0, 5), (2, 3, 8, 5),
    (0, 1, 3, 2), (4, 5, 2, 2), (2, 3, 1, 3), (2, 3, 6, 3), (0, 1, 6, 5), (0, 1, 1, 5),
    (2, 3, 3, 2), (0, 1, 2, 5), (2, 3, 4, 2), (4, 5, 4, 2), (2, 3, 9, 5), (2, 3, 7, 5),
    (0, 1, 4, 2), (2, 3, 0, 2), (0, 1, 5, 2), (4, 5, 3, 2), (4, 5, 1, 5),
], dtype=np.int32)
