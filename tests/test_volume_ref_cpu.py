"""Whole-volume inference without a GPU: the numpy restatement of the two kernels (tests/volume_ref.py) against the host code they stand in for
(``SlidingWindowPredictor.predict``, ``SliceDataset(phase='test')``), bit for bit; the host-side plan; ``predict_volume(where='host')`` on a CPU stub
step against a hand-rolled loop.  The GPU tests (tests/test_gpu_volume.py) hold the kernels to the same host code on the same cases."""
import warnings

import numpy as np
import pytest
import torch

import volume_ref as R
from afcm_amd.data import SliceDataset
from afcm_amd.predictor import SlidingWindowPredictor, patch_indices


def _host_predict(volume_shape, patch_shape, stride_shape, halo, batch, predictions, prediction_channel):
    idx = patch_indices(volume_shape, patch_shape, stride_shape)
    p = SlidingWindowPredictor(out_channels=predictions.shape[1], patch_halo=halo, prediction_channel=prediction_channel)
    with warnings.catch_warnings(), np.errstate(divide='ignore', invalid='ignore'):
        warnings.simplefilter('ignore', RuntimeWarning)
        return p.predict(volume_shape, ((predictions[i:i + batch], idx[i:i + batch]) for i in range(0, len(idx), batch)))


@pytest.mark.parametrize('name', sorted(R.ACCUMULATOR_CASES))
def test_gather_reference_equals_the_host_predictor(name):
    volume_shape, patch_shape, stride_shape, halo, batch, channels, pc = R.ACCUMULATOR_CASES[name]
    origins = R.origins(volume_shape, patch_shape, stride_shape)
    assert [tuple(o) for o in origins] == [tuple(s.start for s in ix) for ix in patch_indices(volume_shape, patch_shape, stride_shape)]
    predictions = R.random_predictions(len(origins), channels, patch_shape, seed=11)
    want = _host_predict(volume_shape, patch_shape, stride_shape, halo, batch, predictions, pc)
    got, _, mask = R.predict(volume_shape, origins, predictions, batch, halo, pc)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got, want, equal_nan=True)
    if name == 'a_ragged_d1':
        assert len(origins) == 100 and len(origins) % batch != 0 and origins[:, 2].max() == 28
        assert set(np.unique(mask)) == {1, 2}
    if name == 'c_broadcast_quirk':                         # the zero halo on interior z sides distorts the volume: not what halo (2, 4, 4) gives
        b = R.ACCUMULATOR_CASES['b_deep']
        assert not np.array_equal(got, R.predict(b[0], origins, predictions, batch, b[3], None)[0], equal_nan=True)
    if name == 'e_mask_wraps':
        assert len(origins) == 289
        assert int((mask == 0).sum()) == 4 and np.isinf(got[mask == 0]).all()        # 256 visits wrap to 0: the quotient is +-inf


def test_gather_reference_takes_16bit_predictions_exactly():
    volume_shape, patch_shape, stride_shape, halo, batch, channels, pc = R.ACCUMULATOR_CASES['b_deep']
    origins = R.origins(volume_shape, patch_shape, stride_shape)
    half = R.random_predictions(len(origins), channels, patch_shape, seed=12).astype(np.float16)
    want = _host_predict(volume_shape, patch_shape, stride_shape, halo, batch, half, pc)
    assert np.array_equal(R.predict(volume_shape, origins, half, batch, halo, pc)[0], want, equal_nan=True)


def _dataset_items(src, hw, thickness, slice_num, lo, hi):
    ds = SliceDataset({'raw': src}, phase='test', patch_shape=(1,) + hw, stride_shape=(1, 8, 8), thickness=[] if thickness is None else [thickness],
                      slice_num=slice_num, min_value=lo, max_value=hi)
    items = [ds[i] for i in range(len(ds))]
    return torch.stack([it[0] for it in items]).numpy(), torch.stack([it[1] for it in items]).numpy()


@pytest.mark.parametrize('name', sorted(R.ASSEMBLY_CASES))
def test_assembly_reference_equals_the_slice_dataset(name):
    shape, dtype, hw, thickness, slice_num, (lo, hi) = R.ASSEMBLY_CASES[name]
    src = R.source(shape, dtype)
    want_a, want_idx = _dataset_items(src, hw, thickness, slice_num, lo, hi)
    got_a, got_idx = R.assemble(src, 0, shape[0], slice_num, thickness, hw[0], hw[1], lo, hi)
    assert got_a.dtype == want_a.dtype == np.float32 and got_a.shape == want_a.shape == (shape[0], slice_num) + hw
    assert np.array_equal(got_a.view(np.uint32), want_a.view(np.uint32))                 # bit for bit (the sign of a zero included)
    assert np.array_equal(got_idx.view(np.uint32), want_idx.view(np.uint32))
    if slice_num == 4:                                     # zero planes at both ends (depth 23, thickness 5: targets 0-4 lack the slice before,
        before, after = R.zero_plane_targets(shape[0], thickness)          # 15-22 the second after)
        assert shape[0] != 23 or (before, after) == (list(range(5)), list(range(15, 23)))
        pad_value = np.float32(np.clip(2 * ((0.0 - lo) / (hi - lo)) - 1, -1, 1))
        assert (got_a[before, 0] == pad_value).all() and (got_a[after, 3] == pad_value).all() and not (got_a[len(before):, 0] == pad_value).all()
        if lo != 0.0:
            assert pad_value != -1
    # a run in the middle and one that ends at the last slice are the same rows
    for first, count in ((shape[0] // 3, 4), (shape[0] - 3, 3)):
        part_a, part_idx = R.assemble(src, first, count, slice_num, thickness, hw[0], hw[1], lo, hi)
        assert np.array_equal(part_a, got_a[first:first + count]) and np.array_equal(part_idx, got_idx[first:first + count])


def test_plan_origins_and_bounding_boxes():
    from afcm_amd.volume import PatchPlan
    volume_shape, patch_shape, stride_shape = (12, 40, 44), (8, 16, 16), (4, 8, 8)
    idx = patch_indices(volume_shape, patch_shape, stride_shape)
    plan = PatchPlan(volume_shape, idx)
    assert len(plan) == len(idx) == 2 * 4 * 5 and plan.patch_shape == patch_shape
    assert plan.origins.dtype == np.int32 and np.array_equal(plan.origins, R.origins(volume_shape, patch_shape, stride_shape))
    assert plan.bounding_box(0, 1) == ((0, 8), (0, 16), (0, 16))
    assert plan.bounding_box(3, 3) == ((0, 8), (0, 24), (0, 44))          # x origins 24, 28 of row 0 and 0 of row 1
    assert plan.bounding_box(len(idx) - 1, 1) == ((4, 12), (24, 40), (28, 44))
    assert plan.bounding_box(0, len(idx)) == ((0, 12), (0, 40), (0, 44))
    for first, count in ((-1, 2), (0, 0), (len(idx) - 1, 2)):
        with pytest.raises(RuntimeError, match='not inside a plan'):
            plan.bounding_box(first, count)


def test_plan_and_predictor_argument_errors():
    from afcm_amd.torch_utils.ops.volume_ops import assemble_slices, halo_accumulate
    from afcm_amd.volume import DevicePredictor, PatchPlan
    good = (slice(0, 4), slice(0, 8), slice(0, 8))
    with pytest.raises(RuntimeError, match='not inside the volume'):      # patch outside the volume
        PatchPlan((6, 16, 16), [good, (slice(4, 8), slice(0, 8), slice(0, 8))])
    with pytest.raises(RuntimeError, match='not inside the volume'):
        PatchPlan((6, 16, 16), [(slice(-1, 3), slice(0, 8), slice(0, 8))])
    with pytest.raises(RuntimeError, match='the first patch has'):
        PatchPlan((6, 16, 16), [good, (slice(0, 4), slice(0, 8), slice(0, 7))])
    with pytest.raises(RuntimeError, match='no patches'):
        PatchPlan((6, 16, 16), [])
    with pytest.raises(RuntimeError, match='non-negative'):               # negative halo
        DevicePredictor(patch_halo=(0, -1, 0))
    with pytest.raises(RuntimeError, match='ROCm device'):
        DevicePredictor().allocate((6, 16, 16), 'cpu')
    p = DevicePredictor(patch_halo=(2, 4, 4))
    p.volume_shape = (12, 40, 44)                                         # (allocate needs a device; the plan is host arithmetic)
    with pytest.raises(AssertionError, match='Not enough patch overlap'): # overlap smaller than the halo, via validate_halo
        p.plan((8, 16, 16), (7, 8, 8))
    assert len(p.plan((8, 16, 16), (4, 8, 8))) == 40
    # the ops refuse host tensors and the geometry the kernel does not implement before anything is launched
    with pytest.raises(RuntimeError, match='no CPU'):
        assemble_slices(torch.zeros(4, 8, 8, dtype=torch.uint8), 0, 2, (1, 8, 8), thickness=2)
    with pytest.raises(RuntimeError, match='patch depth 2'):
        assemble_slices(torch.zeros(4, 8, 8, dtype=torch.uint8), 0, 2, (2, 8, 8), thickness=2)
    with pytest.raises(RuntimeError, match='z stride 2'):
        assemble_slices(torch.zeros(4, 8, 8, dtype=torch.uint8), 0, 2, (1, 8, 8), thickness=2, stride_shape=(2, 8, 8))
    with pytest.raises(RuntimeError, match='needs a thickness'):
        assemble_slices(torch.zeros(4, 8, 8, dtype=torch.uint8), 0, 2, (1, 8, 8))
    with pytest.raises(RuntimeError, match='no CPU'):
        halo_accumulate(torch.zeros(1, 4, 8, 8), torch.zeros(1, 4, 8, 8, dtype=torch.uint8), torch.zeros(1, 1, 1, 8, 8),
                        torch.zeros(4, 3, dtype=torch.int32), 0, (0, 0, 0))


class CpuStubStep:
    """``fake_B`` is a fixed function of ``real_A`` and ``gen_c``; ``gen_z`` is drawn as the real step draws it (and recorded)."""

    def __init__(self):
        self.draws = []

    def set_test_input(self, real_A, slice_idx):
        self.real_A, self.gen_c = real_A, slice_idx
        self.gen_z = torch.randn([real_A.shape[0], 8])
        self.draws.append(self.gen_z)

    def test(self):
        self.fake_B = self.real_A[:, 0:1] * 0.5 - self.real_A[:, 2:3] * 0.25 + self.gen_c[:, :, None, None] + 0.125 * self.gen_z[:, :1, None, None]


def test_predict_volume_host_arm_is_the_hand_rolled_loop():
    from afcm_amd.volume import predict_volume
    src = R.source((11, 30, 40), np.uint8, seed=8)
    kw = dict(raw_internal_path_in='raw', thickness=5, patch_hw=(32, 32), batch_size=4, patch_halo=(0, 4, 4), heads=('prediction', 'input'))
    torch.manual_seed(4)
    step = CpuStubStep()
    got = predict_volume(step, {'raw': src}, where='host', **kw)
    assert [tuple(z.shape) for z in step.draws] == [(4, 8), (4, 8), (3, 8)]         # three batches, the last one ragged

    torch.manual_seed(4)
    ds = SliceDataset({'raw': src}, phase='test', patch_shape=(1, 32, 32), stride_shape=(1, 1, 1), thickness=[5], slice_num=4)
    want = {h: (np.zeros((1, 11, 32, 32), np.float32), np.zeros((1, 11, 32, 32), np.uint8)) for h in kw['heads']}
    p = SlidingWindowPredictor(out_channels=1, patch_halo=(0, 4, 4))
    hand = CpuStubStep()
    for first in range(0, 11, 4):
        items = [ds[i] for i in range(first, min(first + 4, 11))]
        hand.set_test_input(torch.stack([it[0] for it in items]), torch.stack([it[1] for it in items]))
        hand.test()
        p.accumulate(*want['prediction'], hand.fake_B.unsqueeze(2), [it[2] for it in items], (11, 32, 32))
        p.accumulate(*want['input'], hand.real_A[:, 1:2].unsqueeze(2), [it[2] for it in items], (11, 32, 32))
    for h in kw['heads']:
        assert got[h].shape == (1, 11, 32, 32) and got[h].dtype == torch.float32
        assert np.array_equal(got[h].numpy(), want[h][0] / want[h][1], equal_nan=True)
    # every voxel is visited once (one patch per slice), so the input head is the loader's own channel 1
    assert np.array_equal(got['input'].numpy()[0], R.assemble(src, 0, 11, 4, 5, 32, 32)[0][:, 1])
    with pytest.raises(ValueError):
        predict_volume(step, {'raw': src}, where='nowhere', **kw)
    with pytest.raises(AssertionError, match='Not enough patch overlap'):
        predict_volume(step, {'raw': src}, where='host', **dict(kw, patch_halo=(1, 4, 4)))


def test_volume_kernels_use_no_scratch_and_no_lds():
    """Code-object metadata of the built volume.o: both kernels, every dtype instance, without scratch, spills or LDS (DESIGN section 8g quotes the
    registers).  ``slice_assemble_kernel`` produces 16 output bytes per thread, as ``batch_assemble_kernel`` does, and is held to the same bound:
    64 VGPRs, the largest allocation that still gives 8 waves per SIMD (min(8, 512 / allocation)): the occupancy bound, not a measured need.
    ``halo_accumulate_kernel`` keeps its 32.  The object is a build product; a tree that has the library but not the object compiles this one file."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, 'afcm_amd', 'csrc')
    if not os.path.exists(os.path.join(csrc, 'volume.o')):
        subprocess.check_call(['make', '-C', csrc, 'volume.o'])
    sys.path.insert(0, os.path.join(root, 'tools'))
    from kernel_resources import kernel_resources
    kernels = [k for k in kernel_resources(os.path.join(csrc, 'volume.o')) if 'slice_assemble_kernel' in k['name'] or 'halo_accumulate_kernel' in k['name']]
    assert len(kernels) == 4 * 3 + 3, [k['name'] for k in kernels]
    for k in kernels:
        assert k.get('scratch', 0) == 0 and k.get('vgpr_spill', 0) == 0 and k.get('sgpr_spill', 0) == 0 and k.get('lds', 0) == 0, k
        assert k.get('vgpr', 0) <= (64 if 'slice_assemble_kernel' in k['name'] else 32), k
