"""The 7 x 7 x 7 volume SSIM without a GPU: the numpy reference of the layer sums (tests/volume_ssim_ref.py) against itself in another axis order
and against ``evaluation.structural_similarity`` (scipy's uniform_filter), the host finisher ``evaluate_3D_from_stats`` against
``evaluation.evaluate_3D`` on float64 arrays, and the built kernels' resources.  tests/test_gpu_volume_ssim.py holds the kernel to the same reference."""
import os
import subprocess
import sys

import numpy as np
import pytest

import plane_metrics_ref as P
import volume_ssim_ref as R
from afcm_amd import evaluation as E

TOL_PSNR_DB, TOL_SSIM, TOL_MAE_REL = 1e-9, 1e-10, 2e-6      # the finishers' bounds of tests/test_gpu_volume.py
SHAPES = [(7, 7, 7), (8, 9, 10), (13, 23, 71), (9, 70, 135)]
PAIRS = {'noise': R.noise_pair, 'blob': R.blob_pair}


@pytest.mark.parametrize('kind', sorted(PAIRS))
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_reference_in_two_axis_orders_and_against_uniform_filter(shape, kind):
    ref, test = (a.astype(np.float64) for a in PAIRS[kind](shape, seed=sum(shape)))
    if kind == 'blob' and min(shape) > 7:
        assert (ref == 0).any() and (ref > 0).any()          # an exactly-zero background and a body
    a, b = R.layer_sums(ref, test, (0, 1, 2)), R.layer_sums(ref, test, (2, 1, 0))
    assert a.shape == (shape[0] - 6,) and np.isfinite(a).all()
    rel = np.abs(a - b) / np.abs(a)
    nwin = (shape[0] - 6) * (shape[1] - 6) * (shape[2] - 6)
    got, want = a.sum() / nwin, E.structural_similarity(ref, test)
    print(f'{shape} {kind}: orders differ by {rel.max():.2e} relative; mean {got!r} against uniform_filter {want!r}: {abs(got - want) / abs(want):.2e} relative')
    assert (rel <= 1e-12).all()
    assert abs(got - want) <= 1e-12 * abs(want)


def _from_stats(pred, target):
    return E.evaluate_3D_from_stats(P.table(target, pred), R.layer_sums(target, pred), target.shape)


@pytest.mark.parametrize('kind', sorted(PAIRS))
@pytest.mark.parametrize('shape', SHAPES[1:], ids=str)
def test_finisher_equals_evaluate_3D_on_float64_arrays(shape, kind):
    target, pred = (a.astype(np.float64) for a in PAIRS[kind](shape, seed=3))
    got, want = _from_stats(pred, target), E.evaluate_3D(pred, target)
    print(got, want)
    assert abs(got[0] - want[0]) <= TOL_PSNR_DB and abs(got[1] - want[1]) <= TOL_SSIM and abs(got[2] - want[2]) <= TOL_MAE_REL * want[2]


def test_finisher_data_range_value_error_and_identical_volumes():
    target, pred = (a.astype(np.float64) for a in R.noise_pair((8, 9, 10), seed=5))
    signed_t, signed_p = target * 2 - 1, pred * 2 - 1                     # a target with negative values: data range 2, 6.02 dB more
    assert signed_t.min() < 0
    got, want = _from_stats(signed_p, signed_t), E.evaluate_3D(signed_p, signed_t)
    assert abs(got[0] - want[0]) <= TOL_PSNR_DB and abs(got[1] - want[1]) <= TOL_SSIM and abs(got[2] - want[2]) <= TOL_MAE_REL * want[2]
    one = _from_stats(pred, target)
    assert abs(_from_stats(pred * 2, target)[0] - E.evaluate_3D(pred * 2, target)[0]) <= TOL_PSNR_DB      # the PREDICTION may leave [-1, 1]
    assert one[0] == pytest.approx(E.evaluate_3D(pred, target)[0], abs=TOL_PSNR_DB)
    for bad in (target * 1.5, target - 1.5):                              # the target leaves [-1, 1]: both raise the same error
        with pytest.raises(ValueError, match='outside the range expected'):
            E.evaluate_3D(pred, bad)
        with pytest.raises(ValueError, match='outside the range expected'):
            _from_stats(pred, bad)
    same = _from_stats(target, target)
    assert same[0] == float('inf') == E.evaluate_3D(target, target)[0]
    assert abs(same[1] - 1.0) <= TOL_SSIM and same[2] == 0.0
    with pytest.raises(ValueError, match='layer sums'):                   # a table and layer sums that do not belong to the shape
        E.evaluate_3D_from_stats(P.table(target, pred), np.zeros(3), target.shape)
    with pytest.raises(ValueError, match='layer sums'):
        E.evaluate_3D_from_stats(P.table(target, pred)[:-1], R.layer_sums(target, pred), target.shape)


def test_ops_refuse_cpu_tensors_and_shape_mismatch_before_loading_anything():
    import torch
    from afcm_amd import evaluation_device
    from afcm_amd.torch_utils.ops import volume_metrics
    assert (volume_metrics.TILE_Y, volume_metrics.TILE_X) == (16, 64)
    x = torch.zeros(8, 9, 10)
    with pytest.raises(RuntimeError, match='no CPU'):
        volume_metrics.volume_ssim_layers(x[None], x[None])
    with pytest.raises(RuntimeError, match='no CPU'):
        evaluation_device.evaluate_3D(x, x)
    with pytest.raises(RuntimeError, match='one shape'):
        evaluation_device.evaluate_3D(x, x[:7])


def test_volume_ssim_kernels_use_no_scratch():
    """Code-object metadata of the built metrics.o: the two new kernels without scratch or spills, the staged z-sums within the 64 KB of static LDS
    (DESIGN section 8h quotes the registers).  The object is a build product; a tree that has the library but not the object compiles this one file."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, 'afcm_amd', 'csrc')
    if not os.path.exists(os.path.join(csrc, 'metrics.o')):
        subprocess.check_call(['make', '-C', csrc, 'metrics.o'])
    sys.path.insert(0, os.path.join(root, 'tools'))
    from kernel_resources import kernel_resources
    kernels = {k['name'].split('(')[0].split('::')[-1]: k for k in kernel_resources(os.path.join(csrc, 'metrics.o')) if 'volume_ssim' in k['name']}
    assert sorted(kernels) == ['volume_ssim_finish_kernel', 'volume_ssim_kernel'], sorted(kernels)
    for k in kernels.values():
        assert k.get('scratch', 0) == 0 and k.get('vgpr_spill', 0) == 0 and k.get('sgpr_spill', 0) == 0, k
    # 5 x 22 x 70 float64 z-sums + four wave partials; two workgroups per CU need <= 80 KB each and <= 128 VGPRs at 256 threads
    assert kernels['volume_ssim_kernel']['lds'] == 5 * 22 * 70 * 8 + 4 * 8 and kernels['volume_ssim_kernel']['vgpr'] <= 128, kernels['volume_ssim_kernel']
    assert kernels['volume_ssim_finish_kernel'].get('lds', 0) == 0
