"""The device-side schedule without a GPU: the float64 restatement of the blur (tests/schedule_ref.py) against the golden captured from the
reference; ``DeviceSchedule.host_values`` against the reference's expressions; ``LRSchedule`` against torch's schedulers driven as train.py drives
them; the new entry points' refusals; the code-object resources of the built kernels.  tests/test_gpu_schedule.py holds the kernels to the same
restatements."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import schedule_ref as R
from afcm_amd.schedule import DeviceSchedule, LRSchedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    from afcm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_restatement_equals_the_reference_golden():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'U3_gauss61_filter2d.npz'))
    x, y, r, dx = (g[k] for k in ('x', 'y', 'r', 'dx'))
    assert x.shape == (1, 2, 72, 80)
    taps = R.reference_taps(10.0)
    assert taps.dtype == np.float32 and np.array_equal(taps, g['f'])            # the committed filter is the reference's sigma-10 taps, bit for bit
    assert np.abs(taps - taps[::-1]).max() <= 2.0 ** -23 * taps.max()              # symmetric to a rounding of exp2: the op is its own adjoint
    got = R.blur_ref(x, 10.0)
    assert np.abs(got - y).max() <= 1e-5 * np.abs(y).max()
    got_dx = R.blur_ref(r, 10.0)                                                # backward is the same op on the gradient
    assert np.abs(got_dx - dx).max() <= 1e-5 * np.abs(dx).max()
    assert np.array_equal(R.blur_ref(x, 0.3), x.astype(np.float64)) and R.reference_taps(0.0) is None


@pytest.mark.parametrize('ramp', [None, 0.05])
def test_host_values_are_the_reference_expressions(ramp):
    for total in R.TOTAL_ITERS:
        got = DeviceSchedule.host_values(total, 16, blur_init_sigma=10, blur_fade_kimg=100, ema_kimgs=10, ramp=ramp)
        sigma, radius, beta = R.reference_schedule(total, 16, 10, 100, 10, ramp)
        assert R.bits(got['blur_sigma']) == R.bits(sigma) and R.bits(got['blur_radius']) == R.bits(radius) and R.bits(got['ema_beta']) == R.bits(beta)
        assert got['total_iters'] == total
    assert DeviceSchedule.host_values(16, 16, 10, 100)['blur_radius'] == 29.0 and DeviceSchedule.host_values(100_000, 16, 10, 100)['blur_sigma'] == 0.0
    assert DeviceSchedule.host_values(99_984, 16, 10, 100)['blur_radius'] == 0.0 and DeviceSchedule.host_values(100_016, 16, 10, 100)['blur_sigma'] == 0.0
    off = DeviceSchedule.host_values(16, 16, blur_init_sigma=10, blur_fade_kimg=0, ema_kimgs=10, ramp=ramp)
    assert off['blur_sigma'] == 0.0 and off['blur_radius'] == 0.0
    if ramp is not None:                                                        # the ramp holds beta down early on and lets go of it later
        assert DeviceSchedule.host_values(16, 16, ema_kimgs=10, ramp=ramp)['ema_beta'] == 0.5 ** (16 / 0.8)
        assert DeviceSchedule.host_values(10 ** 6, 16, ema_kimgs=10, ramp=ramp)['ema_beta'] == 0.5 ** (16 / 10000)


def test_radius_over_a_whole_fade_never_grows():
    radii = [DeviceSchedule.host_values(t, 16, 10, 100)['blur_radius'] for t in range(0, 100_016 + 1, 16)]
    assert radii[0] == 30.0 and radii[-1] == 0.0 and all(a >= b for a, b in zip(radii, radii[1:])) and set(radii) == set(float(r) for r in range(31))


class _Opt:                                                                      # the fields of the reference's options that get_scheduler reads
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _reference_scheduler(optimizer, opt):
    """models/utils.py:56-66."""
    from torch.optim import lr_scheduler
    if opt.lr_policy == 'linear':
        def lambda_rule(epoch):
            return 1.0 - max(0, epoch + opt.epoch_count - opt.n_epochs) / float(opt.n_epochs_decay + 1)
        return lr_scheduler.LambdaLR(optimizer, lr_lambda=lambda_rule)
    if opt.lr_policy == 'step':
        return lr_scheduler.StepLR(optimizer, step_size=opt.lr_decay_iters, gamma=0.1)
    return lr_scheduler.CosineAnnealingLR(optimizer, T_max=opt.n_epochs, eta_min=0)


@pytest.mark.parametrize('epoch_count', [1, 30])
@pytest.mark.parametrize('policy', ['linear', 'step', 'cosine'])
def test_lr_schedule_follows_torch_schedulers(policy, epoch_count):
    import warnings
    opt = _Opt(lr_policy=policy, epoch_count=epoch_count, n_epochs=50, n_epochs_decay=50, lr_decay_iters=50)
    optimizer = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=0.0002, betas=(0.0, 0.99))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                                          # "scheduler.step() before optimizer.step()": the reference's order
        scheduler = _reference_scheduler(optimizer, opt)
        mine = LRSchedule(policy, 0.0002, epoch_count=epoch_count, n_epochs=50, n_epochs_decay=50, lr_decay_iters=50)
        assert mine.lr_at(0) == 0.0002
        seen = []
        for k in range(1, 101):
            scheduler.step()                                                     # train.py:44, before the epoch's first batch
            want = optimizer.param_groups[0]['lr']
            assert R.rel(mine.lr_at(k), want) <= 1e-15, (policy, k, mine.lr_at(k), want)
            seen.append(want)
    assert min(seen) < 0.5 * max(seen)                                           # the policy did decay inside the range
    assert mine.lr_at(37) == LRSchedule(policy, 0.0002, epoch_count=epoch_count, n_epochs=50, n_epochs_decay=50, lr_decay_iters=50).lr_at(37)


def test_plateau_is_refused():
    with pytest.raises(NotImplementedError, match='plateau'):
        LRSchedule('plateau', 0.0002)
    with pytest.raises(NotImplementedError, match='not implemented'):
        LRSchedule('exponential', 0.0002)
    with pytest.raises(RuntimeError, match='ROCm device'):
        DeviceSchedule('cpu', lr_G=0.0002)


def test_new_entry_points_and_their_refusals(lib):
    from afcm_amd import _lib
    for name in ('afcm_schedule_advance', 'afcm_gauss_blur', 'afcm_gauss_blur_rmax', 'afcm_ema_multi', 'afcm_adam_multi_capturable_lr'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.afcm_abi_version() == 13 and lib.afcm_gauss_blur_rmax() >= 30
    one = ctypes.c_void_p(64)                                                    # never dereferenced: every call below is refused before a launch
    assert lib.afcm_schedule_advance(None, 16, 10.0, 100.0, 10.0, -1.0, None) == _lib.E_INVALID and b'null block' in lib.afcm_last_error()
    assert lib.afcm_schedule_advance(one, 0, 10.0, 100.0, 10.0, -1.0, None) == _lib.E_INVALID and b'below 1' in lib.afcm_last_error()
    for y, x, s in ((None, one, one), (one, None, one), (one, ctypes.c_void_p(128), None), (one, one, ctypes.c_void_p(128))):
        assert lib.afcm_gauss_blur(y, x, s, 1, 8, 8, 1.0, None, None) == _lib.E_INVALID
    y, x, s = ctypes.c_void_p(64), ctypes.c_void_p(128), ctypes.c_void_p(192)
    assert lib.afcm_gauss_blur(y, x, s, 0, 8, 8, 1.0, None, None) == _lib.E_INVALID
    cap = lib.afcm_gauss_blur_rmax()
    for sigma in ((cap + 1) / 3.0, -1.0, float('nan')):
        assert lib.afcm_gauss_blur(y, x, s, 1, 8, 8, sigma, None, None) == _lib.E_INVALID and b'sigma' in lib.afcm_last_error()
    assert lib.afcm_ema_multi(None, 1, 1, 0.5, None, None) == _lib.E_INVALID and lib.afcm_ema_multi(one, 0, 1, 0.5, None, None) == _lib.E_INVALID
    assert lib.afcm_ema_multi(one, 1, 0, 0.5, None, None) == _lib.E_INVALID and lib.afcm_ema_multi(one, 1, 1, 1.5, None, None) == _lib.E_INVALID
    assert lib.afcm_adam_multi_capturable_lr(one, 1, 1, one, None, 0.0, 0.99, 1e-8, 1.0, 1, 1e5, -1e5, 0, None) == _lib.E_INVALID
    assert b'null learning rate' in lib.afcm_last_error()
    assert lib.afcm_adam_multi_capturable_lr(None, 1, 1, one, one, 0.0, 0.99, 1e-8, 1.0, 1, 1e5, -1e5, 0, None) == _lib.E_INVALID
    assert lib.afcm_adam_multi_capturable_lr(one, 1, 1, None, one, 0.0, 0.99, 1e-8, 1.0, 1, 1e5, -1e5, 0, None) == _lib.E_INVALID


def test_python_wrappers_refuse_before_any_launch():
    from afcm_amd.optim import FusedScrubAdam
    from afcm_amd.torch_utils.ops.gauss_blur import gauss_blur
    x = torch.zeros(1, 1, 8, 8)
    with pytest.raises(RuntimeError, match='no CPU'):
        gauss_blur(x, sigma=1.0)
    with pytest.raises(RuntimeError, match='sigma or schedule'):
        gauss_blur(x)
    with pytest.raises(RuntimeError, match=r'\[N, C, H, W\]'):
        gauss_blur(x[0], sigma=1.0)
    with pytest.raises(RuntimeError, match=r'float64 \[8\]'):
        gauss_blur(x, schedule=torch.zeros(8))
    with pytest.raises(ValueError, match='capturable=True'):
        FusedScrubAdam([torch.nn.Parameter(torch.zeros(1))], lr_dev=torch.zeros(1, dtype=torch.float64))
    with pytest.raises(ValueError, match='float64 device tensor'):
        FusedScrubAdam([torch.nn.Parameter(torch.zeros(1))], capturable=True, lr_dev=torch.zeros(1, dtype=torch.float64))


def test_schedule_kernels_use_no_scratch():
    """Code-object metadata of the built schedule.o, blur.o, ema.o and optim.o: no scratch and no spills in any kernel; LDS only in the two blur
    passes (DESIGN section 8j quotes the registers).  The objects are build products; a tree that has the library but not an object compiles it."""
    csrc = os.path.join(ROOT, 'afcm_amd', 'csrc')
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from kernel_resources import kernel_resources
    want = {'schedule.o': ['schedule_advance_kernel'], 'blur.o': ['gauss_rows_kernel', 'gauss_cols_kernel'], 'ema.o': ['ema_multi_kernel'],
            'optim.o': ['adam_multi_kernel']}
    for obj, names in want.items():
        if not os.path.exists(os.path.join(csrc, obj)):
            subprocess.check_call(['make', '-C', csrc, obj])
        found = kernel_resources(os.path.join(csrc, obj))
        for name in names:
            kernels = [k for k in found if name in k['name']]
            assert len(kernels) == 1, (name, [k['name'] for k in found])
            k = kernels[0]
            assert k.get('scratch', 0) == 0 and k.get('vgpr_spill', 0) == 0 and k.get('sgpr_spill', 0) == 0, k
            assert k.get('vgpr', 0) <= 128, k                                      # two 256-thread workgroups per SIMD at least
            assert (k.get('lds', 0) > 0) == (obj == 'blur.o') and k.get('lds', 0) <= 40 * 1024, k
