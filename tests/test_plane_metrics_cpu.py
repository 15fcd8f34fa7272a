"""The bookkeeping between the device kernel's statistics table and the reference's validation numbers, with no GPU: the finishers
``evaluation.evaluate_*_from_stats`` applied to the float64 numpy table of tests/plane_metrics_ref.py must reproduce
``evaluation.evaluate_2D`` / ``evaluate_slice`` / ``evaluate_one`` on the same arrays.

Tolerances: 1e-10 on SSIM, 1e-9 dB on PSNR, 2e-6 relative on MAE (the existing functions average float32 arrays in float32: pairwise
summation over <= 2^20 elements bounds that at about 20 * 2^-24).

Which dtype the arrays have matters to the EXISTING functions, not to the table: on float32 arrays ``psnr_2D`` divides by the maximum in
float32 and ``ThreeD_psnr`` forms its joint range in float32, one rounding of 2^-24 per element that the float64 table does not make
(measured here: 1.5e-7 dB at 16 x 16, 1.4e-8 dB at 32 x 48, 4e-10 dB at 16 planes of 256 x 256).  PSNR and SSIM are therefore compared on
float64 arrays that hold the same float32-representable values, where both sides divide in float64; MAE is compared on the float32
arrays, where the existing function's float32 mean is the thing the 2e-6 covers."""
import numpy as np
import pytest

import plane_metrics_ref as R
from afcm_amd import evaluation as E

TOL_SSIM, TOL_PSNR_DB, TOL_MAE_REL = 1e-10, 1e-9, 2e-6


def _tables_by_axis(real, fake):
    return [R.table(np.moveaxis(real, a, 0), np.moveaxis(fake, a, 0)) for a in range(3)]


def _close(got, want, mae32):
    assert abs(got[0] - want[0]) <= TOL_PSNR_DB, (got[0], want[0])
    assert abs(got[1] - want[1]) <= TOL_SSIM, (got[1], want[1])
    assert abs(got[2] - want[2]) <= TOL_MAE_REL * abs(want[2]), (got[2], want[2])
    assert abs(got[2] - float(mae32)) <= TOL_MAE_REL * abs(float(mae32)), (got[2], mae32)


def _batch(seed=0, empty=(2,)):
    real, fake = R.noisy_pair((4, 1, 1, 16, 16), seed)
    for i in empty:
        real[i] = 0.0
    return real, fake


def test_evaluate_2D_with_one_empty_slice():
    real, fake = _batch()
    t = R.table(real[:, 0, 0], fake[:, 0, 0])
    assert t[2, 0] == 0.0 and (t[[0, 1, 3], 0] > 0).all()
    got = E.evaluate_2D_from_stats(t, 16, 16)
    want = E.evaluate_2D(fake.astype(np.float64), real.astype(np.float64))
    _close(got, want, E.evaluate_2D(fake, real)[2])
    # the empty slice is left out of the PSNR / SSIM means but stays in the whole-batch MAE
    keep = [0, 1, 3]
    assert abs(got[1] - np.mean([E.structural_similarity(real[i, 0, 0], fake[i, 0, 0]) for i in keep])) <= TOL_SSIM
    assert abs(got[2] - np.abs(real.astype(np.float64) - fake).mean()) <= 1e-15


def test_evaluate_2D_all_empty_is_none():
    real, fake = _batch(1, empty=(0, 1, 2, 3))
    assert E.evaluate_2D(fake, real) is None
    assert E.evaluate_2D_from_stats(R.table(real[:, 0, 0], fake[:, 0, 0]), 16, 16) is None


def test_identical_pair_gives_inf_psnr_and_unit_ssim():
    real, _ = _batch(2, empty=())
    t = R.table(real[:, 0, 0], real[:, 0, 0])
    got, want = E.evaluate_2D_from_stats(t, 16, 16), E.evaluate_2D(real.astype(np.float64), real.astype(np.float64))
    assert got[0] == want[0] == np.inf
    assert abs(got[1] - 1.0) <= TOL_SSIM and abs(want[1] - 1.0) <= TOL_SSIM
    assert got[2] == want[2] == 0.0


def test_zero_maximum_prediction_gives_nan_psnr_as_numpy_does():
    real, fake = _batch(3, empty=())
    fake[1] = 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        want = E.evaluate_2D(fake.astype(np.float64), real.astype(np.float64))
    got = E.evaluate_2D_from_stats(R.table(real[:, 0, 0], fake[:, 0, 0]), 16, 16)
    assert np.isnan(want[0]) and np.isnan(got[0])
    assert abs(got[1] - want[1]) <= TOL_SSIM and abs(got[2] - want[2]) <= TOL_MAE_REL * want[2]


def test_negative_reference_value_selects_data_range_2():
    real, fake = _batch(4, empty=())
    real[1, 0, 0, 3, 5] = -0.25
    t = R.table(real[:, 0, 0], fake[:, 0, 0])
    got = E.evaluate_2D_from_stats(t, 16, 16)
    want = E.evaluate_2D(fake.astype(np.float64), real.astype(np.float64))
    _close(got, want, E.evaluate_2D(fake, real)[2])
    # the range really is 2 for that slice: 20 log10(2) dB above the same sums at range 1
    one = 10 * np.log10(1.0 / (t[1, 5] / 256))
    assert abs(E._psnr_2D_from_row(t[1], 256) - (one + 20 * np.log10(2.0))) <= TOL_PSNR_DB


def test_out_of_range_reference_raises_as_float_data_range_does():
    """``_float_data_range`` sees the MAX-NORMALISED reference (psnr_2D), whose maximum is 1 by construction: a reference value above 1 alone
    does not raise in ``evaluate_2D`` and must not raise in the finisher; a minimum below minus the maximum does, in both."""
    real, fake = _batch(5, empty=())
    real[0, 0, 0, 2, 2] = 1.5
    got = E.evaluate_2D_from_stats(R.table(real[:, 0, 0], fake[:, 0, 0]), 16, 16)
    _close(got, E.evaluate_2D(fake.astype(np.float64), real.astype(np.float64)), E.evaluate_2D(fake, real)[2])
    real[0, 0, 0, 4, 4] = -1.75
    with pytest.raises(ValueError, match='outside the range expected'):
        E.evaluate_2D(fake.astype(np.float64), real.astype(np.float64))
    with pytest.raises(ValueError, match='outside the range expected'):
        E.evaluate_2D_from_stats(R.table(real[:, 0, 0], fake[:, 0, 0]), 16, 16)
    # and the check of peak_signal_noise_ratio itself on an un-normalised image above 1, which the finishers never call
    with pytest.raises(ValueError, match='outside the range expected'):
        E.peak_signal_noise_ratio(np.full((8, 8), 1.5), np.zeros((8, 8)))


@pytest.fixture(scope='module')
def volume():
    real, fake = R.noisy_pair((8, 9, 10), 6)
    real[3] = 0.25                                        # one constant slice PAIR along axis 0: ThreeD_psnr's running-mean branch
    fake[3] = 0.25
    real[5] = 0.0                                         # and one empty target slice, for evaluate_slice's skip
    return real, fake


def test_evaluate_one_with_a_constant_slice_pair(volume):
    real, fake = volume
    tabs = _tables_by_axis(real, fake)
    assert tabs[0][3, 0] == tabs[0][3, 1] == tabs[0][3, 2] == tabs[0][3, 3] == 0.25
    got = E.evaluate_one_from_stats(tabs, real.shape)
    want = E.evaluate_one(fake.astype(np.float64), real.astype(np.float64))
    _close(got, want, E.evaluate_one(fake, real)[2])
    # the branch matters: counting the constant pair as 0 dB instead moves the mean far outside the tolerance
    naive = sum(10 * np.log10((max(r[0], r[2]) - min(r[1], r[3])) ** 2 / (r[4] / n)) for t, n in zip(tabs, (90, 80, 72)) for r in t
                if max(r[0], r[2]) > min(r[1], r[3])) / 27
    assert abs(naive - want[0]) > 1e-3


def test_evaluate_slice(volume):
    real, fake = volume
    fake = fake.copy()
    fake[3] = fake[2]                                     # (an identical pair would make the mean PSNR inf: covered above)
    t = R.table(real, fake)
    assert t[5, 0] == 0.0
    got = E.evaluate_slice_from_stats(t, 9, 10)
    want = E.evaluate_slice(fake.astype(np.float64), real.astype(np.float64))
    _close(got, want, E.evaluate_slice(fake, real)[2])


def test_float32_arrays_move_psnr_by_the_float32_divide_only():
    """On float32 arrays the existing ``psnr_2D`` rounds l / l.max() to float32.  Bound: each normalised value moves by <= 2^-25 (half an ulp
    below 1), each difference by <= 2^-24, so the sum of squares S = sum d^2 moves by <= 2 * 2^-24 * sum |d| + n 2^-48 <= 2^-23 sqrt(n S) (1 + small),
    i.e. PSNR by <= (10 / ln 10) * 2^-23 * sqrt(n / S) dB.  SSIM is unaffected (no division of the inputs)."""
    real, fake = _batch(7, empty=())
    real, fake = real * np.float32(0.9), fake * np.float32(0.8)      # maxima that are no powers of two: the float32 quotients do round
    t = R.table(real[:, 0, 0], fake[:, 0, 0])
    got, want32 = E.evaluate_2D_from_stats(t, 16, 16), E.evaluate_2D(fake, real)
    bound = max((10 / np.log(10)) * 2.0 ** -23 * np.sqrt(256 / row[5]) * 1.01 for row in t)
    print(f'float32-array PSNR difference {abs(got[0] - want32[0]):.3e} dB (bound {bound:.3e})')
    assert 0 < abs(got[0] - want32[0]) <= bound
    assert abs(got[0] - E.evaluate_2D(fake.astype(np.float64), real.astype(np.float64))[0]) <= TOL_PSNR_DB
    assert abs(got[1] - want32[1]) <= TOL_SSIM


def test_table_shape_is_checked():
    with pytest.raises(ValueError, match='statistics table'):
        E.evaluate_2D_from_stats(np.zeros((4, 7)), 16, 16)
    with pytest.raises(ValueError, match='three tables'):
        E.evaluate_one_from_stats([np.zeros((8, 8)), np.zeros((9, 8))], (8, 9, 10))


def test_reference_table_matches_a_window_loop():
    """tests/plane_metrics_ref.py against the plainest statement there is: a Python loop over windows, on one 8 x 9 plane."""
    real, fake = R.noisy_pair((1, 8, 9), 8)
    r, t = real[0].astype(np.float64), fake[0].astype(np.float64)
    s = 0.0
    for i in range(2):
        for j in range(3):
            a, b = r[i:i + 7, j:j + 7].ravel(), t[i:i + 7, j:j + 7].ravel()
            ux, uy = a.mean(), b.mean()
            vx, vy, vxy = a.var(ddof=1), b.var(ddof=1), ((a - ux) * (b - uy)).sum() / 48
            s += ((2 * ux * uy + R.C1) * (2 * vxy + R.C2)) / ((ux ** 2 + uy ** 2 + R.C1) * (vx + vy + R.C2))
    tab = R.table(real, fake)
    assert abs(tab[0, 7] - s) <= 1e-12 * abs(s)
    assert abs(tab[0, 7] / 6 - E.structural_similarity(r, t)) <= TOL_SSIM
    assert np.array_equal(R.unit_map(real * 2 - 1), E.to_unit_range(real * 2 - 1))


def test_new_ops_refuse_cpu_tensors():
    import torch
    from afcm_amd import evaluation_device, validation
    from afcm_amd.torch_utils.ops import plane_metrics
    x = torch.zeros(2, 8, 8)
    for fn in (lambda: plane_metrics.plane_stats(x, x), lambda: evaluation_device.evaluate_2D(x[:, None], x[:, None]),
               lambda: evaluation_device.evaluate_slice(x, x), lambda: evaluation_device.evaluate_one(x, x)):
        with pytest.raises(RuntimeError, match='no CPU'):
            fn()

    class Step:
        def set_input(self, a, b):
            self.real_B = self.fake_B = b

        def test(self):
            pass
    with pytest.raises(RuntimeError, match='no CPU'):
        validation.validate(Step(), [(x[:, None], x[:, None])])
    with pytest.raises(ValueError, match="'device' or 'host'"):
        validation.validate(Step(), [], metrics='gpu')
