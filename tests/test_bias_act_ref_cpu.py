"""tests/bias_act_ref.py checked without a GPU: the restatement against the aten oracle and its float64 autograd, the bar against honest
float32 arithmetic, the swish overflow of the reference's expression order, and the construction of the GPU file's inputs.

Measured here, the C that the float32 evaluation of the restated formulas needs (worst err / (2^-24 F) per mode over all activations,
the layouts of test (a) and the saturation grids of test (c)):  mode 0: 0.76 (softplus),  mode 1: 0.80 (swish),  mode 2: 0.84 (swish);
linear / relu / lrelu stay below 0.21.  The kernels on an MI355X need at most 1.40 (table in test_gpu_bias_act.py), hence C = 8.
"""
import numpy as np
import pytest
import torch

import bias_act_ref as R
from oracle import aten_ops as ops

F32 = R.F32


def _close(got, want, what):
    err = np.abs(got - want)
    lim = 1e-12 * np.abs(want) + 1e-300
    assert (err <= lim).all(), (what, float(err.max()), int(np.argmax(err - lim)))


@pytest.mark.parametrize('tuned', [False, True], ids=['defaults', 'gain_clamp'])
@pytest.mark.parametrize('act', R.ACTS)
def test_restatement_matches_the_oracle_and_its_autograd(act, tuned):
    """Mode 0 against oracle.aten_ops.bias_act, modes 1 and 2 against its first and double backward (the oracle's own y as the saved
    output), float64, 1e-12 relative, inputs away from the kinks and the clamp."""
    shape, dim = (3, 5, 7, 9), 1
    g = torch.Generator().manual_seed(11 + R.ACTS.index(act))
    x, r, q = (torch.randn(shape, generator=g, dtype=torch.float64) * s for s in (1.0, 1.0, 1.0))
    b = torch.randn(shape[dim], generator=g, dtype=torch.float64) * 0.3
    alpha = R.ALPHA if tuned else R.DEF_ALPHA[act]
    gain = float(np.float32(R.GAIN)) if tuned else float(np.float32(R.DEF_GAIN[act]))      # the restatement rounds parameters to float32
    clamp = float(np.float32(R.CLAMP[act])) if tuned else None
    alpha = float(np.float32(alpha))
    x.requires_grad_(True)
    y = ops.bias_act(x, b, dim=dim, act=act, alpha=alpha, gain=gain, clamp=clamp)
    z = (x + b.reshape(1, -1, 1, 1)).detach()
    assert int((z.abs() < 1e-6).sum()) == 0
    if clamp is not None:
        free = ops.bias_act(x.detach(), b, dim=dim, act=act, alpha=alpha, gain=gain)
        assert int(((free.abs() - clamp).abs() < 1e-9).sum()) == 0
        assert 0.1 < float((free.abs() > clamp).double().mean()) < 0.6, 'the clamp does not bite on a visible share'
    _close(R.ref(0, act, x, b, None, None, None, dim, alpha, gain, clamp), R.f64(y), f'{act} y')
    dx, = torch.autograd.grad((y * r).sum(), x, create_graph=True)
    _close(R.ref(1, act, r, b, x, y, None, dim, alpha, gain, clamp), R.f64(dx), f'{act} dx')
    d2 = torch.autograd.grad((dx * q).sum(), x)[0] if dx.requires_grad else torch.zeros_like(x)
    want2 = R.ref(2, act, q, b, x, y, r, dim, alpha, gain, clamp)
    _close(want2, R.f64(d2), f'{act} d2x')
    if act in R.SECOND:
        assert np.abs(want2).max() > 1e-3
    else:
        assert not want2.any()


def test_restatement_ieee_selections():
    """NaN and the infinities in mode 0: what the op's docstring states."""
    x = np.array([np.nan, np.inf, -np.inf, 0.5])
    limits = {'linear': (np.inf, -np.inf), 'relu': (np.inf, 0.0), 'lrelu': (np.inf, -np.inf), 'tanh': (1.0, -1.0), 'sigmoid': (1.0, 0.0),
              'elu': (np.inf, -1.0), 'selu': (np.inf, -R.SELU_SCALE * R.SELU_ALPHA), 'softplus': (np.inf, 0.0), 'swish': (np.inf, 0.0)}
    for act in R.ACTS:
        with np.errstate(all='ignore'):
            y = R.ref(0, act, x, None, None, None, None, 0, 0.25, 2.0, None)
            yc = R.ref(0, act, x, None, None, None, None, 0, 0.25, 2.0, 1.5)
        assert (y[0] == 0.0) if act == 'relu' else np.isnan(y[0]), act
        assert y[1] == 2.0 * limits[act][0] and y[2] == pytest.approx(2.0 * limits[act][1], rel=1e-15), (act, y)
        assert yc[0] == (0.0 if act == 'relu' else -1.5), (act, yc)
        assert yc[1] == 1.5 and yc[2] == max(-1.5, y[2]) and np.isfinite(y[3]), (act, yc)


def _float32_need(mode, act, args, dim, alpha, gain, clamp):
    """C needed by the float32 evaluation of the restated formulas on these operands."""
    want = R.ref(mode, act, *args, dim, alpha, gain, clamp)
    with np.errstate(all='ignore'):
        got = R.evaluate(mode, act, *args, dim, alpha, gain, clamp, dt=np.float32).astype(np.float64)
    f = R.scale_f(mode, want, args[0], args[1], args[2], args[4], dim, gain)
    assert R.mismatch(got, want, R.bar(mode, want, args[0], args[1], args[2], args[4], dim, gain, F32)) is None, (act, mode)
    return R.needed_c(got, want, f)


def test_bar_admits_honest_float32_arithmetic():
    """The restated formulas in numpy float32 on the fp32 operands of test (a) and on the saturation grids of test (c) stay inside the bar
    with the chosen C; the table of the C they need is printed (and quoted in this file's header)."""
    need = {}
    for act in R.ACTS:
        for layout in R.LAYOUTS:
            o = R.layout_operands(act, layout, F32)
            for mode in (0, 1, 2):
                c = _float32_need(mode, act, R.mode_operands(o, mode), o['dim'], o['alpha'], o['gain'], o['clamp'])
                need[act, mode] = max(need.get((act, mode), 0.0), c)
        for mode in R.SATURATION_MODES.get(act, ()):
            c = _float32_need(mode, act, R.saturation_case(act, mode, F32), 0, 0.0, R.GRID_GAIN, None)
            need[act, mode] = max(need[act, mode], c)
    for act in R.ACTS:
        print(f'{act:<9s}' + ''.join(f'  mode {m}: {need[act, m]:6.3f}' for m in (0, 1, 2)))
    assert max(need.values()) <= R.C
    assert R.C <= 64 and R.C == 2.0 ** round(np.log2(R.C))


# the two expression orders of the kernel's swish gradients, in numpy float32 exactly as written
def _swish_written(order, mode, x, xr):
    f = np.float32
    x, xr = f(x), f(xr)
    e = np.exp(xr)
    d = e + f(1)
    if order == 'old':
        return x * e * (xr + d) / (d * d) if mode == 1 else x * e * (xr * (f(2) - d) + f(2) * d) / (d * d * d)
    s = e / d
    return x * s * ((xr + d) / d) if mode == 1 else x * s * ((xr * (f(2) - d) + f(2) * d) / (d * d))


def test_swish_gradient_overflow_of_the_old_order():
    """float32, left to right: the reference's order gives inf (mode 1) and nan (mode 2) at xr = 40, x = 7000, where the true values are
    7000 and -2e-12; the re-associated order stays finite and inside the bar at all nine points.  These are the points of test (c)."""
    old, new = {}, {}
    for xr in (35.0, 39.5, 40.0):
        for x in (1e3, 7e3, 6e4):
            for mode in (1, 2):
                with np.errstate(all='ignore'):
                    old[mode, xr, x] = float(_swish_written('old', mode, x, xr))
                    new[mode, xr, x] = float(_swish_written('new', mode, x, xr))
                a = (np.array([x]), None, np.array([xr]), None, None)
                want = R.ref(mode, 'swish', *a, 0, 0.0, 1.0, None)
                lim = R.bar(mode, want, a[0], None, a[2], None, 0, 1.0, F32)
                print(f'mode {mode} xr {xr} x {x}: old {old[mode, xr, x]!r} new {new[mode, xr, x]!r} true {want[0]!r}')
                assert np.isfinite(new[mode, xr, x]) and abs(new[mode, xr, x] - want[0]) <= lim[0], (mode, xr, x)
    assert old[1, 40.0, 7e3] == np.inf and np.isnan(old[2, 40.0, 7e3])
    assert old[1, 40.0, 6e4] == np.inf and np.isnan(old[2, 40.0, 6e4])
    assert not all(np.isfinite(v) for v in old.values())


def test_gpu_cases_are_what_they_say():
    """Input construction of test_gpu_bias_act.py: no swish element inside the clamp margin (moved, never dropped: the shapes are whole),
    every clamp bites, the layouts reach the kernel they name, the second-trip shapes pass one full grid, the grids straddle the cuts."""
    n = 0
    for name, o in R.swish_clamp_cases():
        assert R.swish_margin_count(o['x'], o['b'], o['dim'], o['gain'], o['clamp']) == 0, name
        assert o['x'].shape == o['y'].shape == o['g'].shape and np.isfinite(o['x']).all(), name
        n += 1
    assert n == 3 * len(R.LAYOUTS) + 3 * len(R.SECOND_TRIP) + 3 * len(R.DISPATCH) + 2 * len(R.AUTOGRAD_LAYOUTS)
    for act in R.ACTS:
        for dtype in R.DTYPES:
            o = R.layout_operands(act, R.LAYOUTS[0], dtype)
            share = float((np.abs(o['y']) >= float(np.float32(o['clamp']))).mean())
            assert 0.1 < share < 0.6, (act, dtype, share)
            assert 3 <= o['b'].size <= 7
    tails = []
    for lid, shape, dim in R.LAYOUTS:
        for dtype in R.DTYPES:
            assert R.kernel_of(shape, dim, dtype, True) == ('vector' if lid == 'vec' else 'element'), (lid, dtype)
        tails.append(int(np.prod(shape)) % 4)
    assert sorted(tails[1:4]) == [1, 2, 3] and len(R.LAYOUTS[4][1]) == 2
    for cid, kernel, shapes in R.SECOND_TRIP:
        for dtype in R.DTYPES:
            numel = int(np.prod(shapes[dtype]))
            assert R.kernel_of(shapes[dtype], 1, dtype, True) == kernel and R.trips(kernel, numel, dtype) == 2, (cid, dtype)
            assert numel * 8 * 5 < 200e6
            if kernel == 'element':
                assert numel % 4 == 2 and (numel >> 2) > R.GRID_THREADS
    for case in R.DISPATCH:
        assert R.kernel_of(case[1], case[2], F32, case[3]) == case[4] and R.kernel_of(case[1], case[2], R.F16, case[3]) == case[5]
    assert R.kernel_of(R.OFFSET_SHAPE, 1, R.BF16, True) == 'vector' and R.kernel_of(R.OFFSET_SHAPE, 1, R.BF16, True, aligned=False) == 'element'
    for dtype in R.DTYPES:
        pts = R.saturation_points(dtype)
        for cut in (40.0, 80.0):
            above, below = pts[pts > cut].min(), pts[pts < cut].max()
            assert cut in pts and -cut in pts and (above - cut) == (cut - below) <= cut * 4 * R.UNIT[dtype], (dtype, cut)
        assert (dtype == F32) != (1000.0 in pts) and (dtype == R.F16) == (65504.0 in pts)
        assert (R.forwarded_magnitudes(dtype).max() > 1e29) == (dtype != R.F16)
