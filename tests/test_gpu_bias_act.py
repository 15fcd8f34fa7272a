"""afcm_bias_act's two kernels (afcm_amd/csrc/bias_act.hip: bias_act_vec_kernel, bias_act_kernel) against the float64 restatement of
tests/bias_act_ref.py: EVERY element of every result inside

    |got - want| <= u_T |want| + C 2^-24 F + m_T,     F = |want| + |gain dy| (1 + |x| max(1, |xref + b|))

(u_T one rounding of the stored type, m_T its smallest normal, F the scale of the fp32 cancellation floors).  Single modes run through the
plugin surface, which lets the saved tensors be chosen; the autograd wiring runs through ops.bias_act.  tests/test_bias_act_ref_cpu.py
checks the restatement, that the bar admits honest float32 arithmetic, and that the inputs here are what they claim to be.

C.  The C each fp32 result needs, worst err / (2^-24 F) on an MI355X over the cases of test (a) and the grids of test (c):

               mode 0   mode 1   mode 2                   mode 0   mode 1   mode 2
    linear      0.15     0.00     0.00        elu          0.56     0.41     0.58
    relu        0.15     0.00     0.00        selu         0.92     0.75     0.73
    lrelu       0.20     0.09     0.00        softplus     1.40     0.49     0.28
    tanh        1.20     0.55     0.62        swish        0.43     0.82     1.26
    sigmoid     0.51     0.21     0.16

(every other fp32 case of this file: at most 1.38).  The float32 evaluation of the restated formulas on the CPU needs at most 0.84
(test_bias_act_ref_cpu.py).  C = R.C = 8 is the smallest power of two at or above four times the GPU's worst, 1.40; the margin is for
expf / logf of 1 to 2 ulp.  The swish gradients at the overflow points (inf / nan before the re-association in act_eval<9>) never entered
the measurement: the table is of the fixed kernel.
"""
import numpy as np
import pytest
import torch

import bias_act_ref as R

pytestmark = pytest.mark.gpu

F32, F16, BF16 = R.F32, R.F16, R.BF16
dtype_id = R.DTYPE_ID.get


def _dev(a, dtype):
    """float64 numpy of representable values -> device tensor; None -> the plugin's empty tensor."""
    return torch.empty([0], dtype=dtype, device='cuda') if a is None else R.tensor(a, dtype).cuda()


def _plugin_call(mode, act, tensors, dim, alpha, gain, clamp):
    from afcm_amd.torch_utils import custom_ops
    plugin = custom_ops.get_plugin('bias_act_plugin')
    x = tensors[0]
    y = plugin.bias_act(*tensors, mode, dim, R.INDEX[act], alpha, gain, -1.0 if clamp is None else clamp)
    assert y.dtype == x.dtype and y.shape == x.shape and y.is_contiguous()
    return R.f64(y)


def _check(what, mode, act, args, dim, alpha, gain, clamp, dtype, where=None, tensors=None, finite=False):
    """One launch of one mode on float64 operands ``args`` = (x, b, xref, yref, dy) against the restatement; returns the C it needed."""
    with np.errstate(all='ignore'):
        want = R.ref(mode, act, *args, dim, alpha, gain, clamp)
        lim = R.bar(mode, want, args[0], args[1], args[2], args[4], dim, gain, dtype)
        f = R.scale_f(mode, want, args[0], args[1], args[2], args[4], dim, gain)
    got = _plugin_call(mode, act, tensors or [_dev(a, dtype) for a in args], dim, alpha, gain, clamp)
    need = R.needed_c(got, want, f, dtype)
    print(f'need {what} {act} mode {mode} {dtype_id(dtype)} {need:.3f}')
    if finite:
        assert np.isfinite(got).all(), f'{what} {act} mode {mode} {dtype}: non-finite at {np.flatnonzero(~np.isfinite(got))[:8]}'
    bad = R.mismatch(got, want, lim, where)
    assert bad is None, f'{what} {act} mode {mode} {dtype} dim {dim} gain {gain} clamp {clamp}: {bad}'
    return got


# ------------------------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize('dtype', R.DTYPES, ids=dtype_id)
@pytest.mark.parametrize('layout', R.LAYOUTS, ids=lambda l: l[0])
@pytest.mark.parametrize('act', R.ACTS)
def test_every_activation_mode_type_and_kernel(act, layout, dtype):
    """The three modes of one activation, per element: the vector kernel, the element kernel with 1, 2 and 3 tail elements and on [N, C];
    5 to 7 bias channels, alpha 0.3, gain 1.3, a clamp that bites on a fifth to a half of the elements (asserted on the CPU).  The saved
    output is the rounded forward result, so modes 1 and 2 mask exactly the elements a forward launch stored on the clamp."""
    o = R.layout_operands(act, layout, dtype)
    for mode in (0, 1, 2):
        _check('a/' + layout[0], mode, act, R.mode_operands(o, mode), o['dim'], o['alpha'], o['gain'], o['clamp'], dtype)


# ------------------------------------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize('dtype', R.DTYPES, ids=dtype_id)
@pytest.mark.parametrize('case', R.SECOND_TRIP, ids=lambda c: c[0])
def test_second_trip_of_both_loops(case, dtype):
    """Tensors just past one full grid (2048 workgroups x 256 lanes x one vector): every lane of the first workgroups runs its loop
    twice; the element kernel's shape leaves 2 tail elements that start past the full grid.  Swish mode 2 reads every operand."""
    cid, kernel, shapes = case
    o = R.second_trip_operands(case, dtype)
    numel = o['x'].size
    assert R.trips(kernel, numel, dtype) == 2 and R.kernel_of(shapes[dtype], 1, dtype, True) == kernel
    assert R.swish_margin_count(o['x'], o['b'], 1, o['gain'], o['clamp']) == 0
    _check('b/' + cid, 2, 'swish', R.mode_operands(o, 2), 1, o['alpha'], o['gain'], o['clamp'], dtype, where=R.position(kernel, numel, dtype))


# ------------------------------------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize('dtype', R.DTYPES, ids=dtype_id)
@pytest.mark.parametrize('act, mode', [(a, m) for a, ms in R.SATURATION_MODES.items() for m in ms])
def test_saturation_grids(act, mode, dtype):
    """Around the |x| > 80 cuts of the forward and the xref > 40 cut of the swish gradients: the representable neighbours of the cuts on
    both sides, points up to the largest value of the type, and for the swish gradients forwarded operands up to 6e4 (1e30 where the
    type holds it) -- loss-scaled gradients.  Finite everywhere and inside the bar.  Before the re-association in act_eval<9> swish
    mode 1 gave inf from xref = 39.5 at x = 6e4 (from just below 40 at x = 7e3), mode 2 nan from 39.5 at x = 1e3, and both at every
    point from 20 up to the cut at x = 1e30: all six swish gradient cases failed."""
    args = R.saturation_case(act, mode, dtype)
    _check('c', mode, act, args, 0, 0.0, R.GRID_GAIN, None, dtype, finite=True)


# ------------------------------------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize('which', [0, 2, 3, 4], ids=['x', 'xref', 'yref', 'dy'])
@pytest.mark.parametrize('dtype', R.DTYPES, ids=dtype_id)
def test_operand_at_a_storage_offset_of_one_element(dtype, which):
    """A vector-eligible shape with ONE operand a contiguous view one element into its storage: the host must see the pointer and take
    the element kernel (a 16-byte access there would be misaligned)."""
    o = R.offset_operands(dtype)
    args = R.mode_operands(o, 2)
    tensors = [_dev(a, dtype) for a in args]
    n = tensors[which].numel()
    buf = torch.zeros(n + 8, dtype=dtype, device='cuda')
    view = buf[1:1 + n].view(tensors[which].shape)
    view.copy_(tensors[which])
    assert view.is_contiguous() and view.data_ptr() % 16 != 0 and all(t.data_ptr() % 16 == 0 for i, t in enumerate(tensors) if i != which)
    tensors[which] = view
    _check('d/offset', 2, 'tanh', args, 1, o['alpha'], o['gain'], o['clamp'], dtype, tensors=tensors)


@pytest.mark.parametrize('dtype', R.DTYPES, ids=dtype_id)
@pytest.mark.parametrize('act', R.DISPATCH_ACTS)
@pytest.mark.parametrize('case', R.DISPATCH, ids=lambda c: c[0])
def test_host_dispatch_without_bias_and_below_one_vector(case, act, dtype):
    """b = None with numel % V != 0 (element kernel) and with numel % V = 0 at an odd inner (vector kernel: without a bias the inner
    size does not matter); fewer elements than one vector; one element."""
    o = R.dispatch_operands(case, act, dtype)
    for mode in (0, 1, 2):
        _check('d/' + case[0], mode, act, R.mode_operands(o, mode), o['dim'], o['alpha'], o['gain'], o['clamp'], dtype)


# ------------------------------------------------------------------------------------------------------------------------------ (e)
def _sum_bar(t, dim, dtype):
    """(float64 sum of ``t`` over every axis but ``dim``, its bar): n terms accumulated in fp32 in any order err by at most
    (n - 1) 2^-24 sum|t_i|, and the result is rounded once to the stored type."""
    axes = tuple(i for i in range(t.ndim) if i != dim)
    n = t.size // t.shape[dim]
    s = t.sum(axis=axes)
    return s, R.UNIT[dtype] * np.abs(s) + n * R.EPS32 * np.abs(t).sum(axis=axes) + R.TINY[dtype]


@pytest.mark.parametrize('dtype', R.AUTOGRAD_DTYPES, ids=dtype_id)
@pytest.mark.parametrize('shape, dim', R.AUTOGRAD_LAYOUTS, ids=lambda v: str(v).replace(' ', ''))
@pytest.mark.parametrize('act', R.AUTOGRAD_ACTS)
def test_layouts_through_the_autograd_op(act, shape, dim, dtype):
    """dim = 0, the last and a middle dim of 1-D to 5-D inputs through ops.bias_act: y, dx and the second-order d_x per element against
    the restatement on the op's own saved tensors; db and d_b against the float64 sum of the very dx / d_x the GPU returned (the
    reduction apart from the kernel's rounding).  lrelu: the second-order terms are exactly zero or None."""
    from afcm_amd.torch_utils.ops import bias_act as ba
    o = R.autograd_operands(act, shape, dim, dtype)
    alpha, gain, clamp = o['alpha'], o['gain'], o['clamp']
    x, b = (_dev(o[k], dtype).requires_grad_(True) for k in ('x', 'b'))
    r, q = _dev(o['g'], dtype), _dev(o['q'], dtype)
    y = ba.bias_act(x, b, dim=dim, act=act, alpha=alpha, gain=gain, clamp=clamp)
    dx, db = torch.autograd.grad(y, [x, b], r, create_graph=True)
    d_x, d_b = torch.autograd.grad(dx, [x, b], q, allow_unused=True)
    assert y.dtype == dx.dtype == db.dtype == dtype and y.shape == dx.shape == x.shape and db.shape == b.shape
    saved = R.f64(y)

    def held(name, got, mode, args):
        want = R.ref(mode, act, *args, dim, alpha, gain, clamp)
        bad = R.mismatch(got, want, R.bar(mode, want, args[0], args[1], args[2], args[4], dim, gain, dtype))
        assert bad is None, f'{act} {shape} dim {dim} {dtype} {name}: {bad}'

    held('y', saved, 0, (o['x'], o['b'], None, None, None))
    held('dx', R.f64(dx), 1, (o['g'], o['b'], o['x'], saved, None))
    s, lim = _sum_bar(R.f64(dx), dim, dtype)
    assert R.mismatch(R.f64(db), s, lim) is None, f'{act} {shape} dim {dim} {dtype} db: {R.mismatch(R.f64(db), s, lim)}'
    if act == 'lrelu':
        assert d_x is None or not bool(d_x.any())
        assert d_b is None or not bool(d_b.any())
        return
    assert d_x.dtype == d_b.dtype == dtype and d_x.shape == x.shape and d_b.shape == b.shape
    held('d_x', R.f64(d_x), 2, (o['q'], o['b'], o['x'], saved, o['g']))
    s, lim = _sum_bar(R.f64(d_x), dim, dtype)
    assert R.mismatch(R.f64(d_b), s, lim) is None, f'{act} {shape} dim {dim} {dtype} d_b: {R.mismatch(R.f64(d_b), s, lim)}'


@pytest.mark.parametrize('dtype', R.AUTOGRAD_DTYPES, ids=dtype_id)
@pytest.mark.parametrize('act', ['tanh', 'swish'])
def test_non_contiguous_operands_give_the_contiguous_bits(act, dtype):
    """channels_last and transposed x, an expanded (stride 0) and a transposed incoming gradient: bit-identical to the contiguous copies."""
    from afcm_amd.torch_utils.ops import bias_act as ba
    bits = lambda t: t.contiguous().view(torch.int32 if dtype == F32 else torch.int16)

    def run(x, b, dim, dy):
        x, b = x.detach().requires_grad_(True), b.detach().requires_grad_(True)
        y = ba.bias_act(x, b, dim=dim, act=act, gain=R.GAIN, clamp=R.CLAMP[act])
        dx, db = torch.autograd.grad(y, [x, b], dy(y), create_graph=True)
        d_x, d_b = torch.autograd.grad(dx, [x, b], dy(dx))
        return [y, dx, db, d_x, d_b]

    x4 = _dev(R.rounded((2, 5, 6, 8), dtype, 5100), dtype)
    x2 = _dev(R.rounded((9, 6), dtype, 5101), dtype)
    b4, b2 = _dev(R.rounded((5,), dtype, 5102, 0.3), dtype), _dev(R.rounded((9,), dtype, 5103, 0.3), dtype)
    g4 = _dev(R.rounded((2, 6, 5, 8), dtype, 5104), dtype)
    ones = lambda t: torch.ones_like(t, memory_format=torch.contiguous_format)
    expanded = lambda t: torch.ones([], dtype=dtype, device='cuda').expand_as(t)
    cases = [
        ('channels_last x', run(x4.contiguous(memory_format=torch.channels_last), b4, 1, ones), run(x4, b4, 1, ones)),
        ('transposed x', run(x2.t(), b2, 1, ones), run(x2.t().contiguous(), b2, 1, ones)),
        ('expanded dy', run(x4, b4, 1, expanded), run(x4, b4, 1, ones)),
        ('transposed dy', run(x4, b4, 1, lambda t: g4.transpose(1, 2)), run(x4, b4, 1, lambda t: g4.transpose(1, 2).contiguous())),
    ]
    assert not x4.contiguous(memory_format=torch.channels_last).is_contiguous() and not x2.t().is_contiguous()
    assert not expanded(x4).is_contiguous() and not g4.transpose(1, 2).is_contiguous()
    for what, got, want in cases:
        for name, a, c in zip(['y', 'dx', 'db', 'd_x', 'd_b'], got, want):
            assert a.shape == c.shape and torch.equal(bits(a), bits(c)), f'{act} {dtype} {what}: {name} differs'
    # y.sum().backward(): the gradient autograd itself expands
    x = x4.detach().requires_grad_(True)
    ba.bias_act(x, b4, dim=1, act=act, gain=R.GAIN, clamp=R.CLAMP[act]).sum().backward()
    assert torch.equal(bits(x.grad), bits(cases[2][2][1]))


# ------------------------------------------------------------------------------------------------------------------------------ (f)
@pytest.mark.parametrize('dtype', [F32, F16], ids=dtype_id)
@pytest.mark.parametrize('layout', R.LAYOUTS[:2], ids=lambda l: l[0])
@pytest.mark.parametrize('edge', ['gain0', 'clamp0'])
def test_zero_gain_and_zero_clamp(edge, layout, dtype):
    """gain = 0 (the yy = 0 branch) and clamp = 0 (an empty open interval): every mode of every activation gives 0 everywhere."""
    for act in R.ACTS:
        o = R.layout_operands(act, layout, dtype)
        gain, clamp = (0.0, o['clamp']) if edge == 'gain0' else (o['gain'], 0.0)
        for mode in (0, 1, 2):
            args = R.mode_operands(o, mode)
            assert not R.ref(mode, act, *args, o['dim'], o['alpha'], gain, clamp).any()
            got = _plugin_call(mode, act, [_dev(a, dtype) for a in args], o['dim'], o['alpha'], gain, clamp)
            assert not got.any(), f'{edge} {act} mode {mode} {dtype}: {np.count_nonzero(got)} elements are not 0'


@pytest.mark.parametrize('dtype', R.DTYPES, ids=dtype_id)
@pytest.mark.parametrize('alpha', [0.0, -0.5, 1.0])
def test_lrelu_alpha_edges(alpha, dtype):
    for layout in R.LAYOUTS[:2]:
        o = R.layout_operands('lrelu', layout, dtype)
        # the saved output of THIS alpha (with alpha <= 0 the sign of y no longer tells the side of x: the contract reads y)
        y = R.quantize(R.ref(0, 'lrelu', o['x'], o['b'], None, None, None, o['dim'], alpha, o['gain'], o['clamp']), dtype)
        o = dict(o, y=y)
        for mode in (0, 1, 2):
            _check('f/alpha', mode, 'lrelu', R.mode_operands(o, mode), o['dim'], alpha, o['gain'], o['clamp'], dtype)


@pytest.mark.parametrize('dtype', R.DTYPES, ids=dtype_id)
@pytest.mark.parametrize('act', ['relu', 'lrelu', 'elu', 'selu'])
def test_kink_at_plus_and_minus_zero(act, dtype):
    """x + b exactly +0 and -0 among ordinary values: the forward value, then modes 1 and 2 on the saved output the GPU itself stored
    and on hand-made +0 / -0 saved outputs.  The side of the kink is the sign test of the SAVED output (relu, lrelu: y > 0; elu, selu:
    y >= 0), so a zero output has slope 0 / alpha for relu / lrelu and slope 1 / scale for elu / selu."""
    x = np.array([0.5, -0.5, 0.0, -0.0, -0.0, 2.0, -2.0, 0.25, 0.0, -1.0])
    b = np.array([-0.5, 0.5, 0.0, 0.0, -0.0, 0.0, 0.0, 0.0, -0.0, 1.0])
    z = x + b
    assert (z[:5] == 0).all() and np.signbit(z[4]) and not np.signbit(z[:4]).any()
    g = R.quantize(R.rounded(x.shape, dtype, 5200) + 3.0, dtype)      # forwarded operands far from 0: a wrong side is a visible error
    q = R.quantize(R.rounded(x.shape, dtype, 5201) + 3.0, dtype)
    saved = _check('f/kink', 0, act, (x, b, None, None, None), 0, 0.3, R.GAIN, None, dtype)
    flipped = np.where(z == 0, -saved, saved)                      # the other zero at the kink
    for yref in (saved, flipped):
        _check('f/kink', 1, act, (g, b, x, yref, None), 0, 0.3, R.GAIN, None, dtype)
        _check('f/kink', 2, act, (q, b, x, yref, g), 0, 0.3, R.GAIN, None, dtype)


def test_empty_tensor():
    from afcm_amd.torch_utils.ops import bias_act as ba
    for dtype in R.DTYPES:
        x = torch.empty([0, 3, 4], dtype=dtype, device='cuda')
        b = torch.zeros([3], dtype=dtype, device='cuda')
        y = ba.bias_act(x, b, dim=1, act='swish', clamp=1.0)
        assert y.shape == x.shape and y.dtype == dtype
        e = torch.empty([0], dtype=dtype, device='cuda')
        from afcm_amd.torch_utils import custom_ops
        y = custom_ops.get_plugin('bias_act_plugin').bias_act(x, b, e, e, e, 0, 1, R.INDEX['swish'], 0.0, 1.0, -1.0)
        assert y.shape == x.shape and y.dtype == dtype


def test_argument_errors_are_raised_by_the_wrappers():
    from afcm_amd.torch_utils import custom_ops
    from afcm_amd.torch_utils.ops import bias_act as ba
    plugin = custom_ops.get_plugin('bias_act_plugin')
    x = torch.zeros([2, 3, 4], device='cuda')
    e = torch.empty([0], device='cuda')
    with pytest.raises(AssertionError):
        ba.bias_act(x, torch.zeros([4], device='cuda'), dim=1, act='lrelu')
    with pytest.raises(RuntimeError, match='same number of elements'):
        plugin.bias_act(x, torch.zeros([4], device='cuda'), e, e, e, 0, 1, R.INDEX['lrelu'], 0.2, 1.0, -1.0)
    with pytest.raises(RuntimeError, match='same dtype'):
        ba.bias_act(x, torch.zeros([3], device='cuda', dtype=torch.float16), dim=1, act='lrelu')
    with pytest.raises(RuntimeError, match='same dtype'):
        plugin.bias_act(x, torch.zeros([3], device='cuda', dtype=torch.bfloat16), e, e, e, 0, 1, R.INDEX['lrelu'], 0.2, 1.0, -1.0)
    with pytest.raises(KeyError):
        ba.bias_act(x, None, act='gelu')
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------------ (g)
NON_FINITE = [(R.LAYOUTS[0], F32), (R.LAYOUTS[0], F16), (R.LAYOUTS[0], BF16), (R.LAYOUTS[1], F32)]


@pytest.mark.parametrize('clamped', [False, True], ids=['free', 'clamp'])
@pytest.mark.parametrize('layout, dtype', NON_FINITE, ids=lambda v: v[0] if isinstance(v, tuple) else dtype_id(v))
@pytest.mark.parametrize('act', R.ACTS)
def test_non_finite_inputs_forward(act, layout, dtype, clamped):
    """NaN, +inf and -inf among finite neighbours, mode 0: the restatement with IEEE selections.  Without a clamp NaN stays NaN except
    for relu, which selects 0; with a clamp a NaN selects -clamp (relu: 0); infinities go to the activation's limit (times the gain,
    then clamped).  The NaN masks are equal, infinite results equal, and every finite element -- the neighbours in the same vector and
    in the next lane's -- is inside the bar.  The kernels agreed with the restatement and with the reference plugin's selections."""
    o = R.layout_operands(act, layout, dtype)
    x = o['x'].copy().reshape(-1)
    spots = {np.nan: [0, 13, 258, x.size - 1], np.inf: [5, 14, 1023, x.size - 2], -np.inf: [6, 15, 1024, x.size - 3]}
    for v, at in spots.items():
        x[at] = v
    x = x.reshape(o['x'].shape)
    clamp = o['clamp'] if clamped else None
    got = _check('g', 0, act, (x, o['b'], None, None, None), o['dim'], o['alpha'], o['gain'], clamp, dtype)
    flat = got.reshape(-1)
    if clamped:
        assert np.isfinite(flat).all() and (flat[spots[np.nan]] == (0.0 if act == 'relu' else -float(np.float32(clamp)))).all()
    else:
        assert (np.isnan(flat).sum() == (0 if act == 'relu' else 4)) and (np.isnan(flat[spots[np.nan]]).all() or act == 'relu')
