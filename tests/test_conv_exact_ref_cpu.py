"""The exact conv2d tests' helper (conv_exact_ref.py) on a machine without a GPU: its float64 reference against the plain formulas,
the exactness conditions of every case in its tables, which kernel each case reaches (asked of the library's own plan queries, so a
case that changes family after a dispatch change fails here) and the teeth of the forward cases."""
import os

import pytest
import torch
import torch.nn.functional as F

import conv_exact_ref as R

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
HALVES = [BF16, F16]


@pytest.fixture(scope='module')
def lib():
    from afcm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def _plain(node):
    """(y, dx, dw, ds, dd, dxs) of a node from the written-out formulas (transposed conv, weight-gradient contraction, plane sums)."""
    x, w, s, d, b, dy, pad, st = node.x, node.w, node.s, node.d, node.b, node.dy, node.pad, node.stride
    xs = x if s is None else x * s[:, :, None, None]
    c = F.conv2d(xs, w, padding=pad, stride=st)
    y = c if d is None else c * d[:, :, None, None]
    if b is not None:
        y = y + b[None, :, None, None]
    dys = dy if d is None else dy * d[:, :, None, None]
    oh, ow = x.shape[2] - ((y.shape[2] - 1) * st - 2 * pad + w.shape[2]), x.shape[3] - ((y.shape[3] - 1) * st - 2 * pad + w.shape[3])
    dxs = F.conv_transpose2d(dys, w, padding=pad, stride=st, output_padding=(oh, ow))
    dx = dxs if s is None else dxs * s[:, :, None, None]
    dw = torch.nn.grad.conv2d_weight(xs, w.shape, dys, stride=st, padding=pad)
    ds = None if s is None else (x * dxs).sum([2, 3])
    dd = None if d is None else (dy * c).sum([2, 3])
    return y, dx, dw, ds, dd, dxs


def _same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.shape == b.shape and torch.equal(a, b), what


NODE_CASES = ([(c.shape, c.kind, 3, 1) for c in R.FWD16 if c.shape[0] is not None and c.shape[0] * c.shape[3] * c.shape[4] < 20000]
              + [(c.shape, c.kind, 1, 1) for c in R.FWD16_1X1] + [(s, 'small', 3, 1) for s in R.NODES] + [(s, k, 3, 2) for s, k in R.STRIDE2])


@pytest.mark.parametrize('shape,kind,ks,stride', NODE_CASES, ids=R.case_id)
def test_reference_equals_the_plain_formulas(shape, kind, ks, stride):
    """Everything is an integer below 2^53 in float64, so autograd and the written-out formulas agree bit for bit."""
    st = R.ladder(kind, F16)[0]
    node = R.draw_node(shape, st, 3, ks=ks, stride=stride, scales=stride == 1, bias=stride == 1)
    y, dx, dw, ds, dd, dxs = _plain(node)
    for a, b, what in ((node.y, y, 'y'), (node.dx, dx, 'dx'), (node.dw, dw, 'dw'), (node.ds, ds, 'ds'), (node.dd, dd, 'dd'), (node.dxs, dxs, 'dxs')):
        _same(a, b, what)
    v = node.forward_variants()
    assert torch.equal(v[(stride == 1, stride == 1)], node.y)
    assert torch.equal(v[(False, False)], R.conv_ref(node.x, node.w, node.s, None, None, node.pad, stride))


def test_r1_reference_equals_the_transposed_conv_formula():
    n, cin, cout, h, w, pad = R.R1_CASE
    g = R.gen(1)
    x, wt = R.pick([n, cin, h, w], (-2, -1, 1, 2), g), R.pick([cout, cin, 3, 3], (-1, 1), g)
    dy = R.pm1([n, cout, h + 2 * pad - 2, w + 2 * pad - 2], g)
    dx, gw = R.r1_ref(x, wt, dy, pad)
    wr = wt.clone().requires_grad_(True)
    dx2 = F.conv_transpose2d(dy, wr, padding=pad)
    gw2, = torch.autograd.grad(dx2.square().sum(), wr)
    assert torch.equal(dx, dx2.detach()) and torch.equal(gw, gw2)


def test_helpers():
    t = torch.tensor([257.0, 1.0], dtype=torch.float64)
    assert R.representable(t, F16) and not R.representable(t, BF16)
    assert R.quantum(torch.tensor([0.75, 2.0], dtype=torch.float64)) == 0.25 and R.quantum(torch.tensor([6.0, -2.0], dtype=torch.float64)) == 2.0
    a, b = torch.tensor([1.0, 2.0]), torch.tensor([1.0, 3.0])
    assert R.mismatch(a, a.double()) is None and '1 of 2' in R.mismatch(a, b.double(), 'y') and '(1,)' in R.mismatch(a, b.double())
    node = R.draw_node((1, 2, 3, 4, 6, 1), dict(x=(1000.0,), w=(1,), s=(0,), d=(0,), b=(1,), dy=(1,)), 0)
    assert any('not representable' in f for f in node.failures(BF16)) and not node.failures(F32)
    node = R.draw_node((1, 2, 3, 4, 6, 1), dict(x=(2.0 ** 12,), w=(2.0 ** 12 + 1,), s=(0,), d=(0,), b=(1,), dy=(1,)), 0)
    assert any('2^24' in f for f in node.failures(F32))


# ---- the exactness conditions of every case ---------------------------------------------------------------------------------------
def _forward_cases():
    for dt in HALVES:
        for c in R.FWD16 + R.PITCHED16:
            yield c, dt, 3, False
        for c in R.FWD16_1X1:
            yield c, dt, 1, False
    for c in R.FWD32_SPLIT + R.FWD32_NATIVE:
        yield c, F32, 3, True
    for c in R.FWD32_NATIVE_1X1:
        yield c, F32, 1, True


@pytest.mark.parametrize('case,dtype,ks,in_scale', list(_forward_cases()), ids=R.case_id)
def test_forward_cases_are_exact_and_have_teeth(case, dtype, ks, in_scale):
    shape = R.shape_at_256(case)
    node = R.forward_node(shape, case, dtype, ks, in_scale=in_scale, bias=not in_scale)
    node.check(dtype, ('y',))
    # teeth: without one tap of one input channel every interior pixel of every output plane changes (a non-zero activation times a
    # non-zero weight, scaled by a power of two) -- and for +-1 operands any single dropped term flips the sum's parity
    assert bool((node.x != 0).all()) and bool((node.w != 0).all())
    w2 = node.w.clone()
    w2[:, shape[1] // 2, ks // 2, 0] = 0
    sl = slice(0, min(shape[0], 2))
    full = R.conv_ref(node.x[sl], node.w, None if node.s is None else node.s[sl], None if node.d is None else node.d[sl], node.b, node.pad)
    cut = R.conv_ref(node.x[sl], w2, None if node.s is None else node.s[sl], None if node.d is None else node.d[sl], node.b, node.pad)
    assert torch.equal(full, node.y[sl])
    m = 2 if ks == 3 else 0
    assert bool((full != cut)[:, :, m:full.shape[2] - m, m:full.shape[3] - m].all())
    if case.kind == 'pm1':
        assert bool((node.c % 2 == (shape[1] * ks * ks) % 2)[:, :, m:node.c.shape[2] - m, m:node.c.shape[3] - m].all())


@pytest.mark.parametrize('dtype', HALVES + [F32], ids=str)
def test_gradient_cases_are_exact(dtype):
    if dtype != F32:
        for c in R.FWD16_1X1:
            R.onebyone_node(c, dtype).check(dtype, ('y', 'dx'))
        for c in R.WGRAD16_GRANULE + R.WGRAD16_DWORD:
            R.wgrad_node(c, dtype).check(dtype, ('dw',))
        for shape in R.WGRAD_DOTS + [R.WGRAD_DOTS_NONE]:
            R.dots_node(shape, dtype).check(dtype, ('dx', 'dw'))
        for shape, kind in R.STRIDE2:
            R.stride2_node(shape, kind, dtype).check(dtype, ('y', 'dx', 'dw'))
    else:
        for c in R.WGRAD32:
            R.wgrad_node(c, dtype).check(dtype, ('dw',))
    for shape in R.NODES:
        node = R.full_node(shape, dtype)
        node.check(dtype)
        assert len(set(node.s.flatten().tolist())) > 1 and len(set(node.d.flatten().tolist())) > 1


# ---- coverage: which kernel each case reaches, from the library's own plan -----------------------------------------------------------
def test_conv_cases_reach_every_family(lib):
    reached = set()
    # one round of the 64-row persistent launch: 3 workgroups per compute unit of the device, or of 256 units where there is none
    one_round = R.conv_plan(lib, F16, 256, 8, 16, 126, 126, 3, 2).grid
    for dt in HALVES:
        for c in R.FWD16:
            shape = R.with_batch(lib, c, dt)
            if one_round == 768:
                assert shape == R.shape_at_256(c)
            pl = R.conv_plan(lib, dt, *shape[:5], 3, shape[5])
            assert (pl.family, pl.fast) == (c.family, c.fast), (c, pl)
            assert pl.kernel == (R.K_DIRECT if c.family == R.DIRECT else R.K_X16)
            if c.shape[0] is None:
                assert pl.items > pl.grid and pl.items % pl.grid != 0, (c, pl)
                assert pl.grid % 8 == 0 and (pl.grid == one_round or c.family == R.ROWS96)
            elif c.family != R.DIRECT:
                assert pl.items <= pl.grid
            reached.add(('x16', pl.family, pl.rows, pl.fast, 'second round' if c.shape[0] is None else 'one round'))
        for c in R.PITCHED16:
            n, cin, cout, h, w, pad = c.shape
            ld = (w + 2 * pad - 2 + 31) // 32 * 32
            pl = R.conv_plan(lib, dt, n, cin, cout, h, w, 3, pad, x_pitch=(w + 31) // 32 * 32 + 32, y_pitch=ld)
            assert ld != w + 2 * pad - 2 and (pl.family, pl.fast) == (c.family, c.fast), (c, pl)
            reached.add(('pitched', pl.fast))
        for c in R.FWD16_1X1:
            pl = R.conv_plan(lib, dt, *c.shape[:5], 1, 0)
            assert (pl.family, pl.kernel) == (c.family, R.K_GENERAL16), (c, pl)
            reached.add(('1x1', pl.rows))
            n, cin, cout, h, w, _ = c.shape                     # the data gradient: channels swapped
            reached.add(('1x1', R.conv_plan(lib, dt, n, cout, cin, h, w, 1, 0).rows))
        for c in R.FWD32_SPLIT:
            shape = R.with_batch(lib, c, dt, split=True)
            pl = R.conv_plan(lib, dt, *shape[:5], 3, shape[5], split=True)
            assert (pl.family, pl.kernel, pl.fast) == (c.family, R.K_SPLIT, 0), (c, pl)
            reached.add(('split', pl.family, 'second round' if pl.items > pl.grid else 'one round'))
    for c in R.FWD32_NATIVE + R.FWD32_NATIVE_1X1:
        ks = 1 if c in R.FWD32_NATIVE_1X1 else 3
        pl = R.conv_plan(lib, F32, *c.shape[:5], ks, c.shape[5])
        assert (pl.family, pl.kernel) == (c.family, R.K_F32), (c, pl)
        reached.add(('fp32', ks, pl.rows))
    want = {('x16', R.ROWS64, 64, 0, 'one round'), ('x16', R.ROWS64, 64, 1, 'one round'), ('x16', R.ROWS64, 64, 0, 'second round'),
            ('x16', R.ROWS64, 64, 1, 'second round'), ('x16', R.ROWS96, 96, 1, 'second round'), ('x16', R.ROWS96, 96, 0, 'one round'),
            ('x16', R.ROWS128, 128, 1, 'one round'), ('x16', R.ROWS128_64, 64, 0, 'one round'), ('x16', R.DIRECT, 64, 0, 'one round'),
            ('pitched', 0), ('pitched', 1), ('1x1', 64), ('1x1', 128), ('split', R.ROWS64, 'one round'), ('split', R.ROWS64, 'second round'),
            ('fp32', 3, 64), ('fp32', 3, 128), ('fp32', 1, 128)}
    assert want <= reached, sorted(want - reached, key=str)


def test_wgrad_cases_reach_every_kernel_and_reduction(lib):
    reached = set()
    for dt in HALVES:
        for c in R.WGRAD16_GRANULE:
            pl = R.wgrad_plan(lib, dt, *c.shape[:5], c.ks, c.shape[5])
            assert (pl.kernel, pl.x16, pl.small) == (R.WG_GRANULE, c.x16, 1), (c, pl)
            q_last = (c.shape[4] + 2 * c.shape[5] - c.ks + 1) % 64
            assert (32 < q_last <= 48) == (c.x16 == 0)
            reached.add(('granule', c.ks, pl.x16))
            reached.add(('reduce', pl.reduce))
        for c in R.WGRAD16_DWORD:
            pl = R.wgrad_plan(lib, dt, *c.shape[:5], 3, c.shape[5])
            assert (pl.kernel, pl.pad_odd) == (R.WG_DWORD, c.shape[5]), (c, pl)
            reached.add(('dword', pl.pad_odd))
            reached.add(('reduce', pl.reduce))
            if c.shape[5] == 1:                                  # at its default the same inputs are framed: a pad-2 granule gradient
                n, cin, cout, h, w, _ = c.shape
                assert R.wgrad_plan(lib, dt, n, cin, cout, h, w, 3, 2).kernel == R.WG_GRANULE
        for shape in R.WGRAD_DOTS:
            pl = R.wgrad_plan(lib, dt, *shape[:5], 3, shape[5], dots=True)
            assert pl is not None and pl.reduce == R.RED_DOTS and pl.splits_img * shape[0] == pl.splits, (shape, pl)
            reached.add(('reduce', pl.reduce))
        assert R.wgrad_plan(lib, dt, *R.WGRAD_DOTS_NONE[:5], 3, 2, dots=True) is None
    for c in R.WGRAD32:
        pl = R.wgrad_plan(lib, F32, *c.shape[:5], c.ks, c.shape[5])
        assert pl.kernel == R.WG_F32
        reached.add(('fp32', c.ks, pl.pad_odd))
    # one case each for split counts < 8, 8..63 and >= 64, and the scalar reduction's 315 elements
    picks = {R.RED4_256: (2, 64, 64, 6, 18, 0), R.RED4_64: (2, 64, 64, 6, 14, 2), R.RED4_16: (4, 64, 1, 32, 256, 0), R.RED_SCALAR: (1, 5, 7, 6, 14, 2)}
    for red, shape in picks.items():
        ks = 1 if shape[2] == 1 else 3
        pl = R.wgrad_plan(lib, F16, *shape[:5], ks, shape[5])
        lo, hi = {R.RED4_256: (1, 7), R.RED4_64: (8, 63), R.RED4_16: (64, 1 << 30), R.RED_SCALAR: (1, 1 << 30)}[red]
        assert pl.reduce == red and lo <= pl.splits <= hi, (shape, pl)
        assert any(tuple(c.shape) == shape for c in R.WGRAD16_GRANULE + R.WGRAD16_DWORD)
    assert (5 * 7 * 9) % 4 != 0
    want = {('granule', 3, 1), ('granule', 3, 0), ('granule', 1, 1), ('dword', 0), ('dword', 1), ('fp32', 3, 0), ('fp32', 3, 1), ('fp32', 1, 0),
            ('reduce', R.RED_SCALAR), ('reduce', R.RED4_256), ('reduce', R.RED4_64), ('reduce', R.RED4_16), ('reduce', R.RED_DOTS)}
    assert want <= reached, sorted(want - reached, key=str)


def test_plan_queries_are_pure_host_and_check_their_arguments(lib):
    from afcm_amd import _lib
    import ctypes
    out = (ctypes.c_int32 * 8)()
    assert lib.afcm_conv2d_plan(1, 2, 8, 64, 30, 46, 3, 3, 0, 0, 0, out) == _lib.E_INVALID and b'padding' in lib.afcm_last_error()
    assert lib.afcm_conv2d_plan(0, 2, 8, 64, 30, 46, 3, 1, 0, 0, 1, out) == _lib.E_INVALID
    assert lib.afcm_conv2d_wgrad_plan(1, 2, 8, 64, 30, 46, 2, 0, 0, 0, 0, out) == _lib.E_INVALID
    # the 181-channel layers: 128 + 64 rows forward, and the data gradient of a 64 -> 91 layer on 96-row blocks
    assert R.conv_plan(lib, BF16, 2, 64, 181, 36, 36, 3, 2).family == R.ROWS128_64
    assert R.conv_plan(lib, BF16, 2, 64, 91, 36, 36, 3, 2).family == R.ROWS96
