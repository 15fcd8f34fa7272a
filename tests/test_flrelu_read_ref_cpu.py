"""CPU tests of tests/flrelu_read_ref.py: the byte layouts round-trip, the given-codes reference reproduces float64 autograd on the
oracle, and every parametrization of tests/test_gpu_flrelu_sign_window.py has teeth -- a sign window misplaced by one row or one
column, or one 16 x 16 block of codes read as 0, moves the reference by at least 5x the error that GPU test allows.  The last
is what makes the GPU bounds meaningful, and it needs no GPU."""
import numpy as np
import pytest
import torch

import flrelu_read_ref as R


# ------------------------------------------------------------------------------------------------- layouts
@pytest.mark.parametrize('layout', [0, 1, 2])
@pytest.mark.parametrize('rows,cols', [(1, 1), (7, 13), (66, 35), (131, 97), (64, 64), (65, 17)])
def test_layouts_round_trip(layout, rows, cols):
    rng = np.random.default_rng(rows * 1000 + cols)
    codes = rng.integers(0, 4, size=(2, 3, rows, cols)).astype(np.uint8)
    s = R.encode_codes(codes, layout)
    assert s.dtype == np.uint8 and tuple(s.shape[2:]) == R.sign_tensor_shape(layout, rows, cols)
    back = R.decode_codes(s, layout)
    assert np.array_equal(back[:, :, :rows, :cols], codes)
    back[:, :, :rows, :cols] = 0
    assert not back.any(), 'padding must decode to code 0'
    assert np.array_equal(R.encode_codes(R.decode_codes(s, layout), layout), s)


def test_layout_byte_addresses():
    """The encoders against the address formulas of the kernels' comments, element by element."""
    rng = np.random.default_rng(1)
    rows, cols = 133, 41
    codes = rng.integers(0, 4, size=(1, 1, rows, cols)).astype(np.uint8)
    s0, s1, s2 = (R.encode_codes(codes, k)[0, 0] for k in (0, 1, 2))
    nV4 = s2.shape[0] // 16
    flat2 = s2.reshape(-1)
    for y in range(rows):
        for x in range(cols):
            want = int(codes[0, 0, y, x])
            assert (int(s0[y, x >> 2]) >> (2 * (x & 3))) & 3 == want                      # SG3OPS/filtered_lrelu.cpp:87-94
            q = y >> 2
            assert (int(s1[q, x]) >> (2 * (y & 3))) & 3 == want                           # csrc/filtered_lrelu_mfma.hip
            V, gq = q >> 2, q & 3
            addr = ((((x >> 4) * nV4 + (V >> 2)) * 4 + gq) * 16 + (x & 15)) * 4 + (V & 3)   # csrc/filtered_lrelu_wave.hip
            assert (int(flat2[addr]) >> (2 * (y & 3))) & 3 == want


def test_window_codes_edges():
    codes = np.arange(1, 13, dtype=np.uint8).reshape(1, 1, 3, 4) % 4
    w = R.window_codes(codes, 5, 6, -1, -2)
    for y in range(5):
        for x in range(6):
            yy, xx = y - 2, x - 1
            want = codes[0, 0, yy, xx] if 0 <= yy < 3 and 0 <= xx < 4 else 0
            assert w[0, 0, y, x] == want
    assert not R.window_codes(codes, 5, 6, 4, 0).any() and not R.window_codes(codes, 5, 6, 0, -5).any()


@pytest.mark.parametrize('up,fu,pad', [(2, 'f12', [9, 8, 9, 8]), (2, 'f12', [-5, -2, 0, -7]), (2, 'f12', [13, 30, -1, 12]), (4, 'f24u', [-6, -9, -3, 40]),
                                       (4, 'f24u', [21, 20, 35, -11]), (1, 'f12', [6, 5, 7, -3]), (3, 'f24', [1, 2, -4, 31])])
@pytest.mark.parametrize('flip', [False, True])
def test_upsample_fir_is_the_definition(up, fu, pad, flip):
    """The zero-skipping up-FIR of read_reference against oracle.direct_np.upfirdn2d (odd sizes, crops on either side)."""
    from oracle import direct_np as dnp
    x = np.random.default_rng(up).standard_normal((1, 2, 11, 14))
    f = R.filters()[fu]
    want = dnp.upfirdn2d(x, f, up=up, padding=pad, gain=float(up * up), flip_filter=flip)
    got = R.upsample_fir(x, f, up, pad, flip)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-13


# ------------------------------------------------------------------------------------------------- reference vs autograd
def _autograd_dx(x, fu, fd, r, cfg):
    from oracle import aten_ops as ops
    up, down, px0, px1, py0, py1, gain, slope, clamp, flip = cfg[:10]
    xs = torch.from_numpy(x).double().requires_grad_(True)
    y = ops.filtered_lrelu(xs, fu=torch.from_numpy(np.asarray(fu)).double(), fd=torch.from_numpy(np.asarray(fd)).double(), b=None, up=up, down=down,
                           padding=[px0, px1, py0, py1], gain=gain, slope=slope, clamp=clamp, flip_filter=flip)
    assert tuple(y.shape) == r.shape
    gx, = torch.autograd.grad((y * torch.from_numpy(r)).sum(), xs)
    return gx.numpy()


def _given_codes_dx(x, fu, fd, r, cfg):
    """dx of sum(y * r) by the sign-reading reference: definition-level codes of the forward, configuration of _backward_cfg."""
    from afcm_amd.torch_utils.ops import filtered_lrelu as flr
    from oracle import direct_np as dnp
    up, down, px0, px1, py0, py1, gain, slope, clamp, flip = cfg[:10]
    u = dnp.upfirdn2d(x, fu, up=up, padding=[px0, px1, py0, py1], gain=float(up * up), flip_filter=flip)
    _, codes = dnp.lrelu_codes(u, gain, slope, clamp)
    bcfg = flr._backward_cfg(cfg, torch.from_numpy(np.asarray(fu)), torch.from_numpy(np.asarray(fd)), x.shape, r.shape, 0)
    return R.read_reference(r, fd, fu, bcfg, codes), codes, bcfg


@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('m', range(16))
@pytest.mark.parametrize('kern', list(R.KERNELS))
def test_reference_matches_autograd(kern, m, flip):
    case = R.sweep_case(kern, m, (m + 5) % 16 if flip else m)
    S = R.sweep_setup(case)
    cfg = S['cfg'][:9] + (flip,) + S['cfg'][10:]
    want = _autograd_dx(S['x'], S['fu'], S['fd'], S['r'], cfg)
    got, codes, bcfg = _given_codes_dx(S['x'], S['fu'], S['fd'], S['r'], cfg)
    assert (codes == 2).any() and (codes == 1).any() and (codes == 0).any(), 'the clamp must fire'
    assert bcfg[11] % 16 == case['my'] % 16 and bcfg[10] % 16 == case['mx'] % 16
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12, np.abs(got - want).max()


@pytest.mark.parametrize('kind', ['sufd', 'fusd'])
def test_reference_matches_autograd_2d_filters(kind):
    """One forward of each radial kind: separable up with the 12 x 12 down filter, and the 12 x 12 filter up with separable down."""
    F = R.filters()
    fu, fd = (F['f12'], F['r12']) if kind == 'sufd' else (F['r12'], F['f12'])
    rng = np.random.default_rng(4)
    x = rng.standard_normal((1, 2, 13, 17)) * 4.0
    cfg = (2, 2, 9, 8, 7, 10, R.GAIN, R.SLOPE, 0.5, kind == 'fusd', 0, 0, 0)
    yh, yw = R.out_size(13, 2, 2, 7, 10, 12, 12), R.out_size(17, 2, 2, 9, 8, 12, 12)
    r = rng.standard_normal((1, 2, yh, yw))
    want = _autograd_dx(x, fu, fd, r, cfg)
    got, codes, _ = _given_codes_dx(x, fu, fd, r, cfg)
    assert (codes == 2).any()
    assert np.abs(got - want).max() <= 1e-12, np.abs(got - want).max()


# ------------------------------------------------------------------------------------------------- coverage of the GPU parametrization
SWEEP = R.sweep_cases()
DIRECT = R.matrix_core_cases() + R.layout0_cases() + R.act_cases()


def test_sweep_reaches_every_kernel_case_and_row_residue():
    pairs = {(c['read_kern'], c['my'] % 16) for c in SWEEP}
    assert len(pairs) == 48
    assert {(c['read_kern'], c['mx'] % 16) for c in SWEEP} == pairs
    for c in SWEEP:
        up, down = R.KERNELS[c['kern']][:2]
        assert c['padding'][2] % 16 == (c['my'] + 12 * (up // 2) - 1) % 16         # sy = py0 - (fu taps - 1), fu taps = 12 up / 2
        F = R.filters()
        fu, fd = R.KERNELS[c['kern']][2:]
        yw = R.out_size(c['w'], up, down, c['padding'][0], c['padding'][1], len(F[fu]), len(F[fd]))
        assert yw % 2 == 0 and c['w'] % 2 == 0 and 4 <= yw <= 30
    # bf16: every dshift of every read kernel
    assert {(c['read_kern'], R.read_plan(c)[1]) for c in SWEEP if c['dtype'] == 'bfloat16'} == \
        {('u2d2', 0), ('u2d2', 1), ('u4d2', 0), ('u4d2', 1), ('u2d4', 0), ('u2d4', 1), ('u2d4', 2), ('u2d4', 3)}
    assert sum(c['mx'] != c['my'] and c['h'] == 20 for c in SWEEP) == 9


def test_sweep_heights_reach_every_strip_count():
    """rows = yh - oy0 of the read call on both sides of the 32- and 48-row thresholds of flrelu_plan."""
    got = {k: set() for k in R.KERNELS}
    for c in SWEEP:
        oy0, _, rows, toh, strips = R.read_plan(c)
        got[c['read_kern']].add((rows, toh, strips))
        if rows == 33 and c['read_kern'] == 'u2d2':
            assert c['h'] <= 32 and oy0 < 0, 'the 48-row strip reached only because oy0 < 0'
    assert {(32, 32, 1), (33, 48, 1), (48, 48, 1), (49, 32, 2), (72, 32, 3)} <= got['u2d2']
    for k in ('u4d2', 'u2d4'):
        assert {(32, 32, 1), (33, 32, 2), (64, 32, 2), (71, 32, 3)} <= got[k]


def test_direct_calls_cover_the_offsets_and_plan_thresholds():
    ids = [c['id'] for c in DIRECT]
    assert len(set(ids)) == len(ids)
    for c in DIRECT:
        sxs = [o[0] for o in c['offsets']]
        sys_ = [o[1] for o in c['offsets']]
        if c['layout'] == 0:
            assert {s % 4 for s in sxs if s > 0} == {0, 1, 2, 3} and {s % 4 for s in sxs if s < 0} == {0, 1, 2, 3}
        else:
            assert {s % 16 for s in sxs} == set(range(16))
            assert c['yw'] % 2 == 0 and c['shape'][3] % 2 == 0
        assert {s % 16 for s in sys_} == set(range(16))
        assert c['shape'][0] * c['shape'][1] <= 4
        kinds = {o[2] for o in c['offsets']}
        if c['dtype'] == 'bfloat16':
            assert kinds == {'sx', 'sy'}               # (flrelu_read_ref.direct_case: the float16 twin carries the other windows)
            assert c['id'].replace('bfloat16', 'float16') in ids or c['family'] == 'act'
            continue
        assert {'above', 'left', 'below', 'right', 'outside'} <= kinds
        sx, sy, _ = next(o for o in c['offsets'] if o[2] == 'outside')
        assert sx >= 4 * R.sign_tensor_shape(0, c['rows'], c['cols'])[1], 'wholly outside the tensor, padding included'
    by = {c['id']: c for c in DIRECT}
    # fp32 strip kernel: one segment (yh <= 96) and two ((yh + 48) / 96)
    for k in R.KERNELS:
        assert by[f'strip-{k}-float32']['yh'] <= 96
    assert all(by[i]['yh'] >= 144 for i in ('strip-u2d2-tall-float32', 'strip-u4d2-tall-float32', 'strip-u2d4-tall-float32'))
    for d in ('float16', 'bfloat16'):
        assert by[f'tile-u2d2-yh38-{d}']['yh'] <= 40 < by[f'tile-u2d2-yh70-{d}']['yh']          # 20- / 35-row tiles
        assert by[f'tile-u2d4-yw9-{d}']['yw'] <= 40 < by[f'tile-u2d4-yw41-{d}']['yw']           # 16- / 32-column tiles
        for i in ('tile-u2d2-yh38', 'tile-u2d2-yh70', 'tile-u2d4-yw9', 'tile-u2d4-yw41', 'tile-u4d2'):
            assert by[f'{i}-{d}']['shape'][3] % 2 == 1, 'odd widths: no matrix-core case'
        # matrix cores: more than two strips (32 rows) / tiles
        assert by[f'wave-u2d2-tall70-{d}']['yh'] > 64 and by[f'mfma_tile-u2d2-tall70-{d}']['yh'] > 64


# ------------------------------------------------------------------------------------------------- teeth
def _moved(ref, other, allowed):
    return np.abs(other - ref).max() / allowed


@pytest.mark.parametrize('case', SWEEP, ids=[c['id'] for c in SWEEP])
def test_teeth_sweep(case):
    from oracle import direct_np as dnp
    S = R.sweep_setup(case)
    up, down, px0, px1, py0, py1 = S['cfg'][:6]
    u = dnp.upfirdn2d(S['x'], S['fu'], up=up, padding=[px0, px1, py0, py1], gain=float(up * up))
    _, codes = dnp.lrelu_codes(u, R.GAIN, R.SLOPE, R.CLAMP)
    b = S['bcfg']
    ref = R.read_reference(S['r'], S['fd'], S['fu'], b, codes)
    assert ref.shape == S['x'].shape
    allowed = S['tol'] * max(1.0, np.abs(ref).max())
    sx, sy = b[10], b[11]
    assert _moved(ref, R.read_reference(S['r'], S['fd'], S['fu'], b[:11] + (sy + 1,) + b[12:], codes), allowed) >= R.TEETH
    assert _moved(ref, R.read_reference(S['r'], S['fd'], S['fu'], b[:10] + (sx + 1,) + b[11:], codes), allowed) >= R.TEETH
    urows, ucols = R.upsampled_grid(S['r'].shape, b, S['fd'])
    z = R.zero_block(codes, sx, sy, urows, ucols)
    assert _moved(ref, R.read_reference(S['r'], S['fd'], S['fu'], b, z), allowed) >= R.TEETH


@pytest.mark.parametrize('case', DIRECT, ids=[c['id'] for c in DIRECT])
def test_teeth_direct(case):
    S = R.direct_setup(case)
    weak = []
    for sx, sy, kind in case['offsets']:
        ref = R.read_reference(S['dy'], S['fu'], S['fd'], R.direct_cfg(case, sx, sy), S['codes'])
        allowed = case['tol'] * max(1.0, np.abs(ref).max())
        if kind == 'outside':
            # no code is read: the result is the all-codes-0 one, and its teeth are that the codes of ANY window inside move it
            assert np.array_equal(ref, R.read_reference(S['dy'], S['fu'], S['fd'], R.direct_cfg(case, sx, sy), S['codes'] * 0))
            other = R.read_reference(S['dy'], S['fu'], S['fd'], R.direct_cfg(case, 0, sy), S['codes'])
            if _moved(ref, other, allowed) < R.TEETH:
                weak.append((sx, sy, kind, 'inside'))
            continue
        for what, other in (('sy+1', R.read_reference(S['dy'], S['fu'], S['fd'], R.direct_cfg(case, sx, sy + 1), S['codes'])),
                            ('sx+1', R.read_reference(S['dy'], S['fu'], S['fd'], R.direct_cfg(case, sx + 1, sy), S['codes'])),
                            ('block', R.read_reference(S['dy'], S['fu'], S['fd'], R.direct_cfg(case, sx, sy),
                                                       R.zero_block(S['codes'], sx, sy, case['urows'], case['ucols'])))):
            f = _moved(ref, other, allowed)
            if f < R.TEETH:
                weak.append((sx, sy, kind, what, round(f, 2)))
    assert not weak, weak
