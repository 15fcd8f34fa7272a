"""The sign-reading filtered_lrelu kernels at every offset of the sign window (csrc/filtered_lrelu*.hip; the backward pass of the op).

Each kernel family has address arithmetic of its own for the window of 2-bit codes at (sx, sy): the wave kernels move every strip's
origin up by oy0 = -(m / down) output rows (m = sy mod 16), rebuild their constant fragments with rows moved by dshift = m % down,
select dword groups out where the window leaves the tensor and lean on the buffer descriptor for negative column blocks; the LDS-tile
kernels stage a window of row-quad bytes; the layout-0 kernels shift bytes by sx & 3.  The generator's four paddings reach 4 of the
48 (kernel case, sy mod 16) pairs, and a comparison of dx with autograd on the oracle has to allow for flipped leaky-ReLU branches
(relative L2 at 1.2 - 8 %), which a strip reading one row off passes.

Here every comparison is a max-abs over ALL elements of the result, no mask, against tests/flrelu_read_ref.read_reference driven
by the codes the kernel actually read, on the 16-bit-rounded input in float64: with the codes given the op is linear, so the bounds
are the project's forward bounds -- fp32 2e-5, matrix cores 6e-3 (f16) / 4e-2 (bf16), exact kernels on 16-bit data 4e-3 / 3e-2, all
x max(1, |ref|max).  tests/test_flrelu_read_ref_cpu.py shows on the CPU that each case below has teeth: the window moved by one row
or column, or one 16 x 16 block of codes read as 0, changes the reference by 5 bounds or more.

Measured on an MI355X, worst case of each family as a fraction of max(1, |ref|max), next to its bound:
    padding sweep (wave)      f16 6.8e-4 / 6e-3    bf16 5.1e-3 / 4e-2
    wave, direct calls        f16 6.4e-4 / 6e-3    bf16 9.4e-3 / 4e-2
    LDS-tile matrix cores     f16 8.1e-4 / 6e-3    bf16 9.9e-3 / 4e-2
    exact LDS tile, 16-bit    f16 4.7e-4 / 4e-3    bf16 3.3e-3 / 3e-2
    fp32: strip 2.9e-7, radial 2.7e-7, pointwise 7.1e-8, in-place activation 6.8e-8 / 2e-5
"""
import numpy as np
import pytest
import torch

import flrelu_read_ref as R

pytestmark = pytest.mark.gpu

SWEEP = R.sweep_cases()
MATRIX = R.matrix_core_cases()
LAYOUT0 = R.layout0_cases()
ACT = R.act_cases()

# every (read kernel, sy mod 16) pair of the wave kernels runs at least once
assert len({(c['read_kern'], c['my'] % 16) for c in SWEEP}) == 48

_filters = {}


def _f(name):
    """The filter as a device tensor, one per name: _mfma_workspace keys its cache on the tensors' addresses."""
    if name is None:
        return None
    if name not in _filters:
        _filters[name] = torch.from_numpy(R.filters()[name]).cuda()
    return _filters[name]


def _dev(a, dtype):
    return torch.from_numpy(a).to(getattr(torch, dtype)).cuda()


def _err(got, ref):
    """(max-abs error over all elements, allowed error / tol)."""
    got = got.detach().double().cpu().numpy()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max()), max(1.0, float(np.abs(ref).max()))


# ------------------------------------------------------------------------------------------------- a: padding sweep, public op
@pytest.mark.parametrize('case', SWEEP, ids=[c['id'] for c in SWEEP])
def test_wave_read_kernels_padding_sweep(case):
    """Forward through the public op (writes layout 2), autograd backward, dx against the reference on the decoded sign tensor:
    py0 = px0 = m + (fu taps - 1) - 16 k puts the backward's window at sy = sx = m (mod 16) for every m, so every
    (oy0, dshift) of flrelu_plan runs for every read kernel; plus px0 != py0, and heights that put rows = yh - oy0 on both sides of
    the 32- and 48-row thresholds (one 32-row strip, the 48-row strip reached through oy0 alone, two and three strips)."""
    from afcm_amd.torch_utils.ops import filtered_lrelu as flr
    S = R.sweep_setup(case)
    up, down, fu, fd = R.KERNELS[case['kern']]
    xg = _dev(S['x'], case['dtype']).requires_grad_(True)
    got = flr.filtered_lrelu(xg, fu=_f(fu), fd=_f(fd), b=None, up=up, down=down, padding=case['padding'], gain=R.GAIN, slope=R.SLOPE, clamp=R.CLAMP)
    assert got.grad_fn.sign_layout == 2, 'expected the wave-autonomous kernels'
    assert tuple(got.shape) == S['r'].shape
    si = got.grad_fn.saved_tensors[2].cpu().numpy()                      # (before the backward pass frees it)
    r = _dev(S['r'], case['dtype'])
    dx, = torch.autograd.grad((got.float() * r.float()).sum(), xg)
    codes = R.decode_codes(si, 2)
    assert (codes == 2).any() and (codes == 1).any(), 'the clamp must fire'
    ref = R.read_reference(S['r'], S['fd'], S['fu'], S['bcfg'], codes)
    err, scale = _err(dx, ref)
    print(f'{case["id"]}: sx, sy = {S["bcfg"][10]}, {S["bcfg"][11]}; plan (oy0, dshift, rows, toh, strips) = {R.read_plan(case)}; '
          f'dx max-abs {err:.3e}, bound {S["tol"] * scale:.3e}')
    assert err <= S['tol'] * scale, f'{case["id"]}: dx max-abs {err:.3e} > {S["tol"] * scale:.3e}'


# ------------------------------------------------------------------------------------------------- b, c: direct read calls
def _direct(case, run):
    """The offsets of one geometry: `run(dy, si, sx, sy)` -> result tensor; every offset is compared, the failures are reported
    together (which sx / sy residues fail is what locates a bug)."""
    S = R.direct_setup(case)
    dy = _dev(S['dy'], case['dtype'])
    s = R.encode_codes(S['codes'], case['layout'])
    assert tuple(s.shape[2:]) == R.sign_tensor_shape(case['layout'], case['rows'], case['cols'])
    codes = R.decode_codes(s, case['layout'])                             # what the tensor holds, padding included
    si = torch.from_numpy(s).cuda()
    bad, worst = [], 0.0
    for sx, sy, kind in case['offsets']:
        got = run(dy, si, sx, sy)
        ref = R.read_reference(S['dy'], S['fu'], S['fd'], R.direct_cfg(case, sx, sy), codes)
        if kind == 'outside':
            assert np.array_equal(ref, R.read_reference(S['dy'], S['fu'], S['fd'], R.direct_cfg(case, sx, sy), codes * 0))
        err, scale = _err(got, ref)
        worst = max(worst, err / scale)
        if not err <= case['tol'] * scale:
            bad.append((sx, sy, kind, f'{err:.3e} > {case["tol"] * scale:.3e}'))
    print(f'{case["id"]}: {len(case["offsets"])} offsets, worst max-abs / max(1, |ref|max) {worst:.3e}, bound {case["tol"]:.1e}')
    assert not bad, f'{case["id"]}: {len(bad)} of {len(case["offsets"])} offsets (sx, sy, kind, error): {bad}'


def _op(case):
    from afcm_amd.torch_utils.ops import filtered_lrelu as flr

    def run(dy, si, sx, sy):
        y, so, layout, _ = flr._run(dy, _f(case['fu']), _f(case['fd']), None, si, R.direct_cfg(case, sx, sy), False, no_fallback=True)
        assert so is None and layout == case['layout'] and y.dtype == dy.dtype
        return y
    return run


@pytest.mark.parametrize('case', MATRIX, ids=[c['id'] for c in MATRIX])
def test_matrix_core_read_kernels_window_offsets(case):
    """Wave (layout 2) and LDS-tile (layout 1) kernels on synthetic codes: sx and sy through all 16 residues, windows that start
    above / left of the tensor, run past its bottom / right edge, or lie wholly outside it (dx = the all-codes-0 result)."""
    _direct(case, _op(case))


@pytest.mark.parametrize('case', LAYOUT0, ids=[c['id'] for c in LAYOUT0])
def test_layout0_read_kernels_window_offsets(case):
    """The families that read row-major codes: the fp32 strip kernel (one and two row segments), the exact LDS-tile kernels on
    16-bit planes of odd width (both tile shapes of up 2 / down 2 and of up 2 / down 4), the two radial kinds, the pointwise kernel
    with padding; sx through every residue mod 4 with both signs."""
    _direct(case, _op(case))


@pytest.mark.parametrize('case', ACT, ids=[c['id'] for c in ACT])
def test_act_inplace_window_offsets(case):
    from afcm_amd.torch_utils.ops import filtered_lrelu as flr

    def run(dy, si, sx, sy):
        y = dy.clone()
        assert flr._act_inplace(y, si, sx, sy, R.GAIN, R.SLOPE, R.INF, False) is None
        return y
    _direct(case, run)


@pytest.mark.parametrize('kern', list(R.KERNELS))
def test_workspace_cache_keeps_row_residues_apart(kern):
    """_mfma_workspace keys the prepared fragments of a layout-2 read call on sy mod 16 (their rows move by dshift, their phase by
    oy0): calls that differ only in that residue must not share fragments, calls 16 rows apart may, and a repeat of the first call
    after the others returns the same bits."""
    case = next(c for c in MATRIX if c['name'] == f'wave-{kern}' and c['dtype'] == 'float16')
    run = _op(case)
    S = R.direct_setup(case)
    dy = _dev(S['dy'], case['dtype'])
    s = R.encode_codes(S['codes'], 2)
    codes, si = R.decode_codes(s, 2), torch.from_numpy(s).cuda()
    down = case['down']
    first = None
    for sy in (3, 3 + down + 1, 3 + 16, 2, 3):           # another dshift and oy0; the same residue 16 rows on; a neighbour; the repeat
        got = run(dy, si, 5, sy)
        err, scale = _err(got, R.read_reference(S['dy'], S['fu'], S['fd'], R.direct_cfg(case, 5, sy), codes))
        assert err <= case['tol'] * scale, f'{kern} sy {sy}: {err:.3e} > {case["tol"] * scale:.3e}'
        if first is None:
            first = got.clone()
    assert torch.equal(got, first), 'the repeated call must return the bits of the first'


def test_layout2_read_call_refuses_a_sign_tensor_of_another_shape():
    """The wave kernels take sh / 16 row groups and swb / 16 column blocks from the tensor's shape: afcm_filtered_lrelu refuses a
    layout-2 tensor that is no whole number of them on the host, before anything is launched."""
    from afcm_amd.torch_utils.ops import filtered_lrelu as flr
    case = next(c for c in MATRIX if c['id'] == 'wave-u2d2-float16')
    dy = torch.zeros(case['shape'], device='cuda', dtype=torch.float16)
    for sh, swb in ((17, 64), (16, 60), (24, 48)):
        si = torch.zeros([*case['shape'][:2], sh, swb], device='cuda', dtype=torch.uint8)
        with pytest.raises(RuntimeError, match='layout 2'):
            flr._run(dy, _f(case['fu']), _f(case['fd']), None, si, R.direct_cfg(case, 0, 0), False, no_fallback=True)
