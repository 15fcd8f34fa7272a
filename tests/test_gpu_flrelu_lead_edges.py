"""The wave filtered_lrelu kernels where their early requests point outside the plane (csrc/filtered_lrelu_wave.hip).

A strip asks for its input pieces two column groups ahead, for its skip rows a group ahead and -- the aligned sign-reading
up-2 / down-2 kernels -- for its codes two groups ahead; a piece that crosses the plane's left or right edge is asked for by whole 16-byte
loads (lanes outside the row beyond the descriptor, a lane across column 0 from the row's start) and put right when it is parked.
On the workload's planes nearly all of those requests land inside the plane; here
nearly none do: planes narrower than one 32-column piece, of one to three column groups, of fewer rows than a strip, skip operands of
one to three column-block pairs, operands that sit in NaN and that end where their allocation ends.  Every request past an edge has to be
dropped by the plane's buffer descriptor and nothing requested early may reach a result.

Bars: those of tests/test_gpu_flrelu_wave.py (fraction of max(1, |ref|max): 6e-3 float16, 4e-2 bfloat16) against oracle/aten_ops
(forward) and the float64 reference with the codes given of tests/flrelu_read_ref.py (sign-reading call), plus bit-for-bit equality
between a call on operands embedded in NaN and the same call on compact copies."""
import numpy as np
import pytest
import torch

import flrelu_read_ref as R
from flrelu_read_ref import geometry as _geometry

pytestmark = pytest.mark.gpu

DTYPES = [('float16', R.TOL_MATRIX['float16']), ('bfloat16', R.TOL_MATRIX['bfloat16'])]


def _in_nan(t, pitched):
    """`t` as a view into a larger buffer that holds NaN (0xff for the uint8 sign tensor) everywhere else: in front of the first plane,
    behind the last one and, `pitched`, in the padding of every row (as _pitched of tests/test_gpu_row_pitch.py)."""
    from afcm_amd.torch_utils.ops import _rows
    n, c, h, w = t.shape
    ld = (w + 31) // 32 * 32 + 32 if pitched else w
    front, back = 2 * ld + 64, 3 * ld + 40
    fill = 0xff if t.dtype == torch.uint8 else float('nan')
    buf = torch.full([front + n * c * h * ld + back], fill, dtype=t.dtype, device=t.device)
    v = buf[front:front + n * c * h * ld].view(n, c, h, ld)[..., :w]
    v.copy_(t)
    assert _rows.pitch_of(v) == ld and v.is_contiguous() == (not pitched)
    return v


def _forward_ref(x, skip, osc, kern, padding, clamp):
    from oracle import aten_ops as ops
    up, down, fu, fd = R.KERNELS[kern]
    F = R.filters()
    ref = ops.filtered_lrelu(x.float().cpu(), fu=torch.from_numpy(F[fu]), fd=torch.from_numpy(F[fd]), b=None, up=up, down=down, padding=padding,
                             gain=R.GAIN, slope=R.SLOPE, clamp=clamp)
    if skip is not None:
        ref = ref + skip.float().cpu()
    if osc is not None:
        ref = ref * osc.cpu().reshape(ref.shape[0], ref.shape[1], 1, 1)
    return ref


def _close(got, want, tol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.isfinite(got).all(), f'{what}: not finite'
    err = np.abs(got - want).max()
    assert err <= tol * max(1.0, np.abs(want).max()), f'{what}: max-abs {err:.3e}'


def _setup(kern, yh, yw, dtype, seed):
    up, down, fu, fd = R.KERNELS[kern]
    F = R.filters()
    # (mx by width: px0 = 0 / 8 / 4 for up 2, -4 / 4 / 0 for up 4 -- the first piece starts at column 0, 4 or 2 columns left of it (its first
    # lane straddles column 0 by 2 or 1 dwords), or inside the plane)
    h, w, padding = _geometry(kern, yh, yw, mx={20: 13, 36: 9, 52: 13}.get(yw, 5))
    cfg = (up, down, *padding, R.GAIN, R.SLOPE, R.CLAMP, False, 0, 0, 0)
    torch.manual_seed(seed)
    x = torch.randn(2, 3, h, w)
    x[0, 0] *= 40.0                                     # reaches the clamp of 8: code 2 occurs, the strip repeats on the exact path
    x = x.to(getattr(torch, dtype)).cuda()
    return x, torch.from_numpy(F[fu]).cuda(), torch.from_numpy(F[fd]).cuda(), cfg, padding


@pytest.mark.parametrize('dtype,tol', DTYPES)
@pytest.mark.parametrize('yh', [4, 36])
@pytest.mark.parametrize('yw', [4, 20, 36])
@pytest.mark.parametrize('kern', ['u2d2', 'u2d4', 'u4d2'])
def test_narrow_planes_forward_write_and_aligned_read(kern, yw, yh, dtype, tol):
    """Forward (codes written) and the sign-reading call behind its backward (aligned, oy0 < 0) on planes of one to three column
    groups and 4 / 36 rows, dense and row-pitched, operands in NaN: finite, equal to the compact call bit for bit, at the bar."""
    from afcm_amd.torch_utils.ops import filtered_lrelu as flr
    x, fu, fd, cfg, padding = _setup(kern, yh, yw, dtype, 100 * yh + yw)
    y0, s0, lay, _ = flr._run(x, fu, fd, None, None, cfg, True)
    assert lay == 2 and tuple(y0.shape[2:]) == (yh, yw), 'expected the wave kernels'
    _close(y0.float().cpu(), _forward_ref(x, None, None, kern, padding, R.CLAMP), tol, f'{kern} {yh}x{yw} y')
    for pitched in (False, True):
        y1, s1, _, _ = flr._run(_in_nan(x, pitched), fu, fd, None, None, cfg, True, pitched_out=pitched)
        assert torch.equal(y1, y0) and torch.equal(s1, s0), f'forward, operands in NaN, pitched {pitched}'
    # the transposed op with these codes
    bcfg = flr._backward_cfg(cfg, fu, fd, x.shape, y0.shape, 2)
    assert bcfg[11] % 16 >= bcfg[1], 'the read call must start above the plane (oy0 = -((sy mod 16) / down) < 0)'
    g = torch.randn(y0.shape).to(y0.dtype).cuda()
    d0, _, _, p0 = flr._run(g, fd, fu, None, s0, bcfg, False, want_plane_sum=True)
    assert d0.shape == x.shape
    want = R.read_reference(g.double().cpu().numpy(), fd.cpu().numpy(), fu.cpu().numpy(), bcfg, R.decode_codes(s0.cpu().numpy(), 2))
    _close(d0.double().cpu(), want, tol, f'{kern} {yh}x{yw} dx, given codes')
    _close(p0.sum(2).cpu(), d0.float().sum([2, 3]).cpu(), 2e-2, f'{kern} {yh}x{yw} plane sums')
    for pitched in (False, True):
        d1, _, _, p1 = flr._run(_in_nan(g, pitched), fd, fu, None, _in_nan(s0, False), bcfg, False, want_plane_sum=True, pitched_out=pitched)
        assert torch.equal(d1, d0) and torch.equal(p1, p0), f'sign-reading call, operands in NaN, pitched {pitched}'


@pytest.mark.parametrize('dtype,tol', DTYPES)
@pytest.mark.parametrize('pitched', [False, True], ids=['dense', 'pitched'])
@pytest.mark.parametrize('yw', [36, 52, 68])
@pytest.mark.parametrize('kern,yh', [('u2d2', 20), ('u2d2', 36), ('u2d2', 70), ('u2d4', 36), ('u4d2', 36)])
def test_skip_forward_column_block_pairs(kern, yh, yw, pitched, dtype, tol):
    """Forward with the encoder-skip operand over 3 / 4 / 5 output column blocks = two pairs with the last one half filled, two
    pairs, three pairs with the last one half filled: the request for a pair at the top of the group before its first down-x pass
    and its park at the top of that group, at the first, at a middle and at the last pair of a strip (32-row strips, the 48-row
    strip, down 4, up 4), skip and x in NaN."""
    from afcm_amd.torch_utils.ops import filtered_lrelu as flr
    x, fu, fd, cfg, padding = _setup(kern, yh, yw, dtype, 7 * yh + yw)
    n, c = x.shape[:2]
    skip = torch.randn(n, c, yh, yw).to(x.dtype).cuda()
    osc = (torch.rand(n * c) + 0.5).cuda()
    for write in (True, False):                          # training forward (codes written) and inference
        y0, s0, lay, _ = flr._run(x, fu, fd, None, None, cfg, write, oscale=osc, skip=skip)
        assert (lay == 2 or not write) and tuple(y0.shape[2:]) == (yh, yw)
        _close(y0.float().cpu(), _forward_ref(x, skip, osc, kern, padding, R.CLAMP), tol, f'{kern} {yh}x{yw} y, skip, codes written {write}')
        y1, s1, _, _ = flr._run(_in_nan(x, pitched), fu, fd, None, None, cfg, write, oscale=osc, skip=_in_nan(skip, pitched), pitched_out=pitched)
        assert torch.equal(y1, y0), f'skip forward, operands in NaN, codes written {write}'
        assert not write or torch.equal(s1, s0)


@pytest.mark.parametrize('dtype,tol', DTYPES)
@pytest.mark.parametrize('kern', ['u2d2', 'u2d4', 'u4d2'])
def test_last_plane_ends_with_its_allocation(kern, dtype, tol):
    """x, skip, the cotangent and the sign tensor each fill an allocation of their own to its last byte (sizes in whole 512-byte
    blocks of the allocator): the requests that run ahead of the last plane's last strip fall behind the tensor and must be dropped
    by the plane's descriptor.  Asserts the results only."""
    from afcm_amd.torch_utils.ops import filtered_lrelu as flr
    yh, yw = 36, 20
    x, fu, fd, cfg, padding = _setup(kern, yh, yw, dtype, 11)
    x = torch.cat([x, x.flip(0)], 1)                     # [2, 6, h, w]

    def own(t):
        """A copy in an allocation that ends with the tensor: padded with leading planes to whole 512-byte blocks."""
        per = t[0, 0].numel() * t.element_size()
        lead = next(k for k in range(512) if ((t.shape[0] * t.shape[1] + k) * per) % 512 == 0)
        buf = torch.empty([t.shape[0] * t.shape[1] + lead, *t.shape[2:]], dtype=t.dtype, device=t.device)
        v = buf[lead:].view(t.shape)
        v.copy_(t)
        assert (v.data_ptr() + v.numel() * v.element_size()) == buf.data_ptr() + buf.numel() * buf.element_size()
        return v

    n, c = x.shape[:2]
    skip = torch.randn(n, c, yh, yw).to(x.dtype).cuda()
    y0, s0, lay, _ = flr._run(own(x), fu, fd, None, None, cfg, True, skip=own(skip))
    assert lay == 2
    _close(y0.float().cpu(), _forward_ref(x, skip, None, kern, padding, R.CLAMP), tol, f'{kern} y')
    bcfg = flr._backward_cfg(cfg, fu, fd, x.shape, y0.shape, 2)
    g = torch.randn(y0.shape).to(y0.dtype).cuda()
    d0, _, _, _ = flr._run(own(g), fd, fu, None, own(s0), bcfg, False)
    want = R.read_reference(g.double().cpu().numpy(), fd.cpu().numpy(), fu.cpu().numpy(), bcfg, R.decode_codes(s0.cpu().numpy(), 2))
    _close(d0.double().cpu(), want, tol, f'{kern} dx, given codes')
