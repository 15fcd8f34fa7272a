"""filtered_lrelu, every kernel family, bit for bit against the float64 definition (cases, data and the proof that equality is the
right bar: tests/flrelu_exact_ref.py, tests/test_flrelu_exact_ref_cpu.py).

Every quantity a kernel rounds on these operands is representable in its dtype, so the float64 result rounded once is the only
right answer: outputs, every sign code of the upsampled extent (no mask around 0: the pre-activations are integers, exact zeros
read code 0, an element exactly at the clamp is not clamped), the inference forward, the skip / plane-factor epilogue, the
transposed call on the written codes and -- where the unrounded dx is representable -- its plane sums are compared with equality.
Equality is numeric: the sign of a zero is not compared.  Each case runs dense and row-pitched."""
import numpy as np
import pytest
import torch

import flrelu_exact_ref as E
import flrelu_read_ref as R

pytestmark = pytest.mark.gpu

CASES = E.cases()


def _dev(a, dtype, pitched=False):
    """float64 array -> device tensor of `dtype`; `pitched`: a row-pitched view whose padding columns hold NaN."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(getattr(torch, dtype)).cuda()
    assert torch.equal(t.double().cpu(), torch.from_numpy(np.ascontiguousarray(a))), 'operands must be values of the dtype'
    if not pitched:
        return t
    n, c, h, w = t.shape
    ld = (w + 31) // 32 * 32 + 32
    buf = torch.full([n, c, h, ld], float('nan'), dtype=t.dtype, device=t.device)
    buf[..., :w] = t
    return buf[..., :w]


def _same(got, want, what):
    """Numeric equality of a device tensor with a float64 array, element by element."""
    got = got.double().cpu().numpy()
    assert got.shape == want.shape, f'{what}: shape {got.shape}, expected {want.shape}'
    bad = got != want
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.size} elements differ, first at {i}: {got[i]!r}, expected {want[i]!r}')


@pytest.mark.parametrize('pitched', [False, True], ids=['dense', 'pitched'])
@pytest.mark.parametrize('case', CASES, ids=[c['id'] for c in CASES])
def test_exact(case, pitched, monkeypatch):
    from afcm_amd.torch_utils.ops import _rows
    from afcm_amd.torch_utils.ops import filtered_lrelu as flr
    monkeypatch.setattr(_rows, 'MAX_OVERHEAD', 10.0)       # pitched outputs for these narrow planes too (the layout rule leaves them dense)
    d, ref, dtype = E.data(case), E.reference(case), case['dtype']
    fu, fd = torch.from_numpy(d['fu']).cuda(), torch.from_numpy(d['fd']).cuda()
    b = None if d['b'] is None else _dev(d['b'], dtype)
    osc = None if d['oscale'] is None else torch.from_numpy(d['oscale']).float().cuda()
    skip = lambda: None if d['skip'] is None else _dev(d['skip'], dtype, pitched)
    cfg = E.forward_cfg(case)

    # sign-writing forward
    y, s, lay, _ = flr._run(_dev(d['x'], dtype, pitched), fu, fd, b, None, cfg, True, oscale=osc, skip=skip(), pitched_out=pitched)
    assert lay == case['layout'], f'expected the {case["family"]} kernels'
    assert y.is_contiguous() == (not pitched or lay != 2)        # (the wave kernels address rows by pitch; the others get dense copies)
    _same(y, ref['expected_y'], 'y, codes written')

    # every code of the upsampled extent that an output reads (with these paddings: all of it but the last down - 1 rows / columns)
    codes = R.decode_codes(s.cpu().numpy(), lay)
    rows, cols = ref['codes'].shape[2:]
    used = (case['yh'] - 1) * case['down'] + len(d['fd']), (case['yw'] - 1) * case['down'] + len(d['fd'])
    assert rows - case['down'] < used[0] <= rows and cols - case['down'] < used[1] <= cols
    assert codes.shape[2] >= used[0] and codes.shape[3] >= used[1]
    want = ref['codes'][:, :, :used[0], :used[1]]
    got = codes[:, :, :used[0], :used[1]]
    bad = got != want
    assert not bad.any(), (f'{int(bad.sum())} sign codes differ, first at {np.argwhere(bad)[0].tolist()}: {got[bad][0]}, expected {want[bad][0]} '
                           f'(gain X2 there: {(ref["u"] * case["gain"])[:, :, :used[0], :used[1]][bad][0]})')

    # inference forward: no sign tensor, the same numbers
    y2, s2, _, _ = flr._run(_dev(d['x'], dtype, pitched), fu, fd, b, None, cfg, False, oscale=osc, skip=skip(), pitched_out=pitched)
    assert s2 is None
    _same(y2, ref['expected_y'], 'y, inference')
    assert torch.equal(y2, y)

    # the transposed call on the written codes
    bcfg = E.backward_cfg(case)
    dx, _, _, psum = flr._run(_dev(d['g'], dtype, pitched), fd, fu, None, s, bcfg, False, want_plane_sum=True, pitched_out=pitched)
    _same(dx, ref['expected_dx'], 'dx')
    assert (psum is not None) == (lay != 0)
    if psum is not None and E.dx_representable(case):
        _same(psum.sum(2), ref['psum'], 'plane sums')
