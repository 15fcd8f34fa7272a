"""afcm_upfirdn2d's three kernels (afcm_amd/csrc/upfirdn2d.hip: the gather kernel, the LDS tile kernel, the 16-bit rows kernel) against the
float64 restatement of tests/upfirdn_ref.py, forward and input gradient, with and without flip, EVERY output element against its own
derived bound ((K + 3) 2^-24 of the sum of magnitudes, plus half a unit in the last place of a 16-bit output; exactly +0 where no sample is
met).  No tolerance here comes from an observed error.  tests/test_upfirdn_ref_cpu.py checks the restatement, that the bound tells four
wrong kernels from a right one on these very cases, and that each list reaches the kernel it names.  2-D [fh, fw] filters: one call is one
launch."""
import pytest
import torch

import upfirdn_ref as U

pytestmark = pytest.mark.gpu

F32, F16, BF16 = U.F32, U.F16, U.BF16


def _op(x, f, case, flip):
    from afcm_amd.torch_utils.ops import upfirdn2d as ufd
    return ufd.upfirdn2d(x, f, up=list(case.up), down=list(case.down), padding=list(case.padding), flip_filter=flip, gain=case.gain)


def _forward_and_gradient(case, dtype, flip):
    x, f, r = U.inputs(case, dtype)
    xg = x.cuda().requires_grad_(True)
    y = _op(xg, f.cuda(), case, flip)
    assert y.dtype == dtype and tuple(y.shape) == tuple(r.shape)
    dx, = torch.autograd.grad(y, xg, r.cuda())
    assert dx.dtype == dtype
    return U.f64(y.detach().cpu()), U.f64(dx.cpu())


def _check(kind, name, dtype):
    case = U.BY_NAME[kind][name]
    for flip in (False, True):
        y, ybar, dx, dxbar = U.reference(kind, name, dtype, flip)
        got_y, got_dx = _forward_and_gradient(case, dtype, flip)
        bad = U.mismatch(got_y, y, ybar)
        assert bad is None, f'{case} {dtype} flip={flip} y ({U.kernel_of(case, dtype)} kernel): {bad}'
        bad = U.mismatch(got_dx, dx, dxbar)
        assert bad is None, f'{case} {dtype} flip={flip} dx: {bad}'


@pytest.mark.parametrize('name, dtype', U.GATHER_PARAMS, ids=U.param_id)
def test_gather_kernel(name, dtype):
    """Per-axis factors, crops deeper than the up factor, paddings beyond the filter, outputs around the 64 x 4 block, a 1 x 1 input, the
    second trip of the grid-stride loop (planes past 16 384 held to the same bound as the first), 4096 taps -- in all three types."""
    _check('gather', name, dtype)


def test_gather_kernel_refuses_more_than_4096_taps():
    case = U.TAPS_TOO_MANY
    x, f, _ = U.inputs(case, F32)
    with pytest.raises(RuntimeError, match='filters larger than 4096 taps are not supported'):
        _op(x.cuda(), f.cuda(), case, False)


@pytest.mark.parametrize('name, dtype', U.TILE_PARAMS, ids=U.param_id)
def test_tile_kernel(name, dtype):
    """Planes smaller than the filter, outputs of exactly 64 / 65 columns and 32 / 33 rows, tiles of nothing but padding, odd / even / negative
    tile origins at up 2; fp32 always, 16-bit wherever the host leaves the shape to this kernel (odd widths, padx0 4 at up 1 and 7 at up 2)."""
    _check('tile', name, dtype)


@pytest.mark.parametrize('name, dtype', U.ROWS_PARAMS, ids=U.param_id)
def test_rows_kernel(name, dtype):
    """Widths from one dword to two column groups, heights around each RPT, every left padding the first column group covers, every top
    padding up to 7, one plane and three (only plane 0 holds the tensor's very first group).  The cases named w2_padx0_* (and the two
    generated ones of that shape): a plane 2 columns wide whose first group starts 4 columns to the left, so that the tensor's SECOND row
    starts before the tensor too.  The rows kernel read row 1 of plane 0 as zeros and gave plane 1 of one-row planes plane 0's row (every
    one of these cases failed, as did the two of the tile list whose shape this is); launch_rows now leaves the shape to the tile kernel."""
    _check('rows', name, dtype)


@pytest.mark.parametrize('name, dtype', U.AGREE_PARAMS, ids=U.param_id)
def test_rows_and_tile_kernels_agree_bit_for_bit(name, dtype):
    """The same 16-bit problem on an aligned x (rows kernel) and on a contiguous x that starts 2 bytes past a 4-byte boundary (launch_rows
    refuses: tile kernel).  Both meet the taps in the same order; filters below 4 x 4 (rows: taps skipped; tile: zero taps multiplied) included."""
    case = U.BY_NAME['rows'][name]
    assert U.kernel_of(case, dtype) == 'rows' and U.kernel_of(case, dtype, aligned=False) == 'tile'
    x, f, _ = U.inputs(case, dtype)
    x, f = x.cuda(), f.cuda()
    buf = torch.zeros(x.numel() + 8, dtype=dtype, device='cuda')
    shifted = buf[1:1 + x.numel()].view(x.shape)
    shifted.copy_(x)
    assert x.data_ptr() % 4 == 0 and shifted.data_ptr() % 4 == 2 and shifted.is_contiguous()
    for flip in (False, True):
        a, b = _op(x, f, case, flip), _op(shifted, f, case, flip)
        assert a.data_ptr() % 4 == 0 and b.data_ptr() % 4 == 0
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (case, dtype, flip)


@pytest.mark.parametrize('dtype', U.DTYPES, ids=U.param_id)
@pytest.mark.parametrize('hw, pad', [((8, 10), 0), ((5, 6), 2), ((1, 2), 0), ((33, 66), 0)], ids=str)
def test_one_tap_up2_is_zero_stuffing_bit_for_bit(hw, pad, dtype):
    """The call of the stride-2 convolution's backward (ops/conv2d.py, _StridedConv2d.backward): a one-tap filter, up 2, padding
    [0, fw - 2 w, 0, fh - 2 h].  For finite dy the result IS the zero-stuffed dy: the values unchanged, +0 everywhere else."""
    from afcm_amd.torch_utils.ops import upfirdn2d as ufd
    h, w = hw
    g = torch.Generator().manual_seed(7 + h)
    dy = torch.randn([2, 3, h, w], generator=g).to(dtype).cuda()
    fh, fw = 2 * h + pad, 2 * w + pad
    full = ufd.upfirdn2d(dy, torch.ones([1, 1], device='cuda'), up=2, padding=[0, fw - 2 * w, 0, fh - 2 * h])
    want = dy.new_zeros([2, 3, fh, fw])
    want[:, :, :2 * h:2, :2 * w:2] = dy
    assert full.shape == want.shape and full.dtype == dtype
    bits = torch.int32 if dtype == F32 else torch.int16
    assert torch.equal(full.view(bits), want.view(bits))


@pytest.mark.parametrize('dtype', U.DTYPES, ids=U.param_id)
def test_separable_entry(dtype):
    """The 1-D filter entry: two launches ([1, fw] along x with gain 1, then [fh, 1] along y), the intermediate rounded to the tensor's type."""
    case = U.SEPARABLE
    x, f, r = U.inputs(case, dtype)
    for flip in (False, True):
        xg = x.cuda().requires_grad_(True)
        y = _op(xg, f.cuda(), case, flip)
        dx, = torch.autograd.grad(y, xg, r.cuda())
        want, bar = U.separable(U.f64(x), U.f64(f), case.up, case.down, case.padding, flip, case.gain, dtype)
        bad = U.mismatch(U.f64(y.detach().cpu()), want, bar)
        assert bad is None, f'{dtype} flip={flip} y: {bad}'
        gup, gdown, gpad, gflip = U.grad_call(case.xshape[2:], case.fshape * 2, case.up, case.down, case.padding, flip)
        want, bar = U.separable(U.f64(r), U.f64(f), gup, gdown, gpad, gflip, case.gain, dtype)
        bad = U.mismatch(U.f64(dx.cpu()), want, bar)
        assert bad is None, f'{dtype} flip={flip} dx: {bad}'


def test_rows_kernel_32_bit_offset_guard():
    """One bf16 buffer of 64 x 64 planes: just under 2^31 input bytes the rows kernel runs, with one plane more launch_rows refuses and the
    tile kernel runs.  In both runs the first, a middle and the last plane equal, bit for bit, the same three planes run as a launch of their
    own.  The size is the edge under test."""
    g = U.OFFSET_GUARD
    h, w = g['hw']
    p_rows = g['planes_rows']
    free, _ = torch.cuda.mem_get_info()
    if free < 8 * 2 ** 30:
        pytest.skip(f'needs about 3 GiB of device memory with headroom; {free / 2 ** 30:.1f} GiB are free')
    from afcm_amd.torch_utils.ops import upfirdn2d as ufd
    buf = torch.empty([p_rows + 1, 1, h, w], dtype=BF16, device='cuda')
    chunk = 2 ** 14
    gen = torch.Generator(device='cuda').manual_seed(5)
    for i in range(0, p_rows + 1, chunk):
        buf[i:i + chunk].normal_(generator=gen)
    f = torch.randn(g['fshape'], generator=torch.Generator().manual_seed(6)).cuda()
    kw = dict(down=list(g['down']), padding=list(g['padding']))
    for planes, kernel in ((p_rows, 'rows'), (p_rows + 1, 'tile')):
        assert U.expected_kernel(BF16, (planes, 1, h, w), g['fshape'], (1, 1), g['down'], g['padding']) == kernel
        assert (planes * h * w * 2 < 2 ** 31) == (kernel == 'rows')
        x = buf[:planes]
        y = ufd.upfirdn2d(x, f, **kw)
        picks = [0, planes // 2 + 1, planes - 1]
        alone = ufd.upfirdn2d(x[picks].contiguous(), f, **kw)
        assert U.expected_kernel(BF16, (3, 1, h, w), g['fshape'], (1, 1), g['down'], g['padding']) == 'rows'
        assert torch.equal(y[picks].view(torch.int16), alone.view(torch.int16)), (planes, kernel)
        assert bool(alone.float().abs().sum(dim=(1, 2, 3)).gt(0).all())
        del y, alone
