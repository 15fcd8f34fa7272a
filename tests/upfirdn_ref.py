"""float64 restatement of upfirdn2d with per-axis factors (afcm_amd/csrc/upfirdn2d.hip), FROM THE OP'S DEFINITION (the header of that file,
SURVEY.md Appendix A), not from any kernel body; its explicit transpose; a DERIVED per-element bound on |kernel - float64|; the host
conditions that pick one of the three kernels (from the comments above launch_rows / launch_tile); and the cases that
tests/test_upfirdn_ref_cpu.py (no GPU: the restatement against the oracle, hand-worked values, the transpose, the bound against an fp32
emulation and four wrong ones, which kernel each case reaches) and tests/test_gpu_upfirdn2d.py (the kernels against the restatement) share.

The definition.  z is x with sample (iy, ix) at (iy * uy, ix * ux) and zeros elsewhere, then py0 / px0 zeros in front and py1 / px1 behind
(negative: crop).  w = f * gain, reversed in both axes unless ``flip``.  y[oy, ox] = sum_{ky, kx} w[ky, kx] z[oy * dy + ky, ox * dx + kx],
for the yh x yw outputs of out_size().  Everything here is numpy float64 on the host; factors and paddings are (x, y) / (x0, x1, y0, y1)."""
import collections
import functools
import zlib

import numpy as np
import torch

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = (F32, F16, BF16)
U24 = 2.0 ** -24                                          # unit roundoff of fp32
_FORMAT = {F16: (10, -14), BF16: (7, -126)}               # fraction bits, exponent of the smallest normal number

Case = collections.namedtuple('Case', 'name xshape fshape up down padding gain')


def out_size(xh, xw, fh, fw, up, down, padding):
    """(yh, yw): the formula of ops/upfirdn2d.py:_launch."""
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = up, down, padding
    return (xh * uy + py0 + py1 - fh + dy) // dy, (xw * ux + px0 + px1 - fw + dx) // dx


def _source(n, up, p0, count):
    """For the first ``count`` positions of one axis of z: the index of the sample that sits there, n (an appended zero) where none does."""
    u = np.arange(count) - p0
    hit = (u >= 0) & (u < n * up) & (u % up == 0)
    return np.where(hit, u // up, n)


def _taps(f2d, flip, gain):
    f = np.asarray(f2d, dtype=np.float64)
    assert f.ndim == 2
    return (f if flip else f[::-1, ::-1]) * float(gain)


def upfirdn2d(x, f2d, up=(1, 1), down=(1, 1), padding=(0, 0, 0, 0), flip=False, gain=1.0):
    x = np.asarray(x, dtype=np.float64)
    w = _taps(f2d, flip, gain)
    (n, c, xh, xw), (fh, fw), (ux, uy), (dx, dy), (px0, _, py0, _) = x.shape, w.shape, up, down, padding
    yh, yw = out_size(xh, xw, fh, fw, up, down, padding)
    assert yh >= 1 and yw >= 1
    zh, zw = (yh - 1) * dy + fh, (yw - 1) * dx + fw      # the part of z the outputs reach
    xe = np.zeros((n, c, xh + 1, xw + 1))
    xe[:, :, :xh, :xw] = x
    z = xe[:, :, _source(xh, uy, py0, zh)][:, :, :, _source(xw, ux, px0, zw)]
    y = np.zeros((n, c, yh, yw))
    for ky in range(fh):
        for kx in range(fw):
            y += w[ky, kx] * z[:, :, ky:ky + (yh - 1) * dy + 1:dy, kx:kx + (yw - 1) * dx + 1:dx]
    return y


def adjoint(r, xhw, f2d, up=(1, 1), down=(1, 1), padding=(0, 0, 0, 0), flip=False, gain=1.0):
    """dx = the transpose of upfirdn2d(., f2d, ...) on [.., xh, xw] inputs, applied to r -- by scatter: every output adds w[ky, kx] r[oy, ox]
    to position (oy * dy + ky, ox * dx + kx) of z, and sample (iy, ix) collects what arrived at (iy * uy + py0, ix * ux + px0)."""
    r = np.asarray(r, dtype=np.float64)
    w = _taps(f2d, flip, gain)
    (xh, xw), (fh, fw), (ux, uy), (dx, dy), (px0, _, py0, _) = xhw, w.shape, up, down, padding
    n, c, yh, yw = r.shape
    assert (yh, yw) == out_size(xh, xw, fh, fw, up, down, padding)
    zh, zw = (yh - 1) * dy + fh, (yw - 1) * dx + fw
    dz = np.zeros((n, c, zh + 1, zw + 1))                  # (the last row and column stay zero: samples no output reaches)
    for ky in range(fh):
        for kx in range(fw):
            dz[:, :, ky:ky + (yh - 1) * dy + 1:dy, kx:kx + (yw - 1) * dx + 1:dx] += w[ky, kx] * r
    py, px = np.arange(xh) * uy + py0, np.arange(xw) * ux + px0
    py, px = np.where((py >= 0) & (py < zh), py, zh), np.where((px >= 0) & (px < zw), px, zw)
    return dz[:, :, py][:, :, :, px]


def grad_call(xhw, fshape, up, down, padding, flip):
    """The forward call that ops/upfirdn2d.py's backward makes on the cotangent: (up, down, padding, flip)."""
    (xh, xw), (fh, fw), (ux, uy), (dx, dy), (px0, _, py0, _) = xhw, fshape, up, down, padding
    yh, yw = out_size(xh, xw, fh, fw, up, down, padding)
    p = (fw - px0 - 1, xw * ux - yw * dx + px0 - ux + 1, fh - py0 - 1, xh * uy - yh * dy + py0 - uy + 1)
    return down, up, p, not flip


def half_ulp(mag, dtype):
    """Half a unit in the last place of the 16-bit ``dtype`` at magnitude ``mag`` (its subnormal spacing below the smallest normal)."""
    fbits, emin = _FORMAT[dtype]
    _, ex = np.frexp(mag)                                  # mag = m 2^ex, m in [0.5, 1): the exponent is ex - 1
    return np.ldexp(0.5, np.maximum(ex - 1, emin) - fbits)


def bound(x, f2d, up=(1, 1), down=(1, 1), padding=(0, 0, 0, 0), flip=False, gain=1.0, out_dtype=F32, y=None, x_err=None):
    """Per-element bound on |kernel - float64|.  Every kernel rounds tap = f * gain once to fp32 and accumulates at most K = fh fw fused
    multiply-adds in fp32 from inputs that convert exactly: |acc - y| <= (K + 3) 2^-24 S with S the op on |x|, |f|, |gain| (K roundings of
    the chain, one of the tap, slack for 1 / (1 - K u) up to K = 4096).  A 16-bit output adds half a unit in the last place at
    |y| + that bound (from_f32 rounds to nearest even).  Where S == 0 the bound is 0: the output must be exactly +0.
    ``x_err``: a bound on |the input the kernel really gets - x| (the second pass of the separable entry); it reaches the output through
    the same op, S_err, and adds (1 + (K + 3) 2^-24) S_err."""
    f = np.abs(np.asarray(f2d, dtype=np.float64))
    k = f.shape[0] * f.shape[1]
    assert k <= 4096
    s = upfirdn2d(np.abs(np.asarray(x, dtype=np.float64)), f, up, down, padding, flip, abs(float(gain)))
    b = (k + 3) * U24 * s
    if x_err is not None:
        b = b + (1 + (k + 3) * U24) * upfirdn2d(x_err, f, up, down, padding, flip, abs(float(gain)))
    if out_dtype != F32:
        if y is None:
            y = upfirdn2d(x, f2d, up, down, padding, flip, gain)
        b = b + half_ulp(np.abs(y) + b, out_dtype)
    return np.where((s == 0) & (x_err is None), 0.0, b)


def mismatch(got, want, bar):
    """None, or a description of the worst element of ``got`` (any float array) outside its own bound / a zero-bound element that is not +0."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape == bar.shape, (got.shape, want.shape, bar.shape)
    err = np.abs(got - want)
    bad = ~(err <= bar) | ((bar == 0) & np.signbit(got))
    if not bad.any():
        return None
    i = np.unravel_index(np.argmax(np.where(bad, err - bar, -np.inf)), got.shape)
    return f'{int(bad.sum())} of {bad.size} elements outside their bound; worst at {tuple(int(v) for v in i)}: got {got[i]!r}, want {want[i]!r}, bound {bar[i]:.3e}'


# ---- which kernel the host picks ------------------------------------------------------------------------------------------------------------
def rows_first_column(up, padx0):
    """a0 of the rows kernel's first column group: the even column its 16-byte loads start from (<= 0; -2 or -4 with left padding)."""
    c0 = -padx0 if up == 1 else (-padx0 + (padx0 & 1)) // 2
    return c0 - (c0 & 1)


def expected_kernel(dtype, x_shape, f_shape, up, down, padding, aligned=True):
    """'rows' | 'tile' | 'gather', from the conditions in the comments above launch_rows and launch_tile.  ``aligned``: x and y start on
    4-byte boundaries."""
    n, c, xh, xw = x_shape
    fh, fw = f_shape
    yh, yw = out_size(xh, xw, fh, fw, up, down, padding)
    small = up[0] == up[1] and down[0] == down[1] and fh <= 4 and fw <= 4 and (up[0], down[0]) in ((1, 1), (1, 2), (2, 1))
    if not small:
        return 'gather'
    planes = n * c
    rows = (dtype != F32 and aligned and xw % 2 == 0 and yw % 2 == 0
            and planes * xh * xw * 2 < 2 ** 31 and planes * yh * yw < 2 ** 31      # 32-bit buffer offsets / element indices
            and padding[0] <= (3 if up[0] == 1 else 6)                             # the first group starts at most 4 columns left of the plane
            and xw + rows_first_column(up[0], padding[0]) >= 0)                    # ... and no further left than one row is wide
    return 'rows' if rows else 'tile'


# ---- shared cases ---------------------------------------------------------------------------------------------------------------------------
def _case(name, xshape, fshape, up=(1, 1), down=(1, 1), padding=(0, 0, 0, 0), gain=1.0):
    return Case(name, tuple(xshape), tuple(fshape), tuple(up), tuple(down), tuple(padding), float(gain))


def _gather_cases():
    c = []
    # per-axis factors (ux, uy, dx, dy), filters [4, 4] and [2, 3] in turn
    for i, (fac, pad) in enumerate([((2, 1, 1, 1), (2, 1, 1, 2)), ((1, 2, 1, 1), (1, 1, 0, 1)), ((1, 1, 2, 1), (1, 2, 2, 1)), ((1, 1, 1, 2), (0, 2, 1, 0)),
                                    ((3, 2, 2, 3), (2, 3, 1, 2)), ((2, 2, 2, 2), (1, 2, 2, 1)), ((2, 2, 4, 4), (3, 2, 1, 1)), ((4, 4, 2, 2), (2, 3, 3, 2)),
                                    ((4, 4, 1, 1), (2, 1, 0, 3)), ((1, 1, 4, 4), (1, 2, 2, 1)), ((3, 3, 1, 1), (1, 0, 2, 1)), ((1, 1, 3, 3), (2, 1, 1, 2))]):
        c.append(_case('factors_%d%d%d%d' % fac, (1, 3, 11, 13), ((4, 4), (2, 3))[i % 2], fac[:2], fac[2:], pad, (1.0, 4.0, 0.5)[i % 3]))
    # up 4: the generator's filter shapes
    c.append(_case('up4_f1x12', (1, 2, 5, 9), (1, 12), (4, 4), (1, 1), (7, 4, 0, 0), 4.0))
    c.append(_case('up4_f12x1', (1, 2, 9, 5), (12, 1), (4, 4), (1, 1), (0, 0, 7, 4), 4.0))
    c.append(_case('up4_f5x3', (1, 2, 6, 7), (5, 3), (4, 4), (1, 1), (3, 0, 4, 0), 16.0))
    c.append(_case('up4_f24x24', (2, 2, 9, 10), (24, 24), (4, 4), (1, 1), (13, 10, 13, 10), 16.0))
    c.append(_case('up4_down2_f24x24', (1, 2, 9, 10), (24, 24), (4, 4), (2, 2), (13, 10, 12, 11), 16.0))
    # the loss blur's two passes
    c.append(_case('blur_f1x61', (1, 2, 9, 70), (1, 61), padding=(30, 30, 0, 0)))
    c.append(_case('blur_f61x1', (1, 2, 70, 9), (61, 1), padding=(0, 0, 30, 30)))
    # paddings: none, uneven, crops deeper than the up factor on either side, larger than the filter
    c.append(_case('pad_zero_f5x3', (1, 2, 9, 11), (5, 3)))
    c.append(_case('pad_uneven_f5x3', (1, 2, 9, 11), (5, 3), (1, 1), (2, 2), (3, 0, 1, 4)))
    c.append(_case('crop_up2_lo', (1, 2, 9, 11), (6, 6), (2, 2), (1, 1), (-3, 4, -5, 6), 4.0))
    c.append(_case('crop_up2_hi', (1, 2, 9, 11), (6, 6), (2, 2), (1, 1), (4, -5, 6, -3), 4.0))
    c.append(_case('crop_up4_lo', (1, 2, 7, 8), (8, 8), (4, 4), (1, 1), (-3, 9, -5, 11), 16.0))
    c.append(_case('crop_up4_hi', (1, 2, 7, 8), (8, 8), (4, 4), (1, 1), (9, -5, 11, -3), 16.0))
    c.append(_case('crop_up4_down2', (1, 2, 7, 8), (8, 8), (4, 4), (2, 2), (-5, 6, -3, 8), 16.0))
    c.append(_case('crop_up3_down2', (1, 2, 7, 8), (5, 3), (3, 3), (2, 2), (-4, 3, -5, 7), 0.5))
    c.append(_case('crop_up2x_down3y', (1, 2, 14, 8), (2, 3), (2, 1), (1, 3), (-3, 2, -5, 1)))
    c.append(_case('pad_beyond_filter', (1, 2, 3, 4), (5, 3), padding=(7, 6, 9, 8)))
    c.append(_case('pad_beyond_filter_up2', (1, 2, 3, 4), (5, 3), (2, 2), (1, 1), (9, 6, 11, 8), 4.0))
    # output widths / heights around the 64 x 4 block
    for yh, yw in ((1, 1), (3, 63), (4, 64), (5, 65), (9, 130)):
        c.append(_case('out_%dx%d' % (yh, yw), (1, 2, yh + 4, yw + 2), (5, 3)))
    c.append(_case('out_65x9_down2', (1, 2, 12, 133), (2, 3), (1, 2), (2, 1), (1, 0, 0, 1)))
    c.append(_case('in_1x1', (1, 3, 1, 1), (2, 3), (2, 1), (1, 1), (2, 2, 1, 1)))
    c.append(_case('in_1x1_up3_down2', (2, 1, 1, 1), (5, 3), (3, 3), (2, 2), (2, 3, 4, 2)))
    # more blocks than the launch's cap of 256 * 64: planes past 16 384 take the second trip of the grid-stride loop
    c.append(_case('planes_16400', (16400, 1, 3, 3), (5, 5), padding=(2, 2, 2, 2)))
    # kMaxTaps
    c.append(_case('taps_4096', (1, 2, 5, 7), (64, 64), padding=(32, 31, 32, 31)))
    return c


_TILE_FACTORS = ((1, 1), (1, 2), (2, 1))


def _tile_cases():
    c = []
    # planes smaller than a filter and up: the product of factors, inputs and filter shapes, full-convolution padding plus a little
    i = 0
    for u, d in _TILE_FACTORS:
        for xh, xw in ((1, 1), (1, 2), (2, 1), (2, 2), (3, 5)):
            for fh, fw in ((1, 1), (2, 2), (4, 1), (1, 4), (4, 4)):
                pad = (fw - 1 + i % 2, fw - 1 + (i // 2) % 2 + d - 1, fh - 1 + (i // 3) % 2, fh - 1 + i % 3 + d - 1)
                c.append(_case('small_u%dd%d_x%dx%d_f%dx%d' % (u, d, xh, xw, fh, fw), (1, 3, xh, xw), (fh, fw), (u, u), (d, d), pad, float(u * u)))
                i += 1
    # outputs of exactly TOX / TOX + 1 columns and TOY / TOY + 1 rows
    c.append(_case('out_32x64_u1d1', (1, 2, 32, 64), (4, 4), padding=(2, 1, 2, 1)))
    c.append(_case('out_33x65_u1d1', (1, 2, 33, 65), (4, 4), padding=(2, 1, 2, 1)))
    c.append(_case('out_32x64_u1d2', (1, 2, 64, 128), (4, 4), (1, 1), (2, 2), (2, 1, 2, 1)))
    c.append(_case('out_33x65_u1d2', (1, 2, 65, 129), (4, 4), (1, 1), (2, 2), (2, 1, 2, 1)))
    c.append(_case('out_32x64_u2d1', (1, 2, 16, 32), (4, 4), (2, 2), (1, 1), (2, 1, 2, 1), 4.0))
    c.append(_case('out_33x65_u2d1', (1, 2, 16, 32), (4, 4), (2, 2), (1, 1), (2, 2, 2, 2), 4.0))
    # a left / top padding of 10 (input tiles whose first rows / columns are all padding), and of more than a whole output tile
    for u, d in _TILE_FACTORS:
        c.append(_case('pad10_left_u%dd%d' % (u, d), (1, 2, 5, 7), (4, 4), (u, u), (d, d), (10, 1, 2, 1), float(u * u)))
        c.append(_case('pad10_top_u%dd%d' % (u, d), (1, 2, 5, 7), (3, 4), (u, u), (d, d), (2, 1, 10, 0), float(u * u)))
    c.append(_case('tile_of_padding_top', (1, 1, 3, 5), (4, 4), padding=(2, 1, 40, 0)))
    c.append(_case('tile_of_padding_left', (1, 1, 3, 5), (4, 3), padding=(70, 0, 1, 2)))
    c.append(_case('tile_of_padding_top_u2d1', (1, 1, 3, 5), (4, 4), (2, 2), (1, 1), (2, 1, 41, 0), 4.0))
    # up 2: odd and even tile origins (the second tile starts at 64 - padx0, 32 - pady0), negative ones
    for pad in ((3, 2, 2, 3), (2, 3, 3, 2), (-1, 4, -2, 5), (-3, 6, -4, 7), (7, 2, 1, 2)):
        c.append(_case('u2d1_pad_%d_%d_%d_%d' % pad, (1, 2, 20, 40), (4, 4), (2, 2), (1, 1), pad, 4.0))
    c.append(_case('u1d1_padx0_4', (1, 2, 9, 12), (4, 4), padding=(4, 1, 2, 1)))
    c.append(_case('u1d2_odd_width', (1, 2, 9, 13), (4, 4), (1, 1), (2, 2), (1, 2, 1, 1)))
    return c


def _rows_dims(n, u, d, p0, f, want):
    """(input size, p1) of one axis with out == want (want None: input size n and the first p1 that makes out even and >= 2)."""
    cands = [(n, p1) for p1 in range(0, 10)] if want is None else [(m, p1) for p1 in (1, 0, 2, 3, 4, 5, 6, 7, -1, -2, -3, -4, -5, -6, -7, -8, -9) for m in range(1, 40)]
    for m, p1 in cands:
        total = m * u + p0 + p1
        out = (total - f + d) // d
        if total >= f and (out == want if want is not None else (out >= 2 and out % 2 == 0)):
            return m, p1
    raise AssertionError((n, u, d, p0, f, want))


ROWS_SUSPECT = 'w2_padx0_3_second_row'


def _rows_cases():
    # the tensor's first column group starts 4 columns left of a plane that is 2 wide: its SECOND row starts before the tensor as well
    c = [_case(ROWS_SUSPECT, (1, 1, 2, 2), (4, 4), padding=(3, 2, 2, 1)),
         _case('w2_padx0_3_three_rows_3planes', (1, 3, 3, 2), (4, 4), padding=(3, 2, 2, 1)),
         _case('w2_padx0_3_down2', (1, 1, 4, 2), (4, 4), (1, 1), (2, 2), (3, 1, 1, 1)),
         _case('w2_padx0_6_up2_second_row', (1, 1, 2, 2), (4, 4), (2, 2), (1, 1), (6, 1, 2, 1), 4.0)]
    filters = ((4, 4), (3, 2), (4, 4), (1, 4), (2, 2), (4, 4), (4, 1), (1, 1))
    i = 0
    for u, d in _TILE_FACTORS:
        rpt = 4 if (u, d) == (1, 2) else 8
        heights = (1, 2, 3, rpt - 1, rpt, rpt + 1)
        for px0 in range(4 if u == 1 else 7):
            for xw in (2, 4, 6, 8, 10, 16):
                fh, fw = filters[(i + i // 6) % len(filters)]
                py0 = (3 * i + i // 8) % 8
                planes = (1, 3)[(i + i // 6) % 2]
                _, px1 = _rows_dims(xw, u, d, px0, fw, None)
                xh, py1 = _rows_dims(None, u, d, py0, fh, heights[(i + i // 6) % 6])
                c.append(_case('u%dd%d_px%d_w%d_%d' % (u, d, px0, xw, i), (1, planes, xh, xw), (fh, fw), (u, u), (d, d), (px0, px1, py0, py1),
                               float(u * u)))
                i += 1
    return c


GATHER_CASES = _gather_cases()
TILE_CASES = _tile_cases()
ROWS_CASES = _rows_cases()
BY_NAME = {'gather': {c.name: c for c in GATHER_CASES}, 'tile': {c.name: c for c in TILE_CASES}, 'rows': {c.name: c for c in ROWS_CASES}}
assert all(len(BY_NAME[k]) == len(v) for k, v in (('gather', GATHER_CASES), ('tile', TILE_CASES), ('rows', ROWS_CASES)))


def kernel_of(case, dtype, aligned=True):
    return expected_kernel(dtype, case.xshape, case.fshape, case.up, case.down, case.padding, aligned)


GATHER_PARAMS = [(c.name, dt) for c in GATHER_CASES for dt in DTYPES]
TILE_PARAMS = [(c.name, dt) for c in TILE_CASES for dt in DTYPES if kernel_of(c, dt) == 'tile']
ROWS_PARAMS = [(c.name, dt) for c in ROWS_CASES for dt in (F16, BF16)]
# the problems run twice, on an aligned x (rows kernel) and on one that starts 2 bytes past a 4-byte boundary (tile kernel): bit for bit
AGREE_PARAMS = [(c.name, dt) for i, c in enumerate(ROWS_CASES) for dt in (F16, BF16) if i % 4 == (0 if dt == F16 else 2) and kernel_of(c, dt) == 'rows']
# the rows-list cases whose first group starts further left than a row is wide: launch_rows leaves them to the tile kernel
ROWS_LEFT_TO_TILE = sorted(c.name for c in ROWS_CASES if c.xshape[3] + rows_first_column(c.up[0], c.padding[0]) < 0)
SEPARABLE = _case('separable_f8_up2', (1, 2, 9, 12), (8,), (2, 2), (1, 1), (4, 3, 4, 3), 4.0)
TAPS_TOO_MANY = _case('taps_4160', (1, 1, 5, 7), (65, 64), padding=(32, 31, 33, 31))
OFFSET_GUARD = dict(hw=(64, 64), planes_rows=2 ** 31 // (64 * 64 * 2) - 1, fshape=(4, 4), down=(2, 2), padding=(1, 1, 1, 1))


def param_id(p):
    return p if isinstance(p, str) else str(p).replace('torch.', '')


def _seed(case):
    return zlib.crc32(case.name.encode())


def inputs(case, dtype):
    """(x, f, r): seeded normal data of order 1, x and the cotangent r rounded to ``dtype``; f float32, random and asymmetric."""
    g = torch.Generator().manual_seed(_seed(case))
    x = torch.randn(case.xshape, generator=g).to(dtype)
    f = torch.randn(case.fshape, generator=g)
    n, c, xh, xw = case.xshape
    fh, fw = (case.fshape * 2)[-2:] if len(case.fshape) == 1 else case.fshape
    r = torch.randn((n, c) + out_size(xh, xw, fh, fw, case.up, case.down, case.padding), generator=g).to(dtype)
    return x, f, r


def f64(t):
    return t.double().numpy()


@functools.lru_cache(maxsize=None)
def reference(kind, name, dtype, flip):
    """(y, bound on y, dx, bound on dx) of a listed case, float64: computed once, shared, read-only."""
    case = BY_NAME[kind][name]
    x, f, r = (f64(t) for t in inputs(case, dtype))
    kw = dict(up=case.up, down=case.down, padding=case.padding, flip=flip, gain=case.gain)
    y = upfirdn2d(x, f, **kw)
    dx = adjoint(r, case.xshape[2:], f, **kw)
    gup, gdown, gpad, gflip = grad_call(case.xshape[2:], case.fshape, case.up, case.down, case.padding, flip)
    out = (y, bound(x, f, out_dtype=dtype, y=y, **kw), dx, bound(r, f, gup, gdown, gpad, gflip, case.gain, out_dtype=dtype, y=dx))
    for a in out:
        a.setflags(write=False)
    return out


def round_to(a, dtype):
    """float64 array -> the float64 values of its elements rounded to nearest even into ``dtype``."""
    return f64(torch.from_numpy(np.ascontiguousarray(a)).to(dtype))


def separable(x, f1d, up, down, padding, flip, gain, dtype):
    """(y, bound): the 1-D entry of ops/upfirdn2d.py -- the [1, fw] pass along x with gain 1, its result rounded to ``dtype``, then the
    [fh, 1] pass along y with ``gain``.  The kernel's intermediate is within e1 = bound(pass 1) + |rounding| of the rounded one."""
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = up, down, padding
    a = dict(up=(ux, 1), down=(dx, 1), padding=(px0, px1, 0, 0), flip=flip, gain=1.0)
    y1 = upfirdn2d(x, f1d[None, :], **a)
    r1 = round_to(y1, dtype)
    e1 = bound(x, f1d[None, :], out_dtype=dtype, y=y1, **a) + np.abs(y1 - r1)
    b = dict(up=(1, uy), down=(1, dy), padding=(0, 0, py0, py1), flip=flip, gain=gain)
    y = upfirdn2d(r1, f1d[:, None], **b)
    return y, bound(r1, f1d[:, None], out_dtype=dtype, y=y, x_err=e1, **b)
