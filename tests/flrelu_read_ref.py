"""Sign-reading filtered_lrelu with the codes GIVEN: a float64 numpy reference, the three byte layouts of the sign tensor, and the
case tables of tests/test_gpu_flrelu_sign_window.py (test-only; no GPU).

The backward pass of filtered_lrelu is the op itself in sign-reading mode: up / down and the filters swapped, the activation
replaced by a lookup of the 2-bit code the forward wrote (bit 0: the element was negative -> * slope; bit 1: it was clamped -> 0)
in a window of the sign tensor at offset (sx, sy).  With the codes an INPUT the op is linear in x: no leaky-ReLU branch can flip,
so every element of a kernel's dx can be held to its rounding bound -- which a comparison with autograd on the oracle cannot do for
16-bit data (tests/test_gpu_flrelu_wave.py compares in relative L2 for that reason).

    u = upfirdn2d(x, fu, up, padding, gain=up^2)
    c = codes[Y + sy, X + sx] inside the code array, else 0                 (csrc/flrelu_common.h fetch_codes4)
    v = u * gain * (slope if c & 1 else 1) * (0 if c & 2 else 1)
    y = upfirdn2d(v, fd, down)

The case tables live here because two modules need the same parametrization: the GPU tests run it, and
tests/test_flrelu_read_ref_cpu.py proves without a GPU that each case has teeth -- that a window misplaced by one row or column,
or one 16 x 16 block of codes read as 0, moves the reference by several times what the GPU test allows.
"""
import functools

import numpy as np

from oracle import direct_np as dnp

INF = float('inf')


# ------------------------------------------------------------------------------------------------- the reference
def window_codes(codes, rows, cols, sx, sy):
    """codes[..., Y + sy, X + sx] for Y < rows, X < cols; 0 outside the code array."""
    codes = np.asarray(codes)
    out = np.zeros(codes.shape[:-2] + (rows, cols), dtype=np.uint8)
    y0, y1 = max(0, -sy), min(rows, codes.shape[-2] - sy)
    x0, x1 = max(0, -sx), min(cols, codes.shape[-1] - sx)
    if y1 > y0 and x1 > x0:
        out[..., y0:y1, x0:x1] = codes[..., y0 + sy:y1 + sy, x0 + sx:x1 + sx]
    return out


def read_activation(u, gain, slope, sx, sy, codes):
    """The activation of a sign-reading call on the upsampled grid (also the whole of filtered_lrelu_act_ in READ mode)."""
    u = np.asarray(u, dtype=np.float64)
    c = window_codes(codes, u.shape[2], u.shape[3], sx, sy)
    factor = np.array([1.0, slope, 0.0, 0.0])              # (slope if c & 1 else 1) * (0 if c & 2 else 1), by code
    return u * gain * factor[c]


def read_reference(x, fu, fd, cfg, codes):
    """float64 result of `_run(x, fu, fd, None, si, cfg, False)` where `codes` [N, C, rows, cols] is what `si` decodes to.
    cfg: the 13-tuple of afcm_amd.torch_utils.ops.filtered_lrelu._run (the clamp is not applied: the codes carry it; the layout
    entry is not read either).  fu / fd: 1-D (separable), 2-D or None."""
    up, down, px0, px1, py0, py1, gain, slope, _, flip, sx, sy = cfg[:12]
    fu = None if fu is None else np.asarray(fu, dtype=np.float64)
    fd = None if fd is None else np.asarray(fd, dtype=np.float64)
    u = upsample_fir(x, fu, up, [px0, px1, py0, py1], bool(flip))
    v = read_activation(u, gain, slope, sx, sy, codes)
    return dnp.upfirdn2d(v, fd, down=down, flip_filter=bool(flip))


def _up_axis(x, taps, up, lo, hi, axis):
    """Along `axis`: zero-insert by `up`, pad by lo / hi (negative = crop), out[y] = sum_t taps[t] z[y + t] -- visiting only the
    samples that are not inserted zeros: z[y + t] = x[i] where y + t - lo = up i."""
    n, k = x.shape[axis], len(taps)
    nout = n * up + lo + hi - (k - 1)
    assert nout >= 1
    out = np.zeros(x.shape[:axis] + (nout,) + x.shape[axis + 1:])
    at = lambda sl: (slice(None),) * axis + (sl,)
    for t in range(k):
        i0, i1 = max(0, -((lo - t) // up)), min(n - 1, (nout - 1 + t - lo) // up)
        if i1 >= i0:
            out[at(slice(up * i0 + lo - t, up * i1 + lo - t + 1, up))] += taps[t] * x[at(slice(i0, i1 + 1))]
    return out


def upsample_fir(x, fu, up, padding, flip):
    """oracle.direct_np.upfirdn2d(x, fu, up=up, padding=padding, gain=up^2, flip_filter=flip).  For a separable filter the same
    sums without the inserted zeros, rows before columns (up^2 x fewer products: the 278^2 planes of the generator-shaped tests
    take 0.3 s instead of 3); test_flrelu_read_ref_cpu.py holds the two against each other."""
    x = np.asarray(x, dtype=np.float64)
    if fu is None or np.ndim(fu) != 1:
        return dnp.upfirdn2d(x, fu, up=up, padding=padding, gain=float(up * up), flip_filter=flip)
    px0, px1, py0, py1 = padding
    taps = np.asarray(fu, dtype=np.float64) * up
    if not flip:
        taps = taps[::-1]
    return _up_axis(_up_axis(x, taps, up, px0, px1, 3), taps, up, py0, py1, 2)


# ------------------------------------------------------------------------------------------------- the byte layouts
def sign_tensor_shape(layout, rows, cols):
    """[sh, swb] of the uint8 tensor that holds rows x cols codes, as afcm_filtered_lrelu_shapes() sizes it for a sign-writing call
    (csrc/filtered_lrelu.hip shapes_and_plan)."""
    cols16 = (cols + 15) & ~15
    if layout == 0:
        return rows, cols16 // 4
    shq = (rows + 3) // 4
    if layout == 2:
        shq = (shq + 15) & ~15
    return shq, cols16


def _quads(codes, shq, swq):
    """codes [N, C, rows, cols] -> row-quad bytes [N, C, shq, swq]: one byte = 4 rows of one column, row r at bits 2r."""
    n, c, rows, cols = codes.shape
    buf = np.zeros((n, c, 4 * shq, swq), dtype=np.uint8)
    buf[:, :, :rows, :cols] = codes
    buf = buf.reshape(n, c, shq, 4, swq)
    return (buf[:, :, :, 0] | (buf[:, :, :, 1] << 2) | (buf[:, :, :, 2] << 4) | (buf[:, :, :, 3] << 6)).astype(np.uint8)


def _unquads(q):
    n, c, shq, swq = q.shape
    return np.stack([(q >> (2 * r)) & 3 for r in range(4)], axis=3).reshape(n, c, 4 * shq, swq)


def encode_codes(codes, layout):
    """2-bit codes [N, C, rows, cols] -> the uint8 sign tensor of `layout`, padding zero.
    0: row-major, 4 columns per byte (oracle.direct_np.pack_codes_rowmajor; SG3OPS/filtered_lrelu.cpp:87-94).
    1: row-quad bytes [ceil(rows / 4)][ceil16(cols)] (csrc/filtered_lrelu_mfma.hip).
    2: column-blocked row-quads, see decode_layout2 (csrc/filtered_lrelu_wave.hip)."""
    codes = np.asarray(codes).astype(np.uint8)
    assert codes.ndim == 4 and codes.max(initial=0) <= 3
    if layout == 0:
        return dnp.pack_codes_rowmajor(codes)
    shq, swq = sign_tensor_shape(layout, codes.shape[2], codes.shape[3])
    q = _quads(codes, shq, swq)
    if layout == 1:
        return q
    assert layout == 2
    n, c = q.shape[:2]
    b = q.reshape(n, c, shq // 16, 4, 4, swq // 16, 16)                   # [V / 4][V % 4][gq][blk][col in block]
    return np.ascontiguousarray(np.transpose(b, (0, 1, 5, 2, 4, 6, 3))).reshape(n, c, shq, swq)


def decode_layout2(s, sh_rows):
    """uint8 [N, C, shq, swq] buffer in layout 2 -> codes [N, C, 4 shq, swq].  Byte of quad-row q, column c:
    [c / 16][V / 4][q % 4][c % 16][V % 4] with V = q / 4 (csrc/filtered_lrelu_wave.hip)."""
    n, c, shq, swq = s.shape
    assert shq % 16 == 0 and swq % 16 == 0
    b = s.reshape(n, c, swq // 16, shq // 16, 4, 16, 4)                   # [blk][V4][gq][col in block][V % 4]
    b = np.transpose(b, (0, 1, 3, 6, 4, 2, 5)).reshape(n, c, shq, swq)    # quad-row = (V4 * 4 + V % 4) * 4 + gq; col = blk * 16 + col in block
    codes = np.stack([(b >> (2 * r)) & 3 for r in range(4)], axis=3).reshape(n, c, 4 * shq, swq)
    return codes[:, :, :sh_rows]


def decode_codes(s, layout):
    """The inverse of encode_codes: EVERY code the tensor holds, padding included -- [N, C, sh, 4 swb] (layout 0) or
    [N, C, 4 sh, swb] (layouts 1, 2): the array a kernel's window is taken from."""
    s = np.asarray(s)
    assert s.dtype == np.uint8 and s.ndim == 4
    if layout == 0:
        return np.stack([(s >> (2 * k)) & 3 for k in range(4)], axis=-1).reshape(*s.shape[:3], 4 * s.shape[3])
    if layout == 1:
        return _unquads(s)
    assert layout == 2
    return decode_layout2(s, 4 * s.shape[2])


# ------------------------------------------------------------------------------------------------- filters and kernel cases
@functools.lru_cache(maxsize=None)
def filters():
    """The 12- and 24-tap filters of the 256^2 generator (oracle.generator.plan) and the 12 x 12 radial filter of the layer
    schedule's radial configuration, as float32 numpy arrays."""
    from oracle import generator as ogen
    pl = ogen.plan(256, 4, 1, {})
    by = {L['name']: L for L in pl['enc'] + pl['dec']}
    f12, f24 = by['encoder_4']['fu'], by['encoder_4']['fd']
    assert tuple(f12.shape) == (12,) and tuple(f24.shape) == (24,) and tuple(by['L3_52_512']['fu'].shape) == (24,)
    from afcm_amd import layer_schedule
    rl = layer_schedule.plan(256, 4, 1, {'use_radial_filters': True})
    fr = next(L['fd'] for L in rl['enc'] + rl['dec'] if L['fd'] is not None and L['fd'].ndim == 2)
    assert tuple(fr.shape) == (12, 12)
    return {'f12': np.asarray(f12, dtype=np.float32), 'f24': np.asarray(f24, dtype=np.float32), 'f24u': np.asarray(by['L3_52_512']['fu'], dtype=np.float32),
            'r12': np.asarray(fr, dtype=np.float32)}


# kernel case -> (up, down, up filter, down filter) of a call: the three resampling cases of the model
KERNELS = {'u2d2': (2, 2, 'f12', 'f12'), 'u2d4': (2, 4, 'f12', 'f24'), 'u4d2': (4, 2, 'f24u', 'f12')}
# the sign-reading call behind a forward of each case (up / down and the filters swapped)
BACKWARD_OF = {'u2d2': 'u2d2', 'u2d4': 'u4d2', 'u4d2': 'u2d4'}
GAIN, SLOPE = float(np.sqrt(2)), 0.2
CLAMP = 8.0            # of the forwards of the padding sweep; a sign-reading call takes none (the codes carry it)

# bounds of the project: fraction of max(1, |ref|max).  fp32: TOL of tests/test_gpu_ops.py; matrix cores: the forward bounds of
# test_filtered_lrelu_16bit_matrix_core_path / test_wave_kernels_*; exact kernels on 16-bit data: test_filtered_lrelu_16bit_io.
TOL_F32 = 2e-5
TOL_MATRIX = {'float16': 6e-3, 'bfloat16': 4e-2}
TOL_EXACT16 = {'float16': 4e-3, 'bfloat16': 3e-2}
TEETH = 5.0            # a misplaced window must move the reference by this many times the allowed error


def out_size(n, up, down, p0, p1, fut, fdt):
    """Output extent of the op along one axis (0 or less: invalid), csrc/filtered_lrelu.hip shapes_and_plan."""
    c = n * up + p0 + p1 - (fut - 1)
    return (c - (fdt - 1) + (down - 1)) // down if c > fdt - 1 else 0


def first_pad(n, up, down, p0, fut, fdt, even, at_least=1):
    """The first p1 >= p0 for which the output is valid, `at_least` long (and its extent even, if asked for)."""
    p1 = p0
    while True:
        o = out_size(n, up, down, p0, p1, fut, fdt)
        if o >= at_least and not (even and o % 2):
            return p1
        p1 += 1


def geometry(kern, yh, yw, mx=5, my=6):
    """Input size and padding of a forward of `kern` with a yh x yw output whose backward reads its codes at (mx, my) mod 16 (my >= up:
    the aligned sign-reading call moves its strips' origin up, oy0 < 0): px0 / py0 as sweep_case, the input extent the
    smallest even one for which px1 >= px0 - up gives exactly the output asked for."""
    up, down, fu, fd = KERNELS[kern]
    F = filters()
    fut, fdt = len(F[fu]), len(F[fd])
    k = up // 2

    def axis(t, m):
        p0 = m + fut - 1 - 16 * k
        need = (t - 1) * down + 1 + (fdt - 1) + (fut - 1)          # n up + p0 + p1 for the smallest upsampled extent that gives t outputs
        n = max(2, -(-(need - 2 * p0) // up))
        n += n & 1
        p1 = need - n * up - p0
        assert out_size(n, up, down, p0, p1, fut, fdt) == t
        return n, p0, p1

    w, px0, px1 = axis(yw, mx)
    h, py0, py1 = axis(yh, my)
    return h, w, [px0, px1, py0, py1]


# ------------------------------------------------------------------------------------------------- (a) padding sweep, public op
def sweep_case(kern, mx, my, h=20, w=20, dtype='float16', seed=0):
    """One forward of the public op whose backward reads its codes at (sx, sy) = (mx, my) mod 16: px0 = mx + (fu taps - 1) - 16 k
    (k = 1 for up 2, 2 for up 4), px1 the first value >= px0 that gives an output of even width, 4 at least; likewise py0 / py1 from my
    (any parity)."""
    up, down, fu, fd = KERNELS[kern]
    F = filters()
    fut, fdt = len(F[fu]), len(F[fd])
    k = up // 2
    px0, py0 = mx + fut - 1 - 16 * k, my + fut - 1 - 16 * k
    px1 = first_pad(w, up, down, px0, fut, fdt, True, 4)
    py1 = first_pad(h, up, down, py0, fut, fdt, False, 4)
    return dict(kern=kern, read_kern=BACKWARD_OF[kern], mx=mx, my=my, h=h, w=w, dtype=dtype, padding=[px0, px1, py0, py1], seed=seed,
                id=f'{kern}-mx{mx}-my{my}-{h}x{w}-{dtype}')


def read_plan(case):
    """(oy0, dshift, rows, toh, strips) of the wave read kernel behind a sweep case, restated from flrelu_plan
    (csrc/filtered_lrelu.hip): sy = py0 - (fu taps - 1), m = sy mod 16, oy0 = -(m / down'), dshift = m % down' with down' the read
    call's down = the forward's up; strips of 32 rows, or one of 48 for up 2 / down 2 when 32 < rows <= 48."""
    up = KERNELS[case['kern']][0]
    m = case['my'] % 16
    oy0, dshift = -(m // up), m % up
    rows = case['h'] - oy0
    toh = 48 if (case['read_kern'] == 'u2d2' and 32 < rows <= 48) else 32
    return oy0, dshift, rows, toh, -(-rows // toh)


def sweep_cases():
    cases = []
    for kern in KERNELS:
        up = KERNELS[kern][0]
        for m in range(16):
            cases.append(sweep_case(kern, m, m))
        # bf16: one m per dshift value of the read kernel (m % up), on different oy0
        for m in {2: (6, 13), 4: (4, 9, 14, 3)}[up]:
            cases.append(sweep_case(kern, m, m, dtype='bfloat16', seed=4 if (kern, m) == ('u4d2', 14) else 1))    # (seeds: see BF16_SEEDS)
        # px0 != py0
        for mx, my in ((3, 12), (14, 1), (8, 7)):
            cases.append(sweep_case(kern, mx, my))
        # heights: rows = h - oy0 of the read call on both sides of the strip thresholds (see read_plan; checked in
        # test_flrelu_read_ref_cpu.py::test_sweep_heights_reach_every_strip_count)
        if kern == 'u2d2':
            hm = [(28, 8), (30, 6), (42, 12), (42, 14), (70, 5)]        # rows 32 | 33 (48-row strip only through oy0) | 48 | 49 (two strips) | 72 (three)
        elif kern == 'u2d4':                                            # read kernel up 4 / down 2
            hm = [(28, 9), (30, 6), (58, 12), (70, 3)]                  # rows 32 | 33 | 64 | 71
        else:                                                           # read kernel up 2 / down 4
            hm = [(30, 11), (30, 12), (61, 15), (70, 6)]                # rows 32 | 33 | 64 | 71
        for h, m in hm:
            cases.append(sweep_case(kern, (m + 5) % 16, m, h=h))
    return cases


def sweep_cfg(case):
    up, down = KERNELS[case['kern']][:2]
    return (up, down, *case['padding'], GAIN, SLOPE, CLAMP, False, 0, 0, 0)


def sweep_setup(case):
    """Everything but the GPU of a sweep case: x and the cotangent r as float64 arrays of 16-bit-representable values, the
    forward cfg and the cfg of the sign-reading call behind its backward (filtered_lrelu._backward_cfg, layout 2), the filters, the bound.
    Clamp 8 with planes scaled past it, as test_wave_kernels_clamp does, so that code 2 occurs."""
    import zlib
    import torch
    from afcm_amd.torch_utils.ops import filtered_lrelu as flr
    up, down, fu, fd = KERNELS[case['kern']]
    F = filters()
    rng = np.random.default_rng(zlib.crc32(case['id'].encode()) + case['seed'])
    h, w = case['h'], case['w']
    x = rng.standard_normal((2, 2, h, w))
    x[0, 0] *= 40.0
    x[1, 1, : h // 2] *= 12.0
    x[1, 0, :, : w // 3] *= 300.0
    if case['dtype'] == 'bfloat16':
        x *= 100.0                # most elements clamp (gradient 0), see direct_inputs: the bf16 bound needs the sparser factors
    px0, px1, py0, py1 = case['padding']
    yh, yw = out_size(h, up, down, py0, py1, len(F[fu]), len(F[fd])), out_size(w, up, down, px0, px1, len(F[fu]), len(F[fd]))
    r = rng.standard_normal((2, 2, yh, yw)) * (32.0 if case['dtype'] == 'bfloat16' else 1.0)      # (bf16: |ref|max stays above 1)
    cfg = sweep_cfg(case)
    bcfg = flr._backward_cfg(cfg, torch.from_numpy(F[fu]), torch.from_numpy(F[fd]), x.shape, r.shape, 2)
    return dict(x=round_to(x, case['dtype']), r=round_to(r, case['dtype']), cfg=cfg, bcfg=bcfg, fu=F[fu], fd=F[fd],
                tol=TOL_MATRIX[case['dtype']])


def upsampled_grid(shape, cfg, fu):
    """(rows, cols) of the upsampled grid of a call: the window a sign-reading call takes from the code array."""
    up, _, px0, px1, py0, py1 = cfg[:6]
    fw, fh = (1, 1) if fu is None else (fu.shape[-1], fu.shape[0])
    return shape[2] * up + py0 + py1 - (fh - 1), shape[3] * up + px0 + px1 - (fw - 1)


# ------------------------------------------------------------------------------------------------- (b), (c) direct read calls
def offsets(rows, cols, urows, ucols, mod_x=16):
    """(sx, sy, kind) of the direct read calls on a rows x cols code array seen through a urows x ucols window: 16 consecutive sy,
    16 (or 2 x mod_x + 1, both signs, for the byte-shifting layout 0) consecutive sx, windows that start above / left of the tensor,
    windows that run past its bottom / right edge (by up to half the window: a window that keeps only a sliver of the tensor reads too
    few codes for a misplacement to show), and one that lies wholly outside."""
    out = [(5, sy, 'sy') for sy in range(16)]
    out += [(sx, 6, 'sx') for sx in (range(16) if mod_x == 16 else range(-4, 5))]
    out += [(-1, 3, 'left'), (-7, -2, 'above-left'), (2, -1, 'above'), (-(ucols // 3), -(urows // 2), 'above-left'), (4, -(urows // 2), 'above')]
    out += [(3, rows - urows + 5, 'below'), (cols - ucols + 9, 2, 'right'), (cols - 2 * ucols // 3, rows - 2 * urows // 3, 'below-right'),
            (cols - ucols // 2, 7, 'right'), (1, rows - urows // 2, 'below')]
    out += [(((cols + 15) & ~15) + 3, 3, 'outside')]
    return out


def direct_case(name, family, layout, dtype, up, down, fu, fd, n, c, h, w, pad0=None, flip=False, mod_x=16, tol=None, seed=0):
    """One geometry of a direct sign-reading call `_run(dy, fu, fd, None, si, cfg, False)`; the offsets are swept inside.
    fu / fd: keys of filters() or None (pointwise).  pad0 = (px0, py0); px1 / py1 are the first values that give a valid output
    (of even width for the matrix-core kernels)."""
    F = filters()
    fut_w = 1 if fu is None else F[fu].shape[-1]
    fut_h = 1 if fu is None else F[fu].shape[0]
    fdt_w = 1 if fd is None else F[fd].shape[-1]
    fdt_h = 1 if fd is None else F[fd].shape[0]
    px0, py0 = pad0 if pad0 is not None else (fut_w - 1 - 2, fut_h - 1 - 3)
    px1 = first_pad(w, up, down, px0, fut_w, fdt_w, layout != 0)
    py1 = first_pad(h, up, down, py0, fut_h, fdt_h, False)
    urows, ucols = h * up + py0 + py1 - (fut_h - 1), w * up + px0 + px1 - (fut_w - 1)
    # the sign tensor of a forward whose upsampled grid is 20 rows / 23 columns larger than this call's, so that the 16 consecutive offsets keep the window inside it (a real backward's is larger
    # by the other filter's taps - 1 at least; what matters here is that windows can start inside it and run off every edge)
    rows, cols = urows + 20, ucols + 23
    offs = offsets(rows, cols, urows, ucols, mod_x)
    if dtype == 'bfloat16':
        seed = BF16_SEEDS.get(name, seed)
        # windows inside the tensor only.  Where a part of the window lies outside, that part passes unchanged (code 0) and sets
        # |ref|max, and the bf16 bound of 4e-2 |ref|max is then no smaller than what a window moved by one row changes (measured:
        # 1.5 - 4.5 bounds); the float16 cases, whose bound is 7x tighter, carry those windows for both types -- the element type
        # enters the kernels' loads and stores only, not the sign-window arithmetic.
        offs = [o for o in offs if o[2] in ('sy', 'sx')]
    return dict(name=name, family=family, layout=layout, dtype=dtype, up=up, down=down, fu=fu, fd=fd, shape=(n, c, h, w),
                padding=[px0, px1, py0, py1], flip=flip, urows=urows, ucols=ucols, rows=rows, cols=cols, seed=seed,
                yh=out_size(h, up, down, py0, py1, fut_h, fdt_h), yw=out_size(w, up, down, px0, px1, fut_w, fdt_w),
                tol=tol, offsets=offs, id=f'{name}-{dtype}')


def direct_cfg(case, sx, sy):
    return (case['up'], case['down'], *case['padding'], GAIN, SLOPE, INF, case['flip'], sx, sy, case['layout'])


def direct_inputs(case):
    """(dy fp32 draw [N, C, h, w], codes uint8 [N, C, rows, cols] in {0, 1, 2}).  Code 3 is never written by a kernel.
    The codes are uniform, except for bf16: its bound is 4e-2 (3e-2) of |ref|max, and a window of uniform codes moved by one row
    moves the reference by 3 - 4.5 bounds only -- the down filter averages the ~12 (up 2 / down 2) to ~50 (down 4) independent
    factors under its taps, so the change is (std / mean of the factor) / sqrt(taps) of the result.  With codes (0, 1, 2) drawn
    at (0.04, 0.04, 0.92) the factor's std / mean is 4.1 instead of 1.1 and the same move costs 5 bounds or more (asserted in
    tests/test_flrelu_read_ref_cpu.py)."""
    import zlib
    rng = np.random.default_rng(zlib.crc32(case['id'].encode()) + case['seed'])
    dy = (rng.standard_normal(case['shape']) * (32.0 if case['dtype'] == 'bfloat16' else 1.0)).astype(np.float32)      # (bf16: |ref|max stays above 1)
    p = (0.04, 0.04, 0.92) if case['dtype'] == 'bfloat16' else (1 / 3, 1 / 3, 1 / 3)
    codes = rng.choice(3, size=case['shape'][:2] + (case['rows'], case['cols']), p=p).astype(np.uint8)
    return dy, codes


def direct_setup(case):
    """dy as a float64 array of values the case's dtype represents, the codes, the two filters (arrays or None)."""
    dy, codes = direct_inputs(case)
    F = filters()
    return dict(dy=round_to(dy, case['dtype']), codes=codes, fu=None if case['fu'] is None else F[case['fu']],
                fd=None if case['fd'] is None else F[case['fd']])


# Seeds of the bf16 cases.  A window moved by one row moves the reference by 3.5 - 9 bf16 bounds depending on the draw (the 24-tap
# down filter changes by a quarter of its peak per upsampled row at most: 6 bounds is the ceiling there); these draws clear the 5
# that test_flrelu_read_ref_cpu.py asks for at every offset.
BF16_SEEDS = {'wave-u2d4': 5, 'wave-u4d2': 1, 'wave-u2d2-tall70': 4, 'mfma_tile-u2d2': 1, 'mfma_tile-u2d4': 1, 'mfma_tile-u4d2': 2,
              'mfma_tile-u2d2-tall70': 4, 'tile-u2d4-yw41': 5}


def matrix_core_cases():
    """(b): layout 2 (wave) and layout 1 (LDS tile), the three kernel cases, both 16-bit types."""
    cases = []
    for dtype in ('float16', 'bfloat16'):
        for layout, fam in ((2, 'wave'), (1, 'mfma_tile')):
            for kern, (up, down, fu, fd) in KERNELS.items():
                cases.append(direct_case(f'{fam}-{kern}', fam, layout, dtype, up, down, fu, fd, 1, 2, 18, 20, tol=TOL_MATRIX[dtype]))
            # more than two strips / tiles
            cases.append(direct_case(f'{fam}-u2d2-tall70', fam, layout, dtype, 2, 2, 'f12', 'f12', 1, 1, 70, 12, tol=TOL_MATRIX[dtype]))
    return cases


def layout0_cases():
    """(c): the layout-0 families.  The separable tile kernels are what a 16-bit call of odd width gets."""
    T32 = TOL_F32
    cases = []
    # fp32 strip kernel: the three cases; output heights on both sides of 96 (one segment / two)
    for kern, (up, down, fu, fd) in KERNELS.items():
        cases.append(direct_case(f'strip-{kern}', 'strip', 0, 'float32', up, down, fu, fd, 1, 2, 19, 21, mod_x=4, tol=T32))
    cases.append(direct_case('strip-u2d2-tall', 'strip', 0, 'float32', 2, 2, 'f12', 'f12', 1, 1, 150, 9, mod_x=4, tol=T32))
    cases.append(direct_case('strip-u4d2-tall', 'strip', 0, 'float32', 4, 2, 'f24u', 'f12', 1, 1, 72, 7, mod_x=4, tol=T32))
    cases.append(direct_case('strip-u2d4-tall', 'strip', 0, 'float32', 2, 4, 'f12', 'f24', 1, 1, 300, 21, mod_x=4, tol=T32))
    # exact LDS-tile kernels, 16-bit with an odd width: yh on both sides of 40 (up 2 / down 2: 20- / 35-row tiles), yw on both sides
    # of 40 (up 2 / down 4: 16- / 32-column tiles), up 4 / down 2
    for dtype in ('float16', 'bfloat16'):
        t = TOL_EXACT16[dtype]
        cases.append(direct_case('tile-u2d2-yh38', 'tile', 0, dtype, 2, 2, 'f12', 'f12', 1, 2, 38, 19, mod_x=4, tol=t))
        cases.append(direct_case('tile-u2d2-yh70', 'tile', 0, dtype, 2, 2, 'f12', 'f12', 1, 1, 70, 17, mod_x=4, tol=t))
        cases.append(direct_case('tile-u2d4-yw9', 'tile', 0, dtype, 2, 4, 'f12', 'f24', 1, 2, 30, 25, mod_x=4, tol=t))
        cases.append(direct_case('tile-u2d4-yw41', 'tile', 0, dtype, 2, 4, 'f12', 'f24', 1, 1, 34, 89, mod_x=4, tol=t))
        cases.append(direct_case('tile-u4d2', 'tile', 0, dtype, 4, 2, 'f24u', 'f12', 1, 2, 17, 19, mod_x=4, tol=t))
    # radial kinds, fp32: separable up with 12 x 12 down; 12 x 12 up with separable down
    cases.append(direct_case('sufd-u2d2', 'tile', 0, 'float32', 2, 2, 'f12', 'r12', 1, 2, 21, 23, mod_x=4, tol=T32))
    cases.append(direct_case('sufd-u4d2', 'tile', 0, 'float32', 4, 2, 'f24u', 'r12', 1, 1, 15, 18, mod_x=4, tol=T32, flip=True))
    cases.append(direct_case('fusd-u2d2', 'tile', 0, 'float32', 2, 2, 'r12', 'f12', 1, 2, 23, 19, mod_x=4, tol=T32))
    cases.append(direct_case('fusd-u2d4', 'tile', 0, 'float32', 2, 4, 'r12', 'f24', 1, 1, 40, 38, mod_x=4, tol=T32, flip=True))
    # pointwise kernel with non-zero px0, py0 (1 x 1 filters, identity taps)
    cases.append(direct_case('pointwise', 'pointwise', 0, 'float32', 1, 1, None, None, 2, 2, 21, 37, pad0=(3, 2), mod_x=4, tol=T32))
    cases.append(direct_case('pointwise', 'pointwise', 0, 'float16', 1, 1, None, None, 1, 2, 9, 50, pad0=(-2, 5), mod_x=4, tol=TOL_EXACT16['float16']))
    return cases


def act_cases():
    """(c), last item: the in-place activation of the generic path (`_act_inplace`), a pointwise kernel launch without padding."""
    return [direct_case('act', 'act', 0, 'float32', 1, 1, None, None, 2, 2, 23, 35, pad0=(0, 0), mod_x=4, tol=TOL_F32),
            direct_case('act', 'act', 0, 'bfloat16', 1, 1, None, None, 1, 2, 7, 70, pad0=(0, 0), mod_x=4, tol=TOL_EXACT16['bfloat16'])]


def round_to(a, dtype):
    """float array -> float64 array of the values `dtype` ('float32' / 'float16' / 'bfloat16') represents them by."""
    import torch
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(getattr(torch, dtype)).double().numpy()


# ------------------------------------------------------------------------------------------------- teeth
def zero_block(codes, sx, sy, urows, ucols):
    """`codes` with one 16-row x 16-column block (aligned in the tensor, as the layout-2 kernels fetch them) set to 0: the block
    under the centre of the part of the window that lies inside the tensor.  None when no part does."""
    rows, cols = codes.shape[-2:]
    y0, y1 = max(0, sy), min(rows, sy + urows)
    x0, x1 = max(0, sx), min(cols, sx + ucols)
    if y1 <= y0 or x1 <= x0:
        return None
    by, bx = ((y0 + y1) // 2) & ~15, ((x0 + x1) // 2) & ~15
    out = codes.copy()
    out[..., by:by + 16, bx:bx + 16] = 0
    return out
