"""float64 / exact restatements of the per-plane passes (afcm_amd/csrc/conv2d_planes.hip: scale_planes, axpy_planes, plane_dot*, amax_bits, split16,
unscale) and of layer_bwd_coefs (modulation.hip), each FROM ITS HEADER COMMENT, not from the kernel body; integer models of the kernels' index
arithmetic and launch geometry (which loop trips run, which launch exceeds its block cap, where the row reciprocal is inexact); and the cases
that tests/test_plane_passes_ref_cpu.py (no GPU: the restatements against hand-computed values, the cases against the integer models) and
tests/test_gpu_plane_passes.py (the kernels against the restatements) share.  Everything here is torch on whatever device its inputs are on."""
import itertools

import numpy as np
import torch

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = (BF16, F16, F32)
NAN, INF = float('nan'), float('inf')


def esize(dtype):
    return 4 if dtype == F32 else 2


def vec_elems(dtype):
    """E: elements of one 16-byte vector."""
    return 16 // esize(dtype)


def data(shape, dtype, seed):
    """Seeded normal data, drawn on the host in fp32 and rounded to ``dtype`` (the same values in the CPU and the GPU test)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype)


def pitched(t, ld, fill=NAN):
    """A row-pitched copy of t ([N, C, H, W] -> a view of [N, C, H, ld]) whose padding columns hold ``fill``."""
    n, c, h, w = t.shape
    assert ld >= w
    buf = torch.full([n, c, h, ld], fill, dtype=t.dtype, device=t.device)
    buf[..., :w] = t
    return buf[..., :w]


# ---- restatements -----------------------------------------------------------------------------------------------------------------------
def plane_dot(a, b=None, w=None):
    """(sum, bar): out[plane] = sum over the plane of a * b (b None: of a) in float64 -- over ``[..., :w]`` of a pitched buffer -- and the
    project's bound for an fp32-accumulated result against it (test_plane_dot_matches_torch): 1e-5 * sum |a| |b| + 1e-6."""
    a = a.double() if w is None else a[..., :w].double()
    b = torch.ones_like(a) if b is None else (b.double() if w is None else b[..., :w].double())
    return (a * b).sum(dim=(2, 3)), 1e-5 * (a.abs() * b.abs()).sum(dim=(2, 3)) + 1e-6


def gate_real(flags, gz, next_scale=None, gskip=None):
    """[planes] bool: the planes of afcm_plane_dot_gated_ld that take the real dot product -- flagged in any slot, or (gskip given) the two
    sums cancel: 8 |gz - nsc gsk| < |gz| + |nsc gsk|.  float64; the tests keep every plane a factor of two away from the threshold."""
    real = (flags != 0).any(dim=-1).reshape(-1)
    if gskip is not None:
        z = gz.double().reshape(-1)
        k = gskip.double().reshape(-1) * (1.0 if next_scale is None else next_scale.double().reshape(-1))
        real = real | (8 * (z - k).abs() < z.abs() + k.abs())
    return real


def gate_closed_form(out_scale, gz, next_scale=None, gskip=None):
    """out = osc * (gz - nsc * gsk) of the other planes, every operation rounded to fp32 (nsc, gsk None: 1, 0)."""
    assert all(t is None or t.dtype == F32 for t in (out_scale, gz, next_scale, gskip))
    k = torch.zeros_like(gz) if gskip is None else (gskip if next_scale is None else next_scale * gskip)
    return out_scale * (gz - k)


def layer_bwd_coefs(psum, out_scale=None, next_scale=None, bias=None, gz=None, dysy=None):
    """float64, from the comment above layer_bwd_coefs_kernel (psum [N, O, slots]; the others [N, O], bias [O]):
        ps[n, o]     = sum over the slots of psum
        db[o]        = sum_n ps / d                       (d = out_scale, None: 1)
        d_next[n, o] = <g, z> / s_next                    (0 where s_next == 0)
        d_out[n, o]  = (<dys, y> - b ps) / d^2            (b = bias, None: 0)
    Returns {name: (value, bar)} for the outputs whose inputs are given; bar = 1e-5 of the sum of the magnitudes of the output's terms."""
    p = psum.double()
    ps = p.sum(dim=2)
    d = torch.ones_like(ps) if out_scale is None else out_scale.double()
    out = {'db': ((ps / d).sum(dim=0), 1e-5 * (p.abs().sum(dim=2) / d.abs()).sum(dim=0))}
    if next_scale is not None and gz is not None:
        ns = next_scale.double()
        v = torch.where(ns != 0, gz.double() / torch.where(ns != 0, ns, torch.ones_like(ns)), torch.zeros_like(ns))
        out['d_next'] = (v, 1e-5 * v.abs())
    if out_scale is not None and dysy is not None:
        b = torch.zeros(ps.shape[1], dtype=torch.float64, device=ps.device) if bias is None else bias.double()
        out['d_out'] = ((dysy.double() - b * ps) / d ** 2, 1e-5 * (dysy.double().abs() + b.abs() * p.abs().sum(dim=2)) / d ** 2)
    return out


def bound_word(value):
    """The int32 word amax_bits leaves for a largest magnitude ``value``: its fp32 bit pattern."""
    return torch.tensor([value], dtype=F32).view(torch.int32)


def unscale(t, bound_a=None, bound_b=None):
    """t * (1 / (g_a g_b)) in fp32, g from conv2d.pow2_factor of each bound word (None: 1) -- a power of two, so the product is exact."""
    from afcm_amd.torch_utils.ops.conv2d import pow2_factor
    g = (1.0 if bound_a is None else pow2_factor(bound_a)) * (1.0 if bound_b is None else pow2_factor(bound_b))
    assert np.frexp(g)[0] == 0.5
    return t * torch.tensor(1.0 / g, dtype=F32, device=t.device)


def scale_planes(x, scale, out_dtype):
    """y[plane] = x[plane] * scale[plane] (None: 1): the fp32 product, rounded to nearest even into ``out_dtype``."""
    v = x.float()
    if scale is not None:
        v = v * scale.float().reshape(x.shape[0], x.shape[1], 1, 1)
    return v.to(out_dtype)


def axpy_planes(a, b, scale):
    """y[plane] = a[plane] + scale[plane] * b[plane] (None: 1), summed in fp32, one rounding into the tensors' type."""
    sb = b.float() if scale is None else scale.float().reshape(a.shape[0], a.shape[1], 1, 1) * b.float()
    return (a.float() + sb).to(a.dtype)


def bits(t):
    """The bit patterns of a floating-point tensor."""
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def same_values(got, want):
    """Elementwise passes are exact: the same NaN positions, bit-identical everywhere else (infinities and signed zeros included)."""
    assert got.dtype == want.dtype and got.shape == want.shape
    nan = want.isnan()
    return bool(torch.equal(got.isnan(), nan)) and bool(torch.equal(bits(got)[~nan], bits(want)[~nan]))


# ---- integer models of the kernels ------------------------------------------------------------------------------------------------------
def ceil_div(a, b):
    return -(-a // b)


def rows_reciprocal(nvec):
    """The 32-bit round-up reciprocal plane_dot_rows_kernel divides by: ceil(2^32 / nvec), truncated to 32 bits (nvec == 1: 0)."""
    return (((1 << 32) + nvec - 1) // nvec) & 0xffffffff


def rows_quotient(ic, nvec, fixed=True):
    """row of vector ``ic`` (numpy int64 array) as the kernel computes it: umulhi(ic, reciprocal); ``fixed``: nvec == 1 takes ic itself and a
    quotient whose row starts after ic steps back by one."""
    ic = np.asarray(ic, dtype=np.uint64)
    row = (ic * np.uint64(rows_reciprocal(nvec))) >> np.uint64(32)
    if fixed:
        if nvec == 1:
            row = ic.copy()
        row = row - (row * np.uint64(nvec) > ic).astype(np.uint64)
    return row.astype(np.int64)


def rows_first_wrong(h, w, dtype, fixed):
    """The first vector index of an h x w plane whose row differs from ic // nvec, or None."""
    nvec = ceil_div(w, vec_elems(dtype))
    ic = np.arange(h * nvec, dtype=np.int64)
    bad = np.nonzero(rows_quotient(ic, nvec, fixed) != ic // nvec)[0]
    return int(bad[0]) if bad.size else None


def rows_host_admits(h, w, dtype, lda=0, ldb=0):
    """afcm_plane_dot_ld's shape checks (pointer alignment apart)."""
    lda, ldb = lda or w, ldb or w
    return (lda >= w and ldb >= w and w >= vec_elems(dtype) and (esize(dtype) == 4 or (w | lda | ldb) % 2 == 0)
            and h * max(lda, ldb) < (1 << 31) // 16)


def rows_variant(h, w, dtype):
    """('wave' | 'workgroup', trips of the 4-vector loop of the busiest lane)."""
    wave = h * w * esize(dtype) <= 16384
    total = h * ceil_div(w, vec_elems(dtype))
    return ('wave' if wave else 'workgroup'), ceil_div(total, 4 * (64 if wave else 256))


def dense_variant(hw, dtype):
    return 'wave' if hw * esize(dtype) <= 16384 else 'workgroup'


def dense_split(plane, hw, dtype):
    """(head, nv, tail) of plane ``plane``: scalar elements before the first 16-byte boundary, whole vectors, scalar elements after."""
    e = vec_elems(dtype)
    head = min((e - (plane * hw) % e) % e, hw)
    nv = (hw - head) // e
    return head, nv, hw - head - nv * e


def dense_trips(nv, dtype, hw, with_b):
    """{loop: lanes x trips} of plane_dot_kernel (4-load, 2-load, 1-load tails) or plane_dot_wave_kernel (2-load, 1-load) over nv vectors."""
    wave = dense_variant(hw, dtype) == 'wave'
    nthr = 64 if wave else 256
    out = {'load4': 0, 'load2': 0, 'load1': 0}
    for t in range(nthr):
        i = t
        if not wave and with_b:
            while i + 3 * nthr < nv:
                out['load4'] += 1
                i += 4 * nthr
        while i + nthr < nv:
            out['load2'] += 1
            i += 2 * nthr
        if i < nv:
            out['load1'] += 1
    return out


def launch_blocks(kernel, planes, hw):
    """(blocks the work asks for, the cap of the launch) of the grid-stride kernels."""
    groups = planes * ceil_div(hw, 4)
    if kernel in ('scale_planes', 'split16'):
        return ceil_div(groups, 256), (2048 if kernel == 'scale_planes' else 4096)
    if kernel == 'unscale':
        return ceil_div(planes * hw, 256), 2048
    if kernel == 'amax_bits':
        return max(1, ceil_div(planes * hw // 16, 256)), 2048
    if kernel == 'axpy_planes':                                   # grid.y: one plane per workgroup row
        return planes, 65535
    raise KeyError(kernel)


def amax_vector_path(hw, byte_offset):
    return byte_offset % 16 == 0 and hw % 4 == 0


# ---- shared cases -----------------------------------------------------------------------------------------------------------------------
def _row_shapes(dtype):
    e = vec_elems(dtype)
    tall = 16384 // (e * esize(dtype)) + 6                        # w == E and h * w * esize > 16384: the workgroup variant
    shapes = [(15, h, e) for h in (1, 5, 70)] + [(1, 5, e), (5, 5, e), (15, tall, e), (1, tall, e)]
    shapes += [(15, h, w) for w in ((10, 14) if e == 8 else (5, 7)) for h in (5, 70)]
    shapes += [(1, 40, 100), (5, 40, 100), (15, 40, 100), (1, 70, 150), (5, 70, 150), (15, 70, 150)]
    return shapes


PLANE_SPLITS = {1: (1, 1), 5: (1, 5), 15: (3, 5)}                 # planes -> (N, C)
ROW_CASES = [(dt, p, h, w) for dt in DTYPES for (p, h, w) in _row_shapes(dt)]
ROW_BIG = (F32, 1, 258, 16368, 16368 + 16)                        # (dtype, planes, h, w, pitch): the round-up reciprocal is one over in row 256


def row_pitches(w):
    """Two different pitches for a w-wide plane (even, no multiple of 16 bytes apart from chance: rows start on 4-byte boundaries only)."""
    lda = (w + 7) // 8 * 8 + 10
    return lda, lda + 22


def row_operands(dtype, planes, h, w, seed=11):
    n, c = PLANE_SPLITS[planes]
    return data((n, c, h, w), dtype, seed), data((n, c, h, w), dtype, seed + 1)


GATED_SHAPES = [(BF16, 5, 8), (F32, 5, 4), (BF16, 70, 150), (F32, 70, 150)]     # (dtype, h, w): w == E on the wave variant, one workgroup shape
GATED_KINDS = ('plain', 'flagged', 'cancel', 'plain', 'flagged', 'cancel', 'plain', 'flagged')     # 8 planes: two workgroups of four waves, mixed
GATED_SLOTS = 3
GATED_MODES = ('all', 'no_next_scale', 'no_gskip')


def gated_inputs(mode, seed=3):
    """(flags [8, 3] int32, osc, gz, nsc | None, gsk | None), fp32 [8].  'flagged': the last slot only.  'cancel': nsc gsk = (31/32) gz, the
    difference is 1/63 of the two sizes (threshold 1/8); the others: nsc gsk = -gz / 2, the difference is all of them."""
    g = torch.Generator().manual_seed(seed)
    p = len(GATED_KINDS)
    flags = torch.zeros([p, GATED_SLOTS], dtype=torch.int32)
    for i, kind in enumerate(GATED_KINDS):
        if kind == 'flagged':
            flags[i, GATED_SLOTS - 1] = 1 + i
    osc = torch.rand(p, generator=g) + 0.5
    gz = (torch.rand(p, generator=g) + 1.0) * torch.tensor([1.0, -1.0] * (p // 2))
    nsc = None if mode == 'no_next_scale' else torch.rand(p, generator=g) + 0.5
    ratio = torch.tensor([31.0 / 32.0 if kind == 'cancel' else -0.5 for kind in GATED_KINDS])
    gsk = None if mode == 'no_gskip' else gz * ratio / (1.0 if nsc is None else nsc)
    return flags, osc, gz, nsc, gsk


def _dense_sizes(dtype):
    e, es = vec_elems(dtype), esize(dtype)
    wave = [1, 2, e - 1] + [e * nv + 3 for nv in (63, 64, 65, 127, 128, 129)] + [16384 // es, 16384 // es + 1]
    group = [e * nv + 3 for nv in (1024, 1025, 1279, 1280, 1281, 1535, 1536, 1537, 1791, 1792, 1793, 2047)]
    return wave + group


DENSE_CASES = [(dt, hw) for dt in DTYPES for hw in _dense_sizes(dt)]
DENSE_NC = (3, 5)                                                 # 15 planes: an odd hw puts each on a different 16-byte phase

SCALE_PAIRS = [(F32, F32), (F32, BF16), (F32, F16), (BF16, BF16), (F16, F16), (BF16, F32), (F16, F32)]
SCALE_SHAPES = [(3, 5, 1, hw) for hw in (1, 2, 3, 7, 8)] + [(2, 3, 6, 10)]
SCALE_BIG = (8, 16, 130, 130)                                     # 128 planes x 4225 groups of 4: 2113 workgroups against a cap of 2048


def scale_input(shape, dtype, seed=21):
    """Normal data with NaN, +-inf, a value that overflows float16 and a signed zero planted where the shape has room."""
    x = data(shape, dtype, seed)
    flat = x.view(-1)
    for i, v in zip(range(0, flat.numel(), max(1, flat.numel() // 6)), (NAN, INF, -INF, 1e5, -0.0, -7e4)):
        flat[i] = v
    return x


def plane_scale(n, c, seed=22):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand([n, c], generator=g) + 0.5) * torch.tensor([1.0, -1.0] * ((n * c + 1) // 2))[:n * c].view(n, c)


AXPY_CASES = [(65600, 8), (3, 8 * 2049)]                          # (planes, hw): past grid.y's 65535; three grid.x blocks per plane
UNSCALE_NUMELS = (1, 255, 257, 2048 * 256 + 300)
UNSCALE_BOUNDS = ((3.7, 1234.5), (3.7, None), (None, 2.0 ** -20), (None, None))
SPLIT_BIG = (2, 17, 352, 352)                                     # 4 212 736 elements: 4114 workgroups against a cap of 4096
AMAX_BIG = 2900                                                   # 2900^2 elements: 2054 workgroups against a cap of 2048
COEF_CASES = list(itertools.product((1, 2, 64, 65, 130), (1, 5), (1, 3)))     # (N, O, slots)


def coef_inputs(n, o, slots, seed=31):
    """psum [n, o, slots], out_scale, next_scale (exact zeros among its entries), bias [o], gz, dysy -- fp32."""
    g = torch.Generator().manual_seed(seed + 1000 * n + 10 * o + slots)
    psum = torch.randn([n, o, slots], generator=g)
    osc = torch.rand([n, o], generator=g) + 0.5
    nsc = torch.rand([n, o], generator=g) + 0.5
    nsc.view(-1)[::3] = 0.0
    return psum, osc, nsc, torch.randn([o], generator=g), torch.randn([n, o], generator=g), torch.randn([n, o], generator=g)
