"""Re-layouts of an operand and the audit of base-pointer preconditions (test_view_layouts_cpu.py, test_gpu_view_layouts.py).

A kernel sees an operand through a base pointer and strides.  The Python ops promise that ANY tensor of the right shape and dtype
computes what a fresh dense one computes; the kernels promise much less: dense or row-pitched planes whose base lies on a grid of 4,
8 or 16 bytes.  Between the two stand ``.contiguous()``, ``_rows.rows`` and ``_rows.dense`` -- and a contiguous view may sit at any
element offset of its storage (``buf[1:].view(shape)``), where ``.contiguous()`` leaves it.

``variants(t)`` yields named re-layouts of ``t`` with equal values and shape; ``PRECONDITIONS`` lists, per C entry point, which
arguments are tensor base pointers and the alignment each needs, with the line it was read from; ``audit(lib, monkeypatch)`` puts a
wrapper around each listed function that refuses a call whose pointer is off its grid BEFORE forwarding it, so that a missing
copy in the Python layer shows as an AssertionError naming the entry point and the argument, and nothing is launched.

No GPU, no library needed.
"""
import collections
import ctypes

import torch

F32, F16, BF16 = 0, 1, 2                    # dtype codes of the C ABI (afcm_amd/_lib.py)
ESIZE = {F32: 4, F16: 2, BF16: 2}
SLACK = 8                                   # spare elements of an offset variant's buffer


# ---- re-layouts ----------------------------------------------------------------------------------------------------------------------------
def _offset(t, k):
    buf = torch.empty([t.numel() + SLACK], dtype=t.dtype, device=t.device)
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def slice_of(t, dim, lead, extra):
    """``t`` as the slice [lead, lead + size) along ``dim`` of a fresh tensor that is ``extra`` larger there (the rest: NaN)."""
    shape = list(t.shape)
    shape[dim] += extra
    big = torch.full(shape, float('nan'), dtype=t.dtype, device=t.device)
    v = big.narrow(dim, lead, t.shape[dim])
    v.copy_(t)
    return v


def row_extra(w):
    """Columns by which the buffer of ``row_slice`` is wider than the view: the row stride w + extra is odd, so it is neither w nor a
    pitch of _rows.py (those are even)."""
    return 3 if w % 2 == 0 else 4


def per_plane(t):
    """The [N, C, 1, 1] tensor ``t`` is an expansion of, or None."""
    if t.ndim != 4:
        return None
    pc = t[:, :, :1, :1]
    return pc if bool((t == pc).all()) else None


def variants(t, cotangent=False):
    """(name, tensor) pairs: ``t`` in every layout of the module docstring that its rank allows.  ``expanded`` only for a cotangent
    that is constant on every plane (the caller draws such a one for this variant)."""
    t = t.detach()
    yield 'aligned', t.contiguous().clone()
    yield 'offset1', _offset(t, 1)
    yield 'offset2', _offset(t, 2)
    if t.ndim == 4:
        yield 'channels_last', t.contiguous().clone(memory_format=torch.channels_last)
    if t.ndim >= 2:
        yield 'channel_slice', slice_of(t, 1, 1, 2)
    if t.ndim >= 2:
        yield 'row_slice', slice_of(t, t.ndim - 1, 1, row_extra(t.shape[-1]))
    if cotangent and per_plane(t) is not None:
        yield 'expanded', per_plane(t).contiguous().clone().expand(t.shape)


def variant(t, name, cotangent=False):
    for k, v in variants(t, cotangent):
        if k == name:
            return v
    raise KeyError(f'{name}: no such layout for a tensor of shape {tuple(t.shape)}')


def dense_strides(shape):
    out, s = [], 1
    for n in reversed(shape):
        out.append(s)
        s *= n
    return tuple(reversed(out))


def check_claim(name, v, base_align=64):
    """What the layout ``name`` claims about ``v``, asserted.  ``base_align``: the alignment of fresh allocations on v's device (CPU:
    64 bytes; the caching device allocator: 512)."""
    e, shape, stride = v.element_size(), tuple(v.shape), tuple(v.stride())
    lead = v.data_ptr() - v.untyped_storage().data_ptr()
    assert v.untyped_storage().data_ptr() % base_align == 0, 'the allocation itself is not aligned'
    if name == 'aligned':
        assert v.is_contiguous() and lead == 0
    elif name in ('offset1', 'offset2'):
        k = int(name[-1])
        assert v.is_contiguous() and lead == k * e
        assert v.data_ptr() % 16 == (k * e) % 16 and v.data_ptr() % 4 == (k * e) % 4
    elif name == 'channels_last':
        n, c, h, w = shape
        assert lead == 0 and stride == (h * w * c, 1, w * c, c)
        assert v.is_contiguous() == (c == 1 or h * w == 1)
    elif name == 'channel_slice':
        inner = 1
        for k in shape[2:]:
            inner *= k
        assert lead == inner * e and stride[0] == (shape[1] + 2) * inner and stride[1:] == dense_strides(shape)[1:]
        assert v.is_contiguous() == (shape[0] == 1)
    elif name == 'row_slice':
        ld = shape[-1] + row_extra(shape[-1])
        assert lead == e and ld % 2 == 1 and stride[-1] == 1 and (len(shape) < 2 or shape[-2] == 1 or stride[-2] == ld)
        assert stride == dense_strides(shape[:-1] + (ld,))
    elif name == 'expanded':
        assert stride[2:] == (0, 0) and lead == 0
    else:
        raise KeyError(name)


# ---- the audit table -----------------------------------------------------------------------------------------------------------------------
def esize(code):
    """Any element-aligned base: a kernel that reads this operand element by element, or that looks at the address itself and takes
    vector accesses only where it allows them."""
    return ESIZE[code]


# arg: index into the entry point's arguments; field: member of the argument struct (arg is then the struct pointer) or None;
# align: bytes, or a function of the dtype code; dt: where this pointer's dtype code is (an (arg, field) pair) if not the entry's;
# cite: where the value was read.
Ptr = collections.namedtuple('Ptr', 'name arg field align cite dt', defaults=(None,))
# dtype: (arg, field) of the dtype code, None for fp32-only entry points; count: index of the element count of a struct ARRAY argument
Entry = collections.namedtuple('Entry', 'ptrs dtype count', defaults=(None, None))

_X16 = 'a 16-bit image is fetched in 8-byte raw buffer loads at dword offsets from its base: csrc/conv2d.hip:145 (comment), :477-499'
_MOD = 'csrc/modulation.hip: every access of the bank kernels is a scalar float load or store'
_MODULATION_FIELDS = ('w', 't', 'magnitude', 'w_hat', 'wsq', 'scale', 's_eff', 'd', 'r', 'g_hat', 'g_s', 'g_d', 'dw', 'dt', 'workspace')


def _flrelu_ptrs():
    return [
        Ptr('x', 0, 'x', 4, 'csrc/filtered_lrelu.hip:81 "aligned 16-bit pairs", csrc/filtered_lrelu_mfma.hip:210 "one 16-byte load from a 4-byte '
                            'aligned address", csrc/filtered_lrelu_wave.hip:243 "aligned dword pairs" (with the even widths and pitches of '
                            'filtered_lrelu.hip:84, :259 every row then starts on a dword); fp32: element size'),
        Ptr('skip', 0, 'skip', 4, 'as x: read by the same staged epilogue (csrc/filtered_lrelu.hip:259 even skip_pitch)'),
        Ptr('b', 0, 'b', esize, 'one scalar load per plane: csrc/filtered_lrelu.hip:29, filtered_lrelu_mfma.hip:285, _strip.hip:111, _tile.hip:267'),
        Ptr('signs', 0, 'signs', 4, 'the codes are read and written in dwords: csrc/filtered_lrelu.hip:50, csrc/filtered_lrelu_strip.hip:122, '
                                    'csrc/filtered_lrelu_wave.hip:391'),
        Ptr('fu', 0, 'fu', 4, 'float32 filter taps, scalar loads'),
        Ptr('fd', 0, 'fd', 4, 'float32 filter taps, scalar loads'),
        Ptr('oscale', 0, 'oscale', 4, 'float32 per-plane factor, one scalar load per plane'),
        Ptr('oscale2', 0, 'oscale2', 4, 'float32 per-plane factor, one scalar load per plane'),
    ]


PRECONDITIONS = {
    # ---- conv2d forward / data gradient
    'afcm_conv2d_ld': Entry([
        Ptr('x', 1, None, 4, _X16 + '; the direct kernel reads 2-byte elements (csrc/conv2d_direct.hip:108), the fp32 kernel dwords (csrc/conv2d.hip:175)'),
        Ptr('wpacked', 2, None, 16, '16-byte loads of the packed image: csrc/conv2d.hip:165, :436'),
        Ptr('oscale', 3, None, 4, 'float32 buffer loads from oscale + n * cout: csrc/conv2d.hip:661-671 (any cout: dword alignment)'),
        Ptr('obias', 4, None, 4, 'as oscale: csrc/conv2d.hip:662-672'),
    ], (5, None)),
    'afcm_conv2d_split': Entry([
        Ptr('x_parts', 1, None, 4, _X16 + ' (the split form of the same kernel)'),
        Ptr('wpacked', 2, None, 16, '16-byte loads of the packed image: csrc/conv2d.hip:436'),
        Ptr('oscale', 3, None, 4, 'csrc/conv2d.hip:661-671'),
        Ptr('obias', 4, None, 4, 'csrc/conv2d.hip:662-672'),
        Ptr('bound_a', 16, None, 4, 'one uint32 word'),
        Ptr('bound_b', 17, None, 4, 'one uint32 word'),
    ], (5, None)),
    'afcm_conv2d_stride2': Entry([
        Ptr('x', 1, None, 4, '8-byte raw buffer loads at dword offsets from the image base: csrc/conv2d.hip:898, :910'),
        Ptr('wpacked', 2, None, 16, '16-byte loads of the packed image: csrc/conv2d.hip:872'),
    ], (3, None)),
    # ---- conv2d weight gradient
    'afcm_conv2d_wgrad_ld': Entry([
        Ptr('dy', 2, None, 4, 'csrc/conv2d_wgrad.hip:532 "one granule = 8 pixels from a 4-byte aligned address" (LDS-DMA kernel), :1151 4-byte pieces '
                              '(dword kernel); fp32: element size.  The host checks even widths and pitches only (:1194, :1197)'),
        Ptr('x', 3, None, 4, 'as dy'),
    ], (4, None)),
    'afcm_conv2d_wgrad_dots_ld': Entry([
        Ptr('dy', 3, None, 4, 'csrc/conv2d_wgrad.hip:532 (the LDS-DMA kernel is the only one with this form: :1163)'),
        Ptr('x', 4, None, 4, 'as dy'),
        Ptr('wref', 5, None, 4, 'scalar float loads: csrc/conv2d_wgrad.hip:1055'),
    ], (6, None)),
    # ---- weight packing (float32 weights in, the kernels' image out)
    'afcm_conv2d_pack_weights': Entry([
        Ptr('dst', 0, None, 32, 'AFCM_REQUIRE csrc/conv2d.hip:1515'),
        Ptr('w', 1, None, 4, 'scalar float loads: csrc/conv2d.hip:1192')]),
    'afcm_conv2d_pack_weights2': Entry([
        Ptr('dst_fwd', 0, None, 32, 'AFCM_REQUIRE csrc/conv2d.hip:1515'),
        Ptr('dst_dgrad', 1, None, 32, 'AFCM_REQUIRE csrc/conv2d.hip:1515'),
        Ptr('w', 2, None, 4, 'scalar float loads: csrc/conv2d.hip:1192')]),
    'afcm_conv2d_pack_weights_bk': Entry([
        Ptr('dst', 0, None, 32, 'AFCM_REQUIRE csrc/conv2d.hip:1515'),
        Ptr('w', 1, None, 4, 'scalar float loads: csrc/conv2d.hip:1192')]),
    'afcm_conv2d_pack_split': Entry([
        Ptr('w', 1, None, 4, 'scalar float loads: csrc/conv2d.hip:1290'),
        Ptr('bound', 2, None, 4, 'one uint32 word')]),
    # ---- per-plane passes and the fp32 split
    'afcm_scale_planes': Entry([
        Ptr('y', 0, None, esize, 'the kernel takes vector accesses only where both bases allow them: csrc/conv2d_planes.hip:23', (4, None)),
        Ptr('x', 1, None, esize, 'csrc/conv2d_planes.hip:23', (3, None)),
        Ptr('scale', 2, None, 4, 'one scalar float load per element group: csrc/conv2d_planes.hip:27'),
    ]),
    'afcm_plane_dot': Entry([
        Ptr('a', 1, None, 16, 'AFCM_REQUIRE csrc/conv2d_planes.hip:522'),
        Ptr('b', 2, None, 16, 'AFCM_REQUIRE csrc/conv2d_planes.hip:522'),
    ], (3, None)),
    'afcm_plane_dot_ld': Entry([
        Ptr('a', 1, None, 4, 'AFCM_REQUIRE csrc/conv2d_planes.hip:548'),
        Ptr('b', 2, None, 4, 'AFCM_REQUIRE csrc/conv2d_planes.hip:548'),
    ], (3, None)),
    'afcm_plane_dot_gated_ld': Entry([
        Ptr('a', 1, None, 4, 'AFCM_REQUIRE csrc/conv2d_planes.hip:548 (shared host code)'),
        Ptr('b', 2, None, 4, 'AFCM_REQUIRE csrc/conv2d_planes.hip:548'),
    ], (3, None)),
    'afcm_split16': Entry([
        Ptr('parts', 0, None, 8, 'AFCM_REQUIRE csrc/conv2d_planes.hip:444'),
        Ptr('x', 1, None, 16, 'AFCM_REQUIRE csrc/conv2d_planes.hip:444'),
        Ptr('scale', 2, None, 4, 'scalar float loads'),
        Ptr('bound', 3, None, 4, 'one uint32 word'),
    ]),
    'afcm_amax_bits': Entry([
        Ptr('out', 0, None, 4, 'AFCM_REQUIRE csrc/conv2d_planes.hip:458'),
        Ptr('x', 1, None, 4, 'AFCM_REQUIRE csrc/conv2d_planes.hip:458; 16-byte loads only where the base allows them (:83)'),
        Ptr('scale', 4, None, 4, 'scalar float loads: csrc/conv2d_planes.hip:94'),
    ]),
    'afcm_plane_dot_parts': Entry([
        Ptr('parts', 1, None, 8, 'AFCM_REQUIRE csrc/conv2d_planes.hip:471'),
        Ptr('b', 4, None, 16, 'AFCM_REQUIRE csrc/conv2d_planes.hip:471'),
        Ptr('bound', 8, None, 4, 'one uint32 word'),
    ]),
    'afcm_unscale': Entry([Ptr('t', 0, None, 4, 'scalar float accesses')]),
    # ---- filtered_lrelu, upfirdn2d
    'afcm_filtered_lrelu': Entry(_flrelu_ptrs(), (0, 'dtype')),
    'afcm_filtered_lrelu_act': Entry([
        Ptr('x', 0, None, esize, 'the pointwise kernel reads and writes element by element: csrc/filtered_lrelu.hip:44-47'),
        Ptr('signs', 1, None, 4, 'one dword of codes per thread: csrc/filtered_lrelu.hip:50')], (2, None)),
    'afcm_upfirdn2d': Entry([
        Ptr('y', 0, None, esize, 'vector stores only where the address allows them: csrc/upfirdn2d.hip:162'),
        Ptr('x', 1, None, esize, 'the rows kernel (16-byte buffer loads) is taken only for 4-byte aligned x and y: csrc/upfirdn2d.hip:353; '
                                 'the tile and gather kernels read element by element'),
        Ptr('f', 2, None, 4, 'float32 taps, scalar loads'),
    ], (3, None)),
    # ---- dense and small ops
    'afcm_modulation_bank_fwd': Entry([Ptr(k, 0, k, 4, _MOD) for k in _MODULATION_FIELDS], None, 1),
    'afcm_modulation_bank_bwd': Entry([Ptr(k, 0, k, 4, _MOD) for k in _MODULATION_FIELDS], None, 1),
    'afcm_layer_bwd_coefs': Entry([Ptr(k, i, None, 4, _MOD) for k, i in (('db', 0), ('d_next', 1), ('d_out', 2), ('psum', 3), ('out_scale', 5),
                                                                        ('next_scale', 6), ('bias', 7), ('gz', 8), ('dysy', 9))]),
    'afcm_fc_act_fwd': Entry([
        Ptr('y', 0, None, 16, 'AFCM_REQUIRE csrc/fc_bank.hip:336'),
        Ptr('x', 1, None, 16, 'AFCM_REQUIRE csrc/fc_bank.hip:336'),
        Ptr('w', 2, None, 16, 'AFCM_REQUIRE csrc/fc_bank.hip:336'),
        Ptr('b', 3, None, 4, 'scalar float loads'),
    ]),
    'afcm_fc_act_bwd': Entry([
        Ptr('gy', 3, None, 16, 'AFCM_REQUIRE csrc/fc_bank.hip:356'),
        Ptr('y', 4, None, 16, 'AFCM_REQUIRE csrc/fc_bank.hip:356'),
    ]),
    'afcm_mapping_input_fwd': Entry([Ptr(k, i, None, 4, 'csrc/fc_bank.hip:265: scalar float accesses')
                                     for i, k in enumerate(('x0', 'z', 'c', 'ew', 'eb'))]),
    'afcm_mapping_input_bwd': Entry([Ptr(k, i, None, 4, 'csrc/fc_bank.hip:286: scalar float accesses')
                                     for i, k in enumerate(('dew', 'deb', 'gx0', 'c', 'ew', 'eb'))]
                                    + [Ptr('workspace', 12, None, 4, 'AFCM_REQUIRE csrc/fc_bank.hip:381')]),
    'afcm_pool_blocks_fwd': Entry([
        Ptr('y', 0, None, 4, 'scalar float stores: csrc/bias_act.hip:226'),
        Ptr('x', 1, None, esize, 'element loads: csrc/bias_act.hip:222'),
    ], (2, None)),
    'afcm_pool_blocks_bwd': Entry([
        Ptr('dx', 0, None, esize, 'element stores: csrc/bias_act.hip:236'),
        Ptr('gy', 1, None, 4, 'scalar float loads: csrc/bias_act.hip:236'),
    ], (2, None)),
    'afcm_l1_partials': Entry([Ptr(k, i, None, 4, 'scalar float accesses: csrc/optim.hip:158-163') for i, k in enumerate(('partials', 'a', 'b'))]),
    'afcm_l1_grad': Entry([Ptr(k, i, None, 4, 'scalar float accesses: csrc/optim.hip:167-170') for i, k in enumerate(('ga', 'a', 'b', 'gout'))]),
    'afcm_gauss_blur': Entry([
        Ptr('y', 0, None, 4, 'scalar float stores: csrc/blur.hip:197'),
        Ptr('x', 1, None, 4, 'scalar float loads into the LDS tile: csrc/blur.hip:77, :145'),
        Ptr('tmp', 2, None, 4, 'vector stores only where the address allows them: csrc/blur.hip:115'),
        Ptr('block', 7, None, 8, 'doubles of the schedule block'),
    ]),
}


# ---- the audit -----------------------------------------------------------------------------------------------------------------------------
def _addr(v):
    """The integer address behind a pointer argument as ctypes callers pass it (None, int, c_void_p, an array of c_void_p's element)."""
    if v is None:
        return 0
    if isinstance(v, int):
        return v
    return int(getattr(v, 'value', 0) or 0)


def _structs(obj, count):
    """The struct(s) behind a struct-pointer argument: a struct instance (ctypes passes it by reference), a pointer to one, or an array."""
    if isinstance(obj, ctypes.Array):
        return [obj[i] for i in range(len(obj) if count is None else count)]
    if hasattr(obj, 'contents'):
        return [obj.contents]
    return [getattr(obj, '_obj', obj)]               # (byref() result or the instance itself)


def _lookup(args, where, count=None):
    arg, field = where
    if field is None:
        return [args[arg]]
    return [getattr(s, field) for s in _structs(args[arg], count)]


def violations(name, args):
    """[(argument name, address, alignment)] for the pointers of a call of ``name`` that are off their grid."""
    entry = PRECONDITIONS[name]
    count = None if entry.count is None else int(args[entry.count])
    bad = []
    for p in entry.ptrs:
        values = _lookup(args, (p.arg, p.field), count)
        if callable(p.align):
            where = p.dt or entry.dtype
            codes = _lookup(args, where, count)
            if len(codes) != len(values):
                codes = codes * len(values)
        else:
            codes = [None] * len(values)
        for k, (v, code) in enumerate(zip(values, codes)):
            a = _addr(v)
            need = p.align(int(code)) if callable(p.align) else p.align
            if a and a % need:
                bad.append((p.name if len(values) == 1 else f'{p.name}[{k}]', a, need))
    return bad


def audit(lib, monkeypatch, names=None):
    """Wrap every listed entry point of ``lib`` (the loaded library object, or a stand-in with the same attributes): a call with a
    pointer off its grid raises AssertionError BEFORE it is forwarded, any other call is forwarded, and its name is recorded when it
    returned 0 (a launch; an entry point that declined the shape, AFCM_E_NOKERNEL, or refused its arguments launched nothing).
    Returns the list of recorded names."""
    calls = []

    def wrap(name, fn):
        def audited(*args):
            bad = violations(name, args)
            assert not bad, f'{name}: ' + '; '.join(f'{arg} = {addr:#x} is not {need}-byte aligned ({addr % need} past)' for arg, addr, need in bad)
            rc = fn(*args)
            if rc == 0:
                calls.append(name)
            return rc
        return audited

    for name in (PRECONDITIONS if names is None else names):
        monkeypatch.setattr(lib, name, wrap(name, getattr(lib, name)))
    return calls
