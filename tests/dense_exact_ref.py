"""Operands, float64 references and case tables for the exact dense-layer tests (test_dense_exact_ref_cpu.py, test_gpu_dense_exact.py):
the fc_act layers (csrc/fc_bank.hip), the style affine bank (csrc/affine_bank.hip) and the rows of the mapping input stage.

The dense kernels multiply and accumulate in fp32 on v_mfma_f32_16x16x4_f32.  With operands that are small integers times powers of
two and power-of-two gains alpha / beta, every partial sum of every order is a multiple of one quantum q and below 2^24 q, hence
exact: the split of the K chunks over 4 or 16 waves, the LDS reduction order, a contraction of ``v * alpha + bias`` into one fma, the
two-tiles-per-trip loop and the 16-row accumulation passes cannot change a bit.  Each element has ONE right answer, the float64
result converts to it exactly, and the GPU tests compare with ``torch.equal``.  At least one operand of every contraction is dense
+-1 (``pm1``): a dropped or doubled term flips the parity of the sum.

The conditions are conditions on the INPUTS, checked here on the float64 reference and never on the code under test
(``failures()`` of every case): every operand and every result is an fp32 value, and the absolute term sum behind every result,
counted in quanta, stays below 2^24.  A draw that fails is redrawn from the next seed, ``SEEDS`` draws in all; the conditions are never
relaxed, and a case that no draw satisfies is an error -- no case of any table may be dropped.

Leaky ReLU is not exact but exactly reproducible once the sum in front of it is exact: forward y = fl32(fl32(u * 0.2f) * G) for
u <= 0, fl32(u * G) otherwise (``lrelu32``, numpy float32); backward gp = fl32(gy * G) where the SAVED OUTPUT is > 0, else
fl32(gy * fl32(G * 0.2f)) (``gp32``: -0, +0 and negative outputs take the slope).  Sums of such gp are no longer order-independent,
so the lrelu backward cases (``FcLreluBwd``) use single-term cotangents: gy is non-zero at one column pi(n) = (7 n + t) mod cout per
row, pi injective on the rows that carry a cotangent, so every dx, dw and db element is one product of numbers +-2^e (times G or
G * 0.2 rounded once), or exactly zero.  Where the batch has more rows than the layer has columns (n > cout) no injective pi over
all rows exists: a launch then gives a cotangent to one window of cout consecutive rows, the other rows get none (their dx rows must
be exact zeros), and the windows take turns.  The shifts t are swept until every column has been hit.
"""
import collections
import math

import numpy as np
import torch

from conv_exact_ref import F64, LIMIT, case_id, dot_units, gen, pick, pm1, pow2, quantum, representable  # noqa: F401  (re-exported)

F32 = torch.float32
SEEDS = 3                                             # draws per case before it is an error
G32 = np.float32(1.41421356237309504880)              # kFcGain
S32 = np.float32(0.2)                                 # kFcSlope
GS32 = np.float32(G32 * S32)                          # the constant-folded kFcGain * kFcSlope of fc_gp


# ---- the float32 leaky-ReLU rules -----------------------------------------------------------------------------------------------------
def lrelu32(u):
    """act(u) of fc_act_fwd_kernel on a float64 tensor of fp32 values: two separately rounded products on the slope side."""
    v = u.numpy().astype(np.float32)
    assert (v.astype(np.float64) == u.numpy()).all()
    y = np.where(v > 0, v * G32, (v * S32) * G32)
    assert y.dtype == np.float32
    return torch.from_numpy(y.astype(np.float64))


def gp32(gy, y):
    """fc_gp: gy * (y > 0 ? G : fl32(G * 0.2f)) on float64 tensors of fp32 values."""
    g = gy.numpy().astype(np.float32)
    s = y.numpy().astype(np.float32)
    out = g * np.where(s > 0, G32, GS32).astype(np.float32)
    assert out.dtype == np.float32
    return torch.from_numpy(out.astype(np.float64))


# ---- failure messages -------------------------------------------------------------------------------------------------------------------
def lane_class(i):
    """(i % 16, i // 16 % 4): the lane's row or column of a 16 x 16 tile (lane & 15) and the tile's place among four -- the wave, the k
    slot or the lane group (lane >> 4) the index went through."""
    return (int(i) % 16, int(i) // 16 % 4)


def mismatch(got, ref, what=''):
    """None when ``got`` equals the float64 ``ref`` cast to fp32 bit for bit (-0 == +0), else the count, the first differing index, both
    values and the lane class of each coordinate of that index."""
    want = ref.to(F32)
    got = got.detach().cpu()
    if got.shape != want.shape or got.dtype != F32:
        return f'{what}: {got.dtype} {tuple(got.shape)} instead of float32 {tuple(want.shape)}'
    if torch.equal(got, want):
        return None
    bad = (got != want) | torch.isnan(got)
    idx = tuple(bad.nonzero()[0].tolist())
    return (f'{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at {idx}: {got[idx].item()!r} != {want[idx].item()!r}, '
            f'lane class (index % 16, index // 16 % 4) per coordinate {[lane_class(i) for i in idx]}')


def assert_exact(got, ref, what=''):
    msg = mismatch(got, ref, what)
    assert msg is None, msg


def _conditions(stored, sums):
    bad = [f'{k} is not representable in float32' for k, v in stored.items() if v is not None and not representable(v, F32)]
    bad += [f'the fp32 sums of {k} reach {u:.3g} quanta (limit 2^24)' for k, u in sums.items() if not u < LIMIT]
    return bad


def _draw(make, key, cache):
    """The first of SEEDS draws of a case whose ``failures()`` is empty (one reference per case, shared and left unchanged)."""
    if key not in cache:
        why = None
        for k in range(SEEDS):
            case = make(1000 * k)
            why = case.failures()
            if not why:
                case.seed = 1000 * k
                cache[key] = case
                break
        else:
            raise AssertionError(f'no exact draw for {key}: {why}')
    return cache[key]


def _set_dot(a, b, target):
    """Flip signs of the +-1 vector ``a`` in place until <a, b> == target (b +-1, target of the parity of len(a))."""
    s = int((a * b).sum())
    assert (s - target) % 2 == 0 and abs(target) <= a.numel()
    want = 1.0 if s > target else -1.0
    idx = ((a * b) == want).nonzero().flatten()[:abs(s - target) // 2]
    a[idx] = -a[idx]
    assert int((a * b).sum()) == target


# ---- fc_act forward -----------------------------------------------------------------------------------------------------------------------
NS = (1, 16, 17, 32, 33, 64)                          # NT = 1 / 2 / 4, a dead-row tail in each
FWD_CIN = (16, 48, 144, 2032, 2048, 2064, 4608)
FWD_COUT_OP = (16, 48)                                # through fc_bank.fc_act
FWD_COUT_ABI = (1, 5, 18, 20, 33)                     # through afcm_fc_act_fwd: cout % 16 != 0
FWD_CIN_ABI = (48, 2064)                              # the 4-wave and (n <= 32) the 16-wave form
ACTS = ('linear', 'lrelu')
PLANTED = ((0, 0.0), (-4, -1.0), (4, 1.0))            # (dot of the +-1 rows, bias): u exactly 0, exactly negative, positive


def nt_class(n):
    return 1 if n <= 16 else 2 if n <= 32 else 4


class FcFwd:
    """y = act(alpha * x @ w.T + beta * b).  w is dense +-1; x holds {+-1, +-2, +-3} except its first three rows, which are +-1 so that
    three elements of u can be planted: exactly 0, exactly negative and positive (row 0, columns 0..2; where the layer has fewer than
    three columns, rows 0..2 of column 0; the single element of n = cout = 1 is the zero)."""

    def __init__(self, n, cin, cout, act, bias, seed=0):
        self.n, self.cin, self.cout, self.act = n, cin, cout, act
        g = gen(seed + 7 * n + cin + 131 * cout)
        self.alpha = 2.0 ** -(2 + (n + cin // 16) % 3)
        self.beta = 2.0 ** (cout % 3 - 1)
        x = pick([n, cin], (-3, -2, -1, 1, 2, 3), g)
        x[:3] = pm1([min(n, 3), cin], g)
        w = pm1([cout, cin], g)
        b = pick([cout], (-3, -2, -1, 1, 2, 3), g)
        self.planted = []
        for p, (dot, bp) in enumerate(PLANTED):
            r, c = (0, p) if cout >= 3 else (p, 0)
            if r >= n or c >= cout:
                continue
            if cout >= 3:
                _set_dot(w[c], x[0], dot)
                b[c] = bp
            else:
                _set_dot(x[r], w[0], dot)
                b[0] = 0.0
            self.planted.append((r, c))
        self.x, self.w, self.b = x, w, (b if bias else None)
        self.u = self.alpha * (x @ w.t()) + (self.beta * b if bias else 0.0)
        self.y = lrelu32(self.u) if (act == 'lrelu' and representable(self.u, F32)) else self.u

    def failures(self):
        q = self.alpha * quantum(self.x) * quantum(self.w)
        units = self.alpha * float((self.x.abs() @ self.w.abs().t()).max())
        if self.b is not None:
            q = min(q, self.beta * quantum(self.b))
            units += self.beta * float(self.b.abs().max())
        bad = _conditions(dict(x=self.x, w=self.w, b=self.b, u=self.u, y=self.y),
                          dict(dot=dot_units(self.x, self.w, self.cin), u=units / q))
        signs = [float(self.u[r, c]) for r, c in self.planted]
        want = [0.0, -1.0, 1.0][:len(signs)]
        if [math.copysign(1.0, s) if s else 0.0 for s in signs] != want:
            bad.append(f'planted elements of u are {signs}')
        return bad


_FWD = {}


def fc_fwd(n, cin, cout, act, bias):
    return _draw(lambda s: FcFwd(n, cin, cout, act, bias, s), ('fwd', n, cin, cout, act, bias), _FWD)


def fwd_op_cases(n, cin):
    """Every (cout, act, bias) of one (n, cin) through the op: the full cross product."""
    return [(cout, act, bias) for cout in FWD_COUT_OP for act in ACTS for bias in (True, False)]


def fwd_abi_cases(n):
    return [(cin, cout, act, bias) for cin in FWD_CIN_ABI for cout in FWD_COUT_ABI for act in ACTS for bias in (True, False)]


# ---- fc_act backward, linear ------------------------------------------------------------------------------------------------------------
BWD_CIN = (16, 48)
BWD_COUT = (16, 64, 80, 144)                          # 1, 4, 5, 9 row tiles of 16 over 4 waves, two tiles per trip, trips of 8
SUBSETS = (('dx', 'dw', 'db'), ('dx',), ('dw',), ('db',), ('dw', 'db'))


class FcLinearBwd:
    """dx = alpha gy @ w, dw = alpha gy.T @ x, db = beta sum_n gy of the linear layer; gy is dense +-1, the operand of all three sums."""

    def __init__(self, n, cin, cout, seed=0):
        self.n, self.cin, self.cout = n, cin, cout
        g = gen(seed + 11 * n + cin + 17 * cout)
        self.alpha = 2.0 ** -(1 + (n + cout // 16) % 3)
        self.beta = 2.0 ** (cin // 16 % 2 + 1)
        self.x = pick([n, cin], (-3, -2, -1, 1, 2, 3), g)
        self.w = pick([cout, cin], (-2, -1, 1, 2), g)
        self.b = pick([cout], (-3, -2, -1, 1, 2, 3), g)
        self.gy = pm1([n, cout], g)
        self.y = self.alpha * (self.x @ self.w.t()) + self.beta * self.b
        self.dx = self.alpha * (self.gy @ self.w)
        self.dw = self.alpha * (self.gy.t() @ self.x)
        self.db = self.beta * self.gy.sum(0)

    def failures(self):
        qy = min(self.alpha, self.beta)
        return _conditions(dict(x=self.x, w=self.w, b=self.b, gy=self.gy, y=self.y, dx=self.dx, dw=self.dw, db=self.db),
                           dict(y=(self.alpha * dot_units(self.x, self.w, self.cin) + self.beta * 3) / qy,
                                dx=dot_units(self.gy, self.w, self.cout), dw=dot_units(self.gy, self.x, self.n), db=float(self.n)))


_BWD = {}


def fc_linear_bwd(n, cin, cout):
    return _draw(lambda s: FcLinearBwd(n, cin, cout, s), ('lin', n, cin, cout), _BWD)


# ---- fc_act backward, lrelu, single-term cotangents ---------------------------------------------------------------------------------------
Y_CLASSES = (1.0, -1.0, 0.0, -0.0, 2.0 ** -100, -2.0 ** -100)             # no subnormals: their comparison hangs on the denormal mode
PI_STEP = 7                                                                # coprime to every cout of BWD_COUT


def pi(n, t, cout):
    return (PI_STEP * n + t) % cout


class FcLreluBwd:
    """The saved output ``y`` is CHOSEN (C ABI): class (t + n) % 6 of Y_CLASSES at the element (n, pi(n, t)), so every launch of a case
    with six or more rows, and the sweep of every case, brings each class together with a non-zero cotangent.  x, w and gy are +-2^e."""

    def __init__(self, n, cout, seed=0):
        self.n, self.cin, self.cout = n, 16, cout
        g = gen(seed + 13 * n + 19 * cout)
        self.alpha = 2.0 ** -(1 + n % 2)
        self.beta = 2.0 ** (cout // 16 % 2)
        vals = [s * 2.0 ** e for s in (-1, 1) for e in (-1, 0, 1, 2)]
        self.x = pick([n, 16], vals, g)
        self.w = pick([cout, 16], vals, g)
        self.gvals = pick([n], [s * 2.0 ** e for s in (-1, 1) for e in (-1, 0, 1)], g)
        rows, cols = torch.arange(n)[:, None], torch.arange(cout)[None, :]
        cls = ((cols - PI_STEP * rows) % cout + rows) % 6                  # (t + n) % 6 at column pi(n, t)
        self.y = torch.tensor(Y_CLASSES, dtype=F64)[cls]
        self.cls = cls
        # shifts: in order, every t that still hits a new column; windows: cout consecutive rows each
        live = min(n, cout)
        self.launches, seen = [], set()
        for t in range(cout):
            hit = {pi(r, t, cout) for r in range(live)}
            if not hit <= seen:
                seen |= hit
                self.launches += [(t, v) for v in range(0, n, cout)]

    def gy(self, t, v):
        """The cotangent of launch (t, v): row r of [v, v + cout) holds gvals[r] at column pi(r, t), everything else is zero."""
        gy = torch.zeros([self.n, self.cout], dtype=F64)
        r = torch.arange(v, min(v + self.cout, self.n))
        gy[r, (PI_STEP * r + t) % self.cout] = self.gvals[r]
        return gy

    def ref(self, t, v):
        gp = gp32(self.gy(t, v), self.y)
        return dict(dx=self.alpha * (gp @ self.w), dw=self.alpha * (gp.t() @ self.x), db=self.beta * gp.sum(0))

    def failures(self):
        bad = _conditions(dict(x=self.x, w=self.w, y=self.y), {})
        for t, v in self.launches:
            gy = self.gy(t, v)
            nz = gy != 0
            if int(nz.sum(1).max()) > 1 or int(nz.sum(0).max()) > 1:
                bad.append(f'launch {(t, v)}: more than one term in a sum')
            bad += [f'launch {(t, v)}: {m}' for m in _conditions(dict(gy=gy, **self.ref(t, v)), {})]
        return bad


_LRELU = {}


def fc_lrelu_bwd(n, cout):
    return _draw(lambda s: FcLreluBwd(n, cout, s), ('lrelu', n, cout), _LRELU)


# ---- affine bank ------------------------------------------------------------------------------------------------------------------------
BANK_NS = (1, 16, 17, 33)                             # one 16-row pass, exactly one, two and three (dW / db accumulate)
BANK_K = ((16, 0), (48, 0), (32, 1024), (512, 1024))  # (kw, kg); (32, 1024): 66 chunks, 17 per wave: the 8-deep loop and the tail
BANK_COUTS = ((8, 24, 7), (65, 130, 16))              # a partial 16-row block; 2 and 3 row blocks of 64 with a 1-row and a 2-row last one
Bank = collections.namedtuple('Bank', 'n kw kg couts idx drop')
BANK_CASES = ([Bank(n, kw, kg, couts, None, ()) for n in BANK_NS for kw, kg in BANK_K for couts in BANK_COUTS]
              + [Bank(19, 32, 1024, (8, 8, 16, 4), (3, 0, 3, 1), (1,))])   # shared, non-consecutive latents; layer 1 has no cotangent


class AffineBank:
    """styles_l = scale_l (gain_l x_l @ W_l.T + bgain_l b_l), x_l = [ws[:, idx_l] | g], and every gradient.  W and the cotangents are
    dense +-1, ws and g hold {+-1, +-2, +-3}; the gains are powers of two, the last layer's scale is 0.125 (ToRGB)."""

    def __init__(self, case, seed=0):
        self.case = case
        n, kw, kg, couts, idx, drop = case
        g = gen(seed + 23 * n + kw + kg + sum(couts))
        nl = len(couts)
        self.idx = list(range(1, 1 + nl)) if idx is None else list(idx)
        self.scale = [1.0] * (nl - 1) + [0.125]
        self.wgain = [2.0 ** -(2 + l % 3) for l in range(nl)]
        self.bgain = [2.0 ** (l % 2) for l in range(nl)]
        self.ws = pick([n, max(self.idx) + 2, kw], (-3, -2, -1, 1, 2, 3), g)
        self.g = pick([n, kg], (-3, -2, -1, 1, 2, 3), g) if kg else None
        self.W = [pm1([c, kw + kg], g) for c in couts]
        self.b = [pick([c], (-3, -2, -1, 1, 2, 3), g) for c in couts]
        self.dy = [None if l in drop else pm1([n, c], g) for l, c in enumerate(couts)]
        self.alpha = [a * s for a, s in zip(self.wgain, self.scale)]
        self.beta = [a * s for a, s in zip(self.bgain, self.scale)]
        xs = [self.ws[:, i] if kg == 0 else torch.cat((self.ws[:, i], self.g), 1) for i in self.idx]
        self.y = [al * (x @ W.t()) + be * b for x, W, b, al, be in zip(xs, self.W, self.b, self.alpha, self.beta)]
        zero = [torch.zeros([n, c], dtype=F64) for c in couts]
        dys = [z if d is None else d for z, d in zip(zero, self.dy)]
        self.dW = [al * (d.t() @ x) for d, x, al in zip(dys, xs, self.alpha)]
        self.db = [be * d.sum(0) for d, be in zip(dys, self.beta)]
        dxs = [al * (d @ W) for d, W, al in zip(dys, self.W, self.alpha)]                  # [n, K] per layer
        self.dws = torch.zeros_like(self.ws)
        for i, dx in zip(self.idx, dxs):
            self.dws[:, i] += dx[:, :kw]
        self.dg = sum(dx[:, kw:] for dx in dxs) if kg else None
        self.xs, self.dys = xs, dys

    def failures(self):
        n, kw, kg, couts, _, _ = self.case
        stored = dict(ws=self.ws, g=self.g, dws=self.dws, dg=self.dg)
        sums = {}
        qa = min(self.alpha)
        for l, c in enumerate(couts):
            stored.update({f'W{l}': self.W[l], f'b{l}': self.b[l], f'y{l}': self.y[l], f'dW{l}': self.dW[l], f'db{l}': self.db[l]})
            sums[f'y{l}'] = (self.alpha[l] * dot_units(self.xs[l], self.W[l], kw + kg) + self.beta[l] * 3) / min(self.alpha[l], self.beta[l])
            sums[f'dW{l}'] = dot_units(self.dys[l], self.xs[l], n) if self.dy[l] is not None else 0.0
            sums[f'db{l}'] = float(n)
        # the input gradient: every layer's rows, each layer at its own alpha, in quanta of the smallest alpha
        sums['dx'] = sum(a * c for a, c in zip(self.alpha, couts)) / qa
        return _conditions(stored, sums)


_BANK = {}


def affine_bank_case(case):
    return _draw(lambda s: AffineBank(case, s), case, _BANK)


def bank_id(case):
    return f'n{case.n}-k{case.kw}+{case.kg}-' + 'x'.join(map(str, case.couts)) + ('-shared' if case.idx else '')
