"""Shared by test_adam_ref_cpu.py and test_gpu_optim_edges.py: a plain restatement of the update rule that afcm_amd/optim.py documents
(gradient * grad_scale, then the NaN/Inf scrub, then torch.optim.Adam's arithmetic with ONE step count per parameter group), the
comparison rule, and the case tables (seeds, sizes, hyper-parameters), so that the CPU file and the GPU file look at the same tensors.

``adam_run(..., dtype=torch.float64)`` is the reference.  ``adam_run(..., dtype=torch.float32)`` is the same rule in the kernel's number
format, written in the operation order of torch's foreach Adam (lerp, mul + addcmul, sqrt / bc2_sqrt + eps, addcdiv); its distance E_t
from the float64 run is what fp32 rounding alone does, and every tolerance is computed from it (``bound``):

    E_k <= 2 * E_t + 2**-23 * max|x64|         per tensor, per step, for x in p, m, v

The factor 2 is the "last bit or two" that csrc/optim.hip claims over the eager sequence; the additive ulp covers a tensor where the
float32 run happens to be exact.  E_t never comes from the code under test.

``fault=`` restates the rule wrongly in one named way (FAULTS); test_adam_ref_cpu.py uses it to show that every case table below
would notice that mistake by at least 10x the bound.
"""
import collections
import math

import torch

BETAS = [(0.0, 0.99), (0.9, 0.999)]            # the reference model's setting (the kernel's shortcut that never reads m), and torch's default
LRS = [0.0025, 0.0002]                         # the reference model's, and a smaller one: the tightest for the count faults
LR_TIGHT = 0.0002
EPS = 1e-8
ULP32 = 2.0 ** -23
TEETH = 10.0
SENTINEL = 0x7FE5A5A5                          # a quiet NaN with a payload: read as a float it poisons the result, compared as int32

# the ways the rule could be restated wrongly.  'frozen' takes the count at which the step count stops advancing ('frozen:2')
FAULTS = ['count+1', 'frozen', 'no_bc2', 'scrub_first', 'inf_swapped']

Step = collections.namedtuple('Step', 'p m v count')


# ---------------------------------------------------------------------------------------------------------------- the rule
def scrubbed_grad(g, grad_scale=1.0, scrub=True, posinf=1e5, neginf=-1e5, dtype=torch.float64, fault=None):
    """The gradient the update consumes: ``g * grad_scale`` first, then nan -> 0, +inf -> posinf, -inf -> neginf."""
    g = g.detach().to(dtype)
    if fault == 'inf_swapped':
        posinf, neginf = neginf, posinf
    if fault == 'scrub_first':
        if scrub:
            g = torch.nan_to_num(g, nan=0.0, posinf=posinf, neginf=neginf)
        return g * grad_scale
    g = g * grad_scale
    if scrub:
        g = torch.nan_to_num(g, nan=0.0, posinf=posinf, neginf=neginf)
    return g


def adam_run(p0s, grad_schedule, lr, betas, eps=EPS, scrub=True, posinf=1e5, neginf=-1e5, grad_scale=1.0, dtype=torch.float64, fault=None):
    """``grad_schedule[k][i]`` is parameter i's gradient in step k, or None.  Returns one Step(p, m, v, count) per step: lists over the
    parameters, cloned.  One step count per group: the largest count in the group + 1, given to every parameter that has a gradient;
    a parameter without one keeps p, m, v and its count.  Bias corrections are Python doubles."""
    beta1, beta2 = betas
    ps = [p.detach().to(dtype).clone() for p in p0s]
    ms = [torch.zeros_like(p) for p in ps]
    vs = [torch.zeros_like(p) for p in ps]
    counts = [0] * len(ps)
    out = []
    for grads in grad_schedule:
        live = [i for i, g in enumerate(grads) if g is not None]
        if live:
            t = max(counts) + 1
            for i in live:
                counts[i] = t
            if fault == 'count+1':
                t = t + 1
            elif fault is not None and fault.startswith('frozen:'):
                t = min(t, int(fault.split(':')[1]))
            bc1 = 1.0 - beta1 ** t
            bc2 = 1.0 if fault == 'no_bc2' else 1.0 - beta2 ** t
            step_size = lr / bc1
            bc2_sqrt = math.sqrt(bc2)
            for i in live:
                g = scrubbed_grad(grads[i], grad_scale, scrub, posinf, neginf, dtype, fault)
                ms[i].lerp_(g, 1.0 - beta1)
                vs[i].mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
                denom = (vs[i].sqrt() / bc2_sqrt).add_(eps)
                ps[i].addcdiv_(ms[i], denom, value=-step_size)
        out.append(Step([p.clone() for p in ps], [m.clone() for m in ms], [v.clone() for v in vs], list(counts)))
    return out


# ---------------------------------------------------------------------------------------------------------------- the comparison
def float32_error(x32, x64):
    """E_t: the error of the float32 run, over the elements where the float64 run is finite."""
    fin = torch.isfinite(x64)
    return (x32.to(torch.float64)[fin] - x64[fin]).abs().max().item() if bool(fin.any()) else 0.0


def bound(x32, x64):
    """2 * E_t + one fp32 ulp of the largest magnitude, over the elements where the float64 run is finite."""
    fin = torch.isfinite(x64)
    return 2.0 * float32_error(x32, x64) + ULP32 * x64[fin].abs().max().item() if bool(fin.any()) else 0.0


def judge(got, x32, x64):
    """(E_k, bound, problem): the error of ``got`` against the float64 run over its finite elements, the bound, and a message if the
    non-finite elements differ in kind -- got must be NaN / +inf / -inf exactly where the float64 run is."""
    got = got.detach().to('cpu', torch.float64).reshape(x64.shape)
    fin = torch.isfinite(x64)
    problem = None
    if not torch.equal(torch.isnan(got), torch.isnan(x64)):
        problem = 'NaN at %d elements, float64 run at %d' % (int(torch.isnan(got).sum()), int(torch.isnan(x64).sum()))
    elif not torch.equal(torch.isinf(got), torch.isinf(x64)) or not torch.equal(got[torch.isinf(x64)], x64[torch.isinf(x64)]):
        problem = 'infinities differ from the float64 run'
    e_k = (got[fin] - x64[fin]).abs().max().item() if bool(fin.any()) else 0.0
    return e_k, bound(x32, x64), problem


class Comparison:
    """Collects, over the steps of one test, the error of every tensor against the float64 run; ``finish`` prints the figures and asserts
    the bound for all of them at once, so that one run shows every miss."""

    def __init__(self, name):
        self.name, self.ratios, self.shares, self.misses = name, [], [], []

    def add(self, got, step32, step64, where):
        """``got``: {'p' | 'm' | 'v': list of tensors in the order of the case}."""
        for key in ('p', 'm', 'v'):
            for i, x in enumerate(got.get(key, [])):
                x32, x64 = getattr(step32, key)[i], getattr(step64, key)[i]
                e_k, b, problem = judge(x, x32, x64)
                e_t = float32_error(x32, x64)
                if e_t > 0:
                    self.ratios.append(e_k / e_t)
                if b > 0:
                    self.shares.append(e_k / b)
                if problem is not None:
                    self.misses.append('%s: %s[%d]: %s' % (where, key, i, problem))
                elif e_k > b:
                    self.misses.append('%s: %s[%d] (%d elements): E_k %.3e > bound %.3e = 2 * E_t %.3e + ulp * max|x|' % (where, key, i, x64.numel(), e_k, b, e_t))

    def summary(self):
        return '%s: E_k / E_t max %.2f, median %.2f; E_k / bound max %.3f over %d tensors' % (
            self.name, max(self.ratios, default=0.0), sorted(self.ratios)[len(self.ratios) // 2] if self.ratios else 0.0,
            max(self.shares, default=0.0), len(self.shares))

    def finish(self):
        print(self.summary())
        assert not self.misses, '%s\n%d misses, the first:\n%s' % (self.summary(), len(self.misses), '\n'.join(self.misses[:6]))


def bits(x):
    """The float32 bit patterns, as int32 on the CPU (NaN payloads and the sign of zero count)."""
    return x.detach().contiguous().view(torch.int32).cpu()


# ---------------------------------------------------------------------------------------------------------------- the case tables
def _randn(gen, n, scale=1.0):
    return torch.randn(n, generator=gen, dtype=torch.float32) * scale


def _magnitude(k):
    return 10.0 ** (k % 4 - 2)


def _case(sizes, steps, seed, lr, betas, present=None, stagger=True, **hyper):
    """p0 ~ N(0, 1); gradient of tensor i in step k ~ N(0, 1) * 10**((k + i) mod 4 - 2), or 10**(k mod 4 - 2) for every tensor without
    ``stagger``; ``present(k, i)`` False: no gradient."""
    gen = torch.Generator().manual_seed(seed)
    p0s = [_randn(gen, n) for n in sizes]
    sched = [[_randn(gen, n, _magnitude(k + i if stagger else k)) if (present is None or present(k, i)) else None for i, n in enumerate(sizes)] for k in range(steps)]
    return dict(p0s=p0s, sched=sched, kw=dict(lr=lr, betas=betas, eps=EPS, **hyper))


def run_both(case, steps=None, fault=None):
    """(float32 run, float64 run) of a case, or of its first ``steps`` steps."""
    sched = case['sched'] if steps is None else case['sched'][:steps]
    return (adam_run(case['p0s'], sched, dtype=torch.float32, fault=fault, **case['kw']),
            adam_run(case['p0s'], sched, dtype=torch.float64, fault=fault, **case['kw']))


# (a) capturable, eager: 6 steps, a fresh gradient at every step
A_SIZES = [7, 64, 4100, 16384, 16385, 40000]
A_STEPS = 6
A_CASES = [(betas, lr) for betas in BETAS for lr in LRS]


def case_a(betas, lr):
    return _case(A_SIZES, A_STEPS, 11, lr, betas)


# (b) capturable, the optimizer step in a graph: 2 eager steps + 4 replays, and a 7th step for the checkpoint's readers
B_EAGER, B_REPLAYS = 2, 4
B_CASES = [(betas, LR_TIGHT) for betas in BETAS]


def case_b(betas, lr):
    return _case(A_SIZES, B_EAGER + B_REPLAYS + 1, 12, lr, betas)


# (c) load_state_dict into a capturable optimizer that has already stepped: the donor's 2 steps + 1 are the reference, the receiver's
# 5 steps run on gradients of their own (case_c_receiver) and must leave no trace
C_SIZES = [7, 4100, 16385]
C_DONOR, C_RECEIVER = 2, 5
C_CASES = [(betas, LR_TIGHT) for betas in BETAS]


def case_c(betas, lr):
    return _case(C_SIZES, C_DONOR + 1, 13, lr, betas)


def case_c_receiver(betas, lr):
    return _case(C_SIZES, C_RECEIVER, 14, lr, betas)


# (d) alignment and tails: slices of two flat buffers at the given element offsets modulo 4, gaps of >= 8 sentinel elements
D_OFFSETS = [(0, 0), (0, 1), (3, 0), (2, 2), (1, 3)]
D_SIZES = [1, 3, 4, 5, 255, 1024, 1027, 16383, 16384, 16385, 32769]
D_STEPS = 2
D_GAP = 8
D_CASES = [(off, betas, wg) for off in D_OFFSETS for betas in BETAS for wg in (False, True)]


def d_layout(offset):
    """(start of every slice, length of the flat buffer): every start is ``offset`` modulo 4, at least D_GAP elements lie between two
    slices and at both ends."""
    starts, pos = [], 0
    for n in D_SIZES:
        pos += D_GAP
        pos += (offset - pos) % 4
        starts.append(pos)
        pos += n
    return starts, pos + D_GAP + 4


def case_d(betas):
    # (no stagger: with two steps only, a tensor whose second gradient is 1000 times smaller than its first hardly moves in step 2, and
    # a wrong count in that step would go unnoticed)
    return _case(D_SIZES, D_STEPS, 15, LR_TIGHT, betas, stagger=False)


# (e) table search and groups: 130 tensors in two groups, and one 1-element tensor on its own
E_CYCLE = [1, 7, 64, 4100, 16384, 16385, 40000]
E_SIZES = {'130': [E_CYCLE[i % len(E_CYCLE)] for i in range(130)], '1': [1]}
E_GROUPS = [dict(lr=0.0025, betas=(0.0, 0.99)), dict(lr=0.0002, betas=(0.9, 0.999))]
E_STEPS = 3


def e_split(which):
    """Indices of the tensors of the two groups (the single tensor has one group, the second hyper-parameter set)."""
    n = len(E_SIZES[which])
    return [list(range(0, n // 2)), list(range(n // 2, n))] if n > 1 else [[], [0]]


def case_e(which, group):
    """The case of ONE group (the groups are independent runs of the rule); tensors in the order of e_split(which)[group]."""
    sizes = [E_SIZES[which][i] for i in e_split(which)[group]]
    return _case(sizes, E_STEPS, 16 + group, **E_GROUPS[group]) if sizes else None


# (f) changing gradient sets: five parameters, 5 steps; tensor 1 has a gradient at steps 2 and 4 only (counted from 1), tensor 3 never
F_SIZES = [7, 4100, 16385, 64, 40000]
F_STEPS = 5
F_SOMETIMES, F_NEVER = 1, 3
F_CASES = [(betas, LR_TIGHT) for betas in BETAS]


def f_present(k, i):
    return (k + 1) in (2, 4) if i == F_SOMETIMES else i != F_NEVER


def case_f(betas, lr):
    return _case(F_SIZES, F_STEPS, 18, lr, betas, present=f_present)


# (g) scrub matrix: the special values at the head, in the middle and in the last three elements; three such steps, the values rotated by
# three places from one step to the next, so that every one of them has stood in the last three elements (and in the one-element tail
# chunk of the 16385-element tensor) once; then one step of ordinary gradients, in which p shows what the scrub left in m and v (1e15 in
# the same tensor makes the bound on m and v themselves wide)
G_SPECIALS = [float('nan'), float('inf'), float('-inf'), -0.0, 1e-30, 1e5, 1e15]
G_SIZES = [16385, 7]
G_SPECIAL_STEPS = 3
G_STEPS = G_SPECIAL_STEPS + 1
G_SCRUBS = {'default': dict(scrub=True), 'custom': dict(scrub=True, posinf=7.0, neginf=-3.0), 'off': dict(scrub=False)}
G_SCALES = [1.0, 0.125]
G_CASES = [(s, scale, betas) for s in G_SCRUBS for scale in G_SCALES for betas in BETAS]


def case_g(scrub, scale, betas):
    case = _case(G_SIZES, G_STEPS, 19, LR_TIGHT, betas, stagger=False, grad_scale=scale, **G_SCRUBS[scrub])     # (the last step: N(0, 1) * 10)
    for k, grads in enumerate(case['sched'][:G_SPECIAL_STEPS]):
        sp = torch.tensor(G_SPECIALS[3 * k % 7:] + G_SPECIALS[:3 * k % 7], dtype=torch.float32)
        for g in grads:
            n = g.numel()
            g[:7] = sp
            if n > 7:
                g[n // 2:n // 2 + 7] = sp
                g[n - 3:] = sp[:3]
    return case


def teeth_cases():
    """(id, case, frozen count, the faults that change this case's inputs).  The count faults and the missing bias correction apply to
    every case.  The scrub faults need something to scrub: 'inf_swapped' an infinite gradient with the scrub on, 'scrub_first' also a
    grad_scale other than 1 -- elsewhere they restate the same rule."""
    count = ['count+1', 'frozen', 'no_bc2']
    out = []
    for betas, lr in A_CASES:
        out.append(('a-%s-%g' % (betas[0], lr), case_a(betas, lr), 1, count))
    for betas, lr in B_CASES:
        out.append(('b-%s' % betas[0], case_b(betas, lr), B_EAGER, count))
    for betas, lr in C_CASES:
        out.append(('c-%s' % betas[0], case_c(betas, lr), 1, count))
    for betas in BETAS:
        out.append(('d-%s' % betas[0], case_d(betas), 1, count))
    for which in E_SIZES:
        for group in (0, 1):
            if case_e(which, group) is not None:
                out.append(('e-%s-g%d' % (which, group), case_e(which, group), 1, count))
    for betas, lr in F_CASES:
        out.append(('f-%s' % betas[0], case_f(betas, lr), 1, count))
    for scrub, scale, betas in G_CASES:
        faults = count + ([] if scrub == 'off' else ['inf_swapped'] + (['scrub_first'] if scale != 1.0 else []))
        out.append(('g-%s-%g-%s' % (scrub, scale, betas[0]), case_g(scrub, scale, betas), 1, faults))
    return out
