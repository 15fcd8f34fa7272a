#!/usr/bin/env python3
"""Golden vectors for the intensity training augmentation (afcm_amd/augment_intensity.py, afcm_batch_assemble_noise), captured from the reference's
own classes.

data/augment/transforms.py cannot be imported where cv2 / skimage are absent (its top-level imports), so ``RandomContrast``,
``AdditiveGaussianNoise`` and ``AdditivePoissonNoise`` (transforms.py:115-133, 619-644) are compiled on their own from the reference's syntax tree at
generation time, given ``numpy`` as the module gives it, and driven by a scripted ``random_state``: ``uniform`` returns listed values (the decision
draw, then the parameter), ``normal(0, std, size)`` returns ``std * z`` for a recorded array ``z`` of standard normals and ``poisson(lam, size)`` a
recorded array of counts, so that every case's parameters and fields are known.  The three are composed in the order this project applies them
(contrast, Gaussian, Poisson) on float64 planes that hold float32 values, as ``Normalize`` hands them on before ``ToTensor`` casts; the outputs are
stored as float64, before that cast.  Only inputs, scripted draws and outputs are stored (tests/golden/A2_augment_intensity.npz).

    python tools/gen_golden_augment_intensity.py <reference checkout>
"""
import ast
import os
import sys

import numpy as np

PROB = 0.2                                                                   # configs/defaults.py:85, 88


def extract_classes(path, names):
    tree = ast.parse(open(path).read())
    nodes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in names]
    ns = {'np': np}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, 'exec'), ns)
    return [ns[n] for n in names]


class Scripted:
    """A ``random_state`` that returns the listed values in order and refuses a call past them."""

    def __init__(self, uniform=(), z=None, counts=None):
        self.u, self.z, self.counts = list(uniform), z, counts

    def uniform(self, *args):
        return self.u.pop(0)

    def normal(self, loc, scale, size):
        z, self.z = self.z, None
        assert loc == 0 and z.shape == tuple(size)
        return scale * z

    def poisson(self, lam, size):
        counts, self.counts = self.counts, None
        assert counts.shape == tuple(size)
        return counts


def plane(h, w, seed):
    """A normalised uint8 plane with NaN-free float32 values, held as float64 [1, h, w]."""
    raw = np.random.default_rng(seed).integers(0, 256, (1, h, w)).astype(np.float64)
    return np.clip(2.0 * (raw / 255.0) - 1.0, -1, 1).astype(np.float32).astype(np.float64)


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    contrast_cls, gauss_cls, poisson_cls = extract_classes(os.path.join(sys.argv[1], 'data/augment/transforms.py'),
                                                           ['RandomContrast', 'AdditiveGaussianNoise', 'AdditivePoissonNoise'])
    rng = np.random.default_rng(7)
    h, w = 12, 18
    x = np.stack([plane(h, w, seed=s)[0] for s in (1, 2)])                    # two planes; each case uses one of them
    below, above = 0.05, 0.75
    # decision draws (contrast, Gaussian, Poisson): every combination of executed / not, then a draw EQUAL to the probability (not executed: the
    # comparison is strict) and one just below it
    decisions = [tuple(below if (c >> j) & 1 else above for j in range(3)) for c in range(8)]
    decisions += [(PROB, PROB, PROB), (np.nextafter(PROB, 0), above, np.nextafter(PROB, 0))]
    cases, zs, counts, outs = [], [], [], []
    for n, draws in enumerate(decisions):
        alpha, mean = float(rng.uniform(0.5, 1.5)) if n != 1 else 1.4375, (0.0, 0.25)[n % 2]     # case 1, contrast alone: the clip acts
        std, lam = float(rng.uniform(0.0, 1.0)), float(rng.uniform(0.0, 1.0))
        z = rng.standard_normal((1, h, w))
        k = rng.poisson(lam, (1, h, w))
        m = x[n % 2][None]
        c = Scripted(uniform=[draws[0], alpha])
        g = Scripted(uniform=[draws[1], std], z=z)
        p = Scripted(uniform=[draws[2], lam], counts=k)
        m = contrast_cls(c, alpha=(0.5, 1.5), mean=mean, execution_probability=PROB)(m)
        m = gauss_cls(g, scale=(0.0, 1.0), execution_probability=PROB)(m)
        m = poisson_cls(p, lam=(0.0, 1.0), execution_probability=PROB)(m)
        executed = [d < PROB for d in draws]
        for scripted, ran in zip((c, g, p), executed):                       # a transform that ran took its parameter, one that did not took nothing
            assert len(scripted.u) == (0 if ran else 1)
        assert (g.z is None) == executed[1] and (p.counts is None) == executed[2] and m.shape == (1, h, w) and m.dtype == np.float64
        cases.append(list(draws) + [alpha, mean, std, lam, n % 2])
        zs.append(z[0]), counts.append(k[0]), outs.append(m[0])
    out = dict(x=x, prob=np.float64(PROB), cases=np.array(cases, dtype=np.float64), z=np.stack(zs), counts=np.stack(counts).astype(np.int64),
               out=np.stack(outs))
    dst = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'A2_augment_intensity.npz')
    np.savez_compressed(dst, **out)
    print('wrote', dst, {k: v.shape for k, v in out.items()}, os.path.getsize(dst), 'bytes')


if __name__ == '__main__':
    main()
