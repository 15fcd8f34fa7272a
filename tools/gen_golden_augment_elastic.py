#!/usr/bin/env python3
"""Golden vectors for the elastic training augmentation (afcm_amd/augment_elastic.py, afcm_batch_assemble_elastic), captured from the reference's
own class.

data/augment/transforms.py cannot be imported where cv2 / skimage are absent (its top-level imports), so ``ElasticDeformation``
(transforms.py:138-191) is compiled on its own from the reference's syntax tree at generation time, given ``numpy``, ``gaussian_filter`` and
``map_coordinates`` as the module gives them, and driven by a scripted ``random_state``: ``uniform()`` returns the listed decision draw and
``randn(*shape)`` returns recorded fields in the order the class asks for them (``dz`` first, with ``apply_3d`` only, then ``dy``, ``dx``), so that
every case's fields are known.  The planes are float64 [1, 24, 32] holding float32 values, as ``Normalize`` hands them on before ``ToTensor`` casts;
the outputs are stored as float64, before that cast.  Only inputs, scripted draws, fields and outputs are stored
(tests/golden/E1_augment_elastic.npz).

    python tools/gen_golden_augment_elastic.py <reference checkout>
"""
import ast
import os
import sys

import numpy as np
from scipy.ndimage import gaussian_filter, map_coordinates

PROB = 0.1                                                                   # configs/defaults.py:78


def extract_class(path, name):
    tree = ast.parse(open(path).read())
    nodes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == name]
    ns = {'np': np, 'gaussian_filter': gaussian_filter, 'map_coordinates': map_coordinates}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, 'exec'), ns)
    return ns[name]


class Scripted:
    """A ``random_state`` that returns the listed values in order and refuses a call past them."""

    def __init__(self, uniform, fields):
        self.u, self.fields = [uniform], list(fields)

    def uniform(self):
        return self.u.pop(0)

    def randn(self, *shape):
        field = self.fields.pop(0)
        assert field.shape == tuple(shape)
        return field


def plane(h, w, seed):
    """A normalised uint8 plane with float32 values, held as float64 [1, h, w]: smooth structure plus noise, so that interpolation matters."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    raw = np.clip(128 + 90 * np.sin(0.5 * y + 0.3 * x + seed) + rng.integers(-30, 31, (h, w)), 0, 255).astype(np.uint8).astype(np.float64)
    return np.clip(2.0 * (raw / 255.0) - 1.0, -1, 1).astype(np.float32).astype(np.float64)[None]


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    cls = extract_class(os.path.join(sys.argv[1], 'data/augment/transforms.py'), 'ElasticDeformation')
    rng = np.random.default_rng(11)
    h, w = 24, 32
    x = np.stack([plane(h, w, seed=s)[0] for s in (1, 2)])
    below = 0.03
    # (decision draw, order, apply_3d, sigma, alpha): every order with sigma 50 (401 taps folded over a 24-pixel line, displacements of several
    # periods) and with sigma 2 (a banded operator, displacements of a few pixels), apply_3d both ways, not executed, and a draw EQUAL to the
    # probability (not executed: the comparison is strict) beside one just below it
    specs = [(below, order, True, 50.0, 2000.0) for order in (0, 1, 3)] + [(below, order, False, 2.0, 30.0) for order in (0, 1, 3)]
    specs += [(below, 3, False, 50.0, 2000.0), (below, 3, True, 2.0, 30.0), (0.75, 3, True, 50.0, 2000.0), (PROB, 3, True, 50.0, 2000.0),
              (float(np.nextafter(PROB, 0)), 1, True, 2.0, 30.0)]
    cases, fields, outs = [], [], []
    for n, (draw, order, apply_3d, sigma, alpha) in enumerate(specs):
        f = rng.standard_normal((3, 1, h, w))                               # dz, dy, dx
        state = Scripted(draw, f if apply_3d else f[1:])
        m = cls(state, order, alpha=alpha, sigma=sigma, execution_probability=PROB, apply_3d=apply_3d)(x[n % 2][None])
        executed = draw < PROB
        assert not state.u and len(state.fields) == (0 if executed else (3 if apply_3d else 2))
        assert m.shape == (1, h, w) and m.dtype == np.float64 and (executed or m is not None and np.array_equal(m[0], x[n % 2]))
        cases.append([draw, order, float(apply_3d), sigma, alpha, n % 2])
        fields.append(f[:, 0]), outs.append(m[0])
    out = dict(x=x, prob=np.float64(PROB), cases=np.array(cases, dtype=np.float64), fields=np.stack(fields), out=np.stack(outs))
    dst = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'E1_augment_elastic.npz')
    np.savez_compressed(dst, **out)
    print('wrote', dst, {k: v.shape for k, v in out.items()}, os.path.getsize(dst), 'bytes')


if __name__ == '__main__':
    main()
