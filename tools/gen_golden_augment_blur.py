#!/usr/bin/env python3
"""Golden vectors for the Gaussian blur training augmentation (afcm_amd/augment_blur.py, afcm_batch_assemble_blur), captured from the reference's
own class.

data/augment/transforms.py cannot be imported where cv2 / skimage are absent (its top-level imports), so ``GaussianBlur3D``
(transforms.py:716-726) is compiled on its own from the reference's syntax tree at generation time.  The class reads two module globals and is
given both: ``random``, a seeded ``random.Random`` (the class draws from Python's global generator; an instance has the same methods and the same
stream for a seed), wrapped so that every draw it consumes is recorded; and ``gaussian``, which stands in for ``skimage.filters.gaussian``:

    gaussian = lambda x, sigma: scipy.ndimage.gaussian_filter(x, sigma, mode='nearest', truncate=4.0)

skimage is absent where this was generated; that its function makes this scipy call on a float array is its documented behaviour, not something
measured here.  The planes are float64 [1, 24, 32] holding float32 values, as ``Normalize`` hands them on before ``ToTensor`` casts, one of them
all zeros (a thick-slice plane outside the volume: it costs its draws too); the outputs are stored as float64, before that cast.  Only inputs, the
seed, the consumed draws and outputs are stored (tests/golden/A3_augment_blur.npz).

    python tools/gen_golden_augment_blur.py <reference checkout>
"""
import ast
import os
import random
import sys

import numpy as np
from scipy.ndimage import gaussian_filter

SEED = 716
SIGMA = (0.1, 2.0)                                                           # configs/defaults.py:80-82
PROB = 0.5
CASES = 12


class Recorded:
    """The two methods the class calls, passed through to a ``random.Random`` with every value noted."""

    def __init__(self, seed):
        self.rng, self.log = random.Random(seed), []

    def random(self):
        self.log.append(self.rng.random())
        return self.log[-1]

    def uniform(self, lo, hi):
        self.log.append(self.rng.uniform(lo, hi))
        return self.log[-1]


def extract_class(path, name, rng):
    tree = ast.parse(open(path).read())
    nodes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == name]
    ns = {'random': rng, 'gaussian': lambda x, sigma: gaussian_filter(x, sigma, mode='nearest', truncate=4.0)}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, 'exec'), ns)
    return ns[name]


def plane(h, w, seed):
    """A normalised uint8 plane with float32 values, held as float64 [1, h, w]: smooth structure plus noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    raw = np.clip(128 + 90 * np.sin(0.5 * y + 0.3 * x + seed) + rng.integers(-30, 31, (h, w)), 0, 255).astype(np.uint8).astype(np.float64)
    return np.clip(2.0 * (raw / 255.0) - 1.0, -1, 1).astype(np.float32).astype(np.float64)[None]


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    rng = Recorded(SEED)
    cls = extract_class(os.path.join(sys.argv[1], 'data/augment/transforms.py'), 'GaussianBlur3D', rng)
    transform = cls(sigma=list(SIGMA), execution_probability=PROB)
    h, w = 24, 32
    x = np.stack([plane(h, w, seed=1), plane(h, w, seed=2), np.zeros((1, h, w))])
    which, draws, outs = [], [], []
    for n in range(CASES):
        before = len(rng.log)
        m = transform(x[n % 3])
        used = rng.log[before:]
        assert m.shape == (1, h, w) and m.dtype == np.float64 and len(used) in (1, 2) and (len(used) == 2) == (used[0] < PROB)
        assert len(used) == 2 or np.array_equal(m, x[n % 3])
        which.append(n % 3), draws.append(used + [np.nan] * (2 - len(used))), outs.append(m)
    draws = np.array(draws, dtype=np.float64)
    executed = ~np.isnan(draws[:, 1])
    assert 3 <= executed.sum() <= CASES - 3 and executed[np.array(which) == 2].any()       # both outcomes, and a blurred plane of zeros
    out = dict(x=x, seed=np.int64(SEED), sigma=np.array(SIGMA), prob=np.float64(PROB), which=np.array(which, dtype=np.int64), draws=draws,
               out=np.stack(outs))
    dst = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'A3_augment_blur.npz')
    np.savez_compressed(dst, **out)
    print('wrote', dst, {k: v.shape for k, v in out.items()}, os.path.getsize(dst), 'bytes', 'executed', int(executed.sum()))


if __name__ == '__main__':
    main()
