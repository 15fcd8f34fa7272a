#!/usr/bin/env python3
"""Golden vectors for the geometric training augmentation (afcm_amd/augment.py, afcm_batch_assemble_aug), captured from the reference's own classes.

data/augment/transforms.py cannot be imported where cv2 / skimage are absent (its top-level imports), so ``RandomFlip``, ``RandomRotate90`` and
``RandomRotate`` (transforms.py:25-112) are compiled on their own from the reference's syntax tree at generation time, given ``numpy`` and
``scipy.ndimage.rotate`` as the module gives them, and driven by a scripted ``random_state`` whose ``uniform`` / ``randint`` return listed values,
so that every case's parameters are known.  The three are composed in configuration order (configs/defaults.py:62-76) with the configuration's
arguments -- flip axes [1, 2], rotation axes [[2, 1]], angle_spectrum 45, mode 'reflect' -- on normalised [1, H, W] planes.  Only inputs,
parameters and outputs are stored (tests/golden/A1_augment.npz).

    python tools/gen_golden_augment.py <reference checkout>
"""
import ast
import os
import sys

import numpy as np
from scipy.ndimage import rotate


def extract_classes(path, names):
    tree = ast.parse(open(path).read())
    nodes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in names]
    ns = {'np': np, 'rotate': rotate}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, 'exec'), ns)
    return [ns[n] for n in names]


class Scripted:
    """A ``random_state`` that returns the listed values in order and refuses a call past them."""

    def __init__(self, uniform=(), randint=()):
        self.u, self.r = list(uniform), list(randint)

    def uniform(self, *args):
        return self.u.pop(0)

    def randint(self, *args):
        return self.r.pop(0)


def plane(h, w, seed):
    """A normalised uint8 plane: data.normalize's values, float32 [1, h, w]."""
    raw = np.random.default_rng(seed).integers(0, 256, (1, h, w)).astype(np.float64)
    return np.clip(2.0 * (raw / 255.0) - 1.0, -1, 1).astype(np.float32)


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    flip_cls, rot90_cls, rotate_cls = extract_classes(os.path.join(sys.argv[1], 'data/augment/transforms.py'),
                                                      ['RandomFlip', 'RandomRotate90', 'RandomRotate'])
    out = {}
    rng = np.random.default_rng(3)
    for name, (h, w), ks in (('sq', (16, 16), (0, 1, 2, 3)), ('ob', (12, 20), (0, 2))):
        x = plane(h, w, seed=h * w)
        # every flip x k combination at one oblique angle, then random parameters over the whole spectrum, the ends and 0 included
        cases = [(fh, fw, k, 37) for fh in (0, 1) for fw in (0, 1) for k in ks]
        cases += [(0, 0, 0, a) for a in (-45, -1, 0, 1, 44)]
        cases += [(int(rng.integers(0, 2)), int(rng.integers(0, 2)), int(rng.choice(ks)), int(rng.integers(-45, 45))) for _ in range(12)]
        got = []
        for fh, fw, k, angle in cases:
            flips = Scripted(uniform=[0.75 if fh else 0.25, 0.75 if fw else 0.25])           # an axis is flipped when uniform() > axis_prob
            turns = Scripted(randint=[k])
            spin = Scripted(randint=[0, angle])                                              # the axes pair's index, then the angle
            m = flip_cls(flips, axes=[1, 2])(x)
            m = rot90_cls(turns)(m)
            m = rotate_cls(spin, angle_spectrum=45, axes=[[2, 1]], mode='reflect')(m)
            assert not (flips.u or turns.r or spin.r) and m.shape == x.shape and m.dtype == np.float32
            got.append(np.ascontiguousarray(m))
        out[f'{name}_x'] = x
        out[f'{name}_params'] = np.array(cases, dtype=np.int64)
        out[f'{name}_out'] = np.stack(got)
    dst = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'A1_augment.npz')
    np.savez_compressed(dst, **out)
    print('wrote', dst, {k: v.shape for k, v in out.items()}, os.path.getsize(dst), 'bytes')


if __name__ == '__main__':
    main()
