#!/usr/bin/env python3
"""Golden vectors for the per-plane normalisers (afcm_amd/normalise.py, csrc/normalise.hip), captured from the reference's own classes.

data/augment/transforms.py cannot be imported where cv2 / skimage are absent (its top-level imports), so ``Standardize`` and
``PercentileNormalizer`` (transforms.py:552-601) are compiled on their own from the reference's syntax tree at generation time, given ``numpy`` as
the module gives it, and called with the configuration's arguments (configs/defaults.py:52-57 for the train phase, 109-114 for the test phase)
on small [1, H, W] planes of the four source dtypes.  Only inputs, outputs and the ``np.percentile`` / ``np.mean`` / ``np.std`` values are stored
(tests/golden/N1_normalise.npz).

    python tools/gen_golden_normalise.py <reference checkout>
"""
import ast
import os
import sys

import numpy as np

PERCENTILES = ((1.0, 99.6), (0.0, 100.0))                  # the train default, the test default (per-plane min-max scaling)
FIXED = (100.0, 40.0)                                      # an explicit (mean, std)
SHAPES = ((5, 7), (16, 16), (33, 47))


def extract_classes(path, names):
    tree = ast.parse(open(path).read())
    nodes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in names]
    ns = {'np': np}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, 'exec'), ns)
    return [ns[n] for n in names]


def plane(h, w, dtype, seed):
    """A bright blob on a dark, partly zero background: the histogram of an MR slice in small."""
    rng = np.random.default_rng(seed)
    v = rng.gamma(2.0, 40.0, size=(1, h, w))
    v[rng.random((1, h, w)) < 0.25] = 0.0
    if np.dtype(dtype) == np.int16:
        v = v * 8.0 - 300.0
    if np.dtype(dtype).kind in 'iu':
        info = np.iinfo(dtype)
        return np.clip(np.rint(v), info.min, info.max).astype(dtype)
    return (v - 20.0).astype(dtype)


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    standardize, percentile = extract_classes(os.path.join(sys.argv[1], 'data/augment/transforms.py'), ['Standardize', 'PercentileNormalizer'])
    out = {'percentiles': np.array(PERCENTILES), 'fixed': np.array(FIXED)}
    for dtype in (np.uint8, np.int16, np.float32, np.float64):
        for h, w in SHAPES:
            name = f'{np.dtype(dtype).name}_{h}x{w}'
            x = plane(h, w, dtype, seed=h * w + np.dtype(dtype).itemsize)
            out[f'{name}_x'] = x
            for j, (pmin, pmax) in enumerate(PERCENTILES):
                out[f'{name}_p{j}'] = np.asarray(percentile(pmin=pmin, pmax=pmax)(x))
                out[f'{name}_p{j}_bounds'] = np.array([np.percentile(x, pmin), np.percentile(x, pmax)], dtype=np.float64)
            out[f'{name}_s'] = np.asarray(standardize()(x))
            out[f'{name}_s_moments'] = np.array([np.mean(x), np.std(x)], dtype=np.float64)
            out[f'{name}_f'] = np.asarray(standardize(mean=FIXED[0], std=FIXED[1])(x))
    dst = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'N1_normalise.npz')
    np.savez_compressed(dst, **out)
    print('wrote', dst, len(out), 'arrays', os.path.getsize(dst), 'bytes')


if __name__ == '__main__':
    main()
