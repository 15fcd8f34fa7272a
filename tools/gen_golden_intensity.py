"""Captures tests/golden/I1_rescale_intensity.npz from the reference's own ``rescale_intensity`` (data/prepare_h5.py:9-26) followed by its caller's
``around`` / ``clip(0, 255)`` / ``uint8`` (:38-41).

    python tools/gen_golden_intensity.py --reference /path/to/AFCM

The function is compiled out of the module's syntax tree by name: the module itself cannot be imported (its top level needs SimpleITK and h5py and
runs a conversion loop).  One small volume in the four source dtypes: a zero background of about 40 %, a few negative voxels, a gamma-distributed
foreground.  For the float32 case the file also records the share of voxels at which the reference (float32 arithmetic, as numpy keeps a float32
array's type) and the float64 statement of include/afcm_hip.h differ, and the largest difference in grey levels.
"""
import argparse
import ast
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import intensity_ref as R  # noqa: E402

SHAPE, SEED, PERCENTILES = (8, 40, 40), 20, (0.5, 99.5)


def reference_function(tree_root, name='rescale_intensity', module='data/prepare_h5.py'):
    path = os.path.join(tree_root, module)
    tree = ast.parse(open(path).read(), filename=path)
    found = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name == name]
    assert len(found) == 1, f'{name} not found in {path}'
    scope = {'np': np}
    exec(compile(ast.Module(body=found, type_ignores=[]), path, 'exec'), scope)
    return scope[name]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference tree')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'I1_rescale_intensity.npz'))
    args = ap.parse_args()
    fn = reference_function(args.reference)
    out = {'percentiles': np.array(PERCENTILES)}
    for dtype in R.DTYPES:
        name = np.dtype(dtype).name
        volume = R.skewed_volume(SHAPE, dtype, SEED)
        got = fn(volume.copy(), percentils=list(PERCENTILES))
        got = np.clip(np.around(got), 0, 255).astype('uint8')
        out[f'volume_{name}'], out[f'rescaled_{name}'] = volume, got
        ours = R.rescale(volume, PERCENTILES)[0]
        diff = np.abs(ours.astype(np.int16) - got.astype(np.int16))
        print(f'{name}: background {np.mean(volume <= 0):.3f}, negatives {int((volume < 0).sum())}, differing voxels {int((diff > 0).sum())} of {diff.size}'
              f' (largest {int(diff.max())})')
        if name == 'float32':
            out['float32_differing_share'] = np.array(float((diff > 0).mean()))
            out['float32_largest_difference'] = np.array(int(diff.max()))
    np.savez_compressed(args.out, **out)
    print(f'{args.out}: {os.path.getsize(args.out)} bytes')


if __name__ == '__main__':
    main()
