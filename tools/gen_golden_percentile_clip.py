"""Captures tests/golden/I2_percentile_clip.npz from the reference's own ``StandardNIIDataset.__percentile_clip`` (data/cmsrnii_dataset.py:79-103)
followed by its caller's ``(x * 255).astype('uint8')`` (:110-111).

    python tools/gen_golden_percentile_clip.py --reference /path/to/AFCM

The function is compiled out of the module's syntax tree by name, as tools/gen_golden_intensity.py does it: the module itself cannot be imported (its
top level needs SimpleITK).  It is a method whose name is mangled inside its class, so the ``FunctionDef`` is taken from the ``ClassDef`` body and
called with ``None`` for ``self``.  One small volume in the four source dtypes: a zero background of about 30 %, a negative tail of about 10 % (none
for uint8), a gamma-distributed foreground.  Per dtype and for ``strictlyPositive`` true and false: the reference's uint8 volume and its two bounds
(recomputed the way the function does, since it does not return them), the share of voxels at which the reference and the float64 statement of
include/afcm_hip.h differ, and the largest difference in grey levels.
"""
import argparse
import ast
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import percentile_clip_ref as R  # noqa: E402

SHAPE, SEED, PERCENTILES = (8, 40, 40), 21, (0.5, 99.5)


def reference_function(tree_root, name='__percentile_clip', owner='StandardNIIDataset', module='data/cmsrnii_dataset.py'):
    path = os.path.join(tree_root, module)
    tree = ast.parse(open(path).read(), filename=path)
    classes = [node for node in tree.body if isinstance(node, ast.ClassDef) and node.name == owner]
    assert len(classes) == 1, f'{owner} not found in {path}'
    found = [node for node in classes[0].body if isinstance(node, ast.FunctionDef) and node.name == name]
    assert len(found) == 1, f'{name} not found in {owner}'
    scope = {'np': np}
    exec(compile(ast.Module(body=found, type_ignores=[]), path, 'exec'), scope)      # at module level: the name is not mangled
    return scope[name]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference tree')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'I2_percentile_clip.npz'))
    args = ap.parse_args()
    fn = reference_function(args.reference)
    out = {'percentiles': np.array(PERCENTILES), 'numpy_version': np.array(np.__version__)}
    for dtype in R.DTYPES:
        name = np.dtype(dtype).name
        volume = R.signed_volume(SHAPE, dtype, SEED)
        out[f'volume_{name}'] = volume
        for positive in (True, False):
            tag = f'{name}_{"positive" if positive else "signed"}'
            with np.errstate(all='ignore'):
                got = fn(None, volume.copy(), p_min=PERCENTILES[0], p_max=PERCENTILES[1], strictlyPositive=positive)
                got = (got * 255).astype('uint8')
            v_min, v_max = np.percentile(volume, list(PERCENTILES))
            if v_min < 0 and positive:
                v_min = 0
            out[f'clipped_{tag}'], out[f'bounds_{tag}'] = got, np.array([v_min, v_max], dtype=np.float64)
            ours, stats = R.clip(volume, PERCENTILES, positive)
            diff = np.abs(ours.astype(np.int16) - got.astype(np.int16))
            out[f'differing_share_{tag}'] = np.array(float((diff > 0).mean()))
            out[f'largest_difference_{tag}'] = np.array(int(diff.max()))
            print(f'{tag}: zeros {np.mean(volume == 0):.3f}, negatives {np.mean(volume < 0):.3f}, bounds {float(v_min)!r} {float(v_max)!r} (statement '
                  f'{stats[0]!r} {stats[1]!r}), differing voxels {int((diff > 0).sum())} of {diff.size} (largest {int(diff.max())})')
    np.savez_compressed(args.out, **out)
    print(f'{args.out}: {os.path.getsize(args.out)} bytes')


if __name__ == '__main__':
    main()
