"""Percentile-clip normalisation: what the device op costs, launch group by launch group, beside the foreground rescaling and the host function.

Per source dtype and for a (64, 256, 256) and a (160, 256, 256) synthetic volume (a gamma-distributed foreground over a 30 % zero background and a
10 % negative tail; uint8 has no negatives), four device arms, each ``--inner`` calls between two device events:
  bounds     torch_utils.ops.intensity_ops.percentile_bounds: the select's histogram and scan launches (uint8 1 + 1, int16 2 + 2, float32 4 + 4,
             float64 8 + 8)
  map        afcm_clip_normalize alone, on bounds already in place
  clip       percentile_clip, both together
  rescale    rescale_intensity on the same volume: the same loads, the foreground select (uint8 1, int16 1, float32 4, float64 8 digit passes)
The arms alternate inside every repeat, so drift of the box falls on all of them alike; median, minimum and maximum per call are reported, and the
select's time per digit pass for the signed keys (bounds / passes) and for the foreground keys (rescale minus the clip's map, which stands in for
the rescaling's own map of the same loads and stores, / passes).  ``percentile_clip_host`` is timed with a host clock and its result compared
with the device's: volume equal, bounds numerically equal.  ``--background 0 --negative 0`` gives a volume that is all foreground, on which the
foreground select counts every voxel too: what the two selects differ by there is the cost of the signed key itself.

    python tools/bench_percentile_clip.py [--repeats 10] [--inner 10] [--background 0.3] [--negative 0.1] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def volume_of(shape, dtype, seed, background=0.3, negative=0.1):
    rng = np.random.default_rng(seed)
    v = rng.gamma(2.0, 300.0, size=shape) + 8.0                             # + 8: with no background asked for, no voxel rounds to zero
    u = rng.random(shape)
    v[u < background] = 0.0
    tail = u > 1.0 - negative
    v[tail] = -rng.gamma(2.0, 40.0, size=int(tail.sum()))
    if np.dtype(dtype) == np.uint8:
        return np.clip(np.rint(v / 8.0), 0, 255).astype(np.uint8)
    if np.dtype(dtype) == np.int16:
        return np.clip(np.rint(v), -32768, 32767).astype(np.int16)
    return v.astype(dtype)


def spread(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--inner', type=int, default=10, help='calls between two device events')
    ap.add_argument('--host-repeats', type=int, default=2)
    ap.add_argument('--depths', type=int, nargs='+', default=[64, 160])
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--background', type=float, default=0.3, help='share of zero voxels')
    ap.add_argument('--negative', type=float, default=0.1, help='share of negative voxels (uint8: they clip to zero)')
    ap.add_argument('--out', default=None, help='also write the JSON result here')
    args = ap.parse_args()
    import torch
    from afcm_amd import _lib
    from afcm_amd.intensity import percentile_clip_host
    from afcm_amd.torch_utils.ops.intensity_ops import percentile_bounds, percentile_clip, percentile_plan, rescale_intensity, rescale_plan
    if not torch.cuda.is_available():
        raise SystemExit('bench_percentile_clip.py needs a GPU: a time taken without one says nothing')
    lib = _lib.load()
    pair = (0.5, 99.5)
    result = dict(bench='percentile_clip', percentiles=pair, background=args.background, negative=args.negative, repeats=args.repeats, inner=args.inner, cases=[])
    print(f'percentile_clip, {args.inner} calls per event pair, {args.repeats} repeats: us per call, median [min, max]')
    ok = True
    for depth in args.depths:
        shape = (depth, args.res, args.res)
        for k, dtype in enumerate((np.uint8, np.int16, np.float32, np.float64)):
            name = np.dtype(dtype).name
            v = volume_of(shape, dtype, 50 + k, args.background, args.negative)
            dev = torch.from_numpy(v).cuda()
            out = torch.empty(shape, dtype=torch.uint8, device='cuda')
            stats = percentile_bounds(dev, pair)
            code, stream = _lib.source_code(dev.dtype, 'bench'), torch.cuda.current_stream().cuda_stream

            def map_only():
                _lib.launched(lib.afcm_clip_normalize(out.data_ptr(), stats.data_ptr(), dev.data_ptr(), code, *shape, dev.stride(0), stream), 'clip_normalize')
            arms = dict(bounds=lambda: percentile_bounds(dev, pair), map=map_only, clip=lambda: percentile_clip(dev, pair, out=out),
                        rescale=lambda: rescale_intensity(dev, pair, out=out))
            for fn in arms.values():                                        # code objects, allocator
                fn()
            torch.cuda.synchronize()
            times = {a: [] for a in arms}
            for _ in range(args.repeats):
                for a, fn in arms.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.inner):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    times[a].append(e0.elapsed_time(e1) * 1e3 / args.inner)
            got, got_stats = percentile_clip(dev, pair)
            host = []
            for _ in range(args.host_repeats):
                t0 = time.perf_counter()
                want, want_stats = percentile_clip_host(v, pair)
                host.append((time.perf_counter() - t0) * 1e3)
            equal = bool(np.array_equal(got.cpu().numpy(), want) and np.array_equal(got_stats.cpu().numpy(), want_stats, equal_nan=True))
            ok = ok and equal
            signed, foreground = percentile_plan(v.size, dev.dtype), rescale_plan(v.size, dev.dtype)
            row = dict(shape=shape, dtype=name, passes=signed['passes'], groups=signed['groups'], rescale_passes=foreground['passes'],
                       rescale_groups=foreground['groups'], us={a: spread(t) for a, t in times.items()}, host_ms=spread(host), equal=equal)
            row['select_us_per_pass'] = row['us']['bounds']['median'] / signed['passes']
            row['rescale_select_us_per_pass'] = (row['us']['rescale']['median'] - row['us']['map']['median']) / foreground['passes']
            result['cases'].append(row)
            cells = '  '.join(f'{a} {s["median"]:7.1f} [{s["min"]:.1f}, {s["max"]:.1f}]' for a, s in row['us'].items())
            print(f'{str(shape):16s} {name:8s} passes {signed["passes"]} / {foreground["passes"]}  {cells}  per pass {row["select_us_per_pass"]:.1f} / '
                  f'{row["rescale_select_us_per_pass"]:.1f}  host {row["host_ms"]["median"]:.0f} ms  {"equal" if equal else "DIFFERENT"}')
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
