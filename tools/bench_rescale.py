"""Intensity rescaling: what the device op costs against the host ways, on one box.

Per source dtype, one synthetic (180, 256, 256) volume (a gamma-distributed foreground over a 40 % zero background):
  device     torch_utils.ops.intensity_ops.rescale_intensity on the uploaded volume: the first call of the process ("cold": code-object load, allocator)
             and then ``--repeats`` warm calls, each between two device events; the upload itself is timed apart
  host       intensity.rescale_intensity_host (float64 statement, numpy)
  float32    for the float32 volume, the reference's way: numpy percentiles and arithmetic in the array's own type
Then ``predict_volume`` on a raw int16 subject with the full-width 256^2 generator: ``rescale=`` on the device against rescaling on the host first.
Host times are a host clock; device times are device events around work on one stream.  The device and host results are compared bit for bit.

    python tools/bench_rescale.py [--repeats 10] [--depth 180] [--no-predict]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def volume_of(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    v = rng.gamma(2.0, 300.0, size=shape)
    v[rng.random(shape) < 0.4] = 0.0
    if np.dtype(dtype) == np.uint8:
        return np.clip(np.rint(v / 8.0), 0, 255).astype(np.uint8)
    if np.dtype(dtype) == np.int16:
        return np.clip(np.rint(v), 0, 32767).astype(np.int16)
    return v.astype(dtype)


def float32_way(volume, percentiles=(0.5, 99.5)):
    """What numpy does with the reference's expression on a float32 volume: percentiles and arithmetic stay float32."""
    mask = volume > 0
    fg = volume[mask]
    lo, hi = np.percentile(fg, percentiles[0]), np.percentile(fg, percentiles[1])
    level = np.clip(np.round((fg - lo) / (hi - lo) * 255), 1, 255)
    out = np.zeros(volume.shape, dtype=np.uint8)
    out[mask] = level.astype(np.uint8)
    return out


def spread(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--host-repeats', type=int, default=2)
    ap.add_argument('--depth', type=int, default=180)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--no-predict', action='store_true')
    args = ap.parse_args()
    import torch
    from afcm_amd.intensity import rescale_intensity_host
    from afcm_amd.torch_utils.ops.intensity_ops import rescale_intensity, rescale_plan
    if not torch.cuda.is_available():
        raise SystemExit('bench_rescale.py needs a GPU: a time taken without one says nothing')
    shape = (args.depth, args.res, args.res)
    result = dict(bench='rescale_intensity', shape=shape, dtypes={})
    print(f'rescale_intensity on {shape}: device events per call (us), host clock per call (ms)')
    for k, dtype in enumerate((np.float32, np.uint8, np.int16, np.float64)):
        name = np.dtype(dtype).name
        v = volume_of(shape, dtype, 30 + k)
        t0 = time.perf_counter()
        dev = torch.from_numpy(v).cuda()
        torch.cuda.synchronize()
        upload_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        out, stats = rescale_intensity(dev)
        torch.cuda.synchronize()
        cold_ms = (time.perf_counter() - t0) * 1e3
        warm = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out, stats = rescale_intensity(dev)
            e1.record()
            torch.cuda.synchronize()
            warm.append(e0.elapsed_time(e1) * 1e3)
        host = []
        for _ in range(args.host_repeats):
            t0 = time.perf_counter()
            want, want_stats = rescale_intensity_host(v)
            host.append((time.perf_counter() - t0) * 1e3)
        equal = bool(np.array_equal(out.cpu().numpy(), want) and np.array_equal(stats.cpu().numpy(), want_stats))
        row = dict(plan=rescale_plan(v.size, dev.dtype), upload_ms=upload_ms, cold_ms=cold_ms, warm_us=spread(warm), host_ms=spread(host), equal=equal)
        if name == 'float32':
            ref = []
            for _ in range(args.host_repeats):
                t0 = time.perf_counter()
                other = float32_way(v)
                ref.append((time.perf_counter() - t0) * 1e3)
            row['float32_way_ms'] = spread(ref)
            row['float32_way_differing_share'] = float((other != want).mean())
        result['dtypes'][name] = row
        print(f'{name:8s} passes {row["plan"]["passes"]} groups {row["plan"]["groups"]:3d}  upload {upload_ms:7.2f} ms  cold {cold_ms:8.2f} ms  warm median '
              f'{row["warm_us"]["median"]:8.1f} us [{row["warm_us"]["min"]:.1f}, {row["warm_us"]["max"]:.1f}]  host median {row["host_ms"]["median"]:8.1f} ms '
              f'[{row["host_ms"]["min"]:.1f}, {row["host_ms"]["max"]:.1f}]' + (f'  float32 way {row["float32_way_ms"]["median"]:.1f} ms' if name == 'float32' else '')
              + f'  {"bit-identical" if equal else "DIFFERENT"}')

    if not args.no_predict:
        from afcm_amd import layer_schedule as sched
        from afcm_amd.networks_stylegan3 import Stylegan3Generator
        from afcm_amd.stylegan3_model import StyleGAN3GeneratorStep
        from afcm_amd.volume import predict_volume
        torch.manual_seed(0)
        G = Stylegan3Generator(z_dim=512, c_dim=1, w_dim=512, img_resolution=args.res, img_channels_in=4, img_channels_out=1, mapping_kwargs=dict(num_layers=8),
                               synthesis_kwargs=dict(dict(sched.DEFAULT_SYNTHESIS_KWARGS), compute_dtype=torch.bfloat16)).cuda()
        step = StyleGAN3GeneratorStep(G, ema=True)
        raw = volume_of(shape, np.int16, 40)
        kw = dict(raw_internal_path_in='raw', thickness=5, patch_hw=(args.res, args.res), batch_size=16, patch_halo=(0, 8, 8))

        def fed():
            return predict_volume(step, {'raw': raw}, where='device', rescale=(0.5, 99.5), **kw)['prediction']

        def host_first():
            return predict_volume(step, {'raw': rescale_intensity_host(raw)[0]}, where='device', **kw)['prediction']
        arms, outs = {'device_rescale': [], 'host_rescale_first': []}, {}
        for name, fn in (('device_rescale', fed), ('host_rescale_first', host_first)):
            fn()
        for _ in range(3):
            for name, fn in (('device_rescale', fed), ('host_rescale_first', host_first)):
                torch.manual_seed(1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs[name] = fn()
                torch.cuda.synchronize()
                arms[name].append((time.perf_counter() - t0) * 1e3)
        result['predict_volume_ms'] = {k: spread(v) for k, v in arms.items()}
        result['predict_volume_equal'] = bool(torch.equal(outs['device_rescale'], outs['host_rescale_first']))
        for k, v in result['predict_volume_ms'].items():
            print(f'predict_volume {k:20s} median {v["median"]:9.1f} ms [{v["min"]:.1f}, {v["max"]:.1f}]')
        print(f'the two arms\' volumes are {"bit-identical" if result["predict_volume_equal"] else "DIFFERENT"}')
    print(json.dumps(result))
    f32 = result['dtypes']['float32']
    return 0 if all(r['equal'] for r in result['dtypes'].values()) and f32['warm_us']['median'] * 1e-3 < f32['host_ms']['median'] else 1


if __name__ == '__main__':
    sys.exit(main())
