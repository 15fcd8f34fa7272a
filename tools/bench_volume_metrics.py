"""The reference's per-subject metrics (evaluate.py:73-87: evaluate_3D + evaluate_slice) of one predicted volume: host way against device way.

One synthetic (64, 256, 256) subject (afcm_amd/synthetic.py) as the target and a noisy copy as the prediction, both float32 in the network's range and
already on the device, as predict_volume(where='device') leaves them.  Two arms, alternated in one process after a warm-up of each:
  (a) host    what evaluate.py does: copy the prediction to the host, to_unit_range, float64, evaluation.evaluate_3D + evaluate_slice (the target's
              float64 copy is made once, outside the clock: evaluate.py reads it from disk)
  (b) device  volume.volume_metrics(with_3d=True), the metric half of evaluate_volume: three plane_stats, afcm_volume_ssim, one copy, the numpy finishers
              (it also returns evaluate_one, which the host arm does not compute)
Wall time is a host clock from a synchronised device to the tuples on the host.  The device arm's launches alone are timed with device events, and
afcm_volume_ssim on its own, whose time gives the read bandwidth of its z-sum stage: every staged voxel is requested seven times per image.
Exit status 0: the six numbers agree within the finishers' test bounds and (b) beats (a) by more than the largest spread of an arm.

    python tools/bench_volume_metrics.py [--depth 64] [--res 256] [--repeats 3]
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d <dir> -- python3 tools/bench_volume_metrics.py --kernel-only 4
        (counters in a run of their own: afcm_volume_ssim alone, N launches on the same subject, nothing timed)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOL_PSNR_DB, TOL_SSIM, TOL_MAE_REL = 1e-9, 1e-10, 2e-6      # tests/test_gpu_volume.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, default=64)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--kernel-only', type=int, default=0, metavar='N', help='launch afcm_volume_ssim N times on the subject and exit (for a counter pass)')
    args = ap.parse_args()

    import numpy as np
    import torch
    from afcm_amd import evaluation, synthetic
    from afcm_amd.torch_utils.ops.plane_metrics import plane_stats
    from afcm_amd.torch_utils.ops.volume_metrics import TILE_X, TILE_Y, volume_ssim_layers
    from afcm_amd.volume import volume_metrics
    if not torch.cuda.is_available():
        raise SystemExit('bench_volume_metrics.py needs a GPU: a time taken without one says nothing')
    dev = torch.device('cuda:0')
    d, h, w = args.depth, args.res, args.res
    target = synthetic.mr_like_slices(d, 1, args.res, seed=0)[:, 0].contiguous()
    fake = (target * 1.05 + 0.04 * torch.randn(target.shape, generator=torch.Generator().manual_seed(1))).to(dev)     # overshoots [-1, 1]: the clip acts
    target64 = evaluation.to_unit_range(target.numpy()).astype(np.float64)
    target = target.to(dev)
    if args.kernel_only:
        for _ in range(args.kernel_only):
            layers = volume_ssim_layers(target[None], fake[None], unit_map=True)
        torch.cuda.synchronize()
        print(f'{args.kernel_only} launches of afcm_volume_ssim on ({d}, {h}, {w}); SSIM {float(layers.sum()) / ((d - 6) * (h - 6) * (w - 6))!r}')
        return 0

    def host():
        pred64 = evaluation.to_unit_range(fake.cpu().numpy()).astype(np.float64)
        return evaluation.evaluate_3D(pred64, target64) + evaluation.evaluate_slice(pred64, target64)

    def device():
        out = volume_metrics(fake, target, from_network_range=True, with_3d=True)
        return out['3d'] + out['slice']

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        numbers = fn()
        return (time.perf_counter() - t0) * 1e3, numbers

    arms, numbers = {'host': [], 'device': []}, {}
    fns = {'host': host, 'device': device}
    for name in arms:                                                          # warm-up: allocator pools, the first launches, scipy's first call
        clock(fns[name])
    for rep in range(args.repeats):
        for name in arms:
            ms, numbers[name] = clock(fns[name])
            arms[name].append(ms)

    views = ((0, 1, 2), (1, 0, 2), (2, 0, 1))
    events = {}
    for what, fn in (('all metric launches', lambda: ([plane_stats(target.permute(*p), fake.permute(*p), unit_map=True) for p in views],
                                                      volume_ssim_layers(target[None], fake[None], unit_map=True))),
                     ('volume_ssim', lambda: volume_ssim_layers(target[None], fake[None], unit_map=True))):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(20):
            fn()
        e1.record()
        torch.cuda.synchronize()
        events[what] = e0.elapsed_time(e1) * 1e3 / 20

    # bytes of the z-sum stage, from the shape: per (z origin, tile) every voxel under the tile's windows, seven z-neighbours, two float32 images
    staged = sum((min(TILE_Y, h - 6 - y0) + 6) * (min(TILE_X, w - 6 - x0) + 6) for y0 in range(0, h - 6, TILE_Y) for x0 in range(0, w - 6, TILE_X))
    requested, resident = (d - 6) * staged * 7 * 2 * 4, d * h * w * 2 * 4
    seconds = events['volume_ssim'] * 1e-6

    print(f'volume metrics of one ({d}, {h}, {w}) float32 subject and its target, both on the device; {args.repeats} repeats of the alternation host / '
          f'device after one warm-up of each arm')
    print(f'{"arm":8s} {"ms/volume per repeat":36s} {"mean":>10s} {"spread (max - min)":>20s}')
    stats = {}
    for name, v in arms.items():
        stats[name] = dict(per_repeat_ms=v, mean_ms=sum(v) / len(v), spread_ms=max(v) - min(v))
        print(f'{name:8s} {"  ".join(f"{x:10.3f}" for x in v):36s} {stats[name]["mean_ms"]:10.3f} {stats[name]["spread_ms"]:20.3f}')
    spread = max(s['spread_ms'] for s in stats.values())
    gain = stats['host']['mean_ms'] - stats['device']['mean_ms']
    print(f'host - device = {gain:.3f} ms/volume (largest spread of an arm: {spread:.3f} ms), {stats["host"]["mean_ms"] / stats["device"]["mean_ms"]:.1f}x')
    print(f'launches alone (device events, mean of 20): all metric launches {events["all metric launches"]:.1f} us, afcm_volume_ssim {events["volume_ssim"]:.1f} us')
    print(f'afcm_volume_ssim reads: {requested / 1e6:.1f} MB requested by the z-sum stage (the subject and its target occupy {resident / 1e6:.1f} MB: '
          f'{requested / resident:.2f} requests per resident byte) = {requested / seconds / 1e12:.3f} TB/s over the WHOLE kernel time (z-sums, the column walk and '
          f'the layer pass together: a lower bound for the stage); {resident / seconds / 1e12:.3f} TB/s counted once')
    names = ('psnr', 'ssim', 'mae', 'psnr_slice', 'ssim_slice', 'mae_slice')
    diffs = {}
    for i, n in enumerate(names):
        a, b = numbers['host'][i], numbers['device'][i]
        diffs[n] = abs(a - b) / abs(a) if n.startswith('mae') else abs(a - b)
        print(f'{n:11s} host {a!r:24} device {b!r:24} difference {diffs[n]:.3e}{" relative" if n.startswith("mae") else " dB" if n.startswith("psnr") else ""}')
    agree = all(diffs[n] <= (TOL_MAE_REL if n.startswith('mae') else TOL_PSNR_DB if n.startswith('psnr') else TOL_SSIM) for n in names)
    print(f'the six numbers {"agree" if agree else "DO NOT agree"} within {TOL_PSNR_DB} dB / {TOL_SSIM} / {TOL_MAE_REL} relative')
    print(json.dumps(dict(bench='volume_metrics', depth=d, res=args.res, arms=stats, launches_us=events, zsum_requested_bytes=requested, resident_bytes=resident,
                          host_minus_device_ms=gain, largest_spread_ms=spread, device_beats_host=gain > spread, differences=diffs, numbers_agree=agree)))
    return 0 if (agree and gain > spread) else 1


if __name__ == '__main__':
    sys.exit(main())
