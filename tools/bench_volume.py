"""Whole-volume inference on the full-width 256^2 generator: what one subject costs, host way against device way.

Two arms over the same synthetic (64, 256, 256) uint8 subject (afcm_amd/synthetic.py), alternated in one process after a warm-up of each and the whole
alternation repeated:
  (a) host    volume.predict_volume(where='host'): SliceDataset items built in numpy, one upload per batch, the EMA forward,
              SlidingWindowPredictor.accumulate behind a device -> host copy per batch (the package's path before the device arm existed)
  (b) device  volume.predict_volume(where='device'): the subject uploaded once, afcm_slice_assemble + the EMA forward + afcm_halo_accumulate per
              batch, map / mask at the end; nothing is read back inside the loop
Wall time per volume is a host clock around the call, ended by a synchronise (the host arm has synchronised by its copies already; the device arm's
result stays on the device, as evaluate_volume consumes it).  The two new launches alone are also timed with device events.  The two volumes are
compared bit for bit.  Exit status 0: the volumes are equal and (b) beats (a) by more than the largest spread of an arm.

    python tools/bench_volume.py [--depth 64] [--batch 16] [--repeats 3] [--dtype bf16]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--depth', type=int, default=64)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--thickness', type=int, default=5)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp16', 'fp32'])
    args = ap.parse_args()

    import torch
    from afcm_amd import layer_schedule as sched, synthetic
    from afcm_amd.networks_stylegan3 import Stylegan3Generator
    from afcm_amd.stylegan3_model import StyleGAN3GeneratorStep
    from afcm_amd.torch_utils.ops.volume_ops import assemble_slices, halo_accumulate
    from afcm_amd.volume import PatchPlan, predict_volume
    from afcm_amd.predictor import patch_indices
    if not torch.cuda.is_available():
        raise SystemExit('bench_volume.py needs a GPU: a time taken without one says nothing')
    dev = torch.device('cuda:0')
    dtype = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}[args.dtype]
    torch.manual_seed(0)
    G = Stylegan3Generator(z_dim=512, c_dim=1, w_dim=512, img_resolution=args.res, img_channels_in=4, img_channels_out=1, mapping_kwargs=dict(num_layers=8),
                           synthesis_kwargs=dict(dict(sched.DEFAULT_SYNTHESIS_KWARGS), compute_dtype=dtype)).to(dev)
    step = StyleGAN3GeneratorStep(G, ema=True)
    # one subject: MR-like slices in the network's range, back to the uint8 values the loader reads
    subject = ((synthetic.mr_like_slices(args.depth, 1, args.res, seed=0)[:, 0] + 1) * 127.5).round().clamp(0, 255).to(torch.uint8).numpy()
    kw = dict(raw_internal_path_in='raw', thickness=args.thickness, patch_hw=(args.res, args.res), batch_size=args.batch, patch_halo=(0, 8, 8))

    def clock(where):
        torch.manual_seed(1)                                                   # set_test_input draws gen_z: the same draws for both arms
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = predict_volume(step, {'raw': subject}, where=where, **kw)['prediction']
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    arms, volumes = {'host': [], 'device': []}, {}
    for name in arms:                                                          # warm-up: allocator pools, workspace caches, the first launches
        clock(name)
    for rep in range(args.repeats):
        for name in arms:
            ms, volumes[name] = clock(name)
            arms[name].append(ms)
    equal = torch.equal(volumes['device'].cpu(), volumes['host'])

    # the two new launches alone, by device events, on the shapes of one batch
    volume = torch.from_numpy(subject).to(dev)
    shape = (args.depth, args.res, args.res)
    plan = PatchPlan(shape, patch_indices(shape, (1, args.res, args.res), (1, 1, 1)))
    pmap, mask = torch.zeros((1,) + shape, device=dev), torch.zeros((1,) + shape, dtype=torch.uint8, device=dev)
    fake = step.fake_B[:args.batch]
    count = int(fake.shape[0])
    events = {}
    for what, fn in (('slice_assemble', lambda: assemble_slices(volume, 0, count, (1, args.res, args.res), thickness=args.thickness)),
                     ('halo_accumulate', lambda: halo_accumulate(pmap, mask, fake, plan.table(dev), 0, (0, 8, 8), box=plan.bounding_box(0, count)))):
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

    batches = -(-args.depth // args.batch)
    print(f'volume prediction, {args.res}^2 full-width generator ({args.dtype} training dtype, EMA copy in {step.netG_ema.synthesis.compute_dtype}), one '
          f'({args.depth}, {args.res}, {args.res}) uint8 subject, thickness {args.thickness}, batch {args.batch} ({batches} batches), {args.repeats} repeats of the '
          f'alternation after one warm-up of each arm; fake_B is {step.fake_B.dtype}')
    print(f'{"arm":8s} {"ms/volume per repeat":36s} {"mean":>9s} {"ms/batch":>9s} {"spread (max - min)":>20s}')
    stats = {}
    for name, v in arms.items():
        stats[name] = dict(per_repeat_ms=v, mean_ms=sum(v) / len(v), spread_ms=max(v) - min(v))
        print(f'{name:8s} {"  ".join(f"{x:10.3f}" for x in v):36s} {stats[name]["mean_ms"]:9.3f} {stats[name]["mean_ms"] / batches:9.3f} {stats[name]["spread_ms"]:20.3f}')
    spread = max(s['spread_ms'] for s in stats.values())
    gain = stats['host']['mean_ms'] - stats['device']['mean_ms']
    print(f'host - device = {gain:.3f} ms/volume (largest spread of an arm: {spread:.3f} ms), {stats["host"]["mean_ms"] / stats["device"]["mean_ms"]:.2f}x; '
          f'launches alone (device events, one batch of {count}): slice_assemble {events["slice_assemble"]:.1f} us, halo_accumulate {events["halo_accumulate"]:.1f} us')
    print(f'the two arms\' volumes are {"bit-identical" if equal else "DIFFERENT"}')
    print(json.dumps(dict(bench='volume_predict', res=args.res, depth=args.depth, batch=args.batch, thickness=args.thickness, dtype=args.dtype, arms=stats,
                          launches_us=events, host_minus_device_ms=gain, largest_spread_ms=spread, device_beats_host=gain > spread, volumes_equal=equal)))
    return 0 if (equal and gain > spread) else 1


if __name__ == '__main__':
    sys.exit(main())
