"""Validation loop on the full-width 256^2 generator: what the metrics cost per batch, host way against device way.

Three arms over the same 8 validation batches (after 2 warm-up batches each), alternated in one process and the whole alternation repeated:
  (a) floor   set_input + test() per batch, synchronised per batch: the EMA generator's forward alone
  (b) host    validation.validate(metrics='host'): copy both images to the host, to_unit_range, evaluation.evaluate_2D (the reference's way)
  (c) device  validation.validate(metrics='device'): afcm_plane_metrics per batch, one copy of the tables at the end
Wall time per batch is a host clock around a loop that ends in a synchronise (the floor synchronises per batch, (b) by its copies, (c) by its
final copy).  For (c) the metric launches alone are also timed with device events around the 8 batches' plane_stats calls.  The metric values
of (b) and (c) are printed side by side and checked against the test tolerances (1e-9 dB, 1e-10, 2e-6 relative); a third row repeats (b) on float64
copies of its arrays, which separates the float32 division of psnr_2D on float32 arrays from everything else.  Exit status 0: the values agree and
(c) beats (b) by more than the largest spread of an arm.

    python tools/bench_validation.py [--batch 16] [--batches 8] [--warmup 2] [--repeats 3] [--dtype bf16]
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
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--batches', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp16', 'fp32'])
    args = ap.parse_args()

    import torch
    from afcm_amd import evaluation_device, layer_schedule as sched, synthetic
    from afcm_amd.networks_stylegan3 import Stylegan3Generator
    from afcm_amd.stylegan3_model import StyleGAN3GeneratorStep
    from afcm_amd.validation import validate
    if not torch.cuda.is_available():
        raise SystemExit('bench_validation.py needs a GPU: a time taken without one says nothing')
    dev = torch.device('cuda:0')
    dtype = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}[args.dtype]
    torch.manual_seed(0)
    G = Stylegan3Generator(z_dim=512, c_dim=1, w_dim=512, img_resolution=args.res, img_channels_in=4, img_channels_out=1, mapping_kwargs=dict(num_layers=8),
                           synthesis_kwargs=dict(dict(sched.DEFAULT_SYNTHESIS_KWARGS), compute_dtype=dtype)).to(dev)
    step = StyleGAN3GeneratorStep(G, ema=True)
    data = [synthetic.generator_inputs(args.batch, size=args.res, seed=s, device=dev)[:2] for s in range(args.warmup + args.batches)]
    warm, timed = data[:args.warmup], data[args.warmup:]

    def floor(batches):
        for real_A, real_B in batches:
            step.set_input(real_A, real_B)
            step.test()
            torch.cuda.synchronize()

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / len(timed) * 1e3, out

    arms = {'floor': [], 'host': [], 'device': []}
    values = {}
    for rep in range(args.repeats):
        for name in ('floor', 'host', 'device'):
            torch.manual_seed(1)                                               # set_input draws gen_z: the same draws for every arm
            if name == 'floor':
                floor(warm)
                ms, _ = clock(lambda: floor(timed))
            else:
                validate(step, warm, metrics=name)
                ms, values[name] = clock(lambda: validate(step, timed, metrics=name))
            arms[name].append(ms)

    # where a difference between the two arms comes from: the host arm once more on float64 copies of the same mapped float32 arrays, so that
    # psnr_2D divides by the maxima in float64 as the table does (on float32 arrays numpy divides in float32: one rounding of 2^-24 per element)
    import numpy as np
    from afcm_amd import evaluation
    torch.manual_seed(1)
    validate(step, warm, metrics='device')                                     # (the same gen_z draws as the timed loops)
    per_batch = []
    for real_A, real_B in timed:
        step.set_input(real_A, real_B)
        step.test()
        pred, target = (evaluation.to_unit_range(t[:, 0].float().cpu().numpy()).astype(np.float64)[:, None, None] for t in (step.fake_B, step.real_B))
        per_batch.append(evaluation.evaluate_2D(pred, target))
    counted = [r for r in per_batch if r is not None]
    values['host_f64'] = dict(psnr=float(np.mean([r[0] for r in counted])), ssim=float(np.mean([r[1] for r in counted])),
                              mae=float(np.mean([r[2] for r in counted])), batches=len(per_batch), batches_counted=len(counted))

    # the metric launches alone, by device events, on the last batch's images (three kernels per call)
    fake, real = step.fake_B, step.real_B
    for _ in range(3):
        evaluation_device.batch_stats(fake, real)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(len(timed)):
        evaluation_device.batch_stats(fake, real)
    e1.record()
    torch.cuda.synchronize()
    metric_us = e0.elapsed_time(e1) * 1e3 / len(timed)

    print(f'validation loop, {args.res}^2 full-width generator ({args.dtype} training dtype, EMA copy in {step.netG_ema.synthesis.compute_dtype}), '
          f'batch {args.batch}, {len(timed)} batches after {len(warm)} warm-up, {args.repeats} repeats of the alternation; fake_B is {fake.dtype}')
    print(f'{"arm":8s} {"ms/batch per repeat":36s} {"mean":>8s} {"spread (max - min)":>20s}')
    stats = {}
    for name, v in arms.items():
        stats[name] = dict(per_repeat_ms=v, mean_ms=sum(v) / len(v), spread_ms=max(v) - min(v))
        print(f'{name:8s} {"  ".join(f"{x:9.3f}" for x in v):36s} {stats[name]["mean_ms"]:8.3f} {stats[name]["spread_ms"]:20.3f}')
    spread = max(s['spread_ms'] for s in stats.values())
    gain = stats['host']['mean_ms'] - stats['device']['mean_ms']
    print(f'host - device = {gain:.3f} ms/batch (largest spread of an arm: {spread:.3f} ms); device - floor = '
          f'{stats["device"]["mean_ms"] - stats["floor"]["mean_ms"]:.3f} ms/batch; metric launches alone (device events): {metric_us:.1f} us/batch')
    print(f'{"":8s} {"psnr [dB]":>20s} {"ssim":>20s} {"mae":>20s}  counted')
    for name in ('host', 'device', 'host_f64'):
        r = values[name]
        print(f'{name:8s} {r["psnr"]:20.12f} {r["ssim"]:20.15f} {r["mae"]:20.15f}  {r["batches_counted"]}/{r["batches"]}')
    h, d = values['host'], values['device']
    diffs = dict(psnr_db=abs(h['psnr'] - d['psnr']), ssim=abs(h['ssim'] - d['ssim']), mae_rel=abs(h['mae'] - d['mae']) / h['mae'])
    agree = diffs['psnr_db'] <= 1e-9 and diffs['ssim'] <= 1e-10 and diffs['mae_rel'] <= 2e-6 and h['batches_counted'] == d['batches_counted']
    print(f'differences: psnr {diffs["psnr_db"]:.3e} dB, ssim {diffs["ssim"]:.3e}, mae {diffs["mae_rel"]:.3e} relative -> '
          f'{"agree" if agree else "DISAGREE"} at 1e-9 dB / 1e-10 / 2e-6')
    f = values['host_f64']
    print(f'device against the host arm on float64 copies: psnr {abs(f["psnr"] - d["psnr"]):.3e} dB, ssim {abs(f["ssim"] - d["ssim"]):.3e}, '
          f'mae {abs(f["mae"] - d["mae"]) / f["mae"]:.3e} relative')
    print(json.dumps(dict(bench='validation', res=args.res, batch=args.batch, batches=len(timed), dtype=args.dtype, arms=stats, metric_launches_us_per_batch=metric_us,
                          host_minus_device_ms=gain, largest_spread_ms=spread, device_beats_host=gain > spread, values=values, differences=diffs, values_agree=agree)))
    return 0 if (agree and gain > spread) else 1


if __name__ == '__main__':
    sys.exit(main())
