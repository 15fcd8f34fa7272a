"""What the device-side schedule costs: the blur with sigma on the device against the tap construction + filter2d it replaces, the one-launch EMA
against the multi-tensor lerp + a copy per buffer, and the scheduled TrainingGraph against the unscheduled one with the EMA between replays.  Each
subcommand is its own process (run each under its own time limit; chain them with && from a script):

    python tools/bench_schedule.py blur [--repeats 5]
    python tools/bench_schedule.py ema  [--repeats 5]
    python tools/bench_schedule.py step [--repeats 5] [--steps 10]

The project's method: device events around a run of launches (host time: a host clock around the same calls, not synchronised), the arms interleaved
in one process after a warm-up of each, the alternation repeated, every repeat printed with the spread.  No timing here is gated by a test; the
numbers go to DESIGN section 8j."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return max(v) - min(v)


def timed(fn, launches):
    """(device us, host us) per call of fn over `launches` calls: events on the stream, a host clock around the enqueueing."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    host = (time.perf_counter() - t0) * 1e6 / launches
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches, host


def alternate(arms, repeats, launches):
    """{name: fn} -> {name: {device_us, host_us: per repeat, mean, spread}}; a warm-up pass of every arm first."""
    for fn in arms.values():
        timed(fn, max(2, launches // 4))
    out = {name: dict(device_us=[], host_us=[]) for name in arms}
    for _ in range(repeats):
        for name, fn in arms.items():
            d, h = timed(fn, launches)
            out[name]['device_us'].append(d), out[name]['host_us'].append(h)
    for name, s in out.items():
        for k in ('device_us', 'host_us'):
            s[k + '_mean'], s[k + '_spread'] = sum(s[k]) / len(s[k]), spread(s[k])
        print(f'  {name:22s} device us {"  ".join(f"{x:8.1f}" for x in s["device_us"])}  mean {s["device_us_mean"]:8.1f} spread {s["device_us_spread"]:6.1f}'
              f'   host us mean {s["host_us_mean"]:8.1f} spread {s["host_us_spread"]:6.1f}')
    return out


def verdict(new, old, key='device_us'):
    diff, box = new[key + '_mean'] - old[key + '_mean'], max(new[key + '_spread'], old[key + '_spread'])
    return f'{diff:+.1f} us ({key[:-3]}), largest spread {box:.1f}: ' + ('no difference' if abs(diff) <= box else ('faster' if diff < 0 else 'SLOWER'))


def blur(args):
    import numpy as np
    import torch
    from afcm_amd.torch_utils.ops import upfirdn2d
    from afcm_amd.torch_utils.ops.gauss_blur import gauss_blur

    def parent_blur(img, sigma):                                                # StyleGAN3GeneratorStep._blur without a schedule, call for call
        blur_size = np.floor(sigma * 3)
        if blur_size <= 0:
            return img
        f = torch.arange(-blur_size, blur_size + 1, device=img.device).div(sigma).square().neg().exp2()
        return upfirdn2d.filter2d(img, f / f.sum())

    results = {}
    for shape in ((16, 5, 256, 256), (16, 1, 256, 256)):
        x = torch.randn(shape, device='cuda')
        g = torch.randn(shape, device='cuda')
        for sigma in (10.0, 2.0, 0.0):
            print(f'blur {shape} sigma {sigma}: {x.numel() * 4 / 1e6:.1f} MB per pass over the tensor')
            xg = x.clone().requires_grad_(True)

            def both(op):
                torch.autograd.grad(op(xg, sigma), xg, g)

            arms = {'new forward': lambda: gauss_blur(x, sigma=sigma), 'parent forward': lambda: parent_blur(x, sigma),
                    'new fwd+bwd': lambda: both(lambda t, s: gauss_blur(t, sigma=s)), 'parent fwd+bwd': lambda: both(lambda t, s: parent_blur(t, s))}
            if sigma == 0.0:                                                    # the parent returns its input: nothing to launch, nothing to differentiate
                arms = {'new forward': arms['new forward'], 'new fwd+bwd': arms['new fwd+bwd']}
            stats = alternate(arms, args.repeats, args.launches)
            if sigma > 0:
                print('  forward: new - parent', verdict(stats['new forward'], stats['parent forward']))
                print('  fwd+bwd: new - parent', verdict(stats['new fwd+bwd'], stats['parent fwd+bwd']))
            results[f'{shape} sigma {sigma}'] = stats
    print(json.dumps(dict(bench='schedule_blur', results=results)))
    return 0


def full_generator(dev, res=256):
    import torch
    from afcm_amd import layer_schedule as sched
    from afcm_amd.networks_stylegan3 import Stylegan3Generator
    torch.manual_seed(0)
    return Stylegan3Generator(z_dim=512, c_dim=1, w_dim=512, img_resolution=res, img_channels_in=4, img_channels_out=1, mapping_kwargs=dict(num_layers=8),
                              synthesis_kwargs=dict(dict(sched.DEFAULT_SYNTHESIS_KWARGS), compute_dtype=torch.bfloat16)).to(dev)


def ema(args):
    import copy
    import torch
    from afcm_amd.stylegan3_model import update_ema
    from afcm_amd.torch_utils.ops.ema_ops import EmaTable
    dev = torch.device('cuda:0')
    G = full_generator(dev)
    G_ema = copy.deepcopy(G).eval()
    with torch.no_grad():
        for p in G.parameters():
            p.add_(torch.randn_like(p) * 0.01)
    table = EmaTable(G_ema, G)
    n_par, n_buf = len(list(G.parameters())), len(list(G.buffers()))
    mb = sum(p.numel() for p in G.parameters()) * 4 / 1e6
    print(f'ema: {n_par} parameters ({mb:.1f} MB) + {n_buf} buffers; floor: read p, read and write p_ema = {3 * mb:.1f} MB')
    stats = alternate({'new (one launch)': lambda: table.update(beta=0.9989), 'parent update_ema': lambda: update_ema(G_ema, G, 16, 10 ** 6, 10.0, 0.05)},
                      args.repeats, args.launches)
    new = stats['new (one launch)']
    print(f'  achieved {3 * mb / new["device_us_mean"]:.3f} TB/s')
    print('  device: new - parent', verdict(new, stats['parent update_ema']))
    print('  host:   new - parent', verdict(new, stats['parent update_ema'], 'host_us'))
    print(json.dumps(dict(bench='schedule_ema', parameters=n_par, buffers=n_buf, megabytes=mb, arms=stats)))
    return 0


def step(args):
    import torch
    from afcm_amd.networks_discriminator import CoModDiscriminator
    from afcm_amd.schedule import DeviceSchedule
    from afcm_amd.stylegan3_model import StyleGAN3Step
    from afcm_amd.training import TrainingGraph
    from bench_train_feed import synthetic_set
    dev = torch.device('cuda:0')
    def make_set():                                                             # one per arm: a set carries the cursor its graph reads
        ds = synthetic_set(args.subjects, args.depth, 256, dev)
        items = ds.epoch_items(0)
        ds.load_epoch(items[:len(items) // args.batch * args.batch])
        return ds

    def make(schedule):
        G = full_generator(dev)
        D = CoModDiscriminator(c_dim=0, img_resolution=256, img_channels=5, channel_base=int(0.5 * 32768), channel_max=512, num_fp16_res=4, conv_clamp=256,
                               block_kwargs=dict(fp16_dtype=torch.bfloat16), epilogue_kwargs=dict(mbstd_group_size=16)).to(dev)
        return StyleGAN3Step(G, D, lr_G=0.0025, lr_D=0.0025, capturable=True, ema=True, schedule=schedule, blur_init_sigma=10.0, blur_fade_kimg=100.0)

    # the scheduled arm: sigma fading from 10, EMA inside the graph.  The unscheduled arm is what a replayed run was before: sigma frozen at capture
    # (10: the same 61 taps) and update_ema on the host between replays
    sched_step = make(DeviceSchedule(dev, blur_init_sigma=10.0, blur_fade_kimg=100.0, ema_kimgs=10.0, ramp=0.05, lr_G=0.0025))
    scheduled = TrainingGraph(sched_step, make_set(), args.batch, warmup=3)
    plain_step = make(None)
    plain_step.blur_sigma = 10.0
    plain = TrainingGraph(plain_step, make_set(), args.batch, warmup=3)
    seen = [0]

    def replay_scheduled():
        if scheduled.dataset.position + args.batch > scheduled.dataset.rows:
            scheduled.rewind()
        scheduled.replay()

    def replay_plain():
        if plain.dataset.position + args.batch > plain.dataset.rows:
            plain.rewind()
        plain.replay()
        seen[0] += args.batch
        plain_step.update_ema(args.batch, seen[0], 10.0, 0.05)

    print(f'full StyleGAN3Step at 256^2, batch {args.batch}, bf16, EMA on: scheduled TrainingGraph (blur fading, EMA inside) against the unscheduled one + '
          f'host update_ema between replays; {args.steps} iterations per pass')
    stats = alternate({'scheduled': replay_scheduled, 'unscheduled + host ema': replay_plain}, args.repeats, args.steps)
    for name, s in stats.items():
        print(f'  {name}: {s["device_us_mean"] / 1e3:.3f} ms per iteration (spread {s["device_us_spread"] / 1e3:.3f}), host {s["host_us_mean"] / 1e3:.3f} ms '
              f'(spread {s["host_us_spread"] / 1e3:.3f})')
    print(json.dumps(dict(bench='schedule_step', batch=args.batch, arms=stats)))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['blur', 'ema', 'step'])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--subjects', type=int, default=4)
    ap.add_argument('--depth', type=int, default=64)
    ap.add_argument('--batch', type=int, default=16)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_schedule.py needs a GPU: a time taken without one says nothing')
    return {'blur': blur, 'ema': ema, 'step': step}[args.what](args)


if __name__ == '__main__':
    sys.exit(main())
