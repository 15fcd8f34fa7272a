"""What the device-side training log costs, on the full-width generator's table and on the full D + G training graph:

    python tools/bench_trainlog.py launch [--repeats 5] [--launches 20]     the statistics launch alone, the Adam launch alone, the pair as a step runs it
    python tools/bench_trainlog.py step   [--repeats 5] [--steps 10]        the replayed TrainingGraph with a log against the same graph without one

Each subcommand is its own process (run each under its own time limit; chain them with && from a script).  The method is tools/bench_schedule.py's:
device events around a run of launches, the arms interleaved in one process after a warm-up of each, the alternation repeated, every repeat printed
with the spread.  No timing here is gated by a test; the numbers go to profiles/trainlog_cost.txt and DESIGN section 8s."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_schedule import alternate, full_generator, verdict  # noqa: E402


def launch(args):
    import torch
    from afcm_amd import _lib
    from afcm_amd.optim import FusedScrubAdam
    dev = torch.device('cuda:0')
    G = full_generator(dev)
    params = list(G.parameters())
    for p in params:
        p.grad = torch.randn_like(p) * 1e-3
    opt = FusedScrubAdam(params, lr=1e-4, betas=(0.0, 0.99), stats=True)
    opt.step()                                                                   # builds the pointer table and the moments
    (rows, table, _), = opt._tables.values()
    partials, chunks = opt.grad_stats()
    lib, stream, vp = _lib.load(), _lib.stream_ptr(table), lambda t: ctypes.c_void_p(t.data_ptr())
    mb = sum(p.numel() for p in params) * 4 / 1e6
    print(f'launch: {len(rows)} tensors, {chunks} chunks of {lib.afcm_adam_chunk_elems()} elements, {mb:.1f} MB of gradients; the statistics launch reads '
          f'{mb:.1f} MB, the Adam launch (beta1 = 0: m is not read) moves {6 * mb:.1f} MB')

    def stats():
        _lib.launched(lib.afcm_grad_stats(vp(table), len(rows), chunks, 1.0, vp(partials), stream), 'grad_stats')

    def adam():
        _lib.launched(lib.afcm_adam_multi(vp(table), len(rows), chunks, 1e-4, 0.0, 0.99, 1.0, 1.0 - 0.99, 0.5, 1e-8, 1.0, 1, 1e5, -1e5, 0, stream), 'adam_multi')

    def pair():
        stats(), adam()

    res = alternate({'stats alone': stats, 'adam alone': adam, 'stats + adam': pair}, args.repeats, args.launches)
    s, a, both = res['stats alone']['device_us_mean'], res['adam alone']['device_us_mean'], res['stats + adam']['device_us_mean']
    print(f'  stats alone / adam alone = {s / a:.3f} (asked: at or below 0.25); stats alone {mb / s:.3f} TB/s, adam alone {6 * mb / a:.3f} TB/s')
    print(f'  in front of the Adam launch the statistics add {both - a:.1f} us ({(both - a) / a * 100:.1f} % of the Adam launch)')
    print('  (back-to-back statistics launches re-read gradients the last-level cache may still hold; the pair is the order a step runs them in)')
    print(json.dumps(dict(bench='trainlog_launch', tensors=len(rows), chunks=chunks, megabytes=mb, arms=res)))
    return 0


def step(args):
    import torch
    from afcm_amd.networks_discriminator import CoModDiscriminator
    from afcm_amd.schedule import DeviceSchedule
    from afcm_amd.stylegan3_model import StyleGAN3Step
    from afcm_amd.trainlog import DeviceTrainLog
    from afcm_amd.training import TrainingGraph
    from bench_train_feed import synthetic_set
    dev = torch.device('cuda:0')

    def make_set():                                                              # one per arm: a set carries the cursor its graph reads
        ds = synthetic_set(args.subjects, args.depth, 256, dev)
        items = ds.epoch_items(0)
        ds.load_epoch(items[:len(items) // args.batch * args.batch])
        return ds

    def make(log):
        G = full_generator(dev)
        D = CoModDiscriminator(c_dim=0, img_resolution=256, img_channels=5, channel_base=int(0.5 * 32768), channel_max=512, num_fp16_res=4, conv_clamp=256,
                               block_kwargs=dict(fp16_dtype=torch.bfloat16), epilogue_kwargs=dict(mbstd_group_size=16)).to(dev)
        schedule = DeviceSchedule(dev, blur_init_sigma=10.0, blur_fade_kimg=100.0, lr_G=0.0025)
        return StyleGAN3Step(G, D, lr_G=0.0025, lr_D=0.0025, capturable=True, schedule=schedule, blur_init_sigma=10.0, blur_fade_kimg=100.0, log=log)

    logged = TrainingGraph(make(DeviceTrainLog(4096, dev)), make_set(), args.batch, warmup=3)
    plain = TrainingGraph(make(None), make_set(), args.batch, warmup=3)

    def replay(graph):
        def one():
            if graph.dataset.position + args.batch > graph.dataset.rows:
                graph.rewind()
            graph.replay()
        return one

    print(f'full StyleGAN3Step at 256^2, batch {args.batch}, bf16, scheduled: the replayed TrainingGraph with a log (two statistics launches, one gather, one '
          f'append per iteration) against the same graph without one; {args.steps} iterations per pass')
    res = alternate({'with a log': replay(logged), 'without (the parent)': replay(plain)}, args.repeats, args.steps)
    for name, s in res.items():
        print(f'  {name}: {s["device_us_mean"] / 1e3:.3f} ms per iteration (spread {s["device_us_spread"] / 1e3:.3f}), host {s["host_us_mean"] / 1e3:.3f} ms '
              f'(spread {s["host_us_spread"] / 1e3:.3f})')
    print('  with - without:', verdict(res['with a log'], res['without (the parent)']))
    rows, lost = logged.step.log.read()
    print(f'  the log after the run: {len(rows)} rows, {lost} lost, last row G_L1 {rows[-1][12]:.4f}, G sumsq {rows[-1][16]:.4e}, G scrubbed {rows[-1][17:20].tolist()}, '
          f'D sumsq {rows[-1][20]:.4e}, D scrubbed {rows[-1][21:24].tolist()}')
    print(json.dumps(dict(bench='trainlog_step', batch=args.batch, arms=res)))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['launch', 'step'])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--subjects', type=int, default=4)
    ap.add_argument('--depth', type=int, default=64)
    ap.add_argument('--batch', type=int, default=16)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_trainlog.py needs a GPU: a time taken without one says nothing')
    return {'launch': launch, 'step': step}[args.what](args)


if __name__ == '__main__':
    sys.exit(main())
