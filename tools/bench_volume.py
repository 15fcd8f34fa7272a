"""Whole-volume inference on the full-width 256^2 generator: what one subject costs, host way against device way against device + shared encoder.

Three arms over the same synthetic (64, 256, 256) uint8 subject (afcm_amd/synthetic.py), alternated in one process after a warm-up of each and the
whole alternation repeated, at every ``--thickness`` (5 and 8, the shipped configurations):
  (a) host    volume.predict_volume(where='host'): SliceDataset items built in numpy, one upload per batch, the EMA forward,
              SlidingWindowPredictor.accumulate behind a device -> host copy per batch (the package's path before the device arm existed)
  (b) device  volume.predict_volume(where='device'): the subject uploaded once, afcm_slice_assemble + the EMA forward + afcm_halo_accumulate per
              batch, map / mask at the end; nothing is read back inside the loop
  (c) shared  (b) with share_encoder=True: the generator's encoder once per thick-slice group of a batch, its state handed to the decoder batch
              by afcm_group_expand
Wall time per volume is a host clock around the call, ended by a synchronise (the host arm has synchronised by its copies already; the device arms'
results stay on the device, as evaluate_volume consumes them).  The new launches alone are also timed with device events.  The volumes are compared
bit for bit.  A gain of (c) over (b) is claimed only where the difference of the means exceeds the larger spread of the two arms.  Exit status 0:
the host and device volumes are equal and (b) beats (a) by more than the largest spread of the two, at every thickness.

    python tools/bench_volume.py [--depth 64] [--batch 16] [--repeats 3] [--dtype bf16] [--thickness 5 8] [--out FILE]
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
    ap.add_argument('--thickness', type=int, nargs='+', default=[5, 8])
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp16', 'fp32'])
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()

    import torch
    from afcm_amd import layer_schedule as sched, synthetic
    from afcm_amd.networks_stylegan3 import Stylegan3Generator
    from afcm_amd.stylegan3_model import StyleGAN3GeneratorStep
    from afcm_amd.torch_utils.ops.group_ops import GroupExpand
    from afcm_amd.torch_utils.ops.volume_ops import assemble_slices, halo_accumulate
    from afcm_amd.volume import GroupTables, PatchPlan, predict_volume
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
    lines = []

    def say(text):
        print(text)
        lines.append(text)

    def timed(fn, warm=3, reps=20):
        """us per call by device events."""
        for _ in range(warm):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    shape = (args.depth, args.res, args.res)
    plan = PatchPlan(shape, patch_indices(shape, (1, args.res, args.res), (1, 1, 1)))
    batches = -(-args.depth // args.batch)
    results, ok = [], True
    for thickness in args.thickness:
        kw = dict(raw_internal_path_in='raw', thickness=thickness, patch_hw=(args.res, args.res), batch_size=args.batch, patch_halo=(0, 8, 8))
        modes = {'host': dict(where='host'), 'device': dict(where='device'), 'shared': dict(where='device', share_encoder=True)}

        def clock(name):
            torch.manual_seed(1)                                               # set_test_input draws gen_z: the same draws for every arm
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = predict_volume(step, {'raw': subject}, **modes[name], **kw)['prediction']
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out

        arms, volumes = {name: [] for name in modes}, {}
        for name in arms:                                                      # warm-up: allocator pools, workspace caches, the first launches
            clock(name)
        for rep in range(args.repeats):
            for name in arms:
                ms, volumes[name] = clock(name)
                arms[name].append(ms)
        equal = torch.equal(volumes['device'].cpu(), volumes['host'])
        shared_equal = torch.equal(volumes['shared'], volumes['device'])
        shared_diff = float((volumes['shared'] - volumes['device']).abs().max())

        # the new launches alone, by device events, on the shapes of one batch
        volume = torch.from_numpy(subject).to(dev)
        pmap, mask = torch.zeros((1,) + shape, device=dev), torch.zeros((1,) + shape, dtype=torch.uint8, device=dev)
        count = min(args.batch, args.depth)
        fake = step.fake_B[:count] if step.fake_B.shape[0] >= count else torch.zeros(count, 1, args.res, args.res, device=dev)
        events = {'slice_assemble': timed(lambda: assemble_slices(volume, 0, count, (1, args.res, args.res), thickness=thickness)),
                  'halo_accumulate': timed(lambda: halo_accumulate(pmap, mask, fake, plan.table(dev), 0, (0, 8, 8), box=plan.bounding_box(0, count)))}
        tables = GroupTables(plan, args.batch, thickness, dev)
        groups, leaders = tables.batch(0)
        a, _ = assemble_slices(volume, 0, count, (1, args.res, args.res), thickness=thickness)
        S = step.netG_ema.synthesis
        with torch.no_grad():
            state = S.encode(a.index_select(0, leaders))
            skips = [state.E_features[layer.out_size[0]] for layer, skip in zip([getattr(S, n) for n in S.layer_names], S._skip_plan()) if skip]
            expand = GroupExpand([state.x, state.img_global] + skips, count)
            events['group_expand'] = timed(lambda: expand.run(groups))
            events['encode_G'] = timed(lambda: S.encode(a.index_select(0, leaders)), reps=5)
            events['encode_B'] = timed(lambda: S.encode(a), reps=5)
        rows = expand.host.view(-1, 5).tolist()                                # (dst, src, block bytes, chunk0, G | kind << 32) per tensor
        written_mb = sum(r[2] * count for r in rows) / 1e6
        source_mb = sum(r[2] * (r[4] & 0xFFFFFFFF) for r in rows) / 1e6        # read G / B of what is written; the repeats come from the caches

        say(f'volume prediction, {args.res}^2 full-width generator ({args.dtype} training dtype, EMA copy in {step.netG_ema.synthesis.compute_dtype}), one '
            f'({args.depth}, {args.res}, {args.res}) uint8 subject, thickness {thickness}, batch {args.batch} ({batches} batches), {args.repeats} repeats of the '
            f'alternation after one warm-up of each arm; fake_B is {step.fake_B.dtype}; encoder batch sizes of the shared arm: {tables.encoder_batches}')
        say(f'{"arm":8s} {"ms/volume per repeat":36s} {"mean":>9s} {"ms/batch":>9s} {"spread (max - min)":>20s}')
        stats = {}
        for name, v in arms.items():
            stats[name] = dict(per_repeat_ms=v, mean_ms=sum(v) / len(v), spread_ms=max(v) - min(v))
            say(f'{name:8s} {"  ".join(f"{x:10.3f}" for x in v):36s} {stats[name]["mean_ms"]:9.3f} {stats[name]["mean_ms"] / batches:9.3f} {stats[name]["spread_ms"]:20.3f}')
        spread = max(stats['host']['spread_ms'], stats['device']['spread_ms'])
        gain = stats['host']['mean_ms'] - stats['device']['mean_ms']
        shared_spread = max(stats['device']['spread_ms'], stats['shared']['spread_ms'])
        shared_gain = stats['device']['mean_ms'] - stats['shared']['mean_ms']
        say(f'host - device = {gain:.3f} ms/volume (larger spread of the two: {spread:.3f} ms), {stats["host"]["mean_ms"] / stats["device"]["mean_ms"]:.2f}x')
        say(f'device - shared = {shared_gain:.3f} ms/volume = {shared_gain / batches:.3f} ms/batch (larger spread of the two: {shared_spread:.3f} ms), '
            f'{stats["device"]["mean_ms"] / stats["shared"]["mean_ms"]:.2f}x: ' + ('a gain' if shared_gain > shared_spread else 'no gain shown'))
        say(f'launches alone (device events, first batch of {count}, G = {len(leaders)}): slice_assemble {events["slice_assemble"]:.1f} us, halo_accumulate '
            f'{events["halo_accumulate"]:.1f} us, group_expand {events["group_expand"]:.1f} us for {len(rows)} tensors, {written_mb:.1f} MB written from '
            f'{source_mb:.1f} MB of sources ({written_mb / 1e6 / (events["group_expand"] * 1e-6):.2f} TB/s of stores); the encoder half alone on G = {len(leaders)} rows {events["encode_G"]:.0f} us, on '
            f'{count} rows {events["encode_B"]:.0f} us')
        say(f'host and device volumes are {"bit-identical" if equal else "DIFFERENT"}; shared and device volumes are '
            f'{"bit-identical" if shared_equal else f"DIFFERENT (max abs {shared_diff:.3e})"}')
        say('')
        results.append(dict(bench='volume_predict', res=args.res, depth=args.depth, batch=args.batch, thickness=thickness, dtype=args.dtype, arms=stats,
                            launches_us=events, group_expand_written_mb=written_mb, group_expand_source_mb=source_mb, encoder_batches=tables.encoder_batches, host_minus_device_ms=gain,
                            largest_spread_ms=spread, device_beats_host=gain > spread, volumes_equal=equal, device_minus_shared_ms=shared_gain,
                            shared_spread_ms=shared_spread, shared_beats_device=shared_gain > shared_spread, shared_volume_equal=shared_equal,
                            shared_volume_max_abs_diff=shared_diff))
        ok = ok and equal and gain > spread
    for r in results:
        print(json.dumps(r))
        lines.append(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
