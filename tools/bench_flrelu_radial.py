#!/usr/bin/env python3
"""Radial (StyleGAN3-R) filtered_lrelu: fused kernels against the generic composition, in one process (GPU).

Per radial layer of the full-width 256^2 generator at batch B: the forward (sign write, the SUFD kernel) and the transposed backward
(sign read, the FUSD kernel), each timed against filtered_lrelu._run_generic (upfirdn2d up -> activation -> upfirdn2d down) on the
same operands, the two interleaved repeat by repeat.  Reported: us per call (best repeat), algorithmic GB/s (read x, write y, 2 bits
per element of the sign grid) and the fraction of the FP32-vector bound (157.3 TFLOP/s) of the FIR FLOPs counted below.  --rotate K
cycles through K copies of the operands (cold caches).  --step adds the generator training step, radial against the default filters.

  FLOPs (2 per FMA, no tile halo): separable up-FIR  Hin Wup FUT + Hup Wup FUT;  2-D down  Hout Wout FD^2;
                                   2-D up-FIR  Hup Wup FUT^2;  separable down  Hup Wout FD + Hout Wout FD
  (Hup x Wup: the activated grid the outputs need, (out - 1) down + FD; FUT = taps per polyphase branch)
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from afcm_amd import layer_schedule as sched  # noqa: E402
from afcm_amd.torch_utils.ops import filtered_lrelu as flr  # noqa: E402

PEAK_FP32 = 157.3e12


def fir_flops(up, down, fu, fd, hin, hout):
    """FLOPs of one plane of the fused op (square planes)."""
    fut = fu.shape[-1] // up
    fdt = fd.shape[-1]
    hup = (hout - 1) * down + fdt
    f = 0
    if fu.ndim == 1:
        f += hin * hup * fut + hup * hup * fut
    else:
        f += hup * hup * fut * fut
    if fd.ndim == 1:
        f += hup * hout * fdt + hout * hout * fdt
    else:
        f += hout * hout * fdt * fdt
    return 2 * f


def time_pair(fa, fb, iters, repeats):
    """Interleaved best-of-`repeats` timing (us per call) of two launch sequences."""
    best = [float('inf'), float('inf')]
    for fn in (fa, fb):
        fn(0)
    torch.cuda.synchronize()
    for _ in range(repeats):
        for j, fn in enumerate((fa, fb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(iters):
                fn(i)
            e1.record()
            e1.synchronize()
            best[j] = min(best[j], e0.elapsed_time(e1) * 1e3 / iters)
    return best


def layers(args, dtype):
    pl = sched.plan(256, 4, 1, {'use_radial_filters': True})
    kw = pl['kw']
    rows = []
    for L in pl['enc'] + pl['dec']:
        if L['fd'] is None or L['fd'].ndim != 2 or (args.layers and L['name'] not in args.layers.split(',')):
            continue
        h = L['in_size'] + L['k'] - 1
        x = torch.randn(args.batch, L['cout'], h, h, device='cuda', dtype=dtype)
        fu, fd = L['fu'].cuda(), L['fd'].cuda()
        cfg = (L['up'], L['down'], *L['padding'], 2 ** 0.5, 0.2, float(kw['conv_clamp']), False, 0, 0, 0)
        y, s, layout, _ = flr._run(x, fu, fd, None, None, cfg, True, no_fallback=True)
        bcfg = flr._backward_cfg(cfg, fu, fd, x.shape, y.shape, layout)
        g = torch.randn_like(y)
        K = max(1, args.rotate)
        xs = [x] + [x.clone() for _ in range(K - 1)]
        gs = [g] + [g.clone() for _ in range(K - 1)]
        ss = [s] + [s.clone() for _ in range(K - 1)]
        keep = [None] * K

        def fwd_fused(i):
            keep[i % K] = flr._run(xs[i % K], fu, fd, None, None, cfg, True, no_fallback=True)

        def fwd_generic(i):
            keep[i % K] = flr._run_generic(xs[i % K], fu, fd, None, None, cfg, True)

        def bwd_fused(i):
            keep[i % K] = flr._run(gs[i % K], fd, fu, None, ss[i % K], bcfg, False, no_fallback=True)

        def bwd_generic(i):
            keep[i % K] = flr._run_generic(gs[i % K], fd, fu, None, ss[i % K], bcfg, False)

        tf = time_pair(fwd_fused, fwd_generic, args.iters, args.repeats)
        tb = time_pair(bwd_fused, bwd_generic, args.iters, args.repeats)
        planes = x.shape[0] * x.shape[1]
        es = x.element_size()
        nbytes = planes * (es * (x.shape[2] * x.shape[3] + y.shape[2] * y.shape[3])) + s.numel()
        flf = planes * fir_flops(L['up'], L['down'], L['fu'], L['fd'], h, y.shape[2])
        flb = planes * fir_flops(L['down'], L['up'], L['fd'], L['fu'], y.shape[2], h)
        row = dict(layer=L['name'], dtype=str(dtype).split('.')[-1], shape=list(x.shape), out=list(y.shape),
                   fwd_us=round(tf[0], 1), fwd_generic_us=round(tf[1], 1), bwd_us=round(tb[0], 1), bwd_generic_us=round(tb[1], 1),
                   fwd_GBps=round(nbytes / tf[0] / 1e3, 1), bwd_GBps=round(nbytes / tb[0] / 1e3, 1),
                   fwd_fp32_bound=round(flf / (tf[0] * 1e-6) / PEAK_FP32, 3), bwd_fp32_bound=round(flb / (tb[0] * 1e-6) / PEAK_FP32, 3))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del xs, gs, ss, keep, x, g, s, y
        torch.cuda.empty_cache()
    return rows


def step_time(dtype, radial, args):
    from afcm_amd import synthetic
    from afcm_amd.layer_schedule import DEFAULT_SYNTHESIS_KWARGS
    from afcm_amd.networks_stylegan3 import Stylegan3Generator
    from afcm_amd.stylegan3_model import StyleGAN3GeneratorStep
    torch.manual_seed(0)
    G = Stylegan3Generator(z_dim=512, c_dim=1, w_dim=512, img_resolution=256, img_channels_in=4, img_channels_out=1,
                           mapping_kwargs=dict(num_layers=8),
                           synthesis_kwargs=dict(DEFAULT_SYNTHESIS_KWARGS, use_radial_filters=radial, compute_dtype=dtype)).cuda()
    step = StyleGAN3GeneratorStep(G, lambda_L1=100.0)
    a, b, z, c = synthetic.generator_inputs(args.batch, size=256, seed=1, device='cuda')
    step.set_input(a, b, z, c)
    for _ in range(args.step_warmup):
        step.optimize_parameters()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.step_iters):
        step.optimize_parameters()
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1) / args.step_iters
    del step, G
    torch.cuda.empty_cache()
    return ms


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--rotate', type=int, default=1, help='cycle through this many copies of the operands (cold caches)')
    ap.add_argument('--dtypes', default='float32,bfloat16')
    ap.add_argument('--layers', default='', help='comma-separated layer names (default: every radial layer)')
    ap.add_argument('--no-layers', action='store_true')
    ap.add_argument('--radial-step-only', action='store_true', help='--step: time the radial configuration only (for a kernel trace)')
    ap.add_argument('--step', action='store_true', help='also time the 256^2 generator training step, radial against default')
    ap.add_argument('--step-iters', type=int, default=5)
    ap.add_argument('--step-warmup', type=int, default=2)
    args = ap.parse_args()
    dtypes = [getattr(torch, d) for d in args.dtypes.split(',')]
    print(json.dumps(dict(tool='bench_flrelu_radial', batch=args.batch, rotate=args.rotate, iters=args.iters, repeats=args.repeats,
                          device=torch.cuda.get_device_name())))
    if not args.no_layers:
        for dtype in dtypes:
            rows = layers(args, dtype)
            slower = [r['layer'] for r in rows if r['fwd_us'] >= r['fwd_generic_us'] or r['bwd_us'] >= r['bwd_generic_us']]
            tot = {k: round(sum(r[k] for r in rows), 1) for k in ('fwd_us', 'fwd_generic_us', 'bwd_us', 'bwd_generic_us')}
            print(json.dumps(dict(summary=str(dtype).split('.')[-1], fused_not_faster=slower, **tot)), flush=True)
    if args.step:
        for dtype in dtypes:
            if args.radial_step_only:
                print(json.dumps(dict(step=str(dtype).split('.')[-1], batch=args.batch, radial_ms=round(step_time(dtype, True, args), 2))))
                continue
            t_def = step_time(dtype, False, args)
            t_rad = step_time(dtype, True, args)
            print(json.dumps(dict(step=str(dtype).split('.')[-1], batch=args.batch, default_ms=round(t_def, 2), radial_ms=round(t_rad, 2),
                                  ratio=round(t_rad / t_def, 3))), flush=True)


if __name__ == '__main__':
    main()
