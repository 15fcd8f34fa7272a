"""The CoModGAN generator at full width (256^2, channel_base 16384, channel_max 512, batch 16, fp32), forward + backward, with the fused and the
unfused arm of networks_comodgan.IMPL; and the epilogue kernel on its own at the up-2 layers' shapes:

    python tools/bench_comod.py generator [--repeats 5] [--steps 5] [--batch 16]
    python tools/bench_comod.py epilogue  [--repeats 5] [--launches 20] [--batch 16]

Each subcommand is its own process (run each under its own time limit).  The method is tools/bench_schedule.py's: device events around a run of
launches, the arms interleaved in one process after a warm-up of each, the alternation repeated, every repeat printed with the spread.  No time is
asserted anywhere; the numbers go to profiles/comodgan_arms.txt and DESIGN section 8."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_schedule import alternate, verdict  # noqa: E402


def generator(args):
    import torch
    from afcm_amd import networks_comodgan as nc
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    G = nc.CoModGenerator(z_dim=512, c_dim=0, w_dim=512, img_resolution=256, img_channels_in=4, img_channels_out=1,
                          synthesis_kwargs=dict(channel_base=16384, channel_max=512, cond_mod=True, skip_resolution=256, conv_clamp=256)).to(dev).train()
    params = list(G.parameters())
    z, x = torch.randn(args.batch, 512, device=dev), torch.randn(args.batch, 4, 256, 256, device=dev)
    r = torch.randn(args.batch, 1, 256, 256, device=dev)
    print(f'CoModGenerator 256^2, batch {args.batch}, fp32, {sum(p.numel() for p in params) / 1e6:.1f} M parameters: forward + backward of (y * r).sum(), '
          f'noise_mode random, {args.steps} iterations per pass')

    def arm(impl):
        def one():
            nc.IMPL = impl
            y = G(z, None, x, noise_mode='random')
            torch.autograd.grad((y * r).sum(), params)
        return one

    res = alternate({'fused': arm('fused'), 'unfused': arm('unfused')}, args.repeats, args.steps)
    for name, s in res.items():
        print(f'  {name}: {s["device_us_mean"] / 1e3:.2f} ms per iteration (spread {s["device_us_spread"] / 1e3:.2f})')
    print('  fused - unfused:', verdict(res['fused'], res['unfused']))
    print(json.dumps(dict(bench='comod_generator', batch=args.batch, arms=res)))
    return 0


def epilogue(args):
    import torch
    from afcm_amd.torch_utils.ops import bias_act
    from afcm_amd.torch_utils.ops.modconv_epilogue import modconv_epilogue
    dev = torch.device('cuda:0')
    results = {}
    for up, o, h in ((2, 64, 128), (2, 128, 64), (2, 256, 32), (1, 64, 256)):
        n = args.batch
        t = torch.randn(n, up * up * o, h, h, device=dev).requires_grad_(True)
        d, b = (torch.rand(n, o, device=dev) + 0.5).requires_grad_(True), torch.randn(o, device=dev).requires_grad_(True)
        nz, s = torch.randn(n, 1, up * h, up * h, device=dev), torch.tensor(0.1, device=dev).requires_grad_(True)
        dy = torch.randn(n, o, up * h, up * h, device=dev)
        mb = t.numel() * 4 / 1e6
        y = modconv_epilogue(t, d, b, nz, s, up=up, gain=2 ** 0.5, clamp=256)

        def fwd():
            modconv_epilogue(t.detach(), d.detach(), b.detach(), nz, s.detach(), up=up, gain=2 ** 0.5, clamp=256)

        def bwd():
            torch.autograd.grad(y, [t, d, b, s], dy, retain_graph=True)

        def parts():                                                            # the unfused arm's passes over a full-resolution tensor
            full = t.detach().reshape(n, o, up * h, up * h)
            bias_act.bias_act(torch.addcmul(nz * s.detach(), full, d.detach()[:, :, None, None]), b.detach(), act='lrelu', gain=2 ** 0.5, clamp=256)

        print(f'epilogue up {up}, {n} x {o} planes of {up * h}^2: {mb:.1f} MB in t, as much in y')
        res = alternate({'forward': fwd, 'backward': bwd, 'addcmul + bias_act': parts}, args.repeats, args.launches)
        f, bw = res['forward']['device_us_mean'], res['backward']['device_us_mean']
        print(f'  forward {2 * mb / f:.3f} TB/s (reads t, writes y; + the noise plane), backward {4 * mb / bw:.3f} TB/s (reads dy, y, t, writes d_t; + noise)')
        results[f'up{up}_o{o}_h{h}'] = res
    print(json.dumps(dict(bench='comod_epilogue', batch=args.batch, results=results)))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['generator', 'epilogue'])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--batch', type=int, default=16)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_comod.py needs a GPU: a time taken without one says nothing')
    return {'generator': generator, 'epilogue': epilogue}[args.what](args)


if __name__ == '__main__':
    sys.exit(main())
