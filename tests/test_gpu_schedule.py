"""The device-side schedule on the GPU: ``afcm_schedule_advance`` against ``DeviceSchedule.host_values``; ``gauss_blur`` against the float64
restatement (tests/schedule_ref.py) and the golden captured from the reference; ``afcm_ema_multi`` against float64 under a derived bound;
``afcm_adam_multi_capturable_lr`` against ``_d``; the scheduled training step, ``TrainingGraph`` and ``train_epochs`` on tiny networks."""
import numpy as np
import pytest
import torch

import schedule_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

# The kernels' tiles (csrc/blur.hip): the row pass owns 4 rows x 256 columns per workgroup, the column pass 64 rows x 64 columns.
ROWS_TW, COLS_TH = 256, 64
BAR = 2e-5                                                                      # the project's fp32 kernel bar, DESIGN section 2: x max|y_ref|


def _schedule(**kw):
    from afcm_amd.schedule import DeviceSchedule
    kw.setdefault('lr_G', 0.0002)
    return DeviceSchedule('cuda', **kw)


# ---- 1. the schedule kernel ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('ramp', [None, 0.05])
def test_advance_equals_host_values(ramp):
    from afcm_amd.schedule import DeviceSchedule
    kw = dict(blur_init_sigma=10.0, blur_fade_kimg=100.0, ema_kimgs=10.0, ramp=ramp)
    for total in R.TOTAL_ITERS:
        s = _schedule(total_iters=total - 16, lr_G=0.0002, lr_D=0.0001, **kw)
        s.block[6:] = torch.tensor([3.5, -2.25], dtype=torch.float64)           # spare slots: advance must not touch them
        s.advance(16)
        got = s.block.cpu().numpy()
        want = DeviceSchedule.host_values(total, 16, **kw)
        for slot, key in enumerate(('total_iters', 'blur_sigma', 'blur_radius')):
            assert R.bits(got[slot]) == R.bits(want[key]), (total, key, got[slot], want[key])
        assert R.rel(got[3], want['ema_beta']) <= 1e-15, (total, got[3], want['ema_beta'])
        assert got[4:].tolist() == [0.0002, 0.0001, 3.5, -2.25]
        assert s.read() == dict(total_iters=float(total), blur_sigma=want['blur_sigma'], blur_radius=want['blur_radius'], ema_beta=got[3], lr_G=0.0002,
                                lr_D=0.0001)
    off = _schedule(blur_init_sigma=10.0, blur_fade_kimg=0.0)
    off.advance(16)
    assert off.block.cpu().tolist()[:4] == [16.0, 0.0, 0.0, 0.0]                # no fade: no blur; no ema_kimgs: beta 0.5 ** (16 / 1e-8) = 0
    with pytest.raises(ValueError, match='radius'):
        _schedule(blur_init_sigma=(_rmax() + 1) / 3.0, blur_fade_kimg=1.0)
    with pytest.raises(RuntimeError, match='below 1'):
        off.advance(0)


def _rmax():
    from afcm_amd.torch_utils.ops.gauss_blur import rmax
    return rmax()


def test_captured_advance_replays_like_eager_advances():
    kw = dict(blur_init_sigma=2.0, blur_fade_kimg=0.05, ema_kimgs=10.0, ramp=0.05, total_iters=7)
    eager, replayed = _schedule(**kw), _schedule(**kw)
    for _ in range(5):
        eager.advance(4)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode='thread_local'):
        replayed.advance(4)
    assert replayed.read()['total_iters'] == 7.0                                # a capture records, it does not run
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(eager.block, replayed.block) and eager.read()['total_iters'] == 27.0
    state = eager.state_dict()
    assert state == dict(total_iters=27.0, lr_G=0.0002, lr_D=0.0002)
    other = _schedule(**kw)
    other.load_state_dict(state)
    other.advance(4), eager.advance(4)
    assert torch.equal(other.block, eager.block)
    other.set_lr(0.0001)
    assert other.read()['lr_G'] == other.read()['lr_D'] == 0.0001 and other.read()['total_iters'] == 31.0      # lr_D defaults to lr_G
    other.set_lr(0.0003, 0.0004)
    assert (other.read()['lr_G'], other.read()['lr_D'], other.lr_G, other.lr_D) == (0.0003, 0.0004, 0.0003, 0.0004)


# ---- 2. the blur ------------------------------------------------------------------------------------------------------------------------------

_MEASURED = {}


def _blur_case(x, sigma):
    """gauss_blur(x, sigma) against the float64 restatement under the fp32 bar; returns the output."""
    from afcm_amd.torch_utils.ops.gauss_blur import gauss_blur
    y = gauss_blur(x.cuda(), sigma=sigma)
    assert y.dtype == torch.float32 and y.shape == x.shape
    want = R.blur_ref(x.numpy(), sigma)
    err = np.abs(y.cpu().numpy() - want).max() / np.abs(want).max()
    _MEASURED[(tuple(x.shape), sigma)] = err
    print(f'gauss_blur {tuple(x.shape)} sigma {sigma}: max error {err:.3e} of max|y_ref|')
    assert err <= BAR, (tuple(x.shape), sigma, err)
    return y


def test_blur_equals_the_reference_golden():
    from afcm_amd.torch_utils.ops.gauss_blur import gauss_blur
    g = load_golden('U3_gauss61_filter2d')
    x, y, r, dx = (torch.from_numpy(np.array(g[k])) for k in ('x', 'y', 'r', 'dx'))
    got = _blur_case(x, 10.0)
    assert (got.cpu() - y).abs().max() <= BAR * y.abs().max()
    xg = x.cuda().requires_grad_(True)
    got_dx, = torch.autograd.grad(gauss_blur(xg, sigma=10.0), xg, r.cuda())
    assert (got_dx.cpu() - dx).abs().max() <= BAR * dx.abs().max()
    assert np.abs(got_dx.cpu().numpy() - R.blur_ref(r.numpy(), 10.0)).max() <= BAR * np.abs(R.blur_ref(r.numpy(), 10.0)).max()


@pytest.mark.parametrize('shape, sigma', [
    ((1, 1, 16, 24), 10.0),                                                     # the radius exceeds both extents
    ((3, 5, 40, 40), 2.0),
    ((2, 1, COLS_TH - 1, ROWS_TW - 1), 2.0), ((2, 1, COLS_TH - 1, ROWS_TW - 1), 10.0),      # one short of the tile in both directions
    ((1, 2, COLS_TH + 1, ROWS_TW + 1), 2.0), ((1, 2, COLS_TH + 1, ROWS_TW + 1), 10.0),      # one past it: a second workgroup of one row / one column
    ((1, 2, 19, 23), 0.34),                                                     # radius 1: three taps, the tail group alone
    ((1, 1, 70, 90), 'cap'),                                                    # the largest radius the kernels are built for
])
def test_blur_against_float64(shape, sigma):
    if sigma == 'cap':
        sigma = (_rmax() + 0.5) / 3.0
        assert int(np.floor(3 * sigma)) == _rmax()
    x = torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape)))
    _blur_case(x, sigma)


def test_blur_radius_zero_is_a_copy_and_nan_stays_in_its_window():
    from afcm_amd.torch_utils.ops.gauss_blur import gauss_blur
    x = torch.randn(2, 3, 37, 70, generator=torch.Generator().manual_seed(1)).cuda()
    x[0, 1, 5, 6] = float('nan')
    x[1, 2, 0, 0] = float('inf')
    for sigma in (0.3, 0.0):
        y = gauss_blur(x, sigma=sigma)
        assert y.data_ptr() != x.data_ptr() and torch.equal(y.view(torch.int32), x.view(torch.int32))
    x = torch.randn(1, 2, 40, 45, generator=torch.Generator().manual_seed(2)).cuda()
    x[0, 1, 3, 41] = float('nan')                                               # the window is clipped by the top and the right edge
    y = gauss_blur(x, sigma=2.0)                                                # radius 6
    want = torch.zeros_like(x, dtype=torch.bool)
    want[0, 1, 0:10, 35:45] = True
    assert torch.equal(torch.isnan(y), want) and bool(torch.isfinite(y[~want]).all())
    with pytest.raises(RuntimeError, match='exceeds'):
        gauss_blur(x, sigma=(_rmax() + 1) / 3.0)


def test_blur_sigma_from_the_block():
    from afcm_amd.torch_utils.ops.gauss_blur import gauss_blur
    x = torch.randn(2, 2, 70, 300, generator=torch.Generator().manual_seed(3)).cuda()
    s = _schedule(blur_init_sigma=10.0, blur_fade_kimg=100.0, total_iters=49_984)
    for total in (50_000, 99_984, 93_344):                                     # sigma 5, 0.0016 (radius 0) and 0.6656 (radius 1, after a host write)
        if total != 50_000:
            s.load_state_dict(dict(total_iters=total - 16, lr_G=0.0002, lr_D=0.0002))
        s.advance(16)
        sigma = s.read()['blur_sigma']
        assert sigma == s.host_values(total, 16, 10.0, 100.0)['blur_sigma']
        assert torch.equal(gauss_blur(x, schedule=s), gauss_blur(x, sigma=sigma))
        assert torch.equal(gauss_blur(x, schedule=s.block), gauss_blur(x, sigma=sigma))
    for radius in (_rmax() + 1.0, -1.0, float('nan')):                          # the device cannot raise: every output is NaN
        block = torch.tensor([0.0, 20.0, radius, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64, device='cuda')
        assert bool(torch.isnan(gauss_blur(x, schedule=block)).all())
    half = gauss_blur(x.to(torch.bfloat16), sigma=2.0)                          # other dtypes: converted up and back
    assert half.dtype == torch.bfloat16 and torch.equal(half, gauss_blur(x.to(torch.bfloat16).float(), sigma=2.0).to(torch.bfloat16))


def test_blur_is_self_adjoint_and_twice_differentiable():
    from afcm_amd.torch_utils.ops.gauss_blur import gauss_blur
    gen = torch.Generator().manual_seed(4)
    x, g, s = (torch.randn(2, 3, 50, 61, generator=gen).cuda() for _ in range(3))
    for sigma in (2.0, 10.0):
        a = (gauss_blur(x, sigma=sigma).double() * g.double()).sum().item()
        b = (x.double() * gauss_blur(g, sigma=sigma).double()).sum().item()
        assert R.rel(a, b) <= 1e-5, (sigma, a, b)
    xg, rg = x.clone().requires_grad_(True), g.clone().requires_grad_(True)
    first, = torch.autograd.grad(gauss_blur(xg, sigma=2.0), xg, rg, create_graph=True)
    assert first.requires_grad and torch.equal(first.detach(), gauss_blur(g, sigma=2.0))
    second, = torch.autograd.grad(first, rg, s)                                 # the R1 term's path: through the backward of the blur
    assert torch.equal(second, gauss_blur(s, sigma=2.0))
    twice, = torch.autograd.grad(gauss_blur(gauss_blur(xg, sigma=2.0), sigma=2.0), xg, g)
    assert torch.equal(twice, gauss_blur(gauss_blur(g, sigma=2.0), sigma=2.0))


# ---- 3. the EMA launch ------------------------------------------------------------------------------------------------------------------

BETAS = (0.9989, 0.5, 0.25, 1e-6, 0.0, 1.0)
GUARD = 8


def _ema_case():
    """Lerp rows of 1, 3, 4, chunk - 1, chunk, chunk + 1 elements and one that starts an element into its buffer, copy rows of a 0-dim float32, an
    int64 buffer and 7 bytes; every row lies between guard bands inside a larger buffer."""
    from afcm_amd import _lib
    chunk = _lib.load().afcm_adam_chunk_elems()
    gen = torch.Generator().manual_seed(5)
    sizes = [1, 3, 4, chunk - 1, chunk, chunk + 1, 1000]
    offsets, at = [], GUARD
    for i, n in enumerate(sizes):
        at = (at + 3) // 4 * 4 + (1 if i == len(sizes) - 1 else 0)              # 16-byte aligned starts; the last row one element off
        offsets.append(at)
        at += n + GUARD
    total = at
    src = torch.randn(total, generator=gen).cuda()
    dst = torch.randn(total, generator=gen).cuda()
    dst[offsets[1]:offsets[1] + 3] = src[offsets[1]:offsets[1] + 3]             # a row with p_ema == p
    pairs = [(dst[o:o + n], src[o:o + n], _lib.EMA_LERP) for o, n in zip(offsets, sizes)]
    assert all(d.data_ptr() % 16 == 0 for d, _, _ in pairs[:-1]) and pairs[-1][0].data_ptr() % 16 == 4
    scalar_src, scalar_dst = torch.full([3], 1.5).cuda(), torch.zeros(3).cuda()
    long_src = torch.arange(-5, 6, dtype=torch.int64).cuda() * (1 << 40)
    long_dst = torch.zeros(11, dtype=torch.int64).cuda()
    byte_src = torch.arange(1, 24, dtype=torch.uint8).cuda()
    byte_dst = torch.zeros(23, dtype=torch.uint8).cuda()
    pairs += [(scalar_dst[1], scalar_src[1], _lib.EMA_COPY), (long_dst[2:9], long_src[2:9], _lib.EMA_COPY), (byte_dst[9:16], byte_src[9:16], _lib.EMA_COPY)]
    assert pairs[-3][0].dim() == 0
    return pairs, (src, dst), [(scalar_dst, scalar_src, 1, 2), (long_dst, long_src, 2, 9), (byte_dst, byte_src, 9, 16)]


@pytest.mark.parametrize('beta', BETAS)
def test_ema_rows_against_float64(beta):
    from afcm_amd.torch_utils.ops.ema_ops import EmaTable
    pairs, (src, dst), copies = _ema_case()
    src0, dst0 = src.clone(), dst.clone()
    table = EmaTable.from_pairs(pairs)
    table.update(beta=beta)
    assert torch.equal(src, src0)
    touched = torch.zeros_like(dst, dtype=torch.bool)
    worst = 0.0
    for d, s, _ in pairs[:7]:
        o, n = (d.data_ptr() - dst.data_ptr()) // 4, d.numel()
        touched[o:o + n] = True
        want, bound = R.lerp_ref(src0[o:o + n], dst0[o:o + n], beta)
        err = (d.double() - want).abs()
        assert bool((err <= bound).all()), (n, beta, (err / bound).max().item())
        worst = max(worst, (err / bound.clamp_min(1e-300)).max().item())
        if beta == 1.0:
            assert torch.equal(d, dst0[o:o + n])                                # beta 1 leaves p_ema
        if beta == 0.0:
            assert torch.equal(d, s)                                            # beta 0 gives p
    print(f'ema lerp beta {beta}: largest error {worst:.3f} of the bound 2^-21 max(|p|, |p_ema|)')
    assert torch.equal(pairs[1][0], pairs[1][1])                                # p_ema == p gives p, whatever beta
    assert torch.equal(dst[~touched], dst0[~touched])                           # the guard bands
    for d, s, lo, hi in copies:
        assert torch.equal(d[lo:hi], s[lo:hi]) and bool((d[:lo] == 0).all()) and bool((d[hi:] == 0).all())
    # beta from the block
    pairs2, (src2, dst2), _ = _ema_case()
    block = torch.tensor([0.0, 0.0, 0.0, beta, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64, device='cuda')
    EmaTable.from_pairs(pairs2).update(schedule=block)
    assert torch.equal(dst2, dst)


def _tiny_G(compute_dtype=torch.bfloat16):
    from afcm_amd.networks_stylegan3 import Stylegan3Generator
    from test_gpu_train_batch import TINY
    g = load_golden('G1_tiny128')
    G = Stylegan3Generator(z_dim=32, c_dim=1, w_dim=32, img_resolution=128, img_channels_in=4, img_channels_out=1, mapping_kwargs=dict(num_layers=2),
                           synthesis_kwargs=dict(TINY, compute_dtype=compute_dtype)).eval()
    G.load_state_dict({k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith('sd/')}, strict=True)
    return G.cuda()


def _tiny_D():
    """The 128^2 discriminator of tests/golden/D2_tiny128_clamp.npz with its 128^2 ... 16^2 blocks in bfloat16, on the project's conv kernels.  The fp32
    blocks run on the framework's convolution, whose weight gradient at these sizes is not reproducible from run to run (two identically built
    unscheduled steps differ by up to 6e-8 in the 128^2 ... 16^2 blocks' weights after one iteration, measured on the MI355X; the 8^2 and 4^2 blocks are
    equal): equal bits can only be asked of steps whose large blocks run in 16 bits."""
    from afcm_amd.networks_discriminator import CoModDiscriminator
    g = load_golden('D2_tiny128_clamp')
    res, _, cb, cm, group, clamp = [int(v) for v in g['meta']]
    D = CoModDiscriminator(c_dim=0, img_resolution=res, img_channels=5, channel_base=cb, channel_max=cm, conv_clamp=clamp, num_fp16_res=4,
                           block_kwargs=dict(fp16_dtype=torch.bfloat16), epilogue_kwargs=dict(mbstd_group_size=group))
    D.load_state_dict({k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith('sd/')}, strict=True)
    return D.cuda()


def _full_step(schedule=None, **kw):
    from afcm_amd.stylegan3_model import StyleGAN3Step
    return StyleGAN3Step(_tiny_G(), _tiny_D(), lr_G=0.0002, lr_D=0.0002, capturable=True, schedule=schedule, **kw)


def test_update_ema_kernel_against_the_foreach_path():
    from afcm_amd.stylegan3_model import StyleGAN3GeneratorStep, update_ema
    import copy
    s = _schedule(ema_kimgs=10.0, ramp=0.05, total_iters=100)
    step = StyleGAN3GeneratorStep(_tiny_G(), lr_G=0.0002, capturable=True, ema=True, schedule=s)
    gen = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for p in step.netG.parameters():
            p.add_(torch.randn(p.shape, generator=gen).cuda() * 0.1)
        for b in step.netG.buffers():
            if b.is_floating_point():
                b.add_(1.0)
    theirs = copy.deepcopy(step.netG_ema)
    before = [p.detach().clone() for p in step.netG_ema.parameters()]
    s.advance(4)
    step.update_ema()
    beta = update_ema(theirs, step.netG, 4, 104, ema_kimgs=10.0, ramp=0.05)
    assert R.rel(beta, s.read()['ema_beta']) <= 1e-15 and 0 < beta < 1
    n_buffers = 0
    for p, pe0, mine, other in zip(step.netG.parameters(), before, step.netG_ema.parameters(), theirs.parameters()):
        want, bound = R.lerp_ref(p.detach(), pe0, beta)
        assert bool(((mine.detach().double() - want).abs() <= bound).all()) and bool(((other.detach().double() - want).abs() <= bound).all())
    for b, mine, other in zip(step.netG.buffers(), step.netG_ema.buffers(), theirs.buffers()):
        assert torch.equal(mine, b) and torch.equal(other, b)
        n_buffers += 1
    assert n_buffers > 10 and any(not torch.equal(a, b) for a, b in zip(before, step.netG_ema.parameters()))
    with pytest.raises(RuntimeError, match='schedule'):
        StyleGAN3GeneratorStep(_tiny_G(), ema=True).update_ema()


# ---- 4. Adam with the learning rate on the device ---------------------------------------------------------------------------------------------

def test_adam_lr_on_the_device_equals_the_launch_scalar():
    from afcm_amd.optim import FusedScrubAdam
    shapes = [(33, 7), (5,), (16385,), (3, 5, 7)]

    def params():
        gen = torch.Generator().manual_seed(7)
        return [torch.nn.Parameter(torch.randn(s, generator=gen).cuda()) for s in shapes]

    lr = 0.0002
    s = _schedule(lr_G=lr, lr_D=3.0)
    pa, pb = params(), params()
    a = FusedScrubAdam(pa, lr=lr, betas=(0.0, 0.99), capturable=True, lr_dev=s.lr_G_dev)
    b = FusedScrubAdam(pb, lr=lr, betas=(0.0, 0.99), capturable=True)
    gen = torch.Generator().manual_seed(8)

    def one():
        for p, q in zip(pa, pb):
            g = torch.randn(p.shape, generator=gen).cuda()
            p.grad, q.grad = g.clone(), g.clone()
        a.step(), b.step()
        for p, q in zip(pa, pb):
            assert torch.equal(p, q)
            for k in ('exp_avg', 'exp_avg_sq'):
                assert torch.equal(a.state[p][k], b.state[q][k])

    before = [p.detach().clone() for p in pa]
    for _ in range(3):
        one()
    assert all(not torch.equal(p, q) for p, q in zip(pa, before))
    s.set_lr(lr / 2, 3.0)                                                       # the device scalar alone: a's param_groups still say lr
    b.set_lr(lr / 2)
    assert a.param_groups[0]['lr'] == lr and s.read()['lr_D'] == 3.0
    moved = [p.detach().clone() for p in pa]
    one()
    assert all(not torch.equal(p, q) for p, q in zip(pa, moved)) and a.device_step() == b.device_step() == 4


# ---- 5. the steps -------------------------------------------------------------------------------------------------------------------------

def _nets(step):
    return [p.detach() for name in step.model_names for p in getattr(step, 'net' + name).parameters()]


def test_scheduled_step_with_the_blur_off_equals_the_unscheduled_step():
    """Sigma stays below 1/3 (radius 0): the scheduled path -- the blur's copy, the learning rates from the block -- adds nothing."""
    from afcm_amd import synthetic
    a, b, z, c = synthetic.generator_inputs(2, size=128, z_dim=32, seed=0, device='cuda')
    kw = dict(blur_init_sigma=0.3, blur_fade_kimg=1.0)
    s = _schedule(lr_G=0.0002, **kw)
    mine, plain = _full_step(schedule=s, **kw), _full_step(**kw)
    start = [p.clone() for p in _nets(mine)]
    total = 0
    for _ in range(3):
        total += 2
        s.advance(2)
        for step in (mine, plain):
            step.set_input(a, b, z, c)
            step.optimize_parameters(cur_nimg=total)
    assert plain.blur_sigma == s.read()['blur_sigma'] > 0 and s.read()['blur_radius'] == 0.0
    assert len(_nets(mine)) == len(_nets(plain)) and all(torch.equal(p, q) for p, q in zip(_nets(mine), _nets(plain)))
    assert all(not torch.equal(p, q) for p, q in zip(_nets(mine), start))


def test_training_graph_with_a_schedule_equals_eager_scheduled_steps(monkeypatch):
    """blur_init_sigma 2 (radius 6, the block's state before the first step) fading over 13 images at batch 2: ``advance`` runs before each step's
    blur, so the six iterations run at radius 5, 4, 3, 2, 1 and 0; the EMA's beta ramps.  Replays against eager iterations of the same scheduled step: the same kernels without the graph."""
    from afcm_amd.schedule import DeviceSchedule
    from afcm_amd.training import TrainingGraph, train_epoch
    from test_gpu_train_batch import _tiny_set
    from test_gpu_volume import _counting
    ds, items = _tiny_set()
    items = items[:12]
    z = torch.randn(2, 32, generator=torch.Generator().manual_seed(9)).cuda()
    kw = dict(blur_init_sigma=2.0, blur_fade_kimg=0.013, ema_kimgs=10.0, ramp=0.05)
    assert [DeviceSchedule.host_values(t, 2, **kw)['blur_radius'] for t in (2, 4, 6, 8, 10, 12)] == [5.0, 4.0, 3.0, 2.0, 1.0, 0.0]

    eager = _full_step(schedule=_schedule(**kw), ema=True, **{k: kw[k] for k in ('blur_init_sigma', 'blur_fade_kimg')})
    train_epoch(eager, ds, 2, items[:6], gen_z=z)                               # the three steps the graph's warm-up runs ...
    assert eager.schedule.read()['total_iters'] == 6.0
    eager.schedule.load_state_dict(dict(total_iters=0, lr_G=0.0002, lr_D=0.0002))      # ... and undoes in the block
    train_epoch(eager, ds, 2, items, gen_z=z)

    step = _full_step(schedule=_schedule(**kw), ema=True, **{k: kw[k] for k in ('blur_init_sigma', 'blur_fade_kimg')})
    ds.load_epoch(items)
    graph = TrainingGraph(step, ds, 2, warmup=3, fixed_z=True, gen_z=z)
    torch.cuda.synchronize()
    assert step.schedule.block.cpu().tolist() == [0.0, 2.0, 6.0, 0.0, 0.0002, 0.0002, 0.0, 0.0]      # the warm-up restored the block
    copies = []
    _counting(monkeypatch, copies)
    for _ in range(6):
        graph.replay()
    monkeypatch.undo()
    assert copies == [], copies                                                  # no device -> host copy inside the replays
    torch.cuda.synchronize()
    got, want = step.schedule.read(), DeviceSchedule.host_values(12, 2, **kw)
    assert got['total_iters'] == 12.0 and got['blur_sigma'] == want['blur_sigma'] > 0.0 and got['blur_radius'] == 0.0
    assert R.rel(got['ema_beta'], want['ema_beta']) <= 1e-15 and torch.equal(step.schedule.block, eager.schedule.block)
    assert step.model_names == ['G', 'D', 'G_ema'] and step.optimizer_G.device_step() == 9
    for p, q in zip(_nets(step), _nets(eager)):
        assert torch.equal(p, q)
    assert all(bool(torch.isfinite(p).all()) for p in _nets(step))
    assert any(not torch.equal(p, q) for p, q in zip(step.netG.parameters(), step.netG_ema.parameters()))


def test_train_epochs_follows_the_learning_rate_schedule():
    from afcm_amd.schedule import LRSchedule
    from afcm_amd.training import train_epochs
    from test_gpu_train_batch import _tiny_set
    ds, _ = _tiny_set()
    z = torch.randn(2, 32, generator=torch.Generator().manual_seed(10)).cuda()
    decaying = LRSchedule('linear', 0.0002, epoch_count=1, n_epochs=2, n_epochs_decay=2)
    constant = LRSchedule('linear', 0.0002, epoch_count=1, n_epochs=100, n_epochs_decay=100)
    assert decaying.lr_at(1) == 0.0002 and decaying.lr_at(2) == 0.0002 * (1.0 - 1 / 3.0) and constant.lr_at(2) == 0.0002
    finals, seen = {}, []
    for name, lrs, graph in (('graph', decaying, True), ('eager', decaying, False), ('constant', constant, True)):
        s = _schedule(blur_init_sigma=2.0, blur_fade_kimg=0.03, ema_kimgs=10.0, ramp=0.05)       # the blur fades out inside the first epoch
        step = _full_step(schedule=s, ema=True)
        steps = train_epochs(step, ds, 2, range(1, 3), lrs, 5, graph=graph, gen_z=z,
                             on_epoch=(lambda e, st: seen.append((e, st.schedule.read()['lr_G']))) if name == 'graph' else None)
        assert steps == 18 and s.read()['total_iters'] == 36.0
        assert s.read()['lr_G'] == s.read()['lr_D'] == lrs.lr_at(2) == step.optimizer_G.param_groups[0]['lr'] == step.optimizer_D.param_groups[0]['lr']
        assert step.optimizer_G.device_step() == 18
        finals[name] = [p.clone() for p in _nets(step)]
    assert seen == [(1, 0.0002), (2, decaying.lr_at(2))]
    differing = [(i, (p - q).abs().max().item()) for i, (p, q) in enumerate(zip(finals['graph'], finals['eager'])) if not torch.equal(p, q)]
    print(f'train_epochs graph against eager: {len(differing)} of {len(finals["graph"])} tensors differ', differing[:8])
    assert all(torch.equal(p, q) for p, q in zip(finals['graph'], finals['eager']))
    assert any(not torch.equal(p, q) for p, q in zip(finals['graph'], finals['constant']))
