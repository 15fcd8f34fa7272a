"""The training log on the device (csrc/trainlog.hip, afcm_amd/trainlog.py): afcm_grad_stats and afcm_trainlog_append against their numpy
restatement (tests/trainlog_ref.py) bit for bit, the Adam launch untouched by the statistics launch in front of it, the steps' rows against the
steps' own loss tensors, schedule block, step counts and gradients, and the log of a replayed graph against the log of eager steps."""
import ctypes

import numpy as np
import pytest
import torch

import trainlog_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu


def _lib():
    from afcm_amd import _lib
    return _lib


def _chunk():
    return int(_lib().load().afcm_adam_chunk_elems())


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint64)


def _same_log(a, b):
    """Rows and head of two logs, or of a log and a snapshot, as bit patterns (a NaN column equals itself)."""
    a, b = (t._buf if hasattr(t, '_buf') else t for t in (a, b))
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


# ---- 1. the statistics kernel ------------------------------------------------------------------------------------------------------------------

def _stats_case():
    """Parameters of 1, 3, 5, 1023, chunk - 1, chunk, chunk + 1 and 2 chunk + 5 elements and one more that gets no gradient.  The gradient of the
    chunk + 1 tensor is a view 4 bytes into its buffer (the element-by-element path, across a chunk seam); the others are 16-byte aligned."""
    chunk = _chunk()
    sizes = [1, 3, 5, 1023, chunk - 1, chunk, chunk + 1, 2 * chunk + 5]
    rng = np.random.default_rng(21)
    grads = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-5, 5, n)).astype(np.float32) for n in sizes]
    nan, pinf, ninf = np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)
    grads[0][0] = nan                                                                    # a first element that is the last one too
    grads[1][0], grads[1][2] = pinf, ninf                                                # first and last
    grads[2][4] = nan                                                                    # the element-by-element tail of an aligned tensor (5 = 4 + 1)
    grads[3][0], grads[3][1022], grads[3][1020] = ninf, pinf, nan                        # first, last (tail of 3), inside the tail
    grads[4][chunk - 2] = nan                                                            # last element of a chunk one short of full
    grads[5][0], grads[5][chunk - 1] = nan, ninf                                         # a whole chunk: the unrolled path
    grads[6][chunk - 1], grads[6][chunk] = pinf, nan                                     # both sides of a seam, element-by-element path
    grads[7][chunk - 1], grads[7][chunk], grads[7][2 * chunk - 1], grads[7][2 * chunk] = nan, pinf, ninf, nan     # both seams, aligned path
    grads[7][2 * chunk + 4] = pinf                                                       # the last chunk's tail (5 = 4 + 1)
    grads[7][5:9] = [-0.0, 1e-40, -3e-44, 1.1754942e-38]                                 # a signed zero and denormals
    grads[6][3:6] = [-0.0, 7e-41, -1e-45]
    grads[5][17] = 3e38                                                                  # finite; +inf under a scale of 2
    grads[6][18] = -3e38
    params = [torch.nn.Parameter(torch.zeros(n, device='cuda')) for n in sizes + [7]]
    for i, (p, g) in enumerate(zip(params, grads)):
        if i == 6:
            buf = torch.zeros(g.size + 8, device='cuda')
            view = buf[1:1 + g.size]
            view.copy_(torch.from_numpy(g))
            p.grad = view
        else:
            p.grad = torch.from_numpy(g).cuda()
    aligned = [p.grad.data_ptr() % 16 == 0 for p in params[:-1]]
    assert aligned == [True] * 6 + [False, True] and params[6].grad.data_ptr() % 16 == 4 and params[-1].grad is None
    return chunk, sizes, grads, aligned, params


@pytest.fixture(scope='module')
def stats_case():
    return _stats_case()


@pytest.mark.parametrize('scale', [1.0, 0.5, 1.0 / 3.0, 2.0])
def test_grad_stats_equal_the_restatement_bit_for_bit(stats_case, scale):
    from afcm_amd.optim import FusedScrubAdam
    chunk, sizes, grads, aligned, params = stats_case
    opt = FusedScrubAdam(params, lr=1e-3, betas=(0.0, 0.99), stats=True)
    assert opt.grad_stats()[1] == 0 and opt.grad_stats()[0].shape == (sum((n + chunk - 1) // chunk for n in sizes + [7]), 4)
    want = R.table_partials(list(zip(grads, aligned)), scale, chunk)
    opt.step(grad_scale=scale)
    partials, chunks = opt.grad_stats()
    assert chunks == want.shape[0] == partials.shape[0] - 1                              # the parameter without a gradient has no rows
    first = partials[:chunks].clone()
    opt.step(grad_scale=scale)                                                           # the same gradients again: the same bits
    assert opt.grad_stats()[1] == chunks and np.array_equal(_bits(partials[:chunks]), _bits(first))
    got = first.cpu().numpy()
    print(f'scale {scale}: sumsq {got[:, 0].sum():.6e}, counts {got[:, 1:].sum(0).tolist()}')
    assert np.array_equal(got[:, 1:], want[:, 1:])
    assert np.array_equal(got[:, 0].view(np.uint64), want[:, 0].view(np.uint64)), (got[:, 0], want[:, 0])
    planted = [8.0, 5.0, 4.0]
    assert got[:, 1:].sum(0).tolist() == (planted if scale < 2.0 else [8.0, 6.0, 5.0])  # 3e38 and -3e38 overflow under 2
    assert float(partials[chunks:].abs().sum()) == 0.0                                   # nothing is written past the table's chunks
    assert all(bool(torch.isfinite(p).all()) for p in params)                            # the scrub did its work


# ---- 2. the append kernel -----------------------------------------------------------------------------------------------------------------------

def _append(log, block=None, step_G=None, step_D=None, losses=None, part_G=None, chunks_G=0, part_D=None, chunks_D=0, capacity=None, null_log=False):
    L = _lib()
    return L.load().afcm_trainlog_append(None if null_log else _vp(log.log), log.capacity if capacity is None else capacity, _vp(log.head), _vp(block),
                                         _vp(step_G), _vp(step_D), _vp(losses), _vp(part_G), chunks_G, _vp(part_D), chunks_D, L.stream_ptr(log.log))


@pytest.mark.parametrize('tensors', [1, 255, 256, 257, 600])
def test_append_reduces_in_the_stated_order(tensors):
    """`tensors` one-chunk tensors: 1, 255, 256, 257 and 600 rows of partials, the seams of 'thread t adds rows t, t + 256, ...' and of the tree."""
    from afcm_amd.optim import FusedScrubAdam
    from afcm_amd.trainlog import DeviceTrainLog
    gen = torch.Generator().manual_seed(tensors)
    params = [torch.nn.Parameter(torch.zeros(3, device='cuda')) for _ in range(tensors)]
    for i, p in enumerate(params):
        p.grad = (torch.randn(3, generator=gen) * 10.0 ** float(torch.randint(-4, 5, (1,), generator=gen))).cuda()
        if i % 7 == 3:
            p.grad[i % 3] = float('nan') if i % 2 else float('inf')
    opt = FusedScrubAdam(params, lr=1e-3, betas=(0.0, 0.99), stats=True, capturable=True)
    opt.step()
    partials, chunks = opt.grad_stats()
    assert chunks == tensors
    host = partials.cpu().numpy()
    other = torch.from_numpy(host[::-1].copy() * 3.0).cuda()                             # a second table: other values, same shape
    block = torch.tensor([12.0, 1.5, 4.0, 0.999, 2e-4, 1e-4, 0.0, 0.0], dtype=torch.float64, device='cuda')
    losses = torch.tensor([0.5, 1.25, float('nan'), 3.0, 1e-3], dtype=torch.float32, device='cuda')
    step_D = torch.full([1], 41.0, dtype=torch.float32, device='cuda')
    log = DeviceTrainLog(4, 'cuda')
    assert _append(log, block, opt._step_dev[(0, params[0].device)], step_D, losses, partials, chunks, other, chunks) == 0
    assert _append(log, None, opt._step_dev[(0, params[0].device)], None, losses, partials, chunks, None, 0) == 0
    rows, lost = log.read()
    assert lost == 0 and rows.shape == (2, R.COLS)
    want0 = R.append_row(0, block.cpu().numpy(), 1.0, 41.0, losses.cpu().numpy(), host, other.cpu().numpy())
    want1 = R.append_row(1, None, 1.0, None, losses.cpu().numpy(), host, None)
    assert R.same_bits(rows[0], want0), (rows[0], want0)
    assert R.same_bits(rows[1], want1), (rows[1], want1)
    assert np.isnan(rows[1][1:9]).all() and np.isnan(rows[1][10]) and np.isnan(rows[1][20:]).all() and np.isnan(rows[0][13])
    assert rows[0][1:9].tolist() == block.cpu().tolist()
    assert rows[0][17] + rows[0][18] == float(sum(1 for i in range(tensors) if i % 7 == 3))


def test_ring_wraps_and_the_entry_point_refuses_bad_arguments():
    from afcm_amd.trainlog import DeviceTrainLog
    L = _lib()
    log = DeviceTrainLog(4, 'cuda')
    losses = torch.zeros(5, dtype=torch.float32, device='cuda')
    for s in range(6):
        losses.fill_(float(s))
        assert _append(log, losses=losses) == 0
    rows, lost = log.read()
    assert rows[:, 0].tolist() == [2.0, 3.0, 4.0, 5.0] and lost == 2 and rows[:, 11].tolist() == [2.0, 3.0, 4.0, 5.0]
    rows, lost = log.read(since=3)
    assert rows[:, 0].tolist() == [3.0, 4.0, 5.0] and lost == 0
    rows, lost = log.read(since=1)
    assert rows[:, 0].tolist() == [2.0, 3.0, 4.0, 5.0] and lost == 1
    assert log.read(since=9)[0].shape == (0, R.COLS)
    before = log.snapshot()
    assert _append(log, losses=losses, capacity=0) == L.E_INVALID and b'capacity' in L.load().afcm_last_error()
    assert _append(log, losses=losses, null_log=True) == L.E_INVALID and b'null' in L.load().afcm_last_error()
    assert _append(log, losses=losses, chunks_G=-1) == L.E_INVALID
    assert L.load().afcm_trainlog_append(_vp(log.log), 4, None, None, None, None, None, None, 0, None, 0, L.stream_ptr(log.log)) == L.E_INVALID
    torch.cuda.synchronize()
    assert _same_log(log, before) and int(log.head.item()) == 6            # the argument check launched nothing
    one = DeviceTrainLog(1, 'cuda')
    for s in range(3):
        assert _append(one) == 0
    rows, lost = one.read()
    assert rows[:, 0].tolist() == [2.0] and lost == 2 and np.isnan(rows[0, 1:]).all()


# ---- 3. the Adam launch is untouched --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('capturable', [False, True])
def test_adam_with_statistics_equals_adam_without(capturable):
    from afcm_amd.optim import FusedScrubAdam
    chunk = _chunk()
    shapes = [(33, 7), (5,), (chunk + 1,), (3, 5, 7)]

    def params():
        gen = torch.Generator().manual_seed(7)
        return [torch.nn.Parameter(torch.randn(s, generator=gen).cuda()) for s in shapes]

    pa, pb = params(), params()
    a = FusedScrubAdam(pa, lr=1e-3, betas=(0.0, 0.99), capturable=capturable, stats=True)
    b = FusedScrubAdam(pb, lr=1e-3, betas=(0.0, 0.99), capturable=capturable)
    assert b._stats == {} and b.stats is False
    gen = torch.Generator().manual_seed(8)
    for it in range(3):
        for p, q in zip(pa, pb):
            g = torch.randn(p.shape, generator=gen).cuda()
            if it == 1:
                g.view(-1)[0], g.view(-1)[-1] = float('nan'), float('-inf')
            p.grad, q.grad = g.clone(), g.clone()
        a.step(grad_scale=0.5), b.step(grad_scale=0.5)
        for p, q in zip(pa, pb):
            assert torch.equal(p, q) and bool(torch.isfinite(p).all())
            for k in ('exp_avg', 'exp_avg_sq'):
                assert torch.equal(a.state[p][k], b.state[q][k])
        counts = a.grad_stats()[0][:a.grad_stats()[1], 1:].sum(0).tolist()
        assert counts == ([4.0, 0.0, 4.0] if it == 1 else [0.0, 0.0, 0.0])
    snap = a.snapshot()
    kept = a.grad_stats()[0].clone()
    a.grad_stats()[0].fill_(-1.0)
    a.restore(snap)
    assert torch.equal(a.grad_stats()[0], kept) and a.grad_stats()[1] == 5


# ---- 4. the steps -----------------------------------------------------------------------------------------------------------------------------

TINY = dict(channel_base=256, channel_max=8, num_layers=14, num_critical=2, margin_size=10, output_scale=0.25, skip_resolution=128, conv_kernel=3,
            filter_size=6, lrelu_upsampling=2, use_radial_filters=False, conv_clamp=256, magnitude_ema_beta=0.5 ** (16 / 20e3), cond_mod=True)


def _tiny_G(compute_dtype=torch.bfloat16):
    """The 128^2 generator of tests/golden/G1_tiny128.npz, as tests/test_gpu_schedule.py builds it."""
    from afcm_amd.networks_stylegan3 import Stylegan3Generator
    g = load_golden('G1_tiny128')
    G = Stylegan3Generator(z_dim=32, c_dim=1, w_dim=32, img_resolution=128, img_channels_in=4, img_channels_out=1, mapping_kwargs=dict(num_layers=2),
                           synthesis_kwargs=dict(TINY, compute_dtype=compute_dtype)).eval()
    G.load_state_dict({k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith('sd/')}, strict=True)
    return G.cuda()


def _tiny_D():
    """The 128^2 discriminator of tests/golden/D2_tiny128_clamp.npz with its large blocks in bfloat16 (on the project's conv kernels: reproducible)."""
    from afcm_amd.networks_discriminator import CoModDiscriminator
    g = load_golden('D2_tiny128_clamp')
    res, _, cb, cm, group, clamp = [int(v) for v in g['meta']]
    D = CoModDiscriminator(c_dim=0, img_resolution=res, img_channels=5, channel_base=cb, channel_max=cm, conv_clamp=clamp, num_fp16_res=4,
                           block_kwargs=dict(fp16_dtype=torch.bfloat16), epilogue_kwargs=dict(mbstd_group_size=group))
    D.load_state_dict({k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith('sd/')}, strict=True)
    return D.cuda()


def _schedule(**kw):
    from afcm_amd.schedule import DeviceSchedule
    return DeviceSchedule('cuda', lr_G=0.0002, **kw)


def _full_step(schedule=None, **kw):
    from afcm_amd.stylegan3_model import StyleGAN3Step
    return StyleGAN3Step(_tiny_G(), _tiny_D(), lr_G=0.0002, lr_D=0.0002, capturable=True, schedule=schedule, **kw)


def _nets(step):
    return [p.detach() for name in step.model_names for p in getattr(step, 'net' + name).parameters()]


def _restated_stats(net, chunk):
    """The four statistics of a network's gradients as they stand, through the restatement: table order is parameter order, without the ones that
    have no gradient."""
    tensors = [(p.grad.detach().clone().cpu().numpy().reshape(-1), p.grad.data_ptr() % 16 == 0) for p in net.parameters() if p.grad is not None]
    return R.reduce_partials(R.table_partials(tensors, 1.0, chunk))


def _small_set(depth=4):
    """tests/test_gpu_train_batch.py's two synthetic subjects at `depth` slices each: an epoch of 2 * depth rows."""
    from afcm_amd.training import DeviceSliceSet
    zz, yy, xx = np.meshgrid(np.linspace(-1, 1, depth), np.linspace(-1, 1, 120), np.linspace(-1, 1, 140), indexing='ij')
    sources = []
    for s in range(2):
        body = np.clip(1.2 - (zz ** 2 * 0.3 + yy ** 2 + xx ** 2), 0, 1)
        sources.append({'t1': np.round(body * (0.6 + 0.4 * np.sin(7 * xx + s) * np.cos(5 * yy + zz)) * 255).astype(np.uint8),
                        't2': np.round(body * (0.5 + 0.5 * np.cos(4 * xx - s) * np.sin(6 * yy + zz)) * 255).astype(np.uint8)})
    ds = DeviceSliceSet(sources, patch_shape=(1, 128, 128), raw_internal_path_in=['t1'], raw_internal_path_out=['t2'], thickness=[5], device='cuda')
    return ds, ds.epoch_items(11)


def test_step_rows_equal_the_steps_own_tensors():
    """Three eager D + G iterations with a schedule and a log, the same three without a log.  In the third a hook plants 5 NaN and 3 +inf into one
    generator gradient: row 2 counts them, and the scrub keeps the parameters finite in both arms."""
    from afcm_amd import synthetic
    from afcm_amd.trainlog import COLUMNS, DeviceTrainLog
    chunk = _chunk()
    a, b, z, c = synthetic.generator_inputs(2, size=128, z_dim=32, seed=0, device='cuda')
    kw = dict(blur_init_sigma=2.0, blur_fade_kimg=0.013)
    log = DeviceTrainLog(8, 'cuda')
    mine, plain = _full_step(schedule=_schedule(**kw), log=log, **kw), _full_step(schedule=_schedule(**kw), **kw)
    assert mine.optimizer_G.stats and mine.optimizer_D.stats and not plain.optimizer_G.stats and not plain.optimizer_D.stats and plain.log is None
    k_nan, j_inf = 5, 3
    planting = [False]

    def plant(g):
        if not planting[0]:
            return g
        g = g.clone()
        g.view(-1)[:k_nan] = float('nan')
        g.view(-1)[-j_inf:] = float('inf')
        return g

    for step in (mine, plain):
        target = max((p for n, p in step.netG.synthesis.named_parameters() if n.endswith('weight') and p.ndim == 4), key=lambda p: p.numel())
        target.register_hook(plant)
    col = {name: i for i, name in enumerate(COLUMNS)}
    for it in range(3):
        planting[0] = it == 2
        for step in (mine, plain):
            step.schedule.advance(2)
            step.set_input(a, b, z, c)
            step.optimize_parameters()
        rows, lost = log.read()
        assert lost == 0 and rows.shape == (it + 1, len(COLUMNS)) and rows[:, 0].tolist() == [float(s) for s in range(it + 1)]
        row = rows[it]
        for name in ('G_GAN', 'G_L1', 'D_real', 'D_fake', 'Dr1'):
            assert row[col[name]] == float(getattr(mine, 'loss_' + name).detach()), name
        assert np.isfinite(row[11:16]).all()
        assert row[1:9].tolist() == mine.schedule.block.cpu().tolist() and row[col['total_iters']] == 2.0 * (it + 1) and row[col['lr_G']] == 0.0002
        assert row[col['step_G']] == mine.optimizer_G.device_step() == it + 1 and row[col['step_D']] == mine.optimizer_D.device_step() == it + 1
        want_G, want_D = _restated_stats(mine.netG, chunk), _restated_stats(mine.netD, chunk)
        print(f'step {it}: G {row[16:20].tolist()} D {row[20:24].tolist()}')
        assert R.same_bits(row[16:20], want_G), (row[16:20], want_G)
        assert R.same_bits(row[20:24], want_D), (row[20:24], want_D)
        assert row[16] > 0 and row[20] > 0
        assert row[17:20].tolist() == ([float(k_nan), float(j_inf), 0.0] if it == 2 else [0.0, 0.0, 0.0]) and row[21:24].tolist() == [0.0, 0.0, 0.0]
    assert len(_nets(mine)) == len(_nets(plain)) and all(torch.equal(p, q) for p, q in zip(_nets(mine), _nets(plain)))
    assert all(bool(torch.isfinite(p).all()) for p in _nets(mine))


def test_generator_only_step_without_a_schedule():
    """No discriminator, no schedule, an optimizer that counts its steps on the host: the D columns, the block and the four losses the step does not
    have are NaN."""
    from afcm_amd import synthetic
    from afcm_amd.stylegan3_model import StyleGAN3GeneratorStep
    from afcm_amd.trainlog import DeviceTrainLog
    a, b, z, c = synthetic.generator_inputs(2, size=128, z_dim=32, seed=0, device='cuda')
    log = DeviceTrainLog(2, 'cuda')
    step = StyleGAN3GeneratorStep(_tiny_G(), lr_G=0.0002, log=log)
    for _ in range(2):
        step.set_input(a, b, z, c)
        step.optimize_parameters()
    rows, lost = log.read()
    assert lost == 0 and rows[:, 0].tolist() == [0.0, 1.0] and rows[:, 9].tolist() == [1.0, 2.0]
    row = rows[1]
    assert row[12] == float(step.loss_G_L1.detach()) and np.isnan(row[[11, 13, 14, 15]]).all()
    assert np.isnan(row[1:9]).all() and np.isnan(row[10]) and np.isnan(row[20:24]).all()
    assert R.same_bits(row[16:20], _restated_stats(step.netG, _chunk())) and row[16] > 0 and row[17:20].tolist() == [0.0, 0.0, 0.0]
    with pytest.raises(RuntimeError, match='own device'):
        StyleGAN3GeneratorStep(step.netG, log=DeviceTrainLog(2, 'cpu'))


# ---- 5. the graph -----------------------------------------------------------------------------------------------------------------------------

def test_replayed_graph_leaves_the_log_of_eager_steps(monkeypatch):
    from afcm_amd.trainlog import DeviceTrainLog
    from afcm_amd.training import TrainingGraph, train_epoch
    from test_gpu_volume import _counting
    ds, items = _small_set()
    assert len(items) == 8
    z = torch.randn(2, 32, generator=torch.Generator().manual_seed(9)).cuda()
    kw = dict(blur_init_sigma=2.0, blur_fade_kimg=0.013)
    eager = _full_step(schedule=_schedule(**kw), log=DeviceTrainLog(8, 'cuda'), **kw)
    train_epoch(eager, ds, 2, items, gen_z=z)

    step = _full_step(schedule=_schedule(**kw), log=DeviceTrainLog(8, 'cuda'), **kw)
    ds.load_epoch(items)
    graph = TrainingGraph(step, ds, 2, warmup=3, fixed_z=True, gen_z=z, undo_warmup=True)
    torch.cuda.synchronize()
    assert int(step.log.head.item()) == 0 and float(step.log.log.abs().sum()) == 0.0     # the warm-up's three rows are gone
    assert float(step.optimizer_G.grad_stats()[0].abs().sum()) == 0.0 and float(step.optimizer_D.grad_stats()[0].abs().sum()) == 0.0
    copies = []
    _counting(monkeypatch, copies)
    for _ in range(4):
        graph.replay()
    assert copies == [], copies                                                          # nothing inside the replays reads the device
    rows, lost = step.log.read()
    monkeypatch.undo()
    assert copies == [('cpu', (8 * R.COLS + 1,))], copies                                # rows and head: one device -> host copy
    assert lost == 0 and rows[:, 0].tolist() == [0.0, 1.0, 2.0, 3.0] and rows[:, 1].tolist() == [2.0, 4.0, 6.0, 8.0]
    assert rows[:, 9].tolist() == rows[:, 10].tolist() == [1.0, 2.0, 3.0, 4.0]
    assert _same_log(step.log, eager.log) and torch.equal(step.log.log, eager.log.log) and torch.equal(step.log.head, eager.log.head)
    assert R.same_bits(rows, eager.log.read()[0]) and np.isfinite(rows[:, 11:]).all() and (rows[:, 16] > 0).all() and (rows[:, 20] > 0).all()
    for p, q in zip(_nets(step), _nets(eager)):
        assert torch.equal(p, q)

    # without undo_warmup the rows of the warm-up stay in the ring, and the head goes back all the same
    kept = _full_step(schedule=_schedule(**kw), log=DeviceTrainLog(8, 'cuda'), **kw)
    ds.load_epoch(items)
    TrainingGraph(kept, ds, 2, warmup=2, fixed_z=True, gen_z=z)
    torch.cuda.synchronize()
    assert int(kept.log.head.item()) == 0 and kept.log.log[:2, 0].tolist() == [0.0, 1.0] and float(kept.log.log[2:].abs().sum()) == 0.0


def test_train_epochs_logs_the_same_with_and_without_the_graph():
    from afcm_amd.schedule import LRSchedule
    from afcm_amd.trainlog import COLUMNS, DeviceTrainLog
    from afcm_amd.training import train_epochs
    ds, _ = _small_set()
    z = torch.randn(2, 32, generator=torch.Generator().manual_seed(10)).cuda()
    lrs = LRSchedule('linear', 0.0002, epoch_count=1, n_epochs=1, n_epochs_decay=1)
    logs, seen = {}, []
    for graph in (True, False):
        step = _full_step(schedule=_schedule(blur_init_sigma=2.0, blur_fade_kimg=0.01), log=DeviceTrainLog(8, 'cuda'))
        steps = train_epochs(step, ds, 2, range(1, 3), lrs, 5, graph=graph, gen_z=z,
                             on_epoch=(lambda e, st: seen.append((e,) + st.log.read(since=4 * (e - 1)))) if graph else None)
        assert steps == 8
        logs[graph] = step.log
    assert [(e, rows[:, 0].tolist(), lost) for e, rows, lost in seen] == [(1, [0.0, 1.0, 2.0, 3.0], 0), (2, [4.0, 5.0, 6.0, 7.0], 0)]
    rows, lost = logs[True].read()
    assert lost == 0 and rows[:, 0].tolist() == [float(s) for s in range(8)] and rows[:, 1].tolist() == [2.0 * (s + 1) for s in range(8)]
    assert rows[:4, COLUMNS.index('lr_G')].tolist() == [lrs.lr_at(1)] * 4 and rows[4:, COLUMNS.index('lr_D')].tolist() == [lrs.lr_at(2)] * 4
    assert lrs.lr_at(2) < lrs.lr_at(1)
    assert _same_log(logs[True], logs[False]) and torch.equal(logs[True].log, logs[False].log) and torch.equal(logs[True].head, logs[False].head)
