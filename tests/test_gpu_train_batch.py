"""Training batches on the GPU: ``afcm_batch_assemble`` against stacked ``SliceDataset(phase='train', thickness=[t])`` items (equal bits), its
16-bit outputs, ``out=``, the device cursor, invalid table rows against the numpy restatement (tests/train_batch_ref.py, where the cases live and
where the restatement itself is held to the loader), the host-side checks, and ``train_epoch`` / ``TrainingGraph`` on the tiny 128^2 generator.
Every comparison is exact (``torch.equal`` on bit patterns, NaN items compared as NaN)."""

import numpy as np
import pytest
import torch

import train_batch_ref as T
from conftest import load_golden
from test_train_batch_ref_cpu import dataset_items

pytestmark = pytest.mark.gpu

_BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


def _same_bits(got, want):
    want = torch.as_tensor(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    assert torch.equal(got.cpu().view(_BITS[want.dtype]), want.view(_BITS[want.dtype]))


def _same_or_nan(got, want):
    want = torch.as_tensor(want)
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(got[~nan].view(_BITS[want.dtype]), want[~nan].view(_BITS[want.dtype]))


@pytest.fixture(scope='module')
def loader_items():
    """{(dtype name, hw, k): (A, B, slice_idx) of the 23 shuffled rows as the training loader builds them}, computed on first use."""
    cache = {}

    def get(dtype, hw, k):
        key = (np.dtype(dtype).name, hw, k)
        if key not in cache:
            lo, hi = T.value_range(dtype)
            cache[key] = dataset_items(T.subjects(dtype), T.shuffled_items(k), hw, k, lo, hi)
        return cache[key]
    return get


def _device_set(dtype, hw, k, **kw):
    from afcm_amd.training import DeviceSliceSet
    lo, hi = T.value_range(dtype)
    return DeviceSliceSet(T.subjects(dtype), patch_shape=(1,) + hw, raw_internal_path_in=['t1'], raw_internal_path_out=['t2'], thickness=T.THICKNESSES,
                          slice_num=k, min_value=lo, max_value=hi, device='cuda', **kw)


@pytest.mark.parametrize('k', [4, 1])
@pytest.mark.parametrize('hw', T.PATCHES)
@pytest.mark.parametrize('dtype', T.DTYPES)
def test_batches_equal_stacked_training_items(dtype, hw, k, loader_items):
    want = loader_items(dtype, hw, k)
    ds = _device_set(dtype, hw, k)
    pool, vols = T.pool_and_table(ds.volumes, ('t1', 't2'))
    assert torch.equal(ds.pool.cpu(), torch.from_numpy(pool)) and torch.equal(ds.vols.cpu(), torch.from_numpy(vols)) and len(ds) == 23
    ds.load_epoch(T.shuffled_items(k))
    batches = list(ds.batches(T.BATCH))
    assert [int(b[0].shape[0]) for b in batches] == [5, 5, 5, 5, 3]                      # the last batch is ragged
    assert len(list(ds.batches(T.BATCH, drop_last=True))) == 4
    for j, name in enumerate(('A', 'B', 'slice_idx')):
        _same_bits(torch.cat([b[j] for b in batches]), want[j])
    if k == 1:                                              # no thickness at all: the loader's -1 and its -0.0 label
        lo, hi = T.value_range(dtype)
        items = T.shuffled_items(1, thickness=False)
        ds.load_epoch(items)
        a, b, c = ds.batch(0, 23)
        for got, w in zip((a, b, c), dataset_items(ds.volumes, items, hw, 1, lo, hi)):
            _same_bits(got, w)
        assert bool(torch.signbit(c).all())


@pytest.mark.parametrize('out_dtype', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('hw', T.PATCHES)
def test_16bit_outputs_are_one_more_rounding(out_dtype, hw, loader_items):
    for dtype in (np.uint8, np.float32):
        want = loader_items(dtype, hw, 4)
        ds = _device_set(dtype, hw, 4)
        ds.load_epoch(T.shuffled_items(4))
        for first in range(0, 23, T.BATCH):
            a, b, c = ds.batch(first, min(T.BATCH, 23 - first), dtype=out_dtype)
            sl = slice(first, first + T.BATCH)
            _same_bits(a, torch.from_numpy(want[0][sl]).to(out_dtype))
            _same_bits(b, torch.from_numpy(want[1][sl]).to(out_dtype))
            _same_bits(c, want[2][sl])


@pytest.mark.parametrize('k', [4, 1])
@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
def test_batch_items_equal_slice_assembly(dtype, k):
    """The two loader entry points against each other: every row of a batch is ``assemble_slices`` on the row's own volumes, target by target --
    ``A[i]`` and ``slice_idx[i]`` the call on ``vol_a`` with the row's thickness, ``B[i]`` the ``slice_num=1`` call on ``vol_b``."""
    from afcm_amd.torch_utils.ops.volume_ops import assemble_slices
    hw = (12, 10)
    lo, hi = T.value_range(dtype)
    ds = _device_set(dtype, hw, k)
    items = T.shuffled_items(k)
    ds.load_epoch(items)
    a, b, c = ds.batch(0, len(items))
    volumes = [ds.pool[off:off + d * hs * ws].view(d, hs, ws) for off, d, hs, ws in ds.vols_host.tolist()]
    for i, (va, vb, idx, t) in enumerate(items.tolist()):
        want_a, want_c = assemble_slices(volumes[va], idx, 1, (1,) + hw, thickness=t, slice_num=k, min_value=lo, max_value=hi)
        want_b, _ = assemble_slices(volumes[vb], idx, 1, (1,) + hw, slice_num=1, min_value=lo, max_value=hi)
        _same_bits(a[i:i + 1], want_a.cpu())
        _same_bits(c[i:i + 1], want_c.cpu())
        _same_bits(b[i:i + 1], want_b.cpu())


def test_out_writes_in_place_and_repeats_bit_for_bit(loader_items):
    want = loader_items(np.uint8, (12, 10), 4)
    ds = _device_set(np.uint8, (12, 10), 4)
    ds.load_epoch(T.shuffled_items(4))
    out = (torch.full((5, 4, 12, 10), 7., device='cuda'), torch.full((5, 1, 12, 10), 7., device='cuda'), torch.full((5, 1), 7., device='cuda'))
    ptrs = [t.data_ptr() for t in out]
    got = ds.batch(5, 5, out=out)
    assert all(g is o for g, o in zip(got, out)) and [t.data_ptr() for t in got] == ptrs
    for g, w in zip(got, want):
        _same_bits(g, w[5:10])
    first_run = [t.clone() for t in out]
    for t in out:
        t.fill_(-3.)
    ds.batch(5, 5, out=out)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out, first_run))
    # an output that does not start on a 16-byte boundary: rows stored element by element, the same bits
    wide = torch.full((5 * 4 * 12 * 10 + 1,), 7., device='cuda')
    shifted = wide[1:].view(5, 4, 12, 10)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    ds.batch(5, 5, out=(shifted, out[1], out[2]))
    _same_bits(shifted, want[0][5:10])
    assert float(wide[0]) == 7.


def test_cursor_moves_the_batch_through_the_table():
    from afcm_amd.torch_utils.ops.batch_ops import advance_cursor
    ds = _device_set(np.int16, (16, 16), 4)
    ds.load_epoch(T.shuffled_items(4))
    plain = ds.batch(0, 10)
    assert int(ds.cursor.cpu()) == 0
    got = []
    for _ in range(2):
        got.append(ds.batch(0, 5, use_cursor=True))
        advance_cursor(ds.cursor, 5)
    assert int(ds.cursor.cpu()) == 10
    for j in range(3):
        assert torch.equal(torch.cat([g[j] for g in got]).view(torch.int32), plain[j].view(torch.int32))
    # first counts from the cursor; rows past the table are NaN items
    tail = ds.batch(10, 5, use_cursor=True)
    want = ds.batch(20, 3)
    assert all(torch.equal(t[:3].view(torch.int32), w.view(torch.int32)) and bool(torch.isnan(t[3:]).all()) for t, w in zip(tail, want))
    ds.load_epoch(T.shuffled_items(4))
    assert int(ds.cursor.cpu()) == 0 and ds.position == 0


def test_invalid_rows_are_nan_items_where_the_restatement_puts_them():
    from afcm_amd.torch_utils.ops.batch_ops import assemble_batch
    ds = _device_set(np.uint8, (16, 16), 4)
    pool, vols = T.pool_and_table(ds.volumes, ('t1', 't2'))
    items = T.shuffled_items(4)
    kinds = T.invalid_rows(vols)
    table = items.copy()
    for j, kind in enumerate(sorted(kinds)):
        table[1 + 2 * j] = kinds[kind]                      # rows 1, 3, ..., 17, every one of them inside the middle subject of the pool
    d_table = torch.from_numpy(table).cuda()
    for k in (4, 1):
        want = T.assemble_batch(pool, vols, table, 0, 23, k, 16, 16)
        assert int(np.isnan(want[2]).sum()) == (9 if k == 4 else 8)
        got = assemble_batch(ds.pool, ds.vols, d_table, 0, 23, (16, 16), slice_num=k)
        for g, w in zip(got, want):
            _same_or_nan(g, w)
    # rows past the table and a cursor outside it
    got = assemble_batch(ds.pool, ds.vols, d_table, 20, 5, (16, 16))
    for g, w in zip(got, T.assemble_batch(pool, vols, table, 20, 5, 4, 16, 16)):
        _same_or_nan(g, w)
    for cursor in (-1, 23, 1 << 40):
        got = assemble_batch(ds.pool, ds.vols, d_table, 0, 2, (16, 16), cursor=torch.tensor([cursor], dtype=torch.int64, device='cuda'))
        assert all(bool(torch.isnan(g).all()) for g in got)
    # an unusable descriptor of the middle subject takes out exactly the items that name it
    d_items = torch.from_numpy(items).cuda()
    for kind, edited in T.bad_descriptors(vols, pool.size).items():
        want = T.assemble_batch(pool, edited, items, 0, 23, 4, 16, 16)
        got = assemble_batch(ds.pool, torch.from_numpy(edited).cuda(), d_items, 0, 23, (16, 16))
        for g, w in zip(got, want):
            _same_or_nan(g, w)
    # 16-bit NaN items
    got = assemble_batch(ds.pool, ds.vols, d_table, 0, 23, (16, 16), dtype=torch.bfloat16)
    assert torch.equal(torch.isnan(got[0]).cpu(), torch.from_numpy(np.isnan(T.assemble_batch(pool, vols, table, 0, 23, 4, 16, 16)[0])))


def test_host_checks_raise_before_any_launch():
    from afcm_amd import _lib
    from afcm_amd.torch_utils.ops.batch_ops import advance_cursor, assemble_batch
    ds = _device_set(np.uint8, (16, 16), 4)
    items = torch.from_numpy(T.shuffled_items(4)).cuda()
    out = (torch.full((2, 4, 16, 16), 7., device='cuda'), torch.full((2, 1, 16, 16), 7., device='cuda'), torch.full((2, 1), 7., device='cuda'))
    lib = _lib.load()

    def call(**edit):
        args = dict(a=out[0].data_ptr(), b=out[1].data_ptr(), slice_idx=out[2].data_ptr(), pool=ds.pool.data_ptr(), pool_elems=ds.pool.numel(),
                    src_dtype=_lib.SRC_U8, vols=ds.vols.data_ptr(), n_vols=6, items=items.data_ptr(), n_items=23, cursor=None, first=0, count=2, k=4,
                    h=16, w=16, out_dtype=_lib.F32, min_value=0., max_value=255., stream=_lib.stream_ptr(ds.pool))
        args.update(edit)
        rc = lib.afcm_batch_assemble(*args.values())
        return rc, lib.afcm_last_error().decode()

    for edit, message in [(dict(a=None), 'null output'), (dict(b=None), 'null output'), (dict(slice_idx=None), 'null output'), (dict(pool=None), 'null output'),
                          (dict(vols=None), 'null output'), (dict(items=None), 'null output'), (dict(src_dtype=4), 'source dtype 4'),
                          (dict(src_dtype=-1), 'source dtype -1'), (dict(out_dtype=3), 'output dtype 3'), (dict(count=0), 'every extent must be positive'),
                          (dict(h=0), 'every extent must be positive'), (dict(w=-1), 'every extent must be positive'),
                          (dict(n_vols=0), 'every extent must be positive'), (dict(n_items=0), 'every extent must be positive'),
                          (dict(pool_elems=0), 'every extent must be positive'), (dict(first=-1), 'first row -1 is negative'),
                          (dict(k=2), 'slice number 2 is not 1 or 4'), (dict(max_value=0.), 'is not above min_value'),
                          (dict(count=2 ** 31 - 1, h=2 ** 20, w=2 ** 20), 'workgroups exceed the grid')]:
        rc, error = call(**edit)
        assert rc == _lib.E_INVALID and message in error, (edit, rc, error)
    assert lib.afcm_cursor_advance(None, 1, _lib.stream_ptr(ds.pool)) == _lib.E_INVALID and 'null cursor' in lib.afcm_last_error().decode()
    assert call()[0] == 0                                   # the unedited call is a good one
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out[0]).any()) and float(out[0].max()) <= 1.

    for t in out:
        t.fill_(7.)
    with pytest.raises(RuntimeError, match='is not above min_value'):
        assemble_batch(ds.pool, ds.vols, items, 0, 2, (16, 16), min_value=1., max_value=1., out=out)
    with pytest.raises(RuntimeError, match='slice number 2'):
        assemble_batch(ds.pool, ds.vols, items, 0, 2, (16, 16), slice_num=2, out=out)
    with pytest.raises(RuntimeError, match='no CPU'):
        assemble_batch(ds.pool, ds.vols, items.cpu(), 0, 2, (16, 16), out=out)
    with pytest.raises(RuntimeError, match='no CPU'):
        assemble_batch(ds.pool, ds.vols, items, 0, 2, (16, 16), out=out, cursor=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(RuntimeError, match=r'out A must be a contiguous torch.float16'):
        assemble_batch(ds.pool, ds.vols, items, 0, 2, (16, 16), dtype=torch.float16, out=out)
    with pytest.raises(RuntimeError, match=r'out B must be a contiguous torch.float32 \(3, 1, 16, 16\)'):
        assemble_batch(ds.pool, ds.vols, items, 0, 3, (16, 16), out=(torch.zeros(3, 4, 16, 16, device='cuda'), out[1], out[2]))
    with pytest.raises(RuntimeError, match='are not inside the loaded epoch of 0'):
        ds.batch(0, 2)
    ds.load_epoch(T.shuffled_items(4)[:10])
    with pytest.raises(RuntimeError, match=r'rows \[8, 11\) are not inside the loaded epoch of 10'):
        ds.batch(8, 3)
    with pytest.raises(RuntimeError, match='do not fit the device table of 23'):
        ds.load_epoch(np.zeros((24, 4), dtype=np.int32))
    with pytest.raises(RuntimeError, match=r'int32 \[n, 4\]'):
        ds.load_epoch(np.zeros((4, 4), dtype=np.int64))
    with pytest.raises(RuntimeError, match='cursor must be an int64'):
        advance_cursor(torch.zeros(1, dtype=torch.int32, device='cuda'), 1)
    assert all(bool((t == 7.).all()) for t in out)          # nothing was launched


TINY = dict(channel_base=256, channel_max=8, num_layers=14, num_critical=2, margin_size=10, output_scale=0.25, skip_resolution=128, conv_kernel=3,
            filter_size=6, lrelu_upsampling=2, use_radial_filters=False, conv_clamp=256, magnitude_ema_beta=0.5 ** (16 / 20e3), cond_mod=True)


def _tiny_step(compute_dtype=torch.float32, **kw):
    """The 128^2 generator of tests/golden/G1_tiny128.npz in a generator step."""
    from afcm_amd.networks_stylegan3 import Stylegan3Generator
    from afcm_amd.stylegan3_model import StyleGAN3GeneratorStep
    g = load_golden('G1_tiny128')
    G = Stylegan3Generator(z_dim=32, c_dim=1, w_dim=32, img_resolution=128, img_channels_in=4, img_channels_out=1, mapping_kwargs=dict(num_layers=2),
                           synthesis_kwargs=dict(TINY, compute_dtype=compute_dtype)).eval()
    G.load_state_dict({k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith('sd/')}, strict=True)
    return StyleGAN3GeneratorStep(G.cuda(), lr_G=0.0025, lambda_L1=100.0, **kw)


def _tiny_set():
    """Two uint8 subjects of (9, 120, 140) into 128 x 128 (a pad in y, a crop in x), thickness 5; an epoch table of 18 rows."""
    from afcm_amd.training import DeviceSliceSet
    zz, yy, xx = np.meshgrid(np.linspace(-1, 1, 9), np.linspace(-1, 1, 120), np.linspace(-1, 1, 140), indexing='ij')
    sources = []
    for s in range(2):
        body = np.clip(1.2 - (zz ** 2 * 0.3 + yy ** 2 + xx ** 2), 0, 1)
        sources.append({'t1': np.round(body * (0.6 + 0.4 * np.sin(7 * xx + s) * np.cos(5 * yy + zz)) * 255).astype(np.uint8),
                        't2': np.round(body * (0.5 + 0.5 * np.cos(4 * xx - s) * np.sin(6 * yy + zz)) * 255).astype(np.uint8)})
    ds = DeviceSliceSet(sources, patch_shape=(1, 128, 128), raw_internal_path_in=['t1'], raw_internal_path_out=['t2'], thickness=[5], device='cuda')
    return ds, ds.epoch_items(11)


def _state(step):
    st = step.optimizer_G.state
    out = [p.detach().clone() for p in step.netG.parameters()]
    out += [st[p][name].clone() for p in step.netG.parameters() if p in st for name in ('exp_avg', 'exp_avg_sq')]
    if step.netG_ema is not None:
        out += [p.detach().clone() for p in step.netG_ema.parameters()]
    return out


def test_train_epoch_device_and_host_arms_leave_the_same_bits(monkeypatch):
    from afcm_amd.training import train_epoch
    from test_gpu_volume import _counting
    ds, items = _tiny_set()
    assert len(ds) == 18 and items.shape == (18, 4)
    finals, copies = {}, []
    for where in ('device', 'host'):
        step = _tiny_step(ema=True)
        before = _state(step)
        torch.manual_seed(3)                                # set_input draws gen_z: the same draws for both arms
        if where == 'device':
            _counting(monkeypatch, copies)
        total = train_epoch(step, ds, 4, items[:12], total_iters=100, ema_kimgs=10.0, ramp=0.05, where=where)
        if where == 'device':
            monkeypatch.undo()
            assert copies == [], copies                     # no device -> host copy, no scalar read inside the loop
        assert total == 112
        finals[where] = _state(step)
        assert len(finals[where]) > len(list(step.netG.parameters())) * 3 - 1
        assert any(not torch.equal(a, b) for a, b in zip(finals[where], before))       # the steps did train
        assert all(bool(torch.isfinite(t).all()) for t in finals[where])
    assert len(finals['device']) == len(finals['host'])
    for a, b in zip(finals['device'], finals['host']):
        assert torch.equal(a, b)
    # a ragged epoch: 18 rows in batches of 4 are five steps, the last one of 2
    step = _tiny_step()
    assert train_epoch(step, ds, 4, items, where='device') == 20


def test_training_graph_replays_equal_eager_steps():
    """Three warm-up steps and three replays against six eager steps on the same rows and the same ``gen_z``: a capture records the step without
    running it, the warm-up runs real ones (as tests/test_gpu_optim.py counts them for ``capture_step``).  The generator computes in bfloat16, as in
    that test: with float32 compute a replayed step is not bit-identical to an eager one even through ``capture_step`` on fixed inputs (71 of the 98
    parameters differ by up to 6e-8 after three replays, measured on the MI355X; the fed graph differs from eager by the same order there, and its
    batches are the right ones), so equal bits cannot be asked of the float32 step; in bfloat16 both graphs equal eager."""
    from afcm_amd.training import TrainingGraph, train_epoch
    ds, items = _tiny_set()
    items = items[:12]
    z = torch.randn(4, 32, generator=torch.Generator().manual_seed(9)).cuda()
    eager = _tiny_step(compute_dtype=torch.bfloat16, capturable=True)
    for _ in range(2):                                      # the rows the warm-up consumes, then the rows of the replays: the same twelve
        train_epoch(eager, ds, 4, items, gen_z=z)
    want = [p.detach().clone() for p in eager.netG.parameters()]

    step = _tiny_step(compute_dtype=torch.bfloat16, capturable=True)
    ds.load_epoch(items)
    graph = TrainingGraph(step, ds, 4, warmup=3, fixed_z=True, gen_z=z)
    assert int(ds.cursor.cpu()) == 0 and ds.position == 0   # the warm-up leaves the cursor at row 0
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(ds.cursor.cpu()) == 12 and step.optimizer_G.device_step() == 6
    for a, b in zip(step.netG.parameters(), want):
        assert torch.equal(a.detach(), b)
    assert all(bool(torch.isfinite(p).all()) for p in want)
    with pytest.raises(RuntimeError, match='0 rows remain of an epoch of 12'):
        graph.replay()
    graph.load_epoch(items)                                 # refreshed in place: the graph goes on from row 0
    graph.replay()
    torch.cuda.synchronize()
    assert int(ds.cursor.cpu()) == 4
    fresh = ds.batch(0, 4)
    assert torch.equal(graph.real_A, fresh[0]) and torch.equal(graph.real_B, fresh[1]) and torch.equal(graph.slice_idx, fresh[2])
