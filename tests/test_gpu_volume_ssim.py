"""afcm_volume_ssim on the GPU: the kernel's [volumes, d - 6] float64 layer sums against the numpy reference of tests/volume_ssim_ref.py, layer by layer.

Shapes are the smallest at which the kernel's 16 x 64 tiles of window origins, its 6-voxel apron or a stride can go wrong: one window (7, 7, 7), an odd
small volume (8, 9, 10), d in {7, 8, 13} crossed with h / w of TILE + 5 / + 6 / + 7 (one origin short of a full tile, exactly a full tile, the first
origin of the next tile), and two volumes of 2 x 2 tiles behind a volume stride that is not d h w.  The reference is fed the values the kernel loads
(16-bit tensors widened to float32, ``to_unit_range`` where ``unit_map`` is set).

Tolerances.  Noise and MR-like blob inputs: 1e-12 relative to the layer sum, the bound of the plane table's columns 4-7 (float64 sums of <= 65 536 terms
in another order differ by about N 2^-53 at worst).  Measured on the MI355X: see DESIGN section 8h.  Constant pairs: every window within the a-priori rounding
bound 8 x 343 x 2^-53 / c2 = 8.5e-11 relative of the closed form, hence a layer within that bound times its window count."""
import itertools

import numpy as np
import pytest
import torch

import volume_ref
import volume_ssim_ref as R

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
REL = 1e-12
TOL_PSNR_DB, TOL_SSIM, TOL_MAE_REL = 1e-9, 1e-10, 2e-6      # the finishers' bounds of tests/test_gpu_volume.py
PAIRS = {'noise': R.noise_pair, 'blob': R.blob_pair}
_CACHE = {}


def _layers(*a, **k):
    from afcm_amd.torch_utils.ops.volume_metrics import volume_ssim_layers
    return volume_ssim_layers(*a, **k)


def _tiles():
    from afcm_amd.torch_utils.ops.volume_metrics import TILE_X, TILE_Y
    return TILE_Y, TILE_X


def _pair(kind, shape):
    """(target, prediction) float32 numpy + the float64 reference layer sums, computed once per input and left unchanged."""
    key = (kind,) + tuple(shape)
    if key not in _CACHE:
        ref, test = PAIRS[kind](shape, seed=shape[0] * 100003 + shape[1] * 1009 + shape[2])
        _CACHE[key] = (ref, test, R.layer_sums(ref, test))
        for a in _CACHE[key]:
            a.setflags(write=False)
    return _CACHE[key]


def _check(got, want, what, ok=None):
    """``want`` [volumes, d - 6]; ``ok``: mask of the layers that are expected finite (the others must be NaN)."""
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, want.shape)
    ok = np.ones(want.shape, bool) if ok is None else ok
    assert np.isnan(got[~ok]).all() and np.isfinite(got[ok]).all(), (what, got)
    rel = np.abs(got[ok] - want[ok]) / np.abs(want[ok])
    print(f'{what}: max relative error of a layer sum = {rel.max():.3e}')
    assert (rel <= REL).all(), (what, rel.max())
    return rel.max()


def _edge_shapes():
    ty, tx = 16, 64                                         # asserted against the module's TILE_Y / TILE_X in the test: parametrisation runs without the package
    return [(7, 7, 7), (8, 9, 10)] + [(d, ty + dy, tx + dx) for d, dy, dx in itertools.product((7, 8, 13), (5, 6, 7), (5, 6, 7))]


@pytest.mark.parametrize('kind', sorted(PAIRS))
@pytest.mark.parametrize('shape', _edge_shapes(), ids=str)
def test_layer_sums_match_float64_numpy(shape, kind):
    assert _tiles() == (16, 64)
    ref, test, want = _pair(kind, shape)
    _check(_layers(torch.tensor(ref).cuda()[None], torch.tensor(test).cuda()[None]), want[None], f'{kind} {shape}')


@pytest.mark.parametrize('kind', sorted(PAIRS))
def test_two_volumes_of_two_by_two_tiles_behind_a_padded_volume_stride(kind):
    ty, tx = _tiles()
    d, h, w = 8, ty + 6 + 9, tx + 6 + 11
    first, second = _pair(kind, (d, h, w)), PAIRS[kind]((d, h, w), seed=99)
    refs, tests = np.stack([first[0], second[0]]), np.stack([first[1], second[1]])
    want = np.stack([first[2], R.layer_sums(second[0], second[1])])
    wide_r, wide_t = (torch.full((2, d + 1, h, w), float('nan'), device='cuda') for _ in range(2))
    wide_r[:, :d], wide_t[:, :d] = torch.tensor(refs).cuda(), torch.tensor(tests).cuda()
    r, t = wide_r[:, :d], wide_t[:, :d]
    assert r.stride(0) == (d + 1) * h * w != d * h * w
    _check(_layers(r, t), want, f'{kind} 2 x {(d, h, w)}')


@pytest.mark.parametrize('a,b', [(0.3, 0.7), (1.0, 1.0)])
@pytest.mark.parametrize('shape', [(7, 7, 7), (8, 22, 70), (13, 23, 71)], ids=str)
def test_constant_pairs_within_the_a_priori_rounding_bound(shape, a, b):
    fa, fb = float(np.float32(a)), float(np.float32(b))      # the values the kernel loads
    window = (2 * fa * fb + R.C1) / (fa * fa + fb * fb + R.C1)           # both variances and the covariance are zero: c2 cancels
    nwin = (shape[1] - 6) * (shape[2] - 6)
    got = _layers(torch.full((1,) + shape, a, device='cuda'), torch.full((1,) + shape, b, device='cuda')).cpu().numpy()
    assert got.shape == (1, shape[0] - 6)
    err = np.abs(got - nwin * window).max()
    print(f'constant {a} / {b} {shape}: layer sums within {err / (nwin * window):.3e} relative of {nwin} x {window!r} (bound {R.CONSTANT_WINDOW_BOUND:.2e})')
    assert err <= R.CONSTANT_WINDOW_BOUND * nwin * abs(window)


@pytest.mark.parametrize('dt_test', DTYPES, ids=str)
@pytest.mark.parametrize('dt_ref', DTYPES, ids=str)
def test_all_dtype_pairs(dt_ref, dt_test):
    ref, test, _ = _pair('noise', (8, 9, 10))
    r, t = torch.tensor(ref).to(dt_ref), torch.tensor(test).to(dt_test)
    want = R.layer_sums(r.float().numpy(), t.float().numpy())
    _check(_layers(r.cuda()[None], t.cuda()[None]), want[None], f'{dt_ref} / {dt_test}')


@pytest.mark.parametrize('dt', [torch.float32, torch.float16], ids=str)
def test_unit_map_on_and_off(dt):
    from afcm_amd.evaluation import to_unit_range
    ref, test, _ = _pair('noise', (8, 9, 10))
    r, t = (torch.tensor(ref) * 2.2 - 1.1).to(dt), (torch.tensor(test) * 2.2 - 1.1).to(dt)       # network range, overshooting: the clip acts
    rn, tn = to_unit_range(r.float().numpy()), to_unit_range(t.float().numpy())
    assert rn.min() == 0.0 and rn.max() == 1.0 and np.array_equal(rn, R.unit_map(r.float().numpy()))
    on = _layers(r.cuda()[None], t.cuda()[None], unit_map=True)
    off = _layers(r.cuda()[None], t.cuda()[None])
    _check(on, R.layer_sums(rn, tn)[None], f'unit_map on {dt}')
    _check(off, R.layer_sums(r.float().numpy(), t.float().numpy())[None], f'unit_map off {dt}')
    assert not torch.equal(on, off)


def test_strided_views_are_read_in_place():
    ref, test, want = _pair('noise', (8, 9, 10))
    # stored x-major, read through permute
    rx, tx = (torch.tensor(np.ascontiguousarray(a.transpose(2, 1, 0))).cuda() for a in (ref, test))
    rv, tv = rx.permute(2, 1, 0)[None], tx.permute(2, 1, 0)[None]
    assert rv.shape == (1, 8, 9, 10) and rv.stride()[1:] == (1, 8, 72) and rv.data_ptr() == rx.data_ptr()
    _check(_layers(rv, tv), want[None], 'x-major through permute')
    _check(_layers(rv, torch.tensor(test).cuda()[None]), want[None], 'x-major target, dense prediction')
    # channel 0 of a [C, D, H, W] tensor (the predictor's map): the other channels are never read
    maps = torch.full((3, 8, 9, 10), float('nan'), device='cuda')
    maps[0] = torch.tensor(test).cuda()
    _check(_layers(torch.tensor(ref).cuda()[None], maps[:1]), want[None], 'channel 0 of [C, D, H, W]')
    # every second voxel of a larger volume
    big_r, big_t = (torch.full((1, 16, 18, 20), float('nan'), device='cuda') for _ in range(2))
    big_r[:, ::2, ::2, ::2], big_t[:, ::2, ::2, ::2] = torch.tensor(ref).cuda(), torch.tensor(test).cuda()
    view = big_r[:, ::2, ::2, ::2]
    assert view.stride() == (16 * 18 * 20, 2 * 18 * 20, 2 * 20, 2)
    _check(_layers(view, big_t[:, ::2, ::2, ::2]), want[None], 'every second voxel')


@pytest.mark.parametrize('z', [0, 3, 8, 12])
def test_one_nan_voxel_poisons_exactly_the_layers_whose_windows_hold_it(z):
    ref, test, want = _pair('noise', (13, 9, 10))
    t = torch.tensor(test).cuda()
    t[z, 4, 5] = float('nan')
    ok = np.ones((1, 7), bool)
    ok[0, max(0, z - 6):min(z, 6) + 1] = False               # window origins z - 6 ... z, clipped to [0, d - 7]
    assert 1 <= (~ok).sum() <= 7
    _check(_layers(torch.tensor(ref).cuda()[None], t[None]), want[None], f'NaN at depth {z}', ok=ok)


def _two_tile_inputs():
    ty, tx = _tiles()
    ref, test, _ = _pair('noise', (8, ty + 15, tx + 17))
    return torch.tensor(ref).cuda()[None], torch.tensor(test).cuda()[None]


def test_two_calls_give_identical_bits():
    r, t = _two_tile_inputs()
    a = _layers(r, t)
    torch.empty(1 << 20, device='cuda').normal_()           # other work (and other workspace addresses) in between
    assert torch.equal(a, _layers(r, t))


def test_capturable_into_a_graph():
    r, t = _two_tile_inputs()
    eager = _layers(r, t)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _layers(r, t)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_argument_errors():
    from afcm_amd import _lib
    z = lambda *s: torch.zeros(*s, device='cuda')
    with pytest.raises(RuntimeError, match='smaller than the 7 x 7 x 7 SSIM window'):
        _layers(z(1, 6, 9, 9), z(1, 6, 9, 9))
    with pytest.raises(RuntimeError, match='smaller than the 7 x 7 x 7 SSIM window'):
        _layers(z(1, 9, 9, 6), z(1, 9, 9, 6))
    with pytest.raises(RuntimeError, match='one shape'):
        _layers(z(1, 8, 9, 10), z(1, 8, 10, 9))
    with pytest.raises(RuntimeError, match='one shape'):
        _layers(z(8, 9, 10), z(8, 9, 10))
    with pytest.raises(RuntimeError, match='no CPU'):
        _layers(z(1, 8, 9, 10), torch.zeros(1, 8, 9, 10))
    with pytest.raises(RuntimeError, match='float32/float16/bfloat16'):
        _layers(z(1, 8, 9, 10).double(), z(1, 8, 9, 10).double())
    # the raw ABI: a dtype code that does not exist, refused on the host with a message and nothing launched
    lib = _lib.load()
    x, out = z(1, 8, 9, 10), torch.full((1, 2), 7.0, dtype=torch.float64, device='cuda')
    ws = torch.empty(max(1, lib.afcm_volume_ssim_workspace_bytes(1, 8, 9, 10)), dtype=torch.uint8, device='cuda')
    assert lib.afcm_volume_ssim_workspace_bytes(1, 8, 9, 10) == 2 * 8 and lib.afcm_volume_ssim_workspace_bytes(1, 6, 9, 10) == 0
    for codes, message in (((3, 0), b'dtypes 3 / 0'), ((0, -1), b'dtypes 0 / -1')):
        rc = lib.afcm_volume_ssim(out.data_ptr(), x.data_ptr(), x.data_ptr(), *codes, 1, 8, 9, 10, *x.stride(), *x.stride(), 0, R.C1, R.C2, ws.data_ptr(),
                                  _lib.stream_ptr(x))
        assert rc == _lib.E_INVALID and message in lib.afcm_last_error()
    rc = lib.afcm_volume_ssim(out.data_ptr(), x.data_ptr(), x.data_ptr(), 0, 0, 0, 8, 9, 10, *x.stride(), *x.stride(), 0, R.C1, R.C2, ws.data_ptr(),
                              _lib.stream_ptr(x))
    assert rc == _lib.E_INVALID and b'0 volumes' in lib.afcm_last_error()
    torch.cuda.synchronize()
    assert (out == 7.0).all()


def _agree(name, got, want):
    print(f'{name}: device {got}')
    print(f'{name}: host   {want}')
    print(f'{name}: differences psnr {abs(got[0] - want[0]):.3e} dB, ssim {abs(got[1] - want[1]):.3e}, mae {abs(got[2] - want[2]) / want[2]:.3e} relative')
    assert abs(got[0] - want[0]) <= TOL_PSNR_DB
    assert abs(got[1] - want[1]) <= TOL_SSIM
    assert abs(got[2] - want[2]) <= TOL_MAE_REL * want[2]


def test_device_evaluate_3D_matches_the_host_function():
    from afcm_amd import evaluation as E, evaluation_device as D
    ty, tx = _tiles()
    for kind, shape in (('noise', (8, 9, 10)), ('blob', (13, ty + 7, tx + 7))):
        ref, test, _ = _pair(kind, shape)
        _agree(f'evaluate_3D {kind} {shape}', D.evaluate_3D(torch.tensor(test).cuda(), torch.tensor(ref).cuda()),
               E.evaluate_3D(test.astype(np.float64), ref.astype(np.float64)))
    ref, test, _ = _pair('noise', (8, 9, 10))
    r, t = torch.tensor(ref).cuda() * 2 - 1, torch.tensor(test).cuda() * 2 - 1
    _agree('evaluate_3D from the network range', D.evaluate_3D(t, r, from_network_range=True),
           E.evaluate_3D(E.to_unit_range(t.cpu().numpy()).astype(np.float64), E.to_unit_range(r.cpu().numpy()).astype(np.float64)))
    same = D.evaluate_3D(torch.tensor(ref).cuda(), torch.tensor(ref).cuda())
    assert same[0] == float('inf') and abs(same[1] - 1.0) <= TOL_SSIM and same[2] == 0.0
    with pytest.raises(ValueError, match='outside the range expected'):
        D.evaluate_3D(torch.tensor(test).cuda(), torch.tensor(ref).cuda() * 1.5)


class StubStep:
    """``fake_B`` is a fixed function of ``real_A`` and ``gen_c`` (the stub of tests/test_gpu_volume.py); no host read."""

    def set_test_input(self, real_A, slice_idx):
        self.real_A, self.gen_c = real_A.cuda(), slice_idx.cuda()
        self.gen_z = torch.randn([real_A.shape[0], 8], device='cuda')

    def test(self):
        self.fake_B = self.real_A[:, 0:1] * 0.5 - self.real_A[:, 2:3] * 0.25 + self.gen_c[:, :, None, None]


def _counting(monkeypatch, copies):
    """Counts device -> host copies and scalar reads the way tests/test_gpu_volume.py does."""
    cpu, to, item, tolist = torch.Tensor.cpu, torch.Tensor.to, torch.Tensor.item, torch.Tensor.tolist

    def counted_cpu(self, *a, **k):
        if self.is_cuda:
            copies.append(('cpu', tuple(self.shape)))
        return cpu(self, *a, **k)

    def counted_to(self, *a, **k):
        out = to(self, *a, **k)
        if self.is_cuda and not out.is_cuda:
            copies.append(('to', tuple(self.shape)))
        return out

    def scalar_read(name, fn):
        def wrapped(self, *a, **k):
            if self.is_cuda:
                copies.append((name, tuple(self.shape)))
            return fn(self, *a, **k)
        return wrapped
    monkeypatch.setattr(torch.Tensor, 'cpu', counted_cpu)
    monkeypatch.setattr(torch.Tensor, 'to', counted_to)
    monkeypatch.setattr(torch.Tensor, 'item', scalar_read('item', item))
    monkeypatch.setattr(torch.Tensor, 'tolist', scalar_read('tolist', tolist))


def test_evaluate_volume_with_3d_copies_once(monkeypatch):
    from afcm_amd import evaluation as E
    from afcm_amd.volume import evaluate_volume
    src = volume_ref.source((11, 30, 40), np.uint8, seed=8)                # the subject of test_gpu_volume.py::test_loop_with_a_stub_step
    kw = dict(raw_internal_path_in='raw', thickness=5, patch_hw=(32, 32), batch_size=4, patch_halo=(0, 4, 4))
    target = torch.from_numpy(volume_ref.assemble(volume_ref.source((11, 30, 40), np.uint8, seed=9), 0, 11, 1, None, 32, 32)[0][:, 0]).cuda()
    plain = evaluate_volume(StubStep(), {'raw': src}, target, **kw)
    assert '3d' not in plain
    copies = []
    _counting(monkeypatch, copies)
    out = evaluate_volume(StubStep(), {'raw': src}, target, with_3d=True, **kw)
    monkeypatch.undo()
    assert copies == [('cpu', ((11 + 32 + 32) * 8 + 11 - 6,))], copies       # the three tables and the layer sums, together, once; no scalar read
    assert out['slice'] == plain['slice'] and out['one'] == plain['one'] and torch.equal(out['prediction'], plain['prediction'])
    pred64 = E.to_unit_range(out['prediction'][0].cpu().numpy()).astype(np.float64)
    target64 = E.to_unit_range(target.cpu().numpy()).astype(np.float64)
    _agree('evaluate_volume 3d', out['3d'], E.evaluate_3D(pred64, target64))
