"""afcm_plane_metrics on the GPU: the kernel's [planes, 8] float64 table against the numpy table of tests/plane_metrics_ref.py.

Inputs are seeded, in [0, 1], prediction = target + N(0, 0.05) clipped.  Shapes are the smallest at which a tile seam, an apron or a stride
can go wrong with the kernel's 64 x 64 tiles: one window (7 x 7), one row / column of windows (7 x 40, 40 x 7), an odd small plane (8 x 23),
a plane that crosses the tile in both directions by a non-multiple with seams inside windows (71 x 133), and the workload's own 256 x 256.

Tolerance, relative to the float64 table: columns 0-3 exact (extrema of exactly converted values); columns 4-7 within 1e-12 -- float64 sums
of <= 65 536 non-negative terms in another order differ by about N 2^-53 at worst (7e-12 is the worst case, rounding errors of random sign
stay orders below: two float64 summation orders of the SSIM mean differed by <= 3e-15 over these shapes on the CPU); an fp32-moment variant
differed by 1.7e-9 on noise and more on flat regions, which is why the kernel computes in float64."""
import numpy as np
import pytest
import torch

import plane_metrics_ref as R

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
REL = 1e-12
_CACHE = {}


def _pair(planes, h, w):
    """(target, prediction) float32 numpy + the float64 reference table, computed once per shape."""
    key = (planes, h, w)
    if key not in _CACHE:
        real, fake = R.noisy_pair((planes, h, w), seed=planes * 100003 + h * 1009 + w)
        _CACHE[key] = (real, fake, R.table(real, fake))
        for a in _CACHE[key]:
            a.setflags(write=False)
    return _CACHE[key]


def _check(got, want, what=''):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.array_equal(got[:, :4], want[:, :4]), (what, got[:, :4], want[:, :4])
    rel = np.abs(got[:, 4:] - want[:, 4:]) / np.maximum(np.abs(want[:, 4:]), 1e-300)
    print(f'{what}: max relative error of columns 4-7 = {rel.max(0)}')
    assert (rel <= REL).all(), (what, rel.max(0))


def _stats(*a, **k):
    from afcm_amd.torch_utils.ops.plane_metrics import plane_stats
    return plane_stats(*a, **k)


@pytest.mark.parametrize('planes', [1, 5])
@pytest.mark.parametrize('h,w', [(7, 7), (7, 40), (40, 7), (8, 23), (71, 133)])
def test_table_matches_float64_numpy(planes, h, w):
    real, fake, want = _pair(planes, h, w)
    _check(_stats(torch.tensor(real).cuda(), torch.tensor(fake).cuda()), want, f'{planes} x {h} x {w}')


def test_workload_plane_256():
    real, fake, want = _pair(1, 256, 256)
    _check(_stats(torch.tensor(real).cuda(), torch.tensor(fake).cuda()), want, '1 x 256 x 256')


@pytest.mark.parametrize('dt_test', DTYPES, ids=str)
@pytest.mark.parametrize('dt_ref', DTYPES, ids=str)
def test_all_dtype_pairs(dt_ref, dt_test):
    """The kernel converts each input exactly, so the reference is the float64 table of the ROUNDED inputs."""
    real, fake, _ = _pair(5, 8, 23)
    r, t = torch.tensor(real).to(dt_ref), torch.tensor(fake).to(dt_test)
    _check(_stats(r.cuda(), t.cuda()), R.table(r.double().numpy(), t.double().numpy()), f'{dt_ref} / {dt_test}')


@pytest.mark.parametrize('h,w', [(8, 23), (71, 133)])
@pytest.mark.parametrize('dt', [torch.float32, torch.float16], ids=str)
def test_unit_map_is_to_unit_range_bit_for_bit(h, w, dt):
    from afcm_amd.evaluation import to_unit_range
    real, fake, _ = _pair(5, h, w)
    # network range, overshooting both ends so that the clip acts, with values whose (x + 1) and / 2 both round
    r = (torch.tensor(real) * 2.2 - 1.1).to(dt)
    t = (torch.tensor(fake) * 2.2 - 1.1).to(dt)
    rn, tn = to_unit_range(r.float().numpy()), to_unit_range(t.float().numpy())
    assert rn.dtype == np.float32 and rn.min() == 0.0 and rn.max() == 1.0
    got = _stats(r.cuda(), t.cuda(), unit_map=True)
    _check(got, R.table(rn, tn), f'unit_map {dt} {h} x {w}')
    assert np.array_equal(R.table(r.float().numpy(), t.float().numpy(), map_to_unit=True), R.table(rn, tn))


def test_unit_map_elementwise_bits():
    """Every mapped value on its own: plane p is 0 everywhere except one pixel, so max t of plane p IS the mapped value of that pixel
    (mapped values are >= 0), compared bit for bit with ``to_unit_range``."""
    from afcm_amd.evaluation import to_unit_range
    rng = np.random.default_rng(11)
    vals = np.concatenate([rng.uniform(-1.2, 1.2, 500), [-1.0, 1.0, 0.0, -0.99999994, 0.99999994, 1e-8, -1e-8]]).astype(np.float32)
    x = np.full((len(vals), 7, 7), -1.0, dtype=np.float32)
    x[:, 3, 4] = vals
    g = _stats(torch.tensor(x).cuda(), torch.tensor(x).cuda(), unit_map=True).cpu().numpy()
    assert np.array_equal(g[:, 2], to_unit_range(vals).astype(np.float64))
    assert np.array_equal(g[:, 0], g[:, 2]) and (g[:, 1] == 0).all() and (g[:, 4] == 0).all()


def test_strided_axis_slicings_of_a_volume_are_read_in_place():
    real, fake = R.noisy_pair((8, 9, 10), seed=77)
    r, t = torch.tensor(real).cuda(), torch.tensor(fake).cuda()
    for perm in ((0, 1, 2), (1, 0, 2), (2, 0, 1)):
        rv, tv = r.permute(*perm), t.permute(*perm)
        assert rv.data_ptr() == r.data_ptr()
        want = R.table(np.ascontiguousarray(real.transpose(perm)), np.ascontiguousarray(fake.transpose(perm)))
        _check(_stats(rv, tv), want, f'axis {perm[0]}')
    # and two different layouts in one call: a column-strided target (every second column of a wider tensor) against a dense prediction
    wide = torch.zeros(8, 9, 20, device='cuda')
    wide[:, :, ::2] = r
    _check(_stats(wide[:, :, ::2], t), R.table(real, fake), 'column stride 2')


def test_two_calls_give_identical_bits():
    real, fake, _ = _pair(5, 71, 133)
    r, t = torch.tensor(real).cuda(), torch.tensor(fake).cuda()
    a = _stats(r, t)
    torch.empty(1 << 20, device='cuda').normal_()         # other work (and other workspace addresses) in between
    b = _stats(r, t)
    assert torch.equal(a, b)


def test_capturable_into_a_graph():
    real, fake, want = _pair(5, 71, 133)
    r, t = torch.tensor(real).cuda(), torch.tensor(fake).cuda()
    eager = _stats(r, t)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _stats(r, t)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    t.copy_(r)                                            # replays read the inputs as they are NOW
    graph.replay()
    torch.cuda.synchronize()
    assert (out[:, 4:7] == 0).all() and torch.equal(out[:, 0], eager[:, 0])


def test_plane_smaller_than_the_window_raises_with_the_c_message():
    x = torch.zeros(2, 6, 9, device='cuda')
    with pytest.raises(RuntimeError, match='smaller than the 7 x 7 SSIM window'):
        _stats(x, x)
    with pytest.raises(RuntimeError, match='smaller than the 7 x 7 SSIM window'):
        _stats(x.transpose(1, 2), x.transpose(1, 2))
    with pytest.raises(RuntimeError, match='one shape'):
        _stats(torch.zeros(2, 8, 9, device='cuda'), torch.zeros(2, 9, 8, device='cuda'))


def test_device_metrics_match_the_host_functions():
    """evaluation_device.* = kernel + finisher, against evaluation.* on float64 host copies (PSNR 1e-9 dB, SSIM 1e-10, MAE 2e-6 relative)."""
    from afcm_amd import evaluation as E, evaluation_device as D
    real, fake = R.noisy_pair((8, 9, 10), seed=78)
    real[3] = fake[3] = 0.25
    r, t = torch.tensor(real).cuda(), torch.tensor(fake).cuda()
    r64, t64 = real.astype(np.float64), fake.astype(np.float64)
    fake2 = fake.copy()
    fake2[3] = fake[2]
    real2 = real.copy()
    real2[5] = 0.0
    cases = [(D.evaluate_one(t, r), E.evaluate_one(t64, r64)),
             (D.evaluate_slice(torch.tensor(fake2).cuda(), torch.tensor(real2).cuda()), E.evaluate_slice(fake2.astype(np.float64), real2.astype(np.float64))),
             (D.evaluate_2D(torch.tensor(fake2).cuda()[:, None, None], torch.tensor(real2).cuda()[:, None, None], from_network_range=False),
              E.evaluate_2D(fake2.astype(np.float64)[:, None, None], real2.astype(np.float64)[:, None, None]))]
    for got, want in cases:
        print(got, want)
        assert abs(got[0] - want[0]) <= 1e-9 and abs(got[1] - want[1]) <= 1e-10 and abs(got[2] - want[2]) <= 2e-6 * want[2]
