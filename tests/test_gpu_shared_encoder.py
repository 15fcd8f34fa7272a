"""Shared-encoder inference on the GPU: ``Stylegan3Generator.forward(cond_groups=...)`` (the encoder once per conditioning image, the state handed
to the decoder batch by ``afcm_group_expand``) against the same forward with the conditioning rows repeated; ``SynthesisNetwork.encode`` /
``decode`` against ``forward``; ``predict_volume(share_encoder=True)`` against ``share_encoder=False``; the refusals.

The equality bar.  Each sample's arithmetic should not depend on the batch it rides in, and the encoder's batch size (G instead of B) is all that
differs between the arms, so the comparisons are ``torch.equal``.  ``_bar`` asks the UNSHARED code whether that premise holds, never the grouped path:
  1. the whole-forward probe: ``forward`` on the first g rows against the first g rows of ``forward`` on all B rows, for every g the test uses.  On
     the MI355X it is NOT bit-equal, in any dtype (tiny 128^2: 1.8e-7 ... 2.7e-7 fp32, 7.3e-4 fp16, 5.9e-3 bf16).  The cause is no kernel switch: the
     reference's style pre-normalisation ``s * s.square().mean().rsqrt()`` (NET:43; the style-coefficient kernel, ``afcm_style_coefs_fwd`` / the
     modulation bank) takes its mean over the WHOLE batch, so a decoder sample's styles depend on its batch; the demodulation cancels the factor up to
     rounding.  Mapping network and encoder are bit-equal across batch sizes.
  2. so the probe that bears on this feature is the encoder's: ``encode`` on g rows against the first g rows of ``encode`` on B rows, every tensor of
     the state.  Both arms run the mapping network and the decoder at batch B; where the encoder probe is bit-equal, nothing is left that may
     differ, and the bar is 0 = ``torch.equal`` -- tighter than the whole-forward figure, which the issue's rule would allow.  Only where the encoder
     probe is not bit-equal does the bar become the whole-forward probe's max-abs difference."""
import numpy as np
import pytest
import torch

import volume_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

TINY = dict(channel_base=256, channel_max=8, num_layers=14, num_critical=2, margin_size=10, output_scale=0.25, skip_resolution=128, conv_kernel=3,
            filter_size=6, lrelu_upsampling=2, use_radial_filters=False, conv_clamp=256, magnitude_ema_beta=0.5 ** (16 / 20e3), cond_mod=True)

# groups of a batch of four: G = 1; G = B (the identity); a group that begins in the batch before (a straddling batch); non-monotone with repeats
PATTERNS = {'one_group': [0, 0, 0, 0], 'identity': [0, 1, 2, 3], 'straddling': [0, 1, 1, 1], 'non_monotone': [2, 0, 2, 1]}


def _tiny_G(compute_dtype):
    from afcm_amd.networks_stylegan3 import Stylegan3Generator
    g = load_golden('G1_tiny128')
    G = Stylegan3Generator(z_dim=32, c_dim=1, w_dim=32, img_resolution=128, img_channels_in=4, img_channels_out=1, mapping_kwargs=dict(num_layers=2),
                           synthesis_kwargs=dict(TINY, compute_dtype=compute_dtype)).eval()
    G.load_state_dict({k[3:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith('sd/')}, strict=True)
    return G.cuda()


@pytest.fixture(scope='module')
def G32():
    return _tiny_G(torch.float32)


def _inputs(seed=7, batch=4):
    g = torch.Generator(device='cuda').manual_seed(seed)
    z = torch.randn(batch, 32, generator=g, device='cuda')
    c = torch.rand(batch, 1, generator=g, device='cuda')
    a = torch.rand(batch, 4, 128, 128, generator=g, device='cuda') * 2 - 1
    return z, c, a


def _probe_forward(G, z, c, a_rows, sizes):
    """max |forward(first g rows) - forward(all rows)[:g]| over ``sizes``, from the unshared code alone; 0.0 = bit-equal for every g."""
    full = G(z, c, a_rows)
    worst = 0.0
    for g in sorted(set(sizes)):
        part = G(z[:g], c[:g], a_rows[:g])
        if not torch.equal(part, full[:g]):
            worst = max(worst, float((part - full[:g]).abs().max()))
            print(f'probe: forward on {g} rows differs from the first {g} of {len(z)} rows by {float((part - full[:g]).abs().max()):.3e}')
    return worst


def _probe_encoder(G, a_rows, sizes):
    """Is every tensor of ``encode``'s state on g rows bit-equal to the first g rows of the state on all rows, for every g of ``sizes``?"""
    S = G.synthesis
    full = S.encode(a_rows)
    same = True
    for g in sorted(set(sizes)):
        part = S.encode(a_rows[:g])
        pairs = [(part.x, full.x), (part.img_global, full.img_global)] + [(part.E_features[k], full.E_features[k]) for k in full.E_features]
        for p, f in pairs:
            if not torch.equal(p, f[:g]):
                same = False
                print(f'probe: the encoder state {tuple(p.shape)} on {g} rows differs from the first {g} of {len(a_rows)} rows')
    return same


def _bar(G, z, c, a_rows, sizes):
    """0.0 (``torch.equal``) where the encoder is bit-equal across the batch sizes met, else the whole-forward probe's figure (module docstring)."""
    forward = _probe_forward(G, z, c, a_rows, sizes)
    encoder_same = _probe_encoder(G, a_rows, sizes)
    print(f'probes on {sorted(set(sizes))} of {len(z)} rows: whole forward max-abs {forward:.3e}, encoder state {"bit-equal" if encoder_same else "DIFFERENT"}')
    return 0.0 if encoder_same else forward


def _assert_within(got, want, bar, what):
    diff = float((got - want).abs().max())
    print(f'{what}: max |shared - repeated| = {diff:.3e}, bar {bar:.3e}')
    if bar == 0.0:
        assert torch.equal(got, want), what
    else:
        assert diff <= bar, (what, diff, bar)


def _grouped_against_repeated(G, name):
    z, c, a = _inputs()
    groups = PATTERNS[name]
    n_groups = max(groups) + 1
    a_unique = a[:n_groups].contiguous()
    gdev = torch.tensor(groups, dtype=torch.int32, device='cuda')
    with torch.no_grad():
        a_rows = a_unique[gdev.long()]
        bar = _bar(G, z, c, a_rows, [n_groups])
        want = G(z, c, a_rows)
        got = G(z, c, a_unique, cond_groups=gdev)
    assert got.shape == want.shape == (4, 1, 128, 128) and got.dtype == want.dtype == torch.float32
    assert torch.isfinite(want).all()
    _assert_within(got, want, bar, name)


@pytest.mark.parametrize('name', sorted(PATTERNS))
def test_fp32_generator_grouped_equals_repeated(G32, name):
    _grouped_against_repeated(G32, name)


def test_encode_decode_is_forward(G32):
    z, c, a = _inputs(seed=8)
    S = G32.synthesis
    with torch.no_grad():
        ws = G32.mapping(z, c)
        want = S(ws, a, noise_mode='const')
        state = S.encode(a)
        assert torch.equal(S.decode(ws, state, noise_mode='const'), want)
        assert state.x.shape[0] == 4 and state.img_global.shape == (4, 1024) and len(state.E_features) >= 1
        identity = torch.arange(4, dtype=torch.int32, device='cuda')
        assert torch.equal(S.decode(ws, state, groups=identity, noise_mode='const'), want)     # the expansion as a plain copy
    ws_g = G32.mapping(z, c)                                 # with gradients, as in training: the re-cut forward is the forward
    y, y_forward = S.decode(ws_g, S.encode(a)), S(ws_g, a)
    assert y.requires_grad and torch.equal(y.detach(), y_forward.detach())


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('name', ['straddling', 'non_monotone'])
def test_16bit_generator_takes_the_row_pitched_path(monkeypatch, dtype, name):
    """The tiny 128^2 generator in 16 bits runs its layers as the fused node on row-pitched tensors (148-wide planes at a pitch of 160): the
    expanded skip maps must come out row-pitched too, or the comparison would pass without touching that path."""
    from afcm_amd import networks_stylegan3 as net
    from afcm_amd.torch_utils.ops import _rows
    G = _tiny_G(dtype)
    seen = []
    expand = net.group_ops.group_expand

    def recording(tensors, groups):
        out = expand(tensors, groups)
        seen.append((list(tensors), out))
        return out
    monkeypatch.setattr(net.group_ops, 'group_expand', recording)
    _grouped_against_repeated(G, name)
    assert len(seen) == 1                                    # one launch for the whole state
    sources, outs = seen[0]
    maps = [(s, o) for s, o in zip(sources, outs) if o.ndim == 4]
    pitched = [(s, o) for s, o in maps if _rows.pitch_of(o) != o.shape[3]]
    assert pitched, [(tuple(o.shape), o.stride()) for _, o in maps]
    for s, o in maps:
        assert _rows.pitch_of(o) == _rows.pitch_of(s) and o.shape[0] == 4 and o.dtype == dtype
    for _, o in pitched:                                     # finite padding, as every kernel that writes a pitched tensor leaves it
        assert torch.isfinite(_rows.whole_buffer(o).float()).all()


# ---- the loop --------------------------------------------------------------------------------------------------------------------------------

def _subject():
    """The MR-like (11, 120, 136) uint8 subject of tests/test_gpu_volume.py: a smooth bright blob on an exactly-zero background."""
    zz, yy, xx = np.meshgrid(np.linspace(-1, 1, 11), np.linspace(-1, 1, 120), np.linspace(-1, 1, 136), indexing='ij')
    body = np.clip(1.2 - (zz ** 2 * 0.3 + yy ** 2 + xx ** 2), 0, 1) * (0.6 + 0.4 * np.sin(7 * xx) * np.cos(5 * yy + zz))
    return body, np.round(body * 255).astype(np.uint8)


class GroupedStub:
    """A step that takes the group tables and uses them as the generator step does: ``fake_B`` is computed from the LEADERS' rows of ``real_A``
    spread by ``groups``, so it equals the ungrouped result only if every sample's group leader carries that sample's ``A``.  No host read."""

    def __init__(self):
        self.calls = []

    def set_test_input(self, real_A, slice_idx, groups=None, leaders=None):
        self.real_A, self.gen_c = real_A.cuda(), slice_idx.cuda()
        self.gen_z = torch.randn([real_A.shape[0], 8], device='cuda')
        self.groups, self.leaders = groups, leaders
        self.calls.append((real_A.shape[0], None if groups is None else (groups.dtype, tuple(groups.shape), leaders.dtype, tuple(leaders.shape))))

    def test(self):
        a = self.real_A if self.groups is None else self.real_A.index_select(0, self.leaders)[self.groups.long()]
        self.fake_B = a[:, 0:1] * 0.5 - a[:, -1:] * 0.25 + self.gen_c[:, :, None, None] + self.gen_z[:, :1, None, None]


def _counting(monkeypatch, copies, uploads):
    """Device -> host copies and scalar reads, counted as tests/test_gpu_volume.py::_counting counts them; host -> device copies in ``uploads``."""
    cpu, to, item, tolist = torch.Tensor.cpu, torch.Tensor.to, torch.Tensor.item, torch.Tensor.tolist

    def counted_cpu(self, *a, **k):
        if self.is_cuda:
            copies.append(('cpu', tuple(self.shape)))
        return cpu(self, *a, **k)

    def counted_to(self, *a, **k):
        out = to(self, *a, **k)
        if self.is_cuda and not out.is_cuda:
            copies.append(('to', tuple(self.shape)))
        if out.is_cuda and not self.is_cuda:
            uploads.append(tuple(self.shape))
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


LOOP_CASES = {
    # thickness 5, batch 4 over 11 slices: groups {0-4}, {5-9}, {10}: a single-group batch, a straddling batch, a ragged batch of two groups
    't5': (dict(thickness=5, slice_num=4), [1, 2, 2]),
    't2': (dict(thickness=2, slice_num=4), [2, 2, 2]),
    'one_slice': (dict(thickness=None, slice_num=1), [4, 4, 3]),
}


@pytest.mark.parametrize('case', sorted(LOOP_CASES))
def test_loop_tables_with_a_stub_step(monkeypatch, case):
    """Every case of the loop with a step that USES the tables (so wrong tables change the volume), both heads, and the copy counts."""
    from afcm_amd.volume import GroupTables, PatchPlan, predict_volume
    from afcm_amd.predictor import patch_indices
    opts, encoder_batches = LOOP_CASES[case]
    _, src = _subject()
    kw = dict(raw_internal_path_in='raw', patch_hw=(128, 128), batch_size=4, patch_halo=(0, 8, 8), heads=('prediction', 'input'), **opts)

    def arm(step, **more):
        torch.manual_seed(5)
        return predict_volume(step, {'raw': src}, **kw, **more)
    plain, shared = GroupedStub(), GroupedStub()
    want, got = arm(plain), arm(shared, share_encoder=True)
    for head in ('prediction', 'input'):
        assert got[head].is_cuda and got[head].shape == want[head].shape == (1, 11, 128, 128)
        assert torch.equal(got[head], want[head]), head
    assert [c[0] for c in shared.calls] == [c[0] for c in plain.calls] == [4, 4, 3]          # the batch partition does not change
    assert all(c[1] is None for c in plain.calls)
    assert [c[1][3][0] for c in shared.calls] == encoder_batches
    assert all(c[1][0] == torch.int32 and c[1][1] == (c[0],) and c[1][2] == torch.int64 for c in shared.calls)
    plan = PatchPlan((11, 128, 128), patch_indices((11, 128, 128), (1, 128, 128), (1, 1, 1)))
    assert GroupTables(plan, 4, opts['thickness'] if opts['slice_num'] == 4 else None, 'cuda').encoder_batches == encoder_batches

    copies, uploads, base_uploads = [], [], []
    _counting(monkeypatch, copies, base_uploads)
    arm(GroupedStub())
    monkeypatch.undo()
    _counting(monkeypatch, copies, uploads)
    arm(GroupedStub(), share_encoder=True)
    monkeypatch.undo()
    assert copies == [], copies                              # no device -> host copy and no scalar read in either arm
    assert len(uploads) == len(base_uploads) + 1, (uploads, base_uploads)   # the group tables of the whole volume: one upload


@pytest.fixture(scope='module')
def tiny_step(G32):
    from afcm_amd.stylegan3_model import StyleGAN3GeneratorStep
    return StyleGAN3GeneratorStep(G32, ema=True)


@pytest.mark.parametrize('case', ['t5', 't2'])
def test_loop_with_the_tiny_ema_generator(tiny_step, case):
    from afcm_amd.volume import predict_volume
    opts, _ = LOOP_CASES[case]
    _, src = _subject()
    kw = dict(raw_internal_path_in='raw', patch_hw=(128, 128), batch_size=4, patch_halo=(0, 8, 8), heads=('prediction', 'input'), **opts)

    def arm(**more):
        torch.manual_seed(3)                                # set_test_input draws gen_z: the same draws for both arms
        return predict_volume(tiny_step, {'raw': src}, **kw, **more)
    want, got = arm(), arm(share_encoder=True)
    assert tiny_step.test_groups is not None and tiny_step.test_groups.dtype == torch.int32
    # the premise of the equality bar, asked of the unshared code on the loop's own first batch, for every encoder batch size the loop meets
    from afcm_amd.torch_utils.ops.volume_ops import assemble_slices
    a, idx = assemble_slices(torch.from_numpy(src).cuda(), 0, 4, (1, 128, 128), thickness=opts['thickness'], slice_num=4)
    z = torch.randn(4, 32, generator=torch.Generator(device='cuda').manual_seed(1), device='cuda')
    with torch.no_grad():
        bar = _bar(tiny_step.netG_ema, z, idx, a, [1, 2])
    for head in ('prediction', 'input'):
        assert got[head].shape == want[head].shape == (1, 11, 128, 128) and torch.isfinite(want[head]).all()
        _assert_within(got[head], want[head], bar if head == 'prediction' else 0.0, f'{case} {head}')
    assert float(want['prediction'].std()) > 0


def test_evaluate_volume_inherits_share_encoder(tiny_step):
    from afcm_amd.volume import evaluate_volume
    body, src = _subject()
    target_src = np.round(np.clip(body * 1.1 + 0.03 * np.random.default_rng(2).standard_normal(body.shape), 0, 1) * 255).astype(np.uint8)
    target = torch.from_numpy(R.assemble(target_src, 0, 11, 1, None, 128, 128)[0][:, 0]).cuda()      # normalised as the loader normalises
    kw = dict(raw_internal_path_in='raw', thickness=5, patch_hw=(128, 128), batch_size=4, patch_halo=(0, 8, 8))
    torch.manual_seed(3)
    want = evaluate_volume(tiny_step, {'raw': src}, target, **kw)
    torch.manual_seed(3)
    got = evaluate_volume(tiny_step, {'raw': src}, target, share_encoder=True, **kw)
    assert torch.equal(got['prediction'], want['prediction'])
    assert got['slice'] == want['slice'] and got['one'] == want['one'] and all(np.isfinite(v) for v in got['slice'] + got['one'])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------

def test_refusals(G32, tiny_step):
    from afcm_amd.volume import evaluate_volume, predict_volume
    z, c, a = _inputs(seed=9)
    groups = torch.tensor([0, 1, 1, 1], dtype=torch.int32, device='cuda')
    S = G32.synthesis
    with torch.no_grad():
        ws = G32.mapping(z, c)
        state = S.encode(a[:2])
    with pytest.raises(RuntimeError, match='no_grad'):                       # gradients enabled
        G32(z, c, a[:2], cond_groups=groups)
    with pytest.raises(RuntimeError, match='no_grad'):
        S.decode(ws, state, groups=groups)
    with torch.no_grad():
        G32.train()
        try:
            with pytest.raises(RuntimeError, match='eval'):                  # training mode: dropout
                S.decode(ws, state, groups=groups)
        finally:
            G32.eval()
        with pytest.raises(RuntimeError, match='update_emas'):
            S.decode(ws, state, groups=groups, update_emas=True)
        for bad in (groups[:3], groups.long(), groups.float(), torch.cat([groups, groups])):
            with pytest.raises(RuntimeError, match='int32 tensor'):
                S.decode(ws, state, groups=bad)
        assert torch.isfinite(S.decode(ws, state, groups=groups)).all()     # and the module still works
    _, src = _subject()
    kw = dict(raw_internal_path_in='raw', thickness=5, patch_hw=(128, 128), batch_size=4, patch_halo=(0, 8, 8))
    with pytest.raises(ValueError, match="where='device'"):
        predict_volume(tiny_step, {'raw': src}, where='host', share_encoder=True, **kw)
    with pytest.raises(ValueError):
        evaluate_volume(tiny_step, {'raw': src}, torch.zeros(11, 128, 128, device='cuda'), where='host', share_encoder=True, **kw)
    with pytest.raises(RuntimeError, match='come together'):
        tiny_step.set_test_input(a, c, groups=groups)
    with pytest.raises(RuntimeError, match='groups must be int32'):
        tiny_step.set_test_input(a, c, groups=groups.long(), leaders=torch.tensor([0, 1], device='cuda'))
    with pytest.raises(RuntimeError, match='leaders must be int64'):
        tiny_step.set_test_input(a, c, groups=groups, leaders=torch.tensor([0, 1], dtype=torch.int32, device='cuda'))
