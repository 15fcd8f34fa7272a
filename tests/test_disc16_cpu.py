"""The float64 references of test_gpu_disc16.py, checked on their own (no GPU, no compiled library): the rounding node, the case
lists, and the conditions the comparison rule needs from the references alone -- a non-zero E wherever the bar is computed from
it, leaky-ReLU branch disagreement between the two references below the cap, bias_act inputs outside their margins."""
import pytest
import torch

import disc16_ref as R
from conftest import load_golden


@pytest.mark.parametrize('dtype', R.DTYPES, ids=str)
def test_rounding_node_is_idempotent_exact_and_twice_differentiable(dtype):
    torch.manual_seed(0)
    x = torch.randn(257, dtype=torch.float64).requires_grad_(True)
    y = R.rnd(x, dtype)
    assert torch.equal(y, y.to(dtype).double())                       # representable
    assert torch.equal(R.rnd(y, dtype), y)                            # idempotent
    assert not torch.equal(y, x)                                      # and it does round
    rep = R.randn16([257], dtype, 1)                                  # a representable cotangent comes back unchanged ...
    raw = torch.randn(257, dtype=torch.float64)                       # ... any other is rounded
    for ct, want in ((rep, rep), (raw, R.quantize(raw, dtype))):
        ct = ct.clone().requires_grad_(True)
        g, = torch.autograd.grad(y, x, ct, create_graph=True)
        assert torch.equal(g, want)
        # the backward of that backward: the cotangent of g flows to ct through the node again
        for ct2, want2 in ((rep, rep), (raw, R.quantize(raw, dtype))):
            gg, = torch.autograd.grad(g, ct, ct2, retain_graph=True)
            assert torch.equal(gg, want2)
    # composed under create_graph: d/dw of sum (d<rnd(w x), r>/dx)^2 is the gradient of rounded values
    w = torch.tensor(1.2345678, dtype=torch.float64, requires_grad=True)
    g, = torch.autograd.grad(R.rnd(w * x, dtype).sum(), x, create_graph=True)
    h, = torch.autograd.grad(g.square().sum(), w)
    assert torch.isfinite(h) and h != 0


def test_stride2_cases_cover_the_tile_shapes_they_name():
    tiles = []
    for cid, n, cin, cout, h, w, want in R.DOWN3:
        p, q = R.down_out(h), R.down_out(w)
        tile = R.choose_tile_s2(p, q)
        assert tile == want, (cid, (p, q), tile)
        tiles.append((cid, p, q) + tile)
    assert any(tw == 2 for *_, tw in tiles) and any(tw == 64 for *_, tw in tiles) and any(tw % 8 for *_, tw in tiles)
    assert any(q % tw and not p % th for _, p, q, th, tw in tiles)            # ragged last tile in x only
    assert any(p % th and not q % tw for _, p, q, th, tw in tiles)            # in y only
    assert any(p % th and q % tw for _, p, q, th, tw in tiles)                # in both
    assert any(p < 128 // tw for _, p, q, th, tw in tiles)                    # plane shorter than the tile could be
    assert {5, 37} <= {c[2] for c in R.DOWN3} and {1, 127, 128, 129, 200} <= {c[3] for c in R.DOWN3}
    assert any(c[4] % 2 for c in R.DOWN3)
    assert sorted(h + 1 + ((h + 1) & 1) for _, _, _, _, h, _, _ in R.DOWN3[:4]) == [34, 66, 130, 258]      # blurred production widths
    for cid, n, cin, cout, h, w, pad, one_tap in R.S2:
        fh, fw = h + 2 * pad - 2, w + 2 * pad - 2
        p, q = (h + 2 * pad - 3) // 2 + 1, (w + 2 * pad - 3) // 2 + 1
        assert one_tap == (fw % 2 == 0 and q % 2 == 0), cid
        if one_tap:
            assert fw - 2 * q == 0 and fh - 2 * p == (-1 if fh % 2 else 0), cid
    assert {(c[6], c[7]) for c in R.S2} >= {(1, True), (2, True), (0, False), (2, False)}
    assert any(c[7] and (c[4] + 2 * c[6]) % 2 for c in R.S2) and any(c[7] and not (c[4] + 2 * c[6]) % 2 for c in R.S2)


@pytest.mark.parametrize('dtype', R.DTYPES, ids=str)
def test_bias_act_inputs_leave_no_element_inside_the_margins(dtype):
    for case in R.BIAS_ACT:
        cid, shape, act, gain, clamp, with_b = case
        x, b = R.bias_act_inputs(case, dtype)
        assert tuple(x.shape) == shape and torch.equal(x, R.quantize(x, dtype))
        kink, edge = R.bias_act_margins(x, b, act, gain, clamp, dtype)
        assert not bool(kink.any()) and not bool(edge.any()), cid
        if clamp is not None and clamp < 10:
            y = R.ops.bias_act(x, b, act=act, gain=gain, clamp=clamp)
            assert 0.05 < float((y.abs() >= clamp).double().mean()) < 0.6, cid        # the clamp bites


def _nonzero_E(p, e, rules, what):
    for k, rule in rules.items():
        if rule == 'e4':
            assert float((e[k] - p[k]).abs().max()) > 0, (what, k, 'E = 0: a rounding node is missing')


@pytest.mark.parametrize('dtype', R.DTYPES, ids=str)
def test_references_of_one_conv_case_differ_wherever_the_bar_comes_from_E(dtype):
    for mode, (n, cin, cout, h, w), pad in (('down3', R.DOWN3[-1][1:6], 0), ('s2', R.S2[-1][1:6], R.S2[-1][6]), ('down1', R.PLAIN[-1][2:], 0)):
        ks = 1 if mode.endswith('1') else 3
        fn = R.conv_reference(mode, pad)
        lv = R.conv_inputs(dtype, 7, n, cin, cout, h, w, ks)
        with torch.no_grad():
            shape = fn(lv, R.Lowp(dtype, False)).shape
        r, q = R.cotangents(dtype, 7, shape, lv['x'].shape)
        p, e, _ = R.both_references(fn, lambda: lv, 'x', ['w'], r, q, dtype)
        _nonzero_E(p, e, R.conv_rules(mode), mode)


@pytest.mark.parametrize('dtype', R.DTYPES, ids=str)
@pytest.mark.parametrize('case', R.BLOCKS, ids=lambda c: c[0])
def test_references_of_the_blocks_differ_and_agree_on_branches(case, dtype):
    fn = R.block_reference(case)
    sd, x = R.block_state(case), R.block_input(case, dtype)
    leaves = lambda: dict(sd, x=x)
    with torch.no_grad():
        shape = fn(leaves(), R.Lowp(dtype, False)).shape
    r, q = R.cotangents(dtype, 11, shape, x.shape)
    p, e, (lp, le) = R.both_references(fn, leaves, 'x', list(sd), r, q, dtype)
    _nonzero_E(p, e, {k: R.chain_rule(p, e, k) for k in p}, case[0])
    assert [k for k in p if R.chain_rule(p, e, k) == 'zero'] == [f'{t}/d{k}' for t in ('sq', 'q') for k in sd if k.endswith('bias')]
    for layer in [k for k in R.BLOCK_LAYERS if case[2] == 0 or k != 'fromrgb']:
        assert R.sign_share(le.trace[f'b.{layer}.'], lp.trace[f'b.{layer}.']) < R.SIGN_SHARE_CAP, layer


@pytest.mark.parametrize('dtype', R.DTYPES, ids=str)
def test_references_of_the_network_differ_and_agree_on_branches(dtype):
    g = load_golden(R.NETWORK)
    p, e, (lp, le) = R.network_references(g, dtype)
    _nonzero_E(p, e, {k: R.chain_rule(p, e, k) for k in p}, R.NETWORK)
    assert all(k.startswith('gr1/') and k.endswith('bias') for k in p if R.chain_rule(p, e, k) == 'zero')
    assert set(lp.trace) == set(le.trace) and len(lp.trace) == 3 * 5 + 1 + 1 and len(lp.passes) == len(le.passes) == 3
    wide = {}
    for n_pass in range(3):
        for k in lp.passes[n_pass]:
            if not k.endswith('skip.'):
                po, eo = lp.passes[n_pass][k], le.passes[n_pass][k]
                share = R.sign_share(eo, po)
                assert R.branch_allowance(po, eo) == min(share, R.SIGN_SHARE_CAP) + 2.0 / eo.numel() <= R.SIGN_SHARE_CAP + 2.0 / eo.numel()
                if share >= R.SIGN_SHARE_CAP:
                    wide[(n_pass, k)] = round(share * 1e3, 2)
    assert wide == R.NETWORK_WIDE[dtype], wide          # where the references alone exceed the cap: the allowance is the cap there


def test_network_factor_follows_the_cotangent():
    """Which gradients a flipped branch decision reaches (disc16_ref.network_factor)."""
    none = {0: [], 1: [], 2: []}
    assert all(R.network_factor(k, none) == R.E_FACTOR for k in ('real_logits', 'r1_grads', 'g_img', 'gr1/b4.out.weight', 'greal/b128.conv0.bias'))
    f = {0: [], 1: ['b16.conv0.'], 2: []}
    hit = {k for k in ('real_logits', 'gen_logits', 'r1_grads', 'g_img', 'gr1/b4.out.weight', 'gfake/b128.conv0.weight', 'greal/b128.fromrgb.bias',
                       'greal/b64.skip.weight', 'greal/b16.conv0.weight', 'greal/b16.skip.weight', 'greal/b16.conv1.bias', 'greal/b8.conv0.weight',
                       'greal/b4.fc.weight') if R.network_factor(k, f) == R.BRANCH_FLIP_FACTOR}
    assert hit == {'r1_grads', 'gr1/b4.out.weight', 'greal/b128.fromrgb.bias', 'greal/b64.skip.weight', 'greal/b16.conv0.weight'}
    assert R.BRANCH_FLIP_FACTOR <= 1.0
