"""The yardstick of tests/test_gpu_generator_grad16.py, proven without a GPU (tests/gen16_grad_ref.py): the oracle's `store` hook and
the imposed codes change nothing by themselves, the code conversion round-trips through the three sign-tensor layouts, and the
criterion RESOLVES a wiring error: the exact oracle with the cotangent entering one layer's output multiplied by s (what a wrong style
factor on one arm, or a <g, z> handed to the wrong layer, does) is graded as if it were the device and must be rejected.

Resolution (default, batch 2; measured).  Gradients are linear in the injected factor, so each place has a smallest s that the criterion
rejects, 1 + (s - 1) / max_k (err[k] / bound[k]):

    place                                        f16 yardstick    bf16 yardstick
    encoder_5  (its output is also L8's skip)    1.010            1.067
    encoder_12 (deep encoder)                    1.010            1.067
    L4_52_8    (decoder)                         1.010            1.110
    (with the HBM tensors alone in the yardstick, gen16_grad_ref.storage(internal=False): 1.004 - 1.008 and 1.053 - 1.059)

The test asserts the bars set in advance: s = 1.05 is rejected under the f16 yardstick and s = 1.25 under the bf16 one, at every place; it
prints the figures above.  s = 1.05 at a layer moves every parameter upstream of it by 5.0e-2 and the encoder through the skip by 1 - 5e-2.
"""
import numpy as np
import pytest
import torch

import flrelu_read_ref as R
import gen16_grad_ref as H

PLACES = ['encoder_5', 'encoder_12', 'L4_52_8']
_CACHE = {}


def _shared(case='default-b2'):
    """The device-independent runs of a case, once per session: the oracle on its own decisions (with its pre-activations), its own
    codes, the exact oracle with those imposed and the two storage-rounded oracles."""
    if case not in _CACHE:
        pl = H.setup(case)[0]
        pre = {}
        free = H.run_oracle(case, preact=pre)
        codes = H.own_codes(pl, pre)
        exact = H.run_oracle(case, codes=codes)
        yard = {dn: H.run_oracle(case, codes=codes, store=H.storage(dt)) for dn, dt in H.DTYPES.items()}
        _CACHE[case] = dict(pl=pl, pre=pre, free=free, codes=codes, exact=exact, yard=yard)
    return _CACHE[case]


def _identical(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert (a[k] is None) == (b[k] is None), k
        assert a[k] is None or torch.equal(a[k], b[k]), f'{k}: differs by {float((a[k] - b[k]).abs().max()):.3e}'


def test_store_hook_is_inert_and_sees_every_stored_tensor():
    S = _shared()
    seen = []

    def identity(x, name):
        seen.append(name)
        return x
    _identical(H.run_oracle('default-b2', store=identity), S['free'])
    want = ['input']
    for L in S['pl']['enc']:
        want += [L['name'] + '.conv', L['name']]
    want.append('e_16x16.conv')
    for L in S['pl']['dec']:
        want += [L['name'] + '.conv', L['name']]
    assert [k for k in seen if not H.is_internal(k)] == want                    # the HBM tensors, in order
    inner = ['xb', 'up.taps', 'up.pass', 'pre', 'act', 'down.taps', 'down.pass']
    for L in H.layers(S['pl']):
        got = [k.split('.flr.')[1] for k in seen if k.startswith(L['name'] + '.flr.')]
        assert got == [t for t in inner if not (t.endswith('.pass') and L[t[0] == 'u' and 'fu' or 'fd'] is None)], (L['name'], got)
    assert seen.count('e_16x16') == 1
    assert sorted(k for k in seen if k.endswith('.weight')) == sorted([L['name'] + '.weight' for L in H.layers(S['pl'])] + ['e_16x16.weight'])


def test_imposing_the_oracles_own_codes_changes_nothing():
    S = _shared()
    _identical(S['exact'], S['free'])


@pytest.mark.parametrize('case', ['default-b2', 'clamp1-b2'])
def test_codes_round_trip_through_the_three_layouts(case):
    pl = H.setup(case)[0]
    if case in _CACHE:
        pre = _CACHE[case]['pre']
    else:
        pre = {}
        H.run_oracle(case, preact=pre, grads=False)
    codes = H.own_codes(pl, pre)
    names = [L['name'] for L in H.layers(pl)]
    for shift in range(3):                                       # every layer through every layout
        layouts = [(i + shift) % 3 for i in range(len(names))]
        records = [(R.encode_codes(codes[k].numpy(), lay), lay) for k, lay in zip(names, layouts)]
        back = H.codes_from_signs(pl, records)
        for k, (s, lay) in zip(names, records):
            rows, cols = codes[k].shape[2:]
            assert tuple(s.shape[2:]) == tuple(R.sign_tensor_shape(lay, rows, cols)), (k, lay)
            assert torch.equal(back[k][:, :, :rows, :cols], codes[k]), (k, lay)
            assert int(back[k].sum()) == int(codes[k].sum()), (k, lay)                 # the padding decodes to 0
    # ... and the decoded codes are what branch_report takes: the only decisions that differ from the oracle's are its exact zeros
    # (own_codes takes aten's derivative there), all inside the allowance even when that is 0 wide
    back.update({k: codes[k] for k in H.PLAIN})
    torgb = [L['name'] for L in pl['dec'] if L['torgb']]
    for name, differ, outside in H.branch_report(pl, back, pre, pre, pre):
        assert outside == 0 and differ == (0 if name in torgb else int((pre[name][0] == 0).sum())), (name, differ, outside)


def test_clamp1_clamps_an_encoder_layer_and_a_demodulating_decoder_layer():
    pl = H.setup('clamp1-b2')[0]
    assert pl['conv_clamp'] == 1.0
    pre = {}
    H.run_oracle('clamp1-b2', preact=pre, grads=False)
    codes = H.own_codes(pl, pre)
    frac = {k: float((v == 2).double().mean()) for k, v in codes.items()}
    print({k: round(f, 5) for k, f in frac.items() if f})
    assert any(frac[L['name']] > 0 for L in pl['enc'])
    assert any(frac[L['name']] > 0 for L in pl['dec'] if not L['torgb'])


def test_the_yardstick_passes_its_own_bar_and_a_coarser_type_does_not():
    S = _shared()
    for dn in H.DTYPES:
        passed, worst, table = H.grade(S['yard'][dn], S['exact'], S['yard'][dn])
        assert passed and worst <= 1.0 + 1e-12, (dn, worst)
        Y = [y for _, _, y, _ in table[1:]]
        print(f'{dn}: Y median {np.median(Y):.2e}, max {max(Y):.2e} ({table[1 + int(np.argmax(Y))][0]}), output {table[0][2]:.2e}')
    # three bits fewer per store (bf16 storage graded against the f16 yardstick) is a factor of 8 in every rounding: outside the margin of 4
    passed, worst, table = H.grade(S['yard']['bf16'], S['exact'], S['yard']['f16'])
    assert not passed, H.format_table(table)


@pytest.mark.parametrize('place', PLACES)
def test_criterion_rejects_one_wrong_cotangent_factor(place):
    S = _shared()
    assert place in [L['name'] for L in H.layers(S['pl'])]
    if place == 'encoder_5':
        L = next(L for L in S['pl']['enc'] if L['name'] == place)
        assert L['store'] and any(D['skip'] and D['skip_key'] == L['store_key'] for D in S['pl']['dec'])
    for dn, s in (('f16', 1.05), ('bf16', 1.25)):
        got = H.run_oracle('default-b2', codes=S['codes'], store=H.cotangent_error(place, s))
        assert torch.equal(got['output'], S['exact']['output'])                      # identity forward
        passed, worst, table = H.grade(got, S['exact'], S['yard'][dn])
        over = [k for k, e, _, b in table if e > b]
        # linear in s - 1: the smallest factor this place's worst parameter would still be rejected at
        res = 1 + (s - 1) / max(e / b for _, e, _, b in table)
        print(f'{place} s = {s} under the {dn} yardstick: {len(over)} of {len(table)} tensors over the bar, worst err / Y {worst:.1f}; '
              f'smallest s rejected {res:.4f}')
        assert not passed, f'{place}: s = {s} passes the {dn} criterion\n' + H.format_table(table)
