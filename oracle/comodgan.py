"""Functional restatement of the reference's CoModGAN generator (oracle; test-only), driven by a state dict with the keys of
``CoModGenerator.state_dict()`` and built from the pieces the oracle already has: ``conv2d_layer`` / ``fully_connected`` /
``conv2d_resample`` of oracle/discriminator.py (for up > 1 the DEFINITION: zero-insert, FIR with gain up^2, true convolution),
``bias_act`` / ``upsample2d`` of oracle/aten_ops.py and ``mapping`` of oracle/generator.py.

Follows (reference tree) CMG = models/networks/CoModGAN:
  modulated_conv2d   CMG/layers.py:20-65, always the unfused arithmetic (scale the activations by the styles, convolve with the shared
                     weight, multiply by the demodulation coefficients, add the noise)
  SynthesisLayer     CMG/layers.py:253-305       ToRGBLayer   :310-325       SynthesisBlock ('skip', fp32)   :330-450
  SynthesisNetwork   CMG/generator.py:29-125     CoModGenerator   :545-572
Runs in the dtype of its inputs: float64 as ground truth, float32 as the yardstick of what float32 arithmetic alone loses
(tests/comodgan_ref.py).  Nothing random happens in here: the noise planes and the dropout mask are arguments.

``noise``: 'none', 'const' (the layers' ``noise_const`` buffers) or a dict {layer prefix: plane [N, 1, R, R]} (the planes that
noise_mode='random' drew).  ``dropout_mask``: fc_in's output is multiplied by it (already scaled by 1 / (1 - p)); None: eval mode or p = 0.

Test instrumentation, not part of the reference: ``fault`` (a string or None) plants ONE wiring fault, so that a test can prove that its
criterion notices each of them (tests/test_comodgan_oracle_cpu.py); ``FAULTS`` lists them.  Pinned by tests/golden/K*.npz.
"""
import numpy as np
import torch

from . import aten_ops as ops
from .discriminator import conv2d_layer, conv2d_resample, fully_connected, setup_filter
from .generator import mapping

FAULTS = {
    'torgb_no_weight_gain': 'ToRGB styles not multiplied by 1 / sqrt(in_channels k^2)',
    'phase_order': "the four output phases of an up-2 layer interleaved in the order (px, py)",
    'no_d_noise_strength': 'no gradient reaches noise_strength',
    'skip_before_act': "the encoder skip added before conv0's activation instead of after it",
    'no_dcoefs_dweight': "the demodulation coefficients' contribution to d weight dropped",
    'no_dcoefs_dstyles': "the demodulation coefficients' contribution to d styles dropped",
    'clamp_no_gain': 'act_clamp not multiplied by gain',
    'conv1_next_w': "conv1 modulated by the block's next w instead of the block's one mod_vector",
}


def _plane(sd, p, noise):
    if noise == 'none' or (p + 'noise_strength') not in sd:
        return None
    if noise == 'const':
        return sd[p + 'noise_const']
    return noise[p]


def synthesis_layer(sd, p, x, w, up=1, act='lrelu', noise='none', gain=1, conv_clamp=None, filt=None, fault=None, pre_act_add=None):
    """SynthesisLayer.forward(x, w, gain=gain) (layers.py:286-305); kernel size and channels are the weight's.  ``pre_act_add``: only the
    'skip_before_act' fault uses it."""
    assert fault is None or fault in FAULTS
    filt = setup_filter([1, 3, 3, 1]) if filt is None else filt
    weight = sd[p + 'weight']
    ks = int(weight.shape[2])
    styles = fully_connected(sd, p + 'affine.', w)
    wd = weight.detach() if fault == 'no_dcoefs_dweight' else weight
    sdm = styles.detach() if fault == 'no_dcoefs_dstyles' else styles
    dcoefs = ((wd[None] * sdm[:, None, :, None, None]).square().sum(dim=[2, 3, 4]) + 1e-8).rsqrt()          # layers.py:48-51
    x = x * styles[:, :, None, None]
    x = conv2d_resample(x, weight, f=filt.to(x.dtype), up=up, padding=ks // 2, flip_weight=(up == 1))
    if fault == 'phase_order' and up == 2:
        n, o, h, wd_ = x.shape
        x = x.reshape(n, o, h // 2, 2, wd_ // 2, 2).transpose(3, 5).reshape(n, o, h, wd_)          # [.., i, py, j, px] -> [.., i, px, j, py]
    x = x * dcoefs[:, :, None, None]
    plane = _plane(sd, p, noise)
    if plane is not None:
        strength = sd[p + 'noise_strength']
        x = x + plane.to(x.dtype) * (strength.detach() if fault == 'no_d_noise_strength' else strength)
    if pre_act_add is not None:
        x = x + pre_act_add
    act_gain = ops.ACTIVATIONS[act][2] * gain
    act_clamp = None if conv_clamp is None else (conv_clamp if fault == 'clamp_no_gain' else conv_clamp * gain)
    return ops.bias_act(x, sd[p + 'bias'], act=act, gain=act_gain, clamp=act_clamp)


def torgb_layer(sd, p, x, w, conv_clamp=None, fault=None):
    """ToRGBLayer.forward (layers.py:321-325): modulated by styles / sqrt(in_channels k^2), no demodulation, padding 0, linear + clamp."""
    weight = sd[p + 'weight']
    styles = fully_connected(sd, p + 'affine.', w)
    if fault != 'torgb_no_weight_gain':
        styles = styles * (1 / np.sqrt(weight.shape[1] * weight.shape[2] ** 2))
    x = conv2d_resample(x * styles[:, :, None, None], weight)
    return ops.bias_act(x, sd[p + 'bias'], clamp=conv_clamp)


def synthesis_block(sd, p, x, img, ws, global_w, cond_mod=False, skip=None, noise='none', conv_clamp=None, filt=None, fault=None, gain=1):
    """SynthesisBlock.forward, architecture 'skip', fp32 (layers.py:396-450).  ``ws`` [N, num_conv + num_torgb, w_dim]; ``skip``: the encoder
    feature that is added after conv0's activation, or None (``include_skip=False`` or no features); the first block (no ``conv0`` in the state
    dict) takes ``x`` straight into conv1.  Returns (x, img)."""
    filt = setup_filter([1, 3, 3, 1]) if filt is None else filt
    w = ws[:, 0]
    mod = torch.cat([w, global_w], 1) if cond_mod else w                       # one vector for conv0, conv1 and torgb (layers.py:414-417)
    mod1 = mod
    if fault == 'conv1_next_w':
        mod1 = torch.cat([ws[:, 1], global_w], 1) if cond_mod else ws[:, 1]
    kw = dict(noise=noise, conv_clamp=conv_clamp, filt=filt, gain=gain)
    lf = fault if fault in ('phase_order', 'no_d_noise_strength', 'no_dcoefs_dweight', 'no_dcoefs_dstyles', 'clamp_no_gain') else None
    if (p + 'conv0.weight') in sd:
        if fault == 'skip_before_act' and skip is not None:
            x = synthesis_layer(sd, p + 'conv0.', x, mod, up=2, fault=lf, pre_act_add=skip, **kw)
        else:
            x = synthesis_layer(sd, p + 'conv0.', x, mod, up=2, fault=lf, **kw)
            if skip is not None:
                x = x + skip
    x = synthesis_layer(sd, p + 'conv1.', x, mod1, fault=lf, **kw)
    if img is not None:
        img = ops.upsample2d(img, filt.to(img.dtype))
    if (p + 'torgb.weight') in sd:
        y = torgb_layer(sd, p + 'torgb.', x, mod, conv_clamp=conv_clamp, fault=fault)
        img = img + y if img is not None else y
    return x, img


def synthesis(sd, ws, img_in, img_resolution, skip_resolution=256, cond_mod=False, conv_clamp=None, noise='const', dropout_mask=None,
              prefix='synthesis.', fault=None):
    """SynthesisNetwork.forward (generator.py:90-125): the encoder (its layers never clamp), the bottleneck, the blocks."""
    filt = setup_filter([1, 3, 3, 1])
    log2 = int(np.log2(img_resolution))
    dt = sd[prefix + 'fc_in.weight'].dtype
    ws = ws.to(dt)
    if skip_resolution >= 4:
        final = int(np.log2(skip_resolution))
        skips = [True] * (final - 1) + [False] * max(0, log2 - final)
    else:
        skips = [False] * log2
    feats = {}
    x = conv2d_layer(sd, prefix + 'e_fromrgb.con_layer.', img_in.to(dt), 1, act='lrelu')
    for r in range(log2, 2, -1):
        x = conv2d_layer(sd, f'{prefix}e_b{r}.conv_layer0.', x, 3, act='lrelu')
        feats[2 ** r] = x
        x = conv2d_layer(sd, f'{prefix}e_b{r}.conv_layer1.', x, 3, act='lrelu', down=2, filt=filt.to(dt))
    x = conv2d_layer(sd, prefix + 'e_4x4.', x, 3, act='lrelu')
    feats[4] = x
    g = fully_connected(sd, prefix + 'fc_in.', x.flatten(1), act='lrelu')
    if dropout_mask is not None:
        g = g * dropout_mask.to(dt)
    x = fully_connected(sd, prefix + 'fc_out.', g, act='lrelu').reshape(-1, x.shape[1], 4, 4)
    if skips[0]:
        x = x + feats[4]
    kw = dict(cond_mod=cond_mod, noise=noise, conv_clamp=conv_clamp, filt=filt, fault=fault)
    x, img = synthesis_block(sd, prefix + 'block_early.', x, None, ws[:, 0:2], g, **kw)
    idx = 1
    for r, on in zip(range(3, log2 + 1), skips[1:]):
        x, img = synthesis_block(sd, f'{prefix}b{2 ** r}.', x, img, ws[:, idx:idx + 3], g, skip=feats[2 ** r] if on else None, **kw)
        idx += 2
    return img


def num_ws(img_resolution):
    """block_early's conv1, two convolutions per later block, the last block's torgb (generator.py:70-81)."""
    return 1 + 2 * (int(np.log2(img_resolution)) - 2) + 1


def generator(sd, z, c, cond_img, img_resolution, mapping_layers=8, skip_resolution=256, cond_mod=False, conv_clamp=None, noise='const',
              dropout_mask=None, fault=None):
    """CoModGenerator.forward (generator.py:563-572) with truncation_psi=1; ``c`` is read only when the state dict has a label embedding."""
    ws = mapping(sd, z, c, num_ws(img_resolution), mapping_layers)
    return synthesis(sd, ws, cond_img, img_resolution, skip_resolution=skip_resolution, cond_mod=cond_mod, conv_clamp=conv_clamp, noise=noise,
                     dropout_mask=dropout_mask, fault=fault)
