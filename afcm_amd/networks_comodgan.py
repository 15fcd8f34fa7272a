"""The CoModGAN generator -- the baseline of the AFCM generator, ``netG: 'comodgan'`` of the reference's ``define_G``
(models/utils.py:153-160): ``CoModGenerator`` and its blocks with the reference's class names, constructor arguments, ``forward()``
signatures and state-dict keys (models/networks/CoModGAN/layers.py:214-450, generator.py:29-125, 545-572), so that a reference
``*_net_G.pth`` loads with ``strict=True``.  ``Conv2dLayer``, ``FullyConnectedLayer`` and ``MappingNetwork`` are those of
networks_discriminator.py.

The modulated convolution always runs the reference's UNFUSED arithmetic (``fused_modconv=False``: scale the activations by the
styles, convolve with the shared weight, demodulate the result) in ``train()`` and ``eval()`` alike; the reference's grouped-conv
form in ``eval()`` is the same function in another rounding order.  ``IMPL`` chooses how a ``SynthesisLayer`` runs it:

  'unfused'  the reference's decomposition on the existing ops: ``conv2d_resample`` (for up=2 a transposed convolution, then the
             4x4 FIR over a full-resolution intermediate), then ``x * dcoefs + noise``, then ``bias_act``.
  'fused'    the convolution on the MFMA conv ops with the styles as its input scale, then ONE pass of the HIP epilogue
             (torch_utils/ops/modconv_epilogue.py: demodulation, noise, bias, lrelu, gain, clamp).  For up=2 the transposed
             convolution and its blur are folded into four 3x3 stride-1 kernels on the low-resolution input
             (``fold_up2_weights``), and the epilogue interleaves the four phases as it writes.

The fused arm covers 3x3 kernels, 'lrelu', and for up=2 the [1,3,3,1] filter; everything else takes the unfused arm.

Refused (``NotImplementedError``): 16-bit blocks (``num_fp16_res > 0``: every shipped comodgan configuration runs fp32),
``channel_attention``, the 'orig' / 'resnet' block architectures, mapper / synthesizer names other than ``MappingNetwork`` /
``SynthesisNetwork``, and shared-encoder inference (``encode`` / ``decode`` / ``cond_groups``).
"""
import numpy as np
import torch

from .networks_discriminator import Conv2dLayer, FullyConnectedLayer, MappingNetwork
from .torch_utils.ops import bias_act, conv2d_resample, upfirdn2d

IMPL = 'fused'          # 'fused' | 'unfused': module switch, read at every SynthesisLayer.forward

_FOLD_FILTER = [1, 3, 3, 1]
_TAPS = {}              # (dtype, device) -> the fold's tap table A [2, 3, 3]


def _fold_taps(dtype, device):
    """A[p][d][k] = g[2 (d - 1) - p + 1 + k] with g = 2 * [1, 3, 3, 1] / 8 (the per-axis filter with its share of the gain 4), 0 where
    the index leaves 0..3: the weight of tap k of the 3-tap kernel in tap d of output phase p's low-resolution kernel."""
    a = _TAPS.get((dtype, device))
    if a is not None:
        return a
    g = [0.25, 0.75, 0.75, 0.25]
    a = torch.zeros([2, 3, 3], dtype=torch.float64)
    for p in range(2):
        for d in range(3):
            for k in range(3):
                idx = 2 * (d - 1) - p + 1 + k
                if 0 <= idx <= 3:
                    a[p, d, k] = g[idx]
    # quarters: exact in every float type.  Uploaded once per (dtype, device): a captured step finds it made by its warm-up runs
    a = _TAPS[(dtype, device)] = a.to(device=device, dtype=dtype)
    return a


def fold_up2_weights(w):
    """The up-2 layer (``conv2d_resample(x, w, f=[1,3,3,1], up=2, padding=1, flip_weight=False)``: transposed stride-2 convolution,
    pad, 4x4 FIR with gain 4) as four 3x3 stride-1 correlations of the LOW-resolution input: returns W4 [4 O, I, 3, 3] with
    ``conv2d(x, W4, padding=1)[n, (py 2 + px) O + o, i, j] = y[n, o, 2 i + py, 2 j + px]``.  Built in torch, so autograd yields dw."""
    o, i, kh, kw = w.shape
    assert kh == 3 and kw == 3
    a = _fold_taps(w.dtype, w.device)
    return torch.einsum('oiyx,pdy,qex->pqoide', w, a, a).reshape(4 * o, i, 3, 3)


def unfold_phases(t):
    """[N, 4 O, H, W] in ``fold_up2_weights``' channel order -> [N, O, 2 H, 2 W] (depth to space; what the epilogue kernel does as it writes)."""
    n, c, h, w = t.shape
    return t.reshape(n, 2, 2, c // 4, h, w).permute(0, 3, 4, 1, 5, 2).reshape(n, c // 4, 2 * h, 2 * w)


class E_fromrgb(torch.nn.Module):
    """layers.py:214-223."""

    def __init__(self, in_channels, out_channels, kernel_size=1, activation='lrelu', conv_clamp=None):
        super().__init__()
        self.con_layer = Conv2dLayer(in_channels, out_channels, kernel_size=1, activation=activation, trainable=True, conv_clamp=conv_clamp,
                                     channels_last=False)

    def forward(self, x, y):
        t = self.con_layer(y)
        return t if x is None else x + t


class E_block(torch.nn.Module):
    """layers.py:228-248."""

    def __init__(self, res, tmp_channels, out_channels, kernel_size=3, activation='lrelu', conv_clamp=None, resample_filter=[1, 3, 3, 1],
                 channel_attention=False):
        super().__init__()
        if channel_attention:
            raise NotImplementedError('E_block: channel_attention=True is not part of this package')
        self.res = res
        self.channel_attention = channel_attention
        self.conv_layer0 = Conv2dLayer(tmp_channels, tmp_channels, kernel_size=kernel_size, activation=activation, trainable=True,
                                       conv_clamp=conv_clamp, channels_last=False)
        self.conv_layer1 = Conv2dLayer(tmp_channels, out_channels, kernel_size=kernel_size, activation=activation, down=2, trainable=True,
                                       resample_filter=resample_filter, conv_clamp=conv_clamp, channels_last=False)

    def forward(self, x, E_features):
        x = self.conv_layer0(x)
        E_features[2 ** self.res] = x
        return self.conv_layer1(x)


def _dcoefs(weight, styles):
    """rsqrt(sum_{i,k} (w[o,i,k] s[n,i])^2 + 1e-8) [N, O] (layers.py:48-51), factorised as s^2 @ (sum_k w^2)^T: no [N, O, I, k, k] tensor."""
    return (styles.square() @ weight.square().sum([2, 3]).t() + 1e-8).rsqrt()


class SynthesisLayer(torch.nn.Module):
    """layers.py:253-305."""

    def __init__(self, in_channels, out_channels, w_dim, resolution, kernel_size=3, up=1, use_noise=True, activation='lrelu',
                 resample_filter=[1, 3, 3, 1], conv_clamp=None, channels_last=False):
        super().__init__()
        self.resolution = resolution
        self.up = up
        self.use_noise = use_noise
        self.activation = activation
        self.conv_clamp = conv_clamp
        self.register_buffer('resample_filter', upfirdn2d.setup_filter(resample_filter))
        self.padding = kernel_size // 2
        self.act_gain = bias_act.activation_funcs[activation].def_gain
        # what the fused arm covers: 3x3, lrelu, and for up=2 the fold's filter
        self.foldable = (kernel_size == 3 and activation == 'lrelu' and (up == 1 or (up == 2 and list(resample_filter) == _FOLD_FILTER)))
        self.affine = FullyConnectedLayer(w_dim, in_channels, bias_init=1)
        self.weight = torch.nn.Parameter(torch.randn([out_channels, in_channels, kernel_size, kernel_size]))
        if use_noise:
            self.register_buffer('noise_const', torch.randn([resolution, resolution]))
            self.noise_strength = torch.nn.Parameter(torch.zeros([]))
        self.bias = torch.nn.Parameter(torch.zeros([out_channels]))

    def forward(self, x, w, noise_mode='random', fused_modconv=True, gain=1):
        """``fused_modconv`` is accepted and ignored (see the module docstring)."""
        assert noise_mode in ['random', 'const', 'none']
        if IMPL not in ('fused', 'unfused'):
            raise ValueError(f"networks_comodgan.IMPL is 'fused' or 'unfused', got {IMPL!r}")
        in_resolution = self.resolution // self.up
        want = [self.weight.shape[1], in_resolution, in_resolution]
        assert list(x.shape[1:]) == want, f'SynthesisLayer: expected [N, {want}], got {list(x.shape)}'
        styles = self.affine(w)
        dcoefs = _dcoefs(self.weight, styles)
        plane = None
        if self.use_noise and noise_mode == 'random':
            plane = torch.randn([x.shape[0], 1, self.resolution, self.resolution], device=x.device)
        if self.use_noise and noise_mode == 'const':
            plane = self.noise_const
        act_gain = self.act_gain * gain
        act_clamp = self.conv_clamp * gain if self.conv_clamp is not None else None
        if IMPL == 'fused' and self.foldable:
            from .torch_utils.ops import conv2d as conv_ops
            from .torch_utils.ops.modconv_epilogue import modconv_epilogue
            weight = fold_up2_weights(self.weight) if self.up == 2 else self.weight
            t = conv_ops.scaled_conv2d(x, weight, styles, None, 1)
            return modconv_epilogue(t, dcoefs, self.bias, plane, self.noise_strength if plane is not None else None, up=self.up,
                                    alpha=bias_act.activation_funcs['lrelu'].def_alpha, gain=act_gain, clamp=act_clamp)
        x = x * styles.reshape(x.shape[0], -1, 1, 1)
        x = conv2d_resample.conv2d_resample(x=x, w=self.weight, f=self.resample_filter, up=self.up, padding=self.padding,
                                            flip_weight=(self.up == 1))
        d = dcoefs.reshape(x.shape[0], -1, 1, 1)
        x = torch.addcmul(plane * self.noise_strength, x, d) if plane is not None else x * d          # fma.fma(x, dcoefs, noise)
        return bias_act.bias_act(x, self.bias, act=self.activation, gain=act_gain, clamp=act_clamp)


class ToRGBLayer(torch.nn.Module):
    """layers.py:310-325: modulated 1x1 without demodulation, then bias (+ clamp)."""

    def __init__(self, in_channels, out_channels, w_dim, kernel_size=1, conv_clamp=None, channels_last=False):
        super().__init__()
        self.conv_clamp = conv_clamp
        self.affine = FullyConnectedLayer(w_dim, in_channels, bias_init=1)
        self.weight = torch.nn.Parameter(torch.randn([out_channels, in_channels, kernel_size, kernel_size]))
        self.bias = torch.nn.Parameter(torch.zeros([out_channels]))
        self.weight_gain = 1 / np.sqrt(in_channels * (kernel_size ** 2))

    def forward(self, x, w, fused_modconv=True):
        styles = self.affine(w) * self.weight_gain
        x = x * styles.reshape(x.shape[0], -1, 1, 1)
        x = conv2d_resample.conv2d_resample(x=x, w=self.weight)          # padding 0, as modulated_conv2d's default
        return bias_act.bias_act(x, self.bias, clamp=self.conv_clamp)


class SynthesisBlock(torch.nn.Module):
    """layers.py:330-450, the 'skip' architecture in fp32."""

    def __init__(self, in_channels, out_channels, w_dim, global_w_dim, resolution, img_channels, is_last, up=2, to_rgb=True, architecture='skip',
                 resample_filter=[1, 3, 3, 1], conv_clamp=None, use_fp16=False, fp16_channels_last=False, cond_mod=False, early_channels=0,
                 channel_attention=False, **layer_kwargs):
        assert architecture in ['orig', 'skip', 'resnet']
        super().__init__()
        if architecture != 'skip':
            raise NotImplementedError(f"SynthesisBlock: architecture {architecture!r} is not part of this package ('skip' only)")
        if use_fp16:
            raise NotImplementedError('SynthesisBlock: 16-bit blocks (use_fp16 / num_fp16_res > 0) are not part of this package')
        if channel_attention:
            raise NotImplementedError('SynthesisBlock: channel_attention=True is not part of this package')
        self.in_channels = in_channels
        self.w_dim = w_dim
        self.resolution = resolution
        self.img_channels = img_channels
        self.is_last = is_last
        self.architecture = architecture
        self.use_fp16 = use_fp16
        self.channels_last = False
        self.register_buffer('resample_filter', upfirdn2d.setup_filter(resample_filter))
        self.num_conv = 0
        self.num_torgb = 0
        self.cond_mod = cond_mod
        self.channel_attention = channel_attention
        if not cond_mod:
            global_w_dim = 0
        if in_channels != 0:
            self.conv0 = SynthesisLayer(in_channels, out_channels, w_dim=w_dim + global_w_dim, resolution=resolution, up=up,
                                        resample_filter=resample_filter, conv_clamp=conv_clamp, channels_last=False, **layer_kwargs)
            self.num_conv += 1
        self.conv1 = SynthesisLayer(early_channels if early_channels > 0 else out_channels, out_channels, w_dim=w_dim + global_w_dim,
                                    resolution=resolution, conv_clamp=conv_clamp, channels_last=False, **layer_kwargs)
        self.num_conv += 1
        if to_rgb and (is_last or architecture == 'skip'):
            self.torgb = ToRGBLayer(out_channels, img_channels, w_dim=w_dim + global_w_dim, conv_clamp=conv_clamp, channels_last=False)
            self.num_torgb += 1

    def forward(self, x, img, ws, global_w, E_features=None, include_skip=True, force_fp32=False, fused_modconv=None, **layer_kwargs):
        assert list(ws.shape[1:]) == [self.num_conv + self.num_torgb, self.w_dim], f'b{self.resolution}: ws {list(ws.shape)}'
        w_iter = iter(ws.unbind(dim=1))
        x_skip = E_features[self.resolution].to(torch.float32) if E_features is not None else None
        w = next(w_iter)
        mod_vector = torch.cat((w, global_w), 1) if self.cond_mod else w        # ONE vector for conv0, conv1 and torgb (layers.py:414-417)
        if self.in_channels == 0:
            x = self.conv1(x, mod_vector, **layer_kwargs)
        else:
            half = self.resolution // 2
            assert list(x.shape[1:]) == [self.in_channels, half, half], f'b{self.resolution}: x {list(x.shape)}'
            x = self.conv0(x.to(torch.float32), mod_vector, **layer_kwargs)
            if include_skip and x_skip is not None:
                x = x + x_skip                                                  # after the activation (layers.py:432-434)
            x = self.conv1(x, mod_vector, **layer_kwargs)
        if img is not None:
            half = self.resolution // 2
            assert list(img.shape[1:]) == [self.img_channels, half, half], f'b{self.resolution}: img {list(img.shape)}'
            img = upfirdn2d.upsample2d(img, self.resample_filter)
        if self.is_last or self.architecture == 'skip':
            y = self.torgb(x, mod_vector).to(torch.float32)
            img = img.add_(y) if img is not None else y
        assert x.dtype == torch.float32 and (img is None or img.dtype == torch.float32)
        return x, img


class SynthesisNetwork(torch.nn.Module):
    """generator.py:29-125: the conditional encoder (e_fromrgb, e_b*, e_4x4, fc_in / dropout / fc_out), then the synthesis blocks that take
    the encoder's features as skips and its global vector next to w."""

    def __init__(self, w_dim, img_resolution, img_channels_in, img_channels_out, channel_base=32768, channel_max=512, num_fp16_res=0,
                 activation='lrelu', resample_filter=[1, 3, 3, 1], dropout_rate=0.5, skip_resolution=256, channel_attention=False, **block_kwargs):
        assert img_resolution >= 4 and img_resolution & (img_resolution - 1) == 0
        super().__init__()
        if num_fp16_res > 0:
            raise NotImplementedError('SynthesisNetwork: num_fp16_res > 0 (16-bit blocks) is not part of this package: every shipped comodgan '
                                      'configuration runs fp32')
        if channel_attention:
            raise NotImplementedError('SynthesisNetwork: channel_attention=True is not part of this package')
        self.compute_dtype = torch.float32          # what StyleGAN3GeneratorStep reads (and, on the EMA copy, sets): fp32 is all there is
        self.w_dim = w_dim
        self.img_resolution = img_resolution
        self.img_resolution_log2 = int(np.log2(img_resolution))
        self.img_channels_in = img_channels_in
        self.img_channels_out = img_channels_out
        self.block_resolutions = [2 ** i for i in range(2, self.img_resolution_log2 + 1)]
        self.channels_dict = {res: min(channel_base // res, channel_max) for res in self.block_resolutions}
        ch = self.channels_dict
        self.num_ws = 0
        for res in range(self.img_resolution_log2, 2, -1):
            if res == self.img_resolution_log2:
                self.e_fromrgb = E_fromrgb(in_channels=img_channels_in, out_channels=ch[2 ** res], kernel_size=1, activation='lrelu', conv_clamp=None)
            setattr(self, f'e_b{res}', E_block(res=res, tmp_channels=ch[2 ** res], out_channels=ch[2 ** res // 2], kernel_size=3, activation='lrelu',
                                               conv_clamp=None, resample_filter=resample_filter))
        self.e_4x4 = Conv2dLayer(ch[4], ch[4], kernel_size=3, activation=activation, conv_clamp=None)
        self.fc_in = FullyConnectedLayer(ch[4] * (4 ** 2), ch[4] * 2, activation=activation)
        self.dropout = torch.nn.Dropout(p=dropout_rate)
        self.fc_out = FullyConnectedLayer(ch[4] * 2, ch[4] * (4 ** 2), activation=activation)
        self.block_early = SynthesisBlock(0, ch[4], w_dim=w_dim, global_w_dim=ch[4] * 2, resolution=4, img_channels=img_channels_out, is_last=False,
                                          use_fp16=False, channel_attention=channel_attention, **block_kwargs)
        self.num_ws += self.block_early.num_conv
        for res in self.block_resolutions[1:]:
            is_last = (res == self.img_resolution)
            block = SynthesisBlock(ch[res // 2], ch[res], w_dim=w_dim, global_w_dim=ch[4] * 2, resolution=res, img_channels=img_channels_out,
                                   is_last=is_last, use_fp16=False, channel_attention=channel_attention, **block_kwargs)
            self.num_ws += block.num_conv
            if is_last:
                self.num_ws += block.num_torgb
            setattr(self, f'b{res}', block)
        if skip_resolution >= 4:
            final_skip = int(np.log2(skip_resolution))
            self.skip_connects = [True] * (final_skip - 1) + [False] * max(0, self.img_resolution_log2 - final_skip)
        else:
            self.skip_connects = [False] * self.img_resolution_log2

    def encode(self, *args, **kwargs):
        raise NotImplementedError('comodgan SynthesisNetwork: encode / decode (shared-encoder inference) is not part of this package')

    decode = encode

    def forward(self, ws, img_in, update_emas=False, **block_kwargs):
        """``update_emas`` is accepted and ignored (this generator keeps no activation statistics)."""
        assert list(ws.shape[1:]) == [self.num_ws, self.w_dim], f'ws: expected [N, {self.num_ws}, {self.w_dim}], got {list(ws.shape)}'
        ws = ws.to(torch.float32)
        block_ws = [ws.narrow(1, 0, self.block_early.num_conv + self.block_early.num_torgb)]
        w_idx = self.block_early.num_conv
        for res in self.block_resolutions[1:]:
            block = getattr(self, f'b{res}')
            block_ws.append(ws.narrow(1, w_idx, block.num_conv + block.num_torgb))
            w_idx += block.num_conv
        E_features = {}
        x = self.e_fromrgb(None, img_in)
        for res in range(self.img_resolution_log2, 2, -1):
            x = getattr(self, f'e_b{res}')(x, E_features)
        x = self.e_4x4(x)
        E_features[4] = x
        x = self.dropout(self.fc_in(x.flatten(1)))
        img_global = x
        x = self.fc_out(x).reshape(-1, self.channels_dict[4], 4, 4)
        if self.skip_connects[0]:
            x = x + E_features[4]
        x, img = self.block_early(x, None, block_ws[0], img_global, **block_kwargs)
        for res, cur_ws, skip in zip(self.block_resolutions[1:], block_ws[1:], self.skip_connects[1:]):
            x, img = getattr(self, f'b{res}')(x, img, cur_ws, img_global, E_features, skip, **block_kwargs)
        return img


class CoModGenerator(torch.nn.Module):
    """generator.py:545-572.  ``mapping_kwargs`` / ``synthesis_kwargs`` may carry the configuration's ``name`` (get_mapper / get_synthesizer):
    'MappingNetwork' and 'SynthesisNetwork' are the ones that exist here."""

    def __init__(self, z_dim, c_dim, w_dim, img_resolution, img_channels_in, img_channels_out, mapping_kwargs={}, synthesis_kwargs={}):
        super().__init__()
        mapping_kwargs, synthesis_kwargs = dict(mapping_kwargs), dict(synthesis_kwargs)
        for what, kw, only in (('mapper', mapping_kwargs, 'MappingNetwork'), ('synthesizer', synthesis_kwargs, 'SynthesisNetwork')):
            name = kw.pop('name', only)
            if name != only:
                raise NotImplementedError(f'CoModGenerator: {what} {name!r} is not part of this package ({only!r} only)')
        self.z_dim = z_dim
        self.c_dim = c_dim
        self.w_dim = w_dim
        self.img_resolution = img_resolution
        self.img_channels_in = img_channels_in
        self.img_channels_out = img_channels_out
        self.synthesis = SynthesisNetwork(w_dim=w_dim, img_resolution=img_resolution, img_channels_in=img_channels_in,
                                          img_channels_out=img_channels_out, **synthesis_kwargs)
        self.num_ws = self.synthesis.num_ws
        self.mapping = MappingNetwork(z_dim=z_dim, c_dim=c_dim, w_dim=w_dim, num_ws=self.num_ws, **mapping_kwargs)

    def forward(self, z, c, cond_img, ref_img=None, truncation_psi=1, truncation_cutoff=None, cond_groups=None, **synthesis_kwargs):
        if cond_groups is not None:
            raise NotImplementedError('CoModGenerator: cond_groups (shared-encoder inference, share_encoder=True) is not part of this package: '
                                      'run the volume loops with share_encoder=False')
        ws = self.mapping(z=z, c=c, truncation_psi=truncation_psi, img_in=ref_img, truncation_cutoff=truncation_cutoff)
        return self.synthesis(ws, cond_img, **synthesis_kwargs)
