"""Whole-volume inference: a stack of thick slices in, the synthesised volume out (the reference's evaluate.py: per subject, StandardPredictor
walks the test loader, runs the EMA generator on each batch, strips the halo, accumulates into a [C, D, H, W] map and divides by the visit count).

``predict_volume(where='device')`` keeps the whole loop on the device: the source volume and the table of patch origins are uploaded once, every
batch's ``A`` / ``slice_idx`` come from ``afcm_slice_assemble``, the EMA forward runs on the HIP kernels, and the prediction is added into the map by
``afcm_halo_accumulate`` -- no host read inside the loop.  ``where='host'`` is the path the package had before (``SliceDataset`` items built in numpy,
``SlidingWindowPredictor.accumulate`` behind a device -> host copy per batch and head) and exists as the comparison arm; both arms give the same bits.
"""
import numpy as np
import torch

from . import evaluation
from .data import SliceDataset, open_volumes
from .intensity import percentile_clip_host, rescale_intensity_host
from .predictor import SlidingWindowPredictor, patch_indices, validate_halo
from .torch_utils.ops.intensity_ops import percentile_clip, percentile_fractions, rescale_intensity
from .torch_utils.ops.plane_metrics import plane_stats
from .torch_utils.ops.volume_metrics import volume_ssim_layers
from .torch_utils.ops.volume_ops import assemble_slices, halo_accumulate


class PatchPlan:
    """The host-side plan of one volume's patches: ``origins`` int32 [P, 3] (z, y, x of every patch's first voxel, in loader order), the common
    ``patch_shape``, and the bounding box of any run of patches.  ``indices``: tuples of (z, y, x) slices as ``predictor.patch_indices`` and
    ``SliceDataset.raw_slices`` hold them.  Raises for a patch that is not inside the volume or whose shape differs from the first one's."""

    def __init__(self, volume_shape, indices):
        self.volume_shape = tuple(int(v) for v in volume_shape)
        if len(self.volume_shape) != 3 or min(self.volume_shape) < 1:
            raise RuntimeError(f'PatchPlan: expected a (D, H, W) volume shape, got {self.volume_shape}')
        indices = list(indices)
        if not indices:
            raise RuntimeError('PatchPlan: no patches')
        self.patch_shape = tuple(int(s.stop - s.start) for s in indices[0])
        self.origins = np.empty([len(indices), 3], dtype=np.int32)
        for i, index in enumerate(indices):
            if len(index) != 3:
                raise RuntimeError(f'PatchPlan: patch {i} has {len(index)} axes, expected (z, y, x)')
            for axis, (s, n, p) in enumerate(zip(index, self.volume_shape, self.patch_shape)):
                if s.step not in (None, 1) or s.start is None or s.stop is None or s.start < 0 or s.stop > n or s.stop - s.start < 1:
                    raise RuntimeError(f'PatchPlan: patch {i} {tuple((int(q.start), int(q.stop)) for q in index)} is not inside the volume {self.volume_shape}')
                if s.stop - s.start != p:
                    raise RuntimeError(f'PatchPlan: patch {i} has extent {s.stop - s.start} on axis {axis}, the first patch has {p}')
                self.origins[i, axis] = s.start
        self._tables = {}

    def __len__(self):
        return self.origins.shape[0]

    def bounding_box(self, first, count):
        """((z0, z1), (y0, y1), (x0, x1)) of the patches [first, first + count)."""
        if count < 1 or first < 0 or first + count > len(self):
            raise RuntimeError(f'PatchPlan: patches [{first}, {first + count}) are not inside a plan of {len(self)}')
        o = self.origins[first:first + count]
        lo, hi = o.min(axis=0), o.max(axis=0)
        return tuple((int(lo[a]), int(hi[a]) + self.patch_shape[a]) for a in range(3))

    def table(self, device):
        """The origin table on ``device``, uploaded once per plan and device."""
        device = torch.device(device)
        if device not in self._tables:
            self._tables[device] = torch.from_numpy(self.origins).to(device)
        return self._tables[device]


class DevicePredictor:
    """``SlidingWindowPredictor`` with the map, the visit mask and the accumulation on the device (same constructor arguments):

        p = DevicePredictor(out_channels=1, patch_halo=(0, 8, 8))
        p.allocate(volume_shape, device)                       # zeroed float32 map / uint8 mask [C, D, H, W]
        plan = p.plan(patch_shape, stride_shape)               # validate_halo + patch_indices -> PatchPlan (or pass a PatchPlan of your own)
        for first in range(0, len(plan), batch):
            p.accumulate(prediction, plan, first)              # [B, C, d, h, w] or [B, C, h, w], patches [first, first + B) of the plan
        volume = p.finish()                                    # map / mask, a device tensor (inf / nan where the mask is 0, as numpy gives)

    ``accumulate`` is one launch without a host read; the map is bit-identical to the host predictor's (afcm_halo_accumulate, include/afcm_hip.h)."""

    def __init__(self, out_channels=1, patch_halo=(4, 8, 8), prediction_channel=None):
        self.out_channels, self.patch_halo, self.prediction_channel = int(out_channels), tuple(int(v) for v in patch_halo), prediction_channel
        if len(self.patch_halo) != 3 or min(self.patch_halo) < 0:
            raise RuntimeError(f'DevicePredictor: patch_halo must be three non-negative values, got {self.patch_halo}')
        self.volume_shape = self.prediction_map = self.normalization_mask = None

    def allocate(self, volume_shape, device):
        if torch.device(device).type != 'cuda':
            raise RuntimeError(f'DevicePredictor needs a ROCm device (got {device}); the host predictor is afcm_amd.predictor.SlidingWindowPredictor')
        self.volume_shape = tuple(int(v) for v in volume_shape)
        shape = ((self.out_channels if self.prediction_channel is None else 1),) + self.volume_shape
        self.prediction_map = torch.zeros(shape, dtype=torch.float32, device=device)
        self.normalization_mask = torch.zeros(shape, dtype=torch.uint8, device=device)
        return self.prediction_map, self.normalization_mask

    def plan(self, patch_shape, stride_shape):
        if self.volume_shape is None:
            raise RuntimeError('DevicePredictor.plan: call allocate() first')
        validate_halo(self.patch_halo, patch_shape, stride_shape)
        return PatchPlan(self.volume_shape, patch_indices(self.volume_shape, tuple(patch_shape), tuple(stride_shape)))

    def accumulate(self, prediction, plan, first):
        if self.prediction_map is None:
            raise RuntimeError('DevicePredictor.accumulate: call allocate() first')
        if plan.volume_shape != self.volume_shape:
            raise RuntimeError(f'DevicePredictor.accumulate: the plan is for a volume {plan.volume_shape}, the map for {self.volume_shape}')
        patch = tuple(int(v) for v in (prediction.shape[2:] if prediction.dim() == 5 else (1,) + tuple(prediction.shape[2:])))
        if patch != plan.patch_shape:
            raise RuntimeError(f'DevicePredictor.accumulate: prediction patches are {patch}, the plan\'s {plan.patch_shape}')
        count = int(prediction.shape[0])
        halo_accumulate(self.prediction_map, self.normalization_mask, prediction, plan.table(self.prediction_map.device), first, self.patch_halo,
                        prediction_channel=self.prediction_channel, box=plan.bounding_box(int(first), count))

    def finish(self):
        """models/predictor.py:215: float32 / uint8 is one IEEE float32 division per voxel in torch as in numpy."""
        return self.prediction_map / self.normalization_mask


class GroupTables:
    """Which samples of every batch of a plan share their conditioning stack ``A``.  With four-slice inputs the stack of target ``idx`` is a function
    of ``idx // thickness`` alone (afcm_slice_assemble: ``idx_a = (idx / t) * t``), so that quotient names the group; ``thickness=None`` (one-slice
    inputs): every sample is its own group.  Built on the host from the plan's z origins and uploaded ONCE per volume; ``batch(first)`` returns
    device views: ``groups`` int32 [B], each sample's group numbered from 0 within its batch, and ``leaders`` int64 [G], the batch position of
    the first member of each group.  ``encoder_batches``: G of every batch, for reports."""

    def __init__(self, plan, batch_size, thickness, device):
        z = plan.origins[:, 0].astype(np.int64)
        keys = z // int(thickness) if thickness is not None else np.arange(len(plan), dtype=np.int64)
        groups, leaders, self._spans, self.encoder_batches = [], [], {}, []
        for first in range(0, len(plan), batch_size):
            k = keys[first:first + batch_size]
            _, lead, inverse = np.unique(k, return_index=True, return_inverse=True)
            order = np.argsort(lead, kind='stable')                            # groups numbered by first appearance in the batch
            rank = np.empty_like(order)
            rank[order] = np.arange(len(order))
            self._spans[first] = (len(k), sum(self.encoder_batches), len(lead))
            groups.append(rank[inverse.reshape(-1)])
            leaders.append(lead[order])
            self.encoder_batches.append(len(lead))
        flat = np.concatenate(groups + leaders).astype(np.int64)
        table = torch.from_numpy(flat).to(device)                              # the one upload
        self._groups = table[:len(plan)].to(torch.int32)
        self._leaders = table[len(plan):]

    def batch(self, first):
        count, lead0, n_groups = self._spans[first]
        return self._groups[first:first + count], self._leaders[lead0:lead0 + n_groups]


def _input_head(real_A):
    """models/predictor.py:152-158: the input head is the target's own thick slice, channel 1 of a four-slice input (a view, no copy)."""
    return real_A[:, 1:2] if real_A.shape[1] > 1 else real_A


@torch.no_grad()
def predict_volume(step, source, *, raw_internal_path_in, thickness, slice_num=4, patch_hw, batch_size, patch_halo=(0, 8, 8), heads=('prediction',),
                   where='device', min_value=0., max_value=255., rescale=None, clip=None, share_encoder=False, normalise=None):
    """One subject through the EMA generator: ``source`` (a mapping {internal path: array [D, Hs, Ws]} or an HDF5 file name) -> {head: [C, D, H, W]}
    with ``heads`` out of 'prediction' (``fake_B``) and 'input' (the thick slice each target falls into).  ``step`` needs
    ``set_test_input(real_A, slice_idx)``, ``test()``, ``real_A`` and ``fake_B`` [B, C, H, W] (``StyleGAN3GeneratorStep`` built with ``ema=True``).
    ``patch_hw`` = (H, W): every slice is centre-cropped / padded to it, so the volume is (D, H, W) and a patch is one whole slice; ``thickness`` is
    the slice thickness of the input (None only with ``slice_num`` 1).  ``where='device'`` returns device tensors and reads nothing back inside the
    loop; ``where='host'`` returns CPU tensors, the same bits.  Both arms draw ``gen_z`` batch by batch in the same order.
    ``rescale=(q_lo, q_hi)``: the source is a raw scanner volume and goes through ``intensity.rescale_intensity`` with those percentiles first -- on
    the device after the upload (``where='device'``, still no host read) or through ``rescale_intensity_host`` -- so the loop sees a uint8 volume, the
    same one in both arms.  None: the source is taken as it is.
    ``clip=(p_min, p_max)``: the same for a subject that is normalised the ``cmsrnii`` way -- ``intensity.percentile_clip`` with those percentiles
    (and its defaults: the volume is its own reference, the lower bound not below 0) on the device, ``percentile_clip_host`` on the host.  ``clip``
    and ``rescale`` exclude each other.
    ``share_encoder=True`` (``where='device'`` only): with four-slice inputs the ``thickness`` consecutive targets of one thick slice carry the same
    ``A`` bit for bit, so the step is told which rows of a batch are equal (``set_test_input(a, slice_idx, groups, leaders)``) and runs the
    generator's encoder once per group instead of once per sample.  The batch partition does not change; a group that straddles a batch boundary
    is encoded once in each batch.  With ``slice_num`` 1 or no thickness every sample is its own group.
    ``normalise``: a ``NormaliseConfig`` (afcm_amd/normalise.py) -- a model trained under the reference's ``PercentileNormalizer`` or ``Standardize``
    needs it at inference: every input plane is normalised by its own percentiles or moments, by ``assemble_slices(normalise=)`` on the device and
    by ``SliceDataset(normalise=)`` on the host, the same bits."""
    if where not in ('device', 'host'):
        raise ValueError(f"where must be 'device' or 'host', got {where!r}")
    if share_encoder and where != 'device':
        raise ValueError("share_encoder=True needs where='device'")
    heads = tuple(heads)
    if not heads or any(h not in ('prediction', 'input') for h in heads):
        raise ValueError(f"heads are 'prediction' and 'input', got {heads!r}")
    path = raw_internal_path_in if isinstance(raw_internal_path_in, str) else list(raw_internal_path_in)[0]
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f'batch_size {batch_size}')
    patch_shape, stride_shape = (1, int(patch_hw[0]), int(patch_hw[1])), (1, 1, 1)      # one patch per slice: the y / x strides never come into play
    validate_halo(patch_halo, patch_shape, stride_shape)
    if rescale is not None and clip is not None:
        raise ValueError('predict_volume: rescale= and clip= are two normalisations of a raw source; give one')
    if rescale is not None:
        percentile_fractions(rescale, 'predict_volume: rescale')
    if clip is not None:
        percentile_fractions(clip, 'predict_volume: clip')
    out_channels = {}

    def channels(head, t):                                    # the map's channel count is the head's, known at the first batch
        return out_channels.setdefault(head, int(t.shape[1]))

    if where == 'host':
        if rescale is not None:
            source = {path: rescale_intensity_host(open_volumes(source, [path])[path], rescale)[0]}
        if clip is not None:
            source = {path: percentile_clip_host(open_volumes(source, [path])[path], clip)[0]}
        ds = SliceDataset(source, phase='test', patch_shape=patch_shape, stride_shape=stride_shape, raw_internal_path_in=[path], raw_internal_path_out=[path],
                          thickness=[] if thickness is None else [thickness], slice_num=slice_num, min_value=min_value, max_value=max_value,
                          normalise=normalise)
        volume_shape = tuple(ds.raw[path].shape)
        predictors, maps = {}, {}
        for first in range(0, len(ds), batch_size):
            items = [ds[i] for i in range(first, min(first + batch_size, len(ds)))]
            step.set_test_input(torch.stack([it[0] for it in items]), torch.stack([it[1] for it in items]))
            step.test()
            for head in heads:
                t = (step.fake_B if head == 'prediction' else _input_head(step.real_A)).unsqueeze(2)
                if head not in predictors:
                    predictors[head] = SlidingWindowPredictor(out_channels=channels(head, t), patch_halo=patch_halo)
                    maps[head] = predictors[head].allocate(volume_shape)
                t = t.float() if t.dtype == torch.bfloat16 else t          # numpy has no bfloat16; the widening is exact
                predictors[head].accumulate(maps[head][0], maps[head][1], t, [it[2] for it in items], volume_shape)
        with np.errstate(divide='ignore', invalid='ignore'):
            return {head: torch.from_numpy(maps[head][0] / maps[head][1]) for head in heads}

    device = next(step.netG.parameters()).device if hasattr(step, 'netG') else torch.device('cuda')
    src = open_volumes(source, [path])[path]
    volume = torch.from_numpy(np.ascontiguousarray(src)).to(device)                    # the loop's one upload of the subject
    if rescale is not None:
        volume = rescale_intensity(volume, rescale)[0]
    if clip is not None:
        volume = percentile_clip(volume, clip)[0]
    volume_shape = (int(volume.shape[0]),) + patch_shape[1:]
    plan = PatchPlan(volume_shape, patch_indices(volume_shape, patch_shape, stride_shape))
    predictors = {}
    shared = GroupTables(plan, batch_size, thickness if slice_num == 4 else None, device) if share_encoder else None
    for first in range(0, len(plan), batch_size):
        a, slice_idx = assemble_slices(volume, first, min(batch_size, len(plan) - first), patch_shape, thickness=thickness, slice_num=slice_num,
                                       min_value=min_value, max_value=max_value, stride_shape=stride_shape, normalise=normalise)
        if shared is None:
            step.set_test_input(a, slice_idx)
        else:
            step.set_test_input(a, slice_idx, *shared.batch(first))
        step.test()
        for head in heads:
            t = step.fake_B if head == 'prediction' else _input_head(step.real_A)
            if head not in predictors:
                predictors[head] = DevicePredictor(out_channels=channels(head, t), patch_halo=patch_halo)
                predictors[head].allocate(volume_shape, t.device)
            predictors[head].accumulate(t, plan, first)
    return {head: predictors[head].finish() for head in heads}


def volume_metrics(fake, target, *, from_network_range=True, with_3d=False):
    """The metric half of ``evaluate_volume`` for a predicted volume ``fake`` and its ``target`` ([D, H, W] device tensors of one shape): the three
    axes' statistics tables (and, ``with_3d``, the d - 6 layer sums of ``afcm_volume_ssim`` behind them) gathered on the device and copied to the host
    ONCE, then the numpy finishers.  The axial table serves 'slice', 'one' and '3d' alike.  Returns {'slice': ..., 'one': ...[, '3d': ...]}."""
    d, h, w = (int(v) for v in fake.shape)
    views = ((0, 1, 2), (1, 0, 2), (2, 0, 1))
    tables = [plane_stats(target.permute(*p), fake.permute(*p), unit_map=from_network_range) for p in views]
    if not with_3d:
        tables = torch.cat(tables).cpu().numpy()
    else:                                                  # one flat tensor, one copy: the three tables, then the layer sums
        layers = volume_ssim_layers(target[None], fake[None], unit_map=from_network_range)
        flat = torch.cat([t.reshape(-1) for t in tables] + [layers.reshape(-1)]).cpu().numpy()
        tables, layers = flat[:(d + h + w) * 8].reshape(d + h + w, 8), flat[(d + h + w) * 8:]
    by_axis = (tables[:d], tables[d:d + h], tables[d + h:])
    out = {'slice': evaluation.evaluate_slice_from_stats(by_axis[0], h, w), 'one': evaluation.evaluate_one_from_stats(by_axis, (d, h, w))}
    if with_3d:
        out['3d'] = evaluation.evaluate_3D_from_stats(by_axis[0], layers, (d, h, w))
    return out


def evaluate_volume(step, source, target, *, from_network_range=True, with_3d=False, **predict_kwargs):
    """``predict_volume(where='device')`` followed by the reference's per-volume metrics (evaluate.py:73-87) without leaving the device:
    ``evaluation_device.evaluate_slice`` (the per-slice means evaluate.py reports as psnr_slice / ssim_slice) and ``evaluate_one`` (slices along all
    three axes) of channel 0 of the prediction against ``target`` [D, H, W], a device tensor.  With ``from_network_range`` (the default) both are
    mapped to [0, 1] on load by ``to_unit_range``, evaluate.py:76-77's ``(clip(x, -1, 1) + 1) / 2`` for the prediction, so ``target`` is expected in the
    network's range, normalised as the loader normalises its volumes; pass False when both already are in [0, 1].  The three statistics tables
    are gathered on the device and copied once: that copy is the only device -> host transfer and the only synchronise of the whole call.
    ``with_3d=True`` adds ``evaluate_3D`` (volume PSNR and the 7^3-window SSIM evaluate.py:81 reports first) as ``'3d'``: the layer sums of
    ``afcm_volume_ssim`` travel in that same copy, behind the three tables.  ``rescale=(q_lo, q_hi)`` (a ``predict_volume`` keyword) takes a raw
    scanner volume as the source and rescales it on the device after the upload, still without a host read; ``clip=(p_min, p_max)`` does the same
    with the percentile clip; ``normalise=NormaliseConfig(...)`` normalises every input plane by its own statistics, as in ``predict_volume``.
    Returns {'slice': (psnr, ssim, mae), 'one': (psnr, ssim, mae), 'prediction': [C, D, H, W] device tensor} and, on request, '3d': (psnr, ssim, mae)."""
    if predict_kwargs.get('where', 'device') != 'device':
        raise ValueError("evaluate_volume runs on the device; for host arrays use predict_volume(where='host') and afcm_amd.evaluation")
    predict_kwargs['heads'] = ('prediction',)
    prediction = predict_volume(step, source, **predict_kwargs)['prediction']
    fake = prediction[0]
    if not isinstance(target, torch.Tensor) or target.device != fake.device:
        raise RuntimeError('evaluate_volume: the target must be a tensor on the prediction\'s device (upload it once, outside the loop)')
    if target.shape != fake.shape:
        raise RuntimeError(f'evaluate_volume: the target is {tuple(target.shape)}, the predicted volume {tuple(fake.shape)}')
    return dict(volume_metrics(fake, target, from_network_range=from_network_range, with_3d=with_3d), prediction=prediction)
