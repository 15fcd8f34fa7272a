"""The training side of the data path: the training set resident on the device, one launch per batch, and the reference's inner training loop
(train.py:45-77) on top of it.

``DeviceSliceSet`` uploads every volume of every subject once into one pool tensor and describes an epoch as an int32 table of
``(vol_a, vol_b, idx, thickness)`` rows; ``afcm_batch_assemble`` (torch_utils/ops/batch_ops.py) turns ``count`` rows of that table into the batch
``SliceDataset(phase='train')`` items would stack to, bit for bit.  ``train_epoch`` is the loop ``for data in dataset: set_input; optimize_parameters;
EMA`` with the batches from the device (or, ``where='host'``, from ``SliceDataset``: the comparison arm).  ``TrainingGraph`` is that loop's body as one
replayed graph that reads its batch through a device-side cursor: no host data work between steps.  With ``DeviceSliceSet(augment=AugmentConfig(...))``
a float64 table of parameter rows (afcm_amd/augment.py) travels beside the item table and every batch comes out of ``afcm_batch_assemble_aug``
flipped, turned and rotated as the reference's training transforms do it, inside the same launch.  With
``DeviceSliceSet(intensity=IntensityConfig(...))`` a second float64 table (afcm_amd/augment_intensity.py) carries the item's contrast change and the key
and parameters of its Gaussian and Poisson noise, generated inside ``afcm_batch_assemble_noise``.  With
``DeviceSliceSet(elastic=ElasticConfig(...))`` a third float64 table (afcm_amd/augment_elastic.py) carries the decision, the scale and the key of
the item's elastic deformation, and every batch goes through ``afcm_batch_assemble_elastic``: between the geometric and the intensity transforms.
With ``DeviceSliceSet(blur=BlurConfig(...))`` a fourth float64 table (afcm_amd/augment_blur.py) carries every plane's decision, sigma and host-made
weights of the reference's ``GaussianBlur3D``, and every batch goes through ``afcm_batch_assemble_blur``: after the elastic deformation, before
the intensity transforms.
With ``DeviceSliceSet(normalise=NormaliseConfig(...))`` (afcm_amd/normalise.py) every plane goes through the reference's ``PercentileNormalizer`` or
``Standardize`` instead of the fixed ``Normalize``: ``afcm_plane_norm_stats`` writes each plane's coefficients into a buffer the set owns and
``afcm_batch_assemble_norm`` applies them, with or without the geometric table.
"""
import random

import numpy as np
import torch

from . import _lib
from . import augment_blur, augment_elastic, augment_intensity
from .augment import AugmentConfig, apply_host, augment_rows, checked_rows, identity_rows
from .data import SliceDataset, open_volumes
from .intensity import percentile_clip_host, rescale_intensity_host
from .normalise import checked_config, refuse_with
from .torch_utils.ops.batch_ops import advance_cursor, assemble_batch, blur_workspace_bytes, elastic_workspace_bytes
from .stylegan3_model import capture_graph, require_capturable
from .torch_utils.ops.intensity_ops import percentile_clip, percentile_fractions, rescale_intensity


class DeviceSliceSet:
    """All subjects' volumes in one device pool, addressed by a table of training items.

    ``sources``: one mapping ``{internal path: ndarray [D, Hs, Ws]}`` or HDF5 file name per subject, as ``SliceDataset`` takes them.  The volumes of
    ``raw_internal_path_in[0]`` and of every output modality are uploaded uncropped (the kernel crops / pads each to ``patch_shape[1:]`` from its own
    extent) into one 1-D tensor of their common dtype; ``vols`` int64 [subjects * modalities, 4] holds (element offset, depth, hs, ws).
    ``device=None`` builds the host-side tables only (``epoch_items`` and ``host_batch`` work, nothing is uploaded).
    ``rescale=(q_lo, q_hi)``: the sources are raw scanner volumes; each is uploaded as it is and passed through ``rescale_intensity`` with those
    percentiles into a uint8 pool, volume by volume, so the subjects' raw dtypes may differ; ``host_batch`` rescales with
    ``rescale_intensity_host``, the same bits.  None: the volumes are pooled as they are.
    ``clip=(p_min, p_max)``: the same with ``percentile_clip`` / ``percentile_clip_host`` (each volume its own reference, the lower bound not below
    0), the normalisation of ``dataset_mode: cmsrnii``.  ``clip`` and ``rescale`` exclude each other.
    ``augment``: an ``AugmentConfig`` (afcm_amd/augment.py; 'train' only) -- the set keeps a float64 [len(self), 8] device table of parameter rows
    beside the item table, ``epoch_augment`` draws an epoch's rows, ``load_epoch`` uploads them and every batch goes through
    ``afcm_batch_assemble_aug``.  None: no table, ``afcm_batch_assemble``.
    ``intensity``: an ``IntensityConfig`` (afcm_amd/augment_intensity.py; 'train' only, with or without ``augment``) -- a float64 [len(self), 36]
    device table beside the others, ``epoch_intensity`` draws an epoch's rows, ``load_epoch`` uploads them and every batch goes through
    ``afcm_batch_assemble_noise``.  None: no table, the launches above.
    ``elastic``: an ``ElasticConfig`` (afcm_amd/augment_elastic.py; 'train' only, with or without the other two) -- a float64 [len(self), 4]
    device table beside the others, ``epoch_elastic`` draws an epoch's rows, ``load_epoch`` uploads them and every batch goes through
    ``afcm_batch_assemble_elastic``.  The set builds the two smoothing operators of its patch size once (``elastic_ops``, host and device) and owns
    the launch's workspace, grown to the largest batch asked for (a captured graph keeps the one it was captured with).  None: no table, the
    launches above.
    ``blur``: a ``BlurConfig`` (afcm_amd/augment_blur.py; 'train' only, with or without the other three) -- a float64
    [len(self), 20 (slice_num + 1)] device table beside the others, ``epoch_blur`` draws an epoch's rows, ``load_epoch`` uploads them and every
    batch goes through ``afcm_batch_assemble_blur``, whose workspace (the elastic launches' included) the set owns in the same way.  None: no
    table, the launches above.
    ``normalise``: a ``NormaliseConfig`` (afcm_amd/normalise.py; any phase, with or without ``augment``, not with the other three) -- every plane
    of every item is normalised by its own percentiles or moments: two launches per batch, ``afcm_plane_norm_stats`` into the set's persistent
    float64 [batch, slice_num + 1, 4] coefficient buffer (``norm_coef``, grown to the largest batch asked for; a captured graph keeps the one it
    was captured with), then ``afcm_batch_assemble_norm``.  None: the launches above, exactly."""

    def __init__(self, sources, phase='train', patch_shape=(1, 256, 256), raw_internal_path_in=('raw',), raw_internal_path_out=('raw',),
                 rand_output=False, cat_inputs=False, thickness=(), slice_num=4, min_value=0.0, max_value=255.0, device='cuda', rescale=None, augment=None, clip=None,
                 intensity=None, elastic=None, blur=None, normalise=None):
        if checked_config(normalise, 'DeviceSliceSet') is not None:
            refuse_with('DeviceSliceSet', intensity=intensity, elastic=elastic, blur=blur)
        self.normalise, self.norm_coef = normalise, None
        if phase not in ('train', 'val', 'test'):
            raise RuntimeError(f"DeviceSliceSet: phase must be 'train', 'val' or 'test', got {phase!r}")
        if cat_inputs:
            raise RuntimeError('DeviceSliceSet: cat_inputs=True is not supported (no shipped configuration uses it); use SliceDataset for it')
        patch_shape = tuple(int(v) for v in patch_shape)
        if len(patch_shape) != 3 or patch_shape[0] != 1 or min(patch_shape) < 1:
            raise RuntimeError(f'DeviceSliceSet: patch_shape must be (1, H, W), got {patch_shape}')
        _lib.require_slice_num(slice_num, 'DeviceSliceSet')
        if augment is not None:
            if not isinstance(augment, AugmentConfig):
                raise RuntimeError(f'DeviceSliceSet: augment must be an AugmentConfig or None, got {type(augment).__name__}')
            if phase != 'train':
                raise RuntimeError(f"DeviceSliceSet: augmentation belongs to the 'train' phase, got phase {phase!r}")
            augment.check_patch(patch_shape[1:], 'DeviceSliceSet')
        self.augment = augment
        if intensity is not None:
            if not isinstance(intensity, augment_intensity.IntensityConfig):
                raise RuntimeError(f'DeviceSliceSet: intensity must be an IntensityConfig or None, got {type(intensity).__name__}')
            if phase != 'train':
                raise RuntimeError(f"DeviceSliceSet: augmentation belongs to the 'train' phase, got phase {phase!r}")
        self.intensity = intensity
        if elastic is not None:
            if not isinstance(elastic, augment_elastic.ElasticConfig):
                raise RuntimeError(f'DeviceSliceSet: elastic must be an ElasticConfig or None, got {type(elastic).__name__}')
            if phase != 'train':
                raise RuntimeError(f"DeviceSliceSet: augmentation belongs to the 'train' phase, got phase {phase!r}")
        self.elastic = elastic
        if blur is not None:
            if not isinstance(blur, augment_blur.BlurConfig):
                raise RuntimeError(f'DeviceSliceSet: blur must be a BlurConfig or None, got {type(blur).__name__}')
            if phase != 'train':
                raise RuntimeError(f"DeviceSliceSet: augmentation belongs to the 'train' phase, got phase {phase!r}")
        self.blur = blur
        # the smoothing operators of the patch size, once: host (the comparison arm) and device
        self.elastic_ops_host = None if elastic is None else tuple(augment_elastic.smoothing_operator(elastic.sigma, n) for n in patch_shape[1:])
        self.elastic_ops = self.elastic_workspace = None
        self.phase, self.patch_shape, self.rand_output, self.slice_num = phase, patch_shape, bool(rand_output), int(slice_num)
        self.raw_internal_path_in, self.raw_internal_path_out = list(raw_internal_path_in), list(raw_internal_path_out)
        self.thickness = [int(t) for t in thickness]
        if any(t < 1 for t in self.thickness) or (slice_num == 4 and not self.thickness):
            raise RuntimeError(f'DeviceSliceSet: thicknesses {self.thickness} with slice number {slice_num}: every thickness must be at least 1, and '
                               f'slice number 4 needs one')
        if not max_value > min_value:
            raise RuntimeError(f'DeviceSliceSet: max_value {max_value} is not above min_value {min_value}')
        self.min_value, self.max_value = float(min_value), float(max_value)
        self.paths = list(dict.fromkeys(self.raw_internal_path_in[:1] + self.raw_internal_path_out))
        self.volumes = [open_volumes(s, self.paths) for s in sources]
        if not self.volumes:
            raise RuntimeError('DeviceSliceSet: no subjects')
        self.rescale = None if rescale is None else tuple(float(q) for q in rescale)
        self.clip = None if clip is None else tuple(float(q) for q in clip)
        if self.rescale is not None and self.clip is not None:
            raise RuntimeError('DeviceSliceSet: rescale= and clip= are two normalisations of raw sources; give one')
        if self.rescale is not None:
            percentile_fractions(self.rescale, 'DeviceSliceSet: rescale')
        if self.clip is not None:
            percentile_fractions(self.clip, 'DeviceSliceSet: clip')
        normalised = self.rescale is not None or self.clip is not None
        dtypes = sorted({str(v.dtype) for subject in self.volumes for v in subject.values()})
        if not normalised and len(dtypes) != 1:
            raise RuntimeError(f'DeviceSliceSet: mixed source dtypes {dtypes}: the pool holds one dtype, convert the volumes first')
        for name in dtypes:
            _lib.source_code(np.dtype(name), 'DeviceSliceSet')
        self.source_dtype = np.dtype(np.uint8) if normalised else np.dtype(dtypes[0])
        rows, offset, self.depths = [], 0, []
        for s, subject in enumerate(self.volumes):
            shapes = {p: tuple(int(n) for n in subject[p].shape) for p in self.paths}
            if len(set(shapes.values())) != 1 or len(shapes[self.paths[0]]) != 3:
                raise RuntimeError(f'DeviceSliceSet: subject {s}: the input and output volumes must have one [D, H, W] shape, got {shapes}')
            d, hs, ws = shapes[self.paths[0]]
            if min(d, hs, ws) < 1:
                raise RuntimeError(f'DeviceSliceSet: subject {s}: empty volume {shapes[self.paths[0]]}')
            self.depths.append(d)
            for _ in self.paths:
                rows.append((offset, d, hs, ws))
                offset += d * hs * ws
        self.vols_host = np.array(rows, dtype=np.int64)
        self.pool_elems = offset
        # (subject, idx) of every slice in serial order, and where each subject's first row lies
        self._subject = np.repeat(np.arange(len(self.depths), dtype=np.int64), self.depths)
        self._idx = np.concatenate([np.arange(d, dtype=np.int64) for d in self.depths])
        self._host_sets, self._host_rescaled = {}, {}
        self.device = None if device is None else torch.device(device)
        self.pool = self.vols = self.items = self.cursor = self.augment_table = self.intensity_table = self.elastic_table = self.blur_table = None
        self.rows = self.position = 0
        if self.device is not None:
            if self.device.type != 'cuda':
                raise RuntimeError(f'DeviceSliceSet needs a ROCm device (got {self.device}); device=None builds the host-side tables only')
            if not normalised:
                pool = np.concatenate([np.ascontiguousarray(subject[p]).reshape(-1) for subject in self.volumes for p in self.paths])
                self.pool = torch.from_numpy(pool).to(self.device)                       # the one upload of the training set
            else:
                self.pool = torch.empty(self.pool_elems, dtype=torch.uint8, device=self.device)
                raw = [subject[p] for subject in self.volumes for p in self.paths]
                for (at, d, hs, ws), v in zip(rows, raw):                                # each volume raw, normalised into its place in the pool
                    uploaded, place = torch.from_numpy(np.ascontiguousarray(v)).to(self.device), self.pool[at:at + d * hs * ws].view(d, hs, ws)
                    if self.rescale is not None:
                        rescale_intensity(uploaded, self.rescale, out=place)
                    else:
                        percentile_clip(uploaded, self.clip, out=place)
            self.vols = torch.from_numpy(self.vols_host).to(self.device)
            # persistent (a captured graph holds their addresses): the epoch's table, refreshed in place, and the row a graph's next batch starts at
            self.items = torch.full((len(self), 4), -1, dtype=torch.int32, device=self.device)
            self.cursor = torch.zeros(1, dtype=torch.int64, device=self.device)
            if self.augment is not None:                                                 # persistent as the item table is: row r belongs to item row r
                self.augment_table = torch.from_numpy(identity_rows(len(self))).to(self.device)
            if self.intensity is not None:
                self.intensity_table = torch.from_numpy(augment_intensity.identity_rows(len(self))).to(self.device)
            if self.elastic is not None:
                self.elastic_table = torch.from_numpy(augment_elastic.identity_rows(len(self))).to(self.device)
                self.elastic_ops = tuple(torch.from_numpy(op).to(self.device) for op in self.elastic_ops_host) + (self.elastic.spline_order,)
            if self.blur is not None:
                self.blur_table = torch.from_numpy(augment_blur.identity_rows(len(self), self.slice_num)).to(self.device)

    def __len__(self):
        return int(self._idx.shape[0])

    def epoch_items(self, seed_or_generator=None, shuffle=None):
        """The int32 [len(self), 4] table of one epoch, rows (vol_a, vol_b, idx, thickness); every (subject, idx) appears exactly once.  'train':
        the rows are shuffled (unless ``shuffle`` is False), the thickness is drawn uniformly per row from the list (-1 for an empty list) and,
        with ``rand_output``, ``vol_b`` uniformly from the output modalities; 'val' / 'test': serial order, ``thickness[0]``, the last output
        modality.  The draws come from a ``numpy.random.Generator`` (``seed_or_generator``: one, or a seed for ``default_rng``) in a fixed order:
        the permutation, the thicknesses, the modalities.  The reference's own stream -- ``random.choice`` inside DataLoader workers plus the sampler's
        permutation -- depends on worker scheduling and cannot be reproduced; the distribution is the same."""
        rng = seed_or_generator if isinstance(seed_or_generator, np.random.Generator) else np.random.default_rng(seed_or_generator)
        n, train, m = len(self), self.phase == 'train', len(self.paths)
        order = rng.permutation(n) if (train if shuffle is None else shuffle) else np.arange(n)
        subject, idx = self._subject[order], self._idx[order]
        if not self.thickness:
            thickness = np.full(n, -1, dtype=np.int64)
        elif train:
            thickness = np.asarray(self.thickness, dtype=np.int64)[rng.integers(0, len(self.thickness), n)]
        else:
            thickness = np.full(n, self.thickness[0], dtype=np.int64)
        out_columns = np.array([self.paths.index(p) for p in self.raw_internal_path_out], dtype=np.int64)
        if train and self.rand_output:
            column_b = out_columns[rng.integers(0, len(out_columns), n)]
        else:
            column_b = np.full(n, out_columns[-1], dtype=np.int64)
        column_a = self.paths.index(self.raw_internal_path_in[0])
        return np.stack([subject * m + column_a, subject * m + column_b, idx, thickness], axis=1).astype(np.int32)

    def _checked_items(self, items):
        items = np.ascontiguousarray(np.asarray(items))
        if items.ndim != 2 or items.shape[1] != 4 or items.dtype != np.int32 or items.shape[0] < 1:
            raise RuntimeError(f'DeviceSliceSet: an item table is int32 [n, 4] with n >= 1, got {items.dtype} {items.shape}')
        return items

    def epoch_augment(self, seed_or_generator=None, rows=None):
        """The float64 [rows, 8] parameter table of one epoch (``rows``: ``len(self)`` when None), drawn by ``augment.augment_rows`` from the
        set's ``AugmentConfig``; call it after ``epoch_items`` on the same generator, as ``train_epochs`` does."""
        if self.augment is None:
            raise RuntimeError('DeviceSliceSet.epoch_augment: this set was built without augment=AugmentConfig(...)')
        rng = seed_or_generator if isinstance(seed_or_generator, np.random.Generator) else np.random.default_rng(seed_or_generator)
        return augment_rows(self.augment, len(self) if rows is None else rows, self.patch_shape[1:], rng)

    def _checked_augment(self, augment, n, what):
        """The parameter table that goes with an item table of ``n`` rows: ``augment`` checked, identity rows for None, None for a set without
        augmentation (which refuses a table)."""
        if self.augment is None:
            if augment is not None:
                raise RuntimeError(f'DeviceSliceSet.{what}: an augment table for a set built without augment=AugmentConfig(...)')
            return None
        return identity_rows(n) if augment is None else checked_rows(augment, n, f'DeviceSliceSet.{what}')

    def epoch_intensity(self, seed_or_generator=None, rows=None):
        """The float64 [rows, 36] intensity table of one epoch (``rows``: ``len(self)`` when None), drawn by ``augment_intensity.intensity_rows``
        from the set's ``IntensityConfig``; call it after ``epoch_items`` and ``epoch_augment`` on the same generator, as ``train_epochs`` does."""
        if self.intensity is None:
            raise RuntimeError('DeviceSliceSet.epoch_intensity: this set was built without intensity=IntensityConfig(...)')
        rng = seed_or_generator if isinstance(seed_or_generator, np.random.Generator) else np.random.default_rng(seed_or_generator)
        return augment_intensity.intensity_rows(self.intensity, len(self) if rows is None else rows, rng)

    def _checked_intensity(self, intensity, n, what):
        """``_checked_augment`` for the intensity table."""
        if self.intensity is None:
            if intensity is not None:
                raise RuntimeError(f'DeviceSliceSet.{what}: an intensity table for a set built without intensity=IntensityConfig(...)')
            return None
        return augment_intensity.identity_rows(n) if intensity is None else augment_intensity.checked_rows(intensity, n, f'DeviceSliceSet.{what}')

    def epoch_elastic(self, seed_or_generator=None, rows=None):
        """The float64 [rows, 4] elastic table of one epoch (``rows``: ``len(self)`` when None), drawn by ``augment_elastic.elastic_rows`` from the
        set's ``ElasticConfig``; call it after ``epoch_items``, ``epoch_augment`` and ``epoch_intensity`` on the same generator, as
        ``train_epochs`` does."""
        if self.elastic is None:
            raise RuntimeError('DeviceSliceSet.epoch_elastic: this set was built without elastic=ElasticConfig(...)')
        rng = seed_or_generator if isinstance(seed_or_generator, np.random.Generator) else np.random.default_rng(seed_or_generator)
        return augment_elastic.elastic_rows(self.elastic, len(self) if rows is None else rows, rng)

    def _checked_elastic(self, elastic, n, what):
        """``_checked_augment`` for the elastic table."""
        if self.elastic is None:
            if elastic is not None:
                raise RuntimeError(f'DeviceSliceSet.{what}: an elastic table for a set built without elastic=ElasticConfig(...)')
            return None
        return augment_elastic.identity_rows(n) if elastic is None else augment_elastic.checked_rows(elastic, n, f'DeviceSliceSet.{what}')

    def epoch_blur(self, seed_or_generator=None, rows=None):
        """The float64 [rows, 20 (slice_num + 1)] blur table of one epoch (``rows``: ``len(self)`` when None), drawn by ``augment_blur.blur_rows``
        from the set's ``BlurConfig``.  The reference's class draws from Python's ``random``, so the draws come from a ``random.Random``
        (``seed_or_generator``: one, or an int seed for one), not from the numpy generator the other tables share."""
        if self.blur is None:
            raise RuntimeError('DeviceSliceSet.epoch_blur: this set was built without blur=BlurConfig(...)')
        rng = seed_or_generator if isinstance(seed_or_generator, random.Random) else random.Random(seed_or_generator)
        return augment_blur.blur_rows(self.blur, len(self) if rows is None else rows, self.slice_num, rng)

    def _checked_blur(self, blur, n, what):
        """``_checked_augment`` for the blur table."""
        if self.blur is None:
            if blur is not None:
                raise RuntimeError(f'DeviceSliceSet.{what}: a blur table for a set built without blur=BlurConfig(...)')
            return None
        if blur is None:
            return augment_blur.identity_rows(n, self.slice_num)
        return augment_blur.checked_rows(blur, n, self.slice_num, f'DeviceSliceSet.{what}')

    def load_epoch(self, items, augment=None, intensity=None, elastic=None, blur=None):
        """Uploads the table into the persistent device table (rows past it are marked invalid) and puts the cursor back to row 0.  A set built
        with ``augment`` takes the epoch's parameter rows (``epoch_augment``) the same way, identity rows when none are given; one built with
        ``intensity`` its intensity rows (``epoch_intensity``) likewise, one built with ``elastic`` its elastic rows (``epoch_elastic``), one built
        with ``blur`` its blur rows (``epoch_blur``)."""
        self._need_device('load_epoch')
        items = self._checked_items(items)
        if items.shape[0] > self.items.shape[0]:
            raise RuntimeError(f'DeviceSliceSet.load_epoch: {items.shape[0]} rows do not fit the device table of {self.items.shape[0]} (one per slice)')
        augment = self._checked_augment(augment, items.shape[0], 'load_epoch')
        intensity = self._checked_intensity(intensity, items.shape[0], 'load_epoch')
        elastic = self._checked_elastic(elastic, items.shape[0], 'load_epoch')
        blur = self._checked_blur(blur, items.shape[0], 'load_epoch')
        self.items[:items.shape[0]].copy_(torch.from_numpy(items), non_blocking=False)
        self.items[items.shape[0]:].fill_(-1)
        if augment is not None:
            self.augment_table[:items.shape[0]].copy_(torch.from_numpy(augment), non_blocking=False)
            self.augment_table[items.shape[0]:].copy_(torch.from_numpy(identity_rows(len(self) - items.shape[0])))
        if intensity is not None:
            self.intensity_table[:items.shape[0]].copy_(torch.from_numpy(intensity), non_blocking=False)
            self.intensity_table[items.shape[0]:].copy_(torch.from_numpy(augment_intensity.identity_rows(len(self) - items.shape[0])))
        if elastic is not None:
            self.elastic_table[:items.shape[0]].copy_(torch.from_numpy(elastic), non_blocking=False)
            self.elastic_table[items.shape[0]:].copy_(torch.from_numpy(augment_elastic.identity_rows(len(self) - items.shape[0])))
        if blur is not None:
            self.blur_table[:items.shape[0]].copy_(torch.from_numpy(blur), non_blocking=False)
            self.blur_table[items.shape[0]:].copy_(torch.from_numpy(augment_blur.identity_rows(len(self) - items.shape[0], self.slice_num)))
        self.rows = int(items.shape[0])
        self.rewind()

    def rewind(self):
        self._need_device('rewind')
        self.cursor.zero_()
        self.position = 0

    def _need_device(self, what):
        if self.pool is None:
            raise RuntimeError(f'DeviceSliceSet.{what}: this set was built with device=None (host-side tables only)')

    def batch(self, first, count, out=None, dtype=torch.float32, use_cursor=False):
        """``(A, B, slice_idx)`` of the rows ``[first, first + count)`` of the loaded epoch (counted from the cursor with ``use_cursor``)."""
        self._need_device('batch')
        first, count = int(first), int(count)
        if not use_cursor and (count < 1 or first < 0 or first + count > self.rows):
            raise RuntimeError(f'DeviceSliceSet.batch: rows [{first}, {first + count}) are not inside the loaded epoch of {self.rows} (load_epoch first)')
        more = {}
        if self.elastic is not None or self.blur is not None:
            order = None if self.elastic is None else self.elastic.spline_order
            if self.blur is not None:                                                        # the blur launches' workspace holds the elastic ones'
                need = blur_workspace_bytes(count, self.slice_num, *self.patch_shape[1:], order)
            else:
                need = elastic_workspace_bytes(count, self.slice_num, *self.patch_shape[1:], order)
            if self.elastic_workspace is None or self.elastic_workspace.numel() < need:   # a larger batch than any before: a new one; a graph keeps its own
                self.elastic_workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
            more = dict(workspace=self.elastic_workspace)
            if self.elastic is not None:
                more.update(elastic=self.elastic_table, elastic_ops=self.elastic_ops)
            if self.blur is not None:
                more.update(blur=self.blur_table)
        if self.normalise is not None:
            if self.norm_coef is None or self.norm_coef.shape[0] < count:                 # a larger batch than any before: a new one; a graph keeps its own
                self.norm_coef = torch.empty((count, self.slice_num + 1, 4), dtype=torch.float64, device=self.device)
            more = dict(normalise=self.normalise, norm_coef=self.norm_coef)
        return assemble_batch(self.pool, self.vols, self.items, first, count, self.patch_shape[1:], slice_num=self.slice_num, min_value=self.min_value,
                              max_value=self.max_value, dtype=dtype, out=out, cursor=self.cursor if use_cursor else None, augment=self.augment_table,
                              intensity=self.intensity_table, independent_planes=self.intensity is not None and self.intensity.independent_planes, **more)

    def batches(self, batch_size, drop_last=False, dtype=torch.float32):
        """The loaded epoch batch by batch; the last batch is partial unless ``drop_last``, as the reference's loader leaves it."""
        batch_size = int(batch_size)
        if batch_size < 1:
            raise RuntimeError(f'DeviceSliceSet.batches: batch size {batch_size}')
        for first in range(0, self.rows, batch_size):
            count = min(batch_size, self.rows - first)
            if count < batch_size and drop_last:
                return
            yield self.batch(first, count, dtype=dtype)

    def _host_volumes(self, subject):
        """The subject's volumes as the pool holds them: as given, or rescaled / clipped by the host function."""
        if self.rescale is None and self.clip is None:
            return self.volumes[subject]
        if subject not in self._host_rescaled:
            self._host_rescaled[subject] = {p: rescale_intensity_host(v, self.rescale)[0] if self.rescale is not None else percentile_clip_host(v, self.clip)[0]
                                            for p, v in self.volumes[subject].items()}
        return self._host_rescaled[subject]

    def host_batch(self, items, first, count, device=None, augment=None, intensity=None, elastic=None, blur=None, normalise=None):
        """The same batch through ``SliceDataset(phase='train', thickness=[t])`` items, stacked and uploaded: the comparison arm of tests and
        benchmark.  ``augment``: the parameter table that goes with ``items`` (a set built with ``augment`` only); ``augment.apply_host`` applies
        row ``first + j`` to ``A`` and ``B`` of item ``first + j``.  ``intensity``: the intensity table that goes with ``items`` (a set built with
        ``intensity`` only), applied after it by ``augment_intensity.apply_host``.  ``elastic``: the elastic table that goes with ``items`` (a set
        built with ``elastic`` only), applied between the two by ``augment_elastic.apply_host``.  ``blur``: the blur table that goes with
        ``items`` (a set built with ``blur`` only), applied between the elastic and the intensity arms by ``augment_blur.apply_host``.  A row the
        kernel would refuse raises here.  ``normalise``: a ``NormaliseConfig`` -- the items come from ``SliceDataset(normalise=)``, every plane
        through ``normalise_host`` before the geometric transforms; not with ``intensity``, ``elastic`` or ``blur``."""
        if checked_config(normalise, 'DeviceSliceSet.host_batch') is not None:
            refuse_with('DeviceSliceSet.host_batch', intensity=intensity, elastic=elastic, blur=blur)
        items = self._checked_items(items)
        elastic = None if elastic is None else self._checked_elastic(elastic, items.shape[0], 'host_batch')
        blur = None if blur is None else self._checked_blur(blur, items.shape[0], 'host_batch')
        augment = None if augment is None else self._checked_augment(augment, items.shape[0], 'host_batch')
        intensity = None if intensity is None else self._checked_intensity(intensity, items.shape[0], 'host_batch')
        m = len(self.paths)
        a, b, c = [], [], []
        for j, (vol_a, vol_b, idx, t) in enumerate(items[first:first + count].tolist()):
            subject, column_b = divmod(vol_b, m)
            if not (0 <= vol_b < m * len(self.volumes)) or vol_a != subject * m + self.paths.index(self.raw_internal_path_in[0]):
                raise RuntimeError(f'DeviceSliceSet.host_batch: row ({vol_a}, {vol_b}, {idx}, {t}) does not pair the input and an output of one subject')
            key = (subject, column_b, normalise)
            if key not in self._host_sets:
                self._host_sets[key] = SliceDataset(self._host_volumes(subject), phase='train', patch_shape=self.patch_shape, stride_shape=(1, 1, 1),
                                                    raw_internal_path_in=self.raw_internal_path_in[:1], raw_internal_path_out=[self.paths[column_b]],
                                                    slice_num=self.slice_num, min_value=self.min_value, max_value=self.max_value,
                                                    normalise=normalise)
            ds = self._host_sets[key]
            ds.thickness = [] if t == -1 else [t]
            if not 0 <= idx < len(ds):
                raise RuntimeError(f'DeviceSliceSet.host_batch: slice {idx} of a subject of {len(ds)}')
            item = ds[idx]
            if augment is not None:
                item['A'], item['B'] = apply_host(item['A'], augment[first + j]), apply_host(item['B'], augment[first + j])
            if elastic is not None:                                                      # all planes of the item, the target included: one deformation
                both = augment_elastic.apply_host(torch.cat([item['A'], item['B']]), elastic[first + j], self.elastic, self.elastic_ops_host)
                item['A'], item['B'] = both[:-1], both[-1:]
            if blur is not None:                                                         # every plane its own record: those of A, then B
                both = augment_blur.apply_host(torch.cat([item['A'], item['B']]), blur[first + j])
                item['A'], item['B'] = both[:-1], both[-1:]
            if intensity is not None:
                independent = self.intensity.independent_planes
                item['A'] = augment_intensity.apply_host(item['A'], intensity[first + j], independent, 0)
                item['B'] = augment_intensity.apply_host(item['B'], intensity[first + j], independent, self.slice_num)
            a.append(item['A'])
            b.append(item['B'])
            c.append(torch.from_numpy(item['slice_idx']))
        device = device if device is not None else (self.device if self.device is not None else 'cpu')
        return torch.stack(a).to(device), torch.stack(b).to(device), torch.stack(c).to(device)


def _label(step, slice_idx):
    """The label as ``set_test_input`` hands it to the generator: ``slice_idx`` [B, 1], zeros for an unconditional one."""
    return slice_idx if step.netG.c_dim > 0 else torch.zeros_like(slice_idx)


def _fed_step(step, schedule, batch_size, batch, gen_z, cur_nimg=None):
    """One training step on the batch ``batch()`` returns, as ``train_epoch``, ``TrainingGraph`` and ``train_epochs`` all run it: with a
    ``schedule`` (the step's own ``DeviceSchedule``) ``schedule.advance(batch_size)`` first -- total_iters, sigma and beta are the block's -- and,
    when the step has an EMA copy and the schedule an ``ema_kimgs``, ``step.update_ema()`` last."""
    if schedule is not None:
        schedule.advance(batch_size)
    a, b, slice_idx = batch()
    step.set_input(a, b, gen_z=gen_z, gen_c=_label(step, slice_idx))
    step.optimize_parameters(cur_nimg=cur_nimg)
    if schedule is not None and schedule.ema_kimgs is not None and step.netG_ema is not None:
        step.update_ema()


def train_epoch(step, dataset, batch_size, items, total_iters=0, ema_kimgs=None, ramp=None, where='device', gen_z=None, augment=None,
                intensity=None, elastic=None, blur=None):
    """The inner loop of the reference's train.py:45-77 over the epoch table ``items`` (``DeviceSliceSet.epoch_items``): per batch
    ``total_iters += batch_size``, ``step.set_input(A, B, gen_c=slice_idx)``, ``step.optimize_parameters(cur_nimg=total_iters)`` and, when the step
    has an EMA copy and ``ema_kimgs`` is given, ``step.update_ema(batch_size, total_iters, ema_kimgs, ramp)``.  The last batch is partial, as the
    reference's loader leaves it.  ``where='device'``: the batches come from ``afcm_batch_assemble``, nothing is read back from the device;
    ``where='host'``: from ``SliceDataset`` items (``DeviceSliceSet.host_batch``), the same bits.  Both arms draw ``gen_z`` in the same order
    (``gen_z``: a fixed [batch_size, z_dim] tensor instead of a draw per batch).  ``augment``: the epoch's parameter table
    (``DeviceSliceSet.epoch_augment``) for a set built with ``augment``, ``intensity``: the epoch's intensity table (``epoch_intensity``) for one built with ``intensity``, ``elastic``: the epoch's elastic table
    (``epoch_elastic``) for one built with ``elastic`` (the host arm is ``augment_elastic.apply_host``), ``blur``: the epoch's blur table (``epoch_blur``) for one built with ``blur`` (the host arm is
    ``augment_blur.apply_host``); both arms apply them.  A set built with ``normalise`` feeds both arms through its normaliser.  Works with ``StyleGAN3GeneratorStep`` and
    ``StyleGAN3Step`` alike.
    Returns the new ``total_iters``."""
    if where not in ('device', 'host'):
        raise ValueError(f"where must be 'device' or 'host', got {where!r}")
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f'batch_size {batch_size}')
    items = dataset._checked_items(items)
    n = int(items.shape[0])
    device = next(step.netG.parameters()).device
    augment = dataset._checked_augment(augment, n, 'train_epoch')
    intensity = dataset._checked_intensity(intensity, n, 'train_epoch')
    elastic = dataset._checked_elastic(elastic, n, 'train_epoch')
    blur = dataset._checked_blur(blur, n, 'train_epoch')
    if where == 'device':
        dataset.load_epoch(items, augment, intensity, elastic, blur)
    schedule = getattr(step, 'schedule', None) if where == 'device' else None
    for first in range(0, n, batch_size):
        count = min(batch_size, n - first)
        batch = (lambda: dataset.batch(first, count)) if where == 'device' else (
            lambda: dataset.host_batch(items, first, count, device=device, augment=augment, intensity=intensity, elastic=elastic, blur=blur,
                                       normalise=dataset.normalise))
        total_iters += batch_size
        _fed_step(step, schedule, batch_size, batch, None if gen_z is None else gen_z[:count], cur_nimg=total_iters)
        if schedule is None and ema_kimgs is not None and getattr(step, 'netG_ema', None) is not None:
            step.update_ema(batch_size, total_iters, ema_kimgs=ema_kimgs, ramp=ramp)
    return total_iters


class TrainingGraph:
    """One training step fed from the device as ONE graph: ``assemble_batch`` into persistent tensors at the cursor, ``advance_cursor(batch_size)``,
    ``set_input``, ``optimize_parameters()`` -- ``stylegan3_model.capture_step``'s recipe (a side stream for warm-up and capture, a step built with
    ``capturable=True`` and without gradient buckets) with the batch inside the graph.  ``dataset`` must have an epoch loaded (``load_epoch``) of at
    least ``batch_size`` rows.  The warm-up runs real steps on the first rows, as ``capture_step``'s does, and leaves the cursor at row 0.

    ``replay()`` refreshes ``gen_z`` in place (``normal_()``, outside the graph; not with ``fixed_z``) and replays: one asynchronous launch, no
    synchronise.  It consumes ``batch_size`` rows and raises once fewer remain: the graph has ``drop_last`` geometry, so an epoch table should be a
    multiple of ``batch_size`` long.  ``load_epoch`` may be called between replays (the table is refreshed in place); ``rewind()`` starts the same
    table again.  The blur schedule and the EMA update stay on the host between replays, as with ``capture_step`` -- unless the step was built with
    a ``DeviceSchedule`` (afcm_amd/schedule.py): then the captured body begins with ``schedule.advance(batch_size)`` and, when the step has an EMA copy
    and the schedule an ``ema_kimgs``, ends with ``step.update_ema()``; sigma, beta and the learning rates are read from the schedule block at every
    replay, and the warm-up leaves the block as it found it.  ``undo_warmup=True`` puts the networks' parameters and buffers and the optimizers' state
    back as well (in place: the graph keeps pointing at them), so that the warm-up's real steps leave no trace; the default keeps them, as
    ``capture_step`` does.  A step built with ``log=DeviceTrainLog(...)`` appends a row in every warm-up step and in every replay; the warm-up always puts
    the log's ``head`` back, and with ``undo_warmup=True`` the ring's contents and the optimizers' gradient statistics as well.  ``gen_z``: the initial (with ``fixed_z``: the only) latent batch; drawn when None.  A dataset built with ``augment``
    is captured with ``afcm_batch_assemble_aug``: the parameter table is persistent as the item table is, and the cursor moves through both; one built with
    ``intensity`` with ``afcm_batch_assemble_noise``, its table persistent in the same way; one built with ``elastic`` with the launches of
    ``afcm_batch_assemble_elastic`` -- a fixed number, each skipping on the device the items whose flag is 0 -- and the graph keeps the workspace
    it was captured with; one built with ``blur`` with the launches of ``afcm_batch_assemble_blur``, fixed in number as well, the workspace kept
    likewise; one built with ``normalise`` with ``afcm_plane_norm_stats`` and ``afcm_batch_assemble_norm``, the coefficient buffer kept likewise."""

    def __init__(self, step, dataset, batch_size, warmup=3, fixed_z=False, dtype=torch.float32, gen_z=None, undo_warmup=False):
        require_capturable(step, 'TrainingGraph')
        dataset._need_device('TrainingGraph')
        batch_size = int(batch_size)
        if batch_size < 1 or dataset.rows < batch_size:
            raise RuntimeError(f'TrainingGraph: batch size {batch_size} with a loaded epoch of {dataset.rows} rows (load_epoch first)')
        self.step, self.dataset, self.batch_size, self.fixed_z = step, dataset, batch_size, bool(fixed_z)
        device = dataset.device
        h, w = dataset.patch_shape[1:]
        self.real_A = torch.empty((batch_size, dataset.slice_num, h, w), dtype=dtype, device=device)
        self.real_B = torch.empty((batch_size, 1, h, w), dtype=dtype, device=device)
        self.slice_idx = torch.empty((batch_size, 1), dtype=torch.float32, device=device)
        self.gen_z = torch.randn([batch_size, step.netG.z_dim], device=device) if gen_z is None else gen_z.to(device).clone()
        if tuple(self.gen_z.shape) != (batch_size, step.netG.z_dim):
            raise RuntimeError(f'TrainingGraph: gen_z must be [{batch_size}, {step.netG.z_dim}], got {tuple(self.gen_z.shape)}')

        schedule = getattr(step, 'schedule', None)
        saved = None if schedule is None else schedule.block.clone()
        optimizers = [opt for opt in (step.optimizer_G, getattr(step, 'optimizer_D', None)) if opt is not None]
        log = getattr(step, 'log', None)
        logged = None if log is None else log.snapshot()
        if undo_warmup:
            tensors = [t for name in step.model_names for net in [getattr(step, 'net' + name)] for t in list(net.parameters()) + list(net.buffers())]
            before = [t.detach().clone() for t in tensors], [opt.snapshot() for opt in optimizers]

        def cursor_batch():
            out = dataset.batch(0, batch_size, out=(self.real_A, self.real_B, self.slice_idx), use_cursor=True)
            advance_cursor(dataset.cursor, batch_size)
            return out

        def next_rows():                                      # what replay() does around the graph
            if dataset.position + batch_size > dataset.rows:
                dataset.rewind()
            if not self.fixed_z:
                self.gen_z.normal_()
            dataset.position += batch_size

        def leave_no_trace():
            dataset.rewind()
            if saved is not None:
                schedule.block.copy_(saved)               # the warm-up's steps are real ones, but total_iters stays where it was
            if log is not None:                           # the warm-up's rows stay in the ring unless it is undone; the serials go on from where they were
                log.restore(logged, head_only=not undo_warmup)
            if undo_warmup:
                with torch.no_grad():
                    for t, v in zip(tensors, before[0]):
                        t.copy_(v)
                for opt, state in zip(optimizers, before[1]):
                    opt.restore(state)

        self.graph = capture_graph(lambda: _fed_step(step, schedule, batch_size, cursor_batch, self.gen_z), warmup, next_rows, leave_no_trace)
        self.elastic_workspace = dataset.elastic_workspace    # the captured launches point into it, whatever the set allocates later
        self.norm_coef = dataset.norm_coef                    # likewise the coefficients of a set built with normalise

    def load_epoch(self, items, augment=None, intensity=None, elastic=None, blur=None):
        self.dataset.load_epoch(items, augment, intensity, elastic, blur)

    def rewind(self):
        self.dataset.rewind()

    def replay(self):
        if self.dataset.position + self.batch_size > self.dataset.rows:
            raise RuntimeError(f'TrainingGraph.replay: {self.dataset.rows - self.dataset.position} rows remain of an epoch of {self.dataset.rows}, a batch '
                               f'needs {self.batch_size}: load_epoch() or rewind()')
        if not self.fixed_z:
            self.gen_z.normal_()
        self.graph.replay()
        self.dataset.position += self.batch_size


def train_epochs(step, dataset, batch_size, epochs, lr_schedule, rng, graph=True, on_epoch=None, gen_z=None):
    """The outer loop of the reference's train.py:38-45 for a step built with a ``DeviceSchedule``.  ``epochs``: an iterable of epoch numbers
    (``range(epoch_count, n_epochs + n_epochs_decay + 1)``).  Per epoch: ``step.set_lr(lr_schedule.lr_at(k))`` for G and D, k = 1 for the first
    (``update_learning_rate()`` at the top of every epoch); ``dataset.epoch_items(rng)``, for a set built with ``augment`` ``epoch_augment(rng)``
    right after it, for one built with ``intensity`` ``epoch_intensity(rng)`` after that, for one built with ``elastic`` ``epoch_elastic(rng)`` after that, for one built with ``blur`` ``epoch_blur`` last -- from a ``random.Random``
    seeded by one extra draw of ``rng``, ``rng.integers(0, 2 ** 63)``, taken only when ``blur`` is configured -- and ``load_epoch``; then replays of ONE ``TrainingGraph``
    built in the first epoch (``graph=False``: eager steps, the same kernels) until fewer than ``batch_size`` rows remain; ``on_epoch(epoch, step)``
    -- validation and checkpoints are the caller's, through ``validation.validate`` and ``step.save_networks``.  ``rng``: a seed or a
    ``numpy.random.Generator``; an int seeds one generator for the whole run.  ``gen_z``: one fixed [batch_size, z_dim] latent batch for every step
    instead of a draw per step.  The graph is built with ``undo_warmup=True``, so the run is the same steps on the same rows with and
    without the graph.  A step built with ``log=DeviceTrainLog(...)`` leaves one row per step in device memory, the same rows with and without the graph;
    nothing here reads them: ``step.log.read()`` inside ``on_epoch`` is one device -> host copy per epoch.  Returns the number of steps run."""
    schedule = getattr(step, 'schedule', None)
    if schedule is None:
        raise RuntimeError('train_epochs needs a step built with schedule=DeviceSchedule(...)')
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f'batch_size {batch_size}')
    rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
    runner, steps = None, 0
    for k, epoch in enumerate(epochs, start=1):
        lr = lr_schedule.lr_at(k)
        step.set_lr(lr, lr)
        items = dataset.epoch_items(rng)
        augment = dataset.epoch_augment(rng) if dataset.augment is not None else None
        intensity = dataset.epoch_intensity(rng) if dataset.intensity is not None else None
        elastic = dataset.epoch_elastic(rng) if dataset.elastic is not None else None
        blur = dataset.epoch_blur(random.Random(int(rng.integers(0, 2 ** 63)))) if dataset.blur is not None else None
        dataset.load_epoch(items, augment, intensity, elastic, blur)
        if dataset.rows < batch_size:
            raise RuntimeError(f'train_epochs: an epoch of {dataset.rows} rows is shorter than a batch of {batch_size}')
        if graph and runner is None:
            runner = TrainingGraph(step, dataset, batch_size, fixed_z=gen_z is not None, gen_z=gen_z, undo_warmup=True)
        for first in range(0, dataset.rows - batch_size + 1, batch_size):
            if graph:
                runner.replay()
            else:
                _fed_step(step, schedule, batch_size, lambda: dataset.batch(first, batch_size), gen_z)
            steps += 1
        if on_epoch is not None:
            on_epoch(epoch, step)
    return steps
