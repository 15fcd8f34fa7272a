"""Geometric training augmentation as parameter rows: the reference's ``RandomFlip``, ``RandomRotate90`` and ``RandomRotate``
(data/augment/transforms.py:25-112, offered for the train phase by configs/defaults.py:62-76) for the device loader.

All three are gathers once an item's parameters are known, so an epoch's augmentation is a float64 table of one row per item,
``(flip_h, flip_w, k, angle, c, s, off_y, off_x)``, beside the int32 item table: ``augment_rows`` draws it, ``afcm_batch_assemble_aug``
(torch_utils/ops/batch_ops.py) applies it inside the batch launch, ``apply_host`` applies it with numpy / scipy as the reference's classes do -- the
comparison arm.  The rotation's coefficients are computed here, on the host, with the functions ``scipy.ndimage.rotate`` itself uses
(``scipy.special.cosdg`` / ``sindg``: ``math.cos(math.radians(a))`` differs from ``cosdg(a)`` in the last bit at most integer angles), so the kernel
evaluates no trigonometric function and the two arms agree bit for bit.
"""
import dataclasses

import numpy as np
import torch
from scipy import ndimage, special

ROW = 8                                                   # flip_h, flip_w, k, angle, c, s, off_y, off_x


@dataclasses.dataclass(frozen=True)
class AugmentConfig:
    """``flip_axes``: the axes ``RandomFlip`` may flip, a subset of {1, 2} -- H and W of the plane in the reference's [D, H, W] numbering (its
    default, axis 0, flips the single slice onto itself).  ``rotate90``: ``RandomRotate90``, square patches only.  ``angle_spectrum``: ``RandomRotate``
    with ``axes=[[2, 1]]``, ``order=0``, ``mode='reflect'`` and this spectrum (an int >= 1), None to leave it off."""
    flip_axes: tuple = ()
    rotate90: bool = False
    angle_spectrum: object = None

    def __post_init__(self):
        axes = tuple(self.flip_axes)
        if any(isinstance(a, bool) or not isinstance(a, (int, np.integer)) or a not in (1, 2) for a in axes) or len(set(axes)) != len(axes):
            raise RuntimeError(f'AugmentConfig: flip_axes must be distinct axes out of 1 (H) and 2 (W), got {self.flip_axes!r}')
        object.__setattr__(self, 'flip_axes', tuple(int(a) for a in axes))
        if not isinstance(self.rotate90, (bool, np.bool_)):
            raise RuntimeError(f'AugmentConfig: rotate90 must be a bool, got {self.rotate90!r}')
        object.__setattr__(self, 'rotate90', bool(self.rotate90))
        s = self.angle_spectrum
        if s is not None:
            if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or s < 1:
                raise RuntimeError(f'AugmentConfig: angle_spectrum must be an int >= 1 or None, got {s!r}')
            object.__setattr__(self, 'angle_spectrum', int(s))

    def check_patch(self, patch_hw, what):
        h, w = (int(v) for v in patch_hw)
        if self.rotate90 and h != w:
            raise RuntimeError(f'{what}: rotate90 needs a square patch, got [{h}, {w}] (a quarter turn would change the item\'s shape)')


def rotation(angle, patch_hw):
    """``(c, s, off_y, off_x)`` of ``scipy.ndimage.rotate(plane, angle, reshape=False)`` on an [h, w] plane, as that function forms them."""
    h, w = (int(v) for v in patch_hw)
    c, s = special.cosdg(angle), special.sindg(angle)
    matrix = np.array([[c, s], [-s, c]])
    centre = (np.array([h, w]) - 1) / 2
    off = centre - matrix @ centre
    return float(c), float(s), float(off[0]), float(off[1])


def identity_rows(n):
    """``n`` rows that change nothing: no flip, no turn, angle 0."""
    rows = np.zeros((int(n), ROW), dtype=np.float64)
    rows[:, 4] = 1.0
    return rows


def make_rows(flip_h, flip_w, k, angle, patch_hw):
    """Rows from given parameters (arrays of one length, or scalars broadcast against them)."""
    flip_h, flip_w, k, angle = np.broadcast_arrays(*(np.atleast_1d(np.asarray(v)) for v in (flip_h, flip_w, k, angle)))
    rows = identity_rows(len(angle))
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = flip_h, flip_w, k, angle
    for a in np.unique(angle):
        rows[angle == a, 4:] = rotation(int(a), patch_hw)
    return rows


def augment_rows(config, n, patch_hw, rng):
    """float64 [n, 8]: one draw of ``config``'s transforms per item.  The distributions are the reference's -- an axis is flipped when
    ``uniform() > 0.5``, ``k = integers(0, 4)``, ``angle = integers(-S, S)`` -- from a ``numpy.random.Generator`` in a fixed order: the flips
    ([n, len(flip_axes)], one column per axis in ``flip_axes`` order), then the ``k``s, then the angles; a transform that is off draws nothing.
    The reference's own stream is not reproduced: it reseeds every transform with one fixed seed per subject
    (transforms.py:729-769), so every item of a subject gets the same draw."""
    if not isinstance(config, AugmentConfig):
        raise RuntimeError(f'augment_rows: config must be an AugmentConfig, got {type(config).__name__}')
    if not isinstance(rng, np.random.Generator):
        raise RuntimeError(f'augment_rows: rng must be a numpy.random.Generator, got {type(rng).__name__}')
    n = int(n)
    if n < 1:
        raise RuntimeError(f'augment_rows: {n} rows')
    config.check_patch(patch_hw, 'augment_rows')
    flips = np.zeros((n, 2), dtype=bool)
    if config.flip_axes:
        draws = rng.uniform(size=(n, len(config.flip_axes))) > 0.5
        for j, axis in enumerate(config.flip_axes):
            flips[:, axis - 1] = draws[:, j]
    k = rng.integers(0, 4, n) if config.rotate90 else np.zeros(n, dtype=np.int64)
    s = config.angle_spectrum
    angle = rng.integers(-s, s, n) if s is not None else np.zeros(n, dtype=np.int64)
    return make_rows(flips[:, 0], flips[:, 1], k, angle, patch_hw)


def checked_rows(rows, n, what):
    rows = np.ascontiguousarray(np.asarray(rows))
    if rows.ndim != 2 or rows.shape[1] != ROW or rows.dtype != np.float64 or rows.shape[0] != int(n):
        raise RuntimeError(f'{what}: an augment table is float64 [{int(n)}, {ROW}], one row per item, got {rows.dtype} {rows.shape}')
    return rows


def apply_host(planes, row):
    """The host arm: ``row`` applied to a [C, H, W] tensor or ndarray as the reference's classes apply it to each [1, H, W] plane -- ``np.flip``,
    ``np.rot90(m, k, (1, 2))``, ``scipy.ndimage.rotate(m, angle, axes=(2, 1), reshape=False, order=0, mode='reflect', cval=-1)``.  All three are
    gathers, so applying them to the float32 item gives the bits that applying them before the cast gives.  Returns the type it was given."""
    row = np.asarray(row, dtype=np.float64)
    if row.shape != (ROW,):
        raise RuntimeError(f'apply_host: a parameter row has {ROW} values, got shape {row.shape}')
    m = planes.numpy() if isinstance(planes, torch.Tensor) else np.asarray(planes)
    if m.ndim != 3:
        raise RuntimeError(f'apply_host: planes must be [C, H, W], got shape {tuple(m.shape)}')
    flip_h, flip_w, k, angle = (int(v) for v in row[:4])
    if (flip_h, flip_w, k, angle) != tuple(row[:4]) or flip_h not in (0, 1) or flip_w not in (0, 1) or k not in (0, 1, 2, 3):
        raise RuntimeError(f'apply_host: flips are 0 or 1, k is 0..3 and the angle a whole number of degrees, got {row[:4].tolist()}')
    if k % 2 and m.shape[1] != m.shape[2]:
        raise RuntimeError(f'apply_host: an odd number of quarter turns needs square planes, got {tuple(m.shape)}')
    if tuple(row[4:]) != rotation(angle, m.shape[1:]):
        raise RuntimeError(f'apply_host: the row\'s coefficients {row[4:].tolist()} are not those of angle {angle} on [{m.shape[1]}, {m.shape[2]}]')
    if flip_h:
        m = np.flip(m, 1)
    if flip_w:
        m = np.flip(m, 2)
    m = np.rot90(m, k, (1, 2))
    m = ndimage.rotate(m, angle, axes=(2, 1), reshape=False, order=0, mode='reflect', cval=-1)
    m = np.ascontiguousarray(m)
    return torch.from_numpy(m) if isinstance(planes, torch.Tensor) else m
