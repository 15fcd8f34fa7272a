"""numpy restatement of the two kernels of afcm_amd/csrc/volume.hip AS THE KERNELS COMPUTE: ``assemble`` evaluates every output element from its own
coordinates (crop / pad offset, plane position, normalisation in the type numpy gives the expression), ``accumulate`` is the per-voxel gather over the
batch's patches in ascending order.  Independent of afcm_amd/predictor.py and afcm_amd/data.py, against which tests/test_volume_ref_cpu.py holds it;
tests/test_gpu_volume.py holds the kernels against the host code directly.  Also the accumulator cases both test files share."""
import numpy as np

# name: (volume shape, patch shape, stride shape, halo, batch, channels, prediction_channel)
ACCUMULATOR_CASES = {
    'a_ragged_d1': ((5, 40, 44), (1, 16, 16), (1, 8, 8), (0, 4, 4), 3, 1, None),
    'b_deep': ((12, 40, 44), (8, 16, 16), (4, 8, 8), (2, 4, 4), 3, 1, None),
    'c_broadcast_quirk': ((12, 40, 44), (8, 16, 16), (4, 8, 8), (0, 4, 4), 3, 1, None),
    'd_prediction_channel': ((6, 24, 24), (4, 12, 12), (2, 6, 6), (1, 2, 2), 5, 2, 1),
    'e_mask_wraps': ((1, 32, 32), (1, 16, 16), (1, 1, 1), (0, 0, 0), 16, 1, None),
}


def source(shape, dtype, seed=3):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if dtype == np.int16:
        return rng.integers(-300, 1200, shape).astype(np.int16)
    return (rng.standard_normal(shape) * 400 + 400).astype(dtype)


ASSEMBLY_CASES = {   # name: (source shape, dtype, (H, W), thickness, slice_num, (min, max))
    'crop_u8': ((23, 40, 36), np.uint8, (32, 32), 5, 4, (0., 255.)),
    'pad_u8': ((23, 28, 30), np.uint8, (32, 32), 5, 4, (0., 255.)),
    'crop_and_pad_u8': ((23, 40, 27), np.uint8, (32, 32), 5, 4, (0., 255.)),
    'single_slice': ((23, 28, 36), np.uint8, (32, 32), 5, 1, (0., 255.)),
    'single_slice_no_thickness': ((23, 28, 36), np.uint8, (32, 32), None, 1, (0., 255.)),
    'pad_i16': ((23, 28, 30), np.int16, (32, 32), 5, 4, (-100., 900.)),
    'pad_f32': ((23, 28, 30), np.float32, (32, 32), 5, 4, (-100., 900.)),
    'crop_f32': ((23, 40, 36), np.float32, (32, 32), 5, 4, (-100., 900.)),
    'pad_f64': ((23, 28, 30), np.float64, (32, 32), 5, 4, (-100., 900.)),
    # rows that are no whole number of 16-byte runs.  W = 10: float32 rows of 40 bytes start on and off a 16-byte boundary in turn, 16-bit rows are
    # one run and a tail of 2; W = 6: shorter than a 16-bit run.  x cropped (u8, f32, f64) and padded (i16), y padded (f32) and cropped (the rest)
    'tail_u8': ((11, 13, 18), np.uint8, (12, 10), 3, 4, (0., 255.)),
    'tail_f32': ((11, 9, 23), np.float32, (12, 10), 5, 4, (-100., 900.)),
    'tail_i16_k1': ((7, 16, 7), np.int16, (12, 10), None, 1, (-100., 900.)),
    'narrow_f64': ((7, 20, 16), np.float64, (8, 6), 2, 4, (-100., 900.)),
}


def zero_plane_targets(depth, thickness):
    """The targets whose plane 0 (the thick slice before the target's own) and whose plane 3 (the second after it) lie outside the volume."""
    own = [(i // thickness) * thickness for i in range(depth)]
    return [i for i in range(depth) if own[i] - thickness < 0], [i for i in range(depth) if own[i] + 2 * thickness > depth - 1]


def starts(n, k, s):
    """Patch origins along one axis: regular strides, the last patch pulled back to end at the border."""
    out = list(range(0, n - k + 1, s))
    if out[-1] + k < n:
        out.append(n - k)
    return out


def origins(volume_shape, patch_shape, stride_shape):
    """int32 [P, 3], z outermost."""
    axes = [starts(n, k, s) for n, k, s in zip(volume_shape, patch_shape, stride_shape)]
    return np.array([(z, y, x) for z in axes[0] for y in axes[1] for x in axes[2]], dtype=np.int32)


def random_predictions(count, channels, patch_shape, seed):
    """An independent float32 tensor per patch (NOT the volume's own voxels: an ordering error must show)."""
    return np.random.default_rng(seed).standard_normal((count, channels) + tuple(patch_shape)).astype(np.float32)


def _cover(o, p, n, a, v):
    """One axis of the kernel's halo_cover for the voxel coordinates ``v``: (covered, patch coordinate)."""
    lo = 0 if o == 0 else o + a
    border_stop = o + p == n
    hi = n if border_stop else o + p - a
    src = np.zeros_like(v) if (not border_stop and a == 0) else v - o
    return (v >= lo) & (v < hi) & (src >= 0) & (src < p), src


def accumulate(prediction_map, mask, prediction, patch_origins, halo, prediction_channel=None):
    """One launch of halo_accumulate_kernel: every voxel walks the batch's patches in ascending order; one float32 add and one wrapping uint8
    increment per covering patch.  prediction [B, C, d, h, w] (any float dtype numpy widens exactly); in place."""
    cm, D, H, W = prediction_map.shape
    p = prediction.shape[2:]
    vz, vy, vx = np.arange(D), np.arange(H), np.arange(W)
    for i, (oz, oy, ox) in enumerate(np.asarray(patch_origins)):
        cz, sz = _cover(int(oz), p[0], D, halo[0], vz)
        cy, sy = _cover(int(oy), p[1], H, halo[1], vy)
        cx, sx = _cover(int(ox), p[2], W, halo[2], vx)
        if not (cz.any() and cy.any() and cx.any()):
            continue
        at = np.ix_(vz[cz], vy[cy], vx[cx])
        frm = np.ix_(sz[cz], sy[cy], sx[cx])
        for c in range(cm):
            src = prediction[i, prediction_channel if prediction_channel is not None else c]
            prediction_map[c][at] = prediction_map[c][at] + src[frm].astype(np.float32)
            mask[c][at] = mask[c][at] + np.uint8(1)


def predict(volume_shape, patch_origins, predictions, batch, halo, prediction_channel=None):
    """Batches of ``batch`` patches in sequence, then map / mask.  Returns (quotient, map, mask)."""
    cm = 1 if prediction_channel is not None else predictions.shape[1]
    prediction_map = np.zeros((cm,) + tuple(volume_shape), dtype=np.float32)
    mask = np.zeros((cm,) + tuple(volume_shape), dtype=np.uint8)
    for first in range(0, len(patch_origins), batch):
        accumulate(prediction_map, mask, predictions[first:first + batch], patch_origins[first:first + batch], halo, prediction_channel)
    with np.errstate(divide='ignore', invalid='ignore'):
        return prediction_map / mask, prediction_map, mask


def _crop_offset(have, want):
    return (have - want) // 2 if want < have else -((want - have) // 2)


def _normalised(m, lo, hi):
    """data.normalize's expression on an array of m's type: float32 arithmetic for a float32 array (numpy keeps the array's type against Python
    scalars, so min and max - min are rounded to float32 first), float64 for everything else; then one rounding to float32."""
    if m.dtype == np.float32:
        v = np.float32(2) * ((m - np.float32(lo)) / np.float32(hi - lo)) - np.float32(1)
    else:
        m = m.astype(np.float64)
        v = 2.0 * ((m - lo) / (hi - lo)) - 1.0
    return np.minimum(np.maximum(v, -1), 1).astype(np.float32)


def assemble(src, first, count, k, thickness, h, w, lo=0.0, hi=255.0):
    """slice_assemble_kernel, element by element (vectorised over a plane): A [count, k, h, w] float32 and slice_idx [count, 1] float32.
    ``thickness`` None is the loader's -1 (k = 1 only)."""
    depth, hs, ws = src.shape
    t = -1 if thickness is None else int(thickness)
    oy, ox = _crop_offset(hs, h), _crop_offset(ws, w)
    ys, xs = np.arange(h) + oy, np.arange(w) + ox
    inside = ((ys >= 0) & (ys < hs))[:, None] & ((xs >= 0) & (xs < ws))[None, :]
    yc, xc = np.clip(ys, 0, hs - 1), np.clip(xs, 0, ws - 1)
    a = np.empty((count, k, h, w), dtype=np.float32)
    slice_idx = np.empty((count, 1), dtype=np.float32)
    for i in range(count):
        idx = first + i
        idx_a = (idx // t) * t if k == 4 else idx
        for plane in range(k):
            pos = idx_a + (plane - 1) * t if k == 4 else idx
            if pos < 0 or pos > depth - 1:
                m = np.zeros((h, w), dtype=np.float64)                                   # a plane of float64 zeros before normalisation
            else:
                m = np.where(inside, src[pos][np.ix_(yc, xc)], np.zeros((), dtype=src.dtype))   # a padded pixel: a zero of the source's type
            a[i, plane] = _normalised(m, lo, hi)
        slice_idx[i, 0] = np.float32(idx - idx_a) / np.float32(t)
    return a, slice_idx
