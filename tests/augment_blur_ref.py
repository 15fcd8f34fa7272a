"""An independent restatement of the reference's ``GaussianBlur3D`` (data/augment/transforms.py:716-726) with scipy called directly on the
``[1, h, w]`` plane the loader hands the class: ``gaussian_filter(x, sigma, mode='nearest', truncate=4.0)``, the call skimage's ``gaussian``
documents for a float array (skimage itself is not installed where these tests run).  Nothing here is shared with afcm_amd/augment_blur.py."""
import numpy as np
from scipy.ndimage import gaussian_filter

SHAPES = [(1, 3, 2), (1, 5, 7), (1, 20, 23), (1, 64, 64), (1, 256, 256)]
SIGMAS = [0.1, 0.12, 0.125, 0.3, 0.374, 0.376, 0.9, 1.0, 1.37, 2.0, 3.3, 4.1]


def blur(volume, sigma):
    """The class's filter on one ``[1, h, w]`` float64 volume."""
    return gaussian_filter(np.asarray(volume, dtype=np.float64), sigma, mode='nearest', truncate=4.0)


def volume(shape, seed, float32_valued):
    """Normalised-looking values in [-1, 1]: any float64, or float64 holding float32 values (what ``Normalize`` hands on from a uint8 source)."""
    v = np.random.default_rng(seed).uniform(-1.0, 1.0, shape)
    return v.astype(np.float32).astype(np.float64) if float32_valued else v


def numpy_blur_item(planes, row, cols=20):
    """The stage on a float32 [k, h, w] item from the row's records, through scipy-free numpy written a second time: explicit loops over the taps
    on padded lines (np.pad 'edge'), so that the GPU tests' NaN cases have a restatement that shares no code with the module."""
    out = planes.copy()
    for p, rec in enumerate(np.asarray(row, dtype=np.float64).reshape(-1, cols)):
        if rec[0] != 1.0:
            continue
        r, w = int(rec[2]), rec[3:]
        v = planes[p].astype(np.float64)
        t = v * w[0]
        for j in range(r, 0, -1):
            t = t + (v + v) * w[j]
        for axis in (0, 1):
            n = t.shape[axis]
            pad = np.pad(t, [(r, r) if a == axis else (0, 0) for a in (0, 1)], mode='edge')
            take = lambda s: pad[s:s + n] if axis == 0 else pad[:, s:s + n]
            acc = take(r) * w[0]
            for j in range(r, 0, -1):
                acc = acc + (take(r - j) + take(r + j)) * w[j]
            t = acc
        out[p] = t.astype(np.float32)
    return out


# every kind of invalid plane record: name -> (column within the record, value)
INVALID = {
    'flag 2': (0, 2.0), 'flag 0.5': (0, 0.5), 'flag nan': (0, np.nan),
    'sigma nan': (1, np.nan), 'sigma 0': (1, 0.0), 'sigma -1': (1, -1.0), 'sigma inf': (1, np.inf),
    'radius 17': (2, 17.0), 'radius 0.5': (2, 0.5), 'radius -1': (2, -1.0), 'radius nan': (2, np.nan),
    'weight inf': (4, np.inf), 'weight -inf': (3, -np.inf), 'weight nan': (19, np.nan),
}
