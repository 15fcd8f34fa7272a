"""An independent restatement of the reference's ``ElasticDeformation`` (data/augment/transforms.py:138-191) with scipy called directly on the
``[1, h, w]`` plane the loader hands the class: ``gaussian_filter`` for the three (or two) displacement fields, ``map_coordinates`` for the read.
Nothing here is shared with afcm_amd/augment_elastic.py: no folded operator, no index folding, no spline recursion of the project's own.

scipy's ``mode='reflect'`` prefilter is the exact interpolating spline only on long lines (its residual falls off as ``(sqrt(3) - 2)^(2n)`` and is
at rounding level from about n = 16), so every comparison against this module uses planes of at least 20 in both extents."""
import numpy as np
from scipy.ndimage import gaussian_filter, map_coordinates, spline_filter

MIN_EXTENT = 20


def displacement(field, sigma, alpha):
    """``gaussian_filter(field, sigma, mode='reflect') * alpha`` on the ``[1, h, w]`` volume the class filters; float64 [h, w]."""
    field = np.asarray(field, dtype=np.float64)
    assert min(field.shape) >= MIN_EXTENT
    return (gaussian_filter(field[None], sigma, mode='reflect') * alpha)[0]


def coefficients(plane):
    """scipy's own cubic prefilter of a plane, mode 'reflect'."""
    plane = np.asarray(plane, dtype=np.float64)
    assert min(plane.shape) >= MIN_EXTENT
    return spline_filter(plane, order=3, mode='reflect')


def deform(plane, dy, dx, order, dz=None):
    """``map_coordinates`` of the ``[1, h, w]`` plane at ``(z + dz, y + dy, x + dx)``, as the class calls it; float64 [h, w]."""
    plane = np.asarray(plane, dtype=np.float64)
    assert min(plane.shape) >= MIN_EXTENT
    h, w = plane.shape
    z, y, x = np.meshgrid(np.arange(1), np.arange(h), np.arange(w), indexing='ij')
    dz = np.zeros((1, h, w)) if dz is None else np.asarray(dz, dtype=np.float64)[None]
    return map_coordinates(plane[None], (z + dz, y + dy[None], x + dx[None]), order=order, mode='reflect')[0]


def elastic(plane, draw, fields, order, alpha, sigma, probability, apply_3d):
    """The whole class for one plane: ``draw`` is the decision draw, ``fields = (Fz, Fy, Fx)`` the three standard normal fields in the order the
    class draws them (``Fz`` is drawn with ``apply_3d`` only, and ignored without)."""
    if not draw < probability:
        return np.asarray(plane, dtype=np.float64)
    fz, fy, fx = fields
    dz = displacement(fz, sigma, alpha) if apply_3d else None
    return deform(plane, displacement(fy, sigma, alpha), displacement(fx, sigma, alpha), order, dz)


# every kind of invalid elastic row: name -> (column, value)
INVALID = {
    'flag 2': (0, 2.0), 'flag 0.5': (0, 0.5), 'flag -1': (0, -1.0), 'flag nan': (0, np.nan),
    'alpha nan': (1, np.nan), 'alpha inf': (1, np.inf), 'alpha -inf': (1, -np.inf), 'alpha above 2^20': (1, np.nextafter(2.0 ** 20, np.inf)),
    'alpha below -2^20': (1, -np.nextafter(2.0 ** 20, np.inf)),
    'key_lo -1': (2, -1.0), 'key_lo 2^32': (2, 2.0 ** 32), 'key_lo fraction': (2, 7.5), 'key_lo nan': (2, np.nan), 'key_lo inf': (2, np.inf),
    'key_hi -1': (3, -1.0), 'key_hi 2^32': (3, 2.0 ** 32), 'key_hi fraction': (3, 0.25), 'key_hi nan': (3, np.nan),
}
