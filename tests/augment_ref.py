"""numpy restatement of the augmenting gather of batch_augment_kernel (afcm_amd/csrc/batch.hip), without scipy: for a parameter row
``(flip_h, flip_w, k, angle, c, s, off_y, off_x)`` the item-plane pixel every output pixel reads -- the reference's chain RandomFlip, RandomRotate90,
RandomRotate (data/augment/transforms.py:25-112) walked backwards in exact integer arithmetic and float64 operations rounded one by one, as the
kernel evaluates it.  tests/test_augment_ref_cpu.py holds it to the golden captured from the reference's classes, to ``scipy.ndimage.rotate``,
``np.flip`` and ``np.rot90``; tests/test_gpu_augment.py holds the kernel to ``afcm_amd.augment.apply_host``, which that file holds to this one."""
import numpy as np


def reflect(i, n):
    """Half-sample symmetric reflection of integer coordinates into [0, n): (d c b a | a b c d | d c b a), any number of periods."""
    m = np.mod(i, 2 * n)                                  # numpy's mod is non-negative for a positive modulus
    return np.where(m >= n, 2 * n - 1 - m, m)


def row_valid(row, h, w):
    """The kernel's check of a parameter row."""
    flip_h, flip_w, k, _, c, s, off_y, off_x = (float(v) for v in row)
    return bool(flip_h in (0.0, 1.0) and flip_w in (0.0, 1.0) and k in (0.0, 1.0, 2.0, 3.0) and (k in (0.0, 2.0) or h == w) and
                abs(c) <= 1.0 and abs(s) <= 1.0 and abs(off_y) <= h + w and abs(off_x) <= h + w)


def source_index(row, h, w):
    """``(sy, sx)`` int64 [h, w]: output pixel (y, x) of the augmented plane is item-plane pixel (sy[y, x], sx[y, x])."""
    assert row_valid(row, h, w), row
    flip_h, flip_w, k = (int(v) for v in row[:3])
    c, s, off_y, off_x = (np.float64(v) for v in row[4:])
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    iy = (y * c + x * s) + off_y
    ix = (y * (-s) + x * c) + off_x
    ry = reflect(np.floor(iy + 0.5).astype(np.int64), h)
    rx = reflect(np.floor(ix + 0.5).astype(np.int64), w)
    # numpy.rot90(p1, k)[ry, rx] = p1[py, px]
    py, px = {0: (ry, rx), 1: (rx, w - 1 - ry), 2: (h - 1 - ry, w - 1 - rx), 3: (h - 1 - rx, ry)}[k]
    return (h - 1 - py if flip_h else py), (w - 1 - px if flip_w else px)


def augment_planes(planes, row):
    """[C, h, w] -> [C, h, w]: every plane gathered through the row's source index."""
    planes = np.asarray(planes)
    sy, sx = source_index(row, planes.shape[1], planes.shape[2])
    return np.ascontiguousarray(planes[:, sy, sx])
