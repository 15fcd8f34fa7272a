"""Independent scalar restatements for the intensity augmentation (afcm_amd/augment_intensity.py, batch_intensity_kernel in afcm_amd/csrc/batch.hip):
Philox4x32-10 on Python integers, Box-Muller through the ``math`` library, the Poisson count by a plain search and the three transforms' arithmetic
on Python floats (IEEE doubles, one rounding per operation).  tests/test_augment_intensity_ref_cpu.py holds the numpy host arm to these, to the
generator's published known answers and to the golden captured from the reference's classes; tests/test_gpu_augment_intensity.py holds the kernel to
the host arm."""
import math

import numpy as np

M0, M1, W0, W1, MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF

# (counter, key, output) of Philox4x32-10: the Random123 known-answer tests
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

# every kind of invalid row, as (column, value) edits of a valid row with J = 24: what the host arm refuses and the kernel turns into a NaN item
INVALID = {'contrast flag 2': (0, 2.0), 'Gaussian flag one half': (3, 0.5), 'Poisson flag -1': (5, -1.0), 'flag not a number': (3, np.nan),
           'alpha infinite': (1, np.inf), 'alpha not a number': (1, np.nan), 'mean infinite': (2, -np.inf), 'mean not a number': (2, np.nan),
           'std negative': (4, -0.5), 'std infinite': (4, np.inf), 'std not a number': (4, np.nan), 'key_lo 2^32': (7, 2.0 ** 32), 'key_hi negative': (8, -1.0),
           'key_lo fractional': (7, 0.5), 'key_hi not a number': (8, np.nan), 'J of 25': (9, 25.0), 'J negative': (9, -1.0), 'J fractional': (9, 1.5),
           'J not a number': (9, np.nan), 'T_0 negative': (10, -1.0), 'T_5 fractional': (15, 1000.5), 'T_23 above 2^32': (33, 2.0 ** 32 + 1),
           'T_7 not a number': (17, np.nan)}


def philox4x32(counter, key, rounds=10):
    c0, c1, c2, c3 = (int(v) for v in counter)
    k0, k1 = (int(v) for v in key)
    for _ in range(rounds):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def pixel_word(key, y, x, stream, plane=0):
    return philox4x32((x >> 2, y, stream | (plane << 1), 0), key)[x & 3]


def normal_math(key, y, x, plane=0):
    """The pixel's normal with the C library's log / cos / sin in place of the project's series."""
    w = philox4x32((x >> 2, y, plane << 1, 0), key)
    wa, wb = (w[0], w[1]) if (x & 3) < 2 else (w[2], w[3])
    u1, u2 = (wa + 0.5) / 2.0 ** 32, wb / 2.0 ** 32
    r = math.sqrt(-2.0 * math.log(u1))
    return r * (math.cos(2.0 * math.pi * u2) if (x & 1) == 0 else math.sin(2.0 * math.pi * u2))


def count(word, cuts):
    n = 0
    for t in cuts:
        if word >= t:
            n += 1
    return n


def transform_pixel(t, contrast=None, noise=None, count=None):
    """One pixel: ``contrast = (alpha, mean)``, ``noise = (std, z)``, ``count`` an integer."""
    t = float(t)
    if contrast is not None:
        alpha, mean = contrast
        t = mean + alpha * (t - mean)
        t = -1.0 if t < -1.0 else (1.0 if t > 1.0 else t)
    if noise is not None:
        t = t + noise[0] * noise[1]
    if count is not None:
        t = t + float(count)
    return t
