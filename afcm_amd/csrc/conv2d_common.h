// Definitions shared by the conv2d units: conv2d.hip (forward, stride 2, data gradient, weight packing), conv2d_wgrad.hip (weight
// gradient) and conv2d_planes.hip (per-plane passes, the fp32 split).
#pragma once
#include <type_traits>

#include "common.h"

namespace afcm {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

// the power of two g with g * bound in [2^14, 2^15) for a magnitude-bound word (amax_bits_kernel); *inverse = 1 / g
__device__ __forceinline__ float pow2_factor(unsigned bound_bits, float* inverse = nullptr) {
    const float b = __uint_as_float(bound_bits);
    int e = 15;                                              // non-finite bound (a NaN fails the comparison): g = 1
    if (b <= 3.4028234664e38f) frexpf(fmaxf(b, 1e-30f), &e); // b = f * 2^e, f in [0.5, 1)
    if (inverse) *inverse = ldexpf(1.f, e - 15);
    return ldexpf(1.f, 15 - e);
}

}  // namespace afcm
