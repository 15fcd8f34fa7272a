// What the loader kernels share (volume.hip: one volume, consecutive slices; batch.hip: a table of training items over a pool of volumes).
#pragma once
#include "common.h"

namespace afcm {

constexpr int VOL_THREADS = 256;

// One source element normalised as numpy evaluates data.normalize on an array of the source's type: float64 arithmetic for u8 / i16 / f64, float32
// for f32 (numpy keeps a float32 array's type against Python scalars).  `inside` false: a padded pixel, a zero of the source type.
// Every operation is rounded on its own (-ffp-contract=off); the clip keeps a NaN, as numpy.clip does.
template <typename S>
__device__ __forceinline__ float normalised(const S* __restrict__ src, long long i, bool inside, double lo, double range) {
    const double m = inside ? (double)src[i] : 0.0;
    double v = 2.0 * ((m - lo) / range) - 1.0;
    v = v < -1.0 ? -1.0 : (v > 1.0 ? 1.0 : v);
    return (float)v;
}
template <>
__device__ __forceinline__ float normalised<float>(const float* __restrict__ src, long long i, bool inside, double lo, double range) {
    const float m = inside ? src[i] : 0.0f;
    float v = 2.0f * ((m - (float)lo) / (float)range) - 1.0f;
    v = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
    return v;
}

// transforms.py:250-275 for one axis: the source coordinate of output coordinate 0
__host__ __device__ __forceinline__ long long crop_offset(long long have, long long want) {
    return want < have ? (have - want) / 2 : -((want - have) / 2);
}

}  // namespace afcm
