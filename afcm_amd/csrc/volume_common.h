// The loader item, stated once for both loader kernels (volume.hip: one volume, consecutive slices; batch.hip: a table of training items over a
// pool of volumes): data/cmsr_dataset.py:98-155 for one output plane -- the thick-slice position and the label, centre crop / constant pad,
// Normalize to [-1, 1], one rounding to the output dtype.  A thread produces a run of consecutive x of one output row and stores it at once.
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

// Where input plane `plane` of target slice idx lies: the thick slices at -1, 0, +1, +2 thickness around the target's own, idx_a (k = 4), or the
// slice itself (k = 1), and the label, the target's place inside its thick slice (k = 1 with t = -1: -0.0f, as the host's division gives it).
struct thick_slice {
    int idx, idx_a, t;
    long long pos;
    __device__ __forceinline__ float label() const { return (float)(idx - idx_a) / (float)t; }
};
__device__ __forceinline__ thick_slice thick_slice_of(int idx, int t, int k, int plane) {
    const int idx_a = k == 4 ? (idx / t) * t : idx;
    return {idx, idx_a, t, k == 4 ? (long long)idx_a + (long long)(plane - 1) * t : idx};
}

// RUN consecutive x, from x0, of row y of the [h, w] item plane cut from slice `pos` of volume [depth, hs, ws] (rows contiguous, stride_z between
// slices), normalised.  Elements at x >= w are never stored and read nothing.  Every offset is 64-bit.
template <typename S, int RUN>
__device__ __forceinline__ void assembled_run(float (&v)[RUN], const S* __restrict__ volume, long long depth, long long hs, long long ws,
                                              long long stride_z, long long pos, int y, int x0, int h, int w, double lo, double range) {
    if (pos < 0 || pos > depth - 1) {
        const float z = normalised<double>(nullptr, 0, false, lo, range);      // a plane of float64 zeros before normalisation
#pragma unroll
        for (int j = 0; j < RUN; ++j) v[j] = z;
    } else {
        const long long ys = y + crop_offset(hs, h), xs0 = x0 + crop_offset(ws, w);   // crop offset (> 0) or minus the leading pad
        const bool row_inside = ys >= 0 && ys < hs;
        const long long at = pos * stride_z + ys * ws + xs0;
#pragma unroll
        for (int j = 0; j < RUN; ++j) {
            const bool inside = row_inside && xs0 + j >= 0 && xs0 + j < ws && x0 + j < w;
            v[j] = normalised<S>(volume, at + j, inside, lo, range);
        }
    }
}

// 16 bytes of output per thread
template <typename T>
constexpr int run_length = 16 / (int)sizeof(T);

// one value, so that the store below stays one store whatever the optimiser does around it
template <typename T, int RUN>
using run_of = T __attribute__((ext_vector_type(RUN)));

// v rounded to T at out = row + x0 of a row of w elements: one store of the whole run where it fits the row and the address allows it
template <typename T, int RUN>
__device__ __forceinline__ void store_run(T* __restrict__ out, const float (&v)[RUN], int x0, int w) {
    if (x0 + RUN <= w && (uintptr_t)out % (sizeof(T) * RUN) == 0) {
        run_of<T, RUN> pack;
#pragma unroll
        for (int j = 0; j < RUN; ++j) pack[j] = (T)v[j];
        *reinterpret_cast<run_of<T, RUN>*>(out) = pack;
    } else {                                                                   // the tail of a row, or a row that does not start on a run boundary
#pragma unroll
        for (int j = 0; j < RUN; ++j)
            if (x0 + j < w) out[j] = (T)v[j];
    }
}

// f(type_tag<S>, type_tag<T>) for the source and output element types of the two codes (both checked by the caller)
template <typename X>
struct type_tag {
    using type = X;
};
template <typename F>
static int dispatch_src_out(int src_dtype, int out_dtype, F&& f) {
    auto with_src = [&](auto s) -> int {
        if (out_dtype == AFCM_F32) return f(s, type_tag<float>{});
        if (out_dtype == AFCM_F16) return f(s, type_tag<f16_t>{});
        return f(s, type_tag<bf16_t>{});
    };
    switch (src_dtype) {
        case AFCM_SRC_U8: return with_src(type_tag<uint8_t>{});
        case AFCM_SRC_I16: return with_src(type_tag<int16_t>{});
        case AFCM_SRC_F32: return with_src(type_tag<float>{});
        default: return with_src(type_tag<double>{});
    }
}

}  // namespace afcm
