// Per-plane normalisers on the device: the reference's PercentileNormalizer and Standardize (data/augment/transforms.py:552-601, channelwise
// False), whose coefficients are a statistic of each [1, h, w] item plane.  See include/afcm_hip.h for the statement kept.
//   norm_stats_kernel        one 256-thread workgroup per (item, plane): reads the plane through the loaders' crop / pad / row validation and
//                            writes coef[item][plane] = (sub, div, stat0, stat1) in float64.  Two instances of one body: the items of a pool
//                            (afcm_plane_norm_stats) and a run of slices of one volume (afcm_slice_norm_stats).
//   batch_norm_kernel        batch_augment_kernel's thread shape, gather and stores with the value (m - sub) / div, then the optional Normalize
//   slice_norm_kernel        slice_assemble_kernel's likewise
// Percentile mode: an exact radix select, most significant digit first, 8 bits per pass (u8 one pass, i16 two, f32 four, f64 eight) under the
// order-preserving keys of intensity.hip's percentile clip (floats: -0.0 -> +0.0, the sign bit flipped for non-negatives, all bits inverted
// for negatives; int16 biased by 32768).  The four ranks -- floor and floor + 1 of each percentile's virtual index -- are known from h w alone.
// A pass counts, per distinct prefix the ranks have reached, the pixels that carry it into one of four 256-bin LDS histograms (integer LDS adds:
// any order gives the same counts); then wave r scans the histogram of rank r, four bins per lane, and carries prefix and residual rank on.
// NaNs are counted apart: one makes every coefficient NaN, as numpy's percentile does.  The lerp is numpy's, every operation rounded on its own.
// Standardize mode, THE summation order (afcm_amd/normalise.py mirrors it operation by operation): thread t adds the values of pixels
// t, t + 256, t + 512, ... of the row-major [h, w] plane in that order onto +0.0; the 256 partials are added by the tree
// part[t] += part[t + off] for off = 128, 64, ..., 1 (t < off).  mean = sum / n.  The sum of squared deviations takes d = m - mean, d * d and the
// same order again; std = sqrt(ss / n), the division and the root correctly rounded.  Everything is float64 whatever the source type.
// No global atomics, no allocation, no host read: every launch runs on `stream` and can be captured.
#include "batch_common.h"

namespace afcm {

constexpr int PN_THREADS = 256;
constexpr int PN_WAVES = PN_THREADS / 64;
constexpr int PN_RANKS = 4;                           // i and i + 1 of the low percentile, i and i + 1 of the high one: one wave each
constexpr int PN_DIGIT = 8;
constexpr int PN_BINS = 1 << PN_DIGIT;
static_assert(PN_WAVES == PN_RANKS && PN_BINS == 4 * 64, "wave r scans rank r's histogram, four bins per lane");

// the order-preserving key of a source element, the test for a NaN, and the key's value widened exactly to double
template <typename S>
struct norm_key;
template <>
struct norm_key<uint8_t> {
    typedef uint32_t key_t;
    static constexpr int bits = 8;
    __device__ static __forceinline__ bool nan(uint8_t) { return false; }
    __device__ static __forceinline__ key_t key(uint8_t v) { return v; }
    __device__ static __forceinline__ double value(key_t k) { return (double)k; }
};
template <>
struct norm_key<int16_t> {
    typedef uint32_t key_t;
    static constexpr int bits = 16;
    __device__ static __forceinline__ bool nan(int16_t) { return false; }
    __device__ static __forceinline__ key_t key(int16_t v) { return (uint32_t)((int)v + 32768); }
    __device__ static __forceinline__ double value(key_t k) { return (double)((int)k - 32768); }
};
template <>
struct norm_key<float> {
    typedef uint32_t key_t;
    static constexpr int bits = 32;
    __device__ static __forceinline__ bool nan(float v) { return (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u; }
    __device__ static __forceinline__ key_t key(float f) {
        uint32_t v = __float_as_uint(f);
        if (v == 0x80000000u) v = 0u;                                          // -0.0 and +0.0 are one key
        return (v & 0x80000000u) ? ~v : v | 0x80000000u;
    }
    __device__ static __forceinline__ double value(key_t k) { return (double)__uint_as_float((k & 0x80000000u) ? k ^ 0x80000000u : ~k); }
};
template <>
struct norm_key<double> {
    typedef unsigned long long key_t;
    static constexpr int bits = 64;
    __device__ static __forceinline__ bool nan(double v) {
        return ((unsigned long long)__double_as_longlong(v) & 0x7fffffffffffffffull) > 0x7ff0000000000000ull;
    }
    __device__ static __forceinline__ key_t key(double f) {
        unsigned long long v = (unsigned long long)__double_as_longlong(f);
        if (v == 0x8000000000000000ull) v = 0ull;
        return (v >> 63) ? ~v : v | 0x8000000000000000ull;
    }
    __device__ static __forceinline__ double value(key_t k) {
        return __longlong_as_double((long long)((k >> 63) ? k ^ 0x8000000000000000ull : ~k));
    }
};

// Pixel e of the row-major [h, w] item plane cut from one source slice [hs, ws]: the centred crop, or a padded zero of the source type
template <typename S>
struct item_plane {
    const S* slice;
    long long hs, ws, oy, ox;
    int w;
    __device__ __forceinline__ S at(int e) const {
        const int y = e / w, x = e - y * w;
        const long long ys = y + oy, xs = x + ox;
        return ys >= 0 && ys < hs && xs >= 0 && xs < ws ? slice[ys * ws + xs] : (S)0;
    }
};

// numpy's `linear` percentile with its _lerp; every product and sum rounded on its own
__device__ __forceinline__ double pn_lerp(double a, double b, double g) {
    const double d = b - a;
    return g >= 0.5 ? b - d * (1.0 - g) : a + d * g;
}

// part[0] = the tree sum of the 256 partials (the header's order); every thread returns it
__device__ __forceinline__ double pn_tree(double* part, double mine, int tid) {
    __syncthreads();                                                           // the previous tree's readers are done
    part[tid] = mine;
    __syncthreads();
    for (int off = PN_THREADS / 2; off >= 1; off >>= 1) {
        if (tid < off) part[tid] = part[tid] + part[tid + off];
        __syncthreads();
    }
    return part[0];
}

struct norm_params {
    int mode;                                         // AFCM_NORM_*
    double p0, p1, eps;                               // percentile: the two fractions; fixed: mean, std
};

// The coefficients of one plane by one workgroup.  `valid`, `outside` and the mode are the same in every thread, so every barrier is met by all.
template <typename S>
__device__ __forceinline__ void plane_coefficients(double* __restrict__ coef, bool valid, bool outside, const item_plane<S>& pl, int n,
                                                   const norm_params& np, uint32_t* hist, double* part) {
    typedef norm_key<S> K;
    typedef typename K::key_t key_t;
    const int tid = threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (!valid) {
        if (tid < 4) coef[tid] = nan;
        return;
    }
    if (np.mode == AFCM_NORM_FIXED || (np.mode == AFCM_NORM_STANDARDIZE && outside)) {      // nothing to read: given floats, or a plane of zeros
        const double mean = np.mode == AFCM_NORM_FIXED ? np.p0 : 0.0, std = np.mode == AFCM_NORM_FIXED ? np.p1 : 0.0;
        if (tid == 0) coef[0] = mean, coef[1] = std < np.eps ? np.eps : std, coef[2] = mean, coef[3] = std;      // numpy.clip keeps a NaN
        return;
    }
    if (np.mode == AFCM_NORM_STANDARDIZE) {
        double acc = 0.0;
        for (int e = tid; e < n; e += PN_THREADS) acc = acc + (double)pl.at(e);
        const double mean = pn_tree(part, acc, tid) / (double)n;
        acc = 0.0;
        for (int e = tid; e < n; e += PN_THREADS) {
            const double d = (double)pl.at(e) - mean;
            acc = acc + d * d;
        }
        const double std = __dsqrt_rn(pn_tree(part, acc, tid) / (double)n);
        if (tid == 0) coef[0] = mean, coef[1] = std < np.eps ? np.eps : std, coef[2] = mean, coef[3] = std;
        return;
    }
    if (outside) {                                                             // every order statistic of a plane of zeros is 0
        if (tid == 0) coef[0] = 0.0, coef[1] = (0.0 - 0.0) + np.eps, coef[2] = 0.0, coef[3] = 0.0;
        return;
    }
    // the four ranks and the two fractional parts: n alone decides them (a NaN is counted, and then decides the result)
    __shared__ unsigned long long s_prefix[PN_RANKS];
    __shared__ unsigned s_rank[PN_RANKS], s_nans;
    __shared__ int s_group[PN_RANKS];
    double g[2];
    {
        const double q[2] = {np.p0, np.p1};
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const double vi = q[p] * (double)(n - 1), fl = floor(vi);
            g[p] = vi - fl;
            unsigned i = (unsigned)fl;
            if (i > (unsigned)(n - 1)) i = (unsigned)(n - 1);                  // q <= 1 keeps vi <= n - 1; only a guard
            if (tid == 0) s_rank[2 * p] = i, s_rank[2 * p + 1] = i + 1 < (unsigned)(n - 1) ? i + 1 : (unsigned)(n - 1);
        }
    }
    if (tid < PN_RANKS) s_prefix[tid] = 0ull, s_group[tid] = 0;
    if (tid == 0) s_nans = 0u;
    const int wave = tid >> 6, lane = tid & 63;
    for (int pass = 0; pass < K::bits / PN_DIGIT; ++pass) {
        const int shift = K::bits - PN_DIGIT * (pass + 1);
        for (int i = tid; i < PN_RANKS * PN_BINS; i += PN_THREADS) hist[i] = 0u;
        __syncthreads();
        key_t prefix[PN_RANKS];
        bool lead[PN_RANKS];
#pragma unroll
        for (int r = 0; r < PN_RANKS; ++r) prefix[r] = (key_t)s_prefix[r], lead[r] = s_group[r] == r;
        for (int e = tid; e < n; e += PN_THREADS) {
            const S v = pl.at(e);
            if (K::nan(v)) {
                if (pass == 0) atomicAdd(&s_nans, 1u);
                continue;
            }
            const key_t key = K::key(v);
            const int digit = (int)((key >> shift) & (key_t)(PN_BINS - 1));
            const key_t top = pass == 0 ? (key_t)0 : key >> (shift + PN_DIGIT);      // the first pass has no digits above its own
#pragma unroll
            for (int r = 0; r < PN_RANKS; ++r)
                if (lead[r] && top == prefix[r]) {
                    atomicAdd(&hist[r * PN_BINS + digit], 1u);
                    break;
                }
        }
        __syncthreads();
        {                                                                      // wave r: the bin of rank r among the pixels that carry its prefix
            const uint32_t* h4 = hist + s_group[wave] * PN_BINS + 4 * lane;
            const unsigned c[4] = {h4[0], h4[1], h4[2], h4[3]};
            const unsigned own = c[0] + c[1] + c[2] + c[3], want = s_rank[wave];
            unsigned incl = own;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned up = __shfl_up(incl, off, 64);
                if (lane >= off) incl += up;
            }
            unsigned below = incl - own;
            if (below <= want && want < incl) {                                // one lane at most; none only when NaNs are missing from the counts
                int bin = 0;
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    if (bin == j && want >= below + c[j]) below += c[j], bin = j + 1;
                s_prefix[wave] = (s_prefix[wave] << PN_DIGIT) | (unsigned long long)(4 * lane + bin);      // only this wave touches entry `wave` here
                s_rank[wave] = want - below;
            }
        }
        __syncthreads();
        if (tid == 0) {                                                        // ranks that still share a prefix share the first one's histogram
            for (int r = 0; r < PN_RANKS; ++r) {
                int first = r;
                for (int o = r - 1; o >= 0; --o)
                    if (s_prefix[o] == s_prefix[r]) first = o;
                s_group[r] = first;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        double lo = nan, hi = nan;
        if (s_nans == 0u) {
            lo = pn_lerp(K::value((key_t)s_prefix[0]), K::value((key_t)s_prefix[1]), g[0]);
            hi = pn_lerp(K::value((key_t)s_prefix[2]), K::value((key_t)s_prefix[3]), g[1]);
        }
        coef[0] = lo, coef[1] = (hi - lo) + np.eps, coef[2] = lo, coef[3] = hi;
    }
}

// POOL: workgroup (i, plane) of a batch of pool items, plane k the target; otherwise plane `plane` of target slice first + i of one volume
template <typename S, bool POOL>
__global__ __launch_bounds__(PN_THREADS) void norm_stats_kernel(double* __restrict__ coef, const S* __restrict__ src, long long pool_elems,
                                                                const long long* __restrict__ vols, int n_vols, const int* __restrict__ items,
                                                                int n_items, const long long* __restrict__ cursor, int depth, int hs, int ws,
                                                                long long stride_z, int thickness, int first, int k, int h, int w,
                                                                norm_params np) {
    __shared__ uint32_t hist[PN_RANKS * PN_BINS];
    __shared__ double part[PN_THREADS];
    const int planes = POOL ? k + 1 : k;
    const int plane = (int)(blockIdx.x % planes), i = (int)(blockIdx.x / planes);
    bool valid = true;
    long long d = depth, sh = hs, sw = ws, plane_elems = stride_z, pos;
    const S* volume = src;
    if (POOL) {
        const batch_item it = item_of(i, pool_elems, vols, n_vols, items, n_items, cursor, first, k);
        valid = it.valid, d = it.depth, sh = it.hs, sw = it.ws, plane_elems = it.hs * it.ws;
        volume = src + (plane < k ? it.off_a : it.off_b);
        pos = thick_slice_of(it.idx, it.t, plane < k ? k : 1, plane).pos;
    } else {
        pos = thick_slice_of(first + i, thickness, k, plane).pos;
    }
    const bool outside = pos < 0 || pos > d - 1;
    const item_plane<S> pl = {valid && !outside ? volume + pos * plane_elems : nullptr, sh, sw, crop_offset(sh, h), crop_offset(sw, w), w};
    plane_coefficients<S>(coef + (long long)blockIdx.x * 4, valid, outside, pl, h * w, np, hist, part);
}

// One source element under its plane's coefficients, float64 for every source type: (m - sub) / div, then the optional Normalize
// clip(2 * ((v - lo) / range) - 1, -1, 1) (a NaN stays), one rounding to float32.  `inside` false: a padded pixel or a plane of zeros.
template <typename S>
__device__ __forceinline__ float normalised_by(const S* __restrict__ src, long long i, bool inside, double sub, double div, bool then, double lo,
                                               double range) {
    const double m = inside ? (double)src[i] : 0.0;
    double v = (m - sub) / div;
    if (then) {
        v = 2.0 * ((v - lo) / range) - 1.0;
        v = v < -1.0 ? -1.0 : (v > 1.0 ? 1.0 : v);
    }
    return (float)v;
}

// assembled_run with normalised_by in place of normalised
template <typename S, int RUN>
__device__ __forceinline__ void normalised_run(float (&v)[RUN], const S* __restrict__ volume, long long depth, long long hs, long long ws,
                                               long long stride_z, long long pos, int y, int x0, int h, int w, double sub, double div, bool then,
                                               double lo, double range) {
    if (pos < 0 || pos > depth - 1) {
        const float z = normalised_by<double>(nullptr, 0, false, sub, div, then, lo, range);
#pragma unroll
        for (int j = 0; j < RUN; ++j) v[j] = z;
    } else {
        const long long ys = y + crop_offset(hs, h), xs0 = x0 + crop_offset(ws, w);
        const bool row_inside = ys >= 0 && ys < hs;
        const long long at = pos * stride_z + ys * ws + xs0;
#pragma unroll
        for (int j = 0; j < RUN; ++j) {
            const bool inside = row_inside && xs0 + j >= 0 && xs0 + j < ws && x0 + j < w;
            v[j] = normalised_by<S>(volume, at + j, inside, sub, div, then, lo, range);
        }
    }
}

// batch_augment_kernel (a null augment: the identity row) with the plane's coefficients in place of the fixed Normalize
template <typename S, typename T, int RUN>
__global__ __launch_bounds__(VOL_THREADS) void batch_norm_kernel(T* __restrict__ a, T* __restrict__ b, float* __restrict__ slice_idx,
                                                                 const S* __restrict__ pool, long long pool_elems,
                                                                 const long long* __restrict__ vols, int n_vols, const int* __restrict__ items,
                                                                 int n_items, const double* __restrict__ augment, const double* __restrict__ coef,
                                                                 int then, const long long* __restrict__ cursor, int first, int k, int h, int w,
                                                                 int runs, long long total, double lo, double range) {
    const long long e = (long long)blockIdx.x * VOL_THREADS + threadIdx.x;
    if (e >= total) return;
    const int x0 = (int)(e % runs) * RUN;
    long long r = e / runs;
    const int y = (int)(r % h);
    r /= h;
    const int plane = (int)(r % (k + 1));                                      // plane k: the target B
    const int i = (int)(r / (k + 1));

    const batch_item it = item_of(i, pool_elems, vols, n_vols, items, n_items, cursor, first, k);
    augment_row g = {augment == nullptr, true, false, false, 0, 1.0, 0.0, 0.0, 0.0};   // no table: the identity
    if (it.valid && augment != nullptr) g = augment_row_of(augment + it.row * 8, h, w);
    const bool valid = it.valid && g.valid;
    const thick_slice at = thick_slice_of(it.idx, it.t, plane < k ? k : 1, plane);
    if (plane == 0 && y == 0 && x0 == 0) slice_idx[i] = valid ? at.label() : __builtin_nanf("");

    const double* __restrict__ cf = coef + ((long long)i * (k + 1) + plane) * 4;
    const double sub = cf[0], div = cf[1];
    const S* __restrict__ volume = pool + (plane < k ? it.off_a : it.off_b);
    float v[RUN];
    if (!valid) {
#pragma unroll
        for (int j = 0; j < RUN; ++j) v[j] = __builtin_nanf("");
    } else if (g.identity || at.pos < 0 || at.pos > it.depth - 1) {            // the contiguous read; a plane outside the volume is a constant
        normalised_run<S, RUN>(v, volume, it.depth, it.hs, it.ws, it.hs * it.ws, at.pos, y, x0, h, w, sub, div, then != 0, lo, range);
    } else {
        const double yc = (double)y * g.c, ys = (double)y * (-g.s);
        const long long oy = crop_offset(it.hs, h), ox = crop_offset(it.ws, w), slice = at.pos * (it.hs * it.ws);
#pragma unroll
        for (int j = 0; j < RUN; ++j) {
            v[j] = 0.0f;
            if (x0 + j < w) {                                                  // elements past the row are never stored and read nothing
                int sy, sx;
                g.source(yc, ys, x0 + j, h, w, sy, sx);
                const long long yv = sy + oy, xv = sx + ox;                    // the item plane's pixel in the volume's slice, or in the padding
                v[j] = normalised_by<S>(volume, slice + yv * it.ws + xv, yv >= 0 && yv < it.hs && xv >= 0 && xv < it.ws, sub, div, then != 0, lo,
                                        range);
            }
        }
    }
    store_run<T, RUN>((plane < k ? a + (((long long)i * k + plane) * h + y) * w : b + ((long long)i * h + y) * w) + x0, v, x0, w);
}

// slice_assemble_kernel with the plane's coefficients in place of the fixed Normalize
template <typename S, typename T, int RUN>
__global__ __launch_bounds__(VOL_THREADS) void slice_norm_kernel(T* __restrict__ a, float* __restrict__ slice_idx, const S* __restrict__ src,
                                                                 const double* __restrict__ coef, int then, int depth, int hs, int ws,
                                                                 long long stride_z, int first, int k, int thickness, int h, int w, int runs,
                                                                 long long total, double lo, double range) {
    const long long e = (long long)blockIdx.x * VOL_THREADS + threadIdx.x;
    if (e >= total) return;
    const int x0 = (int)(e % runs) * RUN;
    long long r = e / runs;
    const int y = (int)(r % h);
    r /= h;                                                                    // r = i * k + plane: the plane's row of the coefficient table
    const int plane = (int)(r % k);
    const int i = (int)(r / k);
    const thick_slice at = thick_slice_of(first + i, thickness, k, plane);
    if (plane == 0 && y == 0 && x0 == 0) slice_idx[i] = at.label();
    float v[RUN];
    normalised_run<S, RUN>(v, src, depth, hs, ws, stride_z, at.pos, y, x0, h, w, coef[r * 4 + 0], coef[r * 4 + 1], then != 0, lo, range);
    store_run<T, RUN>(a + (r * h + y) * w + x0, v, x0, w);
}

// what both statistics entry points ask of the mode and its parameters; `what` names the caller
static int check_norm_mode(const char* what, int32_t mode, double p0, double p1, double eps) {
    AFCM_REQUIRE(mode >= AFCM_NORM_PERCENTILE && mode <= AFCM_NORM_FIXED, "%s: mode %d is not AFCM_NORM_PERCENTILE / STANDARDIZE / FIXED", what, mode);
    AFCM_REQUIRE(mode != AFCM_NORM_PERCENTILE || (p0 >= 0.0 && p0 <= p1 && p1 <= 1.0), "%s: percentile fractions %g, %g: 0 <= q_lo <= q_hi <= 1", what,
                 p0, p1);
    AFCM_REQUIRE(eps == eps, "%s: eps is a NaN", what);
    return AFCM_OK;
}

template <bool POOL, typename... Args>
static int launch_norm_stats(int32_t src_dtype, long long groups, hipStream_t s, double* coef, const void* src, Args... args) {
    const dim3 grid((unsigned)groups), block(PN_THREADS);
    switch (src_dtype) {
        case AFCM_SRC_U8: hipLaunchKernelGGL((norm_stats_kernel<uint8_t, POOL>), grid, block, 0, s, coef, (const uint8_t*)src, args...); break;
        case AFCM_SRC_I16: hipLaunchKernelGGL((norm_stats_kernel<int16_t, POOL>), grid, block, 0, s, coef, (const int16_t*)src, args...); break;
        case AFCM_SRC_F32: hipLaunchKernelGGL((norm_stats_kernel<float, POOL>), grid, block, 0, s, coef, (const float*)src, args...); break;
        default: hipLaunchKernelGGL((norm_stats_kernel<double, POOL>), grid, block, 0, s, coef, (const double*)src, args...); break;
    }
    return hip_status(hipGetLastError());
}

}  // namespace afcm

extern "C" int afcm_norm_plan(int32_t src_dtype, int32_t mode, int32_t* plan) {
    using namespace afcm;
    AFCM_REQUIRE(plan != nullptr, "norm_plan: null plan");
    AFCM_REQUIRE(src_dtype >= AFCM_SRC_U8 && src_dtype <= AFCM_SRC_F64, "norm_plan: source dtype %d is not AFCM_SRC_U8 / I16 / F32 / F64", src_dtype);
    AFCM_REQUIRE(mode >= AFCM_NORM_PERCENTILE && mode <= AFCM_NORM_FIXED, "norm_plan: mode %d is not AFCM_NORM_PERCENTILE / STANDARDIZE / FIXED", mode);
    const int key_bits = src_dtype == AFCM_SRC_U8 ? 8 : (src_dtype == AFCM_SRC_I16 ? 16 : (src_dtype == AFCM_SRC_F32 ? 32 : 64));
    plan[0] = PN_THREADS;
    plan[1] = mode == AFCM_NORM_PERCENTILE ? key_bits / PN_DIGIT : (mode == AFCM_NORM_STANDARDIZE ? 2 : 0);     // times the plane is read
    plan[2] = PN_DIGIT;
    plan[3] = PN_RANKS;
    return AFCM_OK;
}

extern "C" int afcm_plane_norm_stats(double* coef, const void* pool, int64_t pool_elems, int32_t src_dtype, const int64_t* vols, int32_t n_vols,
                                     const int32_t* items, int32_t n_items, const int64_t* cursor, int32_t first, int32_t count, int32_t k, int32_t h,
                                     int32_t w, int32_t mode, double p0, double p1, double eps, void* stream) {
    using namespace afcm;
    AFCM_REQUIRE(coef != nullptr && pool != nullptr && vols != nullptr && items != nullptr, "plane_norm_stats: null coefficients, pool or table");
    AFCM_REQUIRE(src_dtype >= AFCM_SRC_U8 && src_dtype <= AFCM_SRC_F64, "plane_norm_stats: source dtype %d is not AFCM_SRC_U8 / I16 / F32 / F64", src_dtype);
    AFCM_REQUIRE(count > 0 && h > 0 && w > 0 && n_vols > 0 && n_items > 0 && pool_elems > 0,
                 "plane_norm_stats: %d items of [%d, %d] from %d volumes, a table of %d rows, a pool of %lld elements: every extent must be positive", count,
                 h, w, n_vols, n_items, (long long)pool_elems);
    AFCM_REQUIRE((long long)h * w <= (1LL << 30), "plane_norm_stats: a plane of [%d, %d] has more than 2^30 pixels", h, w);
    AFCM_REQUIRE(first >= 0, "plane_norm_stats: first row %d is negative", first);
    AFCM_REQUIRE(k == 1 || k == 4, "plane_norm_stats: slice number %d is not 1 or 4", k);
    AFCM_REQUIRE(((uintptr_t)coef & 7) == 0, "plane_norm_stats: the coefficients must be 8-byte aligned");
    const int rc = check_norm_mode("plane_norm_stats", mode, p0, p1, eps);
    if (rc != AFCM_OK) return rc;
    const long long groups = (long long)count * (k + 1);
    AFCM_REQUIRE(groups < (1LL << 31), "plane_norm_stats: %lld workgroups exceed the grid", groups);
    const norm_params np = {mode, p0, p1, eps};
    return launch_norm_stats<true>(src_dtype, groups, (hipStream_t)stream, coef, pool, (long long)pool_elems, (const long long*)vols, n_vols,
                                   (const int*)items, n_items, (const long long*)cursor, 0, 0, 0, 0LL, 1, first, k, h, w, np);
}

extern "C" int afcm_slice_norm_stats(double* coef, const void* src, int32_t src_dtype, int32_t depth, int32_t hs, int32_t ws, int64_t src_stride_z,
                                     int32_t first, int32_t count, int32_t k, int32_t thickness, int32_t h, int32_t w, int32_t mode, double p0,
                                     double p1, double eps, void* stream) {
    using namespace afcm;
    AFCM_REQUIRE(coef != nullptr && src != nullptr, "slice_norm_stats: null coefficients or source");
    AFCM_REQUIRE(src_dtype >= AFCM_SRC_U8 && src_dtype <= AFCM_SRC_F64, "slice_norm_stats: source dtype %d is not AFCM_SRC_U8 / I16 / F32 / F64", src_dtype);
    AFCM_REQUIRE(depth > 0 && hs > 0 && ws > 0 && h > 0 && w > 0, "slice_norm_stats: source [%d, %d, %d] -> [%d, %d]: every extent must be positive", depth,
                 hs, ws, h, w);
    AFCM_REQUIRE((long long)h * w <= (1LL << 30), "slice_norm_stats: a plane of [%d, %d] has more than 2^30 pixels", h, w);
    AFCM_REQUIRE(src_stride_z >= 0, "slice_norm_stats: source z stride %lld is negative", (long long)src_stride_z);
    AFCM_REQUIRE(count > 0 && first >= 0 && (long long)first + count <= depth, "slice_norm_stats: slices [%d, %lld) are not inside a volume of %d", first,
                 (long long)first + count, depth);
    AFCM_REQUIRE(k == 1 || k == 4, "slice_norm_stats: slice number %d is not 1 or 4", k);
    AFCM_REQUIRE(thickness != 0 && (k == 1 || thickness >= 1), "slice_norm_stats: thickness %d with slice number %d", thickness, k);
    AFCM_REQUIRE(((uintptr_t)coef & 7) == 0, "slice_norm_stats: the coefficients must be 8-byte aligned");
    const int rc = check_norm_mode("slice_norm_stats", mode, p0, p1, eps);
    if (rc != AFCM_OK) return rc;
    const norm_params np = {mode, p0, p1, eps};
    return launch_norm_stats<false>(src_dtype, (long long)count * k, (hipStream_t)stream, coef, src, 0LL, (const long long*)nullptr, 0,
                                    (const int*)nullptr, 0, (const long long*)nullptr, depth, hs, ws, (long long)src_stride_z, thickness, first, k, h, w,
                                    np);
}

extern "C" int afcm_batch_assemble_norm(void* a, void* b, float* slice_idx, const void* pool, int64_t pool_elems, int32_t src_dtype, const int64_t* vols,
                                        int32_t n_vols, const int32_t* items, int32_t n_items, const double* augment, const double* coef,
                                        int32_t then_normalize, const int64_t* cursor, int32_t first, int32_t count, int32_t k, int32_t h, int32_t w,
                                        int32_t out_dtype, double min_value, double max_value, void* stream) {
    using namespace afcm;
    AFCM_REQUIRE(a != nullptr && b != nullptr && slice_idx != nullptr && pool != nullptr && vols != nullptr && items != nullptr && coef != nullptr,
                 "batch_assemble_norm: null output, label, pool, table or coefficients");
    AFCM_REQUIRE(src_dtype >= AFCM_SRC_U8 && src_dtype <= AFCM_SRC_F64, "batch_assemble_norm: source dtype %d is not AFCM_SRC_U8 / I16 / F32 / F64",
                 src_dtype);
    AFCM_REQUIRE(out_dtype >= AFCM_F32 && out_dtype <= AFCM_BF16, "batch_assemble_norm: output dtype %d is not AFCM_F32 / AFCM_F16 / AFCM_BF16", out_dtype);
    AFCM_REQUIRE(count > 0 && h > 0 && w > 0 && n_vols > 0 && n_items > 0 && pool_elems > 0,
                 "batch_assemble_norm: %d items of [%d, %d] from %d volumes, a table of %d rows, a pool of %lld elements: every extent must be positive",
                 count, h, w, n_vols, n_items, (long long)pool_elems);
    AFCM_REQUIRE(first >= 0, "batch_assemble_norm: first row %d is negative", first);
    AFCM_REQUIRE(k == 1 || k == 4, "batch_assemble_norm: slice number %d is not 1 or 4", k);
    AFCM_REQUIRE(then_normalize == 0 || then_normalize == 1, "batch_assemble_norm: then_normalize %d is not 0 or 1", then_normalize);
    AFCM_REQUIRE(max_value > min_value, "batch_assemble_norm: max_value %g is not above min_value %g", max_value, min_value);
    AFCM_REQUIRE(augment == nullptr || (long long)h + w <= (1LL << 28),
                 "batch_assemble_norm: a patch of [%d, %d]: h + w above 2^28 takes the rotated coordinates out of the int32 range", h, w);
    AFCM_REQUIRE(((uintptr_t)coef & 7) == 0, "batch_assemble_norm: the coefficients must be 8-byte aligned");
    const double range = max_value - min_value;
    return dispatch_src_out(src_dtype, out_dtype, [&](auto s_tag, auto t_tag) -> int {
        using S = typename decltype(s_tag)::type;
        using T = typename decltype(t_tag)::type;
        constexpr int RUN = run_length<T>;
        const int runs = cdiv(w, RUN);
        const double threads = (double)count * (k + 1) * h * runs;             // checked before the product is formed in 64 bits
        AFCM_REQUIRE(threads / VOL_THREADS < 2147483647.0, "batch_assemble_norm: %.0f workgroups exceed the grid", threads / VOL_THREADS);
        const long long total = (long long)count * (k + 1) * h * runs;
        const long long groups = (total + VOL_THREADS - 1) / VOL_THREADS;
        hipLaunchKernelGGL((batch_norm_kernel<S, T, RUN>), dim3((unsigned)groups), dim3(VOL_THREADS), 0, (hipStream_t)stream, (T*)a, (T*)b, slice_idx,
                           (const S*)pool, (long long)pool_elems, (const long long*)vols, n_vols, (const int*)items, n_items, augment, coef,
                           (int)then_normalize, (const long long*)cursor, first, k, h, w, runs, total, min_value, range);
        return hip_status(hipGetLastError());
    });
}

extern "C" int afcm_slice_assemble_norm(void* a, float* slice_idx, const void* src, int32_t src_dtype, int32_t out_dtype, int32_t depth, int32_t hs,
                                        int32_t ws, int64_t src_stride_z, const double* coef, int32_t then_normalize, int32_t first, int32_t count,
                                        int32_t k, int32_t thickness, int32_t h, int32_t w, double min_value, double max_value, void* stream) {
    using namespace afcm;
    AFCM_REQUIRE(a != nullptr && slice_idx != nullptr && src != nullptr && coef != nullptr, "slice_assemble_norm: null output, label, source or coefficients");
    AFCM_REQUIRE(src_dtype >= AFCM_SRC_U8 && src_dtype <= AFCM_SRC_F64, "slice_assemble_norm: source dtype %d is not AFCM_SRC_U8 / I16 / F32 / F64",
                 src_dtype);
    AFCM_REQUIRE(out_dtype >= AFCM_F32 && out_dtype <= AFCM_BF16, "slice_assemble_norm: output dtype %d is not AFCM_F32 / AFCM_F16 / AFCM_BF16", out_dtype);
    AFCM_REQUIRE(depth > 0 && hs > 0 && ws > 0 && h > 0 && w > 0, "slice_assemble_norm: source [%d, %d, %d] -> [%d, %d]: every extent must be positive",
                 depth, hs, ws, h, w);
    AFCM_REQUIRE(src_stride_z >= 0, "slice_assemble_norm: source z stride %lld is negative", (long long)src_stride_z);
    AFCM_REQUIRE(count > 0 && first >= 0 && (long long)first + count <= depth, "slice_assemble_norm: slices [%d, %lld) are not inside a volume of %d", first,
                 (long long)first + count, depth);
    AFCM_REQUIRE(k == 1 || k == 4, "slice_assemble_norm: slice number %d is not 1 or 4", k);
    AFCM_REQUIRE(thickness != 0 && (k == 1 || thickness >= 1), "slice_assemble_norm: thickness %d with slice number %d", thickness, k);
    AFCM_REQUIRE(then_normalize == 0 || then_normalize == 1, "slice_assemble_norm: then_normalize %d is not 0 or 1", then_normalize);
    AFCM_REQUIRE(max_value > min_value, "slice_assemble_norm: max_value %g is not above min_value %g", max_value, min_value);
    AFCM_REQUIRE(((uintptr_t)coef & 7) == 0, "slice_assemble_norm: the coefficients must be 8-byte aligned");
    const double range = max_value - min_value;
    return dispatch_src_out(src_dtype, out_dtype, [&](auto s_tag, auto t_tag) -> int {
        using S = typename decltype(s_tag)::type;
        using T = typename decltype(t_tag)::type;
        constexpr int RUN = run_length<T>;
        const int runs = cdiv(w, RUN);
        const double threads = (double)count * k * h * runs;                   // checked before the product is formed in 64 bits
        AFCM_REQUIRE(threads / VOL_THREADS < 2147483647.0, "slice_assemble_norm: %.0f output elements exceed the grid", (double)count * k * h * w);
        const long long total = (long long)count * k * h * runs;
        const long long groups = (total + VOL_THREADS - 1) / VOL_THREADS;
        hipLaunchKernelGGL((slice_norm_kernel<S, T, RUN>), dim3((unsigned)groups), dim3(VOL_THREADS), 0, (hipStream_t)stream, (T*)a, slice_idx,
                           (const S*)src, coef, (int)then_normalize, depth, hs, ws, (long long)src_stride_z, first, k, thickness, h, w, runs, total,
                           min_value, range);
        return hip_status(hipGetLastError());
    });
}
