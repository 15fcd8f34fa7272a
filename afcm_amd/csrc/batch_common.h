// What the training-batch kernels share (batch.hip: the one-launch batch; elastic.hip and augment_blur.hip: the batch with an elastic deformation / a Gaussian blur, several launches): the
// item row and its checks, the geometric and the intensity parameter rows, scipy's integer 'reflect', Philox4x32-10 with the normals made from it,
// and the intensity transforms on one run of pixels.  See include/afcm_hip.h for the semantics kept.
#pragma once
#include "common.h"
#include "volume_common.h"

namespace afcm {

// [offset, offset + depth hs ws) inside [0, pool_elems) with positive extents, without forming a product that could overflow
__device__ __forceinline__ bool descriptor_ok(long long off, long long depth, long long hs, long long ws, long long pool_elems) {
    if (depth <= 0 || hs <= 0 || ws <= 0 || ws > pool_elems || hs > pool_elems / ws) return false;
    const long long plane = hs * ws;
    if (depth > pool_elems / plane) return false;
    return off >= 0 && off <= pool_elems - depth * plane;
}

// Sample i of a launch for batch_augment_kernel: batch_assemble_kernel's own row and descriptor checks, statement for statement (that kernel keeps
// them in its body: routed through this function its instances compile to a different instruction order, and they are held to the one they have)
struct batch_item {
    bool valid;
    long long row, off_a, off_b, depth, hs, ws;
    int idx, t;
};
__device__ __forceinline__ batch_item item_of(int i, long long pool_elems, const long long* __restrict__ vols, int n_vols, const int* __restrict__ items,
                                              int n_items, const long long* __restrict__ cursor, int first, int k) {
    const long long c0 = cursor != nullptr ? cursor[0] : 0;
    bool valid = c0 >= 0 && c0 < n_items;
    const long long row = valid ? c0 + first + i : 0;
    valid = valid && row < n_items;
    int va = 0, vb = 0, idx = 0, t = 1;
    if (valid) {
        va = items[row * 4 + 0], vb = items[row * 4 + 1], idx = items[row * 4 + 2], t = items[row * 4 + 3];
        valid = va >= 0 && va < n_vols && vb >= 0 && vb < n_vols && t != 0 && (k == 1 || t >= 1);
    }
    long long off_a = 0, off_b = 0, depth = 1, hs = 1, ws = 1;
    if (valid) {
        const long long* da = vols + (long long)va * 4;
        const long long* db = vols + (long long)vb * 4;
        off_a = da[0], depth = da[1], hs = da[2], ws = da[3], off_b = db[0];
        valid = descriptor_ok(off_a, depth, hs, ws, pool_elems) && descriptor_ok(off_b, db[1], db[2], db[3], pool_elems) && db[1] == depth &&
                db[2] == hs && db[3] == ws && idx >= 0 && idx < depth;
    }
    return {valid, row, off_a, off_b, depth, hs, ws, idx, valid ? t : 1};
}

// scipy.ndimage's 'reflect' for an integer coordinate: (d c b a | a b c d | d c b a), any number of periods.  2n and |i| fit an int (the entry point
// bounds h + w, the kernel the offsets)
__device__ __forceinline__ int reflect_index(int i, int n) {
    i = i < 0 ? -i - 1 : i;                                                    // the pattern is even about -1/2
    if (i < n) return i;                                                       // inside, or one mirror below 0: nearly every pixel of a rotation
    const unsigned period = 2u * (unsigned)n;
    const unsigned m = (unsigned)i < period ? (unsigned)i : (unsigned)i % period;     // the division only past the first period
    return (int)(m < (unsigned)n ? m : period - 1u - m);
}

// One parameter row of the augment table (flip_h, flip_w, k, angle, c, s, off_y, off_x): the output pixel's source in the item plane, the chain of
// transforms.py walked backwards -- RandomRotate (nearest, reflect), RandomRotate90, RandomFlip
struct augment_row {
    bool valid, identity, flip_h, flip_w;
    int quarter;
    double c, s, off_y, off_x;
    __device__ __forceinline__ void source(double yc, double ys, int x, int h, int w, int& sy, int& sx) const {
        const double iy = (yc + (double)x * s) + off_y;                        // yc = y * c, ys = y * (-s): once per run
        const double ix = (ys + (double)x * c) + off_x;
        const int ry = reflect_index((int)floor(iy + 0.5), h), rx = reflect_index((int)floor(ix + 0.5), w);
        int py = ry, px = rx;                                                  // numpy.rot90(p1, quarter)[ry][rx] = p1[py][px]; h == w for odd turns
        if (quarter == 1) py = rx, px = w - 1 - ry;
        if (quarter == 2) py = h - 1 - ry, px = w - 1 - rx;
        if (quarter == 3) py = h - 1 - rx, px = ry;
        sy = flip_h ? h - 1 - py : py;
        sx = flip_w ? w - 1 - px : px;
    }
};
__device__ __forceinline__ augment_row augment_row_of(const double* __restrict__ p, int h, int w) {
    const double fh = p[0], fw = p[1], q = p[2], c = p[4], s = p[5], oy = p[6], ox = p[7];
    const double reach = (double)h + (double)w;
    // every comparison is false for a NaN
    const bool valid = (fh == 0.0 || fh == 1.0) && (fw == 0.0 || fw == 1.0) && (q == 0.0 || q == 2.0 || ((q == 1.0 || q == 3.0) && h == w)) &&
                       fabs(c) <= 1.0 && fabs(s) <= 1.0 && fabs(oy) <= reach && fabs(ox) <= reach;
    const bool identity = fh == 0.0 && fw == 0.0 && q == 0.0 && c == 1.0 && s == 0.0 && oy == 0.0 && ox == 0.0;
    return {valid, identity, fh == 1.0, fw == 1.0, valid ? (int)q : 0, c, s, oy, ox};
}

// ---- intensity augmentation: RandomContrast, AdditiveGaussianNoise, AdditivePoissonNoise (data/augment/transforms.py:115-133, 619-644) -----------
// Philox4x32-10 (Salmon et al. 2011): four 32-bit words from a 128-bit counter and a 64-bit key
struct philox_words {
    unsigned w[4];
};
__device__ __forceinline__ philox_words philox4x32(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return {{c0, c1, c2, c3}};
}

// ln(x) of a positive normal double from + - x / only (afcm_amd/augment_intensity.py: log_series, the statement both arms evaluate operation by
// operation): frexp by bits, m into [sqrt(1/2), sqrt(2)), s = (m - 1) / (m + 1), the odd series by Horner from 1/23 down
__device__ __forceinline__ double log_series(double x) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(x);
    double m = __longlong_as_double((long long)((bits & 0x800FFFFFFFFFFFFFull) | 0x3FE0000000000000ull));   // [1/2, 1)
    int e = (int)((bits >> 52) & 0x7FF) - 1022;
    if (m < 0.7071067811865476) m *= 2.0, e -= 1;
    const double s = (m - 1.0) / (m + 1.0), s2 = s * s;
    double acc = 1.0 / 23.0;
#pragma unroll
    for (int k = 21; k >= 1; k -= 2) acc = acc * s2 + 1.0 / (double)k;
    return (double)e * 0.6931471805599453 + 2.0 * (s * acc);
}

constexpr double inv_factorial(int n) {
    double f = 1.0;
    for (int i = 2; i <= n; ++i) f *= (double)i;                               // exact up to 21! < 2^66 with 2^18 | 21!: 48 significant bits
    return 1.0 / f;
}

// sin and cos of 2 pi u, u in [0, 1): the quadrant of 4u, Taylor series of the remainder in [0, pi / 2) by Horner (sincos_turns)
__device__ __forceinline__ void sincos_turns(double u, double& sn, double& cs) {
    const double t = u * 4.0, q = floor(t);
    const double r = (t - q) * 1.5707963267948966, r2 = r * r;
    double a = inv_factorial(21);
#pragma unroll
    for (int n = 19; n >= 1; n -= 2) a = inv_factorial(n) - r2 * a;
    const double s = r * a;
    double c = inv_factorial(20);
#pragma unroll
    for (int n = 18; n >= 0; n -= 2) c = inv_factorial(n) - r2 * c;
    const int quadrant = (int)q & 3;
    sn = quadrant == 0 ? s : (quadrant == 1 ? c : (quadrant == 2 ? -s : -c));
    cs = quadrant == 0 ? c : (quadrant == 1 ? -s : (quadrant == 2 ? -c : s));
}

// Box-Muller on one word pair: two standard normals; the square root and the division are the correctly rounded ones
__device__ __forceinline__ void normal_pair(unsigned wa, unsigned wb, double& z0, double& z1) {
    const double u1 = ((double)wa + 0.5) * (1.0 / 4294967296.0), u2 = (double)wb * (1.0 / 4294967296.0);
    const double r = __dsqrt_rn(-2.0 * log_series(u1));
    double sn, cs;
    sincos_turns(u2, sn, cs);
    z0 = r * cs, z1 = r * sn;
}

// One row of the intensity table (include/afcm_hip.h): 0-2 contrast flag, alpha, mean; 3-4 Gaussian flag, std; 5-6 Poisson flag, lam; 7-8 the key;
// 9 J; 10-33 the cut points T_0 ... T_23
constexpr int INTENSITY_ROW = 36, INTENSITY_CUTS = 24;
struct intensity_row {
    bool valid, contrast, gaussian, poisson;
    double alpha, mean, std;
    unsigned key_lo, key_hi;
    int cuts;
};
__device__ __forceinline__ bool whole_in(double v, double hi) { return v >= 0.0 && v <= hi && floor(v) == v; }
__device__ __forceinline__ intensity_row intensity_row_of(const double* __restrict__ p) {
    const double fc = p[0], alpha = p[1], mean = p[2], fg = p[3], std = p[4], fp = p[5], k0 = p[7], k1 = p[8], cuts = p[9];
    const double big = 1.7976931348623157e308;
    // every comparison is false for a NaN
    bool valid = (fc == 0.0 || fc == 1.0) && (fg == 0.0 || fg == 1.0) && (fp == 0.0 || fp == 1.0) && fabs(alpha) <= big && fabs(mean) <= big &&
                 std >= 0.0 && std <= big && whole_in(k0, 4294967295.0) && whole_in(k1, 4294967295.0) && whole_in(cuts, (double)INTENSITY_CUTS);
    const int n = valid ? (int)cuts : 0;
    for (int j = 0; j < n; j += 4) {                                           // four loads in flight; j + u <= 23 stays inside the row
#pragma unroll
        for (int u = 0; u < 4; ++u) valid = valid && (j + u >= n || whole_in(p[10 + j + u], 4294967296.0));
    }
    return {valid, fc == 1.0, fg == 1.0, fp == 1.0, alpha, mean, std, valid ? (unsigned)k0 : 0u, valid ? (unsigned)k1 : 0u, n};
}

// Contrast, Gaussian and Poisson noise of the valid row n (its table row at `row`) on the run v of RUN pixels from (y, x0) of the field `field`
// (0, or plane << 1 with independent planes): float64 on the float32 values, one rounding back.  Pixel x takes lane x & 3 of
// Philox(counter (x >> 2, y, stream | field, 0), key of the row): a run starts at a multiple of 4, so a thread makes RUN / 4 calls per stream.
// The caller asks only for a row that sets a flag: a row without one leaves the bits as they are and pays for no Philox call.
template <int RUN>
__device__ __forceinline__ void intensity_apply(float (&v)[RUN], const intensity_row& n, const double* __restrict__ row, int x0, int y, unsigned field) {
    static_assert(RUN % 4 == 0, "a run is whole Philox calls");
    double t[RUN];
#pragma unroll
    for (int j = 0; j < RUN; ++j) t[j] = (double)v[j];
    if (n.contrast) {
#pragma unroll
        for (int j = 0; j < RUN; ++j) {
            const double c = n.mean + n.alpha * (t[j] - n.mean);
            t[j] = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);                      // a NaN stays
        }
    }
    if (n.gaussian) {
#pragma unroll
        for (int q = 0; q < RUN / 4; ++q) {
            const philox_words p = philox4x32((unsigned)(x0 >> 2) + q, (unsigned)y, field, 0u, n.key_lo, n.key_hi);
            double z[4];
            normal_pair(p.w[0], p.w[1], z[0], z[1]);
            normal_pair(p.w[2], p.w[3], z[2], z[3]);
#pragma unroll
            for (int j = 0; j < 4; ++j) t[4 * q + j] = t[4 * q + j] + n.std * z[j];
        }
    }
    if (n.poisson) {
        unsigned word[RUN];
        int hits[RUN];
#pragma unroll
        for (int q = 0; q < RUN / 4; ++q) {
            const philox_words p = philox4x32((unsigned)(x0 >> 2) + q, (unsigned)y, field | 1u, 0u, n.key_lo, n.key_hi);
#pragma unroll
            for (int j = 0; j < 4; ++j) word[4 * q + j] = p.w[j], hits[4 * q + j] = 0;
        }
        for (int c = 0; c < n.cuts; c += 4) {                                  // inversion by sequential search: the cut points at or below the word
            double cut[4];                                                     // four loads in flight; c + u <= 23 stays inside the row
#pragma unroll
            for (int u = 0; u < 4; ++u) cut[u] = row[10 + c + u];
#pragma unroll
            for (int u = 0; u < 4; ++u) {                                      // a whole cut point: the comparison in integers; 2^32, or past J: never
                const bool live = c + u < n.cuts && cut[u] <= 4294967295.0;
                const unsigned t_u = live ? (unsigned)cut[u] : 0xFFFFFFFFu;
#pragma unroll
                for (int j = 0; j < RUN; ++j) hits[j] += live && word[j] >= t_u ? 1 : 0;
            }
        }
#pragma unroll
        for (int j = 0; j < RUN; ++j) t[j] = t[j] + (double)hits[j];
    }
#pragma unroll
    for (int j = 0; j < RUN; ++j) v[j] = (float)t[j];
}

// batch.hip: the checks, the (source, output) dispatch and the launch of the one-launch batch; elastic.hip assembles its float32 scratch through it
int launch_batch(void* a, void* b, float* slice_idx, const void* pool, int64_t pool_elems, int32_t src_dtype, const int64_t* vols, int32_t n_vols,
                 const int32_t* items, int32_t n_items, const double* augment, const double* intensity, int32_t independent_planes,
                 const int64_t* cursor, int32_t first, int32_t count, int32_t k, int32_t h, int32_t w, int32_t out_dtype, double min_value,
                 double max_value, void* stream);

// elastic.hip: the launches of afcm_batch_assemble_elastic; augment_blur.hip has them write the deformed float32 item into its scratch
// (apply_intensity false: the gather leaves the intensity transforms to the stage after it)
int launch_elastic(void* a, void* b, float* slice_idx, const void* pool, int64_t pool_elems, int32_t src_dtype, const int64_t* vols, int32_t n_vols,
                   const int32_t* items, int32_t n_items, const double* augment, const double* intensity, int32_t independent_planes,
                   const double* elastic, const double* smooth_h, const double* smooth_w, int32_t spline_order, void* workspace,
                   int64_t workspace_bytes, const int64_t* cursor, int32_t first, int32_t count, int32_t k, int32_t h, int32_t w, int32_t out_dtype,
                   double min_value, double max_value, void* stream, bool apply_intensity);

}  // namespace afcm
