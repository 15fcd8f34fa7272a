// Per-plane passes around the convolutions (conv2d.hip, conv2d_wgrad.hip): plane scaling (scale_planes), the fused gradient sum
// (axpy_planes), per-plane dot products (plane_dot*), and the fp32 split of an operand into 16-bit parts with its magnitude bound
// (amax_bits, split16, unscale, plane_dot_parts).
#include "conv2d_common.h"

namespace afcm {

// 4 consecutive elements as one vector access (8 B for 16-bit types, 16 B for fp32); planes are 4-element aligned when hw % 4 == 0
template <typename T> struct Vec4 { T v[4]; } __attribute__((aligned(sizeof(T) * 4)));

// An fp32 value the compiler must form as such.  Left alone it folds the float16 conversion of a product into v_fma_mixlo_f16(a, b, +0): ONE
// rounding of the exact product, not the fp32 product rounded to nearest even (they differ where the fp32 product lands on a float16 tie),
// and -0 + +0 = +0 loses the sign of a zero.
__device__ __forceinline__ float formed_f32(float v) { asm("" : "+v"(v)); return v; }

// y[plane, :] = x[plane, :] * scale[plane]: the fp32 product, rounded to nearest even into y's type.  HBM-bound elementwise pass.
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void scale_planes_kernel(TO* __restrict__ y, const TI* __restrict__ x, const float* __restrict__ scale,
                                                           long long planes, int hw) {
    const int per = (hw + 3) >> 2;
    const long long total = planes * per;
    // vector accesses where every plane starts on a vector boundary of BOTH tensors (a contiguous view may sit at any element offset)
    const bool vec = (hw & 3) == 0 && ((uintptr_t)x & (sizeof(TI) * 4 - 1)) == 0 && ((uintptr_t)y & (sizeof(TO) * 4 - 1)) == 0;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long plane = idx / per;
        const int i0 = (int)(idx - plane * per) << 2;
        const float sc = scale ? scale[plane] : 1.f;
        const TI* xp = x + plane * hw + i0;
        TO* yp = y + plane * hw + i0;
        if (vec) {
            const Vec4<TI> in = *(const Vec4<TI>*)xp;
            Vec4<TO> out;
#pragma unroll
            for (int e = 0; e < 4; e++) out.v[e] = from_f32<TO>(formed_f32(to_f32(in.v[e]) * sc));
            *(Vec4<TO>*)yp = out;
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (i0 + e < hw) yp[e] = from_f32<TO>(formed_f32(to_f32(xp[e]) * sc));
        }
    }
}

// y[plane, :] = a[plane, :] + scale[plane] * b[plane, :] for 16-bit tensors of one layout (r06): the gradient of an encoder feature map that
// feeds BOTH the next encoder layer (a = that layer's data gradient) and a decoder layer's skip input (b = the decoder layer's incoming
// gradient, scale = the styles its epilogue multiplied the sum by).  The op-by-op form was scale_planes (read b, write s b) + autograd's
// accumulation (read both, write the sum): five passes over a 156 MB plane set where this is three, one rounding instead of two.
// 16-byte vectors; hw % 8 == 0 (host).
template <typename T>
__global__ __launch_bounds__(256) void axpy_planes_kernel(T* __restrict__ y, const T* __restrict__ a, const T* __restrict__ b, const float* __restrict__ scale,
                                                          long long planes, int hw) {
    union V16 { uint4 u; T v[8]; };
    const int per = hw >> 3;                                   // 16-byte vectors per plane
    for (long long plane = blockIdx.y; plane < planes; plane += gridDim.y) {
        const float sc = scale ? scale[plane] : 1.f;
        const uint4* ap = (const uint4*)a + plane * per;
        const uint4* bp = (const uint4*)b + plane * per;
        uint4* yp = (uint4*)y + plane * per;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < per; i += gridDim.x * blockDim.x) {
            V16 av, bv, out;
            av.u = ap[i];
            bv.u = bp[i];
#pragma unroll
            for (int e = 0; e < 8; e++) out.v[e] = from_f32<T>(to_f32(av.v[e]) + sc * to_f32(bv.v[e]));
            yp[i] = out.u;
        }
    }
}

// Magnitude bound of a tensor, for the float16 split (split16_kernel): out[0] = max(out[0], bits of max |scale[plane] * x[plane, :]|).
// Magnitudes compare as their bit patterns; r06: over the FINITE elements only (an inf / NaN element keeps its place in the split's first part
// whatever the factor).  The consumers turn the bound into the power of two g with
// g * bound in [2^14, 2^15) (pow2_factor): float16 parts of g * v cannot overflow (65504) and the second part of every element above
// 2^-18 of the bound is a normal number (below that it is a subnormal: 22 significand bits shrink to 11 at 2^-29 of the bound).  One bound
// per TENSOR, not per plane: the contraction sums over the input planes, so a per-plane factor cannot leave the sum (a per-sample one could
// in forward / data gradient, not in the weight gradient, which sums over samples) -- DESIGN.md section 4.4.
// One atomic per workgroup, and only from workgroups that would raise the value (2048 unconditional atomics on one word cost 50 us).
__global__ __launch_bounds__(256) void amax_bits_kernel(unsigned* __restrict__ out, const float* __restrict__ x, long long planes, int hw,
                                                        const float* __restrict__ scale) {
    __shared__ unsigned red[4];
    unsigned m = 0;
    const long long numel = planes * hw;
    const bool vec = (((uintptr_t)x & 15) == 0) && (hw & 3) == 0;
    const long long n4 = vec ? (numel >> 2) : 0;
    const int per = hw >> 2;                                 // 16-byte groups per plane (vec only)
    const long long stride = (long long)gridDim.x * blockDim.x;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    auto fold = [&](const uint4 v, long long g) {
        // non-finite magnitudes (exponent all ones) do not count: one inf or NaN would otherwise take the power-of-two factor -- and with it
        // 22-bit parts -- away from every finite element of the tensor; the split keeps such an element whole in its first part
        const unsigned ax = v.x & 0x7fffffffu, ay = v.y & 0x7fffffffu, az = v.z & 0x7fffffffu, aw = v.w & 0x7fffffffu;
        unsigned a = max(max(ax < 0x7f800000u ? ax : 0u, ay < 0x7f800000u ? ay : 0u), max(az < 0x7f800000u ? az : 0u, aw < 0x7f800000u ? aw : 0u));
        if (scale) {
            a = __float_as_uint(__uint_as_float(a) * __builtin_fabsf(scale[g / per]));              // |s| max|x| = max|s x|
            if (a >= 0x7f800000u) a = 0u;                                                           // (an overflowing or non-finite factor: as above)
        }
        m = max(m, a);
    };
    // four independent 16-byte loads in flight per lane
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const uint4 v0 = ((const uint4*)x)[i], v1 = ((const uint4*)x)[i + stride], v2 = ((const uint4*)x)[i + 2 * stride], v3 = ((const uint4*)x)[i + 3 * stride];
        fold(v0, i); fold(v1, i + stride); fold(v2, i + 2 * stride); fold(v3, i + 3 * stride);
    }
    for (; i < n4; i += stride) fold(((const uint4*)x)[i], i);
    for (long long j = 4 * n4 + (long long)blockIdx.x * blockDim.x + threadIdx.x; j < numel; j += stride) {
        const float v = x[j] * (scale ? scale[j / hw] : 1.f);
        const unsigned a = __float_as_uint(v) & 0x7fffffffu;
        m = max(m, a < 0x7f800000u ? a : 0u);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = max(max(red[0], red[1]), max(red[2], red[3]));
        if (m > __atomic_load_n(out, __ATOMIC_RELAXED)) atomicMax(out, m);
    }
}

// out[plane] = <sum_k parts[k][plane, :], b[plane, :]> / g: the style gradient's dot product <x, dx> of an fp32 conv whose backward kept the
// 16-bit parts of x (split16_kernel) instead of x.  One workgroup per plane; 4 elements per lane and iteration where the plane allows.
template <typename TP>
__global__ __launch_bounds__(256) void plane_dot_parts_kernel(float* __restrict__ out, const TP* __restrict__ parts, long long part_stride, int nparts,
                                                              const float* __restrict__ b, long long planes, int hw, const unsigned* __restrict__ bound) {
    __shared__ float red[4];
    const long long plane = blockIdx.x;
    if (plane >= planes) return;
    const TP* ap = parts + plane * hw;
    const float* bp = b + plane * hw;
    float acc = 0.f;
    if ((hw & 3) == 0 && (part_stride & 3) == 0) {          // 8-byte part loads, 16-byte b loads (the generator's planes: hw % 4 == 0)
        union V8 { uint2 u; TP v[4]; };
        for (int i = threadIdx.x * 4; i < hw; i += blockDim.x * 4) {
            const float4 b0 = *(const float4*)(bp + i);
            const float bv[4] = {b0.x, b0.y, b0.z, b0.w};
            for (int k = 0; k < nparts; k++) {
                V8 a; a.u = *(const uint2*)(ap + k * part_stride + i);
#pragma unroll
                for (int e = 0; e < 4; e++) acc += (float)a.v[e] * bv[e];
            }
        }
    } else {
        for (int i = threadIdx.x; i < hw; i += blockDim.x) {
            float a = 0.f;
            for (int k = 0; k < nparts; k++) a += (float)ap[k * part_stride + i];
            acc += a * bp[i];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float inv = 1.f;
        if (bound) pow2_factor(bound[0], &inv);
        out[plane] = (red[0] + red[1] + red[2] + red[3]) * inv;
    }
}

// t *= 1 / (g_a g_b): the power-of-two factors of two split operands undone (weight gradient of split parts).
__global__ __launch_bounds__(256) void unscale_kernel(float* __restrict__ t, long long numel, const unsigned* __restrict__ bound_a, const unsigned* __restrict__ bound_b) {
    float ia = 1.f, ib = 1.f;
    if (bound_a) pow2_factor(bound_a[0], &ia);
    if (bound_b) pow2_factor(bound_b[0], &ib);
    const float inv = ia * ib;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < numel; i += (long long)gridDim.x * blockDim.x) t[i] *= inv;
}

// Split-precision operands: v = g * scale[plane] * x (g: pow2_factor of the bound word, 1 without one) as a sum of `parts` 16-bit numbers, v ~ a + b (+ c) with a = r16(v), b = r16(v - a),
// c = r16(v - a - b) (round to nearest even; the differences are exact in fp32).  bfloat16: two parts carry 16 significand bits, three
// carry all 24.  float16: two parts carry 22 bits wherever b is a normal number, i.e. for |v| >= 2^-3; below that the error is at most
// 2^-25 ABSOLUTE, so with g the power of two that brings the tensor's largest magnitude near 2^15 it is 2^-40 of that magnitude.
// parts[k] is a dense tensor of the input's shape, part_stride elements after parts[k - 1].  A non-finite v keeps its class in part a
// and zeros in the others (inf - inf would make NaNs of infinities).
template <typename TP, int PARTS>
__global__ __launch_bounds__(256) void split16_kernel(TP* __restrict__ parts, const float* __restrict__ x, const float* __restrict__ scale,
                                                      const unsigned* __restrict__ bound, long long planes, int hw, long long part_stride) {
    const int per = (hw + 3) >> 2;
    const long long total = planes * per;
    const bool vec = (hw & 3) == 0;
    const float gs = bound ? pow2_factor(bound[0]) : 1.f;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long plane = idx / per;
        const int i0 = (int)(idx - plane * per) << 2;
        const float sc = (scale ? scale[plane] : 1.f) * gs;
        const float* xp = x + plane * hw + i0;
        TP* yp = parts + plane * hw + i0;
        float v[4];
        if (vec) {
            const Vec4<float> in = *(const Vec4<float>*)xp;
#pragma unroll
            for (int e = 0; e < 4; e++) v[e] = in.v[e] * sc;
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) v[e] = (i0 + e < hw) ? xp[e] * sc : 0.f;
        }
        Vec4<TP> out[PARTS];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            float r = v[e];
#pragma unroll
            for (int k = 0; k < PARTS; k++) {
                const TP q = (TP)r;
                out[k].v[e] = q;
                const float qf = (float)q;
                r = (__builtin_fabsf(qf) <= 3.4028234664e38f) ? r - qf : 0.f;      // inf / nan: nothing left for the lower parts
            }
        }
#pragma unroll
        for (int k = 0; k < PARTS; k++) {
            if (vec) {
                *(Vec4<TP>*)(yp + k * part_stride) = out[k];
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (i0 + e < hw) yp[k * part_stride + e] = out[k].v[e];
            }
        }
    }
}

// Per-plane reductions: out[plane] = sum a*b (or sum a when b == null).  One workgroup per plane, fp32 accumulate, 16-byte
// loads from the plane's first 16-byte boundary on (both operands share the plane offset; the host checks the base pointers).
template <typename T>
__global__ __launch_bounds__(256) void plane_dot_kernel(float* __restrict__ out, const T* __restrict__ a, const T* __restrict__ b,
                                                        long long planes, int hw) {
    constexpr int E = 16 / (int)sizeof(T);
    union V16 { uint4 u; T v[E]; };
    __shared__ float part[4];
    const long long plane = blockIdx.x;
    if (plane >= planes) return;
    const long long off = plane * hw;
    const T* ap = a + off;
    const T* bp = b ? b + off : nullptr;
    int head = (int)((E - (off % E)) % E);
    if (head > hw) head = hw;
    const int nv = (hw - head) / E;
    float s0 = 0.f, s1 = 0.f;
    {   // ragged ends: fewer than 2E elements in total
        const int tail0 = head + nv * E;
        int i = -1;
        if ((int)threadIdx.x < head) i = threadIdx.x;
        else if ((int)threadIdx.x - head < hw - tail0) i = tail0 + (int)threadIdx.x - head;
        if (i >= 0) s0 = to_f32(ap[i]) * (bp ? to_f32(bp[i]) : 1.f);
    }
    const uint4* av = (const uint4*)(ap + head);
    const uint4* bv = bp ? (const uint4*)(bp + head) : nullptr;
    int i = threadIdx.x;
    if (bv) {
        // four 16-byte loads per operand in flight (128 B per lane) before the first use
        for (; i + 768 < nv; i += 1024) {
            V16 a0, a1, a2, a3, b0, b1, b2, b3;
            a0.u = av[i]; a1.u = av[i + 256]; a2.u = av[i + 512]; a3.u = av[i + 768];
            b0.u = bv[i]; b1.u = bv[i + 256]; b2.u = bv[i + 512]; b3.u = bv[i + 768];
#pragma unroll
            for (int e = 0; e < E; e++) {
                s0 = fmaf(to_f32(a0.v[e]), to_f32(b0.v[e]), s0); s1 = fmaf(to_f32(a1.v[e]), to_f32(b1.v[e]), s1);
                s0 = fmaf(to_f32(a2.v[e]), to_f32(b2.v[e]), s0); s1 = fmaf(to_f32(a3.v[e]), to_f32(b3.v[e]), s1);
            }
        }
    }
    for (; i + 256 < nv; i += 512) {
        V16 a0, a1, b0, b1;
        a0.u = av[i]; a1.u = av[i + 256];
        if (bv) {
            b0.u = bv[i]; b1.u = bv[i + 256];
#pragma unroll
            for (int e = 0; e < E; e++) { s0 = fmaf(to_f32(a0.v[e]), to_f32(b0.v[e]), s0); s1 = fmaf(to_f32(a1.v[e]), to_f32(b1.v[e]), s1); }
        } else {
#pragma unroll
            for (int e = 0; e < E; e++) { s0 += to_f32(a0.v[e]); s1 += to_f32(a1.v[e]); }
        }
    }
    if (i < nv) {
        V16 a0, b0;
        a0.u = av[i];
        if (bv) {
            b0.u = bv[i];
#pragma unroll
            for (int e = 0; e < E; e++) s0 = fmaf(to_f32(a0.v[e]), to_f32(b0.v[e]), s0);
        } else {
#pragma unroll
            for (int e = 0; e < E; e++) s0 += to_f32(a0.v[e]);
        }
    }
    float s = s0 + s1;
#pragma unroll
    for (int off2 = 32; off2 > 0; off2 >>= 1) s += __shfl_down(s, off2, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[plane] = part[0] + part[1] + part[2] + part[3];
}

// Small planes (<= 16 KB): one WAVE per plane, four planes per workgroup -- a 36^2 plane is 180 16-byte pieces, so a
// 256-thread workgroup per plane leaves most lanes without a load and the launch is bound by workgroup turnover.
template <typename T>
__global__ __launch_bounds__(256) void plane_dot_wave_kernel(float* __restrict__ out, const T* __restrict__ a, const T* __restrict__ b,
                                                             long long planes, int hw) {
    constexpr int E = 16 / (int)sizeof(T);
    union V16 { uint4 u; T v[E]; };
    const int lane = threadIdx.x & 63;
    const long long plane = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (plane >= planes) return;
    const long long off = plane * hw;
    const T* ap = a + off;
    const T* bp = b ? b + off : nullptr;
    int head = (int)((E - (off % E)) % E);
    if (head > hw) head = hw;
    const int nv = (hw - head) / E;
    float s0 = 0.f, s1 = 0.f;
    {   // ragged ends: fewer than 2E <= 16 elements in total
        const int tail0 = head + nv * E;
        int i = -1;
        if (lane < head) i = lane;
        else if (lane - head < hw - tail0) i = tail0 + lane - head;
        if (i >= 0) s0 = to_f32(ap[i]) * (bp ? to_f32(bp[i]) : 1.f);
    }
    const uint4* av = (const uint4*)(ap + head);
    const uint4* bv = bp ? (const uint4*)(bp + head) : nullptr;
    int i = lane;
    for (; i + 64 < nv; i += 128) {
        V16 a0, a1, b0, b1;
        a0.u = av[i]; a1.u = av[i + 64];
        if (bv) {
            b0.u = bv[i]; b1.u = bv[i + 64];
#pragma unroll
            for (int e = 0; e < E; e++) { s0 = fmaf(to_f32(a0.v[e]), to_f32(b0.v[e]), s0); s1 = fmaf(to_f32(a1.v[e]), to_f32(b1.v[e]), s1); }
        } else {
#pragma unroll
            for (int e = 0; e < E; e++) { s0 += to_f32(a0.v[e]); s1 += to_f32(a1.v[e]); }
        }
    }
    if (i < nv) {
        V16 a0, b0;
        a0.u = av[i];
        if (bv) {
            b0.u = bv[i];
#pragma unroll
            for (int e = 0; e < E; e++) s0 = fmaf(to_f32(a0.v[e]), to_f32(b0.v[e]), s0);
        } else {
#pragma unroll
            for (int e = 0; e < E; e++) s0 += to_f32(a0.v[e]);
        }
    }
    float s = s0 + s1;
#pragma unroll
    for (int off2 = 32; off2 > 0; off2 >>= 1) s += __shfl_down(s, off2, 64);
    if (lane == 0) out[plane] = s;
}

// Row-pitched operands (planes [h][ld], the first w columns of a row meaningful -- the 16-bit activation layout of DESIGN.md
// section 3): 16-byte vectors within a row; the last vector of a row is shifted back to END at column w (no access past the row,
// the re-read elements are selected out), so nothing depends on what the padding holds.  PER_WAVE: one wave per plane, four
// planes per workgroup (small planes, as plane_dot_wave_kernel).  Needs w >= 16 / sizeof(T).
// Gate of the "dot product by homogeneity" (afcm_plane_dot_gated_ld): a plane none of whose strips could reach the clamp takes
//     out = osc (gz - nsc gsk)                     (nsc, gsk may be NULL: 1, 0)
// and its wave / workgroup leaves without touching a or b; a flagged plane gets the real dot product, and so does a plane whose two
// sums cancel to less than 1/8 of their size (|skip| >> |F(y)| amplifies the rounding of z by that ratio).
struct PlaneGate {
    const int* flags;     // [planes][slots], NULL: no gate
    int slots;
    const float *osc, *gz, *nsc, *gsk;
};
template <typename T, bool PER_WAVE>
__global__ __launch_bounds__(256) void plane_dot_rows_kernel(float* __restrict__ out, const T* __restrict__ a, const T* __restrict__ b,
                                                             long long planes, int h, int w, int lda, int ldb, PlaneGate gate) {
    constexpr int E = 16 / (int)sizeof(T);
    union V16 { uint4 u; T v[E]; };
    __shared__ float part[4];
    const int nthr = PER_WAVE ? 64 : 256;
    const int t = PER_WAVE ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    const long long plane = PER_WAVE ? (long long)blockIdx.x * 4 + (threadIdx.x >> 6) : (long long)blockIdx.x;
    if (plane >= planes) return;                               // PER_WAVE: a whole wave leaves (no barrier below in that mode)
    if (gate.flags != nullptr) {
        int any = 0;                                           // (wave- / workgroup-uniform: every thread reads the same words)
        for (int i = 0; i < gate.slots; i++) any |= gate.flags[plane * gate.slots + i];
        if (!any) {
            // ... unless the two sums cancel: each carries the 16-bit rounding of z / skip (2^-9 relative in bf16), so their difference is
            // trusted down to 1/8 of their size (a skip branch that dwarfs this layer's own output); beyond that the plane takes the real
            // dot product like a flagged one
            const float zz = gate.gz[plane], kk = gate.gsk ? (gate.nsc ? gate.nsc[plane] : 1.f) * gate.gsk[plane] : 0.f;
            const float diff = zz - kk;
            if (!(gate.gsk != nullptr && fabsf(diff) * 8.f < fabsf(zz) + fabsf(kk))) {
                if (t == 0) out[plane] = gate.osc[plane] * diff;
                return;
            }
        }
    }
    const int nvec = (w + E - 1) / E, total = h * nvec;
    // row = ic / nvec by the round-up reciprocal ceil(2^32 / nvec): never below the quotient and, ic < 2^31, at most one above it (from
    // ic * (nvec * magic - 2^32) >= 2^32 on: 257 rows of 4092 vectors) -- a row that starts after ic steps back.  One vector per row
    // (w == E) has no 32-bit reciprocal: row = ic.
    const unsigned magic = nvec > 1 ? (unsigned)((0x100000000ull + (unsigned)nvec - 1) / (unsigned)nvec) : 0u;
    const T* ap = a + plane * h * lda;
    const T* bp = b ? b + plane * h * ldb : nullptr;
    float s0 = 0.f, s1 = 0.f;
    for (int i0 = t; i0 < total; i0 += 4 * nthr) {
        V16 av[4], bv[4];
        int skip[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int i = i0 + u * nthr;
            const int ic = i < total ? i : total - 1;
            int row = nvec > 1 ? (int)__umulhi((unsigned)ic, magic) : ic;
            row -= row * nvec > ic;
            const int col = (ic - row * nvec) * E;
            const int colc = col + E <= w ? col : w - E;
            skip[u] = i < total ? col - colc : E;              // leading elements that an earlier vector already counted (E: none live)
            av[u].u = *(const uint4*)(ap + (size_t)row * lda + colc);
            if (bp) bv[u].u = *(const uint4*)(bp + (size_t)row * ldb + colc);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
#pragma unroll
            for (int e = 0; e < E; e++) {
                const float x = e >= skip[u] ? to_f32(av[u].v[e]) : 0.f;
                const float y = bp ? to_f32(bv[u].v[e]) : 1.f;
                if (u & 1) s1 = fmaf(x, e >= skip[u] ? y : 0.f, s1); else s0 = fmaf(x, e >= skip[u] ? y : 0.f, s0);
            }
        }
    }
    float s = s0 + s1;
#pragma unroll
    for (int off2 = 32; off2 > 0; off2 >>= 1) s += __shfl_down(s, off2, 64);
    if (PER_WAVE) {
        if ((threadIdx.x & 63) == 0) out[plane] = s;
    } else {
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) out[plane] = part[0] + part[1] + part[2] + part[3];
    }
}

}  // namespace afcm

using namespace afcm;

extern "C" int afcm_split16(void* parts, const float* x, const float* scale, const uint32_t* bound, int32_t dtype, int64_t planes, int32_t hw,
                            int32_t nparts, int64_t part_stride, void* stream) {
    AFCM_REQUIRE(parts != nullptr && x != nullptr && planes > 0 && hw > 0, "split16: empty input");
    AFCM_REQUIRE(dtype == AFCM_BF16 || dtype == AFCM_F16, "split16: parts are bfloat16 or float16");
    AFCM_REQUIRE(nparts == 2 || nparts == 3, "split16: 2 or 3 parts (got %d)", nparts);
    AFCM_REQUIRE(part_stride >= planes * (long long)hw && part_stride % 4 == 0, "split16: part stride %lld must cover the tensor and be a multiple of 4", (long long)part_stride);
    AFCM_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)parts & 7) == 0, "split16: x must be 16-byte, parts 8-byte aligned");
    long long blocks = (planes * ((hw + 3) >> 2) + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    dim3 grid((unsigned)blocks), block(256);
    hipStream_t st = (hipStream_t)stream;
#define AFCM_SPLIT(T, K) hipLaunchKernelGGL((split16_kernel<T, K>), grid, block, 0, st, (T*)parts, x, scale, (const unsigned*)bound, (long long)planes, hw, (long long)part_stride)
    if (dtype == AFCM_BF16) { if (nparts == 2) AFCM_SPLIT(bf16_t, 2); else AFCM_SPLIT(bf16_t, 3); }
    else { if (nparts == 2) AFCM_SPLIT(f16_t, 2); else AFCM_SPLIT(f16_t, 3); }
#undef AFCM_SPLIT
    return hip_status(hipGetLastError());
}

extern "C" int afcm_amax_bits(uint32_t* out, const float* x, int64_t planes, int32_t hw, const float* scale, void* stream) {
    AFCM_REQUIRE(out != nullptr && x != nullptr && planes > 0 && hw > 0, "amax_bits: empty input");
    AFCM_REQUIRE(((uintptr_t)out & 3) == 0 && ((uintptr_t)x & 3) == 0, "amax_bits: misaligned pointer");
    long long blocks = (planes * hw / 16 + 255) / 256;          // >= 4 16-byte groups per lane
    blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(amax_bits_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (unsigned*)out, x, (long long)planes, hw, scale);
    return hip_status(hipGetLastError());
}

extern "C" int afcm_plane_dot_parts(float* out, const void* parts, int64_t part_stride, int32_t nparts, const float* b, int32_t dtype, int64_t planes,
                                    int32_t hw, const uint32_t* bound, void* stream) {
    AFCM_REQUIRE(out != nullptr && parts != nullptr && b != nullptr && planes > 0 && hw > 0, "plane_dot_parts: empty input");
    AFCM_REQUIRE(dtype == AFCM_BF16 || dtype == AFCM_F16, "plane_dot_parts: parts are bfloat16 or float16");
    AFCM_REQUIRE(nparts >= 1 && nparts <= 3 && part_stride >= planes * (long long)hw, "plane_dot_parts: 1..3 parts, a stride covering the tensor");
    AFCM_REQUIRE(planes < (1ll << 31), "plane_dot_parts: too many planes");
    AFCM_REQUIRE(((uintptr_t)parts & 7) == 0 && ((uintptr_t)b & 15) == 0, "plane_dot_parts: parts must be 8-byte, b 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == AFCM_BF16) hipLaunchKernelGGL((plane_dot_parts_kernel<bf16_t>), dim3((unsigned)planes), dim3(256), 0, st, out, (const bf16_t*)parts, (long long)part_stride, nparts, b, (long long)planes, hw, (const unsigned*)bound);
    else hipLaunchKernelGGL((plane_dot_parts_kernel<f16_t>), dim3((unsigned)planes), dim3(256), 0, st, out, (const f16_t*)parts, (long long)part_stride, nparts, b, (long long)planes, hw, (const unsigned*)bound);
    return hip_status(hipGetLastError());
}

extern "C" int afcm_unscale(float* t, int64_t numel, const uint32_t* bound_a, const uint32_t* bound_b, void* stream) {
    AFCM_REQUIRE(t != nullptr && numel > 0, "unscale: empty input");
    long long blocks = (numel + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(unscale_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, t, (long long)numel, (const unsigned*)bound_a, (const unsigned*)bound_b);
    return hip_status(hipGetLastError());
}

extern "C" int afcm_scale_planes(void* y, const void* x, const float* scale, int32_t dtype_in, int32_t dtype_out, int64_t planes,
                                 int32_t hw, void* stream) {
    AFCM_REQUIRE(y != nullptr && x != nullptr && planes > 0 && hw > 0, "scale_planes: empty input");
    long long blocks = (planes * ((hw + 3) >> 2) + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    dim3 grid((unsigned)blocks), block(256);
    hipStream_t st = (hipStream_t)stream;
#define AFCM_SP(TI, TO) hipLaunchKernelGGL((scale_planes_kernel<TI, TO>), grid, block, 0, st, (TO*)y, (const TI*)x, scale, (long long)planes, hw)
    if (dtype_in == AFCM_F32 && dtype_out == AFCM_F32) AFCM_SP(float, float);
    else if (dtype_in == AFCM_F32 && dtype_out == AFCM_BF16) AFCM_SP(float, bf16_t);
    else if (dtype_in == AFCM_F32 && dtype_out == AFCM_F16) AFCM_SP(float, f16_t);
    else if (dtype_in == AFCM_BF16 && dtype_out == AFCM_BF16) AFCM_SP(bf16_t, bf16_t);
    else if (dtype_in == AFCM_F16 && dtype_out == AFCM_F16) AFCM_SP(f16_t, f16_t);
    else if (dtype_in == AFCM_BF16 && dtype_out == AFCM_F32) AFCM_SP(bf16_t, float);
    else if (dtype_in == AFCM_F16 && dtype_out == AFCM_F32) AFCM_SP(f16_t, float);
    else { set_error("scale_planes: unsupported dtype pair %d -> %d", dtype_in, dtype_out); return AFCM_E_INVALID; }
#undef AFCM_SP
    return hip_status(hipGetLastError());
}

extern "C" int afcm_axpy_planes(void* y, const void* a, const void* b, const float* scale, int32_t dtype, int64_t planes, int32_t hw, void* stream) {
    AFCM_REQUIRE(y != nullptr && a != nullptr && b != nullptr && planes > 0 && hw > 0, "axpy_planes: empty input");
    AFCM_REQUIRE(dtype == AFCM_F16 || dtype == AFCM_BF16, "axpy_planes: 16-bit tensors only");
    if ((hw & 7) != 0 || ((((uintptr_t)y | (uintptr_t)a | (uintptr_t)b)) & 15) != 0) return AFCM_E_NOKERNEL;
    const int per = hw >> 3;
    // grid.y = planes (one scale per workgroup), grid.x = 1 KB-per-thread-block slices of a plane: >= 4 vectors per thread on the large planes
    const dim3 grid((unsigned)((per + 1023) / 1024), (unsigned)(planes < 65535 ? planes : 65535));
    hipStream_t st = (hipStream_t)stream;
    if (dtype == AFCM_BF16) hipLaunchKernelGGL((axpy_planes_kernel<bf16_t>), grid, dim3(256), 0, st, (bf16_t*)y, (const bf16_t*)a, (const bf16_t*)b, scale, (long long)planes, hw);
    else hipLaunchKernelGGL((axpy_planes_kernel<f16_t>), grid, dim3(256), 0, st, (f16_t*)y, (const f16_t*)a, (const f16_t*)b, scale, (long long)planes, hw);
    return hip_status(hipGetLastError());
}

extern "C" int afcm_plane_dot(float* out, const void* a, const void* b, int32_t dtype, int64_t planes, int32_t hw, void* stream) {
    AFCM_REQUIRE(out != nullptr && a != nullptr && planes > 0 && hw > 0, "plane_dot: empty input");
    AFCM_REQUIRE(planes < (1ll << 31), "plane_dot: too many planes");
    AFCM_REQUIRE((((uintptr_t)a | (uintptr_t)b) & 15) == 0, "plane_dot: operands must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int esize = dtype == AFCM_F32 ? 4 : 2;
    const bool per_wave = (long long)hw * esize <= 16384;
    dim3 grid((unsigned)(per_wave ? (planes + 3) / 4 : planes)), block(256);
#define AFCM_PD(T) do { \
        if (per_wave) hipLaunchKernelGGL((plane_dot_wave_kernel<T>), grid, block, 0, st, out, (const T*)a, (const T*)b, (long long)planes, hw); \
        else hipLaunchKernelGGL((plane_dot_kernel<T>), grid, block, 0, st, out, (const T*)a, (const T*)b, (long long)planes, hw); } while (0)
    switch (dtype) {
        case AFCM_F32: AFCM_PD(float); break;
        case AFCM_F16: AFCM_PD(f16_t); break;
        case AFCM_BF16: AFCM_PD(bf16_t); break;
        default: set_error("plane_dot: bad dtype"); return AFCM_E_INVALID;
    }
#undef AFCM_PD
    return hip_status(hipGetLastError());
}

static int plane_dot_rows(float* out, const void* a, const void* b, int32_t dtype, int64_t planes, int32_t h, int32_t w,
                          int32_t a_pitch, int32_t b_pitch, const PlaneGate& gate, void* stream) {
    AFCM_REQUIRE(out != nullptr && a != nullptr && planes > 0 && h > 0 && w > 0, "plane_dot: empty input");
    AFCM_REQUIRE(planes < (1ll << 31), "plane_dot: too many planes");
    const int esize = dtype == AFCM_F32 ? 4 : 2;
    const int lda = a_pitch ? a_pitch : w, ldb = b_pitch ? b_pitch : w;
    AFCM_REQUIRE(lda >= w && ldb >= w, "plane_dot: row pitches %d / %d are below the width %d", lda, ldb, w);
    AFCM_REQUIRE(w >= 16 / esize, "plane_dot: rows of %d elements are shorter than one 16-byte vector", w);
    AFCM_REQUIRE((((uintptr_t)a | (uintptr_t)b) & 3) == 0 && (esize == 4 || ((w | lda | ldb) & 1) == 0), "plane_dot: rows must start on 4-byte boundaries");
    AFCM_REQUIRE((long long)h * (lda > ldb ? lda : ldb) < (1ll << 31) / 16, "plane_dot: plane is out of range");
    hipStream_t st = (hipStream_t)stream;
    const bool per_wave = (long long)h * w * esize <= 16384;
    dim3 grid((unsigned)(per_wave ? (planes + 3) / 4 : planes)), block(256);
#define AFCM_PDR(T) do { \
        if (per_wave) hipLaunchKernelGGL((plane_dot_rows_kernel<T, true>), grid, block, 0, st, out, (const T*)a, (const T*)b, (long long)planes, h, w, lda, ldb, gate); \
        else hipLaunchKernelGGL((plane_dot_rows_kernel<T, false>), grid, block, 0, st, out, (const T*)a, (const T*)b, (long long)planes, h, w, lda, ldb, gate); } while (0)
    switch (dtype) {
        case AFCM_F32: AFCM_PDR(float); break;
        case AFCM_F16: AFCM_PDR(f16_t); break;
        case AFCM_BF16: AFCM_PDR(bf16_t); break;
        default: set_error("plane_dot: bad dtype"); return AFCM_E_INVALID;
    }
#undef AFCM_PDR
    return hip_status(hipGetLastError());
}

extern "C" int afcm_plane_dot_ld(float* out, const void* a, const void* b, int32_t dtype, int64_t planes, int32_t h, int32_t w,
                                 int32_t a_pitch, int32_t b_pitch, void* stream) {
    return plane_dot_rows(out, a, b, dtype, planes, h, w, a_pitch, b_pitch, PlaneGate{nullptr, 0, nullptr, nullptr, nullptr, nullptr}, stream);
}

extern "C" int afcm_plane_dot_gated_ld(float* out, const void* a, const void* b, int32_t dtype, int64_t planes, int32_t h, int32_t w,
                                       int32_t a_pitch, int32_t b_pitch, const int32_t* flags, int32_t slots, const float* out_scale,
                                       const float* gz, const float* next_scale, const float* gskip, void* stream) {
    AFCM_REQUIRE(flags != nullptr && slots > 0 && out_scale != nullptr && gz != nullptr && b != nullptr, "plane_dot_gated: null pointer");
    return plane_dot_rows(out, a, b, dtype, planes, h, w, a_pitch, b_pitch, PlaneGate{flags, slots, out_scale, gz, next_scale, gskip}, stream);
}
