// Epilogue of the CoModGAN modulated convolution (networks_comodgan.SynthesisLayer) for gfx950, fp32 tensors:
//   y[n, o, U i + py, U j + px] = clamp(lrelu(t[n, (py U + px) O + o, i, j] * dcoefs[n, o] + noise * strength + bias[o]) * gain, +-clamp)
// U = 2: t is the 3x3 convolution with the four folded phase kernels of the up-2 layer and the kernel interleaves the phases
// (depth to space) as it writes; U = 1: the plain layer.  One thread takes V consecutive LOW-resolution pixels of a row, V = 4 / U
// when w % V == 0 and every tensor is 16-byte aligned (every layer of the network), else V = 1: per phase plane one 4 V-byte read,
// per output row one 4 U V-byte store, consecutive over the wave.  No LDS in the forward, no full-resolution intermediate.
// HBM-bound: 4 bytes read and 4 bytes written per output element (12 and 4 backward).
//
// Every element is evaluated in float64 and rounded once, so the result is the correctly rounded value of the formula (the
// clamp compares the rounded value with the clamp rounded to fp32: rounding is monotone, so that is the same number).
//
// Backward (first order only), from dy, the saved y and t:  g = dy * (y > 0 ? 1 : alpha) * gain, 0 where |y| >= clamp
// (bias_act's conventions: the slope alpha AT the kink y == 0, no gradient AT the clamp), then
//   d_t = g * dcoefs,  d_dcoefs[n, o] = sum g * t,  d_bias[o] = sum g,  d_strength = sum g * noise.
// The sums are float64, without atomics, in ONE order:
//   1. per workgroup (plane (n, o), chunk c of 256 V low-resolution pixels, thread t at pixels 256 V c + V t ...): a thread adds its
//      elements in the order (py, px, pixel) onto +0.0; the tree s[t] += s[t + k] for k = 128, 64, ..., 1 -> part[plane][c][3]
//   2. per plane: lane l adds chunks l, l + 64, ... in ascending order; the tree k = 32, ..., 1 -> plane_sum[plane][3]; d_dcoefs
//   3. d_bias[o]: the planes n = 0, 1, ... of channel o in ascending order.  d_strength: thread t adds planes t, t + 256, ... in
//      ascending order, then the tree k = 128, ..., 1.
// so two launches give the same bits (V is a function of the shape and the pointers' alignment).
#include "common.h"

namespace afcm {

struct ModconvEpi {
    float* y;                 // forward: out.  backward: d_t
    const float* t;
    const float* dcoefs;
    const float* bias;
    const float* noise;
    const float* strength;
    const float* dy;
    const float* ysaved;
    double* part;
    long long noise_stride;   // 0: one [UH, UW] plane for every sample
    int n, o, h, w, chunks;
    double alpha, gain;
    float clamp;              // < 0: none
};

constexpr int kEpiThreads = 256;

// K consecutive floats as one 4 K-byte access (the caller guarantees the alignment)
template <int K> __device__ __forceinline__ void load_vec(const float* p, float* out) {
    if (K == 4) { const float4 v = *(const float4*)p; out[0] = v.x; out[K > 1 ? 1 : 0] = v.y; out[K > 2 ? 2 : 0] = v.z; out[K > 3 ? 3 : 0] = v.w; }
    else if (K == 2) { const float2 v = *(const float2*)p; out[0] = v.x; out[K > 1 ? 1 : 0] = v.y; }
    else out[0] = p[0];
}
template <int K> __device__ __forceinline__ void store_vec(float* p, const float* in) {
    if (K == 4) *(float4*)p = make_float4(in[0], in[K > 1 ? 1 : 0], in[K > 2 ? 2 : 0], in[K > 3 ? 3 : 0]);
    else if (K == 2) *(float2*)p = make_float2(in[0], in[K > 1 ? 1 : 0]);
    else p[0] = in[0];
}

// One thread = V consecutive low-resolution pixels of one row (the host picks V > 1 only when w % V == 0 and every tensor is 16-byte aligned):
// V-float loads from each phase plane, U V-float stores per output row.  U V is 4 on the vector path (16-byte stores), U on the element path.
template <int U, int V>
__global__ __launch_bounds__(kEpiThreads) void modconv_epilogue_fwd_kernel(ModconvEpi p) {
    const int plane = blockIdx.x / p.chunks, chunk = blockIdx.x - plane * p.chunks;
    const int hw = p.h * p.w, pix = (chunk * kEpiThreads + threadIdx.x) * V;
    if (pix >= hw) return;
    const int n = plane / p.o, o = plane - n * p.o;
    const int i = pix / p.w, j = pix - i * p.w;
    const double d = (double)p.dcoefs[plane], b = (double)p.bias[o];
    const double s = p.noise ? (double)p.strength[0] : 0.0;
    const long long ohw = (long long)hw * U * U;
    const float* nz = p.noise ? p.noise + (long long)n * p.noise_stride : nullptr;
    float* yp = p.y + (long long)plane * ohw;
#pragma unroll
    for (int py = 0; py < U; py++) {
        float out[U * V], nv[U * V];
        const long long row = (long long)(i * U + py) * (p.w * U) + j * U;
        if (nz) load_vec<U * V>(nz + row, nv);
#pragma unroll
        for (int px = 0; px < U; px++) {
            float tv[V];
            load_vec<V>(p.t + (((long long)n * (U * U) + (py * U + px)) * p.o + o) * hw + pix, tv);
#pragma unroll
            for (int v = 0; v < V; v++) {
                double a = (double)tv[v] * d + b;
                if (nz) a += (double)nv[v * U + px] * s;
                a = (a > 0.0 ? a : a * p.alpha) * p.gain;
                float r = (float)a;
                if (p.clamp >= 0.f) r = fminf(fmaxf(r, -p.clamp), p.clamp);
                out[v * U + px] = r;
            }
        }
        store_vec<U * V>(yp + row, out);
    }
}

template <int U, int V>
__global__ __launch_bounds__(kEpiThreads) void modconv_epilogue_bwd_kernel(ModconvEpi p) {
    __shared__ double red[3][kEpiThreads];
    const int plane = blockIdx.x / p.chunks, chunk = blockIdx.x - plane * p.chunks;
    const int hw = p.h * p.w, pix = (chunk * kEpiThreads + threadIdx.x) * V;
    const int n = plane / p.o, o = plane - n * p.o;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    if (pix < hw) {
        const int i = pix / p.w, j = pix - i * p.w;
        const double d = (double)p.dcoefs[plane];
        const long long ohw = (long long)hw * U * U;
        const float* nz = p.noise ? p.noise + (long long)n * p.noise_stride : nullptr;
        const float* yp = p.ysaved + (long long)plane * ohw;
        const float* dyp = p.dy + (long long)plane * ohw;
#pragma unroll
        for (int py = 0; py < U; py++) {
            const long long row = (long long)(i * U + py) * (p.w * U) + j * U;
            float yv[U * V], dv[U * V], nv[U * V];
            load_vec<U * V>(yp + row, yv);
            load_vec<U * V>(dyp + row, dv);
            if (nz) load_vec<U * V>(nz + row, nv);
#pragma unroll
            for (int px = 0; px < U; px++) {
                const long long ti = (((long long)n * (U * U) + (py * U + px)) * p.o + o) * hw + pix;
                float tv[V], gt[V];
                load_vec<V>(p.t + ti, tv);
#pragma unroll
                for (int v = 0; v < V; v++) {
                    const float yy = yv[v * U + px];
                    double g = (double)dv[v * U + px] * (yy > 0.f ? 1.0 : p.alpha) * p.gain;
                    if (p.clamp >= 0.f && !(yy > -p.clamp && yy < p.clamp)) g = 0.0;
                    gt[v] = (float)(g * d);
                    a0 += g;
                    a1 += g * (double)tv[v];
                    if (nz) a2 += g * (double)nv[v * U + px];
                }
                store_vec<V>(p.y + ti, gt);
            }
        }
    }
    red[0][threadIdx.x] = a0; red[1][threadIdx.x] = a1; red[2][threadIdx.x] = a2;
    __syncthreads();
    for (int k = kEpiThreads / 2; k >= 1; k >>= 1) {
        if ((int)threadIdx.x < k) {
#pragma unroll
            for (int q = 0; q < 3; q++) red[q][threadIdx.x] += red[q][threadIdx.x + k];
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) p.part[(long long)blockIdx.x * 3 + threadIdx.x] = red[threadIdx.x][0];
}

// step 2: one wave per plane
__global__ __launch_bounds__(64) void modconv_epilogue_plane_kernel(double* __restrict__ plane_sum, float* __restrict__ d_dcoefs,
                                                                   const double* __restrict__ part, int chunks) {
    __shared__ double red[3][64];
    const long long plane = blockIdx.x;
    double a[3] = {0.0, 0.0, 0.0};
    for (int c = threadIdx.x; c < chunks; c += 64)
        for (int q = 0; q < 3; q++) a[q] += part[(plane * chunks + c) * 3 + q];
    for (int q = 0; q < 3; q++) red[q][threadIdx.x] = a[q];
    __syncthreads();
    for (int k = 32; k >= 1; k >>= 1) {
        if ((int)threadIdx.x < k)
            for (int q = 0; q < 3; q++) red[q][threadIdx.x] += red[q][threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x < 3) plane_sum[plane * 3 + threadIdx.x] = red[threadIdx.x][0];
    if (threadIdx.x == 0) d_dcoefs[plane] = (float)red[1][0];
}

// step 3: one workgroup
__global__ __launch_bounds__(kEpiThreads) void modconv_epilogue_channel_kernel(float* __restrict__ d_bias, float* __restrict__ d_strength,
                                                                              const double* __restrict__ plane_sum, int n, int o) {
    __shared__ double red[kEpiThreads];
    for (int c = threadIdx.x; c < o; c += kEpiThreads) {
        double a = 0.0;
        for (int s = 0; s < n; s++) a += plane_sum[((long long)s * o + c) * 3];
        d_bias[c] = (float)a;
    }
    if (d_strength == nullptr) return;
    double a = 0.0;
    for (long long q = threadIdx.x; q < (long long)n * o; q += kEpiThreads) a += plane_sum[q * 3 + 2];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int k = kEpiThreads / 2; k >= 1; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) d_strength[0] = (float)red[0];
}

static int modconv_check(const char* what, int n, int o, int h, int w, int u, double alpha, double gain, double clamp) {
    AFCM_REQUIRE(n > 0 && o > 0 && h > 0 && w > 0, "%s: empty tensor (n %d, o %d, h %d, w %d)", what, n, o, h, w);
    AFCM_REQUIRE(u == 1 || u == 2, "%s: the upsampling factor is 1 or 2, got %d", what, u);
    AFCM_REQUIRE((long long)h * w * u * u < (1LL << 31), "%s: an output plane of %d x %d pixels is beyond 2^31", what, h * u, w * u);
    AFCM_REQUIRE((long long)n * o * cdiv(h * w, kEpiThreads) < (1LL << 31) && (long long)n * o < (1LL << 31),
                 "%s: %d x %d planes of %d x %d pixels are more workgroups than one launch has", what, n, o, h, w);
    AFCM_REQUIRE(alpha == alpha && gain > 0.0 && gain < 1e30 && clamp == clamp, "%s: the gain must be positive and finite, the slope and the clamp no NaN", what);
    return AFCM_OK;
}

static bool aligned_to(const void* ptr, int bytes) { return ((uintptr_t)ptr & (uintptr_t)(bytes - 1)) == 0; }

}  // namespace afcm

using namespace afcm;

extern "C" int64_t afcm_modconv_epilogue_workspace_bytes(int32_t n, int32_t o, int32_t h, int32_t w) {
    if (n <= 0 || o <= 0 || h <= 0 || w <= 0 || (long long)h * w >= (1LL << 31)) return 0;
    return ((int64_t)n * o * cdiv(h * w, kEpiThreads) + (int64_t)n * o) * 3 * (int64_t)sizeof(double);
}

extern "C" int afcm_modconv_epilogue_fwd(float* y, const float* t, const float* dcoefs, const float* bias, const float* noise,
                                         const float* noise_strength, int32_t noise_per_sample, int32_t n, int32_t o, int32_t h, int32_t w,
                                         int32_t u, double alpha, double gain, double clamp, void* stream) {
    const int rc = modconv_check("modconv_epilogue_fwd", n, o, h, w, u, alpha, gain, clamp);
    if (rc != AFCM_OK) return rc;
    AFCM_REQUIRE(y && t && dcoefs && bias, "modconv_epilogue_fwd: y, t, dcoefs and bias must be non-null");
    AFCM_REQUIRE((noise == nullptr) == (noise_strength == nullptr), "modconv_epilogue_fwd: noise and noise_strength come together");
    AFCM_REQUIRE(noise_per_sample == 0 || noise_per_sample == 1, "modconv_epilogue_fwd: noise_per_sample is 0 or 1");
    AFCM_REQUIRE(aligned_to(y, 4 * u) && aligned_to(t, 4) && aligned_to(dcoefs, 4) && aligned_to(bias, 4) && aligned_to(noise, 4) &&
                 aligned_to(noise_strength, 4), "modconv_epilogue_fwd: a misaligned pointer");
    ModconvEpi p = {};
    p.y = y; p.t = t; p.dcoefs = dcoefs; p.bias = bias; p.noise = noise; p.strength = noise_strength;
    p.noise_stride = noise_per_sample ? (long long)h * w * u * u : 0;
    const int v = (w % (4 / u) == 0 && aligned_to(y, 16) && aligned_to(t, 16) && aligned_to(noise, 16)) ? 4 / u : 1;
    p.n = n; p.o = o; p.h = h; p.w = w; p.chunks = cdiv(h * w / v, kEpiThreads);
    p.alpha = alpha; p.gain = gain; p.clamp = clamp >= 0.0 ? (float)clamp : -1.f;
    const dim3 grid((unsigned)((long long)n * o * p.chunks)), block(kEpiThreads);
    hipStream_t st = (hipStream_t)stream;
    if (u == 2 && v == 2) hipLaunchKernelGGL((modconv_epilogue_fwd_kernel<2, 2>), grid, block, 0, st, p);
    else if (u == 2) hipLaunchKernelGGL((modconv_epilogue_fwd_kernel<2, 1>), grid, block, 0, st, p);
    else if (v == 4) hipLaunchKernelGGL((modconv_epilogue_fwd_kernel<1, 4>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((modconv_epilogue_fwd_kernel<1, 1>), grid, block, 0, st, p);
    return hip_status(hipGetLastError());
}

extern "C" int afcm_modconv_epilogue_bwd(float* d_t, float* d_dcoefs, float* d_bias, float* d_noise_strength, double* workspace, const float* dy,
                                         const float* y, const float* t, const float* dcoefs, const float* noise, int32_t noise_per_sample,
                                         int32_t n, int32_t o, int32_t h, int32_t w, int32_t u, double alpha, double gain, double clamp,
                                         void* stream) {
    const int rc = modconv_check("modconv_epilogue_bwd", n, o, h, w, u, alpha, gain, clamp);
    if (rc != AFCM_OK) return rc;
    AFCM_REQUIRE(d_t && d_dcoefs && d_bias && workspace && dy && y && t && dcoefs, "modconv_epilogue_bwd: a null pointer among the required tensors");
    AFCM_REQUIRE((noise == nullptr) == (d_noise_strength == nullptr), "modconv_epilogue_bwd: noise and d_noise_strength come together");
    AFCM_REQUIRE(noise_per_sample == 0 || noise_per_sample == 1, "modconv_epilogue_bwd: noise_per_sample is 0 or 1");
    AFCM_REQUIRE(aligned_to(dy, 4 * u) && aligned_to(y, 4 * u) && aligned_to(workspace, 8) && aligned_to(d_t, 4) && aligned_to(t, 4) &&
                 aligned_to(d_dcoefs, 4) && aligned_to(d_bias, 4) && aligned_to(d_noise_strength, 4) && aligned_to(dcoefs, 4) && aligned_to(noise, 4),
                 "modconv_epilogue_bwd: a misaligned pointer");
    ModconvEpi p = {};
    p.y = d_t; p.t = t; p.dcoefs = dcoefs; p.noise = noise; p.dy = dy; p.ysaved = y; p.part = workspace;
    p.noise_stride = noise_per_sample ? (long long)h * w * u * u : 0;
    const int v = (w % (4 / u) == 0 && aligned_to(dy, 16) && aligned_to(y, 16) && aligned_to(t, 16) && aligned_to(d_t, 16) && aligned_to(noise, 16)) ? 4 / u : 1;
    p.n = n; p.o = o; p.h = h; p.w = w; p.chunks = cdiv(h * w / v, kEpiThreads);
    p.alpha = alpha; p.gain = gain; p.clamp = clamp >= 0.0 ? (float)clamp : -1.f;
    const long long planes = (long long)n * o;
    double* plane_sum = workspace + planes * cdiv(h * w, kEpiThreads) * 3;      // (behind the parts of the element path, the most there can be)
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(planes * p.chunks)), block(kEpiThreads);
    if (u == 2 && v == 2) hipLaunchKernelGGL((modconv_epilogue_bwd_kernel<2, 2>), grid, block, 0, st, p);
    else if (u == 2) hipLaunchKernelGGL((modconv_epilogue_bwd_kernel<2, 1>), grid, block, 0, st, p);
    else if (v == 4) hipLaunchKernelGGL((modconv_epilogue_bwd_kernel<1, 4>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((modconv_epilogue_bwd_kernel<1, 1>), grid, block, 0, st, p);
    hipLaunchKernelGGL(modconv_epilogue_plane_kernel, dim3((unsigned)planes), dim3(64), 0, st, plane_sum, d_dcoefs, (const double*)workspace, p.chunks);
    hipLaunchKernelGGL(modconv_epilogue_channel_kernel, dim3(1), block, 0, st, d_bias, d_noise_strength, (const double*)plane_sum, n, o);
    return hip_status(hipGetLastError());
}
