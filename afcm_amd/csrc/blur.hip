// The loss-side Gaussian blur (models/stylegan3_model.py:24-30, 97-103) with sigma read on the DEVICE: f = exp2(-(i / sigma)^2) for i in [-r, r],
// r = floor(3 sigma), normalised by its sum, applied along x and then along y with zero padding r (upfirdn2d.filter2d with a 1-D filter).  fp32
// planes [planes][h][w].  Sigma and radius come from the schedule block (schedule.hip) or, without one, from the launch; the grid depends on neither,
// so a captured pair of launches stays valid while sigma fades.
//   gauss_rows_kernel   x -> tmp, along x.  A workgroup owns ROWS_TH rows x ROWS_TW columns; the rows lie in LDS shifted by r, so that a thread's four
//                       consecutive outputs read 16-byte aligned windows: per four taps one ds_read_b128 of the row and one (broadcast) of the taps
//                       for 16 FMAs.  Radius 0 and an invalid radius: nothing to do, gauss_cols_kernel does not read tmp then.
//   gauss_cols_kernel   tmp -> y, along y.  A workgroup owns COLS_TH rows x 64 columns; a thread owns one column and COLS_RY consecutive rows: per tap
//                       one ds_read_b32 (lanes on consecutive banks) for COLS_RY FMAs.  Radius 0: y = x, a copy without arithmetic (nothing is divided by
//                       sigma).  A radius outside [0, AFCM_BLUR_RMAX] cannot be raised from the device: every output is NaN.
// Zero padding is a range decision in the tile fill: nothing outside the plane is loaded, and a tap only ever multiplies an element of its own window
// (no zero taps), so a NaN input spreads to its (2r + 1)^2 window and no further.  Every output sums its taps in ascending order with fused
// multiply-adds: no atomics, reproducible.
#include "common.h"

#ifndef AFCM_BLUR_RMAX
#define AFCM_BLUR_RMAX 32
#endif

namespace afcm {

constexpr int kBlurTaps = 2 * AFCM_BLUR_RMAX + 1;
constexpr int kBlurTapsPad = round_up(kBlurTaps + 3, 4);                       // the tail group reads a whole float4 of taps
constexpr int ROWS_TW = 256, ROWS_TH = 4;                                      // gauss_rows_kernel: 64 lanes x 4 outputs, one wave per row
constexpr int ROWS_LD = ROWS_TW + 2 * AFCM_BLUR_RMAX + 16;                     // the last window read ends at 252 + 4 * (kBlurTaps / 4) + 8 + 3
constexpr int COLS_TW = 64, COLS_RY = 16, COLS_TH = 4 * COLS_RY;               // gauss_cols_kernel: one lane per column, 16 rows per lane, 4 waves
constexpr int COLS_ROWS = COLS_TH + 2 * AFCM_BLUR_RMAX + 4;                    // the last window read is row 48 + 4 * (kBlurTaps / 4) + 3 + 15
static_assert(AFCM_BLUR_RMAX >= 30 && AFCM_BLUR_RMAX % 4 == 0, "the shipped schedules start at sigma 10 (radius 30)");
static_assert(252 + 4 * (kBlurTaps / 4) + 8 + 3 < ROWS_LD && 48 + 4 * (kBlurTaps / 4) + 3 + 15 < COLS_ROWS, "window reads stay inside the tile");

// sigma and radius of this launch; radius -1: invalid (only a block can hold one, the host entry refuses its own)
__device__ __forceinline__ int blur_radius(const double* __restrict__ block, double sigma_arg, int radius_arg, float& sigma) {
    if (block == nullptr) {
        sigma = (float)sigma_arg;
        return radius_arg;
    }
    sigma = (float)block[1];
    const double r = block[2];
    return (r >= 0.0 && r <= (double)AFCM_BLUR_RMAX) ? (int)r : -1;
}

// the normalised taps in fp32 as the reference forms them: arange(-r, r + 1).div(sigma).square().neg().exp2(), then f / f.sum()
__device__ __forceinline__ void blur_taps(float* __restrict__ raw, float* __restrict__ taps, int r, float sigma) {
    const int t = threadIdx.x;
    if (t < kBlurTapsPad) {
        const float q = (float)(t - r) / sigma;
        raw[t] = t <= 2 * r ? exp2f(-(q * q)) : 0.f;
    }
    __syncthreads();
    if (t < kBlurTapsPad) {
        float sum = 0.f;
        for (int i = 0; i <= 2 * r; ++i) sum += raw[i];
        taps[t] = t <= 2 * r ? raw[t] / sum : 0.f;
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void gauss_rows_kernel(float* __restrict__ out, const float* __restrict__ in, int h, int w, int tiles_x, int tiles_y,
                                                         double sigma_arg, int radius_arg, const double* __restrict__ block) {
    __shared__ __attribute__((aligned(16))) float tile[ROWS_TH * ROWS_LD];
    __shared__ __attribute__((aligned(16))) float taps[kBlurTapsPad];
    __shared__ float raw[kBlurTapsPad];
    float sigma;
    const int r = blur_radius(block, sigma_arg, radius_arg, sigma);
    if (r <= 0) return;
    int b = blockIdx.x;
    const int tx0 = (b % tiles_x) * ROWS_TW;
    b /= tiles_x;
    const int ty0 = (b % tiles_y) * ROWS_TH;
    const long long plane = (long long)(b / tiles_y) * h * w;

    // tile[row][c] = in[ty0 + row][tx0 - r + c], zero outside the plane and past the columns this radius needs
    for (int e = threadIdx.x; e < ROWS_TH * ROWS_LD; e += 256) {
        const int row = e / ROWS_LD, c = e - row * ROWS_LD;
        const int gx = tx0 - r + c, gy = ty0 + row;
        const bool inside = c < ROWS_TW + 2 * r && gx >= 0 && gx < w && gy < h;
        tile[e] = inside ? in[plane + (long long)gy * w + gx] : 0.f;
    }
    blur_taps(raw, taps, r, sigma);

    const int row = threadIdx.x >> 6, x0 = (threadIdx.x & 63) * 4;
    const float* t = tile + row * ROWS_LD + x0;
    float win[8], acc[4] = {0.f, 0.f, 0.f, 0.f};
    *(float4*)&win[0] = *(const float4*)t;
    *(float4*)&win[4] = *(const float4*)(t + 4);
    const int ntaps = 2 * r + 1, full = ntaps >> 2;
    int j = 0;
    for (int g = 0; g < full; ++g, j += 4) {
        const float4 f = *(const float4*)(taps + j);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            acc[k] = __builtin_fmaf(f.x, win[k], acc[k]);
            acc[k] = __builtin_fmaf(f.y, win[k + 1], acc[k]);
            acc[k] = __builtin_fmaf(f.z, win[k + 2], acc[k]);
            acc[k] = __builtin_fmaf(f.w, win[k + 3], acc[k]);
        }
        *(float4*)&win[0] = *(float4*)&win[4];
        *(float4*)&win[4] = *(const float4*)(t + j + 8);
    }
    {   // 2r + 1 is odd: one or three taps remain; a tap past the last one is skipped, never multiplied by zero
        const float4 f = *(const float4*)(taps + j);
        const int rem = ntaps & 3;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            acc[k] = __builtin_fmaf(f.x, win[k], acc[k]);
            if (rem == 3) {
                acc[k] = __builtin_fmaf(f.y, win[k + 1], acc[k]);
                acc[k] = __builtin_fmaf(f.z, win[k + 2], acc[k]);
            }
        }
    }
    const int gx = tx0 + x0, gy = ty0 + row;
    if (gy >= h) return;
    float* o = out + plane + (long long)gy * w + gx;
    if (gx + 4 <= w && ((uintptr_t)o & 15) == 0) {
        *(float4*)o = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (gx + k < w) o[k] = acc[k];
    }
}

__global__ __launch_bounds__(256) void gauss_cols_kernel(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ tmp, int h, int w,
                                                         int tiles_x, int tiles_y, double sigma_arg, int radius_arg, const double* __restrict__ block) {
    __shared__ float tile[COLS_ROWS * COLS_TW];
    __shared__ __attribute__((aligned(16))) float taps[kBlurTapsPad];
    __shared__ float raw[kBlurTapsPad];
    float sigma;
    const int r = blur_radius(block, sigma_arg, radius_arg, sigma);
    int b = blockIdx.x;
    const int tx0 = (b % tiles_x) * COLS_TW;
    b /= tiles_x;
    const int ty0 = (b % tiles_y) * COLS_TH;
    const long long plane = (long long)(b / tiles_y) * h * w;
    const int col = threadIdx.x & 63, y0 = (threadIdx.x >> 6) * COLS_RY;
    const int gx = tx0 + col;

    if (r <= 0) {                                                              // radius 0: the copy; invalid: NaN
        if (gx >= w) return;
        for (int k = 0; k < COLS_RY; ++k) {
            const int gy = ty0 + y0 + k;
            if (gy >= h) return;
            const long long at = plane + (long long)gy * w + gx;
            out[at] = r == 0 ? x[at] : __builtin_nanf("");
        }
        return;
    }

    // tile[c][col] = tmp[ty0 - r + c][tx0 + col], zero outside the plane and past the rows this radius needs
    for (int e = threadIdx.x; e < COLS_ROWS * COLS_TW; e += 256) {
        const int c = e >> 6, lx = e & 63;
        const int gy = ty0 - r + c;
        const bool inside = c < COLS_TH + 2 * r && gy >= 0 && gy < h && tx0 + lx < w;
        tile[e] = inside ? tmp[plane + (long long)gy * w + tx0 + lx] : 0.f;
    }
    blur_taps(raw, taps, r, sigma);

    const float* t = tile + y0 * COLS_TW + col;
    float win[COLS_RY + 3], acc[COLS_RY];
#pragma unroll
    for (int k = 0; k < COLS_RY; ++k) acc[k] = 0.f;
#pragma unroll
    for (int k = 0; k < COLS_RY + 3; ++k) win[k] = t[k * COLS_TW];
    const int ntaps = 2 * r + 1, full = ntaps >> 2;
    int j = 0;
    for (int g = 0; g < full; ++g, j += 4) {
        const float4 f = *(const float4*)(taps + j);
#pragma unroll
        for (int k = 0; k < COLS_RY; ++k) {
            acc[k] = __builtin_fmaf(f.x, win[k], acc[k]);
            acc[k] = __builtin_fmaf(f.y, win[k + 1], acc[k]);
            acc[k] = __builtin_fmaf(f.z, win[k + 2], acc[k]);
            acc[k] = __builtin_fmaf(f.w, win[k + 3], acc[k]);
        }
#pragma unroll
        for (int k = 0; k < COLS_RY - 1; ++k) win[k] = win[k + 4];
#pragma unroll
        for (int k = COLS_RY - 1; k < COLS_RY + 3; ++k) win[k] = t[(j + 4 + k) * COLS_TW];
    }
    {
        const float4 f = *(const float4*)(taps + j);
        const int rem = ntaps & 3;
#pragma unroll
        for (int k = 0; k < COLS_RY; ++k) {
            acc[k] = __builtin_fmaf(f.x, win[k], acc[k]);
            if (rem == 3) {
                acc[k] = __builtin_fmaf(f.y, win[k + 1], acc[k]);
                acc[k] = __builtin_fmaf(f.z, win[k + 2], acc[k]);
            }
        }
    }
    if (gx >= w) return;
#pragma unroll
    for (int k = 0; k < COLS_RY; ++k) {
        const int gy = ty0 + y0 + k;
        if (gy < h) out[plane + (long long)gy * w + gx] = acc[k];
    }
}

}  // namespace afcm

extern "C" int32_t afcm_gauss_blur_rmax(void) { return AFCM_BLUR_RMAX; }

extern "C" int afcm_gauss_blur(float* y, const float* x, float* tmp, int64_t planes, int32_t h, int32_t w, double sigma, const double* block, void* stream) {
    using namespace afcm;
    AFCM_REQUIRE(y != nullptr && x != nullptr && y != x, "gauss_blur: null output or input, or the output is the input");
    AFCM_REQUIRE(planes > 0 && h > 0 && w > 0, "gauss_blur: %lld planes of [%d, %d]: every extent must be positive", (long long)planes, h, w);
    int radius = 0;
    if (block == nullptr) {
        AFCM_REQUIRE(sigma >= 0.0 && sigma * 3.0 < (double)(AFCM_BLUR_RMAX + 1), "gauss_blur: sigma %g is negative, not a number, or its radius floor(3 sigma) exceeds %d",
                     sigma, AFCM_BLUR_RMAX);
        radius = (int)(sigma * 3.0);                                            // floor: the product is not negative
    }
    // the scratch is what the row pass writes: needed unless the host knows that the radius is 0
    AFCM_REQUIRE((block == nullptr && radius == 0) || (tmp != nullptr && tmp != x && tmp != y), "gauss_blur: null scratch, or the scratch is the input or the output");
    const int rows_x = cdiv(w, ROWS_TW), rows_y = cdiv(h, ROWS_TH), cols_x = cdiv(w, COLS_TW), cols_y = cdiv(h, COLS_TH);
    const double most = (double)planes * rows_x * rows_y;                      // the larger of the two grids: COLS_TW * COLS_TH >= ROWS_TW * ROWS_TH
    AFCM_REQUIRE(most < 2147483647.0 && (double)planes * cols_x * cols_y < 2147483647.0, "gauss_blur: %.0f workgroups exceed the grid", most);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gauss_rows_kernel, dim3((unsigned)(planes * rows_x * rows_y)), dim3(256), 0, s, tmp, x, h, w, rows_x, rows_y, sigma, radius, block);
    hipLaunchKernelGGL(gauss_cols_kernel, dim3((unsigned)(planes * cols_x * cols_y)), dim3(256), 0, s, y, x, (const float*)tmp, h, w, cols_x, cols_y, sigma,
                       radius, block);
    return hip_status(hipGetLastError());
}
