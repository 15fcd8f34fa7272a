// Validation metrics (util/evaluation.py behind train.py:83-111): one [planes][8] float64 table of per-plane statistics from which the host
// finishes PSNR / SSIM / MAE with the reference's bookkeeping (afcm_amd/evaluation.py, *_from_stats).  See include/afcm_hip.h for the columns.
//
// Three launches on one stream, no host step between them and no atomics:
//   1. plane_extrema_kernel  one workgroup per (plane, 64 x 64 tile): max / min of both images over the tile  -> workspace [plane][tile][4]
//   2. plane_sums_kernel     one workgroup per (plane, tile): the tile + a 6-pixel apron staged in LDS as fp32 (exact for all three dtypes);
//                            the plane's extrema from (1) (max / min: any order gives the same bits); the three per-pixel sums over the
//                            tile's own pixels; the SSIM map over the tile's own window origins by a thread-per-column walk that keeps the
//                            horizontal 7-sums of the last seven rows in registers                        -> workspace [plane][tile][4]
//   3. plane_finish_kernel   one wave per plane sums the tiles' partials in a fixed order                  -> table [plane][8]
// Every sum is taken in an order that depends on the shape only, so a table is bit-identical from call to call.
// After the load (and the optional fp32 unit-range map) every operation is float64: the SSIM variance cancels against c2 = 3.6e-3 on flat
// regions, where fp32 moments lose the digits the keep-best comparison looks at (DESIGN.md "Validation metrics").
//
// Volume SSIM (evaluate_3D's 7 x 7 x 7 window, util/evaluation.py:123-127): afcm_volume_ssim, the plane walk with one stage in front.  Two launches:
//   1. volume_ssim_kernel    one workgroup per (volume, z origin, 16 x 64 tile of window origins): every thread sums the seven z-neighbours of its
//                            voxels (x, y, xx, yy, xy; float64, straight from global memory) into LDS, then the thread-per-column walk of (2)
//                            above over those z-sums                                                       -> workspace [volume][z origin][tile]
//   2. volume_ssim_finish_kernel  one wave per (volume, z origin) sums that layer's partials in a fixed order -> layers [volume][d - 6]
// Every window is a direct sum of its 343 terms (7 along z, then 7 along x, then 7 along y): no running sums, whose rounding grows with depth.
#include "common.h"

namespace afcm {

constexpr int PM_TILE = 64;                 // tile edge in pixels = window origins per tile row = lanes of a wave
constexpr int PM_WIN = 7;
constexpr int PM_APRON = PM_WIN - 1;
constexpr int PM_LDS = PM_TILE + PM_APRON;  // 70 x 70 fp32 per image: 39.2 KB for both
constexpr int PM_THREADS = 256;
constexpr int PM_ROWS_PER_WAVE = PM_TILE / (PM_THREADS / 64);

struct plane_view {
    const void* p;
    long long stride_plane, stride_row, stride_col;
    int dtype;
};

// One element as fp32, optionally mapped from the network's [-1, 1] to [0, 1] (train.py:93-96): add and multiply are separate fp32 roundings
// (the intrinsics are never contracted) and a NaN stays a NaN, as numpy.clip leaves it.
__device__ __forceinline__ float pm_load(const plane_view& v, long long plane, int y, int x, int unit_map) {
    const long long i = plane * v.stride_plane + (long long)y * v.stride_row + (long long)x * v.stride_col;
    float f;
    if (v.dtype == AFCM_F32) f = ((const float*)v.p)[i];
    else if (v.dtype == AFCM_F16) f = (float)((const f16_t*)v.p)[i];
    else f = (float)((const bf16_t*)v.p)[i];
    if (unit_map) {
        f = __fmul_rn(__fadd_rn(f, 1.0f), 0.5f);
        f = f < 0.f ? 0.f : (f > 1.f ? 1.f : f);
    }
    return f;
}

__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}
__device__ __forceinline__ float wave_max(float s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s = fmaxf(s, __shfl_xor(s, o));
    return s;
}
__device__ __forceinline__ float wave_min(float s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s = fminf(s, __shfl_xor(s, o));
    return s;
}

__global__ __launch_bounds__(PM_THREADS) void plane_extrema_kernel(double* __restrict__ ext, plane_view ref, plane_view test, int h, int w,
                                                                   int tiles_x, int tiles, int unit_map) {
    __shared__ float red[4][PM_THREADS / 64];
    const long long plane = blockIdx.x / tiles;
    const int tile = blockIdx.x % tiles;
    const int y0 = (tile / tiles_x) * PM_TILE, x0 = (tile % tiles_x) * PM_TILE;
    const int th = min(PM_TILE, h - y0), tw = min(PM_TILE, w - x0);
    float rmax = -INFINITY, rmin = INFINITY, tmax = -INFINITY, tmin = INFINITY;
    for (int i = threadIdx.x; i < th * PM_TILE; i += PM_THREADS) {
        const int y = i / PM_TILE, x = i % PM_TILE;
        if (x < tw) {
            const float r = pm_load(ref, plane, y0 + y, x0 + x, unit_map), t = pm_load(test, plane, y0 + y, x0 + x, unit_map);
            rmax = fmaxf(rmax, r); rmin = fminf(rmin, r);
            tmax = fmaxf(tmax, t); tmin = fminf(tmin, t);
        }
    }
    rmax = wave_max(rmax); rmin = wave_min(rmin); tmax = wave_max(tmax); tmin = wave_min(tmin);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][wave] = rmax; red[1][wave] = rmin; red[2][wave] = tmax; red[3][wave] = tmin; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const float* q = red[threadIdx.x];
        const bool mx = (threadIdx.x & 1) == 0;
        float v = q[0];
        for (int k = 1; k < PM_THREADS / 64; ++k) v = mx ? fmaxf(v, q[k]) : fminf(v, q[k]);
        ext[(long long)blockIdx.x * 4 + threadIdx.x] = (double)v;
    }
}

__global__ __launch_bounds__(PM_THREADS) void plane_sums_kernel(double* __restrict__ sums, const double* __restrict__ ext, plane_view ref,
                                                                plane_view test, int h, int w, int tiles_x, int tiles, int unit_map, double c1,
                                                                double c2) {
    __shared__ float lr[PM_LDS][PM_LDS], lt[PM_LDS][PM_LDS];
    __shared__ double red[4][PM_THREADS / 64];
    __shared__ double peak[2];
    const long long plane = blockIdx.x / tiles;
    const int tile = blockIdx.x % tiles;
    const int y0 = (tile / tiles_x) * PM_TILE, x0 = (tile % tiles_x) * PM_TILE;
    const int th = min(PM_TILE, h - y0), tw = min(PM_TILE, w - x0);            // the tile's own pixels
    const int lh = min(PM_LDS, h - y0), lw = min(PM_LDS, w - x0);              // with the apron, inside the image
    for (int i = threadIdx.x; i < lh * PM_LDS; i += PM_THREADS) {
        const int y = i / PM_LDS, x = i % PM_LDS;
        const bool in = x < lw;
        lr[y][x] = in ? pm_load(ref, plane, y0 + y, x0 + x, unit_map) : 0.f;
        lt[y][x] = in ? pm_load(test, plane, y0 + y, x0 + x, unit_map) : 0.f;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave == 0) {                                                           // the plane's maxima from phase 1's tiles
        float rmax = -INFINITY, tmax = -INFINITY;
        const double* e = ext + plane * tiles * 4;
        for (int k = lane; k < tiles; k += 64) { rmax = fmaxf(rmax, (float)e[k * 4 + 0]); tmax = fmaxf(tmax, (float)e[k * 4 + 2]); }
        rmax = wave_max(rmax); tmax = wave_max(tmax);
        if (lane == 0) { peak[0] = (double)rmax; peak[1] = (double)tmax; }
    }
    __syncthreads();

    // columns 4-6 over the tile's own pixels
    const double rpeak = peak[0], tpeak = peak[1];
    double s_sq = 0.0, s_nsq = 0.0, s_abs = 0.0, s_ssim = 0.0;
    for (int i = threadIdx.x; i < th * PM_TILE; i += PM_THREADS) {
        const int y = i / PM_TILE, x = i % PM_TILE;
        if (x < tw) {
            const double r = (double)lr[y][x], t = (double)lt[y][x];
            const double d = r - t, dn = r / rpeak - t / tpeak;                // IEEE divides, as numpy's l / l.max(); a zero peak gives inf / nan
            s_sq += d * d; s_nsq += dn * dn; s_abs += __builtin_fabs(d);
        }
    }

    // column 7: this wave's 16 rows of window origins, lane = column.  hs[k] holds the horizontal 7-sums (x, y, xx, yy, xy) of one staged row;
    // the loop is unrolled by 7 so that the ring's slot is a compile-time index (registers, no scratch).
    const int oy0 = wave * PM_ROWS_PER_WAVE;
    const int nwy = min(th, h - PM_APRON - y0), nwx = min(tw, w - PM_APRON - x0);      // window origins this tile owns (may be <= 0)
    if (oy0 < nwy && nwx > 0) {
        double hs[PM_WIN][5];
        const int rows = min(PM_ROWS_PER_WAVE, nwy - oy0) + PM_APRON;                  // staged rows this wave walks: all inside lh
        const bool col_ok = lane < nwx;
        for (int base = 0; base < rows; base += PM_WIN) {
#pragma unroll
            for (int k = 0; k < PM_WIN; ++k) {
                const int rr = base + k;
                if (rr < rows) {
                    double ax = 0.0, ay = 0.0, axx = 0.0, ayy = 0.0, axy = 0.0;
                    if (col_ok) {
#pragma unroll
                        for (int j = 0; j < PM_WIN; ++j) {
                            const double x = (double)lr[oy0 + rr][lane + j], y = (double)lt[oy0 + rr][lane + j];
                            ax += x; ay += y; axx += x * x; ayy += y * y; axy += x * y;
                        }
                    }
                    hs[k][0] = ax; hs[k][1] = ay; hs[k][2] = axx; hs[k][3] = ayy; hs[k][4] = axy;
                    if (rr >= PM_APRON && col_ok) {
                        double v[5];
#pragma unroll
                        for (int q = 0; q < 5; ++q) {
                            double a = hs[0][q];
#pragma unroll
                            for (int m = 1; m < PM_WIN; ++m) a += hs[m][q];
                            v[q] = a / 49.0;
                        }
                        const double ux = v[0], uy = v[1];
                        const double cov = 49.0 / 48.0;                                // sample covariance
                        const double vx = cov * (v[2] - ux * ux), vy = cov * (v[3] - uy * uy), vxy = cov * (v[4] - ux * uy);
                        s_ssim += ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
                    }
                }
            }
        }
    }

    s_sq = wave_sum(s_sq); s_nsq = wave_sum(s_nsq); s_abs = wave_sum(s_abs); s_ssim = wave_sum(s_ssim);
    if (lane == 0) { red[0][wave] = s_sq; red[1][wave] = s_nsq; red[2][wave] = s_abs; red[3][wave] = s_ssim; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const double* q = red[threadIdx.x];
        sums[(long long)blockIdx.x * 4 + threadIdx.x] = ((q[0] + q[1]) + q[2]) + q[3];
    }
}

__global__ __launch_bounds__(64) void plane_finish_kernel(double* __restrict__ table, const double* __restrict__ ext, const double* __restrict__ sums,
                                                          int tiles) {
    const long long plane = blockIdx.x;
    const int lane = threadIdx.x;
    const double* e = ext + plane * tiles * 4;
    const double* s = sums + plane * tiles * 4;
    float rmax = -INFINITY, rmin = INFINITY, tmax = -INFINITY, tmin = INFINITY;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = lane; k < tiles; k += 64) {
        rmax = fmaxf(rmax, (float)e[k * 4 + 0]); rmin = fminf(rmin, (float)e[k * 4 + 1]);
        tmax = fmaxf(tmax, (float)e[k * 4 + 2]); tmin = fminf(tmin, (float)e[k * 4 + 3]);
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] += s[k * 4 + q];
    }
    rmax = wave_max(rmax); rmin = wave_min(rmin); tmax = wave_max(tmax); tmin = wave_min(tmin);
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = wave_sum(a[q]);
    if (lane == 0) {
        double* row = table + plane * 8;
        row[0] = (double)rmax; row[1] = (double)rmin; row[2] = (double)tmax; row[3] = (double)tmin;
        row[4] = a[0]; row[5] = a[1]; row[6] = a[2]; row[7] = a[3];
    }
}

// ---- volume SSIM: 7 x 7 x 7 window ------------------------------------------------------------------------------------------------------------
constexpr int VS_TILE_Y = 16, VS_TILE_X = 64;           // window origins per tile: rows x columns (columns = lanes of a wave)
constexpr int VS_LDS_Y = VS_TILE_Y + PM_APRON, VS_LDS_X = VS_TILE_X + PM_APRON;     // 5 x 22 x 70 float64 z-sums: 61.6 KB, two workgroups per CU
constexpr int VS_ROWS_PER_WAVE = VS_TILE_Y / (PM_THREADS / 64);
constexpr double VS_NPIX = 343.0;

// A volume as pm_load reads it: `planes` has a plane stride of ONE element, so the "plane" handed to pm_load is the 64-bit element offset of
// voxel (volume, z, 0, 0) itself, which lets the volume and z strides be arbitrary and pm_load stay as it is.
struct volume_view {
    plane_view planes;
    long long stride_volume, stride_z;
};

__global__ __launch_bounds__(PM_THREADS) void volume_ssim_kernel(double* __restrict__ partials, volume_view ref, volume_view test, int layers, int h,
                                                                 int w, int tiles_x, int tiles, int unit_map, double c1, double c2) {
    __shared__ double zs[5][VS_LDS_Y][VS_LDS_X];
    __shared__ double red[PM_THREADS / 64];
    const long long layer = blockIdx.x / tiles;                                        // volume * layers + z origin
    const int tile = blockIdx.x % tiles;
    const long long volume = layer / layers;
    const int z0 = (int)(layer % layers);
    const int y0 = (tile / tiles_x) * VS_TILE_Y, x0 = (tile % tiles_x) * VS_TILE_X;
    const int nwy = min(VS_TILE_Y, h - PM_APRON - y0), nwx = min(VS_TILE_X, w - PM_APRON - x0);    // window origins this tile owns: >= 1 each
    const int lh = nwy + PM_APRON, lw = nwx + PM_APRON;                                // the voxels under them: all inside the volume
    const long long rbase = volume * ref.stride_volume + z0 * ref.stride_z, tbase = volume * test.stride_volume + z0 * test.stride_z;

    // stage A: the seven z-neighbours of every staged voxel, consecutive lanes along x
    for (int i = threadIdx.x; i < lh * VS_LDS_X; i += PM_THREADS) {
        const int y = i / VS_LDS_X, x = i % VS_LDS_X;
        double ax = 0.0, ay = 0.0, axx = 0.0, ayy = 0.0, axy = 0.0;
        if (x < lw) {
#pragma unroll
            for (int k = 0; k < PM_WIN; ++k) {
                const double r = (double)pm_load(ref.planes, rbase + k * ref.stride_z, y0 + y, x0 + x, unit_map);
                const double t = (double)pm_load(test.planes, tbase + k * test.stride_z, y0 + y, x0 + x, unit_map);
                ax += r; ay += t; axx += r * r; ayy += t * t; axy += r * t;
            }
        }
        zs[0][y][x] = ax; zs[1][y][x] = ay; zs[2][y][x] = axx; zs[3][y][x] = ayy; zs[4][y][x] = axy;
    }
    __syncthreads();

    // stage B: plane_sums_kernel's column walk over the z-sums -- this wave's rows of window origins, lane = column
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int oy0 = wave * VS_ROWS_PER_WAVE;
    double s_ssim = 0.0;
    if (oy0 < nwy && lane < nwx) {
        double hs[PM_WIN][5];
        const int rows = min(VS_ROWS_PER_WAVE, nwy - oy0) + PM_APRON;                  // staged rows this wave walks: all inside lh
        for (int base = 0; base < rows; base += PM_WIN) {
#pragma unroll
            for (int k = 0; k < PM_WIN; ++k) {
                const int rr = base + k;
                if (rr < rows) {
#pragma unroll
                    for (int q = 0; q < 5; ++q) {
                        double a = zs[q][oy0 + rr][lane];
#pragma unroll
                        for (int j = 1; j < PM_WIN; ++j) a += zs[q][oy0 + rr][lane + j];
                        hs[k][q] = a;
                    }
                    if (rr >= PM_APRON) {
                        double v[5];
#pragma unroll
                        for (int q = 0; q < 5; ++q) {
                            double a = hs[0][q];
#pragma unroll
                            for (int m = 1; m < PM_WIN; ++m) a += hs[m][q];
                            v[q] = a / VS_NPIX;
                        }
                        const double ux = v[0], uy = v[1];
                        const double cov = VS_NPIX / (VS_NPIX - 1.0);                  // sample covariance
                        const double vx = cov * (v[2] - ux * ux), vy = cov * (v[3] - uy * uy), vxy = cov * (v[4] - ux * uy);
                        s_ssim += ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
                    }
                }
            }
        }
    }
    s_ssim = wave_sum(s_ssim);
    if (lane == 0) red[wave] = s_ssim;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(64) void volume_ssim_finish_kernel(double* __restrict__ out, const double* __restrict__ partials, int tiles) {
    const double* p = partials + (long long)blockIdx.x * tiles;
    double a = 0.0;
    for (int k = threadIdx.x; k < tiles; k += 64) a += p[k];
    a = wave_sum(a);
    if (threadIdx.x == 0) out[blockIdx.x] = a;
}

static inline long long pm_tiles(int h, int w) { return (long long)cdiv(h, PM_TILE) * cdiv(w, PM_TILE); }
static inline long long vs_tiles(int h, int w) { return (long long)cdiv(h - PM_APRON, VS_TILE_Y) * cdiv(w - PM_APRON, VS_TILE_X); }

}  // namespace afcm

extern "C" int64_t afcm_plane_metrics_workspace_bytes(int64_t planes, int32_t h, int32_t w) {
    if (planes <= 0 || h <= 0 || w <= 0) return 0;
    return planes * afcm::pm_tiles(h, w) * 8 * (int64_t)sizeof(double);       // [plane][tile][4] extrema + [plane][tile][4] sums
}

extern "C" int afcm_plane_metrics(double* table, const void* ref, const void* test, int32_t dtype_ref, int32_t dtype_test, int64_t planes, int32_t h,
                                  int32_t w, int64_t ref_stride_plane, int64_t ref_stride_row, int64_t ref_stride_col, int64_t test_stride_plane,
                                  int64_t test_stride_row, int64_t test_stride_col, int32_t unit_map, double c1, double c2, void* workspace,
                                  void* stream) {
    using namespace afcm;
    AFCM_REQUIRE(table != nullptr && ref != nullptr && test != nullptr && workspace != nullptr, "plane_metrics: null table, image or workspace");
    AFCM_REQUIRE(dtype_ref >= AFCM_F32 && dtype_ref <= AFCM_BF16 && dtype_test >= AFCM_F32 && dtype_test <= AFCM_BF16,
                 "plane_metrics: dtypes %d / %d are not AFCM_F32 / AFCM_F16 / AFCM_BF16", dtype_ref, dtype_test);
    AFCM_REQUIRE(planes > 0, "plane_metrics: %lld planes", (long long)planes);
    AFCM_REQUIRE(h >= PM_WIN && w >= PM_WIN, "plane_metrics: a %d x %d plane is smaller than the 7 x 7 SSIM window", h, w);
    const long long tiles = pm_tiles(h, w), blocks = planes * tiles;
    AFCM_REQUIRE(blocks < (1ll << 31), "plane_metrics: %lld planes of %lld tiles exceed the grid", (long long)planes, tiles);
    const plane_view r = {ref, ref_stride_plane, ref_stride_row, ref_stride_col, dtype_ref};
    const plane_view t = {test, test_stride_plane, test_stride_row, test_stride_col, dtype_test};
    double* ext = (double*)workspace;
    double* sums = ext + blocks * 4;
    const int tiles_x = cdiv(w, PM_TILE);
    hipLaunchKernelGGL(plane_extrema_kernel, dim3((unsigned)blocks), dim3(PM_THREADS), 0, (hipStream_t)stream, ext, r, t, h, w, tiles_x, (int)tiles,
                       unit_map);
    hipLaunchKernelGGL(plane_sums_kernel, dim3((unsigned)blocks), dim3(PM_THREADS), 0, (hipStream_t)stream, sums, (const double*)ext, r, t, h, w,
                       tiles_x, (int)tiles, unit_map, c1, c2);
    hipLaunchKernelGGL(plane_finish_kernel, dim3((unsigned)planes), dim3(64), 0, (hipStream_t)stream, table, (const double*)ext, (const double*)sums,
                       (int)tiles);
    return hip_status(hipGetLastError());
}

extern "C" int64_t afcm_volume_ssim_workspace_bytes(int64_t volumes, int32_t d, int32_t h, int32_t w) {
    if (volumes <= 0 || d < afcm::PM_WIN || h < afcm::PM_WIN || w < afcm::PM_WIN) return 0;
    return volumes * (d - afcm::PM_APRON) * afcm::vs_tiles(h, w) * (int64_t)sizeof(double);       // [volume][z origin][tile]
}

extern "C" int afcm_volume_ssim(double* layers, const void* ref, const void* test, int32_t dtype_ref, int32_t dtype_test, int64_t volumes, int32_t d,
                                int32_t h, int32_t w, int64_t ref_stride_volume, int64_t ref_stride_z, int64_t ref_stride_y, int64_t ref_stride_x,
                                int64_t test_stride_volume, int64_t test_stride_z, int64_t test_stride_y, int64_t test_stride_x, int32_t unit_map,
                                double c1, double c2, void* workspace, void* stream) {
    using namespace afcm;
    AFCM_REQUIRE(volumes > 0, "volume_ssim: %lld volumes", (long long)volumes);
    AFCM_REQUIRE(d >= PM_WIN && h >= PM_WIN && w >= PM_WIN, "volume_ssim: a %d x %d x %d volume is smaller than the 7 x 7 x 7 SSIM window", d, h, w);
    AFCM_REQUIRE(layers != nullptr && ref != nullptr && test != nullptr && workspace != nullptr, "volume_ssim: null layers, volume or workspace");
    AFCM_REQUIRE(dtype_ref >= AFCM_F32 && dtype_ref <= AFCM_BF16 && dtype_test >= AFCM_F32 && dtype_test <= AFCM_BF16,
                 "volume_ssim: dtypes %d / %d are not AFCM_F32 / AFCM_F16 / AFCM_BF16", dtype_ref, dtype_test);
    const long long tiles = vs_tiles(h, w), nlayers = volumes * (d - PM_APRON);
    AFCM_REQUIRE(volumes < (1ll << 31) && nlayers < (1ll << 31) && nlayers * tiles < (1ll << 31),
                 "volume_ssim: %lld volumes of %d layers of %lld tiles exceed the grid", (long long)volumes, d - PM_APRON, tiles);
    const volume_view r = {{ref, 1, ref_stride_y, ref_stride_x, dtype_ref}, ref_stride_volume, ref_stride_z};
    const volume_view t = {{test, 1, test_stride_y, test_stride_x, dtype_test}, test_stride_volume, test_stride_z};
    double* partials = (double*)workspace;
    hipLaunchKernelGGL(volume_ssim_kernel, dim3((unsigned)(nlayers * tiles)), dim3(PM_THREADS), 0, (hipStream_t)stream, partials, r, t,
                       d - PM_APRON, h, w, cdiv(w - PM_APRON, VS_TILE_X), (int)tiles,
                       unit_map, c1, c2);
    hipLaunchKernelGGL(volume_ssim_finish_kernel, dim3((unsigned)nlayers), dim3(64), 0, (hipStream_t)stream, layers, (const double*)partials,
                       (int)tiles);
    return hip_status(hipGetLastError());
}
