// Training batches with an elastic deformation on the device: the reference's ElasticDeformation (data/augment/transforms.py:138-191) for the
// [1, h, w] planes of a loader item, after the geometric transforms and before the intensity ones.  Which items execute is known only on the
// device (the table is read through the cursor of a replayed graph), so the launches are fixed per batch and each exits early, per item, where
// the item's flag is 0:
//   elastic_meta_kernel        one thread per item: every table row of the item checked once; status (0 as it is, 1 deform, 2 NaN), alpha, key
//   launch_batch (batch.hip)   the item without the elastic and intensity tables into a float32 scratch: the existing assembly kernels
//   elastic_field_kernel       Fy, Fx: standard normals from Philox counters (x >> 2, y, 0, 1 | 2), float64
//   elastic_smooth_kernel      G_h F, then alpha (G_h F) G_w^T: a 16 x 64 output tile per workgroup, operator rows staged in LDS, float64
//                              multiply and add apart, the sum over m ascending
//   elastic_prefilter_y / _x   order 3: the cubic B-spline coefficients of every plane, one lane per line (rows through an LDS transpose)
//   elastic_gather_kernel      the interpolating read at (y + dy, x + dx), the intensity row where one is given, one store of 4 pixels
// No atomics: every sum has one fixed order, so a batch has the same bits from call to call and the bits of afcm_amd/augment_elastic.py.
// See include/afcm_hip.h for the statement.
#include "batch_common.h"

namespace afcm {

struct elastic_meta {
    int status;                                                                // 0: the item as it is; 1: deformed; 2: an invalid row somewhere: NaN
    unsigned key_lo, key_hi;
    int pad;
    double alpha;
    long long row;                                                             // the item's table row, inside [0, n_items) unless status is 2
};
static_assert(sizeof(elastic_meta) == 32, "one meta record is 32 bytes of the workspace");

constexpr int ELASTIC_ROW = 4;
constexpr double SPLINE_Z = -0.2679491924311227;                               // sqrt(3) - 2, the pole of the cubic B-spline
constexpr double SPLINE_LAST = SPLINE_Z / (SPLINE_Z - 1.0);
constexpr int SPLINE_HORIZON = 40;                                             // |z|^40 = 1.3e-23
constexpr double COORD_MAX = 1073741824.0;                                     // 2^30

__global__ void elastic_meta_kernel(elastic_meta* __restrict__ meta, long long pool_elems, const long long* __restrict__ vols, int n_vols,
                                    const int* __restrict__ items, int n_items, const double* __restrict__ augment,
                                    const double* __restrict__ intensity, const double* __restrict__ elastic, const long long* __restrict__ cursor,
                                    int first, int count, int k, int h, int w) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const batch_item it = item_of(i, pool_elems, vols, n_vols, items, n_items, cursor, first, k);
    elastic_meta m = {2, 0u, 0u, 0, 0.0, 0};
    if (it.valid) {                                                            // the item row's own r: inside [0, n_items) of every table
        bool valid = true;
        if (augment != nullptr) valid = augment_row_of(augment + it.row * 8, h, w).valid;
        if (intensity != nullptr) valid = valid && intensity_row_of(intensity + it.row * INTENSITY_ROW).valid;
        const double* __restrict__ p = elastic + it.row * ELASTIC_ROW;
        const double flag = p[0], alpha = p[1], k0 = p[2], k1 = p[3];
        // every comparison is false for a NaN
        valid = valid && (flag == 0.0 || flag == 1.0) && fabs(alpha) <= 1048576.0 && whole_in(k0, 4294967295.0) && whole_in(k1, 4294967295.0);
        if (valid) m = {flag == 1.0 ? 1 : 0, (unsigned)k0, (unsigned)k1, 0, alpha, it.row};
    }
    meta[i] = m;
}

// field [count][2][h][w]: pixel (y, x) of Fy (f = 0) and Fx (f = 1) is lane x & 3 of Philox(counter (x >> 2, y, 0, 1 + f), key of the row)
__global__ __launch_bounds__(VOL_THREADS) void elastic_field_kernel(const elastic_meta* __restrict__ meta, double* __restrict__ field, int h, int w,
                                                                    int groups, long long total) {
    const long long e = (long long)blockIdx.x * VOL_THREADS + threadIdx.x;
    if (e >= total) return;
    const int x0 = (int)(e % groups) * 4;
    long long r = e / groups;
    const int y = (int)(r % h);
    r /= h;                                                                    // item * 2 + f
    const elastic_meta mt = meta[r >> 1];
    if (mt.status != 1) return;
    const philox_words p = philox4x32((unsigned)(x0 >> 2), (unsigned)y, 0u, 1u + (unsigned)(r & 1), mt.key_lo, mt.key_hi);
    double z[4];
    normal_pair(p.w[0], p.w[1], z[0], z[1]);
    normal_pair(p.w[2], p.w[3], z[2], z[3]);
    double* __restrict__ out = field + (r * h + y) * w + x0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (x0 + j < w) out[j] = z[j];
}

// out[r][c] = sum over m ascending of A[r][m] * B(m, c), the accumulator from +0.0, every product and every addition rounded on its own.
//   y pass: A = G_h [h][h], B(m, c) = field[m][c], out = tmp;      x pass: A = tmp [h][w], B(m, c) = G_w[c][m], out = field, times alpha.
// A workgroup owns a 16 x 64 tile of `out`: thread (lane cx, row group rg) four rows of one column.  Per 64 values of m the 16 rows of A and the
// 64 x 64 block of B are staged in LDS (B with the column fastest, whichever way it lies in memory): the A reads are broadcasts, the B reads
// consecutive.
constexpr int SM_ROWS = 16, SM_COLS = 64, SM_MC = 64, SM_THREADS = 256;
template <bool XPASS>
__global__ __launch_bounds__(SM_THREADS) void elastic_smooth_kernel(const elastic_meta* __restrict__ meta, double* field, double* tmp,
                                                                    const double* __restrict__ op, int h, int w) {
    const elastic_meta mt = meta[blockIdx.z >> 1];
    if (mt.status != 1) return;
    const long long plane = (long long)blockIdx.z * h * w;
    const double* __restrict__ a = XPASS ? tmp + plane : op;
    const double* __restrict__ b = XPASS ? op : field + plane;
    double* __restrict__ out = (XPASS ? field : tmp) + plane;
    const int m_all = XPASS ? w : h;                                           // a is [h][m_all]
    const int r0 = blockIdx.y * SM_ROWS, c0 = blockIdx.x * SM_COLS;
    const int tid = threadIdx.x, cx = tid & 63, rg = tid >> 6;
    __shared__ double a_s[SM_ROWS][SM_MC];
    __shared__ double b_s[SM_MC][SM_COLS + 1];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int m0 = 0; m0 < m_all; m0 += SM_MC) {
        const int ml = min(SM_MC, m_all - m0);
        for (int e = tid; e < SM_ROWS * SM_MC; e += SM_THREADS) {
            const int r = e >> 6, mm = e & 63;
            a_s[r][mm] = r0 + r < h && mm < ml ? a[(long long)(r0 + r) * m_all + m0 + mm] : 0.0;
        }
        for (int e = tid; e < SM_MC * SM_COLS; e += SM_THREADS) {
            if (XPASS) {                                                       // G_w[c][m]: consecutive lanes read consecutive m
                const int cc = e >> 6, mm = e & 63;
                b_s[mm][cc] = c0 + cc < w && mm < ml ? b[(long long)(c0 + cc) * w + m0 + mm] : 0.0;
            } else {
                const int mm = e >> 6, cc = e & 63;
                b_s[mm][cc] = c0 + cc < w && mm < ml ? b[(long long)(m0 + mm) * w + c0 + cc] : 0.0;
            }
        }
        __syncthreads();
        for (int mm = 0; mm < ml; ++mm) {                                      // past ml nothing is added: the staged zeros are never used
            const double bv = b_s[mm][cx];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = acc[u] + a_s[rg * 4 + u][mm] * bv;
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int r = r0 + rg * 4 + u;
        if (r < h && c0 + cx < w) out[(long long)r * w + c0 + cx] = XPASS ? mt.alpha * acc[u] : acc[u];
    }
}

// The cubic B-spline coefficients of a line p[0 .. n) with the half-sample symmetric boundary, z = SPLINE_Z:
//   s = p[reflect(-40)]; s = p[reflect(-k)] + z * s for k = 39 ... 1; c+[0] = p[0] + z * s; c+[k] = p[k] + z * c+[k - 1]
//   c[n - 1] = (z / (z - 1)) * c+[n - 1]; c[k] = z * (c[k + 1] - c+[k]); the coefficient is c[k] * 6
// The y pass: one lane per column, from the float32 scratch plane into the float64 coefficient plane.
constexpr int PF_LINES = 64;
__global__ __launch_bounds__(PF_LINES) void elastic_prefilter_y_kernel(const elastic_meta* __restrict__ meta, const float* __restrict__ sa,
                                                                       const float* __restrict__ sb, double* coef, int k, int h, int w) {
    const int i = blockIdx.z, pl = blockIdx.y, x = blockIdx.x * PF_LINES + threadIdx.x;
    if (meta[i].status != 1 || x >= w) return;
    const long long hw = (long long)h * w;
    const float* __restrict__ p = (pl < k ? sa + ((long long)i * k + pl) * hw : sb + (long long)i * hw) + x;
    double* c = coef + ((long long)i * (k + 1) + pl) * hw + x;
    double s = (double)p[(long long)reflect_index(-SPLINE_HORIZON, h) * w];
    for (int kk = SPLINE_HORIZON - 1; kk >= 1; --kk) s = (double)p[(long long)reflect_index(-kk, h) * w] + SPLINE_Z * s;
    double cp = (double)p[0] + SPLINE_Z * s;
    c[0] = cp;
    for (int y = 1; y < h; ++y) {
        cp = (double)p[(long long)y * w] + SPLINE_Z * cp;
        c[(long long)y * w] = cp;
    }
    double cm = SPLINE_LAST * cp;
    c[(long long)(h - 1) * w] = cm * 6.0;
    for (int y = h - 2; y >= 0; --y) {
        cm = SPLINE_Z * (cm - c[(long long)y * w]);
        c[(long long)y * w] = cm * 6.0;
    }
}

// The x pass, in place on the coefficient plane: one lane per row, 64 rows per workgroup (one wave); the rows pass through LDS 64 columns at a
// time, read and written with consecutive lanes on consecutive x, walked by each lane along its own row
__global__ __launch_bounds__(PF_LINES) void elastic_prefilter_x_kernel(const elastic_meta* __restrict__ meta, double* coef, int k, int h, int w) {
    const int i = blockIdx.z, pl = blockIdx.y, y0 = blockIdx.x * PF_LINES, lane = threadIdx.x;
    if (meta[i].status != 1) return;                                           // the whole workgroup
    double* c = coef + (((long long)i * (k + 1) + pl) * h + y0) * w;           // row y0 of the plane
    const int rows = min(PF_LINES, h - y0);
    const bool live = lane < rows;
    __shared__ double tile[PF_LINES][PF_LINES + 1];
    double s = 0.0, cp = 0.0, cm = 0.0;
    if (live) {                                                                // the causal start reads the row before anything is written to it
        const double* line = c + (long long)lane * w;
        s = line[reflect_index(-SPLINE_HORIZON, w)];
        for (int kk = SPLINE_HORIZON - 1; kk >= 1; --kk) s = line[reflect_index(-kk, w)] + SPLINE_Z * s;
    }
    __syncthreads();
    for (int x0 = 0; x0 < w; x0 += PF_LINES) {
        const int cols = min(PF_LINES, w - x0);
        for (int r = 0; r < rows; ++r)
            if (lane < cols) tile[r][lane] = c[(long long)r * w + x0 + lane];
        __syncthreads();
        if (live) {
            for (int j = 0; j < cols; ++j) {
                cp = tile[lane][j] + SPLINE_Z * (x0 + j == 0 ? s : cp);
                tile[lane][j] = cp;
            }
        }
        __syncthreads();
        for (int r = 0; r < rows; ++r)
            if (lane < cols) c[(long long)r * w + x0 + lane] = tile[r][lane];
        __syncthreads();
    }
    for (int x0 = ((w - 1) / PF_LINES) * PF_LINES; x0 >= 0; x0 -= PF_LINES) {
        const int cols = min(PF_LINES, w - x0);
        for (int r = 0; r < rows; ++r)
            if (lane < cols) tile[r][lane] = c[(long long)r * w + x0 + lane];
        __syncthreads();
        if (live) {
            for (int j = cols - 1; j >= 0; --j) {
                cm = x0 + j == w - 1 ? SPLINE_LAST * tile[lane][j] : SPLINE_Z * (cm - tile[lane][j]);
                tile[lane][j] = cm * 6.0;
            }
        }
        __syncthreads();
        for (int r = 0; r < rows; ++r)
            if (lane < cols) c[(long long)r * w + x0 + lane] = tile[r][lane];
        __syncthreads();
    }
}

// the four cubic B-spline weights of t in [0, 1), u = 1 - t
__device__ __forceinline__ void cubic_weights(double t, double (&wt)[4]) {
    const double u = 1.0 - t;
    wt[0] = ((u * u) * u) / 6.0;
    wt[1] = (((t * t) * (t - 2.0)) * 3.0 + 4.0) / 6.0;
    wt[2] = (((u * u) * (u - 2.0)) * 3.0 + 4.0) / 6.0;
    wt[3] = ((t * t) * t) / 6.0;
}

// One output pixel at the coordinate (cy, cx), both inside [-2^30, 2^30]: order 0 the pixel at floor(c + 0.5), order 1 two by two, order 3 four by
// four taps around floor(c), every index folded by reflect_index; the rows are summed first (x ascending from the first product), then the column
template <int ORDER, typename P>
__device__ __forceinline__ double elastic_sample(const P* __restrict__ p, double cy, double cx, int h, int w) {
    if constexpr (ORDER == 0) {
        const int iy = reflect_index((int)floor(cy + 0.5), h), ix = reflect_index((int)floor(cx + 0.5), w);
        return (double)p[(long long)iy * w + ix];
    } else {
    constexpr int TAPS = ORDER == 1 ? 2 : 4;
    const double fy = floor(cy), fx = floor(cx);
    const double ty = cy - fy, tx = cx - fx;
    double wy[4], wx[4];
    if (ORDER == 1) {
        wy[0] = 1.0 - ty, wy[1] = ty, wx[0] = 1.0 - tx, wx[1] = tx;
    } else {
        cubic_weights(ty, wy);
        cubic_weights(tx, wx);
    }
    const int by = (int)fy - (ORDER == 1 ? 0 : 1), bx = (int)fx - (ORDER == 1 ? 0 : 1);
    int ix[TAPS];
#pragma unroll
    for (int l = 0; l < TAPS; ++l) ix[l] = reflect_index(bx + l, w);
    double acc = 0.0;
#pragma unroll
    for (int m = 0; m < TAPS; ++m) {
        const P* __restrict__ line = p + (long long)reflect_index(by + m, h) * w;
        double r = wx[0] * (double)line[ix[0]];
#pragma unroll
        for (int l = 1; l < TAPS; ++l) r = r + wx[l] * (double)line[ix[l]];
        acc = m == 0 ? wy[0] * r : acc + wy[m] * r;
    }
    return acc;
    }
}

// The output batch: a thread produces 4 consecutive x of one output row (one Philox call per intensity stream)
template <typename T, int ORDER>
__global__ __launch_bounds__(VOL_THREADS) void elastic_gather_kernel(T* __restrict__ a, T* __restrict__ b, float* __restrict__ slice_idx,
                                                                     const elastic_meta* __restrict__ meta, const float* __restrict__ sa,
                                                                     const float* __restrict__ sb, const double* __restrict__ coef,
                                                                     const double* __restrict__ disp, const double* __restrict__ intensity,
                                                                     int independent_planes, int k, int h, int w, int runs, long long total) {
    constexpr int RUN = 4;
    const long long e = (long long)blockIdx.x * VOL_THREADS + threadIdx.x;
    if (e >= total) return;
    const int x0 = (int)(e % runs) * RUN;
    long long r = e / runs;
    const int y = (int)(r % h);
    r /= h;
    const int plane = (int)(r % (k + 1));                                      // plane k: the target B
    const int i = (int)(r / (k + 1));
    const elastic_meta mt = meta[i];
    // the scratch launch wrote the label, NaN for an invalid item or augment row; an invalid intensity or elastic row makes it NaN here
    if (plane == 0 && y == 0 && x0 == 0 && mt.status == 2) slice_idx[i] = __builtin_nanf("");

    const long long hw = (long long)h * w;
    const float* __restrict__ src = plane < k ? sa + ((long long)i * k + plane) * hw : sb + (long long)i * hw;
    float v[RUN];
    if (mt.status == 2) {
#pragma unroll
        for (int j = 0; j < RUN; ++j) v[j] = __builtin_nanf("");
    } else if (mt.status == 0) {                                               // the bits of the launch without the table
#pragma unroll
        for (int j = 0; j < RUN; ++j) v[j] = x0 + j < w ? src[(long long)y * w + x0 + j] : 0.0f;
    } else {
        const double* __restrict__ dy = disp + ((long long)i * 2) * hw + (long long)y * w;
        const double* __restrict__ dx = dy + hw;
        const double* __restrict__ cf = coef + ((long long)i * (k + 1) + plane) * hw;     // order 3 only
#pragma unroll
        for (int j = 0; j < RUN; ++j) {
            v[j] = 0.0f;
            if (x0 + j < w) {                                                  // elements past the row are never stored and read nothing
                const double cy = (double)y + dy[x0 + j], cx = (double)(x0 + j) + dx[x0 + j];
                // before any conversion to an integer; a NaN coordinate fails it too
                if (!(fabs(cy) <= COORD_MAX && fabs(cx) <= COORD_MAX)) v[j] = __builtin_nanf("");
                else if constexpr (ORDER == 3) v[j] = (float)elastic_sample<3, double>(cf, cy, cx, h, w);
                else v[j] = (float)elastic_sample<ORDER, float>(src, cy, cx, h, w);
            }
        }
    }
    if (mt.status != 2 && intensity != nullptr) {
        const double* __restrict__ row = intensity + mt.row * INTENSITY_ROW;
        const intensity_row n = intensity_row_of(row);                         // valid: the meta kernel checked it
        if (n.contrast || n.gaussian || n.poisson) intensity_apply<RUN>(v, n, row, x0, y, independent_planes ? (unsigned)plane << 1 : 0u);
    }
    store_run<T, RUN>((plane < k ? a + (((long long)i * k + plane) * h + y) * w : b + ((long long)i * h + y) * w) + x0, v, x0, w);
}

// the workspace: meta [count], the float32 scratch a [count][k][h][w] and b [count][h][w], field and tmp [count][2][h][w] float64 each and, for
// order 3, the coefficients [count][k + 1][h][w] float64; every part starts on a multiple of 256 bytes
struct elastic_layout {
    int64_t meta, sa, sb, field, tmp, coef, bytes;
};
static elastic_layout layout_of(int64_t count, int64_t k, int64_t h, int64_t w, int order) {
    auto up = [](int64_t v) { return (v + 255) / 256 * 256; };
    elastic_layout l;
    const int64_t hw = h * w;
    l.meta = 0;
    l.sa = up(count * (int64_t)sizeof(elastic_meta));
    l.sb = l.sa + up(count * k * hw * 4);
    l.field = l.sb + up(count * hw * 4);
    l.tmp = l.field + up(count * 2 * hw * 8);
    l.coef = l.tmp + up(count * 2 * hw * 8);
    l.bytes = l.coef + (order == 3 ? up(count * (k + 1) * hw * 8) : 0);
    return l;
}

static int check_geometry(int32_t count, int32_t k, int32_t h, int32_t w, int32_t order, const char* what) {
    AFCM_REQUIRE(order == 0 || order == 1 || order == 3, "%s: spline order %d is not 0, 1 or 3", what, order);
    AFCM_REQUIRE(k == 1 || k == 4, "%s: slice number %d is not 1 or 4", what, k);
    AFCM_REQUIRE(count >= 1 && count <= 32767 && h >= 1 && h <= 32768 && w >= 1 && w <= 32768,
                 "%s: %d items of [%d, %d]: 1 to 32767 items, extents 1 to 32768", what, count, h, w);
    return AFCM_OK;
}

// The launches of afcm_batch_assemble_elastic.  apply_intensity false (augment_blur.hip: a, b are its float32 scratch, out_dtype AFCM_F32): the
// intensity rows are checked as ever, but the gather leaves the transforms to the stage after it
int launch_elastic(void* a, void* b, float* slice_idx, const void* pool, int64_t pool_elems, int32_t src_dtype, const int64_t* vols, int32_t n_vols,
                   const int32_t* items, int32_t n_items, const double* augment, const double* intensity, int32_t independent_planes,
                   const double* elastic, const double* smooth_h, const double* smooth_w, int32_t spline_order, void* workspace,
                   int64_t workspace_bytes, const int64_t* cursor, int32_t first, int32_t count, int32_t k, int32_t h, int32_t w, int32_t out_dtype,
                   double min_value, double max_value, void* stream, bool apply_intensity) {
    AFCM_REQUIRE(elastic != nullptr && smooth_h != nullptr && smooth_w != nullptr && workspace != nullptr,
                 "batch_assemble_elastic: null elastic table, smoothing operator or workspace");
    AFCM_REQUIRE(independent_planes == 0 || independent_planes == 1, "batch_assemble_elastic: independent_planes %d is not 0 or 1", independent_planes);
    AFCM_REQUIRE(out_dtype >= AFCM_F32 && out_dtype <= AFCM_BF16, "batch_assemble: output dtype %d is not AFCM_F32 / AFCM_F16 / AFCM_BF16", out_dtype);
    if (const int rc = check_geometry(count, k, h, w, spline_order, "batch_assemble_elastic")) return rc;
    const elastic_layout l = layout_of(count, k, h, w, spline_order);
    AFCM_REQUIRE(workspace_bytes >= l.bytes, "batch_assemble_elastic: a workspace of %lld bytes, afcm_elastic_plan asks for %lld",
                 (long long)workspace_bytes, (long long)l.bytes);
    AFCM_REQUIRE((uintptr_t)workspace % 256 == 0, "batch_assemble_elastic: the workspace must start on a multiple of 256 bytes");
    char* ws = (char*)workspace;
    elastic_meta* meta = (elastic_meta*)(ws + l.meta);
    float *sa = (float*)(ws + l.sa), *sb = (float*)(ws + l.sb);
    double *field = (double*)(ws + l.field), *tmp = (double*)(ws + l.tmp), *coef = (double*)(ws + l.coef);
    hipStream_t s = (hipStream_t)stream;

    AFCM_REQUIRE(a != nullptr && b != nullptr, "batch_assemble: null output, label, pool or table");
    const int groups = cdiv(w, 4);
    const long long total = (long long)count * (k + 1) * h * groups;           // at most 2^15 * 5 * 2^15 * 2^13: no overflow
    AFCM_REQUIRE((double)total / VOL_THREADS < 2147483647.0, "batch_assemble_elastic: %.0f workgroups exceed the grid", (double)total / VOL_THREADS);
    // the scratch launch first: it makes every other check of the arguments the siblings make, before anything is launched
    if (const int rc = launch_batch(sa, sb, slice_idx, pool, pool_elems, src_dtype, vols, n_vols, items, n_items, augment, nullptr, 0, cursor, first, count,
                                    k, h, w, AFCM_F32, min_value, max_value, stream))
        return rc;
    hipLaunchKernelGGL(elastic_meta_kernel, dim3(cdiv(count, 64)), dim3(64), 0, s, meta, (long long)pool_elems, (const long long*)vols, n_vols,
                       (const int*)items, n_items, augment, intensity, elastic, (const long long*)cursor, first, count, k, h, w);
    const long long field_total = (long long)count * 2 * h * groups;
    hipLaunchKernelGGL(elastic_field_kernel, dim3((unsigned)((field_total + VOL_THREADS - 1) / VOL_THREADS)), dim3(VOL_THREADS), 0, s, meta, field, h, w,
                       groups, field_total);
    const dim3 tiles(cdiv(w, SM_COLS), cdiv(h, SM_ROWS), count * 2);
    hipLaunchKernelGGL(elastic_smooth_kernel<false>, tiles, dim3(SM_THREADS), 0, s, meta, field, tmp, smooth_h, h, w);
    hipLaunchKernelGGL(elastic_smooth_kernel<true>, tiles, dim3(SM_THREADS), 0, s, meta, field, tmp, smooth_w, h, w);
    if (spline_order == 3) {
        hipLaunchKernelGGL(elastic_prefilter_y_kernel, dim3(cdiv(w, PF_LINES), k + 1, count), dim3(PF_LINES), 0, s, meta, sa, sb, coef, k, h, w);
        hipLaunchKernelGGL(elastic_prefilter_x_kernel, dim3(cdiv(h, PF_LINES), k + 1, count), dim3(PF_LINES), 0, s, meta, coef, k, h, w);
    }
    const unsigned blocks = (unsigned)((total + VOL_THREADS - 1) / VOL_THREADS);
    auto gather = [&](auto t_tag) {
        using T = typename decltype(t_tag)::type;
#define AFCM_GATHER(ORDER)                                                                                                                    \
    hipLaunchKernelGGL((elastic_gather_kernel<T, ORDER>), dim3(blocks), dim3(VOL_THREADS), 0, s, (T*)a, (T*)b, slice_idx, meta, sa, sb, coef, field, \
                       apply_intensity ? intensity : nullptr, (int)independent_planes, k, h, w, groups, total)
        if (spline_order == 0) AFCM_GATHER(0);
        else if (spline_order == 1) AFCM_GATHER(1);
        else AFCM_GATHER(3);
#undef AFCM_GATHER
    };
    if (out_dtype == AFCM_F32) gather(type_tag<float>{});
    else if (out_dtype == AFCM_F16) gather(type_tag<f16_t>{});
    else gather(type_tag<bf16_t>{});
    return hip_status(hipGetLastError());
}

}  // namespace afcm

extern "C" int afcm_elastic_plan(int32_t count, int32_t k, int32_t h, int32_t w, int32_t order, int64_t* workspace_bytes, int32_t* launches) {
    using namespace afcm;
    AFCM_REQUIRE(workspace_bytes != nullptr, "elastic_plan: null workspace_bytes");
    if (const int rc = check_geometry(count, k, h, w, order, "elastic_plan")) return rc;
    *workspace_bytes = layout_of(count, k, h, w, order).bytes;
    if (launches != nullptr) *launches = order == 3 ? 8 : 6;
    return AFCM_OK;
}

extern "C" int afcm_batch_assemble_elastic(void* a, void* b, float* slice_idx, const void* pool, int64_t pool_elems, int32_t src_dtype,
                                           const int64_t* vols, int32_t n_vols, const int32_t* items, int32_t n_items, const double* augment,
                                           const double* intensity, int32_t independent_planes, const double* elastic, const double* smooth_h,
                                           const double* smooth_w, int32_t spline_order, void* workspace, int64_t workspace_bytes,
                                           const int64_t* cursor, int32_t first, int32_t count, int32_t k, int32_t h, int32_t w, int32_t out_dtype,
                                           double min_value, double max_value, void* stream) {
    return afcm::launch_elastic(a, b, slice_idx, pool, pool_elems, src_dtype, vols, n_vols, items, n_items, augment, intensity, independent_planes, elastic,
                                smooth_h, smooth_w, spline_order, workspace, workspace_bytes, cursor, first, count, k, h, w, out_dtype, min_value, max_value,
                                stream, true);
}
