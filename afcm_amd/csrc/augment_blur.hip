// Training batches with a Gaussian blur on the device: the reference's GaussianBlur3D (data/augment/transforms.py:716-726) for the [1, h, w]
// planes of a loader item, every plane with its own decision and sigma, after the geometric transforms and the elastic deformation and before the
// intensity ones.  Which planes execute is known only on the device (the table is read through the cursor of a replayed graph), so the launches are
// fixed per batch and a plane whose flag is 0 goes through them on a copy path:
//   blur_meta_kernel           one workgroup per item: every table row of the item checked once, the blur row a thread per double; per item status
//                              and row, per plane flag (0 as it is, 1 blurred, 2 NaN), radius and the pointer to its weights in the table
//   the item into the scratch  float32, without the blur and intensity tables: launch_batch (batch.hip), or with an elastic table launch_elastic
//                              (elastic.hip), whose gather then writes the scratch instead of the outputs
//   blur_rows_kernel           the depth pass and the pass along y: a 32 x 64 output tile per workgroup, the depth-filtered float64 rows with a halo
//                              of `radius` rows staged in LDS, float32 scratch -> float64 intermediate
//   blur_cols_kernel           the pass along x: a 16 x 64 output tile per workgroup, the rows with a halo of `radius` columns staged in LDS, one
//                              rounding to float32, the intensity row where one is given, one store of 4 pixels
// The weights are made by the host (afcm_amd/augment_blur.py): no kernel evaluates an exponential.  Float64 multiply and add apart, the outermost
// pair first, no atomics: a batch has the same bits from call to call and the bits of afcm_amd/augment_blur.py.  See include/afcm_hip.h.
#include "batch_common.h"

extern "C" int afcm_elastic_plan(int32_t count, int32_t k, int32_t h, int32_t w, int32_t order, int64_t* workspace_bytes, int32_t* launches);

namespace afcm {

constexpr int BLUR_R_MAX = 16, BLUR_PLANE_COLS = 3 + BLUR_R_MAX + 1, BLUR_ELASTIC_ROW = 4;

struct blur_item {
    int status;                                                                // 0: a valid item; 2: an invalid row somewhere: NaN
    int pad;
    long long row;                                                             // the item's table row, inside [0, n_items) unless status is 2
};
struct blur_plane {
    int flag;                                                                  // 0: the plane as it is; 1: blurred; 2: a plane of a NaN item
    int radius;
    const double* w;                                                           // w_0 ... w_16 of the plane's record in the table
};
static_assert(sizeof(blur_item) == 16 && sizeof(blur_plane) == 16, "the meta records are 16 bytes of the workspace each");

// One workgroup per item: thread 0 checks the item row and the rows of the other tables, then thread t checks double t of the item's blur row
// (one load deep, where one thread per item would walk 100 dependent loads), and the first k + 1 threads write the plane records
constexpr int BLUR_META_THREADS = 128;
static_assert(BLUR_META_THREADS >= 5 * BLUR_PLANE_COLS, "a thread per double of the longest row");
__global__ __launch_bounds__(BLUR_META_THREADS) void blur_meta_kernel(blur_item* __restrict__ item_meta, blur_plane* __restrict__ plane_meta,
                                                                      long long pool_elems, const long long* __restrict__ vols, int n_vols,
                                                                      const int* __restrict__ items, int n_items, const double* __restrict__ augment,
                                                                      const double* __restrict__ intensity, const double* __restrict__ elastic,
                                                                      const double* __restrict__ blur, const long long* __restrict__ cursor, int first,
                                                                      int k, int h, int w) {
    const int i = blockIdx.x, tid = threadIdx.x;
    __shared__ long long row_s;
    __shared__ int valid_s;
    if (tid == 0) {
        const batch_item it = item_of(i, pool_elems, vols, n_vols, items, n_items, cursor, first, k);
        bool valid = it.valid;                                                 // the item row's own r: inside [0, n_items) of every table
        if (valid && augment != nullptr) valid = augment_row_of(augment + it.row * 8, h, w).valid;
        if (valid && intensity != nullptr) valid = intensity_row_of(intensity + it.row * INTENSITY_ROW).valid;
        if (valid && elastic != nullptr) {                                     // elastic_meta_kernel's check
            const double* __restrict__ p = elastic + it.row * BLUR_ELASTIC_ROW;
            valid = (p[0] == 0.0 || p[0] == 1.0) && fabs(p[1]) <= 1048576.0 && whole_in(p[2], 4294967295.0) && whole_in(p[3], 4294967295.0);
        }
        valid_s = valid ? 1 : 0;
        row_s = valid ? it.row : 0;
    }
    __syncthreads();
    const int planes = k + 1, cols = planes * BLUR_PLANE_COLS;
    const double* __restrict__ row = blur + row_s * cols;
    bool ok = valid_s != 0;
    if (ok && tid < cols) {                                                    // every comparison is false for a NaN
        const double big = 1.7976931348623157e308, v = row[tid];
        const int c = tid % BLUR_PLANE_COLS;
        ok = c == 0 ? (v == 0.0 || v == 1.0) : (c == 1 ? (v > 0.0 && v <= big) : (c == 2 ? whole_in(v, (double)BLUR_R_MAX) : fabs(v) <= big));
    }
    const bool valid = __syncthreads_and(ok ? 1 : 0) != 0;
    if (tid == 0) item_meta[i] = {valid ? 0 : 2, 0, row_s};
    if (tid < planes) {
        const double* rec = row + tid * BLUR_PLANE_COLS;
        blur_plane m = {2, 0, nullptr};
        if (valid) m = {rec[0] == 1.0 ? 1 : 0, (int)rec[2], rec + 3};
        plane_meta[i * planes + tid] = m;
    }
}

__device__ __forceinline__ int clamp_index(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// One line pass: t = v_0 w_0, then t = t + (v_-j + v_+j) w_j for j = radius ... 1, every operation rounded on its own.  `at(d)`: the element d
// places from the output's own
template <typename F>
__device__ __forceinline__ double blur_taps(const double* __restrict__ wt, int radius, F&& at) {
    double t = at(0) * wt[0];
    for (int j = radius; j >= 1; --j) t = t + (at(-j) + at(j)) * wt[j];
    return t;
}

// A workgroup owns a ROWS x COLS tile of one plane; workgroup b of the launch is tile (b % tiles_x, (b / tiles_x) % tiles_y) of plane
// b / (tiles_x tiles_y), the planes of item i being i (k + 1) ... + k, the target last
constexpr int BLUR_THREADS = 256;
constexpr int BLUR_ROWS_TILE_H = 32, BLUR_ROWS_TILE_W = 64;                    // the pass along y
constexpr int BLUR_COLS_TILE_H = 16, BLUR_COLS_TILE_W = 64;                    // the pass along x: 16 threads of 4 pixels per row
// the staged line: the tile, the halo on both sides, and 2 more so that the rows of a half wave start 4 banks apart
constexpr int BLUR_COLS_STRIDE = BLUR_COLS_TILE_W + 2 * BLUR_R_MAX + 2;

// The depth pass (a line of one element: every neighbour is the element itself) and the pass along y.  Rows [r0 - radius, r0 + rows + radius),
// clamped into the plane, are read from the float32 scratch, depth-filtered and staged; thread (column cx, row group rg) then filters 8 rows of one
// column: consecutive lanes read consecutive doubles
__global__ __launch_bounds__(BLUR_THREADS) void blur_rows_kernel(const blur_plane* __restrict__ plane_meta, const float* __restrict__ sa,
                                                                 const float* __restrict__ sb, double* __restrict__ mid, int k, int h, int w,
                                                                 int tiles_x, int tiles_y) {
    int b = blockIdx.x;
    const int c0 = (b % tiles_x) * BLUR_ROWS_TILE_W;
    b /= tiles_x;
    const int r0 = (b % tiles_y) * BLUR_ROWS_TILE_H, plane = b / tiles_y;
    const blur_plane pl = plane_meta[plane];
    if (pl.flag != 1) return;                                                  // the whole workgroup: the pass along x reads the scratch itself
    __shared__ double wt[BLUR_R_MAX + 1];
    __shared__ double col[BLUR_ROWS_TILE_H + 2 * BLUR_R_MAX][BLUR_ROWS_TILE_W];
    const int tid = threadIdx.x, radius = pl.radius;
    if (tid <= radius) wt[tid] = pl.w[tid];
    __syncthreads();
    const long long hw = (long long)h * w;
    const int i = plane / (k + 1), p = plane % (k + 1);
    const float* __restrict__ src = p < k ? sa + ((long long)i * k + p) * hw : sb + (long long)i * hw;
    const int rows = min(BLUR_ROWS_TILE_H, h - r0), staged = rows + 2 * radius;
    for (int e = tid; e < staged * BLUR_ROWS_TILE_W; e += BLUR_THREADS) {
        const int rr = e / BLUR_ROWS_TILE_W, cc = e % BLUR_ROWS_TILE_W;
        double t = 0.0;
        if (c0 + cc < w) {
            const double v = (double)src[(long long)clamp_index(r0 - radius + rr, h) * w + c0 + cc];
            t = blur_taps(wt, radius, [&](int) { return v; });
        }
        col[rr][cc] = t;
    }
    __syncthreads();
    const int cx = tid % BLUR_ROWS_TILE_W, rg = tid / BLUR_ROWS_TILE_W;
    constexpr int PER_THREAD = BLUR_ROWS_TILE_H / (BLUR_THREADS / BLUR_ROWS_TILE_W);
    if (c0 + cx >= w) return;
    double* __restrict__ out = mid + (long long)plane * hw + (long long)r0 * w + c0 + cx;
    for (int u = 0; u < PER_THREAD; ++u) {
        const int rr = rg * PER_THREAD + u;
        if (rr < rows) out[(long long)rr * w] = blur_taps(wt, radius, [&](int d) { return col[rr + radius + d][cx]; });
    }
}

// The pass along x and the rest of the chain: a thread produces 4 consecutive x of one output row (one Philox call per intensity stream)
template <typename T>
__global__ __launch_bounds__(BLUR_THREADS) void blur_cols_kernel(T* __restrict__ a, T* __restrict__ b, float* __restrict__ slice_idx,
                                                                 const blur_item* __restrict__ item_meta, const blur_plane* __restrict__ plane_meta,
                                                                 const float* __restrict__ sa, const float* __restrict__ sb,
                                                                 const double* __restrict__ mid, const double* __restrict__ intensity,
                                                                 int independent_planes, int k, int h, int w, int tiles_x, int tiles_y) {
    constexpr int RUN = 4, RUNS = BLUR_COLS_TILE_W / RUN;
    int bid = blockIdx.x;
    const int tx = bid % tiles_x;
    bid /= tiles_x;
    const int ty = bid % tiles_y, plane_of_batch = bid / tiles_y;
    const int c0 = tx * BLUR_COLS_TILE_W, r0 = ty * BLUR_COLS_TILE_H;
    const int i = plane_of_batch / (k + 1), plane = plane_of_batch % (k + 1);  // plane k: the target B
    const blur_item mt = item_meta[i];
    const blur_plane pl = plane_meta[plane_of_batch];
    const int tid = threadIdx.x, radius = pl.radius;
    // the scratch launch wrote the label, NaN for an invalid item, augment or elastic row; an invalid intensity or blur row makes it NaN here
    if (plane == 0 && tx == 0 && ty == 0 && tid == 0 && mt.status == 2) slice_idx[i] = __builtin_nanf("");

    const long long hw = (long long)h * w;
    __shared__ double wt[BLUR_R_MAX + 1];
    __shared__ double line[BLUR_COLS_TILE_H][BLUR_COLS_STRIDE];
    if (pl.flag == 1) {                                                        // the whole workgroup
        if (tid <= radius) wt[tid] = pl.w[tid];
        const int rows = min(BLUR_COLS_TILE_H, h - r0), span = BLUR_COLS_TILE_W + 2 * radius;
        const double* __restrict__ m = mid + (long long)plane_of_batch * hw + (long long)r0 * w;
        for (int e = tid; e < rows * span; e += BLUR_THREADS) {
            const int rr = e / span, cc = e % span;
            line[rr][cc] = m[(long long)rr * w + clamp_index(c0 - radius + cc, w)];
        }
        __syncthreads();
    }
    const int row = tid / RUNS, xl = (tid % RUNS) * RUN;
    const int y = r0 + row, x0 = c0 + xl;
    if (y >= h || x0 >= w) return;
    const float* __restrict__ src = plane < k ? sa + ((long long)i * k + plane) * hw : sb + (long long)i * hw;
    float v[RUN];
    if (pl.flag == 2) {
#pragma unroll
        for (int j = 0; j < RUN; ++j) v[j] = __builtin_nanf("");
    } else if (pl.flag == 0) {                                                 // the bits of the launch without the table
#pragma unroll
        for (int j = 0; j < RUN; ++j) v[j] = x0 + j < w ? src[(long long)y * w + x0 + j] : 0.0f;
    } else {
#pragma unroll
        for (int j = 0; j < RUN; ++j) {                                        // elements past the row are never stored
            v[j] = 0.0f;
            if (x0 + j < w) v[j] = (float)blur_taps(wt, radius, [&](int d) { return line[row][xl + j + radius + d]; });
        }
    }
    if (mt.status != 2 && intensity != nullptr) {
        const double* __restrict__ irow = intensity + mt.row * INTENSITY_ROW;
        const intensity_row n = intensity_row_of(irow);                        // valid: the meta kernel checked it
        if (n.contrast || n.gaussian || n.poisson) intensity_apply<RUN>(v, n, irow, x0, y, independent_planes ? (unsigned)plane << 1 : 0u);
    }
    store_run<T, RUN>((plane < k ? a + (((long long)i * k + plane) * h + y) * w : b + ((long long)i * h + y) * w) + x0, v, x0, w);
}

// the workspace: the item and plane records, the float32 scratch a [count][k][h][w] and b [count][h][w], the float64 intermediate
// [count][k + 1][h][w] and, with an elastic table, the workspace of its launches; every part starts on a multiple of 256 bytes
struct blur_layout {
    int64_t item_meta, plane_meta, sa, sb, mid, elastic, elastic_bytes, bytes;
};
static int blur_layout_of(int32_t count, int32_t k, int32_t h, int32_t w, int32_t order, const char* what, blur_layout& l) {
    AFCM_REQUIRE(k == 1 || k == 4, "%s: slice number %d is not 1 or 4", what, k);
    AFCM_REQUIRE(count >= 1 && count <= 32767 && h >= 1 && h <= 32768 && w >= 1 && w <= 32768,
                 "%s: %d items of [%d, %d]: 1 to 32767 items, extents 1 to 32768", what, count, h, w);
    AFCM_REQUIRE(order == -1 || order == 0 || order == 1 || order == 3, "%s: spline order %d is not 0, 1 or 3 (-1: no elastic table)", what, order);
    auto up = [](int64_t v) { return (v + 255) / 256 * 256; };
    const int64_t hw = (int64_t)h * w, n = count;
    l.item_meta = 0;
    l.plane_meta = up(n * (int64_t)sizeof(blur_item));
    l.sa = l.plane_meta + up(n * (k + 1) * (int64_t)sizeof(blur_plane));
    l.sb = l.sa + up(n * k * hw * 4);
    l.mid = l.sb + up(n * hw * 4);
    l.elastic = l.mid + up(n * (k + 1) * hw * 8);
    l.elastic_bytes = 0;
    if (order != -1)
        if (const int rc = afcm_elastic_plan(count, k, h, w, order, &l.elastic_bytes, nullptr)) return rc;
    l.bytes = l.elastic + up(l.elastic_bytes);
    return AFCM_OK;
}

}  // namespace afcm

extern "C" int afcm_blur_plan(int32_t count, int32_t k, int32_t h, int32_t w, int32_t elastic_order, int64_t* workspace_bytes, int32_t* launches) {
    using namespace afcm;
    AFCM_REQUIRE(workspace_bytes != nullptr, "blur_plan: null workspace_bytes");
    blur_layout l;
    if (const int rc = blur_layout_of(count, k, h, w, elastic_order, "blur_plan", l)) return rc;
    *workspace_bytes = l.bytes;
    if (launches != nullptr) {
        int32_t inner = 1;                                                     // the assembly launch, or the elastic launches around it
        if (elastic_order != -1) afcm_elastic_plan(count, k, h, w, elastic_order, &l.elastic_bytes, &inner);
        *launches = 3 + inner;
    }
    return AFCM_OK;
}

extern "C" int afcm_batch_assemble_blur(void* a, void* b, float* slice_idx, const void* pool, int64_t pool_elems, int32_t src_dtype, const int64_t* vols,
                                        int32_t n_vols, const int32_t* items, int32_t n_items, const double* augment, const double* intensity,
                                        int32_t independent_planes, const double* elastic, const double* smooth_h, const double* smooth_w,
                                        int32_t spline_order, const double* blur, void* workspace, int64_t workspace_bytes, const int64_t* cursor,
                                        int32_t first, int32_t count, int32_t k, int32_t h, int32_t w, int32_t out_dtype, double min_value,
                                        double max_value, void* stream) {
    using namespace afcm;
    AFCM_REQUIRE(blur != nullptr && workspace != nullptr, "batch_assemble_blur: null blur table or workspace");
    AFCM_REQUIRE(independent_planes == 0 || independent_planes == 1, "batch_assemble_blur: independent_planes %d is not 0 or 1", independent_planes);
    AFCM_REQUIRE(out_dtype >= AFCM_F32 && out_dtype <= AFCM_BF16, "batch_assemble: output dtype %d is not AFCM_F32 / AFCM_F16 / AFCM_BF16", out_dtype);
    AFCM_REQUIRE(a != nullptr && b != nullptr, "batch_assemble: null output, label, pool or table");
    blur_layout l;
    if (const int rc = blur_layout_of(count, k, h, w, elastic != nullptr ? spline_order : -1, "batch_assemble_blur", l)) return rc;
    AFCM_REQUIRE(elastic == nullptr || spline_order != -1, "batch_assemble_blur: spline order -1 with an elastic table");
    AFCM_REQUIRE(workspace_bytes >= l.bytes, "batch_assemble_blur: a workspace of %lld bytes, afcm_blur_plan asks for %lld", (long long)workspace_bytes,
                 (long long)l.bytes);
    AFCM_REQUIRE((uintptr_t)workspace % 256 == 0, "batch_assemble_blur: the workspace must start on a multiple of 256 bytes");
    const long long planes = (long long)count * (k + 1);
    const int rows_x = cdiv(w, BLUR_ROWS_TILE_W), rows_y = cdiv(h, BLUR_ROWS_TILE_H), cols_x = cdiv(w, BLUR_COLS_TILE_W), cols_y = cdiv(h, BLUR_COLS_TILE_H);
    const long long rows_groups = planes * rows_x * rows_y, cols_groups = planes * cols_x * cols_y;   // at most 163835 * 512 * 2048: no overflow
    AFCM_REQUIRE(rows_groups <= 2147483647LL && cols_groups <= 2147483647LL, "batch_assemble_blur: %lld workgroups exceed the grid", cols_groups);
    char* ws = (char*)workspace;
    blur_item* item_meta = (blur_item*)(ws + l.item_meta);
    blur_plane* plane_meta = (blur_plane*)(ws + l.plane_meta);
    float *sa = (float*)(ws + l.sa), *sb = (float*)(ws + l.sb);
    double* mid = (double*)(ws + l.mid);
    hipStream_t s = (hipStream_t)stream;

    // the scratch launches first: they make every other check of the arguments the siblings make, before anything is launched
    if (elastic != nullptr) {
        if (const int rc = launch_elastic(sa, sb, slice_idx, pool, pool_elems, src_dtype, vols, n_vols, items, n_items, augment, intensity,
                                          independent_planes, elastic, smooth_h, smooth_w, spline_order, ws + l.elastic, l.elastic_bytes, cursor, first,
                                          count, k, h, w, AFCM_F32, min_value, max_value, stream, false))
            return rc;
    } else if (const int rc = launch_batch(sa, sb, slice_idx, pool, pool_elems, src_dtype, vols, n_vols, items, n_items, augment, nullptr, 0, cursor,
                                           first, count, k, h, w, AFCM_F32, min_value, max_value, stream)) {
        return rc;
    }
    hipLaunchKernelGGL(blur_meta_kernel, dim3(count), dim3(BLUR_META_THREADS), 0, s, item_meta, plane_meta, (long long)pool_elems,
                       (const long long*)vols, n_vols, (const int*)items, n_items, augment, intensity, elastic, blur, (const long long*)cursor, first, k, h, w);
    hipLaunchKernelGGL(blur_rows_kernel, dim3((unsigned)rows_groups), dim3(BLUR_THREADS), 0, s, plane_meta, sa, sb, mid, k, h, w, rows_x, rows_y);
    auto columns = [&](auto t_tag) {
        using T = typename decltype(t_tag)::type;
        hipLaunchKernelGGL((blur_cols_kernel<T>), dim3((unsigned)cols_groups), dim3(BLUR_THREADS), 0, s, (T*)a, (T*)b, slice_idx, item_meta, plane_meta, sa,
                           sb, mid, intensity, (int)independent_planes, k, h, w, cols_x, cols_y);
    };
    if (out_dtype == AFCM_F32) columns(type_tag<float>{});
    else if (out_dtype == AFCM_F16) columns(type_tag<f16_t>{});
    else columns(type_tag<bf16_t>{});
    return hip_status(hipGetLastError());
}

extern "C" void afcm_blur_tiles(int32_t* rows_tile_h, int32_t* rows_tile_w, int32_t* cols_tile_h, int32_t* cols_tile_w) {
    *rows_tile_h = afcm::BLUR_ROWS_TILE_H, *rows_tile_w = afcm::BLUR_ROWS_TILE_W, *cols_tile_h = afcm::BLUR_COLS_TILE_H, *cols_tile_w = afcm::BLUR_COLS_TILE_W;
}
