// Training batches on the device: the train-phase loader item (data/cmsr_dataset.py:98-152) for a batch of unrelated (subject, slice, thickness)
// rows of a DEVICE item table, over a pool that holds every volume of the training set.
//   batch_assemble_kernel   A [count, k, h, w], B [count, 1, h, w] and the labels in one launch; a thread produces a run of RUN consecutive x of one
//                           output row (item, plane and row decoding, the table reads and the guards happen once per run) and stores it at once
//   batch_augment_kernel    the same launch with the item's flips, quarter turns and nearest-neighbour rotation (data/augment/transforms.py:25-112)
//                           from a DEVICE table of float64 parameter rows: a gather through the same crop / pad / normalise read
//   batch_intensity_kernel  either of the two with the item's contrast change, Gaussian and Poisson noise (transforms.py:115-133, 619-644) from a
//                           DEVICE table of float64 rows: a Philox4x32-10 field keyed per item, normals and counts from IEEE operations only
//   cursor_advance_kernel   cursor[0] += by, one thread: the table position of a captured graph moves on the device
// The tables cannot be checked on the host, so the kernels check every row before they read the pool; an invalid item reads nothing and comes out as
// NaN.  No LDS, no atomics; every pool offset is 64-bit.  See include/afcm_hip.h for the semantics kept.  The rows' readers and checks, Philox
// and the intensity arithmetic are in batch_common.h, shared with elastic.hip.
#include "batch_common.h"

namespace afcm {

template <typename S, typename T, int RUN>
__global__ __launch_bounds__(VOL_THREADS) void batch_assemble_kernel(T* __restrict__ a, T* __restrict__ b, float* __restrict__ slice_idx,
                                                                     const S* __restrict__ pool, long long pool_elems,
                                                                     const long long* __restrict__ vols, int n_vols, const int* __restrict__ items,
                                                                     int n_items, const long long* __restrict__ cursor, int first, int k, int h, int w,
                                                                     int runs, long long total, double lo, double range) {
    const long long e = (long long)blockIdx.x * VOL_THREADS + threadIdx.x;
    if (e >= total) return;
    const int x0 = (int)(e % runs) * RUN;
    long long r = e / runs;
    const int y = (int)(r % h);
    r /= h;
    const int plane = (int)(r % (k + 1));                                      // plane k: the target B
    const int i = (int)(r / (k + 1));

    // the item's row and its two volumes, checked before anything is read from the pool
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
    const thick_slice at = thick_slice_of(idx, valid ? t : 1, plane < k ? k : 1, plane);      // B: the k = 1 item of volume vb
    if (plane == 0 && y == 0 && x0 == 0) slice_idx[i] = valid ? at.label() : __builtin_nanf("");

    float v[RUN];
    if (!valid) {
#pragma unroll
        for (int j = 0; j < RUN; ++j) v[j] = __builtin_nanf("");
    } else {
        assembled_run<S, RUN>(v, pool + (plane < k ? off_a : off_b), depth, hs, ws, hs * ws, at.pos, y, x0, h, w, lo, range);
    }
    store_run<T, RUN>((plane < k ? a + (((long long)i * k + plane) * h + y) * w : b + ((long long)i * h + y) * w) + x0, v, x0, w);
}


template <typename S, typename T, int RUN>
__global__ __launch_bounds__(VOL_THREADS) void batch_augment_kernel(T* __restrict__ a, T* __restrict__ b, float* __restrict__ slice_idx,
                                                                    const S* __restrict__ pool, long long pool_elems,
                                                                    const long long* __restrict__ vols, int n_vols, const int* __restrict__ items,
                                                                    int n_items, const double* __restrict__ augment,
                                                                    const long long* __restrict__ cursor, int first, int k, int h, int w, int runs,
                                                                    long long total, double lo, double range) {
    const long long e = (long long)blockIdx.x * VOL_THREADS + threadIdx.x;
    if (e >= total) return;
    const int x0 = (int)(e % runs) * RUN;
    long long r = e / runs;
    const int y = (int)(r % h);
    r /= h;
    const int plane = (int)(r % (k + 1));                                      // plane k: the target B
    const int i = (int)(r / (k + 1));

    const batch_item it = item_of(i, pool_elems, vols, n_vols, items, n_items, cursor, first, k);
    augment_row g = {false, false, false, false, 0, 1.0, 0.0, 0.0, 0.0};
    if (it.valid) g = augment_row_of(augment + it.row * 8, h, w);              // the item row's own r: inside [0, n_items)
    const bool valid = it.valid && g.valid;
    const thick_slice at = thick_slice_of(it.idx, it.t, plane < k ? k : 1, plane);
    if (plane == 0 && y == 0 && x0 == 0) slice_idx[i] = valid ? at.label() : __builtin_nanf("");

    const S* __restrict__ volume = pool + (plane < k ? it.off_a : it.off_b);
    float v[RUN];
    if (!valid) {
#pragma unroll
        for (int j = 0; j < RUN; ++j) v[j] = __builtin_nanf("");
    } else if (g.identity || at.pos < 0 || at.pos > it.depth - 1) {            // the contiguous read; a plane outside the volume is a constant
        assembled_run<S, RUN>(v, volume, it.depth, it.hs, it.ws, it.hs * it.ws, at.pos, y, x0, h, w, lo, range);
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
                v[j] = normalised<S>(volume, slice + yv * it.ws + xv, yv >= 0 && yv < it.hs && xv >= 0 && xv < it.ws, lo, range);
            }
        }
    }
    store_run<T, RUN>((plane < k ? a + (((long long)i * k + plane) * h + y) * w : b + ((long long)i * h + y) * w) + x0, v, x0, w);
}


// batch_augment_kernel's item (the gather with an augment table, the contiguous read without one), then contrast, Gaussian and Poisson noise in
// float64 on the float32 item, one rounding back.  Pixel (y, x) of plane pl takes lane x & 3 of Philox(counter (x >> 2, y, stream | P << 1, 0),
// key of the row): a run starts at a multiple of 4, so a thread makes RUN / 4 calls per stream, and only in an item whose row sets the flag.
template <typename S, typename T, int RUN>
__global__ __launch_bounds__(VOL_THREADS) void batch_intensity_kernel(T* __restrict__ a, T* __restrict__ b, float* __restrict__ slice_idx,
                                                                      const S* __restrict__ pool, long long pool_elems,
                                                                      const long long* __restrict__ vols, int n_vols, const int* __restrict__ items,
                                                                      int n_items, const double* __restrict__ augment,
                                                                      const double* __restrict__ intensity, int independent_planes,
                                                                      const long long* __restrict__ cursor, int first, int k, int h, int w, int runs,
                                                                      long long total, double lo, double range) {
    static_assert(RUN % 4 == 0, "a run is whole Philox calls");
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
    intensity_row n = {false, false, false, false, 1.0, 0.0, 0.0, 0u, 0u, 0};
    const double* __restrict__ row = intensity + (it.valid ? it.row : 0) * INTENSITY_ROW;    // the item row's own r: inside [0, n_items)
    if (it.valid) {
        if (augment != nullptr) g = augment_row_of(augment + it.row * 8, h, w);
        n = intensity_row_of(row);
    }
    const bool valid = it.valid && g.valid && n.valid;
    const thick_slice at = thick_slice_of(it.idx, it.t, plane < k ? k : 1, plane);
    if (plane == 0 && y == 0 && x0 == 0) slice_idx[i] = valid ? at.label() : __builtin_nanf("");

    const S* __restrict__ volume = pool + (plane < k ? it.off_a : it.off_b);
    float v[RUN];
    if (!valid) {
#pragma unroll
        for (int j = 0; j < RUN; ++j) v[j] = __builtin_nanf("");
    } else if (g.identity || at.pos < 0 || at.pos > it.depth - 1) {            // the contiguous read; a plane outside the volume is a constant
        assembled_run<S, RUN>(v, volume, it.depth, it.hs, it.ws, it.hs * it.ws, at.pos, y, x0, h, w, lo, range);
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
                v[j] = normalised<S>(volume, slice + yv * it.ws + xv, yv >= 0 && yv < it.hs && xv >= 0 && xv < it.ws, lo, range);
            }
        }
    }
    if (valid && (n.contrast || n.gaussian || n.poisson))                      // a row without a flag: the bits of the launch without the table
        intensity_apply<RUN>(v, n, row, x0, y, independent_planes ? (unsigned)plane << 1 : 0u);
    store_run<T, RUN>((plane < k ? a + (((long long)i * k + plane) * h + y) * w : b + ((long long)i * h + y) * w) + x0, v, x0, w);
}

__global__ void cursor_advance_kernel(long long* __restrict__ cursor, long long by) {
    if (blockIdx.x == 0 && threadIdx.x == 0) cursor[0] += by;
}

// all three entry points: the checks, the (source, output) dispatch and the launch; augment and intensity null: the plain kernel; intensity given:
// the noise kernel, with or without an augment table
int launch_batch(void* a, void* b, float* slice_idx, const void* pool, int64_t pool_elems, int32_t src_dtype, const int64_t* vols, int32_t n_vols,
                 const int32_t* items, int32_t n_items, const double* augment, const double* intensity, int32_t independent_planes,
                 const int64_t* cursor, int32_t first, int32_t count, int32_t k, int32_t h, int32_t w, int32_t out_dtype, double min_value,
                 double max_value, void* stream) {
    AFCM_REQUIRE(a != nullptr && b != nullptr && slice_idx != nullptr && pool != nullptr && vols != nullptr && items != nullptr,
                 "batch_assemble: null output, label, pool or table");
    AFCM_REQUIRE(src_dtype >= AFCM_SRC_U8 && src_dtype <= AFCM_SRC_F64, "batch_assemble: source dtype %d is not AFCM_SRC_U8 / I16 / F32 / F64", src_dtype);
    AFCM_REQUIRE(out_dtype >= AFCM_F32 && out_dtype <= AFCM_BF16, "batch_assemble: output dtype %d is not AFCM_F32 / AFCM_F16 / AFCM_BF16", out_dtype);
    AFCM_REQUIRE(count > 0 && h > 0 && w > 0 && n_vols > 0 && n_items > 0 && pool_elems > 0,
                 "batch_assemble: %d items of [%d, %d] from %d volumes, a table of %d rows, a pool of %lld elements: every extent must be positive", count, h,
                 w, n_vols, n_items, (long long)pool_elems);
    AFCM_REQUIRE(first >= 0, "batch_assemble: first row %d is negative", first);
    AFCM_REQUIRE(k == 1 || k == 4, "batch_assemble: slice number %d is not 1 or 4", k);
    AFCM_REQUIRE(max_value > min_value, "batch_assemble: max_value %g is not above min_value %g", max_value, min_value);
    AFCM_REQUIRE(augment == nullptr || (long long)h + w <= (1LL << 28),
                 "batch_assemble_aug: a patch of [%d, %d]: h + w above 2^28 takes the rotated coordinates out of the int32 range", h, w);
    const double range = max_value - min_value;
    return dispatch_src_out(src_dtype, out_dtype, [&](auto s_tag, auto t_tag) -> int {
        using S = typename decltype(s_tag)::type;
        using T = typename decltype(t_tag)::type;
        constexpr int RUN = run_length<T>;
        const int runs = cdiv(w, RUN);
        const double threads = (double)count * (k + 1) * h * runs;             // checked before the product is formed in 64 bits
        AFCM_REQUIRE(threads / VOL_THREADS < 2147483647.0, "batch_assemble: %.0f workgroups exceed the grid", threads / VOL_THREADS);
        const long long total = (long long)count * (k + 1) * h * runs;
        const long long groups = (total + VOL_THREADS - 1) / VOL_THREADS;
        if (intensity != nullptr)
            hipLaunchKernelGGL((batch_intensity_kernel<S, T, RUN>), dim3((unsigned)groups), dim3(VOL_THREADS), 0, (hipStream_t)stream, (T*)a, (T*)b,
                               slice_idx, (const S*)pool, (long long)pool_elems, (const long long*)vols, n_vols, (const int*)items, n_items, augment,
                               intensity, (int)independent_planes, (const long long*)cursor, first, k, h, w, runs, total, min_value, range);
        else if (augment == nullptr)
            hipLaunchKernelGGL((batch_assemble_kernel<S, T, RUN>), dim3((unsigned)groups), dim3(VOL_THREADS), 0, (hipStream_t)stream, (T*)a, (T*)b,
                               slice_idx, (const S*)pool, (long long)pool_elems, (const long long*)vols, n_vols, (const int*)items, n_items,
                               (const long long*)cursor, first, k, h, w, runs, total, min_value, range);
        else
            hipLaunchKernelGGL((batch_augment_kernel<S, T, RUN>), dim3((unsigned)groups), dim3(VOL_THREADS), 0, (hipStream_t)stream, (T*)a, (T*)b,
                               slice_idx, (const S*)pool, (long long)pool_elems, (const long long*)vols, n_vols, (const int*)items, n_items, augment,
                               (const long long*)cursor, first, k, h, w, runs, total, min_value, range);
        return hip_status(hipGetLastError());
    });
}

}  // namespace afcm

extern "C" int afcm_batch_assemble(void* a, void* b, float* slice_idx, const void* pool, int64_t pool_elems, int32_t src_dtype, const int64_t* vols,
                                   int32_t n_vols, const int32_t* items, int32_t n_items, const int64_t* cursor, int32_t first, int32_t count, int32_t k,
                                   int32_t h, int32_t w, int32_t out_dtype, double min_value, double max_value, void* stream) {
    return afcm::launch_batch(a, b, slice_idx, pool, pool_elems, src_dtype, vols, n_vols, items, n_items, nullptr, nullptr, 0, cursor, first, count, k,
                              h, w, out_dtype, min_value, max_value, stream);
}

extern "C" int afcm_batch_assemble_aug(void* a, void* b, float* slice_idx, const void* pool, int64_t pool_elems, int32_t src_dtype, const int64_t* vols,
                                       int32_t n_vols, const int32_t* items, int32_t n_items, const double* augment, const int64_t* cursor, int32_t first,
                                       int32_t count, int32_t k, int32_t h, int32_t w, int32_t out_dtype, double min_value, double max_value,
                                       void* stream) {
    using namespace afcm;
    AFCM_REQUIRE(augment != nullptr, "batch_assemble_aug: null augment table");
    return launch_batch(a, b, slice_idx, pool, pool_elems, src_dtype, vols, n_vols, items, n_items, augment, nullptr, 0, cursor, first, count, k, h, w,
                        out_dtype, min_value, max_value, stream);
}

extern "C" int afcm_batch_assemble_noise(void* a, void* b, float* slice_idx, const void* pool, int64_t pool_elems, int32_t src_dtype, const int64_t* vols,
                                         int32_t n_vols, const int32_t* items, int32_t n_items, const double* augment, const double* intensity,
                                         int32_t independent_planes, const int64_t* cursor, int32_t first, int32_t count, int32_t k, int32_t h,
                                         int32_t w, int32_t out_dtype, double min_value, double max_value, void* stream) {
    using namespace afcm;
    AFCM_REQUIRE(intensity != nullptr, "batch_assemble_noise: null intensity table");
    AFCM_REQUIRE(independent_planes == 0 || independent_planes == 1, "batch_assemble_noise: independent_planes %d is not 0 or 1", independent_planes);
    return launch_batch(a, b, slice_idx, pool, pool_elems, src_dtype, vols, n_vols, items, n_items, augment, intensity, independent_planes, cursor, first,
                        count, k, h, w, out_dtype, min_value, max_value, stream);
}

extern "C" int afcm_cursor_advance(int64_t* cursor, int64_t by, void* stream) {
    using namespace afcm;
    AFCM_REQUIRE(cursor != nullptr, "cursor_advance: null cursor");
    hipLaunchKernelGGL(cursor_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (long long*)cursor, (long long)by);
    return hip_status(hipGetLastError());
}
