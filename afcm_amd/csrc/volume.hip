// Whole-volume inference: the two ends of the reference's volume loop (evaluate.py -> StandardPredictor.__call__) on the device.
//   slice_assemble_kernel   the test-phase loader item (data/cmsr_dataset.py:98-155: centre crop / constant pad, the four thick slices around the
//                           target, Normalize to [-1, 1]) for a run of target slices of one source volume: the shared body of volume_common.h,
//                           one thread per run of consecutive x of one output row
//   halo_accumulate_kernel  remove_halo + "map[index] += patch; mask[index] += 1" (models/predictor.py:17-51,173-200) for one batch, in gather
//                           form: one thread per voxel of the batch's bounding box walks the batch's patches in ascending order
// Neither kernel stages anything in LDS or uses an atomic; every volume offset is 64-bit.  See include/afcm_hip.h for the semantics kept.
#include "common.h"
#include "volume_common.h"

namespace afcm {

// Arguments checked on the host.  A thread owns the run of RUN consecutive x at x0 of row y of input plane `plane` of target slice idx.
template <typename S, typename T, int RUN>
__global__ __launch_bounds__(VOL_THREADS) void slice_assemble_kernel(T* __restrict__ a, float* __restrict__ slice_idx, const S* __restrict__ src,
                                                                     int depth, int hs, int ws, long long stride_z, int first, int k,
                                                                     int thickness, int h, int w, int runs, long long total, double lo,
                                                                     double range) {
    const long long e = (long long)blockIdx.x * VOL_THREADS + threadIdx.x;
    if (e >= total) return;
    const int x0 = (int)(e % runs) * RUN;
    long long r = e / runs;
    const int y = (int)(r % h);
    r /= h;
    const int plane = (int)(r % k);
    const int i = (int)(r / k);
    const thick_slice at = thick_slice_of(first + i, thickness, k, plane);
    if (plane == 0 && y == 0 && x0 == 0) slice_idx[i] = at.label();
    float v[RUN];
    assembled_run<S, RUN>(v, src, depth, hs, ws, stride_z, at.pos, y, x0, h, w, lo, range);
    store_run<T, RUN>(a + (r * h + y) * w + x0, v, x0, w);
}

struct halo_axis {
    int p, n, a;        // patch extent, volume extent, halo
};

// remove_halo's new_slices for one axis: does the patch at origin o cover voxel v, and from which patch coordinate.
__device__ __forceinline__ bool halo_cover(const halo_axis& ax, int o, int v, int& src) {
    const int lo = o == 0 ? 0 : o + ax.a;
    const bool border_stop = o + ax.p == ax.n;
    const int hi = border_stop ? ax.n : o + ax.p - ax.a;
    src = (!border_stop && ax.a == 0) ? 0 : v - o;      // the reference's patch[..., :1], broadcast by numpy over the whole range
    return v >= lo && v < hi && src >= 0 && src < ax.p;
}

template <typename T>
__global__ __launch_bounds__(VOL_THREADS) void halo_accumulate_kernel(float* __restrict__ map, uint8_t* __restrict__ mask, const T* __restrict__ pred,
                                                                      long long sb, long long sc, long long sd, long long sh, long long sw,
                                                                      const int* __restrict__ origins, int count, halo_axis az, halo_axis ay,
                                                                      halo_axis ax, int prediction_channel, int z0, int y0, int x0, int bd, int bh,
                                                                      int bw, long long total) {
    const long long e = (long long)blockIdx.x * VOL_THREADS + threadIdx.x;
    if (e >= total) return;
    const int x = x0 + (int)(e % bw);
    long long r = e / bw;
    const int y = y0 + (int)(r % bh);
    r /= bh;
    const int z = z0 + (int)(r % bd);
    const int cm = (int)(r / bd);
    const long long c_off = (long long)(prediction_channel >= 0 ? prediction_channel : cm) * sc;
    const long long at = (((long long)cm * az.n + z) * ay.n + y) * ax.n + x;
    float acc = 0.f;
    unsigned visits = 0;
    bool touched = false;
    for (int i = 0; i < count; ++i) {
        const int oz = origins[i * 3 + 0], oy = origins[i * 3 + 1], ox = origins[i * 3 + 2];
        int pz, py, px;
        if (halo_cover(az, oz, z, pz) && halo_cover(ay, oy, y, py) && halo_cover(ax, ox, x, px)) {
            if (!touched) { acc = map[at]; visits = mask[at]; touched = true; }
            acc += (float)pred[(long long)i * sb + c_off + (long long)pz * sd + (long long)py * sh + (long long)px * sw];
            ++visits;
        }
    }
    if (touched) { map[at] = acc; mask[at] = (uint8_t)visits; }
}

}  // namespace afcm

extern "C" int afcm_slice_assemble(void* a, float* slice_idx, const void* src, int32_t src_dtype, int32_t out_dtype, int32_t depth, int32_t hs,
                                   int32_t ws, int64_t src_stride_z, int32_t first, int32_t count, int32_t k, int32_t thickness, int32_t h, int32_t w,
                                   double min_value, double max_value, void* stream) {
    using namespace afcm;
    AFCM_REQUIRE(a != nullptr && slice_idx != nullptr && src != nullptr, "slice_assemble: null output, label or source");
    AFCM_REQUIRE(src_dtype >= AFCM_SRC_U8 && src_dtype <= AFCM_SRC_F64, "slice_assemble: source dtype %d is not AFCM_SRC_U8 / I16 / F32 / F64", src_dtype);
    AFCM_REQUIRE(out_dtype >= AFCM_F32 && out_dtype <= AFCM_BF16, "slice_assemble: output dtype %d is not AFCM_F32 / AFCM_F16 / AFCM_BF16", out_dtype);
    AFCM_REQUIRE(depth > 0 && hs > 0 && ws > 0 && h > 0 && w > 0, "slice_assemble: source [%d, %d, %d] -> [%d, %d]: every extent must be positive", depth,
                 hs, ws, h, w);
    AFCM_REQUIRE(src_stride_z >= 0, "slice_assemble: source z stride %lld is negative", (long long)src_stride_z);
    AFCM_REQUIRE(count > 0 && first >= 0 && (long long)first + count <= depth, "slice_assemble: slices [%d, %lld) are not inside a volume of %d", first,
                 (long long)first + count, depth);
    AFCM_REQUIRE(k == 1 || k == 4, "slice_assemble: slice number %d is not 1 or 4", k);
    AFCM_REQUIRE(thickness != 0 && (k == 1 || thickness >= 1), "slice_assemble: thickness %d with slice number %d", thickness, k);
    AFCM_REQUIRE(max_value > min_value, "slice_assemble: max_value %g is not above min_value %g", max_value, min_value);
    const double range = max_value - min_value;
    return dispatch_src_out(src_dtype, out_dtype, [&](auto s_tag, auto t_tag) -> int {
        using S = typename decltype(s_tag)::type;
        using T = typename decltype(t_tag)::type;
        constexpr int RUN = run_length<T>;
        const int runs = cdiv(w, RUN);
        const double threads = (double)count * k * h * runs;                   // checked before the product is formed in 64 bits
        AFCM_REQUIRE(threads / VOL_THREADS < 2147483647.0, "slice_assemble: %.0f output elements exceed the grid", (double)count * k * h * w);
        const long long total = (long long)count * k * h * runs;
        const long long groups = (total + VOL_THREADS - 1) / VOL_THREADS;
        hipLaunchKernelGGL((slice_assemble_kernel<S, T, RUN>), dim3((unsigned)groups), dim3(VOL_THREADS), 0, (hipStream_t)stream, (T*)a, slice_idx,
                           (const S*)src, depth, hs, ws, (long long)src_stride_z, first, k, thickness, h, w, runs, total, min_value, range);
        return hip_status(hipGetLastError());
    });
}

extern "C" int afcm_halo_accumulate(float* map, uint8_t* mask, const void* pred, int32_t dtype, int64_t stride_b, int64_t stride_c, int64_t stride_d,
                                    int64_t stride_h, int64_t stride_w, int32_t channels, const int32_t* origins, int32_t table_len, int32_t first,
                                    int32_t count, int32_t pd, int32_t ph, int32_t pw, int32_t halo_z, int32_t halo_y, int32_t halo_x, int32_t D, int32_t H,
                                    int32_t W, int32_t map_channels, int32_t prediction_channel, int32_t z0, int32_t z1, int32_t y0, int32_t y1, int32_t x0,
                                    int32_t x1, void* stream) {
    using namespace afcm;
    AFCM_REQUIRE(map != nullptr && mask != nullptr && pred != nullptr && origins != nullptr, "halo_accumulate: null map, mask, prediction or origin table");
    AFCM_REQUIRE(dtype >= AFCM_F32 && dtype <= AFCM_BF16, "halo_accumulate: dtype %d is not AFCM_F32 / AFCM_F16 / AFCM_BF16", dtype);
    AFCM_REQUIRE(D > 0 && H > 0 && W > 0 && pd > 0 && ph > 0 && pw > 0 && channels > 0 && map_channels > 0,
                 "halo_accumulate: volume [%d, %d, %d], patch [%d, %d, %d], %d -> %d channels: every extent must be positive", D, H, W, pd, ph, pw, channels,
                 map_channels);
    AFCM_REQUIRE(pd <= D && ph <= H && pw <= W, "halo_accumulate: patch [%d, %d, %d] is larger than the volume [%d, %d, %d]", pd, ph, pw, D, H, W);
    AFCM_REQUIRE(halo_z >= 0 && halo_y >= 0 && halo_x >= 0, "halo_accumulate: negative halo (%d, %d, %d)", halo_z, halo_y, halo_x);
    AFCM_REQUIRE(halo_z <= pd && halo_y <= ph && halo_x <= pw, "halo_accumulate: halo (%d, %d, %d) exceeds the patch [%d, %d, %d]", halo_z, halo_y, halo_x, pd,
                 ph, pw);
    AFCM_REQUIRE(count > 0 && first >= 0 && (long long)first + count <= table_len, "halo_accumulate: patches [%d, %lld) are not inside a table of %d", first,
                 (long long)first + count, table_len);
    AFCM_REQUIRE(z0 >= 0 && z0 < z1 && z1 <= D && y0 >= 0 && y0 < y1 && y1 <= H && x0 >= 0 && x0 < x1 && x1 <= W,
                 "halo_accumulate: box [%d, %d) x [%d, %d) x [%d, %d) is empty or outside the volume [%d, %d, %d]", z0, z1, y0, y1, x0, x1, D, H, W);
    AFCM_REQUIRE(prediction_channel >= -1 && prediction_channel < channels, "halo_accumulate: prediction channel %d of %d", prediction_channel, channels);
    AFCM_REQUIRE(prediction_channel >= 0 ? map_channels == 1 : map_channels == channels,
                 "halo_accumulate: a map of %d channels for a prediction of %d channels (prediction channel %d)", map_channels, channels, prediction_channel);
    const int bd = z1 - z0, bh = y1 - y0, bw = x1 - x0;
    const long long total = (long long)map_channels * bd * bh * bw;
    AFCM_REQUIRE((total + VOL_THREADS - 1) / VOL_THREADS < (1ll << 31), "halo_accumulate: %lld box voxels exceed the grid", total);
    const halo_axis az = {pd, D, halo_z}, ay = {ph, H, halo_y}, ax = {pw, W, halo_x};
    const int* o = origins + (long long)first * 3;
    const dim3 grid((unsigned)((total + VOL_THREADS - 1) / VOL_THREADS)), block(VOL_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == AFCM_F32)
        hipLaunchKernelGGL(halo_accumulate_kernel<float>, grid, block, 0, s, map, mask, (const float*)pred, stride_b, stride_c, stride_d, stride_h, stride_w,
                           o, count, az, ay, ax, prediction_channel, z0, y0, x0, bd, bh, bw, total);
    else if (dtype == AFCM_F16)
        hipLaunchKernelGGL(halo_accumulate_kernel<f16_t>, grid, block, 0, s, map, mask, (const f16_t*)pred, stride_b, stride_c, stride_d, stride_h, stride_w,
                           o, count, az, ay, ax, prediction_channel, z0, y0, x0, bd, bh, bw, total);
    else
        hipLaunchKernelGGL(halo_accumulate_kernel<bf16_t>, grid, block, 0, s, map, mask, (const bf16_t*)pred, stride_b, stride_c, stride_d, stride_h,
                           stride_w, o, count, az, ay, ax, prediction_channel, z0, y0, x0, bd, bh, bw, total);
    return hip_status(hipGetLastError());
}
