// The G_ema update of the reference's training loop (train.py:74-77) for every tensor of the generator in ONE launch: parameters are lerped
// (p_ema <- p.lerp(p_ema, beta)), buffers of any dtype are copied byte for byte.  Run eagerly that is one multi-tensor lerp plus a copy_ per buffer,
// of the order of a hundred launches per step; here a table-driven kernel like adam_multi_kernel (optim.hip): a device table sorted by chunk0, a
// binary search per workgroup, 16-byte accesses where both pointers of the row allow them.  Beta is a launch scalar or slot 3 of the schedule block
// (schedule.hip), so a captured launch follows the ramp.  HBM-bound: reads p and p_ema, writes p_ema.  No atomics, no LDS.
#include "common.h"

namespace afcm {

// torch's lerp(p, p_ema, w), the form of optim.hip's first moment: the product fused into the sum
__device__ __forceinline__ float ema_lerp(float p, float p_ema, float w) {
    const float d = p_ema - p;
    return (w < 0.5f) ? __builtin_fmaf(w, d, p) : __builtin_fmaf(-d, 1.f - w, p_ema);
}

__global__ __launch_bounds__(256) void ema_multi_kernel(const afcm_ema_entry* __restrict__ table, int n, double beta_arg, const double* __restrict__ block) {
    const float w = (float)(block != nullptr ? block[3] : beta_arg);
    const long long chunk = blockIdx.x;
    int lo = 0, hi = n - 1;
    while (lo < hi) {                                                          // the row this chunk belongs to (wave-uniform)
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].chunk0 <= chunk) lo = mid; else hi = mid - 1;
    }
    const afcm_ema_entry e = table[lo];
    const long long base = (chunk - e.chunk0) * kAdamChunk;
    const long long end = min(base + (long long)kAdamChunk, (long long)e.numel);
    const bool vec = (((size_t)e.dst | (size_t)e.src) & 15) == 0;
    if (e.kind == AFCM_EMA_LERP) {
        float* __restrict__ pe = (float*)e.dst;
        const float* __restrict__ p = (const float*)e.src;
        if (vec) {
            for (long long i = base + 4 * threadIdx.x; i < end; i += 4 * 256) {
                if (i + 4 <= end) {
                    const float4 a = *(const float4*)(p + i);
                    float4 b = *(float4*)(pe + i);
                    b.x = ema_lerp(a.x, b.x, w); b.y = ema_lerp(a.y, b.y, w); b.z = ema_lerp(a.z, b.z, w); b.w = ema_lerp(a.w, b.w, w);
                    *(float4*)(pe + i) = b;
                } else {
                    for (long long j = i; j < end; j++) pe[j] = ema_lerp(p[j], pe[j], w);
                }
            }
        } else {
            for (long long j = base + threadIdx.x; j < end; j += 256) pe[j] = ema_lerp(p[j], pe[j], w);
        }
    } else {                                                                   // AFCM_EMA_COPY: numel counts bytes
        unsigned char* __restrict__ d = (unsigned char*)e.dst;
        const unsigned char* __restrict__ s = (const unsigned char*)e.src;
        if (vec) {
            for (long long i = base + 16 * threadIdx.x; i < end; i += 16 * 256) {
                if (i + 16 <= end) {
                    *(uint4*)(d + i) = *(const uint4*)(s + i);
                } else {
                    for (long long j = i; j < end; j++) d[j] = s[j];
                }
            }
        } else {
            for (long long j = base + threadIdx.x; j < end; j += 256) d[j] = s[j];
        }
    }
}

}  // namespace afcm

extern "C" int afcm_ema_multi(const afcm_ema_entry* table_dev, int32_t n, int64_t total_chunks, double beta, const double* block, void* stream) {
    using namespace afcm;
    AFCM_REQUIRE(table_dev != nullptr && n > 0, "ema_multi: empty table");
    AFCM_REQUIRE(total_chunks > 0 && total_chunks < (1ll << 31), "ema_multi: %lld chunks is out of range", (long long)total_chunks);
    AFCM_REQUIRE(block != nullptr || (beta >= 0.0 && beta <= 1.0), "ema_multi: beta %g is outside [0, 1]", beta);
    hipLaunchKernelGGL(ema_multi_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, table_dev, n, beta, block);
    return hip_status(hipGetLastError());
}
