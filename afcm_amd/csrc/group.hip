// Shared-encoder inference: the encoder state of G conditioning images repeated for a decoder batch of B samples by a DEVICE index, every tensor of
// the state (bottleneck, skip maps, global vector) in ONE launch: out_k[b] = in_k[groups[b]] over whole per-sample blocks, byte for byte.  A
// table-driven kernel like ema_multi_kernel (ema.hip): a device table sorted by chunk0, a binary search per workgroup; a chunk is kGroupChunk bytes
// of one block of one sample.  A pure copy, HBM-bound: each lane has four 16-byte loads in flight before its first store where both blocks start on
// 16-byte boundaries.  The index cannot be checked on the host, so the kernel checks it before it reads: an invalid sample reads nothing and comes
// out as NaN.  No atomics, no LDS; every offset is 64-bit.  See include/afcm_hip.h for the semantics kept.
#include "common.h"

namespace afcm {

constexpr int kGroupLanes = 256;
constexpr int kGroupInFlight = 4;
constexpr int kGroupChunk = kGroupLanes * kGroupInFlight * 16;             // bytes of one block per workgroup

template <typename E>
__device__ __forceinline__ void group_copy_elems(unsigned char* __restrict__ d, const unsigned char* __restrict__ s, long long from, long long end,
                                                 bool valid, E nan_bits) {
    for (long long j = from + (long long)sizeof(E) * threadIdx.x; j < end; j += (long long)sizeof(E) * kGroupLanes)
        *(E*)(d + j) = valid ? *(const E*)(s + j) : nan_bits;
}

__global__ __launch_bounds__(kGroupLanes) void group_expand_kernel(const afcm_group_entry* __restrict__ table, int n, int batch,
                                                                   const int* __restrict__ groups) {
    const long long chunk = blockIdx.x;
    int lo = 0, hi = n - 1;
    while (lo < hi) {                                                          // the row this chunk belongs to (wave-uniform)
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].chunk0 <= chunk) lo = mid; else hi = mid - 1;
    }
    const afcm_group_entry e = table[lo];
    const long long per_block = (e.block_bytes + kGroupChunk - 1) / kGroupChunk;
    const long long local = chunk - e.chunk0;
    const long long b = local / per_block;
    if (b >= batch) return;                                                    // (the host sized the grid from the same rows)
    const long long base = (local - b * per_block) * kGroupChunk;
    const long long end = min(base + (long long)kGroupChunk, (long long)e.block_bytes);

    const int g = groups[b];
    const bool valid = g >= 0 && g < e.groups;                                 // checked before anything is read from the source
    unsigned char* __restrict__ d = (unsigned char*)e.dst + b * e.block_bytes;
    const unsigned char* __restrict__ s = (const unsigned char*)e.src + (valid ? (long long)g : 0ll) * e.block_bytes;
    const bool two = e.kind == AFCM_GROUP_2B;

    long long done = base;                                                     // bytes below this are moved 16 at a time
    if ((((size_t)d | (size_t)s) & 15) == 0) {
        done = base + ((end - base) & ~15ll);
        const long long i0 = base + 16ll * threadIdx.x;
        uint4 v[kGroupInFlight];
        const unsigned int nan4 = two ? 0x7FFF7FFFu : 0x7FC00000u;
#pragma unroll
        for (int k = 0; k < kGroupInFlight; ++k) {
            const long long i = i0 + (long long)k * 16 * kGroupLanes;
            v[k] = make_uint4(nan4, nan4, nan4, nan4);
            if (valid && i < done) v[k] = *(const uint4*)(s + i);
        }
#pragma unroll
        for (int k = 0; k < kGroupInFlight; ++k) {
            const long long i = i0 + (long long)k * 16 * kGroupLanes;
            if (i < done) *(uint4*)(d + i) = v[k];
        }
    }
    if (done < end) {                                                          // a block's tail, or blocks off the 16-byte grid
        if (two) group_copy_elems<unsigned short>(d, s, done, end, valid, (unsigned short)0x7FFF);
        else group_copy_elems<unsigned int>(d, s, done, end, valid, 0x7FC00000u);
    }
}

}  // namespace afcm

extern "C" int32_t afcm_group_chunk_bytes(void) { return afcm::kGroupChunk; }

extern "C" int afcm_group_expand(const afcm_group_entry* table_dev, const afcm_group_entry* table_host, int32_t n, int32_t batch, const int32_t* groups,
                                 void* stream) {
    using namespace afcm;
    AFCM_REQUIRE(table_dev != nullptr && table_host != nullptr && n > 0, "group_expand: empty table");
    AFCM_REQUIRE(groups != nullptr, "group_expand: null groups");
    AFCM_REQUIRE(batch >= 1, "group_expand: batch %d is below 1", batch);
    long long total = 0;
    for (int k = 0; k < n; ++k) {
        const afcm_group_entry& e = table_host[k];
        AFCM_REQUIRE(e.dst != nullptr && e.src != nullptr, "group_expand: row %d has a null source or destination", k);
        AFCM_REQUIRE(e.kind == AFCM_GROUP_2B || e.kind == AFCM_GROUP_4B, "group_expand: row %d: kind %d is not AFCM_GROUP_2B / AFCM_GROUP_4B", k, e.kind);
        AFCM_REQUIRE(e.block_bytes > 0 && e.block_bytes % e.kind == 0, "group_expand: row %d: a block of %lld bytes is empty or no multiple of %d", k,
                     (long long)e.block_bytes, e.kind);
        AFCM_REQUIRE(e.groups >= 1, "group_expand: row %d: %d groups", k, e.groups);
        AFCM_REQUIRE(e.chunk0 == total, "group_expand: row %d starts at chunk %lld, the rows before it end at %lld", k, (long long)e.chunk0, total);
        const long long per_block = (e.block_bytes - 1) / kGroupChunk + 1;
        AFCM_REQUIRE(per_block < (1ll << 31) / batch, "group_expand: %d blocks of %lld bytes exceed the grid", batch, (long long)e.block_bytes);
        total += per_block * batch;
        AFCM_REQUIRE(total < (1ll << 31), "group_expand: %lld workgroups exceed the grid", total);
    }
    hipLaunchKernelGGL(group_expand_kernel, dim3((unsigned)total), dim3(kGroupLanes), 0, (hipStream_t)stream, table_dev, n, (int)batch,
                       (const int*)groups);
    return hip_status(hipGetLastError());
}
