// The training log on the device: what a replayed training graph leaves behind for the host to read once per epoch.
//   grad_stats_kernel        what the scrub of adam_multi_kernel (optim.hip) is about to see, per chunk of its pointer table: the sum of squares of the
//                            finite scaled gradients and the counts of NaN, +inf and -inf among them.  Reads g only.
//   trainlog_append_kernel   one workgroup: adds the per-chunk rows of the generator's and the discriminator's table, and writes ONE row of
//                            AFCM_TRAINLOG_COLS doubles -- serial, schedule block, step counts, the five losses, the two sets of four statistics --
//                            into a ring at head % capacity; then head += 1.
// No atomics anywhere: every sum has ONE stated order (below), so a row is the same bits from launch to launch, in a graph and out of one.  The
// reference reads its losses on the host every print_freq images (train.py, models/pix2pix_model.py:75 names them); its scrub
// (models/stylegan3_model.py:122-124,132-134) says nothing about what it replaced.
#include "common.h"

namespace afcm {

// The tree both kernels end with: 256 values in LDS, s[t] += s[t + o] for o = 128, 64, 32, 16, 8, 4, 2, 1 (threads t < o), a barrier after each;
// s[0] is the sum.  ((((s0 + s128) + (s64 + s192)) + ...: the pairing is fixed by the thread index alone.)
template <int COLS> __device__ __forceinline__ void tree256(double (*sh)[256], int t) {
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int c = 0; c < COLS; c++) sh[c][t] += sh[c][t + o];
        }
        __syncthreads();
    }
}

// Order of the sum of squares of one chunk (the restatement in tests/trainlog_ref.py follows it):
//   1. thread t adds the squares of ITS elements in ascending index, starting from +0.0, each square formed exactly ((double)gr * (double)gr has 48
//      significant bits) and added in double.  Its elements are adam_multi_kernel's: with a 16-byte-aligned g, elements base + 4 t + 1024 k + {0..3},
//      k = 0, 1, ...; otherwise base + t + 256 k.  A non-finite gr adds +0.0, which changes nothing.
//   2. tree256 over the 256 threads.
// The counts are integers: any order gives the same.  They ride one tree packed into a double each (a chunk has at most 16384 elements).
__global__ __launch_bounds__(256) void grad_stats_kernel(const afcm_adam_entry* __restrict__ table, int n, float grad_scale, double* __restrict__ partials) {
    __shared__ double sh[4][256];
    // which tensor does this chunk belong to: adam_multi_kernel's binary search over the chunk prefix (wave-uniform)
    const long long chunk = blockIdx.x;
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].chunk0 <= chunk) lo = mid; else hi = mid - 1;
    }
    const afcm_adam_entry e = table[lo];
    const long long base = (chunk - e.chunk0) * kAdamChunk;
    const long long end = min(base + (long long)kAdamChunk, (long long)e.numel);
    const float* __restrict__ g = (const float*)e.g;
    const int t = threadIdx.x;
    double s = 0.0;
    unsigned n_nan = 0, n_pos = 0, n_neg = 0;
    auto add = [&](float gg) __attribute__((always_inline)) {
        const float gr = gg * grad_scale;                                       // as adam_multi_kernel forms it: what the scrub sees
        n_nan += gr != gr;
        n_pos += gr == __builtin_inff();
        n_neg += gr == -__builtin_inff();
        const double d = (__builtin_fabsf(gr) < __builtin_inff()) ? (double)gr : 0.0;
        s += d * d;
    };
    const bool vec = ((size_t)g & 15) == 0;
    if (vec && end - base == kAdamChunk) {
        // a whole chunk: the loop below, with four 16-byte loads in flight per thread (same elements, same order)
        const float4* __restrict__ q = (const float4*)(g + base) + t;
#pragma unroll
        for (int k = 0; k < kAdamChunk / 1024; k += 4) {
            const float4 a = q[256 * k], b = q[256 * (k + 1)], c = q[256 * (k + 2)], d = q[256 * (k + 3)];
            add(a.x); add(a.y); add(a.z); add(a.w);
            add(b.x); add(b.y); add(b.z); add(b.w);
            add(c.x); add(c.y); add(c.z); add(c.w);
            add(d.x); add(d.y); add(d.z); add(d.w);
        }
    } else if (vec) {
        for (long long i = base + 4 * t; i < end; i += 4 * 256) {
            if (i + 4 <= end) {
                const float4 a = *(const float4*)(g + i);
                add(a.x); add(a.y); add(a.z); add(a.w);
            } else {
                for (long long j = i; j < end; j++) add(g[j]);
            }
        }
    } else {
        for (long long j = base + t; j < end; j += 256) add(g[j]);
    }
    sh[0][t] = s; sh[1][t] = (double)n_nan; sh[2][t] = (double)n_pos; sh[3][t] = (double)n_neg;
    tree256<4>(sh, t);
    if (t < 4) partials[chunk * 4 + t] = sh[t][0];
}

// Order of each of the eight sums over chunks (four columns of each table): thread t adds rows t, t + 256, t + 512, ... in ascending order,
// starting from +0.0; then tree256.  Row: see AFCM_TRAINLOG_COLS in the header.  head is read by every thread before the first barrier and
// written by thread 0 after the last: a plain store.
__global__ __launch_bounds__(256) void trainlog_append_kernel(double* __restrict__ log, int capacity, long long* __restrict__ head,
                                                              const double* __restrict__ block, const float* __restrict__ step_G,
                                                              const float* __restrict__ step_D, const float* __restrict__ losses,
                                                              const double* __restrict__ partials_G, long long chunks_G,
                                                              const double* __restrict__ partials_D, long long chunks_D) {
    __shared__ double sh[8][256];
    const int t = threadIdx.x;
    const long long h = head[0];
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (partials_G != nullptr) {
        for (long long r = t; r < chunks_G; r += 256) {
#pragma unroll
            for (int c = 0; c < 4; c++) a[c] += partials_G[r * 4 + c];
        }
    }
    if (partials_D != nullptr) {
        for (long long r = t; r < chunks_D; r += 256) {
#pragma unroll
            for (int c = 0; c < 4; c++) a[4 + c] += partials_D[r * 4 + c];
        }
    }
#pragma unroll
    for (int c = 0; c < 8; c++) sh[c][t] = a[c];
    tree256<8>(sh, t);
    if (t < AFCM_TRAINLOG_COLS) {
        const double nan = __builtin_nan("");
        double v;
        if (t == 0) v = (double)h;
        else if (t < 9) v = block != nullptr ? block[t - 1] : nan;
        else if (t == 9) v = step_G != nullptr ? (double)step_G[0] : nan;
        else if (t == 10) v = step_D != nullptr ? (double)step_D[0] : nan;
        else if (t < 16) v = losses != nullptr ? (double)losses[t - 11] : nan;
        else if (t < 20) v = partials_G != nullptr ? sh[t - 16][0] : nan;
        else v = partials_D != nullptr ? sh[t - 16][0] : nan;
        long long slot = h % capacity;
        if (slot < 0) slot += capacity;                                         // (a head that something else overwrote: still inside the ring)
        log[slot * AFCM_TRAINLOG_COLS + t] = v;
    }
    if (t == 0) head[0] = h + 1;
}

}  // namespace afcm

extern "C" int32_t afcm_trainlog_cols(void) { return AFCM_TRAINLOG_COLS; }

extern "C" int afcm_grad_stats(const afcm_adam_entry* table, int32_t n, int64_t total_chunks, float grad_scale, double* partials, void* stream) {
    using namespace afcm;
    AFCM_REQUIRE(table != nullptr && n > 0, "grad_stats: empty table");
    AFCM_REQUIRE(total_chunks > 0 && total_chunks < (1ll << 31), "grad_stats: %lld chunks is out of range", (long long)total_chunks);
    AFCM_REQUIRE(partials != nullptr && ((size_t)partials & 7) == 0, "grad_stats: partials must be a non-null, 8-byte-aligned pointer");
    hipLaunchKernelGGL(grad_stats_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, table, n, grad_scale, partials);
    return hip_status(hipGetLastError());
}

extern "C" int afcm_trainlog_append(double* log, int32_t capacity, int64_t* head, const double* block, const float* step_G, const float* step_D,
                                    const float* losses, const double* partials_G, int64_t chunks_G, const double* partials_D, int64_t chunks_D,
                                    void* stream) {
    using namespace afcm;
    AFCM_REQUIRE(log != nullptr && head != nullptr, "trainlog_append: null log or head");
    AFCM_REQUIRE(capacity >= 1, "trainlog_append: capacity %d is below 1", (int)capacity);
    AFCM_REQUIRE(chunks_G >= 0 && chunks_D >= 0, "trainlog_append: negative chunk count (%lld, %lld)", (long long)chunks_G, (long long)chunks_D);
    hipLaunchKernelGGL(trainlog_append_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, log, (int)capacity, (long long*)head, block, step_G, step_D,
                       losses, partials_G, (long long)chunks_G, partials_D, (long long)chunks_D);
    return hip_status(hipGetLastError());
}
