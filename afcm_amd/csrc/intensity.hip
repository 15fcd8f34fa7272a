// Intensity rescaling (the reference's data/prepare_h5.py:9-41 and evaluate.py:23-40) on the device: the two percentiles of the voxels above zero by
// an exact radix select, then the map onto grey levels 1..255.  See include/afcm_hip.h for the statement kept.
//   rs_hist_kernel   one digit of the keys, most significant first: every workgroup counts its share of the volume in LDS and stores the counts into
//                    its OWN slot of the workspace.  The first pass counts every foreground voxel into one histogram; a later pass counts, per
//                    distinct prefix the four ranks have reached, the voxels that carry that prefix (at most four histograms).
//   rs_scan_kernel   one workgroup: adds the slots, scans, picks each rank's bin, and carries prefix and residual rank forward in the state block at
//                    the head of the workspace.  The first pass's total is n, from which the ranks are formed; the last pass writes lo, hi, n.
//   rs_map_kernel    16 output bytes per thread, read as 16-byte vectors where the source run lies in one row on a 16-byte boundary.
// Keys are the raw bit patterns (foreground is positive, so they order as the values do).  Integer LDS adds only; no global atomic; no host read.
//
// Percentile clip (the reference's StandardNIIDataset.__percentile_clip, data/cmsrnii_dataset.py:79-114) runs the same three kernels on keys of
// either sign: the pc_* traits count EVERY voxel that is not a NaN under an order-preserving key (floats: -0.0 -> +0.0, then the sign bit flipped
// for non-negatives and all bits inverted for negatives; int16: biased by 32768), NaNs are counted apart in one more word of each slot, and the map
// clips to the bounds instead of rescaling the foreground.  afcm_percentile_bounds / afcm_clip_normalize below.
#include "common.h"

namespace afcm {

constexpr int RS_THREADS = 1024;
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_UNROLL = 4;
constexpr int RS_CHUNK = RS_THREADS * RS_UNROLL;      // voxels of one workgroup in one round of the grid
constexpr int RS_RANKS = 4;                           // i and i + 1 of the low percentile, i and i + 1 of the high one
constexpr int RS_MAX_PASSES = 8;
constexpr int RS_DIGIT = 8;                           // bits per digit of the 32- and 64-bit keys
constexpr int RS_WIDE_BITS = 15;                      // the one digit of a positive int16
constexpr int RS_GROUPS = 256;                        // workgroups at most (one per CU)
constexpr int RS_GROUPS_WIDE = 32;                    // ... with 2^15-bin slots, which the one scanning workgroup has to add up
constexpr int RS_MAP_THREADS = 256;
constexpr int RS_MAP_RUN = 16;

struct rs_state {                                     // the head of the workspace
    unsigned long long prefix[RS_RANKS];              // the digits found so far, most significant first
    unsigned long long rank[RS_RANKS];                // the rank among the voxels that carry the prefix
    int                group[RS_RANKS];               // the first rank with the same prefix: its histogram serves this rank too
    double             g[2];                          // the fractional part of the virtual index of each percentile
    unsigned long long n;
    unsigned long long nan;                           // percentile clip: the NaNs, which no histogram holds
};
constexpr int RS_STATE_WORDS = 64;                    // uint32 words kept for the state in front of the slots
static_assert(sizeof(rs_state) <= RS_STATE_WORDS * 4, "the state block outgrew its place");

struct rs_plan {
    int groups, passes, slot_words;
    int bits[RS_MAX_PASSES];
};

static int plan_groups(long long n, int cap) {
    const long long want = (n + RS_CHUNK - 1) / RS_CHUNK;
    return (int)(want < 1 ? 1 : (want > cap ? cap : want));
}

// Signed keys use every bit: 8 / 16 / 32 / 64 of them in 8-bit digits.  int16 takes two passes, since the 2^16 bins of one would be 256 KB of LDS.
// In the first pass word 256 of a slot, which no 8-bit histogram reaches, takes the workgroup's NaN count.
static rs_plan make_signed_plan(long long n, int dtype) {
    rs_plan p = {};
    const int key_bits = dtype == AFCM_SRC_U8 ? 8 : (dtype == AFCM_SRC_I16 ? 16 : (dtype == AFCM_SRC_F32 ? 32 : 64));
    for (int left = key_bits; left > 0; left -= RS_DIGIT) p.bits[p.passes++] = RS_DIGIT;
    p.slot_words = RS_RANKS << RS_DIGIT;
    p.groups = plan_groups(n, RS_GROUPS);
    return p;
}

static rs_plan make_plan(long long n, int dtype) {
    rs_plan p = {};
    if (dtype == AFCM_SRC_U8) p.bits[p.passes++] = 8;
    else if (dtype == AFCM_SRC_I16) p.bits[p.passes++] = RS_WIDE_BITS;
    else {
        const int key_bits = dtype == AFCM_SRC_F32 ? 31 : 63;   // the sign bit of a foreground key is clear
        for (int left = key_bits; left > 0; left -= RS_DIGIT) p.bits[p.passes++] = left < RS_DIGIT ? left : RS_DIGIT;
    }
    const int first = 1 << p.bits[0];
    p.slot_words = p.passes == 1 ? first : (first > RS_RANKS << RS_DIGIT ? first : RS_RANKS << RS_DIGIT);
    p.groups = plan_groups(n, dtype == AFCM_SRC_I16 ? RS_GROUPS_WIDE : RS_GROUPS);
    return p;
}

// Per source type: how it is read, which bit patterns are above zero, the key, and the key widened exactly to double.  nan_word: what fg()
// turns away is counted apart in the first pass (the signed traits below; nothing here).
struct rs_u8 {
    typedef uint8_t raw;
    typedef uint32_t key_t;
    static constexpr int first_words = RS_WAVES << 8;
    static constexpr bool nan_word = false;
    __device__ static __forceinline__ bool fg(raw v) { return v != 0; }
    __device__ static __forceinline__ key_t key(raw v) { return v; }
    __device__ static __forceinline__ double value(unsigned long long k) { return (double)(uint32_t)k; }
};
struct rs_i16 {
    typedef int16_t raw;
    typedef uint32_t key_t;
    static constexpr int first_words = 1 << RS_WIDE_BITS;
    static constexpr bool nan_word = false;
    __device__ static __forceinline__ bool fg(raw v) { return v > 0; }
    __device__ static __forceinline__ key_t key(raw v) { return (uint32_t)v; }
    __device__ static __forceinline__ double value(unsigned long long k) { return (double)(uint32_t)k; }
};
struct rs_f32 {                                       // above zero: 0 < bits <= the bits of +inf (NaNs lie above, negatives have the sign bit)
    typedef uint32_t raw;
    typedef uint32_t key_t;
    static constexpr int first_words = RS_WAVES << RS_DIGIT;
    static constexpr bool nan_word = false;
    __device__ static __forceinline__ bool fg(raw v) { return v - 1u < 0x7f800000u; }
    __device__ static __forceinline__ key_t key(raw v) { return v; }
    __device__ static __forceinline__ double value(unsigned long long k) { return (double)__uint_as_float((uint32_t)k); }
};
struct rs_f64 {
    typedef unsigned long long raw;
    typedef unsigned long long key_t;
    static constexpr int first_words = RS_WAVES << RS_DIGIT;
    static constexpr bool nan_word = false;
    __device__ static __forceinline__ bool fg(raw v) { return v - 1ull < 0x7ff0000000000000ull; }
    __device__ static __forceinline__ key_t key(raw v) { return v; }
    __device__ static __forceinline__ double value(unsigned long long k) { return __longlong_as_double((long long)k); }
};

// The signed traits of the percentile clip: fg() is "not a NaN", the key orders values of either sign, value() undoes it, widen() is the voxel
// itself as a double (the map needs no key).
struct pc_u8 {
    typedef uint8_t raw;
    typedef uint32_t key_t;
    static constexpr int first_words = RS_WAVES << RS_DIGIT;
    static constexpr bool nan_word = false;
    __device__ static __forceinline__ bool fg(raw) { return true; }
    __device__ static __forceinline__ key_t key(raw v) { return v; }
    __device__ static __forceinline__ double value(unsigned long long k) { return (double)(uint32_t)k; }
    __device__ static __forceinline__ double widen(raw v) { return (double)v; }
};
struct pc_i16 {
    typedef int16_t raw;
    typedef uint32_t key_t;
    static constexpr int first_words = RS_WAVES << RS_DIGIT;
    static constexpr bool nan_word = false;
    __device__ static __forceinline__ bool fg(raw) { return true; }
    __device__ static __forceinline__ key_t key(raw v) { return (uint32_t)((int)v + 32768); }
    __device__ static __forceinline__ double value(unsigned long long k) { return (double)((int)(uint32_t)k - 32768); }
    __device__ static __forceinline__ double widen(raw v) { return (double)v; }
};
struct pc_f32 {
    typedef uint32_t raw;
    typedef uint32_t key_t;
    static constexpr int first_words = RS_WAVES << RS_DIGIT;
    static constexpr bool nan_word = true;
    __device__ static __forceinline__ bool fg(raw v) { return (v & 0x7fffffffu) <= 0x7f800000u; }
    __device__ static __forceinline__ key_t key(raw v) {
        if (v == 0x80000000u) v = 0u;                                   // -0.0 and +0.0 are one key
        return (v & 0x80000000u) ? ~v : v | 0x80000000u;
    }
    __device__ static __forceinline__ double value(unsigned long long k) {
        const uint32_t u = (uint32_t)k;
        return (double)__uint_as_float((u & 0x80000000u) ? u ^ 0x80000000u : ~u);
    }
    __device__ static __forceinline__ double widen(raw v) { return (double)__uint_as_float(v); }
};
struct pc_f64 {
    typedef unsigned long long raw;
    typedef unsigned long long key_t;
    static constexpr int first_words = RS_WAVES << RS_DIGIT;
    static constexpr bool nan_word = true;
    __device__ static __forceinline__ bool fg(raw v) { return (v & 0x7fffffffffffffffull) <= 0x7ff0000000000000ull; }
    __device__ static __forceinline__ key_t key(raw v) {
        if (v == 0x8000000000000000ull) v = 0ull;
        return (v >> 63) ? ~v : v | 0x8000000000000000ull;
    }
    __device__ static __forceinline__ double value(unsigned long long k) { return __longlong_as_double((long long)((k >> 63) ? k ^ 0x8000000000000000ull : ~k)); }
    __device__ static __forceinline__ double widen(raw v) { return __longlong_as_double((long long)v); }
};

// element e of the [D, H, W] volume: rows contiguous, slices stride_z apart
__device__ __forceinline__ long long rs_offset(unsigned e, unsigned hw, long long stride_z, bool flat) {
    return flat ? (long long)e : (long long)(e / hw) * stride_z + (long long)(e % hw);
}

template <typename TR, bool FIRST>
__global__ __launch_bounds__(RS_THREADS) void rs_hist_kernel(const typename TR::raw* __restrict__ src, unsigned n_total, unsigned hw, long long stride_z,
                                                             int flat, uint32_t* __restrict__ ws, int slot_words, int shift, int bits) {
    typedef typename TR::key_t key_t;
    constexpr int WORDS = FIRST ? TR::first_words : RS_RANKS << RS_DIGIT;
    constexpr bool NANS = FIRST && TR::nan_word;                        // hist[WORDS]: the NaNs this workgroup met
    __shared__ uint32_t hist[WORDS + (NANS ? 1 : 0)];
    const int tid = threadIdx.x, nb = 1 << bits;
    // first pass, contended top digit (a float's exponent): every wave counts into a histogram of its own where 16 of them fit
    const bool per_wave = FIRST && nb * RS_WAVES <= WORDS;
    const int used = FIRST ? (per_wave ? nb * RS_WAVES : nb) : RS_RANKS * nb;
    for (int i = tid; i < used; i += RS_THREADS) hist[i] = 0;
    if (NANS && tid == 0) hist[WORDS] = 0;
    key_t prefix[RS_RANKS];
    bool lead[RS_RANKS];
    if (!FIRST) {
        const rs_state* st = (const rs_state*)ws;
#pragma unroll
        for (int r = 0; r < RS_RANKS; ++r) {
            prefix[r] = (key_t)st->prefix[r];
            lead[r] = st->group[r] == r;
        }
    }
    __syncthreads();
    uint32_t* mine = hist + (per_wave ? (tid >> 6) * nb : 0);
    const key_t mask = (key_t)(nb - 1);
    for (unsigned long long base = (unsigned long long)blockIdx.x * RS_CHUNK; base < n_total; base += (unsigned long long)gridDim.x * RS_CHUNK) {
        typename TR::raw v[RS_UNROLL];
        bool in[RS_UNROLL];
#pragma unroll
        for (int j = 0; j < RS_UNROLL; ++j) {
            const unsigned long long e = base + (unsigned)(j * RS_THREADS + tid);
            in[j] = e < n_total;
            v[j] = in[j] ? src[rs_offset((unsigned)e, hw, stride_z, flat != 0)] : (typename TR::raw)0;
        }
#pragma unroll
        for (int j = 0; j < RS_UNROLL; ++j) {
            if (!in[j]) continue;
            if (!TR::fg(v[j])) {
                if (NANS) atomicAdd(&hist[WORDS], 1u);
                continue;
            }
            const key_t k = TR::key(v[j]);
            const int digit = (int)((k >> shift) & mask);
            if (FIRST) {
                atomicAdd(&mine[digit], 1u);
            } else {
                const key_t top = k >> (shift + bits);
#pragma unroll
                for (int r = 0; r < RS_RANKS; ++r)
                    if (lead[r] && top == prefix[r]) {
                        atomicAdd(&hist[r * nb + digit], 1u);
                        break;
                    }
            }
        }
    }
    __syncthreads();
    uint32_t* slot = ws + RS_STATE_WORDS + (size_t)blockIdx.x * slot_words;
    if (FIRST) {
        for (int b = tid; b < nb; b += RS_THREADS) {
            uint32_t s = hist[b];
            if (per_wave)
                for (int wv = 1; wv < RS_WAVES; ++wv) s += hist[wv * nb + b];
            slot[b] = s;
        }
        if (NANS && tid == 0) slot[nb] = hist[WORDS];
    } else {
        for (int i = tid; i < RS_RANKS * nb; i += RS_THREADS) slot[i] = hist[i];
    }
}

// numpy's `linear` percentile with its _lerp; every product and sum rounded on its own
__device__ __forceinline__ double rs_lerp(double a, double b, double g) {
    const double d = b - a;
    return g >= 0.5 ? b - d * (1.0 - g) : a + d * g;
}

template <typename TR>
__device__ __forceinline__ void rs_finish(const unsigned long long* key, const double* g, unsigned long long n, double* stats) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    stats[0] = n ? rs_lerp(TR::value(key[0]), TR::value(key[1]), g[0]) : nan;
    stats[1] = n ? rs_lerp(TR::value(key[2]), TR::value(key[3]), g[1]) : nan;
    stats[2] = (double)n;
}

// The percentile clip's bounds: n counts the voxels that are not NaN; one NaN makes both bounds NaN, as numpy's partition-and-check does.
template <typename TR>
__device__ __forceinline__ void pc_finish(const unsigned long long* key, const double* g, unsigned long long n, unsigned long long nans,
                                          int strictly_positive, double* stats) {
    double lo = __longlong_as_double(0x7ff8000000000000ll), hi = lo;
    if (n && !nans) {
        lo = rs_lerp(TR::value(key[0]), TR::value(key[1]), g[0]);
        hi = rs_lerp(TR::value(key[2]), TR::value(key[3]), g[1]);
        if (strictly_positive && lo < 0.0) lo = 0.0;
    }
    stats[0] = lo;
    stats[1] = hi;
    stats[2] = (double)(n + nans);
    stats[3] = (double)nans;
}

// mode: RS_FOREGROUND (rs_* traits, stats[0..2]) or the percentile clip's RS_CLIP / RS_CLIP_POSITIVE (pc_* traits, the NaN word, stats[0..3])
constexpr int RS_FOREGROUND = 0, RS_CLIP = 1, RS_CLIP_POSITIVE = 2;

template <int WORDS>
__global__ __launch_bounds__(RS_THREADS) void rs_scan_kernel(uint32_t* __restrict__ ws, int groups, int slot_words, int pass, int bits, int last,
                                                             int dtype, int mode, double q_lo, double q_hi, double* __restrict__ stats) {
    __shared__ uint32_t tot[WORDS];
    __shared__ uint32_t sc[RS_THREADS];
    __shared__ rs_state s;
    __shared__ unsigned long long new_prefix[RS_RANKS], new_rank[RS_RANKS];
    const int tid = threadIdx.x, nb = 1 << bits, nh = pass == 0 ? 1 : RS_RANKS;
    const uint32_t* slots = ws + RS_STATE_WORDS;
    const bool nans = pass == 0 && mode != RS_FOREGROUND && dtype >= AFCM_SRC_F32;      // word nb of every slot: added up like one more bin
    for (int e = tid; e < nh * nb + (nans ? 1 : 0); e += RS_THREADS) {        // unrolled: the loads of 16 slots are in flight together (one by one this loop was the op's time)
        uint32_t t = 0;
#pragma unroll 16
        for (int gi = 0; gi < groups; ++gi) t += slots[(size_t)gi * slot_words + e];
        tot[e] = t;
    }
    __syncthreads();
    // `seg` threads per histogram, each owning `per` neighbouring bins; an inclusive scan of the owners' sums inside each segment
    const int seg = nb < RS_THREADS / nh ? nb : RS_THREADS / nh, per = nb / seg;
    const int hh = tid / seg, j = tid % seg;
    const bool active = hh < nh;
    uint32_t own = 0;
    if (active)
        for (int k = 0; k < per; ++k) own += tot[hh * nb + j * per + k];
    sc[tid] = own;
    __syncthreads();
    for (int off = 1; off < seg; off <<= 1) {
        const uint32_t add = j >= off ? sc[tid - off] : 0u;
        __syncthreads();
        sc[tid] += add;
        __syncthreads();
    }
    if (tid == 0) {
        if (pass == 0) {                                  // n and, from it, the four ranks
            const unsigned long long n = sc[seg - 1];
            s.n = n;
            s.nan = nans ? tot[nb] : 0;
            const double q[2] = {q_lo, q_hi};
            for (int p = 0; p < 2; ++p) {
                unsigned long long i = 0, i1 = 0;
                double g = 0.0;
                if (n) {
                    const double vi = q[p] * (double)(n - 1);
                    const double fl = floor(vi);
                    g = vi - fl;
                    i = (unsigned long long)fl;
                    if (i > n - 1) i = n - 1;             // q <= 1 keeps vi <= n - 1; only a guard
                    i1 = i + 1 < n - 1 ? i + 1 : n - 1;
                }
                s.g[p] = g;
                s.rank[2 * p] = i;
                s.rank[2 * p + 1] = i1;
            }
            for (int r = 0; r < RS_RANKS; ++r) { s.prefix[r] = 0; s.group[r] = 0; }
        } else {
            s = *(const rs_state*)ws;
        }
        for (int r = 0; r < RS_RANKS; ++r) {              // what an empty foreground leaves: bin 0, rank 0
            new_prefix[r] = s.prefix[r] << bits;
            new_rank[r] = 0;
        }
    }
    __syncthreads();
    if (active) {
        const unsigned long long incl = sc[tid], excl = incl - own;
#pragma unroll
        for (int r = 0; r < RS_RANKS; ++r) {
            const unsigned long long want = s.rank[r];
            if (hh == (pass == 0 ? 0 : s.group[r]) && excl <= want && want < incl) {
                unsigned long long c = excl;
                for (int k = 0; k < per; ++k) {
                    const uint32_t cnt = tot[hh * nb + j * per + k];
                    if (want < c + cnt) {
                        new_prefix[r] = (s.prefix[r] << bits) | (unsigned long long)(j * per + k);
                        new_rank[r] = want - c;
                        break;
                    }
                    c += cnt;
                }
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        rs_state* st = (rs_state*)ws;
        for (int r = 0; r < RS_RANKS; ++r) {
            int first = r;
            for (int o = r - 1; o >= 0; --o)
                if (new_prefix[o] == new_prefix[r]) first = o;
            st->prefix[r] = new_prefix[r];
            st->rank[r] = new_rank[r];
            st->group[r] = first;
        }
        st->g[0] = s.g[0];
        st->g[1] = s.g[1];
        st->n = s.n;
        st->nan = s.nan;
        if (last && mode != RS_FOREGROUND) {
            const int sp = mode == RS_CLIP_POSITIVE;
            if (dtype == AFCM_SRC_U8) pc_finish<pc_u8>(new_prefix, s.g, s.n, s.nan, sp, stats);
            else if (dtype == AFCM_SRC_I16) pc_finish<pc_i16>(new_prefix, s.g, s.n, s.nan, sp, stats);
            else if (dtype == AFCM_SRC_F32) pc_finish<pc_f32>(new_prefix, s.g, s.n, s.nan, sp, stats);
            else pc_finish<pc_f64>(new_prefix, s.g, s.n, s.nan, sp, stats);
        } else if (last) {
            if (dtype == AFCM_SRC_U8) rs_finish<rs_u8>(new_prefix, s.g, s.n, stats);
            else if (dtype == AFCM_SRC_I16) rs_finish<rs_i16>(new_prefix, s.g, s.n, stats);
            else if (dtype == AFCM_SRC_F32) rs_finish<rs_f32>(new_prefix, s.g, s.n, stats);
            else rs_finish<rs_f64>(new_prefix, s.g, s.n, stats);
        }
    }
}

// One foreground voxel -> its grey level: clip(rint((v - lo) / (hi - lo) * 255), 1, 255), a NaN (hi == lo at v == lo, inf / inf) -> 1
__device__ __forceinline__ uint8_t rs_level(double v, double lo, double range) {
    const double r = rint((v - lo) / range * 255.0);
    return !(r >= 1.0) ? (uint8_t)1 : (r > 255.0 ? (uint8_t)255 : (uint8_t)r);
}

// Percentile clip, one voxel: trunc((min(max(v, lo), hi) - lo) / (hi - lo) * 255) with numpy's minimum / maximum (a NaN voxel stays one, and
// lo > hi -- strictly_positive over an all-negative reference -- gives hi); a NaN result (NaN bounds, hi == lo, inf / inf) -> 0
__device__ __forceinline__ uint8_t pc_level(double v, double lo, double hi, double range) {
    double t = v < lo ? lo : v;
    t = t > hi ? hi : t;
    const double r = (t - lo) / range * 255.0;
    return !(r >= 0.0) ? (uint8_t)0 : (uint8_t)(int)r;                 // t lies between the bounds, so r <= 255
}

// Item 0 is the `head` bytes up to the output's first 16-byte boundary (a whole run when it starts on one); item k >= 1 the k-th run after it.
// CLIP: TR is a pc_* trait and every voxel goes through pc_level; otherwise the foreground goes through rs_level.
template <typename TR, bool CLIP>
__global__ __launch_bounds__(RS_MAP_THREADS) void rs_map_kernel(uint8_t* __restrict__ out, const typename TR::raw* __restrict__ src,
                                                                const double* __restrict__ stats, unsigned n_total, unsigned hw, long long stride_z,
                                                                int flat, unsigned head, unsigned items) {
    typedef typename TR::raw raw;
    const unsigned k = blockIdx.x * RS_MAP_THREADS + threadIdx.x;
    if (k >= items) return;
    const unsigned long long e0l = k == 0 ? 0ull : (unsigned long long)head + (unsigned long long)(k - 1) * RS_MAP_RUN;
    if (e0l >= n_total) return;
    const unsigned e0 = (unsigned)e0l;
    const unsigned want = k == 0 ? head : (unsigned)RS_MAP_RUN;
    const unsigned cnt = n_total - e0 < want ? n_total - e0 : want;
    const double lo = stats[0], hi = stats[1], range = hi - lo;
    const bool full = cnt == RS_MAP_RUN;
    union {
        raw v[RS_MAP_RUN];
        uint4 q[sizeof(raw)];
    } in;
    const long long off0 = rs_offset(e0, hw, stride_z, flat != 0);
    const bool one_run = flat || (e0 % hw) + RS_MAP_RUN <= hw;          // rows follow each other inside a slice
    if (full && one_run && ((uintptr_t)(src + off0) & 15) == 0) {
        const uint4* p = (const uint4*)(src + off0);
#pragma unroll
        for (int i = 0; i < (int)sizeof(raw); ++i) in.q[i] = p[i];
    } else {
#pragma unroll
        for (int i = 0; i < RS_MAP_RUN; ++i)
            in.v[i] = (unsigned)i < cnt ? src[rs_offset(e0 + i, hw, stride_z, flat != 0)] : (raw)0;
    }
    union {
        uint8_t b[RS_MAP_RUN];
        uint4 q;
    } o;
#pragma unroll
    for (int i = 0; i < RS_MAP_RUN; ++i) {
        if constexpr (CLIP) o.b[i] = pc_level(TR::widen(in.v[i]), lo, hi, range);
        else o.b[i] = TR::fg(in.v[i]) ? rs_level(TR::value(TR::key(in.v[i])), lo, range) : (uint8_t)0;
    }
    if (full && ((uintptr_t)(out + e0) & 15) == 0) {
        *(uint4*)(out + e0) = o.q;
    } else {
#pragma unroll
        for (int i = 0; i < RS_MAP_RUN; ++i)
            if ((unsigned)i < cnt) out[e0 + i] = o.b[i];
    }
}

// The select: `passes` histogram launches on the source, each followed by the one-workgroup scan; the last scan writes `stats`.
template <typename TR>
static int launch_select(double* stats, uint32_t* ws, const void* volume, int dtype, int mode, const rs_plan& plan, unsigned n, unsigned hw,
                         long long stride_z, int flat, double q_lo, double q_hi, hipStream_t s) {
    const typename TR::raw* src = (const typename TR::raw*)volume;
    const dim3 grid(plan.groups), block(RS_THREADS);
    int shift = 0;
    for (int p = 0; p < plan.passes; ++p) shift += plan.bits[p];
    for (int p = 0; p < plan.passes; ++p) {
        const int bits = plan.bits[p];
        shift -= bits;
        if (p == 0)
            hipLaunchKernelGGL((rs_hist_kernel<TR, true>), grid, block, 0, s, src, n, hw, stride_z, flat, ws, plan.slot_words, shift, bits);
        else
            hipLaunchKernelGGL((rs_hist_kernel<TR, false>), grid, block, 0, s, src, n, hw, stride_z, flat, ws, plan.slot_words, shift, bits);
        const int last = p == plan.passes - 1;
        if (bits > RS_DIGIT + 2)
            hipLaunchKernelGGL((rs_scan_kernel<(1 << RS_WIDE_BITS)>), dim3(1), block, 0, s, ws, plan.groups, plan.slot_words, p, bits, last, dtype, mode,
                               q_lo, q_hi, stats);
        else
            hipLaunchKernelGGL((rs_scan_kernel<(RS_RANKS << RS_DIGIT)>), dim3(1), block, 0, s, ws, plan.groups, plan.slot_words, p, bits, last, dtype,
                               mode, q_lo, q_hi, stats);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_status(e);
    }
    return AFCM_OK;
}

template <typename TR, bool CLIP>
static int launch_map(uint8_t* out, const double* stats, const void* volume, unsigned n, unsigned hw, long long stride_z, int flat, hipStream_t s) {
    const unsigned head = RS_MAP_RUN - (unsigned)((uintptr_t)out & (RS_MAP_RUN - 1));
    const unsigned items = 1 + (n > head ? (n - head + RS_MAP_RUN - 1) / RS_MAP_RUN : 0);
    hipLaunchKernelGGL((rs_map_kernel<TR, CLIP>), dim3((items + RS_MAP_THREADS - 1) / RS_MAP_THREADS), dim3(RS_MAP_THREADS), 0, s, out,
                       (const typename TR::raw*)volume, stats, n, hw, stride_z, flat, head, items);
    return hip_status(hipGetLastError());
}

template <typename TR>
static int launch_rescale(uint8_t* out, double* stats, uint32_t* ws, const void* volume, int dtype, const rs_plan& plan, unsigned n, unsigned hw,
                          long long stride_z, int flat, double q_lo, double q_hi, hipStream_t s) {
    const int rc = launch_select<TR>(stats, ws, volume, dtype, RS_FOREGROUND, plan, n, hw, stride_z, flat, q_lo, q_hi, s);
    return rc != AFCM_OK ? rc : launch_map<TR, false>(out, stats, volume, n, hw, stride_z, flat, s);
}

}  // namespace afcm

static bool rs_shape_ok(int64_t n, int32_t src_dtype) { return n >= 1 && n < (1ll << 31) && src_dtype >= AFCM_SRC_U8 && src_dtype <= AFCM_SRC_F64; }

static int rs_write_plan(const afcm::rs_plan& p, int32_t* plan) {
    plan[0] = p.groups;
    plan[1] = afcm::RS_CHUNK;
    plan[2] = p.passes;
    for (int i = 0; i < afcm::RS_MAX_PASSES; ++i) plan[3 + i] = p.bits[i];
    return AFCM_OK;
}

extern "C" int afcm_rescale_plan(int64_t n, int32_t src_dtype, int32_t* plan) {
    using namespace afcm;
    AFCM_REQUIRE(plan != nullptr, "rescale_plan: null plan");
    AFCM_REQUIRE(rs_shape_ok(n, src_dtype), "rescale_plan: %lld voxels of source dtype %d: 1 <= N < 2^31 and AFCM_SRC_U8 / I16 / F32 / F64", (long long)n,
                 src_dtype);
    return rs_write_plan(make_plan(n, src_dtype), plan);
}

extern "C" int64_t afcm_rescale_workspace_bytes(int64_t n, int32_t src_dtype) {
    using namespace afcm;
    if (!rs_shape_ok(n, src_dtype)) return 0;
    const rs_plan p = make_plan(n, src_dtype);
    return 4ll * (RS_STATE_WORDS + (long long)p.groups * p.slot_words);
}

extern "C" int afcm_rescale_intensity(uint8_t* out, double* stats, void* workspace, const void* volume, int32_t src_dtype, int32_t depth, int32_t h,
                                      int32_t w, int64_t src_stride_z, double q_lo, double q_hi, void* stream) {
    using namespace afcm;
    AFCM_REQUIRE(out != nullptr && stats != nullptr && workspace != nullptr && volume != nullptr, "rescale_intensity: null output, stats, workspace or volume");
    AFCM_REQUIRE(src_dtype >= AFCM_SRC_U8 && src_dtype <= AFCM_SRC_F64, "rescale_intensity: source dtype %d is not AFCM_SRC_U8 / I16 / F32 / F64", src_dtype);
    AFCM_REQUIRE(depth > 0 && h > 0 && w > 0, "rescale_intensity: volume [%d, %d, %d]: every extent must be positive", depth, h, w);
    const long long n = (long long)depth * h * w;
    AFCM_REQUIRE(n < (1ll << 31), "rescale_intensity: %lld voxels; a volume must have fewer than 2^31", n);
    AFCM_REQUIRE(src_stride_z >= 0, "rescale_intensity: source z stride %lld is negative", (long long)src_stride_z);
    AFCM_REQUIRE(q_lo >= 0.0 && q_lo <= q_hi && q_hi <= 1.0, "rescale_intensity: percentile fractions %g, %g: 0 <= q_lo <= q_hi <= 1", q_lo, q_hi);
    AFCM_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)stats & 7) == 0, "rescale_intensity: workspace and stats must be 8-byte aligned");
    const rs_plan plan = make_plan(n, src_dtype);
    const unsigned hw = (unsigned)h * (unsigned)w;
    const int flat = src_stride_z == (long long)hw;
    hipStream_t s = (hipStream_t)stream;
    uint32_t* ws = (uint32_t*)workspace;
    switch (src_dtype) {
        case AFCM_SRC_U8:
            return launch_rescale<rs_u8>(out, stats, ws, volume, src_dtype, plan, (unsigned)n, hw, src_stride_z, flat, q_lo, q_hi, s);
        case AFCM_SRC_I16:
            return launch_rescale<rs_i16>(out, stats, ws, volume, src_dtype, plan, (unsigned)n, hw, src_stride_z, flat, q_lo, q_hi, s);
        case AFCM_SRC_F32:
            return launch_rescale<rs_f32>(out, stats, ws, volume, src_dtype, plan, (unsigned)n, hw, src_stride_z, flat, q_lo, q_hi, s);
        default:
            return launch_rescale<rs_f64>(out, stats, ws, volume, src_dtype, plan, (unsigned)n, hw, src_stride_z, flat, q_lo, q_hi, s);
    }
}

// ---- percentile clip ----

extern "C" int afcm_percentile_plan(int64_t n, int32_t src_dtype, int32_t* plan) {
    using namespace afcm;
    AFCM_REQUIRE(plan != nullptr, "percentile_plan: null plan");
    AFCM_REQUIRE(rs_shape_ok(n, src_dtype), "percentile_plan: %lld voxels of source dtype %d: 1 <= N < 2^31 and AFCM_SRC_U8 / I16 / F32 / F64", (long long)n,
                 src_dtype);
    return rs_write_plan(make_signed_plan(n, src_dtype), plan);
}

extern "C" int64_t afcm_percentile_workspace_bytes(int64_t n, int32_t src_dtype) {
    using namespace afcm;
    if (!rs_shape_ok(n, src_dtype)) return 0;
    const rs_plan p = make_signed_plan(n, src_dtype);
    return 4ll * (RS_STATE_WORDS + (long long)p.groups * p.slot_words);
}

// what both entry points ask of a volume; `what` names the caller
static int pc_check_volume(const char* what, int32_t src_dtype, int32_t depth, int32_t h, int32_t w, int64_t src_stride_z) {
    AFCM_REQUIRE(src_dtype >= AFCM_SRC_U8 && src_dtype <= AFCM_SRC_F64, "%s: source dtype %d is not AFCM_SRC_U8 / I16 / F32 / F64", what, src_dtype);
    AFCM_REQUIRE(depth > 0 && h > 0 && w > 0, "%s: volume [%d, %d, %d]: every extent must be positive", what, depth, h, w);
    const long long n = (long long)depth * h * w;
    AFCM_REQUIRE(n < (1ll << 31), "%s: %lld voxels; a volume must have fewer than 2^31", what, n);
    AFCM_REQUIRE(src_stride_z >= 0, "%s: source z stride %lld is negative", what, (long long)src_stride_z);
    return AFCM_OK;
}

extern "C" int afcm_percentile_bounds(double* stats, void* workspace, const void* volume, int32_t src_dtype, int32_t depth, int32_t h, int32_t w,
                                      int64_t src_stride_z, double q_lo, double q_hi, int32_t strictly_positive, void* stream) {
    using namespace afcm;
    AFCM_REQUIRE(stats != nullptr && workspace != nullptr && volume != nullptr, "percentile_bounds: null stats, workspace or volume");
    const int rc = pc_check_volume("percentile_bounds", src_dtype, depth, h, w, src_stride_z);
    if (rc != AFCM_OK) return rc;
    AFCM_REQUIRE(q_lo >= 0.0 && q_lo <= q_hi && q_hi <= 1.0, "percentile_bounds: percentile fractions %g, %g: 0 <= q_lo <= q_hi <= 1", q_lo, q_hi);
    AFCM_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)stats & 7) == 0, "percentile_bounds: workspace and stats must be 8-byte aligned");
    const long long n = (long long)depth * h * w;
    const rs_plan plan = make_signed_plan(n, src_dtype);
    const unsigned hw = (unsigned)h * (unsigned)w;
    const int flat = src_stride_z == (long long)hw, mode = strictly_positive ? RS_CLIP_POSITIVE : RS_CLIP;
    hipStream_t s = (hipStream_t)stream;
    uint32_t* ws = (uint32_t*)workspace;
    switch (src_dtype) {
        case AFCM_SRC_U8:
            return launch_select<pc_u8>(stats, ws, volume, src_dtype, mode, plan, (unsigned)n, hw, src_stride_z, flat, q_lo, q_hi, s);
        case AFCM_SRC_I16:
            return launch_select<pc_i16>(stats, ws, volume, src_dtype, mode, plan, (unsigned)n, hw, src_stride_z, flat, q_lo, q_hi, s);
        case AFCM_SRC_F32:
            return launch_select<pc_f32>(stats, ws, volume, src_dtype, mode, plan, (unsigned)n, hw, src_stride_z, flat, q_lo, q_hi, s);
        default:
            return launch_select<pc_f64>(stats, ws, volume, src_dtype, mode, plan, (unsigned)n, hw, src_stride_z, flat, q_lo, q_hi, s);
    }
}

extern "C" int afcm_clip_normalize(uint8_t* out, const double* stats, const void* volume, int32_t src_dtype, int32_t depth, int32_t h, int32_t w,
                                   int64_t src_stride_z, void* stream) {
    using namespace afcm;
    AFCM_REQUIRE(out != nullptr && stats != nullptr && volume != nullptr, "clip_normalize: null output, stats or volume");
    const int rc = pc_check_volume("clip_normalize", src_dtype, depth, h, w, src_stride_z);
    if (rc != AFCM_OK) return rc;
    AFCM_REQUIRE(((uintptr_t)stats & 7) == 0, "clip_normalize: stats must be 8-byte aligned");
    const unsigned n = (unsigned)((long long)depth * h * w), hw = (unsigned)h * (unsigned)w;
    const int flat = src_stride_z == (long long)hw;
    hipStream_t s = (hipStream_t)stream;
    switch (src_dtype) {
        case AFCM_SRC_U8:
            return launch_map<pc_u8, true>(out, stats, volume, n, hw, src_stride_z, flat, s);
        case AFCM_SRC_I16:
            return launch_map<pc_i16, true>(out, stats, volume, n, hw, src_stride_z, flat, s);
        case AFCM_SRC_F32:
            return launch_map<pc_f32, true>(out, stats, volume, n, hw, src_stride_z, flat, s);
        default:
            return launch_map<pc_f64, true>(out, stats, volume, n, hw, src_stride_z, flat, s);
    }
}
