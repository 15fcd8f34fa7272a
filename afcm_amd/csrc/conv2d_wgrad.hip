// Weight gradient of the dense KxK convolution (conv2d.hip): the fp32 kernel, the two 16-bit LDS-DMA kernels, and the split-K reductions.
#include <type_traits>

#include "conv2d_common.h"

namespace afcm {

// ---------------------------------------------------------------------------------------------
// Weight gradient: dW[o][i][r][s] = sum_n sum_{p,q} dy[n,o,p,q] * x[n,i,p+r-pad,q+s-pad]   (inputs already scaled per plane)
// GEMM with K = pixels: both operands are K-contiguous in NCHW, so the LDS images are plain row copies and the
// 3 column shifts of a tap row come from ONE 5-dword read per row (shift 0: dwords 0-3, shift 2: dwords 1-4,
// shift 1: v_alignbyte of neighbours).  One workgroup = 64 o x 64 i x all taps; 4 waves as 2(o) x 2(i), each
// wave holds KK accumulator tiles of 32x32.  K is split over workgroups by output row; partial sums go to
// a workspace [split][O][I][KK] and are summed by wgrad_reduce_kernel.
constexpr int kWgKQ = 64;        // pixels of one output row per K macro-step

struct WgradParams {
    const void* dy;   // [N, O, P, Q]
    const void* x;    // [N, I, H, W]
    float* part;      // [splits][O][I][KK]
    int N, O, I, H, W, P, Q, pad;
    int lddy, ldx;                // row pitch (elements) of dy / x; = Q / W for dense tensors.  conv2d_wgrad16g_kernel only.
    int splits, steps_per_split;  // K macro-steps = N * rowgroups * qchunks; every 64 x 64 tile gets `splits` workgroups of `steps_per_split` steps
    // conv2d_wgrad16g_kernel, r06: > 0 = splits per IMAGE (splits = N * splits_img): a split never crosses an image, so the slabs of image n are
    // its own weight gradient dW_n -- what the per-plane dot products <x[n, i], dx[n, i]> are read from (wgrad_reduce_dots_kernel)
    int splits_img;
    int qchunks;                  // ceil(Q / kWgKQ)
    int rowgroups;                // ceil(P / R)
};

// fp32 operands, one output row per K macro-step (R = 1).
template <int KS, int XOFF>
__global__ __launch_bounds__(512, 1) void conv2d_wgrad_kernel(WgradParams p) {
    constexpr int R = 1, KK = KS * KS;
    constexpr int PDY = kWgKQ + 8;                 // 72 elements per staged dy row
    constexpr int PX = kWgKQ + 24;                 // 88 elements per staged x row
    constexpr int XW = kWgKQ + 8;                  // staged x columns per row (shifts 0..KS-1, +1 alignment, rounded)
    constexpr int XR = R + KS - 1;                 // staged x rows per channel
    constexpr int DPR_DY = kWgKQ, DPR_X = XW;      // dwords per staged row
    constexpr int LDS_ONE = 64 * R * PDY + 64 * XR * PX;
    constexpr int NBUF = (LDS_ONE * (int)sizeof(float) * 2 <= 150 * 1024) ? 2 : 1;     // double-buffer when it fits the 160 KB LDS (1x1)
    __shared__ __attribute__((aligned(16))) float lds[NBUF * LDS_ONE];
    float* lds_dy = lds;
    float* lds_x = lds + 64 * R * PDY;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wo = wave & 1, wi = (wave >> 1) & 1, th = wave >> 2;     // th: which half of the chunk's pixels this wave accumulates
    const int r32 = lane & 31, h = lane >> 5;
    constexpr int NACC = KK;

    int bid = blockIdx.x;
    const int split = bid % p.splits; bid /= p.splits;
    const int ib = bid % cdiv(p.I, 64);
    const int obk = bid / cdiv(p.I, 64);
    const int o0 = obk * 64, i0 = ib * 64;

    f32x16 acc[NACC];
#pragma unroll
    for (int t = 0; t < NACC; t++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[t][e] = 0.f;

    // ---- staging maps.  Rows of 32 dwords are spread as (row = tid/32 + 8*i, dword = tid%32), so the row-dependent
    // parts of an address advance by a constant per i; the 4-dword tail of every x row is a second small map.
    constexpr int NC = DPR_DY / 32;                 // 32-dword column groups per row (2)
    constexpr int TAILD = DPR_X - 32 * NC;          // dwords of the x-row tail (8)
    static_assert(DPR_DY % 32 == 0 && TAILD > 0 && TAILD <= 8, "staging maps assume 64-pixel chunks");
    constexpr int NDY = (64 * R) / 16;              // dy rows (o * R + rr) per thread
    constexpr int NXM = (64 * XR) / 16;             // x rows (ic * XR + r), main 32*NC dwords
    constexpr int NXT = cdiv(64 * XR * TAILD, 512); // x tail
    const int rb = tid >> 5, dlane = tid & 31;
    unsigned rdy[NDY][NC], rxm[NXM][NC], rxt[NXT];
    // Loads are raw buffer loads: an invalid element (padding row / column, channel past the end) gets the byte offset
    // kOob >= num_records and reads as zero -- no branches, one v_cndmask per load.  The step-dependent part of every address
    // is wave-uniform and lives in the buffer base; the per-thread byte offsets below never change.
    constexpr unsigned kOob = 0x80000000u;
    constexpr bool ROWSAME = (16 % R == 0) && (16 % XR == 0);      // row-in-step index of a thread is the same for all its loads
    unsigned dyoff[NDY], xoff_[NXM], xtoff[NXT];
    int dyr[NDY], xr_[NXM], xtr[NXT], xtc[NXT];
#pragma unroll
    for (int i = 0; i < NDY; i++) {
        const int row = rb + 16 * i;
        const int o = o0 + row / R;
        dyr[i] = row % R;
        dyoff[i] = o < p.O ? (unsigned)(((o * p.P + dyr[i]) * p.Q + dlane) * (int)sizeof(float)) : kOob;
    }
#pragma unroll
    for (int i = 0; i < NXM; i++) {
        const int row = rb + 16 * i;
        const int ic = i0 + row / XR;
        xr_[i] = row % XR;
        xoff_[i] = ic < p.I ? (unsigned)(((ic * p.H + xr_[i]) * p.W + dlane) * (int)sizeof(float)) : kOob;
    }
#pragma unroll
    for (int i = 0; i < NXT; i++) {
        const int j = tid + i * 512;
        const int row = j / TAILD;
        const int ic = i0 + row / XR;
        xtr[i] = row % XR;
        xtc[i] = 32 * NC + j % TAILD;
        xtoff[i] = (row < 64 * XR && ic < p.I) ? (unsigned)(((ic * p.H + xtr[i]) * p.W + xtc[i]) * (int)sizeof(float)) : kOob;
    }

    const int steps_per_img = p.rowgroups * p.qchunks;
    const int s0 = split * p.steps_per_split;
    const int s1 = min(s0 + p.steps_per_split, p.N * steps_per_img);
    // (image, row group, column chunk) of the next step to load; steps are loaded in order, so this advances by carries
    int ld_n = s0 / steps_per_img;
    int ld_rg = (s0 - ld_n * steps_per_img) / p.qchunks;
    int ld_qc = s0 - ld_n * steps_per_img - ld_rg * p.qchunks;

    auto issue_loads = [&]() __attribute__((always_inline)) {
        const int prow0 = ld_rg * R, q0 = ld_qc * kWgKQ;
        const int xorg = (q0 - p.pad) & ~1;
        // uniform bases: everything that does not depend on the lane (may point before the tensor for padding rows: those
        // elements are never fetched)
        const float* dyb = (const float*)p.dy + (size_t)ld_n * p.O * p.P * p.Q + (size_t)prow0 * p.Q + q0;
        const float* xb = (const float*)p.x + (long long)ld_n * p.I * p.H * p.W + (long long)(prow0 - p.pad) * p.W + xorg;
        const __amdgpu_buffer_rsrc_t rs_dy = __builtin_amdgcn_make_buffer_rsrc((void*)dyb, 0, kOob, 0x00020000);
        const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)xb, 0, kOob, 0x00020000);
        unsigned dyrows = 0, xrows = 0;               // validity of the R / XR rows of this step
#pragma unroll
        for (int r = 0; r < R; r++) dyrows |= (unsigned)(prow0 + r < p.P) << r;
#pragma unroll
        for (int r = 0; r < XR; r++) xrows |= (unsigned)((unsigned)(prow0 + r - p.pad) < (unsigned)p.H) << r;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const int dcol = dlane + 32 * c;
            const bool dcok = q0 + dcol < p.Q;
            const bool xcok = (unsigned)(xorg + dcol) < (unsigned)p.W;
            // validity as an offset mask: 0 or kOob, OR-ed into the byte offset (kept arithmetic so that no branch is formed)
            const unsigned dym0 = (unsigned)!(dcok && ((dyrows >> dyr[0]) & 1)) << 31, xm0 = (unsigned)!(xcok && ((xrows >> xr_[0]) & 1)) << 31;
#pragma unroll
            for (int i = 0; i < NDY; i++) {
                const unsigned m = ROWSAME ? dym0 : (unsigned)!(dcok && ((dyrows >> dyr[i]) & 1)) << 31;
                rdy[i][c] = __builtin_amdgcn_raw_buffer_load_b32(rs_dy, (dyoff[i] + 32 * c * 4) | m, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < NXM; i++) {
                const unsigned m = ROWSAME ? xm0 : (unsigned)!(xcok && ((xrows >> xr_[i]) & 1)) << 31;
                rxm[i][c] = __builtin_amdgcn_raw_buffer_load_b32(rs_x, (xoff_[i] + 32 * c * 4) | m, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < NXT; i++) {
            const unsigned m = (unsigned)!(((xrows >> xtr[i]) & 1) && (unsigned)(xorg + xtc[i]) < (unsigned)p.W) << 31;
            rxt[i] = __builtin_amdgcn_raw_buffer_load_b32(rs_x, xtoff[i] | m, 0, 0);
        }
        if (++ld_qc == p.qchunks) {
            ld_qc = 0;
            if (++ld_rg == p.rowgroups) { ld_rg = 0; ld_n++; }
        }
    };
    auto write_lds = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NDY; i++)
#pragma unroll
            for (int c = 0; c < NC; c++) *(unsigned*)(lds_dy + (dyr[i] * 64 + (rb + 16 * i) / R) * PDY + dlane + 32 * c) = rdy[i][c];
#pragma unroll
        for (int i = 0; i < NXM; i++)
#pragma unroll
            for (int c = 0; c < NC; c++) *(unsigned*)(lds_x + (xr_[i] * 64 + (rb + 16 * i) / XR) * PX + dlane + 32 * c) = rxm[i][c];
#pragma unroll
        for (int i = 0; i < NXT; i++) {
            const int j = tid + i * 512;
            if (j / TAILD < 64 * XR) *(unsigned*)(lds_x + (xtr[i] * 64 + (j / TAILD) / XR) * PX + xtc[i]) = rxt[i];
        }
    };

    // Pipeline.  Double-buffered (1x1): while a wave runs the MFMAs of step s from buffer s&1, the others may already be
    // writing step s+1 into the other buffer and have step s+2's global loads in flight: one barrier per step.
    // Single-buffered (3x3): write / barrier / compute / barrier.
    if (s0 < s1) {
        issue_loads();
        write_lds();
        if (NBUF == 2 && s0 + 1 < s1) issue_loads();
    }
    __syncthreads();
    for (int step = s0; step < s1; step++) {
        constexpr int xoff = XOFF;                  // (q0 - pad) & 1 with q0 a multiple of 64: launch-wide constant
        if (NBUF == 2) {
            if (step + 1 < s1) {
                lds_dy = lds + ((step + 1 - s0) & 1) * LDS_ONE;
                lds_x = lds_dy + 64 * R * PDY;
                write_lds();                        // step+1 (its loads were issued one step ago)
                if (step + 2 < s1) issue_loads();
            }
            lds_dy = lds + ((step - s0) & 1) * LDS_ONE;
            lds_x = lds_dy + 64 * R * PDY;
        } else {
            if (step > s0) {
                __syncthreads();
                write_lds();
                __syncthreads();
            }
            if (step + 1 < s1) issue_loads();
        }
        // Both wave halves accumulate every tap; they split the 64 pixels of the chunk (th 0: first 32, th 1: last 32), so a
        // staged x row is read once per 16 pixels and feeds all KS shifts x R rows x KS tap rows.
#pragma unroll
        for (int rr = 0; rr < R; rr++)
#pragma unroll 4
            for (int kq = 0; kq < kWgKQ / 4; kq++) {
                const int k2 = th * (kWgKQ / 4) + kq;
                const float a = lds_dy[(rr * 64 + wo * 32 + r32) * PDY + 2 * k2 + h];
#pragma unroll
                for (int t = 0; t < KK; t++) {
                    const int r = t / KS, sft = t - r * KS;
                    const float b = lds_x[((rr + r) * 64 + wi * 32 + r32) * PX + 2 * k2 + h + sft + xoff];
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[t], 0, 0, 0);
                }
            }
        if (NBUF == 2) __syncthreads();            // everyone done with buffer step&1 and step+1 fully written
    }
    // ---- add the two pixel halves through LDS (the staging buffers are free now): th 1 parks its accumulators, th 0 adds
    // them and writes the partial tile D[row = o][col = i].
    if (NBUF == 1) __syncthreads();
    {
        float* red = (float*)lds;
        constexpr int TPR_CAP = (int)((size_t)NBUF * LDS_ONE / (4 * 16 * 64));     // taps per round
        constexpr int TPR = TPR_CAP < KK ? TPR_CAP : KK;
        static_assert(TPR >= 1, "LDS too small for the half-sum");
        const int wv4 = wave & 3;
#pragma unroll
        for (int t0 = 0; t0 < KK; t0 += TPR) {
            if (t0 > 0) __syncthreads();
            if (th == 1) {
#pragma unroll
                for (int t = t0; t < t0 + TPR && t < KK; t++)
#pragma unroll
                    for (int reg = 0; reg < 16; reg++) red[((wv4 * TPR + (t - t0)) * 16 + reg) * 64 + lane] = acc[t][reg];
            }
            __syncthreads();
            if (th == 0) {
#pragma unroll
                for (int t = t0; t < t0 + TPR && t < KK; t++)
#pragma unroll
                    for (int reg = 0; reg < 16; reg++) acc[t][reg] += red[((wv4 * TPR + (t - t0)) * 16 + reg) * 64 + lane];
            }
        }
    }
    if (th == 0) {
        float* out = p.part + (size_t)split * p.O * p.I * KK;
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            const int o = o0 + wo * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
            const int i = i0 + wi * 32 + r32;
            if (o < p.O && i < p.I) {
                float* dst = out + ((size_t)o * p.I + i) * KK;
#pragma unroll
                for (int t = 0; t < KK; t++) dst[t] = acc[t][reg];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// 16-bit weight gradient of a 3x3 conv with pad 0 or 1, LDS-DMA staged (a 1x1 conv has pad 0 and takes conv2d_wgrad16g_kernel).  Same
// tiling as conv2d_wgrad_kernel (64 o x 64 i x all taps per workgroup, 8 waves = 2(o) x 2(i) x 2(pixel halves)), R = 2 output rows x 64
// pixels per K step, but the operands go HBM -> LDS directly
// (buffer_load_dword ... lds): no staging VGPRs, no ds_write pass, no per-load VALU.  One wave instruction fills 64
// consecutive LDS dwords = two 128-byte rows (64 pixels of two channels), so rows cannot be padded; bank conflicts are
// avoided by an XOR swizzle of the 16-byte granules, applied on the SOURCE address of the load and again on the read:
//     granule g of row r sits at physical granule g ^ ((r >> 1) & 7)            (conflict-free for ds_read_b128's lane groups)
// LDS image of one step (NBUF of them in a ring):
//     dy  [rr 0..1][o 0..63][128 B]                                             16 KB
//     x   [xr 0..XR-1] { main [ch 0..63][128 B] (cols 0..63), tail [ch 0..63][16 B] (cols 64..71) }   XR x 9 KB
// Every piece is predicated by the buffer descriptor: rows outside the image get num_records = 0, channels past the end
// fall behind num_records, columns past the end get the out-of-range offset bit -- all of them read as zero.
typedef __attribute__((ext_vector_type(4))) int i32x4;

template <int LO, int HI, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (LO < HI) {
        f(std::integral_constant<int, LO>{});
        static_for<LO + 1, HI>(f);
    }
}

__device__ __forceinline__ void lds_dma_dword(i32x4 rsrc, unsigned voff, unsigned lds_addr) {
    // M0 carries the wave-uniform LDS destination; lane l lands at lds_addr + 4*l
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dword %1, %2, 0 offen lds" : : "s"(lds_addr), "v"(voff), "s"(rsrc));
}

// 16 bytes per lane: lane l lands at lds_addr + 16*l
__device__ __forceinline__ void lds_dma_b128(i32x4 rsrc, unsigned voff, unsigned lds_addr) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" : : "s"(lds_addr), "v"(voff), "s"(rsrc));
}

__device__ __forceinline__ i32x4 make_rsrc(const void* base, int num_records) {
    // the descriptor is wave-uniform by construction; readfirstlane pins it to SGPRs for the "s" asm operand
    const unsigned long long a = (unsigned long long)base;
    i32x4 r;
    r.x = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
    r.y = __builtin_amdgcn_readfirstlane((int)(unsigned)(a >> 32) & 0xffff);       // stride 0
    r.z = __builtin_amdgcn_readfirstlane(num_records);
    r.w = 0x00020000;
    return r;
}

template <typename T, int KS, int XOFF, int NBUF>
__global__ __launch_bounds__(512, 1) void conv2d_wgrad16_kernel(WgradParams p) {
    static_assert(sizeof(T) == 2 && KS == 3, "16-bit 3x3 only");
    constexpr int R = 2, KK = KS * KS, XR = R + KS - 1;
    constexpr int ROWB = 128;                       // bytes of one staged row (64 pixels)
    constexpr int DY_BYTES = R * 64 * ROWB;
    constexpr int XBLK = 64 * ROWB + 64 * 16;       // one staged x row of all 64 channels: main + tail
    constexpr int BUF = DY_BYTES + XR * XBLK;
    constexpr int NTAILP = (4 * XR) / 8;            // tail pieces per wave
    static_assert((4 * XR) % 8 == 0, "tail pieces must divide over the 8 waves");
    constexpr int NPIECE = 8 + 4 * XR + NTAILP;     // LDS-DMA instructions per wave and step
    __shared__ __attribute__((aligned(256))) char lds[NBUF * BUF];
    const unsigned lds0 = (unsigned)(unsigned long long)(__attribute__((address_space(3))) void*)lds;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wo = wave & 1, wi = (wave >> 1) & 1, th = wave >> 2;     // th: which half of the chunk's pixels this wave accumulates
    const int r32 = lane & 31, h = lane >> 5;

    // XCD-aware block order: the 8 XCDs take workgroups round-robin, so give XCD x a contiguous range of logical ids;
    // logical id = split-major, i.e. one XCD's L2 sees all (o, i) tiles of the same pixels.
    const int tiles_i = cdiv(p.I, 64), tiles = tiles_i * cdiv(p.O, 64);
    int bid = blockIdx.x;
    const int total = tiles * p.splits;
    bid = xcd_order(bid, total);
    const int split = bid / tiles;
    const int tile = bid - split * tiles;
    const int ib = tile % tiles_i, obk = tile / tiles_i;
    const int o0 = obk * 64, i0 = ib * 64;

    f32x16 acc[KK];
#pragma unroll
    for (int t = 0; t < KK; t++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[t][e] = 0.f;

    // ---- load maps.  Wave w owns the row pairs {w, w+8, w+16, w+24} of every 64-row block, so its swizzle key
    // ((row >> 1) & 7) == w is a constant and one per-lane offset serves all of its pieces.
    const int half = lane >> 5, slot = lane & 31;
    const int cdw = ((((slot >> 2) ^ wave) & 7) << 2) | (slot & 3);          // logical dword column of this lane's LDS slot
    const unsigned lp_dy = (unsigned)((2 * wave + half) * p.P * p.Q * 2 + cdw * 4);
    const unsigned lp_x = (unsigned)((2 * wave + half) * p.H * p.W * 2 + cdw * 4);
    const int trow = lane >> 2, tdw = lane & 3;                               // tail piece: 16 channels x 4 dwords
    const unsigned lp_t = (unsigned)(trow * p.H * p.W * 2 + (32 + tdw) * 4);

    const int steps_per_img = p.rowgroups * p.qchunks;
    const int s0 = split * p.steps_per_split;
    const int s1 = min(s0 + p.steps_per_split, p.N * steps_per_img);
    int ld_n = s0 / steps_per_img;
    int ld_rg = (s0 - ld_n * steps_per_img) / p.qchunks;
    int ld_qc = s0 - ld_n * steps_per_img - ld_rg * p.qchunks;
    int ld_buf = 0;

    // Loads of one step: begin_loads() latches the step's uniform state, issue_piece<I>() issues LDS-DMA instruction I of the
    // wave's NPIECE.  The pieces are spread between the MFMAs of the previous step's compute: a dword load occupies the
    // address unit for 16 cycles, so a burst of 26 x 8 waves would stall every wave at the head of the step.
    int c_prow0 = 0, c_q0 = 0, c_xorg = 0, c_live = 0;
    unsigned c_bufa = 0, v_dy = 0, v_x = 0, v_t = 0;
    const T* c_dyn = nullptr;
    const T* c_xn = nullptr;
    const int pq = p.P * p.Q, hw = p.H * p.W;
    auto begin_loads = [&](bool live) __attribute__((always_inline)) {
        c_live = live ? -1 : 0;                                   // a dead step still issues its pieces (with 0 records)
        c_prow0 = ld_rg * R; c_q0 = ld_qc * kWgKQ;
        c_xorg = (c_q0 - p.pad) & ~1;
        c_bufa = lds0 + ld_buf * BUF;
        // per-lane column validity -> offset masks
        v_dy = lp_dy | ((unsigned)!(c_q0 + 2 * cdw < p.Q) << 31);
        v_x = lp_x | ((unsigned)!((unsigned)(c_xorg + 2 * cdw) < (unsigned)p.W) << 31);
        v_t = lp_t | ((unsigned)!((unsigned)(c_xorg + 64 + 2 * tdw) < (unsigned)p.W) << 31);
        c_dyn = (const T*)p.dy + (size_t)ld_n * p.O * pq;
        c_xn = (const T*)p.x + (size_t)ld_n * p.I * hw;
        if (live) {
            if (++ld_qc == p.qchunks) {
                ld_qc = 0;
                if (++ld_rg == p.rowgroups) { ld_rg = 0; ld_n++; }
            }
        }
        if (++ld_buf == NBUF) ld_buf = 0;
    };
    auto issue_piece = [&](auto idx) __attribute__((always_inline)) {
        constexpr int I = decltype(idx)::value;
        if constexpr (I < 8) {
            constexpr int rr = I >> 2, mm = I & 3;
            const int ch0 = o0 + 16 * mm, row = c_prow0 + rr;
            const int inimg = row * p.Q + c_q0;                                // element offset of the piece origin inside a channel
            int nr = ((p.O - ch0) * pq - inimg) * 2;
            nr = (row < p.P && nr > 0) ? (nr & c_live) : 0;
            lds_dma_dword(make_rsrc(c_dyn + (long long)ch0 * pq + inimg, nr), v_dy, c_bufa + rr * (64 * ROWB) + (wave + 8 * mm) * 256);
        } else if constexpr (I < 8 + 4 * XR) {
            constexpr int m = I - 8, xr = m >> 2, mm = m & 3;
            const int ch0 = i0 + 16 * mm, row = c_prow0 - p.pad + xr;
            const int inimg = row * p.W + c_xorg;
            int nr = ((p.I - ch0) * hw - inimg) * 2;
            nr = ((unsigned)row < (unsigned)p.H && nr > 0) ? (nr & c_live) : 0;
            lds_dma_dword(make_rsrc(c_xn + (long long)ch0 * hw + inimg, nr), v_x, c_bufa + DY_BYTES + xr * XBLK + (wave + 8 * mm) * 256);
        } else {
            constexpr int u = I - 8 - 4 * XR;
            const int q = wave + 8 * u;
            const int xr = q >> 2, t = q & 3;
            const int ch0 = i0 + 16 * t, row = c_prow0 - p.pad + xr;
            const int inimg = row * p.W + c_xorg;
            int nr = ((p.I - ch0) * hw - inimg) * 2;
            nr = ((unsigned)row < (unsigned)p.H && nr > 0) ? (nr & c_live) : 0;
            lds_dma_dword(make_rsrc(c_xn + (long long)ch0 * hw + inimg, nr), v_t, c_bufa + DY_BYTES + xr * XBLK + 64 * ROWB + t * 256);
        }
    };
    // pieces [lo, hi) as one unrolled run
    auto issue_range = [&](auto lo, auto hi) __attribute__((always_inline)) {
        constexpr int LO = decltype(lo)::value, HI = decltype(hi)::value;
        static_for<LO, HI>([&](auto i) __attribute__((always_inline)) { issue_piece(i); });
    };

    // ---- fragment read offsets inside a buffer (swizzled); the two 16-pixel groups of this wave's half need their own
    const int rowA = wo * 32 + r32, rowB = wi * 32 + r32;
    const int fA = (rowA >> 1) & 7, fB = (rowB >> 1) & 7;
    unsigned a_off[2], xlo_off[2], xhi_off[2];
#pragma unroll
    for (int kq = 0; kq < 2; kq++) {
        const int g = th * 4 + kq * 2 + h;
        a_off[kq] = rowA * ROWB + ((g ^ fA) << 4);
        xlo_off[kq] = DY_BYTES + rowB * ROWB + ((g ^ fB) << 4);
        xhi_off[kq] = (g + 1 < 8) ? DY_BYTES + rowB * ROWB + (((g + 1) ^ fB) << 4) : DY_BYTES + 64 * ROWB + rowB * 16;
    }

    // ---- pipeline: NBUF-1 steps of loads in flight; a step's loads are waited for (counted vmcnt) before the barrier that
    // precedes its use.
#pragma unroll
    for (int i = 0; i < NBUF - 1; i++) {
        begin_loads(s0 + i < s1);
        issue_range(std::integral_constant<int, 0>{}, std::integral_constant<int, NPIECE>{});
    }
    if (NBUF == 3) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(NPIECE));
    else asm volatile("s_waitcnt vmcnt(0)");
    __syncthreads();
    int cbuf = 0;
    for (int step = s0; step < s1; step++) {
        constexpr int xoff = XOFF;
        begin_loads(step + NBUF - 1 < s1);                 // into the buffer everyone left at the last barrier
        const char* buf = lds + cbuf * BUF;
        typedef typename std::conditional<std::is_same<T, bf16_t>::value, bf16x8, f16x8>::type frag_t;
        static_for<0, 2>([&](auto kqc) __attribute__((always_inline)) {
            constexpr int kq = decltype(kqc)::value;
            frag_t a[R];
#pragma unroll
            for (int rr = 0; rr < R; rr++) a[rr] = *(const frag_t*)(buf + a_off[kq] + rr * (64 * ROWB));
            static_for<0, XR>([&](auto xrc) __attribute__((always_inline)) {
                constexpr int xr = decltype(xrc)::value;
                constexpr int it = kq * XR + xr, NIT = 2 * XR;
                issue_range(std::integral_constant<int, (it * NPIECE) / NIT>{}, std::integral_constant<int, ((it + 1) * NPIECE) / NIT>{});
                const uint4 lo = *(const uint4*)(buf + xlo_off[kq] + xr * XBLK);
                const uint4 hi = *(const uint4*)(buf + xhi_off[kq] + xr * XBLK);
                asm volatile("" : : "v"(hi.y), "v"(hi.z), "v"(hi.w));         // keep the read a full (conflict-free) b128
                const unsigned d[6] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y};
#pragma unroll
                for (int sft = 0; sft < KS; sft++) {
                    union { unsigned u[4]; frag_t f; } b;
                    const int sh = sft + xoff;                            // element shift in [0, 3], compile-time
#pragma unroll
                    for (int w = 0; w < 4; w++) {
                        const unsigned e0 = d[w], e1 = d[w + 1], e2 = d[(w + 2) % 6];
                        const unsigned odd_lo = __builtin_amdgcn_alignbyte(e1, e0, 2);
                        const unsigned odd_hi = __builtin_amdgcn_alignbyte(e2, e1, 2);
                        b.u[w] = (sh == 0) ? e0 : (sh == 1) ? odd_lo : (sh == 2) ? e1 : odd_hi;
                    }
#pragma unroll
                    for (int rr = 0; rr < R; rr++) {
                        const int r = xr - rr;
                        const int t = r * KS + sft;
                        if (r >= 0 && r < KS) {
                            if constexpr (std::is_same<T, bf16_t>::value)
                                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[rr], b.f, acc[t], 0, 0, 0);
                            else
                                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[rr], b.f, acc[t], 0, 0, 0);
                        }
                    }
                }
            });
        });
        // the next step's loads (issued NBUF-2 iterations ago, or just now when NBUF == 2) must have landed
        if (NBUF == 3) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(NPIECE));
        else asm volatile("s_waitcnt vmcnt(0)");
        __syncthreads();
        if (++cbuf == NBUF) cbuf = 0;
    }
    // ---- add the two pixel halves through LDS (the ring is free now): th 1 parks its accumulators, th 0 adds them and
    // writes the partial tile D[row = o][col = i].
    asm volatile("s_waitcnt vmcnt(0)");
    __syncthreads();
    {
        float* red = (float*)lds;
        constexpr int TPR_CAP = (NBUF * BUF) / (4 * 16 * 64 * (int)sizeof(float));     // taps per round
        constexpr int TPR = TPR_CAP < KK ? TPR_CAP : KK;
        static_assert(TPR >= 1, "LDS too small for the half-sum");
        const int wv4 = wave & 3;
#pragma unroll
        for (int t0 = 0; t0 < KK; t0 += TPR) {
            if (t0 > 0) __syncthreads();
            if (th == 1) {
#pragma unroll
                for (int t = t0; t < t0 + TPR && t < KK; t++)
#pragma unroll
                    for (int reg = 0; reg < 16; reg++) red[((wv4 * TPR + (t - t0)) * 16 + reg) * 64 + lane] = acc[t][reg];
            }
            __syncthreads();
            if (th == 0) {
#pragma unroll
                for (int t = t0; t < t0 + TPR && t < KK; t++)
#pragma unroll
                    for (int reg = 0; reg < 16; reg++) acc[t][reg] += red[((wv4 * TPR + (t - t0)) * 16 + reg) * 64 + lane];
            }
        }
    }
    if (th == 0) {
        float* out = p.part + (size_t)split * p.O * p.I * KK;
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            const int o = o0 + wo * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
            const int i = i0 + wi * 32 + r32;
            if (o < p.O && i < p.I) {
                float* dst = out + ((size_t)o * p.I + i) * KK;
#pragma unroll
                for (int t = 0; t < KK; t++) dst[t] = acc[t][reg];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// 16-bit weight gradient, 16-byte LDS-DMA pieces.  The address unit spends about the same time on a wave instruction
// whatever its width, and conv2d_wgrad16_kernel is bound by exactly that (208 dword pieces per step); this variant moves
// the same bytes in 56 pieces of 16 B per lane.  A lane fetches one granule = 8 pixels from a 4-byte aligned address, so
// validity is per granule, not per pixel:
//   * x is staged from column q0 - 8: the granule left of the image is dropped whole (pad = 2: taps reach back 2 columns);
//   * the granule that straddles the right edge of x brings the head of the next row: the wave that loaded it zeroes those
//     pixels in LDS before the barrier;
//   * dy beyond its right edge then multiplies zeros of x (its columns q >= Q pair with x columns >= W), whatever it holds.
// Supported: KS = 3 with pad = 2 (the generator's convs) and KS = 1 with pad = 0; everything else takes the dword kernel.
// LDS image of one step:   dy [rr 0..1][o 64][8 granules]   x main [xr][ch 64][8 granules]   x tail [ch>>3][xr][ch&7][1 granule]
// with granule g of row r at slot g ^ ((r >> 1) & 7); B fragments of tap column s are the 5-dword window
// (granule g).d3, (granule g+1).d0..3 shifted by s.

// SMALL (both tensors below 2^31 bytes): ONE buffer descriptor per tensor for the whole kernel; a piece's position is a 32-bit
// offset added to the lane offsets and its validity (row outside the image, dead step) an OR mask on bit 31.  The general form
// rebuilds a 128-bit descriptor per piece -- 64-bit base, exact record count, validity select, three v_readfirstlane --
// ~45 scalar instructions per piece, 310 per K step of 36 MFMAs: the wave's own instruction stream, not the matrix pipe, set
// the step time (PMC r01e: MFMA pipe 49 % busy, 8.7 SALU per MFMA).
constexpr int kWgradRing = 3;      // LDS ring depth of conv2d_wgrad16g_kernel (2: measured in profiles/r04_wgrad_ring.txt)
// X16 (r05): the same tile on v_mfma_f32_16x16x32 -- a wave's 32 (o) x 32 (i) tile is 2 x 2 tiles of 16 x 16 per tap (the same 144
// accumulator registers), a K step is 32 pixels = FOUR granules, one per 16-lane group: wave th takes pixels 32 th .. 32 th + 31 of the
// chunk.  ds_read_b128 serves the lanes in groups that hold all 16 rows with TWO neighbouring granules (G, G + 1), so the swizzle is
// slot = granule ^ (((row >> 1) & 3) << 1): both row sets of a group take the even XOR values once, G and G + 1 differ in bit 0 (G even)
// or flip bits that keep the even set (G odd: the hi half of the x windows): 16 distinct slots for every read (the (row >> 1) & 7 form
// of the 32x32x16 kernel is conflict-free only when all lanes of a group read the SAME granule).  A/B of the shapes: profiles/r05_*.
template <typename T, int KS, int NBUF, bool SMALL, bool X16 = false>
__global__ __launch_bounds__(512, 1) void conv2d_wgrad16g_kernel(WgradParams p) {
    static_assert(sizeof(T) == 2, "16-bit types only");
    constexpr int R = 2, KK = KS * KS, XR = R + KS - 1;
    auto swz = [](int row) __attribute__((always_inline)) { return X16 ? (((row >> 1) & 3) << 1) : ((row >> 1) & 7); };
    constexpr int ROWB = 128;                       // bytes of one staged row (64 pixels)
    constexpr int DY_BYTES = R * 64 * ROWB;
    constexpr int XMAIN = XR * 64 * ROWB;
    constexpr bool TAIL = KS > 1;
    constexpr int XTAIL = TAIL ? 8 * XR * 8 * 16 : 0;               // [ch>>3][xr][ch&7][16 B]
    constexpr int BUF = DY_BYTES + XMAIN + XTAIL;
    constexpr int NPIECE = R + XR + (TAIL ? 1 : 0);                 // LDS-DMA instructions per wave and step
    constexpr int XLEAD = TAIL ? 8 : 0;                             // x is staged from column q0 - XLEAD
    constexpr unsigned kOob = 0x80000000u;
    static_assert(XR * 8 <= 64, "tail piece: one lane per (xr, channel)");
    __shared__ __attribute__((aligned(1024))) char lds[NBUF * BUF];
    const unsigned lds0 = (unsigned)(unsigned long long)(__attribute__((address_space(3))) void*)lds;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // th: which half of the chunk's pixels this wave accumulates; (wo, wi): its 32 x 32 quadrant of the tile.  The two waves of a SIMD
    // (wave, wave + 4) take DIAGONALLY OPPOSITE quadrants: when a tile's rows 32.. or columns 32.. lie outside the matrix (the last tile of a
    // 91-channel operand: 27 live rows), every SIMD then holds one live and one idle wave instead of two SIMDs holding both
    const int th = wave >> 2, wo = (wave & 1) ^ th, wi = ((wave >> 1) & 1) ^ th;
    const int r32 = lane & 31, h = lane >> 5;

    const int tiles_i = cdiv(p.I, 64), tiles = tiles_i * cdiv(p.O, 64);
    int bid = blockIdx.x;
    bid = xcd_order(bid, tiles * p.splits);          // XCD x: contiguous logical ids (split-major)
    // integer division runs on the vector pipe even for uniform operands: pin the results to SGPRs, or every per-step address
    // and descriptor computation derived from them runs as 64-bit VALU code + v_readfirstlane (measured: ~130 vector
    // instructions per step beside the 36 MFMAs)
    const int split = __builtin_amdgcn_readfirstlane(bid / tiles);
    const int tile = bid - split * tiles;
    const int obk = __builtin_amdgcn_readfirstlane(tile / tiles_i);
    const int ib = tile - obk * tiles_i;
    const int o0 = obk * 64, i0 = ib * 64;

    // 32x32x16: one 32 x 32 tile per tap, element e = MFMA register e; 16x16x32: element 4 (2 ob2 + ib2) + reg of the (ob2, ib2) 16 x 16 tile
    f32x16 acc[KK];
#pragma unroll
    for (int t = 0; t < KK; t++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[t][e] = 0.f;

    // ---- load maps.  Wave w stages rows (channels) 8w..8w+7 of both operands: lane = (row, slot) of an 8-row piece.
    const int prow = 8 * wave + (lane >> 3), pslot = lane & 7;
    const int pg = pslot ^ swz(prow);                                            // logical granule that lives in this slot
    const int pq = p.P * p.lddy, hw = p.H * p.ldx;                                // plane strides (rows by pitch)
    // p.W also feeds per-lane offsets, so the compiler keeps it in a VGPR and then evaluates the (uniform) row addresses of the
    // x pieces on the vector pipe; an explicit scalar copy keeps them on the SALU
    const int Ws = __builtin_amdgcn_readfirstlane(p.ldx), Qs = __builtin_amdgcn_readfirstlane(p.lddy);
    const unsigned lp_dy = (o0 + prow < p.O) ? (unsigned)(prow * pq * 2 + pg * 16) : kOob;
    const unsigned lp_x = (i0 + prow < p.I) ? (unsigned)(prow * hw * 2 + pg * 16) : kOob;
    const int txr = lane >> 3, trow = 8 * wave + (lane & 7);                     // tail piece: lane = (xr, row), lanes >= 8 XR idle
    const unsigned lp_t = (i0 + trow < p.I) ? (unsigned)((trow * hw + txr * p.ldx + 64) * 2) : kOob;
    const long long dy_bytes = (long long)p.N * p.O * pq * 2, x_bytes = (long long)p.N * p.I * hw * 2;
    // SMALL: the two descriptors of the kernel (records = the tensor's bytes: a granule straddling its end reads zeros there)
    const i32x4 rs_dy = make_rsrc(p.dy, SMALL ? (int)dy_bytes : 0), rs_x = make_rsrc(p.x, SMALL ? (int)x_bytes : 0);
    unsigned c_dy32 = 0, c_x32 = 0;                                              // byte offsets of (image n, channel o0 / i0)

    const int steps_per_img = p.rowgroups * p.qchunks;
    int s0 = split * p.steps_per_split;
    int s1 = min(s0 + p.steps_per_split, p.N * steps_per_img);
    if (p.splits_img > 0) {                                                      // image-aligned shares (steps_per_split = ceil(steps_per_img / splits_img))
        const int img = __builtin_amdgcn_readfirstlane(split / p.splits_img), j = split - img * p.splits_img;
        s0 = img * steps_per_img + j * p.steps_per_split;
        s1 = min(s0 + p.steps_per_split, (img + 1) * steps_per_img);
        if (s1 < s0) s1 = s0;                                                    // (a share past the image's last step: zeros)
    }
    // a quadrant wholly outside the matrix: its waves only issue their share of the loads
    const bool quad_dead = o0 + wo * 32 >= p.O || i0 + wi * 32 >= p.I;
    int ld_n = __builtin_amdgcn_readfirstlane(s0 / steps_per_img);
    int ld_rg = __builtin_amdgcn_readfirstlane((s0 - ld_n * steps_per_img) / p.qchunks);
    int ld_qc = s0 - ld_n * steps_per_img - ld_rg * p.qchunks;
    int ld_buf = 0;
    int u_qc = ld_qc;                                                            // chunk (of its row pair) of the step being multiplied

    // state of the step being loaded (c_*) and of the one before it (f_*: the step whose x edge is fixed up next)
    int c_prow0 = 0, c_q0 = 0, c_live = 0, f_q0 = 0, f_live = 0;
    unsigned c_bufa = 0, f_bufa = 0, v_dy = 0, v_x = 0, v_t = 0;
    long long c_dyoff = 0, c_xoff = 0;                                           // byte offsets of the image (n) in dy / x
    auto begin_loads = [&](bool live) __attribute__((always_inline)) {
        f_q0 = c_q0; f_live = c_live; f_bufa = c_bufa;
        c_live = live ? -1 : 0;                                                  // a dead step still issues its pieces (0 records)
        c_prow0 = ld_rg * R; c_q0 = ld_qc * kWgKQ;
        c_bufa = ld_buf * BUF;
        const int xorg = c_q0 - XLEAD;
        v_dy = lp_dy | ((unsigned)!(c_q0 + 8 * pg < p.Q) << 31);
        v_x = lp_x | ((unsigned)!((unsigned)(xorg + 8 * pg) < (unsigned)p.W) << 31);
        v_t = lp_t | ((unsigned)!((unsigned)(xorg + 64) < (unsigned)p.W && (unsigned)(c_prow0 - p.pad + txr) < (unsigned)p.H) << 31);
        c_dyoff = (long long)ld_n * p.O * pq * 2;
        c_xoff = (long long)ld_n * p.I * hw * 2;
        if (SMALL) {
            c_dy32 = (unsigned)((ld_n * p.O + o0) * pq) * 2u;
            c_x32 = (unsigned)((ld_n * p.I + i0) * hw) * 2u;
        }
        if (live) {
            if (++ld_qc == p.qchunks) {
                ld_qc = 0;
                if (++ld_rg == p.rowgroups) { ld_rg = 0; ld_n++; }
            }
        }
        if (++ld_buf == NBUF) ld_buf = 0;
    };
    // records = bytes up to the end of the tensor (a straddling granule's dwords beyond it read as zero), 0 for a dead row
    auto records = [&](long long remaining, bool ok) __attribute__((always_inline)) -> int {
        const int r = remaining > 0x7fffffffll ? 0x7fffffff : (int)remaining;
        return (ok && r > 0) ? (r & c_live) : 0;
    };
    auto issue_piece = [&](auto idx) __attribute__((always_inline)) {
        constexpr int I = decltype(idx)::value;
        if constexpr (SMALL) {
            // offset of the piece (scalar) + lane offset; invalid lanes carry bit 31 in v_*, an invalid piece ORs it in for all
            if constexpr (I < R) {
                constexpr int rr = I;
                const int row = c_prow0 + rr;
                const unsigned soff = c_dy32 + (unsigned)(row * Qs + c_q0) * 2u;
                const unsigned sinv = (row < p.P && c_live) ? 0u : kOob;
                lds_dma_b128(rs_dy, ((v_dy & ~kOob) + soff) | (v_dy & kOob) | sinv, lds0 + c_bufa + rr * (64 * ROWB) + wave * 1024);
            } else if constexpr (I < R + XR) {
                constexpr int xr = I - R;
                const int row = c_prow0 - p.pad + xr;
                const unsigned soff = c_x32 + (unsigned)(row * Ws + c_q0 - XLEAD) * 2u;
                const unsigned sinv = ((unsigned)row < (unsigned)p.H && c_live) ? 0u : kOob;
                lds_dma_b128(rs_x, ((v_x & ~kOob) + soff) | (v_x & kOob) | sinv, lds0 + c_bufa + DY_BYTES + xr * (64 * ROWB) + wave * 1024);
            } else {
                const int row = c_prow0 - p.pad;                                 // lanes add their xr
                const unsigned soff = c_x32 + (unsigned)(row * Ws + c_q0 - XLEAD) * 2u;
                const unsigned sinv = c_live ? 0u : kOob;
                if (lane < 8 * XR)
                    lds_dma_b128(rs_x, ((v_t & ~kOob) + soff) | (v_t & kOob) | sinv, lds0 + c_bufa + DY_BYTES + XMAIN + wave * (XR * 128));
            }
        } else if constexpr (I < R) {
            constexpr int rr = I;
            const int row = c_prow0 + rr;
            const long long off = c_dyoff + ((long long)o0 * pq + row * Qs + c_q0) * 2;
            lds_dma_b128(make_rsrc((const char*)p.dy + off, records(dy_bytes - off, row < p.P)), v_dy,
                         lds0 + c_bufa + rr * (64 * ROWB) + wave * 1024);
        } else if constexpr (I < R + XR) {
            constexpr int xr = I - R;
            const int row = c_prow0 - p.pad + xr;
            const long long off = c_xoff + ((long long)i0 * hw + row * Ws + c_q0 - XLEAD) * 2;
            lds_dma_b128(make_rsrc((const char*)p.x + off, records(x_bytes - off, (unsigned)row < (unsigned)p.H)), v_x,
                         lds0 + c_bufa + DY_BYTES + xr * (64 * ROWB) + wave * 1024);
        } else {
            const int row = c_prow0 - p.pad;                                     // lanes add their xr
            const long long off = c_xoff + ((long long)i0 * hw + row * Ws + c_q0 - XLEAD) * 2;
            if (lane < 8 * XR)
                lds_dma_b128(make_rsrc((const char*)p.x + off, records(x_bytes - off, true)), v_t,
                             lds0 + c_bufa + DY_BYTES + XMAIN + wave * (XR * 128));
        }
    };
    auto issue_range = [&](auto lo, auto hi) __attribute__((always_inline)) {
        constexpr int LO = decltype(lo)::value, HI = decltype(hi)::value;
        static_for<LO, HI>([&](auto i) __attribute__((always_inline)) { issue_piece(i); });
    };
    // zero the pixels right of x's edge inside the granule that straddles it, in the rows this wave loaded (step f_*)
    auto fix_edge = [&]() __attribute__((always_inline)) {
        const int rel = p.W - (f_q0 - XLEAD);                                    // edge column relative to the staged origin
        const int gw = rel >> 3, vw = rel & 7;                                   // granule, valid pixels in it (even)
        if (f_live && vw != 0 && gw >= 0 && gw <= (TAIL ? 8 : 7) && lane < 8 * XR) {
            const int xr = lane >> 3, row = 8 * wave + (lane & 7);
            char* g = lds + f_bufa + DY_BYTES +
                      (gw < 8 ? xr * (64 * ROWB) + row * ROWB + ((gw ^ swz(row)) << 4) : XMAIN + wave * (XR * 128) + lane * 16);
#pragma unroll
            for (int d = 1; d < 4; d++)
                if (2 * d >= vw) *(unsigned*)(g + 4 * d) = 0u;
        }
    };

    // ---- fragment read offsets inside a buffer (swizzled)
    // X16: index 0 / 1 = the 16-row block (ob2 for dy, ib2 for x); lane = (row c16, granule G = 4 th + (lane >> 4)) -- rows 16 apart share
    // the swizzle, so block 1 is block 0 + 16 rows (the tail granule of x: + 2 channel octets)
    const int c16 = lane & 15, g4 = lane >> 4;
    const int rowA = wo * 32 + (X16 ? c16 : r32), rowB = wi * 32 + (X16 ? c16 : r32);
    const int fA = swz(rowA), fB = swz(rowB);
    unsigned a_off[2], x0_off[2], x1_off[2][XR];
#pragma unroll
    for (int kq = 0; kq < 2; kq++) {
        // 32x32x16: 16-pixel groups interleaved over the sibling waves: th 0: 0, 2; th 1: 1, 3
        const int g = X16 ? 4 * th + g4 : kq * 4 + th * 2 + h;
        const int ra = X16 ? rowA + 16 * kq : rowA, rb = X16 ? rowB + 16 * kq : rowB;
        a_off[kq] = ra * ROWB + ((g ^ fA) << 4);
        x0_off[kq] = DY_BYTES + rb * ROWB + ((g ^ fB) << 4);
#pragma unroll
        for (int xr = 0; xr < XR; xr++)
            x1_off[kq][xr] = (g + 1 < 8) ? DY_BYTES + xr * (64 * ROWB) + rb * ROWB + (((g + 1) ^ fB) << 4)
                                         : DY_BYTES + XMAIN + (rb >> 3) * (XR * 128) + xr * 128 + (rb & 7) * 16;
    }

    // ---- pipeline: NBUF-1 steps of loads in flight; a step's loads are waited for (counted vmcnt) before the barrier that
    // precedes its use.
#pragma unroll
    for (int i = 0; i < NBUF - 1; i++) {
        begin_loads(s0 + i < s1);
        issue_range(std::integral_constant<int, 0>{}, std::integral_constant<int, NPIECE>{});
    }
    asm volatile("s_waitcnt vmcnt(0)");
    if (NBUF == 3) {                       // both prologue steps have landed: fix both edges
        fix_edge();
        { const int q = f_q0, l = f_live; const unsigned b = f_bufa; f_q0 = c_q0; f_live = c_live; f_bufa = c_bufa; fix_edge(); f_q0 = q; f_live = l; f_bufa = b; }
    } else {
        f_q0 = c_q0; f_live = c_live; f_bufa = c_bufa;
        fix_edge();
    }
    __syncthreads();
    int cbuf = 0;
    for (int step = s0; step < s1; step++) {
        // LATE (16x16x32, 3x3): the live waves run begin_loads' ~50 scalar / vector instructions after their first iteration's MFMAs
        // instead of between the barrier and the first MFMA of all eight waves at once (their pieces then go out in iterations 1 .. 7):
        // 8.55 -> 8.28 ms in the step (profiles/r05_wgrad_late_ab.txt)
        constexpr bool LATE = X16 && TAIL;
        if constexpr (!LATE) begin_loads(step + NBUF - 1 < s1);                 // into the buffer everyone left at the last barrier
        const char* buf = lds + cbuf * BUF;
        typedef typename std::conditional<std::is_same<T, bf16_t>::value, bf16x8, f16x8>::type frag_t;
        // 16-pixel groups of the chunk that lie beyond the row's end would multiply zeros (rows of 86, 150, 278 pixels end
        // with 22 pixels of a 64-pixel chunk): a wave skips its dead groups and only issues its share of the next loads.  The
        // groups alternate between the two waves that share a SIMD (th 0 / th 1), so a 22-pixel chunk costs both one group.
        const int vq = quad_dead ? 0 : p.Q - u_qc * kWgKQ;
        if (++u_qc == p.qchunks) u_qc = 0;
        // one x row of one 16-pixel group: the next loads' share, the three shifted B fragments, 3 or 6 MFMAs
        auto row_mfmas = [&](auto kqc, auto xrc, const uint4 lo, const uint4 hi, const frag_t* a) __attribute__((always_inline)) {
            constexpr int kq = decltype(kqc)::value, xr = decltype(xrc)::value;
            constexpr int it = kq * XR + xr, NIT = 2 * XR;
            issue_range(std::integral_constant<int, (it * NPIECE) / NIT>{}, std::integral_constant<int, ((it + 1) * NPIECE) / NIT>{});
            asm volatile("" : : "v"(lo.x), "v"(lo.y), "v"(lo.z));               // keep the read a full (conflict-free) b128
            const unsigned d[5] = {lo.w, hi.x, hi.y, hi.z, hi.w};               // pixels 8g+6 .. 8g+15 of the staged row
#pragma unroll
            for (int sft = 0; sft < KS; sft++) {
                union { unsigned u[4]; frag_t f; } b;
#pragma unroll
                for (int w = 0; w < 4; w++)
                    b.u[w] = (sft == 0) ? d[w] : (sft == 1) ? __builtin_amdgcn_alignbyte(d[w + 1], d[w], 2) : d[w + 1];
#pragma unroll
                for (int rr = 0; rr < R; rr++) {
                    const int r = xr - rr;
                    const int t = r * KS + sft;
                    if (r >= 0 && r < KS) {
                        if constexpr (std::is_same<T, bf16_t>::value)
                            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[rr], b.f, acc[t], 0, 0, 0);
                        else
                            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[rr], b.f, acc[t], 0, 0, 0);
                    }
                }
            }
        };
        if constexpr (X16) {
            // one K step of 32 pixels per wave: 8 iterations (x row, 16-channel block of x), each the next loads' share, one window
            // (read one iteration ahead), its KS shifted B fragments and their MFMAs into the (o block, i block) tiles of the taps
            typedef __attribute__((ext_vector_type(4))) float cf32x4;
            auto mma = [&](const frag_t& av, const frag_t& bv, int t, int blk) __attribute__((always_inline)) {
                cf32x4 c = {acc[t][4 * blk + 0], acc[t][4 * blk + 1], acc[t][4 * blk + 2], acc[t][4 * blk + 3]};
                if constexpr (std::is_same<T, bf16_t>::value) c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv, c, 0, 0, 0);
                else c = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bv, c, 0, 0, 0);
                acc[t][4 * blk + 0] = c[0]; acc[t][4 * blk + 1] = c[1]; acc[t][4 * blk + 2] = c[2]; acc[t][4 * blk + 3] = c[3];
            };
            if (th * 32 >= vq) {                       // this wave's 32 pixels lie beyond the row's end: only its share of the next loads
                if constexpr (LATE) begin_loads(step + NBUF - 1 < s1);
                issue_range(std::integral_constant<int, 0>{}, std::integral_constant<int, NPIECE>{});
            } else if constexpr (!TAIL) {
                frag_t a[2][R];
#pragma unroll
                for (int ob2 = 0; ob2 < 2; ob2++)
#pragma unroll
                    for (int rr = 0; rr < R; rr++) a[ob2][rr] = *(const frag_t*)(buf + a_off[ob2] + rr * (64 * ROWB));
                static_for<0, 2 * XR>([&](auto itc) __attribute__((always_inline)) {
                    constexpr int it = decltype(itc)::value, xr = it >> 1, ib2 = it & 1, NIT = 2 * XR;
                    issue_range(std::integral_constant<int, (it * NPIECE) / NIT>{}, std::integral_constant<int, ((it + 1) * NPIECE) / NIT>{});
                    const frag_t bv = *(const frag_t*)(buf + x0_off[ib2] + xr * (64 * ROWB));
#pragma unroll
                    for (int ob2 = 0; ob2 < 2; ob2++) mma(a[ob2][xr], bv, 0, 2 * ob2 + ib2);
                });
            } else {
                frag_t a[2][R];
#pragma unroll
                for (int ob2 = 0; ob2 < 2; ob2++)
#pragma unroll
                    for (int rr = 0; rr < R; rr++) a[ob2][rr] = *(const frag_t*)(buf + a_off[ob2] + rr * (64 * ROWB));
                uint4 lo_n = *(const uint4*)(buf + x0_off[0]);
                uint4 hi_n = *(const uint4*)(buf + x1_off[0][0]);
                static_for<0, 2 * XR>([&](auto itc) __attribute__((always_inline)) {
                    constexpr int it = decltype(itc)::value, xr = it >> 1, ib2 = it & 1, NIT = 2 * XR;
                    const uint4 lo = lo_n, hi = hi_n;
                    if constexpr (it + 1 < NIT) {
                        constexpr int xr1 = (it + 1) >> 1, ib1 = (it + 1) & 1;
                        lo_n = *(const uint4*)(buf + x0_off[ib1] + xr1 * (64 * ROWB));
                        hi_n = *(const uint4*)(buf + x1_off[ib1][xr1]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (LATE) {
                        static_assert(!LATE || NPIECE == NIT - 1, "one piece per iteration after the first");
                        if constexpr (it > 0) issue_piece(std::integral_constant<int, it - 1>{});
                    } else
                        issue_range(std::integral_constant<int, (it * NPIECE) / NIT>{}, std::integral_constant<int, ((it + 1) * NPIECE) / NIT>{});
                    asm volatile("" : : "v"(lo.x), "v"(lo.y), "v"(lo.z));               // keep the read a full (conflict-free) b128
                    const unsigned d[5] = {lo.w, hi.x, hi.y, hi.z, hi.w};               // pixels 8G+6 .. 8G+15 of the staged row
#pragma unroll
                    for (int sft = 0; sft < KS; sft++) {
                        union { unsigned u[4]; frag_t f; } bw;
#pragma unroll
                        for (int w = 0; w < 4; w++)
                            bw.u[w] = (sft == 0) ? d[w] : (sft == 1) ? __builtin_amdgcn_alignbyte(d[w + 1], d[w], 2) : d[w + 1];
#pragma unroll
                        for (int rr = 0; rr < R; rr++) {
                            const int r = xr - rr;
                            if (r >= 0 && r < KS) {
#pragma unroll
                                for (int ob2 = 0; ob2 < 2; ob2++) mma(a[ob2][rr], bw.f, r * KS + sft, 2 * ob2 + ib2);
                            }
                        }
                    }
                    if constexpr (LATE && it == 0) begin_loads(step + NBUF - 1 < s1);
                    __builtin_amdgcn_sched_barrier(0);
                });
            }
        } else if constexpr (!TAIL) {
            static_for<0, 2>([&](auto kqc) __attribute__((always_inline)) {
                constexpr int kq = decltype(kqc)::value;
                if ((kq * 2 + th) * 16 >= vq) {
                    issue_range(std::integral_constant<int, (kq * XR * NPIECE) / (2 * XR)>{}, std::integral_constant<int, ((kq + 1) * XR * NPIECE) / (2 * XR)>{});
                    return;
                }
                frag_t a[R];
#pragma unroll
                for (int rr = 0; rr < R; rr++) a[rr] = *(const frag_t*)(buf + a_off[kq] + rr * (64 * ROWB));
                static_for<0, XR>([&](auto xrc) __attribute__((always_inline)) {
                    constexpr int xr = decltype(xrc)::value;
                    constexpr int it = kq * XR + xr, NIT = 2 * XR;
                    issue_range(std::integral_constant<int, (it * NPIECE) / NIT>{}, std::integral_constant<int, ((it + 1) * NPIECE) / NIT>{});
                    const frag_t b = *(const frag_t*)(buf + x0_off[kq] + xr * (64 * ROWB));
                    constexpr int rr = xr;
                    if constexpr (std::is_same<T, bf16_t>::value) acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[rr], b, acc[0], 0, 0, 0);
                    else acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[rr], b, acc[0], 0, 0, 0);
                });
            });
        } else {
            // The x windows are read one row ahead of their MFMAs, also across the two groups (left to itself the scheduler emits
            // read, wait, multiply for every row: eight exposed LDS round trips per step with only the sibling wave to cover
            // them).  The reads ahead are unconditional -- a dead group's window is simply not used.
            frag_t a[2][R];
#pragma unroll
            for (int rr = 0; rr < R; rr++) a[0][rr] = *(const frag_t*)(buf + a_off[0] + rr * (64 * ROWB));
            uint4 lo_n = *(const uint4*)(buf + x0_off[0]);
            uint4 hi_n = *(const uint4*)(buf + x1_off[0][0]);
            static_for<0, 2>([&](auto kqc) __attribute__((always_inline)) {
                constexpr int kq = decltype(kqc)::value;
                if ((kq * 2 + th) * 16 >= vq) {
                    issue_range(std::integral_constant<int, (kq * XR * NPIECE) / (2 * XR)>{}, std::integral_constant<int, ((kq + 1) * XR * NPIECE) / (2 * XR)>{});
                    if constexpr (kq == 0) {
#pragma unroll
                        for (int rr = 0; rr < R; rr++) a[1][rr] = *(const frag_t*)(buf + a_off[1] + rr * (64 * ROWB));
                        lo_n = *(const uint4*)(buf + x0_off[1]);
                        hi_n = *(const uint4*)(buf + x1_off[1][0]);
                    }
                    return;
                }
                static_for<0, XR>([&](auto xrc) __attribute__((always_inline)) {
                    constexpr int xr = decltype(xrc)::value;
                    const uint4 lo = lo_n, hi = hi_n;
                    if constexpr (xr + 1 < XR) {
                        lo_n = *(const uint4*)(buf + x0_off[kq] + (xr + 1) * (64 * ROWB));
                        hi_n = *(const uint4*)(buf + x1_off[kq][xr + 1 < XR ? xr + 1 : xr]);
                    } else if constexpr (kq == 0) {
                        lo_n = *(const uint4*)(buf + x0_off[1]);
                        hi_n = *(const uint4*)(buf + x1_off[1][0]);
                    }
                    if constexpr (kq == 0 && xr == 1) {
#pragma unroll
                        for (int rr = 0; rr < R; rr++) a[1][rr] = *(const frag_t*)(buf + a_off[1] + rr * (64 * ROWB));
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    row_mfmas(kqc, xrc, lo, hi, a[kq]);
                    __builtin_amdgcn_sched_barrier(0);
                });
            });
        }
        // the next step's loads (issued NBUF-2 iterations ago, or just now when NBUF == 2) must have landed; patch its edge
        if (NBUF == 3) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(NPIECE));
        else { asm volatile("s_waitcnt vmcnt(0)"); f_q0 = c_q0; f_live = c_live; f_bufa = c_bufa; }
        fix_edge();
        __syncthreads();
        if (++cbuf == NBUF) cbuf = 0;
    }
    // ---- add the two pixel halves through LDS (the ring is free now): th 1 parks its accumulators, th 0 adds them and
    // writes the partial tile D[row = o][col = i].
    asm volatile("s_waitcnt vmcnt(0)");
    __syncthreads();
    {
        float* red = (float*)lds;
        constexpr int TPR_CAP = (NBUF * BUF) / (4 * 16 * 64 * (int)sizeof(float));     // taps per round
        constexpr int TPR = TPR_CAP < KK ? TPR_CAP : KK;
        static_assert(TPR >= 1, "LDS too small for the half-sum");
        const int wv4 = wo + 2 * wi;                                     // the quadrant: both pixel halves of it meet in the same slot
#pragma unroll
        for (int t0 = 0; t0 < KK; t0 += TPR) {
            if (t0 > 0) __syncthreads();
            if (th == 1) {
#pragma unroll
                for (int t = t0; t < t0 + TPR && t < KK; t++)
#pragma unroll
                    for (int reg = 0; reg < 16; reg++) red[((wv4 * TPR + (t - t0)) * 16 + reg) * 64 + lane] = acc[t][reg];
            }
            __syncthreads();
            if (th == 0) {
#pragma unroll
                for (int t = t0; t < t0 + TPR && t < KK; t++)
#pragma unroll
                    for (int reg = 0; reg < 16; reg++) acc[t][reg] += red[((wv4 * TPR + (t - t0)) * 16 + reg) * 64 + lane];
            }
        }
    }
    if (th == 0) {
        float* out = p.part + (size_t)split * p.O * p.I * KK;
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            // 16x16x32: element 4 (2 ob2 + ib2) + r of the (ob2, ib2) tile = row 16 ob2 + 4 (lane >> 4) + r, column 16 ib2 + (lane & 15)
            const int o = o0 + wo * 32 + (X16 ? 16 * (reg >> 3) + 4 * g4 + (reg & 3) : (reg & 3) + 8 * (reg >> 2) + 4 * h);
            const int i = i0 + wi * 32 + (X16 ? 16 * ((reg >> 2) & 1) + c16 : r32);
            if (o < p.O && i < p.I) {
                float* dst = out + ((size_t)o * p.I + i) * KK;
#pragma unroll
                for (int t = 0; t < KK; t++) dst[t] = acc[t][reg];
            }
        }
    }
}

// Slabs of the workspace that every tile wrote (WgradParams::splits)
struct WgradSlabs { int splits; };
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(float* __restrict__ dw, const float* __restrict__ part, long long numel, WgradSlabs w) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < numel; idx += (long long)gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int k = 0; k < w.splits; k++) s += part[(size_t)k * numel + idx];
        dw[idx] = s;
    }
}

// Same reduction for numel % 4 == 0 with 16-byte loads and the split index spread over the workgroup: 256 threads =
// COLS float4 columns x (256 / COLS) split groups, group partials summed through LDS.  A 64 -> 64 layer has 36,864 outputs and 256
// splits (151 MB of partials): one thread per output is 144 workgroups of serial 4-byte loads on a 256-CU chip.
template <int COLS>
__global__ __launch_bounds__(256) void wgrad_reduce4_kernel(float* __restrict__ dw, const float* __restrict__ part, long long numel4, WgradSlabs w) {
    constexpr int GROUPS = 256 / COLS;
    typedef __attribute__((ext_vector_type(4))) float f32x4v;
    __shared__ f32x4v red[GROUPS][COLS];
    const int col = threadIdx.x % COLS, grp = threadIdx.x / COLS;
    const long long c4 = (long long)blockIdx.x * COLS + col;
    f32x4v s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
    if (c4 < numel4) {
        const f32x4v* src = (const f32x4v*)part + c4;
        const int splits = w.splits;
        int k = grp;
        for (; k + 3 * GROUPS < splits; k += 4 * GROUPS) {
            const f32x4v v0 = src[(size_t)k * numel4], v1 = src[(size_t)(k + GROUPS) * numel4];
            const f32x4v v2 = src[(size_t)(k + 2 * GROUPS) * numel4], v3 = src[(size_t)(k + 3 * GROUPS) * numel4];
            s0 += v0; s1 += v1; s0 += v2; s1 += v3;
        }
        for (; k < splits; k += GROUPS) s0 += src[(size_t)k * numel4];
    }
    s0 += s1;
    if (GROUPS > 1) {
        red[grp][col] = s0;
        __syncthreads();
        if (grp == 0 && c4 < numel4) {
#pragma unroll
            for (int g = 1; g < GROUPS; g++) s0 += red[g][col];
            ((f32x4v*)dw)[c4] = s0;
        }
    } else if (c4 < numel4) {
        ((f32x4v*)dw)[c4] = s0;
    }
}


// Slab reduction of an IMAGE-ALIGNED weight gradient (WgradParams::splits_img) that also returns, per image n and input channel i,
//     dots[n][i] = sum_{o, tap} wq[o][i][tap] * dW_n[o][i][tap]          dW_n = the sum of image n's slabs, wq = w rounded to the conv's 16-bit type
// = <x[n, i], dx[n, i]> with dx = conv^T(wq, dy): the contraction <dy_n, conv(wq[:, i], x[n, i])> written from the weight side instead of
// the pixel side.  For the layer below this is <g, z> -- the gradient of the styles its epilogue multiplied z by -- which r01-r05 read from
// g and z themselves: a full pass over both tensors (312-624 MB per 276^2 layer, 50-118 us) for numbers that these slabs already hold
// (27-38 MB, read here anyway).  Differs from the pixel-side dot product only by the 16-bit rounding of the STORED dx.
// One workgroup (16 waves) per input channel i; wave q takes images q, q + 16, ...; lane = output row of a block of 64.
template <typename T, int KK>
__global__ __launch_bounds__(1024) void wgrad_reduce_dots_kernel(float* __restrict__ dw, float* __restrict__ dots, const float* __restrict__ part,
                                                                 const float* __restrict__ w, int N, int O, int I, int splits_img) {
    // 16 waves: wave q takes images q, q + 16, ... (one each at batch 16); lane = output row of a block of 64.  (r06, first form: 4 waves, four
    // images each in turn -- 58 us for the 64 -> 64 layer's 38 MB of slabs where the plain reduction took 7.)
    constexpr int NW = 16;
    __shared__ float red[NW - 1][64][KK];
    const int i = blockIdx.x, lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const size_t slab = (size_t)O * I * KK;
    float dotp[4];
#pragma unroll
    for (int k = 0; k < 4; k++) dotp[k] = 0.f;
    for (int ob = 0; ob < O; ob += 64) {
        const int o = ob + lane;
        const bool live = o < O;
        const size_t e0 = ((size_t)(live ? o : O - 1) * I + i) * KK;
        float wq[KK], tot[KK];
#pragma unroll
        for (int t = 0; t < KK; t++) { wq[t] = live ? to_f32(from_f32<T>(w[e0 + t])) : 0.f; tot[t] = 0.f; }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int n = q + NW * k;
            if (n >= N) break;                                  // (wave-uniform)
            float acc[KK];
#pragma unroll
            for (int t = 0; t < KK; t++) acc[t] = 0.f;
            for (int sp = 0; sp < splits_img; sp++) {
                const float* src = part + (size_t)(n * splits_img + sp) * slab + e0;
#pragma unroll
                for (int t = 0; t < KK; t++) acc[t] += src[t];
            }
            float d = 0.f;
#pragma unroll
            for (int t = 0; t < KK; t++) { tot[t] += acc[t]; d = fmaf(wq[t], acc[t], d); }
            dotp[k] += d;
        }
        if (ob > 0) __syncthreads();                            // (the previous block's partials have been read)
        if (q > 0) {
#pragma unroll
            for (int t = 0; t < KK; t++) red[q - 1][lane][t] = tot[t];
        }
        __syncthreads();
        if (q == 0 && live) {
#pragma unroll
            for (int t = 0; t < KK; t++) {
                float s = tot[t];
#pragma unroll
                for (int k = 0; k < NW - 1; k++) s += red[k][lane][t];
                dw[e0 + t] = s;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int n = q + NW * k;
        if (n >= N) break;
        float d = dotp[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) d += __shfl_xor(d, off);
        if (lane == 0) dots[(size_t)n * I + i] = d;
    }
}
}  // namespace afcm

using namespace afcm;


// Split count for the weight gradient: enough workgroups to fill the chip, bounded by the K macro-steps.
static int wgrad_rows_per_step(int dtype) { return dtype == AFCM_F32 ? 1 : 2; }

// Workgroups per 64 x 64 tile.  One workgroup per CU is resident (LDS ring), so aim for ONE full round of the 256 CUs and never one
// workgroup more: rounding up (258 workgroups = two rounds) halves the throughput, and every extra split costs a 36 x 64 x 64 x 4 B
// partial tile written and read back (at 768 workgroups the partials of a 64 -> 64 layer were 2/3 of its time).
// Every tile gets the same count.  (Tiles whose last 32 rows or columns lie outside the matrix skip those quadrants: 3-6 % on the
// 91-channel layers, L11 0.33 -> 0.31 ms.  A two-class plan that gave them 0.6 of a full tile's workgroups on top made those layers
// SLOWER, L11 0.31 -> 0.36: a lone wave per SIMD cannot hide its own LDS latency, a step costs a partial tile nearer 0.8 than 0.6 of a
// full one -- profiles/r05_wgrad_partial_tiles.txt.)
static int wgrad_splits(int n, int cout, int cin, int p_rows) {
    const int tiles = cdiv(cout, 64) * cdiv(cin, 64);
    const long long ksteps = (long long)n * p_rows;   // upper bound on the macro-steps of any dtype
    int s = 256 / tiles;
    if (s > ksteps) s = (int)ksteps;
    return s < 1 ? 1 : s;
}

extern "C" int afcm_conv2d_wgrad_splits(int32_t n, int32_t cout, int32_t cin, int32_t p_rows) {
    return wgrad_splits(n, cout, cin, p_rows);   // slabs of the workspace: the most any tile writes
}

extern "C" int afcm_conv2d_wgrad(float* dw, float* workspace, const void* dy, const void* x, int32_t dtype, int32_t n, int32_t cin,
                                 int32_t cout, int32_t h, int32_t w, int32_t ks, int32_t pad, void* stream) {
    return afcm_conv2d_wgrad_ld(dw, workspace, dy, x, dtype, n, cin, cout, h, w, ks, pad, 0, 0, stream);
}

// Which weight-gradient kernel a call takes and how its K range is cut: the ONE place where wgrad_impl decides it, and what
// afcm_conv2d_wgrad_plan reports.
enum { kWgF32 = 0, kWgDword = 1, kWgGranule = 2 };
enum { kWgReduceScalar = 0, kWgReduce4x256 = 1, kWgReduce4x64 = 2, kWgReduce4x16 = 3, kWgReduceDots = 4 };
struct WgradPlan {
    int kernel;             // kWg*
    int pad_odd;            // XOFF of the fp32 and dword kernels (pad & 1)
    bool x16;               // granule kernel: the 16x16x32 MFMA form (else 32x32x16)
    bool small;             // granule kernel: one descriptor per tensor (both below 2 GB)
    int qchunks, rowgroups;
    int splits, steps_per_split, splits_img;
    int reduce;             // kWgReduce* (for 16-byte aligned dw / workspace; others take the scalar kernel)
};

// AFCM_OK, or AFCM_E_NOKERNEL when `dots` asks for image-aligned shares that this shape does not have
static int wgrad_plan(WgradPlan* pl, int dtype, int n, int cin, int cout, int h, int ldx, int ks, int pad, int P, int Q, int lddy, bool dots) {
    const int R = wgrad_rows_per_step(dtype);
    pl->qchunks = cdiv(Q, kWgKQ);
    pl->rowgroups = cdiv(P, R);
    const long long ksteps = (long long)n * pl->rowgroups * pl->qchunks;
    const bool granule = (ks == 3 && pad == 2) || (ks == 1 && pad == 0);     // 16-byte LDS-DMA pieces; other paddings: 4-byte pieces
    // (16-bit convs that are not granule ones are 3x3 with pad 0 or 1: a 1x1 conv has pad 0)
    pl->kernel = dtype == AFCM_F32 ? kWgF32 : granule ? kWgGranule : kWgDword;
    pl->pad_odd = (ks == 3) ? (pad & 1) : 0;
    pl->splits = wgrad_splits(n, cout, cin, P);
    if (pl->splits > ksteps) pl->splits = (int)ksteps;
    pl->steps_per_split = (int)((ksteps + pl->splits - 1) / pl->splits);
    pl->splits_img = 0;
    if (dots) {
        // image-aligned shares: the same number of workgroups, each inside one image (the granule kernel, a split count that is a
        // multiple of the batch, at most 64 images: what wgrad_reduce_dots_kernel covers) -- else the caller takes its dot products
        // from the tensors themselves
        if (pl->kernel != kWgGranule || n > 64 || pl->splits % n != 0 || pl->splits / n < 1) return AFCM_E_NOKERNEL;
        pl->splits_img = pl->splits / n;
        const long long per_img = (long long)pl->rowgroups * pl->qchunks;
        pl->steps_per_split = (int)((per_img + pl->splits_img - 1) / pl->splits_img);
    }
    // MFMA shape (template flag X16; profiles/r05_conv_shape_ab.txt): 16x16x32 holds a higher clock on the large layers (+3 .. 6 %), but its K
    // step is 32 pixels where the 32x32x16 form skips dead 16-pixel groups: rows whose last 64-pixel chunk holds 33 .. 48 pixels (the 38-wide
    // planes of the 36^2 layers) cost it a whole extra step (-12 % there) -- those keep the 32x32x16 form.
    const int q_last = Q % 64;
    pl->x16 = !(q_last > 32 && q_last <= 48);
    // tensors below 2 GB: one descriptor per tensor; larger ones: a descriptor per LDS-DMA piece (the general form)
    pl->small = (long long)n * cout * P * lddy * 2 < (1ll << 31) - 65536 &&
                (long long)n * cin * h * ldx * 2 < (1ll << 31) - 65536;
    const long long numel = (long long)cout * cin * ks * ks;
    if (pl->splits_img > 0) pl->reduce = kWgReduceDots;
    else if ((numel & 3) != 0) pl->reduce = kWgReduceScalar;
    else pl->reduce = pl->splits >= 64 ? kWgReduce4x16 : pl->splits >= 8 ? kWgReduce4x64 : kWgReduce4x256;
    return AFCM_OK;
}

static int wgrad_impl(float* dw, float* workspace, const void* dy, const void* x, int32_t dtype, int32_t n, int32_t cin,
                      int32_t cout, int32_t h, int32_t w, int32_t ks, int32_t pad, int32_t dy_pitch, int32_t x_pitch, float* dots, const float* wref, void* stream) {
    AFCM_REQUIRE(dw != nullptr && workspace != nullptr && dy != nullptr && x != nullptr, "conv2d_wgrad: null pointer");
    AFCM_REQUIRE(dtype == AFCM_F32 || dtype == AFCM_F16 || dtype == AFCM_BF16, "x must be float32, float16 or bfloat16");
    AFCM_REQUIRE(ks == 1 || ks == 3, "only 1x1 and 3x3 kernels are supported");
    AFCM_REQUIRE(pad >= 0 && pad <= ks - 1, "padding must be in [0, k-1]");
    WgradParams p;
    p.dy = dy; p.x = x; p.part = workspace;
    p.N = n; p.O = cout; p.I = cin; p.H = h; p.W = w; p.pad = pad;
    p.P = h + 2 * pad - ks + 1; p.Q = w + 2 * pad - ks + 1;
    AFCM_REQUIRE(p.P >= 1 && p.Q >= 1, "output must be at least 1x1");
    AFCM_REQUIRE(dtype == AFCM_F32 || (w % 2 == 0 && p.Q % 2 == 0), "16-bit conv2d_wgrad needs even widths (got %d, %d)", w, p.Q);
    p.lddy = dy_pitch ? dy_pitch : p.Q; p.ldx = x_pitch ? x_pitch : w;
    const bool pitched = p.lddy != p.Q || p.ldx != w;
    AFCM_REQUIRE(!pitched || (p.lddy >= p.Q && p.ldx >= w && ((p.lddy | p.ldx) & 1) == 0), "conv2d_wgrad: row pitches %d / %d must be even and cover the widths %d / %d", p.lddy, p.ldx, p.Q, w);
    WgradPlan pl;
    if (wgrad_plan(&pl, dtype, n, cin, cout, h, p.ldx, ks, pad, p.P, p.Q, p.lddy, dots != nullptr) != AFCM_OK) return AFCM_E_NOKERNEL;
    AFCM_REQUIRE(dots == nullptr || wref != nullptr, "conv2d_wgrad_dots: the weight tensor the dot products are taken with is missing");
    p.qchunks = pl.qchunks; p.rowgroups = pl.rowgroups;
    p.splits = pl.splits; p.steps_per_split = pl.steps_per_split; p.splits_img = pl.splits_img;
    const bool granule = pl.kernel == kWgGranule;
    const bool wg_x16 = pl.x16, small = pl.small;
    const long long blocks = (long long)cdiv(cout, 64) * cdiv(cin, 64) * p.splits;
    dim3 grid((unsigned)blocks), block(512);
    hipStream_t st = (hipStream_t)stream;
#define AFCM_WG16(T) do { constexpr int NB = 3; \
                           if (pl.pad_odd == 0) hipLaunchKernelGGL((conv2d_wgrad16_kernel<T, 3, 0, NB>), grid, block, 0, st, p); \
                           else hipLaunchKernelGGL((conv2d_wgrad16_kernel<T, 3, 1, NB>), grid, block, 0, st, p); } while (0)
#define AFCM_WG16G_(T, X) do { constexpr int NB = kWgradRing; \
                            if (small && ks == 3) hipLaunchKernelGGL((conv2d_wgrad16g_kernel<T, 3, NB, true, X>), grid, block, 0, st, p); \
                            else if (small) hipLaunchKernelGGL((conv2d_wgrad16g_kernel<T, 1, NB, true, X>), grid, block, 0, st, p); \
                            else if (ks == 3) hipLaunchKernelGGL((conv2d_wgrad16g_kernel<T, 3, NB, false, X>), grid, block, 0, st, p); \
                            else hipLaunchKernelGGL((conv2d_wgrad16g_kernel<T, 1, NB, false, X>), grid, block, 0, st, p); } while (0)
#define AFCM_WG16G(T) do { if (wg_x16) AFCM_WG16G_(T, true); else AFCM_WG16G_(T, false); } while (0)
    // rows by pitch: the 16-byte LDS-DMA kernel only (a granule straddling x's right edge is zeroed in LDS whatever follows it)
    AFCM_REQUIRE(!pitched || (dtype != AFCM_F32 && granule), "conv2d_wgrad: row pitches need the 16-bit granule kernel (3x3 pad 2 or 1x1 pad 0)");
    switch (dtype) {
        case AFCM_F32:
            if (ks == 3 && pl.pad_odd == 0) hipLaunchKernelGGL((conv2d_wgrad_kernel<3, 0>), grid, block, 0, st, p);
            else if (ks == 3) hipLaunchKernelGGL((conv2d_wgrad_kernel<3, 1>), grid, block, 0, st, p);
            else hipLaunchKernelGGL((conv2d_wgrad_kernel<1, 0>), grid, block, 0, st, p);
            break;
        case AFCM_F16: if (granule) AFCM_WG16G(f16_t); else AFCM_WG16(f16_t); break;
        default: if (granule) AFCM_WG16G(bf16_t); else AFCM_WG16(bf16_t); break;
    }
#undef AFCM_WG16G
#undef AFCM_WG16G_
#undef AFCM_WG16
    int rc = hip_status(hipGetLastError());
    if (rc != AFCM_OK) return rc;
    const long long numel = (long long)cout * cin * ks * ks;
    if (p.splits_img > 0) {
        const dim3 rgrid((unsigned)cin), rblock(1024);
#define AFCM_RD(T) do { if (ks == 3) hipLaunchKernelGGL((wgrad_reduce_dots_kernel<T, 9>), rgrid, rblock, 0, st, dw, dots, (const float*)workspace, wref, n, cout, cin, p.splits_img); \
                        else hipLaunchKernelGGL((wgrad_reduce_dots_kernel<T, 1>), rgrid, rblock, 0, st, dw, dots, (const float*)workspace, wref, n, cout, cin, p.splits_img); } while (0)
        if (dtype == AFCM_F16) AFCM_RD(f16_t); else AFCM_RD(bf16_t);
#undef AFCM_RD
        return hip_status(hipGetLastError());
    }
    const WgradSlabs slabs{p.splits};
    long long rb = (numel + 255) / 256;
    if (rb > 2048) rb = 2048;
    // splits beyond the last populated one were never launched with work: they still wrote zeros (acc = 0)
    if (pl.reduce != kWgReduceScalar && (((uintptr_t)dw | (uintptr_t)workspace) & 15) == 0) {
        const long long n4 = numel / 4;
        if (pl.reduce == kWgReduce4x16) hipLaunchKernelGGL(wgrad_reduce4_kernel<16>, dim3((unsigned)cdiv(n4, 16)), dim3(256), 0, st, dw, (const float*)workspace, n4, slabs);
        else if (pl.reduce == kWgReduce4x64) hipLaunchKernelGGL(wgrad_reduce4_kernel<64>, dim3((unsigned)cdiv(n4, 64)), dim3(256), 0, st, dw, (const float*)workspace, n4, slabs);
        else hipLaunchKernelGGL(wgrad_reduce4_kernel<256>, dim3((unsigned)cdiv(n4, 256)), dim3(256), 0, st, dw, (const float*)workspace, n4, slabs);
    } else {
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)rb), dim3(256), 0, st, dw, (const float*)workspace, numel, slabs);
    }
    return hip_status(hipGetLastError());
}

extern "C" int afcm_conv2d_wgrad_ld(float* dw, float* workspace, const void* dy, const void* x, int32_t dtype, int32_t n, int32_t cin,
                                    int32_t cout, int32_t h, int32_t w, int32_t ks, int32_t pad, int32_t dy_pitch, int32_t x_pitch, void* stream) {
    return wgrad_impl(dw, workspace, dy, x, dtype, n, cin, cout, h, w, ks, pad, dy_pitch, x_pitch, nullptr, nullptr, stream);
}

extern "C" int afcm_conv2d_wgrad_dots_ld(float* dw, float* dots, float* workspace, const void* dy, const void* x, const float* wref, int32_t dtype,
                                         int32_t n, int32_t cin, int32_t cout, int32_t h, int32_t w, int32_t ks, int32_t pad, int32_t dy_pitch,
                                         int32_t x_pitch, void* stream) {
    AFCM_REQUIRE(dots != nullptr, "conv2d_wgrad_dots: dots must be non-null");
    return wgrad_impl(dw, workspace, dy, x, dtype, n, cin, cout, h, w, ks, pad, dy_pitch, x_pitch, dots, wref, stream);
}

// Pure host: the plan afcm_conv2d_wgrad_ld (dots == 0) / afcm_conv2d_wgrad_dots_ld (dots != 0) follow for these arguments
extern "C" int afcm_conv2d_wgrad_plan(int32_t dtype, int32_t n, int32_t cin, int32_t cout, int32_t h, int32_t w, int32_t ks, int32_t pad,
                                      int32_t dy_pitch, int32_t x_pitch, int32_t dots, int32_t out[8]) {
    AFCM_REQUIRE(out != nullptr, "conv2d_wgrad_plan: null pointer");
    AFCM_REQUIRE(dtype == AFCM_F32 || dtype == AFCM_F16 || dtype == AFCM_BF16, "x must be float32, float16 or bfloat16");
    AFCM_REQUIRE(n > 0 && cin > 0 && cout > 0 && h > 0 && w > 0, "x is empty");
    AFCM_REQUIRE(ks == 1 || ks == 3, "only 1x1 and 3x3 kernels are supported");
    AFCM_REQUIRE(pad >= 0 && pad <= ks - 1, "padding must be in [0, k-1]");
    const int P = h + 2 * pad - ks + 1, Q = w + 2 * pad - ks + 1;
    AFCM_REQUIRE(P >= 1 && Q >= 1, "output must be at least 1x1");
    WgradPlan pl;
    const int rc = wgrad_plan(&pl, dtype, n, cin, cout, h, x_pitch ? x_pitch : w, ks, pad, P, Q, dy_pitch ? dy_pitch : Q, dots != 0);
    if (rc != AFCM_OK) return rc;
    out[0] = pl.kernel; out[1] = pl.pad_odd; out[2] = pl.x16 ? 1 : 0; out[3] = pl.small ? 1 : 0; out[4] = pl.splits; out[5] = pl.steps_per_split;
    out[6] = pl.reduce; out[7] = pl.splits_img;
    return AFCM_OK;
}
