// Dense KxK convolution for the modulated / encoder convs of the generator (NET:25-64, NET:505) on gfx950 MFMA.
//
// The reference materialises per-sample weights [N,O,I,k,k] and runs a grouped cuDNN conv (NET:46-63).
// Here the mathematically identical factorisation is used (the non-fused branch of CoModGAN/layers.py:56-65):
//     y[n,o] = d[n,o] * conv(W^, s[n,i] * x[n,i])          W^ shared by the whole batch
// so the contraction is one implicit GEMM  D[o][pixel] = sum_{tap,i} W^[tap][o][i] * xs[n][i][pixel+tap]  with
//   A = weights  (MFMA rows  = output channels), pre-packed K-contiguous by conv2d_pack_weights
//   B = activations (MFMA cols = output pixels), NCHW in HBM, transposed to [pixel][channel] while staging
//       into LDS so that every tap is a pure address offset of the same LDS patch (im2col never exists)
//   D = fp32 accumulators in registers; the per-(n,o) scale is applied in the epilogue.
// 16-bit 3x3 convs use v_mfma_f32_16x16x32_{bf16,f16} (conv2d_fwd16x_kernel), the stride-2 and 16-bit 1x1 convs v_mfma_f32_32x32x16_{bf16,f16};
// fp32 uses v_mfma_f32_32x32x2_f32 (exact fp32, for the <=1e-3 parity path).
// The same kernels compute the data gradient (weights packed transposed + flipped, pad' = k-1-pad).  The weight gradient is in
// conv2d_wgrad.hip, the per-plane passes (scaling, dot products, the fp32 split) in conv2d_planes.hip.
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "conv2d_common.h"
#include "flrelu_mfma_common.h"      // pack2<T>: one v_cvt_pk of exactly a pair

namespace afcm {

template <typename T> struct ConvCfg;
template <> struct ConvCfg<bf16_t> { static constexpr int BK = 16, PITCH = 24; };   // elements; 48-byte rows: conflict-free b128
template <> struct ConvCfg<f16_t>  { static constexpr int BK = 16, PITCH = 24; };
template <> struct ConvCfg<float>  { static constexpr int BK = 8,  PITCH = 9;  };   // 36-byte rows: conflict-free b32

// K-chunk (channels) of the packed weight image for (dtype, kernel size)
static inline int conv_bk(int dtype, int ks);
// conv2d_direct.hip: 16-bit 3x3 convs with at most four input channels (the generator's first layer)
int conv2d_direct_small_cin(const void* x, void* y, const void* wp, const float* oscale, const float* obias, int dtype, int n, int cin, int cout,
                            int h, int w, int pad, int rows_pad, int bk, int ldx, int ldy, hipStream_t st);

constexpr int kPatchMax = 416;   // LDS patch capacity in pixels
constexpr int kPlaneX16 = 416;    // pixels per channel-group plane of conv2d_fwd16x_kernel (a multiple of 16: planes 256 bytes apart) ...
constexpr int kPatchMaxX16 = kPlaneX16 - 4; // ... of which the patch may use all but the last four (the sink of the staging threads past the plane)
constexpr int kPatchMaxS2 = 704; // ... of the stride-2 kernel (two staging items per thread: <= 1024)
constexpr int kSlots = 256;      // output pixels per workgroup

struct ConvParams {
    const void* x;        // [N, Cin, H, W]
    void* y;              // [N, Cout, P, Q]
    const void* wp;       // packed weights [nkc][KK][Opad][BK]
    const float* oscale;  // [N * Cout] or null
    const float* obias;   // [Cout] or null: y = acc * oscale + obias
    int N, Cin, Cout, H, W, P, Q;
    int ldx, ldy;         // row pitch (elements) of x / y; = W / Q for dense tensors
    int pad;
    int TH, TW, PWL, tilesX, tilesY;
    int Opad, nkc;
    int total_blocks;     // conv2d_fwd16x_kernel (persistent workgroups): work items = tiles x images x row blocks; the grid may be smaller
    int o_base;           // conv2d_fwd16x_kernel: first output row of this launch (a layer may be split between the 128- and the 64-row kernel)
    unsigned magicTW;     // ceil(2^32 / TW): j / TW = umulhi(j, magicTW) for the tile-local pixel indices (j < 2^16)
    unsigned magicTX, magicTY, magicN, magicPC;   // ... / tilesX, tilesY, N (block index decode: dividend x divisor < 2^32), / (PWL / 4)
    // split-precision form (conv2d_fwd16x_kernel<bf16, BM, true>): x holds `parts` bf16 tensors [N, Cin, H, ldx] part_bytes apart,
    // the K loop runs over terms x nkc_real chunks, term t reads part (term_parts >> 4 t) & 15; y is fp32
    int nkc_real; unsigned magicNK, term_parts; int part_bytes, last_part_bytes;   // last_part_bytes: offset of the highest part any term reads
    const unsigned* bound_a; const unsigned* bound_b;   // magnitude-bound words of the two operands (or null): their power-of-two factors are undone in the epilogue
};

__host__ __device__ inline unsigned magic_u32(unsigned d) { return (unsigned)((0x100000000ull + d - 1) / d); }   // 0 for d = 1 (see udiv_magic)
__device__ __forceinline__ unsigned udiv_magic(unsigned n, unsigned magic) { return magic ? __umulhi(n, magic) : n; }

template <typename T, int BM_O, int KS>
__global__ __launch_bounds__(256, (sizeof(T) == 4 ? 1 : 2)) void conv2d_fwd_kernel(ConvParams p) {
    typedef ConvCfg<T> C;
    constexpr int BK = C::BK, PITCH = C::PITCH, MI = BM_O / 64, KK = KS * KS;
    constexpr bool F32 = sizeof(T) == 4;
    constexpr int EPV = 16 / sizeof(T);              // elements per 16-byte piece
    constexpr int PPR = BK / EPV;                    // pieces per weight row (2)
    constexpr int NPIECES = KK * BM_O * PPR;
    constexpr int NWP = cdiv(NPIECES, 256);
    __shared__ __attribute__((aligned(16))) T lds[(KK * BM_O + kPatchMax) * PITCH];
    T* lds_w = lds;
    T* lds_p = lds + KK * BM_O * PITCH;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wo = wave & 1, wpx = wave >> 1;
    const int r32 = lane & 31, h = lane >> 5;

    int bid = blockIdx.x;
    // integer division runs on the vector pipe even for uniform operands: pin the results to SGPRs, or everything derived
    // from them (image base, buffer descriptor) sits in VGPRs and every buffer load gets a waterfall loop around it
    const int tx = __builtin_amdgcn_readfirstlane(bid % p.tilesX); bid /= p.tilesX;
    const int ty = __builtin_amdgcn_readfirstlane(bid % p.tilesY); bid /= p.tilesY;
    const int n = __builtin_amdgcn_readfirstlane(bid % p.N);
    const int ob = __builtin_amdgcn_readfirstlane(bid / p.N);
    const int y0 = ty * p.TH, x0 = tx * p.TW;
    const int o0 = ob * BM_O;
    const int PH = p.TH + KS - 1, PWL = p.PWL;
    const int xorg = (x0 - p.pad) & ~1;
    const int xoff = (x0 - p.pad) - xorg;

    // fragment bases (element offsets into LDS)
    int bbase[4], pyv[4], pxv[4];
#pragma unroll
    for (int ti = 0; ti < 4; ti++) {
        const int j = wpx * 128 + ti * 32 + r32;
        int py = j / p.TW, px = j - py * p.TW;
        const bool valid = j < p.TH * p.TW;
        if (!valid) { py = 0; px = 0; }
        pyv[ti] = valid ? y0 + py : p.P;             // invalid slots fall outside the image -> never stored
        pxv[ti] = x0 + px;
        bbase[ti] = (py * PWL + px + xoff) * PITCH + h * (F32 ? 1 : 8);
    }
    int abase[MI];
#pragma unroll
    for (int mi = 0; mi < MI; mi++) abase[mi] = (wo * (BM_O / 2) + mi * 32 + r32) * PITCH + h * (F32 ? 1 : 8);

    f32x16 acc[MI][4];
#pragma unroll
    for (int mi = 0; mi < MI; mi++)
#pragma unroll
        for (int ti = 0; ti < 4; ti++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[mi][ti][e] = 0.f;

    // ---- staging descriptors -------------------------------------------------------------------------------
    // weights: 16-byte pieces, straight copies.  piece j = tid + 256*i -> (tap, o, half-row); 256 is a multiple of the
    // pieces per tap, so both addresses advance by a constant per i.
    constexpr int PPT = BM_O * PPR;                  // pieces per tap (256 or 128)
    constexpr int TPI = 256 / PPT;                   // taps advanced per i
    const int wq = tid % PPT, wtap0 = tid / PPT;
    const int wsrc0 = ((wtap0 * p.Opad) + o0 + wq / PPR) * BK + (wq % PPR) * EPV;
    const int wdst0 = (wtap0 * BM_O + wq / PPR) * PITCH + (wq % PPR) * EPV;
    const int wsrc_step = TPI * p.Opad * BK, wdst_step = TPI * BM_O * PITCH;
    const size_t wchunk = (size_t)KK * p.Opad * BK;
    // patch: one item = 4 pixels x 8 channels
    // lanes 0-31 / 32-63 of a wave take the two channel groups of the same 32 pixel groups: one load instruction then reads
    // two contiguous runs (one per channel) instead of two interleaved streams
    const int cg = F32 ? 0 : (tid >> 5) & 1, pg = F32 ? tid : (tid & 31) + 32 * (tid >> 6);
    const int pcols = PWL >> 2;
    const int prow = pg / pcols, pcol4 = pg - prow * pcols;
    const bool pvalid = prow < PH;
    const int iy = y0 - p.pad + prow, ix = xorg + 4 * pcol4;
    const bool rowok = pvalid && (unsigned)iy < (unsigned)p.H;
    const T* xn = (const T*)p.x + (size_t)n * p.Cin * p.H * p.W;
    const long long pix_off = (long long)(rowok ? iy : 0) * p.W + ix;
    const int pdst = (prow * PWL + 4 * pcol4) * PITCH + cg * 8;

    unsigned wreg[NWP][4];
    unsigned preg[8][F32 ? 4 : 2];
    // 16-bit patch loads are raw buffer loads of 8 bytes (4 pixels of one channel, 4-byte aligned): the row / column
    // validity of a thread never changes, so it is baked into the offset (out of range -> zeros, no branches); a group
    // that straddles the image border keeps its valid half through the and-masks below.
    constexpr unsigned kOob = 0x80000000u;
    const bool d0ok = rowok && (unsigned)ix < (unsigned)p.W, d1ok = rowok && (unsigned)(ix + 2) < (unsigned)p.W;
    const unsigned pmask0 = d0ok ? ~0u : 0u, pmask1 = d1ok ? ~0u : 0u;
    const bool any_partial = __builtin_amdgcn_ballot_w64(d0ok != d1ok) != 0;          // wave-uniform
    // a group whose first half lies left of the image loads from its second half instead (never touch bytes before a row 0)
    const bool lshift = !d0ok && d1ok;
    const bool any_lshift = __builtin_amdgcn_ballot_w64(lshift) != 0;
    const unsigned pvoff = (d0ok || d1ok) ? (unsigned)(((long long)cg * 8 * p.H * p.W + pix_off + (lshift ? 2 : 0)) * (long long)sizeof(T)) : kOob;
    const long long img_bytes = (long long)p.Cin * p.H * p.W * (long long)sizeof(T);
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void*)xn, 0, (int)(img_bytes > 0x7fffffffll ? 0x7fffffffll : img_bytes), 0x00020000);
    const int hw2 = p.H * p.W * (int)sizeof(T);

    auto issue_loads = [&](int kc) __attribute__((always_inline)) {
        const T* wsrcp = (const T*)p.wp + (size_t)kc * wchunk;
#pragma unroll
        for (int i = 0; i < NWP; i++)
            if ((NPIECES % 256 == 0) || tid + i * 256 < NPIECES) {
                const uint4 t = *(const uint4*)(wsrcp + wsrc0 + i * wsrc_step);
                wreg[i][0] = t.x; wreg[i][1] = t.y; wreg[i][2] = t.z; wreg[i][3] = t.w;
            }
        if constexpr (F32) {
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const int ch = kc * BK + cg * 8 + c;
                const bool chok = rowok && ch < p.Cin;
                const T* src = xn + ((long long)ch * p.H * p.W + pix_off);
#pragma unroll
                for (int e = 0; e < 4; e++) preg[c][e] = (chok && (unsigned)(ix + e) < (unsigned)p.W) ? *(const unsigned*)(src + e) : 0u;
            }
        } else {
            // channels past Cin only exist in the last chunk: they read whatever follows (or zeros past the image) and are
            // cleared below; everything else needs no per-load work: the chunk's channel offset rides in the scalar offset
            const bool tailchunk = (kc + 1) * BK > p.Cin;
#pragma unroll
            for (int c = 0; c < 8; c++) {
                typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
                const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(xrs, pvoff, (kc * BK + c) * hw2, 0);
                preg[c][0] = v.x; preg[c][1] = v.y;
            }
            if (tailchunk) {
#pragma unroll
                for (int c = 0; c < 8; c++)
                    if (kc * BK + cg * 8 + c >= p.Cin) { preg[c][0] = 0u; preg[c][1] = 0u; }
            }
        }
    };
    auto write_lds = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NWP; i++)
            if ((NPIECES % 256 == 0) || tid + i * 256 < NPIECES) {
                if (F32) {
                    unsigned* d = (unsigned*)(lds_w + wdst0 + i * wdst_step);
                    d[0] = wreg[i][0]; d[1] = wreg[i][1]; d[2] = wreg[i][2]; d[3] = wreg[i][3];
                } else {
                    *(uint4*)(lds_w + wdst0 + i * wdst_step) = make_uint4(wreg[i][0], wreg[i][1], wreg[i][2], wreg[i][3]);
                }
            }
        if (pvalid) {
            if (F32) {
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    unsigned* d = (unsigned*)(lds_p + pdst + e * PITCH);
#pragma unroll
                    for (int c = 0; c < 8; c++) d[c] = preg[c][e];
                }
            } else {
                if (any_lshift) {
#pragma unroll
                    for (int c = 0; c < 8; c++) preg[c][1] = lshift ? preg[c][0] : preg[c][1];
                }
                if (any_partial) {
#pragma unroll
                    for (int c = 0; c < 8; c++) { preg[c][0] &= pmask0; preg[c][1] &= pmask1; }
                }
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const unsigned sel = (e & 1) ? 0x07060302u : 0x05040100u;
                    uint4 v;
                    v.x = __builtin_amdgcn_perm(preg[1][e >> 1], preg[0][e >> 1], sel);
                    v.y = __builtin_amdgcn_perm(preg[3][e >> 1], preg[2][e >> 1], sel);
                    v.z = __builtin_amdgcn_perm(preg[5][e >> 1], preg[4][e >> 1], sel);
                    v.w = __builtin_amdgcn_perm(preg[7][e >> 1], preg[6][e >> 1], sel);
                    *(uint4*)(lds_p + pdst + e * PITCH) = v;
                }
            }
        }
    };

    issue_loads(0);
    write_lds();
    __syncthreads();
    for (int kc = 0; kc < p.nkc; kc++) {
        if (kc + 1 < p.nkc) issue_loads(kc + 1);
#pragma unroll
        for (int r = 0; r < KS; r++)
#pragma unroll
            for (int s = 0; s < KS; s++) {
                const int tap = r * KS + s;
                const int tapoff = (r * PWL + s) * PITCH;
                if constexpr (F32) {
#pragma unroll
                    for (int k2 = 0; k2 < BK / 2; k2++) {
                        float a[MI], b[4];
#pragma unroll
                        for (int mi = 0; mi < MI; mi++) a[mi] = lds_w[tap * BM_O * PITCH + abase[mi] + 2 * k2];
#pragma unroll
                        for (int ti = 0; ti < 4; ti++) b[ti] = lds_p[bbase[ti] + tapoff + 2 * k2];
#pragma unroll
                        for (int mi = 0; mi < MI; mi++)
#pragma unroll
                            for (int ti = 0; ti < 4; ti++)
                                acc[mi][ti] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi], b[ti], acc[mi][ti], 0, 0, 0);
                    }
                } else {
                    typedef typename std::conditional<std::is_same<T, bf16_t>::value, bf16x8, f16x8>::type frag_t;
                    frag_t a[MI], b[4];
#pragma unroll
                    for (int mi = 0; mi < MI; mi++) a[mi] = *(const frag_t*)(lds_w + tap * BM_O * PITCH + abase[mi]);
#pragma unroll
                    for (int ti = 0; ti < 4; ti++) b[ti] = *(const frag_t*)(lds_p + bbase[ti] + tapoff);
#pragma unroll
                    for (int mi = 0; mi < MI; mi++)
#pragma unroll
                        for (int ti = 0; ti < 4; ti++) {
                            if constexpr (std::is_same<T, bf16_t>::value)
                                acc[mi][ti] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi], b[ti], acc[mi][ti], 0, 0, 0);
                            else
                                acc[mi][ti] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[mi], b[ti], acc[mi][ti], 0, 0, 0);
                        }
                }
            }
        __syncthreads();
        if (kc + 1 < p.nkc) {
            write_lds();
            __syncthreads();
        }
    }

    // ---- epilogue: D[row = channel][col = pixel]; row = (reg&3) + 8*(reg>>2) + 4*h within the 32x32 tile.
    T* yn = (T*)p.y + (size_t)n * p.Cout * p.P * p.Q;
    // per output-row block: all per-channel scales and biases first (clamped index, no branch around the loads: one wait
    // instead of a round trip per row), then the stores
    int poff[4];                                     // pixel offset inside a plane, -1: not stored
#pragma unroll
    for (int ti = 0; ti < 4; ti++) poff[ti] = (pyv[ti] < p.P && pxv[ti] < p.Q) ? pyv[ti] * p.Q + pxv[ti] : -1;
    const float* osn = p.oscale ? p.oscale + (size_t)n * p.Cout : nullptr;
    const int pq = p.P * p.Q;
#pragma unroll
    for (int mi = 0; mi < MI; mi++) {
        float sc[16], ob[16];
        const int obase = o0 + wo * (BM_O / 2) + mi * 32 + 4 * h;
#pragma unroll
        for (int reg = 0; reg < 16; reg++) { sc[reg] = 1.f; ob[reg] = 0.f; }
        if (osn != nullptr) {
#pragma unroll
            for (int reg = 0; reg < 16; reg++) sc[reg] = osn[min(obase + (reg & 3) + 8 * (reg >> 2), p.Cout - 1)];
        }
        if (p.obias != nullptr) {
#pragma unroll
            for (int reg = 0; reg < 16; reg++) ob[reg] = p.obias[min(obase + (reg & 3) + 8 * (reg >> 2), p.Cout - 1)];
        }
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            const int o = obase + (reg & 3) + 8 * (reg >> 2);
            if (o < p.Cout) {
                T* yo = yn + (size_t)o * pq;
#pragma unroll
                for (int ti = 0; ti < 4; ti++)
                    if (poff[ti] >= 0) yo[poff[ti]] = from_f32<T>(acc[mi][ti][reg] * sc[reg] + ob[reg]);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// 16-bit 3x3 forward / data-gradient kernel.  Tile: BM_O channels x 256 pixels, 4 waves as 2(o) x 2(pixel halves), wave tile
// (BM_O / 2) x 128 = MO x 8 accumulator tiles of v_mfma_f32_16x16x32, 2 workgroups per CU.  Kept from the r02 structure (a 32x32x16
// kernel on K-chunks of 16 channels; DESIGN.md, "Retired build switches"):
//   * weights never touch LDS: the packed layout already IS the A-fragment image, so every wave loads its fragments straight from
//     L2 into a register ring, taps ahead of their MFMAs;
//   * the activation patch (transposed NCHW -> [pixel][channel] while staging) is double-buffered in LDS: ONE barrier per K-chunk,
//     and the transposing ds_writes sit among the MFMAs of the running chunk;
//   * XCD-aware tile order: neighbouring tiles of one image (shared halos, same weights) stay on one XCD's L2.
// Measured bounds of the r02 kernel (ablation builds, whole-generator conv bench, baseline 0.92 / 0.96 PF/s fwd / dgrad): weight
// fragments served from L1 +2 %; no barrier +0 %; B fragments read once per chunk +5 %; patch written later in the chunk +0 %; the
// four transposing ds_write_b128 removed (loads and permutes kept) +19 %; the whole activation path removed +38 %.  So the register
// -> LDS transpose that NCHW forces is the limiter; LDS-DMA + ds_read_b64_tr_b16 cannot replace it because the transposing read
// ignores the low three address bits (tools/ubench/tr_align_probe.hip) and the tap columns shift by 1 and 2 pixels.
// r05 moved the tile to v_mfma_f32_16x16x32: the 32x32x16 kernel's >= 256-channel layers held ~1.5 GHz under their MFMA load (all-zero
// operands: +23 %, profiles/r04_power_probe.txt), and on a clock-limited loop the chip holds a higher clock on the 16x16x32 shape than
// on 32x32x16 at equal cycles per flop (MI355X_MICROARCH.md, DVFS give-back item 7).  Same accumulator registers, same operand bytes
// per MFMA cycle; what changed:
//   * a K step is 32 channels of one tap: K-chunks of 32 channels (packed weights [kc][tap][Opad][32], a lane's fragment = 16 bytes at
//     row (lane & 15), channel group (lane >> 4); a wave still reads one contiguous 1 KB per fragment), half as many barriers;
//   * the LDS patch is PLANAR: four planes [channel group of 8][pixel][8 channels], a pixel = 16 bytes, planes a multiple of 256 bytes
//     apart.  A B fragment is 16 consecutive pixels x 4 channel groups; ds_read_b128 serves lanes in four groups of 16 that each hold all
//     16 pixel columns with two of the channel groups, so every group reads 16 consecutive 16-byte slots = all 64 banks once, at any
//     pixel offset (taps shift by 1 and 2 pixels) -- no padding (the [pixel][32 channels] row form conflicts for every odd pitch);
//     a plane holds kPlaneX16 = 416 pixels (patch <= 412 + a 4-pixel sink for the staging threads whose group lies past the patch: no predicate);
//   * B fragments live in a ring of four, read four 16-pixel blocks ahead of their MFMAs (one fragment feeds MO MFMAs = 64 cycles);
//     the tap's column offset is the read's immediate, the row offset is added to the block's base register in place: 32 vector adds
//     per chunk of 72 reads;
//   * weight fragments: buffer loads (lane offset + scalar tap offset: no vector address arithmetic), ring of three taps refilled in
//     place after the tap's last MFMA;
//   * staging: a thread owns 4 pixels x 2 items of 8 channels; one register set, item 0 requested at the top of the chunk and written
//     under tap 4, item 1 requested under tap 5 and written under tap 8.  Lanes 2, 3 (mod 4) of a group write their pixel pairs in
//     swapped order (the permute's selector is a register): 2-way instead of 4-way conflicts on the transposing 16-byte writes;
//   * the issue order is the source order: the loop is written as 72 steps (MO MFMAs, the read four steps ahead, a slice of the
//     staging work) with a scheduling barrier after each.  Left to the scheduler (sched_group_barrier pipelines, as
//     in the r02 kernel) the MFMAs of different taps were reordered around the reads and every read was waited for at once.
// FASTEPI (r06): tiles whose width is a multiple of 16 pixels on rows whose pitch is a multiple of 8 elements (the 276^2 / 278^2 and 256^2
// planes of the generator: 8 x 32 and 4 x 64 tiles on 288- and 256-element rows).  A 16-pixel block of the tile then lies in ONE tile row,
// so the row and column base of its two 8-pixel granules are wave-uniform: they are computed on the scalar unit and ride in the store's
// scalar offset (the general form computes eight granule coordinates, validity and straddle flags per lane and tile: ~170 of the ~270
// vector instructions of a 64-row epilogue), a granule never straddles a tile row or the pitched image row (no pair path), and the B
// fragment bases of a tile are one vector add each (set_bbyte: 8 instead of ~64).  Same stores, same bytes.
template <typename T, int BM_O, bool SPLIT = false, bool FASTEPI = false>
__global__ __launch_bounds__(256, 2) void conv2d_fwd16x_kernel(ConvParams p) {
    static_assert(sizeof(T) == 2, "16-bit types only");
    static_assert(!(SPLIT && FASTEPI), "the fp32-output epilogue has no fast form");
    typedef typename std::conditional<SPLIT, float, T>::type TO;      // output element
    // B fragments: a ring read BRING 16-pixel blocks ahead of their MFMAs.  MO = 4: four (a block = 64 MFMA cycles); MO = 2: three -- a block
    // is 32 cycles, but the three waves of a SIMD take turns, and the fourth slot is the register that decides between 168 (three waves
    // per SIMD) and 169
    constexpr int KS = 3, KK = 9, BK = 32, MO = BM_O / 32, NT = 8, BRING = MO == 4 ? 4 : 3;
    // weight-fragment ring, in fragments: a chunk's KK * MO fragments (tap-major) cycle through ARING slots.  MO = 4: 9 slots = 2.25 taps
    // (3 taps = 48 registers do not fit beside 128 accumulator registers at two waves per SIMD); MO = 2: 6 slots = 3 taps
    constexpr int ARING = MO == 2 ? 6 : 9;
    static_assert((KK * MO) % ARING == 0 && ARING >= 2 * MO, "static slots; a tap's fragments and the next tap's are live together");
    // bytes of one channel-group plane: kPlaneX16 = 416 pixels.  2 buffers x 4 planes = 53,248 bytes per workgroup.  The patch itself may
    // use kPatchMaxX16 = 412 pixels: the last four are the sink of the staging threads whose pixel group lies past the plane (branch-free
    // staging writes every thread's four pixels).  Occupancy: two workgroups per CU for both block heights.  The 64-row kernel fits three
    // by registers (<= 168) and LDS (159,744 of 163,840 bytes) on paper; the wave counters show ~1.7 alive (SQ_WAVE_CYCLES x 4 = 58 % of
    // the dispatch), a grid of two per CU runs as fast as one of three (profiles/r05_conv_persistent.txt), and FORCING three
    // (__launch_bounds__(256, 3), 51 KB planes) cost 17 spilled registers and 15-20 % on those layers: the register budget stays at two
    // (__launch_bounds__(256, 2)); the persistent 64-row launch still sizes its grid for three per CU (conv_persistent_grid(blocks, 3)) so
    // that a CU that does fit a third workgroup gets one.
    constexpr int PLANE_B = kPlaneX16 * 16;
    constexpr int BUF_B = 4 * PLANE_B;
    static_assert(PLANE_B % 256 == 0 && kPatchMaxX16 % 4 == 0, "planes: a multiple of 256 bytes apart, patch + sink inside");
    typedef typename std::conditional<std::is_same<T, bf16_t>::value, bf16x8, f16x8>::type frag_t;
    typedef __attribute__((ext_vector_type(4))) float f32x4;
    typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
    typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
    __shared__ __attribute__((aligned(256))) unsigned char lds[2 * BUF_B];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wo = wave & 1, wpx = wave >> 1;
    const int c16 = lane & 15, g = lane >> 4;
    const int PH = p.TH + KS - 1, PWL = p.PWL;

    // ---- work items.  The workgroup is PERSISTENT (r05): it takes tiles item, item + gridDim.x, ... (the host launches one round of
    // resident workgroups, a multiple of 8: an item's XCD-aware position, xcd_order(), is then the same function of the item index as it
    // was of the hardware block index) and requests the first K-chunk of its NEXT tile during the last K-chunk of the one under way --
    // the staging slots of that chunk used to issue dead loads -- so that a tile starts on a patch that is already in LDS.  What that
    // hides: a new workgroup needed 7-15k cycles from its first instruction to its first barrier (its address set-up is issued
    // in the slots two MFMA-dense older waves leave, then a memory round trip: profiles/r05_conv_prologue_stamps.txt), a quarter of a
    // workgroup's life on the <= 128-channel layers.
    // The 128-row kernel is not persistent: carrying a second tile's staging state across the K loop costs it, at 250 of its 256
    // registers, 19-52 spilled registers in every form tried (its workgroups live 150-200k cycles, the prologue is 3 % of that); the
    // 64-row kernel -- the <= 64-channel and the 181-channel layers, where the prologue is a quarter -- fits in the 168 registers of
    // three waves per SIMD; the 96-row kernel, at two per CU, in 228 registers without spills (3-7 % on the 91-row
    // launches, profiles/r05_conv_bm96_ab.txt).  A non-persistent launch has one item per workgroup (the host sizes the grid accordingly).
    constexpr bool PERSIST = BM_O == 64 || BM_O == 96;
    struct Tile { int y0, x0, n, o0; };
    auto decode = [&](int it) __attribute__((always_inline)) -> Tile {
        const int bid = xcd_order(it, p.total_blocks);
        // block index -> (tile x, tile y, image, row block): multiplications by host-made reciprocals, results pinned to SGPRs
        const unsigned q0 = udiv_magic((unsigned)bid, p.magicTX);
        const int tx = __builtin_amdgcn_readfirstlane(bid - (int)q0 * p.tilesX);
        const unsigned q1 = udiv_magic(q0, p.magicTY);
        const int ty = __builtin_amdgcn_readfirstlane((int)q0 - (int)q1 * p.tilesY);
        const unsigned q2 = udiv_magic(q1, p.magicN);
        const int n = __builtin_amdgcn_readfirstlane((int)q1 - (int)q2 * p.N);
        const int ob = __builtin_amdgcn_readfirstlane((int)q2);
        return Tile{ty * p.TH, tx * p.TW, n, p.o_base + ob * BM_O};
    };

    f32x4 acc[MO][NT];

    // ---- A fragments: straight from the packed weights (one buffer: the whole image, < 2^31 bytes -- host)
    const int wtap_b = p.Opad * BK * 2;                                    // bytes per tap
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void*)p.wp, 0, p.nkc * KK * wtap_b, 0x00020000);
    // ONE lane offset; the row block (o0), the tap and the fragment ride in the scalar offset (as vector offsets the compiler kept four
    // registers per row block in flight: lane offset + 1 KB per fragment)
    const unsigned wlane = (unsigned)(((wo * (BM_O / 2) + c16) * BK + g * 8) * 2);
    auto load_a = [&](int o0s, int kc, int tap, int mo) __attribute__((always_inline)) {
        return __builtin_bit_cast(frag_t, __builtin_amdgcn_raw_buffer_load_b128(wrs, wlane, (kc * KK + tap) * wtap_b + (o0s + mo * 16) * (BK * 2), 0));
    };

    // ---- patch staging: thread = (channel-group parity cg, 4-pixel group pg); item it covers channel group 2 it + cg.
    // Tile-independent geometry first
    const int cg = (tid >> 5) & 1, pg = (tid & 31) + 32 * (tid >> 6);
    const int pcols = PWL >> 2;
    constexpr unsigned kOob = 0x80000000u;
    const long long img_bytes = (long long)p.Cin * p.H * p.ldx * 2ll + (SPLIT ? (long long)p.last_part_bytes : 0ll);
    const int img_records = (int)(img_bytes > 0x7fffffffll ? 0x7fffffffll : img_bytes);
    const int hw2 = p.H * p.ldx * 2;
    // the patch is dense in pixels (PWL = 4 pcols): this thread's pixels are 4 pg .. 4 pg + 3 -- inside the plane whether or not the
    // patch has that row, except for the groups past the plane's end: those write the sink pixels.  Pixel written at step e: e ^ rot
    const int rot = (pg >> 1) & 1;
    const int pgd = 4 * pg < kPatchMaxX16 ? 4 * pg : kPatchMaxX16;
    // steps 0, 2 (+ 32 bytes at step 2): address pdst_a, selector sel_a; steps 1, 3: the other pixel of the pair = pdst_a ^ 16, the other
    // halves = sel_a ^ 0x02020202 (two registers instead of four across the loop)
    const unsigned pdst_a = (unsigned)(pgd * 16 + cg * PLANE_B + rot * 16);
    const unsigned sel_a = rot ? 0x07060302u : 0x05040100u;
    // ... then the state of the tile whose chunks are being STAGED (the tile under way, or the next one during its last chunk)
    unsigned pvoff = kOob, pm_lo = 0, pm_hi = 0;
    bool lshift = false;
    __amdgpu_buffer_rsrc_t xrs = wrs;
    auto stage_tile = [&](const Tile& t) __attribute__((always_inline)) {
        // (the thread's patch coordinates are recomputed from an opaque copy of its index: kept live across the tile loop they -- and
        // everything else the compiler can hoist out of it -- cost the 128-row kernel 52 spilled registers and the 64-row kernel its
        // third workgroup per CU)
        int tid_o = tid;
        asm volatile("" : "+v"(tid_o));
        const int pg_o = (tid_o & 31) + 32 * (tid_o >> 6), cg_o = (tid_o >> 5) & 1;
        const int prow = (int)udiv_magic((unsigned)pg_o, p.magicPC), pcol4 = pg_o - prow * pcols;
        const bool pvalid = prow < PH;
        const int cg = cg_o;
        const int xorg = (t.x0 - p.pad) & ~1;
        const int iy = t.y0 - p.pad + prow, ix = xorg + 4 * pcol4;
        const bool rowok = pvalid && (unsigned)iy < (unsigned)p.H;
        const long long pix_off = (long long)(rowok ? iy : 0) * p.ldx + ix;
        const bool d0ok = rowok && (unsigned)ix < (unsigned)p.W, d1ok = rowok && (unsigned)(ix + 2) < (unsigned)p.W;
        lshift = !d0ok && d1ok;                                                       // never touch bytes before a row 0
        pm_lo = (d0ok && !lshift) ? ~0u : 0u;
        pm_hi = d1ok ? ~0u : 0u;
        pvoff = (d0ok || d1ok) ? (unsigned)(((long long)cg * 8 * p.H * p.ldx + pix_off + (lshift ? 2 : 0)) * 2ll) : kOob;
        // (the descriptor ends with the image -- split form: with the highest part read -- so channels past Cin read zeros in the plain form)
        xrs = __builtin_amdgcn_make_buffer_rsrc((void*)((const T*)p.x + (size_t)t.n * p.Cin * p.H * p.ldx), 0, img_records, 0x00020000);
    };

    // Branch-free, and issued on EVERY chunk (past the last one of the last tile with the out-of-range offset: zeros, no memory
    // traffic): a conditional issue makes the compiler's s_waitcnt for the weight ring assume the path without these loads, and on
    // the path with them that count waits for all of them -- a full memory round trip exposed at the top of every chunk.
    auto issue_patch = [&](unsigned (&pr)[8][2], int kc, bool live, int item) __attribute__((always_inline)) {
        int kcr = kc, sbase = 0;                           // chunk inside its term, byte offset of the term's part (scalar unit)
        if constexpr (SPLIT) {
            const int term = (int)udiv_magic((unsigned)kc, p.magicNK);
            kcr = kc - term * p.nkc_real;
            sbase = (int)((p.term_parts >> (4 * term)) & 15u) * p.part_bytes;
        }
        const int cbase = kcr * BK + item * 16 + cg * 8;
        const int climit = live ? p.Cin : 0;
        const unsigned voff = live ? pvoff : kOob;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            unsigned off = voff;
            if constexpr (SPLIT) off = (cbase + c < climit) ? pvoff : kOob;     // the descriptor runs on into the next part
            const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(xrs, off, sbase + (kcr * BK + item * 16 + c) * hw2, 0);
            pr[c][0] = v.x; pr[c][1] = v.y;
        }
    };
    // edge masks of one channel's two dwords (pixels 0, 1 | 2, 3): unconditional -- any branch here (even a wave-uniform one) cuts
    // the tap loop into basic blocks, and the transpose then runs as one serial block with no MFMA in flight
    auto mask_ch = [&](unsigned (&pr)[8][2], int c) __attribute__((always_inline)) {
        const unsigned lo = pr[c][0] & pm_lo;
        const unsigned hi = (lshift ? pr[c][0] : pr[c][1]) & pm_hi;
        pr[c][0] = lo; pr[c][1] = hi;
    };
    // step e of the transposing write: 8 channels of one pixel = 16 bytes; sbyte: buffer + item planes (scalar)
    auto write_px = [&](unsigned (&pr)[8][2], int e, int sbyte) __attribute__((always_inline)) {
        const unsigned sel = (e & 1) ? (sel_a ^ 0x02020202u) : sel_a;
        u32x4 v;
        v.x = __builtin_amdgcn_perm(pr[1][e >> 1], pr[0][e >> 1], sel);
        v.y = __builtin_amdgcn_perm(pr[3][e >> 1], pr[2][e >> 1], sel);
        v.z = __builtin_amdgcn_perm(pr[5][e >> 1], pr[4][e >> 1], sel);
        v.w = __builtin_amdgcn_perm(pr[7][e >> 1], pr[6][e >> 1], sel);
        *(u32x4*)(lds + ((e & 1) ? (pdst_a ^ 16u) : pdst_a) + (unsigned)sbyte + (e >> 1) * 32) = v;
    };
    // this lane's eight B fragments: bbyte[ti] = byte address of the fragment of the tap ROW under way in the buffer under way (tile-local
    // pixel 128 wpx + 16 ti + lane & 15, channel group lane >> 4) -- walks down the patch rows and over to the other buffer in place;
    // set at the start of a tile (its xoff, the buffer its first chunk is in)
    unsigned bbyte[NT];
    auto set_bbyte = [&](const Tile& t, int buf) __attribute__((always_inline)) {
        const int xoff = (t.x0 - p.pad) & 1;
        int lane_o = tid;                                    // (opaque: see stage_tile; from tid: one register less across the loop than tid AND lane)
        asm volatile("" : "+v"(lane_o));
        lane_o &= 63;
        if constexpr (FASTEPI) {
            // a 16-pixel block lies in one tile row: its row and first column are scalar
            const unsigned lanepart = (unsigned)((lane_o & 15) * 16 + (lane_o >> 4) * PLANE_B);
#pragma unroll
            for (int ti = 0; ti < NT; ti++) {
                const int b16 = wpx * 128 + ti * 16;
                int py = (int)__umulhi((unsigned)b16, p.magicTW), px = b16 - py * p.TW;
                if (b16 >= p.TH * p.TW) { py = 0; px = 0; }
                bbyte[ti] = lanepart + (unsigned)((py * PWL + px + xoff) * 16 + buf * BUF_B);
            }
            return;
        }
#pragma unroll
        for (int ti = 0; ti < NT; ti++) {
            const int j = wpx * 128 + ti * 16 + (lane_o & 15);
            int py = (int)__umulhi((unsigned)j, p.magicTW), px = j - py * p.TW;
            if (j >= p.TH * p.TW) { py = 0; px = 0; }
            bbyte[ti] = (unsigned)((py * PWL + px + xoff) * 16 + (lane_o >> 4) * PLANE_B + buf * BUF_B);
        }
    };

    // ---- the first tile of this workgroup: the one exposed prologue
    int item = blockIdx.x;
    Tile S = decode(item);
    stage_tile(S);
    frag_t ar[ARING];
    unsigned preg[8][2];
    {
        unsigned preg1[8][2];                                // the prologue requests both items at once (the accumulators are not live yet)
        issue_patch(preg, 0, true, 0);
        issue_patch(preg1, 0, true, 1);
#pragma unroll
        for (int q = 0; q < ARING; q++) ar[q] = load_a(S.o0, 0, q / MO, q % MO);
#pragma unroll
        for (int c = 0; c < 8; c++) { mask_ch(preg, c); mask_ch(preg1, c); }
#pragma unroll
        for (int e = 0; e < 4; e++) { write_px(preg, e, 0); write_px(preg1, e, 2 * PLANE_B); }
    }
    int cb = 0;                                              // buffer of the chunk under way
    set_bbyte(S, cb);
    __syncthreads();

    const int last = p.nkc - 1;
    const unsigned rowstep = (unsigned)(PWL * 16);
    for (;;) {
        const int item_n = item + (int)gridDim.x;
        const bool has_next = PERSIST && item_n < p.total_blocks;
#pragma unroll
        for (int mo = 0; mo < MO; mo++)
#pragma unroll
            for (int ti = 0; ti < NT; ti++) acc[mo][ti] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int kc = 0; kc < p.nkc; kc++) {
            const bool fin = kc == last;                    // the tile's last chunk stages chunk 0 of the next tile
            int o0_n = S.o0;                                // row block of the chunk after this one
            if (PERSIST && fin) {
                const Tile N = decode(has_next ? item_n : item);     // (decoded where it is needed: four scalars less across the K loop)
                stage_tile(N);
                o0_n = N.o0;
            }
            const int nxt_b = (cb ^ 1) * BUF_B;
            const bool more = !fin || has_next;
            const int knext = fin ? 0 : kc + 1;
            const unsigned bufstep = (unsigned)((cb ? -BUF_B : BUF_B) - 2 * (int)rowstep);     // to tap row 0 of the other buffer
            frag_t b[BRING];
#pragma unroll
            for (int s = 0; s < BRING; s++) b[s] = *(const frag_t*)(lds + bbyte[s]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int tap = 0; tap < KK; tap++) {
#pragma unroll
                for (int ti = 0; ti < NT; ti++) {
                    const int s = tap * NT + ti;
#pragma unroll
                    for (int mo = 0; mo < MO; mo++) {
                        if constexpr (std::is_same<T, bf16_t>::value)
                            acc[mo][ti] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ar[(tap * MO + mo) % ARING], b[s % BRING], acc[mo][ti], 0, 0, 0);
                        else
                            acc[mo][ti] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ar[(tap * MO + mo) % ARING], b[s % BRING], acc[mo][ti], 0, 0, 0);
                    }
                    const int s2 = s + BRING;
                    if (s2 < KK * NT) {
                        const int t2 = s2 / NT, ti2 = s2 % NT;
                        if (t2 > 0 && t2 % KS == 0) bbyte[ti2] += rowstep;                 // first tap of the next patch row
                        b[s % BRING] = *(const frag_t*)(lds + bbyte[ti2] + (t2 % KS) * 16);
                    }
                    // ---- this step's slice of the staging work
                    if (tap == 0 && ti == 0) issue_patch(preg, knext, more, 0);
                    if (tap == 5 && ti == 0) issue_patch(preg, knext, more, 1);
                    if (tap == 4 || tap == 8) {
                        // item 0 (tap 4) / item 1 (tap 8) of the next chunk into the other buffer: masks under blocks 0-3, a pixel under each of 4-7
                        if (ti < 4) { mask_ch(preg, 2 * ti); mask_ch(preg, 2 * ti + 1); }
                        else write_px(preg, ti - 4, nxt_b + (tap == 8 ? 2 * PLANE_B : 0));
                    }
                    if (tap == 8 && ti >= 4) { bbyte[2 * (ti - 4)] += bufstep; bbyte[2 * (ti - 4) + 1] += bufstep; }   // (the chunk's reads are done)
                    if (ti == NT - 1) {
                        // the tap's ring slots take the fragments ARING ahead now that its MFMAs have read them (past the last tile: the same
                        // fragments again -- no branch around a load)
#pragma unroll
                        for (int mo = 0; mo < MO; mo++) {
                            const int q = tap * MO + mo, q2 = q + ARING;
                            ar[q % ARING] = (q2 < KK * MO) ? load_a(S.o0, kc, q2 / MO, q2 % MO) : load_a(o0_n, knext, (q2 - KK * MO) / MO, q2 % MO);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            cb ^= 1;
            __syncthreads();
        }
        // ---- epilogue of tile S: a 16 x 16 tile has its pixel on the lane (col = lane & 15) and channels 4 g .. 4 g + 3 in the 4 registers
        // (the lane id goes through an empty asm: otherwise pixel coordinates computed for the K loop are kept -- spilled -- for the stores
        // below instead of being recomputed)
        int lane_e = tid;
        asm volatile("" : "+v"(lane_e));
        lane_e &= 63;
        const int c16e = lane_e & 15, ge = lane_e >> 4;
        const int y0 = S.y0, x0 = S.x0, n = S.n, o0 = S.o0;
        if constexpr (!SPLIT) {
            // per 32-channel pass stage [pixel][32 channels] rows (64 bytes, 8-byte chunk c of pixel p at
            // c ^ ((p >> 1) & 7)) and read them back transposed; here a lane stages ONE 8-byte chunk per tile (channels 16 (mo & 1) + 4 g ..),
            // 64 pixels at a time: the staging area (4 KB per wave) lies in the patch buffer the last chunk read -- the other one already
            // holds the next tile's first chunk.
            // For EVERY tile width (even): a granule of 8 tile-local pixels that stays inside one tile row and the image goes out as 16
            // bytes, one that runs over a row end (tile widths that are not multiples of 8: the 5 x 50 tiles of the 150-wide planes, 28, 42)
            // as four pixel pairs with their own coordinates.  (r05: the per-element path below took 86k cycles per workgroup on those
            // tiles -- 16 lanes x 2 bytes per run -- against 10k for this one; it remains for fp32 output.)
            typedef __attribute__((ext_vector_type(4))) short s16x4;
            typedef __attribute__((ext_vector_type(4))) unsigned eu32x4;
            constexpr int EROW = 64;
            unsigned char* const ebuf = lds + (cb ^ 1) * BUF_B + wave * (64 * EROW);
            const int pq = p.P * p.ldy;
            const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc((void*)((T*)p.y + (size_t)n * p.Cout * pq), 0, p.Cout * pq * 2, 0x00020000);
            const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.oscale ? p.oscale + (size_t)n * p.Cout : (const float*)p.y), 0, p.oscale ? p.Cout * 4 : 0, 0x00020000);
            const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.obias ? p.obias : (const float*)p.y), 0, p.obias ? p.Cout * 4 : 0, 0x00020000);
            constexpr unsigned kGOut = 0x80000000u, kOOut = 0xc0000000u;
            const bool has_sc = p.oscale != nullptr, has_ob = p.obias != nullptr;
            f32x4 sc[MO], ob[MO];
#pragma unroll
            for (int mo = 0; mo < MO; mo++) {
                const unsigned sboff = (unsigned)((o0 + wo * (BM_O / 2) + mo * 16 + 4 * ge) * 4);
                sc[mo] = (f32x4){1.f, 1.f, 1.f, 1.f};
                ob[mo] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (has_sc) sc[mo] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srs, sboff, 0, 0));
                if (has_ob) ob[mo] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(brs, sboff, 0, 0));
            }
            // read side: lane = (half hh: granule parity, chalf: channel half, i16: channel / address role inside the 16-lane group)
            const int i16 = lane_e & 15, chalf = (lane_e >> 4) & 1, hh = lane_e >> 5;
            const int q4 = i16 >> 2, p4 = i16 & 3;
            unsigned rd_off[2];
#pragma unroll
            for (int r = 0; r < 2; r++) {
                const int prw = 8 * hh + 4 * r + q4;                 // + 16 pixels per iteration: (prw >> 1) & 7 does not change
                rd_off[r] = prw * EROW + (((chalf * 4 + p4) ^ ((prw >> 1) & 7)) << 3);
            }
            // write side: pixel 16 ti + c16 (its swizzle (pix >> 1) & 7 does not depend on ti), chunk 4 (mo & 1) + g
            unsigned wr_off[2];
#pragma unroll
            for (int k = 0; k < 2; k++) wr_off[k] = (unsigned)(c16e * EROW + (((4 * k + ge) ^ ((c16e >> 1) & 7)) << 3));
            // gfullm bit `it`: this lane's granule goes out as 16 bytes (one tile row, inside the (pitched) image row) -- or not at all (a
            // granule outside the tile or the image: its offset carries the marker); slow_any bit `it` (wave-uniform): SOME lane's granule of
            // iteration `it` needs the pair-by-pair path.  That path is behind a SCALAR branch: under a per-lane predicate only, its ~40
            // vector instructions per granule (two quarter-rate multiplies per pixel pair) were issued with an empty EXEC mask on every tile
            // -- ~3k issue cycles per wave and tile, a third of what a tile of a 64-channel layer has to issue at all.
            unsigned gbyte[8], gfullm = 0, slow_any = 0;
#pragma unroll
            for (int it = 0; it < (FASTEPI ? 0 : 8); it++) {
                const int j0 = wpx * 128 + (2 * it + hh) * 8;
                const int gpy = (int)__umulhi((unsigned)j0, p.magicTW), gpx = j0 - gpy * p.TW;
                const int gy = y0 + gpy, gx = x0 + gpx;
                const bool in_tile = j0 < p.TH * p.TW && gy < p.P;
                const bool valid = in_tile && gx < p.Q;
                const bool straddle = gpx + 8 > p.TW;                    // runs on into the next tile row (whose pixels may be inside the image when these are not)
                const bool slow = in_tile && (straddle || (valid && gx + 8 > p.ldy));
                gbyte[it] = valid ? (unsigned)((gy * p.ldy + gx) * 2) : kGOut;
                if (!slow) gfullm |= 1u << it;
                if (__builtin_amdgcn_ballot_w64(slow) != 0) slow_any |= 1u << it;
            }
#pragma unroll
            for (int mi = 0; mi < (MO + 1) / 2; mi++) {
                const int rowbase = o0 + wo * (BM_O / 2) + mi * 32;
                const int o = rowbase + chalf * 16 + i16;
                // (MO odd -- the 96-row block: the last pass carries 16 channels, its upper half belongs to the other wave's rows)
                const unsigned obyte = (o < p.Cout && mi * 32 + chalf * 16 < BM_O / 2) ? (unsigned)(o * pq * 2) : kOOut;
#pragma unroll
                for (int half = 0; half < 2; half++) {
#pragma unroll
                    for (int k = 0; k < 2; k++) {
                        const int mo = 2 * mi + k;
                        if (mo >= MO) continue;
#pragma unroll
                        for (int t4 = 0; t4 < 4; t4++) {
                            const int ti = 4 * half + t4;
                            uint2 w;
                            w.x = pack2<T>(acc[mo][ti][0] * sc[mo][0] + ob[mo][0], acc[mo][ti][1] * sc[mo][1] + ob[mo][1]);
                            w.y = pack2<T>(acc[mo][ti][2] * sc[mo][2] + ob[mo][2], acc[mo][ti][3] * sc[mo][3] + ob[mo][3]);
                            *(uint2*)(ebuf + wr_off[k] + t4 * (16 * EROW)) = w;
                        }
                    }
                    // same wave wrote and reads: LDS operations of a wave complete in order, no barrier needed
#pragma unroll
                    for (int i4 = 0; i4 < 4; i4++) {
                        const int it = 4 * half + i4;
                        union { s16x4 v[2]; eu32x4 q; } u;
#pragma unroll
                        for (int r = 0; r < 2; r++)
                            u.v[r] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(ebuf + i4 * (16 * EROW) + rd_off[r]));
                        if constexpr (FASTEPI) {
                            // the block's row and first column on the scalar unit; lane half hh takes the second granule (+ 16 bytes)
                            const int b16 = wpx * 128 + 16 * it;
                            const int gpy = (int)__umulhi((unsigned)b16, p.magicTW), gpxs = b16 - gpy * p.TW;
                            const int gy = y0 + gpy, gxs = x0 + gpxs;
                            if (b16 < p.TH * p.TW && gy < p.P && gxs < p.Q) {          // wave-uniform
                                unsigned vo = obyte + 16u * (unsigned)hh;
                                if (gxs + 8 >= p.Q && hh) vo = kGOut;                    // (uniform test first: the image's last granule pair only)
                                __builtin_amdgcn_raw_buffer_store_b128(u.q, yrs, vo, (gy * p.ldy + gxs) * 2, 0);
                            }
                            continue;
                        }
                        const bool full = (gfullm >> it) & 1;
                        // (no branch around the common store: a lane on the pair path sends its 16 bytes out of range)
                        __builtin_amdgcn_raw_buffer_store_b128(u.q, yrs, full ? obyte + gbyte[it] : kGOut, 0, 0);
                        if ((slow_any >> it) & 1) {                       // wave-uniform
                            if (!full) {                                  // the granule runs over the tile row's or the image's right end (even widths: whole pairs)
#pragma unroll
                                for (int w2 = 0; w2 < 4; w2++) {
                                    const int j = wpx * 128 + (2 * it + hh) * 8 + 2 * w2;
                                    const int py = (int)__umulhi((unsigned)j, p.magicTW), px = j - py * p.TW;
                                    const bool ok = j < p.TH * p.TW && y0 + py < p.P && x0 + px < p.Q;
                                    __builtin_amdgcn_raw_buffer_store_b32(u.q[w2], yrs, ok ? obyte + (unsigned)(((y0 + py) * p.ldy + x0 + px) * 2) : kGOut, 0, 0);
                                }
                            }
                        }
                    }
                }
            }
        } else {
            TO* yn = (TO*)p.y + (size_t)n * p.Cout * p.P * p.ldy;
            int poff[NT];                                    // pixel offset inside a plane, -1: not stored
#pragma unroll
            for (int ti = 0; ti < NT; ti++) {
                const int j = wpx * 128 + ti * 16 + c16e;
                const int py = (int)__umulhi((unsigned)j, p.magicTW), px = j - py * p.TW;
                poff[ti] = (j < p.TH * p.TW && y0 + py < p.P && x0 + px < p.Q) ? (y0 + py) * p.ldy + x0 + px : -1;
            }
            const float* osn = p.oscale ? p.oscale + (size_t)n * p.Cout : nullptr;
            const int pq = p.P * p.ldy;
            float ia = 1.f, ib = 1.f;
            if (p.bound_a) pow2_factor(p.bound_a[0], &ia);
            if (p.bound_b) pow2_factor(p.bound_b[0], &ib);
            const float inv = ia * ib;
#pragma unroll
            for (int mo = 0; mo < MO; mo++) {
                float sc[4], ob[4];
                const int obase = o0 + wo * (BM_O / 2) + mo * 16 + 4 * ge;
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    sc[reg] = (osn != nullptr ? osn[min(obase + reg, p.Cout - 1)] : 1.f) * inv;
                    ob[reg] = p.obias != nullptr ? p.obias[min(obase + reg, p.Cout - 1)] : 0.f;
                }
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    const int o = obase + reg;
                    if (o < p.Cout) {
                        TO* yo = yn + (size_t)o * pq;
#pragma unroll
                        for (int ti = 0; ti < NT; ti++)
                            if (poff[ti] >= 0) yo[poff[ti]] = from_f32<TO>(acc[mo][ti][reg] * sc[reg] + ob[reg]);
                    }
                }
            }
        }
        if (!has_next) break;
        // the staging area of the epilogue (the buffer the last chunk read) is the one the next tile's first chunk stages INTO
        if (!SPLIT) __syncthreads();
        S = decode(item_n);
        item = item_n;
        set_bbyte(S, cb);
    }
}

// Stride-2 3x3 kernel (the r02 structure: 32x32x16 MFMAs, K-chunks of 16 channels) for the discriminator's down-sampling convs
// (CoModGAN/generator.py:613-692: blur, then a 3x3 conv at stride 2): the r01/r02 route computed the stride-1 result and decimated it -- four times the MFMAs, a full-resolution
// write and a decimation copy.  Here an output pixel (py, px) reads the patch at (2 py + r, 2 px + s): same packed weights, same
// tap loop, B fragment addresses twice as far apart.  The patch of a tile is ~4x its outputs, so a workgroup takes 128 output
// pixels (two 32-pixel blocks per wave) under a (2 TH + 1) x (2 TW + 2) patch of up to kPatchMaxS2 pixels (two staging items per
// thread), 68 KB of LDS double-buffered: still two workgroups per CU.  Bit-identical to the even pixels of the stride-1 result
// (same K order).  Forward only: the gradients of a strided conv are convolutions with the zero-stuffed dy and keep the stride-1 kernels.
template <typename T, int BM_O>
__global__ __launch_bounds__(256, 2) void conv2d_fwd16s2_kernel(ConvParams p) {
    static_assert(sizeof(T) == 2, "16-bit types only");
    typedef ConvCfg<T> C;
    constexpr int KS = 3, KK = 9, BK = C::BK, PITCH = C::PITCH, MI = BM_O / 64, RING = 3;
    constexpr int NT = 2, PXW = 32 * NT, STRIDE = 2, NITEM = 2, PMAX = kPatchMaxS2;   // 128 output pixels per workgroup, two staging items per thread
    typedef typename std::conditional<std::is_same<T, bf16_t>::value, bf16x8, f16x8>::type frag_t;
    typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
    __shared__ __attribute__((aligned(16))) T lds[2 * PMAX * PITCH + 4 * PITCH];      // + a sink for lanes outside the patch

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wo = wave & 1, wpx = wave >> 1;
    const int r32 = lane & 31, h = lane >> 5;

    int bid = blockIdx.x;
    {
        const int total = gridDim.x;
        bid = xcd_order(bid, total);
    }
    // integer division runs on the vector pipe even for uniform operands: pin the results to SGPRs, or everything derived
    // from them (image base, buffer descriptor) sits in VGPRs and every buffer load gets a waterfall loop around it
    const int tx = __builtin_amdgcn_readfirstlane(bid % p.tilesX); bid /= p.tilesX;
    const int ty = __builtin_amdgcn_readfirstlane(bid % p.tilesY); bid /= p.tilesY;
    const int n = __builtin_amdgcn_readfirstlane(bid % p.N);
    const int ob = __builtin_amdgcn_readfirstlane(bid / p.N);
    const int y0 = ty * p.TH, x0 = tx * p.TW;
    const int o0 = ob * BM_O;
    const int PH = (p.TH - 1) * STRIDE + KS, PWL = p.PWL;
    const int xorg = (x0 * STRIDE - p.pad) & ~1;
    const int xoff = (x0 * STRIDE - p.pad) - xorg;

    int bbase[NT], pyv[NT], pxv[NT];
#pragma unroll
    for (int ti = 0; ti < NT; ti++) {
        const int j = wpx * PXW + ti * 32 + r32;
        int py = j / p.TW, px = j - py * p.TW;
        const bool valid = j < p.TH * p.TW;
        if (!valid) { py = 0; px = 0; }
        pyv[ti] = valid ? y0 + py : p.P;             // invalid slots fall outside the image -> never stored
        pxv[ti] = x0 + px;
        bbase[ti] = (py * STRIDE * PWL + px * STRIDE + xoff) * PITCH + h * 8;
    }

    f32x16 acc[MI][NT];
#pragma unroll
    for (int mi = 0; mi < MI; mi++)
#pragma unroll
        for (int ti = 0; ti < NT; ti++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[mi][ti][e] = 0.f;

    // ---- A fragments: straight from the packed weights
    const T* wlane = (const T*)p.wp + (size_t)(o0 + wo * (BM_O / 2) + r32) * BK + h * 8;
    const size_t wtap = (size_t)p.Opad * BK;                       // elements per tap
    auto load_a = [&](int kc, int tap, int mi) __attribute__((always_inline)) {
        return *(const frag_t*)(wlane + ((size_t)kc * KK + tap) * wtap + mi * 32 * BK);
    };

    // ---- patch staging (one item = 4 pixels x 8 channels), as in conv2d_fwd_kernel
    const int cg = (tid >> 5) & 1, pg = (tid & 31) + 32 * (tid >> 6);
    const int pcols = PWL >> 2;
    const T* xn = (const T*)p.x + (size_t)n * p.Cin * p.H * p.ldx;
    constexpr unsigned kOob = 0x80000000u;
    const long long img_bytes = (long long)p.Cin * p.H * p.ldx * 2ll;
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void*)xn, 0, (int)(img_bytes > 0x7fffffffll ? 0x7fffffffll : img_bytes), 0x00020000);
    const int hw2 = p.H * p.ldx * 2;
    bool pvalid[NITEM], lshift[NITEM];
    int pdst[NITEM];
    unsigned pmask0[NITEM], pmask1[NITEM], pvoff[NITEM];
#pragma unroll
    for (int it = 0; it < NITEM; it++) {
        const int item = pg + 128 * it;
        const int prow = item / pcols, pcol4 = item - prow * pcols;
        pvalid[it] = prow < PH;
        const int iy = y0 * STRIDE - p.pad + prow, ix = xorg + 4 * pcol4;
        const bool rowok = pvalid[it] && (unsigned)iy < (unsigned)p.H;
        const long long pix_off = (long long)(rowok ? iy : 0) * p.ldx + ix;
        pdst[it] = (prow * PWL + 4 * pcol4) * PITCH + cg * 8;
        const bool d0ok = rowok && (unsigned)ix < (unsigned)p.W, d1ok = rowok && (unsigned)(ix + 2) < (unsigned)p.W;
        pmask0[it] = d0ok ? ~0u : 0u; pmask1[it] = d1ok ? ~0u : 0u;
        lshift[it] = !d0ok && d1ok;                                                   // never touch bytes before a row 0
        pvoff[it] = (d0ok || d1ok) ? (unsigned)(((long long)cg * 8 * p.H * p.ldx + pix_off + (lshift[it] ? 2 : 0)) * 2ll) : kOob;
    }

    unsigned preg[NITEM][8][2];
    auto issue_patch = [&](int kc, bool live) __attribute__((always_inline)) {
        const int cbase = kc * BK + cg * 8;
        const int climit = live ? p.Cin : 0;
#pragma unroll
        for (int it = 0; it < NITEM; it++)
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const unsigned off = (cbase + c < climit) ? pvoff[it] : kOob;
                const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(xrs, off, (kc * BK + c) * hw2, 0);
                preg[it][c][0] = v.x; preg[it][c][1] = v.y;
            }
    };
    auto write_patch = [&](int kc, T* dstbuf, int bufbase) __attribute__((always_inline)) {
#pragma unroll
        for (int it = 0; it < NITEM; it++) {
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const unsigned lo = lshift[it] ? 0u : (preg[it][c][0] & pmask0[it]);
                const unsigned hi = (lshift[it] ? preg[it][c][0] : preg[it][c][1]) & pmask1[it];
                preg[it][c][0] = lo; preg[it][c][1] = hi;
            }
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const unsigned sel = (e & 1) ? 0x07060302u : 0x05040100u;
                uint4 v;
                v.x = __builtin_amdgcn_perm(preg[it][1][e >> 1], preg[it][0][e >> 1], sel);
                v.y = __builtin_amdgcn_perm(preg[it][3][e >> 1], preg[it][2][e >> 1], sel);
                v.z = __builtin_amdgcn_perm(preg[it][5][e >> 1], preg[it][4][e >> 1], sel);
                v.w = __builtin_amdgcn_perm(preg[it][7][e >> 1], preg[it][6][e >> 1], sel);
                *(uint4*)(lds + (pvalid[it] ? bufbase + pdst[it] + e * PITCH : 2 * PMAX * PITCH)) = v;
            }
        }
    };

    frag_t ar[RING][MI];
    issue_patch(0, true);
#pragma unroll
    for (int t = 0; t < RING; t++)
#pragma unroll
        for (int mi = 0; mi < MI; mi++) ar[t][mi] = load_a(0, t, mi);
    write_patch(0, lds, 0);
    __syncthreads();

    const int last = p.nkc - 1;
    for (int kc = 0; kc < p.nkc; kc++) {
        const T* cur = lds + (kc & 1) * (PMAX * PITCH);
        T* nxt = lds + ((kc + 1) & 1) * (PMAX * PITCH);
        const bool more = kc < last;
        // B fragments run one tap ahead of their MFMAs in the SAME registers: a tap's MFMAs go pixel-block by pixel-block, and
        // as soon as block ti's fragment has been consumed the next tap's fragment for that block is read into it.  (Read, wait,
        // multiply per tap left ~one LDS round trip exposed per 8 MFMAs with only the other workgroup's wave to cover it.)
        frag_t b[NT];
#pragma unroll
        for (int ti = 0; ti < NT; ti++) b[ti] = *(const frag_t*)(cur + bbase[ti]);
        issue_patch(kc + (int)more, more);
        __builtin_amdgcn_sched_group_barrier(0x100, NT, 0);              // tap 0's fragments first, all in flight together
        __builtin_amdgcn_sched_group_barrier(0x020, 8 * NITEM, 0);
#pragma unroll
        for (int tap = 0; tap < KK; tap++) {
            const int nr = (tap + 1) / KS, ns = (tap + 1) - nr * KS;
            const int tapoff_n = (nr * PWL + ns) * PITCH;                 // next tap's offset (unused on the last tap)
            frag_t a[MI];
#pragma unroll
            for (int mi = 0; mi < MI; mi++) a[mi] = ar[tap % RING][mi];
            // refill this ring slot with the fragments three taps ahead (clamped at the end: no branch around a load)
            {
                const int nt = (tap + RING) % KK;
                const int nk = (tap + RING < KK) ? kc : (more ? kc + 1 : kc);
#pragma unroll
                for (int mi = 0; mi < MI; mi++) ar[tap % RING][mi] = load_a(nk, nt, mi);
            }
#pragma unroll
            for (int ti = 0; ti < NT; ti++) {
#pragma unroll
                for (int mi = 0; mi < MI; mi++) {
                    if constexpr (std::is_same<T, bf16_t>::value)
                        acc[mi][ti] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi], b[ti], acc[mi][ti], 0, 0, 0);
                    else
                        acc[mi][ti] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[mi], b[ti], acc[mi][ti], 0, 0, 0);
                }
                if (tap + 1 < KK) b[ti] = *(const frag_t*)(cur + bbase[ti] + tapoff_n);
            }
            if (tap == 5) {
                // the other buffer (last read one chunk ago); on the last chunk this rewrites stale registers into a buffer
                // nobody reads.  Interleave: one MFMA, then a handful of the transpose's vector instructions.
                write_patch(kc + 1, nxt, ((kc + 1) & 1) * (PMAX * PITCH));
                __builtin_amdgcn_sched_group_barrier(0x020, MI, 0);
#pragma unroll
                for (int ti = 0; ti < NT; ti++) {
#pragma unroll
                    for (int mi = 0; mi < MI; mi++) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x002, 20, 0);
                    }
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x200, 4 * NITEM, 0);
            } else {
                // pin the issue order of the tap: the ring refill first (left alone, the scheduler sinks the loads next to
                // their uses and the three-tap prefetch distance collapses), then per pixel block its MFMAs and the read ahead
                __builtin_amdgcn_sched_group_barrier(0x020, MI, 0);
#pragma unroll
                for (int ti = 0; ti < NT; ti++) {
                    __builtin_amdgcn_sched_group_barrier(0x008, MI, 0);
                    if (tap + 1 < KK) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
            }
        }
        __syncthreads();
    }

    // ---- epilogue: D[row = channel][col = pixel]; row = (reg&3) + 8*(reg>>2) + 4*h within the 32x32 tile.
    if ((p.TW & 7) == 0 && (p.Q & 1) == 0) {        // (an odd output width -- possible at stride 2 -- puts rows on odd elements: element stores below)
        // Tile rows that are multiples of 8 pixels: transpose through LDS (the patch buffers are free after the last barrier)
        // and store 8 pixels = 16 bytes per lane.  A lane holds 16 channels of ONE pixel (4 runs of 4 consecutive channels), so
        // it stages [pixel][32 channels] rows with four 8-byte writes per 32x32 tile, and the transposing read
        // (ds_read_b64_tr_b16: a 16-lane group takes a 4-pixel x 16-channel block, lane i receives channel i of the 4 pixels)
        // hands every lane 4 pixels of one channel.  Per thread and 32-channel pass: 32 packed conversions + 16 ds_write_b64 +
        // 16 transposing reads + 8 stores (the first version staged [channel][pixel] with 64 two-byte writes per pass: the
        // epilogue was 12 % of the whole conv time, 35 % on the 64-channel layers).
        // Row = 64 bytes = eight 8-byte chunks; chunk c of pixel p lives at c ^ ((p >> 1) & 7): conflict-free for the writes
        // (16 consecutive pixels x one chunk) and for the reads (a 32-lane half = both channel halves of 4 pixels).
        typedef __attribute__((ext_vector_type(4))) short s16x4;
        constexpr int EROW = 64;
        unsigned char* ebuf = (unsigned char*)lds + wave * (PXW * EROW);
        T* yn = (T*)p.y + (size_t)n * p.Cout * p.P * p.ldy;
        const float* osn = p.oscale ? p.oscale + (size_t)n * p.Cout : nullptr;
        const int pq = p.P * p.ldy;
        // read side: lane = (half hh: granule parity, chalf: channel half, i16: channel / address role inside the 16-lane group)
        const int i16 = lane & 15, chalf = (lane >> 4) & 1, hh = lane >> 5;
        const int q4 = i16 >> 2, p4 = i16 & 3;
        unsigned rd_off[2];
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int prow = 8 * hh + 4 * r + q4;                 // + 16 pixels per iteration: (prow >> 1) & 7 does not change
            rd_off[r] = prow * EROW + (((chalf * 4 + p4) ^ ((prow >> 1) & 7)) << 3);
        }
        // this lane's 8 granules (8 pixels each, one tile row): plane offset, -1 = outside the image; bit it of gfullm = whole
        int goff[2 * NT];
        unsigned gfullm = 0;
        int gxv[2 * NT];
#pragma unroll
        for (int it = 0; it < 2 * NT; it++) {
            const int j0 = wpx * PXW + (2 * it + hh) * 8;
            const int gpy = (int)__umulhi((unsigned)j0, p.magicTW), gpx = j0 - gpy * p.TW;
            const int gy = y0 + gpy, gx = x0 + gpx;
            goff[it] = (j0 < p.TH * p.TW && gy < p.P && gx < p.Q) ? gy * p.ldy + gx : -1;
            gxv[it] = gx;
            if (gx + 8 <= p.ldy) gfullm |= 1u << it;         // a pitched row has room for the whole granule (columns >= Q: padding)
        }
        const int wr_pix = r32;                                    // + 32 ti
#pragma unroll
        for (int mi = 0; mi < MI; mi++) {
            float sc[16], ob[16];
            const int obase = o0 + wo * (BM_O / 2) + mi * 32 + 4 * h;
#pragma unroll
            for (int reg = 0; reg < 16; reg++) { sc[reg] = 1.f; ob[reg] = 0.f; }
            if (osn != nullptr) {
#pragma unroll
                for (int reg = 0; reg < 16; reg++) sc[reg] = osn[min(obase + (reg & 3) + 8 * (reg >> 2), p.Cout - 1)];
            }
            if (p.obias != nullptr) {
#pragma unroll
                for (int reg = 0; reg < 16; reg++) ob[reg] = p.obias[min(obase + (reg & 3) + 8 * (reg >> 2), p.Cout - 1)];
            }
#pragma unroll
            for (int ti = 0; ti < NT; ti++) {
                const int pix = ti * 32 + wr_pix;
                const int sw = (pix >> 1) & 7;
#pragma unroll
                for (int k4 = 0; k4 < 4; k4++) {                   // registers 4 k4 .. 4 k4 + 3 = channels 4 h + 8 k4 + 0..3
                    uint2 w;
                    w.x = pack2<T>(acc[mi][ti][4 * k4 + 0] * sc[4 * k4 + 0] + ob[4 * k4 + 0], acc[mi][ti][4 * k4 + 1] * sc[4 * k4 + 1] + ob[4 * k4 + 1]);
                    w.y = pack2<T>(acc[mi][ti][4 * k4 + 2] * sc[4 * k4 + 2] + ob[4 * k4 + 2], acc[mi][ti][4 * k4 + 3] * sc[4 * k4 + 3] + ob[4 * k4 + 3]);
                    *(uint2*)(ebuf + pix * EROW + (((h + 2 * k4) ^ sw) << 3)) = w;
                }
            }
            // same wave wrote and reads: LDS operations of a wave complete in order, no barrier needed
            const int o = o0 + wo * (BM_O / 2) + mi * 32 + chalf * 16 + i16;
            T* const yo = yn + (size_t)min(o, p.Cout - 1) * pq;
#pragma unroll
            for (int it = 0; it < 2 * NT; it++) {
                union { s16x4 v[2]; uint4 q; } u;
#pragma unroll
                for (int r = 0; r < 2; r++)
                    u.v[r] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(ebuf + it * (16 * EROW) + rd_off[r]));
                if (goff[it] >= 0 && o < p.Cout) {
                    T* dst = yo + goff[it];
                    if ((gfullm >> it) & 1) {
                        *(uint4*)dst = u.q;
                    } else {                                      // the granule straddles the right edge (even width: whole pairs)
                        const unsigned vv[4] = {u.q.x, u.q.y, u.q.z, u.q.w};
#pragma unroll
                        for (int w2 = 0; w2 < 4; w2++)
                            if (gxv[it] + 2 * w2 < p.Q) ((unsigned*)dst)[w2] = vv[w2];
                    }
                }
            }
        }
        return;
    }
    T* yn = (T*)p.y + (size_t)n * p.Cout * p.P * p.ldy;
    // per output-row block: all per-channel scales and biases first (clamped index, no branch around the loads: one wait
    // instead of a round trip per row), then the stores
    int poff[NT];                                    // pixel offset inside a plane, -1: not stored
#pragma unroll
    for (int ti = 0; ti < NT; ti++) poff[ti] = (pyv[ti] < p.P && pxv[ti] < p.Q) ? pyv[ti] * p.ldy + pxv[ti] : -1;
    const float* osn = p.oscale ? p.oscale + (size_t)n * p.Cout : nullptr;
    const int pq = p.P * p.ldy;
#pragma unroll
    for (int mi = 0; mi < MI; mi++) {
        float sc[16], ob[16];
        const int obase = o0 + wo * (BM_O / 2) + mi * 32 + 4 * h;
#pragma unroll
        for (int reg = 0; reg < 16; reg++) { sc[reg] = 1.f; ob[reg] = 0.f; }
        if (osn != nullptr) {
#pragma unroll
            for (int reg = 0; reg < 16; reg++) sc[reg] = osn[min(obase + (reg & 3) + 8 * (reg >> 2), p.Cout - 1)];
        }
        if (p.obias != nullptr) {
#pragma unroll
            for (int reg = 0; reg < 16; reg++) ob[reg] = p.obias[min(obase + (reg & 3) + 8 * (reg >> 2), p.Cout - 1)];
        }
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            const int o = obase + (reg & 3) + 8 * (reg >> 2);
            if (o < p.Cout) {
                T* yo = yn + (size_t)o * pq;
#pragma unroll
                for (int ti = 0; ti < NT; ti++)
                    if (poff[ti] >= 0) yo[poff[ti]] = from_f32<T>(acc[mi][ti][reg] * sc[reg] + ob[reg]);
            }
        }
    }
}


// ---------------------------------------------------------------------------------------------
// Weight packing: w[O][I][KS][KS] (fp32) -> [nkc][KK][Opad][BK] of T, zero padded.
//   mode 0 (forward):        dst[kc][r*KS+s][o][kk]  = w[o][kc*BK+kk][r][s]
//   mode 1 (data gradient):  roles of O and I swap and taps flip:
//                            dst[kc][r*KS+s][i][kk]  = w[kc*BK+kk][i][KS-1-r][KS-1-s]
template <typename T>
__global__ __launch_bounds__(256) void conv2d_pack_kernel(T* __restrict__ dst, const float* __restrict__ w, int O, int I, int KS,
                                                          int rows, int cols, int rows_pad, int BK, int nkc, int mode) {
    const int KK = KS * KS;
    const long long total = (long long)nkc * KK * rows_pad * BK;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int kk = (int)(idx % BK);
        long long t = idx / BK;
        const int row = (int)(t % rows_pad); t /= rows_pad;
        const int tap = (int)(t % KK);
        const int kc = (int)(t / KK);
        const int col = kc * BK + kk;
        float v = 0.f;
        if (row < rows && col < cols) {
            const int r = tap / KS, s = tap - r * KS;
            if (mode == 0) v = w[(((size_t)row * I + col) * KS + r) * KS + s];
            else v = w[(((size_t)col * I + row) * KS + (KS - 1 - r)) * KS + (KS - 1 - s)];
        }
        dst[idx] = from_f32<T>(v);
    }
}

// Same layout from an LDS tile: a workgroup stages w[o0 .. o0+16)[i0 .. i0+64)[all taps] with coalesced loads (every o is one
// contiguous run of 64 * k*k floats) and emits BOTH images from it as 8-element (16-byte for 16-bit types) stores --
//   forward       dst0[kc = i / BK][tap][row = o][i % BK]            16 rows x BK contiguous per (kc, tap)
//   data gradient dst1[kc = o / BK][k*k-1-tap][row = i][o % BK]      64 rows x BK contiguous per (kc, tap)
// -- so the weights are read once for the two images, the index arithmetic is per 8 elements, and the forward and the backward
// image of a layer come out of ONE launch (a null destination skips that image).  The per-element gather kernel above is kept
// as the definition the layout test checks against.
// tile of the pack: TO output x TI input channels, both at least one K-chunk (the data-gradient image chunks the OUTPUT channels)
template <int BK> struct PackTile { static constexpr int TO = BK > 16 ? 32 : 16, TI = BK > 16 ? 32 : 64; };
template <typename T, int KK, int BK>
__device__ __forceinline__ void pack_tile_body(float* tile, int bx, int by, T* __restrict__ dst0, T* __restrict__ dst1, const float* __restrict__ w,
                                               int O, int I, int rows_pad0, int rows_pad1) {
    constexpr int TO = PackTile<BK>::TO, TI = PackTile<BK>::TI, ROW = TI * KK + 1;             // + 1: the 8 channel runs of a store start 9 floats apart
    struct alignas(8 * sizeof(T)) Out { T v[8]; };
    const int i0 = bx * TI, o0 = by * TO;
    {
        // all of a thread's loads in flight before the first LDS write (left as a loop, each load waited for its predecessor:
        // 36 serial round trips = 10 us for any layer size)
        constexpr int NL = TO * TI * KK / 256;
        static_assert(TO * TI * KK % 256 == 0, "tile size");
        float v[NL];
#pragma unroll
        for (int k = 0; k < NL; k++) {
            const int e = threadIdx.x + 256 * k;
            const int o = e / (TI * KK), r = e - o * (TI * KK);
            const int i = r / KK;
            v[k] = (o0 + o < O && i0 + i < I) ? w[((size_t)(o0 + o) * I + i0) * KK + r] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < NL; k++) {
            const int e = threadIdx.x + 256 * k;
            const int o = e / (TI * KK), r = e - o * (TI * KK);
            tile[o * ROW + r] = v[k];
        }
    }
    __syncthreads();
    constexpr int G = BK / 8;
    if (dst0 != nullptr && o0 < rows_pad0) {
        // items: (kc_local, tap, o, half); cols (i) are written up to the last started K-chunk only
        const int nkc = cdiv(I, BK);
        constexpr int kcl = TI / BK, NIT = kcl * KK * TO * G;
#pragma unroll
        for (int it0 = 0; it0 < NIT; it0 += 256) {
            const int it = it0 + threadIdx.x;
            if (NIT % 256 != 0 && it >= NIT) break;
            const int half = it % G;
            int t = it / G;
            const int o = t % TO; t /= TO;
            const int tap = t % KK, kc = t / KK;
            const int kcg = i0 / BK + kc;
            if (kcg >= nkc) continue;
            Out v;
#pragma unroll
            for (int c = 0; c < 8; c++) v.v[c] = from_f32<T>(tile[o * ROW + (kc * BK + half * 8 + c) * KK + tap]);
            *(Out*)(dst0 + (((size_t)kcg * KK + tap) * rows_pad0 + o0 + o) * BK + half * 8) = v;
        }
    }
    if (dst1 != nullptr && i0 < rows_pad1) {
        const int nkc = cdiv(O, BK);
        constexpr int kcl = TO / BK, NIT = kcl * KK * TI * G;
#pragma unroll
        for (int it0 = 0; it0 < NIT; it0 += 256) {
            const int it = it0 + threadIdx.x;
            if (NIT % 256 != 0 && it >= NIT) break;
            const int half = it % G;
            int t = it / G;
            const int i = t % TI; t /= TI;
            const int tap = t % KK, kc = t / KK;
            const int kcg = o0 / BK + kc;
            if (kcg >= nkc) continue;
            Out v;
#pragma unroll
            for (int c = 0; c < 8; c++) v.v[c] = from_f32<T>(tile[(kc * BK + half * 8 + c) * ROW + i * KK + (KK - 1 - tap)]);
            *(Out*)(dst1 + (((size_t)kcg * KK + tap) * rows_pad1 + i0 + i) * BK + half * 8) = v;
        }
    }
}

template <typename T, int KK, int BK>
__global__ __launch_bounds__(256) void conv2d_pack_tile_kernel(T* __restrict__ dst0, T* __restrict__ dst1, const float* __restrict__ w, int O,
                                                               int I, int rows_pad0, int rows_pad1) {
    __shared__ float tile[PackTile<BK>::TO * (PackTile<BK>::TI * KK + 1)];
    pack_tile_body<T, KK, BK>(tile, blockIdx.x, blockIdx.y, dst0, dst1, w, O, I, rows_pad0, rows_pad1);
}

// the same for a list of layers in one launch (C ABI afcm_conv2d_pack_bank): the table rides in the kernel arguments, a workgroup
// finds its layer by a scalar scan over the first-block table
struct PackBank {
    int count;
    int blk[AFCM_PACK_MAX + 1];
    int gx[AFCM_PACK_MAX];
    afcm_pack_entry e[AFCM_PACK_MAX];
};
template <typename T, int KK, int BK>
__global__ __launch_bounds__(256) void conv2d_pack_bank_kernel(const PackBank b) {
    __shared__ float tile[PackTile<BK>::TO * (PackTile<BK>::TI * KK + 1)];
    int l = 0;
    while (l + 1 < b.count && (int)blockIdx.x >= b.blk[l + 1]) l++;
    const int loc = blockIdx.x - b.blk[l];
    const afcm_pack_entry& e = b.e[l];
    pack_tile_body<T, KK, BK>(tile, loc % b.gx[l], loc / b.gx[l], (T*)e.dst_fwd, (T*)e.dst_dgrad, e.w, e.cout, e.cin, e.rows_pad_fwd, e.rows_pad_dgrad);
}

// The packed image of a split conv's stacked weight parts (afcm_conv2d_split): channel block t (cin16 = 16 nkc_real channels) holds part
// (term_wparts >> 4 t) & 15 of g * w (g: pow2_factor of the bound word, 1 without one) -- part 0 = r16(v), part 1 = r16(v - part 0), ... -- in the layout of conv2d_pack_kernel
// (mode 1: the data gradient's transposed, flipped kernel).
template <typename T>
__global__ __launch_bounds__(256) void conv2d_pack_split_kernel(T* __restrict__ dst, const float* __restrict__ w, const unsigned* __restrict__ bound,
                                                                int O, int I, int rows, int cols, int rows_pad, int nkc_real, int terms,
                                                                unsigned term_wparts, int mode, int BK) {
    constexpr int KS = 3, KK = 9;
    const float gs = bound ? pow2_factor(bound[0]) : 1.f;
    const long long total = (long long)terms * nkc_real * KK * rows_pad * BK;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int kk = (int)(idx % BK);
        long long t = idx / BK;
        const int row = (int)(t % rows_pad); t /= rows_pad;
        const int tap = (int)(t % KK);
        const int kc = (int)(t / KK);
        const int term = kc / nkc_real;
        const int col = (kc - term * nkc_real) * BK + kk;
        float r = 0.f;
        if (row < rows && col < cols) {
            const int rr = tap / KS, ss = tap - rr * KS;
            if (mode == 0) r = w[(((size_t)row * I + col) * KS + rr) * KS + ss];
            else r = w[(((size_t)col * I + row) * KS + (KS - 1 - rr)) * KS + (KS - 1 - ss)];
        }
        r *= gs;
        const int part = (int)((term_wparts >> (4 * term)) & 15u);
        T q = (T)r;
        for (int k = 0; k < part; k++) {
            const float qf = (float)q;
            r = (__builtin_fabsf(qf) <= 3.4028234664e38f) ? r - qf : 0.f;
            q = (T)r;
        }
        dst[idx] = q;
    }
}

static void choose_tile(int P, int Q, int KS, int* TH, int* TW, int* PWL, int patch_max = kPatchMax) {
    // Tile of TH x TW output pixels with TH*TW <= 256 slots and an LDS patch (TH+KS-1) x round4(TW+KS) <= kPatchMax,
    // chosen to maximise the fraction of useful slots.
    double best = -1;
    constexpr double gran_bonus = 0.03;
    for (int tw = 2; tw <= 128; tw += 2) {
        int th = kSlots / tw;
        if (th > P) th = P;
        for (; th >= 1; th--) {
            const int pwl = round_up(tw + KS, 4);
            if ((th + KS - 1) * pwl > patch_max) continue;
            const double tiles = (double)cdiv(P, th) * cdiv(Q, tw);
            const double util = (double)P * Q / (tiles * kSlots);
            // small preference for wide tiles (longer contiguous runs for loads/stores); rows of whole 8-pixel granules
            // get the 16-byte LDS-transposed epilogue of the 16-bit kernel: worth a few % of slot utilisation
            const double score = util + 1e-4 * tw + ((tw & 7) == 0 ? gran_bonus : 0.0);
            if (score > best) { best = score; *TH = th; *TW = tw; *PWL = pwl; }
            break;
        }
    }
}

static void choose_tile_s2(int P, int Q, int* TH, int* TW, int* PWL) {
    // stride-2 kernel: TH x TW output pixels with TH * TW <= 128 slots under a ((TH - 1) 2 + 3) x round4((TW - 1) 2 + 4) patch <= kPatchMaxS2
    double best = -1;
    for (int tw = 2; tw <= 64; tw += 2) {
        int th = 128 / tw;
        if (th > P) th = P;
        for (; th >= 1; th--) {
            const int pwl = round_up((tw - 1) * 2 + 4, 4);
            if (((th - 1) * 2 + 3) * pwl > kPatchMaxS2) continue;
            const double tiles = (double)cdiv(P, th) * cdiv(Q, tw);
            const double util = (double)P * Q / (tiles * 128);
            const double score = util + 1e-4 * tw + ((tw & 7) == 0 ? 0.03 : 0.0);
            if (score > best) { best = score; *TH = th; *TW = tw; *PWL = pwl; }
            break;
        }
    }
}

// Grid of the persistent conv2d_fwd16x_kernel: one round of resident workgroups (compute units x workgroups per CU, a multiple of 8 so that
// the XCD-aware item order is the same function of the item as of the hardware block index), or every item when there are fewer.
// The compute-unit count is a property of the device, read once per device (speed only: any grid size computes the same result).
static int conv_persistent_grid(long long items, int per_cu) {
    static int cus[16] = {0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    int n = (dev >= 0 && dev < 16) ? cus[dev] : 0;
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        if (dev >= 0 && dev < 16) cus[dev] = n;
    }
    const long long slots = (long long)round_up(n * per_cu, 8);
    return (int)(items < slots ? items : slots);
}

// conv2d_fwd16x_kernel<.., FASTEPI>: tile widths that are multiples of 16 on output rows whose pitch is a multiple of 8 elements
static bool conv_fast_epilogue(int TW, int ldy, int Q) {
    return (TW & 15) == 0 && (ldy & 7) == 0 && (Q & 1) == 0;
}

// Which kernel family a stride-1 conv takes, on which tile, over how many work items and workgroups: the ONE place where
// afcm_conv2d_ld and afcm_conv2d_split decide it, and what afcm_conv2d_plan reports.
enum { kConvDirect = 0, kConv96 = 1, kConv128p64 = 2, kConv64 = 3, kConv128 = 4 };
enum { kConvKernelX16 = 0, kConvKernelGeneral16 = 1, kConvKernelF32 = 2, kConvKernelDirect = 3, kConvKernelX16Split = 4 };
struct ConvPlan {
    int family;             // kConv*
    int kernel;             // kConvKernel*
    int rows;               // output rows per block of the launch that `items` / `grid` describe (128 + 64: the 64-row launch)
    int big;                // 128 + 64: 128-row blocks in front of the 64-row one (rows [0, 128 big), one item per workgroup)
    int TH, TW, PWL;        // output tile and LDS patch row (0 for the direct kernel: its tile is fixed, conv2d_direct.hip)
    long long items;        // tiles x images x row blocks
    long long grid;         // workgroups: items, or one round of resident workgroups for the persistent launches
    bool fast;              // conv2d_fwd16x_kernel<.., FASTEPI>
};

static ConvPlan conv_plan(int dtype, int n, int cin, int cout, int P, int Q, int ks, int rows_pad, int ldy, bool split) {
    ConvPlan pl;
    pl.family = kConvDirect; pl.kernel = kConvKernelDirect; pl.rows = 64; pl.big = 0; pl.TH = pl.TW = pl.PWL = 0; pl.items = pl.grid = 0; pl.fast = false;
    const bool x16 = dtype != AFCM_F32 && ks == 3;
    if (!split && x16 && cin <= 4 && cout <= 64) {
        // a handful of input channels: the contraction index is (tap column, channel), no channel padding (conv2d_direct.hip; r06)
        return pl;
    }
    choose_tile(P, Q, ks, &pl.TH, &pl.TW, &pl.PWL, x16 ? kPatchMaxX16 : kPatchMax);
    const long long tiles = (long long)cdiv(Q, pl.TW) * cdiv(P, pl.TH) * n;
    pl.kernel = split ? kConvKernelX16Split : x16 ? kConvKernelX16 : dtype == AFCM_F32 ? kConvKernelF32 : kConvKernelGeneral16;
    pl.fast = !split && x16 && conv_fast_epilogue(pl.TW, ldy, Q);
    // 64-row blocks when they waste fewer padded rows than 128-row blocks
    const bool small = (rows_pad % 128 != 0) || cout <= 64;
    if (!split && x16 && cout > 64 && cout <= 96) {
        // 65 .. 96 output rows (the 91-channel layers): one 96-row block instead of 128 rows of MFMAs for them.  (129 .. 192 rows as two
        // 96-row blocks instead of 128 + 64 measured the same: profiles/r05_conv_bm96_ab.txt)
        pl.family = kConv96; pl.rows = 96;
        pl.items = tiles * cdiv(cout, 96);
        pl.grid = conv_persistent_grid(pl.items, 2);
        return pl;
    }
    if (!split && x16 && rows_pad % 128 == 64 && rows_pad > 128) {
        // ... and both when the rows are 128 k + (1 .. 64) (the 181-channel layers: 192 padded rows): the 128-row kernel moves half the
        // pixel-fragment bytes per flop of the 64-row one, so rows [0, 128 k) go to it and only the last 64 to the 64-row kernel -- two
        // launches, disjoint output rows, the same number of passes over x as three 64-row blocks had
        pl.family = kConv128p64; pl.rows = 64; pl.big = rows_pad / 128;
        pl.items = tiles;
        pl.grid = conv_persistent_grid(pl.items, 3);
        return pl;
    }
    pl.family = small ? kConv64 : kConv128; pl.rows = small ? 64 : 128;
    pl.items = tiles * cdiv(cout, pl.rows);
    // the 64-row 16x16x32 kernel is persistent: one round of three workgroups per CU; every other kernel takes one item per workgroup
    pl.grid = (small && (split || x16)) ? conv_persistent_grid(pl.items, 3) : pl.items;
    return pl;
}

// conv2d_fwd16x_kernel<T, BM_O, SPLIT> on `grid` workgroups; the fast epilogue where the plan allows it (plain outputs only)
template <typename T, int BM_O, bool SPLIT>
static int launch_fwd16x(const ConvParams& p, dim3 grid, bool fast, hipStream_t st) {
    if (!SPLIT && fast) hipLaunchKernelGGL((conv2d_fwd16x_kernel<T, BM_O, false, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((conv2d_fwd16x_kernel<T, BM_O, SPLIT>), grid, dim3(256), 0, st, p);
    return hip_status(hipGetLastError());
}

// ConvParams of a conv of x [n, cin, h, w] into y [n, cout, P, Q] (row pitches ldx / ldy) on output tiles of TH x TW pixels (patch rows
// of PWL), packed weights of rows_pad rows in nkc K-chunks: a plain conv (no split-precision terms), one launch for all rows
static ConvParams conv_params(void* y, const void* x, const void* wp, const float* oscale, const float* obias, int n, int cin, int cout,
                              int h, int w, int P, int Q, int pad, int ldx, int ldy, int TH, int TW, int PWL, int rows_pad, int nkc) {
    ConvParams p;
    p.x = x; p.y = y; p.wp = wp; p.oscale = oscale; p.obias = obias;
    p.N = n; p.Cin = cin; p.Cout = cout; p.H = h; p.W = w;
    p.P = P; p.Q = Q;
    p.pad = pad;
    p.ldx = ldx; p.ldy = ldy;
    p.TH = TH; p.TW = TW; p.PWL = PWL;
    p.tilesX = cdiv(p.Q, p.TW); p.tilesY = cdiv(p.P, p.TH);
    p.magicTW = (unsigned)((0x100000000ull + (unsigned)p.TW - 1) / (unsigned)p.TW);
    p.magicTX = magic_u32((unsigned)p.tilesX); p.magicTY = magic_u32((unsigned)p.tilesY); p.magicN = magic_u32((unsigned)p.N); p.magicPC = magic_u32((unsigned)(p.PWL >> 2));
    p.Opad = rows_pad;
    p.nkc = nkc;
    p.nkc_real = p.nkc; p.magicNK = 0; p.term_parts = 0; p.part_bytes = 0; p.last_part_bytes = 0; p.bound_a = p.bound_b = nullptr; p.total_blocks = 0; p.o_base = 0;
    return p;
}

// `blocks` work items on `pgrid` workgroups (the persistent 64-row 16x16x32 kernel; every other kernel: one workgroup per item); o_base:
// the launch covers output rows from o_base on (16-bit 3x3 16x16x32 kernel only)
template <typename T, int BM_O>
static int launch_conv(ConvParams p, int ks, hipStream_t st, long long blocks, long long pgrid, bool fast, int o_base = 0) {
    p.o_base = o_base;
    AFCM_REQUIRE(blocks > 0 && blocks < (1ll << 31), "conv2d: grid of %lld blocks is out of range", blocks);
    dim3 grid((unsigned)blocks), block(256);
    p.total_blocks = (int)blocks;
    if constexpr (sizeof(T) == 2) {
        // 16-bit: 3x3 on the 16x16x32 kernel (the 64-row kernel is persistent: one round of three workgroups per CU; the 128-row kernel
        // takes one item per workgroup), 1x1 on the general one
        if (ks == 3) return launch_fwd16x<T, BM_O, false>(p, BM_O == 64 ? dim3((unsigned)pgrid) : grid, fast, st);
        hipLaunchKernelGGL((conv2d_fwd_kernel<T, BM_O, 1>), grid, block, 0, st, p);
    } else {
        if (ks == 3) hipLaunchKernelGGL((conv2d_fwd_kernel<T, BM_O, 3>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((conv2d_fwd_kernel<T, BM_O, 1>), grid, block, 0, st, p);
    }
    return hip_status(hipGetLastError());
}

}  // namespace afcm

using namespace afcm;

extern "C" int afcm_conv2d_block_k(int32_t dtype) { return dtype == AFCM_F32 ? ConvCfg<float>::BK : ConvCfg<bf16_t>::BK; }
static inline int afcm::conv_bk(int dtype, int ks) { return (dtype != AFCM_F32 && ks == 3) ? 32 : afcm_conv2d_block_k(dtype); }
extern "C" int afcm_conv2d_block_k_ks(int32_t dtype, int32_t ks) { return conv_bk(dtype, ks); }

template <typename T>
static void launch_pack8(void* dst0, void* dst1, const float* w, int cout, int cin, int ks, int rows_pad0, int rows_pad1, int BK, hipStream_t st) {
    // tiles cover the padded row ranges of both images: o up to rows_pad0 (forward rows) and the last started K-chunk of the
    // data-gradient image, i up to rows_pad1 and the forward image's last K-chunk (rows_pad are multiples of 64 >= the extents)
    const int omax = dst0 ? rows_pad0 : round_up(cout, BK), imax = dst1 ? rows_pad1 : round_up(cin, BK);
    constexpr int BKT = ConvCfg<T>::BK;
    const int ti = BK > 16 ? PackTile<32>::TI : PackTile<BKT>::TI, to = BK > 16 ? PackTile<32>::TO : PackTile<BKT>::TO;
    dim3 grid((unsigned)cdiv(imax > cin ? imax : cin, ti), (unsigned)cdiv(omax > cout ? omax : cout, to)), block(256);
    if constexpr (sizeof(T) == 2) {
        if (BK == 32) {           // the 16x16x32 kernel's image (3x3 only)
            hipLaunchKernelGGL((conv2d_pack_tile_kernel<T, 9, 32>), grid, block, 0, st, (T*)dst0, (T*)dst1, w, cout, cin, rows_pad0, rows_pad1);
            return;
        }
    }
    if (ks == 3) hipLaunchKernelGGL((conv2d_pack_tile_kernel<T, 9, BKT>), grid, block, 0, st, (T*)dst0, (T*)dst1, w, cout, cin, rows_pad0, rows_pad1);
    else hipLaunchKernelGGL((conv2d_pack_tile_kernel<T, 1, BKT>), grid, block, 0, st, (T*)dst0, (T*)dst1, w, cout, cin, rows_pad0, rows_pad1);
}

static int pack_weights2_bk(void* dst_fwd, void* dst_dgrad, const float* w, int32_t dtype, int32_t cout, int32_t cin, int32_t ks,
                            int32_t rows_pad_fwd, int32_t rows_pad_dgrad, int BK, void* stream);
extern "C" int afcm_conv2d_pack_weights2(void* dst_fwd, void* dst_dgrad, const float* w, int32_t dtype, int32_t cout, int32_t cin, int32_t ks,
                                         int32_t rows_pad_fwd, int32_t rows_pad_dgrad, void* stream) {
    return pack_weights2_bk(dst_fwd, dst_dgrad, w, dtype, cout, cin, ks, rows_pad_fwd, rows_pad_dgrad, conv_bk(dtype, ks), stream);
}
extern "C" int afcm_conv2d_pack_weights_bk(void* dst, const float* w, int32_t dtype, int32_t cout, int32_t cin, int32_t ks, int32_t mode,
                                           int32_t rows_pad, int32_t block_k, void* stream) {
    AFCM_REQUIRE(dst != nullptr && w != nullptr, "conv2d_pack_weights: null pointer");
    AFCM_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (forward) or 1 (data gradient)");
    AFCM_REQUIRE(block_k == afcm_conv2d_block_k(dtype) || block_k == conv_bk(dtype, ks), "conv2d_pack_weights_bk: K-chunk %d is not one of this dtype's", block_k);
    return mode == 0 ? pack_weights2_bk(dst, nullptr, w, dtype, cout, cin, ks, rows_pad, 0, block_k, stream)
                     : pack_weights2_bk(nullptr, dst, w, dtype, cout, cin, ks, 0, rows_pad, block_k, stream);
}
static int pack_weights2_bk(void* dst_fwd, void* dst_dgrad, const float* w, int32_t dtype, int32_t cout, int32_t cin, int32_t ks,
                            int32_t rows_pad_fwd, int32_t rows_pad_dgrad, int BK, void* stream) {
    AFCM_REQUIRE(w != nullptr && (dst_fwd != nullptr || dst_dgrad != nullptr), "conv2d_pack_weights: null pointer");
    AFCM_REQUIRE(dtype == AFCM_F32 || dtype == AFCM_F16 || dtype == AFCM_BF16, "dtype must be float32, float16 or bfloat16");
    AFCM_REQUIRE(ks == 1 || ks == 3, "only 1x1 and 3x3 kernels are supported");
    AFCM_REQUIRE(cout > 0 && cin > 0, "conv2d_pack_weights: empty weights");
    AFCM_REQUIRE(dst_fwd == nullptr || (rows_pad_fwd >= cout && rows_pad_fwd % 64 == 0), "rows_pad must be a multiple of 64 covering the rows");
    AFCM_REQUIRE(dst_dgrad == nullptr || (rows_pad_dgrad >= cin && rows_pad_dgrad % 64 == 0), "rows_pad must be a multiple of 64 covering the rows");
    AFCM_REQUIRE((((uintptr_t)dst_fwd | (uintptr_t)dst_dgrad) & 31) == 0, "conv2d_pack_weights: destinations must be 32-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
        case AFCM_F32: launch_pack8<float>(dst_fwd, dst_dgrad, w, cout, cin, ks, rows_pad_fwd, rows_pad_dgrad, BK, st); break;
        case AFCM_F16: launch_pack8<f16_t>(dst_fwd, dst_dgrad, w, cout, cin, ks, rows_pad_fwd, rows_pad_dgrad, BK, st); break;
        default: launch_pack8<bf16_t>(dst_fwd, dst_dgrad, w, cout, cin, ks, rows_pad_fwd, rows_pad_dgrad, BK, st); break;
    }
    return hip_status(hipGetLastError());
}

extern "C" int afcm_conv2d_pack_weights(void* dst, const float* w, int32_t dtype, int32_t cout, int32_t cin, int32_t ks,
                                        int32_t mode, int32_t rows_pad, void* stream) {
    AFCM_REQUIRE(dst != nullptr && w != nullptr, "conv2d_pack_weights: null pointer");
    AFCM_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (forward) or 1 (data gradient)");
    return mode == 0 ? afcm_conv2d_pack_weights2(dst, nullptr, w, dtype, cout, cin, ks, rows_pad, 0, stream)
                     : afcm_conv2d_pack_weights2(nullptr, dst, w, dtype, cout, cin, ks, 0, rows_pad, stream);
}

template <typename T>
static void launch_pack_bank(const PackBank& b, int blocks, int ks, int BK, hipStream_t st) {
    constexpr int BKT = ConvCfg<T>::BK;
    if constexpr (sizeof(T) == 2) {
        if (BK == 32) {
            hipLaunchKernelGGL((conv2d_pack_bank_kernel<T, 9, 32>), dim3(blocks), dim3(256), 0, st, b);
            return;
        }
    }
    if (ks == 3) hipLaunchKernelGGL((conv2d_pack_bank_kernel<T, 9, BKT>), dim3(blocks), dim3(256), 0, st, b);
    else hipLaunchKernelGGL((conv2d_pack_bank_kernel<T, 1, BKT>), dim3(blocks), dim3(256), 0, st, b);
}

extern "C" int afcm_conv2d_pack_bank(const afcm_pack_entry* entries, int32_t count, int32_t dtype, int32_t ks, void* stream) {
    AFCM_REQUIRE(entries != nullptr && count > 0 && count <= AFCM_PACK_MAX, "conv2d_pack_bank: 1..%d entries", AFCM_PACK_MAX);
    AFCM_REQUIRE(dtype == AFCM_F32 || dtype == AFCM_F16 || dtype == AFCM_BF16, "dtype must be float32, float16 or bfloat16");
    AFCM_REQUIRE(ks == 1 || ks == 3, "only 1x1 and 3x3 kernels are supported");
    const int BK = conv_bk(dtype, ks);
    const int ti = BK > 16 ? PackTile<32>::TI : 64, to = BK > 16 ? PackTile<32>::TO : 16;
    PackBank b;
    b.count = count;
    int tot = 0;
    for (int l = 0; l < count; l++) {
        const afcm_pack_entry& e = entries[l];
        AFCM_REQUIRE(e.w != nullptr && (e.dst_fwd != nullptr || e.dst_dgrad != nullptr) && e.cout > 0 && e.cin > 0, "conv2d_pack_bank: entry %d: null pointer or empty weights", l);
        AFCM_REQUIRE(e.dst_fwd == nullptr || (e.rows_pad_fwd >= e.cout && e.rows_pad_fwd % 64 == 0), "conv2d_pack_bank: entry %d: rows_pad must be a multiple of 64 covering the rows", l);
        AFCM_REQUIRE(e.dst_dgrad == nullptr || (e.rows_pad_dgrad >= e.cin && e.rows_pad_dgrad % 64 == 0), "conv2d_pack_bank: entry %d: rows_pad must be a multiple of 64 covering the rows", l);
        AFCM_REQUIRE((((uintptr_t)e.dst_fwd | (uintptr_t)e.dst_dgrad) & 31) == 0, "conv2d_pack_bank: entry %d: destinations must be 32-byte aligned", l);
        // as launch_pack8: tiles cover the padded row ranges of both images
        const int omax = e.dst_fwd ? e.rows_pad_fwd : round_up(e.cout, BK), imax = e.dst_dgrad ? e.rows_pad_dgrad : round_up(e.cin, BK);
        const int gx = cdiv(imax > e.cin ? imax : e.cin, ti), gy = cdiv(omax > e.cout ? omax : e.cout, to);
        b.e[l] = e;
        b.gx[l] = gx;
        b.blk[l] = tot;
        tot += gx * gy;
    }
    b.blk[count] = tot;
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
        case AFCM_F32: launch_pack_bank<float>(b, tot, ks, BK, st); break;
        case AFCM_F16: launch_pack_bank<f16_t>(b, tot, ks, BK, st); break;
        default: launch_pack_bank<bf16_t>(b, tot, ks, BK, st); break;
    }
    return hip_status(hipGetLastError());
}

extern "C" int afcm_conv2d_stride2(void* y, const void* x, const void* wpacked, int32_t dtype, int32_t n, int32_t cin, int32_t cout, int32_t h,
                                   int32_t w, int32_t pad, int32_t rows_pad, void* stream) {
    AFCM_REQUIRE(y != nullptr && x != nullptr && wpacked != nullptr, "conv2d_stride2: null pointer");
    AFCM_REQUIRE(dtype == AFCM_F16 || dtype == AFCM_BF16, "conv2d_stride2: 16-bit activations only");
    AFCM_REQUIRE(n > 0 && cin > 0 && cout > 0 && h > 0 && w > 0 && (w % 2) == 0, "conv2d_stride2: empty x or odd width %d", w);
    AFCM_REQUIRE(pad >= 0 && pad <= 2, "padding must be in [0, k-1]");
    AFCM_REQUIRE(rows_pad >= cout && rows_pad % 128 == 0, "conv2d_stride2: rows_pad must be a multiple of 128 covering cout");
    AFCM_REQUIRE(h + 2 * pad >= 3 && w + 2 * pad >= 3, "output must be at least 1x1");
    const int P = (h + 2 * pad - 3) / 2 + 1, Q = (w + 2 * pad - 3) / 2 + 1;
    int TH, TW, PWL;
    choose_tile_s2(P, Q, &TH, &TW, &PWL);
    const ConvParams p = conv_params(y, x, wpacked, nullptr, nullptr, n, cin, cout, h, w, P, Q, pad, w, Q, TH, TW, PWL, rows_pad,
                                     cdiv(cin, afcm_conv2d_block_k(dtype)));
    const long long blocks = (long long)p.tilesX * p.tilesY * n * cdiv(cout, 128);
    AFCM_REQUIRE(blocks > 0 && blocks < (1ll << 31), "conv2d_stride2: grid of %lld blocks is out of range", blocks);
    AFCM_REQUIRE((long long)cin * h * w * 2ll < (1ll << 31), "conv2d_stride2: image out of range");
    if (dtype == AFCM_F16) hipLaunchKernelGGL((conv2d_fwd16s2_kernel<f16_t, 128>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((conv2d_fwd16s2_kernel<bf16_t, 128>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    return hip_status(hipGetLastError());
}

extern "C" int afcm_conv2d(void* y, const void* x, const void* wpacked, const float* oscale, const float* obias, int32_t dtype, int32_t n,
                           int32_t cin, int32_t cout, int32_t h, int32_t w, int32_t ks, int32_t pad, int32_t rows_pad, void* stream) {
    return afcm_conv2d_ld(y, x, wpacked, oscale, obias, dtype, n, cin, cout, h, w, ks, pad, rows_pad, 0, 0, stream);
}

extern "C" int afcm_conv2d_ld(void* y, const void* x, const void* wpacked, const float* oscale, const float* obias, int32_t dtype, int32_t n,
                              int32_t cin, int32_t cout, int32_t h, int32_t w, int32_t ks, int32_t pad, int32_t rows_pad, int32_t x_pitch,
                              int32_t y_pitch, void* stream) {
    AFCM_REQUIRE(y != nullptr && x != nullptr && wpacked != nullptr, "conv2d: null pointer");
    AFCM_REQUIRE(dtype == AFCM_F32 || dtype == AFCM_F16 || dtype == AFCM_BF16, "x must be float32, float16 or bfloat16");
    AFCM_REQUIRE(n > 0 && cin > 0 && cout > 0 && h > 0 && w > 0, "x is empty");
    AFCM_REQUIRE(ks == 1 || ks == 3, "only 1x1 and 3x3 kernels are supported");
    AFCM_REQUIRE(pad >= 0 && pad <= ks - 1, "padding must be in [0, k-1]");
    AFCM_REQUIRE(dtype == AFCM_F32 || (w % 2 == 0), "16-bit conv2d needs an even input width (got %d)", w);
    AFCM_REQUIRE(rows_pad >= cout && rows_pad % 64 == 0, "rows_pad must be a multiple of 64 covering cout");
    const int P = h + 2 * pad - ks + 1, Q = w + 2 * pad - ks + 1;
    AFCM_REQUIRE(P >= 1 && Q >= 1, "output must be at least 1x1");
    const int ldx = x_pitch ? x_pitch : w, ldy = y_pitch ? y_pitch : Q;
    if (ldx != w || ldy != Q) {
        AFCM_REQUIRE(dtype != AFCM_F32 && ks == 3, "conv2d: row pitches need the 16-bit 3x3 kernel");
        AFCM_REQUIRE(ldx >= w && ldy >= Q && ((ldx | ldy) & 1) == 0, "conv2d: row pitches %d / %d must be even and cover the widths %d / %d", ldx, ldy, w, Q);
        AFCM_REQUIRE((long long)cout * P * ldy < (1ll << 30), "conv2d: pitched output image is out of range");
    }
    AFCM_REQUIRE(dtype == AFCM_F32 || ks != 3 || (long long)cout * P * ldy * 2 < (1ll << 30), "conv2d: 16-bit output image of %lld bytes is out of range (< 2^30)", (long long)cout * P * ldy * 2);
    const ConvPlan pl = conv_plan(dtype, n, cin, cout, P, Q, ks, rows_pad, ldy, false);
    if (pl.family == kConvDirect)
        return conv2d_direct_small_cin(x, y, wpacked, oscale, obias, dtype, n, cin, cout, h, w, pad, rows_pad, 32, ldx, ldy, (hipStream_t)stream);
    ConvParams p = conv_params(y, x, wpacked, oscale, obias, n, cin, cout, h, w, P, Q, pad, ldx, ldy, pl.TH, pl.TW, pl.PWL, rows_pad, cdiv(cin, conv_bk(dtype, ks)));
    hipStream_t st = (hipStream_t)stream;
    if (pl.family == kConv96) {
        AFCM_REQUIRE(pl.items > 0 && pl.items < (1ll << 31), "conv2d: grid of %lld blocks is out of range", pl.items);
        p.total_blocks = (int)pl.items;
        const dim3 g96((unsigned)pl.grid);
        return dtype == AFCM_F16 ? launch_fwd16x<f16_t, 96, false>(p, g96, pl.fast, st) : launch_fwd16x<bf16_t, 96, false>(p, g96, pl.fast, st);
    }
    if (pl.family == kConv128p64) {
        const long long items128 = pl.items * pl.big;
        const int rc = dtype == AFCM_F16 ? launch_conv<f16_t, 128>(p, ks, st, items128, items128, pl.fast)
                                         : launch_conv<bf16_t, 128>(p, ks, st, items128, items128, pl.fast);
        if (rc != AFCM_OK) return rc;
        return dtype == AFCM_F16 ? launch_conv<f16_t, 64>(p, ks, st, pl.items, pl.grid, pl.fast, pl.big * 128)
                                 : launch_conv<bf16_t, 64>(p, ks, st, pl.items, pl.grid, pl.fast, pl.big * 128);
    }
    const bool small = pl.family == kConv64;
    switch (dtype) {
        case AFCM_F32: return small ? launch_conv<float, 64>(p, ks, st, pl.items, pl.grid, pl.fast) : launch_conv<float, 128>(p, ks, st, pl.items, pl.grid, pl.fast);
        case AFCM_F16: return small ? launch_conv<f16_t, 64>(p, ks, st, pl.items, pl.grid, pl.fast) : launch_conv<f16_t, 128>(p, ks, st, pl.items, pl.grid, pl.fast);
        default: return small ? launch_conv<bf16_t, 64>(p, ks, st, pl.items, pl.grid, pl.fast) : launch_conv<bf16_t, 128>(p, ks, st, pl.items, pl.grid, pl.fast);
    }
}

extern "C" int afcm_conv2d_pack_split(void* dst, const float* w, const uint32_t* bound, int32_t dtype, int32_t cout, int32_t cin, int32_t mode,
                                      int32_t rows_pad, int32_t terms, uint32_t term_wparts, void* stream) {
    AFCM_REQUIRE(dst != nullptr && w != nullptr, "conv2d_pack_split: null pointer");
    AFCM_REQUIRE(dtype == AFCM_BF16 || dtype == AFCM_F16, "conv2d_pack_split: parts are bfloat16 or float16");
    AFCM_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (forward) or 1 (data gradient)");
    AFCM_REQUIRE(terms >= 1 && terms <= 8 && cout > 0 && cin > 0, "conv2d_pack_split: 1..8 terms");
    const int rows = mode == 0 ? cout : cin, cols = mode == 0 ? cin : cout;
    AFCM_REQUIRE(rows_pad >= rows && rows_pad % 64 == 0, "rows_pad must be a multiple of 64 covering the rows");
    for (int t = 0; t < terms; t++) AFCM_REQUIRE(((term_wparts >> (4 * t)) & 15u) <= 2, "conv2d_pack_split: parts 0..2");
    const int BK = conv_bk(dtype, 3);
    const int nkc_real = cdiv(cols, BK);
    const long long total = (long long)terms * nkc_real * 9 * rows_pad * BK;
    long long blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == AFCM_BF16) hipLaunchKernelGGL((conv2d_pack_split_kernel<bf16_t>), dim3((unsigned)blocks), dim3(256), 0, st, (bf16_t*)dst, w, (const unsigned*)bound, cout, cin, rows, cols, rows_pad, nkc_real, terms, term_wparts, mode, BK);
    else hipLaunchKernelGGL((conv2d_pack_split_kernel<f16_t>), dim3((unsigned)blocks), dim3(256), 0, st, (f16_t*)dst, w, (const unsigned*)bound, cout, cin, rows, cols, rows_pad, nkc_real, terms, term_wparts, mode, BK);
    return hip_status(hipGetLastError());
}

extern "C" int afcm_conv2d_split(float* y, const void* x_parts, const void* wpacked, const float* oscale, const float* obias, int32_t dtype, int32_t n,
                                 int32_t cin, int32_t cout, int32_t h, int32_t w, int32_t pad, int32_t rows_pad, int32_t terms, uint32_t term_parts,
                                 int64_t part_stride, const uint32_t* bound_a, const uint32_t* bound_b, void* stream) {
    const int ks = 3;
    AFCM_REQUIRE(y != nullptr && x_parts != nullptr && wpacked != nullptr, "conv2d_split: null pointer");
    AFCM_REQUIRE(dtype == AFCM_BF16 || dtype == AFCM_F16, "conv2d_split: parts are bfloat16 or float16");
    AFCM_REQUIRE(n > 0 && cin > 0 && cout > 0 && h > 0 && w > 0, "x is empty");
    AFCM_REQUIRE(pad >= 0 && pad <= ks - 1, "padding must be in [0, k-1]");
    AFCM_REQUIRE(w % 2 == 0, "conv2d_split needs an even input width (got %d)", w);
    AFCM_REQUIRE(rows_pad >= cout && rows_pad % 64 == 0, "rows_pad must be a multiple of 64 covering cout");
    AFCM_REQUIRE(terms >= 1 && terms <= 8, "conv2d_split: 1..8 terms (got %d)", terms);
    int max_part = 0;
    for (int t = 0; t < terms; t++) max_part = std::max(max_part, (int)((term_parts >> (4 * t)) & 15u));
    AFCM_REQUIRE(max_part <= 2, "conv2d_split: parts 0..2");
    AFCM_REQUIRE(part_stride >= (long long)n * cin * h * w && (long long)max_part * part_stride * 2 < (1ll << 31) - (long long)cin * h * w * 2,
                 "conv2d_split: part stride %lld out of range", (long long)part_stride);
    const int P = h + 2 * pad - ks + 1, Q = w + 2 * pad - ks + 1;
    AFCM_REQUIRE(P >= 1 && Q >= 1, "output must be at least 1x1");
    const ConvPlan pl = conv_plan(dtype, n, cin, cout, P, Q, ks, rows_pad, Q, true);
    const int nkc_real = cdiv(cin, conv_bk(dtype, 3));
    ConvParams p = conv_params(y, x_parts, wpacked, oscale, obias, n, cin, cout, h, w, P, Q, pad, w, Q, pl.TH, pl.TW, pl.PWL, rows_pad, nkc_real);
    p.nkc = terms * p.nkc_real;
    p.magicNK = magic_u32((unsigned)p.nkc_real);
    p.term_parts = term_parts;
    p.part_bytes = (int)(part_stride * 2);
    p.last_part_bytes = max_part * p.part_bytes;
    p.bound_a = (const unsigned*)bound_a; p.bound_b = (const unsigned*)bound_b;
    const bool small = pl.family == kConv64;
    const long long blocks = pl.items;
    AFCM_REQUIRE(blocks > 0 && blocks < (1ll << 31), "conv2d_split: grid of %lld blocks is out of range", blocks);
    hipStream_t st = (hipStream_t)stream;
    p.total_blocks = (int)blocks;
    const dim3 pgrid((unsigned)pl.grid);
    if (dtype == AFCM_BF16) return small ? launch_fwd16x<bf16_t, 64, true>(p, pgrid, false, st) : launch_fwd16x<bf16_t, 128, true>(p, pgrid, false, st);
    return small ? launch_fwd16x<f16_t, 64, true>(p, pgrid, false, st) : launch_fwd16x<f16_t, 128, true>(p, pgrid, false, st);
}

// Pure host: the plan afcm_conv2d_ld (split == 0) / afcm_conv2d_split (split != 0) follow for these arguments, rows_pad = cout rounded up to 64
extern "C" int afcm_conv2d_plan(int32_t dtype, int32_t n, int32_t cin, int32_t cout, int32_t h, int32_t w, int32_t ks, int32_t pad, int32_t x_pitch,
                                int32_t y_pitch, int32_t split, int32_t out[8]) {
    AFCM_REQUIRE(out != nullptr, "conv2d_plan: null pointer");
    AFCM_REQUIRE(dtype == AFCM_F32 || dtype == AFCM_F16 || dtype == AFCM_BF16, "x must be float32, float16 or bfloat16");
    AFCM_REQUIRE(n > 0 && cin > 0 && cout > 0 && h > 0 && w > 0, "x is empty");
    AFCM_REQUIRE(ks == 1 || ks == 3, "only 1x1 and 3x3 kernels are supported");
    AFCM_REQUIRE(pad >= 0 && pad <= ks - 1, "padding must be in [0, k-1]");
    AFCM_REQUIRE(!split || (ks == 3 && dtype != AFCM_F32), "conv2d_plan: the split route is 3x3 on 16-bit parts");
    const int P = h + 2 * pad - ks + 1, Q = w + 2 * pad - ks + 1;
    AFCM_REQUIRE(P >= 1 && Q >= 1, "output must be at least 1x1");
    (void)x_pitch;                                    // (no decision depends on the input pitch)
    const ConvPlan pl = conv_plan(dtype, n, cin, cout, P, Q, ks, round_up(cout, 64), (!split && y_pitch) ? y_pitch : Q, split != 0);
    AFCM_REQUIRE(pl.items < (1ll << 31), "conv2d_plan: grid of %lld blocks is out of range", pl.items);
    out[0] = pl.family; out[1] = pl.rows; out[2] = pl.TH; out[3] = pl.TW; out[4] = (int32_t)pl.items; out[5] = (int32_t)pl.grid;
    out[6] = pl.fast ? 1 : 0; out[7] = pl.kernel;
    return AFCM_OK;
}
