// Exact LDS-tile kernels of filtered_lrelu (every dtype; the 16-bit matrix-core kernels replace them where they apply):
// wave64 workgroups, one output tile per workgroup staged through LDS in five register-blocked passes (load+bias, up-FIR along
// x, up-FIR along y + activation + sign codes, down-FIR along x, down-FIR along y + store), fp32 arithmetic throughout.  Filter
// taps are expanded into per-phase polyphase tables in LDS by the kernel itself -- no global filter buffer, so launches on
// different streams never interfere.  Sign codes use layout 0.
//
// Polyphase indexing (derivation in DESIGN.md): for a tile whose upsampled origin is U0,
//   d = U0 - px0,  I0 = ceil(d / up),  ph = up*I0 - d  in [0, up)
//   u[U0 + up*m + a] = sum_j F[kmin(a) + up*j] * x[I0 + m + o(a) + j]
//   o(a) = (a > ph),  kmin(a) = o(a) ? up - (a - ph) : ph - a,   F = flip ? fu : reversed(fu)
#include "flrelu_common.h"

namespace afcm {

// ---------------------------------------------------------------------------------------------
template <typename T, int UP, int DOWN, int FUT, int FD, int TOW, int TOH, int RO, int NT, int SIGN>
struct FlreluTile {
    static constexpr int FU = UP * FUT;
    static constexpr int TUW = (TOW - 1) * DOWN + FD;      // upsampled columns the tile's outputs need
    static constexpr int TUH = (TOH - 1) * DOWN + FD;
    static constexpr int TUWP = round_up(TUW, 16);         // computed/pitched width (16 = one sign dword)
    static constexpr int ROWS_C = 8;                       // upsampled rows per stage-C item
    static constexpr int TUHP = round_up(TUH, ROWS_C);
    static constexpr int MB = ROWS_C / UP;                 // input-row steps per stage-C item
    static constexpr int TIW = TUWP / UP + FUT;
    // LDS row pitches are odd multiples of 4 floats (16 B): lanes that walk down consecutive rows at a fixed
    // column then hit 16 distinct 16-byte slots per ds_read_b128 / ds_write_b128 lane group (conflict-free).
    static constexpr int TIWP = odd4(round_up(TIW + 2, 4));     // sIn pitch (+2: stage B reads 12 floats per item)
    static constexpr int PU = odd4(TUWP);                       // upX / upXY pitch
    static constexpr int PD = odd4(TOW);                        // downX pitch
    static constexpr int TIH = TUHP / UP + FUT;
    static constexpr int SZ_A = cmax(TIH * TIWP, TUHP * PU);    // sIn, later upXY
    static constexpr int SZ_B = cmax(TIH * PU, TUH * PD);       // upX, later downX
    static constexpr int NCOEF = 2 * FU + FD;
    // READ mode: the tile's window of the sign tensor, staged as dwords (16 codes each): per row the
    // dwords covering columns [U0x + sx, U0x + sx + TUWP) -- TUWP/16 + 1 of them because sx is arbitrary.
    static constexpr int SGN_W = TUWP / 16 + 1;
    static constexpr int SGN_WORDS = (SIGN == AFCM_SIGNS_READ) ? TUHP * SGN_W : 0;
    static constexpr int LDS_FLOATS = SZ_A + SZ_B + round_up(NCOEF, 4) + SGN_WORDS;
    static_assert(ROWS_C % UP == 0 && FUT % 2 == 0 && TOW % 4 == 0 && TOH % RO == 0, "tile shape");
    static_assert((TOW * DOWN) % 16 == 0, "sign ownership must fall on dword boundaries");
    static_assert(DOWN * (TOW - 4) + round_up(DOWN * 3 + FD, 4) <= PU, "stage D over-read must stay inside the row");
    static_assert(LDS_FLOATS * 4 <= 160 * 1024, "LDS overflow");

    // Stage the sign window into LDS.  Dwords outside the tensor read as 0 (= values pass unchanged).
    static __device__ __forceinline__ void stage_signs(unsigned* __restrict__ sgn, const FlreluParams& p, int plane,
                                                       int U0x, int U0y, int tid) {
        const unsigned* splane = (const unsigned*)(p.s + (size_t)plane * p.sh * p.swb);
        const int wpr = p.swb >> 2;                         // dwords per sign row
        const int w0 = (U0x + p.sx) >> 4;                   // floor: arithmetic shift
        constexpr int NW = cdiv(TUHP * SGN_W, NT);
        unsigned v[NW];
#pragma unroll
        for (int i = 0; i < NW; i++) {
            const int idx = tid + i * NT;
            const int r = idx / SGN_W, c = idx - r * SGN_W;
            const int Y = U0y + p.sy + r, wi = w0 + c;
            const bool ok = idx < TUHP * SGN_W && (unsigned)Y < (unsigned)p.sh && (unsigned)wi < (unsigned)wpr;
            v[i] = ok ? splane[(size_t)Y * wpr + wi] : 0u;
        }
#pragma unroll
        for (int i = 0; i < NW; i++) {
            const int idx = tid + i * NT;
            if (idx < TUHP * SGN_W) sgn[idx] = v[i];
        }
    }

    // ---- stage B: up-FIR along x.  One item = one input row x 4 input columns -> 4*UP outputs.
    template <int PH>
    static __device__ __forceinline__ void up_x(const float* __restrict__ sIn, float* __restrict__ upX,
                                                const float* __restrict__ cu, int tid) {
        float c[UP][FUT];
#pragma unroll
        for (int a = 0; a < UP; a++)
#pragma unroll
            for (int j = 0; j < FUT; j++) c[a][j] = cu[a * FUT + j];
        constexpr int NCH = TUWP / (4 * UP);
        constexpr int NIN4 = cdiv(4 + FUT, 4);
        for (int item = tid; item < TIH * NCH; item += NT) {
            const int ch = item / TIH, r = item - ch * TIH;     // consecutive lanes -> consecutive rows
            const float* src = sIn + r * TIWP + 4 * ch;
            float in[NIN4 * 4];
#pragma unroll
            for (int i = 0; i < NIN4; i++) {
                float4 t = *(const float4*)(src + 4 * i);
                in[4 * i] = t.x; in[4 * i + 1] = t.y; in[4 * i + 2] = t.z; in[4 * i + 3] = t.w;
            }
            float out[4 * UP];
#pragma unroll
            for (int mm = 0; mm < 4; mm++)
#pragma unroll
                for (int a = 0; a < UP; a++) {
                    const int o = (a > PH) ? 1 : 0;
                    float acc = 0.f;
#pragma unroll
                    for (int j = 0; j < FUT; j++) acc = fmaf(c[a][j], in[mm + o + j], acc);
                    out[mm * UP + a] = acc;
                }
            float* dst = upX + r * PU + 4 * UP * ch;
#pragma unroll
            for (int q = 0; q < UP; q++) *(float4*)(dst + 4 * q) = make_float4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]);
        }
    }

    // ---- stage C: up-FIR along y + gain + leaky ReLU + clamp + sign codes.  One item = 4 columns x 8 rows.
    template <int PH>
    static __device__ __forceinline__ void up_y_act(const float* __restrict__ upX, float* __restrict__ upXY,
                                                    const float* __restrict__ cu, const unsigned* __restrict__ sgn, int tid,
                                                    const FlreluParams& p, int plane, int U0x, int U0y, bool lastX, bool lastY) {
        float c[UP][FUT];
#pragma unroll
        for (int a = 0; a < UP; a++)
#pragma unroll
            for (int j = 0; j < FUT; j++) c[a][j] = cu[a * FUT + j];
        constexpr int NG = TUWP / 4;
        constexpr int NRB = TUHP / ROWS_C;
        constexpr int NIN = MB + FUT;
        unsigned char* splane = p.s + (size_t)plane * p.sh * p.swb;
        for (int item = tid; item < NG * NRB; item += NT) {
            const int rb = item / NG, g = item - rb * NG;
            float4 in[NIN];
#pragma unroll
            for (int i = 0; i < NIN; i++) in[i] = *(const float4*)(upX + (rb * MB + i) * PU + 4 * g);
            const int X = U0x + 4 * g;
            // READ mode: bit offset of this item's 4 codes inside the staged dword pair
            const int sbit = (((U0x + p.sx) & 15) + 4 * g) * 2;
            const int sw0 = sbit >> 5, sshift = sbit & 31;
#pragma unroll
            for (int mm = 0; mm < MB; mm++)
#pragma unroll
                for (int a = 0; a < UP; a++) {
                    const int o = (a > PH) ? 1 : 0;
                    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int j = 0; j < FUT; j++) {
                        const float w = c[a][j];
                        const float4 v = in[mm + o + j];
                        acc.x = fmaf(w, v.x, acc.x);
                        acc.y = fmaf(w, v.y, acc.y);
                        acc.z = fmaf(w, v.z, acc.z);
                        acc.w = fmaf(w, v.w, acc.w);
                    }
                    const int row = rb * ROWS_C + mm * UP + a;
                    const int Y = U0y + row;
                    unsigned codes = 0;
                    if (SIGN == AFCM_SIGNS_READ) {
                        const unsigned lo = sgn[row * SGN_W + sw0];
                        const unsigned hi = (sw0 + 1 < SGN_W) ? sgn[row * SGN_W + sw0 + 1] : 0u;
                        codes = __builtin_amdgcn_alignbit(hi, lo, sshift) & 0xffu;
                    }
                    unsigned c0 = act_elem<SIGN>(acc.x, p.gain, p.slope, p.clamp, codes);
                    unsigned c1 = act_elem<SIGN>(acc.y, p.gain, p.slope, p.clamp, codes >> 2);
                    unsigned c2 = act_elem<SIGN>(acc.z, p.gain, p.slope, p.clamp, codes >> 4);
                    unsigned c3 = act_elem<SIGN>(acc.w, p.gain, p.slope, p.clamp, codes >> 6);
                    *(float4*)(upXY + row * PU + 4 * g) = acc;
                    if (SIGN == AFCM_SIGNS_WRITE) {
                        // 4 lanes of a quad hold 16 consecutive columns: assemble one dword.
                        int byte = (int)(c0 | (c1 << 2) | (c2 << 4) | (c3 << 6));
                        int word = quad_or(byte << ((g & 3) << 3));
                        const bool ownX = (4 * g < TOW * DOWN) || lastX;
                        const bool ownY = (row < TOH * DOWN) || lastY;
                        if ((g & 3) == 0 && ownX && ownY && (X >> 2) < p.swb && Y < p.sh)
                            *(int*)(splane + (size_t)Y * p.swb + (X >> 2)) = word;
                    }
                }
        }
    }

    // ---- stage D: down-FIR along x.  One item = one upsampled row x 4 outputs.
    static __device__ __forceinline__ void down_x(const float* __restrict__ upXY, float* __restrict__ downX,
                                                  const float* __restrict__ cdl, int tid) {
        float cd[FD];
#pragma unroll
        for (int k = 0; k < FD; k++) cd[k] = cdl[k];
        constexpr int NCD = TOW / 4;
        constexpr int NIN4 = cdiv(DOWN * 3 + FD, 4);
        for (int item = tid; item < TUH * NCD; item += NT) {
            const int ch = item / TUH, r = item - ch * TUH;     // consecutive lanes -> consecutive rows
            const float* src = upXY + r * PU + DOWN * 4 * ch;
            float in[NIN4 * 4];
#pragma unroll
            for (int i = 0; i < NIN4; i++) {
                float4 t = *(const float4*)(src + 4 * i);
                in[4 * i] = t.x; in[4 * i + 1] = t.y; in[4 * i + 2] = t.z; in[4 * i + 3] = t.w;
            }
            float out[4];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < FD; k++) acc = fmaf(cd[k], in[DOWN * t + k], acc);
                out[t] = acc;
            }
            *(float4*)(downX + r * PD + 4 * ch) = make_float4(out[0], out[1], out[2], out[3]);
        }
    }

    // ---- stage E: down-FIR along y + store.  One item = 2 output columns x RO output rows.
    static __device__ __forceinline__ void down_y_store(const float* __restrict__ downX, const float* __restrict__ cdl,
                                                        int tid, const FlreluParams& p, int plane, int O0x, int O0y) {
        float cd[FD];
#pragma unroll
        for (int k = 0; k < FD; k++) cd[k] = cdl[k];
        constexpr int NCP = TOW / 2;
        constexpr int NROW = DOWN * (RO - 1) + FD;
        T* yp = (T*)p.y + (size_t)plane * p.yh * p.yw;
        for (int item = tid; item < NCP * (TOH / RO); item += NT) {
            const int rbk = item / NCP, cp = item - rbk * NCP;
            const int p0 = rbk * RO;
            float2 acc[RO];
#pragma unroll
            for (int t = 0; t < RO; t++) acc[t] = make_float2(0.f, 0.f);
#pragma unroll
            for (int i = 0; i < NROW; i++) {
                const float2 v = *(const float2*)(downX + (DOWN * p0 + i) * PD + 2 * cp);
#pragma unroll
                for (int t = 0; t < RO; t++) {
                    const int k = i - DOWN * t;
                    if (k >= 0 && k < FD) {
                        acc[t].x = fmaf(cd[k], v.x, acc[t].x);
                        acc[t].y = fmaf(cd[k], v.y, acc[t].y);
                    }
                }
            }
            const int ox = O0x + 2 * cp;
#pragma unroll
            for (int t = 0; t < RO; t++) {
                const int oy = O0y + p0 + t;
                if (oy < p.yh) {
                    T* dst = yp + (size_t)oy * p.yw + ox;
                    if (sizeof(T) == 4 && ox + 1 < p.yw && ((p.yw & 1) == 0)) {
                        // even plane widths: the pair starts on an 8-byte boundary -- one store instead of two interleaved ones
                        *(float2*)dst = acc[t];
                    } else {
                        if (ox < p.yw) dst[0] = from_f32<T>(acc[t].x);
                        if (ox + 1 < p.yw) dst[1] = from_f32<T>(acc[t].y);
                    }
                }
            }
        }
    }
};

// What flrelu_sep_kernel and flrelu_radial_kernel share word for word.  Macros, not functions: as __device__ __forceinline__
// helpers every one of these pieces changed the instructions of the kernels that used it, and the kernels keep the
// instructions they were measured with.  The macros read the kernel's p, tid, K, sgn and template parameters.
//
// LDS layout (two tile buffers, the coefficient tables, the READ mode's sign window), block decode and polyphase origin of the
// tile.  XCD-aware order: consecutive logical tiles (neighbours of one plane, shared halos) stay on one XCD / one L2.
#define FLRELU_TILE_PROLOGUE()                                                                                         \
    __shared__ __attribute__((aligned(16))) float lds[K::LDS_FLOATS];                                                  \
    float* bufA = lds; float* bufB = lds + K::SZ_A; float* coef = lds + K::SZ_A + K::SZ_B;                             \
    unsigned* sgn = (unsigned*)(lds + K::SZ_A + K::SZ_B + round_up(K::NCOEF, 4));                                      \
    const int tid = threadIdx.x;                                                                                       \
    int bid = xcd_order(blockIdx.x, gridDim.x);                                                                        \
    const int tx = bid % p.tilesX; bid /= p.tilesX;                                                                    \
    const int ty = bid % p.tilesY, plane = bid / p.tilesY;                                                             \
    const int O0x = tx * TOW, O0y = ty * TOH, U0x = O0x * DOWN, U0y = O0y * DOWN;                                      \
    const int I0x = -floor_div(p.px0 - U0x, UP), phx = pos_mod(p.px0 - U0x, UP);                                       \
    const int I0y = -floor_div(p.py0 - U0y, UP), phy = pos_mod(p.py0 - U0y, UP)

// Stage A: input tile + bias into `dst` (zero outside the image, without bias: the bias is added before padding).  All global
// loads of the tile are issued back to back before the first LDS write, so the tile pays one HBM round trip, not one per element.
#define FLRELU_TILE_STAGE_A(dst)                                                                                   \
    {                                                                                                              \
        const T* xp = (const T*)p.x + (size_t)plane * p.xh * p.xw;                                                 \
        const float bias = p.b ? to_f32(((const T*)p.b)[plane % p.C]) : 0.f;                                       \
        constexpr int NLD = cdiv(K::TIH * K::TIWP, NT);                                                            \
        T raw[NLD]; bool ok[NLD];                                                                                  \
        _Pragma("unroll") for (int i = 0; i < NLD; i++) {                                                          \
            const int idx = tid + i * NT;                                                                          \
            const int r = idx / K::TIWP, c = idx - r * K::TIWP;                                                    \
            const int iy = I0y + r, ix = I0x + c;                                                                  \
            ok[i] = (idx < K::TIH * K::TIWP) && (unsigned)ix < (unsigned)p.xw && (unsigned)iy < (unsigned)p.xh;    \
            raw[i] = ok[i] ? xp[(size_t)iy * p.xw + ix] : from_f32<T>(0.f);                                        \
        }                                                                                                          \
        if (SIGN == AFCM_SIGNS_READ) K::stage_signs(sgn, p, plane, U0x, U0y, tid);                                 \
        _Pragma("unroll") for (int i = 0; i < NLD; i++) {                                                          \
            const int idx = tid + i * NT;                                                                          \
            if (idx < K::TIH * K::TIWP) (dst)[idx] = ok[i] ? to_f32(raw[i]) + bias : 0.f;                          \
        }                                                                                                          \
    }                                                                                                              \
    __syncthreads()

// Stages B and C (separable up-FIR), each on the compile-time phase of the tile and with the barrier after it
#define FLRELU_TILE_UP_X(cuX)                                                                             \
    switch (phx) {                                                                                    \
        case 0: K::template up_x<0>(bufA, bufB, cuX, tid); break;                                     \
        case 1: K::template up_x<1>(bufA, bufB, cuX, tid); break;                                     \
        case 2: if (UP > 2) K::template up_x<(UP > 2 ? 2 : 0)>(bufA, bufB, cuX, tid); break;          \
        default: if (UP > 2) K::template up_x<(UP > 2 ? 3 : 0)>(bufA, bufB, cuX, tid); break;         \
    }                                                                                                 \
    __syncthreads()
#define FLRELU_TILE_UP_Y_ACT(cuY)                                                                                                     \
    switch (phy) {                                                                                                                    \
        case 0: K::template up_y_act<0>(bufB, bufA, cuY, sgn, tid, p, plane, U0x, U0y, lastX, lastY); break;                          \
        case 1: K::template up_y_act<1>(bufB, bufA, cuY, sgn, tid, p, plane, U0x, U0y, lastX, lastY); break;                          \
        case 2: if (UP > 2) K::template up_y_act<(UP > 2 ? 2 : 0)>(bufB, bufA, cuY, sgn, tid, p, plane, U0x, U0y, lastX, lastY); break;   \
        default: if (UP > 2) K::template up_y_act<(UP > 2 ? 3 : 0)>(bufB, bufA, cuY, sgn, tid, p, plane, U0x, U0y, lastX, lastY); break;  \
    }                                                                                                                                 \
    __syncthreads()

template <typename T, int UP, int DOWN, int FUT, int FD, int TOW, int TOH, int RO, int NT, int SIGN>
__global__ __launch_bounds__(NT) void flrelu_sep_kernel(FlreluParams p, const float* __restrict__ fu,
                                                        const float* __restrict__ fd) {
    typedef FlreluTile<T, UP, DOWN, FUT, FD, TOW, TOH, RO, NT, SIGN> K;
    FLRELU_TILE_PROLOGUE();
    float *cuX = coef, *cuY = cuX + K::FU, *cdl = cuY + K::FU;
    if (tid < K::FU) {      // polyphase coefficient tables
        const int a = tid / FUT, j = tid - a * FUT;
        {
            const int kmin = (a > phx) ? UP - (a - phx) : phx - a;
            const int k = kmin + UP * j;
            cuX[tid] = p.flip ? fu[k] : fu[K::FU - 1 - k];
        }
        {
            const int kmin = (a > phy) ? UP - (a - phy) : phy - a;
            const int k = kmin + UP * j;
            cuY[tid] = p.flip ? fu[k] : fu[K::FU - 1 - k];
        }
    }
    if (tid < FD) cdl[tid] = p.flip ? fd[tid] : fd[FD - 1 - tid];

    FLRELU_TILE_STAGE_A(bufA);
    FLRELU_TILE_UP_X(cuX);
    const bool lastX = (tx == p.tilesX - 1), lastY = (ty == p.tilesY - 1);
    FLRELU_TILE_UP_Y_ACT(cuY);
    K::down_x(bufA, bufB, cdl, tid);
    __syncthreads();
    K::down_y_store(bufB, cdl, tid, p, plane, O0x, O0y);
}

// ---------------------------------------------------------------------------------------------
// Radial (non-separable) forms of the tile kernel: one of the two filters is a full FD x FD (or FU x FU) 2-D filter, the
// other stays separable.  StyleGAN3-R's layers produce exactly these two argument sets ("filtered_lrelu with
// radial filters"):
//   SUFD  separable up, 2-D down (forward of a radial layer): stages A-C as above, then D + E become one 2-D decimating FIR
//         over the activated tile.  One item = 4 output columns x R2 output rows; every upsampled row the item reads feeds all
//         the item's outputs whose tap window covers it, even / odd taps in the two halves of packed FMAs.
//   FUSD  2-D up, separable down (backward of a radial layer): stage A as above, then B + C become one 2-D polyphase up-FIR
//         + gain / activation / clamp / codes.  One item = 4 input columns x 2 input rows -> 8 x 4 upsampled elements; the x
//         phase offset is folded into a 7-tap table with one zero (as in the strip kernel) so the two x phases of a column share
//         an input and form one packed FMA.  Stages D and E as above.
// The 2-D coefficient tables live in LDS and are read at wave-uniform addresses (broadcast).  Inside one upsampled / input row of
// an item, the loops over its output rows and columns are unrolled: the row's data, read once, serves every output of the item
// whose tap window covers it.  The loop over the item's rows stays ROLLED (#pragma unroll 1): unrolled, the compiler hoists every
// LDS read of the item and spills (256 VGPRs and 0.4-1.5 KB of scratch per lane).  Sign codes use the tile family's layout 0.
enum { FLRELU_SEP = 0, FLRELU_SUFD = 1, FLRELU_FUSD = 2 };       // = family - FLRELU_FAMILY_TILE_SEP (launch_tile)
static_assert(FLRELU_FAMILY_TILE_SUFD - FLRELU_FAMILY_TILE_SEP == FLRELU_SUFD && FLRELU_FAMILY_TILE_FUSD - FLRELU_FAMILY_TILE_SEP == FLRELU_FUSD, "modes");

template <typename T, int MODE, int UP, int DOWN, int FUT, int FD, int TOW, int TOH, int RO, int NT, int SIGN>
struct FlreluRadialTile : FlreluTile<T, UP, DOWN, FUT, FD, TOW, TOH, RO, NT, SIGN> {
    typedef FlreluTile<T, UP, DOWN, FUT, FD, TOW, TOH, RO, NT, SIGN> B;
    static constexpr int FU = B::FU, TUWP = B::TUWP, TUHP = B::TUHP, TIH = B::TIH, TIWP = B::TIWP, PU = B::PU, SGN_W = B::SGN_W;
    // SUFD: 2-D down table [FD][FD] after the separable up tables; FUSD: 2-D up table [UP][FUT][16] (7 x-phase pairs + pad),
    // then the separable down taps
    static constexpr int R2 = 2;                                 // SUFD output rows per item
    static constexpr int CU2_ROW = 16;
    static constexpr int NCOEF = MODE == FLRELU_SUFD ? 2 * FU + FD * FD : UP * FUT * CU2_ROW + FD;
    static constexpr int LDS_FLOATS = B::SZ_A + B::SZ_B + round_up(NCOEF, 4) + B::SGN_WORDS;
    static_assert(MODE == FLRELU_SUFD || MODE == FLRELU_FUSD, "mode");
    static_assert(MODE != FLRELU_SUFD || (DOWN % 2 == 0 && FD % 2 == 0 && TOH % R2 == 0 && TOW % 4 == 0), "SUFD item shape");
    static_assert(MODE != FLRELU_FUSD || (UP == 2 && FUT == 6 && TUHP % 4 == 0 && (TUWP / 8) % 2 == 0), "FUSD item shape");
    static_assert(MODE != FLRELU_FUSD || B::SZ_B >= TIH * TIWP, "FUSD stages the input tile in the second buffer");
    static_assert((2 * FU) % 4 == 0, "2-D down table must start on a 16-byte boundary");
    static_assert(LDS_FLOATS * 4 <= 160 * 1024, "LDS overflow");

    // ---- SUFD stage D': 2-D decimating FIR + store.  upXY rows DOWN * p0 + i, i < DOWN * (R2 - 1) + FD.
    static __device__ __forceinline__ void down_2d_store(const float* __restrict__ upXY, const float* __restrict__ cd2, int tid,
                                                         const FlreluParams& p, int plane, int O0x, int O0y) {
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        constexpr int NC4 = TOW / 4;
        constexpr int NROW = DOWN * (R2 - 1) + FD;
        constexpr int NIN4 = cdiv(DOWN * 3 + FD, 4);
        T* yp = (T*)p.y + (size_t)plane * p.yh * p.yw;
        for (int item = tid; item < NC4 * (TOH / R2); item += NT) {
            const int rbk = item / NC4, c4 = item - rbk * NC4;
            const int p0 = rbk * R2;
            f32x2 acc[R2][4];
#pragma unroll
            for (int t = 0; t < R2; t++)
#pragma unroll
                for (int o = 0; o < 4; o++) acc[t][o] = (f32x2){0.f, 0.f};
#pragma unroll 1
            for (int i = 0; i < NROW; i++) {                     // (rolled: unrolled, the compiler hoists every LDS read and spills)
                const float* src = upXY + (DOWN * p0 + i) * PU + DOWN * 4 * c4;
                float in[NIN4 * 4];
#pragma unroll
                for (int q = 0; q < NIN4; q++) {
                    const float4 v = *(const float4*)(src + 4 * q);
                    in[4 * q] = v.x; in[4 * q + 1] = v.y; in[4 * q + 2] = v.z; in[4 * q + 3] = v.w;
                }
#pragma unroll
                for (int t = 0; t < R2; t++) {
                    const int k = i - DOWN * t;
                    if (k >= 0 && k < FD) {
                        float c[FD];
#pragma unroll
                        for (int q = 0; q < FD / 4; q++) {
                            const float4 v = *(const float4*)(cd2 + k * FD + 4 * q);
                            c[4 * q] = v.x; c[4 * q + 1] = v.y; c[4 * q + 2] = v.z; c[4 * q + 3] = v.w;
                        }
#pragma unroll
                        for (int o = 0; o < 4; o++)
#pragma unroll
                            for (int k2 = 0; k2 < FD / 2; k2++)
                                acc[t][o] = __builtin_elementwise_fma((f32x2){c[2 * k2], c[2 * k2 + 1]},
                                                                      (f32x2){in[DOWN * o + 2 * k2], in[DOWN * o + 2 * k2 + 1]}, acc[t][o]);
                    }
                }
            }
            const int ox = O0x + 4 * c4;
#pragma unroll
            for (int t = 0; t < R2; t++) {
                const int oy = O0y + p0 + t;
                if (oy < p.yh) {
                    T* dst = yp + (size_t)oy * p.yw + ox;
                    float v[4];
#pragma unroll
                    for (int o = 0; o < 4; o++) v[o] = acc[t][o].x + acc[t][o].y;
                    if (sizeof(T) == 4 && ox + 3 < p.yw && (p.yw & 3) == 0) {
                        *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
                    } else {
#pragma unroll
                        for (int o = 0; o < 4; o++)
                            if (ox + o < p.yw) dst[o] = from_f32<T>(v[o]);
                    }
                }
            }
        }
    }

    // ---- FUSD stage B': 2-D polyphase up-FIR + gain + leaky ReLU + clamp + sign codes.  sIn -> upXY (pitch PU).
    template <int PHY>
    static __device__ __forceinline__ void up_2d_act(const float* __restrict__ sIn, float* __restrict__ upXY,
                                                     const float* __restrict__ cu2, const unsigned* __restrict__ sgn, int tid,
                                                     const FlreluParams& p, int plane, int U0x, int U0y, bool lastX, bool lastY) {
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        constexpr int MB2 = 2;                                   // input rows per item (4 upsampled rows)
        constexpr int NCH = TUWP / 8;                            // 4-input-column chunks per row (8 upsampled columns)
        constexpr int NRB = TUHP / (MB2 * UP);
        constexpr int NINR = MB2 + FUT;
        unsigned char* splane = p.s + (size_t)plane * p.sh * p.swb;
        for (int item = tid; item < NCH * NRB; item += NT) {
            const int rb = item / NCH, ch = item - rb * NCH;      // consecutive lanes -> consecutive chunks (lane pairs share a dword)
            f32x2 acc[MB2][UP][4];                              // (x phase 0, x phase 1) of input column mx, upsampled row (mm, ay)
#pragma unroll
            for (int mm = 0; mm < MB2; mm++)
#pragma unroll
                for (int ay = 0; ay < UP; ay++)
#pragma unroll
                    for (int mx = 0; mx < 4; mx++) acc[mm][ay][mx] = (f32x2){0.f, 0.f};
#pragma unroll 1
            for (int ri = 0; ri < NINR; ri++) {                  // (rolled, as in down_2d_store)
                const float* src = sIn + (rb * MB2 + ri) * TIWP + 4 * ch;
                float in[12];
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    const float4 v = *(const float4*)(src + 4 * q);
                    in[4 * q] = v.x; in[4 * q + 1] = v.y; in[4 * q + 2] = v.z; in[4 * q + 3] = v.w;
                }
#pragma unroll
                for (int mm = 0; mm < MB2; mm++)
#pragma unroll
                    for (int ay = 0; ay < UP; ay++) {
                        const int jy = ri - mm - ((ay > PHY) ? 1 : 0);
                        if (jy >= 0 && jy < FUT) {
                            f32x2 c[7];
                            const float* crow = cu2 + (ay * FUT + jy) * CU2_ROW;
#pragma unroll
                            for (int q = 0; q < 4; q++) {
                                const float4 v = *(const float4*)(crow + 4 * q);
                                if (2 * q < 7) c[2 * q] = (f32x2){v.x, v.y};
                                if (2 * q + 1 < 7) c[2 * q + 1] = (f32x2){v.z, v.w};
                            }
#pragma unroll
                            for (int mx = 0; mx < 4; mx++)
#pragma unroll
                                for (int t = 0; t < 7; t++)
                                    acc[mm][ay][mx] = __builtin_elementwise_fma(c[t], (f32x2){in[mx + t], in[mx + t]}, acc[mm][ay][mx]);
                        }
                    }
            }
            const int X = U0x + 8 * ch;
            const int sbit = (((U0x + p.sx) & 15) + 8 * ch) * 2;  // READ mode: bit offset of the chunk's 8 codes in the staged window
            const int sw0 = sbit >> 5, sshift = sbit & 31;
#pragma unroll
            for (int mm = 0; mm < MB2; mm++)
#pragma unroll
                for (int ay = 0; ay < UP; ay++) {
                    const int row = rb * MB2 * UP + mm * UP + ay;
                    const int Y = U0y + row;
                    unsigned codes = 0;
                    if (SIGN == AFCM_SIGNS_READ) {
                        const unsigned lo = sgn[row * SGN_W + sw0];
                        const unsigned hi = (sw0 + 1 < SGN_W) ? sgn[row * SGN_W + sw0 + 1] : 0u;
                        codes = __builtin_amdgcn_alignbit(hi, lo, sshift) & 0xffffu;
                    }
                    float v[8];
                    unsigned bits = 0;
#pragma unroll
                    for (int mx = 0; mx < 4; mx++) {
                        v[2 * mx] = acc[mm][ay][mx].x;
                        v[2 * mx + 1] = acc[mm][ay][mx].y;
                    }
#pragma unroll
                    for (int e = 0; e < 8; e++) bits |= act_elem<SIGN>(v[e], p.gain, p.slope, p.clamp, codes >> (2 * e)) << (2 * e);
                    float* dst = upXY + row * PU + 8 * ch;
                    *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
                    *(float4*)(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
                    if (SIGN == AFCM_SIGNS_WRITE) {
                        // 2 lanes of a pair hold 16 consecutive columns: assemble one dword
                        int word = (int)(bits << ((ch & 1) << 4));
                        word |= __builtin_amdgcn_mov_dpp(word, 0xB1, 0xF, 0xF, true);     // quad_perm [1,0,3,2]
                        const bool ownX = (8 * ch < TOW * DOWN) || lastX;
                        const bool ownY = (row < TOH * DOWN) || lastY;
                        if ((ch & 1) == 0 && ownX && ownY && (X >> 2) < p.swb && Y < p.sh)
                            *(int*)(splane + (size_t)Y * p.swb + (X >> 2)) = word;
                    }
                }
        }
    }
};

template <typename T, int MODE, int UP, int DOWN, int FUT, int FD, int TOW, int TOH, int RO, int NT, int SIGN>
__global__ __launch_bounds__(NT) void flrelu_radial_kernel(FlreluParams p, const float* __restrict__ fu,
                                                           const float* __restrict__ fd) {
    typedef FlreluRadialTile<T, MODE, UP, DOWN, FUT, FD, TOW, TOH, RO, NT, SIGN> K;
    FLRELU_TILE_PROLOGUE();

    // coefficient tables (flip_filter flips both axes of a 2-D filter: F2[ky][kx] = flip ? f[ky][kx] : f[n-1-ky][n-1-kx])
    if constexpr (MODE == FLRELU_SUFD) {
        float *cuX = coef, *cuY = coef + K::FU, *cd2 = coef + 2 * K::FU;
        if (tid < K::FU) {
            const int a = tid / FUT, j = tid - a * FUT;
            const int kx = ((a > phx) ? UP - (a - phx) : phx - a) + UP * j;
            const int ky = ((a > phy) ? UP - (a - phy) : phy - a) + UP * j;
            cuX[tid] = p.flip ? fu[kx] : fu[K::FU - 1 - kx];
            cuY[tid] = p.flip ? fu[ky] : fu[K::FU - 1 - ky];
        }
        for (int i = tid; i < FD * FD; i += NT) cd2[i] = p.flip ? fd[i] : fd[FD * FD - 1 - i];
    } else {
        float *cu2 = coef, *cdl = coef + UP * FUT * K::CU2_ROW;
        for (int i = tid; i < UP * FUT * K::CU2_ROW; i += NT) {
            const int row = i / K::CU2_ROW, e = i - row * K::CU2_ROW;
            const int ay = row / FUT, jy = row - ay * FUT;
            const int t = e >> 1, ax = e & 1;
            const int jx = t - ((ax > phx) ? 1 : 0);
            float v = 0.f;
            if (t < 7 && jx >= 0 && jx < FUT) {
                const int ky = ((ay > phy) ? UP - (ay - phy) : phy - ay) + UP * jy;
                const int kx = ((ax > phx) ? UP - (ax - phx) : phx - ax) + UP * jx;
                v = p.flip ? fu[ky * K::FU + kx] : fu[(K::FU - 1 - ky) * K::FU + (K::FU - 1 - kx)];
            }
            cu2[i] = v;
        }
        if (tid < FD) cdl[tid] = p.flip ? fd[tid] : fd[FD - 1 - tid];
    }

    float* sIn = MODE == FLRELU_FUSD ? bufB : bufA;     // FUSD: the 2-D up stage writes the activated tile to bufA
    FLRELU_TILE_STAGE_A(sIn);
    const bool lastX = (tx == p.tilesX - 1), lastY = (ty == p.tilesY - 1);
    if constexpr (MODE == FLRELU_SUFD) {
        const float *cuX = coef, *cuY = coef + K::FU;
        FLRELU_TILE_UP_X(cuX);
        FLRELU_TILE_UP_Y_ACT(cuY);
        K::down_2d_store(bufA, coef + 2 * K::FU, tid, p, plane, O0x, O0y);
    } else {
        const float *cu2 = coef, *cdl = coef + UP * FUT * K::CU2_ROW;
        if (phy == 0) K::template up_2d_act<0>(bufB, bufA, cu2, sgn, tid, p, plane, U0x, U0y, lastX, lastY);
        else K::template up_2d_act<1>(bufB, bufA, cu2, sgn, tid, p, plane, U0x, U0y, lastX, lastY);
        __syncthreads();
        K::down_x(bufA, bufB, cdl, tid);
        __syncthreads();
        K::down_y_store(bufB, cdl, tid, p, plane, O0x, O0y);
    }
}

// ---------------------------------------------------------------------------------------------
// The plan's row of kTileShapes -> template arguments (6 taps per polyphase branch, 384 threads in every shape)
template <typename T, int I = 0>
static int launch_tile(const afcm_filtered_lrelu_args* a, const FlreluPlan& pl, const FlreluParams& p, hipStream_t st) {
    if constexpr (I < sizeof(kTileShapes) / sizeof(kTileShapes[0])) {
        if (pl.shape != I) return launch_tile<T, I + 1>(a, pl, p, st);
        constexpr FlreluTileShape S = kTileShapes[I];
        constexpr int MODE = S.family - FLRELU_FAMILY_TILE_SEP, FUT = 6, FD = FUT * S.down, NT = 384;
        const long long blocks = (long long)p.tilesX * p.tilesY * a->n * a->c;
        AFCM_REQUIRE(blocks > 0 && blocks < (1ll << 31), "filtered_lrelu: grid of %lld blocks is out of range", blocks);
        dim3 grid((unsigned)blocks), block(NT);
        with_sign_mode(a->sign_mode, [&](auto sign) {
            constexpr int SIGN = decltype(sign)::value;
            if constexpr (MODE == FLRELU_SEP) hipLaunchKernelGGL((flrelu_sep_kernel<T, S.up, S.down, FUT, FD, S.tow, S.toh, S.ro, NT, SIGN>), grid, block, 0, st, p, a->fu, a->fd);
            else hipLaunchKernelGGL((flrelu_radial_kernel<T, MODE, S.up, S.down, FUT, FD, S.tow, S.toh, S.ro, NT, SIGN>), grid, block, 0, st, p, a->fu, a->fd);
        });
        return hip_status(hipGetLastError());
    }
    return AFCM_E_NOKERNEL;
}

int flrelu_launch_tile(const afcm_filtered_lrelu_args* a, const FlreluPlan& pl, const FlreluParams& p, hipStream_t st) {
    return with_dtype(a->dtype, [&](auto t) { return launch_tile<decltype(t)>(a, pl, p, st); });
}

}  // namespace afcm
