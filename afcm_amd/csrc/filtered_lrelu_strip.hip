// fp32 strip kernel of filtered_lrelu (r03; separable filters, planes below 2^30 elements).  Sign codes use layout 0.
// One WAVE owns a strip of SW output columns x SH output rows of one plane and marches down it one input
// row per step, with every intermediate in registers or in the wave's own 1-3 KB of LDS -- no workgroup barrier, no tile halo in y
// (the tile kernel of filtered_lrelu_tile.hip recomputes (FD - DOWN) upsampled rows per 20-row tile, 1.55x the useful FMAs at up 2 / down 2 and 4.4x at
// down 4), and an instruction stream close to the arithmetic: profiles/r03_flrelu_fp32_pmc.txt has the tile kernel 75 % VALU-issue-
// bound at 289 vector operations per output where the four FIR passes need 47 packed FMAs.
//   lane l <-> input columns I0x + l, I0x + 64 + l (CPL column blocks).  Per step (input row I0y + it):
//     up-x   the row goes through LDS so that a lane sees its 6 right neighbours: UP upsampled columns per lane, 7 taps each (the
//            phase-dependent one-column offset o(a) of the polyphase form is folded into a 7-tap table with one zero: no selects)
//     up-y   a ring of the last 6 up-x rows in registers (static indices: the step loop is unrolled over the ring period) + the new
//            row -> UP upsampled rows x UP columns, 7 taps each; gain, leaky ReLU, clamp, 2-bit codes (written as whole dwords by
//            the first lane of each 16-column group after a DPP OR-reduction; READ: the row's sign dwords are fetched one step ahead
//            by the first lanes and spread through LDS)
//     down-x the UP activated rows go through LDS; lane j reads the FD taps of output column j (8-byte reads, even / odd taps in the
//            two halves of packed FMAs)
//     down-y scatter form: each new down-x row adds into the FD / DOWN output rows it contributes to (a ring of 6 accumulators,
//            static indices); the accumulator that received its last tap is stored and reset.
//   Signs: a strip owns the SW DOWN upsampled columns of its outputs (a multiple of 16: whole dwords), a segment the SH DOWN rows of
//   its outputs, the last strip / segment the rest.  The last 6 columns have no full tap support: they compute on zero padding, own nothing.
#include "flrelu_common.h"

namespace afcm {

template <int LO, int HI, typename F>
__device__ __forceinline__ void strip_static_for(F&& f) {
    if constexpr (LO < HI) {
        f(std::integral_constant<int, LO>{});
        strip_static_for<LO + 1, HI>(f);
    }
}

template <int UP, int DOWN, int CPL_, int SIGN_>
struct StripGeom {
    static constexpr int FUT = 6, FU = FUT * UP, FD = FUT * DOWN;
    // CPL input columns per lane, in blocks: lane l holds columns l, 64 + l, ... of the strip's 64 CPL (coalesced row loads; the up
    // stages run once per block, the right halo -- 6 columns -- is paid once per strip: 87.5 % of the columns useful at CPL 2, 75 % at 1)
    // The host picks CPL per configuration: 1 for up 2 / down 2 (48-column strips quantise the generator's plane widths better than
    // 112-column ones: enc3 forward 0.91 vs 1.06 ms) and up 4 (registers), 2 for down 4 (56 output lanes instead of 24: 1.26 vs 1.68 ms)
    static constexpr int CPL = CPL_;
    static constexpr int NC = 64 * CPL;                         // input columns of the strip
    static constexpr int SWMAX = (UP * (NC - 6) - FD) / DOWN + 1;                           // outputs with full tap support
    static constexpr int SW = SIGN_ == AFCM_SIGNS_WRITE ? SWMAX / (16 / DOWN) * (16 / DOWN) : SWMAX;   // sign writers: whole dwords per strip
    static constexpr int NU = NC * UP;                          // upsampled columns per row of the strip
    static constexpr int OPL = cdiv(SW, 64);                    // output columns per lane
    static constexpr int PERIOD = (UP == 2 && DOWN == 4) ? 12 : 6;   // steps after which the up-y ring AND the down-y ring repeat
    static constexpr int GS = 16 / UP;                          // lanes per sign dword
    static constexpr int NW = NU / 16 + 1;                      // sign dwords a row's window can touch (READ)
    static_assert(SIGN_ != AFCM_SIGNS_WRITE || (SW * DOWN) % 16 == 0, "sign ownership must fall on dword boundaries");
    static_assert(DOWN * (SW - 1) + FD <= UP * (NC - 6), "the strip's outputs must stay inside the columns with full tap support");
    static_assert((UP * PERIOD) % (DOWN * 6) == 0 && PERIOD % 6 == 0, "ring periods");
    static_assert(NW <= 64, "one lane per sign dword");
};

template <typename T, int UP, int DOWN, int CPL_, int SIGN, bool FASTACT>
__global__ __launch_bounds__(256) void flrelu_strip_kernel(FlreluParams p, const float* __restrict__ fu, const float* __restrict__ fd) {
    typedef StripGeom<UP, DOWN, CPL_, SIGN> G;
    constexpr int FUT = G::FUT, FU = G::FU, FD = G::FD, SW = G::SW, NU = G::NU, NC = G::NC, CPL = G::CPL, OPL = G::OPL, PERIOD = G::PERIOD, GS = G::GS, NW = G::NW;
    __shared__ float s_in[4][NC + 8];                            // input row of the wave + zero pad for the neighbours of the last 6 columns
    __shared__ __attribute__((aligned(16))) float s_u[4][UP][NU];   // the UP activated rows of a step
    __shared__ unsigned s_sg[4][UP][NW + 1];                     // READ: sign dwords of the step's rows

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int SH = cdiv(p.yh, p.tilesY);
    int wt = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);
    if (wt >= p.tilesX * p.tilesY * p.planes) return;
    const int tx = wt % p.tilesX; wt /= p.tilesX;
    const int ty = wt % p.tilesY;
    const int plane = wt / p.tilesY;
    const bool lastX = tx == p.tilesX - 1, lastY = ty == p.tilesY - 1;
    const int O0x = tx * SW, O0y = ty * SH;
    const int U0x = O0x * DOWN, U0y = O0y * DOWN;
    const int I0x = -floor_div(p.px0 - U0x, UP), phx = pos_mod(p.px0 - U0x, UP);
    const int I0y = -floor_div(p.py0 - U0y, UP), phy = pos_mod(p.py0 - U0y, UP);

    // 7-tap polyphase tables (uniform: scalar registers): c7[a][t] multiplies row / column (first + t), t = 0..6
    float cx7[UP][7], cy7[UP][7], cd[FD];
#pragma unroll
    for (int a = 0; a < UP; a++) {
        const int ox = (a > phx) ? 1 : 0, oy = (a > phy) ? 1 : 0;
        const int kx = ox ? UP - (a - phx) : phx - a, ky = oy ? UP - (a - phy) : phy - a;
#pragma unroll
        for (int t = 0; t < 7; t++) {
            const int jx = t - ox, jy = t - oy;
            const int ix = kx + UP * (jx < 0 ? 0 : jx > 5 ? 5 : jx), iy = ky + UP * (jy < 0 ? 0 : jy > 5 ? 5 : jy);
            const float vx = p.flip ? fu[ix] : fu[FU - 1 - ix], vy = p.flip ? fu[iy] : fu[FU - 1 - iy];
            cx7[a][t] = (jx >= 0 && jx < FUT) ? vx : 0.f;
            cy7[a][t] = (jy >= 0 && jy < FUT) ? vy : 0.f;
        }
    }
#pragma unroll
    for (int k = 0; k < FD; k++) cd[k] = p.flip ? fd[k] : fd[FD - 1 - k];
    // the up-x taps as (a, a + 1) pairs in VECTOR registers: with all three tables in the scalar file it overflows (the compiler parked
    // taps in VGPR lanes and read them back every step: 11 of 117 vector instructions per step); pairs keep the packed FMAs
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    f32x2 cxp[UP / 2][7];
#pragma unroll
    for (int a2 = 0; a2 < UP / 2; a2++)
#pragma unroll
        for (int t = 0; t < 7; t++) {
            cxp[a2][t] = (f32x2){cx7[2 * a2][t], cx7[2 * a2 + 1][t]};
            asm volatile("" : "+v"(cxp[a2][t]));
        }

    float* const in_row = s_in[wave];
    if (lane < 8) in_row[NC + lane] = 0.f;
    if (SIGN == AFCM_SIGNS_READ && lane < UP) s_sg[wave][lane][NW] = 0u;
    const T* const xp = (const T*)p.x + (size_t)plane * p.xh * p.xw;
    T* const yp = (T*)p.y + (size_t)plane * p.yh * p.yw;
    unsigned char* const splane = p.s + (size_t)plane * p.sh * p.swb;
    const float bias = p.b ? to_f32(((const T*)p.b)[plane % p.C]) : 0.f;     // added inside the image only (the padding is zero)

    // rows this wave has to walk: the last tap of its last output row, in WRITE mode of the last segment also the last sign row
    const int SHv = min(SH, p.yh - O0y);
    int qmax = DOWN * (SHv - 1) + FD - 1;
    if (SIGN == AFCM_SIGNS_WRITE && lastY) qmax = max(qmax, p.sh - 1 - U0y);
    const int NIT = qmax / UP + 7;

    // READ: dword window of a sign row and this lane's bit offset inside it (column block c: + 128 UP bits)
    const int w0 = floor_div(U0x + p.sx, 16);
    const int sbit = pos_mod(U0x + p.sx, 16) * 2 + 2 * UP * lane;
    const int wpr = p.swb >> 2;
    auto fetch_signs = [&](int it, unsigned (&sg)[UP]) __attribute__((always_inline)) {
#pragma unroll
        for (int a = 0; a < UP; a++) {
            const int Y = U0y + UP * (it - 6) + a + p.sy, wi = w0 + lane;
            const bool ok = lane < NW && (unsigned)Y < (unsigned)p.sh && (unsigned)wi < (unsigned)wpr;
            sg[a] = ok ? ((const unsigned*)(splane + (size_t)(ok ? Y : 0) * p.swb))[ok ? wi : 0] : 0u;
        }
    };
    // the row is requested one step before its use: clamped address (no branch around the load, nothing waits on it here); validity and
    // the bias are applied when the value is consumed
    bool colok[CPL];
    int colx[CPL];
#pragma unroll
    for (int c = 0; c < CPL; c++) {
        const int ix = I0x + 64 * c + lane;
        colok[c] = (unsigned)ix < (unsigned)p.xw;
        colx[c] = min(max(ix, 0), p.xw - 1);
    }
    auto fetch_input = [&](int it, T (&xv)[CPL]) __attribute__((always_inline)) {
        const int iy = min(max(I0y + it, 0), p.xh - 1);
        const T* row = xp + (size_t)iy * p.xw;
#pragma unroll
        for (int c = 0; c < CPL; c++) xv[c] = row[colx[c]];
    };

    f32x2 ring[6][CPL][UP / 2];                                  // up-x rows: (a, a + 1) column pairs
#pragma unroll
    for (int j = 0; j < 6; j++)
#pragma unroll
        for (int c = 0; c < CPL; c++)
#pragma unroll
            for (int a2 = 0; a2 < UP / 2; a2++) ring[j][c][a2] = (f32x2){0.f, 0.f};
    float acc[6][OPL];
#pragma unroll
    for (int j = 0; j < 6; j++)
#pragma unroll
        for (int o = 0; o < OPL; o++) acc[j][o] = 0.f;

    T xnext[CPL];
    fetch_input(0, xnext);
    unsigned sgnext[UP];
#pragma unroll
    for (int a = 0; a < UP; a++) sgnext[a] = 0u;
    if (SIGN == AFCM_SIGNS_READ) fetch_signs(6, sgnext);

    for (int base = 0; base < NIT; base += PERIOD) {
        strip_static_for<0, PERIOD>([&](auto phc) __attribute__((always_inline)) {
            constexpr int ph = decltype(phc)::value;
            const int it = base + ph;
            if (it < NIT) {
                // ---- up-x
                float xin[CPL];
                const bool rowok = (unsigned)(I0y + it) < (unsigned)p.xh;
#pragma unroll
                for (int c = 0; c < CPL; c++) xin[c] = (rowok && colok[c]) ? to_f32(xnext[c]) + bias : 0.f;
                fetch_input(it + 1, xnext);
#pragma unroll
                for (int c = 0; c < CPL; c++) in_row[64 * c + lane] = xin[c];
                __builtin_amdgcn_wave_barrier();
                f32x2 R[CPL][UP / 2];
#pragma unroll
                for (int c = 0; c < CPL; c++) {
                    float nb[7];
                    nb[0] = xin[c];
#pragma unroll
                    for (int t = 1; t < 7; t++) nb[t] = in_row[64 * c + lane + t];
#pragma unroll
                    for (int a2 = 0; a2 < UP / 2; a2++) {
                        f32x2 s0 = (f32x2){0.f, 0.f};
#pragma unroll
                        for (int t = 0; t < 7; t++) s0 = __builtin_elementwise_fma(cxp[a2][t], (f32x2){nb[t], nb[t]}, s0);
                        R[c][a2] = s0;
                    }
                }
                __builtin_amdgcn_wave_barrier();
                if (it >= 6) {
                    // ---- up-y: rows m + t, t = 0..5 in ring[(ph + t) % 6], row m + 6 = R;  m = it - 6
                    if (SIGN == AFCM_SIGNS_READ) {
                        unsigned sg[UP];
#pragma unroll
                        for (int a = 0; a < UP; a++) sg[a] = sgnext[a];
                        fetch_signs(it + 1, sgnext);
#pragma unroll
                        for (int a = 0; a < UP; a++)
                            if (lane < NW) s_sg[wave][a][lane] = sg[a];
                        __builtin_amdgcn_wave_barrier();
                    }
                    const int q0 = UP * (it - 6);                 // first upsampled row of the step, relative to U0y
#pragma unroll
                    for (int ay = 0; ay < UP; ay++) {
#pragma unroll
                        for (int c = 0; c < CPL; c++) {
                            float v[UP];
#pragma unroll
                            for (int a2 = 0; a2 < UP / 2; a2++) {
                                f32x2 s0 = (f32x2){0.f, 0.f};
#pragma unroll
                                for (int t = 0; t < 6; t++) s0 = __builtin_elementwise_fma((f32x2){cy7[ay][t], cy7[ay][t]}, ring[(ph + t) % 6][c][a2], s0);
                                s0 = __builtin_elementwise_fma((f32x2){cy7[ay][6], cy7[ay][6]}, R[c][a2], s0);
                                v[2 * a2] = s0.x;
                                v[2 * a2 + 1] = s0.y;
                            }
                            unsigned codes = 0u;
                            if (SIGN == AFCM_SIGNS_READ) {
                                const int sb = sbit + 128 * UP * c;
                                const unsigned lo = s_sg[wave][ay][sb >> 5], hi = s_sg[wave][ay][(sb >> 5) + 1];
                                codes = __builtin_amdgcn_alignbit(hi, lo, sb & 31);
                            }
                            unsigned nib = 0u;
                            if (SIGN != AFCM_SIGNS_READ && FASTACT) {
                                // 0 <= slope <= 1: leaky ReLU = max(v, slope v); the clamp is a select on the compare the code needs anyway
                                // (NOT a med3: v_med3_f32 turns a NaN into -clamp, act_elem and the reference kernel hand it on) -- the
                                // same values as act_elem bit for bit, NaN included, one instruction fewer per element
#pragma unroll
                                for (int a2 = 0; a2 < UP / 2; a2++) {
                                    const f32x2 g2 = (f32x2){v[2 * a2], v[2 * a2 + 1]} * (f32x2){p.gain, p.gain};
                                    const f32x2 t2 = g2 * (f32x2){p.slope, p.slope};
#pragma unroll
                                    for (int e = 0; e < 2; e++) {
                                        const int ax = 2 * a2 + e;
                                        const float w = fmaxf(g2[e], t2[e]);
                                        unsigned code = __float_as_uint(g2[e]) >> 31;
                                        const bool big = fabsf(w) > p.clamp;            // (false for a NaN)
                                        if (big) code = 2u;
                                        v[ax] = big ? __builtin_copysignf(p.clamp, w) : w;
                                        nib |= code << (2 * ax);
                                    }
                                }
                            } else {
#pragma unroll
                                for (int ax = 0; ax < UP; ax++) nib |= act_elem<SIGN>(v[ax], p.gain, p.slope, p.clamp, codes >> (2 * ax)) << (2 * ax);
                            }
                            if (SIGN == AFCM_SIGNS_WRITE) {
                                int word = (int)(nib << ((lane % GS) * 2 * UP));
                                word |= __builtin_amdgcn_mov_dpp(word, 0xB1, 0xF, 0xF, true);              // quad_perm [1,0,3,2]
                                word |= __builtin_amdgcn_mov_dpp(word, 0x4E, 0xF, 0xF, true);              // quad_perm [2,3,0,1]
                                if (GS == 8) word |= __builtin_amdgcn_mov_dpp(word, 0x141, 0xF, 0xF, true);   // row_half_mirror
                                const int col = 64 * c + lane;
                                const int q = q0 + ay, Y = U0y + q, X0 = U0x + UP * col;
                                const bool own = ((UP * col < SW * DOWN) || lastX) && ((q < SH * DOWN) || lastY);
                                if ((lane % GS) == 0 && col + GS <= NC - 6 && own && (X0 >> 2) < p.swb && Y < p.sh)
                                    *(int*)(splane + (size_t)Y * p.swb + (X0 >> 2)) = word;
                            }
                            if constexpr (UP == 2) *(float2*)(&s_u[wave][ay][UP * (64 * c + lane)]) = make_float2(v[0], v[1]);
                            else *(float4*)(&s_u[wave][ay][UP * (64 * c + lane)]) = make_float4(v[0], v[1], v[2], v[3]);
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                    // ---- down-x and down-y
#pragma unroll
                    for (int ay = 0; ay < UP; ay++) {
                        constexpr int QS_BASE = ((UP * (ph - 6)) % (DOWN * 6) + DOWN * 6) % (DOWN * 6);
                        const int qs = (QS_BASE + ay) % (DOWN * 6);       // the row's index modulo the down-y period (compile time after unrolling)
                        float d[OPL];
#pragma unroll
                        for (int o = 0; o < OPL; o++) {
                            const int j = min(lane + 64 * o, SW - 1);
                            const f32x2* src = (const f32x2*)(&s_u[wave][ay][DOWN * j]);
                            f32x2 e2 = (f32x2){0.f, 0.f};                   // even / odd taps in the two halves
#pragma unroll
                            for (int k2 = 0; k2 < FD / 2; k2++) e2 = __builtin_elementwise_fma((f32x2){cd[2 * k2], cd[2 * k2 + 1]}, src[k2], e2);
                            d[o] = e2.x + e2.y;
                        }
#pragma unroll
                        for (int i = 0; i < 6; i++) {
                            const int slot = ((qs / DOWN - i) % 6 + 6) % 6, k = qs % DOWN + DOWN * i;
#pragma unroll
                            for (int o = 0; o < OPL; o++) acc[slot][o] = fmaf(cd[k], d[o], acc[slot][o]);
                        }
                        if (qs % DOWN == DOWN - 1) {
                            const int slot = ((qs / DOWN - 5) % 6 + 6) % 6;
                            const int pr = (q0 + ay - (FD - 1)) / DOWN;     // exact: q - (FD - 1) is a multiple of DOWN here
                            if (q0 + ay >= FD - 1 && pr < SHv) {
#pragma unroll
                                for (int o = 0; o < OPL; o++) {
                                    const int j = lane + 64 * o;
                                    if (j < SW && O0x + j < p.yw) yp[(size_t)(O0y + pr) * p.yw + O0x + j] = from_f32<T>(acc[slot][o]);
                                }
                            }
#pragma unroll
                            for (int o = 0; o < OPL; o++) acc[slot][o] = 0.f;
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                }
                // the new up-x row replaces the oldest one
#pragma unroll
                for (int c = 0; c < CPL; c++)
#pragma unroll
                    for (int a2 = 0; a2 < UP / 2; a2++) ring[ph % 6][c][a2] = R[c][a2];
            }
        });
    }
}

// ---------------------------------------------------------------------------------------------
template <int UP, int DOWN>
constexpr int kStripCPL = DOWN == 4 ? 2 : 1;                    // CPL by configuration (see StripGeom)

int flrelu_strip_columns(int up, int down, int sign_mode) {
    return with_up_down(up, down, [&](auto u, auto d) {
        constexpr int UP = decltype(u)::value, DOWN = decltype(d)::value, CPL = kStripCPL<UP, DOWN>;
        return sign_mode == AFCM_SIGNS_WRITE ? StripGeom<UP, DOWN, CPL, AFCM_SIGNS_WRITE>::SW : StripGeom<UP, DOWN, CPL, AFCM_SIGNS_NONE>::SW;
    });
}

template <int UP, int DOWN>
static int launch_strip(const afcm_filtered_lrelu_args* a, const FlreluParams& p, hipStream_t st) {
    constexpr int CPL = kStripCPL<UP, DOWN>;
    const long long waves = (long long)p.tilesX * p.tilesY * p.planes;
    AFCM_REQUIRE(waves > 0 && waves < (1ll << 31), "filtered_lrelu: grid of %lld waves is out of range", waves);
    dim3 grid((unsigned)((waves + 3) / 4)), block(256);
    const bool fast = a->slope >= 0.f && a->slope <= 1.f && a->clamp >= 0.f;     // (NaN fails every comparison: general form)
    with_sign_mode(a->sign_mode, [&](auto sign) {
        constexpr int SIGN = decltype(sign)::value;
        constexpr bool FAST = SIGN != AFCM_SIGNS_READ;       // (the sign-reading form only applies the codes: one kernel)
        if (fast) hipLaunchKernelGGL((flrelu_strip_kernel<float, UP, DOWN, CPL, SIGN, FAST>), grid, block, 0, st, p, a->fu, a->fd);
        else hipLaunchKernelGGL((flrelu_strip_kernel<float, UP, DOWN, CPL, SIGN, false>), grid, block, 0, st, p, a->fu, a->fd);
    });
    return hip_status(hipGetLastError());
}

int flrelu_launch_strip(const afcm_filtered_lrelu_args* a, const FlreluPlan& pl, const FlreluParams& p, hipStream_t st) {
    return with_up_down(pl.up, pl.down, [&](auto u, auto d) { return launch_strip<decltype(u)::value, decltype(d)::value>(a, p, st); });
}

}  // namespace afcm
