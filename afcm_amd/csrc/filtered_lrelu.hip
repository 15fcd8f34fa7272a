// filtered_lrelu for gfx950 (MI355X): bias -> zero-insert upsample -> pad/crop -> separable FIR(fu)
// -> * up^2 * gain -> leaky ReLU -> clamp (+ 2-bit sign codes) -> separable FIR(fd) -> decimate, fused in
// one kernel so the up^2-times-larger intermediate never leaves the CU.
//
// Semantics follow the reference op (SG3OPS/filtered_lrelu.py:121-153; edge rules of
// SG3OPS/filtered_lrelu.cu:264-297, 484-505, 564-571).  This unit holds the C entry points, the host plan
// that picks the kernel of a call (flrelu_plan) and the pointwise kernel; the other kernels live in one unit
// per family (flrelu_common.h lists them).
#include <stdlib.h>
#include "flrelu_common.h"

namespace afcm {

// ---------------------------------------------------------------------------------------------
// Pointwise form: up = down = 1 with 1x1 filters (the ToRGB layer, NET:369-372) and the in-place
// activation of the generic fallback (filtered_lrelu_act_, filtered_lrelu.cu:1105-1211).
// One thread = 16 consecutive columns of one row = one sign dword.
template <typename T, int SIGN>
__global__ __launch_bounds__(256) void flrelu_pointwise_kernel(FlreluParams p) {
    const int chunks = (p.yw + 15) >> 4;
    const long long total = (long long)p.tilesY * p.yh * chunks;  // tilesY = planes here
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int ch = (int)(idx % chunks);
        const long long t = idx / chunks;
        const int oy = (int)(t % p.yh);
        const int plane = (int)(t / p.yh);
        const T* xp = (const T*)p.x + (size_t)plane * p.xh * p.xw;
        T* yp = (T*)p.y + (size_t)plane * p.yh * p.yw;
        const float bias = p.b ? to_f32(((const T*)p.b)[plane % p.C]) : 0.f;
        const int iy = oy - p.py0;
        const bool rowIn = (unsigned)iy < (unsigned)p.xh;
        unsigned char* splane = (SIGN != AFCM_SIGNS_NONE) ? p.s + (size_t)plane * p.sh * p.swb : nullptr;
        unsigned word = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int ox0 = ch * 16 + q * 4;
            unsigned codes = 0;
            if (SIGN == AFCM_SIGNS_READ) codes = fetch_codes4(splane, ox0 + p.sx, oy + p.sy, p.sh, p.swb);
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int ox = ox0 + e;
                const int ix = ox - p.px0;
                float v = 0.f;
                if (ox < p.yw && rowIn && (unsigned)ix < (unsigned)p.xw) v = (to_f32(xp[(size_t)iy * p.xw + ix]) + bias) * p.fscale;
                unsigned code = act_elem<SIGN>(v, p.gain, p.slope, p.clamp, codes >> (2 * e));
                word |= code << (2 * (q * 4 + e));
                if (ox < p.yw) yp[(size_t)oy * p.yw + ox] = from_f32<T>(v);
            }
        }
        if (SIGN == AFCM_SIGNS_WRITE && oy < p.sh && ch * 4 < p.swb) *(unsigned*)(splane + (size_t)oy * p.swb + ch * 4) = word;
    }
}

static int launch_pointwise(int dtype, FlreluParams p, int planes, int sign_mode, hipStream_t st) {
    p.tilesY = planes;
    const long long items = (long long)planes * p.yh * ((p.yw + 15) >> 4);
    long long blocks = (items + 255) / 256;
    blocks = blocks > 256 * 32 ? 256 * 32 : blocks < 1 ? 1 : blocks;
    dim3 grid((unsigned)blocks), block(256);
    return with_dtype(dtype, [&](auto t) {
        with_sign_mode(sign_mode, [&](auto sign) { hipLaunchKernelGGL((flrelu_pointwise_kernel<decltype(t), decltype(sign)::value>), grid, block, 0, st, p); });
        return hip_status(hipGetLastError());
    });
}

// ---------------------------------------------------------------------------------------------
// The plan (flrelu_common.h).  Reads a->yw / a->yh as afcm_filtered_lrelu_shapes() computes them; every threshold of the
// family's kernel selection is here and nowhere else.
FlreluPlan flrelu_plan(const afcm_filtered_lrelu_args* a) {
    FlreluPlan pl = {};
    pl.family = FLRELU_FAMILY_NONE;
    pl.up = a->up;
    pl.down = a->down;
    const bool sep = a->fuh == 0 && a->fdh == 0;
    const bool sufd = a->fuh == 0 && a->fdh != 0, fusd = a->fuh != 0 && a->fdh == 0;
    // the three resampling cases of the model: (up, down) with 6 taps per polyphase branch of fu and of fd
    const bool c22 = a->up == 2 && a->down == 2 && a->fuw == 12 && a->fdw == 12;
    const bool c24 = a->up == 2 && a->down == 4 && a->fuw == 12 && a->fdw == 24;
    const bool c42 = a->up == 4 && a->down == 2 && a->fuw == 24 && a->fdw == 12;

    // ---- matrix-core kernels: 16-bit, separable, a prepared workspace, even plane widths (staged loads and stores move aligned
    // 16-bit pairs).  The output width is formed from the arguments: afcm_filtered_lrelu_prepare() plans without a->yw.
    const auto yw_args = [&] { return ((long long)a->xw * a->up + a->px0 + a->px1 - (a->fuw - 1) - (a->fdw - 1) + (a->down - 1)) / a->down; };
    if (a->workspace != nullptr && (a->dtype == AFCM_BF16 || a->dtype == AFCM_F16) && sep && (c22 || c24 || c42) && !(a->xw & 1) && !(yw_args() & 1)) {
        // The wave-autonomous kernels take every matrix-core case without a bias operand; they write / read sign layout 2, the
        // LDS-tile kernels layout 1, so a READ call follows the layout of its tensor.  Otherwise: no bias operand; offsets +
        // out-of-range markers stay below 2^31.  Decided on the plane sizes plus the largest pitch overhead the wave launch
        // accepts -- NOT on the pitches themselves: afcm_filtered_lrelu_shapes() runs before the caller has chosen them.
        const bool wave = a->sign_mode == AFCM_SIGNS_READ
                              ? a->sign_layout == 2
                              : a->b == nullptr && (long long)a->xh * (a->xw + kWavePitchSlack) < (1ll << 28) &&
                                    (long long)a->yh * (a->yw + kWavePitchSlack) < (1ll << 28);
        pl.family = wave ? FLRELU_FAMILY_WAVE : FLRELU_FAMILY_MFMA_TILE;
        pl.tow = a->down == 4 ? MfmaTile<2, 4>::TOW : MfmaTile<2, 2>::TOW;
        pl.toh = 32;
        if (wave) {
            // READ calls: output rows by which the strips' origin moves up (oy0 <= 0) so that every strip's first upsampled row,
            // U0y + sy = (ty TOH + oy0) down + sy, is a multiple of 16 = a row block of the sign tensor (kSignsReadAligned in
            // filtered_lrelu_wave.hip).  Possible when sy is a multiple of gcd(down, 16) = down; costs at most 16 / down - 1 extra
            // rows on top of the plane.  Where sy is not a multiple of `down`, the remaining dshift = (oy0 down + sy) mod 16 < down
            // upsampled rows are those by which the strips' upsampled grid itself starts early: the constant fragments of such a
            // call are prepared with their rows moved by dshift (the tiles have 6-12 spare rows: (TOH - 1) down + taps + dshift
            // <= 16 NVB for every shape), so EVERY read call is aligned.
            if (a->sign_mode == AFCM_SIGNS_READ) {
                const int m = pos_mod(a->sy, 16);
                pl.oy0 = -(m / a->down);
                pl.dshift = m % a->down;
            }
            // Output rows per strip: 32; one 48-row strip for the 36^2 / 38^2 planes (up 2 / down 2).  (Measured and dropped:
            // 16-row strips for down 4, whose 32-row strips need 240-250 registers = two waves per SIMD: at 16 rows a strip still
            // needs 176-199 and computes 1.5x instead of 1.25x its own rows -- forward 1.63 vs 1.89 TB/s over the down-4 layers.)
            const int rows = a->yh - pl.oy0;                  // rows the strips have to cover
            if (c22 && rows > 32 && rows <= kTallTOH) pl.toh = kTallTOH;
        } else if (a->up == 2) {
            // The sign-WRITING kernels (forward) also gain on larger planes whenever 48-row tiles cover the plane with no more
            // padded rows than 32-row tiles (276 rows: 6 x 48 = 9 x 32; 84 rows: 2 x 48 = 3 x 32): 7 % fewer halo rows, a third
            // fewer workgroups -- enc0..3 forward 0.207 / 0.277 / 0.383 -> 0.181 / 0.250 / 0.337 ms.  The sign-READING kernels
            // lose 5-20 % on the same tiles (their staged sign window and keep-mask table scale with the tile), so the transposed
            // op keeps 32 rows.  Up to 7 % more padded rows still pay (the 532- and 512-row planes of the 512^2 generator: 576 vs
            // 544, 528 vs 512 rows -- filtered_lrelu 10.0 -> 9.8 ms per step there); at 12.5 % (256 rows) the gain is gone.
            constexpr int slack = 7;                      // extra padded rows tolerated, in percent
            if ((a->yh > 32 && a->yh <= kTallTOH) ||
                (a->sign_mode != AFCM_SIGNS_READ && 100 * cdiv(a->yh, kTallTOH) * kTallTOH <= (100 + slack) * cdiv(a->yh, 32) * 32))
                pl.toh = kTallTOH;
        }
        pl.tilesX = wave ? 1 : cdiv(a->yw, pl.tow);           // one strip spans the plane's width
        pl.tilesY = cdiv(a->yh - pl.oy0, pl.toh);
        pl.sign_layout = wave ? 2 : 1;
        pl.row_pitch_ok = wave ? 1 : 0;       // the wave kernels address rows by pitch, the LDS-tile kernels take dense tensors
        pl.plane_sum_slots = pl.tilesX * pl.tilesY;
        return pl;
    }

    // ---- 1x1 filters, no resampling: pointwise kernel
    if (a->up == 1 && a->down == 1 && a->fuw == 1 && a->fdw == 1 && a->fuh <= 1 && a->fdh <= 1) {
        pl.family = FLRELU_FAMILY_POINTWISE;
        return pl;
    }

    // ---- fp32: the strip kernel, for planes below 2^30 elements
    const int strip_cols = (c22 || c24 || c42) ? flrelu_strip_columns(a->up, a->down, a->sign_mode) : 0;
    if (a->dtype == AFCM_F32 && sep && strip_cols > 0 && (long long)a->xw * a->xh < (1ll << 30) && (long long)a->yw * a->yh < (1ll << 30)) {
        pl.family = FLRELU_FAMILY_STRIP;
        pl.tow = strip_cols;
        pl.toh = 96;                          // output rows per segment (profiles/r03_flrelu_fp32_strip_rows_sweep.txt)
        pl.tilesX = cdiv(a->yw, pl.tow);
        pl.tilesY = a->yh <= pl.toh ? 1 : (a->yh + pl.toh / 2) / pl.toh;
        return pl;
    }

    // ---- exact LDS tile.  What is left for it: 16-bit calls without a matrix-core case (odd widths, no workspace), fp32 planes
    // of >= 2^30 elements, and the radial layers in every dtype.
    int family = FLRELU_FAMILY_NONE, tow = 64, toh = 20;
    if (sep && c22) {
        // Tile height by mode (measured, fp32, batch 16): the sign-writing forward runs 10 % faster on 20-row tiles (53 KB of LDS:
        // three workgroups per CU instead of two cover its five LDS stages), the sign-reading backward 12 % slower (its staged sign
        // window grows with the halo); planes of <= 40 rows take the 20-row tile both ways (36 rows: 40 computed instead of 70).
        family = FLRELU_FAMILY_TILE_SEP;
        toh = (a->sign_mode != AFCM_SIGNS_READ || a->yh <= 40) ? 20 : 35;
    } else if (sep && c24) {
        // 16-column tiles (46 KB of LDS) only where they also cut the padded columns: planes of <= 40 columns (36 / 38: 48 computed
        // instead of 64).  On the larger planes the 1.31x halo of a 16-column tile costs more than the third workgroup per CU wins.
        family = FLRELU_FAMILY_TILE_SEP;
        tow = a->yw <= 40 ? 16 : 32;
        toh = 12;
    } else if (sep && c42) {
        family = FLRELU_FAMILY_TILE_SEP;      // (20-row tiles: 47 KB of LDS, faster than 35 rows in every mode)
    } else if (sufd && (c22 || c42) && a->fdh == 12) {
        // radial layers (StyleGAN3-R): a 12 x 12 2-D down filter in the forward, the same filter as a 2-D up filter in the backward
        family = FLRELU_FAMILY_TILE_SUFD;
    } else if (fusd && (c22 || c24) && a->fuh == 12) {
        family = FLRELU_FAMILY_TILE_FUSD;
        tow = c22 ? 64 : 32;
        toh = c22 ? 20 : 12;
    }
    // the kernels exist for the rows of kTileShapes and for nothing else
    for (int i = 0; i < (int)(sizeof(kTileShapes) / sizeof(kTileShapes[0])); i++) {
        const FlreluTileShape& s = kTileShapes[i];
        if (s.family != family || s.up != a->up || s.down != a->down || s.tow != tow || s.toh != toh) continue;
        pl.family = family;
        pl.shape = i;
        pl.tow = tow;
        pl.toh = toh;
        pl.tilesX = cdiv(a->yw, tow);
        pl.tilesY = cdiv(a->yh, toh);
    }
    return pl;
}

// shapes() proper: validates the geometry, fills the output fields of `a` and hands back the plan they were read from
static int shapes_and_plan(afcm_filtered_lrelu_args* a, FlreluPlan* pl) {
    AFCM_REQUIRE(a != nullptr, "filtered_lrelu: null args");
    AFCM_REQUIRE(a->up >= 1 && a->down >= 1, "up and down must be at least 1");
    AFCM_REQUIRE(a->fuw >= 1 && a->fdw >= 1 && a->fuh >= 0 && a->fdh >= 0, "fu and fd must not be empty");
    const long long fut_w = a->fuw - 1, fut_h = (a->fuh ? a->fuh : a->fuw) - 1;
    const long long fdt_w = a->fdw - 1, fdt_h = (a->fdh ? a->fdh : a->fdw) - 1;
    const long long cw = (long long)a->xw * a->up + (a->px0 + a->px1) - fut_w;
    const long long ch = (long long)a->xh * a->up + (a->py0 + a->py1) - fut_h;
    AFCM_REQUIRE(cw > fdt_w && ch > fdt_h, "upsampled buffer must be at least the size of downsampling filter");
    const long long yw = (cw - fdt_w + (a->down - 1)) / a->down;
    const long long yh = (ch - fdt_h + (a->down - 1)) / a->down;
    AFCM_REQUIRE(yw > 0 && yh > 0 && yw < (1ll << 31) && yh < (1ll << 31), "output must be at least 1x1");
    a->yw = (int)yw;
    a->yh = (int)yh;
    *pl = flrelu_plan(a);
    a->plane_sum_slots = pl->plane_sum_slots;
    a->row_pitch_ok = pl->row_pitch_ok;
    if (a->sign_mode == AFCM_SIGNS_WRITE) {
        const long long sw_active = yw * a->down - (a->down - 1) + fdt_w;
        const long long sh = yh * a->down - (a->down - 1) + fdt_h;
        a->sign_layout = pl->sign_layout;
        if (pl->sign_layout != 0) {
            // row-quad bytes (one byte = 4 rows of one column); layout 2: column-blocked
            a->sh = (int)((sh + 3) >> 2);
            if (pl->sign_layout == 2) a->sh = (a->sh + 15) & ~15;   // whole dwords: 4 row blocks of 4 quad-rows (filtered_lrelu_wave.hip)
            a->swb = (int)((sw_active + 15) & ~15ll);
        } else {
            a->sh = (int)sh;
            a->swb = (int)(((sw_active + 15) & ~15ll) >> 2);
        }
    }
    return AFCM_OK;
}

}  // namespace afcm

using namespace afcm;

extern "C" int afcm_filtered_lrelu_shapes(afcm_filtered_lrelu_args* a) {
    FlreluPlan pl;
    return shapes_and_plan(a, &pl);
}

extern "C" int afcm_filtered_lrelu(const afcm_filtered_lrelu_args* a, void* stream) {
    AFCM_REQUIRE(a != nullptr && a->x && a->y, "filtered_lrelu: x and y must be non-null");
    AFCM_REQUIRE(a->dtype == AFCM_F32 || a->dtype == AFCM_F16 || a->dtype == AFCM_BF16, "x must be float32, float16 or bfloat16");
    AFCM_REQUIRE(a->n > 0 && a->c > 0 && a->xh > 0 && a->xw > 0, "x is empty");
    AFCM_REQUIRE((long long)a->n * a->c < (1ll << 31), "x is too large");
    afcm_filtered_lrelu_args chk = *a;
    FlreluPlan pl;
    int rc = shapes_and_plan(&chk, &pl);
    if (rc != AFCM_OK) return rc;
    AFCM_REQUIRE(chk.yh == a->yh && chk.yw == a->yw, "y has shape [%d, %d], expected [%d, %d]", a->yh, a->yw, chk.yh, chk.yw);
    if (a->sign_mode != AFCM_SIGNS_NONE) {
        AFCM_REQUIRE(a->signs != nullptr && a->sh > 0 && a->swb > 0 && (a->swb & 3) == 0, "signs must be a [N,C,sh,4k] uint8 tensor");
        if (a->sign_mode == AFCM_SIGNS_WRITE) {
            AFCM_REQUIRE(a->sx == 0 && a->sy == 0, "sign offsets must be zero when writing signs");
            AFCM_REQUIRE(chk.sh == a->sh && chk.swb == a->swb && chk.sign_layout == a->sign_layout,
                         "signs has shape [%d, %d] layout %d, expected [%d, %d] layout %d", a->sh, a->swb, a->sign_layout, chk.sh, chk.swb, chk.sign_layout);
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const bool mfma = pl.family == FLRELU_FAMILY_WAVE || pl.family == FLRELU_FAMILY_MFMA_TILE;
    if ((a->x_pitch && a->x_pitch != a->xw) || (a->y_pitch && a->y_pitch != a->yw) || (a->skip_pitch && a->skip_pitch != a->yw)) {
        AFCM_REQUIRE(pl.row_pitch_ok, "filtered_lrelu: the kernel selected for this call takes dense tensors only (row pitches %d / %d / %d)", a->x_pitch, a->y_pitch, a->skip_pitch);
        AFCM_REQUIRE(a->x_pitch == 0 || a->x_pitch >= a->xw, "x_pitch %d is below the width %d", a->x_pitch, a->xw);
        AFCM_REQUIRE(a->y_pitch == 0 || (a->y_pitch >= a->yw && a->y_pitch % 8 == 0), "y_pitch %d must cover the width %d in whole 16-byte pieces", a->y_pitch, a->yw);
        AFCM_REQUIRE(a->skip_pitch == 0 || a->skip_pitch >= a->yw, "skip_pitch %d is below the width %d", a->skip_pitch, a->yw);
        AFCM_REQUIRE(((a->x_pitch | a->y_pitch | a->skip_pitch) & 1) == 0, "row pitches must be even");
    }
    AFCM_REQUIRE(mfma || (a->oscale == nullptr && a->oscale2 == nullptr && a->skip == nullptr), "filtered_lrelu: oscale / skip need the matrix-core kernels (16-bit dtype, prepared workspace)");
    if (a->sign_mode == AFCM_SIGNS_READ)
        AFCM_REQUIRE((a->sign_layout != 0) == mfma, "sign tensor layout %d does not match the kernel family selected for this call", a->sign_layout);
    // the wave kernels address layout 2 in whole column blocks of 16 and row groups of 16 quad-rows (the shape shapes() gives a
    // sign-writing call): any other shape would be read at the wrong addresses, without a fault
    if (a->sign_mode == AFCM_SIGNS_READ && a->sign_layout == 2)
        AFCM_REQUIRE((a->sh & 15) == 0 && (a->swb & 15) == 0, "signs in layout 2 must have multiples of 16 quad-rows and columns, got [%d, %d]", a->sh, a->swb);
    if (mfma) return flrelu_mfma(a, pl, false, st);

    FlreluParams p;
    p.x = a->x; p.y = a->y; p.b = a->b; p.s = a->signs;
    p.xw = a->xw; p.xh = a->xh; p.yw = a->yw; p.yh = a->yh; p.C = a->c;
    p.px0 = a->px0; p.py0 = a->py0;
    p.tilesX = pl.tilesX; p.tilesY = pl.tilesY;
    p.gain = (float)a->up * (float)a->up * a->gain;
    p.slope = a->slope; p.clamp = a->clamp; p.flip = a->flip_filter;
    p.sx = a->sx; p.sy = a->sy; p.sh = a->sh; p.swb = a->swb;
    p.fscale = 1.f;
    p.planes = a->n * a->c;

    if (pl.family == FLRELU_FAMILY_POINTWISE) {
        // The two 1x1 taps are folded into the launch: NULL (= identity) is the only form the kernel takes.
        if (a->fu != nullptr || a->fd != nullptr) return AFCM_E_NOKERNEL;  // non-identity 1x1 taps: generic path
        return launch_pointwise(a->dtype, p, a->n * a->c, a->sign_mode, st);
    }
    AFCM_REQUIRE(a->fu != nullptr && a->fd != nullptr, "fu and fd must be non-null for resampling filters");
    if (pl.family == FLRELU_FAMILY_STRIP) return flrelu_launch_strip(a, pl, p, st);
    return pl.family == FLRELU_FAMILY_NONE ? AFCM_E_NOKERNEL : flrelu_launch_tile(a, pl, p, st);     // TILE_SEP / _SUFD / _FUSD
}

extern "C" int afcm_filtered_lrelu_prepare(const afcm_filtered_lrelu_args* a, void* stream) {
    AFCM_REQUIRE(a != nullptr && a->workspace != nullptr && a->fu != nullptr && a->fd != nullptr, "filtered_lrelu_prepare: workspace, fu and fd must be non-null");
    const FlreluPlan pl = flrelu_plan(a);
    if (pl.family != FLRELU_FAMILY_WAVE && pl.family != FLRELU_FAMILY_MFMA_TILE) return AFCM_E_NOKERNEL;
    return flrelu_mfma(a, pl, true, (hipStream_t)stream);
}

extern "C" int afcm_filtered_lrelu_act(void* x, uint8_t* signs, int32_t dtype, int32_t n, int32_t c, int32_t h, int32_t w,
                                       int32_t sh, int32_t swb, int32_t sx, int32_t sy, float gain, float slope, float clamp,
                                       int32_t sign_mode, void* stream) {
    AFCM_REQUIRE(x != nullptr && n > 0 && c > 0 && h > 0 && w > 0, "x is empty");
    AFCM_REQUIRE(dtype == AFCM_F32 || dtype == AFCM_F16 || dtype == AFCM_BF16, "x must be float32, float16 or bfloat16");
    if (sign_mode != AFCM_SIGNS_NONE) {
        AFCM_REQUIRE(signs != nullptr && sh > 0 && swb > 0 && (swb & 3) == 0, "signs must be a [N,C,sh,4k] uint8 tensor");
        if (sign_mode == AFCM_SIGNS_WRITE)
            AFCM_REQUIRE(sx == 0 && sy == 0 && sh == h && swb == (((w + 15) & ~15) >> 2), "signs must be [N,C,%d,%d] with zero offsets when writing", h, ((w + 15) & ~15) >> 2);
    }
    FlreluParams p;
    p.x = x; p.y = x; p.b = nullptr; p.s = signs;
    p.xw = w; p.xh = h; p.yw = w; p.yh = h; p.C = c;
    p.px0 = p.py0 = 0; p.tilesX = p.tilesY = 0;
    p.gain = gain; p.slope = slope; p.clamp = clamp; p.flip = 0;
    p.sx = sx; p.sy = sy; p.sh = sh; p.swb = swb; p.fscale = 1.f; p.planes = n * c;
    hipStream_t st = (hipStream_t)stream;
    return launch_pointwise(dtype, p, n * c, sign_mode, st);
}
