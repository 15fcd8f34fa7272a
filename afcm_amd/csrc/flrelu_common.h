// Shared definitions of the filtered_lrelu family: the host plan (which kernel a call runs, on which tiles), the launchers of
// the per-family translation units, and the device helpers that more than one unit uses.
#pragma once
#include <type_traits>

#include "common.h"

namespace afcm {

struct FlreluParams {
    const void* x;
    void* y;
    const void* b;
    unsigned char* s;
    int xw, xh, yw, yh, C;
    int px0, py0;
    int tilesX, tilesY;
    float gain;  // up^2 * gain, formed in fp32 like filtered_lrelu.cu:484
    float slope, clamp;
    int flip;
    int sx, sy, sh, swb;
    float fscale;  // pointwise kernel only: product of the 1x1 filters
    int planes;    // strip kernel only: N * C
};

// ---------------------------------------------------------------------------------------------
// The plan: everything afcm_filtered_lrelu_shapes() reports about the kernel behind a call and everything the launch needs to
// pick that very kernel.  flrelu_plan() (filtered_lrelu.hip) is the only place that decides; it is pure host arithmetic on what
// is known BEFORE the caller allocates: the geometry, the dtype, the sign mode and layout, and whether `workspace` and `b` are
// null -- never the row pitches, which the caller chooses after shapes() has told it whether they are allowed.
enum FlreluFamily {
    FLRELU_FAMILY_NONE = 0, FLRELU_FAMILY_POINTWISE, FLRELU_FAMILY_STRIP,    // no kernel (AFCM_E_NOKERNEL); 1x1 filters, up = down = 1; fp32 separable
    FLRELU_FAMILY_TILE_SEP, FLRELU_FAMILY_TILE_SUFD, FLRELU_FAMILY_TILE_FUSD,   // exact LDS tile: separable / separable up, 2-D down / 2-D up, separable down
    FLRELU_FAMILY_MFMA_TILE, FLRELU_FAMILY_WAVE                              // matrix cores: LDS tile (sign layout 1) / wave kernels (sign layout 2)
};

struct FlreluPlan {
    int family;
    int up, down;              // the (up, down) case; the tap counts follow from it inside a family
    int tow, toh;              // output tile (strip family: columns per strip and output rows per segment)
    int shape;                 // exact LDS tile: row of kTileShapes
    int tilesX, tilesY;        // tiles per plane
    int oy0, dshift;           // wave kernels, READ: origin of the strips (see flrelu_plan)
    int sign_layout;           // layout the family writes and reads: 0 packed codes, 1 row-quad bytes, 2 column-blocked
    int row_pitch_ok;          // the kernel addresses rows by pitch
    int plane_sum_slots;       // tiles per plane of a kernel that can write plane sums, else 0
};

FlreluPlan flrelu_plan(const afcm_filtered_lrelu_args* a);

// The shapes of the exact LDS tile: one row per set of kernels filtered_lrelu_tile.hip builds.  The plan picks a row, the launcher
// instantiates it, so a shape is written down here and nowhere else.  `ro` = output rows per item of the last stage.
struct FlreluTileShape { int family, up, down, tow, toh, ro; };
constexpr FlreluTileShape kTileShapes[] = {
    {FLRELU_FAMILY_TILE_SEP, 2, 2, 64, 20, 5},  {FLRELU_FAMILY_TILE_SEP, 2, 2, 64, 35, 5},  {FLRELU_FAMILY_TILE_SEP, 2, 4, 16, 12, 4},
    {FLRELU_FAMILY_TILE_SEP, 2, 4, 32, 12, 4},  {FLRELU_FAMILY_TILE_SEP, 4, 2, 64, 20, 5},  {FLRELU_FAMILY_TILE_SUFD, 2, 2, 64, 20, 5},
    {FLRELU_FAMILY_TILE_SUFD, 4, 2, 64, 20, 5}, {FLRELU_FAMILY_TILE_FUSD, 2, 2, 64, 20, 5}, {FLRELU_FAMILY_TILE_FUSD, 2, 4, 32, 12, 4},
};

// Tile shapes of the matrix-core families.  The tall variant serves planes of 33..48 output rows (the 36^2 / 38^2 planes of the
// 256^2 generator): ONE 48-row tile instead of two 32-row tiles that are 12 % full in their second row.  The constant fragments
// do not depend on the tile shape (only on up, down and the filters), so both variants share one prepared workspace; the sign
// layout is tile-independent.
template <int UP, int DOWN> struct MfmaTile { static constexpr int TOW = DOWN == 4 ? 32 : 64, TOH = 32; };
constexpr int kTallTOH = 48;
constexpr int kWavePitchSlack = 128;        // elements a row pitch may exceed the plane width by (wave kernels)

// Per-family launchers: each runs the kernel the plan names and nothing else.  `p` arrives filled, tile counts included.
int flrelu_launch_tile(const afcm_filtered_lrelu_args* a, const FlreluPlan& pl, const FlreluParams& p, hipStream_t st);
int flrelu_launch_strip(const afcm_filtered_lrelu_args* a, const FlreluPlan& pl, const FlreluParams& p, hipStream_t st);
int flrelu_strip_columns(int up, int down, int sign_mode);     // output columns per strip; <= 0: no strip kernel for (up, down)
int flrelu_mfma(const afcm_filtered_lrelu_args* a, const FlreluPlan& pl, bool prepare, hipStream_t st);   // family MFMA_TILE / WAVE, or their prepare

// Runtime dtype -> element type: f(T{}).
template <typename F>
static inline int with_dtype(int dtype, F&& f) {
    return dtype == AFCM_F32 ? f(float{}) : dtype == AFCM_F16 ? f(f16_t{}) : f(bf16_t{});
}

// Runtime (up, down) -> compile-time constants, for the three resampling cases of the model: f(UP, DOWN) as integral constants.
template <typename F>
static inline int with_up_down(int up, int down, F&& f) {
    using std::integral_constant;
    switch (up * 10 + down) {
        case 22: return f(integral_constant<int, 2>{}, integral_constant<int, 2>{});
        case 24: return f(integral_constant<int, 2>{}, integral_constant<int, 4>{});
        case 42: return f(integral_constant<int, 4>{}, integral_constant<int, 2>{});
        default: return AFCM_E_NOKERNEL;
    }
}

// Runtime sign mode -> compile-time constant: f(std::integral_constant<int, AFCM_SIGNS_*>{}).
template <typename F>
static inline void with_sign_mode(int sign_mode, F&& f) {
    switch (sign_mode) {
        case AFCM_SIGNS_NONE: f(std::integral_constant<int, AFCM_SIGNS_NONE>{}); break;
        case AFCM_SIGNS_WRITE: f(std::integral_constant<int, AFCM_SIGNS_WRITE>{}); break;
        default: f(std::integral_constant<int, AFCM_SIGNS_READ>{}); break;
    }
}

// ---------------------------------------------------------------------------------------------
// Activation on one element of the upsampled grid.  Returns the 2-bit code in WRITE mode.
template <int SIGN>
__device__ __forceinline__ unsigned act_elem(float& v, float gain, float slope, float clamp, unsigned code_in) {
    v *= gain;
    if (SIGN == AFCM_SIGNS_READ) {
        if (code_in & 1u) v *= slope;
        if (code_in & 2u) v = 0.f;
        return 0u;
    }
    unsigned code = __float_as_uint(v) >> 31;
    if (code) v *= slope;
    if (fabsf(v) > clamp) {
        code = 2u;
        v = (v < 0.f) ? -clamp : clamp;
    }
    return code;
}

// Fetch the packed codes of 4 consecutive elements starting at sign coordinate (X, Y); elements
// outside the tensor read as code 0 (value passes through unchanged).
__device__ __forceinline__ unsigned fetch_codes4(const unsigned char* __restrict__ srow_base, int X, int Y, int sh, int swb) {
    if ((unsigned)Y >= (unsigned)sh) return 0u;
    const unsigned char* row = srow_base + (size_t)Y * swb;
    int b0 = X >> 2;  // arithmetic shift: floor for negative X
    unsigned lo = ((unsigned)b0 < (unsigned)swb) ? row[b0] : 0u;
    unsigned hi = ((unsigned)(b0 + 1) < (unsigned)swb) ? row[b0 + 1] : 0u;
    return ((lo | (hi << 8)) >> ((X & 3) << 1)) & 0xffu;
}

__device__ __forceinline__ int quad_or(int v) {
    // OR-reduce over the 4 lanes of a quad with two DPP quad_perm moves ([1,0,3,2] then [2,3,0,1]).
    v |= __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true);
    v |= __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true);
    return v;
}

}  // namespace afcm
