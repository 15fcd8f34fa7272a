/*
 * afcm_hip.h -- C ABI of libafcm_hip.so: the MI355X (gfx950) kernels behind the
 * `--model stylegan3` generator hot path of zhiyuns/AFCM.
 *
 * This is the drop-in boundary.  Every entry point replaces one function of the reference's
 * native plugins (pybind modules JIT-built by torch_utils/custom_ops.py:59-155); the reference
 * interface each one stands in for is cited above it.  Shorthand:
 *   SG3OPS = models/networks/stylegan3/torch_utils/ops   (in the reference tree)
 *   NET    = models/networks/stylegan3/networks_stylegan3.py
 *
 * Conventions
 *   - plain C: device pointers + sizes; no torch / ATen types.  All tensor pointers are DEVICE
 *     pointers into contiguous NCHW storage; filters are DEVICE float32 arrays as in the
 *     reference (filtered_lrelu.cpp:26).
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Launches are
 *     asynchronous; no call allocates, synchronises or keeps global mutable state, so all
 *     of them are re-entrant across streams and capturable into a hipGraph.  (The reference
 *     is not: global filter buffers g_fbuf/c_fbuf, filtered_lrelu.cu:77-78.)
 *   - return value: 0 = launched; AFCM_E_NOKERNEL (-1) = no specialised kernel for these
 *     parameters (the reference's `return_code = -1`, filtered_lrelu.cpp:52-56 -- the host
 *     falls back to the generic upfirdn2d + act path); AFCM_E_INVALID (-2) = argument check
 *     failed (the reference's TORCH_CHECK); >= 1000 = 1000 + hipError_t of the launch.
 *   - dtype codes: AFCM_F32, AFCM_F16, AFCM_BF16 (bf16 is new capability; the reference
 *     plugin accepts half/float only).  Arithmetic is always fp32 inside the kernels, with TWO exceptions:
 *     afcm_plane_metrics / afcm_volume_ssim (validation metrics, end of this header) compute in float64 after their loads; afcm_slice_assemble
 *     (after it) normalises in the type numpy gives the loader's expression, float64 for every source but float32.
 */
#ifndef AFCM_HIP_H
#define AFCM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AFCM_ABI_VERSION 13  /* 13: + afcm_grad_stats, afcm_trainlog_append, afcm_trainlog_cols (the training log on the device, end of this header; additions to v13: no existing entry point or struct changes, so the number stays).  13: + afcm_rescale_intensity, afcm_rescale_workspace_bytes, afcm_rescale_plan (intensity rescaling; additions only, so the number stays).  13: + afcm_volume_ssim, afcm_volume_ssim_workspace_bytes (the 7^3-window SSIM map's layer sums; additions only, so the number stays).  13: + afcm_slice_assemble, afcm_halo_accumulate (whole-volume inference; additions only, so the number stays).  13: + afcm_adam_multi_capturable_d (an addition only, so the number stays).  13 (r08): + afcm_conv2d_plan, afcm_conv2d_wgrad_plan (pure-host queries of the dispatch; additions only, so the number stays).  13 (r07): + afcm_plane_metrics, afcm_plane_metrics_workspace_bytes (additions only: no existing entry point or struct changes, so the number stays).  13 (r06): + afcm_noop, afcm_pool_blocks_fwd / _bwd, afcm_adam_multi_capturable, afcm_conv2d_wgrad_dots_ld, afcm_mapping_input_bwd_workspace_bytes, afcm_axpy_planes, afcm_l1_partials, afcm_l1_grad, afcm_fc_act_fwd / _bwd, afcm_mapping_input_fwd / _bwd (additions only; see the end of this header for the r06 entry points).  12 (r05): + afcm_conv2d_block_k_ks, afcm_conv2d_pack_weights_bk; the packed layout's K-chunk depends on (dtype, kernel size): 16-bit 3x3 images are [nkc][9][rows_pad][32] for the v_mfma 16x16x32 kernel (the pack / conv entry points keep their signatures).  11 (r04): + afcm_amax_bits, afcm_split16, afcm_conv2d_pack_split, afcm_conv2d_split, afcm_unscale, afcm_plane_dot_parts (additions only).  10 (r04): + afcm_filtered_lrelu_args.clamp_flags (appended), afcm_plane_dot_gated_ld; the runtime getenv switches are gone.  9 (r03): + afcm_affine_bank_*, afcm_modulation_bank_*, afcm_conv2d_pack_bank, afcm_conv2d_stride2 (additions only; every v8 entry point and struct is unchanged) */

enum { AFCM_F32 = 0, AFCM_F16 = 1, AFCM_BF16 = 2 };
enum { AFCM_OK = 0, AFCM_E_NOKERNEL = -1, AFCM_E_INVALID = -2 };
enum { AFCM_SIGNS_NONE = 0, AFCM_SIGNS_WRITE = 1, AFCM_SIGNS_READ = 2 };

/* Library / device introspection. */
int afcm_abi_version(void);
/* Human-readable description of the last AFCM_E_INVALID on this thread. */
const char* afcm_last_error(void);
/* An empty one-wave launch on `stream`: what a launch costs the host and the device's front end with no work behind it
 * (bench.py's `host_calibration`).  No counterpart in the reference (its launches go through ATen). */
int afcm_noop(void* stream);

/* ------------------------------------------------------------------------------------------
 * filtered_lrelu -- fused bias -> zero-insert upsample -> pad/crop -> FIR(fu) * up^2 ->
 *                   * gain -> leaky ReLU -> clamp -> FIR(fd) -> decimate.
 *
 * Replaces plugin `filtered_lrelu(x, fu, fd, b, si, up, down, px0, px1, py0, py1, sx, sy, gain,
 * slope, clamp, flip_filter, writeSigns) -> (y, so, return_code)`
 *   SG3OPS/filtered_lrelu.cpp:16-209, kernels SG3OPS/filtered_lrelu.cu:139-1099.
 *
 * Sign tensor (2 bits per element of the upsampled grid, bit0 = value was negative, value 2 =
 * clamped): uint8 [N, C, sh, swb] with element x of a row in byte x>>2 at bits 2*(x&3) -- the
 * reference's shape and packing (filtered_lrelu.cpp:87-94).  In WRITE mode sx = sy = 0 is
 * required (the reference never writes with an offset: filtered_lrelu.py:115,263).
 * In READ mode element (X, Y) of this call's upsampled grid uses code (X + sx, Y + sy); codes
 * outside the tensor leave the value unchanged (filtered_lrelu.cu:564-571).
 * Separable filters: fuh == 0 / fdh == 0 and fu/fd hold fuw / fdw taps (the reference's
 * "shape [n, 0] indicates separable", filtered_lrelu.cpp:49-50).
 * ---------------------------------------------------------------------------------------- */
typedef struct afcm_filtered_lrelu_args {
    const void* x;          /* [N, C, xh, xw]                                  */
    void*       y;          /* [N, C, yh, yw]   (allocated by the caller)      */
    const void* b;          /* [C] same dtype as x, or NULL                    */
    uint8_t*    signs;      /* [N, C, sh, swb] or NULL                         */
    const float* fu;        /* device, fuw taps (separable) or fuh*fuw         */
    const float* fd;        /* device, fdw taps (separable) or fdh*fdw         */
    int32_t dtype;          /* AFCM_F32 / AFCM_F16 / AFCM_BF16                 */
    int32_t n, c, xh, xw, yh, yw;
    int32_t fuw, fuh, fdw, fdh;     /* fuh/fdh == 0: separable                 */
    int32_t up, down;
    int32_t px0, px1, py0, py1;
    int32_t sx, sy;         /* sign offsets                                    */
    int32_t sh, swb;        /* sign tensor rows / bytes per row                */
    float   gain, slope, clamp;     /* clamp = +inf to disable                 */
    int32_t flip_filter;
    int32_t sign_mode;      /* AFCM_SIGNS_*                                    */
    void*   workspace;      /* NULL, or afcm_filtered_lrelu_workspace_bytes() of device memory filled by
                               afcm_filtered_lrelu_prepare() for THIS (fu, fd, up, down, px0, py0, gain, flip, dtype):
                               enables the matrix-core kernels for 16-bit dtypes                              */
    int32_t sign_layout;    /* 0: row-major 2-bit codes (reference layout); 1: row-quad bytes written by the
                               matrix-core kernels ([N,C,ceil(sh/4),swq]); set by afcm_filtered_lrelu_shapes(),
                               must be passed back unchanged with the sign tensor in READ mode; 2: column-blocked
                               row-quads of the wave kernels (sh and swb multiples of 16, checked in READ mode)  */
    int32_t plane_sum_slots;/* set by afcm_filtered_lrelu_shapes(): partial sums per plane the selected kernel emits (0: none) */
    float*  plane_sum;      /* NULL, or fp32 [N*C][plane_sum_slots]: the matrix-core kernels store the sum of every output tile
                               (no atomics); summed over slots and N in a backward call this is the bias gradient
                               (db = dx.sum([0,2,3]), SG3OPS/filtered_lrelu.py:266) without a second pass over dx.        */
    const float* oscale;    /* NULL, or fp32 [N*C]: y = (filtered_lrelu(...) + skip) * oscale[n*C + c].  Matrix-core kernels only.
                               Lets the caller fold per-plane factors that would otherwise be separate passes over the tensor:
                               the NEXT layer's style modulation s[n,i] (NET:46-47, forward) and the demodulation d[n,o]
                               of the conv that produced x (NET:50-52, backward: the op is linear in dy given the codes). */
    const void*  skip;      /* NULL, or [N, C, yh, yw] of x's dtype: the encoder feature added after the activation
                               (x + x_skip, NET:376-377), added before oscale.  Matrix-core kernels only.                */
    const float* oscale2;   /* NULL, or a second fp32 [N*C] factor multiplied with oscale (backward: demodulation x styles) */
    int32_t x_pitch, y_pitch, skip_pitch;
                            /* row pitch of x / y / skip in ELEMENTS; 0 = dense (pitch = width).  A pitched tensor is
                               [N, C, H, pitch] in memory with the first W columns of every row meaningful (MI355X layout of the
                               16-bit activation stream: rows start on 64-byte boundaries).  Only the
                               kernels for which afcm_filtered_lrelu_shapes() reports row_pitch_ok take a pitch; they accept
                               x_pitch / skip_pitch up to width + 128 and y_pitch up to 64 * ceil(yw / 64) (AFCM_E_INVALID beyond),
                               and with y_pitch set they write finite values to every column of y up to the pitch (columns
                               >= yw are padding).                                                                              */
    int32_t row_pitch_ok;   /* set by afcm_filtered_lrelu_shapes(): 1 if the kernel selected for these arguments accepts pitches */
    int32_t* clamp_flags;   /* NULL, or int32 [N*C][plane_sum_slots] (sign-writing calls of the wave kernels, i.e. plane_sum_slots > 0 and
                               no bias operand): slot = 1 if that strip's activations could reach the clamp (it then took the exact
                               per-element path), else 0.  Every slot is written.  A plane whose slots are all 0 went through linear
                               filters around a pure leaky ReLU: there filtered_lrelu is positively homogeneous of degree 1, which
                               the caller may use to derive <dL/dy, y> from <g, z> (afcm_plane_dot_gated_ld).                      */
} afcm_filtered_lrelu_args;

/* Output / sign-tensor geometry for the arguments above (filtered_lrelu.cpp:61-94). Fills yh, yw
 * and, for WRITE mode, sh, swb.  Pure host arithmetic. */
int afcm_filtered_lrelu_shapes(afcm_filtered_lrelu_args* a);
/* Fused argument sets: the separable 12 / 24-tap cases (up 2 / down 2, up 2 / down 4, up 4 / down 2), and the radial ones, where
 * one filter is 12 x 12 (fuh / fdh = 12) and the other separable: fu 12 or 24 taps with fd 12 x 12 (up 2 or 4, down 2), and fu 12 x 12
 * with fd 12 or 24 taps (up 2, down 2 or 4).  Their sign tensors use layout 0.  Every other 2-D argument set returns AFCM_E_NOKERNEL.
 * Base pointers (not checked here: the caller keeps them): x, y and skip on 4-byte boundaries -- the 16-bit kernels move aligned pairs and
 * 16-byte pieces of pixels from dword addresses, which with the even widths and pitches required above puts every row on one --, signs on
 * a 4-byte boundary (the codes are read and written in dwords), b at any element, fu / fd / oscale / oscale2 fp32. */
int afcm_filtered_lrelu(const afcm_filtered_lrelu_args* a, void* stream);

/* Matrix-core path (16-bit dtypes, the separable 12/24-tap cases of the generator): the FIR passes run as banded
 * Toeplitz products on v_mfma_f32_16x16x32_{bf16,f16}.  The constant Toeplitz fragments depend only on the layer
 * configuration; build them once per layer with afcm_filtered_lrelu_prepare() into `workspace` (this replaces the
 * reference's per-call setup_filters_kernel + copy to __constant__ memory, filtered_lrelu.cu:87-117, without any
 * global state).  Returns AFCM_E_NOKERNEL when the configuration has no matrix-core kernel. */
int64_t afcm_filtered_lrelu_workspace_bytes(void);
int afcm_filtered_lrelu_prepare(const afcm_filtered_lrelu_args* a, void* stream);

/* In-place gain -> leaky ReLU -> clamp with sign write/read, used by the generic fallback.
 * Replaces plugin `filtered_lrelu_act_(x, si, sx, sy, gain, slope, clamp, writeSigns) -> so`
 *   SG3OPS/filtered_lrelu.cpp:213-290, kernel SG3OPS/filtered_lrelu.cu:1105-1211.
 * signs: uint8 [N, C, h, swb] with swb = ceil16(w)/4 in WRITE mode, on a 4-byte boundary (one dword of codes per thread); x at any element. */
int afcm_filtered_lrelu_act(void* x, uint8_t* signs, int32_t dtype, int32_t n, int32_t c, int32_t h, int32_t w,
                            int32_t sh, int32_t swb, int32_t sx, int32_t sy, float gain, float slope, float clamp,
                            int32_t sign_mode, void* stream);

/* ------------------------------------------------------------------------------------------
 * upfirdn2d -- zero-insert upsample, pad/crop, 2-D FIR, decimate.
 * Replaces plugin `upfirdn2d(x, f, upx, upy, downx, downy, padx0, padx1, pady0, pady1, flip, gain) -> y`
 *   SG3OPS/upfirdn2d.cpp:16-98, kernels SG3OPS/upfirdn2d.cu:29-375.
 * f is a device float32 [fh, fw] array (a separable filter is two calls, as in
 * SG3OPS/upfirdn2d.py:244-245).  y: [N, C, yh, yw] with yw = (xw*upx + padx0 + padx1 - fw + downx) / downx.
 * x and y may sit at any element offset: the 16-bit rows kernel (16-byte loads) is taken only when both lie on 4-byte boundaries, the other
 * kernels read element by element (same taps in the same order: the result does not depend on the choice).
 * ---------------------------------------------------------------------------------------- */
int afcm_upfirdn2d(void* y, const void* x, const float* f, int32_t dtype, int32_t n, int32_t c, int32_t xh, int32_t xw,
                   int32_t yh, int32_t yw, int32_t fh, int32_t fw, int32_t upx, int32_t upy, int32_t downx, int32_t downy,
                   int32_t padx0, int32_t pady0, int32_t flip, float gain, void* stream);

/* ------------------------------------------------------------------------------------------
 * bias_act -- y = clamp(act(x + b) * gain); grad = 1: first-order backward from saved x/y;
 * grad = 2: second-order.  act: 1 linear, 2 relu, 3 lrelu, 4 tanh, 5 sigmoid, 6 elu, 7 selu,
 * 8 softplus, 9 swish (the reference's cuda_idx, SG3OPS/bias_act.py:21-31).
 * Replaces plugin `bias_act(x, b, xref, yref, dy, grad, dim, act, alpha, gain, clamp) -> y`
 *   SG3OPS/bias_act.cpp:32-90, kernel SG3OPS/bias_act.cu:23-147.
 * x is viewed as [outer, nb, inner] with the bias indexed by the middle dimension
 * (nb = 0 / b = NULL: no bias).  xref / yref / dy may be NULL when the mode does not need them.
 * ---------------------------------------------------------------------------------------- */
int afcm_bias_act(void* y, const void* x, const void* b, const void* xref, const void* yref, const void* dy,
                  int32_t dtype, int64_t numel, int64_t inner, int32_t nb, int32_t grad, int32_t act, float alpha,
                  float gain, float clamp, void* stream);


/* ------------------------------------------------------------------------------------------
 * Dense convolution behind modulated_conv2d / the encoder convs.
 *
 * The reference has no native conv: `modulated_conv2d` (NET:25-64) builds per-sample weights
 * and calls a grouped F.conv2d (cuDNN) through conv2d_gradfix.conv2d (SG3OPS/conv2d_gradfix.py:37-58),
 * and EncoderLayer calls conv2d_gradfix.conv2d directly (NET:505).  These entry points replace that
 * conv call with MFMA implicit-GEMM kernels using the equivalent shared-weight form
 *     y[n,o] = oscale[n,o] * conv(W, x[n]),   x pre-scaled per (n,i) plane by afcm_scale_planes.
 * All of them are cross-correlations (F.conv2d semantics) with stride 1, k in {1,3}, 0 <= pad <= k-1.
 * ---------------------------------------------------------------------------------------- */

/* K-chunk (channels) of the packed weight layout.
 * afcm_conv2d_block_k(dtype): the fp32, 1x1 and stride-2 (afcm_conv2d_stride2) kernels -- 16 for 16-bit, 8 for fp32;
 * afcm_conv2d_block_k_ks(dtype, ks): the stride-1 kernel for this kernel size -- 32 for 16-bit 3x3 (one v_mfma_f32_16x16x32 K step),
 * else as above.  afcm_conv2d[_ld], afcm_conv2d_split and the pack entry points below use this one. */
int afcm_conv2d_block_k(int32_t dtype);
int afcm_conv2d_block_k_ks(int32_t dtype, int32_t ks);

/* Pack fp32 weights w[cout][cin][k][k] into the kernel layout [ceil(cols/BK)][k*k][rows_pad][BK] of
 * `dtype` (BK = afcm_conv2d_block_k_ks(dtype, ks)), zero padded.  mode 0: forward (rows = cout, cols = cin).  mode 1: data gradient
 * (rows = cin, cols = cout, taps flipped).  rows_pad: multiple of 64, >= rows. */
int afcm_conv2d_pack_weights(void* dst, const float* w, int32_t dtype, int32_t cout, int32_t cin, int32_t ks,
                             int32_t mode, int32_t rows_pad, void* stream);

/* Both images of one layer in ONE launch (training: the forward packs what its backward will need): dst_fwd as mode 0,
 * dst_dgrad as mode 1 of afcm_conv2d_pack_weights; either may be NULL.  Destinations 32-byte aligned. */
int afcm_conv2d_pack_weights2(void* dst_fwd, void* dst_dgrad, const float* w, int32_t dtype, int32_t cout, int32_t cin, int32_t ks,
                              int32_t rows_pad_fwd, int32_t rows_pad_dgrad, void* stream);
/* afcm_conv2d_pack_weights with an explicit K-chunk: block_k = afcm_conv2d_block_k(dtype) (the image afcm_conv2d_stride2 reads) or
 * afcm_conv2d_block_k_ks(dtype, ks). */
int afcm_conv2d_pack_weights_bk(void* dst, const float* w, int32_t dtype, int32_t cout, int32_t cin, int32_t ks, int32_t mode,
                                int32_t rows_pad, int32_t block_k, void* stream);

/* y[n, cout, h+2*pad-k+1, w+2*pad-k+1] = oscale[n*cout+o] * sum W * x + obias[o].   oscale / obias (fp32) may be NULL.
 * obias is the layer bias the reference adds at the head of filtered_lrelu (x + b before the padding, NET:371 ->
 * SG3OPS/filtered_lrelu.py:133): the conv output IS the whole unpadded image, so adding it in this epilogue is the same
 * arithmetic and saves the conversion work in filtered_lrelu's input staging.
 * For the data gradient call it with the mode-1 packing, cin/cout swapped and pad' = k-1-pad. */
int afcm_conv2d(void* y, const void* x, const void* wpacked, const float* oscale, const float* obias, int32_t dtype, int32_t n,
                int32_t cin, int32_t cout, int32_t h, int32_t w, int32_t ks, int32_t pad, int32_t rows_pad, void* stream);
/* The same with row-pitched activations (x: [N, cin, h, x_pitch], y: [N, cout, P, y_pitch] in memory, the first w / Q columns of
 * a row meaningful; 0 = dense).  MI355X layout of the 16-bit activation stream: rows start on 64-byte boundaries.
 * Pitches are taken by the 16-bit 3x3 kernel only.  Columns >= w of x are never used; columns >= Q of y are padding: the kernel
 * writes finite values up to the next multiple of 8 past Q (the tail of a row's last 8-pixel granule) and leaves the rest of the
 * padding UNWRITTEN.
 * Base pointers (not checked here: the caller keeps them): x and y on 4-byte boundaries -- a 16-bit image is fetched in 8-byte buffer loads
 * at dword offsets from its base, which is why widths and pitches are even --, wpacked on 16 bytes (32 as afcm_conv2d_pack_weights writes
 * it), oscale / obias fp32. */
int afcm_conv2d_ld(void* y, const void* x, const void* wpacked, const float* oscale, const float* obias, int32_t dtype, int32_t n,
                   int32_t cin, int32_t cout, int32_t h, int32_t w, int32_t ks, int32_t pad, int32_t rows_pad, int32_t x_pitch,
                   int32_t y_pitch, void* stream);

/* Pure host (no device memory, works without a GPU): which kernel afcm_conv2d_ld (split == 0) or afcm_conv2d_split (split != 0: dtype is
 * the parts' type, ks 3) runs for these arguments with rows_pad = cout rounded up to 64, from the function both entry points dispatch
 * through.  out[0] family: 0 direct (cin <= 4), 1 96-row blocks, 2 128-row blocks + one 64-row block, 3 64-row blocks, 4 128-row blocks;
 * out[1] rows per block of the launch that out[4] / out[5] describe (family 2: its 64-row launch; the 128-row launch in front of it
 * takes one work item per workgroup); out[2], out[3] output tile TH x TW (0 for the direct kernel, whose tile is fixed);
 * out[4] work items (tiles x images x row blocks); out[5] workgroups -- fewer than out[4] when a persistent launch (64-row and 96-row
 * 16-bit 3x3) takes more than one round: one round is 3 (2 for 96 rows) workgroups per compute unit of the current device, 256 units
 * when there is no device; out[6] 1: the 16-byte transposed ("fast") epilogue; out[7] kernel: 0 conv2d_fwd16x (16-bit 3x3), 1 the
 * general 16-bit kernel (1x1), 2 the fp32 kernel, 3 direct, 4 conv2d_fwd16x on split operands. */
int afcm_conv2d_plan(int32_t dtype, int32_t n, int32_t cin, int32_t cout, int32_t h, int32_t w, int32_t ks, int32_t pad, int32_t x_pitch,
                     int32_t y_pitch, int32_t split, int32_t out[8]);

/* Weight gradient dw[cout][cin][k][k] (fp32) = sum_n sum_pixels dy[n,o,p,q] * x[n,i,p+r-pad,q+s-pad].
 * workspace: fp32 [afcm_conv2d_wgrad_splits(...)][cout][cin][k][k]. */
int afcm_conv2d_wgrad_splits(int32_t n, int32_t cout, int32_t cin, int32_t p_rows);
int afcm_conv2d_wgrad(float* dw, float* workspace, const void* dy, const void* x, int32_t dtype, int32_t n, int32_t cin,
                      int32_t cout, int32_t h, int32_t w, int32_t ks, int32_t pad, void* stream);
/* The same with row-pitched operands (0 = dense); 16-bit, 3x3 pad 2 or 1x1 pad 0 only.  Columns >= w of x are never used; of dy,
 * the columns up to the next multiple of 8 past Q must hold FINITE values (they multiply zeros): afcm_conv2d_ld writes exactly those
 * columns, afcm_filtered_lrelu writes the whole pitch.
 * Base pointers (not checked here: the caller keeps them): dy and x on 4-byte boundaries (a lane fetches 4-byte pieces or, in the granule
 * kernel, 16 bytes = 8 pixels from a dword address; widths and pitches are even); dw and workspace fp32, the 16-byte reduction is taken
 * only where both allow it. */
int afcm_conv2d_wgrad_ld(float* dw, float* workspace, const void* dy, const void* x, int32_t dtype, int32_t n, int32_t cin,
                         int32_t cout, int32_t h, int32_t w, int32_t ks, int32_t pad, int32_t dy_pitch, int32_t x_pitch, void* stream);
/* afcm_conv2d_wgrad_ld that ALSO returns dots[n][cin] = sum_{o, tap} wq[o][i][tap] * dW_n[o][i][tap] (r06), dW_n = image n's share of the weight
 * gradient, wq = wref [cout][cin][ks][ks] (fp32) rounded to the operands' 16-bit type: by bilinearity this is <x[n, i], dx[n, i]> with
 * dx = conv^T(wq, dy) -- for a conv whose input carries a per-plane style factor s (modulated_conv2d, NET:41-63) the gradient of s times s,
 * which the host otherwise takes from a pass over x and dx (afcm_plane_dot_ld).  The K range is split over workgroups WITHIN images; available
 * for the 16-bit granule kernel (3x3 pad 2, 1x1 pad 0) when the split count of afcm_conv2d_wgrad_splits() is a multiple of n <= 64, else
 * AFCM_E_NOKERNEL (nothing launched: call afcm_conv2d_wgrad_ld and afcm_plane_dot_ld).  Same workspace and the same base alignment of dy
 * and x (4 bytes) as afcm_conv2d_wgrad_ld. */
int afcm_conv2d_wgrad_dots_ld(float* dw, float* dots, float* workspace, const void* dy, const void* x, const float* wref, int32_t dtype, int32_t n,
                              int32_t cin, int32_t cout, int32_t h, int32_t w, int32_t ks, int32_t pad, int32_t dy_pitch, int32_t x_pitch,
                              void* stream);

/* Pure host: the plan of afcm_conv2d_wgrad_ld (dots == 0) or afcm_conv2d_wgrad_dots_ld (dots != 0; AFCM_E_NOKERNEL where that one declines).
 * out[0] kernel: 0 fp32, 1 16-bit with 4-byte LDS-DMA pieces (3x3 pad 0 / 1), 2 16-bit granule kernel (3x3 pad 2, 1x1 pad 0); out[1] pad
 * parity of kernels 0 and 1; out[2] granule kernel: 1 the 16x16x32 MFMA form, 0 the 32x32x16 one; out[3] granule kernel: 1 one descriptor
 * per tensor (both operands below 2 GB); out[4] split count (slabs written); out[5] K macro-steps per split; out[6] the reduction:
 * 0 scalar (k*k*cout*cin not a multiple of 4), 1 / 2 / 3 the 16-byte one with 256 / 64 / 16 columns per workgroup (splits < 8, 8..63,
 * >= 64), 4 the image-aligned one that also writes dots; out[7] splits per image (dots) or 0. */
int afcm_conv2d_wgrad_plan(int32_t dtype, int32_t n, int32_t cin, int32_t cout, int32_t h, int32_t w, int32_t ks, int32_t pad,
                           int32_t dy_pitch, int32_t x_pitch, int32_t dots, int32_t out[8]);

/* y[plane, :] = x[plane, :] * scale[plane] with dtype conversion (style modulation s[n,i] of NET:46-47 and the
 * demodulation d[n,o] of NET:50-52 applied to activations instead of weights).  scale may be NULL (pure cast).  Every element is
 * the fp32 product rounded once, to nearest even, into y's type (the sign of a zero kept).  x and y may sit at
 * any element offset: 4-element vector accesses are taken only when hw % 4 == 0 and both bases are aligned to them. */
int afcm_scale_planes(void* y, const void* x, const float* scale, int32_t dtype_in, int32_t dtype_out, int64_t planes,
                      int32_t hw, void* stream);

/* out[plane] = sum_i a[plane,i] * b[plane,i]  (b == NULL: plain sum); fp32 accumulation.  Used for the style /
 * demodulation / bias gradients.  a and b on 16-byte boundaries (AFCM_E_INVALID otherwise). */
int afcm_plane_dot(float* out, const void* a, const void* b, int32_t dtype, int64_t planes, int32_t hw, void* stream);
/* The same over planes of h rows x w columns with row pitches (elements; 0 = dense); padding columns are never read.  Rows of at
 * least one 16-byte vector (w >= 16 / element size; w equal to it included), starting on 4-byte boundaries, h * max(pitch) < 2^27. */
int afcm_plane_dot_ld(float* out, const void* a, const void* b, int32_t dtype, int64_t planes, int32_t h, int32_t w,
                      int32_t a_pitch, int32_t b_pitch, void* stream);
/* The demodulation gradient's dot product by homogeneity (fused layer node, NET:41-57 backward): for a plane whose clamp_flags
 * (afcm_filtered_lrelu_args, [planes][slots]) are all 0,  out = out_scale * (gz - next_scale * gskip)  -- <dys, y> = d <dL/dy, y> =
 * d (<g, z> - s_next <g, skip>) by Euler's identity for the degree-1 homogeneous filtered_lrelu -- and neither a nor b is read;
 * a flagged plane gets the real dot product sum a * b, and so does a plane whose two sums cancel below 1/8 of their size
 * (|gz - next_scale gskip| * 8 < |gz| + |next_scale gskip|: a skip branch far larger than the layer's own output would amplify the
 * 16-bit rounding of z by that ratio).  next_scale / gskip may be NULL (1 / 0). */
int afcm_plane_dot_gated_ld(float* out, const void* a, const void* b, int32_t dtype, int64_t planes, int32_t h, int32_t w,
                            int32_t a_pitch, int32_t b_pitch, const int32_t* flags, int32_t slots, const float* out_scale,
                            const float* gz, const float* next_scale, const float* gskip, void* stream);

/* ------------------------------------------------------------------------------------------
 * The small-tensor half of modulated_conv2d (NET:41-57), fp32, forward and exact backward.  The reference runs it as
 * ~35 eager elementwise / reduction / matmul launches per layer and step; these are 1 + 1 + 1 + 2 launches.
 *   weight_norm:  w_hat[o] = w[o] * rsqrt(mean_{i,k} w[o]^2) (NET:42), wsq[o,i] = sum_k w_hat[o,i,k]^2, scale[o] kept for backward.
 *                 bwd: dw from g_hat (dL/dw_hat, may be NULL) and g_wsq (dL/dwsq, may be NULL).
 *   style_coefs:  s_hat = t * rsqrt(mean_{n,i} t^2) (NET:43, whole batch; r[0] keeps the factor),
 *                 d[n,o] = rsqrt(sum_i s_hat[n,i]^2 wsq[o,i] + 1e-8) (NET:50-52 factorised over the shared weights),
 *                 s_eff = s_hat * rsqrt(magnitude[0]) (input gain, NET:346,55-57; magnitude NULL: 1).
 *                 demodulate == 0 (ToRGB, NET:362): s_eff = t * gain only, d / wsq unused.
 *                 bwd: dt from g_s (dL/ds_eff, may be NULL) and g_d (dL/dd, may be NULL); NULL = zeros, both NULL: dt = 0.
 *                 g_wsq (may be NULL: not computed, the buffer is not touched) = dL/dwsq.
 *                 workspace: n*cin + n*cout + n*ceil(cin/64) floats.
 * ---------------------------------------------------------------------------------------- */
int afcm_weight_norm_fwd(float* w_hat, float* wsq, float* scale, const float* w, int32_t cout, int32_t cin, int32_t kk, void* stream);
int afcm_weight_norm_bwd(float* dw, const float* g_hat, const float* g_wsq, const float* w_hat, const float* scale, int32_t cout,
                         int32_t cin, int32_t kk, void* stream);
int afcm_style_coefs_fwd(float* s_eff, float* d, float* r, const float* t, const float* wsq, const float* magnitude, int32_t n, int32_t cin,
                         int32_t cout, int32_t demodulate, void* stream);
int afcm_style_coefs_bwd(float* dt, float* g_wsq, float* workspace, const float* g_s, const float* g_d, const float* t, const float* d,
                         const float* wsq, const float* magnitude, const float* r, int32_t n, int32_t cin, int32_t cout, int32_t demodulate,
                         void* stream);

/* Small-tensor tail of a fused layer's backward (afcm_amd/torch_utils/ops/fused_layer.py): from the per-tile plane sums of
 * dys that the transposed filtered_lrelu emitted (psum [n, cout, slots]) and two plane dot products, the gradients of the
 * bias (db [cout] = sum_n ps / d), of the next layer's styles (d_next [n, cout] = <g, z> / s_next) and of the demodulation
 * coefficients (d_out [n, cout] = (<dys, y> - b ps) / d^2).  Any of db / d_next / d_out may be NULL; out_scale, bias may be NULL. */
int afcm_layer_bwd_coefs(float* db, float* d_next, float* d_out, const float* psum, int32_t slots, const float* out_scale,
                         const float* next_scale, const float* bias, const float* gz, const float* dysy, int32_t n, int32_t cout,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * Generator update: gradient scale (1/world after the all-reduce), the NaN/Inf scrub of the gradients
 * (models/stylegan3_model.py:122-124,132-134: torch.nan_to_num(grad, nan=0, posinf=1e5, neginf=-1e5)) and the Adam step
 * (models/comodgan_model.py:19-20: torch.optim.Adam(lr, betas=(0, 0.99), eps=1e-8)) for EVERY parameter tensor in one
 * launch.  Replaces ~110 nan_to_num launches + torch's multi-tensor Adam passes; arithmetic follows torch's foreach
 * implementation operation by operation.  All tensors fp32.
 * `table` is a DEVICE array of n entries sorted by chunk0 (chunk0 = number of afcm_adam_chunk_elems()-sized chunks of
 * the tensors before this one); total_chunks = chunk0 + chunks of the last entry.  step_size = lr / (1 - beta1^t),
 * bias_correction2_sqrt = sqrt(1 - beta2^t), one_minus_beta* = 1 - beta*: all evaluated on the host in double as torch does
 * (1.f - 0.999f differs from (float)(1.0 - 0.999) by 5e-5 relative).
 * write_grad != 0 stores the scaled + scrubbed gradient back (what the reference leaves in .grad).
 * ---------------------------------------------------------------------------------------- */
typedef struct afcm_adam_entry {
    void*   p;        /* parameter, updated in place     */
    void*   g;        /* gradient                        */
    void*   m;        /* exp_avg, updated in place       */
    void*   v;        /* exp_avg_sq, updated in place    */
    int64_t numel;
    int64_t chunk0;
} afcm_adam_entry;
int32_t afcm_adam_chunk_elems(void);
int afcm_adam_multi(const afcm_adam_entry* table, int32_t n, int64_t total_chunks, float step_size, float beta1, float beta2,
                    float one_minus_beta1, float one_minus_beta2, float bias_correction2_sqrt, float eps, float grad_scale, int32_t scrub, float posinf, float neginf,
                    int32_t write_grad, void* stream);
/* afcm_adam_multi for a step captured into a hipGraph (r06): the step count is a DEVICE float (step_dev[0], advanced by one before the update)
 * and the bias corrections 1 - beta^t are formed on the device from it (in double), so a replayed launch applies the corrections of ITS step;
 * `lr` is the plain learning rate.  Same update arithmetic otherwise. */
int afcm_adam_multi_capturable(const afcm_adam_entry* table_dev, int32_t n, int64_t total_chunks, float* step_dev, float lr, float beta1, float beta2,
                               float eps, float grad_scale, int32_t scrub, float posinf, float neginf, int32_t write_grad, void* stream);
/* The same with lr and the betas in double: one_minus_beta* = (float)(1.0 - beta*) and the bias corrections come from the betas as given, as
 * in afcm_adam_multi, so m and v agree with it (and with torch) to the last bit or two.  The float entry point above can only form
 * 1.f - beta*, which moves exp_avg_sq by 1.7e-5 relative at beta2 = 0.999 and by 9e-7 at 0.99; it stays for its callers. */
int afcm_adam_multi_capturable_d(const afcm_adam_entry* table_dev, int32_t n, int64_t total_chunks, float* step_dev, double lr, double beta1, double beta2,
                                 float eps, float grad_scale, int32_t scrub, float posinf, float neginf, int32_t write_grad, void* stream);
/* The same with the learning rate on the DEVICE: the kernel reads lr_dev[0] (a double: slot 4 or 5 of the schedule block below), so one captured launch
 * follows a learning-rate schedule.  Everything else is afcm_adam_multi_capturable_d, bit for bit.  AFCM_E_INVALID: as there, and a null lr_dev. */
int afcm_adam_multi_capturable_lr(const afcm_adam_entry* table_dev, int32_t n, int64_t total_chunks, float* step_dev, const double* lr_dev, double beta1,
                                  double beta2, float eps, float grad_scale, int32_t scrub, float posinf, float neginf, int32_t write_grad, void* stream);

/* ------------------------------------------------------------------------------------------
 * The style affine layers of all SynthesisLayers at once (NET:349-352 `styles = self.affine(cat(w, global_w))`, FullyConnectedLayer
 * NET:69-104; ToRGB's extra factor NET:351 rides in alpha / beta): for layer l
 *     y_l[n][c] = alpha_l * sum_k x_l[n][k] W_l[c][k] + beta_l * b_l[c],   x_l[n] = [ w[n][w_index_l][0:kw] | g[n][0:kg] ]
 * and its gradients (dW_l = alpha_l dy_l^T x_l, db_l = beta_l sum_n dy_l, dws[n][l] / dg[n] = the two halves of alpha_l dy_l W_l, dg summed
 * over the layers).  All fp32, rows 16-byte aligned, kw and kg multiples of 4, kw + kg <= 1536, at most AFCM_AFFINE_MAX layers;
 * AFCM_E_NOKERNEL otherwise (the caller runs the layers one by one).  Replaces 15 cat + 15 GEMM launches forward and 30 GEMMs + 15
 * reductions + 14 accumulations backward by 1 + 3 launches.  No atomics: bit-reproducible.
 * y / dy / dweight / dbias are HOST arrays of `layers` device pointers ([n][cout_l], [cout_l][kw + kg], [cout_l]); a NULL dy_l means
 * zeros, NULL dweight_l / dbias_l are skipped, dweight == dbias == NULL skips the weight pass, dws == NULL the input pass.
 * dws: [n][layers][kw], dg: [n][kg]; workspace: afcm_affine_bank_workspace_bytes() bytes (input pass only).
 * ---------------------------------------------------------------------------------------- */
#define AFCM_AFFINE_MAX 16
typedef struct afcm_affine_bank {
    int32_t layers, n, kw, kg;
    int64_t w_stride_n, w_stride_l;               /* elements between batch rows / between latents of the ws tensor */
    const float* w;                               /* ws: w[n * w_stride_n + w_index_l * w_stride_l + k] */
    const float* g;                               /* [n][kg] or NULL when kg == 0 */
    const float* weight[AFCM_AFFINE_MAX];         /* [cout_l][kw + kg] */
    const float* bias[AFCM_AFFINE_MAX];           /* [cout_l] or NULL */
    int32_t cout[AFCM_AFFINE_MAX];
    int32_t w_index[AFCM_AFFINE_MAX];
    float alpha[AFCM_AFFINE_MAX], beta[AFCM_AFFINE_MAX];
} afcm_affine_bank;
int64_t afcm_affine_bank_workspace_bytes(const afcm_affine_bank* a);
int afcm_affine_bank_fwd(const afcm_affine_bank* a, float* const* y, void* stream);
int afcm_affine_bank_bwd(const afcm_affine_bank* a, const float* const* dy, float* const* dweight, float* const* dbias, float* dws, float* dg,
                         void* workspace, void* stream);

/* ----------------------------------------------------------------------------------------
 * Modulation bank: afcm_weight_norm_* and afcm_style_coefs_* (above) for a LIST of layers in 2 launches forward and 3 backward, whatever
 * the number of layers -- the decoder's 15 SynthesisLayers take 29 + 44 launches one by one (NET:41-57, 346-352 per layer).  Same
 * arithmetic, same kernels' bodies: bit-identical to the per-layer entry points.  Per layer, forward:
 *     demodulate != 0:  w [cout][cin][kk] -> w_hat (same shape), wsq [cout][cin], scale [cout];  t [n][cin] -> s_eff [n][cin], d [n][cout], r [1]
 *     demodulate == 0:  t -> s_eff, r (= 1); w / w_hat / wsq / scale / d unused (the caller convolves with w itself)
 * backward (g_hat / g_s / g_d: gradients of w_hat / s_eff / d, NULL = zeros): dw [cout][cin][kk] (NULL: skipped), dt [n][cin];
 * reads the forward's w_hat, wsq, scale, d, r, t, magnitude; workspace: afcm_modulation_bank_workspace_floats() floats per layer.
 * `layers` is a HOST array of `count` <= AFCM_MODULATION_MAX entries; it is copied into the kernel arguments.
 * ---------------------------------------------------------------------------------------- */
#define AFCM_MODULATION_MAX 16
typedef struct afcm_modulation_layer {
    int32_t cout, cin, kk, demodulate;
    const float* w;
    const float* t;
    const float* magnitude;                       /* [1] (input_gain = rsqrt(magnitude), NET:346) or NULL (gain 1) */
    float* w_hat;
    float* wsq;
    float* scale;
    float* s_eff;
    float* d;
    float* r;
    const float* g_hat;                           /* backward only from here on */
    const float* g_s;
    const float* g_d;
    float* dw;
    float* dt;
    float* workspace;
} afcm_modulation_layer;
int64_t afcm_modulation_bank_workspace_floats(int32_t n, int32_t cin, int32_t cout, int32_t demodulate);
int afcm_modulation_bank_fwd(const afcm_modulation_layer* layers, int32_t count, int32_t n, void* stream);
int afcm_modulation_bank_bwd(const afcm_modulation_layer* layers, int32_t count, int32_t n, void* stream);

/* ----------------------------------------------------------------------------------------
 * afcm_conv2d_pack_weights2 for a LIST of layers in one launch: every conv weight of the generator (the encoder's parameters, the
 * decoder's normalised weights from afcm_modulation_bank_fwd) exists before the first convolution of a step, so its 29 pack launches
 * (8 us each) become two (3x3 kernels; the 1x1 ToRGB keeps its own).  Same images bit for bit.  dst_fwd / dst_dgrad: as
 * afcm_conv2d_pack_weights2 (either may be NULL); `entries` is a HOST array of count <= AFCM_PACK_MAX, copied into the kernel arguments.
 * ---------------------------------------------------------------------------------------- */
#define AFCM_PACK_MAX 32
typedef struct afcm_pack_entry {
    void* dst_fwd;
    void* dst_dgrad;
    const float* w;                               /* [cout][cin][ks][ks] fp32 */
    int32_t cout, cin, rows_pad_fwd, rows_pad_dgrad;
} afcm_pack_entry;
int afcm_conv2d_pack_bank(const afcm_pack_entry* entries, int32_t count, int32_t dtype, int32_t ks, void* stream);

/* ----------------------------------------------------------------------------------------
 * fp32 convolution on the 16-bit matrix pipe by split operands.  The reference's fp32 conv is cuDNN's (SG3OPS/conv2d_gradfix.py:37-58
 * behind NET:25-64); gfx950 multiplies bf16 / f16 16x faster than fp32 (2.5 vs 0.157 PFLOP/s), so an fp32 operand v is written as a
 * sum of 16-bit parts, a = r16(v), b = r16(v - a), c = r16(v - a - b) (exact differences), and the product of two such sums is
 * accumulated term by term in the fp32 MFMA accumulators.
 *   float16, 2 parts, terms (b a') + (a b') + (a a'): 22 significand bits -- with both operands first multiplied by a power of two that
 *     brings their largest magnitude near 2^15 (so that b is a normal number wherever it matters; the callers fold the inverse into
 *     oscale), the result is as accurate as an fp32 dot product of the same length (3e-7 of the output scale at K = 4608).
 *   bfloat16 (no range limit, no scaling): 2 parts / the same 3 terms keep ~16 bits (4e-6 of the output scale), 3 parts / the six
 *     terms of order <= 2 keep all 24 (2e-7).
 *
 * afcm_amax_bits: out[0] = max(out[0], bit pattern of max |scale[plane] * x[plane, :]|) (scale NULL: 1) -- the caller zeroes the word
 *   (or passes one that already holds another tensor's bound to get a joint one).  Non-negative floats order like their bit patterns; a NaN
 *   ranks above inf.  The consumers below turn the word into the power of two g with g * bound in [2^14, 2^15) (g = 1 for a non-finite
 *   bound), on the device: no host round trip between the magnitude pass and the split.
 * afcm_split16: parts[k] (k < nparts in {2, 3}) = part k of g * scale[plane] * x[plane, :] (scale NULL: 1; bound NULL: g = 1, the
 *   bfloat16 case), dtype AFCM_F16 or AFCM_BF16, each a dense tensor of x's shape, part_stride ELEMENTS apart (>= planes * hw, a
 *   multiple of 4).  x on a 16-byte, parts on an 8-byte boundary (AFCM_E_INVALID otherwise); afcm_amax_bits takes x at any fp32 element.
 * afcm_conv2d_pack_split: the weight image of a split conv -- channel block t of [terms * cin16] holds part (term_wparts >> 4 t) & 15 of
 *   g * w ([cout][cin][3][3] fp32; g from `bound`, the weights' afcm_amax_bits word, or 1), in the layout of afcm_conv2d_pack_weights
 *   (mode 0: forward, rows = cout; mode 1: data gradient, transposed and flipped, rows = cin and cin16 is cout rounded up to 16):
 *   dst [terms * cin16 / 16][9][rows_pad][16].
 * afcm_conv2d_split: y[n][cout][P][Q] fp32 = oscale[n,o] / (g_a g_b) * sum_t conv(W_t, part_{x(t)}) + obias[o], 3x3, stride 1,
 *   0 <= pad <= 2, w even.  x_parts as written by afcm_split16 on the [n][cin][h][w] tensor (it must hold every part a term names); term
 *   t (t < terms <= 8) reads part (term_parts >> 4 t) & 15 and the channel block t of wpacked (afcm_conv2d_pack_split).  bound_a /
 *   bound_b: the two operands' bound words or NULL (g = 1).  x_parts on a 4-byte boundary (afcm_conv2d_ld's rule; afcm_split16 writes it on 8).
 * afcm_unscale: t[i] /= g_a g_b in place (the weight gradient summed from split parts of dy and x: afcm_conv2d_wgrad_ld per term).
 * afcm_plane_dot_parts: out[plane] = <sum_k parts[k][plane, :], b[plane, :]> / g, b fp32 -- afcm_plane_dot for a tensor that only exists as
 *   its split parts (the style gradient <x, dx> when the backward keeps x's parts instead of x).  parts on an 8-byte, b on a 16-byte
 *   boundary (AFCM_E_INVALID otherwise).
 * ---------------------------------------------------------------------------------------- */
int afcm_amax_bits(uint32_t* out, const float* x, int64_t planes, int32_t hw, const float* scale, void* stream);
int afcm_split16(void* parts, const float* x, const float* scale, const uint32_t* bound, int32_t dtype, int64_t planes, int32_t hw,
                 int32_t nparts, int64_t part_stride, void* stream);
int afcm_unscale(float* t, int64_t numel, const uint32_t* bound_a, const uint32_t* bound_b, void* stream);
int afcm_plane_dot_parts(float* out, const void* parts, int64_t part_stride, int32_t nparts, const float* b, int32_t dtype, int64_t planes,
                         int32_t hw, const uint32_t* bound, void* stream);
int afcm_conv2d_pack_split(void* dst, const float* w, const uint32_t* bound, int32_t dtype, int32_t cout, int32_t cin, int32_t mode,
                           int32_t rows_pad, int32_t terms, uint32_t term_wparts, void* stream);
int afcm_conv2d_split(float* y, const void* x_parts, const void* wpacked, const float* oscale, const float* obias, int32_t dtype, int32_t n,
                      int32_t cin, int32_t cout, int32_t h, int32_t w, int32_t pad, int32_t rows_pad, int32_t terms, uint32_t term_parts,
                      int64_t part_stride, const uint32_t* bound_a, const uint32_t* bound_b, void* stream);

/* ----------------------------------------------------------------------------------------
 * 3x3 convolution at stride 2 (the discriminator's down-sampling convs, CoModGAN/generator.py:613-692, after the blur): 16-bit x
 * [n][cin][h][w] (dense, w even), weights packed by afcm_conv2d_pack_weights_bk(mode 0, block_k = afcm_conv2d_block_k(dtype)) with rows_pad a multiple of 128, y
 * [n][cout][(h + 2 pad - 3) / 2 + 1][(w + 2 pad - 3) / 2 + 1] = the even rows / columns of afcm_conv2d's result (same 16-bit operands, fp32 accumulation; the two
 * kernels sum their K-chunks in a different order -- 16 channels here, 32 in the stride-1 kernel since r05 -- so results agree within 1 ulp
 * of the 16-bit output, not bit for bit: tests/test_gpu_conv.py holds both to a float64 strided conv), at a quarter of its MFMAs and without the full-resolution intermediate.  Forward only (the gradients are stride-1 convolutions with the
 * zero-stuffed dy: afcm_conv2d / afcm_conv2d_wgrad).  x on a 4-byte boundary (8-byte buffer loads at dword offsets, as in afcm_conv2d_ld; not
 * checked here), wpacked on 16 bytes.
 * ---------------------------------------------------------------------------------------- */
int afcm_conv2d_stride2(void* y, const void* x, const void* wpacked, int32_t dtype, int32_t n, int32_t cin, int32_t cout, int32_t h, int32_t w,
                        int32_t pad, int32_t rows_pad, void* stream);

/* AdaptiveAvgPool2d((4, 4)) of the bottleneck (NET:636,683) for planes that divide evenly (r06): y [planes][4][4] fp32 = block means of x
 * [planes][h][w] (16-bit or fp32; h % 4 == w % 4 == 0, else AFCM_E_NOKERNEL), and its backward dx = gy[block] / block size in x's type. */
int afcm_pool_blocks_fwd(float* y, const void* x, int32_t dtype, int64_t planes, int32_t h, int32_t w, void* stream);
int afcm_pool_blocks_bwd(void* dx, const float* gy, int32_t dtype, int64_t planes, int32_t h, int32_t w, void* stream);

/* The generator's L1 term `criterionL1(fake_B, real_B) * lambda_L1` (models/stylegan3_model.py:107; torch.nn.L1Loss, mean reduction) on fp32 tensors
 * (r06): partials[k] = weight / numel * sum over workgroup k's slice of |a - b| (blocks <= 1024; the caller adds them), and the gradient
 * ga = gout[0] * weight / numel * sign(a - b) with gout a DEVICE scalar (the incoming gradient of the loss). */
int afcm_l1_partials(float* partials, const float* a, const float* b, int64_t numel, int32_t blocks, float weight, void* stream);
int afcm_l1_grad(float* ga, const float* a, const float* b, const float* gout, int64_t numel, float weight, void* stream);

/* y[plane][:] = a[plane][:] + scale[plane] * b[plane][:] (r06), 16-bit tensors of ONE layout, hw elements per plane (hw % 8 == 0, 16-byte aligned
 * bases; else AFCM_E_NOKERNEL), scale [planes] fp32 or NULL (1): the accumulation autograd performs for an encoder feature map that feeds the next
 * encoder layer and a decoder layer's skip input (NET:371-377: `x = x + x_skip`), with the decoder's style factor folded in -- three passes
 * over the planes instead of scale_planes + add's five.  Sum in fp32, one rounding. */
int afcm_axpy_planes(void* y, const void* a, const void* b, const float* scale, int32_t dtype, int64_t planes, int32_t hw, void* stream);

/* ----------------------------------------------------------------------------------------
 * Equalised-learning-rate dense layers as one launch per layer and direction (r06): the mapping network's eight FCs and the
 * bottleneck's `fc_in` -- NET:69-104 (`FullyConnectedLayer.forward`: x @ (w * weight_gain).T + b * bias_gain, then bias_act, which the
 * reference runs as addmm / matmul + plugin `bias_act(x, b, xref, yref, dy, grad, dim, act, alpha, gain, clamp)`, SG3OPS/bias_act.cpp:32-90).
 * All tensors fp32, row-major: x [n][cin], w [cout][cin], b [cout] or NULL, y [n][cout].  act: 0 = linear, 1 = lrelu (slope 0.2, gain
 * sqrt 2: bias_act.py:21-31).  alpha = weight_gain, beta = bias_gain.  n <= 64, cin % 16 == 0 (and cout % 16 == 0 for the backward), else
 * AFCM_E_NOKERNEL (the host keeps the GEMM + bias_act composition).  Exact fp32 arithmetic (v_mfma_f32_16x16x4_f32 = an fmaf chain).
 *   afcm_fc_act_fwd:  y = act(alpha * x w^T + beta * b)
 *   afcm_fc_act_bwd:  with gp = gy * act'(y) (from the saved output y, as bias_act.cu:68-73): dx = alpha * gp w, dw = alpha * gp^T x,
 *                     db = beta * colsum(gp); any of dx / dw / db may be NULL (not wanted).
 *   x, w, y (forward) and gy, y (backward) on 16-byte boundaries: rows are read in 16-byte vectors (AFCM_E_INVALID otherwise).
 * afcm_mapping_input_fwd / _bwd: the mapping network's input stage (NET:143-150): x0 [n][zdim + wdim] = cat(normalize(z),
 * normalize(embed(c))) with normalize(v) = v * rsqrt(mean(v^2) + 1e-8) and embed = the linear FC c_dim -> w_dim (weight ew [wdim][cdim],
 * bias eb, gains alpha / beta); cdim = 0: x0 = normalize(z) only.  The backward returns the embedding layer's weight / bias gradients
 * from gx0 = dL/dx0 (z and c carry none).
 * ---------------------------------------------------------------------------------------- */
int afcm_fc_act_fwd(float* y, const float* x, const float* w, const float* b, int32_t n, int32_t cin, int32_t cout, float alpha, float beta,
                    int32_t act, void* stream);
int afcm_fc_act_bwd(float* dx, float* dw, float* db, const float* gy, const float* y, const float* x, const float* w, int32_t n, int32_t cin,
                    int32_t cout, float alpha, float beta, int32_t act, void* stream);
int afcm_mapping_input_fwd(float* x0, const float* z, const float* c, const float* ew, const float* eb, int32_t n, int32_t zdim, int32_t cdim,
                           int32_t wdim, float alpha, float beta, void* stream);
int64_t afcm_mapping_input_bwd_workspace_bytes(int32_t n, int32_t wdim);
/* workspace: afcm_mapping_input_bwd_workspace_bytes() of device memory whose FIRST WORD IS ZERO before the first launch (the kernel leaves it zero):
 * one row of the intermediate gradient per sample + the ticket by which the last workgroup to finish sums the rows (fixed order: reproducible). */
int afcm_mapping_input_bwd(float* dew, float* deb, const float* gx0, const float* c, const float* ew, const float* eb, int32_t n, int32_t zdim,
                           int32_t cdim, int32_t wdim, float alpha, float beta, void* workspace, void* stream);

/* ----------------------------------------------------------------------------------------
 * Validation metrics (r07): the per-plane statistics from which the host finishes the reference's PSNR / SSIM / MAE
 * (util/evaluation.py:6-127 behind the validation loop train.py:83-111; the reference computes them with scikit-image on host copies, one
 * slice at a time).  table [planes][8] float64, for plane p with r / t the loaded values of ref / test:
 *     0, 1  max r, min r          2, 3  max t, min t
 *     4     sum (r - t)^2         5     sum (r / max r - t / max t)^2   (psnr_2D's max-normalised pair, util/evaluation.py:31-37; one IEEE
 *                                       float64 divide per element, so a zero maximum gives inf / nan as numpy does and never traps)
 *     6     sum |r - t|           7     sum of the SSIM map over the (h - 6)(w - 6) windows that lie inside the plane (7 x 7 uniform window,
 *                                       sample covariance: ((2 ux uy + c1)(2 vxy + c2)) / ((ux^2 + uy^2 + c1)(vx + vy + c2)); the reference
 *                                       averages the cropped interior only, so no border mode exists)
 * ref / test: DEVICE images of dtype_ref / dtype_test (they may differ), element (p, y, x) at p * stride_plane + y * stride_row + x * stride_col
 * ELEMENTS: any strides, so the three axis-slicings of a volume and a row-pitched generator output are read in place.  unit_map = 1 maps every
 * loaded value from the network's range first, clip((float(x) + 1.0f) * 0.5f, 0, 1) in fp32 as two separate roundings (train.py:93-96).
 * PRECISION: this is the exception to "arithmetic is fp32" above -- after the load (and the map) every operation is float64.
 * Two phases on the stream, no host step between them: the planes' extrema (column 5 needs them), then the sums.  No atomics: tiles store
 * partials into `workspace` (afcm_plane_metrics_workspace_bytes() bytes, no initialisation needed) and one wave per plane adds them in a fixed
 * order, so the table is bit-identical from call to call.  h, w >= 7 (AFCM_E_INVALID otherwise); NaN inputs are not supported (the extrema
 * skip them).
 * ---------------------------------------------------------------------------------------- */
int64_t afcm_plane_metrics_workspace_bytes(int64_t planes, int32_t h, int32_t w);
int afcm_plane_metrics(double* table, const void* ref, const void* test, int32_t dtype_ref, int32_t dtype_test, int64_t planes, int32_t h, int32_t w,
                       int64_t ref_stride_plane, int64_t ref_stride_row, int64_t ref_stride_col, int64_t test_stride_plane, int64_t test_stride_row,
                       int64_t test_stride_col, int32_t unit_map, double c1, double c2, void* workspace, void* stream);

/* ----------------------------------------------------------------------------------------
 * Whole-volume inference (r08): the two ends of the reference's volume loop (evaluate.py -> StandardPredictor.__call__, models/predictor.py:106-202)
 * on the device -- the loader's item for a run of target slices, and the halo-cropped accumulation of a batch of predictions.  Both validate on
 * the host (AFCM_E_INVALID before any launch), launch on `stream`, never synchronise, use no atomics and form every volume offset in 64 bits.
 * ---------------------------------------------------------------------------------------- */
enum { AFCM_SRC_U8 = 0, AFCM_SRC_I16 = 1, AFCM_SRC_F32 = 2, AFCM_SRC_F64 = 3 };

/* data/cmsr_dataset.py:98-155 (__getitem__ of the test phase) behind transforms.py:250-275 (CropToFixed, centred) and :609-616 (Normalize), for the
 * target slices [first, first + count) of ONE source volume src [depth][hs][ws] of src_dtype (AFCM_SRC_*): element (z, y, x) at
 * z * src_stride_z + y * ws + x ELEMENTS (rows contiguous, any stride in z).  Writes a [count][k][h][w] of out_dtype (AFCM_F32 / F16 / BF16, contiguous)
 * and slice_idx [count] float32.
 *   planes   k = 4: source slices idx_a - t, idx_a, idx_a + t, idx_a + 2t with idx_a = (idx / t) * t, t = thickness >= 1; k = 1: slice idx itself.
 *            A position outside [0, depth - 1] is a plane of float64 zeros BEFORE normalisation.
 *   crop/pad per axis: want < have reads from offset (have - want) / 2; otherwise (want - have) / 2 pixels of padding before and the rest after.
 *            A padded pixel is a zero OF THE SOURCE DTYPE before normalisation.
 *   value    clip(2 * ((m - min) / (max - min)) - 1, -1, 1), each operation rounded on its own, in the type numpy gives the expression: float64 for
 *            u8 / i16 / f64 sources and for the zero planes, FLOAT32 for an f32 source (numpy keeps the array's type against Python scalars:
 *            min and max - min are rounded to float32 first).  Then one rounding to float32, and one more to a 16-bit out_dtype.
 *   label    slice_idx[i] = float32(idx - idx_a) / float32(thickness), one IEEE division (k = 1: idx_a = idx; the loader's "no thickness" is
 *            thickness = -1, which gives -0.0f).
 * One thread per 16 bytes of one output row, as in afcm_batch_assemble below.  AFCM_E_INVALID: null pointers, unknown dtypes, depth / hs / ws / h / w < 1, a slice
 * range outside [0, depth], k not 1 or 4, thickness 0 (or < 1 with k = 4), src_stride_z < 0, max_value <= min_value, more than 2^31 - 1 workgroups. */
int afcm_slice_assemble(void* a, float* slice_idx, const void* src, int32_t src_dtype, int32_t out_dtype, int32_t depth, int32_t hs, int32_t ws,
                        int64_t src_stride_z, int32_t first, int32_t count, int32_t k, int32_t thickness, int32_t h, int32_t w, double min_value,
                        double max_value, void* stream);

/* The per-batch body of StandardPredictor.__call__ (models/predictor.py:173-200) with remove_halo (:17-51): for the patches
 * [first, first + count) of the DEVICE table origins [table_len][3] int32 (z, y, x of each patch's first voxel), add sample i of
 * pred [count][channels][pd][ph][pw] (dtype AFCM_F32 / F16 / BF16, element (i, c, z, y, x) at i * stride_b + c * stride_c + z * stride_d + y * stride_h +
 * x * stride_w ELEMENTS: read as it lies) into map [map_channels][D][H][W] float32 and add 1 to mask (same shape, uint8, wraps at 256 as numpy's does).
 * prediction_channel >= 0: map_channels = 1 and that channel of pred is the source; -1: map channel c takes pred channel c (channels = map_channels).
 * Crop per axis, patch [o, o + p) in a volume of n with halo a: the covered voxels are [o + (o == 0 ? 0 : a), o + p == n ? n : o + p - a), read
 * from patch coordinate v - o -- EXCEPT on an interior stop side with a == 0, where the reference takes patch[..., :1] and numpy broadcasts it:
 * there every covered voxel reads patch coordinate 0 (models/predictor.py:34; reproduced, not repaired).
 * Gather form: one thread per (map channel, voxel) of the box [z0, z1) x [y0, y1) x [x0, x1) -- any box inside the volume that contains the
 * batch's patches; the host knows it from its own index list -- walks the patches in ASCENDING order and, for each that covers its voxel, does one
 * float32 add and one uint8 increment in registers, then stores once.  That is the host's order (sample by sample, batches in launch order), so
 * the map is bit-identical to the host's and the same from run to run.  A thread writes its own voxel only and reads pred only at coordinates
 * inside the patch, whatever the table holds.  AFCM_E_INVALID: null pointers, unknown dtype, a non-positive shape, patch larger than the volume,
 * negative halo or one above the patch extent, [first, first + count) outside the table, a box outside the volume or empty, prediction_channel outside [-1, channels),
 * channels != map_channels without a prediction channel, map_channels != 1 with one, more than 2^31 - 1 workgroups. */
int afcm_halo_accumulate(float* map, uint8_t* mask, const void* pred, int32_t dtype, int64_t stride_b, int64_t stride_c, int64_t stride_d,
                         int64_t stride_h, int64_t stride_w, int32_t channels, const int32_t* origins, int32_t table_len, int32_t first, int32_t count,
                         int32_t pd, int32_t ph, int32_t pw, int32_t halo_z, int32_t halo_y, int32_t halo_x, int32_t D, int32_t H, int32_t W,
                         int32_t map_channels, int32_t prediction_channel, int32_t z0, int32_t z1, int32_t y0, int32_t y1, int32_t x0, int32_t x1,
                         void* stream);

/* ----------------------------------------------------------------------------------------
 * Volume SSIM (r09): the sum of the 3-D SSIM map behind evaluate_3D (util/evaluation.py:123-127, evaluate.py:81), layer by layer.
 * layers [volumes][d - 6] float64: layers[v][z] is the sum of the SSIM map of volume v over the (h - 6)(w - 6) windows whose origin lies in
 * z-layer z -- uniform 7 x 7 x 7 window, means = sums / 343.0, sample covariance (factor 343 / 342), the formula of column 7 of
 * afcm_plane_metrics, valid windows only (the reference averages the cropped interior).  The host adds the d - 6 layers in index order and divides
 * by (d - 6)(h - 6)(w - 6); every other number of evaluate_3D comes from the axial table of afcm_plane_metrics.
 * ref / test: DEVICE volumes of dtype_ref / dtype_test (they may differ), element (v, z, y, x) at v * stride_volume + z * stride_z + y * stride_y +
 * x * stride_x ELEMENTS, offsets formed in 64 bits: any strides, read as they lie.  unit_map as in afcm_plane_metrics.  After the load every
 * operation is float64.  Every window sum is a direct sum of its terms (seven z-neighbours per voxel, seven columns, seven rows): no running sums.
 * Two launches on the stream: one workgroup per (volume, z origin, 16 x 64 tile of window origins) stores one partial into `workspace`
 * (afcm_volume_ssim_workspace_bytes() bytes, no initialisation needed), then one wave per (volume, z origin) adds that layer's partials in a fixed
 * order.  No atomics: the result is bit-identical from call to call.  A NaN voxel makes exactly the layers whose windows contain it NaN.
 * AFCM_E_INVALID: null pointers, unknown dtypes, volumes < 1, d / h / w < 7, more than 2^31 - 1 workgroups.
 * ---------------------------------------------------------------------------------------- */
int64_t afcm_volume_ssim_workspace_bytes(int64_t volumes, int32_t d, int32_t h, int32_t w);
int afcm_volume_ssim(double* layers, const void* ref, const void* test, int32_t dtype_ref, int32_t dtype_test, int64_t volumes, int32_t d, int32_t h,
                     int32_t w, int64_t ref_stride_volume, int64_t ref_stride_z, int64_t ref_stride_y, int64_t ref_stride_x,
                     int64_t test_stride_volume, int64_t test_stride_z, int64_t test_stride_y, int64_t test_stride_x, int32_t unit_map, double c1,
                     double c2, void* workspace, void* stream);

/* ----------------------------------------------------------------------------------------
 * Training batches (r10): data/cmsr_dataset.py:98-152 (__getitem__ of the train phase) for a batch of unrelated items, from a training set that
 * lives on the device.  pool: every volume, pool_elems elements of src_dtype (AFCM_SRC_*).  vols: DEVICE int64 [n_vols][4] = element offset into
 * pool, depth, hs, ws (rows contiguous, slices contiguous).  items: DEVICE int32 [n_items][4] = vol_a, vol_b, idx, thickness.  Sample i is table row
 * r = (cursor ? cursor[0] : 0) + first + i; cursor is a DEVICE scalar, so a captured graph moves through the table with afcm_cursor_advance.
 *   a [count][k][h][w]  the k planes of volume vol_a: k = 4: slices idx_a - t, idx_a, idx_a + t, idx_a + 2t with idx_a = (idx / t) * t; k = 1: slice idx.
 *                       A position outside [0, depth - 1] is a plane of float64 zeros BEFORE normalisation.
 *   b [count][1][h][w]  slice idx of volume vol_b.
 *   slice_idx [count]   float32(idx - idx_a) / float32(t) (k = 1: idx_a = idx; "no thickness" is t = -1, which gives -0.0f).
 * Crop / pad (per volume, from its own hs, ws), the normalisation in numpy's type for the source, the roundings and out_dtype are
 * afcm_slice_assemble's: both kernels call one body (csrc/volume_common.h); a and b are contiguous and both of out_dtype.
 * The tables cannot be checked at launch, so the KERNEL checks every row before it reads the pool.  An item is invalid when its row is outside
 * [0, n_items) (a cursor outside it included); vol_a or vol_b is outside [0, n_vols); a descriptor has a non-positive extent or an
 * [offset, offset + depth hs ws) outside [0, pool_elems); the two descriptors' (depth, hs, ws) differ; idx is outside [0, depth); thickness is 0, or
 * below 1 with k = 4.  An invalid item reads nothing from the pool, and every element of its a, its b and its label is NaN: no table content sends an
 * access outside the pool (the tables themselves must be n_vols and n_items rows long).
 * One launch covers a, b and the labels; a thread produces 16 bytes of one output row and stores them at once (element by element at the end of a row
 * whose width is no multiple of the run, and in rows that do not start on a 16-byte boundary).  No atomics, no LDS, no allocation, no synchronise:
 * both calls launch on `stream` and can be captured.  AFCM_E_INVALID: null pointers (only cursor may be null), unknown dtypes, count / h / w / n_vols /
 * n_items / pool_elems < 1, first < 0, k not 1 or 4, max_value <= min_value, more than 2^31 - 1 workgroups; afcm_cursor_advance: a null cursor.
 * ---------------------------------------------------------------------------------------- */
int afcm_batch_assemble(void* a, void* b, float* slice_idx, const void* pool, int64_t pool_elems, int32_t src_dtype, const int64_t* vols,
                        int32_t n_vols, const int32_t* items, int32_t n_items, const int64_t* cursor, int32_t first, int32_t count, int32_t k, int32_t h,
                        int32_t w, int32_t out_dtype, double min_value, double max_value, void* stream);
/* cursor[0] += by, one thread on `stream` */
int afcm_cursor_advance(int64_t* cursor, int64_t by, void* stream);

/* ----------------------------------------------------------------------------------------
 * Augmented training batches: afcm_batch_assemble with the train phase's geometric transforms (data/augment/transforms.py: RandomFlip 25-50,
 * RandomRotate90 53-80, RandomRotate 83-112 with axes [[2, 1]], order 0, mode 'reflect'; configs/defaults.py:62-76), applied in that order to the
 * cropped / padded, normalised [1, h, w] plane as Transformer.raw_transform() composes them (transforms.py:729-769).
 * augment: DEVICE float64 [n_items][8], row r of sample i the same r as the item row: (flip_h, flip_w, k, angle, c, s, off_y, off_x).  All planes of
 * an item, the target included, share the row.  For an item plane p0 [h, w] (afcm_batch_assemble's):
 *   p1 = p0 flipped along h if flip_h, along w if flip_w                                     (numpy.flip)
 *   p2 = numpy.rot90(p1, k), k in 0..3; odd k needs h == w
 *   p3[y][x] = p2[reflect(floor(iy + 0.5), h)][reflect(floor(ix + 0.5), w)] with, in float64 and every operation rounded on its own,
 *              iy = (y * c + x * s) + off_y,  ix = (y * (-s) + x * c) + off_x,
 *              reflect(i, n) = m < n ? m : 2n - 1 - m with m = i mod 2n taken non-negative (half-sample symmetric, any number of periods):
 *              scipy.ndimage.rotate(p2, angle, reshape=False, order=0, mode='reflect') when c = cosdg(angle), s = sindg(angle) and
 *              off = centre - [[c, s], [-s, c]] centre, centre = ((h - 1) / 2, (w - 1) / 2).  The HOST computes c, s and off; the kernel evaluates no
 *              trigonometric function and does not read `angle`, which is carried for the record.
 * The kernel walks the chain backwards per output pixel -- rotation, quarter turns, flips -- and reads the resulting item-plane coordinate through
 * afcm_batch_assemble's crop / pad / normalise: the reflect acts at the border of the [h, w] item plane, padding included.  A thick-slice plane
 * outside the volume stays the constant it is.  A row with no flip, k = 0, c = 1, s = 0 and both offsets 0 takes afcm_batch_assemble's own
 * contiguous path: the same bits.
 * The kernel checks the row as it checks the item row.  A row is valid when flip_h and flip_w are 0 or 1; k is 0, 1, 2 or 3, and even unless h == w;
 * c, s, off_y, off_x are finite with |c|, |s| <= 1 and |off_y|, |off_x| <= h + w, so that no coordinate leaves the int32 range before the reflect.
 * An item whose item row or parameter row is invalid reads nothing from the pool and is NaN throughout, label included.
 * Thread shape, stores, stream behaviour and AFCM_E_INVALID as afcm_batch_assemble; also AFCM_E_INVALID: a null augment, h + w > 2^28.
 * ---------------------------------------------------------------------------------------- */
int afcm_batch_assemble_aug(void* a, void* b, float* slice_idx, const void* pool, int64_t pool_elems, int32_t src_dtype, const int64_t* vols,
                            int32_t n_vols, const int32_t* items, int32_t n_items, const double* augment, const int64_t* cursor, int32_t first,
                            int32_t count, int32_t k, int32_t h, int32_t w, int32_t out_dtype, double min_value, double max_value, void* stream);

/* ----------------------------------------------------------------------------------------
 * Training batches with intensity augmentation: afcm_batch_assemble (augment null) or afcm_batch_assemble_aug (augment given) followed, per item, by
 * the train phase's intensity transforms (data/augment/transforms.py: RandomContrast 115-133, AdditiveGaussianNoise 619-630, AdditivePoissonNoise
 * 633-644; configs/defaults.py:83-88), in that order, after the geometric ones as the configuration lists them.
 * intensity: DEVICE float64 [n_items][36], row r of sample i the same r as the item row:
 *   0-2   contrast flag, alpha, mean      3-4  Gaussian flag, std      5-6  Poisson flag, lam (carried for the record)
 *   7-8   key_lo, key_hi, integers in [0, 2^32)      9  J      10-33  T_0 ... T_23, integer cut points      34-35  zero, not read
 * p: the float32 value the launch without the table produces, widened to double.  All arithmetic is float64, every operation rounded on its own:
 *   contrast   t = mean + alpha * (t - mean), then t < -1 ? -1 : (t > 1 ? 1 : t): a NaN stays
 *   Gaussian   t = t + std * z
 *   Poisson    t = t + (double)count
 * No clip after the noise (the reference has none).  The result is rounded once to float32, then to out_dtype as the other launches round.
 * The reference adds in float64 BEFORE its float32 cast; here the float32 item is widened back: pixels of an item that executed a transform may differ
 * from the reference's arithmetic by one float32 unit in the last place.
 * The field: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85; ten rounds; counter 0 / key 0 gives
 * 6627e8d5 e169c58d bc57ac4c 9b00dbd8).  Output pixel (y, x) of plane pl (0 ... k - 1: a; k: b) uses word x & 3 of
 * Philox(counter = (x >> 2, y, stream | P << 1, 0), key = (key_lo, key_hi)), stream 0: Gaussian, 1: Poisson, P = pl with independent_planes, else 0:
 * every plane of an item, the target and the zero planes outside the volume included, then receives the same field, as the reference's
 * equally seeded per-plane transformers give it.
 * z: Box-Muller per word pair, (w0, w1) -> lanes 0, 1 and (w2, w3) -> lanes 2, 3: u1 = (w0 + 0.5) 2^-32, u2 = w1 2^-32, r = sqrt(-2 LOG(u1)) with the
 * correctly rounded square root, z = r COS(2 pi u2), r SIN(2 pi u2), with
 *   LOG(x)      m, e = frexp(x); m < 0.7071067811865476: m *= 2, e -= 1; s = (m - 1) / (m + 1), s2 = s * s; acc = 1.0 / 23.0, then
 *               acc = acc * s2 + 1.0 / k for k = 21, 19 ... 1; e * 0.6931471805599453 + 2.0 * (s * acc)
 *   SIN, COS    t = u * 4, q = floor(t), r = (t - q) * 1.5707963267948966, r2 = r * r; a = 1 / 21!, then a = 1 / n! - r2 * a for n = 19, 17 ... 1, S = r * a;
 *               C = 1 / 20!, then C = 1 / n! - r2 * C for n = 18, 16 ... 0; (sin, cos) = (S, C), (C, -S), (-S, -C), (-C, S) for q = 0, 1, 2, 3
 * IEEE + - x / sqrt floor only, so afcm_amd/augment_intensity.py evaluates the same operations in numpy and gets the same bits.
 * count: the number of j < J with word >= T_j.  The host fills T_j = min(floor(F(j) 2^32), 2^32), F the running float64 sum of p_0 = exp(-lam),
 * p_j = p_{j-1} lam / j, up to the first T_j >= 2^32 - 1 (lam <= 4 needs 23).
 * The kernel checks the row as it checks the item row and the augment row, before it reads the pool.  A row is valid when the three flags are 0 or
 * 1; alpha and mean are finite; std is finite and >= 0; key_lo, key_hi are whole numbers in [0, 2^32 - 1]; J is a whole number in [0, 24]; T_j is a
 * whole number in [0, 2^32] for j < J.  A NaN fails every comparison.  An item with an invalid row of any table reads nothing from the pool and is NaN
 * throughout, label included.  A row with all three flags 0 gives the bits of the launch without the table, and pays for no Philox call.
 * Thread shape, stores, stream behaviour and AFCM_E_INVALID as afcm_batch_assemble(_aug); augment may be null; also AFCM_E_INVALID: a null
 * intensity, independent_planes not 0 or 1.
 * ---------------------------------------------------------------------------------------- */
int afcm_batch_assemble_noise(void* a, void* b, float* slice_idx, const void* pool, int64_t pool_elems, int32_t src_dtype, const int64_t* vols,
                              int32_t n_vols, const int32_t* items, int32_t n_items, const double* augment, const double* intensity,
                              int32_t independent_planes, const int64_t* cursor, int32_t first, int32_t count, int32_t k, int32_t h, int32_t w,
                              int32_t out_dtype, double min_value, double max_value, void* stream);

/* ----------------------------------------------------------------------------------------
 * Training batches with an elastic deformation: the reference's ElasticDeformation (data/augment/transforms.py:138-191; configs/defaults.py:77-79,
 * spline_order 3, alpha 2000, sigma 50, execution_probability 0.1) on every [1, h, w] plane of the item, the target included, all planes with one
 * deformation (the reference's equally seeded per-plane transformers).  With depth 1 the z displacement has no effect, so the statement is 2-D.
 * Position in the chain: after the geometric transforms (augment, may be null), before the intensity transforms (intensity, may be null).  The
 * reference lists ElasticDeformation after RandomRotate and before the noise transforms; RandomContrast is not in defaults.py, and this project places
 * it AFTER the deformation -- its clip to [-1, 1] does not commute with the overshoot of a cubic spline.
 * elastic: DEVICE float64 [n_items][4], row r of sample i the same r as the item row: (flag, alpha, key_lo, key_hi).
 * smooth_h [h][h], smooth_w [w][w]: DEVICE float64, the Gaussian filter of the reference folded over its 'reflect' boundary by the HOST
 * (afcm_amd/augment_elastic.py: smoothing_operator); the kernels evaluate no exponential.
 * p: the float32 plane the launch without the elastic and intensity tables produces.  All arithmetic is float64, every operation rounded on its own:
 *   fields   Fy, Fx [h][w]: the Box-Muller normals of afcm_batch_assemble_noise from Philox(counter (x >> 2, y, 0, 1) for Fy, (x >> 2, y, 0, 2) for
 *            Fx, key (key_lo, key_hi)), lane x & 3.  Counter word 3 is 0 in the intensity streams, so the fields collide with neither.
 *   smooth   T[i][x] = sum over m = 0 ... h - 1 ascending of smooth_h[i][m] * Fy[m][x]; S[y][j] = sum over m = 0 ... w - 1 ascending of
 *            T[y][m] * smooth_w[j][m]; each sum starts at +0.0 and is acc = acc + product.  dy = alpha * S; dx likewise from Fx.
 *   coords   cy = (double)y + dy[y][x], cx = (double)x + dx[y][x].  A coordinate that fails |c| <= 2^30 (a NaN fails) reads nothing: the pixel is
 *            NaN.  The test comes before any conversion to an integer.
 *   order 0  p[reflect(floor(cy + 0.5), h)][reflect(floor(cx + 0.5), w)], reflect as in afcm_batch_assemble_aug.
 *   order 1  f = floor(c), t = c - f, weights (1 - t, t) at reflect(f), reflect(f + 1).
 *   order 3  f = floor(c), t = c - f, u = 1 - t, weights ((u u) u) / 6, (((t t)(t - 2)) 3 + 4) / 6, (((u u)(u - 2)) 3 + 4) / 6, ((t t) t) / 6 at
 *            reflect(f - 1 + l), l = 0 ... 3, on the coefficient plane C instead of p.
 *   sum      per tap row a: r_a = wx_0 v_0, then r_a = r_a + wx_l v_l for l ascending; out = wy_0 r_0, then out = out + wy_a r_a for a ascending.
 *   C        the cubic B-spline coefficients with the half-sample symmetric boundary, along y (every column), then along x (every row).  For a
 *            line q[0 ... n) and z = -0.2679491924311227 (sqrt(3) - 2):  s = q[reflect(-40)]; s = q[reflect(-k)] + z * s for k = 39 ... 1;
 *            c+[0] = q[0] + z * s; c+[k] = q[k] + z * c+[k - 1];  c[n - 1] = (z / (z - 1)) * c+[n - 1]; c[k] = z * (c[k + 1] - c+[k]) for
 *            k = n - 2 ... 0; the line becomes c[k] * 6.  This is the exact interpolating spline at every length (scipy's own 'reflect'
 *            prefilter is not below about n = 16; from there the two agree to rounding).
 * The result is rounded once to float32; the intensity transforms, where a table is given, then act on that float32 value as
 * afcm_batch_assemble_noise states; then one rounding to out_dtype.  The reference interpolates the float64 plane BEFORE its float32 cast; here
 * the float32 item is widened back: a deformed pixel may differ from the reference's arithmetic by one float32 unit in the last place.
 * IEEE + - x / sqrt floor only, so afcm_amd/augment_elastic.py evaluates the same operations in numpy and gets the same bits.  No atomics.
 * A row is valid when flag is 0 or 1, alpha is finite with |alpha| <= 2^20, key_lo and key_hi are whole numbers in [0, 2^32 - 1].  An item with an
 * invalid row of any table reads nothing from the pool and is NaN throughout, label included.  An item whose flag is 0 has the bits of the launch
 * without the table, and every launch below skips it.
 * Launches on `stream`, a fixed number per call whatever the flags are (afcm_elastic_plan: 6, or 8 with order 3), no allocation, no synchronise:
 * the item rows' check, the float32 item into the workspace (afcm_batch_assemble / _aug's kernel), the fields, the two smoothing passes (16 x 64
 * output tiles, operator rows staged in LDS), the two prefilter passes (order 3; one lane per line, rows through an LDS transpose), the gather.
 * workspace: DEVICE, on a multiple of 256 bytes, at least the workspace_bytes afcm_elastic_plan gives for (count, k, h, w, order); no
 * initialisation needed, nothing is kept between calls.
 * AFCM_E_INVALID as afcm_batch_assemble_noise (augment and intensity may each be null); also a null elastic, operator or workspace, a workspace
 * that is too small or misaligned, an order outside {0, 1, 3}, count above 32767, h or w above 32768.
 * ---------------------------------------------------------------------------------------- */
int afcm_elastic_plan(int32_t count, int32_t k, int32_t h, int32_t w, int32_t order, int64_t* workspace_bytes, int32_t* launches);
int afcm_batch_assemble_elastic(void* a, void* b, float* slice_idx, const void* pool, int64_t pool_elems, int32_t src_dtype, const int64_t* vols,
                                int32_t n_vols, const int32_t* items, int32_t n_items, const double* augment, const double* intensity,
                                int32_t independent_planes, const double* elastic, const double* smooth_h, const double* smooth_w,
                                int32_t spline_order, void* workspace, int64_t workspace_bytes, const int64_t* cursor, int32_t first, int32_t count,
                                int32_t k, int32_t h, int32_t w, int32_t out_dtype, double min_value, double max_value, void* stream);

/* ----------------------------------------------------------------------------------------
 * Training batches with a Gaussian blur: the reference's GaussianBlur3D (data/augment/transforms.py:716-726; configs/defaults.py:80-82, sigma
 * [0.1, 2], execution_probability 0.5) on every [1, h, w] plane of the item, every plane with its own decision and sigma (the reference draws per
 * plane).  Its filter is skimage.filters.gaussian(x, sigma), by skimage's documentation scipy.ndimage.gaussian_filter(x, sigma, mode='nearest',
 * truncate=4.0) on a float array; the statement below equals that scipy call bit for bit (parity with skimage's own function is not pinned).
 * Position in the chain: after the geometric transforms (augment, may be null) and the elastic deformation (elastic, may be null; with it
 * smooth_h, smooth_w and spline_order as afcm_batch_assemble_elastic takes them), before the intensity transforms (intensity, may be null).
 * blur: DEVICE float64 [n_items][20 (k + 1)], row r of sample i the same r as the item row; 20 doubles per plane, the k planes of A, then B:
 * (flag, sigma, radius, w_0 ... w_16).  The weights are made by the HOST (afcm_amd/augment_blur.py: gaussian_weights): radius = int(4 sigma + 0.5),
 * phi_x = exp(-0.5 / (sigma sigma) x^2) for x = -radius ... radius, over their sum, w_j = phi at +j; the kernels evaluate no exponential and do
 * not read sigma beyond its check.
 * p: the float32 plane the launch without the blur and intensity tables produces.  All arithmetic is float64, every product and every addition
 * rounded on its own, three passes in axis order -- depth (a line of one element), y, x -- each per output element i of a line v[0 ... n):
 *   t = v[i] w_0;  t = t + (v[clamp(i - j, 0, n - 1)] + v[clamp(i + j, 0, n - 1)]) w_j for j = radius, radius - 1, ..., 1
 * so the depth pass is t = p w_0; t = t + (p + p) w_j.  The result is rounded once to float32; the intensity transforms, where a table is given,
 * then act on that float32 value as afcm_batch_assemble_noise states; then one rounding to out_dtype.  The reference filters the float64 plane
 * BEFORE its float32 cast; here the float32 item is widened back: a blurred pixel may differ from the reference's arithmetic by one float32 unit
 * in the last place.  afcm_amd/augment_blur.py evaluates the same operations in numpy and gets the same bits.  No atomics.
 * A plane record is valid when flag is 0 or 1, sigma is finite and > 0, radius is a whole number in [0, 16] and w_0 ... w_16 are finite; a row
 * when all its records are.  An item with an invalid row of any table reads nothing from the pool and is NaN throughout, label included.  A plane
 * whose flag is 0 has the bits of the launch without the table.
 * Launches on `stream`, a fixed number per call whatever the flags are (afcm_blur_plan: 4, or 3 + those of afcm_elastic_plan with an elastic
 * table), no allocation, no synchronise: the float32 item into the workspace (afcm_batch_assemble / _aug's kernel, or the launches of
 * afcm_batch_assemble_elastic with the workspace as their output), the rows' check, the depth and y pass (32 x 64 output tiles, the rows and their
 * halo staged in LDS, float64 out), the x pass with the rest of the chain (16 x 64 output tiles).  afcm_blur_tiles gives those four extents.
 * workspace: DEVICE, on a multiple of 256 bytes, at least the workspace_bytes afcm_blur_plan gives for (count, k, h, w, elastic_order), where
 * elastic_order is the spline order of the elastic table or -1 without one; no initialisation needed, nothing is kept between calls.
 * AFCM_E_INVALID as afcm_batch_assemble_elastic where an elastic table is given and as afcm_batch_assemble_noise otherwise; also a null blur table
 * or workspace, a workspace that is too small or misaligned, count above 32767, h or w above 32768.
 * ---------------------------------------------------------------------------------------- */
int afcm_blur_plan(int32_t count, int32_t k, int32_t h, int32_t w, int32_t elastic_order, int64_t* workspace_bytes, int32_t* launches);
void afcm_blur_tiles(int32_t* rows_tile_h, int32_t* rows_tile_w, int32_t* cols_tile_h, int32_t* cols_tile_w);
int afcm_batch_assemble_blur(void* a, void* b, float* slice_idx, const void* pool, int64_t pool_elems, int32_t src_dtype, const int64_t* vols,
                             int32_t n_vols, const int32_t* items, int32_t n_items, const double* augment, const double* intensity,
                             int32_t independent_planes, const double* elastic, const double* smooth_h, const double* smooth_w, int32_t spline_order,
                             const double* blur, void* workspace, int64_t workspace_bytes, const int64_t* cursor, int32_t first, int32_t count,
                             int32_t k, int32_t h, int32_t w, int32_t out_dtype, double min_value, double max_value, void* stream);

/* ----------------------------------------------------------------------------------------
 * The training loop's time-dependent scalars on the device (r11), so that ONE captured graph stays right for a whole run.
 * The schedule block is a DEVICE array of 8 doubles:
 *   [0] total_iters  images seen: the reference's total_iters / cur_nimg (train.py:50-53), exact in a double
 *   [1] blur_sigma   models/stylegan3_model.py:115-116: max(1 - cur_nimg / (blur_fade_kimg * 1e3), 0) * blur_init_sigma, 0 when blur_fade_kimg <= 0
 *   [2] blur_radius  floor(3 * blur_sigma) (models/stylegan3_model.py:97-98)
 *   [3] ema_beta     train.py:67-77: 0.5 ** (batch / max(ema_nimg, 1e-8)), ema_nimg = ema_kimgs * 1000, with a ramp min(ema_nimg, total_iters * ramp)
 *   [4] lr_G  [5] lr_D   written by the host only (models/utils.py:43-69: one scheduler step per epoch, train.py:44)
 *   [6] [7]          spare, kept zero
 * afcm_schedule_advance: one thread; total_iters += batch, then slots 1-3 from the new total_iters in that order.  ema_ramp < 0: no ramp.  Slots 1 and 2
 * use + - x / floor max in double only (the library is built without contraction): bit-equal to the Python expressions; pow may differ from the
 * host's by rounding.  AFCM_E_INVALID: a null block, batch < 1.
 *
 * afcm_gauss_blur: the blur of models/stylegan3_model.py:24-30, 97-103 on fp32 planes x [planes][h][w] -> y, same size: f = exp2(-(i / sigma)^2) for i in
 * [-r, r], r = floor(3 sigma), normalised by its sum (taps formed in fp32 in the kernel: the division by (float)sigma, exp2f, a sum), applied along x
 * into `scratch` (planes * h * w floats, the caller's) and then along y, zero padding r on each side (upfirdn2d.filter2d with a 1-D filter).  block
 * == NULL: sigma is the argument; otherwise sigma and radius are slots 1 and 2 of the block when the kernels RUN and the argument is ignored.  The
 * two launches' geometry depends on neither.  Radius 0: y = x bit for bit, nothing is divided by sigma.  A block radius outside
 * [0, afcm_gauss_blur_rmax()] cannot be raised from the device: every element of y is NaN.  A NaN input reaches its (2r + 1)^2 window and nothing else.
 * No atomics.  scratch may be null where the host sigma has radius 0.  AFCM_E_INVALID: null y / x / scratch or two of them equal, extents < 1, a host sigma that is negative, NaN or whose radius exceeds
 * the cap, more than 2^31 - 1 workgroups.
 *
 * afcm_ema_multi: train.py:74-77 for every tensor of the generator in one launch.  `table` is a DEVICE array of n rows sorted by chunk0, chunks of
 * afcm_adam_chunk_elems() units as in afcm_adam_multi.  AFCM_EMA_LERP: dst = p_ema, src = p, fp32, numel elements: p_ema <- p.lerp(p_ema, beta) in
 * torch's form -- w = (float)beta, d = p_ema - p: w < 0.5f ? fmaf(w, d, p) : fmaf(-d, 1.f - w, p_ema).  AFCM_EMA_COPY: numel BYTES from src to dst (a
 * buffer of any dtype).  16-byte accesses when both pointers of a row are 16-byte aligned, element by element otherwise and at a row's tail.  beta is
 * the argument or, with a block, its slot 3 when the kernel runs.  AFCM_E_INVALID: an empty table, total_chunks outside [1, 2^31), a host beta
 * outside [0, 1].
 * ---------------------------------------------------------------------------------------- */
#define AFCM_SCHEDULE_SLOTS 8
#define AFCM_EMA_LERP 0
#define AFCM_EMA_COPY 1
typedef struct afcm_ema_entry {
    void*       dst;
    const void* src;
    int64_t     numel;     /* elements (AFCM_EMA_LERP) or bytes (AFCM_EMA_COPY), > 0 */
    int64_t     chunk0;
    int32_t     kind;
    int32_t     reserved;
} afcm_ema_entry;
int afcm_schedule_advance(double* block, int64_t batch, double blur_init_sigma, double blur_fade_kimg, double ema_kimgs, double ema_ramp, void* stream);
int32_t afcm_gauss_blur_rmax(void);
int afcm_gauss_blur(float* y, const float* x, float* scratch, int64_t planes, int32_t h, int32_t w, double sigma, const double* block, void* stream);
int afcm_ema_multi(const afcm_ema_entry* table, int32_t n, int64_t total_chunks, double beta, const double* block, void* stream);

/* ----------------------------------------------------------------------------------------
 * Intensity rescaling: rescale_intensity of data/prepare_h5.py:9-26 with the around / clip / uint8 of its caller (:38-41; evaluate.py:23-40 repeats
 * it) for one volume [depth][h][w] of src_dtype (AFCM_SRC_*) that lives on the device: element (z, y, x) at z * src_stride_z + y * w + x ELEMENTS
 * (rows contiguous, any stride in z, any element offset in the pointer).  N = depth * h * w < 2^31.
 *   foreground   v > 0, decided from the bit pattern: NaN, -inf, -0.0, 0 and negatives are background, +inf and positive denormals foreground,
 *                whatever the denormal mode.  n = the foreground count.
 *   percentiles  for q in (q_lo, q_hi), FRACTIONS in [0, 1] (the percentile / 100, formed by the caller): vi = q * (n - 1), i = floor(vi), g = vi - i,
 *                a = s[i], b = s[min(i + 1, n - 1)] of the sorted foreground s widened exactly to double, d = b - a, p = g >= 0.5 ? b - d * (1 - g) :
 *                a + d * g -- numpy's `linear` method with its _lerp; every operation double and rounded on its own.
 *   map          foreground: clip(rint(((double)v - lo) / (hi - lo) * 255), 1, 255), rint to even, a NaN result (hi == lo at v == lo, inf / inf)
 *                is 1; background: 0.
 * Arithmetic is float64 for EVERY source type.  numpy computes a float32 volume in float32, so for float32 sources the reference's grey level can
 * differ by one at a few voxels in 10^5; for uint8 / int16 / float64 sources the two agree bit for bit.
 * out: uint8 [depth][h][w], contiguous.  stats: DEVICE double[3] = lo, hi, (double)n; n == 0: out is all zeros, lo = hi = NaN.
 * The four order statistics (i and i + 1 of both percentiles) come from ONE most-significant-digit-first radix select over the raw bit patterns
 * (positive values order as their bits do): afcm_rescale_plan's `passes` digits, each pass a histogram launch -- every workgroup counts its share in
 * LDS (integer adds; in the first pass of 8-bit digits each wave has a histogram of its own, since a float's top digit is its exponent) and stores
 * the counts into its own slot of `workspace` -- and a one-workgroup launch that adds the slots, scans, picks each rank's bin and carries prefix and
 * residual rank forward.  n is the first pass's total and the ranks are formed from it on the device.  Then the map: 16 voxels per thread, 16-byte
 * loads where the run lies inside one slice on a 16-byte boundary and a 16-byte store where the output run does, element by element otherwise.
 * No global atomic, no host read, no allocation, no synchronise; `workspace` needs afcm_rescale_workspace_bytes() bytes, 8-byte aligned, and no
 * initialisation.  Bit-identical from call to call.
 * afcm_rescale_plan (pure host): plan[0] = histogram workgroups, plan[1] = voxels of one workgroup per round of the grid (workgroup g counts voxels
 * [(r * plan[0] + g) * plan[1], + plan[1]) in round r), plan[2] = passes, plan[3 + p] = bits of digit p for p < passes (most significant first; the
 * rest 0): 11 values.  afcm_rescale_workspace_bytes (pure host): 0 for arguments afcm_rescale_plan refuses.
 * AFCM_E_INVALID: null pointers, an unknown dtype, extents < 1, N >= 2^31, a negative z stride, fractions outside 0 <= q_lo <= q_hi <= 1 (NaN
 * included), a workspace or stats pointer that is not 8-byte aligned.
 * ---------------------------------------------------------------------------------------- */
int afcm_rescale_plan(int64_t n, int32_t src_dtype, int32_t* plan);
int64_t afcm_rescale_workspace_bytes(int64_t n, int32_t src_dtype);
int afcm_rescale_intensity(uint8_t* out, double* stats, void* workspace, const void* volume, int32_t src_dtype, int32_t depth, int32_t h, int32_t w,
                           int64_t src_stride_z, double q_lo, double q_hi, void* stream);

/* ----------------------------------------------------------------------------------------
 * Percentile-clip normalisation: StandardNIIDataset.__percentile_clip of data/cmsrnii_dataset.py:79-114 with its caller's (x * 255).astype('uint8')
 * (`dataset_mode: cmsrnii`), for volumes that live on the device.  Two entry points: afcm_percentile_bounds takes the two bounds from a reference
 * volume r, afcm_clip_normalize maps a volume x with them; x and r may differ in shape and dtype (the reference's reference_tensor; r = x by default).
 * Both volumes are laid out as afcm_rescale_intensity's: [depth][h][w] of AFCM_SRC_U8 / I16 / F32 / F64, rows contiguous, any stride in z, any
 * element offset, fewer than 2^31 voxels.
 *   bounds       EVERY voxel of r takes part -- zeros, negatives, +-inf, denormals and -0.0.  n = depth * h * w.  For q in (q_lo, q_hi), FRACTIONS
 *                in [0, 1]: vi = q * (n - 1), i = floor(vi), g = vi - i, a = s[i], b = s[min(i + 1, n - 1)] of the sorted voxels s widened exactly to
 *                double, d = b - a, p = g >= 0.5 ? b - d * (1 - g) : a + d * g -- numpy's `linear` method with its _lerp, every operation double and
 *                rounded on its own.
 *   NaN          if r holds any NaN, lo and hi are both NaN (numpy partitions NaNs to the end and checks the last element).
 *   zeros        -0.0 and +0.0 are one key; which of them a bound carries is not pinned (they are equal numerically, and the map gives equal bytes).
 *   strictly_positive   non-zero: lo < 0 becomes 0.0 (a NaN fails the comparison and stays).
 *   map          level = (uint8) trunc(((min(max(v, lo), hi) - lo) / (hi - lo)) * 255.0), double for every source type, each operation rounded on
 *                its own; min / max as numpy's (a NaN voxel stays NaN; lo > hi, which strictly_positive over an all-negative r gives, yields hi).
 *                A NaN result -- NaN bounds, a NaN voxel, hi == lo, inf / inf -- becomes 0.  The reference leaves that cast to numpy, where it is 0
 *                on x86-64 but undefined in C: it is this library's statement, not a pin.
 * The reference function agrees with this statement bit for bit for all four source dtypes wherever numpy returns float64 bounds for a list q (numpy
 * 2.x does, float32 arrays included).  Where it can differ: numpy forms b - a of two neighbouring order statistics in the array's own type before
 * it widens -- in int16 that wraps when they are more than 32767 apart, in float32 it rounds when they are far apart -- and here both are widened
 * first.
 * stats: DEVICE double[4] = lo, hi, (double)n, (double)(number of NaNs in r), written by afcm_percentile_bounds and read by afcm_clip_normalize when
 * its kernel runs.  out: uint8 [depth][h][w], contiguous.
 * The select is afcm_rescale_intensity's, on keys that order values of either sign: a float's bits with -0.0 mapped to +0.0, then the sign bit
 * flipped for non-negatives and every bit inverted for negatives; int16 biased by 32768; uint8 as it is.  NaNs get no key: the first histogram pass
 * counts them apart, in one more word of each workgroup's slot, and the scan adds them.  All digits are 8 bits: uint8 one pass, int16 two (one pass
 * of 2^16 bins would need 256 KB of LDS), float32 four, float64 eight.  afcm_percentile_plan / afcm_percentile_workspace_bytes: as
 * afcm_rescale_plan / afcm_rescale_workspace_bytes (pure host, the same 11 values).  The map has afcm_rescale_intensity's run structure.
 * No global atomic, no host read, no allocation, no synchronise, no scratch; `workspace` needs no initialisation.  Bit-identical from call to call.
 * AFCM_E_INVALID: null pointers, an unknown dtype, extents < 1, N >= 2^31, a negative z stride, fractions outside 0 <= q_lo <= q_hi <= 1 (NaN
 * included), a workspace or stats pointer that is not 8-byte aligned.
 * ---------------------------------------------------------------------------------------- */
int afcm_percentile_plan(int64_t n, int32_t src_dtype, int32_t* plan);
int64_t afcm_percentile_workspace_bytes(int64_t n, int32_t src_dtype);
int afcm_percentile_bounds(double* stats, void* workspace, const void* volume, int32_t src_dtype, int32_t depth, int32_t h, int32_t w,
                           int64_t src_stride_z, double q_lo, double q_hi, int32_t strictly_positive, void* stream);
int afcm_clip_normalize(uint8_t* out, const double* stats, const void* volume, int32_t src_dtype, int32_t depth, int32_t h, int32_t w,
                        int64_t src_stride_z, void* stream);

/* ----------------------------------------------------------------------------------------
 * afcm_group_expand: whole per-sample blocks of several tensors repeated by a DEVICE index, in one launch -- the encoder state of G conditioning
 * images handed to a decoder batch of `batch` samples (SynthesisNetwork.decode with `groups`).  For every row k of the table and every sample b
 *   dst_k[b * block_bytes, + block_bytes) = src_k[groups[b] * block_bytes, + block_bytes)     byte for byte.
 * A block is what lies between two samples of the tensor as allocated: C * H * pitch elements of a row-pitched tensor, padding included, so the
 * output has the source's layout and finite padding wherever the source's producer left it finite.
 * `table_dev` is a DEVICE array of n rows sorted by chunk0, as in afcm_ema_multi; a chunk is afcm_group_chunk_bytes() bytes of ONE block, so row k owns
 * batch * ceil(block_bytes / chunk bytes) chunks starting at chunk0 (sample-major).  `table_host` is the host image of the same rows: the entry point
 * checks it and sizes the grid from it, the kernel reads table_dev only.  `groups` (device, int32 [batch]) is read when the kernel RUNS; nothing is read
 * back.  An index outside [0, groups_k) cannot be raised from the device: that sample reads nothing, and every element of its block in every output is
 * NaN (afcm_batch_assemble's convention; kind says which NaN: AFCM_GROUP_2B stores 0x7FFF, a NaN in fp16 and in bf16, AFCM_GROUP_4B 0x7FC00000).
 * 16 bytes per lane, four in flight, where the source block and the destination block start on 16-byte boundaries; element by element (kind bytes)
 * otherwise and in the last block_bytes % 16 bytes.  Offsets are formed in 64 bits.  No atomics, no LDS, no allocation, no synchronise: capturable.
 * AFCM_E_INVALID: a null table, groups, src or dst; n < 1; batch < 1; a row with groups < 1, a block size of 0 or not a multiple of kind, an unknown
 * kind or a chunk0 that is not the running total of the rows before it; more than 2^31 - 1 workgroups.
 * ---------------------------------------------------------------------------------------- */
#define AFCM_GROUP_2B 2
#define AFCM_GROUP_4B 4
typedef struct afcm_group_entry {
    void*       dst;          /* [batch] blocks */
    const void* src;          /* [groups] blocks */
    int64_t     block_bytes;
    int64_t     chunk0;
    int32_t     groups;       /* G of this tensor */
    int32_t     kind;         /* AFCM_GROUP_2B / AFCM_GROUP_4B: the element size */
} afcm_group_entry;
int32_t afcm_group_chunk_bytes(void);
int afcm_group_expand(const afcm_group_entry* table_dev, const afcm_group_entry* table_host, int32_t n, int32_t batch, const int32_t* groups,
                      void* stream);

/* ----------------------------------------------------------------------------------------
 * The training log on the device (additions to v13): one row of doubles per training step in a ring in DEVICE memory, written by one short launch
 * inside the step, so that a replayed graph can be read once per epoch -- the reference's get_current_losses() (train.py; models/pix2pix_model.py:75
 * names G_GAN, G_L1, D_real, D_fake; Dr1 sits beside them) plus what afcm_adam_multi's scrub replaced without saying so.
 *
 * afcm_grad_stats: over afcm_adam_multi's DEVICE pointer table (same n, total_chunks and grad_scale as the Adam launch it precedes), one 256-thread
 * workgroup per chunk of afcm_adam_chunk_elems() elements.  It reads g only and writes partials[chunk][0..3] (DEVICE doubles, total_chunks rows):
 *   { sumsq, n_nan, n_posinf, n_neginf }   of gr = g * grad_scale formed in float32 as the Adam kernel forms it (a finite g that overflows under
 *   grad_scale counts as infinite); sumsq adds (double)gr * (double)gr of every FINITE gr (the product is exact).
 * Order of sumsq: thread t adds its elements in ascending index from +0.0 -- elements 4 t + 1024 k + {0, 1, 2, 3} of the chunk where g is 16-byte
 * aligned, t + 256 k where it is not (the Adam kernel's two paths, decided by g alone here) --, then one tree over the 256 threads:
 * s[t] += s[t + o] for o = 128, 64, ..., 1.  No atomics: bit-identical from launch to launch.
 * AFCM_E_INVALID: an empty table, total_chunks outside [1, 2^31), a null or misaligned partials.
 *
 * afcm_trainlog_append: one workgroup.  Each of the four columns of partials_G[chunks_G][4] and partials_D[chunks_D][4] is summed over the chunks --
 * thread t adds rows t, t + 256, ... in ascending order from +0.0, then the same tree -- and ONE row of AFCM_TRAINLOG_COLS doubles is written at
 * log[(head % capacity) * AFCM_TRAINLOG_COLS], then head[0] += 1 (one lane, a plain store; head is a DEVICE int64 that starts at 0):
 *   [0]      serial: head before the append
 *   [1..8]   the schedule block's 8 slots as they stand (total_iters, blur_sigma, blur_radius, ema_beta, lr_G, lr_D, two spare)
 *   [9] [10] Adam step counts of G and D (step_G[0], step_D[0]: the capturable optimizers' device floats)
 *   [11..15] G_GAN, G_L1, D_real, D_fake, Dr1 from losses[5] (float32; a NaN there means absent)
 *   [16..19] G: sumsq, NaN count, +inf count, -inf count      [20..23] D: the same four
 * A NULL pointer among block, step_G, step_D, losses, partials_G, partials_D means absent: its columns are NaN.
 * Both launches go to `stream`; no stream, event, allocation or synchronise: capturable, and the captured graph stays one chain.
 * AFCM_E_INVALID: a null log or head, capacity < 1, a negative chunk count.
 * ---------------------------------------------------------------------------------------- */
#define AFCM_TRAINLOG_COLS 24
int32_t afcm_trainlog_cols(void);
int afcm_grad_stats(const afcm_adam_entry* table, int32_t n, int64_t total_chunks, float grad_scale, double* partials, void* stream);
int afcm_trainlog_append(double* log, int32_t capacity, int64_t* head, const double* block, const float* step_G, const float* step_D,
                         const float* losses, const double* partials_G, int64_t chunks_G, const double* partials_D, int64_t chunks_D, void* stream);

/* ----------------------------------------------------------------------------------------
 * Per-plane normalisers (additions to v13): the reference's PercentileNormalizer and Standardize (data/augment/transforms.py:552-601,
 * channelwise False; the first two entries of configs/defaults.py for both phases) inside the two loaders.  They come before every geometric
 * transform, and their coefficients are a statistic of each [1, h, w] item plane m: the plane after the centred crop / zero pad, padded zeros
 * counted, a thick-slice position outside the volume a plane of zeros.  Two launches: the statistics, then the assembly.
 *
 * afcm_plane_norm_stats (the items of afcm_batch_assemble's pool and tables: k planes of a, then b) and afcm_slice_norm_stats (the slices of
 * afcm_slice_assemble: k planes) write coef [count][planes][4] DEVICE float64 = (sub, div, stat0, stat1) per plane, one 256-thread workgroup
 * each.  All arithmetic is float64 whatever the source type, every operation rounded on its own.
 *   AFCM_NORM_PERCENTILE  p0, p1 = pmin / 100, pmax / 100.  lo, hi = numpy's `linear` percentiles: with n = h w and v = q (n - 1), the order
 *                         statistics at floor(v) and min(floor(v) + 1, n - 1) (-0.0 taken as +0.0) combined by numpy's _lerp with g = v - floor(v):
 *                         g >= 0.5 ? b - (b - a) (1 - g) : a + (b - a) g.  sub = lo, div = (hi - lo) + eps, stats lo, hi.  The order statistics
 *                         come from an exact radix select, 8 bits per pass, most significant first (u8 one pass, i16 two, f32 four, f64 eight),
 *                         in LDS histograms.  One NaN in the plane makes all four NaN, as numpy's percentile does.
 *   AFCM_NORM_STANDARDIZE mean = sum / n, std = sqrt(ss / n), ss the sum of (m - mean)^2.  Both sums in ONE order: thread t adds pixels t, t + 256,
 *                         ... of the row-major plane in ascending order onto +0.0, then the tree s[t] += s[t + o] for o = 128, 64, ..., 1.
 *                         sub = mean, div = std < eps ? eps : std (numpy.clip: a NaN stays), stats mean, std.
 *   AFCM_NORM_FIXED       p0, p1 = the given mean and std: sub = p0, div = p1 < eps ? eps : p1; nothing is read.
 * A plane outside the volume reads nothing: lo = hi = 0, or mean = std = 0.  An invalid item row (afcm_batch_assemble's checks) reads nothing
 * and gives four NaNs.  No global atomics (integer LDS adds only), no allocation, no host read: bit-identical from launch to launch, on
 * `stream`, capturable.  afcm_norm_plan: plan[0..3] = threads per workgroup, times the plane is read, bits per digit, ranks selected.
 *
 * afcm_batch_assemble_norm is afcm_batch_assemble_aug (augment may be NULL: afcm_batch_assemble) and afcm_slice_assemble_norm is
 * afcm_slice_assemble -- thread shape, row checks, gather, labels and stores -- with the value of a pixel m of plane p of sample i
 *   v = (m - sub) / div  from coef[i][p],  then, with then_normalize, clip(2 * ((v - min) / (max - min)) - 1, -1, 1) (a NaN stays),
 * in float64 for EVERY source type, then one rounding to float32 and one more to a 16-bit out_dtype.  A nearest-neighbour gather commutes
 * with a pointwise map, so coefficients taken from the un-augmented plane are the reference's order of operations.  min_value / max_value
 * are read only with then_normalize but checked always.
 * AFCM_E_INVALID: as the launches they extend; also a null or misaligned coef, an unknown mode, percentile fractions outside
 * 0 <= p0 <= p1 <= 1, a NaN eps, then_normalize not 0 or 1, a plane of more than 2^30 pixels.
 * ---------------------------------------------------------------------------------------- */
enum { AFCM_NORM_PERCENTILE = 1, AFCM_NORM_STANDARDIZE = 2, AFCM_NORM_FIXED = 3 };
int afcm_norm_plan(int32_t src_dtype, int32_t mode, int32_t* plan);
int afcm_plane_norm_stats(double* coef, const void* pool, int64_t pool_elems, int32_t src_dtype, const int64_t* vols, int32_t n_vols,
                          const int32_t* items, int32_t n_items, const int64_t* cursor, int32_t first, int32_t count, int32_t k, int32_t h, int32_t w,
                          int32_t mode, double p0, double p1, double eps, void* stream);
int afcm_slice_norm_stats(double* coef, const void* src, int32_t src_dtype, int32_t depth, int32_t hs, int32_t ws, int64_t src_stride_z, int32_t first,
                          int32_t count, int32_t k, int32_t thickness, int32_t h, int32_t w, int32_t mode, double p0, double p1, double eps,
                          void* stream);
int afcm_batch_assemble_norm(void* a, void* b, float* slice_idx, const void* pool, int64_t pool_elems, int32_t src_dtype, const int64_t* vols,
                             int32_t n_vols, const int32_t* items, int32_t n_items, const double* augment, const double* coef, int32_t then_normalize,
                             const int64_t* cursor, int32_t first, int32_t count, int32_t k, int32_t h, int32_t w, int32_t out_dtype, double min_value,
                             double max_value, void* stream);
int afcm_slice_assemble_norm(void* a, float* slice_idx, const void* src, int32_t src_dtype, int32_t out_dtype, int32_t depth, int32_t hs, int32_t ws,
                             int64_t src_stride_z, const double* coef, int32_t then_normalize, int32_t first, int32_t count, int32_t k, int32_t thickness,
                             int32_t h, int32_t w, double min_value, double max_value, void* stream);

/* ----------------------------------------------------------------------------------------
 * Epilogue of the CoModGAN modulated convolution (additions to v13: no existing entry point or struct changes, so the number stays;
 * csrc/modconv_epilogue.hip, afcm_amd/networks_comodgan.py).  All tensors contiguous float32.  u = 1 or 2, with (H, W) = (h, w) the
 * LOW resolution:
 *   t [n, u u o, h, w]  the convolution's result; for u = 2 channel (py 2 + px) o + c holds output phase (py, px) of channel c
 *   dcoefs [n, o], bias [o], noise NULL | [u h, u w] (noise_per_sample 0) | [n, 1, u h, u w] (1), noise_strength one DEVICE float (NULL with noise)
 *   y [n, o, u h, u w]:  y[., c, u i + py, u j + px] = clamp(lrelu(t[., (py u + px) o + c, i, j] dcoefs + noise noise_strength + bias) gain, +-clamp)
 * evaluated in float64 and rounded once; lrelu(v) = v > 0 ? v : alpha v; clamp < 0: none, otherwise the clamp rounded to float32.
 * afcm_modconv_epilogue_bwd (first order), with g = dy (y > 0 ? 1 : alpha) gain and g = 0 where |y| >= clamp (the slope alpha at y == 0,
 * no gradient at the clamp: bias_act's conventions):  d_t = g dcoefs in t's layout, d_dcoefs [n, o] = sum g t, d_bias [o] = sum g,
 * d_noise_strength (one float; NULL with noise) = sum g noise.  The sums are float64 in one fixed order (stated in the source file), without
 * atomics: bit-identical from launch to launch.  workspace: afcm_modconv_epilogue_workspace_bytes(n, o, h, w) bytes, 8-byte aligned,
 * written before it is read.  No allocation, no host read, on `stream`, capturable.
 * Tensors that are all 16-byte aligned, with w a multiple of 4 / u, are read and written in 16-byte pieces; any other take 4-byte reads.
 * AFCM_E_INVALID (nothing launched): a null or misaligned pointer (y and dy: 4 u bytes), noise without its strength or the reverse, u not
 * 1 or 2, an empty tensor, a plane of 2^31 pixels or more, a gain that is not positive and finite, a NaN slope or clamp.
 * ---------------------------------------------------------------------------------------- */
int64_t afcm_modconv_epilogue_workspace_bytes(int32_t n, int32_t o, int32_t h, int32_t w);
int afcm_modconv_epilogue_fwd(float* y, const float* t, const float* dcoefs, const float* bias, const float* noise, const float* noise_strength,
                              int32_t noise_per_sample, int32_t n, int32_t o, int32_t h, int32_t w, int32_t u, double alpha, double gain,
                              double clamp, void* stream);
int afcm_modconv_epilogue_bwd(float* d_t, float* d_dcoefs, float* d_bias, float* d_noise_strength, double* workspace, const float* dy,
                              const float* y, const float* t, const float* dcoefs, const float* noise, int32_t noise_per_sample, int32_t n,
                              int32_t o, int32_t h, int32_t w, int32_t u, double alpha, double gain, double clamp, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AFCM_HIP_H */
