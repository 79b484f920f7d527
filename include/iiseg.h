/*
 * iiseg.h -- C ABI of libiiseg_hip.so, the MI355X (gfx950) kernel library behind the
 * iterative-inference hot path of adri-romsor/iterative_inference_segm.
 *
 * The reference has no FFI: its device boundary is the four Theano functions compiled at
 * iterative_inference.py:187-210 (pred_fcn_fn, pred_dae_fn, de_fn, val_fn), whose graphs are
 * made of the Lasagne layers cited per entry point below.  Each entry point replaces the
 * Theano op(s) that those layers lower to.
 *
 * Conventions:
 *   - plain C, no torch types; all tensor pointers are DEVICE pointers to C-contiguous NCHW
 *     float32 unless stated; the caller owns every byte (inputs, outputs, workspaces);
 *   - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*); it never
 *     allocates, never synchronises, and is safe to capture into a hipGraph;
 *   - return value: IISEG_OK (0) or a negative iiseg_status; iiseg_strerror() names it;
 *   - calls on different streams are thread-safe; one stream = program order.
 */
#ifndef IISEG_H
#define IISEG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum iiseg_status {
    IISEG_OK = 0,
    IISEG_ERR_NULL = -1,       /* a required pointer is NULL                         */
    IISEG_ERR_SHAPE = -2,      /* inconsistent / unsupported shape                   */
    IISEG_ERR_ALIGN = -3,      /* pointer not aligned as the kernel requires         */
    IISEG_ERR_LAUNCH = -4,     /* hipLaunchKernel / hipGetLastError failed           */
    IISEG_ERR_UNSUPPORTED = -5 /* valid request, but no kernel variant implements it */
} iiseg_status;

const char* iiseg_strerror(int status);
/* the HIP runtime's name for the error behind the last IISEG_ERR_LAUNCH of this library */
const char* iiseg_last_hip_error(void);
/* ABI version, bumped on any signature change. */
int iiseg_abi_version(void);
/* Name of the GPU architecture the library was compiled for ("gfx950"). */
const char* iiseg_target_arch(void);

/* Launch profiling (measurement only; bench.py's roofline pass).  Between iiseg_profile_begin(capacity)
 * and iiseg_profile_end every kernel launch of this library carries its own start / stop HIP events ON ITS
 * DISPATCH (hipExtLaunchKernelGGL), in launch order; iiseg_profile_count() = launches so far (-1 when
 * off); iiseg_profile_end waits for them and writes the elapsed milliseconds of up to `capacity` launches
 * -- each kernel's execution time on the stream it was launched on, the duration rocprofv3 reports, without
 * the barrier packets separately recorded events put between two kernels (7 % of a 0.18 ms kernel) --
 * and returns their number.  Process-wide state: one profiling pass at a time. */
int iiseg_profile_begin(int capacity);
int iiseg_profile_count(void);
int iiseg_profile_end(float* ms, int capacity);

/* ---------------------------------------------------------------------------------------
 * Implicit-GEMM convolution (stride 1), fp32 MFMA.
 * Replaces: Lasagne Conv2DLayer / DilatedConv2DLayer (+ fused Elemwise bias/ReLU), i.e.
 * Theano CorrMM, at models/fcn8.py:34-85,92-93,102-103; models/fcn_down.py:102-104;
 * models/fcn_up.py:83-86; models/contextmod_dae.py:74-105.  Fusions: the h-concat of
 * models/model_helpers.py:93-94 (two sources, h first), DePool2D of layers/mylayers.py:88-115
 * as an input gather, ElemwiseSumLayer/CroppingLayer of models/fcn_up.py:96-113 as epilogue.
 * ------------------------------------------------------------------------------------- */

#define IISEG_CONV_RELU 1u   /* out = max(out, 0)                                   */
#define IISEG_CONV_UNPOOL 2u /* logical input = eq-mask unpool(up=x1, pre, pooled)  */
/* KxK (K = 3 or 4) stride-2 TRANSPOSED convolution, crop='valid': Deconv2DLayer of FC-DenseNet's
 * TransitionUp (K=3, models/FCDenseNet.py:119 via FC_DenseNet.layers) and of the DAE's
 * unpool_type='standard' (K=4, models/fcn_up.py:41-45; float32 only).  Logical output
 * ((H-1)*2+K, (W-1)*2+K); w is the reference layout W[in][out][K][K] (pass stride_o = K*K,
 * stride_c = Cout*K*K), the spatial flip of Lasagne's gradient form is applied
 * while packing; pad/dil are ignored. */
#define IISEG_CONV_TRANSPOSED2 4u
/* iiseg_conv_c8 only: the split-operand ("bf16x3") fp32-class mode of the 16-bit matrix pipe.  Every
 * bf16 C8 tensor of the call (x1, `up`, add of kind 1, out of kind 1, pool_out) is a hi / lo PAIR in
 * one allocation, (B, 2 C/8, H, W, 8): chunks [0, C/8) of an image = bf16(v), chunks [C/8, 2 C/8) =
 * bf16(v - hi); the packed weights hold two k-groups [W_hi | W_lo] (pack a (Cout, 2 C1) filter built
 * that way with iiseg_conv_halo_bf16_pack); the layer accumulates x_lo W_hi + x_hi W_lo + x_hi W_hi
 * in fp32.  d->C1 stays the logical channel count; C2 must be 0. */
#define IISEG_CONV_X3 8u
/* iiseg_conv_c8_slice only: the logical input is x1 with one zero inserted between neighbouring pixels and a
 * two-pixel zero frame, z[2 i + 2][2 j + 2] = x1[i][j] on (H, W) = (2 h + 3, 2 w + 3) -- a 'valid' 3x3
 * correlation of z with the in / out-swapped filter IS the 3x3 stride-2 'valid' transposed convolution of
 * FC-DenseNet's TransitionUp (models/FCDenseNet.py:118-121; Deconv2DLayer, P3) */
#define IISEG_CONV_ZINS 16u

typedef struct iiseg_conv_desc {
    /* logical input (after concat / unpool): (B, C1 + C2, H, W) */
    int32_t B, C1, C2, H, W;
    /* filter */
    int32_t Cout, KH, KW, pad, dil;
    /* logical output is (H + 2*pad - dil*(KH-1), W + 2*pad - dil*(KW-1)); only the window
     * [oy0, oy0+OH) x [ox0, ox0+OW) is computed and `out` is (B, Cout, OH, OW). */
    int32_t oy0, ox0, OH, OW;
    /* optional epilogue add: out += add[b, co, ay0 + oy, ax0 + ox]; add is (B, Cout, AH, AW) */
    int32_t AH, AW, ay0, ax0;
    uint32_t flags;
    /* packed-weight geometry produced by iiseg_conv_pack_f32 */
    int32_t Kpad, Mpad;
    /* destination as a channel slice of a wider tensor (B, out_ctot, OH, OW), first channel
     * out_c0 -- lets dense blocks grow a preallocated stack without concat copies
     * (ConcatLayer([stack, l]), models/FCDenseNet.py:92).  out_ctot == 0: dense (B, Cout, OH, OW). */
    int32_t out_ctot, out_c0;
    /* destination as a spatial window of a larger plane: the (OH, OW) result is written at
     * (out_y0, out_x0) of planes of size (out_H, out_W).  out_H == 0: dense (OH, OW) planes.
     * Used to compute only the part of a decoder level that reaches the final center crop
     * (models/fcn_up.py:104-113) while every tensor keeps its full-size addressing. */
    int32_t out_H, out_W, out_y0, out_x0;
    /* Winograd path only: parity (0 or 1) of the absolute output row / column at which the 2x2
     * tiles start.  Must be the same for every launch of a layer whose windows are expected to
     * agree bit for bit; pick the parity of the most frequent window origin. */
    int32_t tile_y0, tile_x0;
} iiseg_conv_desc;

/* Number of int32x4 entries of the gather table for `d` (== d->Kpad). */
int iiseg_conv_ktab_entries(const iiseg_conv_desc* d);
/* Fills d->Kpad / d->Mpad for the (C1+C2, KH, KW, Cout) of `d`. */
int iiseg_conv_plan(iiseg_conv_desc* d);

/* Packs reference-layout weights into the kernel layout Wp[Kpad][Mpad] (k = (c*KH+ky)*KW+kx)
 * and builds the gather table.  `w` element (o, c, ky, kx) is read at
 * w[o*stride_o + c*stride_c + ky*KW + kx], which covers Conv2DLayer W[out,in,kh,kw]
 * (stride_o = Cin*KH*KW, stride_c = KH*KW) and DilatedConv2DLayer W[in,out,kh,kw]
 * (stride_o = KH*KW, stride_c = Cout*KH*KW; P11).  wp: Kpad*Mpad floats; ktab: Kpad*4 int32. */
int iiseg_conv_pack_f32(void* stream, const iiseg_conv_desc* d, const float* w,
                        int64_t stride_o, int64_t stride_c, float* wp, int32_t* ktab);

/* out = epilogue(conv(input)).  x2 may be NULL when C2 == 0.  With IISEG_CONV_UNPOOL:
 * x1 = up (B, C1, H/2, W/2), pre (B, C1, H, W), pooled (B, C1, H/2, W/2), C2 must be 0.
 * bias (Cout) and add may be NULL. */
int iiseg_conv_f32(void* stream, const iiseg_conv_desc* d, const float* x1, const float* x2,
                   const float* pre, const float* pooled, const float* wp, const int32_t* ktab,
                   const float* bias, const float* add, float* out);

/* iiseg_conv_f32 that also writes the 2x2/2 max-pool (ignore_border) of its output: the
 * Pool2DLayer that follows the conv (models/fcn_down.py:122, models/fcn8.py:38-45) fused into the
 * epilogue of the halo-tile kernel, saving the pool kernel's read of the full-resolution map.
 * pool_out is the FULL pooled tensor (B, Cout, fullH/2, fullW/2); the pooled positions of the
 * computed window are written in place.  Supported (iiseg_conv_pool_supported) for the 3x3 layers
 * the halo kernel takes (16 < Cout < 256) with an even window origin and whole pooling windows. */
/* 1 when iiseg_conv_f32 runs this (planned, plain: no add / pool / masks) request on the vector-ALU kernel
 * for layers between at most 16 channels on either side (csrc/conv_small.hip: the context module's 1x1 /
 * dilated 3x3 layers, models/contextmod_dae.py:74-105) -- a scheduling fact, for profiles. */
int iiseg_conv_small_supported(const iiseg_conv_desc* d);
int iiseg_conv_pool_supported(const iiseg_conv_desc* d);

/* Which of the direct kernels iiseg_conv_f32 runs a (planned) request on, and with which tiling: the
 * answer of the very dispatch the launch goes through (csrc/conv_igemm.hip), for a plain call -- no fused
 * pool, mask bytes or input BatchNorm -- with or without a skip-add and a bias.  Returns one of
 * IISEG_CONV_KERNEL_* and fills tiles[4] = {BM, BN, pixel tiles, channel tiles}: output channels x
 * pixels of one workgroup's tile, and the grid as pixel tiles x channel tiles.  A descriptor that
 * iiseg_conv_f32 would refuse gives its negative iiseg_status.  Host only: no launch, no allocation,
 * no stream work.  The answer follows the IISEG_CONV_* switches of the process and
 * iiseg_conv_halo_seam. */
#define IISEG_CONV_KERNEL_SMALL 1  /* conv_small_f32_kernel: vector ALU, 16 rows x 64 columns        */
#define IISEG_CONV_KERNEL_HALO 2   /* conv_halo_f32_kernel: 3x3, TH rows x 32 columns (BN = TH * 32) */
#define IISEG_CONV_KERNEL_HALO16 3 /* conv_halo16_f32_kernel: 3x3, at most 16 output channels        */
#define IISEG_CONV_KERNEL_TAPS 4   /* conv_taps_f32_kernel: 1x1, 3x3, transposed 3x3 / 4x4           */
#define IISEG_CONV_KERNEL_IGEMM 5  /* conv_igemm_f32_kernel: any filter, table-driven gather         */
int iiseg_conv_direct_kernel(const iiseg_conv_desc* d, int has_add, int has_bias, int32_t* tiles);
int iiseg_conv_pool_f32(void* stream, const iiseg_conv_desc* d, const float* x1, const float* x2,
                        const float* pre, const float* pooled, const float* wp, const int32_t* ktab,
                        const float* bias, const float* add, float* out, float* pool_out);

/* DePool2D equality masks as BYTES (halo-tile kernels here; the Winograd form has its own entry,
 * iiseg_conv_wino_mask_f32): the reference's DePool2D needs
 * pre == pooled per element (layers/mylayers.py:111-114); instead of keeping the pre-pool map for
 * that comparison, the conv whose epilogue does the pooling can write
 *     mask[b][c][y/2][x/2] bit (y & 1) * 2 + (x & 1) = (pre[b][c][y][x] == pooled[b][c][y/2][x/2])
 * (B, Cout, fullH/2, fullW/2 bytes, same placement rules as pool_out) and the decoder conv can take
 * its IISEG_CONV_UNPOOL input from x1 = up and mask_in = that tensor instead of pre / pooled: 5 bytes
 * read per unpooled element instead of 12, and the largest map of every level is never written or
 * re-read.  iiseg_conv_mask_f32 is iiseg_conv_pool_f32 with both options: `out` may be NULL when
 * pool_out and mask_out are given (the pre-pool map is then not stored at all); with mask_in, pre
 * and pooled are ignored (pass NULL).  Same decisions, bit for bit, as the pre / pooled form.
 * iiseg_conv_mask_supported: 1 if the request runs on a halo kernel (3x3, dil 1, Cout < 256; the
 * pool / mask_out part needs 16 < Cout and whole pooling windows, as iiseg_conv_pool_supported). */
int iiseg_conv_mask_supported(const iiseg_conv_desc* d);
int iiseg_conv_mask_f32(void* stream, const iiseg_conv_desc* d, const float* x1, const float* x2,
                        const float* pre, const float* pooled, const uint8_t* mask_in,
                        const float* wp, const int32_t* ktab, const float* bias, const float* add,
                        float* out, float* pool_out, uint8_t* mask_out);

/* Tiling of the fp32 halo-tile kernel (3x3, dil 1, 16 < Cout < 256).  By default its 32-column pixel tiles
 * run across the seam between consecutive images of the batch (the B * OW columns of a row band laid end to
 * end) wherever that takes fewer tiles than one tile grid per image, OW >= 32, and a fused pool has an even
 * OW; every output is the same sum in the same order under both tilings, bit for bit.
 *   iiseg_conv_halo_seam(on)         on = 0 / 1: per-image / seam tiling for the launches that follow (the
 *                                    default is the environment's IISEG_HALO_SEAM, 1 when unset); on < 0 only
 *                                    asks.  Returns the setting in force.  For A/B timing and tests.
 *   iiseg_conv_halo_seam_launches    launches so far that ran the seam tiling (a scheduling fact) */
int iiseg_conv_halo_seam(int on);
int64_t iiseg_conv_halo_seam_launches(void);

/* 3x3 convolution with at most 16 output channels whose INPUT is normalised and rectified while it
 * is staged: x <- max((x - mean[c]) * (gamma[c] * inv_std[c]) + beta[c], 0) per input channel --
 * BN_ReLU_Conv of FC-DenseNet (models/FCDenseNet.py:12,90,109,123) as one kernel instead of
 * iiseg_bn_relu_f32 + iiseg_conv_f32 (the normalised copy of the growing feature stack is never
 * written).  x is (B, >= C1, H, W) with x_bstride elements between images (the first C1 channels of
 * a stack).  Same arithmetic as iiseg_bn_relu_f32; zero padding pads the normalised map. */
int iiseg_conv_bnrelu_supported(const iiseg_conv_desc* d);
int iiseg_conv_bnrelu_f32(void* stream, const iiseg_conv_desc* d, const float* x, int64_t x_bstride,
                          const float* beta, const float* gamma, const float* mean,
                          const float* inv_std, const float* wp, const int32_t* ktab,
                          const float* bias, float* out);

/* Winograd F(2x2,3x3) form of the same convolution (same call sites as iiseg_conv_f32 for
 * 3x3, dil 1, stride 1 layers with (C1+C2) % 16 == 0, no TRANSPOSED2; with IISEG_CONV_UNPOOL the
 * DePool2D mask is applied while the input transform loads its 4x4 patches, operands as in
 * iiseg_conv_f32):
 * 2.25x fewer fp32 multiplies on the matrix pipe.  Same descriptor (window, placement, channel
 * slice, add, ReLU; Kpad/Mpad are ignored), results equal to iiseg_conv_f32 up to fp32 rounding,
 * and bit-identical between any two windows of one layer launched with the same tile anchor
 * parity (tile_y0 / tile_x0 of the descriptor).
 *   iiseg_conv_wino_supported      1 if `d` can run on this path, else 0
 *   iiseg_conv_wino_weight_elems   floats of the transformed weights U = G g G^T
 *   iiseg_conv_wino_workspace_elems floats of the caller-owned workspace one call needs
 *                                  (transformed input V + products M), for the window in `d`
 *   iiseg_conv_wino_pack_f32       w (layout as in iiseg_conv_pack_f32) -> U, once per layer
 *   iiseg_conv_wino_f32            input transform -> 16 GEMMs -> output transform + epilogue;
 *                                  `stages` selects which of the three kernels are enqueued
 *                                  (IISEG_WINO_ALL normally; single stages let a caller time
 *                                  the MFMA kernel on its own) */
#define IISEG_WINO_INPUT 1u
#define IISEG_WINO_GEMM 2u
#define IISEG_WINO_OUTPUT 4u
#define IISEG_WINO_ALL 7u
/* with IISEG_WINO_FUSED the GEMM stage also applies the output transform + epilogue (the
 * products stay in registers; IISEG_WINO_OUTPUT is ignored): INPUT | GEMM | FUSED is a full call */
#define IISEG_WINO_FUSED 8u
int iiseg_conv_wino_supported(const iiseg_conv_desc* d);
int64_t iiseg_conv_wino_weight_elems(const iiseg_conv_desc* d);
int64_t iiseg_conv_wino_workspace_elems(const iiseg_conv_desc* d);
int iiseg_conv_wino_pack_f32(void* stream, const iiseg_conv_desc* d, const float* w,
                             int64_t stride_o, int64_t stride_c, float* U);
int iiseg_conv_wino_f32(void* stream, const iiseg_conv_desc* d, const float* x1, const float* x2,
                        const float* pre, const float* pooled, const float* U, const float* bias,
                        const float* add, float* workspace, float* out, uint32_t stages);
/* The input transform of the fp32 Winograd calls.  By default plain and mask-byte inputs run the streaming
 * kernel (four consecutive tiles per thread, 16-byte stores, a channel loop per workgroup).  The older
 * per-tile (small maps) and LDS-staged kernels keep: the pre / pooled form of DePool2D; geometries whose
 * staged rows or offsets do not fit the streaming kernel; and two classes that measured no gain on it --
 * launches of fewer than 4096 tiles, and plain maps whose tiles per image fill the LDS-staged kernel's
 * workgroups exactly.  V is the same under every choice, bit for bit.
 *   iiseg_conv_wino_input_wide(on)   on = 0 / 1: never / by the rule above, for the launches that follow
 *                                    (the default is the environment's IISEG_WINO_INPUT_WIDE, 1 when
 *                                    unset); on = 2: also for the two no-gain classes (tests reach the
 *                                    kernel on small maps); on < 0 only asks.  Returns the setting in
 *                                    force.  For A/B timing and tests.
 *   iiseg_conv_wino_input_path(d, mask_bytes)   the kernel a call with this descriptor would run under
 *                                    the setting in force (mask_bytes: IISEG_CONV_UNPOOL from mask
 *                                    bytes): 0 per-tile, 1 LDS-staged, 2 streaming; < 0 an IISEG_ERR_* */
int iiseg_conv_wino_input_wide(int on);
/* The streaming kernel with TWO consecutive tiles per thread: half the staged loads, offsets and results, 24 KB
 * of LDS instead of 48 and 8-byte stores, so that its workgroups fit on a compute unit beside the GEMM's.  It runs
 * wherever the streaming kernel runs and its halved staging buffer holds every workgroup's rows; V is the same,
 * bit for bit.
 *   iiseg_conv_wino_input_narrow(on)   on = 0 / 1 for the launches that follow (the default is the environment's
 *                                      IISEG_WINO_INPUT_NARROW, 1 when unset); on < 0 only asks.  Returns the
 *                                      setting in force.  For A/B timing and tests.
 *   iiseg_conv_wino_input_tiles(d, mask_bytes)   tiles per thread of the streaming kernel for such a call under
 *                                      the settings in force: 4 or 2, 0 where another kernel runs; < 0 an
 *                                      IISEG_ERR_* */
int iiseg_conv_wino_input_narrow(int on);
int iiseg_conv_wino_input_tiles(const iiseg_conv_desc* d, int mask_bytes);
int iiseg_conv_wino_input_path(const iiseg_conv_desc* d, int mask_bytes);
/* The products M of the separate-GEMM forms (iiseg_conv_wino_f32 without IISEG_WINO_FUSED, the GEMM form of
 * iiseg_conv_wino_bf16, the split-K iiseg_conv_gemm_f32 / iiseg_conv_gemm_bf16) lie in the workspace as
 * M[slice][Mpad / 4][Tpad][4], four consecutive output channels of one tile together: the GEMM writes and
 * the output kernels read them in 16-byte pieces.  The size of the workspace is the same, and so is every
 * result, bit for bit.  (A slice of 2 GiB or more keeps M[slice][Mpad][Tpad].)
 *   iiseg_conv_wino_m_quad(on)   on = 0 / 1: M[slice][Mpad][Tpad] with 4-byte pieces / the quad layout, for
 *                                the launches that follow (the default is the environment's
 *                                IISEG_WINO_M_QUAD, 1 when unset); on < 0 only asks.  Returns the setting in
 *                                force.  For A/B timing and tests.  The setting is process-wide and must NOT
 *                                change between the separately launched stages of one layer
 *                                (IISEG_WINO_GEMM, then IISEG_WINO_OUTPUT): the second would read a layout
 *                                the first did not write. */
int iiseg_conv_wino_m_quad(int on);
/* The 256x128 and 128x128 tiles of the fp32 GEMM stage (iiseg_conv_wino_f32 without IISEG_WINO_FUSED and the
 * split-K iiseg_conv_gemm_f32) hold their load and store addressing in scalar registers and one lane offset per
 * operand, which leaves room on a compute unit for waves of another stream's kernels beside four GEMM waves per
 * SIMD.  Loads, the order of the multiply-accumulates, stores and every result are the same, bit for bit.
 *   iiseg_conv_wino_gemm_slim(on)   on = 0 / 1: the addressing in vector registers / the form above, for the
 *                                   launches that follow (the default is the environment's IISEG_WINO_GEMM_SLIM,
 *                                   1 when unset); on < 0 only asks.  Returns the setting in force.  For A/B
 *                                   timing and tests. */
int iiseg_conv_wino_gemm_slim(int on);
/* The Winograd call with the 2x2 max-pool and the DePool2D mask bytes (as iiseg_conv_mask_f32):
 *   pool_out   (may be NULL) the FULL pooled tensor (B, Cout, fullH/2, fullW/2); the pooled
 *              positions of the window are written in place by the output transform (or the fused
 *              kernel's epilogue).  Needs a tile to be one pooling window:
 *              iiseg_conv_wino_pool_supported = even tile anchor (tile_y0 = tile_x0 = 0), even
 *              window origin, even extent unless the window ends at the map's last row / column.
 *   mask_out   (may be NULL, needs pool_out) the mask bytes of those windows, pool_out's shape
 *   out        may be NULL when pool_out is given: the pre-pool map is not stored
 *   mask_in    (may be NULL; IISEG_CONV_UNPOOL) bytes of x1's shape replacing pre / pooled: the
 *              input transform reads up + one byte per 2x2 instead of pre, pooled and up.
 * Same arithmetic as iiseg_conv_wino_f32: the pooled values and the masks equal, bit for bit,
 * iiseg_maxpool2x2_window_f32 / iiseg_maxpool2x2_mask_window_f32 of the stored map. */
int iiseg_conv_wino_pool_supported(const iiseg_conv_desc* d);
int iiseg_conv_wino_mask_f32(void* stream, const iiseg_conv_desc* d, const float* x1, const float* x2,
                             const float* pre, const float* pooled, const uint8_t* mask_in,
                             const float* U, const float* bias, const float* add, float* workspace,
                             float* out, float* pool_out, uint8_t* mask_out, uint32_t stages);

/* ---------------------------------------------------------------------------------------
 * 16-bit MFMA path (BASELINE north_star "fp16 MFMA peak", configs[2] "bf16 with fp32 accumulate"):
 * the same Winograd F(2x2,3x3) convolution with bf16 GEMM operands on v_mfma_f32_32x32x16_bf16
 * and fp32 accumulation.  Tensors at the ABI stay fp32 NCHW; weights are rounded to bf16 when they
 * are packed, activations when the input transform writes its workspace; the 16 GEMMs, the output
 * transform and the epilogue (bias, add, ReLU, window, placement, channel slice -- same descriptor
 * fields as iiseg_conv_wino_f32) run as one kernel.  Statistical parity only (8 significant bits
 * per operand).  Any (C1 + C2) is accepted (channels are zero-padded to the 64-channel k-tile).
 *   iiseg_conv_wino_bf16_supported        1 if `d` can run on this path, else 0
 *   iiseg_conv_wino_bf16_weight_bytes     bytes of the packed bf16 weights U16
 *   iiseg_conv_wino_bf16_workspace_bytes  bytes of caller-owned workspace (transformed input V16;
 *                                         for layers with >= 1024 channels, which run the GEMMs as
 *                                         their own kernel with 256 x 128 blocks, also the fp32
 *                                         products M)
 *   iiseg_conv_wino_bf16_pack             w (layout as in iiseg_conv_pack_f32) -> U16, once per layer
 *   iiseg_conv_wino_bf16                  stages: IISEG_WINO_INPUT | IISEG_WINO_GEMM (= all)
 * ------------------------------------------------------------------------------------- */
int iiseg_conv_wino_bf16_supported(const iiseg_conv_desc* d);
int64_t iiseg_conv_wino_bf16_weight_bytes(const iiseg_conv_desc* d);
int64_t iiseg_conv_wino_bf16_workspace_bytes(const iiseg_conv_desc* d);
int iiseg_conv_wino_bf16_pack(void* stream, const iiseg_conv_desc* d, const float* w,
                              int64_t stride_o, int64_t stride_c, void* U16);
int iiseg_conv_wino_bf16(void* stream, const iiseg_conv_desc* d, const float* x1, const float* x2,
                         const float* pre, const float* pooled, const void* U16, const float* bias,
                         const float* add, void* workspace, float* out, uint32_t stages);

/* bf16-operand GEMM form of the 'valid' K x K layers computed in full into a dense output (fc6 7x7,
 * fc7 / score_fr 1x1: models/fcn8.py:75-85), the counterpart of iiseg_conv_gemm_f32: im2col to a
 * bf16 workspace, one bf16 GEMM (no split-K), bias / ReLU / NCHW store.  U16: ..._weight_bytes bytes
 * from iiseg_conv_gemm_bf16_pack (w layout as in iiseg_conv_pack_f32); workspace: ..._workspace_bytes. */
int iiseg_conv_gemm_bf16_supported(const iiseg_conv_desc* d);
int64_t iiseg_conv_gemm_bf16_weight_bytes(const iiseg_conv_desc* d);
int64_t iiseg_conv_gemm_bf16_workspace_bytes(const iiseg_conv_desc* d);
int iiseg_conv_gemm_bf16_pack(void* stream, const iiseg_conv_desc* d, const float* w,
                              int64_t stride_o, int64_t stride_c, void* U16);
int iiseg_conv_gemm_bf16(void* stream, const iiseg_conv_desc* d, const float* x, const void* U16,
                         const float* bias, void* workspace, float* out);

/* Halo-tile DIRECT 3x3 convolution with bf16 MFMA operands (fp32 accumulate) for the shallow layers
 * the Winograd form does not pay for (few channels, large maps; HBM-bound): same descriptor
 * semantics and fusions as iiseg_conv_f32 / iiseg_conv_pool_f32 for 3x3, dil 1, stride 1 layers
 * (two sources need C1 % 16 == 0).  wp16: iiseg_conv_halo_bf16_weight_bytes bytes, filled by
 * iiseg_conv_halo_bf16_pack from w (layout as in iiseg_conv_pack_f32).  pool_out (may be NULL): the
 * FULL pooled tensor, as in iiseg_conv_pool_f32 (even window origin, whole pooling windows, no add).
 * mask_in / mask_out (may be NULL): DePool2D masks as bytes, see iiseg_conv_mask_f32. */
int iiseg_conv_halo_bf16_supported(const iiseg_conv_desc* d);
int64_t iiseg_conv_halo_bf16_weight_bytes(const iiseg_conv_desc* d);
int iiseg_conv_halo_bf16_pack(void* stream, const iiseg_conv_desc* d, const float* w,
                              int64_t stride_o, int64_t stride_c, void* wp16);
int iiseg_conv_halo_bf16(void* stream, const iiseg_conv_desc* d, const float* x1, const float* x2,
                         const float* pre, const float* pooled, const void* wp16, const float* bias,
                         const float* add, float* out, float* pool_out, const uint8_t* mask_in,
                         uint8_t* mask_out);
/* The same kernel as a trainable module's forward launches it (fwd='bf16'; ops.Conv(fwd16=True)): the four
 * entries above with one refusal lifted -- a two-source layer's first source may have ANY channel count.  The
 * k-tile that holds channel C1 is then staged from both sources (each channel c from x1 if c < C1, else from x2 at
 * plane c - C1, else zero); every other launch runs the code it runs through iiseg_conv_halo_bf16.
 * iiseg_conv_halo_bf16_fwd_check: the status of the host-side checks (IISEG_OK, or why not), no launch. */
int iiseg_conv_halo_bf16_fwd_check(const iiseg_conv_desc* d);
int64_t iiseg_conv_halo_bf16_fwd_weight_bytes(const iiseg_conv_desc* d);
int iiseg_conv_halo_bf16_fwd_pack(void* stream, const iiseg_conv_desc* d, const float* w,
                                  int64_t stride_o, int64_t stride_c, void* wp16);
int iiseg_conv_halo_bf16_fwd(void* stream, const iiseg_conv_desc* d, const float* x1, const float* x2,
                             const float* pre, const float* pooled, const void* wp16, const float* bias,
                             const float* add, float* out, float* pool_out, const uint8_t* mask_in,
                             uint8_t* mask_out);

/* float64 Winograd F(2x2,3x3) form of iiseg_conv_f64 for the wide 3x3 layers of the strict-parity
 * path (stride 1, dil 1, (C1+C2) % 16 == 0, no TRANSPOSED2; with IISEG_CONV_UNPOOL x1 = up, pre,
 * pooled as in iiseg_conv_f64 and the DePool2D mask is applied by the input transform): input transform ->
 * 16 batched GEMMs on v_mfma_f64_16x16x4_f64 (operands by LDS-DMA) -> output transform + epilogue.
 * Same descriptor semantics as iiseg_conv_wino_f32 (window, placement, channel slice, add, ReLU, tile
 * anchor parity tile_y0 / tile_x0); results equal to iiseg_conv_f64 up to float64 rounding.
 * U: iiseg_conv_wino_f64_weight_elems doubles (iiseg_conv_wino_pack_f64, w as in iiseg_conv_pack_f64);
 * workspace: iiseg_conv_wino_f64_workspace_elems doubles, caller-owned. */
int iiseg_conv_wino_f64_supported(const iiseg_conv_desc* d);
int64_t iiseg_conv_wino_f64_weight_elems(const iiseg_conv_desc* d);
int64_t iiseg_conv_wino_f64_workspace_elems(const iiseg_conv_desc* d);
int iiseg_conv_wino_pack_f64(void* stream, const iiseg_conv_desc* d, const double* w,
                             int64_t stride_o, int64_t stride_c, double* U);
int iiseg_conv_wino_f64(void* stream, const iiseg_conv_desc* d, const double* x1, const double* x2,
                        const double* pre, const double* pooled, const double* U, const double* bias,
                        const double* add, double* workspace, double* out);

/* bf16 "C8" activations: the 16-bit MFMA path with the tensors BETWEEN layers already in the matrix
 * pipe's operand format.  A C8 tensor of C channels is (B, ceil(C/8), H, W, 8) bf16 -- the 8 channels
 * a lane feeds to one MFMA are 16 contiguous bytes -- with zero channels beyond C.  Same Lasagne
 * Conv2DLayer(3x3, stride 1) call sites as iiseg_conv_halo_bf16 (models/fcn8.py:34-71,
 * models/fcn_down.py:102-104, models/fcn_up.py:83-86); descriptor semantics as iiseg_conv_f32 with
 * d->C1 / d->C2 = the PHYSICAL channel counts of the C8 inputs (multiples of 16; d->C2 > 0 = channel
 * concat, x1 first) and weights packed by iiseg_conv_halo_bf16_pack for a descriptor with those
 * counts (rows of channels the reference layer does not have are zero).
 *   x1, x2      C8 inputs; with IISEG_CONV_UNPOOL x1 = `up` (B, C1/8, H/2, W/2, 8) and mask_in =
 *               (B, C1/8, H/2, W/2, 8) bytes, bit (y & 1) * 2 + (x & 1) of byte j: pre == pooled for
 *               channel 8 c8 + j at pixel (y, x) (DePool2D, layers/mylayers.py:88-115)
 *   add         NULL (add_kind 0), C8 bf16 (1) or C8 fp32 (2: (B, Cout/8, AH, AW, 8) floats)
 *   out         out_kind 0: not stored (pool_out given), 1: C8 bf16, 2: C8 fp32, 3: NCHW fp32
 *               (B, out_ctot, out_H, out_W), Cout <= 32, no add / pool -- the class-score layer
 *   pool_out    C8 bf16 (B, Cout/8, fullH/2, fullW/2, 8): 2x2 max-pool of the fp32 results, rules as
 *               iiseg_conv_pool_f32; mask_out: the DePool2D mask bytes of those windows, taken from
 *               the fp32 results before rounding (same decisions as the fp32-activation form)
 * Pixel tilings (chosen per launch from its geometry alone; every output is one fixed-order sum
 * whichever runs it): th x tw pixel tiles of one image (256 or 512 pixels, shape chosen for the fewest
 * tiles) or FLAT, 256 consecutive window pixels of the whole batch per workgroup (small windows).  With
 * pool_out the pixels of a tile are ordered by 2x2 pooling windows (even tile shapes; the flat list is
 * a list of windows), so the fused pool is available on every tiling.
 * iiseg_conv_c8_is_flat: 1 if the launch (without pool_out) uses the flat tiling.
 * (environment overrides for timing experiments: IISEG_C8_TILING=1|2, IISEG_C8_TALL=0|1,
 * IISEG_C8_SHAPE=th,tw)
 * iiseg_conv_c8_tiling: out4 = {0 rect-256 / 1 rect-512 / 2 flat, th (flat: patch rows), tw (flat:
 * patch row stride), quad order} of the launch with (pool != 0) or without a fused pool.
 * iiseg_nchw_to_c8 / iiseg_c8_to_nchw: layout converters (fp32 NCHW <-> C8 bf16, C8n chunks/image).
 * iiseg_pool_mask_c8: 2x2 max-pool (+ mask bytes, may be NULL) of the pooled-coordinate window
 * (y0, x0, wh, ww) from a stored piece `pre` (BC8 = B * chunks, PH, PW, 8; bf16, or with pre_f32 the
 * C8 fp32 results of out_kind 2: the same fp32 comparisons as the fused pool) whose corner is at
 * (py0, px0) of the (H, W) map, into the full (BC8, H/2, W/2, 8) pooled / mask tensors. */
int iiseg_conv_c8_supported(const iiseg_conv_desc* d);
int iiseg_conv_c8_is_flat(const iiseg_conv_desc* d);
int iiseg_conv_c8_tiling(const iiseg_conv_desc* d, int pool, int32_t* out4);
/* Test hook (process-wide, not for production use): kind -1 = automatic (default), 0 / 1 / 2 force the
 * rect-256 / rect-512 / flat tiling where it can run the launch; th, tw > 0 fix the RECT tile shape. */
int iiseg_conv_c8_force_tiling(int kind, int th, int tw);
int iiseg_conv_c8(void* stream, const iiseg_conv_desc* d, const void* x1, const void* x2,
                  const uint8_t* mask_in, const void* wp16, const float* bias, const void* add,
                  int add_kind, void* out, int out_kind, void* pool_out, uint8_t* mask_out);
/* iiseg_conv_c8 with x1 a CHANNEL SLICE of a wider C8 tensor: x1 points at the slice's first chunk plane of
 * image 0, x1_ctot = channels per image of the tensor it lies in (0: dense, d->C1) -- the conv reads a dense
 * block's stack in place (models/FCDenseNet.py:92: the ConcatLayer costs no copy) -- and, with
 * IISEG_CONV_ZINS, zero-inserted (d->H, d->W = the zero-inserted size, d->pad = 0).  Plain bf16 launches only
 * (no IISEG_CONV_UNPOOL / IISEG_CONV_X3, d->C2 == 0 with IISEG_CONV_ZINS). */
int iiseg_conv_c8_slice(void* stream, const iiseg_conv_desc* d, const void* x1, int32_t x1_ctot,
                        const void* x2, const uint8_t* mask_in, const void* wp16, const float* bias,
                        const void* add, int add_kind, void* out, int out_kind, void* pool_out,
                        uint8_t* mask_out);
/* DePool2D materialised on C8 tensors (layers/mylayers.py:88-115) for the pooled-coordinate window
 * (y0, x0, wh, ww): out (BC8, H, W, 8) bf16 <- up (BC8, H/2, W/2, 8) where the mask byte's bit (y & 1) * 2 +
 * (x & 1) is set, else 0; elements outside the window are left as they are (rows / columns >= 2 (H/2), 2 (W/2)
 * must be zero in `out`: they are never written).  The decoder levels with >= 1024 input channels unpool this way
 * and convolve the result as a plain layer (LDS-DMA staging) instead of selecting through registers per tile. */
int iiseg_unpool_c8(void* stream, const void* up, const uint8_t* mask, void* out, int BC8, int H, int W,
                    int y0, int x0, int wh, int ww);
/* The two element-wise adjoints of the standard DAE's backward walk on C8 tensors (true-gradient refinement on
 * the 16-bit leg; csrc/c8_grad.hip).  B images of C8n chunks (C8n even: whole 16-channel
 * groups), pooled planes (h2, w2), a pooled-coordinate window (y0, x0, wh, ww) outside which `out` is not written.
 *   iiseg_depool_bwd_c8   adjoint of DePool2D: out[q] = sum over k = 0..3 with bit k of the mask byte set of
 *                         gu[2 qy + (k >> 1)][2 qx + (k & 1)], summed in fp32 from 0 in that order and rounded once
 *                         to bf16 (RNE).  gu (B, C8n, PH, PW, 8) bf16 with PH >= 2 h2, PW >= 2 w2 (the unpaired
 *                         last row / column of an odd map is never read); mask (B, C8n, h2, w2, 8) bytes; out
 *                         (B, C8n, h2, w2, 8) bf16.  gate (NULL, or out's shape, bf16): the result of a channel is
 *                         +0 where gate <= 0 (-0 included) -- iiseg_relu_gate_c8 in the same launch.
 *   iiseg_relu_gate_c8    out = g where pooled > 0, else +0 (relu'(0) = 0); g, pooled, out (B, C8n, h2, w2, 8)
 *                         bf16; out may be g.
 * Max-pool + ReLU backward on C8 is the gate followed by DePool2D of the gated map under the level's own mask
 * bytes (IISEG_CONV_UNPOOL staging of iiseg_conv_c8, or iiseg_unpool_c8).  Before any launch: NULL operands
 * IISEG_ERR_NULL; non-positive sizes, odd C8n, a window outside the planes, PH < 2 h2 or PW < 2 w2
 * IISEG_ERR_SHAPE; tensors not 16-byte (mask: 8-byte) aligned IISEG_ERR_ALIGN; out aliasing gu / gate
 * (depool_bwd) or pooled (relu_gate) IISEG_ERR_UNSUPPORTED. */
int iiseg_depool_bwd_c8(void* stream, const void* gu, const uint8_t* mask, const void* gate, void* out, int B,
                        int C8n, int PH, int PW, int h2, int w2, int y0, int x0, int wh, int ww);
int iiseg_relu_gate_c8(void* stream, const void* g, const void* pooled, void* out, int B, int C8n, int h2, int w2,
                       int y0, int x0, int wh, int ww);
/* The same layer for AT MOST 16 OUTPUT CHANNELS (csrc/conv_c8_m16.hip: v_mfma_f32_16x16x32_bf16, M = 16
 * channels, 16-pixel blocks, 256-pixel th x tw tiles, three workgroups per CU): the DAE's class-score
 * layer (models/fcn_up.py:83-86) and FC-DenseNet's growth-rate-16 dense-block layers
 * (models/FCDenseNet.py:61-146).  Single source (d->C2 == 0), d->C1 = the channels convolved (a multiple
 * of 16): the FIRST d->C1 channels of x1, a C8 tensor of in_ctot >= d->C1 channels per image (0: d->C1).
 *   mask_in     with IISEG_CONV_UNPOOL, as in iiseg_conv_c8
 *   bn_a, bn_b  both NULL, or d->C1 floats each: BatchNorm + ReLU applied to the input while it is staged,
 *               x <- max(bn_a[c] x + bn_b[c], 0) rounded to bf16 (iiseg_bn_fold_f32 makes the pair from
 *               beta, gamma, mean, inv_std); the zero-padding ring stays zero
 *   out         out_kind 1: C8 bf16, the 16 channels [out_c0, out_c0 + 16) of a (B, out_ctot / 8, out_H,
 *               out_W, 8) tensor (out_ctot 0: a dense 16-channel tensor), channels past Cout zero;
 *               out_kind 3: fp32 NCHW (B, out_ctot or Cout, out_H, out_W)
 * weights: iiseg_conv_halo_bf16_pack for this Cout (rows padded to 32).  No add, no pool.
 * iiseg_bn_stats_c8: batch statistics (mean, 1 / sqrt(biased var + eps); P10) of channels [c0, c0 + n) of
 * a C8 tensor of Ctot channels (all multiples of 8), two deterministic stages in double; workspace:
 * iiseg_bn_stats_c8_workspace_elems(n) doubles, caller-owned. */
int iiseg_conv_c8_m16_supported(const iiseg_conv_desc* d);
int iiseg_conv_c8_m16(void* stream, const iiseg_conv_desc* d, const void* x1, int in_ctot,
                      const uint8_t* mask_in, const float* bn_a, const float* bn_b, const void* wp16,
                      const float* bias, void* out, int out_kind);
/* The same with a caller-owned scratch buffer for SPLIT-K launches: on small maps (one tile per image, 40+
 * k-tiles in sequence: the deep dense blocks of FC-DenseNet at 7^2 .. 28^2) the channel range is dealt to
 * 16 / tiles-per-image workgroups per tile, each sums its share from zero into an fp32 slab, and a second
 * launch (one workgroup per tile) adds the slabs in slice order and writes the result -- a fixed association
 * that depends on the layer geometry only, never on the batch.  workspace: iiseg_conv_c8_m16_workspace_bytes(d)
 * bytes (it also holds the per-tile statistics below), 16-byte aligned.  Without a workspace the launch is
 * not split (iiseg_conv_c8_m16). */
int64_t iiseg_conv_c8_m16_workspace_bytes(const iiseg_conv_desc* d);
/* Two more fusions of a dense-block layer (models/FCDenseNet.py:88-92) ride on the same entry point:
 *   stat_mean / stat_inv_std (bf16 C8 output only, needs the workspace): the batch statistics (biased variance,
 *     stat_eps; P10) of the 16 produced channels -- of the stored bf16 values, per-tile sums in double out of the
 *     conv's epilogue, added in a fixed order by a one-workgroup reduction -- written to entries [out_c0,
 *     out_c0 + 16) of the two vectors (iiseg_bn_stats_c8's result up to the order of the double sums);
 *   fold_* (with the statistics): that reduction then also forms the (a, b) pair of the NEXT consumer's
 *     BatchNorm over the first fold_n channels of the stack from the two vectors (iiseg_bn_fold_f32's
 *     arithmetic, one launch less per layer). */
int iiseg_conv_c8_m16_ws(void* stream, const iiseg_conv_desc* d, const void* x1, int in_ctot,
                         const uint8_t* mask_in, const float* bn_a, const float* bn_b, const void* wp16,
                         const float* bias, void* out, int out_kind, void* workspace,
                         int64_t workspace_bytes, float* stat_mean, float* stat_inv_std, double stat_eps,
                         const float* fold_beta, const float* fold_gamma, float* fold_a, float* fold_b,
                         int fold_n);
/* 1x1 convolution on a bf16 C8 tensor (csrc/conv1x1_c8.hip): FC-DenseNet's TransitionDown (BN -> ReLU -> 1x1
 * conv -> 2x2 max-pool, FC_DenseNet.layers.TransitionDown at models/FCDenseNet.py:95) and the SoftmaxLayer's
 * 1x1 score convolution (models/FCDenseNet.py:134) on the dense block's stack.
 *   x        (B, in_ctot / 8, H, W, 8) bf16; the layer reads its first Cin channels (Cin % 16 == 0)
 *   bn_a/b   NULL, or the folded BatchNorm of those channels (iiseg_bn_fold_f32): x <- max(a x + b, 0)
 *   wp       iiseg_conv1x1_c8_pack of w[Cout][Cin_w] (iiseg_conv1x1_c8_weight_bytes bytes)
 *   pool 1:  out = bf16 C8 (B, out_ctot / 8, H / 2, W / 2, 8); channels [out_c0, out_c0 + Cout) receive
 *            maxpool2x2(conv) + bias (ignore_border), a partial last chunk is zero-padded
 *   pool 0:  out = fp32 NCHW (B, Cout, H, W) = conv + bias (out_ctot, out_c0 ignored) */
int64_t iiseg_conv1x1_c8_weight_bytes(int Cout, int Cin);
int iiseg_conv1x1_c8_pack(void* stream, const float* w, int64_t stride_o, int64_t stride_c, int Cout,
                          int Cin_w, int Cin, void* wp);
int iiseg_conv1x1_c8(void* stream, const void* x, int B, int Cin, int in_ctot, int H, int W,
                     const float* bn_a, const float* bn_b, const void* wp, const float* bias, int Cout,
                     int pool, void* out, int out_ctot, int out_c0);
int iiseg_bn_fold_f32(void* stream, const float* beta, const float* gamma, const float* mean,
                      const float* inv_std, float* a, float* b, int n);
int64_t iiseg_bn_stats_c8_workspace_elems(int n);
int iiseg_bn_stats_c8(void* stream, const void* x, int B, int Ctot, int c0, int n, int H, int W,
                      double eps, float* mean, float* inv_std, double* workspace);
int iiseg_nchw_to_c8(void* stream, const float* x, void* out, int B, int C, int H, int W, int C8n);
int iiseg_c8_to_nchw(void* stream, const void* x, float* out, int B, int C, int H, int W, int C8n);
/* The same between a dense fp32 (B, C, H, W) tensor and the chunk planes [c8_0, c8_0 + ceil(C / 8)) of a
 * WIDER C8 tensor of C8tot planes per image (a dense block's stack: models/FCDenseNet.py:92,119-127). */
int iiseg_nchw_to_c8_slice(void* stream, const float* x, void* out, int B, int C, int H, int W, int C8tot,
                           int c8_0);
int iiseg_c8_slice_to_nchw(void* stream, const void* x, float* out, int B, int C, int H, int W, int C8tot,
                           int c8_0);
int iiseg_pool_mask_c8(void* stream, const void* pre, int pre_f32, void* pooled, uint8_t* mask,
                       int BC8, int PH, int PW, int py0, int px0, int H, int W, int y0, int x0, int wh,
                       int ww);
/* The helpers of the IISEG_CONV_X3 mode: fp32 NCHW <-> hi / lo pair (B, 2 C8n, H, W, 8), and the
 * pool of a C8 fp32 piece `pre` (B, C8n, PH, PW, 8) into a pooled hi / lo pair (B, 2 C8n, H/2, W/2, 8)
 * + the (B, C8n, H/2, W/2, 8) mask bytes (same comparisons as iiseg_pool_mask_c8 with pre_f32). */
/* iiseg_conv_c8_split_weights: the filter of an IISEG_CONV_X3 layer, w[co][c][3][3] (element strides
 * stride_o / stride_c as in iiseg_conv_pack_f32) -> out (Cout, 2 Cp, 3, 3) floats = [W_hi | W_lo] with
 * Cp = Cin rounded up to 16, ready for iiseg_conv_halo_bf16_pack with C1 = 2 Cp. */
int iiseg_conv_c8_split_weights(void* stream, const float* w, int64_t stride_o, int64_t stride_c,
                                int Cout, int Cin, float* out);
int iiseg_nchw_to_c8x3(void* stream, const float* x, void* out, int B, int C, int H, int W, int C8n);
int iiseg_c8x3_to_nchw(void* stream, const void* x, float* out, int B, int C, int H, int W, int C8n);
int iiseg_pool_mask_c8x3(void* stream, const void* pre, void* pooled, uint8_t* mask, int B, int C8n,
                         int PH, int PW, int py0, int px0, int H, int W, int y0, int x0, int wh,
                         int ww);

/* im2col + split-K GEMM form of iiseg_conv_f32 for 'valid' (pad 0, dil 1) KxK layers computed in
 * full into a dense output (FCN-8's fc6, models/fcn8.py:75-76): same packed weights `wp` (d->Kpad,
 * d->Mpad from iiseg_conv_plan), the gather-free MFMA GEMM kernel of the Winograd path, partial
 * sums of the K slices added in a fixed order.  workspace: iiseg_conv_gemm_workspace_elems floats;
 * stages: IISEG_WINO_INPUT (im2col) | IISEG_WINO_GEMM | IISEG_WINO_OUTPUT, IISEG_WINO_ALL normally. */
int iiseg_conv_gemm_supported(const iiseg_conv_desc* d);
int64_t iiseg_conv_gemm_workspace_elems(const iiseg_conv_desc* d);
int iiseg_conv_gemm_f32(void* stream, const iiseg_conv_desc* d, const float* x, const float* wp,
                        const float* bias, float* workspace, float* out, uint32_t stages);

/* ---------------------------------------------------------------------------------------
 * 2x2/2 max-pool, ignore_border (floor).  Replaces Pool2DLayer(x, 2): models/fcn8.py:38-72,
 * models/fcn_down.py:122.   x (B,C,H,W) -> out (B,C,H/2,W/2)
 * ------------------------------------------------------------------------------------- */
int iiseg_maxpool2x2_f32(void* stream, const float* x, float* out, int32_t BC, int32_t H,
                         int32_t W);

/* The same for pooled outputs [y0,y0+wh) x [x0,x0+ww) only, written in place into the (H/2, W/2)
 * planes of `out` (loop-invariant borders of the refinement loop are not recomputed). */
int iiseg_maxpool2x2_window_f32(void* stream, const float* x, float* out, int32_t BC, int32_t H,
                                int32_t W, int32_t y0, int32_t x0, int32_t wh, int32_t ww);
int iiseg_maxpool2x2_window_f64(void* stream, const double* x, double* out, int32_t BC, int32_t H,
                                int32_t W, int32_t y0, int32_t x0, int32_t wh, int32_t ww);
/* iiseg_maxpool2x2_window_f32 that also writes the DePool2D mask bytes of those windows into `mask`
 * (uint8, the shape of `out`; bit (y & 1) * 2 + (x & 1) = x == out, see iiseg_conv_mask_f32): for
 * layers whose own epilogue cannot pool (Winograd layers at an odd tile anchor), so that the decoder
 * still reads up + mask bytes instead of the pre-pool map. */
int iiseg_maxpool2x2_mask_window_f32(void* stream, const float* x, float* out, uint8_t* mask,
                                     int32_t BC, int32_t H, int32_t W, int32_t y0, int32_t x0,
                                     int32_t wh, int32_t ww);

/* Equality-mask unpool, materialised (the fused form is IISEG_CONV_UNPOOL).  Replaces
 * DePool2D.get_output_for, layers/mylayers.py:88-115:
 * out[y,x] = (y < 2h && x < 2w && pre[y,x] == pooled[y/2,x/2]) ? up[y/2,x/2] : 0 */
int iiseg_unpool_eqmask_f32(void* stream, const float* up, const float* pre,
                            const float* pooled, float* out, int32_t BC, int32_t H, int32_t W);
/* The same, restricted to the window [y0,y0+wh) x [x0,x0+ww) of the (H,W) planes (in place:
 * elements outside the window are not written). */
int iiseg_unpool_eqmask_window_f32(void* stream, const float* up, const float* pre,
                                   const float* pooled, float* out, int32_t BC, int32_t H,
                                   int32_t W, int32_t y0, int32_t x0, int32_t wh, int32_t ww);

/* ---------------------------------------------------------------------------------------
 * Small-channel transposed convolution (gather form), crop='valid', linear.
 * Replaces Deconv2DLayer (Theano CorrMM_gradInputs): models/fcn8.py:90,100,109;
 * models/fcn_up.py:41-45.  w is the reference layout W[Cin][Cout][K][K]; the kernel applies
 * the spatial flip of Lasagne's filter_flip=True gradient form.
 * Only the window [oy0,oy0+OH) x [ox0,ox0+OW) of the (H-1)*s+K output is produced.
 * Optional: out += add[b, c, ay0+oy, ax0+ox] (add is (B,Cout,AH,AW)); Cout <= 32.
 * ------------------------------------------------------------------------------------- */
typedef struct iiseg_deconv_desc {
    int32_t B, Cin, H, W, Cout, K, stride;
    int32_t oy0, ox0, OH, OW;
    int32_t AH, AW, ay0, ax0;
} iiseg_deconv_desc;

int iiseg_deconv_f32(void* stream, const iiseg_deconv_desc* d, const float* x, const float* w,
                     const float* bias, const float* add, float* out);

/* The same layer by output phase (csrc/deconv_phase.hip): K = 2 * stride, stride 2 or 8, at most 16 channels
 * on either side -- the three FCN-8 upsamplers (models/fcn8.py:90,100,109).  A thread owns an input position
 * and a row phase; the weights are scalar operands.  Same sums in the same order as iiseg_deconv_*.
 * iiseg_deconv_phase_supported: 1 when the request (with / without a skip tensor, f32 / f64) has this form;
 * iiseg_deconv_phase_weight_elems: elements of the packed weight buffer [py][dy][dx][Cin][px][Cout padded];
 * iiseg_deconv_phase_pack_*: W[Cin][Cout][K][K] -> that buffer (once per layer);
 * iiseg_deconv_phase_*: the launch, arguments as iiseg_deconv_* with the packed weights for w. */
int iiseg_deconv_phase_supported(const iiseg_deconv_desc* d, int has_add, int is_f64);
int64_t iiseg_deconv_phase_weight_elems(const iiseg_deconv_desc* d);
int iiseg_deconv_phase_pack_f32(void* stream, const iiseg_deconv_desc* d, const float* w, float* wp);
int iiseg_deconv_phase_pack_f64(void* stream, const iiseg_deconv_desc* d, const double* w, double* wp);
int iiseg_deconv_phase_f32(void* stream, const iiseg_deconv_desc* d, const float* x, const float* wp,
                           const float* bias, const float* add, float* out);
int iiseg_deconv_phase_f64(void* stream, const iiseg_deconv_desc* d, const double* x, const double* wp,
                           const double* bias, const double* add, double* out);

/* ---------------------------------------------------------------------------------------
 * Channel softmax of a center-cropped score map.  Replaces the crop + dimshuffle + reshape +
 * softmax + reshape + dimshuffle tail of models/fcn8.py:115-130,187-191 and
 * models/fcn_up.py:104-113,154-169.   score (B,C,SH,SW) -> out (B,C,H,W), window at (sy0,sx0),
 * C <= 32.  If `minuend` (B,C,H,W) is non-NULL the result is minuend - softmax, which is
 * de_fn's  -(pred_dae - y_hat)  of iterative_inference.py:203-204.
 * ------------------------------------------------------------------------------------- */
int iiseg_crop_softmax_f32(void* stream, const float* score, const float* minuend, float* out,
                           int32_t B, int32_t C, int32_t SH, int32_t SW, int32_t sy0,
                           int32_t sx0, int32_t H, int32_t W);

/* ---------------------------------------------------------------------------------------
 * Fused refinement step.  Replaces, per image, iterative_inference.py:203-204 (de = y - r),
 * :270 (y - step*de), :273 (clip) and the per-pixel part of :275 (||de||_2 over channels):
 *   r = softmax_c(score[window]); de = y - r; if active[b]: y = clip(y - step*de, 0, 1)
 *   partial[b][blk] = sum over the block's pixels of ||de||_2
 * y (B,C,H,W) is updated in place; active (B) int32; partial (B, nblk) float64 where
 * nblk = iiseg_refine_partials(H, W).
 * iiseg_refine_finalize then applies :275-277 per image: norm = sum(partial[b])/(H*W);
 * if active[b]: iters[b] += 1; if norm < eps: active[b] = 0   (update first, then test).
 * ------------------------------------------------------------------------------------- */
int iiseg_refine_partials(int32_t H, int32_t W);
int iiseg_refine_update_f32(void* stream, const float* score, float* y, const int32_t* active,
                            double* partial, int32_t B, int32_t C, int32_t SH, int32_t SW,
                            int32_t sy0, int32_t sx0, int32_t H, int32_t W, float step);
/* iiseg_refine_update_f32 that also writes the updated map as a bf16 C8 tensor y8 (B, C8n, H, W, 8)
 * -- the input format of the DAE's first layer under mma='bf16c8' (iiseg_conv_c8): the conversion
 * pass per refinement step disappears. */
int iiseg_refine_update_c8_f32(void* stream, const float* score, float* y, const int32_t* active,
                               double* partial, void* y8, int32_t C8n, int32_t B, int32_t C,
                               int32_t SH, int32_t SW, int32_t sy0, int32_t sx0, int32_t H, int32_t W,
                               float step);
int iiseg_refine_finalize(void* stream, const double* partial, int32_t* active, int32_t* iters,
                          double* last_norm, int32_t B, int32_t nblk, int32_t HW, double eps);

/* ---------------------------------------------------------------------------------------
 * The context module's last layers and the refinement update as ONE launch.  Replaces
 * models/contextmod_dae.py:98-105 (dilconv6: 3x3 'valid' + ReLU; dilconv7: 1x1 linear; softmax) followed
 * by iterative_inference.py:203-204, 270-277 -- i.e. iiseg_conv_f32 (3x3) + iiseg_conv_f32 (1x1) +
 * iiseg_refine_update_f32 -- for C <= 16 channels on either side (csrc/conv_small.hip):
 *   t = relu(conv3x3_valid(x; wp6, b6)); score = conv1x1(t; wp7, b7); then the refinement step above on
 *   y (B,C,H,W), in place, with the updated y of active images ALSO stored into channels
 *   [cat_c0, cat_c0 + C) of ycat (B, cat_ctot, cat_H, cat_W) at (cat_y0, cat_x0) (the ConcatLayer((h, y))
 *   buffer of contextmod_dae.py:55-59 the next step's first layer reads; NULL: no mirror).
 * x (B, C, H + 2, W + 2); wp6 / wp7: Wp[K][Mpad] of iiseg_conv_pack_f32 for the two layers; partial
 * (B, nblk) with nblk = iiseg_ctx_tail_partials(H, W) -- pass that nblk to iiseg_refine_finalize.
 * y is bit-identical to the three separate launches; the partials are summed per 16 x 64 tile.
 * ------------------------------------------------------------------------------------- */
int iiseg_ctx_tail_partials(int32_t H, int32_t W);
int iiseg_ctx_tail_f32(void* stream, const float* x, const float* wp6, int32_t Mpad6, const float* b6,
                       const float* wp7, int32_t Mpad7, const float* b7, float* y, const int32_t* active,
                       double* partial, float* ycat, int32_t cat_ctot, int32_t cat_c0, int32_t cat_H,
                       int32_t cat_W, int32_t cat_y0, int32_t cat_x0, int32_t B, int32_t C, int32_t H,
                       int32_t W, float step);

/* ---------------------------------------------------------------------------------------
 * Metrics accumulator.  Replaces val_fn, iterative_inference.py:206-210 = metrics.py:11-37
 * (jaccard), :40-65 (accuracy), :144-156 (squared_error, int-void branch):
 *   cm[i*(C+1) + j] += #(argmax_c y == i  and  argmax_c t == j), i < C, j <= C (j == C: void)
 *   sums[0] += sum_px mask * mean_c (y - t[:C])^2 ;  sums[1] += sum_px mask, mask = sum_c t[:C]
 * y (B,C,H,W), t one-hot (B,C+1,H,W) with void last.  cm: C*(C+1) int64, sums: 2 float64,
 * both ACCUMULATED into (zero them first); C <= 31.
 * ------------------------------------------------------------------------------------- */
int iiseg_confusion_f32(void* stream, const float* y, const float* t, int64_t* cm, double* sums,
                        int32_t B, int32_t C, int32_t HW);

/* Same accumulation restricted to images with active[b] != 0.  Used for the per-iteration Jaccard
 * of the validation driver (iterative_inference_valid.py:231,280-288: `valid_mat[:, :, it] +=
 * jacc_iter` only for images still iterating). */
int iiseg_confusion_masked_f32(void* stream, const float* y, const float* t, const int32_t* active,
                               int64_t* cm, double* sums, int32_t B, int32_t C, int32_t HW);
int iiseg_confusion_masked_f64(void* stream, const double* y, const double* t,
                               const int32_t* active, int64_t* cm, double* sums, int32_t B,
                               int32_t C, int32_t HW);

/* Non-finite input detection: *counter += number of NaN / Inf elements of x[0, n) (device counter, no
 * synchronisation).  The fp32 / bf16 kernels do not promise to propagate a NaN that enters the network (their
 * ReLU / max-pool epilogues are bare v_max_f32: build.py EXTRA_FLAGS), where the reference's Theano ops do
 * (models/fcn_down.py:102-104 `rectify`); the product detects non-finite values where they enter instead:
 * weights when a layer is built, image batches here. */
int iiseg_count_nonfinite_f32(void* stream, const float* x, int64_t n, int32_t* counter);
int iiseg_count_nonfinite_f64(void* stream, const double* x, int64_t n, int32_t* counter);

/* ---------------------------------------------------------------------------------------
 * True-gradient mode (BASELINE north_star; NOT in the reference, whose
 * "gradient" is the residual r - y):  E(y) = sum_{c,px} (r(y|h) - y)^2,
 * dE/dy = J_r^T 2(r - y) - 2(r - y).  The convolutions' backward-data passes run on the forward
 * conv entry points with channel-transposed, spatially flipped weights; these are the other
 * adjoints.  All tensors dense NCHW.
 *   sqerr_softmax_bwd : gscore = softmax backward of g_r = 2 (softmax(score window) - y)
 *   depool_bwd        : adjoint of DePool2D w.r.t. its input: masked 2x2 sum (mask pre == pooled)
 *   pool_relu_bwd     : adjoint of maxpool2x2(relu(z)) w.r.t. z given pre = relu(z): the gradient
 *                       goes to every position equal to the window maximum (F4 mask), relu'(0) = 0
 *   grad_update       : grad = gthrough - 2 (r - y); y <- clip(y - step * grad, 0, 1); norm
 *                       partials of grad as in iiseg_refine_update_*
 * ------------------------------------------------------------------------------------- */
int iiseg_sqerr_softmax_bwd_f32(void* stream, const float* score, const float* y, float* gscore,
                                int32_t B, int32_t C, int32_t SH, int32_t SW, int32_t sy0,
                                int32_t sx0, int32_t H, int32_t W);
int iiseg_sqerr_softmax_bwd_f64(void* stream, const double* score, const double* y, double* gscore,
                                int32_t B, int32_t C, int32_t SH, int32_t SW, int32_t sy0,
                                int32_t sx0, int32_t H, int32_t W);
int iiseg_depool_bwd_f32(void* stream, const float* gout, const float* pre, const float* pooled,
                         float* gup, int32_t BC, int32_t H, int32_t W);
int iiseg_depool_bwd_f64(void* stream, const double* gout, const double* pre, const double* pooled,
                         double* gup, int32_t BC, int32_t H, int32_t W);
int iiseg_pool_relu_bwd_f32(void* stream, const float* gpool, const float* pre, const float* pooled,
                            float* gz, int32_t BC, int32_t H, int32_t W);
int iiseg_pool_relu_bwd_f64(void* stream, const double* gpool, const double* pre,
                            const double* pooled, double* gz, int32_t BC, int32_t H, int32_t W);
int iiseg_grad_update_f32(void* stream, const float* score, const float* gthrough, float* y,
                          const int32_t* active, double* partial, int32_t B, int32_t C, int32_t SH,
                          int32_t SW, int32_t sy0, int32_t sx0, int32_t H, int32_t W, float step);
int iiseg_grad_update_f64(void* stream, const double* score, const double* gthrough, double* y,
                          const int32_t* active, double* partial, int32_t B, int32_t C, int32_t SH,
                          int32_t SW, int32_t sy0, int32_t sx0, int32_t H, int32_t W, double step);

/* ---------------------------------------------------------------------------------------
 * Element-wise helpers of the optional noise>0 mask emulation: with
 * dae_dict['noise'] > 0 the reference's DePool2D masks come from a re-evaluation of the down path
 * with GaussianNoiseLayer / DropoutLayer ACTIVE (layers/mylayers.py:91-93, models/fcn_down.py:60-63,
 * 108-111).  The caller supplies the random tensors.
 *   add_noise     : out = x + sigma * eps                       (GaussianNoiseLayer)
 *   dropout_apply : x = x * keep / (1 - p), keep in {0, 1}       (DropoutLayer, rescale=True)
 * ------------------------------------------------------------------------------------- */
int iiseg_add_noise_f32(void* stream, const float* x, const float* eps, float sigma, float* out,
                        int64_t n);
int iiseg_add_noise_f64(void* stream, const double* x, const double* eps, double sigma, double* out,
                        int64_t n);
int iiseg_dropout_apply_f32(void* stream, float* x, const float* keep, float p, int64_t n);
int iiseg_dropout_apply_f64(void* stream, double* x, const double* keep, double p, int64_t n);

/* ---------------------------------------------------------------------------------------
 * Batch-statistics BatchNorm (+ReLU).  Replaces lasagne BatchNormLayer under
 * batch_norm_use_averages=False (iterative_inference.py:187) followed by the rectify
 * NonlinearityLayer of FC-DenseNet's BN_ReLU_Conv (models/FCDenseNet.py:12,90,109,123).
 * x is (B, >=C, H, W) with `bstride` elements between images (a channel-slice view of a stack).
 *   stats : mean[c], inv_std[c] = 1/sqrt(biased_var + eps) over (B,H,W) for c < C
 *   apply : out[b,c] = max((x[b,c] - mean[c]) * (gamma[c] * inv_std[c]) + beta[c], 0), out dense
 * ------------------------------------------------------------------------------------- */
int64_t iiseg_bn_stats_workspace_elems(int32_t C); /* doubles of caller-owned workspace */
int iiseg_bn_stats_f32(void* stream, const float* x, int64_t bstride, int32_t B, int32_t C,
                       int32_t HW, float eps, float* mean, float* inv_std, double* workspace);
int iiseg_bn_relu_f32(void* stream, const float* x, int64_t bstride, int32_t B, int32_t C,
                      int32_t HW, const float* beta, const float* gamma, const float* mean,
                      const float* inv_std, float* out);
/* Stored-average BatchNorm of the DAE's bn=1 layers (lasagne BatchNormLayer at deterministic=True:
 * models/fcn_down.py:112-114, models/fcn_up.py:91-93 under iterative_inference.py:189), in place on
 * the window [y0,y0+wh) x [x0,x0+ww) of the (H,W) planes of x (B,C,H,W):
 *   x = (x - mean[c]) * (gamma[c] * inv_std[c]) + beta[c] */
int iiseg_bn_affine_window_f32(void* stream, float* x, int32_t B, int32_t C, int32_t H, int32_t W,
                               int32_t y0, int32_t x0, int32_t wh, int32_t ww, const float* beta,
                               const float* gamma, const float* mean, const float* inv_std);
int iiseg_bn_affine_window_f64(void* stream, double* x, int32_t B, int32_t C, int32_t H, int32_t W,
                               int32_t y0, int32_t x0, int32_t wh, int32_t ww, const double* beta,
                               const double* gamma, const double* mean, const double* inv_std);
int iiseg_bn_stats_f64(void* stream, const double* x, int64_t bstride, int32_t B, int32_t C,
                       int32_t HW, double eps, double* mean, double* inv_std, double* workspace);
int iiseg_bn_relu_f64(void* stream, const double* x, int64_t bstride, int32_t B, int32_t C,
                      int32_t HW, const double* beta, const double* gamma, const double* mean,
                      const double* inv_std, double* out);

/* ---------------------------------------------------------------------------------------
 * Training FC-DenseNet (csrc/bn_grad.hip).
 * bn_relu_bwd : backward of t = relu(y), y = gamma xhat + beta, xhat = (x - mean) inv_std with BATCH statistics
 *   (mean, inv_std those of x over (B,H,W), N = B HW), for one consumer of a stack: x and gstack are the first C
 *   channels of (B, >=C, H, W) buffers with `bstride` elements between images, g_t = dL/dt is dense (B,C,H,W).
 *     IISEG_BN_BWD_REDUCE : dbeta[c] = sum g_y, dgamma[c] = sum g_y xhat, g_y = g_t [y > 0] (relu'(0) = 0), y
 *                           recomputed from x as iiseg_bn_relu_* forms it; double partial sums in a fixed order
 *                           through `workspace` (iiseg_bn_relu_bwd_workspace_elems(C, HW) doubles: two per channel
 *                           and chunk of the plane), no atomics
 *     IISEG_BN_BWD_APPLY  : gstack[b,c] += gamma[c] inv_std[c] (g_y - dbeta[c] / N - xhat dgamma[c] / N), reading
 *                           dbeta / dgamma
 *   `stages`: either or both (reduce first).  Nothing but gstack's first C channels, dbeta, dgamma and the workspace
 *   is written.  16-byte accesses when HW and bstride are multiples of 16 bytes of elements and x, g_t, gstack are
 *   16-byte aligned; scalar ones otherwise.
 * maxpool2x2_bwd : gz[y,x] = pre[y,x] == pooled[y/2,x/2] ? gpool[y/2,x/2] : 0 inside (2 (H/2), 2 (W/2)), 0 outside:
 *   iiseg_pool_relu_bwd_* without the > 0 gate (the pool of a linear map).  pre, gz (BC,H,W); gpool, pooled
 *   (BC,H/2,W/2).
 * ------------------------------------------------------------------------------------- */
#define IISEG_BN_BWD_REDUCE 1
#define IISEG_BN_BWD_APPLY 2
int64_t iiseg_bn_relu_bwd_workspace_elems(int32_t C, int32_t HW);
int iiseg_bn_relu_bwd_f32(void* stream, const float* x, int64_t bstride, const float* g_t, float* gstack,
                          int32_t B, int32_t C, int32_t HW, const float* beta, const float* gamma,
                          const float* mean, const float* inv_std, float* dbeta, float* dgamma,
                          double* workspace, int32_t stages);
int iiseg_bn_relu_bwd_f64(void* stream, const double* x, int64_t bstride, const double* g_t, double* gstack,
                          int32_t B, int32_t C, int32_t HW, const double* beta, const double* gamma,
                          const double* mean, const double* inv_std, double* dbeta, double* dgamma,
                          double* workspace, int32_t stages);
int iiseg_maxpool2x2_bwd_f32(void* stream, const float* gpool, const float* pre, const float* pooled,
                             float* gz, int32_t BC, int32_t H, int32_t W);
int iiseg_maxpool2x2_bwd_f64(void* stream, const double* gpool, const double* pre, const double* pooled,
                             double* gz, int32_t BC, int32_t H, int32_t W);

/* ---------------------------------------------------------------------------------------
 * float64 variants (strict-parity mode).  The reference's CPU path computes in float64 (Theano
 * floatX default) and DePool2D compares activations for exact equality, so only
 * float64 arithmetic reproduces its mask decisions at near-tied pooling windows.
 * Same semantics and argument meaning as the _f32 entry points; tensors are float64.
 * iiseg_conv_*_f64 cover 1x1 and 3x3 filters (v_mfma_f64_16x16x4_f64); other filter shapes go
 * through iiseg_im2col_f64 + a 1x1 convolution (fc6 of models/fcn8.py:75-76), whose weight matrix
 * is the reference W[out][in*KH*KW] as it lies in memory.  No gather table is needed.
 * ------------------------------------------------------------------------------------- */
int iiseg_conv_plan_f64(iiseg_conv_desc* d);
int iiseg_conv_pack_f64(void* stream, const iiseg_conv_desc* d, const double* w, int64_t stride_o,
                        int64_t stride_c, double* wp);
int iiseg_conv_f64(void* stream, const iiseg_conv_desc* d, const double* x1, const double* x2,
                   const double* pre, const double* pooled, const double* wp, const double* bias,
                   const double* add, double* out);
/* iiseg_conv_f64 with the 2x2 max-pool (Pool2DLayer(x, 2), ignore_border) of the result fused into the epilogue
 * of the halo-tile kernel: pool_out = the FULL pooled tensor (B, Cout, fullH / 2, fullW / 2), written where the
 * computed window has whole pooling windows (as iiseg_conv_pool_f32; out is still stored: DePool2D compares the
 * float64 pre-pool map). */
int iiseg_conv_pool_f64_supported(const iiseg_conv_desc* d);
int iiseg_conv_pool_f64(void* stream, const iiseg_conv_desc* d, const double* x1, const double* x2,
                        const double* pre, const double* pooled, const double* wp, const double* bias,
                        const double* add, double* out, double* pool_out);
/* ... and with the DePool2D masks as bytes (iiseg_conv_mask_f32's convention: bit (y & 1) * 2 + (x & 1) of the
 * window's byte = pre == pooled, here compared in FLOAT64 by the encoder layer's epilogue, so the decisions are
 * those of the pre / pooled form): mask_out (uint8, pool_out's shape) is written next to the pool and `out`
 * may then be NULL -- the float64 pre-pool map is never stored; mask_in (uint8, x1's shape) replaces pre /
 * pooled in the DePool2D staging of the decoder layer. */
int iiseg_conv_mask_f64_supported(const iiseg_conv_desc* d);
int iiseg_conv_mask_f64(void* stream, const iiseg_conv_desc* d, const double* x1, const double* x2,
                        const double* pre, const double* pooled, const uint8_t* mask_in, const double* wp,
                        const double* bias, const double* add, double* out, double* pool_out,
                        uint8_t* mask_out);
/* 1 when iiseg_conv_f64 runs this (planned) request on the halo-tile kernel (conv_halo_f64.hip: plain
 * 3x3 layers, patch staged once per 4 input channels, 16-row MFMA tiles for Cout <= 16) instead of the
 * static-tap kernel; same packed weights, bit-identical results -- a scheduling fact, for profiles. */
int iiseg_conv_halo_f64_supported(const iiseg_conv_desc* d);
/* Split-K GEMM form of iiseg_conv_f64 for deep 1x1 layers computed in full into a dense output (fc6 after
 * iiseg_im2col_f64, fc7, score_fr: models/fcn8.py:75-85): x (B, C1, H, W) is laid out once as V[k][pixel],
 * then the LDS-DMA GEMM kernel of the float64 Winograd path runs on the same packed weights `wp`
 * (iiseg_conv_plan_f64 / _pack_f64); the partial sums of the K slices are added in a fixed order, and the
 * number of slices does not depend on the batch.  workspace: iiseg_conv_gemm_f64_workspace_elems doubles. */
int iiseg_conv_gemm_f64_supported(const iiseg_conv_desc* d);
int64_t iiseg_conv_gemm_f64_workspace_elems(const iiseg_conv_desc* d);
int iiseg_conv_gemm_f64(void* stream, const iiseg_conv_desc* d, const double* x, const double* wp,
                        const double* bias, double* workspace, double* out);
/* x (B,C,H,W) -> out (B, C*KH*KW, H-KH+1, W-KW+1), channel index c*KH*KW + ky*KW + kx */
int iiseg_im2col_f64(void* stream, const double* x, double* out, int32_t B, int32_t C, int32_t H,
                     int32_t W, int32_t KH, int32_t KW);
int iiseg_maxpool2x2_f64(void* stream, const double* x, double* out, int32_t BC, int32_t H,
                         int32_t W);
int iiseg_unpool_eqmask_f64(void* stream, const double* up, const double* pre,
                            const double* pooled, double* out, int32_t BC, int32_t H, int32_t W);
int iiseg_unpool_eqmask_window_f64(void* stream, const double* up, const double* pre,
                                   const double* pooled, double* out, int32_t BC, int32_t H,
                                   int32_t W, int32_t y0, int32_t x0, int32_t wh, int32_t ww);
int iiseg_deconv_f64(void* stream, const iiseg_deconv_desc* d, const double* x, const double* w,
                     const double* bias, const double* add, double* out);
int iiseg_crop_softmax_f64(void* stream, const double* score, const double* minuend, double* out,
                           int32_t B, int32_t C, int32_t SH, int32_t SW, int32_t sy0,
                           int32_t sx0, int32_t H, int32_t W);
int iiseg_refine_update_f64(void* stream, const double* score, double* y, const int32_t* active,
                            double* partial, int32_t B, int32_t C, int32_t SH, int32_t SW,
                            int32_t sy0, int32_t sx0, int32_t H, int32_t W, double step);
int iiseg_confusion_f64(void* stream, const double* y, const double* t, int64_t* cm, double* sums,
                        int32_t B, int32_t C, int32_t HW);

/* ---------------------------------------------------------------------------------------
 * Dense-CRF mean field (the "FCN-8 + CRF" baseline of the reference's crf_inference.py:143-192, which
 * calls pydensecrf's DenseCRF2D).  Model (DESIGN.md "Dense-CRF baseline"): unary
 * U = -log(clamp(P, clip, 1)); Q0 = softmax(-U); colour features I = clamp(floor(255 x), 0, 255) per
 * channel (x taken as already on 0..255 with IISEG_CRF_INPUT_0_255); kernels
 *   k_g(i,j) = exp(-d^2 / (2 sxy_g^2)),  k_b(i,j) = exp(-d^2 / (2 sxy_b^2) - |I_i - I_j|^2 / (2 srgb^2))
 * summed EXACTLY over the in-image pixels j with |dx|, |dy| <= R (j = i included; pydensecrf
 * approximates the sums on a permutohedral lattice); symmetric normalisation
 * n^k_i = 1 / sqrt(sum_j k(i,j)); one iteration
 *   Q' = softmax_l(-U + w_g n^g_i sum_j k_g n^g_j Q_j + w_b n^b_i sum_j k_b n^b_j Q_j)
 * (the w_b term only with IISEG_CRF_BILATERAL).  Tensors (device, NCHW, caller-owned):
 *   P (B,C,H,W) probabilities, X (B,3,H,W) image, U / Q0 / Qin / Qout (B,C,H,W), I (B,3,H,W),
 *   ng / nb (B,H,W).  iiseg_crf_prepare writes U, Q0, I, ng, nb; iiseg_crf_step reads U, Qin, I, ng,
 *   nb and writes Qout (Qin != Qout: ping-pong).  Supported: 1 <= B <= 65535, 2 <= C <= 16,
 *   1 <= R <= 16, H, W >= 1 (any size, also smaller than R), positive sxy_g, sxy_b, srgb,
 *   0 < clip <= 1; anything else is IISEG_ERR_SHAPE before any launch.
 * ------------------------------------------------------------------------------------- */
#define IISEG_CRF_BILATERAL 1u     /* add the appearance (bilateral) kernel            */
#define IISEG_CRF_INPUT_0_255 2u   /* X holds 0..255 values (-test_from_0_255)         */

typedef struct iiseg_crf_desc {
    int32_t B, C, H, W, R;
    uint32_t flags;
    double sxy_g, w_g, sxy_b, srgb, w_b, clip;
} iiseg_crf_desc;

/* host only: 1 when the descriptor is in the supported range, else 0 */
int iiseg_crf_supported(const iiseg_crf_desc* d);
int iiseg_crf_prepare_f32(void* stream, const iiseg_crf_desc* d, const float* P, const float* X, float* U,
                          float* Q0, float* I, float* ng, float* nb);
int iiseg_crf_prepare_f64(void* stream, const iiseg_crf_desc* d, const double* P, const double* X,
                          double* U, double* Q0, double* I, double* ng, double* nb);
int iiseg_crf_step_f32(void* stream, const iiseg_crf_desc* d, const float* U, const float* Qin,
                       const float* I, const float* ng, const float* nb, float* Qout);
int iiseg_crf_step_f64(void* stream, const iiseg_crf_desc* d, const double* U, const double* Qin,
                       const double* I, const double* ng, const double* nb, double* Qout);

/* ---------------------------------------------------------------------------------------
 * Training the context-module DAE (reference train_dae.py, dae kind 'contextmod').
 * Every entry checks its arguments and returns a status before any launch; every sum has a fixed order
 * (the same inputs give the same bits on every run).  Tensors: device, NCHW, C-contiguous.
 *
 * Loss (metrics.py:68-91 crossentropy, :144-156 squared_error with an int `void`): score (B,C,H,W) is the
 * 1x1 layer's output, target (B,C+1,H,W) one-hot with the void channel last, 2 <= C <= 16.
 *   iiseg_ctx_loss_count : cnt[4] = {N_ce, N_se, 1/N_ce, 1/N_se} of the BATCH, N_ce = pixels whose arg-max
 *       channel is not the void channel, N_se = sum of target[:, :C]; an empty mask gives the reciprocal 0,
 *       so the loss and its gradient are then 0 (never NaN).
 *   iiseg_ctx_loss : r = softmax(score); res[3] = {loss, crossentropy, squared_error} with
 *       loss = [CROSSENTROPY] ce + [SQUARED_ERROR] lmb se; g (may be NULL) = dloss/dscore, NORMALISED (it
 *       reads cnt from iiseg_ctx_loss_count); where r[label] is outside [1e-7, 1 - 1e-7] the clip is active
 *       and the cross-entropy term's gradient is 0.
 *   partial: 2 * iiseg_ctx_loss_partials(B, H, W) doubles of scratch.
 *
 * Weight gradient of a 'valid' K x K layer (K = 1 or 3, dilation dil, at most 16 channels on either side):
 *   g_z = out ? gout * [out > 0] : gout                      (B,Cout,OH,OW), OH = H - dil (K - 1)
 *   dW[ci][co][ky][kx] = sum_{b,y,x} x[b,ci,y + ky dil,x + kx dil] g_z[b,co,y,x],  db[co] = sum g_z
 * dW is written in the layer's parameter layout: element (co, ci, tap) at co * so + ci * sc + tap with
 * (so, sc) = (Cin K K, K K) for W[out,in,k,k] or (K K, Cout K K) for W[in,out,k,k].  gz (may be NULL)
 * receives g_z inside (gz_H, gz_W) planes at (gz_y0, gz_x0) -- a zero-bordered buffer on which the data
 * gradient runs as a 'valid' layer; the rest of gz is not touched.  slab: scratch of
 * iiseg_conv_small_wgrad_partials(d, sizeof element) * (Cin Cout K K + Cout) elements.
 *
 * Optimizer step on n scalars (Lasagne's rmsprop / adam with their defaults), lr read from device memory:
 *   RMSPROP: s1 <- 0.9 s1 + (1 - 0.9) g^2;  p <- p - lr g / sqrt(s1 + 1e-6)                 (s2, state unused)
 *   ADAM:    state = {t, 0.9^t, 0.999^t} (start {0, 1, 1}; the powers are running products), advanced first;
 *            alpha = lr sqrt(1 - 0.999^t) / (1 - 0.9^t);  s1 <- 0.9 s1 + (1 - 0.9) g;
 *            s2 <- 0.999 s2 + (1 - 0.999) g^2;  p <- p - alpha s1 / (sqrt(s2) + 1e-8)
 * Each operation is rounded on its own in the tensors' type (no FMA contraction).
 * ------------------------------------------------------------------------------------- */
#define IISEG_LOSS_CROSSENTROPY 1u
#define IISEG_LOSS_SQUARED_ERROR 2u
#define IISEG_OPT_RMSPROP 0
#define IISEG_OPT_ADAM 1

typedef struct iiseg_wgrad_desc {
    int32_t B, Cin, Cout, H, W, K, dil;
    int32_t gz_H, gz_W, gz_y0, gz_x0;
    int32_t reserved;
    int64_t so, sc;
} iiseg_wgrad_desc;

/* host only: number of partials, or a negative status */
int iiseg_ctx_loss_partials(int32_t B, int32_t H, int32_t W);
int iiseg_ctx_loss_count_f32(void* stream, const float* target, double* partial, double* cnt, int32_t B,
                             int32_t C, int32_t H, int32_t W);
int iiseg_ctx_loss_count_f64(void* stream, const double* target, double* partial, double* cnt, int32_t B,
                             int32_t C, int32_t H, int32_t W);
int iiseg_ctx_loss_f32(void* stream, const float* score, const float* target, const double* cnt, float* g,
                       double* partial, double* res, int32_t B, int32_t C, int32_t H, int32_t W,
                       uint32_t flags, double lmb);
int iiseg_ctx_loss_f64(void* stream, const double* score, const double* target, const double* cnt, double* g,
                       double* partial, double* res, int32_t B, int32_t C, int32_t H, int32_t W,
                       uint32_t flags, double lmb);
/* host only: number of slabs for elements of elem_bytes (4 or 8), or a negative status */
int iiseg_conv_small_wgrad_partials(const iiseg_wgrad_desc* d, int32_t elem_bytes);
int iiseg_conv_small_wgrad_f32(void* stream, const iiseg_wgrad_desc* d, const float* x, const float* gout,
                               const float* out, float* gz, float* slab, float* dW, float* db);
int iiseg_conv_small_wgrad_f64(void* stream, const iiseg_wgrad_desc* d, const double* x, const double* gout,
                               const double* out, double* gz, double* slab, double* dW, double* db);
int iiseg_opt_step_f32(void* stream, int32_t kind, float* p, const float* g, float* s1, float* s2,
                       const float* lr, float* state, int64_t n);
int iiseg_opt_step_f64(void* stream, int32_t kind, double* p, const double* g, double* s1, double* s2,
                       const double* lr, double* state, int64_t n);

/* ---------------------------------------------------------------------------------------
 * True-gradient refinement through the context-module DAE: the backward pass w.r.t.
 * the y channels.  Every entry checks its arguments and returns a status before any launch; sums have a fixed
 * order (from 0, output-channel-major / tap-minor sequential FMAs); no atomics.  Tensors: device, NCHW.
 *
 * Masked data gradient of a 'valid' K x K layer (K = 1 or 3, dilation dil, at most 16 channels on either
 * side) whose output map is (OH, OW) and whose input map is (OH + dil (K - 1), OW + dil (K - 1)):
 *   g_z = out ? gout * [out > 0] : gout                       (relu'(0) = 0; out == NULL: a linear layer)
 *   g_x[b][ci][y][x] = sum_{co,ky,kx} W[ci][co][ky][kx] g_z[b][co][y - ky dil][x - kx dil]
 * g_z is formed while gout is read (no pass of its own); positions outside gout count as zero.
 *   gout : (B, Cout, OH, OW), contiguous.
 *   out  : the layer's rectified output, its (OH, OW) map at (out_y0, out_x0) of (B, Cout, out_H, out_W).
 *   W    : the layer's parameter in its own layout: element (co, ci, tap) at co * so + ci * sc + tap with
 *          (so, sc) = (Cin K K, K K) for W[out,in,k,k] or (K K, Cout K K) for W[in,out,k,k].
 *   gx   : only the window (wy0, wx0, WH, WW) of g_x and the input channels [ci0, ci0 + nci) are computed;
 *          they go to channels [gx_c0, gx_c0 + nci) of (B, gx_C, gx_H, gx_W) with the window's corner at
 *          (gx_y0, gx_x0).  Nothing else of gx is touched.
 * iiseg_conv_small_dgrad_blocks: the number of workgroups the launch would have (> 0), or the status the
 * launch would return (host only).
 *
 * Head of the chain, one launch from the score map to the masked gradient at dilconv6's output:
 *   r = softmax(score), g_r = 2 (r - y), g_s = r (g_r - <r, g_r>)   (the bits of iiseg_sqerr_softmax_bwd)
 *   g6[ci] = [out6[ci] > 0] sum_co W7[ci][co] g_s[co]               (out6 == NULL: no mask)
 * score, y, gs (may be NULL): (B, C, H, W); out6, g6: (B, Cin, H, W); W7 the 1x1 layer's parameter, (so, sc)
 * = (Cin, 1) or (1, C); 2 <= C <= 16, Cin <= 16.
 * ------------------------------------------------------------------------------------- */
typedef struct iiseg_dgrad_desc {
    int32_t B, Cin, Cout, K, dil;
    int32_t OH, OW;
    int32_t out_H, out_W, out_y0, out_x0;
    int32_t wy0, wx0, WH, WW;
    int32_t ci0, nci;
    int32_t gx_C, gx_H, gx_W, gx_c0, gx_y0, gx_x0;
    int32_t reserved;
    int64_t so, sc;
} iiseg_dgrad_desc;

int iiseg_conv_small_dgrad_blocks(const iiseg_dgrad_desc* d);
int iiseg_conv_small_dgrad_f32(void* stream, const iiseg_dgrad_desc* d, const float* gout, const float* out,
                               const float* W, float* gx);
int iiseg_conv_small_dgrad_f64(void* stream, const iiseg_dgrad_desc* d, const double* gout, const double* out,
                               const double* W, double* gx);
/* host only: number of workgroups, or a negative status */
int iiseg_ctx_grad_head_blocks(int32_t B, int32_t C, int32_t Cin, int32_t H, int32_t W);
int iiseg_ctx_grad_head_f32(void* stream, const float* score, const float* y, const float* out6, const float* W7,
                            int64_t so, int64_t sc, float* gs, float* g6, int32_t B, int32_t C, int32_t Cin,
                            int32_t H, int32_t W);
int iiseg_ctx_grad_head_f64(void* stream, const double* score, const double* y, const double* out6,
                            const double* W7, int64_t so, int64_t sc, double* gs, double* g6, int32_t B, int32_t C,
                            int32_t Cin, int32_t H, int32_t W);

/* ---------------------------------------------------------------------------------------
 * 16-bit leg of the context-module DAE: a 'valid' K x K layer, K = 1 or 3, dilation
 * dil in {1, 2, 4, 8, 16}, at most 16 channels on either side, on bf16 C8 activations with
 * v_mfma_f32_16x16x32_bf16 (bf16 operands, fp32 accumulation; csrc/conv_c8_dil.hip).  The B operand comes
 * straight from global memory (one 16-byte chunk entry per lane and MFMA, no LDS).  Every output is ONE
 * fixed-order sum: the MFMA chain from zero over the tap pairs (0,1) (2,3) (4,5) (6,7) (8,-), then in fp32
 * + bias, + addend, ReLU, store.  No atomics.  Every entry checks its arguments before any launch.
 *   x8     : (B, 2, H, W, 8) bf16, channels >= Cin are zeros by contract.
 *   wpack  : the packed A operand, iiseg_conv_c8_dil_pack_bytes(K) bytes, 16-byte aligned: image m (tap pair m;
 *            K = 1: one image) as [lane group g][row co][j] bf16 = W[co][ci = 8 (g & 1) + j][tap 2 m + (g >> 1)],
 *            rounded to nearest-even; zero where co >= Cout, ci >= Cin or the tap does not exist.
 *   bias   : Cout floats or NULL.   addend : fp32 (B, Cout, OH, OW) or NULL, (OH, OW) = (H, W) - dil (K - 1).
 *   out    : bf16 C8 (B, 2, out_H, out_W, 8) with the (OH, OW) map at (out_y0, out_x0) -- channels >= Cout are
 *            written as zeros, nothing outside the window is touched -- or, with IISEG_C8DIL_OUT_NCHW, fp32
 *            (B, Cout, out_H, out_W).  out_H == 0: a dense (OH, OW) output.
 * W of the packers: element (co, ci, tap) at co * so + ci * sc + tap (see iiseg_dgrad_desc).
 * ------------------------------------------------------------------------------------- */
#define IISEG_C8DIL_OUT_NCHW 0x100u   /* flags, beside IISEG_CONV_RELU */
typedef struct iiseg_c8dil_desc {
    int32_t B, Cin, Cout, H, W, K, dil;
    int32_t out_H, out_W, out_y0, out_x0;
    uint32_t flags;
} iiseg_c8dil_desc;

/* host only: IISEG_OK or the status a launch of `d` would return */
int iiseg_conv_c8_dil_check(const iiseg_c8dil_desc* d);
/* host only: bytes of the packed operand for K (1 or 3), or a negative status */
int64_t iiseg_conv_c8_dil_pack_bytes(int32_t K);
/* host only: packs host weights into host memory (the arithmetic of the device packer; tests, tools) */
int iiseg_conv_c8_dil_pack_host(const iiseg_c8dil_desc* d, const float* W, int64_t so, int64_t sc, void* wpack);
/* device: W and wpack in device memory; one small launch */
int iiseg_conv_c8_dil_pack(void* stream, const iiseg_c8dil_desc* d, const float* W, int64_t so, int64_t sc,
                           void* wpack);
int iiseg_conv_c8_dil(void* stream, const iiseg_c8dil_desc* d, const void* x8, const void* wpack,
                      const float* bias, const float* addend, void* out);

/* ---------------------------------------------------------------------------------------
 * Training the standard pool / unpool DAE (backward-compatible addition).
 *
 * Weight and bias gradient of a zero-padded 3x3 stride-1 layer out = conv(xpad, W) + b, any channel counts up
 * to 65535 (csrc/conv_wgrad.hip; float on v_mfma_f32_32x32x2_f32, double on the vector ALU):
 *   dW[co][ci0 + ci][ky][kx] = sum_{b,y,x} gz[b,co,y,x] xpad[b,ci,y + ky,x + kx],   db[co] = sum_{b,y,x} gz[b,co,y,x]
 *   x  : (B, Cin, H, W), contiguous; the zero padding `pad` >= 0 on every side is implicit.
 *   gz : (B, Cout, OH, OW) = dL/dout with the ReLU mask already applied, OH = H + 2 pad - 2.
 *   dW : the layer's parameter array with Cin_tot >= ci0 + Cin input channels; element (co, ci0 + ci, tap) at
 *        co * so + (ci0 + ci) * sc + tap, (so, sc) = (Cin_tot 9, 9) for W[out,in,3,3] or (9, Cout 9) for
 *        W[in,out,3,3].  Only those Cout * Cin * 9 elements are written: the two sources of a concat layer are
 *        two calls with their channel offsets.
 *   db : Cout elements, or NULL (the second call of a concat layer).
 *   ws : iiseg_conv_wgrad_workspace_elems(d, sizeof element) elements of scratch (0: may be NULL).
 * The pixel range is split into iiseg_conv_wgrad_slabs(d, ...) slabs, one workgroup per slab and 64 x 64 (double:
 * 32 x 32) channel block; with more than one slab a second launch adds the slabs in slab order.  No atomics:
 * the same inputs give the same bits.  Output pixels whose 3x3 patch lies wholly inside the zero padding (wide
 * pads) contribute to db only and are not multiplied.
 *
 * Grid form of iiseg_opt_step_*: the same arithmetic per element (the same bits), many workgroups; adam's state
 * is read by every workgroup and advanced by a one-thread launch AFTER the grid launch.
 * ------------------------------------------------------------------------------------- */
typedef struct iiseg_conv_wgrad_desc {
    int32_t B, Cin, Cout, H, W, K, pad;   /* K must be 3 */
    int32_t ci0, Cin_tot;
    int32_t reserved[3];
    int64_t so, sc;
} iiseg_conv_wgrad_desc;

/* host only: IISEG_OK or the status a launch of `d` would return */
int iiseg_conv_wgrad_check(const iiseg_conv_wgrad_desc* d);
/* host only: number of pixel slabs (>= 1) for elements of elem_bytes (4 or 8), or a negative status */
int iiseg_conv_wgrad_slabs(const iiseg_conv_wgrad_desc* d, int32_t elem_bytes);
/* host only: elements of `ws` (0 with one slab, else slabs * (Cout Cin 9 + Cout)), or a negative status */
int64_t iiseg_conv_wgrad_workspace_elems(const iiseg_conv_wgrad_desc* d, int32_t elem_bytes);
int iiseg_conv_wgrad_f32(void* stream, const iiseg_conv_wgrad_desc* d, const float* x, const float* gz, float* ws,
                         float* dW, float* db);
int iiseg_conv_wgrad_f64(void* stream, const iiseg_conv_wgrad_desc* d, const double* x, const double* gz, double* ws,
                         double* dW, double* db);
int iiseg_opt_step_grid_f32(void* stream, int32_t kind, float* p, const float* g, float* s1, float* s2,
                            const float* lr, float* state, int64_t n);
int iiseg_opt_step_grid_f64(void* stream, int32_t kind, double* p, const double* g, double* s1, double* s2,
                            const double* lr, double* state, int64_t n);

/* ---------------------------------------------------------------------------------------
 * Training FCN-8 (backward-compatible addition).
 *
 * Weight and bias gradient of a 'valid' K x K stride-1 layer, 1 <= K <= 7, any channel counts up to 65535
 * (csrc/conv_wgrad_kxk.hip; float on v_mfma_f32_32x32x2_f32, double on the vector ALU):
 *   dW[co][ci0 + ci][ky][kx] = sum_{b,y,x} gz[b,co,y,x] x[b,ci,y + ky,x + kx],   db[co] = sum_{b,y,x} gz[b,co,y,x]
 *   x  : an (H, W) window of a larger map, read in place: element (b, ci, y, x) at b x_image + ci x_plane +
 *        (x_y0 + y) x_row + x_x0 + x.  x_row >= x_x0 + W, x_plane >= (x_y0 + H) x_row, x_image >= Cin x_plane.
 *   gz : (B, Cout, OH, OW) contiguous = dL/dout with the ReLU mask already applied, OH = H - K + 1.
 *   dW, db, ws, (so, sc), ci0, Cin_tot : as iiseg_conv_wgrad_* with K^2 taps in place of 9; everything of dW
 *        outside input channels [ci0, ci0 + Cin) is left untouched.  db may be NULL.
 * A workgroup owns 64 x 64 (double: 32 x 32) channels, one filter row and one slab of the pixel range; with more
 * than one slab a second launch adds the slabs in slab order.  No atomics: the same inputs give the same bits.
 *
 * Backward of iiseg_deconv_* on the same descriptor (csrc/deconv_grad.hip; AH, AW, ay0, ax0 are ignored): g =
 * dL/d(window) (B, Cout, OH, OW), zero outside the window (the crop's adjoint); any K, stride, channel counts.
 *   dgrad : gx (B, Cin, H, W) = the transposed convolution's adjoint applied to g.
 *   wgrad : dW (Cin, Cout, K, K) and db (Cout, or NULL); ws = iiseg_deconv_wgrad_partials(d) * (Cin Cout K^2 + Cout)
 *           elements, always required; the partials are added in their order in double.
 *
 * relu_gate : dst[i] = out[i] > 0 ? g[i] : 0 (dst may be g, not out).
 * l2_term   : over the `nranges` <= IISEG_L2_MAX_RANGES ascending disjoint index ranges [ranges[2k], ranges[2k+1])
 *             (a HOST array) of the n-element buffers p and g: g += 2 weight_decay p, *penalty = sum p^2 (double,
 *             fixed order); partial = iiseg_l2_term_partials(nranges) doubles of scratch.
 * ------------------------------------------------------------------------------------- */
#define IISEG_L2_MAX_RANGES 64

typedef struct iiseg_conv_wgrad_kxk_desc {
    int32_t B, Cin, Cout, H, W, K;        /* H, W: the window of x; 1 <= K <= 7 */
    int32_t ci0, Cin_tot;
    int32_t x_y0, x_x0;                   /* the window's origin inside the planes of x */
    int32_t reserved[2];
    int64_t x_row, x_plane, x_image;      /* strides of x, in elements */
    int64_t so, sc;
} iiseg_conv_wgrad_kxk_desc;

/* host only: IISEG_OK or the status a launch of `d` would return */
int iiseg_conv_wgrad_kxk_check(const iiseg_conv_wgrad_kxk_desc* d);
/* host only: number of pixel slabs (>= 1) for elements of elem_bytes (4 or 8), or a negative status */
int iiseg_conv_wgrad_kxk_slabs(const iiseg_conv_wgrad_kxk_desc* d, int32_t elem_bytes);
/* host only: elements of `ws` (0 with one slab, else slabs * (Cout Cin K^2 + Cout)), or a negative status */
int64_t iiseg_conv_wgrad_kxk_workspace_elems(const iiseg_conv_wgrad_kxk_desc* d, int32_t elem_bytes);
int iiseg_conv_wgrad_kxk_f32(void* stream, const iiseg_conv_wgrad_kxk_desc* d, const float* x, const float* gz,
                             float* ws, float* dW, float* db);
int iiseg_conv_wgrad_kxk_f64(void* stream, const iiseg_conv_wgrad_kxk_desc* d, const double* x, const double* gz,
                             double* ws, double* dW, double* db);

int iiseg_deconv_dgrad_f32(void* stream, const iiseg_deconv_desc* d, const float* g, const float* w, float* gx);
int iiseg_deconv_dgrad_f64(void* stream, const iiseg_deconv_desc* d, const double* g, const double* w, double* gx);
/* host only: number of partial sums (>= 1), or a negative status */
int iiseg_deconv_wgrad_partials(const iiseg_deconv_desc* d);
int iiseg_deconv_wgrad_f32(void* stream, const iiseg_deconv_desc* d, const float* x, const float* g, float* ws,
                           float* dW, float* db);
int iiseg_deconv_wgrad_f64(void* stream, const iiseg_deconv_desc* d, const double* x, const double* g, double* ws,
                           double* dW, double* db);

/* The same gradients of a K = 3, stride-2 layer with the products on the 16-bit matrix pipe (csrc/deconv_grad_bf16.hip;
 * DESIGN.md section 23), float32 only: x, g and W (the layer's own fp32 parameter) are rounded once to bf16, nearest
 * even, as they are staged; v_mfma_f32_16x16x32_bf16, fp32 accumulation in an order the descriptor fixes, no atomics.
 *   wgrad : dW and db (or NULL; the sum of the unrounded g in this kernel's own order -- not the bits of
 *           iiseg_deconv_wgrad_f32's); ws = iiseg_deconv_wgrad_bf16_workspace_elems(d) floats: 0 with one slab (the
 *           kernel writes dW and db themselves, ws may be NULL), else slabs * (Cin Cout 9 + Cout), added in slab
 *           order by a second launch.
 *   dgrad : gx; the reduction over Cout is not split: its workspace is 0 elements and ws is ignored.
 * NULL d or a required pointer IISEG_ERR_NULL; sizes as iiseg_deconv_wgrad_f32 (H W <= 2^28) IISEG_ERR_SHAPE; K != 3 or
 * stride != 2, or an output overlapping an input, IISEG_ERR_UNSUPPORTED.  All before any launch. */
/* host only: IISEG_OK or the status a launch of `d` would return */
int iiseg_deconv_grad_bf16_check(const iiseg_deconv_desc* d);
/* host only: number of slabs (>= 1), or a negative status */
int iiseg_deconv_wgrad_bf16_slabs(const iiseg_deconv_desc* d);
/* host only: elements of `ws`, or a negative status */
int64_t iiseg_deconv_wgrad_bf16_workspace_elems(const iiseg_deconv_desc* d);
int64_t iiseg_deconv_dgrad_bf16_workspace_elems(const iiseg_deconv_desc* d);
int iiseg_deconv_wgrad_bf16(void* stream, const iiseg_deconv_desc* d, const float* x, const float* g, float* ws,
                            float* dW, float* db);
int iiseg_deconv_dgrad_bf16(void* stream, const iiseg_deconv_desc* d, const float* g, const float* w, float* ws,
                            float* gx);

int iiseg_relu_gate_f32(void* stream, const float* g, const float* out, float* dst, int64_t n);
int iiseg_relu_gate_f64(void* stream, const double* g, const double* out, double* dst, int64_t n);
/* host only: doubles of `partial`, or a negative status */
int iiseg_l2_term_partials(int32_t nranges);
int iiseg_l2_term_f32(void* stream, const float* p, float* g, int64_t n, const int64_t* ranges, int32_t nranges,
                      double weight_decay, double* partial, double* penalty);
int iiseg_l2_term_f64(void* stream, const double* p, double* g, int64_t n, const int64_t* ranges, int32_t nranges,
                      double weight_decay, double* partial, double* penalty);

/* ---------------------------------------------------------------------------------------
 * Weight gradients on the 16-bit matrix pipe (wgrad='bf16'; backward-compatible addition).
 *
 * iiseg_conv_wgrad_f32's sums for the same descriptor and the same fp32 tensors (csrc/conv_wgrad_bf16.hip), with
 * every x and gz element rounded once to bf16 (to nearest, ties to even) as it is staged and the products formed
 * by v_mfma_f32_32x32x16_bf16 with fp32 accumulators:
 *   dW[co][ci0 + ci][ky][kx] = sum_{b,y,x} bf16(gz[b,co,y,x]) bf16(xpad[b,ci,y + ky,x + kx])
 *   db[co]                   = sum_{b,y,x} gz[b,co,y,x]                        (the unrounded values)
 * The same contract otherwise: slabs of its own plan (iiseg_conv_wgrad_bf16_slabs), a finalize launch that adds
 * them in slab order in double, no atomics, the same inputs give the same bits.
 *   ws : iiseg_conv_wgrad_bf16_workspace_elems(d) floats of scratch (0: may be NULL).
 * ------------------------------------------------------------------------------------- */
/* host only: number of pixel slabs (>= 1), or a negative status */
int iiseg_conv_wgrad_bf16_slabs(const iiseg_conv_wgrad_desc* d);
/* host only: floats of `ws` (0 with one slab, else slabs * (Cout Cin 9 + Cout)), or a negative status */
int64_t iiseg_conv_wgrad_bf16_workspace_elems(const iiseg_conv_wgrad_desc* d);
int iiseg_conv_wgrad_bf16(void* stream, const iiseg_conv_wgrad_desc* d, const float* x, const float* gz, float* ws,
                          float* dW, float* db);
/* The same sums, contract, status codes and NULL rules in the form for few output channels
 * (csrc/conv_wgrad_bf16.hip's co16 form; backward-compatible addition): blocks of 16 output x 64
 * input channels on v_mfma_f32_16x16x32_bf16, any Cout (a ragged last block), slabs and workspace of its own plan.
 * The order of the fp32 additions differs from iiseg_conv_wgrad_bf16's, so the bits may; each is deterministic. */
int iiseg_conv_wgrad_bf16_co16_slabs(const iiseg_conv_wgrad_desc* d);
int64_t iiseg_conv_wgrad_bf16_co16_workspace_elems(const iiseg_conv_wgrad_desc* d);
int iiseg_conv_wgrad_bf16_co16(void* stream, const iiseg_conv_wgrad_desc* d, const float* x, const float* gz,
                               float* ws, float* dW, float* db);
/* db alone, with the bits iiseg_conv_wgrad_f32 gives it for the same descriptor (csrc/conv_wgrad.hip: that kernel's
 * plan, chains and slab order without x and the products; backward-compatible addition): for a caller that forms dW
 * on the 16-bit pipe (db = NULL there) and leaves every db as the fp32 mode has it.
 *   ws : iiseg_conv_wgrad_db_workspace_elems(d) floats of scratch (0 with one slab: may be NULL; else slabs * Cout). */
int64_t iiseg_conv_wgrad_db_workspace_elems(const iiseg_conv_wgrad_desc* d);
int iiseg_conv_wgrad_db_f32(void* stream, const iiseg_conv_wgrad_desc* d, const float* gz, float* ws, float* db);

/* ---------------------------------------------------------------------------------------
 * Data gradients on the 16-bit matrix pipe (dgrad='bf16'; backward-compatible addition).
 *
 * Data gradient of a zero-padded 3x3 stride-1 layer with pad 1 (csrc/conv_dgrad_bf16.hip), from fp32 tensors:
 *   gx[b][ci][y][x] = sum_{co,ky,kx} bf16(W[co][ci0 + ci][ky][kx]) bf16(gz[b][co][y + 1 - ky][x + 1 - kx])
 * with gz zero outside its plane, every operand rounded once (to nearest, ties to even), the products formed by
 * v_mfma_f32_32x32x16_bf16 and accumulated in fp32 in a fixed order: no atomics, the same inputs give the same bits.
 *   gz     : (B, Cout, H, W), contiguous: dL/dout with the ReLU mask already applied.
 *   W      : the layer's fp32 parameter array with Cin_tot >= ci0 + Cin input channels; element (co, ci0 + ci, tap)
 *            at co * so + (ci0 + ci) * sc + tap, (so, sc) = (Cin_tot 9, 9) for W[out,in,3,3] or (9, Cout 9) for
 *            W[in,out,3,3].  Read by iiseg_conv_dgrad_bf16_pack only.
 *   packed : iiseg_conv_dgrad_bf16_pack_elems(d) bf16 elements, 16-byte aligned: the image of the Cin channels that
 *            iiseg_conv_dgrad_bf16_pack writes ([k-tile][tap][co chunk of 8][ci][8 co], zero past Cout and Cin)
 *            and iiseg_conv_dgrad_bf16 reads.  Pack again whenever W has changed.
 *   gx     : (B, Cin, H, W), contiguous.  accumulate = 1: gx += the sums, in place.
 *   gate   : NULL, or a map of gx's shape: the result (after the accumulation) is gx * [gate > 0], relu'(0) = 0.
 * NULL d, gz, W, packed or gx IISEG_ERR_NULL; K != 3, pad != 1, non-positive sizes, more than 65535 channels or
 * images, H W > 2^28, ci0 + Cin > Cin_tot, other strides, accumulate outside {0, 1} IISEG_ERR_SHAPE; packed not
 * 16-byte aligned IISEG_ERR_ALIGN; gx overlapping gz or packed, packed overlapping W IISEG_ERR_UNSUPPORTED.  All
 * before any launch.
 * ------------------------------------------------------------------------------------- */
typedef struct iiseg_conv_dgrad_desc {
    int32_t B, Cin, Cout, H, W, K, pad;   /* K must be 3, pad 1 */
    int32_t ci0, Cin_tot;
    int32_t accumulate;
    int32_t reserved[2];
    int64_t so, sc;
} iiseg_conv_dgrad_desc;

/* host only: IISEG_OK or the status a launch of `d` would return */
int iiseg_conv_dgrad_bf16_check(const iiseg_conv_dgrad_desc* d);
/* host only: bf16 elements of `packed`, or a negative status */
int64_t iiseg_conv_dgrad_bf16_pack_elems(const iiseg_conv_dgrad_desc* d);
int iiseg_conv_dgrad_bf16_pack(void* stream, const iiseg_conv_dgrad_desc* d, const float* W, void* packed);
int iiseg_conv_dgrad_bf16(void* stream, const iiseg_conv_dgrad_desc* d, const float* gz, const void* packed,
                          const float* gate, float* gx);

/* ---------------------------------------------------------------------------------------
 * 'valid' K x K layers on the 16-bit matrix pipe (kxk='bf16'; csrc/conv_kxk_bf16.hip; DESIGN.md section 17;
 * backward-compatible addition).  1 <= K <= 7, stride 1, fp32 tensors; every operand is rounded once (to nearest,
 * ties to even) as it is staged, v_mfma_f32_32x32x16_bf16 accumulates in fp32 in a fixed order, the slabs of a split
 * reduction are added in slab order: no atomics, the same inputs give the same bits.
 *
 * Weight gradient, on iiseg_conv_wgrad_kxk_desc with the operands of iiseg_conv_wgrad_kxk_f32:
 *   dW[co][ci0 + ci][ky][kx] = sum_{b,y,x} bf16(gz[b,co,y,x]) bf16(x[b,ci,y + ky,x + kx]),   db = the fp32 sum of the
 *   unrounded gz.  ws: iiseg_conv_wgrad_kxk_bf16_workspace_elems(d) floats (0 with one slab).
 *
 * Data gradient, on iiseg_conv_dgrad_desc with (H, W) the planes of gz and `pad` ignored:
 *   gx[b][ci][y][x] = sum_{co,ky,kx} bf16(W[co][ci0 + ci][ky][kx]) bf16(gz[b][co][y - ky][x - kx])
 *   gz     : (B, Cout, H, W) contiguous, zero outside its plane (no embedded copy is made).
 *   gx     : (B, Cin, H + K - 1, W + K - 1) contiguous; accumulate, gate as iiseg_conv_dgrad_bf16.
 *   packed : iiseg_conv_dgrad_kxk_bf16_pack_elems(d) bf16 elements, 16-byte aligned, written by
 *            iiseg_conv_dgrad_kxk_bf16_pack from the layer's own parameter ([k-tile of 16 co][tap][co chunk of 8][ci,
 *            padded to 64][8 co], zero past Cout and Cin).  Pack again whenever W has changed.
 *   ws     : iiseg_conv_dgrad_kxk_bf16_workspace_elems(d) floats (0 with one slab of output channels).
 * Statuses as the fp32 / 3x3 siblings: NULL pointers IISEG_ERR_NULL, shapes and strides IISEG_ERR_SHAPE, alignment
 * IISEG_ERR_ALIGN, gx overlapping gz or packed, packed overlapping W IISEG_ERR_UNSUPPORTED; all before any launch.
 * ------------------------------------------------------------------------------------- */
int iiseg_conv_wgrad_kxk_bf16_check(const iiseg_conv_wgrad_kxk_desc* d);
int iiseg_conv_wgrad_kxk_bf16_slabs(const iiseg_conv_wgrad_kxk_desc* d);
int64_t iiseg_conv_wgrad_kxk_bf16_workspace_elems(const iiseg_conv_wgrad_kxk_desc* d);
int iiseg_conv_wgrad_kxk_bf16(void* stream, const iiseg_conv_wgrad_kxk_desc* d, const float* x, const float* gz,
                              float* ws, float* dW, float* db);
int iiseg_conv_dgrad_kxk_bf16_check(const iiseg_conv_dgrad_desc* d);
int iiseg_conv_dgrad_kxk_bf16_slabs(const iiseg_conv_dgrad_desc* d);
int64_t iiseg_conv_dgrad_kxk_bf16_workspace_elems(const iiseg_conv_dgrad_desc* d);
int64_t iiseg_conv_dgrad_kxk_bf16_pack_elems(const iiseg_conv_dgrad_desc* d);
int iiseg_conv_dgrad_kxk_bf16_pack(void* stream, const iiseg_conv_dgrad_desc* d, const float* W, void* packed);
int iiseg_conv_dgrad_kxk_bf16(void* stream, const iiseg_conv_dgrad_desc* d, const float* gz, const void* packed,
                              const float* gate, float* ws, float* gx);

/* ---------------------------------------------------------------------------------------
 * Forward of a 'valid' K x K stride-1 layer on the 16-bit matrix pipe (fwd='bf16'; csrc/conv_kxk_bf16.hip; DESIGN.md
 * section 18; backward-compatible addition).  1 <= K <= 7, fp32 tensors:
 *   z[b][co][y][x] = relu(sum_{ci,ky,kx} bf16(W[co][ci][ky][kx]) bf16(x[b][ci][y + ky][x + kx]) + bias[co])
 * every operand rounded once (to nearest, ties to even) as it is staged, v_mfma_f32_32x32x16_bf16 accumulating in
 * fp32 in a fixed order, the slabs of a split reduction added in slab order, the bias added in fp32: no atomics, the
 * same inputs give the same bits.  No im2col image and no packed copy of W: the parameter is read as it is.
 *   x    : (B, Cin, H, W) contiguous.      W : (Cout, Cin, K, K) contiguous ('oihw'), the layer's own parameter.
 *   bias : Cout floats, or NULL.           z : (B, Cout, H - K + 1, W - K + 1) contiguous.    relu: 0 or 1.
 *   ws   : iiseg_conv_fwd_kxk_bf16_workspace_elems(d) floats (0 with one slab of the reduction).
 * NULL d, x, W, z (ws with several slabs) IISEG_ERR_NULL; K outside 1..7, H or W below K, non-positive sizes, more
 * than 65535 channels or images, H W > 2^28, relu outside {0, 1} IISEG_ERR_SHAPE; alignment IISEG_ERR_ALIGN; z
 * overlapping x or W IISEG_ERR_UNSUPPORTED.  All before any launch.
 * ------------------------------------------------------------------------------------- */
typedef struct iiseg_conv_fwd_kxk_desc {
    int32_t B, Cin, Cout, H, W, K;
    int32_t relu;
    int32_t reserved;
} iiseg_conv_fwd_kxk_desc;

int iiseg_conv_fwd_kxk_bf16_check(const iiseg_conv_fwd_kxk_desc* d);
int iiseg_conv_fwd_kxk_bf16_slabs(const iiseg_conv_fwd_kxk_desc* d);
int64_t iiseg_conv_fwd_kxk_bf16_workspace_elems(const iiseg_conv_fwd_kxk_desc* d);
int iiseg_conv_fwd_kxk_bf16(void* stream, const iiseg_conv_fwd_kxk_desc* d, const float* x, const float* W,
                            const float* bias, float* ws, float* z);

/* ---------------------------------------------------------------------------------------
 * Training forward of FC-DenseNet's dense-block layer -- BatchNorm with batch statistics, ReLU, zero-padded 3 x 3
 * convolution, bias, dropout mask -- as one launch on the 16-bit matrix pipe (fwd='bf16' on FC-DenseNet;
 * csrc/bnrelu_conv_bf16.hip; backward-compatible addition).  fp32 tensors:
 *   y = (x[b][c][i][j] - mean[c]) * (gamma[c] * inv_std[c]) + beta[c]       (iiseg_bn_relu_f32's expression)
 *   t = max(y, 0) inside the map, exactly 0 on the padding ring
 *   z[b][co][i][j] = (sum_{c<n,ky,kx} bf16(W[co][c][ky][kx]) bf16(tpad[b][c][i + ky][j + kx]) + bias[co])
 *                    * keep[b][co][i][j] * (1 / (1 - p))                    (iiseg_dropout_apply_f32's expression;
 *                                                                            keep NULL: no factor)
 * every operand rounded once (to nearest, ties to even) as it is staged, v_mfma_f32_16x16x32_bf16 accumulating in
 * fp32 in a fixed order, the slabs of a split reduction over input channels added in slab order before bias, mask
 * and scale: no atomics, the same inputs give the same bits, and an element's bits do not depend on B (the slab rule
 * reads n, Cout, H and W only).  No packed copy of W: the parameter is read as it is.
 *   x    : (B, cap, H, W) contiguous, channels [0, n) read.     beta, gamma, mean, inv_std : n floats at least.
 *   W    : (Cout, n, 3, 3) contiguous ('oihw').    bias : Cout floats.    keep : (B, Cout, H, W) contiguous or NULL.
 *   z    : (B, out_cap, H, W) contiguous; channels [out_c0, out_c0 + Cout) are written, nothing else.  z may be x
 *          itself (cap == out_cap) with out_c0 >= n.
 *   ws   : iiseg_bnrelu_conv_fwd_bf16_workspace_elems(d) floats (0 with one slab).
 * NULL d, x, a BatchNorm vector, W, bias, z (ws with several slabs) IISEG_ERR_NULL; non-positive sizes, cap < n,
 * out_c0 < 0 or out_c0 + Cout > out_cap, more than 65535 channels or images, H W > 2^28, Cout n 9 >= 2^31, p outside
 * [0, 1) IISEG_ERR_SHAPE; z overlapping what is read of x (other than as above), W, keep or ws
 * IISEG_ERR_UNSUPPORTED.  All before any launch.
 * ------------------------------------------------------------------------------------- */
typedef struct iiseg_bnrelu_conv_desc {
    int32_t B, n, cap, Cout, H, W;
    int32_t out_cap, out_c0;
} iiseg_bnrelu_conv_desc;

/* host only: IISEG_OK or the status a launch of `d` would return */
int iiseg_bnrelu_conv_fwd_bf16_check(const iiseg_bnrelu_conv_desc* d);
int iiseg_bnrelu_conv_fwd_bf16_slabs(const iiseg_bnrelu_conv_desc* d);
int64_t iiseg_bnrelu_conv_fwd_bf16_workspace_elems(const iiseg_bnrelu_conv_desc* d);
int iiseg_bnrelu_conv_fwd_bf16(void* stream, const iiseg_bnrelu_conv_desc* d, const float* x, const float* beta,
                               const float* gamma, const float* mean, const float* inv_std, const float* W,
                               const float* bias, const float* keep, float p, float* ws, float* z);

#ifdef __cplusplus
}
#endif
#endif /* IISEG_H */
