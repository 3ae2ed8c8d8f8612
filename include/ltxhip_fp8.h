/* ltxhip_fp8.h — FP8 (E4M3) checkpoints: fp8-resident block linears in the DiT and the GEMM that reads them.
 *
 * The publisher's `-fp8.safetensors` checkpoints store the block linear weights as F8_E4M3, one byte each, with no scales.  The
 * format is the OCP e4m3fn of gfx950: 1 sign, 4 exponent (bias 7), 3 mantissa bits; largest value 448, no infinity, NaN at 0x7F and
 * 0xFF, subnormals down to 2^-9.  Every e4m3 value is exactly a bf16 value, so nothing here is approximate on the weight side:
 * the arithmetic is that of a bf16 forward whose weights happen to be e4m3-representable.
 *
 * The dtype.  LTX_F8_E4M3 (ltxhip.h) describes ltx_weight::data only.  As a model dtype or an input / output dtype it is refused
 * with LTX_ERR_ARG.  A tensor that is not kept in fp8 (below) is widened on the device to the model dtype, exactly: every
 * constructor that takes ltx_weight accepts fp8 sources, f32 handles included.  The safetensors readers map "F8_E4M3" to it.
 *
 * Residency.  In a bf16 DiT handle four kinds of block linear are stored AS FOUND when their source is fp8, and no bf16 copy of
 * them is ever made: attn1's fused q | k | v (only if all three sources are fp8, else all three are widened), attn1.to_out,
 * ff.net.0.proj and ff.net.2 - half the bytes in HBM, half the upload.  Residency is per block and per kind and is fixed at
 * creation; a mixed file is legal.  Biases, norms, attn2, proj_in / proj_out and every other tensor are widened.
 *
 * The layer.  For a [M, K] bf16, w [N, K] e4m3, sw [N] f32 or absent (= 1), bias [N] bf16 or absent:
 *   acc[m][n] = sum_k f32(a[m][k]) * f32(w[n][k])        f32 accumulation on v_mfma_f32_16x16x32_bf16, w widened in registers
 *   out       = epi(acc * sw[n] + bias[n])                the multiply and the add in f32 (they may contract into one fma); the
 *               epilogue expressions of ltx_op_linear (ltxhip_ops.h), rounded once to bf16: epi 0 bias (optionally the segmented
 *               q | k | v output), 1 GELU-tanh, 2 resid + gate * v (one fma), 3 v + resid
 * K % 16 == 0 and N % 4 == 0.  The checkpoints carry no scales and the loader sets none: sw exists for callers of the op.
 *
 * The forward.  A handle with an fp8-resident layer runs its copy of the forward plan without the norm fold, the row-partial
 * norms and the deferred ff2 (those launches pair bf16 producers and weight-scaling passes with bf16 weights), as a handle with
 * int8 layers does; ltx_op_dit_plan is unchanged.  A block's fp8 layer is its pass-form call with W = the fp8 matrix.  A handle with
 * no fp8 source changes no launch and no bit.  STG modes, per-frame timesteps, keyframes, the step cache and every
 * ltx_pipeline_call* run on whatever the handle holds.
 *
 * Refusals, naming block and kind, the handle unchanged: ltx_dit_set_adapters with an adapter that targets an fp8-resident layer
 * (the merge kernel reads a bf16 base) and ltx_dit_set_int8_linears with a bit on one (its quantise pass reads bf16 rows):
 * LTX_ERR_UNSUPPORTED.  Layers that are not fp8-resident keep both features.  ltx_dit_read_linear on an fp8-resident layer hands
 * out the widened bf16 matrix.
 *
 * The cast (for callers who make an fp8 checkpoint from a bf16 one): q = e4m3(x), round to nearest even, SATURATING: |x| >= 448,
 * infinities included, gives +-448 (0x7E / 0xFE); NaN gives 0x7F | sign; below 2^-6 the result is a multiple of 2^-9; zeros keep
 * their sign.  (A cast that turns values beyond 464 into NaN, as some frameworks' does, is a different function.)
 *
 * Cost: the four kinds take half the device memory; every one of them is slower than its bf16 layer today
 * (x1.4 .. 2.2 per layer, x1.30 on a 28-layer forward at 4992 tokens).
 *
 * Out of scope: attn2, proj_in / proj_out and the text k / v in fp8; adapters and int8 on fp8-resident layers; fp8 activations
 * on the fp8 MFMA; a ring form for small M (any M >= 1 is served, on the smallest tile); measured plans (the tile is a shape
 * rule); scale tensors read from checkpoints.
 * Conventions are those of ltxhip.h (device pointers unless marked HOST, 0 = success, ltx_last_error). */
#ifndef LTXHIP_FP8_H
#define LTXHIP_FP8_H
#include "ltxhip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* mask bits of ltx_dit_get_fp8_linears: the order of LTX_I8_* (ltxhip_int8.h) */
enum { LTX_F8_QKV = 1, LTX_F8_TO_OUT = 2, LTX_F8_FF1 = 4, LTX_F8_FF2 = 8, LTX_F8_ALL = 15 };

/* block_masks_out HOST [num_layers]: which kinds of every block are fp8-resident */
int ltx_dit_get_fp8_linears(const ltx_dit* dit, unsigned char* block_masks_out);

/* ---- the kernels on their own (tests, tools) ----
 * x [rows, D] bf16 with row stride ld elements -> q e4m3 [rows, D] (dense): one pass, every load of a thread before its store.
 * D % 16 == 0, ld % 8 == 0, x and q 16-byte aligned, else LTX_ERR_ARG. */
int ltx_op_cast_fp8(const void* x, int64_t rows, int D, int ld, void* q, ltx_stream stream);
/* q e4m3 [n] -> y [n] of dst_dtype (LTX_F32 or LTX_BF16), exact */
int ltx_op_widen_fp8(const void* q, int64_t n, ltx_dtype dst_dtype, void* y, ltx_stream stream);
/* y [M, N] bf16 = epi(acc * w_scale[n] + bias[n]); a bf16 [M, K], w e4m3 [N, K], w_scale f32 [N] or NULL, bias bf16 [N] or NULL,
 * resid bf16 [M, N] (epi 2, 3), gate f32 [ceil(M / rows_per_batch), N] (epi 2).  seg_width (epi 0 only; 0: none): a power of two
 * dividing N, y is then N / seg_width dense [M, seg_width] matrices one after another.  tile: -1 the shape rule (the largest tile
 * whose grid still gives every CU a block), 0 256x256, 1 256x128, 2 128x128.  Refusals: null tensor, misaligned pointer (a, w,
 * w_scale, gate 16 bytes; y, resid, bias 8): LTX_ERR_ARG; K % 16 != 0, N % 4 != 0, an operand of 2 GiB or more:
 * LTX_ERR_UNSUPPORTED.  ltx_op_gemm_route with LTX_ROUTE_W_FP8 names the tile the rule picks ("w8:128x128", ...). */
int ltx_op_gemm_w8(const void* a, const void* w, const float* w_scale, const void* bias, void* y, int M, int N, int K, int epi,
                   const void* resid, const float* gate, int rows_per_batch, int seg_width, int tile, ltx_stream stream);

#ifdef __cplusplus
}
#endif
#endif
