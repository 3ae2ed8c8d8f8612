/* ltxhip_int8.h — opt-in INT8 (W8A8) linear layers for the DiT on the int8 MFMA of gfx950 (v_mfma_i32_16x16x64_i8).  Handle state,
 * like the adapters, the STG mode and the step cache: with the mode off no launch, plan or bit of any other entry point changes.
 *
 * The definition.  Quantisation is symmetric int8, one scale per row, computed in f32 with IEEE (correctly rounded) division and no
 * contraction.  For a row x[0 .. D):
 *   amax  = max_k |x[k]|
 *   inv   = amax > 0 ? 127.0f / amax : 0
 *   q[k]  = clamp(rintf(x[k] * inv), -127, 127)          round half to even; -128 is never produced
 *   scale = amax / 127.0f                                 a zero row: q = 0, scale = 0
 * Weights W [N, K] get one scale per output channel, sw[n] (a weight's rows are its output channels); activations x [M, K] one per
 * row, sa[m], computed at run time.  Inputs are finite.  A quantised layer is
 *   acc[m][n] = sum_k qa[m][k] * qw[n][k]                 int32, exact: K <= 131072 keeps |acc| <= 127 * 127 * K below 2^31
 *   v         = (float(acc) * sa[m]) * sw[n]              int32 -> f32 rounds to nearest even; the two f32 products in THIS order
 *   out       = epi(v + bias[n])                          the epilogue expressions of ltx_op_linear (ltxhip_ops.h), rounded once to bf16:
 *               epi 0 bias (optionally the segmented q | k | v output), 1 GELU-tanh, 2 resid + gate * v (one fma), 3 v + resid
 * K % 16 == 0 and N % 4 == 0.  The model dtype is bf16 throughout.
 *
 * The norm + quantise pass computes the block's modulated RMS norm in f32,
 *   n[k] = h[k] * r * (1 + scale[g][k]) + shift[g][k],   r = 1 / sqrt(mean(h^2) + eps),   g = row / rows_per_batch,
 * and quantises the f32 n as above: no bf16 rounding in between.
 *
 * In the DiT the mask selects which block linears run in int8: attn1's fused q | k | v, attn1.to_out, ff.net.0.proj (ff1) and ff.net.2
 * (ff2).  The int8 weight copies are made on the device from the weights the forward would otherwise read (the bf16 base, or the
 * LoRA-merged copy) and are a weight-derived cache: ltx_dit_set_adapters after ltx_dit_set_int8_linears is correct, the copies are
 * re-made at the next forward.  Activations of q | k | v and ff1 are quantised straight from the f32 norm; those of to_out and ff2
 * from the bf16 tensors the engine stores (the attention output, the GELU output).  A forward of a handle with int8 layers runs
 * without the norm fold, the row-partial norm and the deferred ff2 (their launches belong to the bf16 path); everything else -
 * skip-layer blend, the STG modes, per-frame timesteps, the step cache, keyframes, every ltx_pipeline_call* - runs on whatever the
 * handle has set.
 *
 * Out of scope: attn2 (to_q, to_out, the text k / v), proj_in / proj_out, the VAE and T5; the row maximum of ff2's input as a
 * by-product of ff1's epilogue; static activation scales; outlier rotation; loading pre-quantised checkpoints; measured plans for
 * gemm_i8 (its tile is a shape rule) and split K.
 * Conventions are those of ltxhip.h (device pointers unless marked HOST, 0 = success, ltx_last_error). */
#ifndef LTXHIP_INT8_H
#define LTXHIP_INT8_H
#include "ltxhip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* mask bits of ltx_dit_set_int8_linears */
enum { LTX_I8_QKV = 1, LTX_I8_TO_OUT = 2, LTX_I8_FF1 = 4, LTX_I8_FF2 = 8, LTX_I8_ALL = 15 };

/* block_masks HOST [num_layers] or NULL: NULL gives every block `mask`; with a list block l takes block_masks[l] & mask (a caller
 * keeps the first and last blocks in bf16 with zeros there).  Bits outside LTX_I8_ALL: LTX_ERR_ARG.  An f32 handle: LTX_ERR_UNSUPPORTED.  Quantises the selected weights on `stream` into int8
 * copies + per-channel scales (2B model, all four kinds: about 1.3 GB); a block or kind that loses its bit frees its copy; all zero
 * frees everything and the forward is again that of a handle that was never touched. */
int ltx_dit_set_int8_linears(ltx_dit* dit, const unsigned char* block_masks, unsigned char mask, ltx_stream stream);
/* block_masks_out HOST [num_layers] */
int ltx_dit_get_int8_linears(const ltx_dit* dit, unsigned char* block_masks_out);

/* ---- the three kernels on their own (tests, tools) ----
 * x [rows, D] bf16 with row stride ld elements -> q int8 [rows, D] (dense) and scale f32 [rows].  D % 16 == 0, D <= 16384, ld % 8 == 0,
 * x and q 16-byte aligned: else LTX_ERR_ARG (null / alignment) or LTX_ERR_UNSUPPORTED (D). */
int ltx_op_quant_rows_i8(const void* x, int64_t rows, int D, int ld, void* q, float* scale, ltx_stream stream);
/* h [rows, D] bf16 (row stride ld) -> q int8 [rows, D], row_scale f32 [rows] of the modulated RMS norm above.  shift / scale: f32 tables
 * of row stride mod_stride (>= D, % 4 == 0), 16-byte aligned, indexed by row / rows_per_batch.  D % 16 == 0, D <= 4096. */
int ltx_op_rownorm_quant_i8(const void* h, int64_t rows, int D, int ld, float eps, const float* shift, const float* scale, int mod_stride,
                            int64_t rows_per_batch, void* q, float* row_scale, ltx_stream stream);
/* y [M, N] bf16 = epi((float(acc) * a_scale[m]) * w_scale[n] + bias[n]); a_q int8 [M, K], w_q int8 [N, K], bias bf16 [N] or NULL,
 * resid bf16 [M, N] (epi 2, 3), gate f32 [ceil(M / rows_per_batch), N] (epi 2).  seg_width (epi 0 only; 0: none): a power of two
 * dividing N, y is then N / seg_width dense [M, seg_width] matrices one after another.  tile: -1 the shape rule, 0 256x256,
 * 1 256x128, 2 128x128.  Refusals: null tensor or scale, misaligned pointer (a_q, w_q, w_scale, gate 16 bytes; y, resid, bias 8):
 * LTX_ERR_ARG; K % 16 != 0, K > 131072, N % 4 != 0, an operand of 2 GiB or more: LTX_ERR_UNSUPPORTED. */
int ltx_op_gemm_i8(const void* a_q, const float* a_scale, const void* w_q, const float* w_scale, const void* bias, void* y,
                   int M, int N, int K, int epi, const void* resid, const float* gate, int rows_per_batch, int seg_width, int tile,
                   ltx_stream stream);
/* acc int32 [M, N] = a_q w_q^T, unscaled: the test of the operand map */
int ltx_op_gemm_i8_raw(const void* a_q, const void* w_q, int* acc, int M, int N, int K, int tile, ltx_stream stream);

#ifdef __cplusplus
}
#endif
#endif
