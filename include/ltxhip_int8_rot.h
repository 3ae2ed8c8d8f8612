/* ltxhip_int8_rot.h — opt-in Hadamard rotation for the INT8 (W8A8) linear layers of ltxhip_int8.h.  One scale per activation row gives
 * a row with a few large channels almost no resolution in its other channels; rotating the row (and the weight's rows along K) by a
 * Hadamard matrix spreads every channel over all of them before the quantiser sees it.  Handle state like the int8 masks: with the
 * rotation mask 0 no launch and no bit of any other path changes.
 *
 * The definition.  For a row x[0 .. D), D a power of two, H x is the UNNORMALISED Walsh-Hadamard transform in natural (Sylvester)
 * order, computed in f32 as log2 D butterfly stages over the bits of the element index in ASCENDING order, h = 1, 2, 4, .. D / 2.  In
 * stage h, for every index e with bit h clear, both results come from the stage's input values:
 *   x[e]     <- x[e] + x[e + h]
 *   x[e + h] <- x[e] - x[e + h]
 * Every output of a stage is one rounded f32 add or subtract: the stage order alone fixes the bits, the order of work inside a stage
 * does not.  There is no multiply and no irrational factor; H H = D I.  Activations are rotated unnormalised (their per-row scale
 * absorbs the magnitude); weights are rotated the same way along K and their stored scale is multiplied by 1 / K, a power of two, so
 * that product is exact:
 *   x W^T == (H x) (H w)^T / K        in real arithmetic.
 * Quantisation of the rotated f32 row is exactly ltxhip_int8.h's (amax, inv = 127 / amax, q = clamp(rintf(v * inv), -127, 127)) with
 *   scale = (amax / 127.0f) * out_scale                     out_scale: 1 for activations, 1 / K for weights
 * and there is no bf16 rounding between rotation and quantisation.  The norm + quantise pass computes ltxhip_int8.h's f32 n (the same
 * statistics, the same expression), rotates it in registers and quantises H n.  The product itself is ltx_op_gemm_i8, untouched.
 *
 * In the DiT a layer rotates iff its bit is set in BOTH the int8 mask of its block and the rotation mask.  A rotating layer's int8
 * weight copy is made from the weight the forward would otherwise read with out_scale = 1 / in; the copies stay a weight-derived cache
 * (ltx_dit_set_adapters afterwards is followed), and changing the rotation mask re-makes the copies of the kinds that changed.
 *
 * Out of scope: a normalised or randomised (sign-flipped) rotation, widths that are not powers of two (block-diagonal rotations),
 * rotating attn2 or the projections, folding H into stored checkpoints.
 * Conventions are those of ltxhip.h (device pointers unless marked HOST, 0 = success, ltx_last_error). */
#ifndef LTXHIP_INT8_ROT_H
#define LTXHIP_INT8_ROT_H
#include "ltxhip_int8.h"
#ifdef __cplusplus
extern "C" {
#endif

/* mask: LTX_I8_* bits, independent of ltx_dit_set_int8_linears (either may be set first).  Refusals, each leaving the handle unchanged:
 * bits outside LTX_I8_ALL: LTX_ERR_ARG; with a non-zero mask an f32 handle, or an inner dimension D for which D or 4 D is not a power
 * of two in 128 .. 16384: LTX_ERR_UNSUPPORTED.  Re-makes the affected int8 copies on `stream`. */
int ltx_dit_set_int8_rotation(ltx_dit* dit, unsigned char mask, ltx_stream stream);
/* mask_out HOST */
int ltx_dit_get_int8_rotation(const ltx_dit* dit, unsigned char* mask_out);

/* ---- the two kernels on their own (tests, tools) ----
 * x [rows, D] bf16 with row stride ld elements -> q int8 [rows, D] (dense) of H x and scale f32 [rows] = (amax / 127) * out_scale.
 * D a power of two, 128 .. 16384 (else LTX_ERR_UNSUPPORTED); out_scale positive and finite, ld % 8 == 0, x and q 16-byte aligned (else
 * LTX_ERR_ARG). */
int ltx_op_hadamard_quant_rows_i8(const void* x, int64_t rows, int D, int ld, float out_scale, void* q, float* scale, ltx_stream stream);
/* ltx_op_rownorm_quant_i8's arguments and norm; q and row_scale are those of H n.  D a power of two, 128 .. 4096. */
int ltx_op_rownorm_hadamard_quant_i8(const void* h, int64_t rows, int D, int ld, float eps, const float* shift, const float* scale, int mod_stride,
                                     int64_t rows_per_batch, void* q, float* row_scale, ltx_stream stream);

#ifdef __cplusplus
}
#endif
#endif
