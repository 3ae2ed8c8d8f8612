/* ltxhip_stg.h — where spatio-temporal guidance (STG) perturbs the guidance branch: the whole transformer block (the reference's
 * only form, ltx_transformer.rs:1098-1123, and the default here) or the self-attention inside it (the published recipes of the
 * 0.9.7 / 0.9.8 models: `stg_mode: attention_values` by default, `attention_skip` as the alternative).
 *
 * The mask is ltxhip.h's: skip_layer_mask HOST f32 [num_layers, B], mask[l, b] == 1 = batch row b is perturbed in block l (the
 * published code uses the opposite polarity).  In block l, for batch row b, with
 *   n = rms_norm(h) * (1 + scale_msa) + shift_msa      the input of attn1
 *   v = to_v(n)                                         bias included, before the head split (no q/k norm, no RoPE)
 *   a                                                   the softmax attention output, before to_out
 *
 *   mode                 row with mask 0     row with mask 1
 *   transformer_block    block runs          block output = block input
 *   attention_skip       to_out(a)           to_out(n)
 *   attention_values     to_out(a)           to_out(v)
 *
 * In the two attention modes everything behind that - to_out with its bias, gate_msa, the residual, cross attention (never
 * perturbed) and the MLP - runs as usual for EVERY row; there is no block-level blend, and a block whose mask row is all ones still
 * runs.  Blocks of the permanent skip list (ltx_dit_set_skip_blocks) are skipped whole in every mode.  The attention modes take
 * mask values 0 and 1 only (anything else: LTX_ERR_ARG); transformer_block keeps blending fractional masks.  The published enum's
 * `residual` acts inside an attention module that owns a residual connection; this model's blocks have none, so it is not offered.
 * Conventions are those of ltxhip.h (device pointers unless marked HOST, 0 = success, ltx_last_error). */
#ifndef LTXHIP_STG_H
#define LTXHIP_STG_H
#include "ltxhip.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef enum { LTX_STG_TRANSFORMER_BLOCK = 0, LTX_STG_ATTENTION_SKIP = 1, LTX_STG_ATTENTION_VALUES = 2 } ltx_stg_mode;

/* Handle state, like the skip list: every forward that receives a skip_layer_mask obeys it - ltx_dit_forward,
 * ltx_dit_forward_frames and the perturbed branch of ltx_pipeline_call / _call_cond / _call_multiscale (both guidance_batch forms).
 * A NULL or all-zero mask returns the bits of LTX_STG_TRANSFORMER_BLOCK in every mode.  An unknown value is LTX_ERR_ARG and leaves
 * the handle as it was. */
int ltx_dit_set_stg_mode(ltx_dit* m, ltx_stg_mode mode);
int ltx_dit_get_stg_mode(const ltx_dit* m, ltx_stg_mode* out);

/* The strings of the published configs: "transformer_block", "attention_skip", "attention_values".  "residual" (see above), an
 * unknown name and NULL are LTX_ERR_ARG with a message that says why.  Host only: no device is touched. */
int ltx_stg_mode_from_name(const char* name, ltx_stg_mode* out);

/* dst[b*S + s, 0:D] = src[b*S + s, 0:D] for every batch row b with rows[b] != 0 and every s < S; all other rows of dst are left
 * alone.  One launch for all selected rows (what the attention modes run per perturbed block: v or n into the buffer to_out reads).
 *   dst [B*S, ldd], src [B*S, lds] of `dtype`; ldd, lds in elements;  rows HOST u8 [B], read before the call returns.
 * 16-byte accesses: D, ldd and lds must be multiples of 16 bytes' worth of elements and both pointers 16-byte aligned, otherwise
 * LTX_ERR_ARG.  No selected row: nothing is launched. */
int ltx_op_stg_fill(void* dst, int ldd, const void* src, int lds, const unsigned char* rows, int B, int S, int D,
                    ltx_dtype dtype, ltx_stream stream);

#ifdef __cplusplus
}
#endif
#endif
