/* ltxhip_int8_attn.h — opt-in INT8 Q K^T self-attention for the DiT on the int8 MFMA of gfx950 (v_mfma_i32_32x32x32_i8): the score
 * product of attn1 runs on int8 operands, K is smoothed by its per-channel mean over the sequence, P V stays bf16 (the published
 * "SageAttention" arithmetic).  Handle state, like the int8 linears of ltxhip_int8.h: with the switch off no launch, plan or bit of
 * any other entry point changes.
 *
 * The definition.  The quantisation rule is that of ltxhip_int8.h: symmetric, scale = amax / 127, inv = amax > 0 ? 127 / amax : 0,
 * q = clamp(rintf(x * inv), -127, 127) (round half to even), a zero group gives q = 0 and scale = 0; f32 with IEEE division, no
 * contraction.  Inputs are what the DiT's self-attention holds after its q/k-norm + RoPE pass: q' bf16, ALREADY multiplied by
 * scale * log2(e) (scores come out in log2 units), k and v bf16, head_dim hd = 64 or 128, D = heads * hd, no key bias.  Per batch
 * row b and head h:
 *   mean[b][c]  = (1 / Sk) sum_j float(k[b][j][c])         f32, for every channel c < D.  Summation order, a function of Sk alone: the
 *                 keys are cut into blocks of 64; P_i[c] adds block i's rows in ascending order from 0; eight chains
 *                 s_r = P_r + P_(r+8) + P_(r+16) + ... (ascending, from 0); mean = (((s_0 + s_1) + (s_2 + s_3)) + ((s_4 + s_5) +
 *                 (s_6 + s_7))) / float(Sk).  No atomics: the result repeats bit for bit.
 *   kc[j][c]    = float(k[j][c]) - mean[c]                  one f32 subtraction.  Softmax does not see it: q . mean is constant along a
 *                 score row.  It takes a per-channel offset of K out of the int8 range (without it the error grows with the offset).
 *   k8, ks      : kc quantised per (head, block of 64 consecutive keys): amax over the block's keys < Sk and the head's hd channels.
 *                 k8 int8 [B, Sk, D], ks f32 [B, heads, ceil(Sk / 64)].
 *   q8, qs      : float(q') quantised per (token, head) over its hd channels.  q8 int8 [B, Sq, D], qs f32 [B, heads, Sq].
 *   acc[i][j]   = sum_d q8[i][d] * k8[j][d]                 int32, exact
 *   s[i][j]     = float(acc[i][j]) * (qs[i] * ks[j / 64])   the scale product first, then ONE fma that also subtracts the running
 *                 maximum: x = fma(float(acc), qs * ks, -m_i)
 *   p           = exp2(x), m_i the exact running row maximum (O and l are rescaled whenever it moves; no first-tile guess, so no
 *                 fallback pass and no counter)
 *   o           = (sum_j bf16(p) * v[j]) / l,  l = sum_j p   f32 accumulation, l from the UNROUNDED p (as the bf16 kernel does), one
 *                 rounding to bf16.
 *
 * In the DiT a flagged block asks the q/k-norm pass for the prescaled q and runs kmean -> quant_qk_i8 -> attention_i8 in place of the
 * bf16 self-attention launch; under an STG attention mode the perturbed batch rows still get no attention launch.  Nothing derived
 * from the weights is cached, so adapters need no rule; the flag is independent of ltx_dit_set_int8_linears and composes with it;
 * every forward form and every ltx_pipeline_call* runs on whatever is set.  attn2 (the text cross-attention) stays bf16.
 *
 * Out of scope: fp8 P V; cross-attention; per-token K scales; fusing the quantisation into the q/k-norm + RoPE pass (the natural
 * follow-up: it would save the read of q and k and one launch); a generated-assembly form of the loop.
 * Conventions are those of ltxhip.h (device pointers unless marked HOST, 0 = success, ltx_last_error). */
#ifndef LTXHIP_INT8_ATTN_H
#define LTXHIP_INT8_ATTN_H
#include "ltxhip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* block_flags HOST [num_layers] or NULL: NULL gives every block `on`; with a list block l runs in int8 where block_flags[l] != 0 and
 * on != 0.  An f32 handle, or a head_dim other than 64 or 128: LTX_ERR_UNSUPPORTED.  The operand buffers (q8, k8, the scales, the mean)
 * are made by the next forward and freed when the last flag clears; the forward is then again that of a handle never touched. */
int ltx_dit_set_int8_attention(ltx_dit* dit, const unsigned char* block_flags, int on, ltx_stream stream);
/* block_flags_out HOST [num_layers], 0 / 1 */
int ltx_dit_get_int8_attention(const ltx_dit* dit, unsigned char* block_flags_out);

/* ---- the three kernels on their own (tests, tools).  Refusals: a null or misaligned pointer (bf16 / int8 tensors and mean: 16 bytes,
 * row strides % 8 == 0; o: 8 bytes, ldo % 4 == 0): LTX_ERR_ARG; a head_dim other than 64 or 128 (kmean: D % 8 != 0), an operand of
 * 2 GiB or more: LTX_ERR_UNSUPPORTED. ----
 * k bf16 [B, Sk, D] with row stride ldk elements -> mean f32 [B, D] */
int ltx_op_kmean(const void* k, int B, int Sk, int D, int ldk, float* mean, ltx_stream stream);
/* q, k bf16 [B, S*, heads * hd] with row strides ldq / ldk; mean f32 [B, heads * hd] -> q8, qs, k8, ks as above */
int ltx_op_quant_qk_i8(const void* q, const void* k, const float* mean, int B, int Sq, int Sk, int heads, int hd, int ldq, int ldk,
                       void* q8, float* qs, void* k8, float* ks, ltx_stream stream);
/* o bf16 [B, Sq, heads * hd] (row stride ldo) from the quantised operands and v bf16 [B, Sk, heads * hd] (row stride ldv) */
int ltx_op_attention_i8(const void* q8, const float* qs, const void* k8, const float* ks, const void* v, void* o,
                        int B, int Sq, int Sk, int heads, int hd, int ldv, int ldo, ltx_stream stream);

#ifdef __cplusplus
}
#endif
#endif
