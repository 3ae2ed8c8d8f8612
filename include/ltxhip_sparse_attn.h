/* ltxhip_sparse_attn.h — opt-in block-sparse self-attention for the DiT: attn1 of a flagged block computes only the 128-query x 64-key
 * score tiles a block map lists (the kernel under the published sparse video-DiT methods: Sliding Tile Attention, Radial Attention,
 * Sparse VideoGen reduce to flash attention that walks a per-query-block list of key tiles).  One kernel that takes ANY map, one map
 * builder (a window over (frame, row, column) plus sink frames); a later policy adds a builder and no kernel.  Handle state, like
 * ltxhip_int8_attn.h: with the switch off no launch, plan or bit of any other entry point changes.
 *
 * The definition.  Inputs are what attn1 holds after its q/k-norm + RoPE pass: q' bf16, ALREADY multiplied by scale * log2(e) (scores
 * come out in log2 units), k and v bf16, head_dim hd = 64 or 128, no key bias.
 *   The block map: uint32 map[MH][NQB][NW], MH = 1 (shared by the heads) or heads, NQB = ceil(Sq / 128), NKT = ceil(Sk / 64),
 *                 NW = ceil(NKT / 32); key tile kt is bit kt & 31 of word kt >> 5.  The map is shared by the batch rows.  Query i of
 *                 head h attends to every key j < Sk whose bit j / 64 is set in row (h or 0, i / 128), and to no other key.
 *   s[i][j]     = sum_d q'[i][d] * k[j][d]                   bf16 x bf16 -> f32
 *   x           = s - m_i,  p = exp2(x)                      m_i the exact running row maximum over the ATTENDED keys; the rescale of
 *                 O and l may be lazy as in the bf16 kernel (skipped while a tile's maximum exceeds m_i by less than 2^5).  The first
 *                 listed tile sets m_i: no first-tile guess, so no fallback pass and no counter.
 *   o           = (sum_j bf16(p) * v[j]) / l,  l = sum_j p   f32 accumulation, l from the UNROUNDED p, one rounding to bf16.
 *   Map edges   : bits at or above NKT are ignored by the kernel; a row with no bit set gives o = 0 for its queries.
 * The granularity is the definition: no element-level mask exists; only the ragged last key tile is masked by key index.  A tile that
 * no row lists is never read.
 *
 * The window map.  Tokens are in the DiT's order (f * H + h) * W + w, S = F * H * W.  Bit (qb, kt) is set iff some query token of block
 * qb and some key token of tile kt satisfy |df| <= wf, |dh| <= wh and |dw| <= ww, or tile kt holds a token of a frame < sink_frames.
 * Every row has its diagonal, so no row is empty.
 *
 * In the DiT a flagged block asks the q/k-norm pass for the prescaled q and runs the sparse launch in place of the bf16 self-attention
 * launch; under an STG attention mode the perturbed batch rows still get no attention launch.  Nothing derived from the weights is
 * cached, so adapters need no rule; every forward form and every ltx_pipeline_call* runs on whatever is set, as long as its token
 * count is the map's S.  attn2 stays dense.
 *
 * Out of scope: token reordering into 3-D tiles (STA's layout - without it the spatial window saves little in row-major order and the
 * saving comes from wf); per-head pattern search; sparse int8 scores; cross-attention; a generated-assembly loop; maps per batch row;
 * keyframe, multiscale second-pass and sharded forms under a map of another S (refused, see below).  Maps chosen from the content,
 * per batch row and head, are ltxhip_sparse_dynamic.h's: a producer on the device in front of this kernel.
 * Conventions are those of ltxhip.h (device pointers unless marked HOST, 0 = success, ltx_last_error). */
#ifndef LTXHIP_SPARSE_ATTN_H
#define LTXHIP_SPARSE_ATTN_H
#include <stddef.h>
#include <stdint.h>
#include "ltxhip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* words of a one-head map for Sq = Sk = S: ceil(S / 128) * ceil(ceil(S / 64) / 32); 0 for S < 1 */
size_t ltx_sparse_map_words(int64_t S);
/* map_out HOST [words], words == ltx_sparse_map_words(F * H * W); a grid side < 1, a negative window or sink count, a null map or
 * another `words`: LTX_ERR_ARG */
int ltx_sparse_window_map(int F, int H, int W, int wf, int wh, int ww, int sink_frames, uint32_t* map_out, size_t words);
/* set bits below NKT divided by NQB * NKT of a one-head map HOST for Sq = Sk = S; -1 on a null map or S < 1 */
double ltx_sparse_map_density(const uint32_t* map, int64_t S);

/* map HOST [map_heads][ltx_sparse_map_words(S)] or NULL.  The handle keeps a device copy; block_flags HOST [num_layers] or NULL
 * (NULL: every block).  A NULL map clears the flags and frees the copy: the handle is then again one never touched.  Refusals, the
 * handle unchanged: an f32 handle, a head_dim other than 64 or 128, a block flagged here and for int8 attention (this setter or
 * ltx_dit_set_int8_attention, whichever comes second): LTX_ERR_UNSUPPORTED; map_heads other than 1 or heads, S < 1, an empty map row:
 * LTX_ERR_ARG.  While any block is flagged a forward whose token count differs from S is refused: LTX_ERR_UNSUPPORTED. */
int ltx_dit_set_sparse_attention(ltx_dit* dit, const uint32_t* map, int map_heads, int64_t S, const unsigned char* block_flags, ltx_stream stream);
/* block_flags_out HOST [num_layers], 0 / 1; map_heads_out, S_out HOST or NULL (0 where nothing is set) */
int ltx_dit_get_sparse_attention(const ltx_dit* dit, unsigned char* block_flags_out, int* map_heads_out, int64_t* S_out);

/* ---- the kernel on its own (tests, tools): o bf16 [B, Sq, heads * hd] (row stride ldo) from q' / k / v bf16 (row strides ldq / ldk /
 * ldv) and map DEVICE [map_heads][ceil(Sq / 128)][ceil(ceil(Sk / 64) / 32)].  Refusals: a null or misaligned pointer (q, k, v: 16 bytes,
 * row strides % 8 == 0; o: 8 bytes, ldo % 4 == 0; map: 4 bytes), a row stride below heads * hd, map_heads other than 1 or heads:
 * LTX_ERR_ARG; a head_dim other than 64 or 128, a row offset of 2 GiB or more: LTX_ERR_UNSUPPORTED. ---- */
int ltx_op_attention_sparse(const void* q, const void* k, const void* v, void* o, const uint32_t* map, int map_heads,
                            int B, int Sq, int Sk, int heads, int hd, int ldq, int ldk, int ldv, int ldo, ltx_stream stream);

#ifdef __cplusplus
}
#endif
#endif
