/* ltxhip_sparse_dynamic.h — content-adaptive block maps for the block-sparse self-attention of ltxhip_sparse_attn.h, built ON THE
 * DEVICE from the forward's own q and k: per batch row, head and 128-query block, on every step (the producer under SpargeAttn's /
 * MInference's pooled block scores and Sparse VideoGen's per-head choice; ltxhip_sparse_attn.h's kernel walks whatever comes out).
 * Handle state like ltxhip_sparse_attn.h: with the switch off no launch, plan or bit of any other entry point changes.  Because the
 * map is made from the q and k of the forward at hand it holds for ANY token count: keyframe and multi-scale forms run.
 *
 * The definition.  Self-attention, Sq = Sk = S.  Inputs are what attn1 holds after its q/k-norm + RoPE pass: q' bf16 ALREADY
 * multiplied by scale * log2(e), k bf16, head_dim hd = 64 or 128.  NQB = ceil(S / 128), NKT = ceil(S / 64), NW = ceil(NKT / 32).
 *   qbar[b][h][qb][d] = (sum_i q'[b][128 qb + i][h][d]) / rows     f32, the block's rows (128, fewer in the last block) added in
 *                       ascending order, ONE division by float(rows)
 *   kbar[b][h][kt][d] = the same over the tile's keys (64, fewer in the last tile)
 *   s^[qb][kt]        = sum_d qbar[qb][d] * kbar[kt][d]            f32 FMA chain, d ascending
 *   w_kt              = keys in tile kt (64, or S - 64 (NKT - 1))
 *   p^[kt]            = w_kt * exp2(s^[kt] - max_kt s^)            the pooled estimate of the tile's softmax mass, up to 1 / T
 *   T                 = sum_kt p^[kt]                              f32, kt ascending
 *   tile j PRECEDES tile i  iff  p^_j > p^_i, or p^_j == p^_i and j < i
 *   before_i          = sum_{j precedes i} p^_j                    f32, j ascending
 *   tile i is SELECTED iff  before_i < mass * T    (the shortest descending prefix that reaches the requested mass of the estimate)
 *                       or  mass >= 1              (every tile: a rule, not left to rounding)
 *                       or  i in {2 qb, 2 qb + 1}, i < NKT   (the diagonal: no row is ever empty)
 *                       or  bit i of the caller's `keep` map row (h or 0, qb) is set   (e.g. a window plus sink frames from
 *                           ltx_sparse_window_map; ltxhip_sparse_attn.h's format, [1 or heads][NQB][NW])
 *   map[b][h][qb][w]    uint32, ltxhip_sparse_attn.h's bit layout, bits at or above NKT zero;  count[b][h][qb] = the row's set bits.
 * Nothing is atomic and every order above is a function of S alone: the maps repeat bit for bit.  A tile whose before_i is within
 * rounding of mass * T may fall on either side; tests/sparse_select_ref.py bounds that margin.
 *
 * The attention then runs ltxhip_sparse_attn.h's kernel with one map per (batch row, head): the kernel takes a map batch stride in
 * words (0: the map is shared by the batch rows, every earlier caller).
 *
 * In the DiT a flagged block asks the q/k-norm pass for the prescaled q, then pool_qk -> sparse_select -> the batched sparse launch;
 * STG runs of unperturbed rows go through the same three launches.  Nothing derived from the weights is cached.  The forward never
 * waits for the device: the counts are read by ltx_dit_sparse_dynamic_density, a tool's call.
 *
 * Out of scope: pooling fused into the q/k-norm pass; a map re-used across steps or layers; sparse int8 scores; token reordering.
 * NO claim about output quality: this repository holds no trained weights, the densities it reports are those of synthetic ones.
 * Conventions are those of ltxhip.h (device pointers unless marked HOST, 0 = success, ltx_last_error). */
#ifndef LTXHIP_SPARSE_DYNAMIC_H
#define LTXHIP_SPARSE_DYNAMIC_H
#include <stddef.h>
#include <stdint.h>
#include "ltxhip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define LTX_SPARSE_DYNAMIC_MAX_S 131072      /* NKT <= 2048: a map row's p^ fit one wave's LDS strip */

/* mass in (0, 1]; keep_map HOST [keep_heads][ltx_sparse_map_words(keep_S)] or NULL (then keep_heads and keep_S are ignored and ANY
 * token count is served; with a keep map a forward of another token count is refused: LTX_ERR_UNSUPPORTED); block_flags HOST
 * [num_layers] or NULL (every block).  mass == 0 with NULL block_flags clears the state and frees the buffers.  Refusals, the handle
 * unchanged: mass outside (0, 1], keep_heads other than 1 or heads, keep_S outside 1 .. LTX_SPARSE_DYNAMIC_MAX_S: LTX_ERR_ARG; an f32
 * handle, a head_dim other than 64 or 128, a block also flagged for int8 attention (this setter or ltx_dit_set_int8_attention,
 * whichever comes second), a handle with a static map set (and ltx_dit_set_sparse_attention while this mode is on - clear the other
 * first): LTX_ERR_UNSUPPORTED.  A forward of more than LTX_SPARSE_DYNAMIC_MAX_S tokens is refused while a block is flagged. */
int ltx_dit_set_sparse_attention_dynamic(ltx_dit* dit, float mass, const uint32_t* keep_map, int keep_heads, int64_t keep_S,
                                         const unsigned char* block_flags, ltx_stream stream);
/* block_flags_out HOST [num_layers], 0 / 1; mass_out, keep_heads_out, keep_S_out HOST or NULL (0 where nothing is set) */
int ltx_dit_get_sparse_attention_dynamic(const ltx_dit* dit, unsigned char* block_flags_out, float* mass_out, int* keep_heads_out, int64_t* keep_S_out);
/* per_block_out HOST [num_layers]: selected tiles / (rows * heads * NQB * NKT) of the handle's last forward (its last chunk of up to
 * eight batch rows; `rows` are the batch rows whose attention ran) for a flagged block, -1 for any other block or before a forward.
 * WAITS for the stream of that forward. */
int ltx_dit_sparse_dynamic_density(ltx_dit* dit, double* per_block_out);

/* ---- the kernels on their own (tests, tools) ---- */
/* qbar f32 [B, heads, ceil(S / 128), hd] and kbar f32 [B, heads, ceil(S / 64), hd] from q' / k bf16 [B, S, heads * hd] (row strides
 * ldq / ldk): one launch, one pass over q and k.  Refusals: a null or misaligned pointer (16 bytes; ldq, ldk % 8 == 0), a row stride
 * below heads * hd: LTX_ERR_ARG; a head_dim other than 64 or 128: LTX_ERR_UNSUPPORTED (offsets are 64-bit: no size limit). */
int ltx_op_pool_qk(const void* q, const void* k, float* qbar, float* kbar, int B, int S, int heads, int hd, int ldq, int ldk, ltx_stream stream);
/* map_out uint32 [B, heads, NQB, NW] and count_out uint32 [B, heads, NQB] from qbar / kbar of ltx_op_pool_qk; keep DEVICE
 * [keep_heads][NQB][NW] or NULL.  Refusals: a null or misaligned pointer (qbar, kbar: 16 bytes), mass outside (0, 1], keep_heads other
 * than 1 or heads with a keep map: LTX_ERR_ARG; a head_dim other than 64 or 128, S above LTX_SPARSE_DYNAMIC_MAX_S: LTX_ERR_UNSUPPORTED. */
int ltx_op_sparse_select(const float* qbar, const float* kbar, const uint32_t* keep, int keep_heads, uint32_t* map_out, uint32_t* count_out,
                         int B, int S, int heads, int hd, float mass, ltx_stream stream);
/* ltx_op_attention_sparse with map_batch_stride WORDS between the maps of two batch rows (0: one map for all of them, the bits of
 * ltx_op_attention_sparse); a stride that is neither 0 nor at least map_heads * NQB * NW: LTX_ERR_ARG */
int ltx_op_attention_sparse_batched(const void* q, const void* k, const void* v, void* o, const uint32_t* map, int map_heads, int64_t map_batch_stride,
                                    int B, int Sq, int Sk, int heads, int hd, int ldq, int ldk, int ldv, int ldo, ltx_stream stream);

#ifdef __cplusplus
}
#endif
#endif
