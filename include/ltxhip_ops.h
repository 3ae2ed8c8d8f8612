/* ltxhip_ops.h — kernel-level C entry points of libltxhip.so.
 *
 * These expose the individual fused HIP kernels behind `ltx_dit_forward` / `ltx_vae_decode`
 * so that parity tests and micro-benchmarks can drive each one through the C ABI with plain
 * device pointers.  Each entry cites the reference code the kernel replaces
 * (FerrisMind/candle-video, src/models/ltx_video/...).  dtype: 0 = f32, 1 = bf16 (ltx_dtype).
 */
#ifndef LTXHIP_OPS_H
#define LTXHIP_OPS_H
#include "ltxhip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* nn::Linear (+ fused epilogue): y[M,N] = epi(x[M,K] @ w[N,K]^T + bias)
 *   epi 0: none | 1: GELU-tanh (ltx_transformer.rs:214-226) | 2: resid + gate[b,:]*y (:900,:934)
 *   | 3: resid + y (:909).  gate f32 [M/rows_per_batch, N]. */
int ltx_op_linear(const void* x, const void* w, const void* bias, void* y, int M, int N, int K, int dtype, int epi,
                  const void* resid, const float* gate, int rows_per_batch, ltx_stream stream);

/* nn::Linear (epi 0, or the residual forms 2 / 3) that also leaves the per-row partial sums of squares of its stored output, one f32 per 128-column
 * group: rowsq[m * ceil(N/128) + g].  The summation order is canonical (independent of the kernel the plan picks), so a
 * consumer can fold an RMS norm of the output rows without a pass over them: the cross-attention q-norm,
 * ltx_transformer.rs:671-678.  ltx_op_rowsq is the stand-alone form on a stored matrix: same values, bit for bit. */
/* bf16 linear layers of at most 512 rows (csrc/gemm_ring.hip): a second, tile-contiguous copy of w ([ceil(N/32)][ceil(K/64)][32][64],
 * zero padded; ltx_op_ring_packed_bytes bytes) lets the small-M kernel stream it in 4-KiB blocks.  Same results as ltx_op_linear;
 * measured to buy nothing for C1 and 4 % for T5-XXL, so the models build these copies only under LTX_RING_PACK=1. */
int64_t ltx_op_ring_packed_bytes(int N, int K);
int ltx_op_ring_pack(const void* w, int N, int K, void* out, ltx_stream stream);
int ltx_op_linear_packed(const void* x, const void* w, const void* w_packed, const void* bias, void* y, int M, int N, int K, int epi,
                         const void* resid, const float* gate, int rows_per_batch, ltx_stream stream);
int ltx_op_linear_rowsq(const void* x, const void* w, const void* bias, void* y, float* rowsq, int M, int N, int K, int dtype, int epi,
                        const void* resid, const float* gate, int rows_per_batch, ltx_stream stream);   /* epi 0, 2, 3 as ltx_op_linear */
int ltx_op_rowsq(const void* x, int64_t rows, int N, int ld, float* rowsq, int dtype, ltx_stream stream);

/* The norm fold of the DiT block (LtxVideoTransformerBlock::forward, ltx_transformer.rs:847-851, 905-909: y = h * r * (1 + sc) + sh
 * in front of the q|k|v and ff1 projections, r = 1 / sqrt(mean(h^2) + eps)), as the two GEMM epilogue sides that replace the norm
 * pass.  bf16, more than 512 rows, batch elements of at least 320 rows; LTX_ERR_ARG for a call the one-wave-per-SIMD kernels do
 * not serve - ltx_op_linear_fold_ok answers that without launching (consumer 0: the producer side, vec_stride = scale2_stride;
 * 1: the consumer side, vec_stride = cvec_stride, rs_n partials per row).  b(m) = m / rows_per_batch.
 *   fold_out (epi 2 / 3 as ltx_op_linear): y = the residual epilogue, rowsq = its row partials (ltx_op_linear_rowsq), and
 *     y2[m][n] = bf16(float(y[m][n] as stored) * (1.0f + scale2[b(m) * scale2_stride + n]))
 *   fold_in (epi 0 / 1, no bias): y = epi(r_m * (x @ w^T) + cvec[b(m) * cvec_stride + n]),
 *     r_m = 1 / sqrt(sum_g rs_sq[m * rs_n + g] / rs_D + eps); rs_n in {4, 8, 12, 16} */
int ltx_op_linear_fold_out(const void* x, const void* w, const void* bias, void* y, void* y2, float* rowsq, const float* scale2, int scale2_stride,
                           int M, int N, int K, int epi, const void* resid, const float* gate, int rows_per_batch, ltx_stream stream);
int ltx_op_linear_fold_in(const void* x, const void* w, void* y, const float* rs_sq, int rs_n, int rs_D, float eps, const float* cvec, int cvec_stride,
                          int M, int N, int K, int epi, int rows_per_batch, ltx_stream stream);
int ltx_op_linear_fold_ok(int M, int N, int K, int epi, int consumer, int rs_n, int vec_stride, int rows_per_batch);
/* cvec[b * cvec_stride + n] = sum_k shift[b * shift_stride + k] * w[n][k] + bias[n]: f32 from bf16 w [N, K] / bias (may be NULL), B <= 8 */
int ltx_op_shift_gemv(const void* w, const void* bias, const float* shift, int shift_stride, int B, int N, int K, float* cvec, int cvec_stride, ltx_stream stream);
/* y = h (.) (1 + scale[b]) on rows [B * rows_per_batch, D]: fold_out's second output as a stand-alone map (same bits) */
int ltx_op_mod_scale(const void* h, const float* scale, int scale_stride, void* y, int B, int64_t rows_per_batch, int D, int dtype, ltx_stream stream);
/* out[n][k] = w[n][k] * (1 + scale[k]): the factor of the fold moved into a copy of the consumer's weights */
int ltx_op_scale_cols(const void* w, const float* scale, void* out, int64_t N, int K, int dtype, ltx_stream stream);

/* The fused q|k|v projection of LtxAttention (ltx_transformer.rs:655-662: to_q, to_k, to_v on the same input) with the
 * output written as N/seg_width DENSE matrices: y[j][M][seg_width] = (x @ w^T + bias)[:, j*seg_width:(j+1)*seg_width].
 * seg_width a power of two dividing N. */
int ltx_op_linear_segmented(const void* x, const void* w, const void* bias, void* y, int M, int N, int K, int seg_width,
                            int dtype, ltx_stream stream);

/* The RMS form of ltx_op_rownorm for rows whose sums of squares are already known (presum [rows, presum_n], the by-product of
 * ltx_op_linear_rowsq / ltx_op_rowsq on x): a pure elementwise map, no row reduction. */
int ltx_op_rownorm_presum(const void* x, void* y, int64_t rows, int D, float eps, const void* weight,
                          const float* scale, const float* shift, int64_t rows_per_batch, int mod_stride, int act,
                          const float* presum, int presum_n, int dtype, ltx_stream stream);

/* A linear layer of at most 512 rows whose K ranges (the shape rule of the library: ltx_op_linear_split_factor(M, N, K), four from
 * K = 8192 up) are left UN-reduced: parts[p][M][N] f32 = x @ w[:, range p]^T, no bias, no epilogue (gemm_ring.hip; the DiT's ff2
 * at few tokens, LtxVideoTransformerBlock::forward ltx_transformer.rs:929-934).  ltx_op_rownorm_deferred finishes the rows:
 * h = resid + gate_b * (((p0 + p1) + ...) + bias) (gate NULL: resid + sum + bias), rounded to the dtype, written to h_out, then
 * y = the row norm of ltx_op_rownorm on h.  Together they return the bits of ltx_op_linear(epi 2 / 3) followed by ltx_op_rownorm. */
int ltx_op_linear_split_factor(int M, int N, int K);
int ltx_op_linear_deferred(const void* x, const void* w, float* parts, int M, int N, int K, ltx_stream stream);
int ltx_op_rownorm_deferred(const float* parts, int nparts, const void* bias, const void* resid, const float* gate, int gate_stride, void* h_out,
                            void* y, int64_t rows, int D, int kind, float eps, const float* scale, const float* shift, int64_t rows_per_batch,
                            int mod_stride, int dtype, ltx_stream stream);

/* RmsNorm / LayerNormNoParams + AdaLN modulate (+SiLU) on rows (ltx_transformer.rs:72-119, 874-889;
 * vae.rs:148-153, 711-739): y = act(norm(x)[*weight]*(1+scale_b)+shift_b). kind 0 RMS / 1 LN. */
int ltx_op_rownorm(const void* x, void* y, int64_t rows, int D, int kind, float eps, const void* weight,
                   const float* scale, const float* shift, int64_t rows_per_batch, int mod_stride, int act,
                   int dtype, ltx_stream stream);

/* q/k RMSNorm(weight, eps) over the full inner dim + apply_rotary_emb, in place (ltx_transformer.rs:671-678, 314-339).
 * cos/sin: f32 [rows, D/2] half-width tables or NULL. */
int ltx_op_qknorm_rope(void* x, int64_t rows, int D, int ld, const void* weight, float eps,
                       const float* cos, const float* sin, int dtype, ltx_stream stream);

/* The same pass the way the DiT calls it (LtxAttention::forward: norm_q / norm_k + RoPE on q and k of one fused projection), in
 * place on a caller-owned buffer: nseg = 1 or 2 segments of D columns per row, segment j of row m at
 * x + m * ld + j * (seg_stride ? seg_stride : D) elements - adjacent column blocks of a [rows, ld] row (seg_stride 0) or dense
 * planes seg_stride elements apart.  Segment 0: x * r * w0 [* w0b], rotated, times out_scale0 (r = 1 / sqrt(mean(x^2) + eps));
 * segment 1: x * r * w1, rotated with the same table row.  w1 NULL needs nseg = 1; w0b may be NULL; cos / sin both or neither.
 * Nothing outside the nseg segments of the first `rows` rows is written. */
int ltx_op_qknorm_rope_segs(void* x, int64_t rows, int D, int ld, int nseg, int64_t seg_stride, const void* w0, const void* w1, const void* w0b,
                            float eps, const float* cos, const float* sin, float out_scale0, int dtype, ltx_stream stream);

/* Diagnostic, read-only: which kernel of csrc/rownorm.hip serves a described call under the current options.  The launchers
 * switch on the same decision.  Nothing is launched, no device and no pointer are needed; dense rows (ld = D) are assumed.
 *   ltx_op_norm_route: ltx_op_rownorm (presum_n = nparts = 0), ltx_op_rownorm_presum (presum_n partials per row) or
 *     ltx_op_rownorm_deferred (nparts K ranges); flags say which operands are passed.  Names: "narrow", "block", "wide", "reread",
 *     "presum", "presum_lean", "wide_defer", "wide_defer4", "block_defer", "block_defer4" ("wide_rows": experiment builds).
 *   ltx_op_qknorm_route: ltx_op_qknorm_rope / ltx_op_qknorm_rope_segs.  Names: "block", "fused4", "fused8", "cached", "reread".
 * Both write "refused" where the launch would fail the described arguments with LTX_ERR_ARG. */
enum { LTX_NORM_SCALE = 1, LTX_NORM_SHIFT = 2, LTX_NORM_WEIGHT = 4 };
int ltx_op_norm_route(int64_t rows, int D, int dtype, int kind, int flags, int act, int64_t rows_per_batch, int presum_n, int nparts, char* name, int cap);
int ltx_op_qknorm_route(int64_t rows, int D, int dtype, char* name, int cap);

/* get_timestep_embedding, dim 256, order [cos | sin]: flavour 0 = the DiT's (ltx_transformer.rs:271-309, frequencies
 * 1/10000^(i/128)), 1 = the VAE's (vae.rs:172-198, exp(-ln(1e4) i / 128), timestep first multiplied by `multiplier` =
 * timestep_scale_multiplier, :1668-1676).  In bf16 the timestep is rounded to bf16 first (:1051).  timesteps: HOST [n], n <= 8;
 * out DEVICE [n,256] of `dtype`.  Blocks until done (it stages its 128-entry table itself). */
int ltx_op_timestep_embedding(const float* timesteps_host, int n, int vae_flavour, float multiplier, int dtype, void* out, ltx_stream stream);

/* LtxVideoRotaryPosEmbed::forward (ltx_transformer.rs:436-524): half-width tables [B*F*H*W, D/2];
 * coords f32 [B*S,3] or NULL (then the (f,h,w) grid scaled by rope_scale*patch/base or raw). */
int ltx_op_rope_table(float* cos, float* sin, const float* coords, int B, int F, int H, int W, int D,
                      const float* rope_scale_host, ltx_stream stream);

/* LtxAttention core (ltx_transformer.rs:699-741): o = softmax(scale q k^T + bias) v, q [B,Sq,heads*hd] etc. */
int ltx_op_attention(const void* q, const void* k, const void* v, void* o, int B, int Sq, int Sk, int heads, int hd,
                     int ldq, int ldk, int ldv, int ldo, float scale, const float* key_bias, int dtype, ltx_stream stream);
/* Diagnostic counters of the self-attention kernels' exact-max second pass (their fixed first-tile softmax max overflowed; the
 * result is exact either way, the pass costs time): counts[0] = head_dim-64 workgroups that re-ran since the last reset,
 * counts[1] = head_dim-128 launches whose gated exact pass ran.  Current device; blocks until the device copy is done. */
int ltx_attention_fallback_counts(unsigned long long counts[2], int reset);
/* Cross attention on UN-normalised queries (bf16, head_dim 64, Sk <= 128): softmax(r_i * scale * q_i . k_j + bias_j) v_j with
 * r_i = 1 / sqrt(sum_g q_rowsq[i*n + g] / D + eps), the RMS-norm scalar of query row i; the norm's weight is expected folded
 * into k by the caller (LtxAttention::forward with norm_q, ltx_transformer.rs:671-678, 719-740). */
int ltx_op_attention_rowsq(const void* q, const void* k, const void* v, void* o, int B, int Sq, int Sk, int heads, int hd,
                           int ldq, int ldk, int ldv, int ldo, float scale, const float* key_bias,
                           const float* q_rowsq, int q_rowsq_n, int q_rowsq_D, float q_rowsq_eps, ltx_stream stream);
/* ltx_op_attention for bf16, head_dim 64, Sk <= 128 with a key bias, run the way the DiT's cross attention runs it (dit.hip): the
 * keys whose bias is above -5000 are moved to the front of their batch row (order kept) and the kernel multiplies only the key
 * blocks that hold them - a masked text token (bias -10000, ltx_transformer.rs:1059-1070) has softmax weight exp(s - 10000 - max)
 * = +0.0f exactly, so the result is that of ltx_op_attention.  q_rowsq may be NULL (then q is used as it is).  counts_out
 * (DEVICE int [B], may be NULL) receives the number of keys kept per batch row.  Blocks until done (temporary buffers). */
int ltx_op_attention_compact(const void* q, const void* k, const void* v, void* o, int B, int Sq, int Sk, int heads, int hd,
                             int ldq, int ldk, int ldv, int ldo, float scale, const float* key_bias,
                             const float* q_rowsq, int q_rowsq_n, int q_rowsq_D, float q_rowsq_eps, int* counts_out, ltx_stream stream);
/* attn2.to_out folded into the cached text context (csrc/xattn_fold.hip, option xattn_fold_vo): with P_h the row-normalised
 * softmax of head h, h + (sum_h P_h V_h) Wo^T + b = h + sum_h P_h (V_h Wo_h^T) + b, and V_h Wo_h^T depends on the prompt and the
 * weights alone.  KP = the largest kept-key count of the batch rows, rounded up to 32.
 *   ltx_op_xattn_fold_route: read-only, the decision the DiT's context build asks - *fold = 1 where a compact bf16 head_dim-64
 *     context of KP columns per head carries vo (heads * KP <= T * D, T = 1/2 measured: profiles/xattn_fold_vo_bench.md), else 0.
 *     No device.
 *   ltx_op_xattn_fold_kp: KP of HOST counts [B].
 *   ltx_op_xattn_fold_build: the build kernel on one layer - v [B,K,heads*64] bf16 and key_bias [B,K] as ltx_op_attention_compact
 *     takes them, wo [D,D] bf16; vo [B][D][heads*KP] bf16 with vo[b][n][h*KP + k] = sum_d wo[n][64h + d] * v_kept[b][k][64h + d]
 *     (f32 accumulation, one bf16 rounding), exact zeros from a row's count on.  Blocks until done.
 *   ltx_op_attention_probs: the cross kernel's P-only mode after the same compaction - p [B*Sq][heads*KP] bf16,
 *     p[row][h*KP + k] = bf16(softmax weight of kept key k), exact zeros from the row's count on.  q_rowsq as in
 *     ltx_op_attention_rowsq, may be NULL.  Blocks until done. */
int ltx_op_xattn_fold_route(int dtype, int head_dim, int heads, int D, int KP, int B, int compact, int* fold);
int ltx_op_xattn_fold_kp(const int* counts_host, int B, int* KP);
int ltx_op_xattn_fold_build(const void* v, const float* key_bias, const void* wo, int B, int K, int heads, int KP, void* vo, int* counts_out, ltx_stream stream);
int ltx_op_attention_probs(const void* q, const void* k, void* p_out, int B, int Sq, int Sk, int heads, int KP, float scale, const float* key_bias,
                           const float* q_rowsq, int q_rowsq_n, float q_rowsq_eps, int* counts_out, ltx_stream stream);
/* Same core for bf16, head_dim 64 or 128, no key bias, with q ALREADY multiplied by scale*log2(e) (the DiT self-attention
 * path folds that factor into the q RMSNorm+RoPE kernel): o = softmax_base2(q' k^T) v. */
int ltx_op_attention_prescaled(const void* q, const void* k, const void* v, void* o, int B, int Sq, int Sk, int heads, int hd,
                               int ldq, int ldk, int ldv, int ldo, ltx_stream stream);

/* LtxVideoCausalConv3d 3x3x3 (vae.rs:415-464) on channels-last x [B,T,H,W,Cin] with reference-layout weight
 * [Cout,Cin,3,3,3] (any dtype `wdtype`); y channels-last [B,T,H,W,Cout]; resid optional [.., Cout]. */
int ltx_op_conv3d(const void* x, const void* w, const void* bias, int wdtype, void* y, const void* resid,
                  int B, int T, int H, int W, int Cin, int Cout, int causal, int dtype, ltx_stream stream);

/* ltx_op_conv3d (no residual) finished with the consumer's per-voxel RMS norm, modulation and activation inside the conv's epilogue
 * (LtxVideoResnetBlock3d: conv1 + norm2, vae.rs:779-801; the encoder's calls pass eps = 1e-8 and no modulation):
 *   y[b,t,h,w,:] = act(r * c * (1 + scale[b*mod_stride + :]) + shift[b*mod_stride + :]),  c = the conv's output row as ltx_op_conv3d
 *   stores it (rounded to bf16), r = 1 / sqrt(mean_n(c^2) + eps); act 0: none, 1: SiLU.
 * scale / shift: f32 DEVICE rows of Cout values, mod_stride floats apart (column slices of one table: mod_stride >= Cout, a
 * multiple of 4, 16-byte aligned pointers), or both NULL: no modulation.  Served by the halo-staged kernel alone: bf16, Cout 128 or
 * 256, Cin a multiple of 64, at least 16 voxels, options gemm_wide_epi on and gemm_off without halo / big; LTX_ERR_ARG for any
 * other call (ltx_op_gemm_route with LTX_ROUTE_PN answers the same question) - never a conv without the norm. */
int ltx_op_conv3d_norm(const void* x, const void* w, const void* bias, int wdtype, void* y, const float* scale, const float* shift, int mod_stride,
                       float eps, int act, int B, int T, int H, int W, int Cin, int Cout, int causal, int dtype, ltx_stream stream);

/* LtxVideoUpsampler3d (vae.rs:1090-1169): conv + depth-to-space(2,2,2) + drop first frame + tiled residual.
 * x [B,T,H,W,Cin] -> y [B,2T-1,2H,2W,Cout/8] channels-last. */
int ltx_op_upsample3d(const void* x, const void* w, const void* bias, int wdtype, void* y,
                      int B, int T, int H, int W, int Cin, int Cout, int causal, int residual, int dtype, ltx_stream stream);

/* LtxVideoDownsampler3d (vae.rs:499-582), the encoder's pixel-unshuffle downsampler: causal conv Cin -> Cout/(st*sh*sw) on the
 * input with st - 1 leading frames repeated, space-to-depth to channel ((c*st + it)*sh + ih)*sw + iw, plus the same
 * re-arrangement of x averaged over groups of Cin*st*sh*sw/Cout consecutive channels.  down_type: 1 spatial (1,2,2),
 * 2 temporal (2,1,1), 3 spatiotemporal (2,2,2) (LTX_DOWN_* of ltxhip_encoder.h; 0, the strided conv, is LTX_ERR_UNSUPPORTED).
 * x [B,T,H,W,Cin] -> y [B,(T+st-1)/st,H/sh,W/sw,Cout] channels-last; w [Cout/(st*sh*sw),Cin,3,3,3]. */
int ltx_op_downsample3d(const void* x, const void* w, const void* bias, int wdtype, void* y,
                        int B, int T, int H, int W, int Cin, int Cout, int down_type, int dtype, ltx_stream stream);

/* conv_out + unpatchify(4) (vae.rs:1626-1654, 1724-1725): x [B,T,H,W,Cin] -> f32 NCTHW [B,Cout/16,T,4H,4W]. */
int ltx_op_conv_out_unpatchify(const void* x, const void* w, const void* bias, int wdtype, float* y,
                               int B, int T, int H, int W, int Cin, int Cout, int causal, int postprocess, int dtype, ltx_stream stream);

/* blend_h / blend_v / blend_t of the tiled decode (vae.rs:1927-2006), in place on b:
 * b[..., x] = a[..., -blend + x]*(1 - x/blend) + b[..., x]*(x/blend) along dim (2=T, 3=H, 4=W); a,b f32 [BC,t,h,w]. */
int ltx_op_blend(const float* a, float* b, int BC, int at, int ah, int aw, int bt, int bh, int bw, int dim, int blend_extent, ltx_stream stream);

/* Diagnostic: which GEMM plan (tile shape / kernel) the dispatcher measured best and cached for a bf16 problem shape
 * (conv = 0: [M,K] x [N,K]^T; conv = 1: K = Cin, ntaps/T/H/W = conv geometry).  Writes a NUL-terminated name
 * ("192x128", "p8:256", ... or "" if the shape has not run yet) into name[cap]. */
int ltx_op_gemm_plan(int M, int N, int K, int conv, int ntaps, int T, int H, int W, char* name, int cap);

/* Diagnostic, read-only: where the GEMM dispatch sends a described call under the current options - "gemm128" (the 128 x 128
 * kernel), "asm32" (experiment builds) or a plan name ("asm16:160x256", "ring:96x96", "halo:64", ...): the forced plan, else
 * the cached one, else the static model's.  Nothing is launched or measured and no pointer is needed: dense operands are
 * assumed.  conv = 1: K = Cin, M = B T H W, ntaps taps; epi 0 .. 6 (bias, GELU, gate + residual, residual, depth-to-space,
 * unpatchify, space-to-depth); dtype as everywhere (1 = bf16).  flags describe the operand fields the dispatch reads.
 * LTX_ERR_ARG where ltx_launch would refuse the call (deferred K ranges / norm-fold operands / the fused output norm on a kernel
 * without them). */
enum { LTX_ROUTE_PN = 1,         /* conv with the fused output norm */
       LTX_ROUTE_DEFER = 2,      /* K-range sums left to the consumer (ltx_op_linear_deferred) */
       LTX_ROUTE_FOLD_IN = 4,    /* ltx_op_linear_fold_in's operands (16 row partials) */
       LTX_ROUTE_FOLD_OUT = 8 }; /* ltx_op_linear_fold_out's operands */
int ltx_op_gemm_route(int M, int N, int K, int conv, int ntaps, int B, int T, int H, int W, int epi, int dtype, int flags, char* name, int cap);

/* Diagnostic, read-only: the decisions of one DiT forward of B <= 8 batch rows under the current options, for a model of
 * heads x head_dim channels, S latent tokens and K text tokens per row and G modulation groups per row (1, or the latent frames
 * of ltx_dit_forward_frames; G divides S); skip_mask: a skip-layer mask is passed.  No handle and no device are needed.
 * out[LTX_DIT_PLAN_FIELDS]: M, MK, NB, Sg, seg, ldqkv (sizes), then fold_q2, presum, nfold, defer_ff2, ff2_parts, dense_qkv, fold_q. */
enum { LTX_DIT_PLAN_FIELDS = 13 };
int ltx_op_dit_plan(int heads, int head_dim, int model_dtype, int io_dtype, int B, int S, int K, int G, int skip_mask, int64_t* out);

#ifdef __cplusplus
}
#endif
#endif
