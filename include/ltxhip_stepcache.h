/* ltxhip_stepcache.h — timestep-aware step caching for the DiT (published as "TeaCache"): on denoise steps whose model input barely
 * moved, the transformer blocks are not run and the block residual of the last computed step is added instead.  Opt-in and
 * approximate by design; every other entry point keeps its launches and its bits.
 *
 * Per step, for the B videos of a call (every guidance branch of a step sees the same latents and timesteps):
 *   h    = proj_in(latents)                                                      model dtype, [B * S, D]
 *   m    = round(rms_norm(h, norm_eps) * (1 + scale_msa) + shift_msa)            block 0's modulated input, model dtype
 *   d    = sum |m - m_prev| / sum |m_prev|                                       both sums in f64, fixed order: results repeat
 * and with the state (acc, whether a previous measurement exists), for step i of N:
 *   compute, acc = 0      no previous measurement, i == 0, i == N - 1, sum |m_prev| == 0, or d not finite
 *   otherwise             acc += poly(d),  poly(x) = (((c0 x + c1) x + c2) x + c3) x + c4  (Horner, f64, from the f32 coefficients);
 *                         reuse iff acc < rel_l1_thresh, else compute and acc = 0
 *   pattern[i]            0: as above; 1: compute (acc = 0); 2: reuse (acc stays).  Steps past n_pattern: 0.
 *   a step that would re-use a cache row that holds no residual (never computed, another sequence length, weights changed since)
 *   computes, and acc = 0.
 * A computed forward stores  resid = h_after_blocks - h_after_proj_in  per cache row; a re-used one runs proj_in, adds resid, and runs
 * the final norm and proj_out: no text context, no RoPE table, no block, no attention.
 * The coefficients are the caller's: a published fit for the checkpoint in use goes into coeff[] (highest power first).  The default
 * is the identity with threshold 0, which never re-uses.
 * Conventions are those of ltxhip.h (device pointers unless marked HOST, 0 = success, ltx_last_error). */
#ifndef LTXHIP_STEPCACHE_H
#define LTXHIP_STEPCACHE_H
#include "ltxhip.h"
#include "ltxhip_cond.h"
#include "ltxhip_guidance.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    float rel_l1_thresh;                /* reuse while the accumulated rescaled distance stays below it; 0: never */
    float coeff[5];                     /* c0 .. c4 of poly */
    const unsigned char* pattern;       /* HOST [n_pattern] or NULL: 0 decide, 1 compute, 2 reuse */
    int n_pattern;
} ltx_step_cache_params;

typedef struct ltx_step_cache ltx_step_cache;

/* rel_l1_thresh 0, coeff {0, 0, 0, 1, 0}, no pattern */
void ltx_step_cache_params_default(ltx_step_cache_params* p);

/* A cache of `rows` batch rows for forwards of `dit` (>= 1; the pipeline call uses 3 * B: one set per guidance branch).  It owns the
 * previous measurement, the residuals [rows][S][D] in the model's dtype (allocated for the S of the first computed forward), a small
 * workspace of partial sums and a pinned pair of doubles.  _reset forgets the measurement, the accumulator and every residual. */
int ltx_step_cache_create(ltx_dit* dit, int rows, ltx_step_cache** out);
void ltx_step_cache_destroy(ltx_step_cache* cache);
int ltx_step_cache_reset(ltx_step_cache* cache);

/* The measurement and the decision of step `step` of `n_steps` for hidden [B, S, in_channels] (io_dtype): cast, proj_in, the time
 * tables (cached per timestep like the forward's), the measure pass, a fixed-order finish, two doubles to the host and ONE stream
 * synchronisation, then the rule above.  frames == 0: timestep HOST [B]; else HOST [B, num_frames], one per latent frame, and S must
 * equal num_frames * height * width (ltx_dit_forward_frames).  *reuse: 0 / 1.  *distance (NULL ok): d as f32, 0 on the first measurement.
 * A cache row is not looked at here: see ltx_step_cache_require. */
int ltx_step_cache_decide(ltx_step_cache* cache, ltx_dit* dit, const void* hidden, const float* timestep, int frames,
                          int B, int S, int num_frames, int height, int width, ltx_dtype io_dtype,
                          int step, int n_steps, const ltx_step_cache_params* params, int* reuse, float* distance, ltx_stream stream);

/* If *reuse and one of the rows [row0, row0 + nrows) holds no residual for sequence length S and the model's present weights:
 * *reuse = 0 and acc = 0 (the step computes).  Host only.  Called between _decide and the step's forwards. */
int ltx_step_cache_require(ltx_step_cache* cache, const ltx_dit* dit, int row0, int nrows, int S, int* reuse);

/* ltx_dit_forward (frames == 0) or ltx_dit_forward_frames (frames != 0: timestep HOST [B, num_frames]) through the cache rows
 * [row0, row0 + B).
 *   reuse == 0   the launches of the uncached forward in their order, plus a copy of h after proj_in and the residual kernel once h is
 *                complete; `out` has the bits of the uncached forward, the rows become valid
 *   reuse != 0   h = proj_in(x) + resid, the final norm, proj_out; enc, enc_mask, rope_scale, video_coords and skip_layer_mask are
 *                not read.  A row without a residual, or with one of another S: LTX_ERR_ARG, naming the row. */
int ltx_dit_forward_cached(ltx_dit* dit, ltx_step_cache* cache, int row0, int reuse, int frames,
                           const void* hidden, const void* enc, const float* timestep, const float* enc_mask,
                           int B, int S, int K, int num_frames, int height, int width,
                           const float* rope_scale, const float* video_coords, const float* skip_layer_mask,
                           ltx_dtype io_dtype, void* out, ltx_stream stream);

/* the residual of cache row `row` as f32 [S, D] (tests); LTX_ERR_ARG when the row holds none */
int ltx_step_cache_read_residual(const ltx_step_cache* cache, int row, float* dst, ltx_stream stream);

/* ltx_pipeline_call / _cond / _sched with the step cache: sched NULL = the scalars of `p`; cond NULL or without held frames = no
 * conditioning.  One _decide per step on the B videos, then every branch forward of the step through ltx_dit_forward_cached with that
 * decision; the cache has 3 * B rows, one set per branch slot (negative prompt, prompt, perturbed prompt), and lives for the call.
 * reused_out HOST u8 [N] (NULL ok): 1 where the step re-used; distance_out HOST f32 [N] (NULL ok).  With rel_l1_thresh 0 and no pattern
 * the latents and the video have the bits of the uncached call.  Keyframe items, the multi-scale call and the sharded forms are not
 * covered. */
int ltx_pipeline_call_cached(ltx_dit* dit, ltx_vae* vae, const ltx_pipeline_params* p, const ltx_guidance_schedule* sched,
                             const ltx_conditioning* cond, const ltx_step_cache_params* cache_params,
                             float* latents, const float* prompt_embeds, const float* prompt_mask,
                             const float* neg_embeds, const float* neg_mask, const float* decode_noise,
                             int B, int K, float* out_video, ltx_stream stream,
                             unsigned char* reused_out, float* distance_out);

/* ---- the two kernels on their own (tests, tools) ----
 * One pass over h and prev [rows, D] (dtype): per row the RMS norm with eps, m = round(n * (1 + scale[g]) + shift[g]) with
 * g = row / rows_per_batch and f32 tables of row stride mod_stride; sums[0] = sum |m - prev|, sums[1] = sum |prev| (DEVICE f64 [2]);
 * m is written over prev.  first != 0: prev is not read, sums[0] = sums[1] = 0.  ws: DEVICE, ltx_op_step_measure_ws_bytes(rows, D,
 * dtype), 16-byte aligned.  D must be a multiple of 128 (at most 4096 in f32, 8192 in bf16): else LTX_ERR_UNSUPPORTED. */
size_t ltx_op_step_measure_ws_bytes(int64_t rows, int D, ltx_dtype dtype);
int ltx_op_step_measure(const void* h, void* prev, const float* shift, const float* scale, int mod_stride, int64_t rows, int D,
                        int64_t rows_per_batch, float eps, ltx_dtype dtype, int first, void* ws, double* sums, ltx_stream stream);
/* r = h - r in place over [rows, D] (dtype), 16-byte accesses: D * sizeof(element) a multiple of 16, aligned pointers */
int ltx_op_step_residual(const void* h, void* r, int64_t rows, int D, ltx_dtype dtype, ltx_stream stream);

#ifdef __cplusplus
}
#endif
#endif
