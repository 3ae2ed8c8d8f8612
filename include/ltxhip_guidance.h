/* ltxhip_guidance.h — guidance that changes over the denoise steps: one (guidance_scale, stg_scale, rescale, perturbed block list)
 * per schedule entry, CFG-star, and the two places a rescale can sit.  The guided recipes of the 0.9.7 / 0.9.8 dev models are of
 * this shape; ltx_pipeline_params (ltxhip.h) carries one value of each for the whole call.
 *
 * A schedule has n entries (1 <= n <= 64).  Step i of a call runs from sigma_i, the i-th of the N + 1 sigmas of the call:
 *   with guidance_timesteps     entry(i) = argmin_j |guidance_timesteps[j] - sigma_i|   (in double on the f32 values, first minimum)
 *   without                     n == 1 (every step) or n == N (entry i is step i); anything else is LTX_ERR_ARG
 * With g, s, r the entry's values, a step runs
 *   text        always
 *   uncond      iff g > 1
 *   perturbed   iff s > 0, the mask ones on the entry's block list (the handle's STG mode decides what that perturbs: ltxhip_stg.h)
 * A step with s == 0 runs no perturbed forward and skips nothing; the handle's permanent skip list is cleared for the whole call.
 *
 * The mix, per batch row over all its elements (t, u, p: the three predictions):
 *   alpha  = <t,u> / (<u,u> + 1e-8)  if cfg_star and the step has uncond, else 1      (sums in f64, alpha rounded to f32 once)
 *   c      = t without uncond;  with it  u' = alpha * u,  c = u' + g * (t - u')
 *   LTX_RESCALE_CFG (the reference, t2v_pipeline.rs:941-962)      LTX_RESCALE_MIX (the published recipes)
 *     if uncond and r > 0:  c *= r * (std t / std c) + (1 - r)      if perturbed:  c += s * (t - p)
 *     if perturbed:  c += s * (t - p)                               if perturbed and r != 1:  c *= r * (std t / std c) + (1 - r)
 * std is unbiased, per batch row, over held and free tokens alike; std c is taken of c as it stands in front of the rescale.  In
 * LTX_RESCALE_MIX an entry with r == 1 is not rescaled (the recipes use 1 as "off").  The scheduler update behind the mix is that of
 * ltx_guidance_step / _stochastic / _held (ltxhip.h, ltxhip_cond.h).
 * Conventions are those of ltxhip.h (device pointers unless marked HOST, 0 = success, ltx_last_error). */
#ifndef LTXHIP_GUIDANCE_H
#define LTXHIP_GUIDANCE_H
#include "ltxhip.h"
#include "ltxhip_cond.h"
#include "ltxhip_upsampler.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef enum { LTX_RESCALE_CFG = 0, LTX_RESCALE_MIX = 1 } ltx_rescale_form;

typedef struct {
    int n;                              /* entries, 1..64 */
    const float* guidance_scale;        /* HOST [n] */
    const float* stg_scale;             /* HOST [n], >= 0 */
    const float* rescale;               /* HOST [n] */
    const int* skip_blocks;             /* HOST: the block lists of all entries, one after the other (may be NULL when every list is empty) */
    const int* skip_offsets;            /* HOST [n + 1]: entry j perturbs skip_blocks[skip_offsets[j] .. skip_offsets[j + 1]) */
    const float* guidance_timesteps;    /* HOST [n] or NULL */
    int cfg_star;                       /* 0 / 1 */
    int rescale_form;                   /* ltx_rescale_form */
} ltx_guidance_schedule;

/* entry_of_step[i] for the N steps that start at sigmas[0 .. N) (HOST, the list ltx_sched_set_timesteps writes).  Host only.
 * LTX_ERR_ARG with a message: n outside 1..64, a NULL array, a non-finite scale or timestep, a negative stg_scale, a negative block
 * index, offsets that do not start at 0 or decrease, an unknown rescale_form, cfg_star outside 0 / 1, an n that matches neither rule. */
int ltx_guidance_schedule_resolve(const ltx_guidance_schedule* sched, const float* sigmas, int N, int* entry_of_step);

/* bytes of the device workspace of ltx_guidance_step_ex for B batch rows of n elements (0 for a bad argument) */
size_t ltx_guidance_ws_bytes(int B, int64_t n);

/* The mix above and the scheduler update in three launches at most: one pass over the predictions for nine sums per batch row
 * (partials per block in `ws`, no floating-point atomics), a fixed-order finish that writes alpha and factor, and the apply pass in
 * 16-byte accesses.  Results repeat bit for bit.
 *   text, uncond, perturbed  [B, n] pred_dtype; uncond / perturbed NULL = that branch is absent (the caller decides by g > 1, s > 0)
 *   latents        f32 [B, n] in place, or NULL (then only noise_pred_out is written)
 *   noise_pred_out f32 [B, n] or NULL
 *   step_noise     NULL: Euler, latents += dt * c;  else f32 [B, n]: x = (1 - sigma_next) * (x - sigma * c) + sigma_next * step_noise
 *   hold           NULL, or DEVICE u8 [B, num_frames] with n == num_frames * frame_elems: held frames keep their latents' bits
 *   ws             DEVICE, ltx_guidance_ws_bytes(B, n), 16-byte aligned
 *   scalars_out    NULL, or DEVICE f32 [B, 2]: (alpha, factor) of every batch row - factor is what the rescale multiplies c by, 1 when
 *                  it does not act */
int ltx_guidance_step_ex(const void* text, const void* uncond, const void* perturbed, ltx_dtype pred_dtype,
                         float* latents, float* noise_pred_out, int B, int64_t n,
                         float guidance_scale, float guidance_rescale, float stg_scale, int cfg_star, int rescale_form,
                         float dt, float sigma, float sigma_next, const float* step_noise,
                         const unsigned char* hold, int num_frames, int64_t frame_elems,
                         void* ws, float* scalars_out, ltx_stream stream);

/* ltx_pipeline_call (cond NULL) or ltx_pipeline_call_cond (cond with a hold mask) under a schedule.  The scalar guidance fields and
 * skip_block_list of `p` are ignored; negative embeddings are required iff some step of the call has g > 1; a block index outside
 * the model is LTX_ERR_ARG.  Every step runs only its own branches; with guidance_batch they are one forward where the step's
 * branches times B fit 8 rows.  A schedule that resolves to the same values on every step, with cfg_star 0 and LTX_RESCALE_CFG, IS
 * the unscheduled call on those values (the same kernels, the same bits). */
int ltx_pipeline_call_sched(ltx_dit* dit, ltx_vae* vae, const ltx_pipeline_params* p, const ltx_guidance_schedule* sched,
                            const ltx_conditioning* cond, float* latents, const float* prompt_embeds, const float* prompt_mask,
                            const float* neg_embeds, const float* neg_mask, const float* decode_noise,
                            int B, int K, float* out_video, ltx_stream stream);

/* ltx_pipeline_call_multiscale with a schedule per pass; either may be NULL: that pass runs on its params' scalars. */
int ltx_pipeline_call_multiscale_sched(ltx_dit* dit, ltx_vae* vae, ltx_upsampler* up,
                                       const ltx_pipeline_params* p_first, const ltx_pipeline_params* p_second,
                                       const ltx_guidance_schedule* sched_first, const ltx_guidance_schedule* sched_second, float adain_factor,
                                       float* latents_lo, const float* noise_hi,
                                       const float* prompt_embeds, const float* prompt_mask, const float* neg_embeds, const float* neg_mask,
                                       const float* decode_noise, int B, int K, float* latents_hi_out, float* out_video, ltx_stream stream);

#ifdef __cplusplus
}
#endif
#endif
