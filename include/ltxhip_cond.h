/* ltxhip_cond.h — image-to-video and clip continuation: latent frames that are GIVEN (the tokens of an encoded image or clip,
 * ltx_vae_encode_tokens) and held while the rest of the video is denoised around them.
 *
 * The reference stops short of this: its transformer takes one timestep per batch row (ltx_transformer.rs:846) and only its
 * scheduler carries a per-token branch (scheduler.rs:511-545) that its trait cannot reach.  The rule is the published
 * first-frame-conditioning rule of the model family, per denoise step i with scheduler timestep t_i:
 *   1. the model sees timestep 0 for the tokens of a held frame and t_i for every other token, in every guidance branch;
 *   2. guidance mix, rescale (statistics over ALL tokens of a batch row) and STG run as without conditioning;
 *   3. the scheduler update moves the tokens that are not held; a held token keeps its value bit for bit.
 * Granularity is the latent frame: tokens are packed frame-major (pack_latents, t2v_pipeline.rs:474-504), so latent frame f of
 * batch row b is the run of height*width tokens starting at token f*height*width.
 * Conventions are those of ltxhip.h (device pointers unless marked HOST, 0 = success, ltx_last_error). */
#ifndef LTXHIP_COND_H
#define LTXHIP_COND_H
#include "ltxhip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ltx_dit_forward with one timestep per (batch row, latent frame):
 *   timestep HOST f32 [B, num_frames];  num_frames, height, width: the latent grid, S == num_frames*height*width in pack order
 *   (also when video_coords is given; otherwise LTX_ERR_ARG).  Every other argument as ltx_dit_forward.
 * A call whose rows each carry one value across their frames IS ltx_dit_forward on those values (the same bits).  Otherwise the
 * time embedding runs once per distinct value of the call and the AdaLN tables hold one row per (batch row, frame); the
 * per-timestep weight copies of norm_fold=2 serve single-timestep calls only and are neither used nor evicted. */
int ltx_dit_forward_frames(ltx_dit* m, const void* hidden, const void* enc, const float* timestep,
                           const float* enc_mask, int B, int S, int K, int num_frames, int height, int width,
                           const float* rope_scale, const float* video_coords, const float* skip_layer_mask,
                           ltx_dtype io_dtype, void* out, ltx_stream stream);

/* ltx_guidance_step / ltx_guidance_step_stochastic (ltxhip.h) that leave held frames alone:
 *   hold  DEVICE u8 [B, num_frames], non-zero = held;  frame_elems = height*width*channels, n == num_frames*frame_elems.
 * The mix and the rescale statistics cover all tokens of a batch row, noise_pred_out (optional) is written for all tokens,
 * latents of held frames are not written; every other token gets the bits of the call without `hold`. */
int ltx_guidance_step_held(const void* text, const void* uncond, const void* perturbed, ltx_dtype pred_dtype,
                           float* latents, float* noise_pred_out, int B, int64_t n,
                           float guidance_scale, float guidance_rescale, float stg_scale, float dt,
                           void* stats_ws, const unsigned char* hold, int num_frames, int64_t frame_elems, ltx_stream stream);
int ltx_guidance_step_stochastic_held(const void* text, const void* uncond, const void* perturbed, ltx_dtype pred_dtype,
                                      float* latents, float* noise_pred_out, int B, int64_t n,
                                      float guidance_scale, float guidance_rescale, float stg_scale,
                                      float sigma, float sigma_next, const float* step_noise,
                                      void* stats_ws, const unsigned char* hold, int num_frames, int64_t frame_elems, ltx_stream stream);

/* latents[b, f] = cond_tokens[b, f] for every held (b, f); everything else - the caller's noise - is untouched.
 *   latents      f32 [B, num_frames*tokens_per_frame, channels], in place
 *   cond_tokens  f32 [B, cond_frames*tokens_per_frame, channels]: ltx_vae_encode_tokens of the image (cond_frames 1) or clip
 *   hold         HOST u8 [B, num_frames]; a held frame f >= cond_frames is LTX_ERR_ARG */
int ltx_cond_apply(float* latents, const float* cond_tokens, int cond_frames, const unsigned char* hold,
                   int B, int num_frames, int tokens_per_frame, int channels, ltx_stream stream);

typedef struct {
    const unsigned char* hold;      /* HOST u8 [B, F'] (F' = (num_frames - 1) / temporal_compression_ratio + 1), 1 = held */
} ltx_conditioning;

/* ltx_pipeline_call with held latent frames (the rule above).  `latents` arrives with the held frames already in place
 * (ltx_cond_apply) and leaves with them unchanged; interrupt, the step hook (it reports t_i), timing, output_latent, the decode-noise
 * mix and the decode are those of ltx_pipeline_call.  cond->hold all zero: ltx_pipeline_call itself, bit for bit.
 * cond or cond->hold NULL: LTX_ERR_ARG. */
int ltx_pipeline_call_cond(ltx_dit* dit, ltx_vae* vae, const ltx_pipeline_params* p, const ltx_conditioning* cond,
                           float* latents, const float* prompt_embeds, const float* prompt_mask,
                           const float* neg_embeds, const float* neg_mask, const float* decode_noise,
                           int B, int K, float* out_video, ltx_stream stream);

#ifdef __cplusplus
}
#endif
#endif
