/* ltxhip_upsampler.h — the latent upsampler of the LTX-Video checkpoint family and the two-pass (multi-scale) pipeline call.
 *
 * The reference has no upsampler (nothing in src/models/ltx_video mentions it): like ltxhip_cond.h and ltxhip_lora.h this goes one
 * step beyond it.  The published multi-scale recipe is: a first denoise pass at reduced resolution, the LATENT UPSAMPLER (a small
 * Conv3d + GroupNorm network that doubles H and W in latent space), an AdaIN statistics match against the low-resolution latents, a
 * partial re-noise, and a short second pass at full resolution that starts in the middle of a schedule.  The parity reference is the
 * torch restatement tests/latent_upsampler_ref.py.
 *
 * The network (every Conv3d kernel 3, padding 1, ZERO padding on T, H and W; GroupNorm 32 groups, eps 1e-5, affine, biased variance):
 *   x = silu(initial_norm(initial_conv(z)))                         Conv3d in_channels -> mid_channels
 *   res_blocks[0 .. n):  r = x; x = silu(norm1(conv1(x))); x = norm2(conv2(x)); x = silu(x + r)
 *   per frame: x = pixel_shuffle(upsampler.0(x), 2)                 Conv2d mid -> 4 mid, k3 p1; channel c*4 + p1*2 + p2 -> (c, 2h+p1, 2w+p2)
 *   post_upsample_res_blocks[0 .. n): the same block
 *   y = final_conv(x)                                               Conv3d mid -> in_channels;  [B,C,F,H,W] -> [B,C,F,2H,2W]
 * Weight names: initial_conv, initial_norm, res_blocks.{i}.{conv1,norm1,conv2,norm2}, upsampler.0, post_upsample_res_blocks.{i}...,
 * final_conv, each with .weight and .bias.
 *
 * Conventions are those of ltxhip.h (device pointers unless marked HOST, 0 = success, ltx_last_error, one handle = one device). */
#ifndef LTXHIP_UPSAMPLER_H
#define LTXHIP_UPSAMPLER_H
#include "ltxhip.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ltx_upsampler ltx_upsampler;

typedef struct {
    int in_channels;             /* latent channels, a multiple of 8 */
    int mid_channels;            /* a multiple of 32 (the GroupNorm groups) */
    int num_blocks_per_stage;    /* 0 .. 16 */
} ltx_upsampler_config;
void ltx_upsampler_config_default(ltx_upsampler_config* cfg);      /* 128, 512, 4 */

/* Every tensor of the list above must be present with the shape the config implies (conv [O,I,3,3,3], upsampler.0 [4 mid, mid,3,3],
 * norms [mid]); a missing one is LTX_ERR_MISSING_WEIGHT, a mis-shaped one LTX_ERR_ARG, both naming the key.  Other names are ignored. */
int ltx_upsampler_create(const ltx_upsampler_config* cfg, const ltx_weight* weights, size_t n_weights,
                         ltx_dtype model_dtype, int device, ltx_upsampler** out);
/* The same from one safetensors file (the mmap reader of ltxhip_weights.h); F32 and BF16 payloads, anything else under one of the
 * model's keys: LTX_ERR_UNSUPPORTED naming the tensor. */
int ltx_upsampler_create_from_file(const ltx_upsampler_config* cfg, const char* path, ltx_dtype model_dtype, int device, ltx_upsampler** out);
void ltx_upsampler_destroy(ltx_upsampler* up);
int ltx_upsampler_get_config(const ltx_upsampler* up, ltx_upsampler_config* out);

/* latents [B,in_channels,F,H,W] io_dtype -> out [B,in_channels,F,2H,2W] io_dtype (un-normalised latents, as the VAE decodes them).
 * A handle of another kind (ltxhip_upsampler_st.h) writes [B,in_channels,Fo,Ho,Wo], the grid of ltx_upsampler_out_shape; the same holds
 * for ltx_latent_upsample_tokens ([B, Fo*Ho*Wo, C]) and ltx_upsampler_warmup below. */
int ltx_upsampler_forward(ltx_upsampler* up, const void* latents, ltx_dtype io_dtype, int B, int F, int H, int W, void* out, ltx_stream stream);

/* The round trip on the packed tokens the denoise loop carries:
 *   tokens_lo [B, F*H*W, C] f32, normalised  ->  un-pack + de-normalise with `vae`'s latents_mean / latents_std / scaling_factor
 *   (ltx_vae_prepare_latents without the noise mix)  ->  forward  ->  normalise + pack (as ltx_vae_encode_tokens)
 *   ->  tokens_hi [B, F*2H*2W, C] f32.
 * The same bits as ltx_vae_prepare_latents, ltx_upsampler_forward (f32 io) and (z - mean) * scaling_factor / std by hand. */
int ltx_latent_upsample_tokens(ltx_upsampler* up, const ltx_vae* vae, const float* tokens_lo, int B, int F, int H, int W,
                               float* tokens_hi, ltx_stream stream);

/* AdaIN, in place on tokens [B,S,C] f32 against ref_tokens [B,S_ref,C] f32, per (b, c) over all tokens of the channel:
 *   out = (x - mean_x) / std_x * std_ref + mean_ref  (std unbiased, n - 1);   x <- x + factor * (out - x).
 * S < 2 or S_ref < 2: LTX_ERR_ARG.  Deterministic (no atomics; f32 partials merged in a fixed order).  Blocks until the temporary
 * statistics buffer is released. */
int ltx_latent_adain(float* tokens, const float* ref_tokens, int B, int S, int S_ref, int C, float factor, ltx_stream stream);

/* x <- (1 - sigma) * x + sigma * noise on n f32 values: the sigma-mix that starts a denoise loop in the middle of a schedule. */
int ltx_latent_renoise(float* tokens, const float* noise, float sigma, size_t n, ltx_stream stream);

/* The first sigma the denoise loop of ltx_pipeline_call(p) runs at a latent grid of S = F*H*W tokens: ltx_sched_set_timesteps on p's
 * parameters after any shift or terminal stretch (HOST, no device work). */
int ltx_pipeline_first_sigma(const ltx_pipeline_params* p, int S, float* sigma0);

/* Start-up control like ltx_warmup: one forward of the geometry on scratch buffers (conv plan measurement for its shapes, workspace
 * sizing).  Blocks until done. */
int ltx_upsampler_warmup(ltx_upsampler* up, int B, int F, int H, int W, ltx_stream stream);

/* The two-pass call.  By construction the bits of the public pieces called by hand:
 *   ltx_pipeline_call(dit, vae, p_first with output_latent = 1, latents_lo, ...)
 *   ltx_latent_upsample_tokens(up, vae, latents_lo, B, F, H, W, latents_hi_out)
 *   ltx_latent_adain(latents_hi_out, latents_lo, B, 4 S, S, C, adain_factor)
 *   ltx_latent_renoise(latents_hi_out, noise_hi, ltx_pipeline_first_sigma(p_second, 4 S), B * 4 S * C)
 *   ltx_pipeline_call(dit, vae, p_second, latents_hi_out, ..., decode_noise, out_video)
 * p_second->height / width must be exactly twice p_first's and num_frames equal, else LTX_ERR_ARG.  (The rule follows the handle's
 * kind, ltxhip_upsampler_st.h: a temporal or spatiotemporal handle needs p_second->num_frames == 2 * p_first->num_frames - 1, a temporal
 * one equal height and width; noise_hi and latents_hi_out are then [B, Fo*Ho*Wo, C], decode_noise [B, C, Fo, Ho, Wo], and the caller
 * owns p_second->frame_rate.)
 *   latents_lo     [B, S, C] f32, the first pass's start noise; holds the first pass's result afterwards
 *   noise_hi       [B, 4 S, C] f32, the noise of the re-noise step
 *   latents_hi_out [B, 4 S, C] f32, the second pass's latents (its result afterwards)
 *   decode_noise   [B, C, F, 2H, 2W] f32 or NULL;  out_video as ltx_pipeline_call with p_second (ignored when it asks for latents)
 * Interrupt flag, step hook and ltx_pipeline_last_steps / ltx_pipeline_last_timing behave as in two consecutive ltx_pipeline_calls
 * (afterwards they describe the second); ltx_pipeline_multiscale_last_timing gives both. */
int ltx_pipeline_call_multiscale(ltx_dit* dit, ltx_vae* vae, ltx_upsampler* up,
                                 const ltx_pipeline_params* p_first, const ltx_pipeline_params* p_second, float adain_factor,
                                 float* latents_lo, const float* noise_hi,
                                 const float* prompt_embeds, const float* prompt_mask, const float* neg_embeds, const float* neg_mask,
                                 const float* decode_noise, int B, int K, float* latents_hi_out, float* out_video, ltx_stream stream);
/* of the last ltx_pipeline_call_multiscale on this thread: ms[0..3] = ltx_pipeline_last_timing of the first pass, ms[4] = upsample +
 * AdaIN + re-noise (wall time, host side included), ms[5..8] = the second pass */
int ltx_pipeline_multiscale_last_timing(float ms[9]);

/* Kernel-level entry (beside the ltx_op_* family of ltxhip_ops.h): GroupNorm on a channels-last tensor.
 *   x, y, resid: [B, F + 2g, H, W, C] of `dtype` (0 = f32, 1 = bf16), g = 1 with LTX_GN_GUARDS (one guard frame at each end of T),
 *   else 0;  y may alias x;  resid (or NULL) is added after the affine;  weight, bias: [C] of `dtype`.
 *   y = act((x - mean) * rsqrt(var + eps) * weight + bias + resid), statistics per (b, group) over the F non-guard frames, biased
 *   variance, computed from per-slab (n, mean, M2) partials merged with Chan's formula in a fixed order: deterministic, no atomics.
 *   With LTX_GN_GUARDS the guard frames of x are not read and those of y are written as zeros.
 * C a multiple of `groups`; 16-byte loads and stores where C / groups is a multiple of the 16-byte chunk (8 bf16 / 4 f32) and a row
 * has at most 1024 chunks, a plain path otherwise.  Blocks until the temporary partials buffer is released. */
enum { LTX_GN_SILU = 1, LTX_GN_GUARDS = 2 };
int ltx_op_groupnorm(const void* x, void* y, const void* resid, const void* weight, const void* bias,
                     int B, int F, int H, int W, int C, int groups, float eps, int flags, int dtype, ltx_stream stream);

#ifdef __cplusplus
}
#endif
#endif
