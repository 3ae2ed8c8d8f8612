/* ltxhip_keyframes.h — keyframe conditioning: conditioning items at any frame of the video, with a strength, and the small
 * per-step noise on hard conditioning.  ltxhip_cond.h holds whole latent frames from frame 0 at full strength; this header is the
 * condition pipeline of the model family on top of the same pieces (ltx_dit_forward_frames, the held step kernels).
 *
 * The reference stops short of this, so the rule is restated here.  Notation: latent grid F' x h x w, hw = h*w, C channels;
 * ts_ratio / sp_ratio the VAE's temporal / spatial compression (8 / 32); sig[i], ts[i] the sigmas and truncated timesteps of the
 * call's schedule (the one ltx_pipeline_call builds for the F'*hw grid tokens).
 *
 * ITEMS.  A conditioning item is {tokens, cond_frames Fc, frame_index n, strength s}: tokens DEVICE f32 [B, Fc*hw, C]
 * (ltx_vae_encode_tokens of an image, Fc = 1, or of a clip at the video's height and width), n a PIXEL frame, s in [0, 1].
 * Position and strength are shared by all batch rows.  Items apply in list order; where two meet, the later one owns the group.
 *   1. n == 0:           latent frames 0..Fc-1 go into grid frames 0..Fc-1.  Requires Fc <= F'.
 *   2. n > 0, Fc == 1:   a keyframe - one EXTRA group.  Requires n % ts_ratio == 0 and n < num_frames.
 *   3. n > 0, Fc >= 2:   a clip - latent frames 0 and 1 become two extra groups, latent frames k >= 2 go into grid frame
 *                        n/ts_ratio + k.  Requires n % ts_ratio == 0 and n/ts_ratio + Fc - 1 <= F' - 1.
 * Anything else is LTX_ERR_ARG with a message that names the item and the value.
 * EXTENDED SEQUENCE.  G = E + F' groups of hw tokens: the E extra groups first, in item order, then the grid in pack order;
 * S_ext = G*hw.  The grid tokens of batch row b start at token E*hw of that row.
 * COORDINATES [B, S_ext, 3].  Grid tokens as ltx_build_video_coords gives them.  An extra group made from latent frame k of an item
 * at n has time coordinate (max(ts_ratio*k - (ts_ratio-1), 0) + n) / frame_rate and the spatial coordinates of a grid frame.
 * PLACEMENT.  The caller fills latents [B, S_ext, C] with its noise.  A placed group becomes a + s*(b - a), a the noise and b the
 * item's frame, in f32; s == 1 writes the item's bits (ltx_cond_apply), s == 0 leaves the noise's bits.  The strength sigma_g of a
 * group is s of the last item that wrote it, 0 where no item did; that item alone is placed.
 * STEP i.  The model sees min((float)ts[i], 1000*(1 - sigma_g)) (f32) for the tokens of group g, in every guidance branch.  Mix,
 * rescale statistics and STG run over all S_ext tokens.  Group g is updated iff (double)sig[i] - 1e-6 < 1 - (double)sigma_g;
 * otherwise it keeps its bits.
 * NOISED HOLDS, with scale c > 0 and caller noise cond_noise DEVICE f32 [steps, B, S_ext*C]: before the forwards of step i every
 * group with sigma_g >= 1 - 1e-6 is set to clean_g + c*sig[i]^2*cond_noise[i]_g, clean_g what placement wrote (kept in a side
 * buffer).  Such a group leaves the call with the value of the last executed step (the published behaviour).  c == 0: no launch, no
 * side buffer.
 * AFTER THE LOOP the E*hw extra tokens of each batch row are dropped and the grid tokens are decoded as by ltx_pipeline_call.
 *
 * Not implemented: conditioning items smaller than the frame (token-granular timesteps), keyframes in
 * ltx_pipeline_call_multiscale*, the sharded multi-GPU forms.
 * Conventions are those of ltxhip.h (device pointers unless marked HOST, 0 = success, ltx_last_error). */
#ifndef LTXHIP_KEYFRAMES_H
#define LTXHIP_KEYFRAMES_H
#include "ltxhip.h"
#include "ltxhip_guidance.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    const float* tokens;    /* DEVICE f32 [B, cond_frames*hw, C] (ITEMS); not read by ltx_cond_layout */
    int cond_frames;        /* Fc >= 1 */
    int frame_index;        /* n: the pixel frame the item's first frame sits at */
    float strength;         /* s in [0, 1] */
} ltx_cond_item;

/* one group of the extended sequence: the item that owns it (-1: none), which latent frame of the item, its strength sigma_g */
typedef struct { int item; int item_frame; float strength; } ltx_cond_group;

/* The layout (ITEMS, EXTENDED SEQUENCE, COORDINATES).  Everything HOST in, HOST out; nothing touches a device.
 *   height, width, num_frames, frame_rate: the video's, in pixels and pixel frames (ltx_pipeline_params)
 *   E, G          out: extra groups and all groups
 *   groups        out, optional: [G] entries, capacity max_groups (G <= F' + 2*n_items); G > max_groups is LTX_ERR_ARG
 *   coords        out, optional: f32 [G*hw, 3] of ONE batch row, at least max_groups*hw*3 values (G > max_groups: LTX_ERR_ARG)
 * n_items == 0 is the plain grid (E = 0).  Owns every refusal of the rule. */
int ltx_cond_layout(const ltx_cond_item* items, int n_items, int height, int width, int num_frames, int frame_rate,
                    int ts_ratio, int sp_ratio, int* E, int* G, ltx_cond_group* groups, int max_groups, float* coords);

/* PLACEMENT of the groups table (HOST [G], from ltx_cond_layout) on latents f32 [B, G*tokens_per_group, channels], in place, one
 * launch for the table.  Groups with item -1 or strength 0 keep their bits. */
int ltx_cond_place(float* latents, const ltx_cond_item* items, int n_items, const ltx_cond_group* groups, int G,
                   int B, int tokens_per_group, int channels, ltx_stream stream);

/* NOISED HOLDS of one step: latents_g = clean_g + scale*sigma^2*noise_g for the groups with strength >= 1 - 1e-6; every other group
 * keeps its bits.  latents, clean, noise: f32 [B, G*tokens_per_group, channels]; scale > 0 and sigma = sig[i] of the step.  One
 * launch over the hard-held groups only (none: no launch). */
int ltx_cond_noise(float* latents, const float* clean, const float* noise, const ltx_cond_group* groups, int G,
                   int B, int tokens_per_group, int channels, float scale, float sigma, ltx_stream stream);

/* STEP i, the update predicate, for hosts that run their own loop with ltx_guidance_step_held (ltxhip_cond.h): hold_out HOST u8 [G],
 * 1 = group g keeps its bits on a step of sigma `sigma`.  Replicate the row per batch row for the kernels' [B, G] table.
 * timesteps_out (optional) HOST f32 [G]: what the model sees for group g when the scheduler timestep is `timestep`. */
int ltx_cond_step_hold(const ltx_cond_group* groups, int G, float sigma, float timestep, unsigned char* hold_out, float* timesteps_out);

/* ltx_pipeline_call under the rule above.
 *   dit, vae, p                              as ltx_pipeline_call
 *   sched                                    a guidance schedule or NULL, meaning as in ltx_pipeline_call_sched
 *   items, n_items                           ITEMS; n_items == 0 is ltx_pipeline_call (or _sched) itself, bit for bit
 *   image_cond_noise_scale, cond_noise       NOISED HOLDS: c >= 0 and DEVICE f32 [steps, B, S_ext*C] (required iff c > 0)
 *   latents                                  DEVICE f32 [B, S_ext, C]: the caller's noise on entry (PLACEMENT happens inside the
 *                                            call), the extended latents on exit - with p->output_latent the caller reads the grid
 *                                            tokens of batch row b at element (b*S_ext + E*hw)*C
 *   the rest                                 as ltx_pipeline_call: decode_noise stays [B, C, F', h, w], out_video has the plain
 *                                            call's shape, p->step_noise is [steps, B, S_ext*C], on_step reports ts[i]; interrupt,
 *                                            timing and presets behave as there
 * One item at frame 0 with s == 1 and c == 0 is ltx_pipeline_call_cond on the placed latents, bit for bit. */
int ltx_pipeline_call_keyframes(ltx_dit* dit, ltx_vae* vae, const ltx_pipeline_params* p, const ltx_guidance_schedule* sched,
                                const ltx_cond_item* items, int n_items, float image_cond_noise_scale, const float* cond_noise,
                                float* latents, const float* prompt_embeds, const float* prompt_mask,
                                const float* neg_embeds, const float* neg_mask, const float* decode_noise,
                                int B, int K, float* out_video, ltx_stream stream);

#ifdef __cplusplus
}
#endif
#endif
