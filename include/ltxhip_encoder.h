/* ltxhip_encoder.h — the encode side of AutoencoderKLLtxVideo (reference: src/models/ltx_video/vae.rs)
 *     LtxVideoEncoder3d                     (:1316-1469)   patchify, conv_in, down blocks, mid block, norm_out, conv_out
 *     LtxVideoDownBlock3d / Downsampler3d   (:841-948, :469-582)
 *     DiagonalGaussianDistribution          (:117-145)
 *     encode / encode_z                     (:2070-2099, :2017-2035)
 *     tiled_encode / temporal_tiled_encode  (:2158-2223, :2294-2357)
 * and normalize_latents + pack_latents on its output (t2v_pipeline.rs:552-571, 474-504).
 * Conventions are those of ltxhip.h (device pointers, 0 = success, ltx_last_error, one handle = one device). */
#ifndef LTXHIP_ENCODER_H
#define LTXHIP_ENCODER_H
#include "ltxhip.h"
#include "ltxhip_presets.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ltx_vae_encoder ltx_vae_encoder;

/* downsample_types entries (DownsampleType, vae.rs:469-497) */
enum { LTX_DOWN_CONV = 0, LTX_DOWN_SPATIAL = 1, LTX_DOWN_TEMPORAL = 2, LTX_DOWN_SPATIOTEMPORAL = 3 };

/* Encoder-side fields of AutoencoderKLLtxVideoConfig (vae.rs:32-103); list fields in config.json order. */
typedef struct {
    int in_channels, latent_channels;
    int n_blocks;                        /* len(block_out_channels), 2..5: n_blocks - 1 down blocks + the mid block */
    int block_out_channels[5];
    int layers_per_block[5];             /* entry n_blocks - 1 is the mid block, built with one resnet less (vae.rs:1382-1383) */
    int spatiotemporal_scaling[4];       /* 0: that down block has no downsampler (vae.rs:886-915) */
    int downsample_types[4];             /* LTX_DOWN_*.  LTX_DOWN_CONV - the stride-2 conv followed by a channel-changing `conv_out`
                                          * resnet (vae.rs:888-900, 918-934), used by no preset - is refused with LTX_ERR_UNSUPPORTED */
    int patch_size, patch_size_t;
    int is_causal;                       /* encoder_causal (vae.rs:63); only 1 is implemented, 0 is LTX_ERR_UNSUPPORTED */
    int spatial_compression_ratio, temporal_compression_ratio;   /* the tiled encodes divide by them (vae.rs:2162-2170, 2298-2303) */
} ltx_vae_encoder_config;

/* The encode-side switch ltx_tiling lacks (use_framewise_encoding, vae.rs:1851); ltx_tiling's sample-space fields are shared.
 * NULL = use_framewise_encoding off. */
typedef struct { int use_framewise_encoding; } ltx_encode_tiling;

void ltx_vae_encoder_config_default(ltx_vae_encoder_config* cfg);   /* Default impl, vae.rs:68-103 */
/* the default with the preset's block_out_channels / layers_per_block and the preset VAE's patch sizes / compression ratios */
int ltx_vae_encoder_config_from_preset(const ltx_preset* preset, ltx_vae_encoder_config* cfg);

/* LtxVideoEncoder3d::new (vae.rs:1329-1423).  Weight names are relative to `encoder.` as the constructor reads them
 * ("conv_in.conv.weight", "down_blocks.0.resnets.0.conv1.conv.weight", "down_blocks.0.downsamplers.0.conv.conv.weight",
 * "mid_block.resnets.0...", "conv_out.conv.weight"); names that carry the `encoder.` prefix are accepted too, every other
 * name is ignored (a whole VAE checkpoint can be passed) - except `norm_out.weight`: the reference applies it when present
 * (vae.rs:1388-1394, ones otherwise); no preset checkpoint has it, the engine's norm_out has no weight, and a checkpoint that
 * carries one is refused with LTX_ERR_UNSUPPORTED rather than encoded wrongly. */
int ltx_vae_encoder_create(const ltx_vae_encoder_config* cfg, const ltx_weight* weights, size_t n_weights,
                           ltx_dtype model_dtype, int device, ltx_vae_encoder** out);
void ltx_vae_encoder_destroy(ltx_vae_encoder* e);
int ltx_vae_encoder_get_config(const ltx_vae_encoder* e, ltx_vae_encoder_config* out);

/* AutoencoderKLLtxVideo::encode (vae.rs:2070-2099) -> the posterior's two tensors.
 *   video      [B,in_channels,F,H,W] video_dtype (f32 or bf16), values in [-1, 1]
 *   mean_out   [B,latent_channels,F',H/32,W/32] f32,  F' = (F-1)/8 + 1
 *   logvar_out the same shape or NULL: moment channel `latent_channels`, replicated (vae.rs:1463-1467)
 *   tiling     NULL = one encoder call.  Else encode_z's dispatch (vae.rs:2017-2035): temporal tiles when
 *              enc_tiling->use_framewise_encoding and F > tile_sample_min_num_frames, else spatial tiles when use_tiling and
 *              H > tile_sample_min_height or W > tile_sample_min_width.  Blends run in latent space on f32 tiles.
 * Errors: LTX_ERR_ARG "input not divisible by patch sizes" (vae.rs:1431-1433) for H, W that the patchify and the down blocks
 * cannot halve evenly, or a frame count a temporal downsampler cannot pair ((F - 1) % 8 != 0 for the default config). */
int ltx_vae_encode(ltx_vae_encoder* e, const void* video, ltx_dtype video_dtype, int B, int F, int H, int W,
                   const ltx_tiling* tiling, const ltx_encode_tiling* enc_tiling,
                   float* mean_out, float* logvar_out, ltx_stream stream);

/* DiagonalGaussianDistribution::sample (vae.rs:135-144) with the noise supplied: out = mean + exp(0.5 * logvar) * eps; n f32 each */
int ltx_vae_posterior_sample(const float* mean, const float* logvar, const float* eps, size_t n, float* out, ltx_stream stream);

/* encode -> mode (eps NULL) or sample (eps [B,latent_channels,F',H/32,W/32] f32) -> normalize_latents with `vae`'s
 * latents_mean / latents_std / scaling_factor (t2v_pipeline.rs:552-571) -> pack_latents (:474-504):
 * tokens_out [B, F'*(H/32)*(W/32), latent_channels] f32, the `latents` of ltx_pipeline_call.  The mirror of ltx_vae_decode_tokens. */
int ltx_vae_encode_tokens(ltx_vae_encoder* e, const ltx_vae* vae, const void* video, ltx_dtype video_dtype,
                          int B, int F, int H, int W, const ltx_tiling* tiling, const ltx_encode_tiling* enc_tiling,
                          const float* eps, float* tokens_out, ltx_stream stream);

/* Start-up control like ltx_warmup: one encode of the geometry on scratch buffers, so that plan measurement and workspace
 * sizing happen here.  Blocks until done. */
int ltx_vae_encoder_warmup(ltx_vae_encoder* e, int B, int F, int H, int W, const ltx_tiling* tiling,
                           const ltx_encode_tiling* enc_tiling, ltx_stream stream);

#ifdef __cplusplus
}
#endif
#endif
