/* ltxhip_upsampler_st.h — the temporal and spatiotemporal kinds of the latent upsampler (ltxhip_upsampler.h holds the spatial kind,
 * the handle type and every entry that runs a handle).
 *
 * The published LatentUpsampler class ships in three kinds; the network is the one of ltxhip_upsampler.h (same keys, GroupNorm and
 * res blocks), only the `upsampler.0` stage and what follows it differ:
 *   kind             upsampler.0.weight                shuffle of conv output channel o                          then
 *   spatial          [4 mid, mid, 3, 3], per frame     o = c*4 + p2*2 + p3        -> (c, f, 2h+p2, 2w+p3)         -
 *   temporal         [2 mid, mid, 3, 3, 3], Conv3d     o = c*2 + p1               -> (c, 2f+p1, h, w)             drop output frame 0
 *   spatiotemporal   [8 mid, mid, 3, 3, 3], Conv3d     o = c*8 + p1*4 + p2*2 + p3 -> (c, 2f+p1, 2h+p2, 2w+p3)     drop output frame 0
 * (Conv3d: kernel 3, zero padding 1 on T, H and W.)  post_upsample_res_blocks and final_conv run on the shuffled tensor
 * [B, mid, 2F-1, Ho, Wo]; F = 1 gives one output frame.  Latent frames F -> 2F-1 are pixel frames n -> 2n-1 (49 -> 97).  The dims=2
 * form of the published class (every conv a Conv2d) is not supported.  The parity reference is tests/latent_upsampler_st_ref.py.
 *
 * A handle made here is an ltx_upsampler: ltx_upsampler_forward, ltx_latent_upsample_tokens, ltx_upsampler_warmup,
 * ltx_upsampler_destroy and ltx_pipeline_call_multiscale take it; their output is sized by ltx_upsampler_out_shape. */
#ifndef LTXHIP_UPSAMPLER_ST_H
#define LTXHIP_UPSAMPLER_ST_H
#include "ltxhip_upsampler.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int in_channels;             /* latent channels, a multiple of 8 */
    int mid_channels;            /* a multiple of 32 (the GroupNorm groups) */
    int num_blocks_per_stage;    /* 0 .. 16 */
    int spatial_upsample;        /* 0 / 1: H, W -> 2H, 2W */
    int temporal_upsample;       /* 0 / 1: F -> 2F - 1;  both 0: LTX_ERR_ARG */
} ltx_upsampler_st_config;
void ltx_upsampler_st_config_default(ltx_upsampler_st_config* cfg);      /* 128, 512, 4, 1, 0 */

/* As ltx_upsampler_create / ltx_upsampler_create_from_file; with flags (1, 0) they ARE those calls (the same handle, the same bits).
 * Missing and mis-shaped keys are named the same way, upsampler.0.weight against its 5-D shape for the two new kinds. */
int ltx_upsampler_create_st(const ltx_upsampler_st_config* cfg, const ltx_weight* weights, size_t n_weights,
                            ltx_dtype model_dtype, int device, ltx_upsampler** out);
int ltx_upsampler_create_from_file_st(const ltx_upsampler_st_config* cfg, const char* path, ltx_dtype model_dtype, int device, ltx_upsampler** out);
/* of any handle (one of ltx_upsampler_create: flags 1, 0) */
int ltx_upsampler_get_st_config(const ltx_upsampler* up, ltx_upsampler_st_config* out);
/* The latent grid a handle maps (F, H, W) to: Fo = 2F - 1 with the temporal flag, Ho = 2H and Wo = 2W with the spatial one (HOST, no
 * device work). */
int ltx_upsampler_out_shape(const ltx_upsampler* up, int F, int H, int W, int* Fo, int* Ho, int* Wo);

/* Kernel-level entry (beside the ltx_op_* family of ltxhip_ops.h): the shuffle stage alone - a 3x3x3 conv, zero padding, whose
 * epilogue places every value where the depth-to-space puts it.
 *   x    [B, F + 2, H, W, Cin] channels-last of `dtype` (0 = f32, 1 = bf16), guard frames (the first and the last) all zero
 *   w    [O, Cin, 3, 3, 3], bias [O] of `wdtype` (checkpoint channel order: o = c*nsub + sub)
 *   y    [B, Fo + 2, Ho, Wo, O / nsub] of `dtype`: frames 1 .. Fo hold the shuffled result (output frame 0 dropped where st = 2), the
 *        two guard frames are written as zeros; every element of y is written exactly once
 * (st, ss) = the temporal and spatial factor: (2,1) nsub 2, (2,2) nsub 8, (1,2) nsub 4 (with st = 2, Fo = 2F - 1, else F; with
 * ss = 2, Ho = 2H and Wo = 2W).  Anything else, O no multiple of 4 nsub or Cin no multiple of 8: LTX_ERR_ARG.  Blocks until the
 * temporary packed weights are released. */
int ltx_op_conv3d_shuffle(const void* x, const void* w, const void* bias, int wdtype, void* y,
                          int B, int F, int H, int W, int Cin, int O, int st, int ss, int dtype, ltx_stream stream);

/* The stand-alone shuffle pass of the spatial kind as an op - what the conv above folds into its epilogue; for measurements and tests.
 *   x [B, F + 2, H, W, 4C] of `dtype`, channel s*C + c with s = p2*2 + p3 (the load-time order)  ->  y [B, F + 2, 2H, 2W, C]:
 *   channel c of (2h + p2, 2w + p3); the guard frames of y are written as zeros, those of x are not read.
 * C a multiple of the 16-byte chunk (8 bf16 / 4 f32), 16-byte aligned tensors.  Asynchronous on `stream`. */
int ltx_op_pixel_shuffle_guarded(const void* x, void* y, int B, int F, int H, int W, int C, int dtype, ltx_stream stream);

#ifdef __cplusplus
}
#endif
#endif
