//! Raw `extern "C"` bindings to `libltxhip.so` — one declaration per entry point of `include/ltxhip.h` that the
//! candle-video shim (`rust/hip_backend.rs`) uses, plus the checkpoint entry points of `include/ltxhip_weights.h`.
//!
//! Struct layouts are mirrored by hand in three places (the C header, the ctypes classes of
//! `candle-video_amd/ltxhip/__init__.py`, and here).  `tests/cabi_layout.c` prints `sizeof` / `offsetof` of the C
//! definitions; `tests/test_cabi_layout_cpu.py` compares them with the ctypes mirrors AND with the `LAYOUT_*` constants
//! below, which the `const _: () = assert!(..)` items tie to the Rust definitions at compile time.
#![allow(non_camel_case_types)]

use core::ffi::{c_char, c_float, c_int, c_void};
use core::mem::{align_of, size_of};

pub const LTX_F32: c_int = 0;
pub const LTX_BF16: c_int = 1;

/// `ltx_weight` (include/ltxhip.h): a named tensor as found in a safetensors file.
#[repr(C)]
pub struct ltx_weight {
    pub name: *const c_char,
    pub data: *const c_void,
    pub dtype: c_int,
    pub ndim: c_int,
    pub shape: [i64; 5],
    pub on_device: c_int,
}

/// `ltx_dit_config`: LtxVideoTransformer3DModelConfig (ltx_transformer.rs:23-58).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ltx_dit_config {
    pub in_channels: c_int,
    pub out_channels: c_int,
    pub patch_size: c_int,
    pub patch_size_t: c_int,
    pub num_attention_heads: c_int,
    pub attention_head_dim: c_int,
    pub cross_attention_dim: c_int,
    pub num_layers: c_int,
    pub norm_eps: c_float,
    pub caption_channels: c_int,
}

/// `ltx_vae_config`: decoder-side fields of AutoencoderKLLtxVideoConfig (vae.rs:32-103).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ltx_vae_config {
    pub latent_channels: c_int,
    pub out_channels: c_int,
    pub n_blocks: c_int,
    pub decoder_block_out_channels: [c_int; 4],
    pub decoder_layers_per_block: [c_int; 5],
    pub decoder_upsample_factor: [c_int; 4],
    pub patch_size: c_int,
    pub patch_size_t: c_int,
    pub timestep_conditioning: c_int,
    pub decoder_causal: c_int,
    pub scaling_factor: c_float,
    pub spatial_compression_ratio: c_int,
    pub temporal_compression_ratio: c_int,
    /// vae.rs:51 - any non-zero entry is refused (LTX_ERR_UNSUPPORTED); n_blocks + 1 entries, config.json order
    pub decoder_inject_noise: [c_int; 5],
    /// vae.rs:52-53 - tiled-repeat residual of each up-block's upsampler
    pub decoder_upsample_residual: [c_int; 4],
    /// vae.rs:40-41 - 0 = spatial-only up-block, refused (LTX_ERR_UNSUPPORTED)
    pub decoder_spatiotemporal_scaling: [c_int; 4],
    /// vae.rs:46-47 - norm3 only; unused by the decoder
    pub resnet_eps: c_float,
}

/// `ltx_tiling`: tiling parameters of AutoencoderKLLtxVideo (vae.rs:1849-1861).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ltx_tiling {
    pub use_tiling: c_int,
    pub use_framewise_decoding: c_int,
    pub tile_sample_min_height: c_int,
    pub tile_sample_min_width: c_int,
    pub tile_sample_min_num_frames: c_int,
    pub tile_sample_stride_height: c_int,
    pub tile_sample_stride_width: c_int,
    pub tile_sample_stride_num_frames: c_int,
}

/// `ltx_t5_config`: T5EncoderConfig (text_encoder.rs:66-113 / quantized_t5_encoder.rs:20-47); default = t5_xxl().
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ltx_t5_config {
    pub vocab_size: c_int,
    pub d_model: c_int,
    pub d_kv: c_int,
    pub d_ff: c_int,
    pub num_layers: c_int,
    pub num_heads: c_int,
    pub relative_attention_num_buckets: c_int,
    pub relative_attention_max_distance: c_int,
    pub layer_norm_epsilon: c_float,
}

/// `ltx_pipeline_params`: arguments of LtxPipeline::call (t2v_pipeline.rs:627-1073).
#[repr(C)]
pub struct ltx_pipeline_params {
    pub height: c_int,
    pub width: c_int,
    pub num_frames: c_int,
    pub frame_rate: c_int,
    pub num_inference_steps: c_int,
    pub sigmas: *const c_float,
    pub guidance_scale: c_float,
    pub guidance_rescale: c_float,
    pub stg_scale: c_float,
    pub skip_block_list: *const c_int,
    pub n_skip_blocks: c_int,
    pub decode_timestep: c_float,
    pub decode_noise_scale: c_float,
    pub output_latent: c_int,
    pub postprocess: c_int,
    pub tiling: *const ltx_tiling,
    pub shift_terminal: c_float,
    pub use_shift_terminal: c_int,
    pub stochastic_sampling: c_int,
    pub step_noise: *const c_float,
    pub interrupt: *const c_int,
    pub on_step: Option<unsafe extern "C" fn(user: *mut c_void, step: c_int, num_steps: c_int, timestep: i64) -> c_int>,
    pub on_step_user: *mut c_void,
}

// ---- layout guard: (size, align) per struct on LP64, compared with tests/cabi_layout.c by tests/test_cabi_layout_cpu.py ----
pub const LAYOUT_LTX_WEIGHT: (usize, usize) = (72, 8);
pub const LAYOUT_LTX_DIT_CONFIG: (usize, usize) = (40, 4);
pub const LAYOUT_LTX_VAE_CONFIG: (usize, usize) = (148, 4);
pub const LAYOUT_LTX_TILING: (usize, usize) = (32, 4);
pub const LAYOUT_LTX_PIPELINE_PARAMS: (usize, usize) = (136, 8);
pub const LAYOUT_LTX_T5_CONFIG: (usize, usize) = (36, 4);
const _: () = assert!(size_of::<ltx_weight>() == LAYOUT_LTX_WEIGHT.0 && align_of::<ltx_weight>() == LAYOUT_LTX_WEIGHT.1);
const _: () = assert!(size_of::<ltx_dit_config>() == LAYOUT_LTX_DIT_CONFIG.0 && align_of::<ltx_dit_config>() == LAYOUT_LTX_DIT_CONFIG.1);
const _: () = assert!(size_of::<ltx_vae_config>() == LAYOUT_LTX_VAE_CONFIG.0 && align_of::<ltx_vae_config>() == LAYOUT_LTX_VAE_CONFIG.1);
const _: () = assert!(size_of::<ltx_tiling>() == LAYOUT_LTX_TILING.0 && align_of::<ltx_tiling>() == LAYOUT_LTX_TILING.1);
const _: () = assert!(size_of::<ltx_pipeline_params>() == LAYOUT_LTX_PIPELINE_PARAMS.0 && align_of::<ltx_pipeline_params>() == LAYOUT_LTX_PIPELINE_PARAMS.1);

const _: () = assert!(size_of::<ltx_t5_config>() == LAYOUT_LTX_T5_CONFIG.0 && align_of::<ltx_t5_config>() == LAYOUT_LTX_T5_CONFIG.1);

/// opaque handles
pub enum ltx_dit {}
pub enum ltx_vae {}
pub enum ltx_t5 {}
/// hipStream_t; null = default stream
pub type ltx_stream = *mut c_void;

extern "C" {
    pub fn ltx_last_error() -> *const c_char;
    pub fn ltx_dit_config_default(cfg: *mut ltx_dit_config);
    pub fn ltx_vae_config_default(cfg: *mut ltx_vae_config);
    pub fn ltx_tiling_default(t: *mut ltx_tiling);

    // VideoTransformer3D (t2v_pipeline.rs:63-83)
    pub fn ltx_dit_create(cfg: *const ltx_dit_config, weights: *const ltx_weight, n_weights: usize, model_dtype: c_int, device: c_int, out: *mut *mut ltx_dit) -> c_int;
    pub fn ltx_dit_create_from_files(cfg: *const ltx_dit_config, path: *const c_char, unified: c_int, model_dtype: c_int, device: c_int, out: *mut *mut ltx_dit) -> c_int;
    pub fn ltx_dit_destroy(m: *mut ltx_dit);
    pub fn ltx_dit_get_config(m: *const ltx_dit, out: *mut ltx_dit_config) -> c_int;
    pub fn ltx_dit_set_skip_blocks(m: *mut ltx_dit, blocks: *const c_int, n: c_int) -> c_int;
    pub fn ltx_dit_context_cache(m: *mut ltx_dit, enable: c_int) -> c_int;
    pub fn ltx_dit_forward(m: *mut ltx_dit, hidden: *const c_void, enc: *const c_void, timestep: *const c_float, enc_mask: *const c_float,
        b: c_int, s: c_int, k: c_int, num_frames: c_int, height: c_int, width: c_int, rope_scale: *const c_float,
        video_coords: *const c_float, skip_layer_mask: *const c_float, io_dtype: c_int, out: *mut c_void, stream: ltx_stream) -> c_int;

    // VaeLtxVideo (t2v_pipeline.rs:91-103)
    pub fn ltx_vae_create(cfg: *const ltx_vae_config, weights: *const ltx_weight, n_weights: usize, model_dtype: c_int, device: c_int, out: *mut *mut ltx_vae) -> c_int;
    pub fn ltx_vae_config_from_json(json_path: *const c_char, cfg: *mut ltx_vae_config) -> c_int;
    pub fn ltx_vae_create_from_files(cfg: *const ltx_vae_config, path: *const c_char, unified: c_int, model_dtype: c_int, device: c_int, out: *mut *mut ltx_vae) -> c_int;
    pub fn ltx_vae_destroy(v: *mut ltx_vae);
    pub fn ltx_vae_get_config(v: *const ltx_vae, out: *mut ltx_vae_config) -> c_int;
    pub fn ltx_vae_set_noise_seed(v: *mut ltx_vae, seed: u64) -> c_int;
    pub fn ltx_vae_injects_noise(v: *const ltx_vae) -> c_int;
    pub fn ltx_vae_latents_mean(v: *const ltx_vae) -> *const c_float;
    pub fn ltx_vae_latents_std(v: *const ltx_vae) -> *const c_float;
    pub fn ltx_vae_decode(v: *mut ltx_vae, latents: *const c_void, io_dtype: c_int, timestep: *const c_float, b: c_int, f: c_int, h: c_int, w: c_int,
        tiling: *const ltx_tiling, postprocess: c_int, out: *mut c_float, stream: ltx_stream) -> c_int;

    // whole LtxPipeline::call on the device (t2v_pipeline.rs:627-1073)
    pub fn ltx_pipeline_params_default(p: *mut ltx_pipeline_params);
    pub fn ltx_pipeline_last_steps(executed: *mut c_int, requested: *mut c_int) -> c_int;
    pub fn ltx_get_option(key: *const c_char, out: *mut c_char, out_bytes: c_int) -> c_int;
    pub fn ltx_pipeline_call(dit: *mut ltx_dit, vae: *mut ltx_vae, p: *const ltx_pipeline_params, latents: *mut c_float, prompt_embeds: *const c_float,
        prompt_mask: *const c_float, neg_embeds: *const c_float, neg_mask: *const c_float, decode_noise: *const c_float, b: c_int, k: c_int,
        out_video: *mut c_float, stream: ltx_stream) -> c_int;

    // device memory + start-up control
    pub fn ltx_device_alloc(bytes: usize, device: c_int, out: *mut *mut c_void) -> c_int;
    pub fn ltx_device_free(p: *mut c_void) -> c_int;
    pub fn ltx_memcpy_h2d(dst_device: *mut c_void, src_host: *const c_void, bytes: usize, stream: ltx_stream) -> c_int;
    pub fn ltx_memcpy_d2h(dst_host: *mut c_void, src_device: *const c_void, bytes: usize, stream: ltx_stream) -> c_int;
    pub fn ltx_stream_synchronize(stream: ltx_stream) -> c_int;
    pub fn ltx_warmup(dit: *mut ltx_dit, vae: *mut ltx_vae, b: c_int, f: c_int, h: c_int, w: c_int, k: c_int, stream: ltx_stream) -> c_int;
    pub fn ltx_set_autotune(enabled: c_int) -> c_int;
    pub fn ltx_plan_save(path: *const c_char) -> c_int;
    pub fn ltx_plan_load(path: *const c_char) -> c_int;

    // text encoder (include/ltxhip_t5.h): T5TextEncoderWrapper (safetensors, bf16) and QuantizedT5EncoderModel (GGUF, masked)
    pub fn ltx_t5_config_default(c: *mut ltx_t5_config);
    pub fn ltx_t5_create(cfg: *const ltx_t5_config, weights: *const ltx_weight, n_weights: usize, model_dtype: c_int, device: c_int, out: *mut *mut ltx_t5) -> c_int;
    pub fn ltx_t5_create_from_gguf(cfg: *const ltx_t5_config, gguf_path: *const c_char, model_dtype: c_int, device: c_int, out: *mut *mut ltx_t5) -> c_int;
    pub fn ltx_t5_destroy(m: *mut ltx_t5);
    pub fn ltx_t5_forward(m: *mut ltx_t5, input_ids: *const i32, b: c_int, s: c_int, out_dtype: c_int, out: *mut c_void, stream: ltx_stream) -> c_int;
    pub fn ltx_t5_forward_masked(m: *mut ltx_t5, input_ids: *const i32, attention_mask: *const c_float, b: c_int, s: c_int, out_dtype: c_int,
                                 out: *mut c_void, stream: ltx_stream) -> c_int;

    // host-side scalar restatements
    pub fn ltx_pcg32_randn(seed: u64, inc: u64, n: usize, out_host: *mut c_float) -> c_int;
    pub fn ltx_pcg32_u32(seed: u64, inc: u64, n: usize, out_host: *mut u32) -> c_int;
}

// ---- include/ltxhip_encoder.h: the encode side of AutoencoderKLLtxVideo (vae.rs:1316-1469, 2017-2099, 2158-2223, 2294-2357) ----

/// `ltx_vae_encoder_config`: encoder-side fields of AutoencoderKLLtxVideoConfig (vae.rs:32-103).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ltx_vae_encoder_config {
    pub in_channels: c_int,
    pub latent_channels: c_int,
    pub n_blocks: c_int,
    pub block_out_channels: [c_int; 5],
    pub layers_per_block: [c_int; 5],
    pub spatiotemporal_scaling: [c_int; 4],
    /// 0 conv (unsupported), 1 spatial, 2 temporal, 3 spatiotemporal
    pub downsample_types: [c_int; 4],
    pub patch_size: c_int,
    pub patch_size_t: c_int,
    pub is_causal: c_int,
    pub spatial_compression_ratio: c_int,
    pub temporal_compression_ratio: c_int,
}

/// `ltx_encode_tiling`: use_framewise_encoding (vae.rs:1851), the switch `ltx_tiling` lacks.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ltx_encode_tiling {
    pub use_framewise_encoding: c_int,
}

pub const ENCODER_LAYOUT_LTX_VAE_ENCODER_CONFIG: (usize, usize) = (104, 4);
pub const ENCODER_LAYOUT_LTX_ENCODE_TILING: (usize, usize) = (4, 4);
const _: () = assert!(size_of::<ltx_vae_encoder_config>() == ENCODER_LAYOUT_LTX_VAE_ENCODER_CONFIG.0 && align_of::<ltx_vae_encoder_config>() == ENCODER_LAYOUT_LTX_VAE_ENCODER_CONFIG.1);
const _: () = assert!(size_of::<ltx_encode_tiling>() == ENCODER_LAYOUT_LTX_ENCODE_TILING.0 && align_of::<ltx_encode_tiling>() == ENCODER_LAYOUT_LTX_ENCODE_TILING.1);

pub enum ltx_vae_encoder {}

extern "C" {
    pub fn ltx_vae_encoder_config_default(cfg: *mut ltx_vae_encoder_config);
    pub fn ltx_vae_encoder_create(cfg: *const ltx_vae_encoder_config, weights: *const ltx_weight, n_weights: usize, model_dtype: c_int, device: c_int, out: *mut *mut ltx_vae_encoder) -> c_int;
    pub fn ltx_vae_encoder_create_from_files(cfg: *const ltx_vae_encoder_config, path: *const c_char, unified: c_int, model_dtype: c_int, device: c_int, out: *mut *mut ltx_vae_encoder) -> c_int;
    pub fn ltx_vae_encoder_destroy(e: *mut ltx_vae_encoder);
    pub fn ltx_vae_encoder_get_config(e: *const ltx_vae_encoder, out: *mut ltx_vae_encoder_config) -> c_int;
    pub fn ltx_vae_encode(e: *mut ltx_vae_encoder, video: *const c_void, video_dtype: c_int, b: c_int, f: c_int, h: c_int, w: c_int,
                          tiling: *const ltx_tiling, enc_tiling: *const ltx_encode_tiling, mean_out: *mut c_float, logvar_out: *mut c_float, stream: ltx_stream) -> c_int;
    pub fn ltx_vae_posterior_sample(mean: *const c_float, logvar: *const c_float, eps: *const c_float, n: usize, out: *mut c_float, stream: ltx_stream) -> c_int;
    pub fn ltx_vae_encode_tokens(e: *mut ltx_vae_encoder, vae: *const ltx_vae, video: *const c_void, video_dtype: c_int, b: c_int, f: c_int, h: c_int, w: c_int,
                                 tiling: *const ltx_tiling, enc_tiling: *const ltx_encode_tiling, eps: *const c_float, tokens_out: *mut c_float, stream: ltx_stream) -> c_int;
    pub fn ltx_vae_encoder_warmup(e: *mut ltx_vae_encoder, b: c_int, f: c_int, h: c_int, w: c_int, tiling: *const ltx_tiling, enc_tiling: *const ltx_encode_tiling, stream: ltx_stream) -> c_int;
}

// ---- include/ltxhip_cond.h: per-frame timesteps and held conditioning frames (image-to-video, clip continuation) ----

/// `ltx_conditioning`: HOST u8 [B, F'] hold mask, 1 = the latent frame is given and held.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ltx_conditioning {
    pub hold: *const u8,
}

pub const COND_LAYOUT_LTX_CONDITIONING: (usize, usize) = (8, 8);
const _: () = assert!(size_of::<ltx_conditioning>() == COND_LAYOUT_LTX_CONDITIONING.0 && align_of::<ltx_conditioning>() == COND_LAYOUT_LTX_CONDITIONING.1);

extern "C" {
    pub fn ltx_dit_forward_frames(m: *mut ltx_dit, hidden: *const c_void, enc: *const c_void, timestep: *const c_float, enc_mask: *const c_float,
                                  b: c_int, s: c_int, k: c_int, num_frames: c_int, height: c_int, width: c_int, rope_scale: *const c_float,
                                  video_coords: *const c_float, skip_layer_mask: *const c_float, io_dtype: c_int, out: *mut c_void, stream: ltx_stream) -> c_int;
    pub fn ltx_guidance_step_held(text: *const c_void, uncond: *const c_void, perturbed: *const c_void, pred_dtype: c_int, latents: *mut c_float,
                                  noise_pred_out: *mut c_float, b: c_int, n: i64, guidance_scale: c_float, guidance_rescale: c_float, stg_scale: c_float,
                                  dt: c_float, stats_ws: *mut c_void, hold: *const u8, num_frames: c_int, frame_elems: i64, stream: ltx_stream) -> c_int;
    pub fn ltx_guidance_step_stochastic_held(text: *const c_void, uncond: *const c_void, perturbed: *const c_void, pred_dtype: c_int, latents: *mut c_float,
                                             noise_pred_out: *mut c_float, b: c_int, n: i64, guidance_scale: c_float, guidance_rescale: c_float,
                                             stg_scale: c_float, sigma: c_float, sigma_next: c_float, step_noise: *const c_float, stats_ws: *mut c_void,
                                             hold: *const u8, num_frames: c_int, frame_elems: i64, stream: ltx_stream) -> c_int;
    pub fn ltx_cond_apply(latents: *mut c_float, cond_tokens: *const c_float, cond_frames: c_int, hold: *const u8, b: c_int, num_frames: c_int,
                          tokens_per_frame: c_int, channels: c_int, stream: ltx_stream) -> c_int;
    pub fn ltx_pipeline_call_cond(dit: *mut ltx_dit, vae: *mut ltx_vae, p: *const ltx_pipeline_params, cond: *const ltx_conditioning, latents: *mut c_float,
                                  prompt_embeds: *const c_float, prompt_mask: *const c_float, neg_embeds: *const c_float, neg_mask: *const c_float,
                                  decode_noise: *const c_float, b: c_int, k: c_int, out_video: *mut c_float, stream: ltx_stream) -> c_int;
}

// ---- include/ltxhip_lora.h: LoRA adapters merged into the DiT's weights on the device ----

/// Opaque adapter object (`ltx_lora`): A / B pairs for block linears, bound to (dims, model dtype, device).
#[repr(C)]
pub struct ltx_lora {
    _private: [u8; 0],
}

extern "C" {
    pub fn ltx_lora_parse_key(key: *const c_char, module_out: *mut c_char, cap: usize, role: *mut c_int) -> c_int;
    pub fn ltx_lora_create(like: *const ltx_dit, tensors: *const ltx_weight, n: usize, strict: c_int, out: *mut *mut ltx_lora, n_unmatched: *mut c_int) -> c_int;
    pub fn ltx_lora_create_from_file(like: *const ltx_dit, path: *const c_char, strict: c_int, out: *mut *mut ltx_lora, n_unmatched: *mut c_int) -> c_int;
    pub fn ltx_lora_destroy(l: *mut ltx_lora);
    pub fn ltx_dit_set_adapters(m: *mut ltx_dit, loras: *const *const ltx_lora, scales: *const c_float, n: c_int, stream: ltx_stream) -> c_int;
    pub fn ltx_dit_adapter_count(m: *const ltx_dit) -> c_int;
    pub fn ltx_dit_read_linear(m: *const ltx_dit, block: c_int, which: c_int, out_dev: *mut c_void, stream: ltx_stream) -> c_int;
    pub fn ltx_op_lora_merge(w0: *const c_void, out: *mut c_void, n_rows: i64, k: c_int, n: c_int, a: *const *const c_void, b: *const *const c_void,
                             r: *const c_int, coef: *const c_float, dtype: c_int, stream: ltx_stream) -> c_int;
}

// ---- include/ltxhip_upsampler.h: the latent upsampler and the two-pass (multi-scale) pipeline call ----

/// Opaque latent upsampler handle (`ltx_upsampler`).
#[repr(C)]
pub struct ltx_upsampler {
    _private: [u8; 0],
}

/// `ltx_upsampler_config`: widths and block count of the upsampler network.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ltx_upsampler_config {
    pub in_channels: c_int,
    pub mid_channels: c_int,
    pub num_blocks_per_stage: c_int,
}

pub const UPSAMPLER_LAYOUT_LTX_UPSAMPLER_CONFIG: (usize, usize) = (12, 4);
const _: () = assert!(size_of::<ltx_upsampler_config>() == UPSAMPLER_LAYOUT_LTX_UPSAMPLER_CONFIG.0 && align_of::<ltx_upsampler_config>() == UPSAMPLER_LAYOUT_LTX_UPSAMPLER_CONFIG.1);

pub const LTX_GN_SILU: c_int = 1;
pub const LTX_GN_GUARDS: c_int = 2;

extern "C" {
    pub fn ltx_upsampler_config_default(cfg: *mut ltx_upsampler_config);
    pub fn ltx_upsampler_create(cfg: *const ltx_upsampler_config, weights: *const ltx_weight, n_weights: usize, model_dtype: c_int, device: c_int,
                                out: *mut *mut ltx_upsampler) -> c_int;
    pub fn ltx_upsampler_create_from_file(cfg: *const ltx_upsampler_config, path: *const c_char, model_dtype: c_int, device: c_int, out: *mut *mut ltx_upsampler) -> c_int;
    pub fn ltx_upsampler_destroy(up: *mut ltx_upsampler);
    pub fn ltx_upsampler_get_config(up: *const ltx_upsampler, out: *mut ltx_upsampler_config) -> c_int;
    pub fn ltx_upsampler_forward(up: *mut ltx_upsampler, latents: *const c_void, io_dtype: c_int, b: c_int, f: c_int, h: c_int, w: c_int, out: *mut c_void,
                                 stream: ltx_stream) -> c_int;
    pub fn ltx_latent_upsample_tokens(up: *mut ltx_upsampler, vae: *const ltx_vae, tokens_lo: *const c_float, b: c_int, f: c_int, h: c_int, w: c_int,
                                      tokens_hi: *mut c_float, stream: ltx_stream) -> c_int;
    pub fn ltx_latent_adain(tokens: *mut c_float, ref_tokens: *const c_float, b: c_int, s: c_int, s_ref: c_int, c: c_int, factor: c_float, stream: ltx_stream) -> c_int;
    pub fn ltx_latent_renoise(tokens: *mut c_float, noise: *const c_float, sigma: c_float, n: usize, stream: ltx_stream) -> c_int;
    pub fn ltx_pipeline_first_sigma(p: *const ltx_pipeline_params, s: c_int, sigma0: *mut c_float) -> c_int;
    pub fn ltx_upsampler_warmup(up: *mut ltx_upsampler, b: c_int, f: c_int, h: c_int, w: c_int, stream: ltx_stream) -> c_int;
    pub fn ltx_pipeline_call_multiscale(dit: *mut ltx_dit, vae: *mut ltx_vae, up: *mut ltx_upsampler, p_first: *const ltx_pipeline_params,
                                        p_second: *const ltx_pipeline_params, adain_factor: c_float, latents_lo: *mut c_float, noise_hi: *const c_float,
                                        prompt_embeds: *const c_float, prompt_mask: *const c_float, neg_embeds: *const c_float, neg_mask: *const c_float,
                                        decode_noise: *const c_float, b: c_int, k: c_int, latents_hi_out: *mut c_float, out_video: *mut c_float,
                                        stream: ltx_stream) -> c_int;
    pub fn ltx_pipeline_multiscale_last_timing(ms: *mut c_float) -> c_int;
    pub fn ltx_op_groupnorm(x: *const c_void, y: *mut c_void, resid: *const c_void, weight: *const c_void, bias: *const c_void, b: c_int, f: c_int, h: c_int,
                            w: c_int, c: c_int, groups: c_int, eps: c_float, flags: c_int, dtype: c_int, stream: ltx_stream) -> c_int;
}

// ---- include/ltxhip_upsampler_st.h: the temporal and spatiotemporal kinds of the latent upsampler (the same handle type) ----

/// `ltx_upsampler_st_config`: the upsampler network and its kind (both flags 0 is refused; (1, 0) is the spatial kind).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ltx_upsampler_st_config {
    pub in_channels: c_int,
    pub mid_channels: c_int,
    pub num_blocks_per_stage: c_int,
    pub spatial_upsample: c_int,
    pub temporal_upsample: c_int,
}

pub const UPSAMPLER_ST_LAYOUT_LTX_UPSAMPLER_ST_CONFIG: (usize, usize) = (20, 4);
const _: () = assert!(size_of::<ltx_upsampler_st_config>() == UPSAMPLER_ST_LAYOUT_LTX_UPSAMPLER_ST_CONFIG.0 && align_of::<ltx_upsampler_st_config>() == UPSAMPLER_ST_LAYOUT_LTX_UPSAMPLER_ST_CONFIG.1);

extern "C" {
    pub fn ltx_upsampler_st_config_default(cfg: *mut ltx_upsampler_st_config);
    pub fn ltx_upsampler_create_st(cfg: *const ltx_upsampler_st_config, weights: *const ltx_weight, n_weights: usize, model_dtype: c_int, device: c_int,
                                   out: *mut *mut ltx_upsampler) -> c_int;
    pub fn ltx_upsampler_create_from_file_st(cfg: *const ltx_upsampler_st_config, path: *const c_char, model_dtype: c_int, device: c_int,
                                             out: *mut *mut ltx_upsampler) -> c_int;
    pub fn ltx_upsampler_get_st_config(up: *const ltx_upsampler, out: *mut ltx_upsampler_st_config) -> c_int;
    pub fn ltx_upsampler_out_shape(up: *const ltx_upsampler, f: c_int, h: c_int, w: c_int, fo: *mut c_int, ho: *mut c_int, wo: *mut c_int) -> c_int;
    pub fn ltx_op_conv3d_shuffle(x: *const c_void, w: *const c_void, bias: *const c_void, wdtype: c_int, y: *mut c_void, b: c_int, f: c_int, h: c_int,
                                 wd: c_int, cin: c_int, o: c_int, st: c_int, ss: c_int, dtype: c_int, stream: ltx_stream) -> c_int;
    pub fn ltx_op_pixel_shuffle_guarded(x: *const c_void, y: *mut c_void, b: c_int, f: c_int, h: c_int, w: c_int, c: c_int, dtype: c_int, stream: ltx_stream) -> c_int;
}

// ---- include/ltxhip_stg.h: what a skip_layer_mask perturbs (the whole block, or the self-attention inside it) ----

/// `ltx_stg_mode` (a C enum: passed as `c_int`).
pub const LTX_STG_TRANSFORMER_BLOCK: c_int = 0;
pub const LTX_STG_ATTENTION_SKIP: c_int = 1;
pub const LTX_STG_ATTENTION_VALUES: c_int = 2;

extern "C" {
    pub fn ltx_dit_set_stg_mode(m: *mut ltx_dit, mode: c_int) -> c_int;
    pub fn ltx_dit_get_stg_mode(m: *const ltx_dit, out: *mut c_int) -> c_int;
    pub fn ltx_stg_mode_from_name(name: *const c_char, out: *mut c_int) -> c_int;
    pub fn ltx_op_stg_fill(dst: *mut c_void, ldd: c_int, src: *const c_void, lds: c_int, rows: *const u8, b: c_int, s: c_int, d: c_int, dtype: c_int,
                           stream: ltx_stream) -> c_int;
}

// ---- include/ltxhip_guidance.h: per-step guidance schedules, CFG-star and the two rescale forms ----

/// `ltx_rescale_form` (a C enum: passed as `c_int`).
pub const LTX_RESCALE_CFG: c_int = 0;
pub const LTX_RESCALE_MIX: c_int = 1;

/// `ltx_guidance_schedule`: HOST arrays, one value per entry; entry j perturbs `skip_blocks[skip_offsets[j] .. skip_offsets[j + 1])`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ltx_guidance_schedule {
    pub n: c_int,
    pub guidance_scale: *const c_float,
    pub stg_scale: *const c_float,
    pub rescale: *const c_float,
    pub skip_blocks: *const c_int,
    pub skip_offsets: *const c_int,
    pub guidance_timesteps: *const c_float,
    pub cfg_star: c_int,
    pub rescale_form: c_int,
}

pub const GUIDANCE_LAYOUT_LTX_GUIDANCE_SCHEDULE: (usize, usize) = (64, 8);
const _: () = assert!(size_of::<ltx_guidance_schedule>() == GUIDANCE_LAYOUT_LTX_GUIDANCE_SCHEDULE.0 && align_of::<ltx_guidance_schedule>() == GUIDANCE_LAYOUT_LTX_GUIDANCE_SCHEDULE.1);

extern "C" {
    pub fn ltx_guidance_schedule_resolve(sched: *const ltx_guidance_schedule, sigmas: *const c_float, n_steps: c_int, entry_of_step: *mut c_int) -> c_int;
    pub fn ltx_guidance_ws_bytes(b: c_int, n: i64) -> usize;
    pub fn ltx_guidance_step_ex(text: *const c_void, uncond: *const c_void, perturbed: *const c_void, pred_dtype: c_int, latents: *mut c_float,
                                noise_pred_out: *mut c_float, b: c_int, n: i64, guidance_scale: c_float, guidance_rescale: c_float, stg_scale: c_float,
                                cfg_star: c_int, rescale_form: c_int, dt: c_float, sigma: c_float, sigma_next: c_float, step_noise: *const c_float,
                                hold: *const u8, num_frames: c_int, frame_elems: i64, ws: *mut c_void, scalars_out: *mut c_float, stream: ltx_stream) -> c_int;
    pub fn ltx_pipeline_call_sched(dit: *mut ltx_dit, vae: *mut ltx_vae, p: *const ltx_pipeline_params, sched: *const ltx_guidance_schedule,
                                   cond: *const ltx_conditioning, latents: *mut c_float, prompt_embeds: *const c_float, prompt_mask: *const c_float,
                                   neg_embeds: *const c_float, neg_mask: *const c_float, decode_noise: *const c_float, b: c_int, k: c_int,
                                   out_video: *mut c_float, stream: ltx_stream) -> c_int;
    pub fn ltx_pipeline_call_multiscale_sched(dit: *mut ltx_dit, vae: *mut ltx_vae, up: *mut ltx_upsampler, p_first: *const ltx_pipeline_params,
                                              p_second: *const ltx_pipeline_params, sched_first: *const ltx_guidance_schedule,
                                              sched_second: *const ltx_guidance_schedule, adain_factor: c_float, latents_lo: *mut c_float,
                                              noise_hi: *const c_float, prompt_embeds: *const c_float, prompt_mask: *const c_float, neg_embeds: *const c_float,
                                              neg_mask: *const c_float, decode_noise: *const c_float, b: c_int, k: c_int, latents_hi_out: *mut c_float,
                                              out_video: *mut c_float, stream: ltx_stream) -> c_int;
}

// ---- include/ltxhip_keyframes.h: conditioning items at any frame, strengths, noised holds ----

/// `ltx_cond_item`: DEVICE f32 tokens [B, cond_frames*hw, C], the PIXEL frame the item sits at, its strength in [0, 1].
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ltx_cond_item {
    pub tokens: *const c_float,
    pub cond_frames: c_int,
    pub frame_index: c_int,
    pub strength: c_float,
}

/// `ltx_cond_group`: one group of the extended sequence - the item that owns it (-1: none), the item's latent frame, its strength.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ltx_cond_group {
    pub item: c_int,
    pub item_frame: c_int,
    pub strength: c_float,
}

pub const KEYFRAMES_LAYOUT_LTX_COND_ITEM: (usize, usize) = (24, 8);
pub const KEYFRAMES_LAYOUT_LTX_COND_GROUP: (usize, usize) = (12, 4);
const _: () = assert!(size_of::<ltx_cond_item>() == KEYFRAMES_LAYOUT_LTX_COND_ITEM.0 && align_of::<ltx_cond_item>() == KEYFRAMES_LAYOUT_LTX_COND_ITEM.1);
const _: () = assert!(size_of::<ltx_cond_group>() == KEYFRAMES_LAYOUT_LTX_COND_GROUP.0 && align_of::<ltx_cond_group>() == KEYFRAMES_LAYOUT_LTX_COND_GROUP.1);

extern "C" {
    pub fn ltx_cond_layout(items: *const ltx_cond_item, n_items: c_int, height: c_int, width: c_int, num_frames: c_int, frame_rate: c_int,
                           ts_ratio: c_int, sp_ratio: c_int, e: *mut c_int, g: *mut c_int, groups: *mut ltx_cond_group, max_groups: c_int,
                           coords: *mut c_float) -> c_int;
    pub fn ltx_cond_place(latents: *mut c_float, items: *const ltx_cond_item, n_items: c_int, groups: *const ltx_cond_group, g: c_int, b: c_int,
                          tokens_per_group: c_int, channels: c_int, stream: ltx_stream) -> c_int;
    pub fn ltx_cond_noise(latents: *mut c_float, clean: *const c_float, noise: *const c_float, groups: *const ltx_cond_group, g: c_int, b: c_int,
                          tokens_per_group: c_int, channels: c_int, scale: c_float, sigma: c_float, stream: ltx_stream) -> c_int;
    pub fn ltx_cond_step_hold(groups: *const ltx_cond_group, g: c_int, sigma: c_float, timestep: c_float, hold_out: *mut u8,
                              timesteps_out: *mut c_float) -> c_int;
    pub fn ltx_pipeline_call_keyframes(dit: *mut ltx_dit, vae: *mut ltx_vae, p: *const ltx_pipeline_params, sched: *const ltx_guidance_schedule,
                                       items: *const ltx_cond_item, n_items: c_int, image_cond_noise_scale: c_float, cond_noise: *const c_float,
                                       latents: *mut c_float, prompt_embeds: *const c_float, prompt_mask: *const c_float, neg_embeds: *const c_float,
                                       neg_mask: *const c_float, decode_noise: *const c_float, b: c_int, k: c_int, out_video: *mut c_float,
                                       stream: ltx_stream) -> c_int;
}

// ---- include/ltxhip_stepcache.h: timestep-aware step caching (re-use of the block residual on steps that barely moved) ----

/// Opaque step cache handle (`ltx_step_cache`): the previous measurement, the block residuals per cache row, the policy's state.
#[repr(C)]
pub struct ltx_step_cache {
    _private: [u8; 0],
}

/// `ltx_step_cache_params`: reuse while the accumulated poly(distance) stays below `rel_l1_thresh`; `pattern` HOST u8 per step
/// (0 decide, 1 compute, 2 reuse) or null.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct ltx_step_cache_params {
    pub rel_l1_thresh: c_float,
    pub coeff: [c_float; 5],
    pub pattern: *const u8,
    pub n_pattern: c_int,
}

pub const STEPCACHE_LAYOUT_LTX_STEP_CACHE_PARAMS: (usize, usize) = (40, 8);
const _: () = assert!(size_of::<ltx_step_cache_params>() == STEPCACHE_LAYOUT_LTX_STEP_CACHE_PARAMS.0 && align_of::<ltx_step_cache_params>() == STEPCACHE_LAYOUT_LTX_STEP_CACHE_PARAMS.1);

extern "C" {
    pub fn ltx_step_cache_params_default(p: *mut ltx_step_cache_params);
    pub fn ltx_step_cache_create(dit: *mut ltx_dit, rows: c_int, out: *mut *mut ltx_step_cache) -> c_int;
    pub fn ltx_step_cache_destroy(cache: *mut ltx_step_cache);
    pub fn ltx_step_cache_reset(cache: *mut ltx_step_cache) -> c_int;
    pub fn ltx_step_cache_decide(cache: *mut ltx_step_cache, dit: *mut ltx_dit, hidden: *const c_void, timestep: *const c_float, frames: c_int,
                                 b: c_int, s: c_int, num_frames: c_int, height: c_int, width: c_int, io_dtype: c_int, step: c_int, n_steps: c_int,
                                 params: *const ltx_step_cache_params, reuse: *mut c_int, distance: *mut c_float, stream: ltx_stream) -> c_int;
    pub fn ltx_step_cache_require(cache: *mut ltx_step_cache, dit: *const ltx_dit, row0: c_int, nrows: c_int, s: c_int, reuse: *mut c_int) -> c_int;
    pub fn ltx_dit_forward_cached(dit: *mut ltx_dit, cache: *mut ltx_step_cache, row0: c_int, reuse: c_int, frames: c_int, hidden: *const c_void,
                                  enc: *const c_void, timestep: *const c_float, enc_mask: *const c_float, b: c_int, s: c_int, k: c_int,
                                  num_frames: c_int, height: c_int, width: c_int, rope_scale: *const c_float, video_coords: *const c_float,
                                  skip_layer_mask: *const c_float, io_dtype: c_int, out: *mut c_void, stream: ltx_stream) -> c_int;
    pub fn ltx_step_cache_read_residual(cache: *const ltx_step_cache, row: c_int, dst: *mut c_float, stream: ltx_stream) -> c_int;
    pub fn ltx_pipeline_call_cached(dit: *mut ltx_dit, vae: *mut ltx_vae, p: *const ltx_pipeline_params, sched: *const ltx_guidance_schedule,
                                    cond: *const ltx_conditioning, cache_params: *const ltx_step_cache_params, latents: *mut c_float,
                                    prompt_embeds: *const c_float, prompt_mask: *const c_float, neg_embeds: *const c_float, neg_mask: *const c_float,
                                    decode_noise: *const c_float, b: c_int, k: c_int, out_video: *mut c_float, stream: ltx_stream,
                                    reused_out: *mut u8, distance_out: *mut c_float) -> c_int;
    pub fn ltx_op_step_measure_ws_bytes(rows: i64, d: c_int, dtype: c_int) -> usize;
    pub fn ltx_op_step_measure(h: *const c_void, prev: *mut c_void, shift: *const c_float, scale: *const c_float, mod_stride: c_int, rows: i64,
                               d: c_int, rows_per_batch: i64, eps: c_float, dtype: c_int, first: c_int, ws: *mut c_void, sums: *mut f64,
                               stream: ltx_stream) -> c_int;
    pub fn ltx_op_step_residual(h: *const c_void, r: *mut c_void, rows: i64, d: c_int, dtype: c_int, stream: ltx_stream) -> c_int;
}

// ---- include/ltxhip_int8.h: opt-in INT8 (W8A8) block linears on the int8 MFMA ----

/// Mask bits of `ltx_dit_set_int8_linears`: attn1's fused q | k | v, attn1.to_out, ff.net.0.proj, ff.net.2.
pub const LTX_I8_QKV: u8 = 1;
pub const LTX_I8_TO_OUT: u8 = 2;
pub const LTX_I8_FF1: u8 = 4;
pub const LTX_I8_FF2: u8 = 8;
pub const LTX_I8_ALL: u8 = 15;

extern "C" {
    pub fn ltx_dit_set_int8_linears(m: *mut ltx_dit, block_masks: *const u8, mask: u8, stream: ltx_stream) -> c_int;
    pub fn ltx_dit_get_int8_linears(m: *const ltx_dit, block_masks_out: *mut u8) -> c_int;
    pub fn ltx_op_quant_rows_i8(x: *const c_void, rows: i64, d: c_int, ld: c_int, q: *mut c_void, scale: *mut c_float, stream: ltx_stream) -> c_int;
    pub fn ltx_op_rownorm_quant_i8(h: *const c_void, rows: i64, d: c_int, ld: c_int, eps: c_float, shift: *const c_float, scale: *const c_float,
                                   mod_stride: c_int, rows_per_batch: i64, q: *mut c_void, row_scale: *mut c_float, stream: ltx_stream) -> c_int;
    pub fn ltx_op_gemm_i8(a_q: *const c_void, a_scale: *const c_float, w_q: *const c_void, w_scale: *const c_float, bias: *const c_void, y: *mut c_void,
                          m: c_int, n: c_int, k: c_int, epi: c_int, resid: *const c_void, gate: *const c_float, rows_per_batch: c_int, seg_width: c_int,
                          tile: c_int, stream: ltx_stream) -> c_int;
    pub fn ltx_op_gemm_i8_raw(a_q: *const c_void, w_q: *const c_void, acc: *mut c_int, m: c_int, n: c_int, k: c_int, tile: c_int, stream: ltx_stream) -> c_int;
}
