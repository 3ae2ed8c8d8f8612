"""Host-side mirror of candle-video's LTX pipeline interface over libltxhip.so (C ABI).

Classes and argument meaning follow the reference (FerrisMind/candle-video,
src/models/ltx_video/):

    LtxVideoTransformer3DModel.forward      ltx_transformer.rs:1029-1172 / trait t2v_pipeline.rs:63-83
    AutoencoderKLLtxVideo.decode            vae.rs:2101-2136 / trait t2v_pipeline.rs:91-103
    FlowMatchEulerDiscreteScheduler         scheduler.rs:646-668 (Scheduler trait)
    LtxPipeline.call                        t2v_pipeline.rs:627-1073

torch is used ONLY as the device-memory / stream provider (tensors in, tensors
out); every computation happens in the HIP library.  There is no CPU fallback:
importing this module without the built library raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# LTXHIP_LIB: a variant build of the SAME library (tools/variants/libltxhip_*.so, the A/B tooling); never a fallback
_LIB_PATH = os.environ.get("LTXHIP_LIB") or os.path.join(os.path.dirname(_HERE), "libltxhip.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"ltxhip: {_LIB_PATH} is missing — build it with `make -C candle-video_amd` "
        "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
lib = C.CDLL(_LIB_PATH)

LTX_F32, LTX_BF16 = 0, 1


class LtxError(RuntimeError):
    pass


lib.ltx_last_error.restype = C.c_char_p


def _check(rc: int):
    if rc != 0:
        raise LtxError(f"[ltxhip rc={rc}] {lib.ltx_last_error().decode()}")


class _Weight(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("dtype", C.c_int), ("ndim", C.c_int),
                ("shape", C.c_int64 * 5), ("on_device", C.c_int)]


class DitConfigC(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("in_channels", "out_channels", "patch_size", "patch_size_t",
                                       "num_attention_heads", "attention_head_dim", "cross_attention_dim", "num_layers")] + \
               [("norm_eps", C.c_float), ("caption_channels", C.c_int)]


class VaeConfigC(C.Structure):
    _fields_ = [("latent_channels", C.c_int), ("out_channels", C.c_int), ("n_blocks", C.c_int),
                ("decoder_block_out_channels", C.c_int * 4), ("decoder_layers_per_block", C.c_int * 5),
                ("decoder_upsample_factor", C.c_int * 4), ("patch_size", C.c_int), ("patch_size_t", C.c_int),
                ("timestep_conditioning", C.c_int), ("decoder_causal", C.c_int), ("scaling_factor", C.c_float),
                ("spatial_compression_ratio", C.c_int), ("temporal_compression_ratio", C.c_int),
                ("decoder_inject_noise", C.c_int * 5), ("decoder_upsample_residual", C.c_int * 4),
                ("decoder_spatiotemporal_scaling", C.c_int * 4), ("resnet_eps", C.c_float)]


class TilingC(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("use_tiling", "use_framewise_decoding", "tile_sample_min_height", "tile_sample_min_width",
                                       "tile_sample_min_num_frames", "tile_sample_stride_height", "tile_sample_stride_width",
                                       "tile_sample_stride_num_frames")]


class PipelineParamsC(C.Structure):
    _fields_ = [("height", C.c_int), ("width", C.c_int), ("num_frames", C.c_int), ("frame_rate", C.c_int),
                ("num_inference_steps", C.c_int), ("sigmas", C.POINTER(C.c_float)),
                ("guidance_scale", C.c_float), ("guidance_rescale", C.c_float), ("stg_scale", C.c_float),
                ("skip_block_list", C.POINTER(C.c_int)), ("n_skip_blocks", C.c_int),
                ("decode_timestep", C.c_float), ("decode_noise_scale", C.c_float),
                ("output_latent", C.c_int), ("postprocess", C.c_int), ("tiling", C.POINTER(TilingC)),
                ("shift_terminal", C.c_float), ("use_shift_terminal", C.c_int),
                ("stochastic_sampling", C.c_int), ("step_noise", C.POINTER(C.c_float)),
                ("interrupt", C.POINTER(C.c_int)), ("on_step", C.c_void_p), ("on_step_user", C.c_void_p)]


StepFn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int64)     # ltx_step_fn


_vp, _i, _i64, _f, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t
_fp = C.POINTER(C.c_float)
_SIGS = {
    "ltx_dit_config_default": [_vp], "ltx_vae_config_default": [_vp], "ltx_tiling_default": [_vp],
    "ltx_dit_create": [_vp, _vp, _sz, _i, _i, _vp], "ltx_dit_destroy": [_vp],
    "ltx_dit_set_skip_blocks": [_vp, _vp, _i], "ltx_dit_context_cache": [_vp, _i], "ltx_dit_get_config": [_vp, _vp],
    "ltx_dit_forward": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp],
    "ltx_vae_create": [_vp, _vp, _sz, _i, _i, _vp], "ltx_vae_destroy": [_vp], "ltx_vae_get_config": [_vp, _vp],
    "ltx_vae_set_noise_seed": [_vp, C.c_uint64], "ltx_vae_injects_noise": [_vp],
    "ltx_vae_latents_mean": [_vp], "ltx_vae_latents_std": [_vp],
    "ltx_vae_decode": [_vp, _vp, _i, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp],
    "ltx_vae_decode_tokens": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp],
    "ltx_vae_prepare_latents": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp],
    "ltx_guidance_step": [_vp, _vp, _vp, _i, _vp, _vp, _i, _i64, _f, _f, _f, _f, _vp, _vp],
    "ltx_guidance_step_stochastic": [_vp, _vp, _vp, _i, _vp, _vp, _i, _i64, _f, _f, _f, _f, _f, _vp, _vp, _vp],
    "ltx_sched_set_timesteps": [_vp, _i, _f, _i, _f, _f, _i, _vp, _vp],
    "ltx_sched_set_timesteps_ex": [_vp, _i, _f, _i, _f, _f, _i, _i, _i, _vp, _vp],
    "ltx_calculate_shift": [_i, _i, _i, _f, _f],
    "ltx_pcg32_randn": [C.c_uint64, C.c_uint64, _sz, _vp],
    "ltx_pcg32_u32": [C.c_uint64, C.c_uint64, _sz, _vp],
    "ltx_device_alloc": [_sz, _i, _vp], "ltx_device_free": [_vp], "ltx_memcpy_h2d": [_vp, _vp, _sz, _vp], "ltx_memcpy_d2h": [_vp, _vp, _sz, _vp],
    "ltx_stream_synchronize": [_vp],
    "ltx_warmup": [_vp, _vp, _i, _i, _i, _i, _i, _vp], "ltx_set_autotune": [_i], "ltx_plan_save": [C.c_char_p], "ltx_plan_load": [C.c_char_p],
    "ltx_pipeline_last_steps": [C.POINTER(C.c_int), C.POINTER(C.c_int)], "ltx_attention_fallback_counts": [C.POINTER(C.c_ulonglong), C.c_int], "ltx_set_option": [C.c_char_p, C.c_char_p], "ltx_get_option": [C.c_char_p, C.c_char_p, C.c_int], "ltx_reset_options": [], "ltx_has_experiments": [],
    "ltx_build_video_coords": [_i, _i, _i, _i, _i, _i, _vp],
    "ltx_pipeline_params_default": [_vp],
    "ltx_pipeline_call": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp],
    "ltx_pipeline_last_timing": [_vp],
    "ltx_prof_enable": [_i], "ltx_prof_report": [_i, _vp, _vp, _vp], "ltx_prof_report_kernel": [_i, _i, _vp, _vp, _vp],
    "ltx_op_linear": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp],
    "ltx_op_linear_segmented": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "ltx_op_ring_packed_bytes": [_i, _i], "ltx_op_ring_pack": [_vp, _i, _i, _vp, _vp],
    "ltx_op_linear_packed": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp],
    "ltx_op_rownorm_presum": [_vp, _vp, _i64, _i, _f, _vp, _vp, _vp, _i64, _i, _i, _vp, _i, _i, _vp],
    "ltx_op_linear_rowsq": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp], "ltx_op_rowsq": [_vp, _i64, _i, _i, _vp, _i, _vp],
    "ltx_op_linear_fold_out": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp],
    "ltx_op_linear_fold_in": [_vp, _vp, _vp, _vp, _i, _i, _f, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "ltx_op_linear_fold_ok": [_i, _i, _i, _i, _i, _i, _i, _i],
    "ltx_op_shift_gemv": [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _vp],
    "ltx_op_mod_scale": [_vp, _vp, _i, _vp, _i, _i64, _i, _i, _vp], "ltx_op_scale_cols": [_vp, _vp, _vp, _i64, _i, _i, _vp],
    "ltx_op_linear_split_factor": [_i, _i, _i], "ltx_op_linear_deferred": [_vp, _vp, _vp, _i, _i, _i, _vp],
    "ltx_op_rownorm_deferred": [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _i64, _i, _i, _f, _vp, _vp, _i64, _i, _i, _vp],
    "ltx_op_attention_compact": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _vp, _vp, _i, _i, _f, _vp, _vp],
    "ltx_op_attention_rowsq": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _vp, _vp, _i, _i, _f, _vp],
    "ltx_op_rownorm": [_vp, _vp, _i64, _i, _i, _f, _vp, _vp, _vp, _i64, _i, _i, _i, _vp],
    "ltx_op_qknorm_rope": [_vp, _i64, _i, _i, _vp, _f, _vp, _vp, _i, _vp],
    "ltx_op_qknorm_rope_segs": [_vp, _i64, _i, _i, _i, _i64, _vp, _vp, _vp, _f, _vp, _vp, _f, _i, _vp],
    "ltx_op_xattn_fold_route": [_i, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_int)], "ltx_op_xattn_fold_kp": [C.POINTER(C.c_int), _i, C.POINTER(C.c_int)],
    "ltx_op_xattn_fold_build": [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp],
    "ltx_op_attention_probs": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _vp, _i, _f, _vp, _vp],
    "ltx_op_norm_route": [_i64, _i, _i, _i, _i, _i, _i64, _i, _i, C.c_char_p, _i], "ltx_op_qknorm_route": [_i64, _i, _i, C.c_char_p, _i],
    "ltx_op_rope_table": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp],
    "ltx_op_timestep_embedding": [_vp, _i, _i, _f, _i, _vp, _vp],
    "ltx_op_attention": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _vp, _i, _vp],
    "ltx_op_attention_prescaled": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "ltx_op_conv3d": [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "ltx_op_conv3d_norm": [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _f, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "ltx_op_upsample3d": [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "ltx_op_conv_out_unpatchify": [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "ltx_op_blend": [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "ltx_op_downsample3d": [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "ltx_op_gemm_plan": [_i, _i, _i, _i, _i, _i, _i, _i, C.c_char_p, _i],
    "ltx_op_gemm_route": [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, C.c_char_p, _i],
    "ltx_op_dit_plan": [_i, _i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_int64)],
    # include/ltxhip_t5.h
    "ltx_t5_config_default": [_vp], "ltx_t5_create": [_vp, _vp, _sz, _i, _i, _vp], "ltx_t5_destroy": [_vp],
    "ltx_t5_forward": [_vp, _vp, _i, _i, _i, _vp, _vp],
    "ltx_t5_create_from_gguf": [_vp, C.c_char_p, _i, _i, _vp], "ltx_t5_forward_masked": [_vp, _vp, _vp, _i, _i, _i, _vp, _vp],
    "ltx_gguf_open": [C.c_char_p, _vp], "ltx_gguf_close": [_vp], "ltx_gguf_count": [_vp], "ltx_gguf_find": [_vp, C.c_char_p],
    "ltx_gguf_tensor": [_vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp], "ltx_gguf_type_info": [_i, _vp, _vp],
    "ltx_gguf_dequantize": [_i, _vp, _i, _i64, _i, _vp, _vp],
    # include/ltxhip_frames.h
    "ltx_video_to_rgb8": [_vp, _i, _i, _i, _i, _vp, _vp], "ltx_write_png": [C.c_char_p, _vp, _i, _i],
    "ltx_save_frames_png": [_vp, _i, _i, _i, _i, C.c_char_p, _vp, _vp],
    "ltx_write_gif": [C.c_char_p, _vp, _i, _i, _i, _i, _i], "ltx_save_video_gif": [_vp, _i, _i, _i, _i, C.c_char_p, _vp],
    # include/ltxhip_presets.h
    "ltx_preset_count": [], "ltx_preset_name": [_i], "ltx_preset_get": [C.c_char_p, _vp], "ltx_pipeline_params_from_preset": [_vp, _vp],
    # include/ltxhip_weights.h
    "ltx_weights_detect_format": [C.c_char_p], "ltx_weights_remap_key": [C.c_char_p, C.c_char_p, _sz],
    "ltx_weights_is_transformer_key": [C.c_char_p], "ltx_weights_is_vae_key": [C.c_char_p],
    "ltx_name_mapper_create": [], "ltx_name_mapper_destroy": [_vp], "ltx_name_mapper_add": [_vp, _i, C.c_char_p, C.c_char_p],
    "ltx_name_mapper_has_mapping": [_vp, C.c_char_p], "ltx_name_mapper_map": [_vp, C.c_char_p, C.c_char_p, _sz],
    "ltx_weights_validate_names": [_vp, _sz, _vp, _sz, _vp, _vp],
    "ltx_safetensors_open": [C.c_char_p, _vp], "ltx_safetensors_close": [_vp], "ltx_safetensors_count": [_vp],
    "ltx_safetensors_tensor": [_vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp],
    "ltx_weights_resolve": [C.c_char_p, C.c_char_p, _sz, _vp],
    "ltx_dit_create_from_files": [_vp, C.c_char_p, _i, _i, _i, _vp], "ltx_vae_create_from_files": [_vp, C.c_char_p, _i, _i, _i, _vp],
    "ltx_vae_config_from_json": [C.c_char_p, _vp], "ltx_vae_encoder_create_from_files": [_vp, C.c_char_p, _i, _i, _i, _vp],
    # ltxhip_team.h: RCCL behind the C ABI (dlopen'ed on first use)
    "ltx_team_unique_id": [_vp], "ltx_team_create": [_vp, _i, _i, _i, _vp], "ltx_team_destroy": [_vp], "ltx_team_size": [_vp], "ltx_team_rank": [_vp],
    "ltx_team_allgather_f32": [_vp, _vp, _vp, _sz, _vp], "ltx_team_exchange_f32": [_vp, _vp, _sz, _i, _vp, _sz, _i, _vp],
}
EXPORTED_SYMBOLS = sorted(list(_SIGS) + ["ltx_last_error"])
for _name, _sig in _SIGS.items():
    _fn = getattr(lib, _name)          # raises AttributeError if the library lacks a declared symbol
    _fn.argtypes = _sig
    if _name not in ("ltx_calculate_shift", "ltx_vae_latents_mean", "ltx_vae_latents_std", "ltx_name_mapper_create",
                     "ltx_name_mapper_destroy", "ltx_safetensors_close", "ltx_safetensors_count", "ltx_team_destroy"):
        _fn.restype = C.c_int
lib.ltx_calculate_shift.restype = C.c_float
lib.ltx_op_ring_packed_bytes.restype = C.c_int64
lib.ltx_vae_latents_mean.restype = C.c_void_p
lib.ltx_vae_latents_std.restype = C.c_void_p
lib.ltx_name_mapper_create.restype = C.c_void_p
lib.ltx_name_mapper_destroy.restype = None
lib.ltx_safetensors_close.restype = None
lib.ltx_safetensors_count.restype = C.c_size_t
lib.ltx_gguf_close.restype = None
lib.ltx_gguf_count.restype = C.c_size_t


class VaeEncoderConfigC(C.Structure):            # ltx_vae_encoder_config (include/ltxhip_encoder.h)
    _fields_ = [("in_channels", C.c_int), ("latent_channels", C.c_int), ("n_blocks", C.c_int),
                ("block_out_channels", C.c_int * 5), ("layers_per_block", C.c_int * 5),
                ("spatiotemporal_scaling", C.c_int * 4), ("downsample_types", C.c_int * 4),
                ("patch_size", C.c_int), ("patch_size_t", C.c_int), ("is_causal", C.c_int),
                ("spatial_compression_ratio", C.c_int), ("temporal_compression_ratio", C.c_int)]


class EncodeTilingC(C.Structure):                # ltx_encode_tiling
    _fields_ = [("use_framewise_encoding", C.c_int)]


# include/ltxhip_encoder.h (kept apart from _SIGS: EXPORTED_SYMBOLS lists the headers that existed before it)
_ENC_SIGS = {
    "ltx_vae_encoder_config_default": [_vp], "ltx_vae_encoder_config_from_preset": [_vp, _vp],
    "ltx_vae_encoder_create": [_vp, _vp, _sz, _i, _i, _vp], "ltx_vae_encoder_destroy": [_vp], "ltx_vae_encoder_get_config": [_vp, _vp],
    "ltx_vae_encode": [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp],
    "ltx_vae_posterior_sample": [_vp, _vp, _vp, _sz, _vp, _vp],
    "ltx_vae_encode_tokens": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp],
    "ltx_vae_encoder_warmup": [_vp, _i, _i, _i, _i, _vp, _vp, _vp],
}
ENCODER_SYMBOLS = sorted(_ENC_SIGS)
for _name, _sig in _ENC_SIGS.items():
    _fn = getattr(lib, _name)
    _fn.argtypes = _sig
    _fn.restype = None if _name in ("ltx_vae_encoder_config_default", "ltx_vae_encoder_destroy") else C.c_int


class ConditioningC(C.Structure):                # ltx_conditioning (include/ltxhip_cond.h)
    _fields_ = [("hold", C.POINTER(C.c_ubyte))]


# include/ltxhip_cond.h (kept apart like the encoder's: EXPORTED_SYMBOLS lists the headers that existed before both)
_COND_SIGS = {
    "ltx_dit_forward_frames": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp],
    "ltx_guidance_step_held": [_vp, _vp, _vp, _i, _vp, _vp, _i, _i64, _f, _f, _f, _f, _vp, _vp, _i, _i64, _vp],
    "ltx_guidance_step_stochastic_held": [_vp, _vp, _vp, _i, _vp, _vp, _i, _i64, _f, _f, _f, _f, _f, _vp, _vp, _vp, _i, _i64, _vp],
    "ltx_cond_apply": [_vp, _vp, _i, _vp, _i, _i, _i, _i, _vp],
    "ltx_pipeline_call_cond": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp],
}
COND_SYMBOLS = sorted(_COND_SIGS)
for _name, _sig in _COND_SIGS.items():
    _fn = getattr(lib, _name)
    _fn.argtypes = _sig
    _fn.restype = C.c_int


# include/ltxhip_lora.h (kept apart like the two above)
_LORA_SIGS = {
    "ltx_lora_parse_key": [C.c_char_p, C.c_char_p, _sz, C.POINTER(C.c_int)],
    "ltx_lora_create": [_vp, _vp, _sz, _i, _vp, _vp], "ltx_lora_create_from_file": [_vp, C.c_char_p, _i, _vp, _vp], "ltx_lora_destroy": [_vp],
    "ltx_dit_set_adapters": [_vp, _vp, _vp, _i, _vp], "ltx_dit_adapter_count": [_vp], "ltx_dit_read_linear": [_vp, _i, _i, _vp, _vp],
    "ltx_op_lora_merge": [_vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _i, _vp],
}
LORA_SYMBOLS = sorted(_LORA_SIGS)
for _name, _sig in _LORA_SIGS.items():
    _fn = getattr(lib, _name)
    _fn.argtypes = _sig
    _fn.restype = None if _name == "ltx_lora_destroy" else C.c_int
class UpsamplerConfigC(C.Structure):             # ltx_upsampler_config (include/ltxhip_upsampler.h)
    _fields_ = [("in_channels", C.c_int), ("mid_channels", C.c_int), ("num_blocks_per_stage", C.c_int)]


# include/ltxhip_upsampler.h (kept apart like the three above)
_UP_SIGS = {
    "ltx_upsampler_config_default": [_vp], "ltx_upsampler_create": [_vp, _vp, _sz, _i, _i, _vp],
    "ltx_upsampler_create_from_file": [_vp, C.c_char_p, _i, _i, _vp], "ltx_upsampler_destroy": [_vp], "ltx_upsampler_get_config": [_vp, _vp],
    "ltx_upsampler_forward": [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp],
    "ltx_latent_upsample_tokens": [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp],
    "ltx_latent_adain": [_vp, _vp, _i, _i, _i, _i, _f, _vp], "ltx_latent_renoise": [_vp, _vp, _f, _sz, _vp],
    "ltx_pipeline_first_sigma": [_vp, _i, _vp], "ltx_upsampler_warmup": [_vp, _i, _i, _i, _i, _vp],
    "ltx_pipeline_call_multiscale": [_vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp],
    "ltx_pipeline_multiscale_last_timing": [_vp],
    "ltx_op_groupnorm": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _i, _i, _vp],
}
UPSAMPLER_SYMBOLS = sorted(_UP_SIGS)
for _name, _sig in _UP_SIGS.items():
    _fn = getattr(lib, _name)
    _fn.argtypes = _sig
    _fn.restype = None if _name in ("ltx_upsampler_config_default", "ltx_upsampler_destroy") else C.c_int
LTX_GN_SILU, LTX_GN_GUARDS = 1, 2


class UpsamplerStConfigC(C.Structure):           # ltx_upsampler_st_config (include/ltxhip_upsampler_st.h)
    _fields_ = [("in_channels", C.c_int), ("mid_channels", C.c_int), ("num_blocks_per_stage", C.c_int),
                ("spatial_upsample", C.c_int), ("temporal_upsample", C.c_int)]


# include/ltxhip_upsampler_st.h (kept apart like the four above)
_UP_ST_SIGS = {
    "ltx_upsampler_st_config_default": [_vp], "ltx_upsampler_create_st": [_vp, _vp, _sz, _i, _i, _vp],
    "ltx_upsampler_create_from_file_st": [_vp, C.c_char_p, _i, _i, _vp], "ltx_upsampler_get_st_config": [_vp, _vp],
    "ltx_upsampler_out_shape": [_vp, _i, _i, _i, _vp, _vp, _vp],
    "ltx_op_conv3d_shuffle": [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "ltx_op_pixel_shuffle_guarded": [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
}
UPSAMPLER_ST_SYMBOLS = sorted(_UP_ST_SIGS)
for _name, _sig in _UP_ST_SIGS.items():
    _fn = getattr(lib, _name)
    _fn.argtypes = _sig
    _fn.restype = None if _name == "ltx_upsampler_st_config_default" else C.c_int


# include/ltxhip_stg.h (kept apart like the five above)
_STG_SIGS = {
    "ltx_dit_set_stg_mode": [_vp, _i], "ltx_dit_get_stg_mode": [_vp, C.POINTER(C.c_int)],
    "ltx_stg_mode_from_name": [C.c_char_p, C.POINTER(C.c_int)],
    "ltx_op_stg_fill": [_vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp],
}
STG_SYMBOLS = sorted(_STG_SIGS)
for _name, _sig in _STG_SIGS.items():
    _fn = getattr(lib, _name)
    _fn.argtypes = _sig
    _fn.restype = C.c_int
LTX_STG_TRANSFORMER_BLOCK, LTX_STG_ATTENTION_SKIP, LTX_STG_ATTENTION_VALUES = 0, 1, 2
STG_MODES = ("transformer_block", "attention_skip", "attention_values")      # ltx_stg_mode, by value


def stg_mode_from_name(name: str) -> int:
    """ltx_stg_mode of a published config's `stg_mode` string (host only; 'residual' and unknown names raise)"""
    out = C.c_int(0)
    _check(lib.ltx_stg_mode_from_name(name.encode() if name is not None else None, C.byref(out)))
    return out.value


class GuidanceScheduleC(C.Structure):            # ltx_guidance_schedule (include/ltxhip_guidance.h)
    _fields_ = [("n", C.c_int), ("guidance_scale", C.POINTER(C.c_float)), ("stg_scale", C.POINTER(C.c_float)), ("rescale", C.POINTER(C.c_float)),
                ("skip_blocks", C.POINTER(C.c_int)), ("skip_offsets", C.POINTER(C.c_int)), ("guidance_timesteps", C.POINTER(C.c_float)),
                ("cfg_star", C.c_int), ("rescale_form", C.c_int)]


# include/ltxhip_guidance.h (kept apart like the six above)
_GUIDANCE_SIGS = {
    "ltx_guidance_schedule_resolve": [_vp, _vp, _i, _vp],
    "ltx_guidance_ws_bytes": [_i, _i64],
    "ltx_guidance_step_ex": [_vp, _vp, _vp, _i, _vp, _vp, _i, _i64, _f, _f, _f, _i, _i, _f, _f, _f, _vp, _vp, _i, _i64, _vp, _vp, _vp],
    "ltx_pipeline_call_sched": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp],
    "ltx_pipeline_call_multiscale_sched": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp],
}
GUIDANCE_SYMBOLS = sorted(_GUIDANCE_SIGS)
for _name, _sig in _GUIDANCE_SIGS.items():
    _fn = getattr(lib, _name)
    _fn.argtypes = _sig
    _fn.restype = C.c_size_t if _name == "ltx_guidance_ws_bytes" else C.c_int
LTX_RESCALE_CFG, LTX_RESCALE_MIX = 0, 1
RESCALE_FORMS = ("cfg", "mix")                   # ltx_rescale_form, by value


class CondItemC(C.Structure):                    # ltx_cond_item (include/ltxhip_keyframes.h)
    _fields_ = [("tokens", C.POINTER(C.c_float)), ("cond_frames", C.c_int), ("frame_index", C.c_int), ("strength", C.c_float)]


class CondGroupC(C.Structure):                   # ltx_cond_group
    _fields_ = [("item", C.c_int), ("item_frame", C.c_int), ("strength", C.c_float)]


# include/ltxhip_keyframes.h (kept apart like the seven above)
_KEYFRAME_SIGS = {
    "ltx_cond_layout": [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp],
    "ltx_cond_place": [_vp, _vp, _i, _vp, _i, _i, _i, _i, _vp],
    "ltx_cond_noise": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _vp],
    "ltx_cond_step_hold": [_vp, _i, _f, _f, _vp, _vp],
    "ltx_pipeline_call_keyframes": [_vp, _vp, _vp, _vp, _vp, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp],
}
KEYFRAME_SYMBOLS = sorted(_KEYFRAME_SIGS)
for _name, _sig in _KEYFRAME_SIGS.items():
    _fn = getattr(lib, _name)
    _fn.argtypes = _sig
    _fn.restype = C.c_int


class StepCacheParamsC(C.Structure):             # ltx_step_cache_params (include/ltxhip_stepcache.h)
    _fields_ = [("rel_l1_thresh", C.c_float), ("coeff", C.c_float * 5), ("pattern", C.POINTER(C.c_ubyte)), ("n_pattern", C.c_int)]


# include/ltxhip_stepcache.h (kept apart like the eight above)
_STEPCACHE_SIGS = {
    "ltx_step_cache_params_default": [_vp], "ltx_step_cache_create": [_vp, _i, _vp], "ltx_step_cache_destroy": [_vp], "ltx_step_cache_reset": [_vp],
    "ltx_step_cache_decide": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp],
    "ltx_step_cache_require": [_vp, _vp, _i, _i, _i, _vp],
    "ltx_dit_forward_cached": [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp],
    "ltx_step_cache_read_residual": [_vp, _i, _vp, _vp],
    "ltx_pipeline_call_cached": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp],
    "ltx_op_step_measure_ws_bytes": [_i64, _i, _i],
    "ltx_op_step_measure": [_vp, _vp, _vp, _vp, _i, _i64, _i, _i64, _f, _i, _i, _vp, _vp, _vp],
    "ltx_op_step_residual": [_vp, _vp, _i64, _i, _i, _vp],
}
STEPCACHE_SYMBOLS = sorted(_STEPCACHE_SIGS)
for _name, _sig in _STEPCACHE_SIGS.items():
    _fn = getattr(lib, _name)
    _fn.argtypes = _sig
    _fn.restype = None if _name in ("ltx_step_cache_params_default", "ltx_step_cache_destroy") else C.c_size_t if _name == "ltx_op_step_measure_ws_bytes" else C.c_int
STEP_COMPUTE, STEP_REUSE = 1, 2                  # values of a step cache pattern (0: decide)


# include/ltxhip_int8.h (kept apart like the nine above)
_INT8_SIGS = {
    "ltx_dit_set_int8_linears": [_vp, _vp, C.c_ubyte, _vp], "ltx_dit_get_int8_linears": [_vp, _vp],
    "ltx_op_quant_rows_i8": [_vp, _i64, _i, _i, _vp, _vp, _vp],
    "ltx_op_rownorm_quant_i8": [_vp, _i64, _i, _i, _f, _vp, _vp, _i, _i64, _vp, _vp, _vp],
    "ltx_op_gemm_i8": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp],
    "ltx_op_gemm_i8_raw": [_vp, _vp, _vp, _i, _i, _i, _i, _vp],
}
INT8_SYMBOLS = sorted(_INT8_SIGS)
for _name, _sig in _INT8_SIGS.items():
    _fn = getattr(lib, _name)
    _fn.argtypes = _sig
    _fn.restype = C.c_int
LTX_I8_QKV, LTX_I8_TO_OUT, LTX_I8_FF1, LTX_I8_FF2, LTX_I8_ALL = 1, 2, 4, 8, 15
INT8_LINEARS = ("qkv", "to_out", "ff1", "ff2")   # the mask bits of ltx_dit_set_int8_linears, lowest first
GEMM_I8_TILES = ("256x256", "256x128", "128x128")


def int8_mask(mask_or_names) -> int:
    """the LTX_I8_* mask of an int, a name of INT8_LINEARS, 'all' / 'none', or a sequence of names"""
    if mask_or_names is None:
        return 0
    if isinstance(mask_or_names, int):
        m = mask_or_names
    else:
        names = [mask_or_names] if isinstance(mask_or_names, str) else list(mask_or_names)
        m = 0
        for n in names:
            if n == "all":
                m |= LTX_I8_ALL
            elif n in INT8_LINEARS:
                m |= 1 << INT8_LINEARS.index(n)
            elif n != "none":
                raise LtxError(f"int8 linears: unknown name {n!r} (one of {INT8_LINEARS}, 'all', 'none')")
    if m < 0 or m > LTX_I8_ALL:
        raise LtxError(f"int8 linears: mask {m} has bits outside LTX_I8_ALL ({LTX_I8_ALL})")
    return m


@dataclass
class StepCacheParams:
    """ltx_step_cache_params: reuse the block residual while the accumulated poly(distance) stays below rel_l1_thresh (0: never);
    coeff = (c0 .. c4), highest power first - a published fit for the checkpoint goes here; pattern: per step 0 decide, 1 compute,
    2 reuse.  The rule is spelled out in include/ltxhip_stepcache.h."""
    rel_l1_thresh: float = 0.0
    coeff: Sequence[float] = (0.0, 0.0, 0.0, 1.0, 0.0)
    pattern: Optional[Sequence[int]] = None

    def to_c(self, keep: list) -> StepCacheParamsC:
        if len(self.coeff) != 5:
            raise LtxError("StepCacheParams: coeff has five values (c0 .. c4)")
        c = StepCacheParamsC()
        c.rel_l1_thresh = float(self.rel_l1_thresh)
        c.coeff = (C.c_float * 5)(*[float(v) for v in self.coeff])
        if self.pattern is not None and len(self.pattern) > 0:
            if any(int(v) < 0 or int(v) > 255 for v in self.pattern):
                raise LtxError("StepCacheParams: pattern values are 0 (decide), 1 (compute) or 2 (reuse)")
            pt = (C.c_ubyte * len(self.pattern))(*[int(v) for v in self.pattern]); keep.append(pt)
            c.pattern, c.n_pattern = C.cast(pt, C.POINTER(C.c_ubyte)), len(self.pattern)
        return c


@dataclass
class GuidanceSchedule:
    """ltx_guidance_schedule: one (guidance_scale, stg_scale, rescale, perturbed block list) per entry; a step takes the entry whose
    guidance_timesteps value is nearest its sigma (without guidance_timesteps: one entry for every step, or one per step).
    rescale_form: 'cfg' (the reference: rescale the CFG mix, then add the STG term) or 'mix' (the published recipes: rescale the whole
    mix on perturbed steps, 1 = off).  The rule is spelled out in include/ltxhip_guidance.h."""
    guidance_scale: Sequence[float]
    stg_scale: Sequence[float]
    rescale: Sequence[float]
    skip_block_list: Optional[Sequence[Sequence[int]]] = None
    guidance_timesteps: Optional[Sequence[float]] = None
    cfg_star: bool = False
    rescale_form: object = "cfg"

    def to_c(self, keep: list) -> GuidanceScheduleC:
        n = len(self.guidance_scale)
        skip = [list(b) for b in self.skip_block_list] if self.skip_block_list is not None else [[] for _ in range(n)]
        if not (len(self.stg_scale) == len(self.rescale) == len(skip) == n) or (self.guidance_timesteps is not None and len(self.guidance_timesteps) != n):
            raise LtxError("GuidanceSchedule: every list must have one value per entry")
        form = RESCALE_FORMS.index(self.rescale_form) if isinstance(self.rescale_form, str) and self.rescale_form in RESCALE_FORMS else self.rescale_form
        if isinstance(form, str):
            raise LtxError(f"GuidanceSchedule: unknown rescale_form {form!r} (one of {RESCALE_FORMS})")
        g, s, r = _floats(self.guidance_scale), _floats(self.stg_scale), _floats(self.rescale)
        flat = [int(b) for blocks in skip for b in blocks]
        offs = [0]
        for blocks in skip:
            offs.append(offs[-1] + len(blocks))
        sb, so = (C.c_int * max(len(flat), 1))(*flat), (C.c_int * (n + 1))(*offs)
        keep += [g, s, r, sb, so]
        c = GuidanceScheduleC(n, C.cast(g, _fp), C.cast(s, _fp), C.cast(r, _fp), C.cast(sb, C.POINTER(C.c_int)), C.cast(so, C.POINTER(C.c_int)), None,
                              int(self.cfg_star), int(form))
        if self.guidance_timesteps is not None:
            gt = _floats(self.guidance_timesteps); keep.append(gt)
            c.guidance_timesteps = C.cast(gt, _fp)
        return c

    def resolve(self, sigmas: Sequence[float]) -> List[int]:
        """entry of every step that starts at sigmas[i] (ltx_guidance_schedule_resolve; host only)"""
        keep = []
        c = self.to_c(keep)
        sg = _floats(sigmas)
        out = (C.c_int * max(len(sigmas), 1))()
        _check(lib.ltx_guidance_schedule_resolve(C.byref(c), sg, len(sigmas), out))
        return list(out)[:len(sigmas)]


# the ten LoRA targets of a block, in the order of ltx_dit_read_linear's `which`
LORA_TARGETS = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v", "attn2.to_out.0",
                "ff.net.0.proj", "ff.net.2")


def _dt(t: torch.dtype) -> int:
    if t == torch.float32:
        return LTX_F32
    if t == torch.bfloat16:
        return LTX_BF16
    raise LtxError(f"unsupported dtype {t}")


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t: torch.Tensor, dtype=None) -> torch.Tensor:
    if not t.is_cuda:
        raise LtxError("tensor must live on the GPU (the library takes device pointers)")
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def _expect(name: str, t: torch.Tensor, shape):
    if tuple(t.shape) != tuple(shape):
        raise LtxError(f"{name}: shape {tuple(t.shape)} does not match the call's geometry {tuple(shape)}")


def _make_weights(weights: Dict[str, torch.Tensor]):
    arr = (_Weight * len(weights))()
    keep = []
    for i, (name, t) in enumerate(weights.items()):
        if t.dtype not in (torch.float32, torch.bfloat16):
            t = t.float()
        t = t.contiguous()
        keep.append(t)
        nb = name.encode()
        keep.append(nb)
        arr[i].name = nb
        arr[i].data = t.data_ptr()
        arr[i].dtype = _dt(t.dtype)
        arr[i].ndim = t.dim()
        for j in range(t.dim()):
            arr[i].shape[j] = t.shape[j]
        arr[i].on_device = 1 if t.is_cuda else 0
    return arr, keep


def _floats(vals) -> "C.Array":
    return (C.c_float * len(vals))(*[float(v) for v in vals])


def _hold_host(hold, B: int, F: int) -> "C.Array":
    """hold [B, F] (tensor or nested sequence, truthy = held) -> HOST u8 array in the order the C side reads"""
    h = hold.detach().cpu().reshape(-1).tolist() if torch.is_tensor(hold) else [v for row in hold for v in (row if isinstance(row, (list, tuple)) else [row])]
    if len(h) != B * F:
        raise LtxError(f"hold must have {B} x {F} entries (batch rows x latent frames), got {len(h)}")
    return (C.c_ubyte * (B * F))(*[1 if v else 0 for v in h])


# ------------------------------------------------------------------ DiT
@dataclass
class LtxVideoTransformer3DModelConfig:          # ltx_transformer.rs:23-58
    in_channels: int = 128
    out_channels: int = 128
    patch_size: int = 1
    patch_size_t: int = 1
    num_attention_heads: int = 32
    attention_head_dim: int = 64
    cross_attention_dim: int = 2048
    num_layers: int = 28
    norm_eps: float = 1e-6
    caption_channels: int = 4096


class LtxVideoTransformer3DModel:
    """impl VideoTransformer3D (t2v_pipeline.rs:63-83) over ltx_dit_*."""

    def __init__(self, config: LtxVideoTransformer3DModelConfig, weights: Dict[str, torch.Tensor],
                 dtype: torch.dtype = torch.bfloat16, device: int = 0):
        self.config = config
        self.dtype = dtype
        c = DitConfigC(config.in_channels, config.out_channels, config.patch_size, config.patch_size_t,
                       config.num_attention_heads, config.attention_head_dim, config.cross_attention_dim,
                       config.num_layers, config.norm_eps, config.caption_channels)
        arr, keep = _make_weights(weights)
        self._h = C.c_void_p()
        _check(lib.ltx_dit_create(C.byref(c), arr, C.c_size_t(len(weights)), _dt(dtype), device, C.byref(self._h)))
        del keep

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:
            lib.ltx_dit_destroy(h)
            self._h = None

    @classmethod
    def from_files(cls, config: "LtxVideoTransformer3DModelConfig", path: str, unified: bool = False,
                   dtype: torch.dtype = torch.bfloat16, device: int = 0) -> "LtxVideoTransformer3DModel":
        """Build from a checkpoint on disk (ltx_dit_create_from_files): `unified` = Official single-file checkpoint
        (keys remapped/split as examples/ltx-video/main.rs:461-499), else the transformer's own file or directory."""
        self = cls.__new__(cls)
        self.config, self.dtype = config, dtype
        c = DitConfigC(config.in_channels, config.out_channels, config.patch_size, config.patch_size_t,
                       config.num_attention_heads, config.attention_head_dim, config.cross_attention_dim,
                       config.num_layers, config.norm_eps, config.caption_channels)
        self._h = C.c_void_p()
        _check(lib.ltx_dit_create_from_files(C.byref(c), path.encode(), int(unified), _dt(dtype), device, C.byref(self._h)))
        return self

    def context_cache(self, enable: bool):
        """keep the text-side projections (caption projection, cross-attention K/V) of repeated forwards with the same
        embeddings/mask pointers; LtxPipeline::call scopes it to one denoise loop."""
        _check(lib.ltx_dit_context_cache(self._h, int(enable)))
        self._ctx_cache = bool(enable)

    def set_skip_block_list(self, blocks: Sequence[int]):
        arr = (C.c_int * max(len(blocks), 1))(*blocks)
        _check(lib.ltx_dit_set_skip_blocks(self._h, arr, len(blocks)))

    def forward(self, hidden_states: torch.Tensor, encoder_hidden_states: torch.Tensor, timestep,
                encoder_attention_mask: Optional[torch.Tensor], num_frames: int, height: int, width: int,
                rope_interpolation_scale: Optional[Tuple[float, float, float]] = None,
                video_coords: Optional[torch.Tensor] = None,
                skip_layer_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        io = hidden_states.dtype if hidden_states.dtype in (torch.float32, torch.bfloat16) else torch.float32
        h = _dev(hidden_states, io)
        e = _dev(encoder_hidden_states, io)
        if h.dim() != 3 or e.dim() != 3:
            raise LtxError("hidden_states must be [B,S,C] and encoder_hidden_states [B,K,C]")
        B, S, _ = h.shape
        K = e.shape[1]
        t = timestep.detach().float().flatten().cpu().tolist() if torch.is_tensor(timestep) else list(timestep)
        if len(t) != B:
            raise LtxError(f"timestep must have {B} entries")
        m = _dev(encoder_attention_mask, torch.float32) if encoder_attention_mask is not None else None
        if getattr(self, "_ctx_cache", False):
            # the cache identifies a context by its device POINTERS: a converted / re-laid-out temporary is freed after this
            # call and its address reused by the next one, which would hit the cache with another context's K/V
            if e.data_ptr() != encoder_hidden_states.data_ptr() or (m is not None and m.data_ptr() != encoder_attention_mask.data_ptr()):
                raise LtxError("context_cache(True) needs encoder_hidden_states / encoder_attention_mask that are already contiguous and of "
                               "the dtype the call uses (hidden_states' dtype / float32): a temporary copy has no stable identity")
        vc = _dev(video_coords, torch.float32) if video_coords is not None else None
        if getattr(self, "_ctx_cache", False) and vc is not None and vc.data_ptr() != video_coords.data_ptr():
            raise LtxError("context_cache(True) needs video_coords that are already a contiguous float32 device tensor: the RoPE "
                           "tables of the scope are kept per coords POINTER, a temporary copy has no stable identity")
        slm = None
        if skip_layer_mask is not None:
            slm = _floats(skip_layer_mask.detach().float().cpu().flatten().tolist())
        rs = _floats(rope_interpolation_scale) if rope_interpolation_scale is not None else None
        out = torch.empty(B, S, self.config.out_channels, dtype=io, device=h.device)
        _check(lib.ltx_dit_forward(self._h, _ptr(h), _ptr(e), _floats(t), _ptr(m), B, S, K, num_frames, height, width,
                                   rs, _ptr(vc), slm, _dt(io), _ptr(out), _stream()))
        return out


    def forward_frames(self, hidden_states: torch.Tensor, encoder_hidden_states: torch.Tensor, timestep,
                       encoder_attention_mask: Optional[torch.Tensor], num_frames: int, height: int, width: int,
                       rope_interpolation_scale: Optional[Tuple[float, float, float]] = None,
                       video_coords: Optional[torch.Tensor] = None,
                       skip_layer_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """forward with one timestep per (batch row, latent frame): timestep [B, num_frames]; (num_frames, height, width) is the
        latent grid and S must equal its product (ltx_dit_forward_frames, include/ltxhip_cond.h).  Inside context_cache(True) the
        tensors must already be contiguous and of the call's dtype, as for forward."""
        io = hidden_states.dtype if hidden_states.dtype in (torch.float32, torch.bfloat16) else torch.float32
        h = _dev(hidden_states, io)
        e = _dev(encoder_hidden_states, io)
        if h.dim() != 3 or e.dim() != 3:
            raise LtxError("hidden_states must be [B,S,C] and encoder_hidden_states [B,K,C]")
        B, S, _ = h.shape
        K = e.shape[1]
        t = torch.as_tensor(timestep, dtype=torch.float32).detach().flatten().cpu().tolist()
        if len(t) != B * num_frames:
            raise LtxError(f"timestep must have {B} x {num_frames} entries (batch rows x latent frames)")
        if num_frames * height * width != S:
            raise LtxError("forward_frames: S must equal num_frames*height*width (tokens in pack order, with or without video_coords)")
        m = _dev(encoder_attention_mask, torch.float32) if encoder_attention_mask is not None else None
        vc = _dev(video_coords, torch.float32) if video_coords is not None else None
        if getattr(self, "_ctx_cache", False) and (e.data_ptr() != encoder_hidden_states.data_ptr() or (m is not None and m.data_ptr() != encoder_attention_mask.data_ptr())
                                                   or (vc is not None and vc.data_ptr() != video_coords.data_ptr())):
            raise LtxError("context_cache(True) needs encoder_hidden_states / encoder_attention_mask / video_coords that are already contiguous "
                           "device tensors of the dtype the call uses: a temporary copy has no stable identity")
        slm = _floats(skip_layer_mask.detach().float().cpu().flatten().tolist()) if skip_layer_mask is not None else None
        rs = _floats(rope_interpolation_scale) if rope_interpolation_scale is not None else None
        out = torch.empty(B, S, self.config.out_channels, dtype=io, device=h.device)
        _check(lib.ltx_dit_forward_frames(self._h, _ptr(h), _ptr(e), _floats(t), _ptr(m), B, S, K, num_frames, height, width,
                                          rs, _ptr(vc), slm, _dt(io), _ptr(out), _stream()))
        return out

    # ---- STG modes (include/ltxhip_stg.h): handle state, so every forward with a skip_layer_mask and LtxPipeline.call obey it
    def set_stg_mode(self, mode):
        """what a skip_layer_mask perturbs: 'transformer_block' (default), 'attention_skip', 'attention_values' - or the ltx_stg_mode value"""
        _check(lib.ltx_dit_set_stg_mode(self._h, stg_mode_from_name(mode) if isinstance(mode, str) else int(mode)))

    @property
    def stg_mode(self) -> str:
        out = C.c_int(0)
        _check(lib.ltx_dit_get_stg_mode(self._h, C.byref(out)))
        return STG_MODES[out.value]

    # ---- INT8 (W8A8) block linears (include/ltxhip_int8.h): handle state, so every forward and LtxPipeline.call run on whatever is set
    def set_int8_linears(self, mask_or_names=0, block_masks: Optional[Sequence] = None):
        """run the named block linears - 'qkv', 'to_out', 'ff1', 'ff2', 'all', or an LTX_I8_* mask - on the int8 MFMA; block_masks: one
        entry per block (same forms), and-ed with the mask (zeros keep a block in bf16).  0 / 'none' frees the int8 copies.  A bf16
        model only.  Enqueued on the current stream; set_adapters afterwards is fine (the copies follow the merged weights)."""
        m = int8_mask(mask_or_names)
        arr = None
        if block_masks is not None:
            bm = [int8_mask(v) for v in block_masks]
            if len(bm) != self.config.num_layers:
                raise LtxError(f"set_int8_linears: block_masks has {len(bm)} entries for {self.config.num_layers} blocks")
            arr = (C.c_ubyte * len(bm))(*bm)
        _check(lib.ltx_dit_set_int8_linears(self._h, arr, m, _stream()))

    @property
    def int8_linears(self) -> List[int]:
        """the LTX_I8_* mask of every block"""
        out = (C.c_ubyte * self.config.num_layers)()
        _check(lib.ltx_dit_get_int8_linears(self._h, out))
        return list(out)

    # ---- LoRA adapters (include/ltxhip_lora.h): handle state, so LtxPipeline.call runs on whatever is set
    def set_adapters(self, loras: Sequence["LtxLora"] = (), scales: Optional[Sequence[float]] = None):
        """effective weights = base + sum_i scales[i] * factor_i * (B_i A_i) on every linear the adapters target (no history: the list
        replaces whatever was set; an empty list restores the base bit for bit).  Enqueued on the current stream."""
        loras = list(loras)
        scales = [1.0] * len(loras) if scales is None else [float(v) for v in scales]
        if len(scales) != len(loras):
            raise LtxError(f"set_adapters: {len(loras)} adapters but {len(scales)} scales")
        arr = (C.c_void_p * max(len(loras), 1))(*[l._h for l in loras])
        _check(lib.ltx_dit_set_adapters(self._h, arr, _floats(scales) if scales else None, len(loras), _stream()))
        self._adapters = loras                  # (not needed by the library - merged weights do not refer to them - but cheap to show)

    def adapter_count(self) -> int:
        return int(lib.ltx_dit_adapter_count(self._h))

    def linear_shape(self, which: int):
        D = self.config.num_attention_heads * self.config.attention_head_dim
        return (4 * D if which == 8 else D, 4 * D if which == 9 else self.config.cross_attention_dim if which in (5, 6) else D)

    def read_linear(self, block: int, which: int, device="cuda") -> torch.Tensor:
        """the current effective [out, in] matrix of linear `which` (index into LORA_TARGETS) of block `block`, model dtype"""
        if not 0 <= which < 10:
            raise LtxError("read_linear: which must be 0..9 (LORA_TARGETS)")
        out = torch.empty(self.linear_shape(which), dtype=self.dtype, device=device)
        _check(lib.ltx_dit_read_linear(self._h, block, which, _ptr(out), _stream()))
        return out


def lora_parse_key(key: str):
    """(module name in Diffusers layout, role) of an adapter tensor name; role 0 = A / down, 1 = B / up, 2 = alpha (host only)"""
    buf = C.create_string_buffer(1024)
    role = C.c_int(0)
    _check(lib.ltx_lora_parse_key(key.encode(), buf, C.c_size_t(len(buf)), C.byref(role)))
    return buf.value.decode(), role.value


class LtxLora:
    """One LoRA adapter (ltx_lora): A / B pairs for block linears, uploaded once in the model dtype of `model`; usable with every
    handle of the same configuration.  n_unmatched: adapter keys on modules that are not block linears."""

    def __init__(self):
        raise LtxError("use LtxLora.from_file or LtxLora.from_tensors")

    @classmethod
    def from_tensors(cls, model: LtxVideoTransformer3DModel, tensors: Dict[str, torch.Tensor], strict: bool = False) -> "LtxLora":
        self = cls.__new__(cls)
        arr, keep = _make_weights(tensors)
        self._h = C.c_void_p()
        nu = C.c_int(0)
        _check(lib.ltx_lora_create(model._h, arr, C.c_size_t(len(tensors)), int(strict), C.byref(self._h), C.byref(nu)))
        del keep
        self.n_unmatched = nu.value
        return self

    @classmethod
    def from_file(cls, model: LtxVideoTransformer3DModel, path: str, strict: bool = False) -> "LtxLora":
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        nu = C.c_int(0)
        _check(lib.ltx_lora_create_from_file(model._h, path.encode(), int(strict), C.byref(self._h), C.byref(nu)))
        self.n_unmatched = nu.value
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:
            lib.ltx_lora_destroy(h)
            self._h = None


# ------------------------------------------------------------------ T5 text encoder (include/ltxhip_t5.h)
class T5ConfigC(C.Structure):
    _fields_ = [("vocab_size", C.c_int), ("d_model", C.c_int), ("d_kv", C.c_int), ("d_ff", C.c_int), ("num_layers", C.c_int),
                ("num_heads", C.c_int), ("relative_attention_num_buckets", C.c_int), ("relative_attention_max_distance", C.c_int),
                ("layer_norm_epsilon", C.c_float)]


@dataclass
class T5EncoderConfig:                           # text_encoder.rs:66-113; defaults = t5_xxl() (:169-184)
    vocab_size: int = 32128
    d_model: int = 4096
    d_kv: int = 64
    d_ff: int = 10240
    num_layers: int = 24
    num_heads: int = 64
    relative_attention_num_buckets: int = 32
    relative_attention_max_distance: int = 128
    layer_norm_epsilon: float = 1e-6


class T5TextEncoder:
    """impl VTextEncoder (text_encoder.rs:597-606) over ltx_t5_*: forward(input_ids) -> [B,S,d_model] in the model dtype."""

    def __init__(self, config: T5EncoderConfig, weights: Optional[Dict[str, torch.Tensor]], dtype: torch.dtype = torch.bfloat16, device: int = 0,
                 gguf_path: Optional[str] = None):
        self.config, self.dtype = config, dtype
        c = T5ConfigC(config.vocab_size, config.d_model, config.d_kv, config.d_ff, config.num_layers, config.num_heads,
                      config.relative_attention_num_buckets, config.relative_attention_max_distance, config.layer_norm_epsilon)
        self._h = C.c_void_p()
        if gguf_path is not None:
            _check(lib.ltx_t5_create_from_gguf(C.byref(c), os.fsencode(gguf_path), _dt(dtype), device, C.byref(self._h)))
            return
        arr, keep = _make_weights(weights)
        _check(lib.ltx_t5_create(C.byref(c), arr, C.c_size_t(len(weights)), _dt(dtype), device, C.byref(self._h)))
        del keep

    @classmethod
    def from_gguf(cls, gguf_path: str, config: Optional[T5EncoderConfig] = None, dtype: torch.dtype = torch.float32, device: int = 0):
        """QuantizedT5EncoderModel::load_with_config (quantized_t5_encoder.rs:575-603): the reference's default text encoder"""
        return cls(config or T5EncoderConfig(), None, dtype, device, gguf_path=gguf_path)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:                    # `lib` is already None when the interpreter is shutting down
            lib.ltx_t5_destroy(h)
            self._h = None

    def forward(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """forward(input_ids) (text_encoder.rs:600-605) / forward(input_ids, Some(mask)) (quantized_t5_encoder.rs:608-650)"""
        ids = input_ids.detach().to("cpu", torch.int32).contiguous()
        if ids.dim() != 2:
            raise LtxError("input_ids must be [B, S]")
        B, S = ids.shape
        out = torch.empty(B, S, self.config.d_model, dtype=self.dtype, device=torch.device("cuda", torch.cuda.current_device()))
        if attention_mask is not None:
            am = attention_mask.detach().to("cpu", torch.float32).contiguous()
            if tuple(am.shape) != (B, S):
                raise LtxError("attention_mask must be [B, S]")
            _check(lib.ltx_t5_forward_masked(self._h, C.c_void_p(ids.data_ptr()), C.c_void_p(am.data_ptr()), B, S, _dt(self.dtype), _ptr(out), _stream()))
        else:
            _check(lib.ltx_t5_forward(self._h, C.c_void_p(ids.data_ptr()), B, S, _dt(self.dtype), _ptr(out), _stream()))
        torch.cuda.current_stream().synchronize()       # the ids were read from host memory asynchronously
        return out


# ------------------------------------------------------------------ GGUF (include/ltxhip_weights.h)
GGML_TYPES = {"F32": 0, "F16": 1, "Q4_0": 2, "Q5_0": 6, "Q8_0": 8, "Q4_K": 12, "Q5_K": 13, "Q6_K": 14, "BF16": 30}


def gguf_type_info(ggml_type: int):
    be, bb = C.c_int(), C.c_int()
    _check(lib.ltx_gguf_type_info(ggml_type, C.byref(be), C.byref(bb)))
    return be.value, bb.value


def gguf_tensors(path: str):
    """[(name, ggml_type, shape outermost-first, raw bytes)] of a GGUF file, in file order (host-side parser, no GPU needed)"""
    h = C.c_void_p()
    _check(lib.ltx_gguf_open(os.fsencode(path), C.byref(h)))
    try:
        out = []
        for i in range(lib.ltx_gguf_count(h)):
            nm, ty, nd, shp, data, nb = C.c_char_p(), C.c_int(), C.c_int(), C.POINTER(C.c_int64)(), C.c_void_p(), C.c_size_t()
            rc = lib.ltx_gguf_tensor(h, i, C.byref(nm), C.byref(ty), C.byref(nd), C.byref(shp), C.byref(data), C.byref(nb))
            raw = C.string_at(data, nb.value) if rc == 0 else None
            out.append((nm.value.decode(), ty.value, tuple(shp[k] for k in range(nd.value)), raw))
        return out
    finally:
        lib.ltx_gguf_close(h)


def gguf_dequantize(ggml_type: int, blocks: bytes, numel: int, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """QTensor::dequantize on the device: raw ggml blocks (host bytes) -> dense [numel] tensor"""
    out = torch.empty(numel, dtype=dtype, device=torch.device("cuda", torch.cuda.current_device()))
    buf = C.create_string_buffer(blocks, len(blocks))
    _check(lib.ltx_gguf_dequantize(ggml_type, buf, 0, numel, _dt(dtype), _ptr(out), _stream()))
    torch.cuda.current_stream().synchronize()
    return out


# ------------------------------------------------------------------ VAE
@dataclass
class AutoencoderKLLtxVideoConfig:               # vae.rs:32-103 (decoder side)
    latent_channels: int = 128
    out_channels: int = 3
    decoder_block_out_channels: Tuple[int, ...] = (256, 512, 1024)
    decoder_layers_per_block: Tuple[int, ...] = (5, 5, 5, 5)
    decoder_upsample_factor: Tuple[int, ...] = (2, 2, 2)
    patch_size: int = 4
    patch_size_t: int = 1
    timestep_conditioning: bool = True
    decoder_causal: bool = False
    scaling_factor: float = 1.0
    spatial_compression_ratio: int = 32
    temporal_compression_ratio: int = 8
    decoder_inject_noise: Tuple[bool, ...] = (False, False, False, False)     # vae.rs:87; blocks whose resnets add noise[h, w] * per_channel_scale (set_noise_seed)
    decoder_upsample_residual: Tuple[bool, ...] = (True, True, True)            # vae.rs:88
    decoder_spatiotemporal_scaling: Tuple[bool, ...] = (True, True, True)       # vae.rs:78; False: that up-block's upsampler is the spatial-only (1, 2, 2) form
    resnet_eps: float = 1e-6                                                    # vae.rs:83 (norm3 only: unused by the decoder)


DOWNSAMPLE_TYPES = {"conv": 0, "spatial": 1, "temporal": 2, "spatiotemporal": 3}      # DownsampleType::parse, vae.rs:477-485


@dataclass
class AutoencoderKLLtxVideoEncoderConfig:        # vae.rs:32-103 (encoder side)
    in_channels: int = 3
    latent_channels: int = 128
    block_out_channels: Tuple[int, ...] = (128, 256, 512, 1024, 2048)
    layers_per_block: Tuple[int, ...] = (4, 6, 6, 2, 2)
    spatiotemporal_scaling: Tuple[bool, ...] = (True, True, True, True)
    downsample_types: Tuple[str, ...] = ("spatial", "temporal", "spatiotemporal", "spatiotemporal")
    patch_size: int = 4
    patch_size_t: int = 1
    is_causal: bool = True
    spatial_compression_ratio: int = 32
    temporal_compression_ratio: int = 8

    def to_c(self) -> "VaeEncoderConfigC":
        c = VaeEncoderConfigC()
        c.in_channels, c.latent_channels, c.n_blocks = self.in_channels, self.latent_channels, len(self.block_out_channels)
        for i, x in enumerate(self.block_out_channels[:5]): c.block_out_channels[i] = x
        for i, x in enumerate(self.layers_per_block[:5]): c.layers_per_block[i] = x
        for i, x in enumerate(self.spatiotemporal_scaling[:4]): c.spatiotemporal_scaling[i] = int(x)
        for i, x in enumerate(self.downsample_types[:4]): c.downsample_types[i] = DOWNSAMPLE_TYPES.get(str(x).lower(), 0) if not isinstance(x, int) else x
        c.patch_size, c.patch_size_t, c.is_causal = self.patch_size, self.patch_size_t, int(self.is_causal)
        c.spatial_compression_ratio, c.temporal_compression_ratio = self.spatial_compression_ratio, self.temporal_compression_ratio
        return c


class DiagonalGaussianDistribution:
    """vae.rs:117-145 over the two tensors ltx_vae_encode writes; sample() takes the noise (the reference draws it from the device RNG)."""

    def __init__(self, mean: torch.Tensor, logvar: torch.Tensor):
        self.mean, self.logvar = mean, logvar

    def mode(self) -> torch.Tensor:
        return self.mean.clone()

    def sample(self, eps: torch.Tensor) -> torch.Tensor:
        e = _dev(eps, torch.float32)
        _expect("eps", e, self.mean.shape)
        out = torch.empty_like(self.mean)
        _check(lib.ltx_vae_posterior_sample(_ptr(self.mean), _ptr(self.logvar), _ptr(e), C.c_size_t(self.mean.numel()), _ptr(out), _stream()))
        return out


class LtxVideoEncoder3d:
    """LtxVideoEncoder3d (vae.rs:1316-1469) over ltx_vae_encoder_*; weight names relative to `encoder.` (or carrying that prefix)."""

    def __init__(self, config: AutoencoderKLLtxVideoEncoderConfig, weights: Dict[str, torch.Tensor],
                 dtype: torch.dtype = torch.bfloat16, device: int = 0):
        self.config, self.dtype = config, dtype
        c = config.to_c()
        arr, keep = _make_weights(weights)
        self._h = C.c_void_p()
        _check(lib.ltx_vae_encoder_create(C.byref(c), arr, C.c_size_t(len(weights)), _dt(dtype), device, C.byref(self._h)))
        del keep

    @classmethod
    def from_files(cls, config: AutoencoderKLLtxVideoEncoderConfig, path: str, unified: bool = False,
                   dtype: torch.dtype = torch.bfloat16, device: int = 0) -> "LtxVideoEncoder3d":
        self = cls.__new__(cls)
        self.config, self.dtype = config, dtype
        c = config.to_c()
        self._h = C.c_void_p()
        _check(lib.ltx_vae_encoder_create_from_files(C.byref(c), path.encode(), int(unified), _dt(dtype), device, C.byref(self._h)))
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:
            lib.ltx_vae_encoder_destroy(h)
            self._h = None

    def get_config(self) -> "VaeEncoderConfigC":
        c = VaeEncoderConfigC()
        _check(lib.ltx_vae_encoder_get_config(self._h, C.byref(c)))
        return c

    def latent_shape(self, B: int, F: int, H: int, W: int):
        r, tr = self.config.spatial_compression_ratio, self.config.temporal_compression_ratio
        return (B, self.config.latent_channels, (F - 1) // tr + 1, H // r, W // r)

    def _video(self, x: torch.Tensor):
        io = x.dtype if x.dtype in (torch.float32, torch.bfloat16) else torch.float32
        v = _dev(x, io)
        if v.dim() != 5 or v.shape[1] != self.config.in_channels:
            raise LtxError("video must be [B, in_channels, F, H, W]")
        return v, io

    def encode(self, x: torch.Tensor, tiling: Optional[TilingC] = None, framewise: bool = False, want_logvar: bool = True):
        v, io = self._video(x)
        B, _, F, H, W = v.shape
        shp = self.latent_shape(B, F, H, W)
        mean = torch.empty(shp, dtype=torch.float32, device=v.device)
        logvar = torch.empty(shp, dtype=torch.float32, device=v.device) if want_logvar else None
        et = EncodeTilingC(int(framewise))
        _check(lib.ltx_vae_encode(self._h, _ptr(v), _dt(io), B, F, H, W, C.byref(tiling) if tiling else None, C.byref(et),
                                  _ptr(mean), _ptr(logvar), _stream()))
        return mean, logvar

    def encode_tokens(self, vae: "AutoencoderKLLtxVideo", x: torch.Tensor, eps: Optional[torch.Tensor] = None,
                      tiling: Optional[TilingC] = None, framewise: bool = False) -> torch.Tensor:
        v, io = self._video(x)
        B, _, F, H, W = v.shape
        shp = self.latent_shape(B, F, H, W)
        e = None
        if eps is not None:
            e = _dev(eps, torch.float32)
            _expect("eps", e, shp)
        out = torch.empty(B, shp[2] * shp[3] * shp[4], shp[1], dtype=torch.float32, device=v.device)
        et = EncodeTilingC(int(framewise))
        _check(lib.ltx_vae_encode_tokens(self._h, vae._h, _ptr(v), _dt(io), B, F, H, W, C.byref(tiling) if tiling else None, C.byref(et),
                                         _ptr(e), _ptr(out), _stream()))
        return out

    def warmup(self, B: int, F: int, H: int, W: int, tiling: Optional[TilingC] = None, framewise: bool = False):
        et = EncodeTilingC(int(framewise))
        _check(lib.ltx_vae_encoder_warmup(self._h, B, F, H, W, C.byref(tiling) if tiling else None, C.byref(et), _stream()))


class AutoencoderKLLtxVideo:
    """impl VaeLtxVideo (t2v_pipeline.rs:91-103) over ltx_vae_*; tiling fields as vae.rs:1744-1758.
    The encode side (encode / forward, vae.rs:2070-2156) exists once load_encoder() has been given the `encoder.*` weights."""

    encoder: Optional["LtxVideoEncoder3d"] = None
    use_framewise_encoding = False

    def load_encoder(self, config: "AutoencoderKLLtxVideoEncoderConfig", weights: Dict[str, torch.Tensor], device: int = 0) -> None:
        self.encoder = LtxVideoEncoder3d(config, weights, self.dtype, device)

    def _encoder(self) -> "LtxVideoEncoder3d":
        if self.encoder is None:
            raise LtxError("this AutoencoderKLLtxVideo has no encoder: call load_encoder(config, weights) first")
        return self.encoder

    def _encode_tiling(self) -> Optional[TilingC]:
        if not (self.use_tiling or self.use_framewise_encoding):
            return None
        return TilingC(int(self.use_tiling), int(self.use_framewise_decoding), self.tile_sample_min_height,
                       self.tile_sample_min_width, self.tile_sample_min_num_frames, self.tile_sample_stride_height,
                       self.tile_sample_stride_width, self.tile_sample_stride_num_frames)

    def encode(self, x: torch.Tensor, return_dict: bool = True):
        """AutoencoderKLLtxVideo::encode (vae.rs:2070-2099): (AutoencoderKLOutput-like dict or None, posterior)."""
        mean, logvar = self._encoder().encode(x, self._encode_tiling(), self.use_framewise_encoding)
        post = DiagonalGaussianDistribution(mean, logvar)
        return ({"latent_dist": post} if return_dict else None), post

    def encode_tokens(self, x: torch.Tensor, eps: Optional[torch.Tensor] = None) -> torch.Tensor:
        """encode -> mode / sample(eps) -> normalize_latents -> pack_latents: the `latents` of LtxPipeline.call"""
        return self._encoder().encode_tokens(self, x, eps, self._encode_tiling(), self.use_framewise_encoding)

    def forward(self, sample: torch.Tensor, temb=None, sample_posterior: bool = False, eps: Optional[torch.Tensor] = None) -> torch.Tensor:
        """AutoencoderKLLtxVideo::forward (vae.rs:2139-2156): encode, mode or sample, decode.  `eps` is the draw of sample()."""
        _, post = self.encode(sample, True)
        if sample_posterior:
            if eps is None:
                raise LtxError("forward(sample_posterior=True) needs eps (the library draws no noise of its own)")
            z = post.sample(eps)
        else:
            z = post.mode()
        return self.decode(z, temb)

    @staticmethod
    def _config_c(config: "AutoencoderKLLtxVideoConfig") -> "VaeConfigC":
        c = VaeConfigC()
        c.latent_channels, c.out_channels = config.latent_channels, config.out_channels
        nb = len(config.decoder_block_out_channels)
        c.n_blocks = nb
        for i in range(nb):
            c.decoder_block_out_channels[i] = config.decoder_block_out_channels[i]
            c.decoder_upsample_factor[i] = config.decoder_upsample_factor[i]
        for i in range(nb + 1):
            c.decoder_layers_per_block[i] = config.decoder_layers_per_block[i]
        for i, x in enumerate(config.decoder_inject_noise[:5]): c.decoder_inject_noise[i] = int(x)
        for i, x in enumerate(config.decoder_upsample_residual[:4]): c.decoder_upsample_residual[i] = int(x)
        for i, x in enumerate(config.decoder_spatiotemporal_scaling[:4]): c.decoder_spatiotemporal_scaling[i] = int(x)
        c.resnet_eps = config.resnet_eps
        c.patch_size, c.patch_size_t = config.patch_size, config.patch_size_t
        c.timestep_conditioning = int(config.timestep_conditioning)
        c.decoder_causal = int(config.decoder_causal)
        c.scaling_factor = config.scaling_factor
        c.spatial_compression_ratio = config.spatial_compression_ratio
        c.temporal_compression_ratio = config.temporal_compression_ratio
        return c

    def _tiling_defaults(self):
        # defaults of examples/ltx-video/main.rs:514-516 (tiling off unless asked)
        self.use_tiling = False
        self.use_framewise_decoding = False
        self.tile_sample_min_height = 512
        self.tile_sample_min_width = 512
        self.tile_sample_min_num_frames = 16
        self.tile_sample_stride_height = 384
        self.tile_sample_stride_width = 384
        self.tile_sample_stride_num_frames = 8

    def __init__(self, config: AutoencoderKLLtxVideoConfig, weights: Dict[str, torch.Tensor],
                 dtype: torch.dtype = torch.bfloat16, device: int = 0):
        self.config = config
        self.dtype = dtype
        c = self._config_c(config)
        arr, keep = _make_weights(weights)
        self._h = C.c_void_p()
        _check(lib.ltx_vae_create(C.byref(c), arr, C.c_size_t(len(weights)), _dt(dtype), device, C.byref(self._h)))
        del keep
        self._tiling_defaults()

    @classmethod
    def from_files(cls, config: "AutoencoderKLLtxVideoConfig", path: str, unified: bool = False,
                   dtype: torch.dtype = torch.bfloat16, device: int = 0) -> "AutoencoderKLLtxVideo":
        """Build from a checkpoint on disk (ltx_vae_create_from_files); see LtxVideoTransformer3DModel.from_files."""
        self = cls.__new__(cls)
        self.config, self.dtype = config, dtype
        c = cls._config_c(config)
        self._h = C.c_void_p()
        _check(lib.ltx_vae_create_from_files(C.byref(c), path.encode(), int(unified), _dt(dtype), device, C.byref(self._h)))
        self.config = self._config_py(self.get_config())       # a vae/config.json beside the weights replaces `config` (main.rs:525-534)
        self._tiling_defaults()
        return self

    def set_noise_seed(self, seed: int) -> None:
        """Noise injection (decoder_inject_noise, vae.rs:741-753): plane k of this handle's life is Pcg32(seed, k).randn(H * W);
        restarts k at 0 (ltx_vae_set_noise_seed)."""
        _check(lib.ltx_vae_set_noise_seed(self._h, C.c_uint64(seed)))

    def injects_noise(self) -> bool:
        """whether any resnet of this decoder injects noise (the flag AND a per_channel_scaleN.weight in the checkpoint, vae.rs:676-689)"""
        return bool(lib.ltx_vae_injects_noise(self._h))

    def get_config(self) -> "VaeConfigC":
        """the engine's effective config (ltx_vae_get_config)"""
        c = VaeConfigC()
        _check(lib.ltx_vae_get_config(self._h, C.byref(c)))
        return c

    @staticmethod
    def _config_py(c: "VaeConfigC") -> "AutoencoderKLLtxVideoConfig":
        nb = c.n_blocks
        return AutoencoderKLLtxVideoConfig(
            latent_channels=c.latent_channels, out_channels=c.out_channels,
            decoder_block_out_channels=tuple(c.decoder_block_out_channels[:nb]), decoder_layers_per_block=tuple(c.decoder_layers_per_block[:nb + 1]),
            decoder_upsample_factor=tuple(c.decoder_upsample_factor[:nb]), patch_size=c.patch_size, patch_size_t=c.patch_size_t,
            timestep_conditioning=bool(c.timestep_conditioning), decoder_causal=bool(c.decoder_causal), scaling_factor=c.scaling_factor,
            spatial_compression_ratio=c.spatial_compression_ratio, temporal_compression_ratio=c.temporal_compression_ratio,
            decoder_inject_noise=tuple(bool(x) for x in c.decoder_inject_noise[:nb + 1]),
            decoder_upsample_residual=tuple(bool(x) for x in c.decoder_upsample_residual[:nb]),
            decoder_spatiotemporal_scaling=tuple(bool(x) for x in c.decoder_spatiotemporal_scaling[:nb]), resnet_eps=c.resnet_eps)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:
            lib.ltx_vae_destroy(h)
            self._h = None

    def _tiling(self) -> Optional[TilingC]:
        if not (self.use_tiling or self.use_framewise_decoding):
            return None
        return TilingC(int(self.use_tiling), int(self.use_framewise_decoding), self.tile_sample_min_height,
                       self.tile_sample_min_width, self.tile_sample_min_num_frames, self.tile_sample_stride_height,
                       self.tile_sample_stride_width, self.tile_sample_stride_num_frames)

    def decode(self, latents: torch.Tensor, timestep=None, postprocess: bool = False, rgb8: bool = False) -> torch.Tensor:
        """rgb8=True: the post-processed video as u8 frames [B, frames, H, W, 3] (main.rs:653-675) from the decoder's last epilogue"""
        io = latents.dtype if latents.dtype in (torch.float32, torch.bfloat16) else torch.float32
        z = _dev(latents, io)
        if z.dim() != 5 or z.shape[1] != self.config.latent_channels:
            raise LtxError("latents must be [B, latent_channels, F, H, W]")
        B, _, F, H, W = z.shape
        t = None
        if timestep is not None:
            tv = timestep.detach().float().flatten().cpu().tolist() if torch.is_tensor(timestep) else list(timestep)
            if len(tv) != B:
                raise LtxError(f"timestep must have {B} entries")
            t = _floats(tv)
        r, tr = self.config.spatial_compression_ratio, self.config.temporal_compression_ratio
        if rgb8:
            out = torch.empty(B, (F - 1) * tr + 1, H * r, W * r, self.config.out_channels, dtype=torch.uint8, device=z.device)
        else:
            out = torch.empty(B, self.config.out_channels, (F - 1) * tr + 1, H * r, W * r, dtype=torch.float32, device=z.device)
        tl = self._tiling()
        _check(lib.ltx_vae_decode(self._h, _ptr(z), _dt(io), t, B, F, H, W, C.byref(tl) if tl else None, 2 if rgb8 else int(postprocess),
                                  _ptr(out), _stream()))
        return out

    def decode_tokens(self, tokens: torch.Tensor, F: int, H: int, W: int, timestep=None, noise: Optional[torch.Tensor] = None,
                      noise_scale=None, postprocess: bool = False) -> torch.Tensor:
        x = _dev(tokens, torch.float32)
        B = x.shape[0]
        t = _floats(list(timestep)) if timestep is not None else None
        ns = _floats(list(noise_scale)) if noise_scale is not None else None
        nz = _dev(noise, torch.float32) if noise is not None else None
        r, tr = self.config.spatial_compression_ratio, self.config.temporal_compression_ratio
        out = torch.empty(B, self.config.out_channels, (F - 1) * tr + 1, H * r, W * r, dtype=torch.float32, device=x.device)
        tl = self._tiling()
        _check(lib.ltx_vae_decode_tokens(self._h, _ptr(x), _ptr(nz), ns, t, B, F, H, W, C.byref(tl) if tl else None,
                                         int(postprocess), _ptr(out), _stream()))
        return out

    def prepare_latents(self, tokens: torch.Tensor, F: int, H: int, W: int, noise: Optional[torch.Tensor] = None,
                        noise_scale=None) -> torch.Tensor:
        """denormalize (+ decode-noise mix) of packed tokens [B,S,C] -> [B,C,F,H,W] f32 (t2v_pipeline.rs:1002-1053)."""
        x = _dev(tokens, torch.float32)
        B = x.shape[0]
        ns = _floats(list(noise_scale)) if noise_scale is not None else None
        nz = _dev(noise, torch.float32) if noise is not None else None
        out = torch.empty_like(x)
        _check(lib.ltx_vae_prepare_latents(self._h, _ptr(x), _ptr(nz), ns, B, F, H, W, _ptr(out), _stream()))
        return out.reshape(B, F, H, W, -1).permute(0, 4, 1, 2, 3).contiguous()

    def latents_mean(self) -> torch.Tensor:
        lib.ltx_vae_latents_mean.restype = C.c_void_p
        p = lib.ltx_vae_latents_mean(self._h)
        out = torch.empty(self.config.latent_channels, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        _hip_memcpy_d2d(out.data_ptr(), p, 4 * self.config.latent_channels)
        return out

    def latents_std(self) -> torch.Tensor:
        lib.ltx_vae_latents_std.restype = C.c_void_p
        p = lib.ltx_vae_latents_std(self._h)
        out = torch.empty(self.config.latent_channels, dtype=torch.float32, device="cuda")
        _hip_memcpy_d2d(out.data_ptr(), p, 4 * self.config.latent_channels)
        return out


def _hip_memcpy_d2d(dst: int, src: int, nbytes: int):
    hip = C.CDLL("libamdhip64.so")
    rc = hip.hipMemcpy(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(nbytes), 3)  # hipMemcpyDeviceToDevice
    if rc != 0:
        raise LtxError(f"hipMemcpy failed rc={rc}")


# ------------------------------------------------------------------ scheduler / host helpers
lib.ltx_calculate_shift.restype = C.c_float


def calculate_shift(seq_len: int, base_seq_len: int = 256, max_seq_len: int = 4096,
                    base_shift: float = 0.5, max_shift: float = 1.15) -> float:
    return float(lib.ltx_calculate_shift(seq_len, base_seq_len, max_seq_len, C.c_float(base_shift), C.c_float(max_shift)))


class FlowMatchEulerDiscreteScheduler:
    """Scheduler trait (t2v_pipeline.rs:28-37) as implemented at scheduler.rs:646-668."""

    def __init__(self, shift: float = 1.0, shift_terminal: Optional[float] = 0.1, stochastic_sampling: bool = False,
                 use_karras_sigmas: bool = False, use_exponential_sigmas: bool = False, use_beta_sigmas: bool = False, invert_sigmas: bool = False):
        if int(use_karras_sigmas) + int(use_exponential_sigmas) + int(use_beta_sigmas) > 1:      # scheduler.rs:85-93
            raise LtxError("Only one of use_beta_sigmas/use_exponential_sigmas/use_karras_sigmas can be enabled.")
        self.shift = shift
        self.shift_terminal = shift_terminal
        self.stochastic_sampling = stochastic_sampling
        self.sigma_kind = 1 if use_karras_sigmas else (2 if use_exponential_sigmas else (3 if use_beta_sigmas else 0))
        self.invert_sigmas = invert_sigmas
        self.sigmas: List[float] = []
        self.timesteps: List[int] = []
        self.step_index = 0

    def set_timesteps(self, sigmas: Sequence[float], mu: Optional[float]) -> List[int]:
        n = len(sigmas)
        sin = _floats(sigmas)
        sout = (C.c_float * (n + 1))()
        tout = (C.c_int64 * n)()
        _check(lib.ltx_sched_set_timesteps_ex(sin, n, C.c_float(mu if mu is not None else 0.0), int(mu is not None),
                                              C.c_float(self.shift), C.c_float(self.shift_terminal or 0.0),
                                              int(self.shift_terminal is not None), self.sigma_kind, int(self.invert_sigmas), sout, tout))
        self.sigmas = list(sout)
        self.timesteps = list(tout)
        self.step_index = 0
        return self.timesteps

    def step(self, noise_pred: torch.Tensor, timestep: int, latents: torch.Tensor, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x + (sigma_next - sigma) * v, or with stochastic_sampling (1 - sigma_next) * (x - sigma * v) + sigma_next * noise
        (`noise` = the randn_like(sample) draw, supplied by the caller); f32, on a copy (scheduler.rs:544-581)."""
        sg, sn = C.c_float(self.sigmas[self.step_index]).value, C.c_float(self.sigmas[self.step_index + 1]).value
        dt = sn - sg
        x = _dev(latents, torch.float32).clone()
        p = _dev(noise_pred)
        B = x.shape[0]
        if self.stochastic_sampling:
            if noise is None:
                raise LtxError("stochastic_sampling: pass the per-step noise (the reference draws randn_like(sample))")
            nz = _dev(noise, torch.float32)
            _check(lib.ltx_guidance_step_stochastic(_ptr(p), None, None, _dt(p.dtype), _ptr(x), None, B, C.c_int64(x[0].numel()),
                                                    C.c_float(1.0), C.c_float(0.0), C.c_float(0.0), C.c_float(sg), C.c_float(sn),
                                                    _ptr(nz), None, _stream()))
            self.step_index += 1
            return x
        _check(lib.ltx_guidance_step(_ptr(p), None, None, _dt(p.dtype), _ptr(x), None, B, C.c_int64(x[0].numel()),
                                     C.c_float(1.0), C.c_float(0.0), C.c_float(0.0), C.c_float(dt), None, _stream()))
        self.step_index += 1
        return x


def guidance_combine(text, uncond=None, perturbed=None, guidance_scale=1.0, guidance_rescale=0.0, stg_scale=0.0):
    """CFG/STG mix of t2v_pipeline.rs:941-964 (returns the f32 combined prediction)."""
    t = _dev(text)
    u = _dev(uncond, t.dtype) if uncond is not None else None
    p = _dev(perturbed, t.dtype) if perturbed is not None else None
    B = t.shape[0]
    out = torch.empty(t.shape, dtype=torch.float32, device=t.device)
    ws = torch.zeros(8 * B, dtype=torch.float64, device=t.device)
    _check(lib.ltx_guidance_step(_ptr(t), _ptr(u), _ptr(p), _dt(t.dtype), None, _ptr(out), B, C.c_int64(t[0].numel()),
                                 C.c_float(guidance_scale), C.c_float(guidance_rescale), C.c_float(stg_scale), C.c_float(0.0),
                                 _ptr(ws), _stream()))
    return out


def _rescale_form(form) -> int:
    if isinstance(form, str):
        if form not in RESCALE_FORMS:
            raise LtxError(f"unknown rescale_form {form!r} (one of {RESCALE_FORMS})")
        return RESCALE_FORMS.index(form)
    return int(form)


def guidance_step_ex(text, latents=None, uncond=None, perturbed=None, guidance_scale=1.0, guidance_rescale=0.0, stg_scale=0.0,
                     cfg_star=False, rescale_form="cfg", dt=0.0, sigma=0.0, sigma_next=0.0, step_noise=None, hold=None, num_frames=None,
                     want_noise_pred=False, want_scalars=False):
    """The mix of include/ltxhip_guidance.h (CFG-star, rescale_form 'cfg' / 'mix') and the scheduler update on a copy of `latents`
    (ltx_guidance_step_ex).  uncond / perturbed None = the branch is absent.  hold [B, num_frames] (device u8 tensor or host values):
    those latent frames keep their bits.  Returns a dict: 'latents' (None without latents), 'noise_pred' f32 (want_noise_pred),
    'scalars' f32 [B, 2] = (alpha, factor) per batch row (want_scalars)."""
    t = _dev(text)
    u = _dev(uncond, t.dtype) if uncond is not None else None
    p = _dev(perturbed, t.dtype) if perturbed is not None else None
    B, n = t.shape[0], t[0].numel()
    x = _dev(latents, torch.float32).clone() if latents is not None else None
    if x is not None and (x.shape[0] != B or x[0].numel() != n):
        raise LtxError("guidance_step_ex: predictions and latents must agree in shape")
    for name, v in (("uncond", u), ("perturbed", p)):
        if v is not None and v.shape != t.shape:
            raise LtxError(f"guidance_step_ex: {name} must have the shape of text")
    nz = _dev(step_noise, torch.float32) if step_noise is not None else None
    if nz is not None and (x is None or nz.numel() != B * n):
        raise LtxError("guidance_step_ex: the stochastic update needs latents and step_noise of their shape")
    hd, nf = None, 1
    if hold is not None:
        if num_frames is None or num_frames < 1 or n % num_frames != 0:
            raise LtxError("guidance_step_ex: hold needs num_frames dividing the per-row element count")
        nf = int(num_frames)
        hd = hold.to(torch.uint8).contiguous() if torch.is_tensor(hold) and hold.is_cuda else torch.tensor(list(_hold_host(hold, B, nf)), dtype=torch.uint8).to(t.device)
        if hd.numel() != B * nf:
            raise LtxError(f"hold must have {B} x {nf} entries")
    out = torch.empty(t.shape, dtype=torch.float32, device=t.device) if want_noise_pred else None
    sc = torch.empty(B, 2, dtype=torch.float32, device=t.device) if want_scalars else None
    ws = torch.empty(max(int(lib.ltx_guidance_ws_bytes(B, C.c_int64(n))), 16) // 8 + 2, dtype=torch.float64, device=t.device)
    _check(lib.ltx_guidance_step_ex(_ptr(t), _ptr(u), _ptr(p), _dt(t.dtype), _ptr(x), _ptr(out), B, C.c_int64(n),
                                    C.c_float(guidance_scale), C.c_float(guidance_rescale), C.c_float(stg_scale), int(bool(cfg_star)), _rescale_form(rescale_form),
                                    C.c_float(dt), C.c_float(sigma), C.c_float(sigma_next), _ptr(nz), _ptr(hd), nf, C.c_int64(n // nf),
                                    _ptr(ws), _ptr(sc), _stream()))
    return {"latents": x, "noise_pred": out, "scalars": sc}


def guidance_combine_ex(text, uncond=None, perturbed=None, guidance_scale=1.0, guidance_rescale=0.0, stg_scale=0.0, cfg_star=False,
                        rescale_form="cfg", want_scalars=False):
    """guidance_combine under include/ltxhip_guidance.h: the f32 combined prediction, or (prediction, scalars [B, 2]) with want_scalars"""
    r = guidance_step_ex(text, None, uncond, perturbed, guidance_scale, guidance_rescale, stg_scale, cfg_star, rescale_form,
                         want_noise_pred=True, want_scalars=want_scalars)
    return (r["noise_pred"], r["scalars"]) if want_scalars else r["noise_pred"]


def pcg32_randn(seed: int, shape: Sequence[int], inc: int = 1442695040888963407) -> torch.Tensor:
    """Pcg32::new(seed, inc).randn(shape) (deterministic_rng.rs; main.rs:568) -> CPU f32 tensor."""
    n = 1
    for s in shape:
        n *= int(s)
    out = torch.empty(n, dtype=torch.float32)
    _check(lib.ltx_pcg32_randn(C.c_uint64(seed), C.c_uint64(inc), C.c_size_t(n), C.c_void_p(out.data_ptr())))
    return out.reshape(*shape)


def pcg32_u32(seed: int, n: int, inc: int = 1442695040888963407) -> torch.Tensor:
    """first n outputs of Pcg32::new(seed, inc).next_u32() as int64 (exact)"""
    import numpy as np
    out = np.empty(n, dtype=np.uint32)
    _check(lib.ltx_pcg32_u32(C.c_uint64(seed), C.c_uint64(inc), C.c_size_t(n), C.c_void_p(out.ctypes.data)))
    return torch.from_numpy(out.astype(np.int64))


def build_video_coords(F: int, H: int, W: int, frame_rate: int = 25, ts_ratio: int = 8, sp_ratio: int = 32) -> torch.Tensor:
    out = torch.empty(F * H * W, 3, dtype=torch.float32)
    _check(lib.ltx_build_video_coords(F, H, W, frame_rate, ts_ratio, sp_ratio, C.c_void_p(out.data_ptr())))
    return out


def pack_latents(x: torch.Tensor) -> torch.Tensor:
    """LtxPipeline::pack_latents with patch sizes 1 (t2v_pipeline.rs:474-504): a pure layout view."""
    b, c, f, h, w = x.shape
    return x.permute(0, 2, 3, 4, 1).reshape(b, f * h * w, c).contiguous()


def cond_apply(latents: torch.Tensor, cond_tokens: torch.Tensor, hold, num_frames: int) -> torch.Tensor:
    """latents[b, f] = cond_tokens[b, f] for the held latent frames (ltx_cond_apply), on a copy.  latents [B, num_frames*hw, C] f32,
    cond_tokens [B, cond_frames*hw, C] f32 (encode_tokens of the image / clip), hold [B, num_frames] truthy = held."""
    lat = _dev(latents, torch.float32).clone()
    ct = _dev(cond_tokens, torch.float32)
    if lat.dim() != 3 or ct.dim() != 3 or lat.shape[0] != ct.shape[0] or lat.shape[2] != ct.shape[2]:
        raise LtxError("cond_apply: latents [B, F*hw, C] and cond_tokens [B, Fc*hw, C] must agree in B and C")
    B, S, Cn = lat.shape
    if num_frames < 1 or S % num_frames != 0 or ct.shape[1] % (S // num_frames) != 0 or ct.shape[1] == 0:
        raise LtxError("cond_apply: token counts must be whole latent frames")
    hw = S // num_frames
    h = _hold_host(hold, B, num_frames)
    _check(lib.ltx_cond_apply(_ptr(lat), _ptr(ct), ct.shape[1] // hw, h, B, num_frames, hw, Cn, _stream()))
    return lat


# ------------------------------------------------------------------ keyframe conditioning (include/ltxhip_keyframes.h)
@dataclass
class ConditioningItem:
    """ltx_cond_item: tokens [B, cond_frames*hw, C] f32 (encode_tokens of an image or clip), the PIXEL frame it sits at, its strength"""
    tokens: Optional[torch.Tensor]
    frame_index: int = 0
    strength: float = 1.0
    cond_frames: Optional[int] = None           # None: tokens.shape[1] // (h*w)


@dataclass
class CondLayout:
    """ltx_cond_layout's result: E extra groups in front of the F' grid frames, G = E + F' groups of hw tokens; groups[g] =
    (item or -1, the item's latent frame, strength); coords [G*hw, 3] of one batch row"""
    E: int
    G: int
    hw: int
    groups: List[tuple]
    coords: torch.Tensor

    def groups_c(self):
        return (CondGroupC * self.G)(*[CondGroupC(i, f, s) for i, f, s in self.groups])


def _items_c(items, hw: int, keep: list, need_tokens: bool):
    arr = (CondItemC * max(len(items), 1))()
    for k, it in enumerate(items):
        fc, t = it.cond_frames, None
        if it.tokens is not None:
            t = _dev(it.tokens, torch.float32); keep.append(t)
            if t.dim() != 3 or t.shape[1] % hw != 0 or (fc is not None and t.shape[1] != fc * hw):
                raise LtxError(f"conditioning item {k}: tokens must be [B, cond_frames*{hw}, C]")
            fc = t.shape[1] // hw
        elif need_tokens or fc is None:
            raise LtxError(f"conditioning item {k}: tokens are required")
        arr[k] = CondItemC(C.cast(C.c_void_p(t.data_ptr() if t is not None else None), C.POINTER(C.c_float)), int(fc), int(it.frame_index), float(it.strength))
    return arr


def cond_layout(items: Sequence[ConditioningItem], height: int, width: int, num_frames: int, frame_rate: int = 25,
                ts_ratio: int = 8, sp_ratio: int = 32) -> CondLayout:
    """ltx_cond_layout: where the items go (host only; an item needs tokens or cond_frames).  Raises LtxError on every refusal."""
    hw = (height // sp_ratio) * (width // sp_ratio)
    keep = []
    arr = _items_c(items, max(hw, 1), keep, False)
    E, G = C.c_int(0), C.c_int(0)
    _check(lib.ltx_cond_layout(arr, len(items), height, width, num_frames, frame_rate, ts_ratio, sp_ratio, C.byref(E), C.byref(G), None, 0, None))
    groups = (CondGroupC * G.value)()
    coords = torch.empty(G.value * hw, 3, dtype=torch.float32)
    _check(lib.ltx_cond_layout(arr, len(items), height, width, num_frames, frame_rate, ts_ratio, sp_ratio, C.byref(E), C.byref(G), groups, G.value,
                               C.c_void_p(coords.data_ptr())))
    return CondLayout(E.value, G.value, hw, [(g.item, g.item_frame, g.strength) for g in groups], coords)


def cond_place(latents: torch.Tensor, items: Sequence[ConditioningItem], layout: CondLayout) -> torch.Tensor:
    """ltx_cond_place on a copy: latents [B, G*hw, C] f32 (the caller's noise); a placed group becomes a + s*(b - a)"""
    lat = _dev(latents, torch.float32).clone()
    if lat.dim() != 3 or lat.shape[1] != layout.G * layout.hw:
        raise LtxError(f"cond_place: latents must be [B, {layout.G * layout.hw}, C]")
    keep = []
    arr = _items_c(items, layout.hw, keep, True)
    for k, t in enumerate(keep):
        if t.shape[0] != lat.shape[0] or t.shape[2] != lat.shape[2] or t.device != lat.device:
            raise LtxError(f"cond_place: item {k} must agree with latents in B, C and device")
    _check(lib.ltx_cond_place(_ptr(lat), arr, len(items), layout.groups_c(), layout.G, lat.shape[0], layout.hw, lat.shape[2], _stream()))
    return lat


def cond_noise(latents: torch.Tensor, clean: torch.Tensor, noise: torch.Tensor, layout: CondLayout, scale: float, sigma: float) -> torch.Tensor:
    """ltx_cond_noise on a copy: the groups of full strength become clean + scale*sigma^2*noise; all three [B, G*hw, C] f32"""
    lat = _dev(latents, torch.float32).clone()
    cl, nz = _dev(clean, torch.float32), _dev(noise, torch.float32)
    if lat.dim() != 3 or lat.shape[1] != layout.G * layout.hw or cl.shape != lat.shape or nz.shape != lat.shape:
        raise LtxError(f"cond_noise: latents, clean and noise must be [B, {layout.G * layout.hw}, C]")
    _check(lib.ltx_cond_noise(_ptr(lat), _ptr(cl), _ptr(nz), layout.groups_c(), layout.G, lat.shape[0], layout.hw, lat.shape[2], float(scale), float(sigma), _stream()))
    return lat


def cond_step_hold(layout: CondLayout, sigma: float, timestep: float = 0.0):
    """ltx_cond_step_hold: ([G] 1 = the group keeps its bits on a step of `sigma`, [G] what the model sees at scheduler timestep `timestep`)"""
    hold = (C.c_ubyte * layout.G)()
    tm = (C.c_float * layout.G)()
    _check(lib.ltx_cond_step_hold(layout.groups_c(), layout.G, float(sigma), float(timestep), hold, tm))
    return list(hold), list(tm)


# ------------------------------------------------------------------ pipeline
@dataclass
class PipelineCall:
    height: int = 512
    width: int = 768
    num_frames: int = 97
    frame_rate: int = 25
    num_inference_steps: int = 7
    sigmas: Optional[List[float]] = None
    guidance_scale: float = 1.0
    guidance_rescale: float = 0.0
    stg_scale: float = 0.0
    skip_block_list: Optional[List[int]] = None
    decode_timestep: float = 0.05
    decode_noise_scale: float = 0.025
    output_latent: bool = False
    postprocess: bool = True
    output_rgb8: bool = False                   # the video as u8 frames [B, frames, H, W, 3] (ltx_pipeline_params::postprocess = 2; main.rs:653-675)
    shift_terminal: Optional[float] = 0.1
    stochastic_sampling: bool = False           # SchedulerConfig::stochastic_sampling (0.9.6-distilled preset)


class LtxPipeline:
    """LtxPipeline (t2v_pipeline.rs:245-302) holding the two boxed components that matter here."""

    def __init__(self, transformer: LtxVideoTransformer3DModel, vae: Optional[AutoencoderKLLtxVideo]):
        self.transformer = transformer
        self.vae = vae
        self.last_timing_ms = (0.0, 0.0, 0.0, 0.0)

    def call(self, args: PipelineCall, latents: torch.Tensor, prompt_embeds: torch.Tensor, prompt_attention_mask: torch.Tensor,
             negative_prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_attention_mask: Optional[torch.Tensor] = None,
             decode_noise: Optional[torch.Tensor] = None, step_noise: Optional[torch.Tensor] = None,
             interrupt=None, on_step=None, hold=None, schedule: Optional["GuidanceSchedule"] = None,
             conditioning_items: Optional[Sequence["ConditioningItem"]] = None, image_cond_noise_scale: float = 0.0,
             cond_noise: Optional[torch.Tensor] = None):
        """Returns (final_latents [B,S,C] f32, video [B,3,frames,H,W] f32 or None).
        conditioning_items: keyframe conditioning (ltx_pipeline_call_keyframes, with `schedule` or without; not with `hold`) - `latents`
        is the caller's noise for the EXTENDED sequence [B, G*hw, C] of cond_layout(conditioning_items, ...), step_noise covers it too,
        the returned latents are the extended ones (the grid tokens start at token E*hw of a row) and the video has the plain call's
        shape.  image_cond_noise_scale > 0 with cond_noise [steps, B, G*hw, C]: the noised holds of full-strength items.
        schedule: a GuidanceSchedule (ltx_pipeline_call_sched, with `hold` or without) - the guidance of every step comes from it and
        the scalar guidance fields and skip_block_list of `args` are ignored.
        hold [B, F'] (truthy = held): image-to-video / clip continuation (ltx_pipeline_call_cond) - `latents` carries the held
        latent frames already (cond_apply); they see timestep 0 and leave the call unchanged.
        step_noise [steps,B,S,C] f32: the per-step draws of the stochastic-sampling scheduler (required iff enabled).
        interrupt: a ctypes.c_int the caller may set from another thread (LtxPipeline::interrupt, t2v_pipeline.rs:266, 861-863);
        on_step(step, num_steps, timestep) -> truthy to stop: the per-step hook.  self.last_steps = (executed, requested)."""
        lat = _dev(latents, torch.float32).clone()
        pe = _dev(prompt_embeds, torch.float32)
        pm = _dev(prompt_attention_mask, torch.float32)
        ne = _dev(negative_prompt_embeds, torch.float32) if negative_prompt_embeds is not None else None
        nm = _dev(negative_prompt_attention_mask, torch.float32) if negative_prompt_attention_mask is not None else None
        dn = _dev(decode_noise, torch.float32) if decode_noise is not None else None
        if pe.dim() != 3 or lat.dim() != 3:
            raise LtxError("latents must be [B, F*H*W, in_channels] and prompt_embeds [B, K, caption_channels]")
        B, K = pe.shape[0], pe.shape[1]
        # latent geometry as LtxPipeline::call derives it (t2v_pipeline.rs:743-747), checked against every tensor handed over:
        # the C entry takes raw pointers, a mismatch would be out-of-bounds device traffic
        tr = self.vae.config.temporal_compression_ratio if self.vae is not None else 8
        sr = self.vae.config.spatial_compression_ratio if self.vae is not None else 32
        F, H, W = (args.num_frames - 1) // tr + 1, args.height // sr, args.width // sr
        Cin = self.transformer.config.in_channels
        S_seq = F * H * W
        if conditioning_items is not None:
            if hold is not None:
                raise LtxError("conditioning_items and hold exclude each other (an item at frame 0 with strength 1 is a held frame)")
            layout = cond_layout(conditioning_items, args.height, args.width, args.num_frames, args.frame_rate, tr, sr)
            S_seq = layout.G * H * W
        _expect("latents", lat, (B, S_seq, Cin))
        _expect("prompt_embeds", pe, (B, K, self.transformer.config.caption_channels))
        _expect("prompt_attention_mask", pm, (B, K))
        if ne is not None: _expect("negative_prompt_embeds", ne, (B, K, self.transformer.config.caption_channels))
        if nm is not None: _expect("negative_prompt_attention_mask", nm, (B, K))
        if dn is not None: _expect("decode_noise", dn, (B, Cin, F, H, W))
        if step_noise is not None: _expect("step_noise", step_noise, (args.num_inference_steps, B, S_seq, Cin))
        keep = []
        p = _params_c(args, self.vae, keep, step_noise)
        if interrupt is not None:
            p.interrupt = C.pointer(interrupt)
        hook_exc = _step_hook(on_step, keep, p)
        video = None
        if not args.output_latent:
            if self.vae is None:
                raise LtxError("decode requested but the pipeline has no VAE")
            # the decoder's own output shape (vae.rs:2101-2136): (F-1)*tr+1 frames, which is num_frames only for tr*k+1
            if args.output_rgb8:
                video = torch.empty(B, (F - 1) * tr + 1, H * sr, W * sr, 3, dtype=torch.uint8, device=lat.device)
            else:
                video = torch.empty(B, 3, (F - 1) * tr + 1, H * sr, W * sr, dtype=torch.float32, device=lat.device)
        if conditioning_items is not None:
            items_c = _items_c(conditioning_items, H * W, keep, True)
            for k, t in enumerate(keep[-len(conditioning_items):] if conditioning_items else []):
                if t.shape[0] != B or t.shape[2] != Cin or t.device != lat.device:
                    raise LtxError(f"conditioning item {k}: tokens must be [{B}, cond_frames*{H * W}, {Cin}] on the latents' device")
            cn = None
            if image_cond_noise_scale > 0.0:
                if cond_noise is None:
                    raise LtxError("image_cond_noise_scale > 0 needs cond_noise [steps, B, S_ext, C]")
                cn = _dev(cond_noise, torch.float32); keep.append(cn)
                _expect("cond_noise", cn, (args.num_inference_steps, B, S_seq, Cin))
            sched = schedule.to_c(keep) if schedule is not None else None
            _check(lib.ltx_pipeline_call_keyframes(self.transformer._h, self.vae._h if self.vae is not None else None, C.byref(p),
                                                   C.byref(sched) if sched is not None else None, items_c, len(conditioning_items),
                                                   float(image_cond_noise_scale), _ptr(cn), _ptr(lat), _ptr(pe), _ptr(pm), _ptr(ne), _ptr(nm), _ptr(dn), B, K,
                                                   _ptr(video), _stream()))
        elif schedule is not None:
            sched = schedule.to_c(keep)
            cond = None
            if hold is not None:
                hh = _hold_host(hold, B, F); keep.append(hh)
                cond = ConditioningC(C.cast(hh, C.POINTER(C.c_ubyte)))
            _check(lib.ltx_pipeline_call_sched(self.transformer._h, self.vae._h if self.vae is not None else None, C.byref(p), C.byref(sched),
                                               C.byref(cond) if cond is not None else None, _ptr(lat), _ptr(pe), _ptr(pm), _ptr(ne), _ptr(nm), _ptr(dn), B, K,
                                               _ptr(video), _stream()))
        elif hold is not None:
            hh = _hold_host(hold, B, F); keep.append(hh)
            cond = ConditioningC(C.cast(hh, C.POINTER(C.c_ubyte)))
            _check(lib.ltx_pipeline_call_cond(self.transformer._h, self.vae._h if self.vae is not None else None, C.byref(p), C.byref(cond),
                                              _ptr(lat), _ptr(pe), _ptr(pm), _ptr(ne), _ptr(nm), _ptr(dn), B, K,
                                              _ptr(video), _stream()))
        else:
            _check(lib.ltx_pipeline_call(self.transformer._h, self.vae._h if self.vae is not None else None, C.byref(p),
                                         _ptr(lat), _ptr(pe), _ptr(pm), _ptr(ne), _ptr(nm), _ptr(dn), B, K,
                                         _ptr(video), _stream()))
        ms = (C.c_float * 4)()
        _check(lib.ltx_pipeline_last_timing(ms))
        self.last_timing_ms = tuple(ms)
        ex, rq = C.c_int(0), C.c_int(0)
        _check(lib.ltx_pipeline_last_steps(C.byref(ex), C.byref(rq)))
        self.last_steps = (ex.value, rq.value)
        if hook_exc:
            raise hook_exc[0]
        return lat, video


# ------------------------------------------------------------------ step cache (include/ltxhip_stepcache.h)
class StepCache:
    """ltx_step_cache: `rows` cache rows for forwards of `model` (the pipeline call uses 3 * B, one set per guidance branch)"""

    def __init__(self, model: LtxVideoTransformer3DModel, rows: int):
        self.model = model
        self.rows = rows
        self._h = C.c_void_p()
        _check(lib.ltx_step_cache_create(model._h, int(rows), C.byref(self._h)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:
            lib.ltx_step_cache_destroy(h)
            self._h = None

    def reset(self):
        _check(lib.ltx_step_cache_reset(self._h))

    def decide(self, hidden_states: torch.Tensor, timestep, num_frames: int, height: int, width: int, step: int, n_steps: int,
               params: StepCacheParams, frames: bool = False):
        """the measurement and the decision of a step for hidden_states [B, S, C] -> (reuse, distance); frames: timestep [B, num_frames]"""
        io = hidden_states.dtype if hidden_states.dtype in (torch.float32, torch.bfloat16) else torch.float32
        h = _dev(hidden_states, io)
        B, S, _ = h.shape
        t = torch.as_tensor(timestep, dtype=torch.float32).detach().flatten().cpu().tolist()
        if len(t) != B * (num_frames if frames else 1):
            raise LtxError(f"timestep must have {B}{' x ' + str(num_frames) if frames else ''} entries")
        keep = []
        pc = params.to_c(keep)
        reuse, dist = C.c_int(0), C.c_float(0.0)
        _check(lib.ltx_step_cache_decide(self._h, self.model._h, _ptr(h), _floats(t), int(frames), B, S, num_frames, height, width, _dt(io),
                                         int(step), int(n_steps), C.byref(pc), C.byref(reuse), C.byref(dist), _stream()))
        return bool(reuse.value), dist.value

    def require(self, row0: int, nrows: int, S: int, reuse: bool) -> bool:
        """reuse, demoted to compute when one of the rows holds no residual for S (ltx_step_cache_require)"""
        r = C.c_int(int(reuse))
        _check(lib.ltx_step_cache_require(self._h, self.model._h, int(row0), int(nrows), int(S), C.byref(r)))
        return bool(r.value)

    def read_residual(self, row: int, S: int) -> torch.Tensor:
        """the residual of a cache row as f32 [S, D]"""
        D = self.model.config.num_attention_heads * self.model.config.attention_head_dim
        out = torch.empty(S, D, dtype=torch.float32, device="cuda")
        _check(lib.ltx_step_cache_read_residual(self._h, int(row), _ptr(out), _stream()))
        return out


def dit_forward_cached(model: LtxVideoTransformer3DModel, cache: StepCache, row0: int, reuse: bool, hidden_states: torch.Tensor,
                       encoder_hidden_states: Optional[torch.Tensor], timestep, encoder_attention_mask: Optional[torch.Tensor],
                       num_frames: int, height: int, width: int, rope_interpolation_scale=None, video_coords: Optional[torch.Tensor] = None,
                       skip_layer_mask: Optional[torch.Tensor] = None, frames: bool = False, K: Optional[int] = None) -> torch.Tensor:
    """model.forward (frames: model.forward_frames, timestep [B, num_frames]) through cache rows [row0, row0 + B)
    (ltx_dit_forward_cached).  reuse: the blocks are not run; encoder_hidden_states may then be None (K: its token count)."""
    io = hidden_states.dtype if hidden_states.dtype in (torch.float32, torch.bfloat16) else torch.float32
    h = _dev(hidden_states, io)
    e = _dev(encoder_hidden_states, io) if encoder_hidden_states is not None else None
    B, S, _ = h.shape
    K = e.shape[1] if e is not None else int(K or 1)
    t = torch.as_tensor(timestep, dtype=torch.float32).detach().flatten().cpu().tolist()
    if len(t) != B * (num_frames if frames else 1):
        raise LtxError(f"timestep must have {B}{' x ' + str(num_frames) if frames else ''} entries")
    m = _dev(encoder_attention_mask, torch.float32) if encoder_attention_mask is not None else None
    vc = _dev(video_coords, torch.float32) if video_coords is not None else None
    if getattr(model, "_ctx_cache", False) and ((e is not None and e.data_ptr() != encoder_hidden_states.data_ptr()) or (m is not None and m.data_ptr() != encoder_attention_mask.data_ptr())
                                                or (vc is not None and vc.data_ptr() != video_coords.data_ptr())):
        raise LtxError("context_cache(True) needs encoder_hidden_states / encoder_attention_mask / video_coords that are already contiguous "
                       "device tensors of the dtype the call uses: a temporary copy has no stable identity")
    slm = _floats(skip_layer_mask.detach().float().cpu().flatten().tolist()) if skip_layer_mask is not None else None
    rs = _floats(rope_interpolation_scale) if rope_interpolation_scale is not None else None
    out = torch.empty(B, S, model.config.out_channels, dtype=io, device=h.device)
    _check(lib.ltx_dit_forward_cached(model._h, cache._h, int(row0), int(bool(reuse)), int(frames), _ptr(h), _ptr(e), _floats(t), _ptr(m), B, S, K,
                                      num_frames, height, width, rs, _ptr(vc), slm, _dt(io), _ptr(out), _stream()))
    return out


def pipeline_call_cached(pipe: "LtxPipeline", args: PipelineCall, params: StepCacheParams, latents: torch.Tensor, prompt_embeds: torch.Tensor,
                         prompt_attention_mask: torch.Tensor, negative_prompt_embeds: Optional[torch.Tensor] = None,
                         negative_prompt_attention_mask: Optional[torch.Tensor] = None, decode_noise: Optional[torch.Tensor] = None,
                         step_noise: Optional[torch.Tensor] = None, hold=None, schedule: Optional["GuidanceSchedule"] = None):
    """LtxPipeline.call (plain, with `hold`, with `schedule`) under the step cache (ltx_pipeline_call_cached)
    -> (latents, video or None, reused [N] list of bool, distance [N] list of float).  pipe.last_timing_ms is updated."""
    lat = _dev(latents, torch.float32).clone()
    pe = _dev(prompt_embeds, torch.float32)
    pm = _dev(prompt_attention_mask, torch.float32)
    ne = _dev(negative_prompt_embeds, torch.float32) if negative_prompt_embeds is not None else None
    nm = _dev(negative_prompt_attention_mask, torch.float32) if negative_prompt_attention_mask is not None else None
    dn = _dev(decode_noise, torch.float32) if decode_noise is not None else None
    if pe.dim() != 3 or lat.dim() != 3:
        raise LtxError("latents must be [B, F*H*W, in_channels] and prompt_embeds [B, K, caption_channels]")
    B, K = pe.shape[0], pe.shape[1]
    tr = pipe.vae.config.temporal_compression_ratio if pipe.vae is not None else 8
    sr = pipe.vae.config.spatial_compression_ratio if pipe.vae is not None else 32
    F, H, W = (args.num_frames - 1) // tr + 1, args.height // sr, args.width // sr
    Cin, Ccap = pipe.transformer.config.in_channels, pipe.transformer.config.caption_channels
    _expect("latents", lat, (B, F * H * W, Cin))
    _expect("prompt_embeds", pe, (B, K, Ccap))
    _expect("prompt_attention_mask", pm, (B, K))
    if ne is not None: _expect("negative_prompt_embeds", ne, (B, K, Ccap))
    if nm is not None: _expect("negative_prompt_attention_mask", nm, (B, K))
    if dn is not None: _expect("decode_noise", dn, (B, Cin, F, H, W))
    if step_noise is not None: _expect("step_noise", step_noise, (args.num_inference_steps, B, F * H * W, Cin))
    keep = []
    p = _params_c(args, pipe.vae, keep, step_noise)
    pc = params.to_c(keep)
    video = None
    if not args.output_latent:
        if pipe.vae is None:
            raise LtxError("decode requested but the pipeline has no VAE")
        if args.output_rgb8:
            video = torch.empty(B, (F - 1) * tr + 1, H * sr, W * sr, 3, dtype=torch.uint8, device=lat.device)
        else:
            video = torch.empty(B, 3, (F - 1) * tr + 1, H * sr, W * sr, dtype=torch.float32, device=lat.device)
    sched = schedule.to_c(keep) if schedule is not None else None
    cond = None
    if hold is not None:
        hh = _hold_host(hold, B, F); keep.append(hh)
        cond = ConditioningC(C.cast(hh, C.POINTER(C.c_ubyte)))
    N = args.num_inference_steps
    reused, dist = (C.c_ubyte * max(N, 1))(), (C.c_float * max(N, 1))()
    _check(lib.ltx_pipeline_call_cached(pipe.transformer._h, pipe.vae._h if pipe.vae is not None else None, C.byref(p),
                                        C.byref(sched) if sched is not None else None, C.byref(cond) if cond is not None else None, C.byref(pc),
                                        _ptr(lat), _ptr(pe), _ptr(pm), _ptr(ne), _ptr(nm), _ptr(dn), B, K, _ptr(video), _stream(), reused, dist))
    ms = (C.c_float * 4)()
    _check(lib.ltx_pipeline_last_timing(ms))
    pipe.last_timing_ms = tuple(ms)
    return lat, video, [bool(v) for v in reused][:N], list(dist)[:N]


# ------------------------------------------------------------------ latent upsampler + two-pass call (include/ltxhip_upsampler.h)
@dataclass
class LatentUpsamplerConfig:
    in_channels: int = 128
    mid_channels: int = 512
    num_blocks_per_stage: int = 4
    spatial_upsample: bool = True         # (True, False): the spatial kind of ltxhip_upsampler.h; the others: ltxhip_upsampler_st.h
    temporal_upsample: bool = False

    def to_c(self) -> "UpsamplerConfigC":
        return UpsamplerConfigC(self.in_channels, self.mid_channels, self.num_blocks_per_stage)

    def to_st_c(self) -> "UpsamplerStConfigC":
        return UpsamplerStConfigC(self.in_channels, self.mid_channels, self.num_blocks_per_stage, int(self.spatial_upsample), int(self.temporal_upsample))

    @property
    def is_spatial_kind(self) -> bool:
        return bool(self.spatial_upsample) and not self.temporal_upsample


class LatentUpsampler:
    """The latent upsampler over ltx_upsampler_*: spatial (H, W x2), temporal (F -> 2F - 1) or both, by the config's two flags; weight
    names as in the headers.  The spatial kind goes through the constructors of ltxhip_upsampler.h, the others through the _st ones."""

    def __init__(self, config: LatentUpsamplerConfig, weights: Dict[str, torch.Tensor], dtype: torch.dtype = torch.bfloat16, device: int = 0):
        self.config, self.dtype = config, dtype
        c = config.to_c()
        arr, keep = _make_weights(weights)
        self._h = C.c_void_p()
        if config.is_spatial_kind:
            _check(lib.ltx_upsampler_create(C.byref(c), arr, C.c_size_t(len(weights)), _dt(dtype), device, C.byref(self._h)))
        else:
            cs = config.to_st_c()
            _check(lib.ltx_upsampler_create_st(C.byref(cs), arr, C.c_size_t(len(weights)), _dt(dtype), device, C.byref(self._h)))
        del keep

    @classmethod
    def from_file(cls, config: LatentUpsamplerConfig, path: str, dtype: torch.dtype = torch.bfloat16, device: int = 0) -> "LatentUpsampler":
        self = cls.__new__(cls)
        self.config, self.dtype = config, dtype
        c = config.to_c()
        self._h = C.c_void_p()
        if config.is_spatial_kind:
            _check(lib.ltx_upsampler_create_from_file(C.byref(c), path.encode(), _dt(dtype), device, C.byref(self._h)))
        else:
            cs = config.to_st_c()
            _check(lib.ltx_upsampler_create_from_file_st(C.byref(cs), path.encode(), _dt(dtype), device, C.byref(self._h)))
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:
            lib.ltx_upsampler_destroy(h)
            self._h = None

    def get_config(self) -> "UpsamplerConfigC":
        c = UpsamplerConfigC()
        _check(lib.ltx_upsampler_get_config(self._h, C.byref(c)))
        return c

    def get_st_config(self) -> "UpsamplerStConfigC":
        c = UpsamplerStConfigC()
        _check(lib.ltx_upsampler_get_st_config(self._h, C.byref(c)))
        return c

    def out_shape(self, F: int, H: int, W: int) -> Tuple[int, int, int]:
        """the latent grid (Fo, Ho, Wo) this handle maps (F, H, W) to (ltx_upsampler_out_shape; host only)"""
        fo, ho, wo = C.c_int(), C.c_int(), C.c_int()
        _check(lib.ltx_upsampler_out_shape(self._h, int(F), int(H), int(W), C.byref(fo), C.byref(ho), C.byref(wo)))
        return fo.value, ho.value, wo.value

    def forward(self, latents: torch.Tensor) -> torch.Tensor:
        """[B, in_channels, F, H, W] (f32 or bf16, un-normalised) -> [B, in_channels, *out_shape(F, H, W)] of the same dtype"""
        io = latents.dtype if latents.dtype in (torch.float32, torch.bfloat16) else torch.float32
        z = _dev(latents, io)
        if z.dim() != 5 or z.shape[1] != self.config.in_channels:
            raise LtxError("latents must be [B, in_channels, F, H, W]")
        B, Cn, F, H, W = z.shape
        out = torch.empty(B, Cn, *self.out_shape(F, H, W), dtype=io, device=z.device)
        _check(lib.ltx_upsampler_forward(self._h, _ptr(z), _dt(io), B, F, H, W, _ptr(out), _stream()))
        return out

    def upsample_tokens(self, vae: "AutoencoderKLLtxVideo", tokens: torch.Tensor, F: int, H: int, W: int) -> torch.Tensor:
        """packed normalised tokens [B, F*H*W, C] f32 -> [B, Fo*Ho*Wo, C] f32 (un-normalise, forward, normalise)"""
        t = _dev(tokens, torch.float32)
        B = t.shape[0]
        _expect("tokens", t, (B, F * H * W, self.config.in_channels))
        fo, ho, wo = self.out_shape(F, H, W)
        out = torch.empty(B, fo * ho * wo, self.config.in_channels, dtype=torch.float32, device=t.device)
        _check(lib.ltx_latent_upsample_tokens(self._h, vae._h, _ptr(t), B, F, H, W, _ptr(out), _stream()))
        return out

    def warmup(self, B: int, F: int, H: int, W: int):
        _check(lib.ltx_upsampler_warmup(self._h, B, F, H, W, _stream()))


def latent_adain(tokens: torch.Tensor, ref_tokens: torch.Tensor, factor: float = 1.0) -> torch.Tensor:
    """AdaIN of tokens [B,S,C] against ref_tokens [B,S_ref,C] (ltx_latent_adain); returns a new tensor"""
    t = _dev(tokens, torch.float32).clone()
    r = _dev(ref_tokens, torch.float32)
    if t.dim() != 3 or r.dim() != 3 or t.shape[0] != r.shape[0] or t.shape[2] != r.shape[2]:
        raise LtxError("tokens [B,S,C] and ref_tokens [B,S_ref,C] must agree on B and C")
    _check(lib.ltx_latent_adain(_ptr(t), _ptr(r), t.shape[0], t.shape[1], r.shape[1], t.shape[2], float(factor), _stream()))
    return t


def latent_renoise(tokens: torch.Tensor, noise: torch.Tensor, sigma: float) -> torch.Tensor:
    """(1 - sigma) * tokens + sigma * noise (ltx_latent_renoise); returns a new tensor"""
    t = _dev(tokens, torch.float32).clone()
    n = _dev(noise, torch.float32)
    _expect("noise", n, t.shape)
    _check(lib.ltx_latent_renoise(_ptr(t), _ptr(n), float(sigma), C.c_size_t(t.numel()), _stream()))
    return t


def _params_c(args: "PipelineCall", vae, keep: list, step_noise: Optional[torch.Tensor] = None) -> "PipelineParamsC":
    """PipelineCall -> ltx_pipeline_params (the buffers it points at are appended to `keep`)"""
    p = PipelineParamsC()
    lib.ltx_pipeline_params_default(C.byref(p))
    p.height, p.width, p.num_frames, p.frame_rate = args.height, args.width, args.num_frames, args.frame_rate
    p.num_inference_steps = args.num_inference_steps
    if args.sigmas is not None:
        s = _floats(args.sigmas); keep.append(s)
        p.sigmas = C.cast(s, C.POINTER(C.c_float))
    p.guidance_scale, p.guidance_rescale, p.stg_scale = args.guidance_scale, args.guidance_rescale, args.stg_scale
    if args.skip_block_list is not None:
        sb = (C.c_int * max(len(args.skip_block_list), 1))(*args.skip_block_list); keep.append(sb)
        p.skip_block_list = C.cast(sb, C.POINTER(C.c_int))
        p.n_skip_blocks = len(args.skip_block_list)
    p.decode_timestep, p.decode_noise_scale = args.decode_timestep, args.decode_noise_scale
    p.output_latent, p.postprocess = int(args.output_latent), (2 if args.output_rgb8 else int(args.postprocess))
    p.shift_terminal = args.shift_terminal if args.shift_terminal is not None else 0.0
    p.use_shift_terminal = int(args.shift_terminal is not None)
    if args.stochastic_sampling:
        if step_noise is None:
            raise LtxError("stochastic_sampling needs step_noise [steps,B,S,C]")
        sn = _dev(step_noise, torch.float32); keep.append(sn)
        p.stochastic_sampling = 1
        p.step_noise = C.cast(C.c_void_p(sn.data_ptr()), C.POINTER(C.c_float))
    tl = vae._tiling() if vae is not None else None
    if tl is not None:
        keep.append(tl)
        p.tiling = C.pointer(tl)
    return p


def _step_hook(on_step, keep: list, *params) -> list:
    """on_step(step, num_steps, timestep) as the per-step hook of every params struct given -> the list an exception of the hook lands in
    (it never unwinds through the C frame: the loop stops, the caller re-raises after the call)"""
    hook_exc = []
    if on_step is not None:
        def _hook(_user, step, num_steps, timestep):
            try:
                return 1 if on_step(step, num_steps, timestep) else 0
            except BaseException as exc:
                hook_exc.append(exc)
                return 1
        cb = StepFn(_hook); keep.append(cb)
        for p in params:
            p.on_step = C.cast(cb, C.c_void_p)
    return hook_exc


def pipeline_first_sigma(args: "PipelineCall", S: int) -> float:
    """the first sigma LtxPipeline.call(args) runs at S latent tokens (ltx_pipeline_first_sigma)"""
    if args.stochastic_sampling:
        raise LtxError("the multi-scale call runs the deterministic scheduler")
    keep = []
    p = _params_c(args, None, keep)
    out = C.c_float(0.0)
    _check(lib.ltx_pipeline_first_sigma(C.byref(p), int(S), C.byref(out)))
    return out.value


class LtxMultiScalePipeline:
    """first pass -> latent upsampler -> AdaIN -> re-noise -> second pass (ltx_pipeline_call_multiscale)"""

    def __init__(self, transformer: LtxVideoTransformer3DModel, vae: AutoencoderKLLtxVideo, upsampler: LatentUpsampler):
        self.transformer, self.vae, self.upsampler = transformer, vae, upsampler
        self.last_timing_ms = (0.0,) * 9

    def call(self, first: PipelineCall, second: PipelineCall, latents_lo: torch.Tensor, noise_hi: torch.Tensor,
             prompt_embeds: torch.Tensor, prompt_attention_mask: torch.Tensor,
             negative_prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_attention_mask: Optional[torch.Tensor] = None,
             decode_noise: Optional[torch.Tensor] = None, adain_factor: float = 1.0, interrupt=None, on_step=None,
             schedule: Optional["GuidanceSchedule"] = None, schedule_second: Optional["GuidanceSchedule"] = None):
        """schedule / schedule_second: a GuidanceSchedule for the first / second pass (ltx_pipeline_call_multiscale_sched); a pass
        without one runs on its PipelineCall's scalars.
        Returns (first-pass latents [B,S,C], second-pass latents [B,Fo*Ho*Wo,C] (4S for the spatial kind), video or None).  interrupt / on_step as LtxPipeline.call;
        both passes see them."""
        lo = _dev(latents_lo, torch.float32).clone()
        nh = _dev(noise_hi, torch.float32)
        pe = _dev(prompt_embeds, torch.float32)
        pm = _dev(prompt_attention_mask, torch.float32)
        ne = _dev(negative_prompt_embeds, torch.float32) if negative_prompt_embeds is not None else None
        nm = _dev(negative_prompt_attention_mask, torch.float32) if negative_prompt_attention_mask is not None else None
        dn = _dev(decode_noise, torch.float32) if decode_noise is not None else None
        if pe.dim() != 3 or lo.dim() != 3:
            raise LtxError("latents must be [B, F*H*W, in_channels] and prompt_embeds [B, K, caption_channels]")
        B, K = pe.shape[0], pe.shape[1]
        tr, sr = self.vae.config.temporal_compression_ratio, self.vae.config.spatial_compression_ratio
        F, H, W = (first.num_frames - 1) // tr + 1, first.height // sr, first.width // sr
        Cin = self.transformer.config.in_channels
        S = F * H * W
        Fo, Ho, Wo = self.upsampler.out_shape(F, H, W)
        S_hi = Fo * Ho * Wo
        # the C entry takes raw pointers: every tensor is checked against the geometry first
        _expect("latents_lo", lo, (B, S, Cin))
        _expect("noise_hi", nh, (B, S_hi, Cin))
        _expect("prompt_embeds", pe, (B, K, self.transformer.config.caption_channels))
        _expect("prompt_attention_mask", pm, (B, K))
        if ne is not None: _expect("negative_prompt_embeds", ne, (B, K, self.transformer.config.caption_channels))
        if nm is not None: _expect("negative_prompt_attention_mask", nm, (B, K))
        if dn is not None: _expect("decode_noise", dn, (B, Cin, Fo, Ho, Wo))
        if first.stochastic_sampling or second.stochastic_sampling:
            raise LtxError("the multi-scale call runs the deterministic scheduler")
        keep = []
        p1, p2 = _params_c(first, self.vae, keep), _params_c(second, self.vae, keep)
        for p in (p1, p2):
            if interrupt is not None:
                p.interrupt = C.pointer(interrupt)
        hook_exc = _step_hook(on_step, keep, p1, p2)
        hi = torch.empty(B, S_hi, Cin, dtype=torch.float32, device=lo.device)
        video = None
        if not second.output_latent:
            if second.output_rgb8:
                video = torch.empty(B, (Fo - 1) * tr + 1, Ho * sr, Wo * sr, 3, dtype=torch.uint8, device=lo.device)
            else:
                video = torch.empty(B, 3, (Fo - 1) * tr + 1, Ho * sr, Wo * sr, dtype=torch.float32, device=lo.device)
        if schedule is not None or schedule_second is not None:
            s1 = schedule.to_c(keep) if schedule is not None else None
            s2 = schedule_second.to_c(keep) if schedule_second is not None else None
            _check(lib.ltx_pipeline_call_multiscale_sched(self.transformer._h, self.vae._h, self.upsampler._h, C.byref(p1), C.byref(p2),
                                                          C.byref(s1) if s1 is not None else None, C.byref(s2) if s2 is not None else None, float(adain_factor),
                                                          _ptr(lo), _ptr(nh), _ptr(pe), _ptr(pm), _ptr(ne), _ptr(nm), _ptr(dn), B, K,
                                                          _ptr(hi), _ptr(video), _stream()))
        else:
            _check(lib.ltx_pipeline_call_multiscale(self.transformer._h, self.vae._h, self.upsampler._h, C.byref(p1), C.byref(p2), float(adain_factor),
                                                    _ptr(lo), _ptr(nh), _ptr(pe), _ptr(pm), _ptr(ne), _ptr(nm), _ptr(dn), B, K,
                                                    _ptr(hi), _ptr(video), _stream()))
        ms = (C.c_float * 9)()
        _check(lib.ltx_pipeline_multiscale_last_timing(ms))
        self.last_timing_ms = tuple(ms)
        if hook_exc:
            raise hook_exc[0]
        return lo, hi, video


# ------------------------------------------------------------------ version presets (include/ltxhip_presets.h; configs.rs:50-283)
class PresetC(C.Structure):
    _fields_ = [("version", C.c_char_p), ("guidance_scale", C.c_float), ("num_inference_steps", C.c_int), ("stg_scale", C.c_float),
                ("rescaling_scale", C.c_float), ("stochastic_sampling", C.c_int), ("skip_block_list", C.c_int * 8), ("n_skip_blocks", C.c_int),
                ("timesteps", C.c_float * 16), ("n_timesteps", C.c_int), ("decode_timestep", C.c_float), ("has_decode_timestep", C.c_int),
                ("decode_noise_scale", C.c_float), ("has_decode_noise_scale", C.c_int), ("transformer", DitConfigC), ("vae", VaeConfigC),
                ("vae_encoder_block_out_channels", C.c_int * 5), ("vae_encoder_layers_per_block", C.c_int * 5),
                ("num_train_timesteps", C.c_int), ("shift", C.c_float), ("use_dynamic_shifting", C.c_int), ("base_shift", C.c_float),
                ("max_shift", C.c_float), ("base_image_seq_len", C.c_int), ("max_image_seq_len", C.c_int), ("shift_terminal", C.c_float),
                ("has_shift_terminal", C.c_int), ("time_shift_exponential", C.c_int)]


@dataclass
class LTXVFullConfig:
    """get_config_by_version's result (configs.rs:40-46): inference settings + the three component configs."""
    version: str
    guidance_scale: float
    num_inference_steps: int
    stg_scale: float
    rescaling_scale: float
    stochastic_sampling: bool
    skip_block_list: List[int]
    timesteps: Optional[List[float]]
    decode_timestep: Optional[float]
    decode_noise_scale: Optional[float]
    transformer: "LtxVideoTransformer3DModelConfig"
    vae: "AutoencoderKLLtxVideoConfig"
    vae_encoder_block_out_channels: List[int]
    vae_encoder_layers_per_block: List[int]
    scheduler: Dict[str, object]

    def pipeline_call(self, height: int, width: int, num_frames: int, **over) -> "PipelineCall":
        """the PipelineCall examples/ltx-video/main.rs:585-646 builds from this preset (ltx_pipeline_params_from_preset)"""
        kw = dict(height=height, width=width, num_frames=num_frames,
                  num_inference_steps=len(self.timesteps) if self.timesteps else self.num_inference_steps, sigmas=self.timesteps,
                  guidance_scale=self.guidance_scale, guidance_rescale=self.rescaling_scale, stg_scale=self.stg_scale,
                  skip_block_list=list(self.skip_block_list) or None,
                  decode_timestep=self.decode_timestep if self.decode_timestep is not None else 0.0,
                  stochastic_sampling=self.stochastic_sampling)
        kw["decode_noise_scale"] = self.decode_noise_scale if self.decode_noise_scale is not None else kw["decode_timestep"]
        kw.update(over)
        return PipelineCall(**kw)


def preset_names() -> List[str]:
    lib.ltx_preset_name.restype = C.c_char_p
    return [lib.ltx_preset_name(i).decode() for i in range(lib.ltx_preset_count())]


def get_config_by_version(version: str) -> LTXVFullConfig:
    """configs.rs:50-70 (aliases; unknown strings fall back to 0.9.5)."""
    p = PresetC()
    _check(lib.ltx_preset_get(version.encode(), C.byref(p)))
    t, v = p.transformer, p.vae
    tcfg = LtxVideoTransformer3DModelConfig(in_channels=t.in_channels, out_channels=t.out_channels, patch_size=t.patch_size, patch_size_t=t.patch_size_t,
                                            num_attention_heads=t.num_attention_heads, attention_head_dim=t.attention_head_dim,
                                            cross_attention_dim=t.cross_attention_dim, num_layers=t.num_layers, norm_eps=t.norm_eps,
                                            caption_channels=t.caption_channels)
    nb = v.n_blocks
    vcfg = AutoencoderKLLtxVideoConfig(latent_channels=v.latent_channels, out_channels=v.out_channels,
                                       decoder_block_out_channels=tuple(v.decoder_block_out_channels[:nb]),
                                       decoder_layers_per_block=tuple(v.decoder_layers_per_block[:nb + 1]),
                                       decoder_upsample_factor=tuple(v.decoder_upsample_factor[:nb]), patch_size=v.patch_size,
                                       patch_size_t=v.patch_size_t, timestep_conditioning=bool(v.timestep_conditioning),
                                       decoder_causal=bool(v.decoder_causal), scaling_factor=v.scaling_factor,
                                       spatial_compression_ratio=v.spatial_compression_ratio, temporal_compression_ratio=v.temporal_compression_ratio)
    return LTXVFullConfig(
        version=p.version.decode(), guidance_scale=p.guidance_scale, num_inference_steps=p.num_inference_steps, stg_scale=p.stg_scale,
        rescaling_scale=p.rescaling_scale, stochastic_sampling=bool(p.stochastic_sampling), skip_block_list=list(p.skip_block_list[:p.n_skip_blocks]),
        timesteps=[float(x) for x in p.timesteps[:p.n_timesteps]] if p.n_timesteps else None,
        decode_timestep=float(p.decode_timestep) if p.has_decode_timestep else None,
        decode_noise_scale=float(p.decode_noise_scale) if p.has_decode_noise_scale else None,
        transformer=tcfg, vae=vcfg, vae_encoder_block_out_channels=list(p.vae_encoder_block_out_channels),
        vae_encoder_layers_per_block=list(p.vae_encoder_layers_per_block),
        scheduler=dict(num_train_timesteps=p.num_train_timesteps, shift=p.shift, use_dynamic_shifting=bool(p.use_dynamic_shifting),
                       base_shift=p.base_shift, max_shift=p.max_shift, base_image_seq_len=p.base_image_seq_len, max_image_seq_len=p.max_image_seq_len,
                       shift_terminal=p.shift_terminal if p.has_shift_terminal else None, time_shift_type="exponential" if p.time_shift_exponential else "linear"))


# ------------------------------------------------------------------ start-up control (include/ltxhip.h)
def warmup(transformer: Optional[LtxVideoTransformer3DModel], vae: Optional["AutoencoderKLLtxVideo"], B: int, F: int, H: int, W: int, K: int = 128):
    """ltx_warmup: plan measurement / workspace sizing for the latent geometry (F, H, W), outside the first real call."""
    _check(lib.ltx_warmup(transformer._h if transformer is not None else None, vae._h if vae is not None else None, B, F, H, W, K, _stream()))


def set_autotune(enabled: bool):
    _check(lib.ltx_set_autotune(int(enabled)))


def set_option(key: str, value=None):
    """ltx_set_option (include/ltxhip.h, run-time options): value None = the option's default"""
    _check(lib.ltx_set_option(key.encode(), None if value is None else str(value).encode()))


def reset_options():
    _check(lib.ltx_reset_options())


def has_experiments() -> bool:
    return bool(lib.ltx_has_experiments())


def attention_fallback_counts(reset: bool = False):
    """(head_dim-64 workgroups, head_dim-128 launches) that took the exact-max second pass since the last reset"""
    out = (C.c_ulonglong * 2)()
    _check(lib.ltx_attention_fallback_counts(out, int(reset)))
    return int(out[0]), int(out[1])


def get_option(key: str):
    """ltx_get_option: the option's current value as text (None: an experiment knob that is not set)"""
    buf = C.create_string_buffer(256)
    if lib.ltx_get_option(key.encode(), buf, 256) != 0:
        if key.startswith("x_"):
            return None
        _check(1)
    return buf.value.decode()


class options:
    """with ltxhip.options(gemm_tune=0, gemm_off="asm16"): ...  - options set for the block, the PREVIOUS values (LTX_OPTIONS'
    or an outer block's) restored after it"""
    def __init__(self, **kw): self.kw = kw
    def __enter__(self):
        self.prev = {k: get_option(k) for k in self.kw}
        for k, v in self.kw.items(): set_option(k, v)
        return self
    def __exit__(self, *a):
        for k, v in self.prev.items(): set_option(k, v)
        return False


def plan_save(path: str):
    _check(lib.ltx_plan_save(path.encode()))


def plan_load(path: str):
    _check(lib.ltx_plan_load(path.encode()))


# ------------------------------------------------------------------ frame output (include/ltxhip_frames.h)
def video_to_rgb8(video: torch.Tensor) -> torch.Tensor:
    """[B,3,F,H,W] f32 (0..255) -> [B,F,H,W,3] u8 on the device (main.rs:659-664: permute, clamp, truncating cast)."""
    v = _dev(video, torch.float32)
    B, _, F, H, W = v.shape
    out = torch.empty(B, F, H, W, 3, dtype=torch.uint8, device=v.device)
    _check(lib.ltx_video_to_rgb8(_ptr(v), B, F, H, W, _ptr(out), _stream()))
    return out


def write_png(path: str, rgb: torch.Tensor):
    """HOST u8 [H,W,3] -> PNG file."""
    t = rgb.detach().to("cpu", torch.uint8).contiguous()
    _check(lib.ltx_write_png(path.encode(), C.c_void_p(t.data_ptr()), t.shape[1], t.shape[0]))


def write_gif(path: str, frames: torch.Tensor, delay_cs: int = 4, speed: int = 30):
    """HOST u8 [N,H,W,3] -> animated GIF (main.rs:683-707: per-frame NeuQuant palette at `speed`, delay, infinite loop)."""
    t = frames.detach().to("cpu", torch.uint8).contiguous()
    _check(lib.ltx_write_gif(path.encode(), C.c_void_p(t.data_ptr()), t.shape[0], t.shape[2], t.shape[1], delay_cs, speed))


def save_video_gif(video: torch.Tensor, path: str):
    """The reference's default output: [B,3,F,H,W] f32 (0..255) on the device -> path (video.gif in main.rs:690)."""
    v = _dev(video, torch.float32)
    B, _, F, H, W = v.shape
    _check(lib.ltx_save_video_gif(_ptr(v), B, F, H, W, path.encode(), _stream()))


def save_frames_png(video: torch.Tensor, out_dir: str) -> int:
    """`--frames` output of examples/ltx-video/main.rs:653-675: out_dir/frame_%04d.png; returns the number written."""
    v = _dev(video, torch.float32)
    B, _, F, H, W = v.shape
    n = C.c_int(0)
    _check(lib.ltx_save_frames_png(_ptr(v), B, F, H, W, out_dir.encode(), C.byref(n), _stream()))
    return n.value


# ------------------------------------------------------------------ kernel-level ops (include/ltxhip_ops.h)
class ops:
    @staticmethod
    def guidance_step(text, latents, uncond=None, perturbed=None, guidance_scale=1.0, guidance_rescale=0.0, stg_scale=0.0, dt=0.0,
                      sigma=None, sigma_next=None, step_noise=None, hold=None, num_frames=None, want_noise_pred=False):
        """One guidance mix + scheduler update on a copy of `latents` [B, ...] f32: Euler (x + dt * v), or with step_noise the
        stochastic update (sigma, sigma_next).  hold [B, num_frames] (DEVICE u8 tensor or host values, truthy = held) selects the
        held-frame kernels (ltx_guidance_step_held / _stochastic_held): those latent frames keep their bits.
        Returns the new latents, or (latents, noise_pred f32) with want_noise_pred."""
        t = _dev(text)
        u = _dev(uncond, t.dtype) if uncond is not None else None
        p = _dev(perturbed, t.dtype) if perturbed is not None else None
        x = _dev(latents, torch.float32).clone()
        B, n = x.shape[0], x[0].numel()
        if t.shape[0] != B or t[0].numel() != n:
            raise LtxError("guidance_step: predictions and latents must agree in shape")
        nz = _dev(step_noise, torch.float32) if step_noise is not None else None
        if nz is not None and (sigma is None or sigma_next is None or nz.numel() != B * n):
            raise LtxError("guidance_step: the stochastic update needs sigma, sigma_next and step_noise of the latents' shape")
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device) if want_noise_pred else None
        ws = torch.zeros(8 * B, dtype=torch.float64, device=x.device)
        g = (C.c_float(guidance_scale), C.c_float(guidance_rescale), C.c_float(stg_scale))
        if hold is None:
            if nz is not None:
                _check(lib.ltx_guidance_step_stochastic(_ptr(t), _ptr(u), _ptr(p), _dt(t.dtype), _ptr(x), _ptr(out), B, C.c_int64(n), *g,
                                                        C.c_float(sigma), C.c_float(sigma_next), _ptr(nz), _ptr(ws), _stream()))
            else:
                _check(lib.ltx_guidance_step(_ptr(t), _ptr(u), _ptr(p), _dt(t.dtype), _ptr(x), _ptr(out), B, C.c_int64(n), *g, C.c_float(dt), _ptr(ws), _stream()))
        else:
            if num_frames is None or num_frames < 1 or n % num_frames != 0:
                raise LtxError("guidance_step: hold needs num_frames dividing the per-row element count")
            if torch.is_tensor(hold) and hold.is_cuda:
                hd = hold.to(torch.uint8).contiguous()
            else:
                hd = torch.tensor(list(_hold_host(hold, B, num_frames)), dtype=torch.uint8).to(x.device)
            if hd.numel() != B * num_frames:
                raise LtxError(f"hold must have {B} x {num_frames} entries")
            if nz is not None:
                _check(lib.ltx_guidance_step_stochastic_held(_ptr(t), _ptr(u), _ptr(p), _dt(t.dtype), _ptr(x), _ptr(out), B, C.c_int64(n), *g,
                                                             C.c_float(sigma), C.c_float(sigma_next), _ptr(nz), _ptr(ws), _ptr(hd), num_frames,
                                                             C.c_int64(n // num_frames), _stream()))
            else:
                _check(lib.ltx_guidance_step_held(_ptr(t), _ptr(u), _ptr(p), _dt(t.dtype), _ptr(x), _ptr(out), B, C.c_int64(n), *g, C.c_float(dt),
                                                  _ptr(ws), _ptr(hd), num_frames, C.c_int64(n // num_frames), _stream()))
        return (x, out) if want_noise_pred else x

    @staticmethod
    def linear(x, w, bias=None, epi=0, resid=None, gate=None, rows_per_batch=1):
        M, K = x.shape
        N = w.shape[0]
        y = torch.empty(M, N, dtype=x.dtype, device=x.device)
        _check(lib.ltx_op_linear(_ptr(x.contiguous()), _ptr(w.contiguous()), _ptr(bias), _ptr(y), M, N, K, _dt(x.dtype), epi,
                                 _ptr(resid), _ptr(gate), rows_per_batch, _stream()))
        return y

    @staticmethod
    def ring_pack(w):
        """-> the tile-contiguous second copy of a bf16 [N, K] weight that the small-M kernel streams (GemmArgs::Wp)"""
        N, K = w.shape
        out = torch.empty(lib.ltx_op_ring_packed_bytes(N, K) // 2, dtype=torch.bfloat16, device=w.device)
        _check(lib.ltx_op_ring_pack(_ptr(w.contiguous()), N, K, _ptr(out), _stream()))
        return out

    @staticmethod
    def linear_packed(x, w, wp, bias=None, epi=0, resid=None, gate=None, rows_per_batch=1):
        """ops.linear with the packed copy of w at hand (bf16; same results)"""
        M, K = x.shape
        N = w.shape[0]
        y = torch.empty(M, N, dtype=x.dtype, device=x.device)
        _check(lib.ltx_op_linear_packed(_ptr(x.contiguous()), _ptr(w.contiguous()), _ptr(wp), _ptr(bias), _ptr(y), M, N, K, epi,
                                        _ptr(resid), _ptr(gate), rows_per_batch, _stream()))
        return y

    @staticmethod
    def linear_rowsq(x, w, bias, epi=0, resid=None, gate=None, rows_per_batch=1):
        """-> (x @ w^T + bias, per-row partial sums of squares of that output per 128-column group [M, ceil(N/128)] f32)"""
        M, K = x.shape
        N = w.shape[0]
        y = torch.empty(M, N, dtype=x.dtype, device=x.device)
        rs = torch.empty(M, (N + 127) // 128, dtype=torch.float32, device=x.device)
        _check(lib.ltx_op_linear_rowsq(_ptr(x.contiguous()), _ptr(w.contiguous()), _ptr(bias), _ptr(y), _ptr(rs), M, N, K, _dt(x.dtype), epi,
                                       _ptr(resid), _ptr(gate), rows_per_batch, _stream()))
        return y, rs

    @staticmethod
    def rowsq(x):
        """the stand-alone form of linear_rowsq's by-product on a stored matrix (same values, bit for bit)"""
        M, N = x.shape
        rs = torch.empty(M, (N + 127) // 128, dtype=torch.float32, device=x.device)
        _check(lib.ltx_op_rowsq(_ptr(x.contiguous()), C.c_int64(M), N, N, _ptr(rs), _dt(x.dtype), _stream()))
        return rs

    @staticmethod
    def linear_fold_ok(M, N, K, epi, consumer, rs_n=0, vec_stride=None, rows_per_batch=None) -> bool:
        """whether the norm fold serves the call (consumer False: linear_fold_out, True: linear_fold_in); nothing is launched"""
        return bool(lib.ltx_op_linear_fold_ok(M, N, K, epi, int(bool(consumer)), rs_n, N if vec_stride is None else vec_stride,
                                              M if rows_per_batch is None else rows_per_batch))

    @staticmethod
    def linear_fold_out(x, w, bias, scale2, epi, resid, gate=None, rows_per_batch=1):
        """producer side of the norm fold (bf16): -> (y = the residual epilogue, y2 = y (.) (1 + scale2[b]), row partials of y).
        scale2 f32 [batch, stride >= N]"""
        M, K = x.shape
        N = w.shape[0]
        y = torch.empty(M, N, dtype=x.dtype, device=x.device); y2 = torch.empty_like(y)
        rs = torch.empty(M, (N + 127) // 128, dtype=torch.float32, device=x.device)
        _check(lib.ltx_op_linear_fold_out(_ptr(x.contiguous()), _ptr(w.contiguous()), _ptr(bias), _ptr(y), _ptr(y2), _ptr(rs), _ptr(scale2), scale2.shape[-1],
                                          M, N, K, epi, _ptr(resid), _ptr(gate), rows_per_batch, _stream()))
        return y, y2, rs

    @staticmethod
    def linear_fold_in(x, w, rs_sq, cvec, epi=0, rows_per_batch=1, rs_D=None, eps=1e-6):
        """consumer side of the norm fold (bf16): epi(r_m * (x @ w^T) + cvec[b]) with r_m from the row partials rs_sq [M, rs_n] f32;
        cvec f32 [batch, stride >= N]"""
        M, K = x.shape
        N = w.shape[0]
        y = torch.empty(M, N, dtype=x.dtype, device=x.device)
        _check(lib.ltx_op_linear_fold_in(_ptr(x.contiguous()), _ptr(w.contiguous()), _ptr(y), _ptr(rs_sq.contiguous()), rs_sq.shape[-1], K if rs_D is None else rs_D,
                                         C.c_float(eps), _ptr(cvec), cvec.shape[-1], M, N, K, epi, rows_per_batch, _stream()))
        return y

    @staticmethod
    def shift_gemv(w, bias, shift, K=None, out_stride=None):
        """cvec [B, N] f32 = shift[:, :K] @ w^T + bias (bf16 w [N, K], bias or None; shift f32 [B, stride >= K])"""
        N, Kw = w.shape
        K = Kw if K is None else K
        B = shift.shape[0]
        out = torch.zeros(B, N if out_stride is None else out_stride, dtype=torch.float32, device=w.device)
        _check(lib.ltx_op_shift_gemv(_ptr(w.contiguous()), _ptr(bias), _ptr(shift), shift.shape[-1], B, N, K, _ptr(out), out.shape[-1], _stream()))
        return out

    @staticmethod
    def mod_scale(h, scale, rows_per_batch):
        """h (.) (1 + scale[b]) in h's dtype: h [B * rows_per_batch, D], scale f32 [B, stride >= D]"""
        rows, D = h.shape
        y = torch.empty_like(h)
        _check(lib.ltx_op_mod_scale(_ptr(h.contiguous()), _ptr(scale), scale.shape[-1], _ptr(y), rows // rows_per_batch, C.c_int64(rows_per_batch), D, _dt(h.dtype), _stream()))
        return y

    @staticmethod
    def stg_fill(dst, src, rows, S, D=None):
        """in place on dst: dst[b*S + s, :D] = src[b*S + s, :D] for the batch rows with rows[b] truthy (ltx_op_stg_fill).  dst, src:
        2-D views [B*S, >= D] of one dtype with unit column stride - their row strides are the leading dimensions, so a column slice
        of a wider matrix (the v segment of q|k|v) is passed as it is"""
        if not dst.is_cuda or not src.is_cuda or dst.dim() != 2 or src.dim() != 2 or dst.dtype != src.dtype or dst.stride(1) != 1 or src.stride(1) != 1:
            raise LtxError("stg_fill: dst and src must be 2-D GPU tensors of one dtype with contiguous rows")
        B = len(rows)
        D = min(dst.shape[1], src.shape[1]) if D is None else D
        if dst.shape[0] != B * S or src.shape[0] != B * S or D > dst.shape[1] or D > src.shape[1]:
            raise LtxError(f"stg_fill: dst / src must have {B} x {S} rows of at least {D} columns")
        r = (C.c_ubyte * max(B, 1))(*[1 if v else 0 for v in rows])
        _check(lib.ltx_op_stg_fill(_ptr(dst), dst.stride(0), _ptr(src), src.stride(0), r, B, S, D, _dt(dst.dtype), _stream()))
        return dst

    @staticmethod
    def scale_cols(w, scale):
        """w[n][k] * (1 + scale[k]) in w's dtype"""
        N, K = w.shape
        out = torch.empty_like(w)
        _check(lib.ltx_op_scale_cols(_ptr(w.contiguous()), _ptr(scale), _ptr(out), C.c_int64(N), K, _dt(w.dtype), _stream()))
        return out

    @staticmethod
    def lora_merge(w0, adapters):
        """out = round(f32(w0) + sum_i coef_i * (B_i A_i)): adapters = [(A [r, K], B [N, r], coef), ...] in w0's dtype (ltx_op_lora_merge)"""
        w0 = _dev(w0); N, K = w0.shape
        As = [_dev(a, w0.dtype) for a, _, _ in adapters]; Bs = [_dev(b, w0.dtype) for _, b, _ in adapters]
        for a, b in zip(As, Bs):
            _expect("A", a, (a.shape[0], K)); _expect("B", b, (N, a.shape[0]))
        n = len(adapters)
        out = torch.empty_like(w0)
        pa = (C.c_void_p * max(n, 1))(*[a.data_ptr() for a in As]); pb = (C.c_void_p * max(n, 1))(*[b.data_ptr() for b in Bs])
        rs = (C.c_int * max(n, 1))(*[a.shape[0] for a in As])
        _check(lib.ltx_op_lora_merge(_ptr(w0), _ptr(out), N, K, n, pa, pb, rs, _floats([c for _, _, c in adapters]) if n else None, _dt(w0.dtype), _stream()))
        return out

    @staticmethod
    def attention_rowsq(q, k, v, heads, scale, key_bias, q_rowsq, eps=1e-5):
        """cross attention on UN-normalised queries: the RMS-norm scalar of each query row comes from q_rowsq [B*Sq, D/128]"""
        B, Sq, D = q.shape
        o = torch.empty_like(q)
        _check(lib.ltx_op_attention_rowsq(_ptr(q.contiguous()), _ptr(k.contiguous()), _ptr(v.contiguous()), _ptr(o), B, Sq, k.shape[1], heads, D // heads,
                                          D, D, D, D, C.c_float(scale), _ptr(key_bias), _ptr(q_rowsq), q_rowsq.shape[-1], D, C.c_float(eps), _stream()))
        return o

    @staticmethod
    def attention_compact(q, k, v, heads, scale, key_bias, q_rowsq=None, eps=1e-5):
        """ops.attention (bf16, head_dim 64, <= 128 keys, key bias) the way the DiT's cross attention runs it: keys whose bias is
        above -5000 compacted to the front, only their key blocks multiplied.  Returns (o, keys kept per batch row)."""
        B, Sq, D = q.shape
        o = torch.empty_like(q)
        cnt = torch.zeros(B, dtype=torch.int32, device=q.device)
        _check(lib.ltx_op_attention_compact(_ptr(q.contiguous()), _ptr(k.contiguous()), _ptr(v.contiguous()), _ptr(o), B, Sq, k.shape[1], heads, D // heads,
                                            D, D, D, D, C.c_float(scale), _ptr(key_bias.contiguous()), _ptr(q_rowsq) if q_rowsq is not None else None,
                                            q_rowsq.shape[-1] if q_rowsq is not None else 0, D, C.c_float(eps), _ptr(cnt), _stream()))
        return o, cnt

    @staticmethod
    def xattn_fold_route(dtype, head_dim, heads, KP, B=1, compact=True, D=None) -> bool:
        """does a text context of KP kept-key columns per head carry vo = V Wo^T (attn2.to_out folded into the context, option
        xattn_fold_vo)?  The decision the DiT's context build asks; nothing is launched, no device is needed."""
        out = C.c_int(0)
        _check(lib.ltx_op_xattn_fold_route(_dt(dtype), head_dim, heads, heads * head_dim if D is None else D, KP, B, int(bool(compact)), C.byref(out)))
        return bool(out.value)

    @staticmethod
    def xattn_fold_kp(counts) -> int:
        """KP of the kept-key counts of the batch rows: the largest, rounded up to the cross kernel's 32-key block"""
        n = len(counts); out = C.c_int(0)
        _check(lib.ltx_op_xattn_fold_kp((C.c_int * n)(*[int(c) for c in counts]), n, C.byref(out)))
        return out.value

    @staticmethod
    def xattn_fold_build(v, key_bias, wo, heads, KP):
        """vo [B, D, heads*KP] = V_kept Wo^T per head (bf16, head_dim 64): (vo, keys kept per batch row)"""
        B, K, D = v.shape
        vo = torch.empty(B, D, heads * KP, dtype=torch.bfloat16, device=v.device)
        cnt = torch.zeros(B, dtype=torch.int32, device=v.device)
        _check(lib.ltx_op_xattn_fold_build(_ptr(v.contiguous()), _ptr(key_bias.contiguous()), _ptr(wo.contiguous()), B, K, heads, KP, _ptr(vo), _ptr(cnt), _stream()))
        return vo, cnt

    @staticmethod
    def attention_probs(q, k, heads, scale, key_bias, KP, q_rowsq=None, eps=1e-5):
        """the cross kernel's P-only mode: p [B, Sq, heads*KP] bf16, the softmax weights of the kept keys (compacted to the front,
        as ops.attention_compact does), zeros behind a row's count: (p, keys kept per batch row)"""
        B, Sq, D = q.shape
        p = torch.empty(B, Sq, heads * KP, dtype=torch.bfloat16, device=q.device)
        cnt = torch.zeros(B, dtype=torch.int32, device=q.device)
        _check(lib.ltx_op_attention_probs(_ptr(q.contiguous()), _ptr(k.contiguous()), _ptr(p), B, Sq, k.shape[1], heads, KP, C.c_float(scale), _ptr(key_bias.contiguous()),
                                          _ptr(q_rowsq) if q_rowsq is not None else None, q_rowsq.shape[-1] if q_rowsq is not None else 0, C.c_float(eps), _ptr(cnt), _stream()))
        return p, cnt

    @staticmethod
    def linear_segmented(x, w, bias, seg_width):
        """x @ w^T + bias written as N/seg_width dense [M, seg_width] matrices (the DiT's q|k|v projection)."""
        M, K = x.shape
        N = w.shape[0]
        y = torch.empty(N // seg_width, M, seg_width, dtype=x.dtype, device=x.device)
        _check(lib.ltx_op_linear_segmented(_ptr(x.contiguous()), _ptr(w.contiguous()), _ptr(bias), _ptr(y), M, N, K, seg_width,
                                           _dt(x.dtype), _stream()))
        return y

    @staticmethod
    def rownorm(x, kind=0, eps=1e-6, weight=None, scale=None, shift=None, rows_per_batch=1, act=0):
        rows, D = x.shape
        y = torch.empty_like(x)
        ms = scale.shape[-1] if scale is not None else 0
        _check(lib.ltx_op_rownorm(_ptr(x.contiguous()), _ptr(y), C.c_int64(rows), D, kind, C.c_float(eps), _ptr(weight),
                                  _ptr(scale), _ptr(shift), C.c_int64(rows_per_batch), ms, act, _dt(x.dtype), _stream()))
        return y

    @staticmethod
    def step_measure(h, prev, shift, scale, rows_per_batch, eps=1e-6, first=False):
        """ltx_op_step_measure: prev [rows, D] is overwritten with the modulated rows of h -> sums f64 [2] on the device
        (sum |m - prev|, sum |prev|); shift / scale f32 [groups, mod_stride]"""
        rows, D = h.shape
        ws = torch.empty(max(int(lib.ltx_op_step_measure_ws_bytes(C.c_int64(rows), D, _dt(h.dtype))), 16), dtype=torch.uint8, device=h.device)
        sums = torch.empty(2, dtype=torch.float64, device=h.device)
        _check(lib.ltx_op_step_measure(_ptr(h), _ptr(prev), _ptr(shift), _ptr(scale), shift.stride(0), C.c_int64(rows), D, C.c_int64(rows_per_batch),
                                       C.c_float(eps), _dt(h.dtype), int(first), _ptr(ws), _ptr(sums), _stream()))
        return sums

    @staticmethod
    def step_residual(h, r):
        """ltx_op_step_residual: r = h - r in place"""
        rows, D = h.shape
        _check(lib.ltx_op_step_residual(_ptr(h), _ptr(r), C.c_int64(rows), D, _dt(h.dtype), _stream()))
        return r

    # ---- the int8 (W8A8) kernels (include/ltxhip_int8.h)
    @staticmethod
    def quant_rows_i8(x):
        """x [rows, D] bf16 (any row stride, unit column stride) -> (q int8 [rows, D], scale f32 [rows])"""
        if x.dim() != 2 or x.stride(1) != 1:
            x = x.contiguous()
        rows, D = x.shape
        q = torch.empty(rows, D, dtype=torch.int8, device=x.device)
        sc = torch.empty(rows, dtype=torch.float32, device=x.device)
        _check(lib.ltx_op_quant_rows_i8(_ptr(x), C.c_int64(rows), D, x.stride(0) if rows > 1 else D, _ptr(q), _ptr(sc), _stream()))
        return q, sc

    @staticmethod
    def rownorm_quant_i8(h, shift, scale, rows_per_batch, eps=1e-6):
        """q, row_scale of the modulated RMS norm of h [rows, D] bf16; shift / scale f32 [groups, mod_stride]"""
        rows, D = h.shape
        h = h.contiguous()
        q = torch.empty(rows, D, dtype=torch.int8, device=h.device)
        sc = torch.empty(rows, dtype=torch.float32, device=h.device)
        _check(lib.ltx_op_rownorm_quant_i8(_ptr(h), C.c_int64(rows), D, D, C.c_float(eps), _ptr(shift), _ptr(scale), shift.stride(0),
                                           C.c_int64(rows_per_batch), _ptr(q), _ptr(sc), _stream()))
        return q, sc

    @staticmethod
    def gemm_i8(a_q, a_scale, w_q, w_scale, bias=None, epi=0, resid=None, gate=None, rows_per_batch=1, seg_width=0, tile=-1):
        """y bf16 = epi((float(a_q w_q^T) * a_scale[m]) * w_scale[n] + bias); seg_width: N / seg_width dense [M, seg_width] matrices;
        tile: -1 the shape rule, or an index into GEMM_I8_TILES"""
        M, K = a_q.shape
        N = w_q.shape[0]
        y = torch.empty((N // seg_width, M, seg_width) if seg_width else (M, N), dtype=torch.bfloat16, device=a_q.device)
        _check(lib.ltx_op_gemm_i8(_ptr(a_q.contiguous()), _ptr(a_scale), _ptr(w_q.contiguous()), _ptr(w_scale), _ptr(bias), _ptr(y), M, N, K, epi,
                                  _ptr(resid), _ptr(gate), rows_per_batch, seg_width, tile, _stream()))
        return y

    @staticmethod
    def gemm_i8_raw(a_q, w_q, tile=-1):
        """the int32 accumulators a_q w_q^T [M, N], unscaled"""
        M, K = a_q.shape
        N = w_q.shape[0]
        acc = torch.empty(M, N, dtype=torch.int32, device=a_q.device)
        _check(lib.ltx_op_gemm_i8_raw(_ptr(a_q.contiguous()), _ptr(w_q.contiguous()), _ptr(acc), M, N, K, tile, _stream()))
        return acc

    @staticmethod
    def linear_deferred(x, w):
        """x @ w^T as UN-reduced K ranges (the library's shape rule): parts [P, M, N] f32 (bf16 layers of at most 512 rows)"""
        M, K = x.shape
        N = w.shape[0]
        P = lib.ltx_op_linear_split_factor(M, N, K)
        parts = torch.empty(P, M, N, dtype=torch.float32, device=x.device)
        _check(lib.ltx_op_linear_deferred(_ptr(x.contiguous()), _ptr(w.contiguous()), _ptr(parts), M, N, K, _stream()))
        return parts

    @staticmethod
    def rownorm_deferred(parts, bias, resid, gate=None, kind=0, eps=1e-6, scale=None, shift=None, rows_per_batch=1):
        """finish the rows of ops.linear_deferred (h = resid + gate * (sum of the parts + bias)) and normalise them: (h, y)"""
        P, rows, D = parts.shape
        h = torch.empty_like(resid); y = torch.empty_like(resid)
        ms = scale.shape[-1] if scale is not None else 0
        _check(lib.ltx_op_rownorm_deferred(_ptr(parts), P, _ptr(bias), _ptr(resid.contiguous()), _ptr(gate), gate.shape[-1] if gate is not None else 0, _ptr(h),
                                           _ptr(y), C.c_int64(rows), D, kind, C.c_float(eps), _ptr(scale), _ptr(shift), C.c_int64(rows_per_batch), ms, _dt(resid.dtype), _stream()))
        return h, y

    @staticmethod
    def rownorm_presum(x, presum, eps=1e-6, weight=None, scale=None, shift=None, rows_per_batch=1, act=0):
        """RMS rownorm of rows whose sums of squares are known (presum [rows, D/128] from linear_rowsq / rowsq): a pure map"""
        rows, D = x.shape
        y = torch.empty_like(x)
        ms = scale.shape[-1] if scale is not None else 0
        _check(lib.ltx_op_rownorm_presum(_ptr(x.contiguous()), _ptr(y), C.c_int64(rows), D, C.c_float(eps), _ptr(weight), _ptr(scale), _ptr(shift),
                                         C.c_int64(rows_per_batch), ms, act, _ptr(presum), presum.shape[-1], _dt(x.dtype), _stream()))
        return y

    @staticmethod
    def qknorm_rope(x, weight, eps=1e-5, cos=None, sin=None):
        x = x.clone().contiguous()
        rows, D = x.shape
        _check(lib.ltx_op_qknorm_rope(_ptr(x), C.c_int64(rows), D, D, _ptr(weight), C.c_float(eps), _ptr(cos), _ptr(sin),
                                      _dt(x.dtype), _stream()))
        return x

    @staticmethod
    def qknorm_rope_segs(x, rows, D, ld, nseg, seg_stride, w0, w1=None, w0b=None, eps=1e-5, cos=None, sin=None, out_scale0=1.0):
        """q/k RMS norm + RoPE the way the DiT calls it, IN PLACE on the caller's buffer x (any shape; never copied): nseg segments
        of D columns of row m at element m * ld + j * (seg_stride or D).  Segment 0: w0 [* w0b], out_scale0; segment 1: w1."""
        if not x.is_contiguous():
            raise LtxError("qknorm_rope_segs: the buffer is used as it lies in memory; pass a contiguous tensor")
        _check(lib.ltx_op_qknorm_rope_segs(_ptr(x), C.c_int64(rows), D, ld, nseg, C.c_int64(seg_stride), _ptr(w0), _ptr(w1), _ptr(w0b),
                                           C.c_float(eps), _ptr(cos), _ptr(sin), C.c_float(out_scale0), _dt(x.dtype), _stream()))
        return x

    @staticmethod
    def norm_route(rows, D, dtype=torch.bfloat16, kind=0, scale=False, shift=None, weight=False, act=0, rows_per_batch=1, presum_n=0, nparts=0) -> str:
        """which kernel of csrc/rownorm.hip serves the described ops.rownorm / rownorm_presum (presum_n partials per row) /
        rownorm_deferred (nparts K ranges) call under the current options: "narrow", "block", "wide", "reread", "presum",
        "presum_lean", "wide_defer", "wide_defer4", "block_defer", "block_defer4" - or "refused" where the op raises LtxError.
        scale / shift / weight: whether the operand is passed (shift defaults to scale).  Nothing is launched; no device is needed."""
        buf = C.create_string_buffer(32)
        flags = (1 if scale else 0) | (2 if (scale if shift is None else shift) else 0) | (4 if weight else 0)
        _check(lib.ltx_op_norm_route(C.c_int64(rows), D, _dt(dtype), kind, flags, act, C.c_int64(rows_per_batch), presum_n, nparts, buf, 32))
        return buf.value.decode()

    @staticmethod
    def qknorm_route(rows, D, dtype=torch.bfloat16) -> str:
        """the same for ops.qknorm_rope / qknorm_rope_segs: "block", "fused4", "fused8", "cached", "reread" or "refused"."""
        buf = C.create_string_buffer(32)
        _check(lib.ltx_op_qknorm_route(C.c_int64(rows), D, _dt(dtype), buf, 32))
        return buf.value.decode()

    @staticmethod
    def timestep_embedding(timesteps, vae_flavour=False, multiplier=1.0, dtype=torch.float32, device="cuda"):
        """get_timestep_embedding(dim 256, [cos | sin]): the DiT's (ltx_transformer.rs:271-309) or the VAE's (vae.rs:172-198)"""
        ts = [float(t) for t in timesteps]
        out = torch.empty(len(ts), 256, dtype=dtype, device=device)
        _check(lib.ltx_op_timestep_embedding(_floats(ts), len(ts), int(bool(vae_flavour)), C.c_float(multiplier), _dt(dtype), _ptr(out), _stream()))
        return out

    @staticmethod
    def rope_table(B, F, H, W, D, coords=None, rope_scale=None, device="cuda"):
        cos = torch.empty(B * F * H * W, D // 2, dtype=torch.float32, device=device)
        sin = torch.empty_like(cos)
        _check(lib.ltx_op_rope_table(_ptr(cos), _ptr(sin), _ptr(coords), B, F, H, W, D,
                                     _floats(rope_scale) if rope_scale is not None else None, _stream()))
        return cos, sin

    @staticmethod
    def attention(q, k, v, heads, scale, key_bias=None):
        B, Sq, D = q.shape
        Sk = k.shape[1]
        o = torch.empty_like(q)
        _check(lib.ltx_op_attention(_ptr(q.contiguous()), _ptr(k.contiguous()), _ptr(v.contiguous()), _ptr(o), B, Sq, Sk, heads, D // heads,
                                    D, D, D, D, C.c_float(scale), _ptr(key_bias), _dt(q.dtype), _stream()))
        return o

    @staticmethod
    def attention_prescaled(q, k, v, heads):
        """bf16, head_dim 64: q already multiplied by scale*log2(e); softmax in base 2 (DiT self-attention fast path)."""
        B, Sq, D = q.shape
        def rows(t):          # a [B, S, D] view whose rows are dense and whose batches are S rows apart keeps its row stride (column slices of a fused buffer)
            return t if t.stride(2) == 1 and t.stride(0) == t.shape[1] * t.stride(1) and t.stride(1) % 8 == 0 else t.contiguous()
        q, k, v = rows(q), rows(k), rows(v)
        o = torch.empty(B, Sq, D, dtype=q.dtype, device=q.device)
        _check(lib.ltx_op_attention_prescaled(_ptr(q), _ptr(k), _ptr(v), _ptr(o), B, Sq, k.shape[1],
                                              heads, D // heads, q.stride(1), k.stride(1), v.stride(1), D, _stream()))
        return o

    @staticmethod
    def conv3d(x_cl, w, bias, causal=False, resid=None):
        B, T, H, W, Cin = x_cl.shape
        Cout = w.shape[0]
        y = torch.empty(B, T, H, W, Cout, dtype=x_cl.dtype, device=x_cl.device)
        _check(lib.ltx_op_conv3d(_ptr(x_cl.contiguous()), _ptr(w.contiguous()), _ptr(bias.to(w.dtype).contiguous()), _dt(w.dtype), _ptr(y), _ptr(resid),
                                 B, T, H, W, Cin, Cout, int(causal), _dt(x_cl.dtype), _stream()))
        return y

    @staticmethod
    def conv3d_norm(x_cl, w, bias, causal=False, eps=1e-6, act=1, scale=None, shift=None):
        """ops.conv3d finished inside the conv's epilogue with the per-voxel RMS norm over all output channels, (1 + scale[b]) and
        shift[b], and SiLU (act=1): conv1 + norm2 of the VAE's resnet.  scale / shift: f32 [B, Cout], dense or column slices of one
        wider table (the decoder's [B, 4 * Cout] modulation table) - the row stride is taken from the tensors; both None: no
        modulation.  LtxError for a call the halo-staged kernel does not serve (f32, widths other than 128 / 256, under 16 voxels)."""
        B, T, H, W, Cin = x_cl.shape
        Cout = w.shape[0]
        if (scale is None) != (shift is None):
            raise LtxError("conv3d_norm: scale and shift come together")
        ms = 0
        if scale is not None:
            for t in (scale, shift):
                if t.dtype != torch.float32 or tuple(t.shape) != (B, Cout) or t.stride(1) != 1:
                    raise LtxError(f"conv3d_norm: scale / shift must be f32 [{B}, {Cout}] with dense rows")
            ms = scale.stride(0) if B > 1 else max(scale.stride(0), Cout)
            if B > 1 and shift.stride(0) != ms:
                raise LtxError("conv3d_norm: scale and shift must share one row stride")
        y = torch.empty(B, T, H, W, Cout, dtype=x_cl.dtype, device=x_cl.device)
        _check(lib.ltx_op_conv3d_norm(_ptr(x_cl.contiguous()), _ptr(w.contiguous()), _ptr(bias.to(w.dtype).contiguous()), _dt(w.dtype), _ptr(y),
                                      _ptr(scale), _ptr(shift), ms, C.c_float(eps), act, B, T, H, W, Cin, Cout, int(causal), _dt(x_cl.dtype), _stream()))
        return y

    @staticmethod
    def upsample3d(x_cl, w, bias, causal=False, residual=True):
        B, T, H, W, Cin = x_cl.shape
        Cout = w.shape[0]
        y = torch.empty(B, 2 * T - 1, 2 * H, 2 * W, Cout // 8, dtype=x_cl.dtype, device=x_cl.device)
        _check(lib.ltx_op_upsample3d(_ptr(x_cl.contiguous()), _ptr(w.contiguous()), _ptr(bias.to(w.dtype).contiguous()), _dt(w.dtype), _ptr(y),
                                     B, T, H, W, Cin, Cout, int(causal), int(residual), _dt(x_cl.dtype), _stream()))
        return y

    @staticmethod
    def conv3d_shuffle(x_cl, w, bias, st, ss, out=None):
        """The latent upsampler's shuffle stage (ltx_op_conv3d_shuffle): x_cl [B, F + 2, H, W, Cin] channels-last with zero guard
        frames, w [O, Cin, 3, 3, 3], factors (st, ss) one of (2,1), (2,2), (1,2) -> the guarded [B, Fo + 2, Ho, Wo, O / (st*ss*ss)].
        out: a pre-allocated (pre-filled) output of that shape, for tests that watch what the kernel leaves alone."""
        x = x_cl.contiguous()
        B, Ft, H, W, Cin = x.shape
        F = Ft - 2
        O = w.shape[0]
        nsub = st * ss * ss
        shape = (B, (2 * F - 1 if st == 2 else F) + 2, ss * H, ss * W, O // max(nsub, 1))
        if out is None:
            out = torch.empty(shape, dtype=x.dtype, device=x.device)
        elif tuple(out.shape) != shape or out.dtype != x.dtype or not out.is_contiguous():
            raise LtxError(f"conv3d_shuffle: out must be a contiguous {shape} tensor of the input's dtype")
        _check(lib.ltx_op_conv3d_shuffle(_ptr(x), _ptr(w.contiguous()), _ptr(bias.to(w.dtype).contiguous()), _dt(w.dtype), _ptr(out),
                                         B, F, H, W, Cin, O, int(st), int(ss), _dt(x.dtype), _stream()))
        return out

    @staticmethod
    def pixel_shuffle_guarded(x_cl, out=None):
        """the spatial kind's stand-alone shuffle pass (ltx_op_pixel_shuffle_guarded): x_cl [B, F + 2, H, W, 4C], channel s*C + c ->
        [B, F + 2, 2H, 2W, C] with zero guard frames; asynchronous"""
        x = x_cl.contiguous()
        B, Ft, H, W, C4 = x.shape
        if out is None:
            out = torch.empty(B, Ft, 2 * H, 2 * W, C4 // 4, dtype=x.dtype, device=x.device)
        _check(lib.ltx_op_pixel_shuffle_guarded(_ptr(x), _ptr(out), B, Ft - 2, H, W, C4 // 4, _dt(x.dtype), _stream()))
        return out

    @staticmethod
    def downsample3d(x_cl, w, bias, down_type):
        """LtxVideoDownsampler3d (vae.rs:499-582) on a channels-last tensor; down_type 1 spatial, 2 temporal, 3 spatiotemporal; Cout = out channels"""
        B, T, H, W, Cin = x_cl.shape
        st, sh, sw = {1: (1, 2, 2), 2: (2, 1, 1), 3: (2, 2, 2)}.get(down_type, (2, 2, 2))
        Cout = w.shape[0] * st * sh * sw
        y = torch.empty(B, (T + st - 1) // st, H // sh, W // sw, Cout, dtype=x_cl.dtype, device=x_cl.device)
        _check(lib.ltx_op_downsample3d(_ptr(x_cl.contiguous()), _ptr(w.contiguous()), _ptr(bias.to(w.dtype).contiguous()), _dt(w.dtype), _ptr(y),
                                       B, T, H, W, Cin, Cout, down_type, _dt(x_cl.dtype), _stream()))
        return y

    @staticmethod
    def gemm_plan(M, N, K, conv=0, ntaps=1, T=1, H=1, W=1) -> str:
        """name of the GEMM plan the dispatcher cached for this bf16 shape ("" before its first run)."""
        buf = C.create_string_buffer(32)
        _check(lib.ltx_op_gemm_plan(M, N, K, conv, ntaps, T, H, W, buf, 32))
        return buf.value.decode()

    @staticmethod
    def gemm_route(M, N, K, conv=0, ntaps=1, B=1, T=1, H=1, W=1, epi=0, dtype=torch.bfloat16, pn=False, defer=False, fold_in=False, fold_out=False) -> str:
        """where the GEMM dispatch sends the described call under the current options: "gemm128", "asm32" or a plan name.
        Nothing is launched or measured; LtxError where the launch would refuse the call."""
        buf = C.create_string_buffer(32)
        flags = (1 if pn else 0) | (2 if defer else 0) | (4 if fold_in else 0) | (8 if fold_out else 0)
        _check(lib.ltx_op_gemm_route(M, N, K, conv, ntaps, B, T, H, W, epi, _dt(dtype), flags, buf, 32))
        return buf.value.decode()

    DIT_PLAN_FIELDS = ("M", "MK", "NB", "Sg", "seg", "ldqkv", "fold_q2", "presum", "nfold", "defer_ff2", "ff2_parts", "dense_qkv", "fold_q")

    @staticmethod
    def dit_plan(heads, head_dim, B, S, K, G=1, dtype=torch.bfloat16, io_dtype=torch.float32, skip_mask=False) -> dict:
        """the decisions of one DiT forward (csrc/dit.hip's ltx_dit_plan) under the current options: sizes as ints, decisions as
        bools (ff2_parts an int).  No handle, no device; nothing is launched."""
        out = (C.c_int64 * len(ops.DIT_PLAN_FIELDS))()
        _check(lib.ltx_op_dit_plan(heads, head_dim, _dt(dtype), _dt(io_dtype), B, S, K, G, int(bool(skip_mask)), out))
        return {k: (int(v) if i < 6 or k == "ff2_parts" else bool(v)) for i, (k, v) in enumerate(zip(ops.DIT_PLAN_FIELDS, out))}

    @staticmethod
    def groupnorm(x_cl, weight, bias, groups=32, eps=1e-5, resid=None, silu=False, guards=False):
        """x_cl [B, F (+ 2 guard frames), H, W, C] channels-last; returns a new tensor (ltx_op_groupnorm)"""
        x = _dev(x_cl)
        B, Ft, H, W, Cn = x.shape
        F = Ft - 2 if guards else Ft
        y = torch.empty_like(x)
        w, b = _dev(weight, x.dtype), _dev(bias, x.dtype)
        r = _dev(resid, x.dtype) if resid is not None else None
        if r is not None:
            _expect("resid", r, x.shape)
        _check(lib.ltx_op_groupnorm(_ptr(x), _ptr(y), _ptr(r), _ptr(w), _ptr(b), B, F, H, W, Cn, groups, float(eps),
                                    (LTX_GN_SILU if silu else 0) | (LTX_GN_GUARDS if guards else 0), _dt(x.dtype), _stream()))
        return y

    @staticmethod
    def blend(a, b, dim, blend_extent):
        """in place on a copy of b; a, b f32 [B,C,t,h,w]."""
        a = a.contiguous(); b = b.clone().contiguous()
        BC = a.shape[0] * a.shape[1]
        _check(lib.ltx_op_blend(_ptr(a), _ptr(b), BC, a.shape[2], a.shape[3], a.shape[4], b.shape[2], b.shape[3], b.shape[4],
                                dim, blend_extent, _stream()))
        return b

    @staticmethod
    def conv_out_unpatchify(x_cl, w, bias, causal=False, postprocess=False):
        B, T, H, W, Cin = x_cl.shape
        Cout = w.shape[0]
        y = torch.empty(B, Cout // 16, T, 4 * H, 4 * W, dtype=torch.float32, device=x_cl.device)
        _check(lib.ltx_op_conv_out_unpatchify(_ptr(x_cl.contiguous()), _ptr(w.contiguous()), _ptr(bias.to(w.dtype).contiguous()), _dt(w.dtype), _ptr(y),
                                              B, T, H, W, Cin, Cout, int(causal), int(postprocess), _dt(x_cl.dtype), _stream()))
        return y


def prof_enable(on: bool):
    _check(lib.ltx_prof_enable(int(on)))


def prof_report(kind: int):
    """-> (total_ms, total_work, count) for kernel class `kind` since prof_enable(True)."""
    ms, work, cnt = C.c_double(), C.c_double(), C.c_longlong()
    _check(lib.ltx_prof_report(kind, C.byref(ms), C.byref(work), C.byref(cnt)))
    return ms.value, work.value, cnt.value


PROF_KERNELS = ("gemm_kernel (128 x 128)", "gemm_big_kernel", "gemm_p8_kernel", "conv_halo_kernel", "gemm_asm_kernel (32x32x16)", "gemm_asm16_kernel", "gemm_ring_kernel",
                "gemm_i8_kernel", "quant_rows_i8_kernel", "rownorm_quant_i8_kernel")      # (the last two are timed in class 4, the row norms)


def prof_report_kernel(kind: int, kernel: int):
    """-> (total_ms, total_work, count) of the launches of class `kind` served by kernel `kernel` (index into PROF_KERNELS)."""
    ms, work, cnt = C.c_double(), C.c_double(), C.c_longlong()
    _check(lib.ltx_prof_report_kernel(kind, kernel, C.byref(ms), C.byref(work), C.byref(cnt)))
    return ms.value, work.value, cnt.value
