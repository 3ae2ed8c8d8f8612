/* ltxhip_lora.h — LoRA adapters for the DiT: style, control, IC and distillation adapters trained on the transformer's
 * attention and feed-forward linears, loaded once and MERGED into the handle's weights on the device.
 *
 * The reference has no LoRA support (nothing in src/models/ltx_video mentions it): like ltxhip_cond.h this goes one step beyond
 * it.  The rule is the published one, W_eff = W + sum_i c_i * (B_i A_i) with c_i = scale_i * alpha_i / r_i (alpha absent: c_i =
 * scale_i); the parity reference is the restatement tests/lora_ref.py.
 *
 * Adapters are merged, not applied at run time: ltx_dit_forward, every GEMM plan and the norm fold are untouched, and the cost
 * moves to the adapter switch (ltx_dit_set_adapters), one read-modify-write pass over every targeted weight with a rank-r MFMA
 * product per output tile (csrc/lora.hip).  Adapters are HANDLE STATE: ltx_pipeline_call / ltx_pipeline_call_cond need no change
 * and simply run on whatever the handle's effective weights are.
 *
 * Targets are the ten block linears of every layer, numbered `which` = 0..9 in this order:
 *   transformer_blocks.{i}.attn1.{to_q, to_k, to_v, to_out.0}   0..3
 *   transformer_blocks.{i}.attn2.{to_q, to_k, to_v, to_out.0}   4..7
 *   transformer_blocks.{i}.ff.net.0.proj, .ff.net.2             8, 9
 *
 * Out of scope (stated, not silently ignored): run-time (unmerged) adapters and adapters per batch row; non-block targets
 * (proj_in, caption_projection, time_embed, proj_out, norms: counted as unmatched, refused under `strict`); DoRA, LoHa and LoKr;
 * VAE or T5 adapters; writing merged checkpoints to disk (ltx_dit_read_linear hands out the merged matrices).
 *
 * Conventions are those of ltxhip.h (device pointers unless marked HOST, 0 = success, ltx_last_error). */
#ifndef LTXHIP_LORA_H
#define LTXHIP_LORA_H
#include "ltxhip.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ltx_lora ltx_lora;

/* Host only (no device needed).  Splits an adapter tensor name into the module it belongs to and its role:
 *   role 0 = A / down, 1 = B / up, 2 = alpha.
 * One leading prefix out of "transformer.", "diffusion_model.", "model.diffusion_model." (or none) is stripped; the suffix is one of
 *   ".lora_A.weight" / ".lora_B.weight",  ".lora_down.weight" / ".lora_up.weight",  ".lora.down.weight" / ".lora.up.weight",  ".alpha";
 * the module name then goes through ltx_weights_remap_key, so Official-layout names resolve to Diffusers names as checkpoints do.
 * Writes the NUL-terminated module name into module_out[cap].  A key that is none of these: LTX_ERR_ARG. */
int ltx_lora_parse_key(const char* key, char* module_out, size_t cap, int* role);

/* Build an adapter for handles of `like`'s configuration.  tensors: the adapter's named tensors (host or device, F32 or BF16).
 *   A [r, in] and B [out, r] must fit the linear of like's config, 1 <= r <= 256; alpha (one element) absent = factor 1, else alpha / r.
 *   Both are uploaded once, rounded to like's model dtype (what merged LoRA in bf16 inference sees).
 * Names that are not adapter keys at all (ltx_lora_parse_key fails) are ignored.  Adapter keys on anything but the ten block
 * linears (or on a block the config does not have) count into *n_unmatched (may be NULL); with strict != 0 the call fails with
 * LTX_ERR_UNSUPPORTED naming the first such key.  An A without its B (or the reverse), a rank mismatch inside a pair, a rank outside
 * 1..256 or a shape that does not fit the linear: LTX_ERR_ARG naming the key.  No usable pair at all: LTX_ERR_MISSING_WEIGHT.
 * The object is bound to (dims, model dtype, device), not to the handle: any handle of equal configuration may use it, and it may
 * be destroyed while merged (the merged weights do not refer to it). */
int ltx_lora_create(const ltx_dit* like, const ltx_weight* tensors, size_t n, int strict, ltx_lora** out, int* n_unmatched);
/* The same from one safetensors file (the mmap reader of ltxhip_weights.h); F32 and BF16 payloads, anything else under an
 * adapter key: LTX_ERR_UNSUPPORTED naming the tensor. */
int ltx_lora_create_from_file(const ltx_dit* like, const char* path, int strict, ltx_lora** out, int* n_unmatched);
void ltx_lora_destroy(ltx_lora* l);

/* Make the handle's effective weights a function of its BASE weights and this list alone (no history), 0 <= n <= 8:
 *   every targeted linear holds round_dtype(f32(W0) + sum_i c_i * (B_i A_i)),  c_i = scales[i] * factor_i, summed in list order;
 *   every other weight is the base bit for bit; n = 0 restores the base bit for bit.
 * scales: HOST f32 [n].  The base is never written: merged weights live in a second buffer per targeted linear (one extra copy of
 * the targeted linears: about 3.8 GB at 2B, 26 GB at 13B, when all ten are targeted), allocated before anything is launched - on an
 * allocation failure the error is returned with the handle unchanged - and freed when the linear is no longer targeted.  For the fused
 * q|k|v and k|v weights an adapter addresses its row range; rows without an adapter are copied.
 * Work is enqueued on `stream`; the caller guarantees that no forward of this handle is in flight on another stream, and orders later
 * forwards on other streams after it.  Every weight-derived cache of the handle is invalidated (also inside an open
 * ltx_dit_context_cache scope): the next forward recomputes them.  An adapter of another configuration, dtype or device: LTX_ERR_ARG. */
int ltx_dit_set_adapters(ltx_dit* m, const ltx_lora* const* loras, const float* scales, int n, ltx_stream stream);
/* number of adapters of the last successful ltx_dit_set_adapters (0: base weights) */
int ltx_dit_adapter_count(const ltx_dit* m);
/* Copy the current effective [out, in] matrix of linear `which` (0..9, the order above) of block `block` into out_dev, model dtype
 * (a row slice of the fused weights).  For tests and for exporting a merged checkpoint. */
int ltx_dit_read_linear(const ltx_dit* m, int block, int which, void* out_dev, ltx_stream stream);

/* Kernel-level entry (beside the ltx_op_* family of ltxhip_ops.h): out[N, K] = round_dtype(f32(w0) + sum_i coef[i] * (B_i A_i)),
 *   w0, out [N, K] (out may not alias w0);  A[i] [r[i], K], B[i] [N, r[i]] device tensors of `dtype` (0 = f32, 1 = bf16);
 *   A, B, r, coef: HOST arrays of n entries, 0 <= n <= 8, 1 <= r[i] <= 256;  K % 8 == 0, any N.
 * bf16: exact bf16 x bf16 products accumulated in f32 on the matrix pipe, the rank walked in ascending blocks of 32, one fresh
 * accumulator per adapter, total = fma(coef[i], acc_i, total) in list order.  f32: the same order with plain f32 FMAs.
 * Blocks until the transposed, rank-padded operand copies it makes are released. */
int ltx_op_lora_merge(const void* w0, void* out, int64_t N, int K, int n, const void* const* A, const void* const* B,
                      const int* r, const float* coef, int dtype, ltx_stream stream);

#ifdef __cplusplus
}
#endif
#endif
