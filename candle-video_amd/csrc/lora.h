// LoRA adapters (include/ltxhip_lora.h): what lora.hip (kernel, adapter objects) and dit.hip (handle state) share.
#pragma once
#include <string>
#include <vector>
#include "model_util.h"
#include "../../include/ltxhip_lora.h"

constexpr int kLoraMaxAdapters = 8, kLoraMaxRank = 256, kLoraLinears = 10;

// One merge launch: out[N, K] = round(f32(w0) + sum_i coef[i] * (B_i A_i)).  The operands arrive PACKED (ltx_launch_lora_pack):
// At[i] [K, r_pad[i]] (A transposed) and Bp[i] [N, r_pad[i]], the rank zero padded to a multiple of 32, so that both are read
// along the rank in 16-byte pieces and the kernel masks rows only.
struct LoraMergeArgs {
    const void* w0 = nullptr; void* out = nullptr; int64_t N = 0; int K = 0; int n = 0;
    const void* At[kLoraMaxAdapters] = {}; const void* Bp[kLoraMaxAdapters] = {};
    int r_pad[kLoraMaxAdapters] = {}; float coef[kLoraMaxAdapters] = {};
};
static inline int ltx_lora_rank_pad(int r) { return (r + 31) / 32 * 32; }
int ltx_launch_lora_merge(const LoraMergeArgs& a, int dtype, hipStream_t s);
// dst [rows, r_pad] (ddt) from src: transpose == 0: [rows, r];  1: [r, rows]  (sdt), columns r..r_pad zero
int ltx_launch_lora_pack(const void* src, int sdt, void* dst, int ddt, int64_t rows, int r, int r_pad, int transpose, hipStream_t s);

struct LoraEntry {                   // one targeted linear of one adapter
    int block = 0, which = 0, r = 0, r_pad = 0;
    float factor = 1.f;              // alpha / r, or 1
    void* At = nullptr; void* Bp = nullptr;      // [in, r_pad], [out, r_pad] model dtype
};
struct ltx_lora {
    ltx_dit_config cfg{}; int dtype = LTX_DT_BF16, device = 0;
    std::vector<LoraEntry> entries;
};
// (dit.hip) what an adapter is bound to
void ltx_dit_describe(const ltx_dit* m, ltx_dit_config* cfg, int* dtype, int* device);
// shape of linear `which` (0..9) under a config: rows, columns
static inline void ltx_lora_linear_shape(const ltx_dit_config& c, int which, int* out, int* in) {
    const int D = c.num_attention_heads * c.attention_head_dim;
    *out = which == 8 ? 4 * D : D;
    *in = which == 9 ? 4 * D : (which == 5 || which == 6) ? c.cross_attention_dim : D;
}
