// LtxVideoTransformer3DModel on MI355X: weight ingestion + forward orchestration.
// Reference: src/models/ltx_video/ltx_transformer.rs (:957-1022 ctor, :1029-1172 forward,
// :820-937 block, :648-750 attention).  One kernel launch per fused stage:
//   per block: rms+AdaLN | fused QKV GEMM | qk-RMSNorm+RoPE | flash attention | to_out GEMM (+gate*x+h)
//              | q GEMM | q-norm | (k,v GEMM | k-norm) | cross attention (key bias) | to_out GEMM (+h)
//              | rms+AdaLN | FF1 GEMM (+GELU-tanh) | FF2 GEMM (+gate*x+h)
#include <cstring>
#include <deque>
#include "model_util.h"
#include "options.h"
#include "../../include/ltxhip_cond.h"
#include "../../include/ltxhip_stg.h"
#include "../../include/ltxhip_stepcache.h"
#include "../../include/ltxhip_int8.h"
#include "../host/step_cache.h"
#include "lora.h"

struct DitBlock {
    LinearW qkv1, o1, q2, kv2, o2, ff1, ff2;
    void *nq1 = nullptr, *nk1 = nullptr, *nq2 = nullptr, *nk2 = nullptr;
};

struct DitCtx {                      // cached text context (text_context below)
    const void* enc = nullptr; const float* mask = nullptr;
    int B = 0, K = 0, iodt = 0; bool valid = false;
    bool fold_q2 = false;            // k additionally carries attn2.norm_q.weight (the q-norm folded into cross attention)
    DevBuf kv, bias;                 // [L][B*K][2D] (k already RMS-normed), [B*K]
    // keys the mask leaves alive, compacted to the front of every batch row (AttnArgs::k_count): the cross-attention kernel then
    // multiplies ceil(count / 32) key blocks instead of ceil(K / 32) - BASELINE's prompts keep 32 of 128 text tokens
    bool compact = false;
    DevBuf kvc, biasc, kidx, kcount; // [L][B*K][2D], [B*K] f32, [B*K] int, [B] int
    // attn2.to_out folded into the context (xattn_fold.hip; compact contexts that ltx_xattn_fold_route accepts): vo = V Wo2^T per
    // layer and batch row, [L][B][D][H * KP] - a function of the prompt AND the weights.  KP: the widest row's kept keys, rounded up
    // to the cross kernel's 32-key block, read back from kcount once per context build.
    bool fold_vo = false, vo_oom = false; int KP = 0, fold_opt = 0;      // fold_opt: option xattn_fold_vo when the entry was built (part of its key); vo_oom: no memory for vo
    DevBuf vo, votab; std::vector<XFoldPtrs> votab_host; int counts_host[8] = {0};
    void release() { kv.release(); bias.release(); kvc.release(); biasc.release(); kidx.release(); kcount.release(); vo.release(); votab.release(); valid = false; }
};

// AdaLayerNormSingle's output for one set of timesteps (ltx_transformer.rs:262-309): a function of the timestep values and the
// weights alone, so the chain (sinusoid -> Linear -> SiLU -> Linear -> SiLU -> Linear(6D) -> + tables: 8 launches per forward) runs
// once per distinct timestep vector of a model and stream; a sampler revisits the same few timesteps for every video.
struct DitTimeEntry {
    float t[8] = {0}; int B = 0; hipStream_t stream = nullptr; bool valid = false; uint64_t used = 0;
    DevBuf ada, adaf;                // [L][B][6D] f32, [2][B][D] f32
    DevBuf cfold; bool cfold_valid = false;      // norm fold: per layer [B][3D] (shift_msa . W_qkv^T + b_qkv) then [B][4D] (shift_mlp . W_ff1^T + b_ff1), f32
    void release() { ada.release(); adaf.release(); cfold.release(); valid = cfold_valid = false; }
};
// norm fold through the weights (norm_fold=2): per layer W_qkv (.) (1 + scale_msa) [3D, D] then W_ff1 (.) (1 + scale_mlp) [4D, D], model dtype.
// Keyed by the TIMESTEP alone (the modulation of a row depends on nothing else): forwards of any batch size at that timestep share the copy.
struct DitWfold {
    float t = 0.f; hipStream_t stream = nullptr; bool valid = false; uint64_t used = 0; DevBuf w;
    void release() { w.release(); valid = false; }
};
constexpr int kDitTimeEntries = 64;
// Per-frame timesteps (ltx_dit_forward_frames): the modulation tables of one [B, G] timestep matrix, one row per (batch row, latent
// frame) - the layouts of DitTimeEntry with B * G modulation groups in place of B batch rows.  Built by a gather from the entries of
// the DISTINCT values (the MLP never runs twice for one value) and keyed on the whole matrix.  A sampler uses one matrix per step: a
// schedule of at most kDitGroupEntries steps (the distilled presets' 7) finds every table again in its next call, a longer one
// gathers its tables anew at every step - launches only (the values' entries stay cached), no wait for the device.
struct DitGroupEntry {
    std::vector<float> t; int B = 0, G = 0; hipStream_t stream = nullptr; bool valid = false; uint64_t used = 0;
    DevBuf ada, adaf, cfold; bool cfold_valid = false;      // [L][B*G][6D], [2][B*G][D], per layer [B*G][3D] then [B*G][4D]
    void release() { ada.release(); adaf.release(); cfold.release(); valid = cfold_valid = false; }
};
constexpr int kDitGroupEntries = 8;

struct ltx_dit {
    ltx_dit_config cfg{};
    int dtype = LTX_DT_BF16;
    int device = 0;
    int D = 0;
    LinearW proj_in, te1, te2, te_lin, cap1, cap2, proj_out;
    void* sst_final = nullptr;       // [2, D]
    void* sst_blocks = nullptr;      // [L, 6, D]
    std::vector<DitBlock> blocks;
    float* rope_freqs = nullptr;     // [D/6]
    float* inv_freq = nullptr;       // [128]
    std::vector<int> skip_blocks;
    int stg_mode = LTX_STG_TRANSFORMER_BLOCK;      // what a skip_layer_mask perturbs (include/ltxhip_stg.h): handle state, like the skip list
    // The five caches of the forward: text_context, time_tables, scaled_weights, group_tables, rope_tables (the last one is rope_key
    // over cosb / sinb: a function of the geometry, not of the weights, and owns no memory).
    std::deque<DitCtx> ctxs;         // deque: entries must not move while `ctx` points at one
    bool ctx_mode = false;
    std::deque<DitTimeEntry> tcache; uint64_t tclock = 0;
    std::deque<DitWfold> wcache;
    std::deque<DitGroupEntry> gcache;
    bool wfold_off = false;          // norm_fold=2 gave up on this handle: more distinct timesteps in flight than scaled-weight copies (a schedule that would re-scale every step), or no memory for a copy
    // RoPE tables of the caching scope (ltx_dit_context_cache: the caller keeps coords / geometry constant inside it): what cosb / sinb hold
    struct { bool valid = false; const float* coords = nullptr; float rs[3] = {0, 0, 0}; bool has_rs = false; int B = 0, S = 0, F = 0, H = 0, W = 0; hipStream_t stream = nullptr; } rope_key;
    // every cache that is a function of the weights (wcache keeps its allocations; wfold_off and the GEMM plans are not touched):
    // the scaled-weight copies, the text contexts (k / v projections and vo = V Wo2^T, DitCtx), the norm fold's per-timestep vectors.
    // A cache added to the forward is added HERE and to release_caches.  Caches that live outside the handle (ltx_step_cache: its
    // residuals are block outputs) compare weights_epoch instead.
    uint64_t weights_epoch = 0;
    void invalidate_weight_derived() {
        ++weights_epoch;
        for (auto& e : wcache) e.valid = false;
        for (auto& e : ctxs) e.valid = false;
        for (auto& e : tcache) e.cfold_valid = false;
        for (auto& e : gcache) e.cfold_valid = false;
        i8_stale = true;
    }
    void release_scaled_weights() { for (auto& e : wcache) e.release(); }      // norm_fold=2 gave up: the copies are never read again
    void release_caches() { auto all = [](auto& c) { for (auto& e : c) e.release(); c.clear(); }; all(ctxs); all(tcache); all(wcache); all(gcache); }
    std::vector<void*> owned;        // every hipMalloc'd weight pointer
    // LoRA (include/ltxhip_lora.h; ltx_dit_set_adapters below).  Per block and weight (qkv1, o1, q2, kv2, o2, ff1, ff2): the BASE
    // pointer, never written after the upload, and the merged second buffer of a targeted weight (null: not targeted).  LinearW::w
    // points at the merged buffer while adapters are active, so the forward reads one pointer either way.
    struct LoraSlots { void* base[7] = {nullptr}; void* merged[7] = {nullptr}; };
    std::vector<LoraSlots> lora_w;
    int n_adapters = 0;
    // INT8 (W8A8) block linears (include/ltxhip_int8.h; ltx_dit_set_int8_linears below).  Per block the mask of its int8 layers and, per
    // kind (bit order: qkv1, o1, ff1, ff2), the int8 copy [out, in] of the weight the forward would otherwise read and its per-channel
    // scales.  A weight-derived cache: invalidate_weight_derived marks the copies stale, the next forward (or set) re-makes them.
    struct I8Slots { void* w[4] = {nullptr}; float* sw[4] = {nullptr}; };
    std::vector<unsigned char> i8_mask;
    std::vector<I8Slots> i8_w;
    bool i8_any = false, i8_stale = false;
    DevBuf a8, a8s;                  // a quantised activation [M, 4D] int8 and its row scales [M] f32
    void free_int8(std::vector<void*>* later = nullptr, int l = -1, int k = -1) {      // every copy, or block l's kind k; later: collect instead of freeing
        for (size_t i = 0; i < i8_w.size(); ++i)
            for (int j = 0; j < 4; ++j) {
                if ((l >= 0 && (int)i != l) || (k >= 0 && j != k)) continue;
                void* ps[2] = {i8_w[i].w[j], i8_w[i].sw[j]};
                for (void* p : ps) if (p) { if (later) later->push_back(p); else (void)hipFree(p); }
                i8_w[i].w[j] = nullptr; i8_w[i].sw[j] = nullptr;
            }
    }
    // workspaces
    DevBuf xin, encin, h, n, qkv, attn, ff, c1, encp, kv2, tproj, e1, emb, embs, temb, ada, adaf, cosb, sinb, bias, orig, orig_hsq, outT, rsq, hsq, parts;
    void free_all() {
        for (void* p : owned) if (p) (void)hipFree(p);
        owned.clear();
        for (auto& ls : lora_w) for (void*& p : ls.merged) if (p) { (void)hipFree(p); p = nullptr; }
        lora_w.clear();
        free_int8(); i8_w.clear(); i8_mask.clear(); i8_any = false;
        a8.release(); a8s.release();
        DevBuf* bs[] = {&xin, &encin, &h, &n, &qkv, &attn, &ff, &c1, &encp, &kv2, &tproj, &e1, &emb, &embs, &temb, &ada, &adaf, &cosb, &sinb, &bias, &orig, &orig_hsq, &outT, &rsq, &hsq, &parts};
        for (DevBuf* b : bs) b->release();
        release_caches();
    }
};

// The step cache (include/ltxhip_stepcache.h): the previous measurement of block 0's modulated input, the block residuals per cache
// row, and the policy's two words of state (host/step_cache.h).
struct ltx_step_cache {
    ltx_dit* dit = nullptr;
    struct Row { bool valid = false; int S = 0; uint64_t epoch = 0; };
    std::vector<Row> rows;
    DevBuf prev, resid, parts, sums;      // [B * S, D] model dtype; [rows][resid_S][D] model dtype; f64 pairs; f64 [2]
    int64_t prev_rows = 0; int resid_S = 0;
    double* host = nullptr;               // pinned [2]
    hipStream_t stream = nullptr; bool used = false;      // the stream of the last launch that touched the buffers
    StepCacheState st;
    void forget() { st = StepCacheState(); for (auto& r : rows) r.valid = false; }
    void* resid_row(int row) const { return (char*)resid.p + (size_t)row * resid_S * dit->D * ltx_dt_size(dit->dtype); }
    // null: row holds a residual for S under the present weights; else why not
    const char* row_unusable(int row, int S) const {
        const Row& r = rows[(size_t)row];
        if (!r.valid) return "holds no residual (never computed, or the cache was reset)";
        if (r.S != S) return "holds the residual of another sequence length";
        if (r.epoch != dit->weights_epoch) return "holds a residual of other weights (the adapters changed)";
        return nullptr;
    }
};
struct StepCacheUse { ltx_step_cache* c = nullptr; int row0 = 0; bool reuse = false; };      // a forward through cache rows [row0, row0 + B)

namespace {

int own_linear(ltx_dit* m, const WeightMap& wm, const std::string& prefix, int in, int out, LinearW* l) {
    LTX_TRY(ltx_load_linear(wm, prefix, in, out, m->dtype, l));
    m->owned.push_back(l->w); if (l->b) m->owned.push_back(l->b);
    return LTX_OK;
}
int own_tensor(ltx_dit* m, const WeightMap& wm, const std::string& name, int64_t numel, void** out) {
    LTX_TRY(ltx_load_tensor(wm, name, numel, m->dtype, out));
    m->owned.push_back(*out);
    return LTX_OK;
}
// fused [sum(out_i), in] linear from several reference linears sharing the same input
int own_fused(ltx_dit* m, const WeightMap& wm, const std::vector<std::string>& prefixes, int in, int out_each, LinearW* l) {
    const int n = (int)prefixes.size();
    const size_t esz = ltx_dt_size(m->dtype);
    l->in = in; l->out = out_each * n;
    HIP_TRY(hipMalloc(&l->w, (size_t)l->out * in * esz)); m->owned.push_back(l->w);
    bool has_bias = wm.find(prefixes[0] + ".bias") != nullptr;
    if (has_bias) { HIP_TRY(hipMalloc(&l->b, (size_t)l->out * esz)); m->owned.push_back(l->b); }
    for (int i = 0; i < n; ++i) {
        const ltx_weight* w = wm.find(prefixes[i] + ".weight");
        if (!w) LTX_FAIL(LTX_ERR_MISSING_WEIGHT, "missing weight '" + prefixes[i] + ".weight'");
        LTX_TRY(ltx_upload_cast(w, (char*)l->w + (size_t)i * out_each * in * esz, m->dtype, (int64_t)out_each * in, prefixes[i] + ".weight"));
        if (has_bias) {
            const ltx_weight* b = wm.find(prefixes[i] + ".bias");
            if (!b) LTX_FAIL(LTX_ERR_MISSING_WEIGHT, "missing weight '" + prefixes[i] + ".bias'");
            LTX_TRY(ltx_upload_cast(b, (char*)l->b + (size_t)i * out_each * esz, m->dtype, out_each, prefixes[i] + ".bias"));
        }
    }
    return LTX_OK;
}

int build(ltx_dit* m, const ltx_weight* weights, size_t n_weights) {
    const ltx_dit_config& c = m->cfg;
    const int D = m->D, L = c.num_layers;
    WeightMap wm(weights, n_weights);
    LTX_TRY(own_linear(m, wm, "proj_in", c.in_channels, D, &m->proj_in));
    LTX_TRY(own_tensor(m, wm, "scale_shift_table", 2 * (int64_t)D, &m->sst_final));
    LTX_TRY(own_linear(m, wm, "time_embed.emb.timestep_embedder.linear_1", 256, D, &m->te1));
    LTX_TRY(own_linear(m, wm, "time_embed.emb.timestep_embedder.linear_2", D, D, &m->te2));
    LTX_TRY(own_linear(m, wm, "time_embed.linear", D, 6 * D, &m->te_lin));
    LTX_TRY(own_linear(m, wm, "caption_projection.linear_1", c.caption_channels, D, &m->cap1));
    LTX_TRY(own_linear(m, wm, "caption_projection.linear_2", D, D, &m->cap2));
    LTX_TRY(own_linear(m, wm, "proj_out", D, c.out_channels, &m->proj_out));
    const size_t esz = ltx_dt_size(m->dtype);
    HIP_TRY(hipMalloc(&m->sst_blocks, (size_t)L * 6 * D * esz)); m->owned.push_back(m->sst_blocks);
    m->blocks.resize(L);
    for (int i = 0; i < L; ++i) {
        const std::string p = "transformer_blocks." + std::to_string(i) + ".";
        DitBlock& b = m->blocks[i];
        LTX_TRY(own_fused(m, wm, {p + "attn1.to_q", p + "attn1.to_k", p + "attn1.to_v"}, D, D, &b.qkv1));
        LTX_TRY(own_linear(m, wm, p + "attn1.to_out.0", D, D, &b.o1));
        LTX_TRY(own_tensor(m, wm, p + "attn1.norm_q.weight", D, &b.nq1));
        LTX_TRY(own_tensor(m, wm, p + "attn1.norm_k.weight", D, &b.nk1));
        LTX_TRY(own_linear(m, wm, p + "attn2.to_q", D, D, &b.q2));
        LTX_TRY(own_fused(m, wm, {p + "attn2.to_k", p + "attn2.to_v"}, c.cross_attention_dim, D, &b.kv2));
        LTX_TRY(own_linear(m, wm, p + "attn2.to_out.0", D, D, &b.o2));
        LTX_TRY(own_tensor(m, wm, p + "attn2.norm_q.weight", D, &b.nq2));
        LTX_TRY(own_tensor(m, wm, p + "attn2.norm_k.weight", D, &b.nk2));
        LTX_TRY(own_linear(m, wm, p + "ff.net.0.proj", D, 4 * D, &b.ff1));
        LTX_TRY(own_linear(m, wm, p + "ff.net.2", 4 * D, D, &b.ff2));
        const ltx_weight* t = wm.find(p + "scale_shift_table");
        if (!t) LTX_FAIL(LTX_ERR_MISSING_WEIGHT, "missing weight '" + p + "scale_shift_table'");
        LTX_TRY(ltx_upload_cast(t, (char*)m->sst_blocks + (size_t)i * 6 * D * esz, m->dtype, 6 * (int64_t)D, p + "scale_shift_table"));
    }
    // RoPE frequency table: theta^linspace(0,1,D/6) * pi/2 with the reference's f32 roundings
    // (ltx_transformer.rs:475-488); exp evaluated correctly rounded (double -> f32).
    {
        int steps = D / 6; if (steps < 1) steps = 1;
        std::vector<float> fr(steps);
        const float theta_ln = (float)std::log(10000.0);
        for (int i = 0; i < steps; ++i) {
            float lin = steps <= 1 ? 0.0f : (float)i * (float)(1.0 / (double)(steps - 1));
            float x = lin * theta_ln;
            float e = (float)std::exp((double)x);
            fr[i] = e * (float)(M_PI / 2.0);
        }
        HIP_TRY(hipMalloc((void**)&m->rope_freqs, sizeof(float) * steps)); m->owned.push_back(m->rope_freqs);
        HIP_TRY(hipMemcpy(m->rope_freqs, fr.data(), sizeof(float) * steps, hipMemcpyHostToDevice));
        // inv_freq_i = 1 / 10000^(i/128)  (ltx_transformer.rs:288-290)
        std::vector<float> inv(128);
        ltx_sinusoid_table(0, inv.data());
        HIP_TRY(hipMalloc((void**)&m->inv_freq, sizeof(float) * 128)); m->owned.push_back(m->inv_freq);
        HIP_TRY(hipMemcpy(m->inv_freq, inv.data(), sizeof(float) * 128, hipMemcpyHostToDevice));
    }
    return LTX_OK;
}

// the seven weights of a block in the order of ltx_dit::LoraSlots; the ten LoRA targets (ltxhip_lora.h's `which`) as
// (weight, row part of a fused weight)
LinearW* dit_slot(DitBlock& b, int slot) {
    LinearW* const ws[7] = {&b.qkv1, &b.o1, &b.q2, &b.kv2, &b.o2, &b.ff1, &b.ff2};
    return ws[slot];
}
constexpr int kLoraSlot[kLoraLinears] = {0, 0, 0, 1, 2, 3, 3, 4, 5, 6}, kLoraPart[kLoraLinears] = {0, 1, 2, 0, 0, 0, 1, 0, 0, 0};
constexpr int kSlotParts[7] = {3, 1, 1, 2, 1, 1, 1}, kSlotFirst[7] = {0, 3, 4, 5, 7, 8, 9};

}  // namespace

extern "C" int ltx_dit_create(const ltx_dit_config* cfg, const ltx_weight* weights, size_t n_weights,
                              ltx_dtype model_dtype, int device, ltx_dit** out) {
    if (!cfg || !weights || !out) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_create: null argument");
    *out = nullptr;
    const int hd = cfg->attention_head_dim;
    if (hd != 16 && hd != 32 && hd != 64 && hd != 128) LTX_FAIL(LTX_ERR_UNSUPPORTED, "attention_head_dim must be 16/32/64/128");
    const int D = cfg->num_attention_heads * hd;
    if (D % 8 != 0 || cfg->in_channels % 8 != 0 || cfg->out_channels % 8 != 0 || cfg->caption_channels % 8 != 0 || cfg->cross_attention_dim % 8 != 0)
        LTX_FAIL(LTX_ERR_UNSUPPORTED, "channel dims must be multiples of 8");
    if (cfg->cross_attention_dim != D) LTX_FAIL(LTX_ERR_UNSUPPORTED, "cross_attention_dim must equal inner_dim (caption projection output feeds attn2)");
    if (cfg->num_layers < 1) LTX_FAIL(LTX_ERR_ARG, "num_layers must be >= 1");
    HIP_TRY(hipSetDevice(device));
    ltx_dit* m = new ltx_dit();
    m->cfg = *cfg; m->dtype = model_dtype == LTX_BF16 ? LTX_DT_BF16 : LTX_DT_F32; m->device = device; m->D = D;
    int rc = build(m, weights, n_weights);
    if (rc == LTX_OK && cfg->attention_head_dim == 128 && m->dtype == LTX_DT_BF16) rc = ltx_attention_q128_prepare();
    if (rc != LTX_OK) { m->free_all(); delete m; return rc; }
    m->lora_w.resize(m->blocks.size());
    for (size_t l = 0; l < m->blocks.size(); ++l)
        for (int slot = 0; slot < 7; ++slot) m->lora_w[l].base[slot] = dit_slot(m->blocks[l], slot)->w;
    *out = m;
    return LTX_OK;
}

extern "C" void ltx_dit_destroy(ltx_dit* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    (void)hipDeviceSynchronize();
    m->free_all();
    delete m;
}

extern "C" int ltx_dit_set_skip_blocks(ltx_dit* m, const int* blocks, int n) {
    if (!m || n < 0 || (n > 0 && !blocks)) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_set_skip_blocks: bad argument");
    m->skip_blocks.assign(blocks, blocks + n);
    return LTX_OK;
}

// ---- STG modes (include/ltxhip_stg.h) ----
extern "C" int ltx_dit_set_stg_mode(ltx_dit* m, ltx_stg_mode mode) {
    if (!m) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_set_stg_mode: null handle");
    const int v = (int)mode;
    if (v != LTX_STG_TRANSFORMER_BLOCK && v != LTX_STG_ATTENTION_SKIP && v != LTX_STG_ATTENTION_VALUES)
        LTX_FAIL(LTX_ERR_ARG, "ltx_dit_set_stg_mode: unknown mode " + std::to_string(v) + " (0 transformer_block, 1 attention_skip, 2 attention_values)");
    m->stg_mode = v;
    return LTX_OK;
}
extern "C" int ltx_dit_get_stg_mode(const ltx_dit* m, ltx_stg_mode* out) {
    if (!m || !out) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_get_stg_mode: null argument");
    *out = (ltx_stg_mode)m->stg_mode;
    return LTX_OK;
}

extern "C" int ltx_dit_get_config(const ltx_dit* m, ltx_dit_config* out) {
    if (!m || !out) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_get_config: null argument");
    *out = m->cfg;
    return LTX_OK;
}

// ---- INT8 (W8A8) block linears (include/ltxhip_int8.h) ----
namespace {
constexpr int kI8Slot[4] = {0, 1, 5, 6};      // dit_slot's index of mask bit i: qkv1, o1, ff1, ff2
// (re-)quantise every selected weight from the pointer the forward reads (LinearW::w: the base, or the LoRA-merged copy)
int int8_quantise(ltx_dit* m, hipStream_t s) {
    for (size_t l = 0; l < m->i8_mask.size(); ++l)
        for (int k = 0; k < 4; ++k) {
            if (!(m->i8_mask[l] >> k & 1)) continue;
            const LinearW* lw = dit_slot(m->blocks[l], kI8Slot[k]);
            LTX_TRY(ltx_launch_quant_rows_i8(lw->w, lw->out, lw->in, lw->in, m->i8_w[l].w[k], m->i8_w[l].sw[k], s));
        }
    m->i8_stale = false;
    return LTX_OK;
}
}  // namespace

extern "C" int ltx_dit_set_int8_linears(ltx_dit* m, const unsigned char* block_masks, unsigned char mask, ltx_stream stream) {
    if (!m) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_set_int8_linears: null handle");
    const int L = m->cfg.num_layers;
    if (mask & ~LTX_I8_ALL) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_set_int8_linears: mask " + std::to_string((int)mask) + " has bits outside LTX_I8_ALL");
    for (int l = 0; block_masks && l < L; ++l)
        if (block_masks[l] & ~LTX_I8_ALL) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_set_int8_linears: block_masks[" + std::to_string(l) + "] has bits outside LTX_I8_ALL");
    std::vector<unsigned char> want((size_t)L);
    bool any = false;
    for (int l = 0; l < L; ++l) { want[l] = block_masks ? (unsigned char)(block_masks[l] & mask) : mask; any = any || want[l]; }
    if (any && m->dtype != LTX_DT_BF16) LTX_FAIL(LTX_ERR_UNSUPPORTED, "ltx_dit_set_int8_linears: the int8 layers take a bf16 model (this handle is f32)");
    if (any && (m->D % 16 != 0 || m->D > 4096)) LTX_FAIL(LTX_ERR_UNSUPPORTED, "ltx_dit_set_int8_linears: the inner dimension must be a multiple of 16, at most 4096");
    HIP_TRY(hipSetDevice(m->device));
    m->i8_mask.resize((size_t)L, 0); m->i8_w.resize((size_t)L);
    // new copies first: nothing changes before every one of them exists
    std::vector<std::pair<int, int>> fresh;
    for (int l = 0; l < L; ++l)
        for (int k = 0; k < 4; ++k) {
            if (!(want[l] >> k & 1) || m->i8_w[l].w[k]) continue;
            const LinearW* lw = dit_slot(m->blocks[l], kI8Slot[k]);
            void* w = nullptr; void* sw = nullptr;
            hipError_t e = hipMalloc(&w, (size_t)lw->out * lw->in);
            if (e == hipSuccess) e = hipMalloc(&sw, (size_t)lw->out * sizeof(float));
            if (e != hipSuccess) {
                (void)hipGetLastError();
                if (w) (void)hipFree(w);
                for (const auto& f : fresh) m->free_int8(nullptr, f.first, f.second);
                LTX_FAIL(LTX_ERR_HIP, std::string("ltx_dit_set_int8_linears: hipMalloc of an int8 weight: ") + hipGetErrorString(e) + " (the handle is unchanged)");
            }
            m->i8_w[l].w[k] = w; m->i8_w[l].sw[k] = reinterpret_cast<float*>(sw); fresh.emplace_back(l, k);
        }
    std::vector<void*> unused;
    for (int l = 0; l < L; ++l)
        for (int k = 0; k < 4; ++k)
            if (!(want[l] >> k & 1)) m->free_int8(&unused, l, k);
    m->i8_mask = want; m->i8_any = any;
    const int rc = any ? int8_quantise(m, (hipStream_t)stream) : LTX_OK;
    if (!any) { m->i8_stale = false; }
    if (!unused.empty()) {                                       // forwards enqueued earlier may still read them
        (void)hipDeviceSynchronize();
        for (void* p : unused) (void)hipFree(p);
    }
    if (!any) { m->a8.release(); m->a8s.release(); }
    return rc;
}
extern "C" int ltx_dit_get_int8_linears(const ltx_dit* m, unsigned char* block_masks_out) {
    if (!m || !block_masks_out) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_get_int8_linears: null argument");
    for (int l = 0; l < m->cfg.num_layers; ++l) block_masks_out[l] = (size_t)l < m->i8_mask.size() ? m->i8_mask[(size_t)l] : 0;
    return LTX_OK;
}

// ---- the GEMMs of a block: one builder per call, used by the plan's fit tests (stand-in operands) and by dit_block (the real ones) ----
namespace {
enum DitForm { kPass,        // the plain call (the norm before it, where there is one, ran as a pass)
               kFold1,       // norm fold: a producer (o2 / ff2) also stores h (.) (1 + scale) into n, a consumer (qkv1 / ff1) reads n and finishes with the row's 1 / rms and cvec
               kFold2,       // norm_fold=2: the consumer reads h and the timestep's scaled weights (the producers run their pass form)
               kDefer };     // ff2 alone: the K ranges are left in parts for the row norm that follows
struct DitOperands {          // the handle's workspaces and one layer's table rows - or aligned non-null stand-ins: a fit test, nothing is launched
    void *h, *n, *qkv, *attn, *ff; float *rsq, *hsq, *parts;
    const float* ada;         // the layer's modulation [NB][6D]: shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp
    const float* ada_next;    // ... of the next block that runs (null: none)
    const float* cfold;       // norm fold: the layer's [NB][3D] then [NB][4D]
    const char* wfold;        // norm_fold=2: the layer's scaled q|k|v then ff1 weights
    float eps;
};
GemmArgs gemm_base(const DitPlan& p, const LinearW& w, const void* A, int lda, void* C, int ldc) {
    GemmArgs g; g.A = A; g.W = w.w; g.C = C; g.bias = w.b; g.M = (int)p.M; g.N = w.out; g.K = w.in; g.lda = lda; g.ldc = ldc;
    return g;
}
// a consumer of the norm fold: out = epi(r_m * acc + cvec), r_m from the producer's row partials; form 2 reads h through the scaled weights
void fold_in(GemmArgs& g, const DitPlan& p, DitForm f, const DitOperands& x, size_t cvec_at, size_t wfold_at) {
    g.bias = nullptr; g.rows_per_batch = p.Sg; g.rs_sq = x.hsq; g.rs_n = p.D / 128; g.rs_D = p.D; g.rs_eps = x.eps; g.cvec = x.cfold + cvec_at; g.cvec_stride = g.N;
    if (f == kFold2) { g.A = x.h; g.W = x.wfold + wfold_at; }
}
// q, k, v leave the fused projection as three DENSE [M, D] matrices (segmented GEMM output) when D is a power
// of two: the attention kernel reads K/V rows of a dense matrix 7-11 % faster than column slices of [M, 3D]
GemmArgs gemm_qkv1(const DitPlan& p, DitForm f, const DitBlock& b, const DitOperands& x) {
    GemmArgs g = gemm_base(p, b.qkv1, x.n, p.D, x.qkv, p.ldqkv);
    if (p.dense_qkv) { g.c_seg_shift = __builtin_ctz((unsigned)p.D); g.c_seg_stride = p.seg; }
    if (f != kPass) fold_in(g, p, f, x, 0, 0);
    return g;
}
GemmArgs gemm_q2(const DitPlan& p, const DitBlock& b, const DitOperands& x) {      // fold_q2: + the row partials of q for the attention kernel
    GemmArgs g = gemm_base(p, b.q2, x.h, p.D, x.qkv, p.D);
    if (p.fold_q2) g.rowsq = x.rsq;
    return g;
}
// to_out folded into the text context (DitCtx::vo): batch row `row` alone - its weights are its own - reads the probabilities
// (x.attn as [M, HK]) against vo [D, HK] of the layer and row; HK = heads * KP
struct DitVo { const void* w = nullptr; int HK = 0, row = 0; };
GemmArgs gemm_o2(const DitPlan& p, DitForm f, const DitBlock& b, const DitOperands& x, const DitVo* vo = nullptr) {      // h += to_out(attn); fold 1: + h (.) (1 + scale_mlp) into n for ff1
    GemmArgs g = gemm_base(p, b.o2, x.attn, p.D, x.h, p.D);
    g.resid = x.h; g.ldr = p.D; g.rowsq = p.presum ? x.hsq : nullptr;
    if (f == kFold1) { g.rows_per_batch = p.Sg; g.C2 = x.n; g.scale2 = x.ada + 4 * p.D; g.scale2_stride = 6 * p.D; }
    if (vo) {
        const size_t esz = ltx_dt_size(p.dt), r0 = (size_t)vo->row * p.S;      // whole batch rows, and their table rows (NB / B per batch row)
        g.M = p.S; g.K = vo->HK; g.lda = vo->HK;
        g.W = (const char*)vo->w + (size_t)vo->row * p.D * vo->HK * esz;
        g.A = (const char*)x.attn + r0 * vo->HK * esz;
        g.C = (char*)x.h + r0 * p.D * esz; g.resid = g.C;
        if (g.rowsq) { g.rowsq += r0 * (p.D / 128); g.rowsq_in_epilogue = 1; }      // (vo_fits: the call reaches gemm_asm16 wherever the plan has presum)
        if (f == kFold1) { g.C2 = (char*)x.n + r0 * p.D * esz; g.scale2 += (size_t)vo->row * (p.NB / p.B) * 6 * p.D; }
    }
    return g;
}
GemmArgs gemm_ff1(const DitPlan& p, DitForm f, const DitBlock& b, const DitOperands& x) {
    GemmArgs g = gemm_base(p, b.ff1, x.n, p.D, x.ff, 4 * p.D);
    if (f != kPass) fold_in(g, p, f, x, (size_t)p.NB * 3 * p.D, (size_t)3 * p.D * p.D * ltx_dt_size(p.dt));
    return g;
}
// h += gate_mlp * ff2(ff); fold 1: + h (.) (1 + scale_msa of the next block that runs) into n for its q|k|v projection; deferred: a bare
// launch (no bias, gate or residual: RowNormArgs::parts finishes the rows)
GemmArgs gemm_ff2(const DitPlan& p, DitForm f, const DitBlock& b, const DitOperands& x) {
    GemmArgs g = gemm_base(p, b.ff2, x.ff, 4 * p.D, x.h, p.D);
    if (f == kDefer) { g.bias = nullptr; g.defer_parts = x.parts; return g; }
    g.resid = x.h; g.ldr = p.D; g.gate = x.ada + 5 * p.D; g.gate_stride = 6 * p.D; g.rows_per_batch = p.Sg; g.rowsq = p.presum ? x.hsq : nullptr;
    if (f == kFold1) { g.C2 = x.n; g.scale2 = x.ada_next + p.D; g.scale2_stride = 6 * p.D; }
    return g;
}
// a builder's plain form through ltx_linear, which writes the same fields from the same values
int linear_of(const LinearW& l, const GemmArgs& g, int dt, int epi, hipStream_t s) {
    return ltx_linear(l, g.A, g.lda, g.C, g.ldc, g.M, dt, epi, s, g.resid, g.ldr, g.gate, g.gate_stride, g.rows_per_batch, g.rowsq);
}
}  // namespace

// Which fusions a forward uses.  Each is decided by asking the kernel family that carries it whether it serves the call the block
// loop WILL launch: the builders above with stand-in operands (the fit tests read the pointers' alignment alone, and hipMalloc
// gives at least 256 bytes).  wf (norm_fold=2's scaled weights) is not here: it depends on the timestep values and the handle's state.
DitPlan ltx_dit_plan(const ltx_dit_config& c, int dt, int iodt, int B, int S, int K, int G, bool skip_mask) {
    DitPlan p; p.dt = dt; p.iodt = iodt; p.B = B; p.S = S; p.K = K;
    const int D = c.num_attention_heads * c.attention_head_dim, hd = c.attention_head_dim;
    p.D = D; p.M = (int64_t)B * S; p.MK = (int64_t)B * K; p.NB = B * G; p.Sg = S / G;
    p.dense_qkv = (D & (D - 1)) == 0 && ltx_opt().dense_qkv;      // dense_qkv=0: column slices of [M, 3D] (A/B aid, and the path of a D that is not a power of two)
    p.seg = p.dense_qkv ? p.M * D : D; p.ldqkv = p.dense_qkv ? D : 3 * D;
    // bf16: q leaves the norm already multiplied by scale*log2(e) (ONE bf16 rounding, of the product), so the
    // attention kernel's exponent is exp2(S - m) with no per-score multiply
    p.fold_q = dt == LTX_DT_BF16 && ltx_attention_prescale_ok(hd);
    const bool bf16 = dt == LTX_DT_BF16;
    void* const a = reinterpret_cast<void*>((uintptr_t)4096); float* const f = reinterpret_cast<float*>(a);
    auto lin = [&](int in, int out) { LinearW w; w.w = a; w.b = a; w.in = in; w.out = out; return w; };
    DitBlock b; b.qkv1 = lin(D, 3 * D); b.q2 = lin(D, D); b.o2 = lin(D, D); b.ff1 = lin(D, 4 * D); b.ff2 = lin(4 * D, D);
    const DitOperands x{a, a, a, a, a, f, f, f, f, f, f, (const char*)a, c.norm_eps};
    // Cross-attention q-norm folded into the attention kernel (bf16, head_dim 64, <= 128 text keys): scores are linear in q, so
    // rms_norm(q) . k = r_row * (q . (k * w_q)) - the q2 projection's epilogue leaves per-row partial sums of squares
    // (GemmArgs::rowsq), w_q = attn2.norm_q.weight rides on the cached k, and the stand-alone pass over q (read + write of
    // [M, D] per layer) disappears.  ltx_transformer.rs:671-678, 719-740.
    // Only where the projection can emit the partials from its own epilogue (a shape-only test: gemm_asm16's fit): behind any
    // other kernel they cost a stand-alone pass, which at small M (C1: 384 tokens) is dearer than the q-norm pass it replaces.
    p.fold_q2 = bf16 && ltx_attention_rowsq_ok(hd, K, D);
    if (p.fold_q2) p.fold_q2 = ltx_gemm_asm16_fits(gemm_q2(p, b, x), EPI_BIAS) || ltx_opt().q2_fold == 2;       // q2_fold=2: fold whatever the shape (tests of the stand-alone partials)
    // The two RMS norms of a block take their rows' sums of squares from the epilogue of the GEMM that wrote h (ff2 of the block
    // before, attn2.to_out of this block: GemmArgs::rowsq) and run as a pure elementwise map; same shape-only condition as the
    // fold above (the partials must come from gemm_asm16's epilogue).  LTX_NORM_PRESUM=0: the row-reducing pass (A/B aid); "2" forces
    // the map whatever the shape (tests).  What it buys is not the missing reduction (a first map, one chunk per thread, took the same
    // 13.5 us per launch) but operand re-use: with four rows per thread the 64 B of f32 modulation per 16-byte chunk are loaded once
    // per four chunks - 13.7 -> 11.0 us per launch, 7.3 -> 6.3 ms of norm passes per video against +0.5 ms in the two epilogues
    // (docs/lab_notes.md R4.4 / R4.7).
    p.presum = bf16 && D % 512 == 0 && (D & (D - 1)) == 0 && D <= 2048;
    if (const int pe = ltx_opt().norm_presum; p.presum)
        p.presum = (pe != 0 && ltx_gemm_asm16_fits(gemm_o2(p, kPass, b, x), EPI_RESID) && ltx_gemm_asm16_fits(gemm_ff2(p, kPass, b, x), EPI_GATE_RESID)) || pe == 2;
    // Norm fold (round 6; GemmArgs::C2 / ::rs_sq, kernels.h): with the partials in hand the norm pass between the layer that writes h
    // and the layer that reads the normalised rows is gone altogether - norm(h) * (1 + sc) + sh times W^T is
    // r_m * ((h (.) (1 + sc)) W^T) + (sh W^T + b): out2 / ff2 also store h (.) (1 + sc_next) into m->n, qkv / ff1 read it and finish
    // with the row's 1 / rms and the per-timestep vector sh W^T + b (cached with the timestep's modulation).  One rounding less than
    // the pass (bf16 of h (1 + sc) instead of bf16 of the modulated, normalised row); norm_fold=0: the pass (A/B arm).
    p.nfold = p.presum && ltx_opt().norm_fold != 0 && p.dense_qkv &&
              ltx_gemm_fold_ok(gemm_o2(p, kFold1, b, x), EPI_RESID) && ltx_gemm_fold_ok(gemm_ff2(p, kFold1, b, x), EPI_GATE_RESID) &&
              ltx_gemm_fold_ok(gemm_qkv1(p, kFold1, b, x), EPI_BIAS) && ltx_gemm_fold_ok(gemm_ff1(p, kFold1, b, x), EPI_GELU);
    // Few tokens (C1's 384: every linear layer is a latency-bound weight stream): ff2, the deepest one (K = 4 D), runs its K ranges as
    // separate blocks (the shape rule: four ranges from K = 8192 up) and leaves their f32 sums in m->parts; the row norm that follows
    // the block - the next block's norm1, or the final LayerNorm - adds them in part order, applies gate * y + h, writes h and goes on
    // normalising the row it has just finished (GemmArgs::defer_parts / RowNormArgs::parts).  Same K partition and order as the
    // in-launch reduction: the same bits.  ff2_defer=0: the in-launch reduction (A/B aid).
    if (bf16 && !skip_mask && ltx_opt().ff2_defer && !p.presum) {
        const GemmArgs g = gemm_ff2(p, kDefer, b, x);
        const int parts = ltx_gemm_split_factor(g);
        if (p.M <= 512 && parts > 1 && ltx_gemm_defer_ok(g, EPI_GATE_RESID)) { p.defer_ff2 = true; p.ff2_parts = parts; }
    }
    return p;
}

namespace {
// ---- the caches of a forward ----
// One policy for the time, group and scaled-weight tables: a valid entry that matches (*hit), else an invalid slot, else a new one
// while there are fewer than cap, else the least recently used.  What a miss does with the slot, and whether it first waits for
// the stream of a victim that is still valid, is the caller's.
template <class E, class Match>
E* cache_slot(std::deque<E>& c, size_t cap, Match match, bool* hit) {
    E *found = nullptr, *lru = nullptr;
    for (auto& e : c) if (e.valid && match(e)) found = &e;
    if ((*hit = found != nullptr)) return found;
    for (auto& e : c) if (!e.valid) return &e;
    if (c.size() < cap) { c.emplace_back(); return &c.back(); }
    for (auto& e : c) if (!lru || e.used < lru->used) lru = &e;
    return lru;
}
struct DitTables { const float *ada = nullptr, *adaf = nullptr, *cfold = nullptr; };      // [L][NB][6D], [2][NB][D], per layer [NB][3D] then [NB][4D] (norm fold; else null)
// AdaLayerNormSingle (:262-267): sinusoid(256) -> Linear -> SiLU -> Linear = embedded_timestep ; SiLU -> Linear(6D) = temb.
// The cached tables of up to 8 timestep values - the rows of a call with one timestep per row - computed on a miss, with the norm fold's per-timestep vectors where the plan folds.
// Unlike the two caches below, a miss does NOT wait for the stream of the entry it overwrites.  On the stream of this call the stream
// orders the writes behind the readers.  A victim of ANOTHER stream is safe only because two forwards of one handle share every
// workspace (m->h, m->tproj, ...), so a caller with two streams has to order the forwards itself; read by the letter of
// gcache / wcache, which do wait, this is the cache that would have to learn it (left as it was: a follow-up).
int time_tables(ltx_dit* m, const DitPlan& p, const float* vals, int nv, hipStream_t s, DitTables* t) {
    const int D = p.D, L = m->cfg.num_layers, dt = p.dt;
    TimeVec tv; tv.n = nv; for (int i = 0; i < 8; ++i) tv.t[i] = i < nv ? vals[i] : 0.f;
    bool hit;
    DitTimeEntry* te = cache_slot(m->tcache, kDitTimeEntries, [&](const DitTimeEntry& e) { return e.B == nv && e.stream == s && !memcmp(e.t, tv.t, sizeof(float) * nv); }, &hit);
    if (!hit) {
        te->valid = false; te->cfold_valid = false;
        LTX_TRY(te->ada.ensure((size_t)L * nv * 6 * D * sizeof(float))); LTX_TRY(te->adaf.ensure((size_t)2 * nv * D * sizeof(float)));
        LTX_TRY(ltx_launch_sinusoid(m->tproj.p, dt, tv, m->inv_freq, 128, /*round_t=*/dt == LTX_DT_BF16, 1.0f, s));
        LTX_TRY(ltx_linear(m->te1, m->tproj.p, 256, m->e1.p, D, nv, dt, EPI_BIAS, s));
        LTX_TRY(ltx_launch_silu(m->e1.p, m->e1.p, (int64_t)nv * D, dt, s));
        LTX_TRY(ltx_linear(m->te2, m->e1.p, D, m->emb.p, D, nv, dt, EPI_BIAS, s));
        LTX_TRY(ltx_launch_silu(m->emb.p, m->embs.p, (int64_t)nv * D, dt, s));
        LTX_TRY(ltx_linear(m->te_lin, m->embs.p, D, m->temb.p, 6 * D, nv, dt, EPI_BIAS, s));
        LTX_TRY(ltx_launch_ada(te->ada.as<float>(), m->sst_blocks, m->temb.p, L, nv, 6 * D, dt, s));
        LTX_TRY(ltx_launch_ada(te->adaf.as<float>(), m->sst_final, m->emb.p, 2, nv, D, dt, s));
        memcpy(te->t, tv.t, sizeof(te->t)); te->B = nv; te->stream = s; te->valid = true;
    }
    te->used = ++m->tclock;
    if (p.nfold && !te->cfold_valid) {                      // once per distinct timestep vector: streams the q|k|v and ff1 weights of every layer once
        LTX_TRY(te->cfold.ensure((size_t)L * nv * 7 * D * sizeof(float)));
        for (int l = 0; l < L; ++l) {
            const float* ada = te->ada.as<float>() + (size_t)l * nv * 6 * D;
            float* cq = te->cfold.as<float>() + (size_t)l * nv * 7 * D;
            LTX_TRY(ltx_launch_shift_gemv(m->blocks[l].qkv1.w, m->blocks[l].qkv1.b, ada, 6 * D, nv, 3 * D, D, cq, 3 * D, s));
            LTX_TRY(ltx_launch_shift_gemv(m->blocks[l].ff1.w, m->blocks[l].ff1.b, ada + 3 * D, 6 * D, nv, 4 * D, D, cq + (size_t)nv * 3 * D, 4 * D, s));
        }
        te->cfold_valid = true;
    }
    *t = DitTables{te->ada.as<float>(), te->adaf.as<float>(), p.nfold ? te->cfold.as<float>() : nullptr};
    return LTX_OK;
}
// One timestep per (batch row, latent frame) (timestep [B, G]).  The MLP runs once per DISTINCT value of the call, eight values a
// launch (each batch of eight is an ordinary cached entry above: the held frames' 0 and the step's t are two values however many
// frames there are), and a gather copies every group's rows out of them.
int group_tables(ltx_dit* m, const DitPlan& p, const float* timestep, hipStream_t s, DitTables* t) {
    const int D = p.D, L = m->cfg.num_layers, NB = p.NB, B = p.B, G = NB / B;
    bool hit;
    DitGroupEntry* ge = cache_slot(m->gcache, kDitGroupEntries, [&](const DitGroupEntry& e) { return e.B == B && e.G == G && e.stream == s && !memcmp(e.t.data(), timestep, sizeof(float) * NB); }, &hit);
    if (!hit && ge->valid && ge->stream != s) HIP_TRY(hipStreamSynchronize(ge->stream));      // (forwards on ITS stream may still read the tables)
    if (!hit || (p.nfold && !ge->cfold_valid)) {
        ge->valid = false; ge->cfold_valid = false;
        std::vector<float> distinct; std::vector<int> idx((size_t)NB);
        for (int i = 0; i < NB; ++i) {
            size_t j = 0;
            while (j < distinct.size() && memcmp(&distinct[j], &timestep[i], sizeof(float)) != 0) ++j;
            if (j == distinct.size()) distinct.push_back(timestep[i]);
            idx[i] = (int)j;
        }
        LTX_TRY(ge->ada.ensure((size_t)L * NB * 6 * D * sizeof(float))); LTX_TRY(ge->adaf.ensure((size_t)2 * NB * D * sizeof(float)));
        if (p.nfold) LTX_TRY(ge->cfold.ensure((size_t)L * NB * 7 * D * sizeof(float)));
        const int nd = (int)distinct.size();
        for (int c0 = 0; c0 < nd; c0 += 8) {
            const int nc = nd - c0 < 8 ? nd - c0 : 8;
            DitTables te;
            LTX_TRY(time_tables(m, p, distinct.data() + c0, nc, s, &te));
            const int* gi = idx.data();      // (read while the launches are enqueued: nothing of a miss waits for the device)
            LTX_TRY(ltx_launch_group_gather(ge->ada.as<float>(), (int64_t)NB * 6 * D, te.ada, (int64_t)nc * 6 * D, gi, c0, nc, L, NB, 6 * D, s));
            LTX_TRY(ltx_launch_group_gather(ge->adaf.as<float>(), (int64_t)NB * D, te.adaf, (int64_t)nc * D, gi, c0, nc, 2, NB, D, s));
            if (p.nfold) {
                LTX_TRY(ltx_launch_group_gather(ge->cfold.as<float>(), (int64_t)NB * 7 * D, te.cfold, (int64_t)nc * 7 * D, gi, c0, nc, L, NB, 3 * D, s));
                LTX_TRY(ltx_launch_group_gather(ge->cfold.as<float>() + (size_t)NB * 3 * D, (int64_t)NB * 7 * D, te.cfold + (size_t)nc * 3 * D, (int64_t)nc * 7 * D, gi, c0, nc, L, NB, 4 * D, s));
            }
        }
        ge->t.assign(timestep, timestep + NB); ge->B = B; ge->G = G; ge->stream = s; ge->valid = true; ge->cfold_valid = p.nfold;
    }
    ge->used = ++m->tclock;
    *t = DitTables{ge->ada.as<float>(), ge->adaf.as<float>(), p.nfold ? ge->cfold.as<float>() : nullptr};
    return LTX_OK;
}
// norm_fold=2 stands down for the rest of the handle's life: the second-output form from here on (speed only), and the copies are
// freed as include/ltxhip.h promises
int give_up_scaled_weights(ltx_dit* m, hipStream_t s) {
    m->wfold_off = true;
    HIP_TRY(hipStreamSynchronize(s));                       // (earlier forwards on this stream may still read the copies)
    m->release_scaled_weights();
    return LTX_OK;
}
// norm_fold=2: the (1 + scale) factor rides on the CONSUMER's weights instead of on a second output of the producer:
// (h (.) (1 + sc)) W^T = h (W (.) (1 + sc))^T.  One scaled copy of the q|k|v and ff1 weights per distinct timestep (1.6 GB at 2B:
// read + written once, then cached like the modulation they are made from - a distilled schedule has 7), all batch rows at one
// timestep (what LtxPipeline::call passes, t2v_pipeline.rs:868); otherwise, or when the schedule has more distinct timesteps
// than copies (norm_fold_copies; the 40-step presets), the second-output form serves.  bf16 rounding moves from h (1 + sc) to W (1 + sc).
// A per-frame call (G > 1: its groups are at different timesteps) never takes this form and never touches the copies or wfold_off.
// *out: the copy this forward reads (null: the form is not taken - the run-time decision `wf` of the block loop).
int scaled_weights(ltx_dit* m, const DitPlan& p, const float* timestep, const float* ada_all, hipStream_t s, const DitWfold** out) {
    *out = nullptr;
    bool wf = p.NB == p.B && p.nfold && ltx_opt().norm_fold == 2 && !m->wfold_off;
    for (int i = 1; i < p.B; ++i) wf = wf && timestep[i] == timestep[0];
    if (!wf) return LTX_OK;
    const int D = p.D, L = m->cfg.num_layers, cap = ltx_opt().norm_fold_copies > 0 ? ltx_opt().norm_fold_copies : 1;
    const size_t esz = ltx_dt_size(p.dt), per_layer = (size_t)7 * D * D * esz;
    const float t0 = timestep[0];
    bool hit;
    DitWfold* we = cache_slot(m->wcache, (size_t)cap, [&](const DitWfold& e) { return e.t == t0 && e.stream == s; }, &hit);
    if (!hit) {
        if (we->valid) {                                    // every copy is in use: the least recently used one is the victim
            // its timestep ran a moment ago: the schedule cycles through more timesteps than copies
            if (m->tclock - we->used < (uint64_t)4 * cap) return give_up_scaled_weights(m, s);
            if (we->stream != s) HIP_TRY(hipStreamSynchronize(we->stream));      // its buffer is re-used (same size); forwards on ITS stream may still read it
            we->valid = false;
        }
        if (we->w.ensure((size_t)L * per_layer) != LTX_OK) {      // no room for another copy
            (void)hipGetLastError();
            return give_up_scaled_weights(m, s);
        }
        for (int l = 0; l < L; ++l) {
            const float* ada = ada_all + (size_t)l * p.NB * 6 * D;
            char* wl = (char*)we->w.p + (size_t)l * per_layer;
            LTX_TRY(ltx_launch_scale_cols(m->blocks[l].qkv1.w, ada + D, wl, 3 * D, D, p.dt, s));
            LTX_TRY(ltx_launch_scale_cols(m->blocks[l].ff1.w, ada + 4 * D, wl + (size_t)3 * D * D * esz, 4 * D, D, p.dt, s));
        }
        we->t = t0; we->stream = s; we->valid = true;
    }
    we->used = m->tclock;
    *out = we;
    return LTX_OK;
}
// Does the plan's to_out call fit in its folded form (A = P, W = vo, K = H * KP, one batch row)?  The plan was made for K = D: where
// it counts on gemm_asm16's epilogue (row partials, the norm fold's second output) the folded call must reach that epilogue too,
// else the context carries no vo for this plan and the forward runs the unfolded path.  The builder with stand-in operands, like the plan's own questions.
bool vo_fits(const ltx_dit* m, const DitPlan& p, const DitCtx* ctx) {
    void* const a = reinterpret_cast<void*>((uintptr_t)4096); float* const f = reinterpret_cast<float*>(a);
    const DitOperands x{a, a, a, a, a, f, f, f, f, f, f, (const char*)a, m->cfg.norm_eps};
    const DitVo vo{a, m->cfg.num_attention_heads * ctx->KP, 0};
    const DitBlock& b = m->blocks[0];
    if (vo.HK % 8 != 0 || vo.HK > p.D) return false;
    if (p.nfold && !ltx_gemm_fold_ok(gemm_o2(p, kFold1, b, x, &vo), EPI_RESID)) return false;
    if (p.presum && !ltx_gemm_asm16_fits(gemm_o2(p, kPass, b, x, &vo), EPI_RESID)) return false;
    return true;
}
// Should this entry carry vo under plan p: the decision step on its KP, and the plan's to_out call in the folded form.  Part of an
// entry's key, so that what a forward computes never depends on which plan built the entry it finds.
bool vo_wanted(const ltx_dit* m, const DitPlan& p, const DitCtx* e) {
    const ltx_dit_config& c = m->cfg;
    return e->KP > 0 && !e->vo_oom && ltx_xattn_fold_route(p.dt, c.attention_head_dim, c.num_attention_heads, p.D, e->KP, e->B, e->compact) && vo_fits(m, p, e);
}
// Text context: caption projection (:186-190), mask bias (:1059-1070) and, for every layer, the cross-attention
// K/V projections + k-RMSNorm (:667-672).  None of it depends on the timestep or the latents, so inside a
// caching scope (ltx_dit_context_cache) it is computed once per (enc, mask) pair instead of once per forward.
int text_context(ltx_dit* m, const DitPlan& p, const void* enc, const float* enc_mask, hipStream_t s, DitCtx** out) {
    const ltx_dit_config& c = m->cfg;
    const int D = p.D, L = c.num_layers, dt = p.dt, B = p.B, K = p.K;
    const int64_t MK = p.MK; const size_t esz = ltx_dt_size(dt);
    DitCtx* ctx = nullptr;
    for (auto& e : m->ctxs) if (e.valid && e.enc == enc && e.mask == enc_mask && e.B == B && e.K == K && e.iodt == p.iodt && e.fold_q2 == p.fold_q2 && e.fold_opt == ltx_opt().xattn_fold_vo && e.fold_vo == vo_wanted(m, p, &e)) ctx = &e;
    *out = ctx;
    if (ctx) return LTX_OK;
    if (m->ctxs.size() >= 4 || !m->ctx_mode) { for (auto& e : m->ctxs) e.valid = false; }
    for (auto& e : m->ctxs) if (!e.valid) { ctx = &e; break; }
    if (!ctx) { m->ctxs.emplace_back(); ctx = &m->ctxs.back(); }
    ctx->enc = enc; ctx->mask = enc_mask; ctx->B = B; ctx->K = K; ctx->iodt = p.iodt; ctx->fold_q2 = p.fold_q2;
    ctx->fold_opt = ltx_opt().xattn_fold_vo; ctx->fold_vo = false; ctx->KP = 0; ctx->vo_oom = false;
    LTX_TRY(ctx->kv.ensure((size_t)L * MK * 2 * D * esz)); LTX_TRY(ctx->bias.ensure(MK * sizeof(float)));
    // Masked text tokens (bias -10000, :1059-1070) get softmax weight exp(s - 10000 - max) = +0.0f: exactly nothing.  Where the
    // short-key-set kernel serves the layer, the keys that are left are moved to the front of their batch row once per context and
    // the kernel sizes its work by their number (device-side count: no host synchronisation in any per-step kernel).
    ctx->compact = enc_mask && dt == LTX_DT_BF16 && ltx_attention_cross64_ok(c.attention_head_dim, K) && ltx_opt().xattn_compact;     // xattn_compact=0: every layer multiplies all K keys (A/B aid)
    if (ctx->compact) {
        LTX_TRY(ctx->kvc.ensure((size_t)L * MK * 2 * D * esz)); LTX_TRY(ctx->biasc.ensure(MK * sizeof(float)));
        LTX_TRY(ctx->kidx.ensure(MK * sizeof(int))); LTX_TRY(ctx->kcount.ensure((size_t)B * sizeof(int)));
    }
    if (enc_mask) LTX_TRY(ltx_launch_mask_bias(ctx->bias.as<float>(), enc_mask, MK, s));
    if (ctx->compact) LTX_TRY(ltx_launch_key_compact(ctx->bias.as<float>(), B, K, ctx->kidx.as<int>(), ctx->kcount.as<int>(), ctx->biasc.as<float>(), s));
    // attn2.to_out folded into the context (xattn_fold.hip) where the decision step can say yes at all (its smallest KP): the counts
    // come back to the host - the one synchronisation of a context build, once per prompt, behind two small kernels and in front of
    // everything else - because KP sizes vo, which is allocated here, before the projections are launched.
    const int H = c.num_attention_heads, hd = c.attention_head_dim;
    if (ctx->compact && B <= 8 && ltx_xattn_fold_route(dt, hd, H, D, 32, B, true)) {
        HIP_TRY(hipMemcpyAsync(ctx->counts_host, ctx->kcount.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        ctx->KP = ltx_xattn_fold_kp(ctx->counts_host, B);
        ctx->fold_vo = vo_wanted(m, p, ctx);      // ... and only where this plan's to_out call runs in the folded form
        if (ctx->fold_vo) {
            (void)ltx_take_oom();
            int rc = ctx->vo.ensure((size_t)L * B * D * H * ctx->KP * esz);
            if (rc == LTX_OK) rc = ctx->votab.ensure((size_t)L * sizeof(XFoldPtrs));
            if (rc != LTX_OK) {      // no memory for vo: this entry runs the unfolded path (and is not rebuilt for it at every forward)
                if (!ltx_take_oom()) return rc;
                ctx->fold_vo = false; ctx->vo_oom = true;
            }
        }
    }
    LTX_TRY(ltx_launch_cast(enc, p.iodt, m->encin.p, dt, MK * c.caption_channels, s));
    LTX_TRY(ltx_linear(m->cap1, m->encin.p, c.caption_channels, m->c1.p, D, (int)MK, dt, EPI_GELU, s));
    LTX_TRY(ltx_linear(m->cap2, m->c1.p, D, m->encp.p, D, (int)MK, dt, EPI_BIAS, s));
    for (int l = 0; l < L; ++l) {
        void* kvl = (char*)ctx->kv.p + (size_t)l * MK * 2 * D * esz;
        LTX_TRY(ltx_linear(m->blocks[l].kv2, m->encp.p, D, kvl, 2 * D, (int)MK, dt, EPI_BIAS, s));
        QkNormRopeArgs k2; k2.x = kvl; k2.rows = MK; k2.D = D; k2.ld = 2 * D; k2.nseg = 1; k2.w0 = m->blocks[l].nk2; k2.eps = 1e-5f;
        if (p.fold_q2) k2.w0b = m->blocks[l].nq2;
        LTX_TRY(ltx_launch_qknorm_rope(k2, dt, s));
    }
    if (ctx->compact) LTX_TRY(ltx_launch_gather_rows(ctx->kv.p, ctx->kvc.p, ctx->kidx.as<int>(), ctx->kcount.as<int>(), L, B, K, (int)(2 * D * esz), s));
    if (ctx->fold_vo) {      // one launch for all layers; the table holds the weights as they are NOW (a LoRA switch invalidates the entry)
        ctx->votab_host.resize(L);
        for (int l = 0; l < L; ++l) ctx->votab_host[l] = XFoldPtrs{m->blocks[l].o2.w, (const char*)ctx->kvc.p + ((size_t)l * MK * 2 * D + D) * esz};
        HIP_TRY(hipMemcpyAsync(ctx->votab.p, ctx->votab_host.data(), (size_t)L * sizeof(XFoldPtrs), hipMemcpyHostToDevice, s));
        XFoldArgs fa; fa.tab = ctx->votab.as<XFoldPtrs>(); fa.vo = ctx->vo.p; fa.L = L; fa.B = B; fa.K = K; fa.ldv = 2 * D; fa.D = D; fa.H = H; fa.KP = ctx->KP;
        LTX_TRY(ltx_launch_xattn_fold(fa, s));
    }
    ctx->valid = true;     // outside a caching scope the entry is invalidated again at the end of this forward
    *out = ctx;
    return LTX_OK;
}
// RoPE tables (:436-524) in cosb / sinb; inside a caching scope the tables of the previous forward are kept when coords / geometry are the same
int rope_tables(ltx_dit* m, const DitPlan& p, int num_frames, int height, int width, const float* rope_scale, const float* video_coords, hipStream_t s) {
    const ltx_dit_config& c = m->cfg;
    auto& rk = m->rope_key;
    const bool same = m->ctx_mode && rk.valid && rk.coords == video_coords && rk.B == p.B && rk.S == p.S && rk.F == num_frames && rk.H == height && rk.W == width &&
                      rk.stream == s && rk.has_rs == (rope_scale != nullptr) && (!rope_scale || !memcmp(rk.rs, rope_scale, sizeof(rk.rs)));
    if (same) return LTX_OK;
    rk.valid = false;
    RopeTableArgs r;
    r.cos = m->cosb.as<float>(); r.sin = m->sinb.as<float>(); r.freqs = m->rope_freqs;
    r.B = p.B; r.D = p.D;
    if (video_coords) {
        r.use_coords = 1; r.coords = video_coords; r.F = 1; r.H = 1; r.W = p.S;
        r.gscale[0] = (float)(1.0 / 20.0); r.gscale[1] = (float)(1.0 / 2048.0); r.gscale[2] = (float)(1.0 / 2048.0);
    } else {
        r.F = num_frames; r.H = height; r.W = width;
        if (rope_scale) {
            r.gscale[0] = (float)((double)rope_scale[0] * c.patch_size_t / 20.0);
            r.gscale[1] = (float)((double)rope_scale[1] * c.patch_size / 2048.0);
            r.gscale[2] = (float)((double)rope_scale[2] * c.patch_size / 2048.0);
        }
    }
    LTX_TRY(ltx_launch_rope_table(r, s));
    rk.coords = video_coords; rk.B = p.B; rk.S = p.S; rk.F = num_frames; rk.H = height; rk.W = width; rk.stream = s;
    rk.has_rs = rope_scale != nullptr; if (rope_scale) memcpy(rk.rs, rope_scale, sizeof(rk.rs));
    rk.valid = m->ctx_mode;
    return LTX_OK;
}

// ---- the block loop ----
struct DitCarry {             // what a block leaves for the next one (and the last one for the final norm)
    bool hsq_valid = false;   // m->hsq holds the partials of the CURRENT contents of h
    bool hs_valid = false;    // m->n holds h (.) (1 + scale) of the norm that comes next (written by the layer that wrote h)
    bool hsq_saved = false;   // m->orig_hsq holds the partials of m->orig (a layer some rows skip)
    bool pending = false; const float* pend_gate = nullptr; const void* pend_bias = nullptr;      // h's rows are still ff2's K-range sums in m->parts
    void take_pending(RowNormArgs& rn, const ltx_dit* m, const DitPlan& p) {      // the row norm that comes next finishes those rows first (RowNormArgs::parts)
        if (!pending) return;
        rn.parts = m->parts.as<float>(); rn.nparts = p.ff2_parts; rn.part_stride = p.M * p.D; rn.d_bias = pend_bias; rn.d_gate = pend_gate; rn.d_gate_stride = 6 * p.D;
        rn.x_out = m->h.p; pending = false;
    }
};
struct DitLayerIn {           // what the forward hands every block
    DitTables tab; const DitWfold* we = nullptr; const DitCtx* ctx = nullptr; const float* skip_layer_mask = nullptr;
    bool fold_vo = false;     // to_out runs on the context's vo (ctx->fold_vo: built only where this plan's to_out call fits in that form)
};
// does block l run: not in the skip list (:1094-1096), not skipped by every row of the mask (all-ones rows make the block an exact identity, :1098-1123).
// In an attention mode (ltxhip_stg.h) the mask perturbs the self-attention and the block runs for every row: only the skip list removes it.
bool block_runs(const ltx_dit* m, const float* skip_layer_mask, int B, int l) {
    for (int sb : m->skip_blocks) if (sb == l) return false;
    if (m->stg_mode != LTX_STG_TRANSFORMER_BLOCK) return true;
    bool all = skip_layer_mask != nullptr;
    for (int b = 0; all && b < B; ++b) all = skip_layer_mask[(size_t)l * B + b] == 1.f;
    return !all;
}
int next_block(const ltx_dit* m, const float* skip_layer_mask, int B, int l) {      // the next block that runs, -1: none
    for (int n = l + 1; n < m->cfg.num_layers; ++n) if (block_runs(m, skip_layer_mask, B, n)) return n;
    return -1;
}

int dit_block(ltx_dit* m, const DitPlan& p, int l, const DitLayerIn& in, DitCarry& st, hipStream_t s) {
    const ltx_dit_config& c = m->cfg;
    const int dt = p.dt, D = p.D, B = p.B, S = p.S, NB = p.NB, H = c.num_attention_heads, hd = c.attention_head_dim;
    const int64_t M = p.M; const size_t esz = ltx_dt_size(dt);
    const bool wf = in.we != nullptr, fold_out = p.nfold && !wf;      // fold_out: the producers write the second output
    const DitBlock& b = m->blocks[l];
    TimeVec mv; mv.n = B; bool any = false;
    for (int i = 0; i < 8; ++i) mv.t[i] = 0.f;
    if (in.skip_layer_mask) for (int bb = 0; bb < B; ++bb) { mv.t[bb] = in.skip_layer_mask[(size_t)l * B + bb]; any |= mv.t[bb] != 0.f; }
    // An attention mode (ltxhip_stg.h; mask values 0 / 1, checked by the forward): the perturbed rows hand to_out their n or v in place
    // of the attention output and the block is otherwise an unmasked one - no copy of the input, no blend, an unmasked block's carry.
    const bool stg_attn = any && m->stg_mode != LTX_STG_TRANSFORMER_BLOCK;
    unsigned char pert[8] = {0};
    if (stg_attn) { for (int bb = 0; bb < B; ++bb) pert[bb] = mv.t[bb] != 0.f; any = false; }
    if (any) {
        HIP_TRY(hipMemcpyAsync(m->orig.p, m->h.p, M * D * esz, hipMemcpyDeviceToDevice, s));
        // the row partials of the kept rows travel with them (restored after the blend): a batch whose rows skip different
        // layers - the guidance branches of a step in one forward - then returns, row for row, the bits of separate forwards
        st.hsq_saved = p.presum && st.hsq_valid;
        if (st.hsq_saved) { LTX_TRY(m->orig_hsq.ensure(M * (D / 128) * sizeof(float))); HIP_TRY(hipMemcpyAsync(m->orig_hsq.p, m->hsq.p, M * (D / 128) * sizeof(float), hipMemcpyDeviceToDevice, s)); }
    }
    const int ln = fold_out ? next_block(m, in.skip_layer_mask, B, l) : -1;
    const float* ada = in.tab.ada + (size_t)l * NB * 6 * D;
    DitOperands x{m->h.p, m->n.p, m->qkv.p, m->attn.p, m->ff.p, m->rsq.as<float>(), m->hsq.as<float>(), m->parts.as<float>(), ada,
                  ln >= 0 ? in.tab.ada + (size_t)ln * NB * 6 * D : nullptr, p.nfold ? in.tab.cfold + (size_t)l * NB * 7 * D : nullptr,
                  wf ? (const char*)in.we->w.p + (size_t)l * 7 * D * D * esz : nullptr, c.norm_eps};
    const DitForm fold_in_form = wf ? kFold2 : kFold1;
    // norm1 + AdaLN (shift_msa = row 0, scale_msa = row 1)
    RowNormArgs rn; rn.x = m->h.p; rn.y = m->n.p; rn.rows = M; rn.D = D; rn.ldx = D; rn.ldy = D;
    rn.kind = 0; rn.eps = c.norm_eps; rn.shift = ada; rn.scale = ada + D; rn.rows_per_batch = p.Sg; rn.mod_stride = 6 * D;
    if (p.presum && st.hsq_valid) { rn.presum = m->hsq.as<float>(); rn.presum_n = D / 128; }
    const bool fold1 = p.nfold && st.hsq_valid && (wf || st.hs_valid);      // the layer that wrote h left its row partials and h (.) (1 + scale_msa) in m->n (or the factor is in the weights): no pass
    // The block's int8 layers (ltxhip_int8.h; the forward's plan then has no norm fold, no row partials and no deferred ff2): the
    // layer's pass-form call with A = the quantised activation in m->a8 / m->a8s and W = the layer's int8 copy
    const unsigned i8 = m->i8_any ? m->i8_mask[(size_t)l] : 0u;
    auto gemm_int8 = [&](int kind, GemmArgs g, int epi) {
        g.A = m->a8.p; g.lda = g.K; g.W = m->i8_w[(size_t)l].w[kind]; g.rowsq = nullptr;
        return ltx_launch_gemm_i8(g, m->a8s.as<float>(), m->i8_w[(size_t)l].sw[kind], epi, -1, s);
    };
    auto norm_int8 = [&]() { RowNormArgs rq = rn; rq.y = m->a8.p; rq.ldy = D; return ltx_launch_rownorm_quant_i8(rq, m->a8s.as<float>(), s); };      // rn's norm, quantised from f32
    const bool qkv8 = (i8 & LTX_I8_QKV) != 0;
    if (qkv8) LTX_TRY(norm_int8());
    else if (!fold1) { st.take_pending(rn, m, p); LTX_TRY(ltx_launch_rownorm(rn, dt, s)); }
    st.hs_valid = false;
    rn.parts = nullptr; rn.nparts = 0; rn.x_out = nullptr; rn.d_bias = nullptr; rn.d_gate = nullptr;
    // self attention
    if (qkv8) LTX_TRY(gemm_int8(0, gemm_qkv1(p, kPass, b, x), EPI_BIAS));
    else LTX_TRY(ltx_launch_gemm(gemm_qkv1(p, fold1 ? fold_in_form : kPass, b, x), dt, EPI_BIAS, s));
    const float attn_scale = 1.0f / std::sqrt((float)hd);
    QkNormRopeArgs qa; qa.x = m->qkv.p; qa.rows = M; qa.D = D; qa.ld = p.ldqkv; qa.seg_stride = p.seg; qa.nseg = 2; qa.w0 = b.nq1; qa.w1 = b.nk1;
    qa.eps = 1e-5f; qa.cos = m->cosb.as<float>(); qa.sin = m->sinb.as<float>();
    if (p.fold_q) qa.out_scale0 = attn_scale * 1.4426950408889634f;
    LTX_TRY(ltx_launch_qknorm_rope(qa, dt, s));
    AttnArgs at; at.q = m->qkv.p; at.k = (char*)m->qkv.p + (size_t)p.seg * esz; at.v = (char*)m->qkv.p + (size_t)2 * p.seg * esz; at.o = m->attn.p;
    at.ldq = at.ldk = at.ldv = p.ldqkv; at.ldo = D; at.B = B; at.Sq = S; at.Sk = S; at.heads = H; at.hd = hd; at.scale = attn_scale;
    at.q_prescaled = p.fold_q ? 1 : 0;
    if (!stg_attn) LTX_TRY(ltx_launch_attention(at, dt, s));
    else {
        auto for_runs = [&](bool perturbed, auto&& fn) -> int {      // fn(b0, b1) for every maximal run [b0, b1) of batch rows that are / are not perturbed
            for (int b0 = 0; b0 < B; ++b0) {
                int b1 = b0;
                while (b1 < B && (pert[b1] != 0) == perturbed) ++b1;
                if (b1 > b0) { LTX_TRY(fn(b0, b1)); b0 = b1; }
            }
            return LTX_OK;
        };
        // attention for the runs of unperturbed batch rows only (one launch per run, none if every row is perturbed): batch rows never
        // interact, so those rows get the bits of the whole-batch launch
        LTX_TRY(for_runs(false, [&](int b0, int b1) {
            AttnArgs ar = at; ar.B = b1 - b0;
            const size_t in_off = (size_t)b0 * S * p.ldqkv * esz;
            ar.q = (const char*)at.q + in_off; ar.k = (const char*)at.k + in_off; ar.v = (const char*)at.v + in_off; ar.o = (char*)at.o + (size_t)b0 * S * D * esz;
            return ltx_launch_attention(ar, dt, s);
        }));
        if (m->stg_mode == LTX_STG_ATTENTION_VALUES) LTX_TRY(ltx_launch_stg_fill(m->attn.p, D, at.v, p.ldqkv, pert, B, S, D, dt, s));      // to_out(v): v with its bias, before the head split
        else if (!fold1 && !qkv8) LTX_TRY(ltx_launch_stg_fill(m->attn.p, D, m->n.p, D, pert, B, S, D, dt, s));      // to_out(n): the norm pass above left n whole in m->n
        else
            // norm fold, or an int8 q | k | v: n is never materialised in bf16 (m->n holds h (.) (1 + scale_msa), the factor rides on the weights, or n went straight to int8), but h is still
            // the block's input here: the row norm over the perturbed batch rows alone, straight into their rows of m->attn
            LTX_TRY(for_runs(true, [&](int b0, int b1) {
                RowNormArgs rp = rn; rp.presum = nullptr; rp.presum_n = 0;
                const size_t row_off = (size_t)b0 * S * D * esz, tab_off = (size_t)b0 * (NB / B) * 6 * D;      // whole batch rows, and their table rows (G per batch row)
                rp.x = (const char*)m->h.p + row_off; rp.y = (char*)m->attn.p + row_off; rp.rows = (int64_t)(b1 - b0) * S;
                rp.shift = ada + tab_off; rp.scale = ada + D + tab_off;
                return ltx_launch_rownorm(rp, dt, s);
            }));
    }
    // h = h + gate_msa * to_out(attn)     (gate_msa = row 2)
    if (i8 & LTX_I8_TO_OUT) {
        GemmArgs g = gemm_base(p, b.o1, m->attn.p, D, m->h.p, D);
        g.resid = m->h.p; g.ldr = D; g.gate = ada + 2 * D; g.gate_stride = 6 * D; g.rows_per_batch = p.Sg;
        LTX_TRY(ltx_launch_quant_rows_i8(m->attn.p, M, D, D, m->a8.p, m->a8s.as<float>(), s));
        LTX_TRY(gemm_int8(1, g, EPI_GATE_RESID));
    } else LTX_TRY(ltx_linear(b.o1, m->attn.p, D, m->h.p, D, (int)M, dt, EPI_GATE_RESID, s, m->h.p, D, ada + 2 * D, 6 * D, p.Sg));
    st.hsq_valid = false;
    // cross attention (no pre-norm, no RoPE, q/k RMSNorm, additive key bias)
    const DitCtx* ctx = in.ctx;
    const char* kvl = (const char*)(ctx->compact ? ctx->kvc.p : ctx->kv.p) + (size_t)l * p.MK * 2 * D * esz;
    AttnArgs ax; ax.q = m->qkv.p; ax.k = kvl; ax.v = kvl + (size_t)D * esz; ax.o = m->attn.p;
    ax.ldq = D; ax.ldk = ax.ldv = 2 * D; ax.ldo = D; ax.B = B; ax.Sq = S; ax.Sk = p.K; ax.heads = H; ax.hd = hd; ax.scale = attn_scale;
    ax.bias = ctx->mask ? ctx->bias.as<float>() : nullptr;
    if (ctx->compact) { ax.bias = ctx->biasc.as<float>(); ax.k_count = ctx->kcount.as<int>(); }
    const int HK = H * ctx->KP;
    if (in.fold_vo) { ax.p_out = m->attn.p; ax.ldp = HK; ax.o = nullptr; }      // the kernel stops at the softmax: P [M, H * KP] in m->attn (H * KP <= D)
    if (p.fold_q2) {
        LTX_TRY(ltx_launch_gemm(gemm_q2(p, b, x), dt, EPI_BIAS, s));
        ax.q_rowsq = m->rsq.as<float>(); ax.q_rowsq_n = D / 128; ax.q_rowsq_D = D; ax.q_rowsq_eps = 1e-5f;
    } else {
        LTX_TRY(linear_of(b.q2, gemm_q2(p, b, x), dt, EPI_BIAS, s));
        QkNormRopeArgs q2; q2.x = m->qkv.p; q2.rows = M; q2.D = D; q2.ld = D; q2.nseg = 1; q2.w0 = b.nq2; q2.eps = 1e-5f;
        LTX_TRY(ltx_launch_qknorm_rope(q2, dt, s));
    }
    LTX_TRY(ltx_launch_attention(ax, dt, s));
    if (in.fold_vo) {      // h += P vo^T + b, one launch per batch row (its vo is its own)
        for (int bb = 0; bb < B; ++bb) {
            const DitVo vo{(const char*)ctx->vo.p + (size_t)l * B * D * HK * esz, HK, bb};
            LTX_TRY(ltx_launch_gemm(gemm_o2(p, fold_out ? kFold1 : kPass, b, x, &vo), dt, EPI_RESID, s));
        }
        st.hs_valid = fold_out;
    } else if (fold_out) { LTX_TRY(ltx_launch_gemm(gemm_o2(p, kFold1, b, x), dt, EPI_RESID, s)); st.hs_valid = true; }
    else LTX_TRY(linear_of(b.o2, gemm_o2(p, kPass, b, x), dt, EPI_RESID, s));
    st.hsq_valid = p.presum;
    // MLP (shift_mlp = row 3, scale_mlp = row 4, gate_mlp = row 5)
    if (p.nfold && st.hsq_valid && (wf || st.hs_valid)) LTX_TRY(ltx_launch_gemm(gemm_ff1(p, fold_in_form, b, x), dt, EPI_GELU, s));
    else {
        rn.shift = ada + 3 * D; rn.scale = ada + 4 * D;
        rn.presum = nullptr; rn.presum_n = 0;
        if (p.presum && st.hsq_valid) { rn.presum = m->hsq.as<float>(); rn.presum_n = D / 128; }
        if (i8 & LTX_I8_FF1) { LTX_TRY(norm_int8()); LTX_TRY(gemm_int8(2, gemm_ff1(p, kPass, b, x), EPI_GELU)); }
        else {
            LTX_TRY(ltx_launch_rownorm(rn, dt, s));
            LTX_TRY(linear_of(b.ff1, gemm_ff1(p, kPass, b, x), dt, EPI_GELU, s));
        }
    }
    st.hs_valid = false;
    if (p.defer_ff2) {
        LTX_TRY(ltx_launch_gemm(gemm_ff2(p, kDefer, b, x), dt, EPI_BIAS, s));
        st.pending = true; st.pend_gate = ada + 5 * D; st.pend_bias = b.ff2.b;
    } else if (ln >= 0) { LTX_TRY(ltx_launch_gemm(gemm_ff2(p, kFold1, b, x), dt, EPI_GATE_RESID, s)); st.hs_valid = true; }
    else if (i8 & LTX_I8_FF2) {
        LTX_TRY(ltx_launch_quant_rows_i8(m->ff.p, M, 4 * D, 4 * D, m->a8.p, m->a8s.as<float>(), s));
        LTX_TRY(gemm_int8(3, gemm_ff2(p, kPass, b, x), EPI_GATE_RESID));
    } else LTX_TRY(linear_of(b.ff2, gemm_ff2(p, kPass, b, x), dt, EPI_GATE_RESID, s));
    st.hsq_valid = p.presum;
    if (!any) return LTX_OK;
    LTX_TRY(ltx_launch_skip_blend(m->h.p, m->orig.p, mv, S, D, dt, s));
    bool binary = true;
    for (int bb = 0; bb < B; ++bb) binary &= mv.t[bb] == 0.f || mv.t[bb] == 1.f;
    if (st.hsq_valid && st.hsq_saved && binary) {          // rows with mask 1 are the block's input again: so are their partials
        const size_t rowb = (size_t)S * (D / 128) * sizeof(float);
        for (int bb = 0; bb < B; ++bb)
            if (mv.t[bb] == 1.f) HIP_TRY(hipMemcpyAsync((char*)m->hsq.p + bb * rowb, (const char*)m->orig_hsq.p + bb * rowb, rowb, hipMemcpyDeviceToDevice, s));
    } else st.hsq_valid = false;
    // m->n was formed from the un-blended rows, for the block after this one; the restored rows need theirs: the producer's
    // expression on the rows as they stand now (for the rows that kept the block: the bits the epilogue wrote)
    st.hs_valid = false;
    if (fold_out && st.hsq_valid && ln >= 0) { LTX_TRY(ltx_launch_mod_scale(m->h.p, x.ada_next + D, 6 * D, m->n.p, NB, p.Sg, D, dt, s)); st.hs_valid = true; }
    return LTX_OK;
}

// one forward of up to 8 batch rows (the per-batch scalars - timesteps, skip-mask rows - travel as kernel arguments).
// G: modulation groups per batch row - 1: one timestep per row (timestep [B]); num_frames: one per latent frame (timestep [B, G],
// tokens in pack order, so a group is a run of S / G rows).  Only the AdaLN look-ups see the groups: they index their tables with
// m / rows_per_batch, which becomes m / (S / G) over tables of B * G rows; attention, RoPE, the text context and the skip-layer
// blend keep S.
int dit_forward_b8(ltx_dit* m, const void* hidden, const void* enc, const float* timestep, int G,
                   const float* enc_mask, int B, int S, int K, int num_frames, int height, int width,
                   const float* rope_scale, const float* video_coords, const float* skip_layer_mask,
                   ltx_dtype io_dtype, void* out, ltx_stream stream, const StepCacheUse* sc = nullptr) {
    if (B < 1 || B > 8) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_forward: internal batch chunk must be 1..8");
    if (S < 1 || K < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_forward: empty sequence");
    if (!video_coords && (int64_t)num_frames * height * width != S)
        LTX_FAIL(LTX_ERR_ARG, "ltx_dit_forward: num_frames*height*width must equal S when video_coords is absent");
    HIP_TRY(hipSetDevice(m->device));
    if (G < 1 || S % G != 0) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_forward: the modulation groups must divide the sequence");
    hipStream_t s = (hipStream_t)stream;
    const ltx_dit_config& c = m->cfg;
    DitPlan plan = ltx_dit_plan(c, m->dtype, io_dtype == LTX_BF16 ? LTX_DT_BF16 : LTX_DT_F32, B, S, K, G, skip_layer_mask != nullptr);
    // a handle with int8 layers (ltxhip_int8.h) runs its copy of the plan without the fusions whose launches pair bf16 producers with
    // bf16 consumers: no norm fold, no row partials for the norms, no deferred ff2 (fold_q2, fold_vo, dense_qkv and fold_q stay)
    if (m->i8_any) { plan.nfold = false; plan.presum = false; plan.defer_ff2 = false; plan.ff2_parts = 0; }
    const DitPlan p = plan;
    const int dt = p.dt, D = p.D, L = c.num_layers;
    const int64_t M = p.M, MK = p.MK; const size_t esz = ltx_dt_size(dt);
    // the workspaces, sized for the plan; nothing is launched before every one of them exists
    const size_t nte = p.NB == p.B ? (size_t)p.B : 8;      // rows of one time-embedding launch: the batch rows, or eight distinct values of a per-frame call
    const size_t MD = M * D * esz, KD = MK * D * esz, part = M * (D / 128) * sizeof(float), rope = M * (D / 2) * sizeof(float);
    const std::pair<DevBuf*, size_t> ws[] = {
        {&m->xin, M * c.in_channels * esz}, {&m->encin, MK * c.caption_channels * esz}, {&m->h, MD}, {&m->n, MD}, {&m->qkv, 3 * MD}, {&m->attn, MD}, {&m->ff, 4 * MD},
        {&m->c1, KD}, {&m->encp, KD}, {&m->kv2, 2 * KD}, {&m->tproj, nte * 256 * esz}, {&m->e1, nte * D * esz}, {&m->emb, nte * D * esz}, {&m->embs, nte * D * esz},
        {&m->temb, nte * 6 * D * esz}, {&m->cosb, rope}, {&m->sinb, rope}, {&m->bias, MK * sizeof(float)}, {&m->outT, M * c.out_channels * esz},
        {&m->rsq, p.fold_q2 ? part : 0}, {&m->hsq, p.presum ? part : 0}, {&m->parts, p.defer_ff2 ? (size_t)p.ff2_parts * M * D * sizeof(float) : 0}, {&m->orig, skip_layer_mask ? MD : 0},
        {&m->a8, m->i8_any ? (size_t)M * 4 * D : 0}, {&m->a8s, m->i8_any ? (size_t)M * sizeof(float) : 0}};
    for (const auto& w : ws) LTX_TRY(w.first->ensure(w.second));
    const bool reuse = sc && sc->reuse;
    if (reuse) {
        for (int b = 0; b < B; ++b)
            if (const char* why = sc->c->row_unusable(sc->row0 + b, S))
                LTX_FAIL(LTX_ERR_ARG, "ltx_dit_forward_cached: reuse asked of cache row " + std::to_string(sc->row0 + b) + ", which " + why);
    } else if (sc) {      // the residuals are laid out for one sequence length: another one starts the cache's rows afresh
        ltx_step_cache* k = sc->c;
        if (k->resid_S != S) { for (auto& r : k->rows) r.valid = false; k->resid_S = S; }
        LTX_TRY(k->resid.ensure(k->rows.size() * (size_t)S * D * esz));
        for (int b = 0; b < B; ++b) k->rows[(size_t)sc->row0 + b].valid = false;
    }

    // inputs -> model dtype (:1045-1047)
    LTX_TRY(ltx_launch_cast(hidden, p.iodt, m->xin.p, dt, p.M * c.in_channels, s));
    // a re-used step: h = proj_in(x) + (h_after_blocks - h_after_proj_in) of the rows' last computed forward, in the projection's epilogue
    if (reuse) LTX_TRY(ltx_linear(m->proj_in, m->xin.p, c.in_channels, m->h.p, D, (int)p.M, dt, EPI_RESID, s, sc->c->resid_row(sc->row0), D));
    else LTX_TRY(ltx_linear(m->proj_in, m->xin.p, c.in_channels, m->h.p, D, (int)p.M, dt, EPI_BIAS, s));
    if (sc && !reuse) HIP_TRY(hipMemcpyAsync(sc->c->resid_row(sc->row0), m->h.p, MD, hipMemcpyDeviceToDevice, s));

    DitLayerIn in; in.skip_layer_mask = skip_layer_mask;
    // a re-used step reads the final norm's table alone: the norm fold's per-timestep vectors (two weight streams per layer) are the
    // blocks' and are not built for it
    DitPlan pt = p; if (reuse) pt.nfold = false;
    LTX_TRY(G == 1 ? time_tables(m, pt, timestep, B, s, &in.tab) : group_tables(m, pt, timestep, s, &in.tab));
    DitCtx* ctx = nullptr;
    DitCarry st;
    if (!reuse) {
        LTX_TRY(scaled_weights(m, p, timestep, in.tab.ada, s, &in.we));
        LTX_TRY(text_context(m, p, enc, enc_mask, s, &ctx)); in.ctx = ctx;
        in.fold_vo = ctx->fold_vo;
        LTX_TRY(rope_tables(m, p, num_frames, height, width, rope_scale, video_coords, s));
        if (m->i8_any && m->i8_stale) LTX_TRY(int8_quantise(m, s));      // the weights changed since the copies were made (adapters)

        for (int l = 0; l < L; ++l)
            if (block_runs(m, skip_layer_mask, B, l)) LTX_TRY(dit_block(m, p, l, in, st, s));
    }
    // the block residual of a computed step: once h is complete - with a deferred ff2 that is behind the final norm, which finishes the rows
    const bool resid_late = sc && !reuse && st.pending;
    if (sc && !reuse && !resid_late) LTX_TRY(ltx_launch_step_residual(m->h.p, sc->c->resid_row(sc->row0), p.M, D, dt, s));

    // final LayerNorm (no affine) + modulation (:1126-1161), proj_out (:1163)
    RowNormArgs rn; rn.x = m->h.p; rn.y = m->n.p; rn.rows = p.M; rn.D = D; rn.ldx = D; rn.ldy = D;
    rn.kind = 1; rn.eps = 1e-6f; rn.shift = in.tab.adaf; rn.scale = in.tab.adaf + (size_t)p.NB * D;
    rn.rows_per_batch = p.Sg; rn.mod_stride = D;
    st.take_pending(rn, m, p);
    LTX_TRY(ltx_launch_rownorm(rn, dt, s));
    if (resid_late) LTX_TRY(ltx_launch_step_residual(m->h.p, sc->c->resid_row(sc->row0), p.M, D, dt, s));
    if (sc && !reuse)
        for (int b = 0; b < B; ++b) sc->c->rows[(size_t)sc->row0 + b] = {true, S, m->weights_epoch};
    void* dst = p.iodt == dt ? out : m->outT.p;
    LTX_TRY(ltx_linear(m->proj_out, m->n.p, D, dst, c.out_channels, (int)p.M, dt, EPI_BIAS, s));
    if (p.iodt != dt) LTX_TRY(ltx_launch_cast(m->outT.p, dt, out, p.iodt, p.M * c.out_channels, s));
    if (ctx && !m->ctx_mode) ctx->valid = false;
    return LTX_OK;
}

// The trait puts no bound on the batch (t2v_pipeline.rs:68-80).  Batch rows never interact in the forward
// (ltx_transformer.rs:1029-1172: every op is per row or per (row, token)), so a larger batch runs as chunks of 8 rows with the
// same results as one call would give.  F: 0 - timestep [B], one per row; else timestep [B, F], one per latent frame: rows whose
// frames all share one value need no groups, and a chunk made of such rows IS the plain forward (the same launches, the same bits,
// norm_fold=2's weight copies included).
int dit_forward_chunks(ltx_dit* m, const void* hidden, const void* enc, const float* timestep, int F,
                       const float* enc_mask, int B, int S, int K, int num_frames, int height, int width,
                       const float* rope_scale, const float* video_coords, const float* skip_layer_mask,
                       ltx_dtype io_dtype, void* out, ltx_stream stream, const StepCacheUse* sc = nullptr) {
    const size_t esz = io_dtype == LTX_BF16 ? 2 : 4;
    const int L = m->cfg.num_layers;
    if (skip_layer_mask && m->stg_mode != LTX_STG_TRANSFORMER_BLOCK)      // the attention modes replace an operand of to_out: there is nothing to blend
        for (size_t i = 0; i < (size_t)L * B; ++i)
            if (skip_layer_mask[i] != 0.f && skip_layer_mask[i] != 1.f)
                LTX_FAIL(LTX_ERR_ARG, "ltx_dit_forward: skip_layer_mask[" + std::to_string(i / B) + ", " + std::to_string(i % B) + "] = " + std::to_string(skip_layer_mask[i]) +
                                      ": the attention STG modes take 0 and 1 only (fractional masks: LTX_STG_TRANSFORMER_BLOCK)");
    std::vector<float> mask_chunk;
    float t_row[8];
    for (int b0 = 0; b0 < B; b0 += 8) {
        const int bc = B - b0 < 8 ? B - b0 : 8;
        const float* slm = skip_layer_mask;
        if (skip_layer_mask && bc != B) {                   // [L, B] -> [L, bc]
            mask_chunk.resize((size_t)L * bc);
            for (int l = 0; l < L; ++l) for (int b = 0; b < bc; ++b) mask_chunk[(size_t)l * bc + b] = skip_layer_mask[(size_t)l * B + b0 + b];
            slm = mask_chunk.data();
        }
        const float* tc = timestep + (size_t)b0 * (F ? F : 1);
        int G = 1;
        if (F) {
            bool uniform = true;
            for (int b = 0; b < bc; ++b) for (int f = 1; f < F; ++f) uniform = uniform && memcmp(&tc[(size_t)b * F + f], &tc[(size_t)b * F], sizeof(float)) == 0;
            if (uniform) { for (int b = 0; b < bc; ++b) t_row[b] = tc[(size_t)b * F]; tc = t_row; } else G = F;
        }
        StepCacheUse use; if (sc) { use = *sc; use.row0 += b0; }
        LTX_TRY(dit_forward_b8(m, (const char*)hidden + (size_t)b0 * S * m->cfg.in_channels * esz, enc ? (const char*)enc + (size_t)b0 * K * m->cfg.caption_channels * esz : nullptr,
                               tc, G, enc_mask ? enc_mask + (size_t)b0 * K : nullptr, bc, S, K, num_frames, height, width, rope_scale,
                               video_coords ? video_coords + (size_t)b0 * S * 3 : nullptr, slm, io_dtype,
                               (char*)out + (size_t)b0 * S * m->cfg.out_channels * esz, stream, sc ? &use : nullptr));
    }
    return LTX_OK;
}

}  // namespace

extern "C" int ltx_dit_forward(ltx_dit* m, const void* hidden, const void* enc, const float* timestep,
                               const float* enc_mask, int B, int S, int K, int num_frames, int height, int width,
                               const float* rope_scale, const float* video_coords, const float* skip_layer_mask,
                               ltx_dtype io_dtype, void* out, ltx_stream stream) {
    if (!m || !hidden || !enc || !timestep || !out) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_forward: null argument");
    if (B < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_forward: batch must be at least 1");
    return dit_forward_chunks(m, hidden, enc, timestep, 0, enc_mask, B, S, K, num_frames, height, width, rope_scale, video_coords, skip_layer_mask, io_dtype, out, stream);
}

// Per-frame timesteps (include/ltxhip_cond.h)
extern "C" int ltx_dit_forward_frames(ltx_dit* m, const void* hidden, const void* enc, const float* timestep,
                                      const float* enc_mask, int B, int S, int K, int num_frames, int height, int width,
                                      const float* rope_scale, const float* video_coords, const float* skip_layer_mask,
                                      ltx_dtype io_dtype, void* out, ltx_stream stream) {
    if (!m || !hidden || !enc || !timestep || !out) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_forward_frames: null argument");
    if (B < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_forward_frames: batch must be at least 1");
    if (num_frames < 1 || height < 1 || width < 1 || (int64_t)num_frames * height * width != S)
        LTX_FAIL(LTX_ERR_ARG, "ltx_dit_forward_frames: S must equal num_frames*height*width (tokens in pack order, with or without video_coords)");
    return dit_forward_chunks(m, hidden, enc, timestep, num_frames, enc_mask, B, S, K, num_frames, height, width, rope_scale, video_coords, skip_layer_mask, io_dtype, out, stream);
}

extern "C" int ltx_dit_context_cache(ltx_dit* m, int enable) {
    if (!m) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_context_cache: null handle");
    for (auto& e : m->ctxs) e.valid = false;
    m->rope_key.valid = false;
    m->ctx_mode = enable != 0;
    return LTX_OK;
}

// ---- step cache (include/ltxhip_stepcache.h) ----
extern "C" void ltx_step_cache_params_default(ltx_step_cache_params* p) {
    if (!p) return;
    const StepCachePolicy d;
    p->rel_l1_thresh = d.thresh; for (int k = 0; k < 5; ++k) p->coeff[k] = d.coeff[k];
    p->pattern = nullptr; p->n_pattern = 0;
}

extern "C" int ltx_step_cache_create(ltx_dit* dit, int rows, ltx_step_cache** out) {
    if (!dit || !out) LTX_FAIL(LTX_ERR_ARG, "ltx_step_cache_create: null argument");
    *out = nullptr;
    if (rows < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_step_cache_create: rows must be at least 1, got " + std::to_string(rows));
    if (!ltx_step_measure_blocks(1, dit->D, dit->dtype))
        LTX_FAIL(LTX_ERR_UNSUPPORTED, "ltx_step_cache_create: inner dim " + std::to_string(dit->D) + " is not a multiple of 128 the measure kernel serves");
    HIP_TRY(hipSetDevice(dit->device));
    ltx_step_cache* c = new ltx_step_cache();
    c->dit = dit; c->rows.resize((size_t)rows);
    int rc = c->sums.ensure(2 * sizeof(double));
    if (rc == LTX_OK && hipHostMalloc((void**)&c->host, 2 * sizeof(double), hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError(); ltx_set_error("ltx_step_cache_create: hipHostMalloc of the result pair"); rc = LTX_ERR_HIP;
    }
    if (rc != LTX_OK) { c->sums.release(); delete c; return rc; }
    *out = c;
    return LTX_OK;
}

extern "C" void ltx_step_cache_destroy(ltx_step_cache* c) {
    if (!c) return;
    (void)hipSetDevice(c->dit->device);
    if (c->used) (void)hipStreamSynchronize(c->stream);      // (launches enqueued on it may still read the buffers)
    c->prev.release(); c->resid.release(); c->parts.release(); c->sums.release();
    if (c->host) (void)hipHostFree(c->host);
    delete c;
}

extern "C" int ltx_step_cache_reset(ltx_step_cache* c) {
    if (!c) LTX_FAIL(LTX_ERR_ARG, "ltx_step_cache_reset: null handle");
    c->forget();
    return LTX_OK;
}

static int step_cache_policy_of(const ltx_step_cache_params* params, const char* who, StepCachePolicy* pol) {
    if (!params) LTX_FAIL(LTX_ERR_ARG, std::string(who) + ": null step cache parameters");
    pol->thresh = params->rel_l1_thresh; for (int k = 0; k < 5; ++k) pol->coeff[k] = params->coeff[k];
    pol->pattern = params->pattern; pol->n_pattern = params->n_pattern;
    if (const char* why = step_cache_policy_error(*pol)) LTX_FAIL(LTX_ERR_ARG, std::string(who) + ": " + why);
    return LTX_OK;
}
// (host/pipeline.hip checks a call's parameters before it touches the device; declared in model_util.h)
int ltx_step_cache_params_check(const ltx_step_cache_params* params, const char* who) { StepCachePolicy pol; return step_cache_policy_of(params, who, &pol); }

extern "C" int ltx_step_cache_decide(ltx_step_cache* c, ltx_dit* m, const void* hidden, const float* timestep, int frames,
                                     int B, int S, int num_frames, int height, int width, ltx_dtype io_dtype,
                                     int step, int n_steps, const ltx_step_cache_params* params, int* reuse, float* distance, ltx_stream stream) {
    if (!c || !m || !hidden || !timestep || !reuse) LTX_FAIL(LTX_ERR_ARG, "ltx_step_cache_decide: null argument");
    if (c->dit != m) LTX_FAIL(LTX_ERR_ARG, "ltx_step_cache_decide: the cache was created for another model handle");
    if (B < 1 || S < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_step_cache_decide: batch and sequence must be at least 1");
    if (n_steps < 1 || step < 0 || step >= n_steps) LTX_FAIL(LTX_ERR_ARG, "ltx_step_cache_decide: step " + std::to_string(step) + " outside 0.." + std::to_string(n_steps - 1));
    if (io_dtype != LTX_F32 && io_dtype != LTX_BF16) LTX_FAIL(LTX_ERR_ARG, "ltx_step_cache_decide: bad dtype");
    if (frames && (num_frames < 1 || height < 1 || width < 1 || (int64_t)num_frames * height * width != S))
        LTX_FAIL(LTX_ERR_ARG, "ltx_step_cache_decide: with per-frame timesteps S must equal num_frames*height*width");
    StepCachePolicy pol;
    LTX_TRY(step_cache_policy_of(params, "ltx_step_cache_decide", &pol));
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    const ltx_dit_config& cfg = m->cfg;
    const int dt = m->dtype, D = m->D, F = frames ? num_frames : 0;
    const size_t esz = ltx_dt_size(dt), iosz = io_dtype == LTX_BF16 ? 2 : 4;
    const int64_t M = (int64_t)B * S;
    LTX_TRY(c->prev.ensure((size_t)M * D * esz));
    c->stream = s; c->used = true;
    if (c->prev_rows != M) { c->st.have_prev = false; c->prev_rows = M; }      // another geometry: nothing to be a distance from
    const bool first = !c->st.have_prev;
    int64_t nblk = 0;
    for (int b0 = 0; b0 < B; b0 += 8) nblk += ltx_step_measure_blocks((int64_t)(B - b0 < 8 ? B - b0 : 8) * S, D, dt);
    LTX_TRY(c->parts.ensure((size_t)nblk * 2 * sizeof(double)));
    float t_row[8];
    int64_t blk0 = 0;
    for (int b0 = 0; b0 < B; b0 += 8) {      // the chunks of dit_forward_chunks, with its collapse of rows whose frames share one timestep
        const int bc = B - b0 < 8 ? B - b0 : 8;
        const float* tc = timestep + (size_t)b0 * (F ? F : 1);
        int G = 1;
        if (F) {
            bool uniform = true;
            for (int b = 0; b < bc; ++b) for (int f = 1; f < F; ++f) uniform = uniform && memcmp(&tc[(size_t)b * F + f], &tc[(size_t)b * F], sizeof(float)) == 0;
            if (uniform) { for (int b = 0; b < bc; ++b) t_row[b] = tc[(size_t)b * F]; tc = t_row; } else G = F;
        }
        DitPlan p = ltx_dit_plan(cfg, dt, io_dtype == LTX_BF16 ? LTX_DT_BF16 : LTX_DT_F32, bc, S, 1, G, false);
        p.nfold = false;                                        // (the tables alone: the norm fold's vectors are the forward's to build)
        const size_t nte = p.NB == p.B ? (size_t)p.B : 8;
        const std::pair<DevBuf*, size_t> ws[] = {
            {&m->xin, p.M * cfg.in_channels * esz}, {&m->h, p.M * D * esz}, {&m->tproj, nte * 256 * esz}, {&m->e1, nte * D * esz}, {&m->emb, nte * D * esz},
            {&m->embs, nte * D * esz}, {&m->temb, nte * 6 * D * esz}};
        for (const auto& w : ws) LTX_TRY(w.first->ensure(w.second));
        LTX_TRY(ltx_launch_cast((const char*)hidden + (size_t)b0 * S * cfg.in_channels * iosz, p.iodt, m->xin.p, dt, p.M * cfg.in_channels, s));
        LTX_TRY(ltx_linear(m->proj_in, m->xin.p, cfg.in_channels, m->h.p, D, (int)p.M, dt, EPI_BIAS, s));
        DitTables tab;
        LTX_TRY(G == 1 ? time_tables(m, p, tc, bc, s, &tab) : group_tables(m, p, tc, s, &tab));
        StepMeasureArgs a;      // block 0's shift_msa / scale_msa: rows 0 and 1 of its table
        a.h = m->h.p; a.prev = (char*)c->prev.p + (size_t)b0 * S * D * esz; a.shift = tab.ada; a.scale = tab.ada + D; a.mod_stride = 6 * D;
        a.rows = p.M; a.D = D; a.rows_per_batch = p.Sg; a.eps = cfg.norm_eps; a.first = first ? 1 : 0; a.part = c->parts.as<double>() + 2 * blk0;
        LTX_TRY(ltx_launch_step_measure(a, dt, s));
        blk0 += ltx_step_measure_blocks(p.M, D, dt);
    }
    LTX_TRY(ltx_launch_step_measure_finish(c->parts.as<double>(), nblk, c->sums.as<double>(), s));
    HIP_TRY(hipMemcpyAsync(c->host, c->sums.p, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));                           // the one wait of a step: the decision is the host's
    const double num = c->host[0], den = c->host[1];
    *reuse = step_cache_decide(&c->st, pol, step, n_steps, num, den, true);
    if (distance) *distance = first ? 0.0f : (float)(num / den);
    return LTX_OK;
}

extern "C" int ltx_step_cache_require(ltx_step_cache* c, const ltx_dit* m, int row0, int nrows, int S, int* reuse) {
    if (!c || !m || !reuse) LTX_FAIL(LTX_ERR_ARG, "ltx_step_cache_require: null argument");
    if (c->dit != m) LTX_FAIL(LTX_ERR_ARG, "ltx_step_cache_require: the cache was created for another model handle");
    if (row0 < 0 || nrows < 1 || (size_t)row0 + (size_t)nrows > c->rows.size())
        LTX_FAIL(LTX_ERR_ARG, "ltx_step_cache_require: rows " + std::to_string(row0) + ".." + std::to_string(row0 + nrows - 1) + " outside the cache's " + std::to_string(c->rows.size()));
    if (!*reuse) return LTX_OK;
    for (int r = row0; r < row0 + nrows; ++r)
        if (c->row_unusable(r, S)) { *reuse = step_cache_demote(&c->st, *reuse, false); break; }
    return LTX_OK;
}

extern "C" int ltx_dit_forward_cached(ltx_dit* m, ltx_step_cache* c, int row0, int reuse, int frames,
                                      const void* hidden, const void* enc, const float* timestep, const float* enc_mask,
                                      int B, int S, int K, int num_frames, int height, int width,
                                      const float* rope_scale, const float* video_coords, const float* skip_layer_mask,
                                      ltx_dtype io_dtype, void* out, ltx_stream stream) {
    if (!m || !c || !hidden || !timestep || !out || (!reuse && !enc)) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_forward_cached: null argument");
    if (c->dit != m) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_forward_cached: the cache was created for another model handle");
    if (B < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_forward_cached: batch must be at least 1");
    if (row0 < 0 || (size_t)row0 + (size_t)B > c->rows.size())
        LTX_FAIL(LTX_ERR_ARG, "ltx_dit_forward_cached: rows " + std::to_string(row0) + ".." + std::to_string(row0 + B - 1) + " outside the cache's " + std::to_string(c->rows.size()));
    if (frames && (num_frames < 1 || height < 1 || width < 1 || (int64_t)num_frames * height * width != S))
        LTX_FAIL(LTX_ERR_ARG, "ltx_dit_forward_cached: with per-frame timesteps S must equal num_frames*height*width (tokens in pack order)");
    const StepCacheUse use{c, row0, reuse != 0};
    c->stream = (hipStream_t)stream; c->used = true;
    return dit_forward_chunks(m, hidden, enc, timestep, frames ? num_frames : 0, enc_mask, B, S, K, num_frames, height, width, rope_scale, video_coords,
                              reuse ? nullptr : skip_layer_mask, io_dtype, out, stream, &use);
}

extern "C" int ltx_step_cache_read_residual(const ltx_step_cache* c, int row, float* dst, ltx_stream stream) {
    if (!c || !dst) LTX_FAIL(LTX_ERR_ARG, "ltx_step_cache_read_residual: null argument");
    if (row < 0 || (size_t)row >= c->rows.size() || !c->rows[(size_t)row].valid)
        LTX_FAIL(LTX_ERR_ARG, "ltx_step_cache_read_residual: row " + std::to_string(row) + " holds no residual");
    HIP_TRY(hipSetDevice(c->dit->device));
    const_cast<ltx_step_cache*>(c)->stream = (hipStream_t)stream;
    return ltx_launch_cast(c->resid_row(row), c->dit->dtype, dst, LTX_DT_F32, (int64_t)c->resid_S * c->dit->D, (hipStream_t)stream);
}

// ---- LoRA adapters (include/ltxhip_lora.h) ----
void ltx_dit_describe(const ltx_dit* m, ltx_dit_config* cfg, int* dtype, int* device) { *cfg = m->cfg; *dtype = m->dtype; *device = m->device; }

extern "C" int ltx_dit_adapter_count(const ltx_dit* m) { return m ? m->n_adapters : 0; }

extern "C" int ltx_dit_set_adapters(ltx_dit* m, const ltx_lora* const* loras, const float* scales, int n, ltx_stream stream) {
    if (!m) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_set_adapters: null handle");
    if (n < 0 || n > kLoraMaxAdapters) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_set_adapters: " + std::to_string(n) + " adapters (0..8)");
    if (n > 0 && (!loras || !scales)) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_set_adapters: null adapter list or scales");
    const int L = m->cfg.num_layers;
    for (int i = 0; i < n; ++i) {
        const ltx_lora* l = loras[i];
        if (!l) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_set_adapters: adapter " + std::to_string(i) + " is null");
        if (l->cfg.num_attention_heads * l->cfg.attention_head_dim != m->D || l->cfg.num_layers != L || l->cfg.cross_attention_dim != m->cfg.cross_attention_dim ||
            l->dtype != m->dtype || l->device != m->device)
            LTX_FAIL(LTX_ERR_ARG, "ltx_dit_set_adapters: adapter " + std::to_string(i) + " was built for another configuration (inner dim " +
                                  std::to_string(l->cfg.num_attention_heads * l->cfg.attention_head_dim) + ", " + std::to_string(l->cfg.num_layers) + " layers), dtype or device");
    }
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t esz = ltx_dt_size(m->dtype);
    // the merge of every target, operands in list order
    std::vector<LoraMergeArgs> plan((size_t)L * kLoraLinears);
    for (int i = 0; i < n; ++i)
        for (const LoraEntry& e : loras[i]->entries) {
            LoraMergeArgs& p = plan[(size_t)e.block * kLoraLinears + e.which];
            p.At[p.n] = e.At; p.Bp[p.n] = e.Bp; p.r_pad[p.n] = e.r_pad; p.coef[p.n] = scales[i] * e.factor; ++p.n;
        }
    auto targeted = [&](int l, int slot) {
        for (int part = 0; part < kSlotParts[slot]; ++part) if (plan[(size_t)l * kLoraLinears + kSlotFirst[slot] + part].n > 0) return true;
        return false;
    };
    // second buffers first: nothing is launched and nothing changes before every one of them exists
    std::vector<void**> fresh;
    for (int l = 0; l < L; ++l)
        for (int slot = 0; slot < 7; ++slot) {
            if (!targeted(l, slot) || m->lora_w[l].merged[slot]) continue;
            const LinearW* lw = dit_slot(m->blocks[l], slot);
            void* p = nullptr;
            const hipError_t e = hipMalloc(&p, (size_t)lw->out * lw->in * esz);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                for (void** q : fresh) { (void)hipFree(*q); *q = nullptr; }
                LTX_FAIL(LTX_ERR_HIP, std::string("ltx_dit_set_adapters: hipMalloc of a merged weight: ") + hipGetErrorString(e) + " (the handle is unchanged)");
            }
            m->lora_w[l].merged[slot] = p; fresh.push_back(&m->lora_w[l].merged[slot]);
        }
    m->invalidate_weight_derived();
    std::vector<void*> unused;
    int rc = LTX_OK;
    for (int l = 0; l < L; ++l)
        for (int slot = 0; slot < 7; ++slot) {
            LinearW* lw = dit_slot(m->blocks[l], slot);
            auto& ls = m->lora_w[l];
            if (!ls.merged[slot]) continue;                    // never targeted: w is the base
            lw->wp.reset(); lw->wp_tried = false;                // (the packed copy, where one was made, is of the weights that go)
            if (!targeted(l, slot)) { lw->w = ls.base[slot]; unused.push_back(ls.merged[slot]); ls.merged[slot] = nullptr; continue; }
            const int parts = kSlotParts[slot], rows = lw->out / parts;
            for (int part = 0; part < parts && rc == LTX_OK; ++part) {
                const size_t off = (size_t)part * rows * lw->in * esz;
                LoraMergeArgs a = plan[(size_t)l * kLoraLinears + kSlotFirst[slot] + part];
                if (a.n > 0) {
                    a.w0 = (const char*)ls.base[slot] + off; a.out = (char*)ls.merged[slot] + off; a.N = rows; a.K = lw->in;
                    rc = ltx_launch_lora_merge(a, m->dtype, s);
                } else if (hipMemcpyAsync((char*)ls.merged[slot] + off, (const char*)ls.base[slot] + off, (size_t)rows * lw->in * esz, hipMemcpyDeviceToDevice, s) != hipSuccess) {
                    ltx_set_error("ltx_dit_set_adapters: hipMemcpyAsync"); rc = LTX_ERR_HIP;
                }
            }
            lw->w = ls.merged[slot];
        }
    m->n_adapters = n;
    if (!unused.empty()) {                                       // forwards enqueued earlier may still read them
        (void)hipDeviceSynchronize();
        for (void* p : unused) (void)hipFree(p);
    }
    return rc;
}

extern "C" int ltx_dit_read_linear(const ltx_dit* m, int block, int which, void* out_dev, ltx_stream stream) {
    if (!m || !out_dev) LTX_FAIL(LTX_ERR_ARG, "ltx_dit_read_linear: null argument");
    if (block < 0 || block >= m->cfg.num_layers || which < 0 || which >= kLoraLinears)
        LTX_FAIL(LTX_ERR_ARG, "ltx_dit_read_linear: block 0.." + std::to_string(m->cfg.num_layers - 1) + ", which 0..9");
    HIP_TRY(hipSetDevice(m->device));
    const LinearW* lw = dit_slot(const_cast<DitBlock&>(m->blocks[block]), kLoraSlot[which]);
    const size_t bytes = (size_t)(lw->out / kSlotParts[kLoraSlot[which]]) * lw->in * ltx_dt_size(m->dtype);
    HIP_TRY(hipMemcpyAsync(out_dev, (const char*)lw->w + (size_t)kLoraPart[which] * bytes, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return LTX_OK;
}
