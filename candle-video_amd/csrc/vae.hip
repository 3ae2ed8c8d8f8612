// AutoencoderKLLtxVideo on MI355X: decode (first part of the file) and encode (second part, "encode side" below).
// Reference: src/models/ltx_video/vae.rs  (:1488-1727 decoder, :755-821 resnet, :1090-1169 upsampler,
// :415-464 conv, :2037-2066 decode_z, :2225-2290 / :2358-2434 tiling, :1927-2006 blends;
// :1316-1469 encoder, :469-582 downsampler, :841-948 down block, :117-145 posterior, :2017-2035 encode_z,
// :2158-2223 / :2294-2357 tiled encodes).
//
// HBM layout: activations are CHANNELS-LAST [B,T,H,W,C] in the model dtype, so that
//   * the conv3d is an implicit GEMM whose K dimension (C_in) is contiguous (16-B coalesced loads,
//     MFMA operands straight from LDS rows), 27 taps accumulated in the same accumulators;
//   * the per-voxel RMS norm over C is a contiguous row reduction;
//   * depth-to-space (+ first-frame drop + tiled residual) and unpatchify are pure index math in
//     the conv epilogues (weights' output channels are re-ordered once at load time so the 4
//     accumulator values a lane owns are contiguous in the destination).
// The packed token layout the denoise loop carries ([B, F*H*W, 128]) IS channels-last, so
// unpack_latents is free on this path.
//
// Tiling: the geometry of both sides' tiled paths is a VaeTilePlan (host/tile_plan.h), built once per call; this file only
// walks it - assemble_spatial (tiles of a plane), place_temporal (windows of frames), batched_leaf_decode (the plan's leaves).
#include <cstring>
#include <deque>
#include "conv3d.h"
#include "options.h"
#include "../host/tile_plan.h"
#include "../../include/ltxhip_frames.h"
#include "../../include/ltxhip_encoder.h"
#include "../../include/ltxhip_ops.h"

extern "C" int ltx_pcg32_randn(uint64_t seed, uint64_t inc, size_t n, float* out_host);   // host/pipeline.hip (utils/deterministic_rng.rs)

struct TimeEmbW { LinearW l1, l2; int dim = 0; };
struct ResnetW { ConvW c1, c2; void* sst = nullptr; void *pcs1 = nullptr, *pcs2 = nullptr; };   // pcs: per_channel_scale{1,2} [C] where the block injects noise (vae.rs:676-689)
struct UpBlockW { ConvW up; TimeEmbW te; std::vector<ResnetW> res; int ch = 0, cin = 0; bool residual = true, temporal = true; };

struct ltx_vae {
    ltx_vae_config cfg{};
    int dtype = LTX_DT_BF16, device = 0;
    ConvW conv_in, conv_out;
    TimeEmbW mid_te, out_te;
    std::vector<ResnetW> mid;
    std::vector<UpBlockW> ups;
    void* sst_out = nullptr;
    float tsm = 1.0f; bool has_tsm = false;
    float *mean = nullptr, *std_ = nullptr, *vtab = nullptr;
    int mid_ch = 0, last_ch = 0;
    std::vector<void*> owned;
    DevBuf zin, X, Y, N, C, tproj, e1, te, mod, tiles[2], tile_lat, stats, predec, rgbtmp;
    std::deque<DevBuf> tilebufs;   // deque: growing it must not move DevBufs that Tile.buf points at
    // CombinedTimestepEmbedder outputs (+ scale_shift_table) per (table, timestep vector, stream): functions of the weights and the
    // timestep alone (a pipeline decodes every video at the same decode_timestep), 5 launches per resnet when recomputed
    struct ModEntry { const void* sst = nullptr; float t[LTX_MAX_BATCH] = {0}; int n = 0; hipStream_t stream = nullptr; uint64_t used = 0; DevBuf buf; };
    std::deque<ModEntry> mods; uint64_t mod_clock = 0;
    // noise injection (vae.rs:741-753): the reference draws an [H, W] plane from the device RNG per injection; here plane k of the
    // handle's life is Pcg32::new(noise_seed, k).randn(H * W) (utils/deterministic_rng.rs), k restarted by ltx_vae_set_noise_seed
    uint64_t noise_seed = 0, noise_ctr = 0; bool any_inject = false;
    DevBuf noise_plane; std::vector<float> noise_host;
    size_t act_bytes_reserved() const { return X.bytes + Y.bytes + N.bytes + C.bytes; }   // activation buffers a decoder call re-uses
    void free_all() {
        for (void* p : owned) if (p) (void)hipFree(p);
        owned.clear();
        DevBuf* bs[] = {&zin, &X, &Y, &N, &C, &tproj, &e1, &te, &mod, &tiles[0], &tiles[1], &tile_lat, &stats, &predec, &noise_plane};
        for (DevBuf* b : bs) b->release();
        for (auto& b : tilebufs) b.release();
        for (auto& e : mods) e.buf.release();
        mods.clear();
    }
};

namespace {

// crop a [t0:t1, h0:h1, w0:w1] window of a channels-last tensor (elements of esz bytes)
__global__ void cl_window_kernel(const unsigned char* src, unsigned char* dst, int esz, int B, int T, int H, int W, int C,
                                 int t0, int t1, int h0, int h1, int w0, int w1) {
    const int nt = t1 - t0, nh = h1 - h0, nw = w1 - w0;
    const int64_t rowb = (int64_t)C * esz;
    const int64_t n = (int64_t)B * nt * nh * nw * rowb;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
        int64_t bb = idx % rowb; int64_t r = idx / rowb;
        int w = (int)(r % nw); r /= nw; int h = (int)(r % nh); r /= nh; int t = (int)(r % nt); int b = (int)(r / nt);
        dst[idx] = src[((((int64_t)b * T + t0 + t) * H + h0 + h) * W + w0 + w) * rowb + bb];
    }
}

// the model's tensors under their bare names: "<prefix>xxx" and "xxx" are both accepted
struct BareNames {
    std::vector<std::string> names; std::vector<ltx_weight> w;
    BareNames(const ltx_weight* weights, size_t n, const std::string& prefix) : w(weights, weights + n) {
        names.reserve(n);
        for (size_t i = 0; i < n; ++i) {
            const std::string nm = w[i].name ? w[i].name : "";
            names.push_back(nm.rfind(prefix, 0) == 0 ? nm.substr(prefix.size()) : nm);
            w[i].name = names[i].c_str();
        }
    }
};

int load_conv(int dt, std::vector<void*>& owned, const WeightMap& wm, const std::string& prefix, int cin, int cout, int mode, int Cf, ConvW* c) {
    const ltx_weight* w = wm.find(prefix + ".conv.weight");
    const ltx_weight* b = wm.find(prefix + ".conv.bias");
    if (!w) LTX_FAIL(LTX_ERR_MISSING_WEIGHT, "missing weight '" + prefix + ".conv.weight'");
    if (!b) LTX_FAIL(LTX_ERR_MISSING_WEIGHT, "missing weight '" + prefix + ".conv.bias'");
    if (ltx_numel(w) != (int64_t)cout * cin * 27) LTX_FAIL(LTX_ERR_ARG, "weight '" + prefix + ".conv.weight': wrong size");
    if (ltx_numel(b) != cout) LTX_FAIL(LTX_ERR_ARG, "weight '" + prefix + ".conv.bias': wrong size");
    return conv_upload(dt, owned, w, b, cin, cout, mode, Cf, c);
}

int load_resnet_convs(int dt, std::vector<void*>& owned, const WeightMap& wm, const std::string& prefix, int ch, ResnetW* r) {
    LTX_TRY(load_conv(dt, owned, wm, prefix + ".conv1", ch, ch, LTX_PERM_NONE, 0, &r->c1));
    return load_conv(dt, owned, wm, prefix + ".conv2", ch, ch, LTX_PERM_NONE, 0, &r->c2);
}

int load_temb(ltx_vae* v, const WeightMap& wm, const std::string& prefix, int dim, TimeEmbW* t) {
    t->dim = dim;
    LTX_TRY(ltx_load_linear(wm, prefix + ".timestep_embedder.linear_1", 256, dim, v->dtype, &t->l1));
    v->owned.push_back(t->l1.w); if (t->l1.b) v->owned.push_back(t->l1.b);
    LTX_TRY(ltx_load_linear(wm, prefix + ".timestep_embedder.linear_2", dim, dim, v->dtype, &t->l2));
    v->owned.push_back(t->l2.w); if (t->l2.b) v->owned.push_back(t->l2.b);
    return LTX_OK;
}

int load_resnet(ltx_vae* v, const WeightMap& wm, const std::string& prefix, int ch, bool inject, ResnetW* r) {
    LTX_TRY(load_resnet_convs(v->dtype, v->owned, wm, prefix, ch, r));
    if (inject) {
        // vae.rs:676-689: vb.pp("per_channel_scaleN").get((C, 1, 1), "weight").ok() - a scale that is absent from the checkpoint
        // under exactly that name is no injection, not an error
        for (int k = 0; k < 2; ++k) {
            const std::string nm = prefix + ".per_channel_scale" + std::to_string(k + 1) + ".weight";
            if (!wm.find(nm)) continue;
            void** dst = k ? &r->pcs2 : &r->pcs1;
            LTX_TRY(ltx_load_tensor(wm, nm, ch, v->dtype, dst)); v->owned.push_back(*dst);
            v->any_inject = true;
        }
    }
    if (v->cfg.timestep_conditioning) {
        LTX_TRY(ltx_load_tensor(wm, prefix + ".scale_shift_table", 4 * (int64_t)ch, v->dtype, &r->sst));
        v->owned.push_back(r->sst);
    }
    return LTX_OK;
}

int build(ltx_vae* v, const ltx_weight* weights, size_t n_weights) {
    const ltx_vae_config& c = v->cfg;
    WeightMap wm0(weights, n_weights);
    const BareNames bare(weights, n_weights, "decoder.");
    WeightMap wm(bare.w.data(), bare.w.size());

    const int nb = c.n_blocks;
    std::vector<int> boc(nb), upf(nb), lpb(nb + 1);
    for (int i = 0; i < nb; ++i) { boc[i] = c.decoder_block_out_channels[nb - 1 - i]; upf[i] = c.decoder_upsample_factor[nb - 1 - i]; }
    for (int i = 0; i <= nb; ++i) lpb[i] = c.decoder_layers_per_block[nb - i];
    v->mid_ch = boc[0];
    LTX_TRY(load_conv(v->dtype, v->owned, wm, "conv_in", c.latent_channels, v->mid_ch, LTX_PERM_NONE, 0, &v->conv_in));
    if (c.timestep_conditioning) LTX_TRY(load_temb(v, wm, "mid_block.time_embedder", 4 * v->mid_ch, &v->mid_te));
    v->mid.resize(lpb[0]);
    for (int i = 0; i < lpb[0]; ++i) LTX_TRY(load_resnet(v, wm, "mid_block.resnets." + std::to_string(i), v->mid_ch, c.decoder_inject_noise[nb] != 0, &v->mid[i]));   // inject list reversed: entry nb is the mid block (vae.rs:1514-1515, 1541)
    v->ups.resize(nb);
    int cur = v->mid_ch;
    for (int bi = 0; bi < nb; ++bi) {
        UpBlockW& u = v->ups[bi];
        const std::string p = "up_blocks." + std::to_string(bi);
        u.residual = c.decoder_upsample_residual[nb - 1 - bi] != 0;   // reversed like the other lists (vae.rs:1516-1517)
        u.ch = boc[bi] / upf[bi];                       // vae.rs:1548
        u.cin = u.ch * upf[bi];                         // upsampler in-channels (vae.rs:1215)
        if (u.cin != cur) LTX_FAIL(LTX_ERR_UNSUPPORTED, "decoder up-block channel chain mismatch");
        u.temporal = c.decoder_spatiotemporal_scaling[nb - 1 - bi] != 0;   // reversed too (vae.rs:1509-1510); false: the (1, 2, 2) upsampler (:1225-1236)
        const int nsub = u.temporal ? 8 : 4;
        if ((u.ch * nsub) % u.cin != 0 || u.cin % nsub != 0) LTX_FAIL(LTX_ERR_UNSUPPORTED, "upsampler residual repeat must be integral");
        LTX_TRY(load_conv(v->dtype, v->owned, wm, p + ".upsamplers.0.conv", u.cin, u.ch * nsub, LTX_PERM_D2S, u.ch, &u.up));
        if (c.timestep_conditioning) LTX_TRY(load_temb(v, wm, p + ".time_embedder", 4 * u.ch, &u.te));
        u.res.resize(lpb[bi + 1]);
        for (int i = 0; i < lpb[bi + 1]; ++i) LTX_TRY(load_resnet(v, wm, p + ".resnets." + std::to_string(i), u.ch, c.decoder_inject_noise[nb - 1 - bi] != 0, &u.res[i]));   // inj[bi + 1] of the reversed list (vae.rs:1561)
        cur = u.ch;
    }
    v->last_ch = cur;
    const int nout = c.out_channels * c.patch_size * c.patch_size;
    LTX_TRY(load_conv(v->dtype, v->owned, wm, "conv_out", cur, nout, LTX_PERM_UNPATCH, 0, &v->conv_out));
    if (c.timestep_conditioning) {
        LTX_TRY(load_temb(v, wm, "time_embedder", 2 * cur, &v->out_te));
        LTX_TRY(ltx_load_tensor(wm, "scale_shift_table", 2 * (int64_t)cur, v->dtype, &v->sst_out)); v->owned.push_back(v->sst_out);
        const ltx_weight* t = wm.find("timestep_scale_multiplier");
        if (t) {
            void* d = nullptr;
            LTX_TRY(ltx_load_tensor(wm, "timestep_scale_multiplier", 1, LTX_DT_F32, &d));
            HIP_TRY(hipMemcpy(&v->tsm, d, sizeof(float), hipMemcpyDeviceToHost)); (void)hipFree(d);
            v->has_tsm = true;
        }
    }
    // latents_mean / latents_std (vae.rs:1827-1838): from weights when present, else 0 / 1
    {
        const int C = c.latent_channels;
        std::vector<float> z(C, 0.f), o(C, 1.f);
        HIP_TRY(hipMalloc((void**)&v->mean, sizeof(float) * C)); v->owned.push_back(v->mean);
        HIP_TRY(hipMalloc((void**)&v->std_, sizeof(float) * C)); v->owned.push_back(v->std_);
        const ltx_weight* lm = wm0.find("latents_mean"); const ltx_weight* ls = wm0.find("latents_std");
        if (lm) LTX_TRY(ltx_upload_cast(lm, v->mean, LTX_DT_F32, C, "latents_mean")); else HIP_TRY(hipMemcpy(v->mean, z.data(), sizeof(float) * C, hipMemcpyHostToDevice));
        if (ls) LTX_TRY(ltx_upload_cast(ls, v->std_, LTX_DT_F32, C, "latents_std")); else HIP_TRY(hipMemcpy(v->std_, o.data(), sizeof(float) * C, hipMemcpyHostToDevice));
    }
    // sinusoid table exp(-ln(1e4) * i / 128) with the reference's f32 roundings (vae.rs:172-198)
    {
        std::vector<float> tab(128);
        ltx_sinusoid_table(1, tab.data());
        HIP_TRY(hipMalloc((void**)&v->vtab, sizeof(float) * 128)); v->owned.push_back(v->vtab);
        HIP_TRY(hipMemcpy(v->vtab, tab.data(), sizeof(float) * 128, hipMemcpyHostToDevice));
    }
    return LTX_OK;
}

// CombinedTimestepEmbedder (vae.rs:236-265) + "+ scale_shift_table" -> f32 [B][rows][C]; *out points at the (cached) result
int time_mod(ltx_vae* v, const TimeEmbW& te, const void* sst, const TimeVec& tv, const float** out, hipStream_t s) {
    const int dt = v->dtype; const int B = tv.n;
    ltx_vae::ModEntry* e = nullptr;
    for (auto& c : v->mods) if (c.sst == sst && c.n == B && c.stream == s && !memcmp(c.t, tv.t, sizeof(float) * B)) e = &c;
    if (!e) {
        constexpr size_t kMax = 256;                       // entries (a decoder has ~21 tables; tiled decodes add leaf-batch sizes)
        if (v->mods.size() < kMax) { v->mods.emplace_back(); e = &v->mods.back(); }
        else { e = &v->mods.front(); for (auto& c : v->mods) if (c.used < e->used) e = &c; }
        e->sst = nullptr;
        LTX_TRY(e->buf.ensure((size_t)B * te.dim * sizeof(float)));
        LTX_TRY(ltx_launch_sinusoid(v->tproj.p, dt, tv, v->vtab, 128, dt == LTX_DT_BF16, v->has_tsm ? v->tsm : 1.0f, s));
        LTX_TRY(ltx_linear(te.l1, v->tproj.p, 256, v->e1.p, te.dim, B, dt, EPI_BIAS, s));
        LTX_TRY(ltx_launch_silu(v->e1.p, v->e1.p, (int64_t)B * te.dim, dt, s));
        LTX_TRY(ltx_linear(te.l2, v->e1.p, te.dim, v->te.p, te.dim, B, dt, EPI_BIAS, s));
        LTX_TRY(ltx_launch_ada(e->buf.as<float>(), sst, v->te.p, 1, B, te.dim, dt, s));
        e->sst = sst; e->n = B; e->stream = s; memcpy(e->t, tv.t, sizeof(float) * B);
    }
    e->used = ++v->mod_clock;
    *out = e->buf.as<float>();
    return LTX_OK;
}

// one injection: the next plane of the handle's noise stream, y = x + plane[h, w] * scale[c] (+ shortcut)
int inject_noise(ltx_vae* v, const void* x, void* y, const void* scale, const void* shortcut, const Dims& d, int ch, hipStream_t s) {
    const int64_t hw = (int64_t)d.H * d.W;
    HIP_TRY(hipStreamSynchronize(s));                       // the previous injection's copy may still be reading the (pageable) host image, its kernel the plane
    v->noise_host.resize((size_t)hw);
    LTX_TRY(ltx_pcg32_randn(v->noise_seed, v->noise_ctr++, (size_t)hw, v->noise_host.data()));
    LTX_TRY(v->noise_plane.ensure((size_t)hw * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(v->noise_plane.p, v->noise_host.data(), (size_t)hw * sizeof(float), hipMemcpyHostToDevice, s));
    return ltx_launch_noise_inject(x, y, v->noise_plane.as<float>(), scale, shortcut, d.vox(), ch, hw, v->dtype, s);
}

// the per-voxel RMS norm + modulation + SiLU of the resnets and of norm_out; shift: f32 [B][mod_stride] rows, the scale ch after it (null: none)
RowNormArgs norm_silu(const void* x, void* y, const Dims& d, int ch, int mod_stride, const float* shift) {
    RowNormArgs rn; rn.x = x; rn.y = y; rn.rows = d.vox(); rn.D = ch; rn.ldx = ch; rn.ldy = ch;
    rn.kind = 0; rn.eps = 1e-8f; rn.act = 1; rn.rows_per_batch = (int64_t)d.T * d.H * d.W; rn.mod_stride = mod_stride;
    if (shift) { rn.shift = shift; rn.scale = shift + ch; }
    return rn;
}

// LtxVideoResnetBlock3d without noise injection (vae.rs:755-821), in place on X with N and C as scratch.
// mod: f32 [B][mod_stride] rows of shift1, scale1, shift2, scale2 (null: no modulation)
int resnet_plain(int dt, int pad_t, const ResnetW& r, int ch, const Dims& d, const float* mod, int mod_stride, void* X, void* N, void* C, hipStream_t s) {
    LTX_TRY(ltx_launch_rownorm(norm_silu(X, N, d, ch, mod_stride, mod), dt, s));
    // norm2 + modulation + SiLU inside conv1's epilogue where one conv tile spans all channels (128 / 256): no pass of
    // its own over the stage's largest tensor
    if (fuse_norm2(dt, pad_t, r.c1, d, ch)) {
        PostNorm pn; pn.on = 1; pn.eps = 1e-8f; pn.act = 1; pn.mod_stride = mod_stride;
        if (mod) { pn.shift = mod + 2 * ch; pn.scale = mod + 3 * ch; }
        LTX_TRY(conv3d(dt, pad_t, r.c1, N, C, d, EPI_BIAS, nullptr, 0, s, &pn));
        return conv3d(dt, pad_t, r.c2, C, X, d, EPI_RESID, X, 0, s);   // X = conv2(..) + X, in place
    }
    LTX_TRY(conv3d(dt, pad_t, r.c1, N, C, d, EPI_BIAS, nullptr, 0, s));
    LTX_TRY(ltx_launch_rownorm(norm_silu(C, N, d, ch, mod_stride, mod ? mod + 2 * ch : nullptr), dt, s));
    return conv3d(dt, pad_t, r.c2, N, X, d, EPI_RESID, X, 0, s);       // X = conv2(..) + X, in place
}

int resnet(ltx_vae* v, const ResnetW& r, const TimeEmbW& te, int ch, const Dims& d, const TimeVec* tv, hipStream_t s) {
    const int dt = v->dtype, pad_t = v->cfg.decoder_causal ? 2 : 1;
    const float* mod = nullptr;
    if (tv && r.sst) LTX_TRY(time_mod(v, te, r.sst, *tv, &mod, s));
    if (!r.pcs1 && !r.pcs2) return resnet_plain(dt, pad_t, r, ch, d, mod, 4 * ch, v->X.p, v->N.p, v->C.p, s);
    LTX_TRY(ltx_launch_rownorm(norm_silu(v->X.p, v->N.p, d, ch, 4 * ch, mod), dt, s));
    LTX_TRY(conv3d(dt, pad_t, r.c1, v->N.p, v->C.p, d, EPI_BIAS, nullptr, 0, s));
    if (r.pcs1) LTX_TRY(inject_noise(v, v->C.p, v->C.p, r.pcs1, nullptr, d, ch, s));        // vae.rs:784
    LTX_TRY(ltx_launch_rownorm(norm_silu(v->C.p, v->N.p, d, ch, 4 * ch, mod ? mod + 2 * ch : nullptr), dt, s));
    if (r.pcs2) {                                                                           // vae.rs:807-819: h = conv2(h); h += noise * scale; h + x
        LTX_TRY(conv3d(dt, pad_t, r.c2, v->N.p, v->C.p, d, EPI_BIAS, nullptr, 0, s));
        return inject_noise(v, v->C.p, v->X.p, r.pcs2, v->X.p, d, ch, s);
    }
    return conv3d(dt, pad_t, r.c2, v->N.p, v->X.p, d, EPI_RESID, v->X.p, 0, s);             // X = conv2(..) + X, in place
}

// LtxVideoDecoder3d::forward on a channels-last latent `z` [B,F,H,W,Clat] (model dtype) -> f32 NCTHW
int decoder_forward(ltx_vae* v, const void* z, int B, int F, int H, int W, const TimeVec* tv, int post, float* out, hipStream_t s) {
    const ltx_vae_config& c = v->cfg;
    const int dt = v->dtype, pad_t = c.decoder_causal ? 2 : 1; const size_t esz = ltx_dt_size(dt);
    // workspace sizing: the largest activation is the last stage
    Dims d{B, F, H, W};
    int64_t max_elems = d.vox() * v->mid_ch;
    {
        Dims q = d;
        for (auto& u : v->ups) { if (u.temporal) q.T = 2 * q.T - 1; q.H *= 2; q.W *= 2; int64_t e = q.vox() * u.ch; if (e > max_elems) max_elems = e; }
    }
    LTX_TRY(v->X.ensure(max_elems * esz)); LTX_TRY(v->Y.ensure(max_elems * esz));
    LTX_TRY(v->N.ensure(max_elems * esz)); LTX_TRY(v->C.ensure(max_elems * esz));
    const int maxdim = 4 * v->mid_ch;
    LTX_TRY(v->tproj.ensure((size_t)B * 256 * esz)); LTX_TRY(v->e1.ensure((size_t)B * maxdim * esz));
    LTX_TRY(v->te.ensure((size_t)B * maxdim * esz)); LTX_TRY(v->mod.ensure((size_t)B * maxdim * sizeof(float)));
    const TimeVec* tvc = (tv && c.timestep_conditioning) ? tv : nullptr;

    LTX_TRY(conv3d(dt, pad_t, v->conv_in, z, v->X.p, d, EPI_BIAS, nullptr, 0, s));
    for (auto& r : v->mid) LTX_TRY(resnet(v, r, v->mid_te, v->mid_ch, d, tvc, s));
    for (auto& u : v->ups) {
        LTX_TRY(conv3d(dt, pad_t, u.up, v->X.p, v->Y.p, d, EPI_D2S, u.residual ? v->X.p : nullptr, 0, s));   // vae.rs:1164-1168
        std::swap(v->X, v->Y);
        if (u.temporal) d.T = 2 * d.T - 1;
        d.H *= 2; d.W *= 2;
        for (auto& r : u.res) LTX_TRY(resnet(v, r, u.te, u.ch, d, tvc, s));
    }
    // norm_out + global scale/shift + SiLU (vae.rs:1687-1723), conv_out + unpatchify
    const int ch = v->last_ch;
    const float* mod = nullptr;
    if (tvc && v->sst_out) LTX_TRY(time_mod(v, v->out_te, v->sst_out, *tvc, &mod, s));
    LTX_TRY(ltx_launch_rownorm(norm_silu(v->X.p, v->N.p, d, ch, 2 * ch, mod), dt, s));
    return conv3d(dt, pad_t, v->conv_out, v->N.p, out, d, EPI_UNPATCH, nullptr, post, s);
}

int crop_cl(const void* src, void* dst, size_t esz, int B, int T, int H, int W, int C, int t0, int t1, int h0, int h1, int w0, int w1, hipStream_t s) {
    int64_t n = (int64_t)B * (t1 - t0) * (h1 - h0) * (w1 - w0) * C * (int64_t)esz;
    hipLaunchKernelGGL(cl_window_kernel, dim3(ltx_grid1d(n, 16384)), dim3(256), 0, s, (const unsigned char*)src, (unsigned char*)dst, (int)esz,
                       B, T, H, W, C, t0, t1, h0, h1, w0, w1);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}

struct Tile { float* p; int t, h, w; };   // f32 NCTHW tile [BC, t, h, w]: decoded samples, or encoded moments

// The spatial walk of tiled_decode and tiled_encode (vae.rs:2259-2290 / :2190-2223): per tile of the plan, row-major,
// produce(row span, col span, take, &tile) fills the tile (take(bytes, &p): the next buffer of `pool`); then blend_v with the
// (already blended) tile above, blend_h with the one to the left, and the tile's kept corner goes into `out` [BC, tile.t, oH, oW].
template <typename Produce>
int assemble_spatial(const VaeTilePlan& plan, Produce produce, int BC, float* out, std::deque<DevBuf>& pool, hipStream_t s) {
    size_t pool_used = 0;
    auto take = [&](size_t bytes, float** p) -> int {
        if (pool_used >= pool.size()) pool.emplace_back();
        DevBuf& b = pool[pool_used++];
        LTX_TRY(b.ensure(bytes));
        *p = b.as<float>();
        return LTX_OK;
    };
    std::vector<Tile> prev, cur;
    int oy = 0;
    for (size_t ri = 0; ri < plan.rows.size(); ++ri) {
        cur.clear();
        int ox = 0, row_h = 0;
        for (size_t ci = 0; ci < plan.cols.size(); ++ci) {
            Tile t{};
            LTX_TRY(produce(plan.rows[ri], plan.cols[ci], take, &t));
            if (ri > 0) {               // blend_v
                BlendArgs ba; ba.a = prev[ci].p; ba.b = t.p; ba.dst = t.p; ba.BC = BC;
                ba.at = prev[ci].t; ba.ah = prev[ci].h; ba.aw = prev[ci].w; ba.a_len = prev[ci].h;
                ba.bt = ba.dt = t.t; ba.bh = ba.dh = t.h; ba.bw = ba.dw = t.w;
                ba.dim = 3; ba.blend = std::min(plan.blend_h, std::min(prev[ci].h, t.h));
                ba.et = t.t; ba.eh = ba.blend; ba.ew = std::min(t.w, prev[ci].w);
                LTX_TRY(ltx_launch_blend(ba, s));
            }
            if (ci > 0) {               // blend_h
                BlendArgs ba; ba.a = cur[ci - 1].p; ba.b = t.p; ba.dst = t.p; ba.BC = BC;
                ba.at = cur[ci - 1].t; ba.ah = cur[ci - 1].h; ba.aw = cur[ci - 1].w; ba.a_len = cur[ci - 1].w;
                ba.bt = ba.dt = t.t; ba.bh = ba.dh = t.h; ba.bw = ba.dw = t.w;
                ba.dim = 4; ba.blend = std::min(plan.blend_w, std::min(cur[ci - 1].w, t.w));
                ba.et = t.t; ba.eh = std::min(t.h, cur[ci - 1].h); ba.ew = ba.blend;
                LTX_TRY(ltx_launch_blend(ba, s));
            }
            cur.push_back(t);
            const int hs = std::min(plan.keep_h, t.h), ws = std::min(plan.keep_w, t.w);
            const int ch = std::min(hs, plan.oH - oy), cw_ = std::min(ws, plan.oW - ox);
            if (ch > 0 && cw_ > 0)
                LTX_TRY(ltx_launch_copy_window(t.p, t.t, t.h, t.w, out, t.t, plan.oH, plan.oW, BC, t.t, ch, cw_, 0, oy, ox, s));
            ox += ws; row_h = hs;
        }
        oy += row_h;
        prev = cur;
    }
    return LTX_OK;
}

// One step of the temporal walks (vae.rs:2400-2434 / :2322-2347): window li arrives as `buf` [BC, phys, oH, oW]; the plan says
// which frame it loses and how many it gives.  Those go into `out` at frame `ot`, blended against the RAW previous window
// (row[idx - 1], not its blended form), which *prev carries from step to step.
struct TWin { const float* p = nullptr; int len = 0, phys = 0; };   // logical start, logical length, physical frame count
int place_temporal(const VaeTilePlan& plan, int li, const float* buf, int phys, TWin* prev, int BC, float* out, int ot, int* keep, hipStream_t s) {
    const VaeTilePlan::Frames f = plan.frames(li, phys);
    const TWin cur{buf + (size_t)f.skip * plan.oH * plan.oW, f.len, phys};
    const int n = std::min(f.keep, plan.oT - ot);
    if (n > 0) {
        LTX_TRY(ltx_launch_copy_window(cur.p, phys, plan.oH, plan.oW, out, plan.oT, plan.oH, plan.oW, BC, n, plan.oH, plan.oW, ot, 0, 0, s));
        if (li > 0) {
            BlendArgs ba; ba.a = prev->p; ba.b = cur.p; ba.dst = out; ba.BC = BC;
            ba.at = prev->phys; ba.ah = plan.oH; ba.aw = plan.oW; ba.a_len = prev->len;
            ba.bt = phys; ba.bh = plan.oH; ba.bw = plan.oW; ba.dt = plan.oT; ba.dh = plan.oH; ba.dw = plan.oW; ba.ot = ot;
            ba.dim = 2; ba.blend = std::min(plan.blend_t, std::min(prev->len, cur.len));
            ba.et = std::min(ba.blend, n); ba.eh = plan.oH; ba.ew = plan.oW;
            LTX_TRY(ltx_launch_blend(ba, s));
        }
    }
    *prev = cur; *keep = f.keep;
    return LTX_OK;
}

// tiled_decode (vae.rs:2225-2290) of a channels-last latent window of F frames; result into `out` [BC, (F-1)*tr+1, oH, oW]
// `pre` (optional): the window's leaf tiles already decoded, in plan order (batched_leaf_decode) - then nothing is decoded here.
int tiled_decode(ltx_vae* v, const void* z, int B, int F, int H, int W, const TimeVec* tv, const VaeTilePlan& plan,
                 float* out, hipStream_t s, const std::vector<float*>* pre = nullptr) {
    const ltx_vae_config& c = v->cfg;
    const int r = c.spatial_compression_ratio, BC = B * c.out_channels;
    const size_t esz = ltx_dt_size(v->dtype);
    auto dims = [&](TileSpan row, TileSpan col, Tile* t) { t->t = (F - 1) * c.temporal_compression_ratio + 1; t->h = (row.i1 - row.i0) * r; t->w = (col.i1 - col.i0) * r; };
    size_t leaf = 0;
    auto next_leaf = [&](TileSpan row, TileSpan col, auto&, Tile* t) -> int {
        if (leaf >= pre->size()) LTX_FAIL(LTX_ERR_ARG, "tiled decode: fewer pre-decoded leaves than tiles");
        dims(row, col, t); t->p = (*pre)[leaf++];
        return LTX_OK;
    };
    auto decode_tile = [&](TileSpan row, TileSpan col, auto& take, Tile* t) -> int {
        const int th = row.i1 - row.i0, tw = col.i1 - col.i0;
        dims(row, col, t);
        LTX_TRY(v->tile_lat.ensure((size_t)B * F * th * tw * c.latent_channels * esz));
        LTX_TRY(crop_cl(z, v->tile_lat.p, esz, B, F, H, W, c.latent_channels, 0, F, row.i0, row.i1, col.i0, col.i1, s));
        LTX_TRY(take((size_t)BC * t->t * t->h * t->w * sizeof(float), &t->p));
        return decoder_forward(v, v->tile_lat.p, B, F, th, tw, tv, 0, t->p, s);
    };
    return pre ? assemble_spatial(plan, next_leaf, BC, out, v->tilebufs, s) : assemble_spatial(plan, decode_tile, BC, out, v->tilebufs, s);
}

// Leaf tiles of the framewise + spatially tiled decode, decoded up front in batches.  The reference's tiled decode is a serial
// loop of independent `decoder.forward` calls on small latents (vae.rs:2382-2408 around :2246-2257; C2: 52 calls of at most
// 3 x 16 x 16 latents), whose first stages cannot fill the chip one tile at a time (the mid block of one tile is 768
// voxels).  Leaves that share a latent shape - the same spatial tile of different temporal windows - are stacked along the
// batch axis (up to 16 samples per decoder call), and the blends then run over the decoded tiles in exactly the reference's
// order (tiled_decode with `pre`).  A decoder call on a batch gives each sample the bits it gets alone: no op crosses samples.
// per_window[li] = the window's leaves in plan order, rows x cols.  LTX_VAE_TILE_BATCH=0: one call per leaf (A/B aid).
int batched_leaf_decode(ltx_vae* v, const void* z, int B, int F, int H, int W, const TimeVec* tv, const VaeTilePlan& plan,
                        std::vector<std::vector<float*>>& per_window, hipStream_t s) {
    const ltx_vae_config& c = v->cfg;
    const int r = c.spatial_compression_ratio, tr = c.temporal_compression_ratio;
    const size_t esz = ltx_dt_size(v->dtype);
    struct Leaf { int li, slot, t0, t1, h0, h1, w0, w1; };
    std::vector<Leaf> leaves;
    for (size_t li = 0; li < plan.windows.size(); ++li) {
        int slot = 0;
        for (const TileSpan& row : plan.rows)
            for (const TileSpan& col : plan.cols) leaves.push_back({(int)li, slot++, plan.windows[li].i0, plan.windows[li].i1, row.i0, row.i1, col.i0, col.i1});
    }
    per_window.assign(plan.windows.size(), std::vector<float*>(plan.rows.size() * plan.cols.size(), nullptr));
    auto elems = [&](const Leaf& l) { return (size_t)B * c.out_channels * ((size_t)(l.t1 - l.t0 - 1) * tr + 1) * ((size_t)(l.h1 - l.h0) * r) * ((size_t)(l.w1 - l.w0) * r); };
    size_t total = 0;
    for (const Leaf& l : leaves) total += elems(l);
    LTX_TRY(v->predec.ensure(total * sizeof(float)));
    // Leaves per decoder call.  The reference tiles to CAP memory (vae.rs:2225-2290), so the batch must not undo that: it is
    // bounded by a share of the memory that is free now, against a generous estimate of one leaf's activations (six tensors
    // of the largest, 128-channel stage + its f32 output), and a call that still fails to allocate is retried with half as
    // many leaves, down to one.  Option vae_tile_batch=n: at most n leaves per call (-1: one).
    int max_n = LTX_MAX_BATCH / B; if (max_n < 1) max_n = 1;
    if (const int n_opt = ltx_opt().vae_tile_batch) max_n = n_opt < 0 ? 1 : std::min(max_n, n_opt);
    if (v->any_inject) max_n = 1;        // a decoder call draws ONE noise plane per injection for its whole batch (vae.rs:741-753): leaves keep their own draws
    std::vector<char> done(leaves.size(), 0);
    float* cursor = v->predec.as<float>();
    for (size_t a = 0; a < leaves.size(); ++a) {
        if (done[a]) continue;
        const Leaf& la = leaves[a];
        const int nf = la.t1 - la.t0, th = la.h1 - la.h0, tw = la.w1 - la.w0;
        int cap = max_n;
        {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
                const double act = 6.0 * (double)B * ((double)(nf - 1) * tr + 1) * (th * r / 4.0) * (tw * r / 4.0) * 128.0 * (double)esz + (double)elems(la) * 4.0;
                const double fit = 0.5 * ((double)free_b + (double)v->act_bytes_reserved()) / (act > 1.0 ? act : 1.0);
                if (fit < (double)cap) cap = fit < 1.0 ? 1 : (int)fit;
            } else (void)hipGetLastError();
        }
        std::vector<size_t> grp;
        for (size_t b = a; b < leaves.size() && (int)grp.size() < cap; ++b) {
            const Leaf& lb = leaves[b];
            if (!done[b] && lb.t1 - lb.t0 == nf && lb.h1 - lb.h0 == th && lb.w1 - lb.w0 == tw) { grp.push_back(b); done[b] = 1; }
        }
        const int n = (int)grp.size();
        const size_t leaf_lat = (size_t)B * nf * th * tw * c.latent_channels * esz, leaf_out = elems(la);
        LTX_TRY(v->tile_lat.ensure(leaf_lat * n));
        TimeVec tvb; tvb.n = n * B;
        for (int k = 0; k < LTX_MAX_BATCH; ++k) tvb.t[k] = 0.f;
        for (int k = 0; k < n; ++k) {
            const Leaf& l = leaves[grp[k]];
            LTX_TRY(crop_cl(z, (char*)v->tile_lat.p + leaf_lat * k, esz, B, F, H, W, c.latent_channels, l.t0, l.t1, l.h0, l.h1, l.w0, l.w1, s));
            per_window[l.li][l.slot] = cursor + leaf_out * k;
            if (tv) for (int b = 0; b < B; ++b) tvb.t[k * B + b] = tv->t[b];
        }
        (void)ltx_take_oom();
        const int rc = decoder_forward(v, v->tile_lat.p, n * B, nf, th, tw, tv ? &tvb : nullptr, 0, cursor, s);
        if (rc != LTX_OK) {
            // only an allocation that did not fit is retried with fewer leaves per call; every other failure (argument, launch)
            // is deterministic and surfaces at once with its own message
            if (n == 1 || !ltx_take_oom()) return rc;
            (void)hipGetLastError();
            for (size_t k : grp) done[k] = 0;
            max_n = n / 2 < 1 ? 1 : n / 2;
            --a;
            continue;
        }
        cursor += leaf_out * n;
    }
    return LTX_OK;
}

struct ScopedBuf : DevBuf { ~ScopedBuf() { release(); } };   // a buffer that lives for one call

int decode_cl(ltx_vae* v, const void* z, int B, int F, int H, int W, const TimeVec* tv, const ltx_tiling* tl, int post, float* out, hipStream_t s) {
    const ltx_vae_config& c = v->cfg;
    const int tr = c.temporal_compression_ratio, BC = B * c.out_channels;
    const size_t esz = ltx_dt_size(v->dtype);
    VaeTilePlan plan;
    LTX_TRY(vae_decode_tile_plan(c.spatial_compression_ratio, tr, tl, F, H, W, &plan));
    const int oT = plan.oT, oH = plan.oH, oW = plan.oW;
    if (plan.mode == VaeTilePlan::kDirect) return decoder_forward(v, z, B, F, H, W, tv, post, out, s);     // vae.rs:2065 (post == 2: RGB8 from conv_out's epilogue)
    // RGB8 output of a TILED decode: the blends run on f32 tiles - decode into a scratch video, convert with the frame kernel (same bits)
    if (post == 2) {
        LTX_TRY(v->rgbtmp.ensure((size_t)BC * oT * oH * oW * sizeof(float)));
        LTX_TRY(decode_cl(v, z, B, F, H, W, tv, tl, 1, v->rgbtmp.as<float>(), s));
        return ltx_video_to_rgb8(v->rgbtmp.as<float>(), B, oT, oH, oW, reinterpret_cast<uint8_t*>(out), (ltx_stream)s);
    }
    if (plan.mode == VaeTilePlan::kSpatial) {
        LTX_TRY(tiled_decode(v, z, B, F, H, W, tv, plan, out, s));
    } else {
        // temporal_tiled_decode (vae.rs:2358-2434)
        ScopedBuf zt;                    // temporal latent window
        std::vector<std::vector<float*>> pre;                 // spatially tiled windows: every leaf decoded up front, in batches
        if (plan.window_tiled) LTX_TRY(batched_leaf_decode(v, z, B, F, H, W, tv, plan, pre, s));
        TWin prev; int ot = 0;
        for (size_t li = 0; li < plan.windows.size(); ++li) {
            const TileSpan win = plan.windows[li]; const int nf = win.i1 - win.i0;
            LTX_TRY(zt.ensure((size_t)B * nf * H * W * c.latent_channels * esz));
            LTX_TRY(crop_cl(z, zt.p, esz, B, F, H, W, c.latent_channels, win.i0, win.i1, 0, H, 0, W, s));
            const int dT = (nf - 1) * tr + 1;
            DevBuf& cur = v->tiles[li & 1];
            LTX_TRY(cur.ensure((size_t)BC * dT * oH * oW * sizeof(float)));
            LTX_TRY(plan.window_tiled ? tiled_decode(v, zt.p, B, nf, H, W, tv, plan, cur.as<float>(), s, &pre[li])
                                      : decoder_forward(v, zt.p, B, nf, H, W, tv, 0, cur.as<float>(), s));
            int keep = 0;
            LTX_TRY(place_temporal(plan, (int)li, cur.as<float>(), dT, &prev, BC, out, ot, &keep, s));
            ot += keep;
        }
        HIP_TRY(hipStreamSynchronize(s));    // zt is freed on the way out: not before the stream is done with it
    }
    if (post) LTX_TRY(ltx_launch_postprocess(out, (int64_t)BC * oT * oH * oW, s));
    return LTX_OK;
}

}  // namespace

extern "C" int ltx_vae_create(const ltx_vae_config* cfg, const ltx_weight* weights, size_t n_weights,
                              ltx_dtype model_dtype, int device, ltx_vae** out) {
    if (!cfg || !weights || !out) LTX_FAIL(LTX_ERR_ARG, "ltx_vae_create: null argument");
    *out = nullptr;
    if (cfg->n_blocks < 1 || cfg->n_blocks > 4) LTX_FAIL(LTX_ERR_ARG, "n_blocks must be 1..4");
    if (cfg->patch_size != 4 || cfg->patch_size_t != 1) LTX_FAIL(LTX_ERR_UNSUPPORTED, "only patch_size=4, patch_size_t=1 are supported");
    if (cfg->latent_channels % 8 != 0) LTX_FAIL(LTX_ERR_UNSUPPORTED, "latent_channels must be a multiple of 8");
    for (int i = 0; i < cfg->n_blocks; ++i) {
        if (cfg->decoder_upsample_factor[i] < 1 || cfg->decoder_block_out_channels[i] % (8 * cfg->decoder_upsample_factor[i]) != 0)
            LTX_FAIL(LTX_ERR_UNSUPPORTED, "decoder channels must be multiples of 8*upsample_factor");
    }
    HIP_TRY(hipSetDevice(device));
    ltx_vae* v = new ltx_vae();
    v->cfg = *cfg; v->dtype = model_dtype == LTX_BF16 ? LTX_DT_BF16 : LTX_DT_F32; v->device = device;
    int rc = build(v, weights, n_weights);
    if (rc != LTX_OK) { v->free_all(); delete v; return rc; }
    *out = v;
    return LTX_OK;
}
extern "C" void ltx_vae_destroy(ltx_vae* v) {
    if (!v) return;
    (void)hipSetDevice(v->device); (void)hipDeviceSynchronize();
    v->free_all(); delete v;
}
extern "C" int ltx_vae_set_noise_seed(ltx_vae* v, uint64_t seed) {
    if (!v) LTX_FAIL(LTX_ERR_ARG, "ltx_vae_set_noise_seed: null handle");
    v->noise_seed = seed; v->noise_ctr = 0; return LTX_OK;
}
extern "C" int ltx_vae_injects_noise(const ltx_vae* v) { return v && v->any_inject ? 1 : 0; }
extern "C" int ltx_vae_get_config(const ltx_vae* v, ltx_vae_config* out) {
    if (!v || !out) LTX_FAIL(LTX_ERR_ARG, "ltx_vae_get_config: null argument");
    *out = v->cfg; return LTX_OK;
}
extern "C" const float* ltx_vae_latents_mean(const ltx_vae* v) { return v ? v->mean : nullptr; }
extern "C" const float* ltx_vae_latents_std(const ltx_vae* v) { return v ? v->std_ : nullptr; }

static int check_decode_args(ltx_vae* v, int B, int F, int H, int W) {
    if (!v) LTX_FAIL(LTX_ERR_ARG, "ltx_vae_decode: null handle");
    if (B < 1 || F < 1 || H < 1 || W < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_vae_decode: bad shape");
    return LTX_OK;
}
// The trait has no batch bound (t2v_pipeline.rs:102); samples never interact in the decoder (vae.rs:2107-2121 even decodes them
// one at a time under use_slicing), so batches beyond the 8 per-sample scalars a launch carries run as chunks of 8.
static size_t out_elems_per_sample(const ltx_vae* v, int F, int H, int W) {
    const ltx_vae_config& c = v->cfg;
    return (size_t)c.out_channels * ((size_t)(F - 1) * c.temporal_compression_ratio + 1) * ((size_t)H * c.spatial_compression_ratio) * ((size_t)W * c.spatial_compression_ratio);
}

extern "C" int ltx_vae_decode(ltx_vae* v, const void* latents, ltx_dtype io_dtype, const float* timestep,
                              int B, int F, int H, int W, const ltx_tiling* tiling, int postprocess,
                              float* out, ltx_stream stream) {
    LTX_TRY(check_decode_args(v, B, F, H, W));
    if (!latents || !out) LTX_FAIL(LTX_ERR_ARG, "ltx_vae_decode: null tensor");
    if (B > 8) {
        const size_t in_b = (size_t)v->cfg.latent_channels * F * H * W * (io_dtype == LTX_BF16 ? 2 : 4), out_b = out_elems_per_sample(v, F, H, W);
        for (int b0 = 0; b0 < B; b0 += 8)
            LTX_TRY(ltx_vae_decode(v, (const char*)latents + b0 * in_b, io_dtype, timestep ? timestep + b0 : nullptr, B - b0 < 8 ? B - b0 : 8, F, H, W, tiling,
                                   postprocess, postprocess == 2 ? reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(out) + b0 * out_b) : out + b0 * out_b, stream));
        return LTX_OK;
    }
    HIP_TRY(hipSetDevice(v->device));
    hipStream_t s = (hipStream_t)stream;
    const int C = v->cfg.latent_channels; const int64_t S = (int64_t)F * H * W;
    LTX_TRY(v->zin.ensure((size_t)B * S * C * ltx_dt_size(v->dtype)));
    LTX_TRY(ltx_launch_ncthw_to_cl(latents, io_dtype == LTX_BF16 ? LTX_DT_BF16 : LTX_DT_F32, v->zin.p, v->dtype, B, C, S, s));
    TimeVec tv; tv.n = B; for (int i = 0; i < 8; ++i) tv.t[i] = (timestep && i < B) ? timestep[i] : 0.f;
    return decode_cl(v, v->zin.p, B, F, H, W, timestep ? &tv : nullptr, tiling, postprocess, out, s);
}

extern "C" int ltx_vae_decode_tokens(ltx_vae* v, const float* tokens, const float* noise, const float* noise_scale,
                                     const float* timestep, int B, int F, int H, int W, const ltx_tiling* tiling,
                                     int postprocess, float* out, ltx_stream stream) {
    LTX_TRY(check_decode_args(v, B, F, H, W));
    if (!tokens || !out) LTX_FAIL(LTX_ERR_ARG, "ltx_vae_decode_tokens: null tensor");
    if (noise && !noise_scale) LTX_FAIL(LTX_ERR_ARG, "ltx_vae_decode_tokens: noise needs noise_scale");
    if (B > 8) {
        const size_t in_e = (size_t)v->cfg.latent_channels * F * H * W, out_b = out_elems_per_sample(v, F, H, W);
        for (int b0 = 0; b0 < B; b0 += 8)
            LTX_TRY(ltx_vae_decode_tokens(v, tokens + b0 * in_e, noise ? noise + b0 * in_e : nullptr, noise ? noise_scale + b0 : nullptr, timestep ? timestep + b0 : nullptr,
                                          B - b0 < 8 ? B - b0 : 8, F, H, W, tiling, postprocess,
                                          postprocess == 2 ? reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(out) + b0 * out_b) : out + b0 * out_b, stream));
        return LTX_OK;
    }
    HIP_TRY(hipSetDevice(v->device));
    hipStream_t s = (hipStream_t)stream;
    const int C = v->cfg.latent_channels; const int64_t S = (int64_t)F * H * W;
    LTX_TRY(v->zin.ensure((size_t)B * S * C * ltx_dt_size(v->dtype)));
    TimeVec ns; ns.n = B; for (int i = 0; i < 8; ++i) ns.t[i] = (noise && i < B) ? noise_scale[i] : 0.f;
    LTX_TRY(ltx_launch_denorm_mix(tokens, v->mean, v->std_, 1.0f / v->cfg.scaling_factor, noise, ns, v->zin.p, v->dtype, B, S, C, s));
    TimeVec tv; tv.n = B; for (int i = 0; i < 8; ++i) tv.t[i] = (timestep && i < B) ? timestep[i] : 0.f;
    return decode_cl(v, v->zin.p, B, F, H, W, timestep ? &tv : nullptr, tiling, postprocess, out, s);
}

extern "C" int ltx_vae_prepare_latents(ltx_vae* v, const float* tokens, const float* noise, const float* noise_scale,
                                       int B, int F, int H, int W, float* out_tokens, ltx_stream stream) {
    LTX_TRY(check_decode_args(v, B, F, H, W));
    if (!tokens || !out_tokens) LTX_FAIL(LTX_ERR_ARG, "ltx_vae_prepare_latents: null tensor");
    if (noise && !noise_scale) LTX_FAIL(LTX_ERR_ARG, "ltx_vae_prepare_latents: noise needs noise_scale");
    if (B > 8) {
        const size_t in_e = (size_t)v->cfg.latent_channels * F * H * W;
        for (int b0 = 0; b0 < B; b0 += 8)
            LTX_TRY(ltx_vae_prepare_latents(v, tokens + b0 * in_e, noise ? noise + b0 * in_e : nullptr, noise ? noise_scale + b0 : nullptr, B - b0 < 8 ? B - b0 : 8, F, H, W,
                                            out_tokens + b0 * in_e, stream));
        return LTX_OK;
    }
    HIP_TRY(hipSetDevice(v->device));
    const int C = v->cfg.latent_channels; const int64_t S = (int64_t)F * H * W;
    TimeVec ns; ns.n = B; for (int i = 0; i < 8; ++i) ns.t[i] = (noise && i < B) ? noise_scale[i] : 0.f;
    return ltx_launch_denorm_mix(tokens, v->mean, v->std_, 1.0f / v->cfg.scaling_factor, noise, ns, out_tokens, LTX_DT_F32, B, S, C,
                                 (hipStream_t)stream);
}

// =====================================================================================================================
// encode side: LtxVideoEncoder3d (vae.rs:1316-1469) + posterior + tiled encodes.  Same layout as the decoder: activations
// channels-last in the model dtype, every 3x3x3 conv through conv3d.h's conv3d (the measured conv kernels, pad_t = 2).
//   patchify            one gather kernel, coalesced on the read side: [B,3,F,H,W] -> [B,F,H/4,W/4,48]
//   resnet              the decoder's, without modulation / noise / timestep (norm2 in conv1's epilogue where that form applies)
//   downsampler         one conv whose epilogue (EPI_S2D, kernels.h: the mirror of EPI_D2S) scatters to the space-to-depth
//                       channel and adds the grouped-mean residual.  The reference convolves the input with st - 1 leading
//                       frames repeated (vae.rs:539-544); with a causal conv that output is the conv of the un-repeated input
//                       with ITS first frame repeated (frame t of the former reads input frames max(t-3,0), max(t-2,0),
//                       max(t-1,0) = frame t-1 of the latter), so the repeat is an index clamp: the first frame's tiles store
//                       twice, and no padded copy exists
//   conv_out            129 output channels padded to 132 with zero weights; one kernel reads its rows and writes mean and the
//                       broadcast logvar in f32 NCTHW (untiled), or the moments [B,129,F',h,w] the tiled paths blend; the
//                       256-channel tensor of vae.rs:1463-1467 never exists
// =====================================================================================================================
struct DownBlockW { std::vector<ResnetW> res; ConvW down; int ch = 0, cout = 0, cc = 0, st = 1, sh = 1, sw = 1, group = 1; bool has_down = false; };

struct ltx_vae_encoder {
    ltx_vae_encoder_config cfg{};
    int dtype = LTX_DT_BF16, device = 0;
    ConvW conv_in, conv_out;
    std::vector<DownBlockW> downs;
    std::vector<ResnetW> mid;
    int mid_ch = 0, nmom = 0, nmom_pad = 0, cin_p = 0;
    std::vector<void*> owned;
    DevBuf X, Y, N, C, mom, ttiles[2], scratch;
    std::deque<DevBuf> tilebufs;
    void free_all() {
        for (void* p : owned) if (p) (void)hipFree(p);
        owned.clear();
        DevBuf* bs[] = {&X, &Y, &N, &C, &mom, &ttiles[0], &ttiles[1], &scratch};
        for (DevBuf* b : bs) b->release();
        for (auto& b : tilebufs) b.release();
    }
};

namespace {

// [B,C,F,H,W] window (t0.., h0.., w0.., extent nt x nh x nw) -> channels-last [B,nt,nh/p,nw/p,C*p*p], packed channel
// (c*p + off_w)*p + off_h (vae.rs:1426-1444 with patch_size_t = 1).  One thread per input element: reads run along W.
template <typename TI, typename TO>
__global__ void patchify_kernel(const TI* __restrict__ x, TO* __restrict__ y, int B, int C, int F, int H, int W,
                                int t0, int h0, int w0, int nt, int nh, int nw, int p) {
    const int64_t n = (int64_t)B * C * nt * nh * nw;
    const int hp = nh / p, wp = nw / p, cp = C * p * p;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
        int w = (int)(idx % nw); int64_t r = idx / nw; int h = (int)(r % nh); r /= nh; int t = (int)(r % nt); r /= nt;
        int c = (int)(r % C); int b = (int)(r / C);
        const float v = to_f32(x[((((int64_t)b * C + c) * F + t0 + t) * H + h0 + h) * W + w0 + w]);
        const int ch = (c * p + (w % p)) * p + (h % p);
        y[((((int64_t)b * nt + t) * hp + h / p) * wp + w / p) * cp + ch] = from_f32<TO>(v);
    }
}

// conv_out's channels-last result [B,S,ld] (first nmom channels) -> f32 NCTHW moments [B,nmom,S]
template <typename T>
__global__ void moments_kernel(const T* __restrict__ x, float* __restrict__ y, int B, int64_t S, int ld, int nmom) {
    const int64_t n = (int64_t)B * nmom * S;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
        int64_t sp = idx % S; int64_t r = idx / S; int c = (int)(r % nmom); int b = (int)(r / nmom);
        y[idx] = to_f32(x[((int64_t)b * S + sp) * ld + c]);
    }
}

// conv_out's channels-last result [B,S,ld] -> mean [B,L,S] f32 and (optional) logvar [B,L,S] = channel L replicated, in one pass
// (the untiled encode: no moments tensor in between)
template <typename T>
__global__ void moments_out_kernel(const T* __restrict__ x, float* __restrict__ mean, float* __restrict__ logvar, int B, int64_t S, int ld, int L) {
    const int64_t n = (int64_t)B * L * S;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
        int64_t sp = idx % S; int64_t r = idx / S; int c = (int)(r % L); int b = (int)(r / L);
        const T* row = x + ((int64_t)b * S + sp) * ld;
        mean[idx] = to_f32(row[c]);
        if (logvar) logvar[idx] = to_f32(row[L]);
    }
}

// moments [B,L+1,S] -> mean [B,L,S] and (optional) logvar [B,L,S] = channel L replicated (vae.rs:1463-1467 + :122-131)
__global__ void moments_split_kernel(const float* __restrict__ mom, float* __restrict__ mean, float* __restrict__ logvar, int B, int L, int64_t S) {
    const int64_t n = (int64_t)B * L * S;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
        int64_t sp = idx % S; int64_t r = idx / S; int c = (int)(r % L); int b = (int)(r / L);
        mean[idx] = mom[((int64_t)b * (L + 1) + c) * S + sp];
        if (logvar) logvar[idx] = mom[((int64_t)b * (L + 1) + L) * S + sp];
    }
}

__global__ void posterior_sample_kernel(const float* __restrict__ mean, const float* __restrict__ logvar, const float* __restrict__ eps,
                                        float* __restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = mean[i] + expf(logvar[i] * 0.5f) * eps[i];                                  // vae.rs:139-143
}

// moments [B,L+1,S] (+ eps [B,L,S] or null = mode) -> tokens [B,S,L] = (z - mean[c]) * sf / std[c]  (t2v_pipeline.rs:552-571, 474-504)
__global__ void moments_tokens_kernel(const float* __restrict__ mom, const float* __restrict__ eps, const float* __restrict__ lmean,
                                      const float* __restrict__ lstd, float sf, float* __restrict__ tok, int B, int L, int64_t S) {
    const int64_t n = (int64_t)B * S * L;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
        int c = (int)(idx % L); int64_t r = idx / L; int64_t sp = r % S; int b = (int)(r / S);
        float z = mom[((int64_t)b * (L + 1) + c) * S + sp];
        if (eps) z = z + expf(mom[((int64_t)b * (L + 1) + L) * S + sp] * 0.5f) * eps[((int64_t)b * L + c) * S + sp];
        tok[idx] = (z - lmean[c]) * sf / lstd[c];
    }
}

inline dim3 enc_grid(int64_t n) { return dim3(ltx_grid1d(n, 65536)); }

void down_stride(int type, int* st, int* sh, int* sw) {      // DownsampleType::stride, vae.rs:487-496
    *st = type == LTX_DOWN_SPATIAL ? 1 : 2; *sh = type == LTX_DOWN_TEMPORAL ? 1 : 2; *sw = *sh;
}

int enc_build(ltx_vae_encoder* e, const ltx_weight* weights, size_t n_weights) {
    const ltx_vae_encoder_config& c = e->cfg;
    const BareNames bare(weights, n_weights, "encoder.");
    WeightMap wm(bare.w.data(), bare.w.size());
    // vae.rs:1388-1394 loads norm_out.weight when the checkpoint has one (no released checkpoint does; else ones): refused, not ignored
    if (wm.find("norm_out.weight")) LTX_FAIL(LTX_ERR_UNSUPPORTED, "encoder checkpoint carries 'norm_out.weight': a weighted norm_out is not implemented (the presets' RMS norm has no weight)");
    const int nb = c.n_blocks;
    e->cin_p = c.in_channels * c.patch_size * c.patch_size * c.patch_size_t;
    LTX_TRY(load_conv(e->dtype, e->owned, wm, "conv_in", e->cin_p, c.block_out_channels[0], LTX_PERM_NONE, 0, &e->conv_in));
    e->downs.resize(nb - 1);
    int cur = c.block_out_channels[0];
    for (int i = 0; i < nb - 1; ++i) {
        DownBlockW& d = e->downs[i];
        const std::string p = "down_blocks." + std::to_string(i);
        d.ch = cur; d.cout = c.block_out_channels[i + 1];
        d.res.resize(c.layers_per_block[i]);
        for (int k = 0; k < c.layers_per_block[i]; ++k) LTX_TRY(load_resnet_convs(e->dtype, e->owned, wm, p + ".resnets." + std::to_string(k), cur, &d.res[k]));
        d.has_down = c.spatiotemporal_scaling[i] != 0;
        if (d.has_down) {
            down_stride(c.downsample_types[i], &d.st, &d.sh, &d.sw);
            const int nsub = d.st * d.sh * d.sw;
            if (d.cout % nsub != 0 || (cur * nsub) % d.cout != 0 || (d.cout / nsub) % 4 != 0)
                LTX_FAIL(LTX_ERR_UNSUPPORTED, "encoder downsampler: channels must divide by the stride volume (and the conv's by 4)");
            d.cc = d.cout / nsub; d.group = cur * nsub / d.cout;                       // vae.rs:516-517
            LTX_TRY(load_conv(e->dtype, e->owned, wm, p + ".downsamplers.0.conv", cur, d.cc, LTX_PERM_NONE, 0, &d.down));
            d.down.st = d.st; d.down.sh = d.sh; d.down.sw = d.sw; d.down.group = d.group;
        } else if (d.cout != cur) LTX_FAIL(LTX_ERR_UNSUPPORTED, "encoder down block without a downsampler cannot change the channel count");
        cur = d.cout;
    }
    e->mid_ch = cur;
    const int nmid = std::max(c.layers_per_block[nb - 1] - 1, 0);                      // vae.rs:1382-1386
    e->mid.resize(nmid);
    for (int k = 0; k < nmid; ++k) LTX_TRY(load_resnet_convs(e->dtype, e->owned, wm, "mid_block.resnets." + std::to_string(k), cur, &e->mid[k]));
    // conv_out: latent_channels + 1 outputs (vae.rs:1396-1405), padded with zero weights to the GEMM's multiple of 4
    e->nmom = c.latent_channels + 1; e->nmom_pad = (e->nmom + 3) / 4 * 4;
    {
        const ltx_weight* w = wm.find("conv_out.conv.weight"); const ltx_weight* b = wm.find("conv_out.conv.bias");
        if (!w) LTX_FAIL(LTX_ERR_MISSING_WEIGHT, "missing weight 'conv_out.conv.weight'");
        if (!b) LTX_FAIL(LTX_ERR_MISSING_WEIGHT, "missing weight 'conv_out.conv.bias'");
        if (ltx_numel(w) != (int64_t)e->nmom * cur * 27) LTX_FAIL(LTX_ERR_ARG, "weight 'conv_out.conv.weight': wrong size");
        if (ltx_numel(b) != e->nmom) LTX_FAIL(LTX_ERR_ARG, "weight 'conv_out.conv.bias': wrong size");
        const size_t wsz = ltx_dt_size(w->dtype == LTX_BF16 ? LTX_DT_BF16 : LTX_DT_F32), bsz = ltx_dt_size(b->dtype == LTX_BF16 ? LTX_DT_BF16 : LTX_DT_F32);
        const size_t wrow = (size_t)cur * 27 * wsz;
        DevBuf pw, pb;
        int rc = pw.ensure((size_t)e->nmom_pad * wrow); if (rc == LTX_OK) rc = pb.ensure((size_t)e->nmom_pad * bsz);
        if (rc == LTX_OK) {
            hipError_t he = hipMemset(pw.p, 0, (size_t)e->nmom_pad * wrow);
            if (he == hipSuccess) he = hipMemset(pb.p, 0, (size_t)e->nmom_pad * bsz);
            if (he == hipSuccess) he = hipMemcpy(pw.p, w->data, (size_t)e->nmom * wrow, w->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
            if (he == hipSuccess) he = hipMemcpy(pb.p, b->data, (size_t)e->nmom * bsz, b->on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
            if (he != hipSuccess) { ltx_set_error(std::string("conv_out padding: ") + hipGetErrorString(he)); rc = LTX_ERR_HIP; }
        }
        if (rc == LTX_OK) {
            ltx_weight pad[2] = {*w, *b};
            pad[0].data = pw.p; pad[0].on_device = 1; pad[0].shape[0] = e->nmom_pad;
            pad[1].data = pb.p; pad[1].on_device = 1; pad[1].shape[0] = e->nmom_pad;
            rc = conv_upload(e->dtype, e->owned, &pad[0], &pad[1], cur, e->nmom_pad, LTX_PERM_NONE, 0, &e->conv_out);
        }
        pw.release(); pb.release();
        if (rc != LTX_OK) return rc;
    }
    return LTX_OK;
}

// latent dims of an encoder call on nt x nh x nw samples, or LTX_ERR_ARG where the reference's reshapes fail
int enc_out_dims(const ltx_vae_encoder* e, int nt, int nh, int nw, int* ot, int* oh, int* ow) {
    const ltx_vae_encoder_config& c = e->cfg;
    if (nt < 1 || nh < 1 || nw < 1 || nt % c.patch_size_t != 0 || nh % c.patch_size != 0 || nw % c.patch_size != 0)
        LTX_FAIL(LTX_ERR_ARG, "input not divisible by patch sizes");                                     // vae.rs:1431-1433
    int t = nt / c.patch_size_t, h = nh / c.patch_size, w = nw / c.patch_size;
    for (const DownBlockW& d : e->downs) {
        if (!d.has_down) continue;
        if ((t + d.st - 1) % d.st != 0 || h % d.sh != 0 || w % d.sw != 0)
            LTX_FAIL(LTX_ERR_ARG, "input not divisible by patch sizes (a downsampler cannot halve frames + 1, height or width evenly)");
        t = (t + d.st - 1) / d.st; h /= d.sh; w /= d.sw;
    }
    *ot = t; *oh = h; *ow = w;
    return LTX_OK;
}

// LtxVideoEncoder3d::forward (vae.rs:1446-1468) on a window of `video` [B,Cin,F,H,W]; moments f32 [B,L+1,t',h',w']
int encoder_forward(ltx_vae_encoder* e, const void* video, int vdt, int B, int F, int H, int W,
                    int t0, int nt, int h0, int nh, int w0, int nw, float* moments, hipStream_t s,
                    float* mean_direct = nullptr, float* logvar_direct = nullptr) {
    const ltx_vae_encoder_config& c = e->cfg;
    const int dt = e->dtype; const size_t esz = ltx_dt_size(dt);
    int ot, oh, ow;
    LTX_TRY(enc_out_dims(e, nt, nh, nw, &ot, &oh, &ow));
    Dims d{B, nt / c.patch_size_t, nh / c.patch_size, nw / c.patch_size};
    int64_t max_elems = d.vox() * std::max(e->cin_p, c.block_out_channels[0]);
    {
        Dims q = d;
        for (const DownBlockW& b : e->downs) {
            max_elems = std::max(max_elems, q.vox() * std::max(b.ch, b.cc));
            if (b.has_down) { q.T = (q.T + b.st - 1) / b.st; q.H /= b.sh; q.W /= b.sw; }
            max_elems = std::max(max_elems, q.vox() * b.cout);
        }
        max_elems = std::max(max_elems, q.vox() * std::max(e->mid_ch, e->nmom_pad));
    }
    if (max_elems * (int64_t)esz >= 2147483648LL - (1 << 20) && B == 1)
        LTX_FAIL(LTX_ERR_UNSUPPORTED, "ltx_vae_encode: one sample's largest activation passes 2 GiB; use the tiled encode");
    LTX_TRY(e->X.ensure(max_elems * esz)); LTX_TRY(e->Y.ensure(max_elems * esz));
    LTX_TRY(e->N.ensure(max_elems * esz)); LTX_TRY(e->C.ensure(max_elems * esz));
    {
        const int64_t n = (int64_t)B * c.in_channels * nt * nh * nw;
#define LTX_PATCHIFY(TI, TO) hipLaunchKernelGGL((patchify_kernel<TI, TO>), enc_grid(n), dim3(256), 0, s, (const TI*)video, (TO*)e->Y.p, \
                                                B, c.in_channels, F, H, W, t0, h0, w0, nt, nh, nw, c.patch_size)
        if (vdt == LTX_DT_BF16) { if (dt == LTX_DT_BF16) LTX_PATCHIFY(bf16_t, bf16_t); else LTX_PATCHIFY(bf16_t, float); }
        else { if (dt == LTX_DT_BF16) LTX_PATCHIFY(float, bf16_t); else LTX_PATCHIFY(float, float); }
#undef LTX_PATCHIFY
        LTX_CHECK_LAUNCH();
    }
    LTX_TRY(conv3d(dt, 2, e->conv_in, e->Y.p, e->X.p, d, EPI_BIAS, nullptr, 0, s));
    for (const DownBlockW& b : e->downs) {
        for (const ResnetW& r : b.res) LTX_TRY(resnet_plain(dt, 2, r, b.ch, d, nullptr, 0, e->X.p, e->N.p, e->C.p, s));
        if (!b.has_down) continue;
        LTX_TRY(conv3d(dt, 2, b.down, e->X.p, e->Y.p, d, EPI_S2D, e->X.p, 0, s));      // conv + scatter + grouped-mean residual in the epilogue
        std::swap(e->X, e->Y);
        d.T = (d.T + b.st - 1) / b.st; d.H /= b.sh; d.W /= b.sw;
    }
    for (const ResnetW& r : e->mid) LTX_TRY(resnet_plain(dt, 2, r, e->mid_ch, d, nullptr, 0, e->X.p, e->N.p, e->C.p, s));
    LTX_TRY(ltx_launch_rownorm(norm_silu(e->X.p, e->N.p, d, e->mid_ch, 0, nullptr), dt, s));      // norm_out + SiLU (vae.rs:1455-1459)
    LTX_TRY(conv3d(dt, 2, e->conv_out, e->N.p, e->C.p, d, EPI_BIAS, nullptr, 0, s));
    const int64_t S = (int64_t)d.T * d.H * d.W, n = (int64_t)B * e->nmom * S;
    if (mean_direct) {
        const int L = c.latent_channels;
        if (dt == LTX_DT_BF16) hipLaunchKernelGGL(moments_out_kernel<bf16_t>, enc_grid((int64_t)B * L * S), dim3(256), 0, s, (const bf16_t*)e->C.p, mean_direct, logvar_direct, B, S, e->nmom_pad, L);
        else hipLaunchKernelGGL(moments_out_kernel<float>, enc_grid((int64_t)B * L * S), dim3(256), 0, s, (const float*)e->C.p, mean_direct, logvar_direct, B, S, e->nmom_pad, L);
        LTX_CHECK_LAUNCH();
        return LTX_OK;
    }
    if (dt == LTX_DT_BF16) hipLaunchKernelGGL(moments_kernel<bf16_t>, enc_grid(n), dim3(256), 0, s, (const bf16_t*)e->C.p, moments, B, S, e->nmom_pad, e->nmom);
    else hipLaunchKernelGGL(moments_kernel<float>, enc_grid(n), dim3(256), 0, s, (const float*)e->C.p, moments, B, S, e->nmom_pad, e->nmom);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}

// tiled_encode (vae.rs:2158-2223) of the frames [t0, t0+nt) of `video`: tiles in sample space, blends on the f32 moments;
// result into `out` [BC, oT, oH, oW]
int tiled_encode(ltx_vae_encoder* e, const void* video, int vdt, int B, int F, int H, int W, int t0, int nt,
                 const VaeTilePlan& plan, float* out, int oT, hipStream_t s) {
    const int BC = B * e->nmom;
    auto encode_tile = [&](TileSpan row, TileSpan col, auto& take, Tile* t) -> int {
        const int nh = row.i1 - row.i0, nw = col.i1 - col.i0;
        LTX_TRY(enc_out_dims(e, nt, nh, nw, &t->t, &t->h, &t->w));
        if (t->t != oT) LTX_FAIL(LTX_ERR_ARG, "tiled encode: tile frame count mismatch");
        LTX_TRY(take((size_t)BC * t->t * t->h * t->w * sizeof(float), &t->p));
        return encoder_forward(e, video, vdt, B, F, H, W, t0, nt, row.i0, nh, col.i0, nw, t->p, s);
    };
    return assemble_spatial(plan, encode_tile, BC, out, e->tilebufs, s);
}

// encode_z (vae.rs:2017-2035) -> e->mom [B,L+1,F',H/r,W/r]; *oT/oH/oW = latent dims
int encode_moments(ltx_vae_encoder* e, const void* video, int vdt, int B, int F, int H, int W, const ltx_tiling* tl,
                   const ltx_encode_tiling* et, int* oT, int* oH, int* oW, hipStream_t s,
                   float* mean_direct = nullptr, float* logvar_direct = nullptr, bool* direct_done = nullptr) {
    const int BC = B * e->nmom;
    VaeTilePlan plan;
    LTX_TRY(vae_encode_tile_plan(e->cfg.spatial_compression_ratio, e->cfg.temporal_compression_ratio, tl, et, F, H, W, &plan));
    if (plan.mode == VaeTilePlan::kDirect) {
        LTX_TRY(enc_out_dims(e, F, H, W, oT, oH, oW));
        if (mean_direct) {       // one encoder call: conv_out's rows go straight to the caller's mean / logvar
            if (direct_done) *direct_done = true;
            return encoder_forward(e, video, vdt, B, F, H, W, 0, F, 0, H, 0, W, nullptr, s, mean_direct, logvar_direct);
        }
        LTX_TRY(e->mom.ensure((size_t)BC * *oT * *oH * *oW * sizeof(float)));
        return encoder_forward(e, video, vdt, B, F, H, W, 0, F, 0, H, 0, W, e->mom.as<float>(), s);
    }
    *oT = plan.oT; *oH = plan.oH; *oW = plan.oW;
    LTX_TRY(e->mom.ensure((size_t)BC * plan.oT * plan.oH * plan.oW * sizeof(float)));
    float* out = e->mom.as<float>();
    const int tile_h = plan.rows[0].i1 - plan.rows[0].i0, tile_w = plan.cols[0].i1 - plan.cols[0].i0;      // the whole plane where the windows are not tiled
    if (plan.mode == VaeTilePlan::kSpatial) {
        int t, h, w; LTX_TRY(enc_out_dims(e, F, tile_h, tile_w, &t, &h, &w));
        if (t != plan.oT) LTX_FAIL(LTX_ERR_ARG, "input not divisible by patch sizes (frame count)");
        return tiled_encode(e, video, vdt, B, F, H, W, 0, F, plan, out, plan.oT, s);
    }
    // temporal_tiled_encode (vae.rs:2294-2357)
    TWin prev; int ot = 0;
    for (size_t li = 0; li < plan.windows.size(); ++li) {
        const TileSpan win = plan.windows[li]; const int nf = win.i1 - win.i0;
        int tt, th, tw;
        LTX_TRY(enc_out_dims(e, nf, tile_h, tile_w, &tt, &th, &tw));
        if (!plan.window_tiled && (th != plan.oH || tw != plan.oW)) LTX_FAIL(LTX_ERR_ARG, "temporal tiled encode: tile plane mismatch");
        DevBuf& cur = e->ttiles[li & 1];
        LTX_TRY(cur.ensure((size_t)BC * tt * plan.oH * plan.oW * sizeof(float)));
        if (plan.window_tiled) LTX_TRY(tiled_encode(e, video, vdt, B, F, H, W, win.i0, nf, plan, cur.as<float>(), tt, s));
        else LTX_TRY(encoder_forward(e, video, vdt, B, F, H, W, win.i0, nf, 0, H, 0, W, cur.as<float>(), s));
        int keep = 0;
        LTX_TRY(place_temporal(plan, (int)li, cur.as<float>(), tt, &prev, BC, out, ot, &keep, s));
        ot += std::max(keep, 0);
    }
    if (ot < plan.oT) LTX_FAIL(LTX_ERR_ARG, "temporal tiled encode: the tiles do not cover the latent frames (frame count / tile parameters)");
    return LTX_OK;
}

int check_encode_args(const char* fn, const ltx_vae_encoder* e, const void* video, int B, int F, int H, int W) {
    if (!e) LTX_FAIL(LTX_ERR_ARG, std::string(fn) + ": null handle");
    if (!video) LTX_FAIL(LTX_ERR_ARG, std::string(fn) + ": null tensor");
    if (B < 1 || F < 1 || H < 1 || W < 1) LTX_FAIL(LTX_ERR_ARG, std::string(fn) + ": bad shape");
    return LTX_OK;
}

}  // namespace

extern "C" void ltx_vae_encoder_config_default(ltx_vae_encoder_config* c) {      // vae.rs:68-103
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->in_channels = 3; c->latent_channels = 128; c->n_blocks = 5;
    const int boc[5] = {128, 256, 512, 1024, 2048}, lpb[5] = {4, 6, 6, 2, 2};
    const int dst[4] = {LTX_DOWN_SPATIAL, LTX_DOWN_TEMPORAL, LTX_DOWN_SPATIOTEMPORAL, LTX_DOWN_SPATIOTEMPORAL};
    for (int i = 0; i < 5; ++i) { c->block_out_channels[i] = boc[i]; c->layers_per_block[i] = lpb[i]; }
    for (int i = 0; i < 4; ++i) { c->spatiotemporal_scaling[i] = 1; c->downsample_types[i] = dst[i]; }
    c->patch_size = 4; c->patch_size_t = 1; c->is_causal = 1;
    c->spatial_compression_ratio = 32; c->temporal_compression_ratio = 8;
}
extern "C" int ltx_vae_encoder_config_from_preset(const ltx_preset* p, ltx_vae_encoder_config* c) {
    if (!p || !c) LTX_FAIL(LTX_ERR_ARG, "ltx_vae_encoder_config_from_preset: null argument");
    ltx_vae_encoder_config_default(c);
    int n = 0;
    while (n < 5 && p->vae_encoder_block_out_channels[n] > 0) ++n;
    if (n < 2) LTX_FAIL(LTX_ERR_ARG, "ltx_vae_encoder_config_from_preset: the preset carries no encoder channel list");
    c->n_blocks = n;
    for (int i = 0; i < 5; ++i) { c->block_out_channels[i] = i < n ? p->vae_encoder_block_out_channels[i] : 0; c->layers_per_block[i] = i < n ? p->vae_encoder_layers_per_block[i] : 0; }
    c->latent_channels = p->vae.latent_channels; c->patch_size = p->vae.patch_size; c->patch_size_t = p->vae.patch_size_t;
    c->spatial_compression_ratio = p->vae.spatial_compression_ratio; c->temporal_compression_ratio = p->vae.temporal_compression_ratio;
    return LTX_OK;
}

extern "C" int ltx_vae_encoder_create(const ltx_vae_encoder_config* cfg, const ltx_weight* weights, size_t n_weights,
                                      ltx_dtype model_dtype, int device, ltx_vae_encoder** out) {
    if (!cfg || !weights || !out) LTX_FAIL(LTX_ERR_ARG, "ltx_vae_encoder_create: null argument");
    *out = nullptr;
    if (cfg->n_blocks < 2 || cfg->n_blocks > 5) LTX_FAIL(LTX_ERR_ARG, "encoder n_blocks must be 2..5");
    if (cfg->patch_size < 1 || cfg->patch_size_t != 1) LTX_FAIL(LTX_ERR_UNSUPPORTED, "encoder: only patch_size_t = 1 is supported");
    if (!cfg->is_causal) LTX_FAIL(LTX_ERR_UNSUPPORTED, "encoder: only the causal encoder (is_causal = 1) is supported");
    if (cfg->in_channels < 1 || cfg->latent_channels < 1) LTX_FAIL(LTX_ERR_ARG, "encoder: bad channel counts");
    if ((cfg->in_channels * cfg->patch_size * cfg->patch_size) % 8 != 0) LTX_FAIL(LTX_ERR_UNSUPPORTED, "encoder: patchified channels must be a multiple of 8");
    for (int i = 0; i < cfg->n_blocks; ++i) {
        if (cfg->block_out_channels[i] < 8 || cfg->block_out_channels[i] % 8 != 0) LTX_FAIL(LTX_ERR_UNSUPPORTED, "encoder block_out_channels must be multiples of 8");
        if (cfg->layers_per_block[i] < 0) LTX_FAIL(LTX_ERR_ARG, "encoder layers_per_block must be >= 0");
    }
    for (int i = 0; i < cfg->n_blocks - 1; ++i) {
        if (!cfg->spatiotemporal_scaling[i]) continue;
        if (cfg->downsample_types[i] == LTX_DOWN_CONV)
            LTX_FAIL(LTX_ERR_UNSUPPORTED, "encoder downsample_type 'conv' (strided conv + channel-changing conv_out resnet, vae.rs:888-934) is not implemented: no preset uses it");
        if (cfg->downsample_types[i] < 0 || cfg->downsample_types[i] > LTX_DOWN_SPATIOTEMPORAL) LTX_FAIL(LTX_ERR_ARG, "encoder: bad downsample_type");
    }
    HIP_TRY(hipSetDevice(device));
    ltx_vae_encoder* e = new ltx_vae_encoder();
    e->cfg = *cfg; e->dtype = model_dtype == LTX_BF16 ? LTX_DT_BF16 : LTX_DT_F32; e->device = device;
    const int rc = enc_build(e, weights, n_weights);
    if (rc != LTX_OK) { e->free_all(); delete e; return rc; }
    *out = e;
    return LTX_OK;
}
extern "C" void ltx_vae_encoder_destroy(ltx_vae_encoder* e) {
    if (!e) return;
    (void)hipSetDevice(e->device); (void)hipDeviceSynchronize();
    e->free_all(); delete e;
}
extern "C" int ltx_vae_encoder_get_config(const ltx_vae_encoder* e, ltx_vae_encoder_config* out) {
    if (!e || !out) LTX_FAIL(LTX_ERR_ARG, "ltx_vae_encoder_get_config: null argument");
    *out = e->cfg; return LTX_OK;
}

extern "C" int ltx_vae_encode(ltx_vae_encoder* e, const void* video, ltx_dtype video_dtype, int B, int F, int H, int W,
                              const ltx_tiling* tiling, const ltx_encode_tiling* enc_tiling,
                              float* mean_out, float* logvar_out, ltx_stream stream) {
    LTX_TRY(check_encode_args("ltx_vae_encode", e, video, B, F, H, W));
    if (!mean_out) LTX_FAIL(LTX_ERR_ARG, "ltx_vae_encode: null tensor");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    int oT, oH, oW;
    bool direct = false;
    LTX_TRY(encode_moments(e, video, video_dtype == LTX_BF16 ? LTX_DT_BF16 : LTX_DT_F32, B, F, H, W, tiling, enc_tiling, &oT, &oH, &oW, s,
                           mean_out, logvar_out, &direct));
    if (direct) return LTX_OK;
    const int L = e->cfg.latent_channels; const int64_t S = (int64_t)oT * oH * oW;
    hipLaunchKernelGGL(moments_split_kernel, enc_grid((int64_t)B * L * S), dim3(256), 0, s, e->mom.as<float>(), mean_out, logvar_out, B, L, S);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}

extern "C" int ltx_vae_posterior_sample(const float* mean, const float* logvar, const float* eps, size_t n, float* out, ltx_stream stream) {
    if (!mean || !logvar || !eps || !out) LTX_FAIL(LTX_ERR_ARG, "ltx_vae_posterior_sample: null tensor");
    if (n == 0) return LTX_OK;
    hipLaunchKernelGGL(posterior_sample_kernel, enc_grid((int64_t)n), dim3(256), 0, (hipStream_t)stream, mean, logvar, eps, out, n);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}

extern "C" int ltx_vae_encode_tokens(ltx_vae_encoder* e, const ltx_vae* vae, const void* video, ltx_dtype video_dtype,
                                     int B, int F, int H, int W, const ltx_tiling* tiling, const ltx_encode_tiling* enc_tiling,
                                     const float* eps, float* tokens_out, ltx_stream stream) {
    LTX_TRY(check_encode_args("ltx_vae_encode_tokens", e, video, B, F, H, W));
    if (!vae || !tokens_out) LTX_FAIL(LTX_ERR_ARG, "ltx_vae_encode_tokens: null argument");
    if (vae->cfg.latent_channels != e->cfg.latent_channels) LTX_FAIL(LTX_ERR_ARG, "ltx_vae_encode_tokens: encoder and VAE disagree on latent_channels");
    if (vae->device != e->device) LTX_FAIL(LTX_ERR_ARG, "ltx_vae_encode_tokens: encoder and VAE live on different devices");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    int oT, oH, oW;
    LTX_TRY(encode_moments(e, video, video_dtype == LTX_BF16 ? LTX_DT_BF16 : LTX_DT_F32, B, F, H, W, tiling, enc_tiling, &oT, &oH, &oW, s));
    const int L = e->cfg.latent_channels; const int64_t S = (int64_t)oT * oH * oW;
    hipLaunchKernelGGL(moments_tokens_kernel, enc_grid((int64_t)B * L * S), dim3(256), 0, s, e->mom.as<float>(), eps, vae->mean, vae->std_,
                       vae->cfg.scaling_factor, tokens_out, B, L, S);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}

extern "C" int ltx_vae_encoder_warmup(ltx_vae_encoder* e, int B, int F, int H, int W, const ltx_tiling* tiling,
                                      const ltx_encode_tiling* enc_tiling, ltx_stream stream) {
    if (!e) LTX_FAIL(LTX_ERR_ARG, "ltx_vae_encoder_warmup: null handle");
    if (B < 1 || F < 1 || H < 1 || W < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_vae_encoder_warmup: bad shape");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t nb = (size_t)B * e->cfg.in_channels * F * H * W * ltx_dt_size(e->dtype);
    LTX_TRY(e->scratch.ensure(nb));
    HIP_TRY(hipMemsetAsync(e->scratch.p, 0, nb, s));
    int oT, oH, oW;
    const int rc = encode_moments(e, e->scratch.p, e->dtype, B, F, H, W, tiling, enc_tiling, &oT, &oH, &oW, s);
    HIP_TRY(hipStreamSynchronize(s));
    e->scratch.release();
    return rc;
}

/* LtxVideoDownsampler3d::forward (vae.rs:534-581) alone: x [B,T,H,W,Cin] channels-last -> y [B,(T+st-1)/st,H/sh,W/sw,Cout] */
extern "C" int ltx_op_downsample3d(const void* x, const void* w, const void* bias, int wdtype, void* y,
                                   int B, int T, int H, int W, int Cin, int Cout, int down_type, int dtype, ltx_stream stream) {
    if (!x || !w || !bias || !y) LTX_FAIL(LTX_ERR_ARG, "ltx_op_downsample3d: null tensor");
    if (down_type == LTX_DOWN_CONV) LTX_FAIL(LTX_ERR_UNSUPPORTED, "ltx_op_downsample3d: downsample_type 'conv' is not implemented");
    if (down_type < 0 || down_type > LTX_DOWN_SPATIOTEMPORAL) LTX_FAIL(LTX_ERR_ARG, "ltx_op_downsample3d: bad downsample_type");
    int st, sh, sw; down_stride(down_type, &st, &sh, &sw);
    const int nsub = st * sh * sw;
    if (B < 1 || T < 1 || H < 1 || W < 1 || Cin < 8 || Cin % 8 != 0 || Cout < nsub || Cout % nsub != 0 || (Cout / nsub) % 4 != 0 || (Cin * nsub) % Cout != 0)
        LTX_FAIL(LTX_ERR_ARG, "ltx_op_downsample3d: bad shape");
    if ((T + st - 1) % st != 0 || H % sh != 0 || W % sw != 0) LTX_FAIL(LTX_ERR_ARG, "ltx_op_downsample3d: frames + 1, height and width must divide by the stride");
    ConvW cw; cw.cin = Cin; cw.cout = Cout / nsub; cw.st = st; cw.sh = sh; cw.sw = sw; cw.group = Cin * nsub / Cout;
    return conv3d_unpacked(dtype == LTX_BF16 ? LTX_DT_BF16 : LTX_DT_F32, 2, cw, w, bias, wdtype == LTX_BF16 ? LTX_DT_BF16 : LTX_DT_F32, LTX_PERM_NONE,
                           x, y, Dims{B, T, H, W}, EPI_S2D, x, 0, (hipStream_t)stream);
}
