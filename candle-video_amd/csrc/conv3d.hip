// The model convs (conv3d.h): weight packing and upload, and the calls' way into ltx_launch_gemm.  Reference: vae.rs:415-464 conv,
// :383-412 temporal padding, :1090-1169 depth-to-space upsampler, :469-582 downsampler.
#include <algorithm>
#include "conv3d.h"
#include "options.h"

namespace {

// dst[tap][n'][i] = src[o][i][tap] ; bias'[n'] = bias[o]
__global__ void pack_conv_kernel(const void* src, int sdt, void* dst, int ddt, int O, int I, int ntaps, int mode, int Cf, int nsub) {
    const int64_t n = (int64_t)O * I * ntaps;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
        int i = (int)(idx % I); int64_t r = idx / I; int np = (int)(r % O); int tap = (int)(r / O);
        int o = np;
        if (mode == LTX_PERM_D2S) { int s = np / Cf, c = np - s * Cf; o = c * nsub + s; }                 // n' = s*Cf + c' (nsub = 8: (2,2,2), 4: (1,2,2))
        else if (mode == LTX_PERM_UNPATCH) { int c = np >> 4, oh = (np >> 2) & 3, ow = np & 3; o = (c * 4 + ow) * 4 + oh; }  // n' = (c*4+oh)*4+ow
        float v = sdt == LTX_DT_BF16 ? (float)reinterpret_cast<const bf16_t*>(src)[((int64_t)o * I + i) * ntaps + tap]
                                     : reinterpret_cast<const float*>(src)[((int64_t)o * I + i) * ntaps + tap];
        if (ddt == LTX_DT_BF16) reinterpret_cast<bf16_t*>(dst)[idx] = (bf16_t)v; else reinterpret_cast<float*>(dst)[idx] = v;
    }
}

int d2s_nsub(int mode, int O, int Cf) { return (mode == LTX_PERM_D2S && Cf > 0) ? O / Cf : 8; }

}  // namespace

int ltx_pack_conv(const void* src_dev, int sdt, void* dst, int ddt, int O, int I, int ntaps, int mode, int Cf, hipStream_t s) {
    hipLaunchKernelGGL(pack_conv_kernel, dim3(ltx_grid1d((int64_t)O * I * ntaps, 16384)), dim3(256), 0, s, src_dev, sdt, dst, ddt, O, I, ntaps, mode, Cf,
                       d2s_nsub(mode, O, Cf));
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}

int conv_upload(int dtype, std::vector<void*>& owned, const ltx_weight* w, const ltx_weight* b, int cin, int cout, int mode, int Cf, ConvW* c, ConvPackFn pack_w) {
    const size_t esz = ltx_dt_size(dtype);
    c->cin = cin; c->cout = cout; c->nsub = d2s_nsub(mode, cout, Cf);
    HIP_TRY(hipMalloc(&c->w, (size_t)cout * cin * 27 * esz)); owned.push_back(c->w);
    HIP_TRY(hipMalloc(&c->b, (size_t)cout * esz + 16)); owned.push_back(c->b);
    for (const ltx_weight* t : {w, b}) {
        const void* src = nullptr; void* tmp = nullptr;
        LTX_TRY(ltx_stage_src(t, &src, &tmp));
        const int sdt = t->dtype == LTX_BF16 ? LTX_DT_BF16 : LTX_DT_F32;
        const int rc = t == b ? ltx_pack_conv(src, sdt, c->b, dtype, cout, 1, 1, mode, Cf, 0)
                     : pack_w ? pack_w(src, sdt, c->w, dtype, cout, cin) : ltx_pack_conv(src, sdt, c->w, dtype, cout, cin, 27, mode, Cf, 0);
        const hipError_t e = hipDeviceSynchronize(); if (tmp) (void)hipFree(tmp);
        if (rc != LTX_OK) return rc;
        if (e != hipSuccess) { ltx_set_error(std::string(t == b ? "pack bias: " : "pack conv: ") + hipGetErrorString(e)); return LTX_ERR_HIP; }
    }
    return LTX_OK;
}

GemmArgs conv_args(const ConvW& cw, const Dims& d, int pad_t, int epi, const PostNorm* pn) {
    GemmArgs g;
    g.W = cw.w; g.bias = cw.b;
    g.M = (int)std::min<int64_t>(d.vox(), 2147483647); g.N = cw.cout; g.K = cw.cin; g.ldc = cw.cout; g.ldr = cw.cout;
    g.conv = 1; g.B = d.B; g.T = d.T; g.H = d.H; g.Wd = d.W; g.Cin = cw.cin;
    g.ntaps = 27; g.kh = 3; g.kw = 3;
    g.pad_t = pad_t;                                  // vae.rs:383-412
    if (epi == EPI_D2S) { g.Cf = cw.cout / cw.nsub; g.Cr = cw.cin / cw.nsub; g.To = cw.nsub == 4 ? d.T : 2 * d.T - 1; g.Ho = 2 * d.H; g.Wo = 2 * d.W; g.d2s_sp = cw.nsub == 4; }
    if (epi == EPI_S2D) { g.s2_st = cw.st; g.s2_sh = cw.sh; g.s2_sw = cw.sw; g.s2_group = cw.group; g.To = (d.T + cw.st - 1) / cw.st; g.Ho = d.H / cw.sh; g.Wo = d.W / cw.sw; }
    if (epi == EPI_D2S_G) {                            // guarded in, guarded out (kernels.h): nsub 2 = (2,1,1), 8 = (2,2,2), 4 = (1,2,2)
        const int ft = cw.nsub == 4 ? 1 : 2, fs = cw.nsub == 2 ? 1 : 2;
        g.Cf = cw.cout / cw.nsub; g.s2_st = ft; g.s2_sh = g.s2_sw = fs;
        g.To = ft == 2 ? 2 * d.T - 3 : d.T; g.Ho = fs * d.H; g.Wo = fs * d.W;
    }
    if (pn && pn->on) { g.pn_on = 1; g.pn_eps = pn->eps; g.pn_act = pn->act; g.pn_mod_stride = pn->mod_stride; g.pn_scale = pn->scale; g.pn_shift = pn->shift; }
    return g;
}

// Samples per conv launch: the fast conv kernels address their operands with 32-bit byte offsets (< 2 GiB per operand).
// Samples never interact in a conv, so a batch whose activations pass that limit (the batched leaf tiles of a tiled decode
// at the last stages) runs as sample groups that fit; a single sample beyond the limit goes to the launcher as it is.
int conv_chunk(int dtype, const ConvW& cw, const Dims& d) {
    if (d.B <= 1) return d.B;
    // the large-tile conv kernels address a window around each tile, not the tensor: whole batch in one launch where they apply
    if (d.vox() < 2147483647 && ltx_gemm_route_kind(conv_args(cw, d, 0, EPI_BIAS), dtype, EPI_BIAS) == LTX_ROUTE_PLAN) return d.B;
    const int64_t per = (int64_t)d.T * d.H * d.W;
    const int64_t lim = (2147483648LL - (1 << 20)) / (per * std::max(cw.cin, cw.cout) * (int64_t)ltx_dt_size(dtype));
    const int64_t nb = (lim >= 1 && lim < d.B) ? lim : d.B;
    return (int)std::min(nb, std::max<int64_t>(2147483647LL / per, 1));      // M = samples x voxels is an int
}

// whether conv1 of a resnet can carry norm2 in its epilogue: bf16, the halo-staged kernel with BN == channels
bool fuse_norm2(int dtype, int pad_t, const ConvW& cw, const Dims& d_all, int ch) {
    Dims d = d_all; d.B = conv_chunk(dtype, cw, d_all);
    const LtxOptions& o = ltx_opt();
    if (!o.vae_fuse_norm || !o.gemm_wide_epi || (o.gemm_off & (LTX_FAM_HALO | LTX_FAM_BIG))) return false;
    if (dtype != LTX_DT_BF16 || (ch != 128 && ch != 256) || cw.cout != ch) return false;
    GemmArgs g = conv_args(cw, d, pad_t, EPI_BIAS);
    // the fused epilogue needs the whole channel row in one tile (BN == channels), i.e. a grid of M / 256 blocks: below about
    // one round of the chip the unfused conv on a plan with more, smaller tiles + the stand-alone norm is faster (C1's
    // 256-channel stage, 78 tiles: 168 us fused vs 108 + 13; decode 5.7 -> 5.45 ms, profiles/r5k_c1_vae_fused_norm_ab.jsonl)
    if ((g.M + 255) / 256 < 192 && o.vae_fuse_norm < 2) return false;
    g.pn_on = 1;                                            // ask the route: the fused call must land on the halo tile as wide as the output
    GemmRoute r;
    return ltx_gemm_route(g, dtype, EPI_BIAS, nullptr, false, &r) == LTX_OK && r.kind == LTX_ROUTE_PLAN && r.plan.fam == kPlanHalo;
}

int conv3d(int dtype, int pad_t, const ConvW& cw, const void* x, void* y, const Dims& d, int epi, const void* resid, int post, hipStream_t s, const PostNorm* pn) {
    const size_t esz = ltx_dt_size(dtype);
    const int64_t per = (int64_t)d.T * d.H * d.W;
    if (d.B < 1 || per < 1) LTX_FAIL(LTX_ERR_ARG, "gemm: empty problem");
    if (per > 2147483647LL) LTX_FAIL(LTX_ERR_ARG, "conv3d: more than 2^31 voxels per sample");
    const int nb = conv_chunk(dtype, cw, d);
    const GemmArgs all = conv_args(cw, d, pad_t, epi, pn);
    size_t out_b, res_b = (size_t)per * cw.cin * esz;     // bytes per sample of the output / residual tensor
    if (epi == EPI_D2S || epi == EPI_D2S_G) out_b = (size_t)all.To * all.Ho * all.Wo * all.Cf * esz;
    else if (epi == EPI_S2D) out_b = (size_t)all.To * all.Ho * all.Wo * cw.cout * cw.st * cw.sh * cw.sw * esz;
    else if (epi == EPI_UNPATCH) out_b = (size_t)(cw.cout / 16) * d.T * (4 * d.H) * (4 * d.W) * sizeof(float);
    else res_b = out_b = (size_t)per * cw.cout * esz;
    for (int b0 = 0; b0 < d.B; b0 += nb) {
        GemmArgs g = all;
        g.B = std::min(nb, d.B - b0); g.M = (int)(g.B * per); g.post = post;
        g.A = (const char*)x + (size_t)b0 * per * cw.cin * esz; g.C = (char*)y + (size_t)b0 * out_b;
        g.resid = resid ? (const char*)resid + (size_t)b0 * res_b : nullptr;
        if (g.pn_scale) g.pn_scale += (size_t)b0 * g.pn_mod_stride;
        if (g.pn_shift) g.pn_shift += (size_t)b0 * g.pn_mod_stride;
        LTX_TRY(ltx_launch_gemm(g, dtype, epi, s));
    }
    return LTX_OK;
}

int conv3d_unpacked(int dtype, int pad_t, ConvW cw, const void* w, const void* bias, int wdt, int mode, const void* x, void* y, const Dims& d, int epi,
                    const void* resid, int post, hipStream_t s, const PostNorm* pn) {
    const size_t esz = ltx_dt_size(dtype);
    const int Cf = cw.cout / cw.nsub;
    DevBuf wb, bb;
    int rc = wb.ensure((size_t)cw.cout * cw.cin * 27 * esz); if (rc == LTX_OK) rc = bb.ensure((size_t)cw.cout * esz + 16);
    if (rc == LTX_OK) rc = ltx_pack_conv(w, wdt, wb.p, dtype, cw.cout, cw.cin, 27, mode, Cf, s);
    if (rc == LTX_OK) rc = ltx_pack_conv(bias, wdt, bb.p, dtype, cw.cout, 1, 1, mode, Cf, s);
    cw.w = wb.p; cw.b = bb.p;
    if (rc == LTX_OK) rc = conv3d(dtype, pad_t, cw, x, y, d, epi, resid, post, s, pn);
    const hipError_t e = hipStreamSynchronize(s);
    wb.release(); bb.release();
    if (rc == LTX_OK && e != hipSuccess) { ltx_set_error(hipGetErrorString(e)); rc = LTX_ERR_HIP; }
    return rc;
}
