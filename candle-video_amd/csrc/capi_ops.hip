// Kernel-level C entry points (include/ltxhip_ops.h) — thin argument marshalling only.
#include "conv3d.h"
#include "../../include/ltxhip_ops.h"
#include "../../include/ltxhip_upsampler_st.h"
#include "../../include/ltxhip_stg.h"
#include "../../include/ltxhip_stepcache.h"
#include "../../include/ltxhip_int8.h"

static inline int dtc(int d) { return d == 1 ? LTX_DT_BF16 : LTX_DT_F32; }

extern "C" int ltx_op_linear(const void* x, const void* w, const void* bias, void* y, int M, int N, int K, int dtype, int epi,
                             const void* resid, const float* gate, int rows_per_batch, ltx_stream stream) {
    if (!x || !w || !y) LTX_FAIL(LTX_ERR_ARG, "ltx_op_linear: null tensor");
    if (epi < 0 || epi > 3) LTX_FAIL(LTX_ERR_ARG, "ltx_op_linear: epi must be 0..3");
    if ((epi == 2 || epi == 3) && !resid) LTX_FAIL(LTX_ERR_ARG, "ltx_op_linear: residual epilogue needs resid");
    if (epi == 2 && (!gate || rows_per_batch < 1)) LTX_FAIL(LTX_ERR_ARG, "ltx_op_linear: gated epilogue needs gate");
    GemmArgs g; g.A = x; g.W = w; g.C = y; g.bias = bias; g.resid = resid; g.gate = gate;
    g.M = M; g.N = N; g.K = K; g.lda = K; g.ldc = N; g.ldr = N; g.rows_per_batch = rows_per_batch > 0 ? rows_per_batch : 1; g.gate_stride = N;
    return ltx_launch_gemm(g, dtc(dtype), epi, (hipStream_t)stream);
}

extern "C" int64_t ltx_op_ring_packed_bytes(int N, int K) { return (int64_t)ltx_ring_packed_bytes(N, K); }
extern "C" int ltx_op_ring_pack(const void* w, int N, int K, void* out, ltx_stream stream) { return ltx_pack_ring_weights(w, N, K, out, (hipStream_t)stream); }
extern "C" int ltx_op_linear_packed(const void* x, const void* w, const void* w_packed, const void* bias, void* y, int M, int N, int K, int epi,
                                    const void* resid, const float* gate, int rows_per_batch, ltx_stream stream) {
    if (!x || !w || !w_packed || !y) LTX_FAIL(LTX_ERR_ARG, "ltx_op_linear_packed: null tensor");
    if (epi < 0 || epi > 3) LTX_FAIL(LTX_ERR_ARG, "ltx_op_linear_packed: epi must be 0..3");
    if ((epi == 2 || epi == 3) && !resid) LTX_FAIL(LTX_ERR_ARG, "ltx_op_linear_packed: residual epilogue needs resid");
    if (epi == 2 && (!gate || rows_per_batch < 1)) LTX_FAIL(LTX_ERR_ARG, "ltx_op_linear_packed: gated epilogue needs gate");
    GemmArgs g; g.A = x; g.W = w; g.Wp = w_packed; g.C = y; g.bias = bias; g.resid = resid; g.gate = gate;
    g.M = M; g.N = N; g.K = K; g.lda = K; g.ldc = N; g.ldr = N; g.rows_per_batch = rows_per_batch > 0 ? rows_per_batch : 1; g.gate_stride = N;
    return ltx_launch_gemm(g, LTX_DT_BF16, epi, (hipStream_t)stream);
}

extern "C" int ltx_op_linear_rowsq(const void* x, const void* w, const void* bias, void* y, float* rowsq, int M, int N, int K, int dtype, int epi,
                                   const void* resid, const float* gate, int rows_per_batch, ltx_stream stream) {
    if (!x || !w || !y || !rowsq) LTX_FAIL(LTX_ERR_ARG, "ltx_op_linear_rowsq: null tensor");
    if (epi != 0 && epi != 2 && epi != 3) LTX_FAIL(LTX_ERR_ARG, "ltx_op_linear_rowsq: epi must be 0, 2 or 3");
    if (epi >= 2 && !resid) LTX_FAIL(LTX_ERR_ARG, "ltx_op_linear_rowsq: residual epilogue needs resid");
    if (epi == 2 && (!gate || rows_per_batch < 1)) LTX_FAIL(LTX_ERR_ARG, "ltx_op_linear_rowsq: gated epilogue needs gate");
    GemmArgs g; g.A = x; g.W = w; g.C = y; g.bias = bias; g.resid = resid; g.gate = gate; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldc = N; g.ldr = N;
    g.rows_per_batch = rows_per_batch > 0 ? rows_per_batch : 1; g.gate_stride = N; g.rowsq = rowsq;
    return ltx_launch_gemm(g, dtc(dtype), epi, (hipStream_t)stream);
}
extern "C" int ltx_op_rowsq(const void* x, int64_t rows, int N, int ld, float* rowsq, int dtype, ltx_stream stream) {
    return ltx_launch_rowsq(x, dtc(dtype), rows, N, ld, rowsq, (hipStream_t)stream);
}

// ---- norm fold (GemmArgs::C2 / ::rs_sq, kernels.h): the two epilogue sides and the three small launchers around them
namespace {
GemmArgs fold_out_args(const void* x, const void* w, const void* bias, void* y, void* y2, float* rowsq, const float* scale2, int scale2_stride,
                       int M, int N, int K, const void* resid, const float* gate, int rows_per_batch) {
    GemmArgs g; g.A = x; g.W = w; g.C = y; g.bias = bias; g.resid = resid; g.gate = gate; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldc = N; g.ldr = N;
    g.rows_per_batch = rows_per_batch > 0 ? rows_per_batch : 1; g.gate_stride = N; g.rowsq = rowsq;
    g.C2 = y2; g.scale2 = scale2; g.scale2_stride = scale2_stride;
    return g;
}
GemmArgs fold_in_args(const void* x, const void* w, void* y, const float* rs_sq, int rs_n, int rs_D, float eps, const float* cvec, int cvec_stride,
                      int M, int N, int K, int rows_per_batch) {
    GemmArgs g; g.A = x; g.W = w; g.C = y; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldc = N;
    g.rows_per_batch = rows_per_batch > 0 ? rows_per_batch : 1;
    g.rs_sq = rs_sq; g.rs_n = rs_n; g.rs_D = rs_D; g.rs_eps = eps; g.cvec = cvec; g.cvec_stride = cvec_stride;
    return g;
}
}  // namespace

extern "C" int ltx_op_linear_fold_out(const void* x, const void* w, const void* bias, void* y, void* y2, float* rowsq, const float* scale2, int scale2_stride,
                                      int M, int N, int K, int epi, const void* resid, const float* gate, int rows_per_batch, ltx_stream stream) {
    if (!x || !w || !y || !y2 || !rowsq || !scale2 || !resid) LTX_FAIL(LTX_ERR_ARG, "ltx_op_linear_fold_out: null tensor");
    if (epi != 2 && epi != 3) LTX_FAIL(LTX_ERR_ARG, "ltx_op_linear_fold_out: epi must be 2 or 3 (the second output rides on the residual epilogues)");
    if (epi == 2 && !gate) LTX_FAIL(LTX_ERR_ARG, "ltx_op_linear_fold_out: gated epilogue needs gate");
    const GemmArgs g = fold_out_args(x, w, bias, y, y2, rowsq, scale2, scale2_stride, M, N, K, resid, gate, rows_per_batch);
    if (!ltx_gemm_fold_ok(g, epi)) LTX_FAIL(LTX_ERR_ARG, "ltx_op_linear_fold_out: not a call the norm fold serves (ltx_op_linear_fold_ok)");
    return ltx_launch_gemm(g, LTX_DT_BF16, epi, (hipStream_t)stream);
}

extern "C" int ltx_op_linear_fold_in(const void* x, const void* w, void* y, const float* rs_sq, int rs_n, int rs_D, float eps, const float* cvec, int cvec_stride,
                                     int M, int N, int K, int epi, int rows_per_batch, ltx_stream stream) {
    if (!x || !w || !y || !rs_sq || !cvec) LTX_FAIL(LTX_ERR_ARG, "ltx_op_linear_fold_in: null tensor");
    if (epi != 0 && epi != 1) LTX_FAIL(LTX_ERR_ARG, "ltx_op_linear_fold_in: epi must be 0 or 1 (the row scale rides on the bias / GELU epilogues)");
    const GemmArgs g = fold_in_args(x, w, y, rs_sq, rs_n, rs_D, eps, cvec, cvec_stride, M, N, K, rows_per_batch);
    if (!ltx_gemm_fold_ok(g, epi)) LTX_FAIL(LTX_ERR_ARG, "ltx_op_linear_fold_in: not a call the norm fold serves (ltx_op_linear_fold_ok)");
    return ltx_launch_gemm(g, LTX_DT_BF16, epi, (hipStream_t)stream);
}

extern "C" int ltx_op_linear_fold_ok(int M, int N, int K, int epi, int consumer, int rs_n, int vec_stride, int rows_per_batch) {
    if (M < 1 || N < 1 || K < 1) return 0;
    // (aligned non-null pointers: a fit test, nothing is launched)
    void* const p = reinterpret_cast<void*>((uintptr_t)4096); float* const f = reinterpret_cast<float*>(p);
    if (consumer) return ltx_gemm_fold_ok(fold_in_args(p, p, p, f, rs_n, K, 1e-6f, f, vec_stride, M, N, K, rows_per_batch), epi) ? 1 : 0;
    return ltx_gemm_fold_ok(fold_out_args(p, p, p, p, p, f, f, vec_stride, M, N, K, p, f, rows_per_batch), epi) ? 1 : 0;
}

extern "C" int ltx_op_shift_gemv(const void* w, const void* bias, const float* shift, int shift_stride, int B, int N, int K, float* cvec, int cvec_stride, ltx_stream stream) {
    return ltx_launch_shift_gemv(w, bias, shift, shift_stride, B, N, K, cvec, cvec_stride, (hipStream_t)stream);
}
extern "C" int ltx_op_mod_scale(const void* h, const float* scale, int scale_stride, void* y, int B, int64_t rows_per_batch, int D, int dtype, ltx_stream stream) {
    if (!h || !scale || !y || B < 1 || rows_per_batch < 1 || D < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_op_mod_scale: bad argument");
    return ltx_launch_mod_scale(h, scale, scale_stride, y, B, rows_per_batch, D, dtc(dtype), (hipStream_t)stream);
}
// the copy of the STG attention modes (ltxhip_stg.h): whole batch rows of src into dst, one launch
extern "C" int ltx_op_stg_fill(void* dst, int ldd, const void* src, int lds, const unsigned char* rows, int B, int S, int D, ltx_dtype dtype, ltx_stream stream) {
    if (!dst || !src || !rows || B < 1 || S < 1 || D < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_op_stg_fill: bad argument");
    return ltx_launch_stg_fill(dst, ldd, src, lds, rows, B, S, D, dtc(dtype), (hipStream_t)stream);
}
extern "C" int ltx_op_scale_cols(const void* w, const float* scale, void* out, int64_t N, int K, int dtype, ltx_stream stream) {
    if (!w || !scale || !out || N < 1 || K < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_op_scale_cols: bad argument");
    return ltx_launch_scale_cols(w, scale, out, N, K, dtc(dtype), (hipStream_t)stream);
}

extern "C" int ltx_op_linear_segmented(const void* x, const void* w, const void* bias, void* y, int M, int N, int K, int seg_width,
                                       int dtype, ltx_stream stream) {
    if (!x || !w || !y) LTX_FAIL(LTX_ERR_ARG, "ltx_op_linear_segmented: null tensor");
    if (seg_width <= 0 || (seg_width & (seg_width - 1)) || N % seg_width) LTX_FAIL(LTX_ERR_ARG, "ltx_op_linear_segmented: seg_width must be a power of two dividing N");
    GemmArgs g; g.A = x; g.W = w; g.C = y; g.bias = bias;
    g.M = M; g.N = N; g.K = K; g.lda = K; g.ldc = seg_width;
    g.c_seg_shift = __builtin_ctz((unsigned)seg_width); g.c_seg_stride = (int64_t)M * seg_width;
    return ltx_launch_gemm(g, dtc(dtype), EPI_BIAS, (hipStream_t)stream);
}

extern "C" int ltx_op_rownorm(const void* x, void* y, int64_t rows, int D, int kind, float eps, const void* weight,
                              const float* scale, const float* shift, int64_t rows_per_batch, int mod_stride, int act,
                              int dtype, ltx_stream stream) {
    if (!x || !y) LTX_FAIL(LTX_ERR_ARG, "ltx_op_rownorm: null tensor");
    RowNormArgs a; a.x = x; a.y = y; a.rows = rows; a.D = D; a.ldx = D; a.ldy = D; a.kind = kind; a.eps = eps; a.weight = weight;
    a.scale = scale; a.shift = shift; a.rows_per_batch = rows_per_batch > 0 ? rows_per_batch : 1; a.mod_stride = mod_stride; a.act = act;
    return ltx_launch_rownorm(a, dtc(dtype), (hipStream_t)stream);
}

extern "C" int ltx_attention_fallback_counts(unsigned long long counts[2], int reset) {
    if (!counts) LTX_FAIL(LTX_ERR_ARG, "ltx_attention_fallback_counts: null output");
    LTX_TRY(ltx_q64_fallback_read(&counts[0], reset));
    return ltx_q128_fallback_read(&counts[1], reset);
}

extern "C" int ltx_op_linear_split_factor(int M, int N, int K) {
    GemmArgs g; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldc = N;
    return ltx_gemm_split_factor(g);
}
extern "C" int ltx_op_linear_deferred(const void* x, const void* w, float* parts, int M, int N, int K, ltx_stream stream) {
    if (!x || !w || !parts) LTX_FAIL(LTX_ERR_ARG, "ltx_op_linear_deferred: null tensor");
    GemmArgs g; g.A = x; g.W = w; g.C = parts; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldc = N; g.defer_parts = parts;
    if (!ltx_gemm_defer_ok(g, EPI_GATE_RESID)) LTX_FAIL(LTX_ERR_ARG, "ltx_op_linear_deferred: bf16 linear layers of at most 512 rows, N % 8 == 0, K % 8 == 0");
    return ltx_launch_gemm(g, LTX_DT_BF16, EPI_BIAS, (hipStream_t)stream);
}
extern "C" int ltx_op_rownorm_deferred(const float* parts, int nparts, const void* bias, const void* resid, const float* gate, int gate_stride, void* h_out,
                                       void* y, int64_t rows, int D, int kind, float eps, const float* scale, const float* shift, int64_t rows_per_batch,
                                       int mod_stride, int dtype, ltx_stream stream) {
    if (!parts || !resid || !h_out || !y) LTX_FAIL(LTX_ERR_ARG, "ltx_op_rownorm_deferred: null tensor");
    RowNormArgs a; a.x = resid; a.y = y; a.rows = rows; a.D = D; a.ldx = D; a.ldy = D; a.kind = kind; a.eps = eps;
    a.scale = scale; a.shift = shift; a.rows_per_batch = rows_per_batch > 0 ? rows_per_batch : 1; a.mod_stride = mod_stride;
    a.parts = parts; a.nparts = nparts; a.part_stride = rows * D; a.d_bias = bias; a.d_gate = gate; a.d_gate_stride = gate_stride; a.x_out = h_out;
    return ltx_launch_rownorm(a, dtc(dtype), (hipStream_t)stream);
}

extern "C" int ltx_op_rownorm_presum(const void* x, void* y, int64_t rows, int D, float eps, const void* weight,
                                     const float* scale, const float* shift, int64_t rows_per_batch, int mod_stride, int act,
                                     const float* presum, int presum_n, int dtype, ltx_stream stream) {
    if (!x || !y || !presum) LTX_FAIL(LTX_ERR_ARG, "ltx_op_rownorm_presum: null tensor");
    RowNormArgs a; a.x = x; a.y = y; a.rows = rows; a.D = D; a.ldx = D; a.ldy = D; a.kind = 0; a.eps = eps; a.weight = weight;
    a.scale = scale; a.shift = shift; a.rows_per_batch = rows_per_batch > 0 ? rows_per_batch : 1; a.mod_stride = mod_stride; a.act = act;
    a.presum = presum; a.presum_n = presum_n;
    return ltx_launch_rownorm(a, dtc(dtype), (hipStream_t)stream);
}

extern "C" int ltx_op_timestep_embedding(const float* timesteps_host, int n, int vae_flavour, float multiplier, int dtype, void* out, ltx_stream stream) {
    if (!timesteps_host || !out) LTX_FAIL(LTX_ERR_ARG, "ltx_op_timestep_embedding: null argument");
    if (n < 1 || n > 8) LTX_FAIL(LTX_ERR_ARG, "ltx_op_timestep_embedding: batch must be 1..8");
    float tab[128]; ltx_sinusoid_table(vae_flavour, tab);
    float* dtab = nullptr;
    HIP_TRY(hipMalloc((void**)&dtab, sizeof(tab)));
    int rc = LTX_OK;
    if (hipMemcpy(dtab, tab, sizeof(tab), hipMemcpyHostToDevice) != hipSuccess) rc = LTX_ERR_HIP;
    if (rc == LTX_OK) {
        TimeVec tv; tv.n = n;
        for (int i = 0; i < n; ++i) tv.t[i] = timesteps_host[i];
        rc = ltx_launch_sinusoid(out, dtc(dtype), tv, dtab, 128, dtc(dtype) == LTX_DT_BF16, multiplier, (hipStream_t)stream);
        if (rc == LTX_OK && hipStreamSynchronize((hipStream_t)stream) != hipSuccess) rc = LTX_ERR_HIP;
    }
    (void)hipFree(dtab);
    return rc;
}

extern "C" int ltx_op_qknorm_rope(void* x, int64_t rows, int D, int ld, const void* weight, float eps,
                                  const float* cos, const float* sin, int dtype, ltx_stream stream) {
    if (!x || !weight) LTX_FAIL(LTX_ERR_ARG, "ltx_op_qknorm_rope: null tensor");
    QkNormRopeArgs a; a.x = x; a.rows = rows; a.D = D; a.ld = ld; a.nseg = 1; a.w0 = weight; a.eps = eps; a.cos = cos; a.sin = sin;
    return ltx_launch_qknorm_rope(a, dtc(dtype), (hipStream_t)stream);
}

extern "C" int ltx_op_qknorm_rope_segs(void* x, int64_t rows, int D, int ld, int nseg, int64_t seg_stride, const void* w0, const void* w1, const void* w0b,
                                       float eps, const float* cos, const float* sin, float out_scale0, int dtype, ltx_stream stream) {
    if (!x || !w0) LTX_FAIL(LTX_ERR_ARG, "ltx_op_qknorm_rope_segs: null tensor");
    if ((cos == nullptr) != (sin == nullptr) || seg_stride < 0) LTX_FAIL(LTX_ERR_ARG, "ltx_op_qknorm_rope_segs: cos and sin go together; seg_stride >= 0");
    QkNormRopeArgs a; a.x = x; a.rows = rows; a.D = D; a.ld = ld; a.nseg = nseg; a.seg_stride = seg_stride; a.w0 = w0; a.w1 = w1; a.w0b = w0b;
    a.eps = eps; a.cos = cos; a.sin = sin; a.out_scale0 = out_scale0;
    return ltx_launch_qknorm_rope(a, dtc(dtype), (hipStream_t)stream);
}

extern "C" int ltx_op_norm_route(int64_t rows, int D, int dtype, int kind, int flags, int act, int64_t rows_per_batch, int presum_n, int nparts, char* name, int cap) {
    if (!name || cap < 1 || rows < 1 || D < 1 || presum_n < 0 || nparts < 0 || (flags & ~7)) LTX_FAIL(LTX_ERR_ARG, "ltx_op_norm_route: bad argument");
    NormRouteArgs r;
    r.dtype = dtc(dtype); r.rows = rows; r.D = D; r.kind = kind; r.act = act; r.rows_per_batch = rows_per_batch > 0 ? rows_per_batch : 1;
    r.scale = (flags & LTX_NORM_SCALE) != 0; r.shift = (flags & LTX_NORM_SHIFT) != 0; r.weight = (flags & LTX_NORM_WEIGHT) != 0;
    r.presum = presum_n != 0; r.presum_n = presum_n; r.parts = nparts != 0; r.nparts = nparts;
    snprintf(name, (size_t)cap, "%s", ltx_rownorm_route_name(ltx_rownorm_route(r).route));
    return LTX_OK;
}
extern "C" int ltx_op_qknorm_route(int64_t rows, int D, int dtype, char* name, int cap) {
    if (!name || cap < 1 || rows < 1 || D < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_op_qknorm_route: bad argument");
    snprintf(name, (size_t)cap, "%s", ltx_qknorm_route_name(ltx_qknorm_route(dtc(dtype), rows, D, nullptr)));
    return LTX_OK;
}

extern "C" int ltx_op_rope_table(float* cos, float* sin, const float* coords, int B, int F, int H, int W, int D,
                                 const float* rope_scale_host, ltx_stream stream) {
    if (!cos || !sin) LTX_FAIL(LTX_ERR_ARG, "ltx_op_rope_table: null tensor");
    int steps = D / 6; if (steps < 1) steps = 1;
    std::vector<float> fr(steps);
    const float theta_ln = (float)std::log(10000.0);
    for (int i = 0; i < steps; ++i) {
        float lin = steps <= 1 ? 0.0f : (float)i * (float)(1.0 / (double)(steps - 1));
        fr[i] = (float)std::exp((double)(lin * theta_ln)) * (float)(M_PI / 2.0);
    }
    float* dfr = nullptr;
    HIP_TRY(hipMalloc((void**)&dfr, sizeof(float) * steps));
    HIP_TRY(hipMemcpy(dfr, fr.data(), sizeof(float) * steps, hipMemcpyHostToDevice));
    RopeTableArgs r; r.cos = cos; r.sin = sin; r.freqs = dfr; r.B = B; r.D = D;
    if (coords) { r.use_coords = 1; r.coords = coords; r.F = 1; r.H = 1; r.W = F * H * W;
                  r.gscale[0] = (float)(1.0 / 20.0); r.gscale[1] = (float)(1.0 / 2048.0); r.gscale[2] = (float)(1.0 / 2048.0); }
    else { r.F = F; r.H = H; r.W = W;
           if (rope_scale_host) { r.gscale[0] = (float)((double)rope_scale_host[0] / 20.0); r.gscale[1] = (float)((double)rope_scale_host[1] / 2048.0); r.gscale[2] = (float)((double)rope_scale_host[2] / 2048.0); } }
    int rc = ltx_launch_rope_table(r, (hipStream_t)stream);
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    (void)hipFree(dfr);
    if (rc != LTX_OK) return rc;
    if (e != hipSuccess) { ltx_set_error(hipGetErrorString(e)); return LTX_ERR_HIP; }
    return LTX_OK;
}

extern "C" int ltx_op_attention(const void* q, const void* k, const void* v, void* o, int B, int Sq, int Sk, int heads, int hd,
                                int ldq, int ldk, int ldv, int ldo, float scale, const float* key_bias, int dtype, ltx_stream stream) {
    if (!q || !k || !v || !o) LTX_FAIL(LTX_ERR_ARG, "ltx_op_attention: null tensor");
    AttnArgs a; a.q = q; a.k = k; a.v = v; a.o = o; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
    a.B = B; a.Sq = Sq; a.Sk = Sk; a.heads = heads; a.hd = hd; a.scale = scale; a.bias = key_bias;
    return ltx_launch_attention(a, dtc(dtype), (hipStream_t)stream);
}

extern "C" int ltx_op_attention_rowsq(const void* q, const void* k, const void* v, void* o, int B, int Sq, int Sk, int heads, int hd,
                                      int ldq, int ldk, int ldv, int ldo, float scale, const float* key_bias,
                                      const float* q_rowsq, int q_rowsq_n, int q_rowsq_D, float q_rowsq_eps, ltx_stream stream) {
    if (!q || !k || !v || !o || !q_rowsq) LTX_FAIL(LTX_ERR_ARG, "ltx_op_attention_rowsq: null tensor");
    AttnArgs a; a.q = q; a.k = k; a.v = v; a.o = o; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
    a.B = B; a.Sq = Sq; a.Sk = Sk; a.heads = heads; a.hd = hd; a.scale = scale; a.bias = key_bias;
    a.q_rowsq = q_rowsq; a.q_rowsq_n = q_rowsq_n; a.q_rowsq_D = q_rowsq_D; a.q_rowsq_eps = q_rowsq_eps;
    return ltx_launch_attention(a, LTX_DT_BF16, (hipStream_t)stream);
}

extern "C" int ltx_op_attention_compact(const void* q, const void* k, const void* v, void* o, int B, int Sq, int Sk, int heads, int hd,
                                        int ldq, int ldk, int ldv, int ldo, float scale, const float* key_bias,
                                        const float* q_rowsq, int q_rowsq_n, int q_rowsq_D, float q_rowsq_eps, int* counts_out, ltx_stream stream) {
    if (!q || !k || !v || !o || !key_bias) LTX_FAIL(LTX_ERR_ARG, "ltx_op_attention_compact: null tensor");
    if (!ltx_attention_cross64_ok(hd, Sk) || B < 1 || ldk != heads * hd || ldv != heads * hd) LTX_FAIL(LTX_ERR_ARG, "ltx_op_attention_compact: bf16, head_dim 64, at most 128 keys, dense k / v rows");
    hipStream_t s = (hipStream_t)stream;
    const int D = heads * hd;
    void *kc = nullptr, *vc = nullptr, *bc = nullptr, *idx = nullptr, *cnt = nullptr;
    auto free_all = [&]() { for (void* p : {kc, vc, bc, idx, cnt}) if (p) (void)hipFree(p); };
    const size_t rows = (size_t)B * Sk;
    if (hipMalloc(&kc, rows * D * 2) != hipSuccess || hipMalloc(&vc, rows * D * 2) != hipSuccess || hipMalloc(&bc, rows * 4) != hipSuccess ||
        hipMalloc(&idx, rows * 4) != hipSuccess || hipMalloc(&cnt, (size_t)B * 4) != hipSuccess) { free_all(); LTX_FAIL(LTX_ERR_HIP, "hipMalloc"); }
    int rc = ltx_launch_key_compact(key_bias, B, Sk, (int*)idx, (int*)cnt, (float*)bc, s);
    if (rc == LTX_OK) rc = ltx_launch_gather_rows(k, kc, (const int*)idx, (const int*)cnt, 1, B, Sk, D * 2, s);
    if (rc == LTX_OK) rc = ltx_launch_gather_rows(v, vc, (const int*)idx, (const int*)cnt, 1, B, Sk, D * 2, s);
    if (rc == LTX_OK) {
        AttnArgs a; a.q = q; a.k = kc; a.v = vc; a.o = o; a.ldq = ldq; a.ldk = D; a.ldv = D; a.ldo = ldo;
        a.B = B; a.Sq = Sq; a.Sk = Sk; a.heads = heads; a.hd = hd; a.scale = scale; a.bias = (const float*)bc; a.k_count = (const int*)cnt;
        if (q_rowsq) { a.q_rowsq = q_rowsq; a.q_rowsq_n = q_rowsq_n; a.q_rowsq_D = q_rowsq_D; a.q_rowsq_eps = q_rowsq_eps; }
        rc = ltx_launch_attention(a, LTX_DT_BF16, s);
    }
    if (rc == LTX_OK && counts_out && hipMemcpyAsync(counts_out, cnt, (size_t)B * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) rc = LTX_ERR_HIP;
    const hipError_t e = hipStreamSynchronize(s);
    free_all();
    if (rc != LTX_OK) return rc;
    if (e != hipSuccess) { ltx_set_error(hipGetErrorString(e)); return LTX_ERR_HIP; }
    return LTX_OK;
}

// ---- attn2.to_out folded into the text context (xattn_fold.hip): the decision, KP, and the two kernels on their own ----
extern "C" int ltx_op_xattn_fold_route(int dtype, int head_dim, int heads, int D, int KP, int B, int compact, int* fold) {
    if (!fold) LTX_FAIL(LTX_ERR_ARG, "ltx_op_xattn_fold_route: null result");
    *fold = ltx_xattn_fold_route(dtc(dtype), head_dim, heads, D, KP, B, compact != 0) ? 1 : 0;
    return LTX_OK;
}
extern "C" int ltx_op_xattn_fold_kp(const int* counts_host, int B, int* KP) {
    if (!counts_host || !KP || B < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_op_xattn_fold_kp: bad argument");
    *KP = ltx_xattn_fold_kp(counts_host, B);
    return LTX_OK;
}
extern "C" int ltx_op_xattn_fold_build(const void* v, const float* key_bias, const void* wo, int B, int K, int heads, int KP, void* vo, int* counts_out, ltx_stream stream) {
    if (!v || !key_bias || !wo || !vo || B < 1 || K < 1 || heads < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_op_xattn_fold_build: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int D = heads * 64;
    void *vc = nullptr, *bc = nullptr, *idx = nullptr, *cnt = nullptr, *tab = nullptr;
    auto free_all = [&]() { for (void* p : {vc, bc, idx, cnt, tab}) if (p) (void)hipFree(p); };
    const size_t rows = (size_t)B * K;
    if (hipMalloc(&vc, rows * D * 2) != hipSuccess || hipMalloc(&bc, rows * 4) != hipSuccess || hipMalloc(&idx, rows * 4) != hipSuccess ||
        hipMalloc(&cnt, (size_t)B * 4) != hipSuccess || hipMalloc(&tab, sizeof(XFoldPtrs)) != hipSuccess) { free_all(); LTX_FAIL(LTX_ERR_HIP, "hipMalloc"); }
    const XFoldPtrs host{wo, vc};
    int rc = ltx_launch_key_compact(key_bias, B, K, (int*)idx, (int*)cnt, (float*)bc, s);
    if (rc == LTX_OK) rc = ltx_launch_gather_rows(v, vc, (const int*)idx, (const int*)cnt, 1, B, K, D * 2, s);
    if (rc == LTX_OK && hipMemcpyAsync(tab, &host, sizeof(host), hipMemcpyHostToDevice, s) != hipSuccess) rc = LTX_ERR_HIP;
    if (rc == LTX_OK) {
        XFoldArgs a; a.tab = (const XFoldPtrs*)tab; a.vo = vo; a.L = 1; a.B = B; a.K = K; a.ldv = D; a.D = D; a.H = heads; a.KP = KP;
        rc = ltx_launch_xattn_fold(a, s);
    }
    if (rc == LTX_OK && counts_out && hipMemcpyAsync(counts_out, cnt, (size_t)B * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) rc = LTX_ERR_HIP;
    const hipError_t e = hipStreamSynchronize(s);
    free_all();
    if (rc != LTX_OK) return rc;
    if (e != hipSuccess) { ltx_set_error(hipGetErrorString(e)); return LTX_ERR_HIP; }
    return LTX_OK;
}
extern "C" int ltx_op_attention_probs(const void* q, const void* k, void* p_out, int B, int Sq, int Sk, int heads, int KP, float scale, const float* key_bias,
                                      const float* q_rowsq, int q_rowsq_n, float q_rowsq_eps, int* counts_out, ltx_stream stream) {
    if (!q || !k || !p_out || !key_bias || B < 1 || heads < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_op_attention_probs: bad argument");
    if (!ltx_attention_cross64_ok(64, Sk)) LTX_FAIL(LTX_ERR_ARG, "ltx_op_attention_probs: at most 128 keys, the short-key-set kernel enabled");
    hipStream_t s = (hipStream_t)stream;
    const int D = heads * 64;
    void *kc = nullptr, *bc = nullptr, *idx = nullptr, *cnt = nullptr;
    auto free_all = [&]() { for (void* p : {kc, bc, idx, cnt}) if (p) (void)hipFree(p); };
    const size_t rows = (size_t)B * Sk;
    if (hipMalloc(&kc, rows * D * 2) != hipSuccess || hipMalloc(&bc, rows * 4) != hipSuccess || hipMalloc(&idx, rows * 4) != hipSuccess ||
        hipMalloc(&cnt, (size_t)B * 4) != hipSuccess) { free_all(); LTX_FAIL(LTX_ERR_HIP, "hipMalloc"); }
    int rc = ltx_launch_key_compact(key_bias, B, Sk, (int*)idx, (int*)cnt, (float*)bc, s);
    if (rc == LTX_OK) rc = ltx_launch_gather_rows(k, kc, (const int*)idx, (const int*)cnt, 1, B, Sk, D * 2, s);
    if (rc == LTX_OK) {
        AttnArgs a; a.q = q; a.k = kc; a.v = kc; a.ldq = D; a.ldk = D; a.ldv = D; a.ldo = D;
        a.B = B; a.Sq = Sq; a.Sk = Sk; a.heads = heads; a.hd = 64; a.scale = scale; a.bias = (const float*)bc; a.k_count = (const int*)cnt;
        a.p_out = p_out; a.ldp = heads * KP;
        if (q_rowsq) { a.q_rowsq = q_rowsq; a.q_rowsq_n = q_rowsq_n; a.q_rowsq_D = D; a.q_rowsq_eps = q_rowsq_eps; }
        rc = ltx_launch_attention(a, LTX_DT_BF16, s);
    }
    if (rc == LTX_OK && counts_out && hipMemcpyAsync(counts_out, cnt, (size_t)B * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) rc = LTX_ERR_HIP;
    const hipError_t e = hipStreamSynchronize(s);
    free_all();
    if (rc != LTX_OK) return rc;
    if (e != hipSuccess) { ltx_set_error(hipGetErrorString(e)); return LTX_ERR_HIP; }
    return LTX_OK;
}

extern "C" int ltx_op_attention_prescaled(const void* q, const void* k, const void* v, void* o, int B, int Sq, int Sk, int heads, int hd,
                                          int ldq, int ldk, int ldv, int ldo, ltx_stream stream) {
    if (!q || !k || !v || !o) LTX_FAIL(LTX_ERR_ARG, "ltx_op_attention_prescaled: null tensor");
    AttnArgs a; a.q = q; a.k = k; a.v = v; a.o = o; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
    a.B = B; a.Sq = Sq; a.Sk = Sk; a.heads = heads; a.hd = hd; a.scale = 1.0f; a.q_prescaled = 1;
    return ltx_launch_attention(a, LTX_DT_BF16, (hipStream_t)stream);
}

namespace {
// (depth-to-space: ConvW's default nsub = 8, the (2, 2, 2) upsampler)
int conv_common(const void* x, const void* w, const void* bias, int wdtype, void* y, const void* resid,
                int B, int T, int H, int W, int Cin, int Cout, int causal, int dtype, int epi, int mode, int post, hipStream_t s, const PostNorm* pn = nullptr) {
    if (!x || !w || !bias || !y) LTX_FAIL(LTX_ERR_ARG, "conv: null tensor");
    const int dt = dtc(dtype), pad_t = causal ? 2 : 1;
    const Dims d{B, T, H, W};
    ConvW cw; cw.cin = Cin; cw.cout = Cout;
    if (pn) {
        // a fused call that the dispatch does not serve is refused before anything is allocated or packed: the route and the
        // refusal that ltx_launch_gemm repeats below (the packed weights and bias are hipMalloc'ed: aligned like w and bias)
        if (B < 1 || T < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) LTX_FAIL(LTX_ERR_ARG, "conv: empty problem");
        ConvW raw = cw; raw.w = const_cast<void*>(w); raw.b = const_cast<void*>(bias);
        GemmArgs g = conv_args(raw, d, pad_t, epi, pn); g.A = x; g.C = y;
        GemmRoute r;
        LTX_TRY(ltx_gemm_route(g, dt, epi, nullptr, false, &r));
        if (const char* why = ltx_gemm_route_refusal(g, r)) LTX_FAIL(LTX_ERR_ARG, why);
    }
    return conv3d_unpacked(dt, pad_t, cw, w, bias, dtc(wdtype), mode, x, y, d, epi, resid, post, s, pn);
}
}  // namespace

extern "C" int ltx_op_conv3d(const void* x, const void* w, const void* bias, int wdtype, void* y, const void* resid,
                             int B, int T, int H, int W, int Cin, int Cout, int causal, int dtype, ltx_stream stream) {
    return conv_common(x, w, bias, wdtype, y, resid, B, T, H, W, Cin, Cout, causal, dtype, resid ? EPI_RESID : EPI_BIAS, LTX_PERM_NONE, 0, (hipStream_t)stream);
}
extern "C" int ltx_op_conv3d_norm(const void* x, const void* w, const void* bias, int wdtype, void* y, const float* scale, const float* shift, int mod_stride,
                                  float eps, int act, int B, int T, int H, int W, int Cin, int Cout, int causal, int dtype, ltx_stream stream) {
    if ((scale == nullptr) != (shift == nullptr)) LTX_FAIL(LTX_ERR_ARG, "ltx_op_conv3d_norm: scale and shift come together (both null: no modulation)");
    if (scale && mod_stride < Cout) LTX_FAIL(LTX_ERR_ARG, "ltx_op_conv3d_norm: mod_stride is the row stride of scale / shift, at least Cout");
    if (act != 0 && act != 1) LTX_FAIL(LTX_ERR_ARG, "ltx_op_conv3d_norm: act must be 0 (none) or 1 (SiLU)");
    if (!(eps >= 0.f)) LTX_FAIL(LTX_ERR_ARG, "ltx_op_conv3d_norm: eps must not be negative");
    PostNorm pn; pn.on = 1; pn.eps = eps; pn.act = act; pn.scale = scale; pn.shift = shift; pn.mod_stride = scale ? mod_stride : 0;
    return conv_common(x, w, bias, wdtype, y, nullptr, B, T, H, W, Cin, Cout, causal, dtype, EPI_BIAS, LTX_PERM_NONE, 0, (hipStream_t)stream, &pn);
}
extern "C" int ltx_op_upsample3d(const void* x, const void* w, const void* bias, int wdtype, void* y,
                                 int B, int T, int H, int W, int Cin, int Cout, int causal, int residual, int dtype, ltx_stream stream) {
    if (Cout % 8 != 0 || Cin % 8 != 0) LTX_FAIL(LTX_ERR_ARG, "upsample3d: channels must be multiples of 8");
    return conv_common(x, w, bias, wdtype, y, residual ? x : nullptr, B, T, H, W, Cin, Cout, causal, dtype, EPI_D2S, LTX_PERM_D2S, 0, (hipStream_t)stream);
}
// the latent upsampler's shuffle stage (ltxhip_upsampler_st.h): guarded in, guarded out, the placement in the conv's epilogue
extern "C" int ltx_op_conv3d_shuffle(const void* x, const void* w, const void* bias, int wdtype, void* y,
                                     int B, int F, int H, int W, int Cin, int O, int st, int ss, int dtype, ltx_stream stream) {
    if (!x || !w || !bias || !y) LTX_FAIL(LTX_ERR_ARG, "ltx_op_conv3d_shuffle: null tensor");
    if (!((st == 2 && ss == 1) || (st == 2 && ss == 2) || (st == 1 && ss == 2))) LTX_FAIL(LTX_ERR_ARG, "ltx_op_conv3d_shuffle: the factors (st, ss) are (2,1), (2,2) or (1,2)");
    if ((dtype != 0 && dtype != 1) || (wdtype != 0 && wdtype != 1)) LTX_FAIL(LTX_ERR_ARG, "ltx_op_conv3d_shuffle: bad dtype");
    const int nsub = st * ss * ss;
    if (B < 1 || F < 1 || H < 1 || W < 1 || F > (1 << 29) || H > (1 << 29) || W > (1 << 29)) LTX_FAIL(LTX_ERR_ARG, "ltx_op_conv3d_shuffle: bad shape");
    if (Cin < 8 || Cin % 8 != 0 || O < 4 * nsub || O % (4 * nsub) != 0) LTX_FAIL(LTX_ERR_ARG, "ltx_op_conv3d_shuffle: Cin must be a multiple of 8 and O a multiple of 4 x the sub-pixel count");
    if ((int64_t)B * (2 * F + 1) * (2 * H) * (2 * W) * std::max(Cin, O) > (1LL << 40)) LTX_FAIL(LTX_ERR_ARG, "ltx_op_conv3d_shuffle: shape too large");
    ConvW cw; cw.cin = Cin; cw.cout = O; cw.nsub = nsub;
    return conv3d_unpacked(dtc(dtype), 1, cw, w, bias, dtc(wdtype), LTX_PERM_D2S, x, y, Dims{B, F + 2, H, W}, EPI_D2S_G, nullptr, 0, (hipStream_t)stream);
}
extern "C" int ltx_op_conv_out_unpatchify(const void* x, const void* w, const void* bias, int wdtype, float* y,
                                          int B, int T, int H, int W, int Cin, int Cout, int causal, int postprocess, int dtype, ltx_stream stream) {
    if (Cout % 16 != 0) LTX_FAIL(LTX_ERR_ARG, "conv_out: Cout must be a multiple of 16 (patch 4x4)");
    return conv_common(x, w, bias, wdtype, y, nullptr, B, T, H, W, Cin, Cout, causal, dtype, EPI_UNPATCH, LTX_PERM_UNPATCH, postprocess, (hipStream_t)stream);
}

extern "C" int ltx_op_blend(const float* a, float* b, int BC, int at, int ah, int aw, int bt, int bh, int bw, int dim, int blend_extent, ltx_stream stream) {
    if (!a || !b || dim < 2 || dim > 4) LTX_FAIL(LTX_ERR_ARG, "ltx_op_blend: bad argument");
    const int ad[3] = {at, ah, aw}, bd[3] = {bt, bh, bw};
    BlendArgs ba; ba.a = a; ba.b = b; ba.dst = b; ba.BC = BC;
    ba.at = at; ba.ah = ah; ba.aw = aw; ba.a_len = ad[dim - 2];
    ba.bt = ba.dt = bt; ba.bh = ba.dh = bh; ba.bw = ba.dw = bw;
    ba.dim = dim; ba.blend = std::min(blend_extent, std::min(ad[dim - 2], bd[dim - 2]));
    ba.et = std::min(at, bt); ba.eh = std::min(ah, bh); ba.ew = std::min(aw, bw);
    if (dim == 2) ba.et = ba.blend; else if (dim == 3) ba.eh = ba.blend; else ba.ew = ba.blend;
    return ltx_launch_blend(ba, (hipStream_t)stream);
}

const char* ltx_gemm_plan_name(int M, int N, int K, int conv, int ntaps, int T, int H, int W);
extern "C" int ltx_op_gemm_plan(int M, int N, int K, int conv, int ntaps, int T, int H, int W, char* name, int cap) {
    if (!name || cap < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_op_gemm_plan: bad argument");
    const char* n = ltx_gemm_plan_name(M, N, K, conv, ntaps, T, H, W);
    snprintf(name, (size_t)cap, "%s", n);
    return LTX_OK;
}

// Read-only probe of the GEMM dispatch: the described call with dense strides and aligned dummy pointers (never dereferenced)
extern "C" int ltx_op_gemm_route(int M, int N, int K, int conv, int ntaps, int B, int T, int H, int W, int epi, int dtype, int flags, char* name, int cap) {
    if (!name || cap < 1 || M < 1 || N < 1 || K < 1 || epi < EPI_BIAS || epi > EPI_D2S_G) LTX_FAIL(LTX_ERR_ARG, "ltx_op_gemm_route: bad argument");
    if (conv && (ntaps < 1 || B < 1 || T < 1 || H < 1 || W < 1 || (int64_t)B * T * H * W != M)) LTX_FAIL(LTX_ERR_ARG, "ltx_op_gemm_route: conv calls need M = B T H W");
    void* const p = reinterpret_cast<void*>((uintptr_t)4096); float* const f = reinterpret_cast<float*>(p);
    const bool res = epi == EPI_GATE_RESID || epi == EPI_RESID;
    GemmArgs g;
    if (flags & LTX_ROUTE_FOLD_IN) g = fold_in_args(p, p, p, f, 16, K, 1e-6f, f, N, M, N, K, M);
    else if (flags & LTX_ROUTE_FOLD_OUT) g = fold_out_args(p, p, p, p, p, f, f, N, M, N, K, p, epi == EPI_GATE_RESID ? f : nullptr, M);
    else {
        g.A = p; g.W = p; g.C = p; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldc = N; g.ldr = N; g.rows_per_batch = M; g.gate_stride = N;
        if (flags & LTX_ROUTE_DEFER) g.defer_parts = f;      // a bare launch: the consumer applies bias, gate and residual
        else { g.bias = p; if (res || epi == EPI_S2D) g.resid = p; if (epi == EPI_GATE_RESID) g.gate = f; }
    }
    if (conv) {
        g.conv = 1; g.B = B; g.T = T; g.H = H; g.Wd = W; g.Cin = K; g.ntaps = ntaps; g.kh = g.kw = ntaps == 27 ? 3 : 1; g.pad_t = 2;
        if (epi == EPI_D2S) { g.Cf = N / 8; g.Cr = K / 8; g.To = 2 * T - 1; g.Ho = 2 * H; g.Wo = 2 * W; }
        if (epi == EPI_S2D) { g.s2_st = g.s2_sh = g.s2_sw = 2; g.To = (T + 1) / 2; g.Ho = H / 2; g.Wo = W / 2; }
        // (the guarded depth-to-space of the latent upsampler: T counts its two guard frames; the factors the channel count admits)
        if (epi == EPI_D2S_G) {
            if (T < 3 || N % 8 != 0) LTX_FAIL(LTX_ERR_ARG, "ltx_op_gemm_route: the guarded depth-to-space call needs T >= 3 and N a multiple of 8");
            const int fs = N % 32 == 0 ? 2 : 1;
            g.pad_t = 1; g.s2_st = 2; g.s2_sh = g.s2_sw = fs; g.Cf = N / (2 * fs * fs); g.To = 2 * T - 3; g.Ho = fs * H; g.Wo = fs * W;
        }
        if (flags & LTX_ROUTE_PN) { g.pn_on = 1; g.pn_eps = 1e-6f; g.pn_act = 1; }
    }
    GemmRoute r;
    LTX_TRY(ltx_gemm_route(g, dtc(dtype), epi, nullptr, false, &r));
    if (const char* why = ltx_gemm_route_refusal(g, r)) LTX_FAIL(LTX_ERR_ARG, why);
    snprintf(name, (size_t)cap, "%s", ltx_gemm_route_name(r));
    return LTX_OK;
}

// Read-only probe of the DiT forward's decisions (dit.hip's ltx_dit_plan): no handle, no device, nothing launched
extern "C" int ltx_op_dit_plan(int heads, int head_dim, int model_dtype, int io_dtype, int B, int S, int K, int G, int skip_mask, int64_t* out) {
    if (!out || heads < 1 || head_dim < 1 || B < 1 || B > 8 || S < 1 || K < 1 || G < 1 || S % G != 0) LTX_FAIL(LTX_ERR_ARG, "ltx_op_dit_plan: bad argument");
    ltx_dit_config c; ltx_dit_config_default(&c);
    c.num_attention_heads = heads; c.attention_head_dim = head_dim; c.cross_attention_dim = heads * head_dim;
    const DitPlan p = ltx_dit_plan(c, dtc(model_dtype), dtc(io_dtype), B, S, K, G, skip_mask != 0);
    const int64_t v[LTX_DIT_PLAN_FIELDS] = {p.M, p.MK, p.NB, p.Sg, p.seg, p.ldqkv, p.fold_q2, p.presum, p.nfold, p.defer_ff2, p.ff2_parts, p.dense_qkv, p.fold_q};
    for (int i = 0; i < LTX_DIT_PLAN_FIELDS; ++i) out[i] = v[i];
    return LTX_OK;
}

// ---- the step cache's kernels on their own (include/ltxhip_stepcache.h) ----
extern "C" size_t ltx_op_step_measure_ws_bytes(int64_t rows, int D, ltx_dtype dtype) {
    return (size_t)ltx_step_measure_blocks(rows, D, dtc((int)dtype)) * 2 * sizeof(double);
}
extern "C" int ltx_op_step_measure(const void* h, void* prev, const float* shift, const float* scale, int mod_stride, int64_t rows, int D,
                                   int64_t rows_per_batch, float eps, ltx_dtype dtype, int first, void* ws, double* sums, ltx_stream stream) {
    if (!h || !prev || !shift || !scale || !ws || !sums) LTX_FAIL(LTX_ERR_ARG, "ltx_op_step_measure: null tensor");
    if (dtype != LTX_F32 && dtype != LTX_BF16) LTX_FAIL(LTX_ERR_ARG, "ltx_op_step_measure: bad dtype");
    if (rows < 1 || rows_per_batch < 1 || mod_stride < D) LTX_FAIL(LTX_ERR_ARG, "ltx_op_step_measure: rows and rows_per_batch must be at least 1 and mod_stride at least D");
    StepMeasureArgs a;
    a.h = h; a.prev = prev; a.shift = shift; a.scale = scale; a.mod_stride = mod_stride; a.rows = rows; a.D = D; a.rows_per_batch = rows_per_batch;
    a.eps = eps; a.first = first != 0; a.part = reinterpret_cast<double*>(ws);
    LTX_TRY(ltx_launch_step_measure(a, dtc((int)dtype), (hipStream_t)stream));
    return ltx_launch_step_measure_finish(a.part, ltx_step_measure_blocks(rows, D, dtc((int)dtype)), sums, (hipStream_t)stream);
}
extern "C" int ltx_op_step_residual(const void* h, void* r, int64_t rows, int D, ltx_dtype dtype, ltx_stream stream) {
    if (dtype != LTX_F32 && dtype != LTX_BF16) LTX_FAIL(LTX_ERR_ARG, "ltx_op_step_residual: bad dtype");
    return ltx_launch_step_residual(h, r, rows, D, dtc((int)dtype), (hipStream_t)stream);
}

// ---- the int8 (W8A8) kernels on their own (include/ltxhip_int8.h) ----
extern "C" int ltx_op_quant_rows_i8(const void* x, int64_t rows, int D, int ld, void* q, float* scale, ltx_stream stream) {
    return ltx_launch_quant_rows_i8(x, rows, D, ld, q, scale, (hipStream_t)stream);
}
extern "C" int ltx_op_rownorm_quant_i8(const void* h, int64_t rows, int D, int ld, float eps, const float* shift, const float* scale, int mod_stride,
                                       int64_t rows_per_batch, void* q, float* row_scale, ltx_stream stream) {
    RowNormArgs a; a.x = h; a.y = q; a.rows = rows; a.D = D; a.ldx = ld; a.ldy = D; a.kind = 0; a.eps = eps; a.shift = shift; a.scale = scale;
    a.mod_stride = mod_stride; a.rows_per_batch = rows_per_batch;
    return ltx_launch_rownorm_quant_i8(a, row_scale, (hipStream_t)stream);
}
extern "C" int ltx_op_gemm_i8(const void* a_q, const float* a_scale, const void* w_q, const float* w_scale, const void* bias, void* y,
                              int M, int N, int K, int epi, const void* resid, const float* gate, int rows_per_batch, int seg_width, int tile,
                              ltx_stream stream) {
    if (epi < 0 || epi > 3) LTX_FAIL(LTX_ERR_ARG, "ltx_op_gemm_i8: epi must be 0..3");
    if (seg_width < 0 || (seg_width > 0 && ((seg_width & (seg_width - 1)) || N % seg_width || epi != 0)))
        LTX_FAIL(LTX_ERR_ARG, "ltx_op_gemm_i8: seg_width must be a power of two dividing N, with epi 0");
    GemmArgs g; g.A = a_q; g.W = w_q; g.C = y; g.bias = bias; g.resid = resid; g.gate = gate;
    g.M = M; g.N = N; g.K = K; g.lda = K; g.ldc = N; g.ldr = N; g.rows_per_batch = rows_per_batch > 0 ? rows_per_batch : 1; g.gate_stride = N;
    if (seg_width > 0) { g.ldc = seg_width; g.c_seg_shift = __builtin_ctz((unsigned)seg_width); g.c_seg_stride = (int64_t)M * seg_width; }
    return ltx_launch_gemm_i8(g, a_scale, w_scale, epi, tile, (hipStream_t)stream);
}
extern "C" int ltx_op_gemm_i8_raw(const void* a_q, const void* w_q, int* acc, int M, int N, int K, int tile, ltx_stream stream) {
    GemmArgs g; g.A = a_q; g.W = w_q; g.C = acc; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldc = N;
    return ltx_launch_gemm_i8(g, nullptr, nullptr, EPI_I8_RAW, tile, (hipStream_t)stream);
}
