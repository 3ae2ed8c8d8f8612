// Small HBM-/latency-bound kernels around the GEMM/attention/conv cores.
#include "common.h"
#include "kernels.h"

namespace {

template <typename T> __device__ __forceinline__ float ld(const void* p, int64_t i) { return to_f32(reinterpret_cast<const T*>(p)[i]); }
__device__ __forceinline__ float ldd(const void* p, int dt, int64_t i) {
    return dt == LTX_DT_BF16 ? (float)reinterpret_cast<const bf16_t*>(p)[i] : reinterpret_cast<const float*>(p)[i];
}
__device__ __forceinline__ void std_(void* p, int dt, int64_t i, float v) {
    if (dt == LTX_DT_BF16) reinterpret_cast<bf16_t*>(p)[i] = (bf16_t)v; else reinterpret_cast<float*>(p)[i] = v;
}
__device__ __forceinline__ float round_dt(float v, int dt) { return dt == LTX_DT_BF16 ? (float)(bf16_t)v : v; }

#define GRID_STRIDE(i, n) for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

// get_timestep_embedding (ltx_transformer.rs:271-309 / vae.rs:172-198): [cos | sin]
__global__ void sinusoid_kernel(void* out, int dt, TimeVec tv, const float* tab, int half, int round_t, float tmul) {
    const int n = tv.n * 2 * half;
    GRID_STRIDE(i, n) {
        int b = (int)(i / (2 * half)), j = (int)(i % (2 * half));
        float t = tv.t[b];
        if (round_t) t = round_dt(t, dt);                   // timestep.to_dtype(model_dtype) (:1051)
        if (tmul != 1.0f) t = round_dt(t * round_dt(tmul, round_t ? dt : LTX_DT_F32), round_t ? dt : LTX_DT_F32);
        float ang = t * tab[j < half ? j : j - half];
        std_(out, dt, i, j < half ? cosf(ang) : sinf(ang));
    }
}

__global__ void silu_kernel(const void* x, void* y, int64_t n, int dt) {
    GRID_STRIDE(i, n) std_(y, dt, i, silu_f(ldd(x, dt, i)));
}

__global__ void cast_kernel(const void* x, int xdt, void* y, int ydt, int64_t n) {
    GRID_STRIDE(i, n) std_(y, ydt, i, ldd(x, xdt, i));
}

__global__ void ada_kernel(float* out, const void* tables, const void* temb, int nl, int B, int width, int dt) {
    const int64_t n = (int64_t)nl * B * width;
    GRID_STRIDE(i, n) {
        int j = (int)(i % width); int64_t r = i / width; int b = (int)(r % B); int l = (int)(r / B);
        out[i] = ldd(tables, dt, (int64_t)l * width + j) + ldd(temb, dt, (int64_t)b * width + j);
    }
}

__global__ void mask_bias_kernel(float* out, const float* mask, int64_t n) {
    GRID_STRIDE(i, n) out[i] = (1.0f - mask[i]) * -10000.0f;      // ltx_transformer.rs:1063
}

// one wave per batch row: ordered compaction of the keys whose bias is above the drop threshold (kernels.h: k_count)
__global__ __launch_bounds__(64) void key_compact_kernel(const float* bias, int K, int* idx, int* count, float* bias_c) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const float* bb = bias + (int64_t)b * K;
    int n = 0;
    for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + lane;
        const float v = k < K ? bb[k] : -INFINITY;
        const bool keep = v > -5000.0f;
        const unsigned long long m = __ballot(keep);
        const int pos = n + __popcll(m & ((1ull << lane) - 1ull));
        if (keep) { idx[(int64_t)b * K + pos] = k; bias_c[(int64_t)b * K + pos] = v; }
        n += __popcll(m);
    }
    if (n == 0) {                                           // every key masked: the mask is a constant shift, keep them all
        for (int k = lane; k < K; k += 64) { idx[(int64_t)b * K + k] = k; bias_c[(int64_t)b * K + k] = bb[k]; }
        n = K;
    }
    for (int k = n + lane; k < K; k += 64) { idx[(int64_t)b * K + k] = 0; bias_c[(int64_t)b * K + k] = -INFINITY; }
    if (lane == 0) count[b] = n;
}

// 16 bytes per thread; one block per destination row
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint4* src, uint4* dst, const int* idx, const int* count, int B, int K, int row_vecs) {
    const int64_t row = blockIdx.x;                         // (l * B + b) * K + pos
    const int pos = (int)(row % K), b = (int)((row / K) % B);
    const int64_t base = row - pos;
    const bool live = pos < count[b];
    const uint4* sp = src + (base + (live ? idx[(int64_t)b * K + pos] : 0)) * row_vecs;
    uint4* dp = dst + row * row_vecs;
    for (int i = threadIdx.x; i < row_vecs; i += 256) dp[i] = live ? sp[i] : make_uint4(0u, 0u, 0u, 0u);
}

__global__ void skip_blend_kernel(void* h, const void* orig, TimeVec m, int64_t rows_per_batch, int D, int dt) {
    const int64_t n = (int64_t)m.n * rows_per_batch * D;
    GRID_STRIDE(i, n) {
        int b = (int)(i / (rows_per_batch * D));
        float mm = m.t[b];
        std_(h, dt, i, ldd(h, dt, i) * (1.0f - mm) + ldd(orig, dt, i) * mm);   // :1112-1123
    }
}

// y = h (.) (1 + scale[b]) in the model dtype: the second output of the norm fold's producers (GemmArgs::C2, gemm_asm.hip - the same
// expression on the rows as stored, so the same bits), for the one place a GEMM epilogue cannot write it: behind the skip-layer blend
__global__ void mod_scale_kernel(const void* h, const float* scale, int scale_stride, void* y, int B, int64_t rows_per_batch, int D, int dt) {
    const int64_t n = (int64_t)B * rows_per_batch * D;
    GRID_STRIDE(i, n) {
        const int b = (int)(i / (rows_per_batch * D)), col = (int)(i % D);
        std_(y, dt, i, ldd(h, dt, i) * (1.0f + scale[(int64_t)b * scale_stride + col]));
    }
}

// STG attention modes (include/ltxhip_stg.h): whole batch rows of src into dst - row (sel[j] * S + s) of both, row_vecs 16-byte
// chunks each, leading dimensions in chunks.  One launch for every selected batch row; a pure HBM copy, 16 bytes per lane.
__global__ __launch_bounds__(256) void stg_fill_kernel(uint4* __restrict__ dst, int64_t ldd_v, const uint4* __restrict__ src, int64_t lds_v, StgRows sel, int64_t S, int row_vecs) {
    const int64_t n = (int64_t)sel.n * S * row_vecs;
    GRID_STRIDE(i, n) {
        const int c = (int)(i % row_vecs); const int64_t t = i / row_vecs;
        const int64_t row = (int64_t)sel.b[(int)(t / S)] * S + t % S;
        dst[row * ldd_v + c] = src[row * lds_v + c];
    }
}

// W'[n][k] = W[n][k] * (1 + scale[k]) in the model dtype (norm fold through the consumer's weights: dit.hip, DitTimeEntry::wfold)
__global__ void scale_cols_kernel(const void* W, const float* scale, void* out, int64_t N, int K, int dt) {
    const int64_t n = N * K;
    GRID_STRIDE(i, n) std_(out, dt, i, ldd(W, dt, i) * (1.0f + scale[(int)(i % K)]));
}

// ---- guidance + Euler (t2v_pipeline.rs:941-964, 227-243; scheduler.rs:576-581) ----
__device__ __forceinline__ float cfg_of(const GuidanceArgs& a, int64_t i, float& t) {
    t = ldd(a.text, a.pred_dtype, i);
    float c = t;
    if (a.uncond) { float u = ldd(a.uncond, a.pred_dtype, i); c = u + (t - u) * a.guidance_scale; }
    return c;
}
__global__ void guidance_stats_kernel(GuidanceArgs a) {
    // per-batch sums for the unbiased std of text and cfg (Tensor::var_keepdim)
    const int b = blockIdx.y;
    double st = 0, sst = 0, sc = 0, ssc = 0;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < a.n_per_batch; j += (int64_t)gridDim.x * blockDim.x) {
        float t; float c = cfg_of(a, (int64_t)b * a.n_per_batch + j, t);
        st += t; sst += (double)t * t; sc += c; ssc += (double)c * c;
    }
    __shared__ double sh[4][256];
    sh[0][threadIdx.x] = st; sh[1][threadIdx.x] = sst; sh[2][threadIdx.x] = sc; sh[3][threadIdx.x] = ssc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) for (int q = 0; q < 4; ++q) sh[q][threadIdx.x] += sh[q][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x < 4) atomicAdd(&a.stats[b * 4 + threadIdx.x], sh[threadIdx.x][0]);
}
// The combined prediction of one element and the scheduler update, ONE body for every kernel that finishes a step (the plain pass,
// the held-frame passes): roundings spelled out - a fused multiply-add exactly where this file's apply kernel has always had one,
// separate roundings elsewhere - so that the bits are a property of the text, not of what a compiler contracts in one kernel or
// another.  ratio: the rescale factor of the element's batch row.
__device__ __forceinline__ float step_pred(const GuidanceArgs& a, float t, float u, float p, float ratio, bool rescale) {
#pragma clang fp contract(off)
    float c = t;
    if (a.uncond) c = __builtin_fmaf(a.guidance_scale, t - u, u);
    if (rescale) {
        const float keep = (1.0f - a.guidance_rescale) * c, resc = ratio * c;
        c = __builtin_fmaf(a.guidance_rescale, resc, keep);
    }
    if (a.pert) c = __builtin_fmaf(a.stg_scale, t - p, c);
    return c;
}
__device__ __forceinline__ float step_update(const GuidanceArgs& a, float x, float c, float noise) {
#pragma clang fp contract(off)
    if (a.step_noise) {
        const float x0 = __builtin_fmaf(-a.sigma, c, x);
        const float keep = (1.0f - a.sigma_next) * x0, fresh = a.sigma_next * noise;
        return keep + fresh;
    }
    return __builtin_fmaf(a.dt, c, x);
}
__device__ __forceinline__ float step_ratio(const GuidanceArgs& a, int b) {
    const double N = (double)a.n_per_batch;
    const double* s = a.stats + b * 4;
    double vt = (s[1] - s[0] * s[0] / N) / (N - 1.0), vc = (s[3] - s[2] * s[2] / N) / (N - 1.0);
    return (float)sqrt(vt) / (float)sqrt(vc);
}
// one element per thread and step, any size and alignment.  a.hold (image-to-video conditioning, include/ltxhip_cond.h): the
// latents of a held frame are left alone; the prediction (noise_out) covers every token.
__global__ void guidance_apply_kernel(GuidanceArgs a) {
    const int64_t n = (int64_t)a.B * a.n_per_batch;
    const bool rescale = a.uncond && a.guidance_rescale > 0.0f;
    GRID_STRIDE(i, n) {
        const int b = (rescale || a.hold) ? (int)(i / a.n_per_batch) : 0;
        const bool held = a.hold && a.hold[(int64_t)b * a.num_frames + (int)((i - (int64_t)b * a.n_per_batch) / a.frame_elems)] != 0;
        if (held && !a.noise_out) continue;
        const float t = ldd(a.text, a.pred_dtype, i);
        const float u = a.uncond ? ldd(a.uncond, a.pred_dtype, i) : 0.f, p = a.pert ? ldd(a.pert, a.pred_dtype, i) : 0.f;
        const float c = step_pred(a, t, u, p, rescale ? step_ratio(a, b) : 1.0f, rescale);
        if (a.noise_out) a.noise_out[i] = c;
        if (held || !a.latents) continue;
        a.latents[i] = step_update(a, a.latents[i], c, a.step_noise ? a.step_noise[i] : 0.f);
    }
}

template <typename P> __device__ __forceinline__ void ld4(const P* p, float* v);
template <> __device__ __forceinline__ void ld4<float>(const float* p, float* v) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(p);
    v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
}
template <> __device__ __forceinline__ void ld4<bf16_t>(const bf16_t* p, float* v) {
    const uint2 x = *reinterpret_cast<const uint2*>(p);
    v[0] = __uint_as_float(x.x << 16); v[1] = __uint_as_float(x.x & 0xffff0000u);
    v[2] = __uint_as_float(x.y << 16); v[3] = __uint_as_float(x.y & 0xffff0000u);
}
// Held frames, 16-byte chunks of four f32 (8 bytes of a bf16 prediction): n_per_batch and frame_elems are multiples of 4, so a chunk
// lies in one frame of one batch row - one division pair per chunk, none per element.  A held chunk reads the predictions only if
// noise_out wants them and never touches the latents.
template <typename P>
__global__ __launch_bounds__(256) void guidance_held_vec_kernel(GuidanceArgs a) {
    const int64_t chunks_per_batch = a.n_per_batch >> 2, chunks_per_frame = a.frame_elems >> 2;
    const int64_t nchunks = (int64_t)a.B * chunks_per_batch;
    const bool rescale = a.uncond && a.guidance_rescale > 0.0f;
    const P* tp = reinterpret_cast<const P*>(a.text); const P* up = reinterpret_cast<const P*>(a.uncond); const P* pp = reinterpret_cast<const P*>(a.pert);
    GRID_STRIDE(ch, nchunks) {
        const int b = (int)(ch / chunks_per_batch);
        const int f = (int)((ch - (int64_t)b * chunks_per_batch) / chunks_per_frame);
        const bool held = a.hold[(int64_t)b * a.num_frames + f] != 0;
        if (held && !a.noise_out) continue;
        const int64_t i = ch << 2;
        float t[4], u[4] = {0.f, 0.f, 0.f, 0.f}, p[4] = {0.f, 0.f, 0.f, 0.f}, c[4];
        ld4<P>(tp + i, t);
        if (up) ld4<P>(up + i, u);
        if (pp) ld4<P>(pp + i, p);
        const float ratio = rescale ? step_ratio(a, b) : 1.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = step_pred(a, t[k], u[k], p[k], ratio, rescale);
        if (a.noise_out) *reinterpret_cast<f32x4*>(a.noise_out + i) = (f32x4){c[0], c[1], c[2], c[3]};
        if (held || !a.latents) continue;
        const f32x4 x = *reinterpret_cast<const f32x4*>(a.latents + i);
        f32x4 nz = {0.f, 0.f, 0.f, 0.f};
        if (a.step_noise) nz = *reinterpret_cast<const f32x4*>(a.step_noise + i);
        f32x4 y;
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = step_update(a, x[k], c[k], nz[k]);
        *reinterpret_cast<f32x4*>(a.latents + i) = y;
    }
}
// ---- the scheduled mix (include/ltxhip_guidance.h): CFG-star, two rescale forms ----
// A batch row of n elements starts at element b * n of every tensor, so with all bases 16-byte aligned (8 for bf16 predictions) the
// row splits the same way in each: `head` elements up to the next 16-byte boundary, nch chunks of four, the rest.  The elements
// outside the chunks (at most 6 of an aligned row; all of them when a base is not aligned: vec == 0) go one by one.
struct RowSplit {
    int64_t head, nch, nsc;
    __device__ __forceinline__ int64_t scalar_elem(int64_t k) const { return k < head ? k : k + 4 * nch; }
};
__device__ __forceinline__ RowSplit row_split(int64_t n, int b, int vec) {
    RowSplit r;
    if (!vec) { r.head = 0; r.nch = 0; r.nsc = n; return r; }
    const int64_t mis = (4 - (((int64_t)b * n) & 3)) & 3;
    r.head = mis < n ? mis : n; r.nch = (n - r.head) >> 2; r.nsc = n - 4 * r.nch;
    return r;
}
enum { MOM_T = 0, MOM_U, MOM_P, MOM_TT, MOM_UU, MOM_PP, MOM_TU, MOM_TP, MOM_UP, MOM_N };
// Sum t, u, p, t^2, u^2, p^2, tu, tp, up of one batch row in f64: everything the mean and variance of any c = at t + au u + ap p
// and CFG-star's alpha need.  HU / HP: the branch exists (an absent one is not read; a template parameter, so no load sits behind a
// runtime select).  Per block: lanes -> wave (shuffles) -> the four waves through LDS in wave order -> ONE partial in part[b][block][9].
template <typename P, bool HU, bool HP>
__global__ __launch_bounds__(256) void guidance_moments_kernel(const P* __restrict__ tp, const P* __restrict__ up, const P* __restrict__ pp,
                                                               int64_t n, int vec, double* __restrict__ part) {
    const int b = blockIdx.y;
    const RowSplit rs = row_split(n, b, vec);
    const int64_t base = (int64_t)b * n;
    double acc[MOM_N];
#pragma unroll
    for (int q = 0; q < MOM_N; ++q) acc[q] = 0.0;
    auto add = [&](float tf, float uf, float pf) {
        const double t = tf; acc[MOM_T] += t; acc[MOM_TT] += t * t;
        if (HU) { const double u = uf; acc[MOM_U] += u; acc[MOM_UU] += u * u; acc[MOM_TU] += t * u; }
        if (HP) { const double p = pf; acc[MOM_P] += p; acc[MOM_PP] += p * p; acc[MOM_TP] += t * p; }
        if (HU && HP) acc[MOM_UP] += (double)uf * (double)pf;
    };
    const int64_t stride = (int64_t)gridDim.x * 256, first = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t ch = first; ch < rs.nch; ch += stride) {
        const int64_t i = base + rs.head + 4 * ch;
        float t[4], u[4] = {0.f, 0.f, 0.f, 0.f}, p[4] = {0.f, 0.f, 0.f, 0.f};
        ld4<P>(tp + i, t);
        if (HU) ld4<P>(up + i, u);
        if (HP) ld4<P>(pp + i, p);
#pragma unroll
        for (int k = 0; k < 4; ++k) add(t[k], u[k], p[k]);
    }
    for (int64_t k = first; k < rs.nsc; k += stride) {
        const int64_t i = base + rs.scalar_elem(k);
        add(to_f32(tp[i]), HU ? to_f32(up[i]) : 0.f, HP ? to_f32(pp[i]) : 0.f);
    }
#pragma unroll
    for (int q = 0; q < MOM_N; ++q)
        for (int o = 32; o > 0; o >>= 1) acc[q] += __shfl_down(acc[q], o, 64);
    __shared__ double sh[4][MOM_N];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < MOM_N; ++q) sh[wave][q] = acc[q];
    }
    __syncthreads();
    if (threadIdx.x < MOM_N) part[((int64_t)b * gridDim.x + blockIdx.x) * MOM_N + threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}
// One block per batch row: the row's partials are summed in one fixed tree, thread 0 turns the nine sums into
// alpha = <t,u> / (<u,u> + 1e-8) and factor = r * (std t / std c) + (1 - r), each computed in f64 and rounded to f32 once.
// use_alpha / resc: the step has them (otherwise 1).  at, au (times alpha), ap: c = at t + au alpha u + ap p in front of the rescale.
__global__ __launch_bounds__(256) void guidance_finish_kernel(const double* __restrict__ part, int nblk, int64_t n, int use_alpha, int resc,
                                                              float at_f, float au_f, float ap_f, float r_f, float* __restrict__ scal, float* __restrict__ scal_out) {
    const int b = blockIdx.x;
    // thread k holds partial k (nblk <= 256: every load is in flight at once, not one round trip per partial); then the moments
    // kernel's own fixed tree - lanes by shuffles, the four waves through LDS in wave order
    double acc[MOM_N];
#pragma unroll
    for (int q = 0; q < MOM_N; ++q) acc[q] = (int)threadIdx.x < nblk ? part[((int64_t)b * nblk + threadIdx.x) * MOM_N + q] : 0.0;
#pragma unroll
    for (int q = 0; q < MOM_N; ++q)
        for (int o = 32; o > 0; o >>= 1) acc[q] += __shfl_down(acc[q], o, 64);
    __shared__ double sh[4][MOM_N];
    __shared__ double S[MOM_N];
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < MOM_N; ++q) sh[threadIdx.x >> 6][q] = acc[q];
    }
    __syncthreads();
    if (threadIdx.x < MOM_N) S[threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
    __syncthreads();
    if (threadIdx.x != 0) return;
    float alpha = 1.0f, factor = 1.0f;
    if (use_alpha) alpha = (float)(S[MOM_TU] / (S[MOM_UU] + 1e-8));
    if (resc) {
        const double N = (double)n, at = at_f, au = (double)au_f * (double)alpha, ap = ap_f, r = r_f;
        const double sc = at * S[MOM_T] + au * S[MOM_U] + ap * S[MOM_P];
        const double scc = at * at * S[MOM_TT] + au * au * S[MOM_UU] + ap * ap * S[MOM_PP] + 2.0 * (at * au * S[MOM_TU] + at * ap * S[MOM_TP] + au * ap * S[MOM_UP]);
        const double nan = __longlong_as_double(0x7ff8000000000000LL);         // one element: the unbiased variance is 0 / 0
        const double vt = n > 1 ? (S[MOM_TT] - S[MOM_T] * S[MOM_T] / N) / (N - 1.0) : nan;
        const double vc = n > 1 ? (scc - sc * sc / N) / (N - 1.0) : nan;
        factor = (float)(r * (sqrt(vt) / sqrt(vc)) + (1.0 - r));
    }
    scal[2 * b] = alpha; scal[2 * b + 1] = factor;
    if (scal_out) { scal_out[2 * b] = alpha; scal_out[2 * b + 1] = factor; }
}
// the combined prediction of one element: roundings spelled out as in step_pred (one fused multiply-add per guidance term)
__device__ __forceinline__ float mix_ex(const GuidanceArgs& a, int form, bool resc, float alpha, float factor, float t, float u, float p) {
#pragma clang fp contract(off)
    float c = t;
    if (a.uncond) { const float us = alpha * u; c = __builtin_fmaf(a.guidance_scale, t - us, us); }
    if (form == 0) {
        if (resc) c = factor * c;
        if (a.pert) c = __builtin_fmaf(a.stg_scale, t - p, c);
    } else {
        if (a.pert) c = __builtin_fmaf(a.stg_scale, t - p, c);
        if (resc) c = c * factor;
    }
    return c;
}
// 16-byte accesses on the chunks of a row (row_split); every load of an iteration is issued in front of its stores.  A chunk whose
// four elements are all held reads the predictions only if noise_out wants them and leaves the latents alone; a chunk that a frame
// boundary cuts writes a held element's own bits back.  scal: (alpha, factor) per batch row, or null (both 1).
template <typename P>
__global__ __launch_bounds__(256) void guidance_apply_ex_kernel(GuidanceArgs a, int form, int resc_i, int vec, const float* __restrict__ scal) {
    const int b = blockIdx.y;
    const int64_t n = a.n_per_batch, base = (int64_t)b * n;
    const RowSplit rs = row_split(n, b, vec);
    const bool resc = resc_i != 0;
    const float alpha = scal ? scal[2 * b] : 1.0f, factor = scal ? scal[2 * b + 1] : 1.0f;
    const P* tp = reinterpret_cast<const P*>(a.text); const P* up = reinterpret_cast<const P*>(a.uncond); const P* pp = reinterpret_cast<const P*>(a.pert);
    const unsigned char* hold = a.hold ? a.hold + (int64_t)b * a.num_frames : nullptr;
    const bool one_frame = hold && (a.frame_elems & 3) == 0 && rs.head == 0;     // a chunk never crosses a frame boundary
    const int64_t stride = (int64_t)gridDim.x * 256, first = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t ch = first; ch < rs.nch; ch += stride) {
        const int64_t j0 = rs.head + 4 * ch, i = base + j0;
        bool h[4] = {false, false, false, false};
        if (one_frame) h[0] = h[1] = h[2] = h[3] = hold[j0 / a.frame_elems] != 0;
        else if (hold) {
#pragma unroll
            for (int k = 0; k < 4; ++k) h[k] = hold[(j0 + k) / a.frame_elems] != 0;
        }
        const bool skip_x = !a.latents || (h[0] && h[1] && h[2] && h[3]);
        if (skip_x && !a.noise_out) continue;
        float t[4], u[4] = {0.f, 0.f, 0.f, 0.f}, p[4] = {0.f, 0.f, 0.f, 0.f}, c[4];
        ld4<P>(tp + i, t);
        if (up) ld4<P>(up + i, u);
        if (pp) ld4<P>(pp + i, p);
        f32x4 x = {0.f, 0.f, 0.f, 0.f}, nz = {0.f, 0.f, 0.f, 0.f};
        if (!skip_x) {
            x = *reinterpret_cast<const f32x4*>(a.latents + i);
            if (a.step_noise) nz = *reinterpret_cast<const f32x4*>(a.step_noise + i);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = mix_ex(a, form, resc, alpha, factor, t[k], u[k], p[k]);
        if (a.noise_out) *reinterpret_cast<f32x4*>(a.noise_out + i) = (f32x4){c[0], c[1], c[2], c[3]};
        if (skip_x) continue;
        f32x4 y;
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = h[k] ? x[k] : step_update(a, x[k], c[k], nz[k]);
        *reinterpret_cast<f32x4*>(a.latents + i) = y;
    }
    for (int64_t k = first; k < rs.nsc; k += stride) {
        const int64_t j = rs.scalar_elem(k), i = base + j;
        const bool held = hold && hold[j / a.frame_elems] != 0;
        const bool skip_x = !a.latents || held;
        if (skip_x && !a.noise_out) continue;
        const float t = to_f32(tp[i]), u = up ? to_f32(up[i]) : 0.f, p = pp ? to_f32(pp[i]) : 0.f;
        const float x = skip_x ? 0.f : a.latents[i], nz = (!skip_x && a.step_noise) ? a.step_noise[i] : 0.f;
        const float c = mix_ex(a, form, resc, alpha, factor, t, u, p);
        if (a.noise_out) a.noise_out[i] = c;
        if (!skip_x) a.latents[i] = step_update(a, x, c, nz);
    }
}
// one block row per (batch row, frame): a held frame is copied in 16-byte chunks (or element-wise when the frame is not a multiple of 4)
__global__ __launch_bounds__(256) void cond_apply_kernel(float* latents, const float* cond, int Fc, const unsigned char* hold, int F, int64_t frame_elems, int vec) {
    const int bf = blockIdx.y, b = bf / F, f = bf - b * F;
    if (!hold[bf] || f >= Fc) return;
    float* dst = latents + (int64_t)bf * frame_elems;
    const float* src = cond + ((int64_t)b * Fc + f) * frame_elems;
    if (vec) {
        const int64_t nv = frame_elems >> 2;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x)
            reinterpret_cast<f32x4*>(dst)[i] = reinterpret_cast<const f32x4*>(src)[i];
    } else {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < frame_elems; i += (int64_t)gridDim.x * blockDim.x) dst[i] = src[i];
    }
}
// Keyframe conditioning (include/ltxhip_keyframes.h).  Both kernels: one block row per (table entry, batch row), one 16-byte chunk
// (vec) or one element per thread and no loop - the grid covers the group, so no load follows a store in a thread.
// cond_place: group tab.group[e] of the latents becomes a + s * (b - a), a its own value (the caller's noise) and b the item's frame;
// s == 1 copies the item's bits (cond_apply_kernel's copy), s == 0 entries never reach the table.
__global__ __launch_bounds__(256) void cond_place_kernel(float* latents, CondPlaceTab tab, int G, int64_t group_elems, int vec) {
    const int e = blockIdx.y, b = blockIdx.z;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (vec ? group_elems >> 2 : group_elems)) return;
    float* dst = latents + ((int64_t)b * G + tab.group[e]) * group_elems;
    const float* src = tab.src[e] + (int64_t)b * tab.src_batch_stride[e];
    const float s = tab.strength[e];
    if (vec) {
        const f32x4 y = reinterpret_cast<const f32x4*>(src)[i];
        if (s == 1.0f) { reinterpret_cast<f32x4*>(dst)[i] = y; return; }
        const f32x4 a = reinterpret_cast<const f32x4*>(dst)[i];
        f32x4 r;
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = __builtin_fmaf(s, y[k] - a[k], a[k]);
        reinterpret_cast<f32x4*>(dst)[i] = r;
    } else {
        const float y = src[i];
        dst[i] = s == 1.0f ? y : __builtin_fmaf(s, y - dst[i], dst[i]);
    }
}
// cond_noise: latents = clean + k * noise on the hard-held groups tab.group[0 .. tab.n); all three tensors are [B, G, group_elems]
__global__ __launch_bounds__(256) void cond_noise_kernel(float* latents, const float* clean, const float* noise, CondGroupTab tab, int G, int64_t group_elems, float k, int vec) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (vec ? group_elems >> 2 : group_elems)) return;
    const int64_t base = ((int64_t)blockIdx.z * G + tab.group[blockIdx.y]) * group_elems;
    if (vec) {
        const f32x4 c = reinterpret_cast<const f32x4*>(clean + base)[i], z = reinterpret_cast<const f32x4*>(noise + base)[i];
        f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = __builtin_fmaf(k, z[j], c[j]);
        reinterpret_cast<f32x4*>(latents + base)[i] = r;
    } else {
        latents[base + i] = __builtin_fmaf(k, noise[base + i], clean[base + i]);
    }
}
// the per-group modulation tables (kernels.h: ltx_launch_group_gather); one thread per 16-byte chunk of a destination row.  The value
// indices of the launch's <= 128 groups travel by value (a kernel argument is copied when the launch is enqueued: no upload to wait for).
__global__ __launch_bounds__(256) void group_gather_kernel(float* dst, int64_t dst_stride, const float* src, int64_t src_stride, GroupIdx idx, int g0, int ng, int c0, int nc, int nl, int width4) {
    const int64_t n = (int64_t)nl * ng * width4;
    GRID_STRIDE(i, n) {
        const int j = (int)(i % width4); const int64_t r = i / width4; const int g = (int)(r % ng), l = (int)(r / ng);
        const int v = idx.v[g] - c0;
        if (v < 0 || v >= nc) continue;
        reinterpret_cast<f32x4*>(dst + l * dst_stride + (int64_t)(g0 + g) * width4 * 4)[j] = reinterpret_cast<const f32x4*>(src + l * src_stride + (int64_t)v * width4 * 4)[j];
    }
}

// denormalize_latents (t2v_pipeline.rs:573-594) + decode-noise mix (:1049-1062); tokens are already channels-last
__global__ void denorm_mix_kernel(const float* lat, const float* mean, const float* sd, float inv_sf, const float* noise,
                                  TimeVec ns, void* out, int dt, int B, int64_t S, int C) {
    const int64_t n = (int64_t)B * S * C;
    GRID_STRIDE(i, n) {
        int c = (int)(i % C); int64_t r = i / C; int64_t s = r % S; int b = (int)(r / S);
        float x = lat[i] * sd[c] * inv_sf + mean[c];
        if (noise) {
            float sc = ns.t[b];
            x = x * (1.0f - sc) + noise[((int64_t)b * C + c) * S + s] * sc;
        }
        std_(out, dt, i, x);
    }
}

__global__ void ncthw_to_cl_kernel(const void* x, int xdt, void* y, int ydt, int B, int C, int64_t S) {
    const int64_t n = (int64_t)B * S * C;
    GRID_STRIDE(i, n) {
        int c = (int)(i % C); int64_t r = i / C; int64_t s = r % S; int b = (int)(r / S);
        std_(y, ydt, i, ldd(x, xdt, ((int64_t)b * C + c) * S + s));
    }
}

__global__ void blend_kernel(BlendArgs a) {
    // dst[..., x] = a[..., a_len - blend + x]*(1 - x/blend) + b[..., x]*(x/blend) along `dim`
    const int64_t n = (int64_t)a.BC * a.et * a.eh * a.ew;
    GRID_STRIDE(i, n) {
        int w = (int)(i % a.ew); int64_t r = i / a.ew; int h = (int)(r % a.eh); r /= a.eh; int t = (int)(r % a.et); int bc = (int)(r / a.et);
        const int off = a.a_len - a.blend;
        const int x = a.dim == 2 ? t : (a.dim == 3 ? h : w);
        const int ta = t + (a.dim == 2 ? off : 0), ha = h + (a.dim == 3 ? off : 0), wa = w + (a.dim == 4 ? off : 0);
        float wgt = (float)x * a.inv_blend;
        int64_t ib = (((int64_t)bc * a.bt + t) * a.bh + h) * a.bw + w;
        int64_t ia = (((int64_t)bc * a.at + ta) * a.ah + ha) * a.aw + wa;
        int64_t id = (((int64_t)bc * a.dt + a.ot + t) * a.dh + a.oh + h) * a.dw + a.ow + w;
        a.dst[id] = a.a[ia] * (1.0f - wgt) + a.b[ib] * wgt;
    }
}

__global__ void copy_window_kernel(const float* src, int t, int h, int w, float* dst, int T, int H, int W, int BC,
                                   int st, int sh, int sw, int ot, int oh, int ow) {
    const int64_t n = (int64_t)BC * st * sh * sw;
    GRID_STRIDE(i, n) {
        int x = (int)(i % sw); int64_t r = i / sw; int y = (int)(r % sh); r /= sh; int z = (int)(r % st); int bc = (int)(r / st);
        dst[(((int64_t)bc * T + ot + z) * H + oh + y) * W + ow + x] = src[(((int64_t)bc * t + z) * h + y) * w + x];
    }
}

__global__ void postprocess_kernel(float* x, int64_t n) {
    GRID_STRIDE(i, n) x[i] = fminf(fmaxf(x[i] * 0.5f + 0.5f, 0.0f), 1.0f) * 255.0f;   // t2v_pipeline.rs:146-155
}

// LtxVideoResnetBlock3d::maybe_inject_noise (vae.rs:741-753) on a channels-last tensor: y = x + noise[h, w] * scale[c], the
// reference's roundings in the model dtype (noise cast first, the product rounded, the sum rounded), then optionally the block's
// shortcut (vae.rs:811-819: result = h + x, one more rounding)
template <typename T>
__global__ void noise_inject_kernel(const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ noise, const T* __restrict__ scale,
                                    const T* __restrict__ resid, int64_t n, int C, int64_t HW) {
    GRID_STRIDE(i, n) {
        const int c = (int)(i % C); const int64_t hw = (i / C) % HW;
        const float p = to_f32((T)(to_f32((T)noise[hw]) * to_f32(scale[c])));
        T v = (T)(to_f32(x[i]) + p);
        if (resid) v = (T)(to_f32(v) + to_f32(resid[i]));
        y[i] = v;
    }
}

inline dim3 grid_for(int64_t n) { return dim3(ltx_grid1d(n, 16384)); }

}  // namespace

int ltx_launch_sinusoid(void* out, int dtype, const TimeVec& tv, const float* tab, int half, int round_t, float tmul, hipStream_t s) {
    if (tv.n < 1 || tv.n > LTX_MAX_BATCH) LTX_FAIL(LTX_ERR_ARG, "batch must be 1..16");
    hipLaunchKernelGGL(sinusoid_kernel, grid_for(tv.n * 2 * half), dim3(256), 0, s, out, dtype, tv, tab, half, round_t, tmul);
    LTX_CHECK_LAUNCH(); return LTX_OK;
}
int ltx_launch_noise_inject(const void* x, void* y, const float* noise, const void* scale, const void* resid, int64_t rows, int C, int64_t HW, int dtype, hipStream_t s) {
    if (!x || !y || !noise || !scale || rows < 1 || C < 1 || HW < 1 || rows % HW != 0) LTX_FAIL(LTX_ERR_ARG, "noise_inject: bad arguments");
    const int64_t n = rows * C;
    if (dtype == LTX_DT_BF16) hipLaunchKernelGGL(noise_inject_kernel<bf16_t>, grid_for(n), dim3(256), 0, s, (const bf16_t*)x, (bf16_t*)y, noise, (const bf16_t*)scale, (const bf16_t*)resid, n, C, HW);
    else hipLaunchKernelGGL(noise_inject_kernel<float>, grid_for(n), dim3(256), 0, s, (const float*)x, (float*)y, noise, (const float*)scale, (const float*)resid, n, C, HW);
    LTX_CHECK_LAUNCH(); return LTX_OK;
}
int ltx_launch_silu(const void* x, void* y, int64_t n, int dtype, hipStream_t s) {
    hipLaunchKernelGGL(silu_kernel, grid_for(n), dim3(256), 0, s, x, y, n, dtype);
    LTX_CHECK_LAUNCH(); return LTX_OK;
}
int ltx_launch_cast(const void* x, int xdt, void* y, int ydt, int64_t n, hipStream_t s) {
    if (n <= 0) return LTX_OK;
    hipLaunchKernelGGL(cast_kernel, grid_for(n), dim3(256), 0, s, x, xdt, y, ydt, n);
    LTX_CHECK_LAUNCH(); return LTX_OK;
}
int ltx_launch_ada(float* out, const void* tables, const void* temb, int nl, int B, int width, int dtype, hipStream_t s) {
    hipLaunchKernelGGL(ada_kernel, grid_for((int64_t)nl * B * width), dim3(256), 0, s, out, tables, temb, nl, B, width, dtype);
    LTX_CHECK_LAUNCH(); return LTX_OK;
}
int ltx_launch_mask_bias(float* out, const float* mask, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(mask_bias_kernel, grid_for(n), dim3(256), 0, s, out, mask, n);
    LTX_CHECK_LAUNCH(); return LTX_OK;
}
int ltx_launch_key_compact(const float* bias, int B, int K, int* idx, int* count, float* bias_c, hipStream_t s) {
    if (!bias || !idx || !count || !bias_c || B < 1 || K < 1) LTX_FAIL(LTX_ERR_ARG, "key_compact: bad argument");
    hipLaunchKernelGGL(key_compact_kernel, dim3((unsigned)B), dim3(64), 0, s, bias, K, idx, count, bias_c);
    LTX_CHECK_LAUNCH(); return LTX_OK;
}
int ltx_launch_gather_rows(const void* src, void* dst, const int* idx, const int* count, int nl, int B, int K, int row_bytes, hipStream_t s) {
    if (!src || !dst || !idx || !count || nl < 1 || B < 1 || K < 1 || row_bytes < 16 || row_bytes % 16 || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15))
        LTX_FAIL(LTX_ERR_ARG, "gather_rows: bad argument");
    if ((int64_t)nl * B * K > 0x7fffffffLL) LTX_FAIL(LTX_ERR_ARG, "gather_rows: too many rows");
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)(nl * B * K)), dim3(256), 0, s, reinterpret_cast<const uint4*>(src), reinterpret_cast<uint4*>(dst), idx, count, B, K, row_bytes / 16);
    LTX_CHECK_LAUNCH(); return LTX_OK;
}
int ltx_launch_skip_blend(void* h, const void* orig, const TimeVec& m, int64_t rows_per_batch, int D, int dtype, hipStream_t s) {
    hipLaunchKernelGGL(skip_blend_kernel, grid_for((int64_t)m.n * rows_per_batch * D), dim3(256), 0, s, h, orig, m, rows_per_batch, D, dtype);
    LTX_CHECK_LAUNCH(); return LTX_OK;
}
int ltx_launch_mod_scale(const void* h, const float* scale, int scale_stride, void* y, int B, int64_t rows_per_batch, int D, int dtype, hipStream_t s) {
    hipLaunchKernelGGL(mod_scale_kernel, grid_for((int64_t)B * rows_per_batch * D), dim3(256), 0, s, h, scale, scale_stride, y, B, rows_per_batch, D, dtype);
    LTX_CHECK_LAUNCH(); return LTX_OK;
}
int ltx_launch_stg_fill(void* dst, int ldd, const void* src, int lds, const unsigned char* rows_host, int B, int64_t S, int D, int dtype, hipStream_t s) {
    const int ch = dtype == LTX_DT_BF16 ? 8 : 4;           // elements of a 16-byte chunk
    if (!dst || !src || !rows_host || B < 1 || S < 1 || D < 1 || ldd < D || lds < D) LTX_FAIL(LTX_ERR_ARG, "stg_fill: bad argument");
    if (D % ch != 0 || ldd % ch != 0 || lds % ch != 0 || ((uintptr_t)dst & 15) || ((uintptr_t)src & 15))
        LTX_FAIL(LTX_ERR_ARG, "stg_fill: the row length and both leading dimensions must be multiples of 16 bytes and both pointers 16-byte aligned");
    StgRows sel; sel.n = 0;
    auto flush = [&]() -> int {
        if (sel.n == 0) return LTX_OK;
        hipLaunchKernelGGL(stg_fill_kernel, grid_for((int64_t)sel.n * S * (D / ch)), dim3(256), 0, s, reinterpret_cast<uint4*>(dst), (int64_t)(ldd / ch),
                           reinterpret_cast<const uint4*>(src), (int64_t)(lds / ch), sel, S, D / ch);
        LTX_CHECK_LAUNCH(); sel.n = 0; return LTX_OK;
    };
    for (int b = 0; b < B; ++b) {                           // (a forward has at most 8 batch rows: one launch)
        if (!rows_host[b]) continue;
        sel.b[sel.n++] = b;
        if (sel.n == LTX_MAX_BATCH) LTX_TRY(flush());
    }
    return flush();
}
int ltx_launch_scale_cols(const void* W, const float* scale, void* out, int64_t N, int K, int dtype, hipStream_t s) {
    hipLaunchKernelGGL(scale_cols_kernel, grid_for(N * K), dim3(256), 0, s, W, scale, out, N, K, dtype);
    LTX_CHECK_LAUNCH(); return LTX_OK;
}
int ltx_launch_guidance_step(const GuidanceArgs& a, hipStream_t s) {
    if (!a.text || a.B < 1 || a.n_per_batch < 1) LTX_FAIL(LTX_ERR_ARG, "guidance: text prediction required");
    if (a.hold && (a.num_frames < 1 || a.frame_elems < 1 || (int64_t)a.num_frames * a.frame_elems != a.n_per_batch))
        LTX_FAIL(LTX_ERR_ARG, "guidance (held): n must equal num_frames * frame_elems");
    const bool rescale = a.uncond && a.guidance_rescale > 0.0f;
    if (rescale) {                                          // (the statistics of ALL tokens of a batch row, held or not)
        if (!a.stats) LTX_FAIL(LTX_ERR_ARG, "guidance: rescale needs a stats workspace");
        HIP_TRY(hipMemsetAsync(a.stats, 0, sizeof(double) * 4 * a.B, s));
        int64_t bx = cdiv64(a.n_per_batch, 256 * 8); if (bx > 1024) bx = 1024; if (bx < 1) bx = 1;
        hipLaunchKernelGGL(guidance_stats_kernel, dim3((unsigned)bx, (unsigned)a.B), dim3(256), 0, s, a);
        LTX_CHECK_LAUNCH();
    }
    // held frames: the 16-byte kernel where every chunk of four lies in one frame and every pointer is aligned for it
    const bool bf = a.pred_dtype == LTX_DT_BF16;
    const uintptr_t pa = bf ? 7 : 15;
    const bool vec = a.hold && a.frame_elems % 4 == 0 && !((uintptr_t)a.text & pa) && !((uintptr_t)a.uncond & pa) && !((uintptr_t)a.pert & pa) &&
                     !((uintptr_t)a.latents & 15) && !((uintptr_t)a.noise_out & 15) && !((uintptr_t)a.step_noise & 15);
    if (vec) {
        const dim3 grid = grid_for((int64_t)a.B * (a.n_per_batch >> 2));
        if (bf) hipLaunchKernelGGL(guidance_held_vec_kernel<bf16_t>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(guidance_held_vec_kernel<float>, grid, dim3(256), 0, s, a);
    } else hipLaunchKernelGGL(guidance_apply_kernel, grid_for((int64_t)a.B * a.n_per_batch), dim3(256), 0, s, a);
    LTX_CHECK_LAUNCH(); return LTX_OK;
}
int ltx_launch_guidance_step_held(const GuidanceArgs& a, hipStream_t s) {
    if (!a.hold) LTX_FAIL(LTX_ERR_ARG, "guidance (held): hold is required");
    return ltx_launch_guidance_step(a, s);
}
// ---- the scheduled mix (include/ltxhip_guidance.h) ----
namespace {
// blocks of the moments pass per batch row: 2048 elements each, 256 at most - a function of n alone, so the partials' order is too
inline int moments_blocks(int64_t n) { const int64_t b = cdiv64(n, 2048); return (int)(b > 256 ? 256 : (b < 1 ? 1 : b)); }
template <typename P>
void launch_moments(const GuidanceArgs& g, bool with_pert, int vec, int nblk, double* part, hipStream_t s) {
    const dim3 grid((unsigned)nblk, (unsigned)g.B);
    // the perturbed prediction is read only where it is part of the rescaled c (LTX_RESCALE_MIX)
    const P* t = reinterpret_cast<const P*>(g.text); const P* u = reinterpret_cast<const P*>(g.uncond); const P* p = with_pert ? reinterpret_cast<const P*>(g.pert) : nullptr;
    if (u && p) hipLaunchKernelGGL((guidance_moments_kernel<P, true, true>), grid, dim3(256), 0, s, t, u, p, g.n_per_batch, vec, part);
    else if (u) hipLaunchKernelGGL((guidance_moments_kernel<P, true, false>), grid, dim3(256), 0, s, t, u, p, g.n_per_batch, vec, part);
    else if (p) hipLaunchKernelGGL((guidance_moments_kernel<P, false, true>), grid, dim3(256), 0, s, t, u, p, g.n_per_batch, vec, part);
    else hipLaunchKernelGGL((guidance_moments_kernel<P, false, false>), grid, dim3(256), 0, s, t, u, p, g.n_per_batch, vec, part);
}
}  // namespace
size_t ltx_guidance_ex_ws_bytes(int B, int64_t n_per_batch) {
    if (B < 1 || n_per_batch < 1) return 0;
    const size_t bytes = (size_t)B * moments_blocks(n_per_batch) * MOM_N * sizeof(double) + (size_t)B * 2 * sizeof(float);
    return (bytes + 15) & ~(size_t)15;
}
int ltx_launch_guidance_step_ex(const GuidanceExArgs& a, hipStream_t s) {
    const GuidanceArgs& g = a.g;
    if (!g.text || g.B < 1 || g.B > 65535 || g.n_per_batch < 1 || g.n_per_batch > (1LL << 40)) LTX_FAIL(LTX_ERR_ARG, "guidance_step_ex: text prediction, 1 <= B <= 65535 and 1 <= n <= 2^40 required");
    if (!g.latents && !g.noise_out && !a.scalars_out) LTX_FAIL(LTX_ERR_ARG, "guidance_step_ex: nothing to write (latents, noise_pred_out and scalars_out are all null)");
    if (a.rescale_form != 0 && a.rescale_form != 1) LTX_FAIL(LTX_ERR_ARG, "guidance_step_ex: unknown rescale_form " + std::to_string(a.rescale_form) + " (0 = LTX_RESCALE_CFG, 1 = LTX_RESCALE_MIX)");
    if (a.cfg_star != 0 && a.cfg_star != 1) LTX_FAIL(LTX_ERR_ARG, "guidance_step_ex: cfg_star must be 0 or 1");
    if (g.step_noise && !g.latents) LTX_FAIL(LTX_ERR_ARG, "guidance_step_ex: the stochastic update needs latents");
    if (g.hold && (g.num_frames < 1 || g.frame_elems < 1 || (int64_t)g.num_frames * g.frame_elems != g.n_per_batch))
        LTX_FAIL(LTX_ERR_ARG, "guidance_step_ex (held): n must equal num_frames * frame_elems");
    if (!a.ws || ((uintptr_t)a.ws & 15)) LTX_FAIL(LTX_ERR_ARG, "guidance_step_ex: a 16-byte aligned workspace of ltx_guidance_ws_bytes(B, n) is required");
    const bool bf = g.pred_dtype == LTX_DT_BF16;
    const uintptr_t pa = bf ? 7 : 15;
    const int vec = !((uintptr_t)g.text & pa) && !((uintptr_t)g.uncond & pa) && !((uintptr_t)g.pert & pa) &&
                    !((uintptr_t)g.latents & 15) && !((uintptr_t)g.noise_out & 15) && !((uintptr_t)g.step_noise & 15);
    const bool use_alpha = a.cfg_star && g.uncond;
    const bool resc = a.rescale_form == 0 ? (g.uncond && g.guidance_rescale > 0.0f) : (g.pert && g.guidance_rescale != 1.0f);
    const bool need = use_alpha || resc;
    const int nblk = moments_blocks(g.n_per_batch);
    double* part = reinterpret_cast<double*>(a.ws);
    float* scal = reinterpret_cast<float*>(part + (size_t)g.B * nblk * MOM_N);
    if (need) {
        const bool with_pert = a.rescale_form == 1 && g.pert;
        if (bf) launch_moments<bf16_t>(g, with_pert, vec, nblk, part, s); else launch_moments<float>(g, with_pert, vec, nblk, part, s);
        LTX_CHECK_LAUNCH();
    }
    if (need || a.scalars_out) {
        // c in front of the rescale = at t + au alpha u + ap p
        float at = g.uncond ? g.guidance_scale : 1.0f, au = g.uncond ? 1.0f - g.guidance_scale : 0.0f, ap = 0.0f;
        if (a.rescale_form == 1 && g.pert) { at += g.stg_scale; ap = -g.stg_scale; }
        hipLaunchKernelGGL(guidance_finish_kernel, dim3((unsigned)g.B), dim3(256), 0, s, part, need ? nblk : 0, g.n_per_batch, use_alpha ? 1 : 0, resc ? 1 : 0,
                           at, au, ap, g.guidance_rescale, scal, a.scalars_out);
        LTX_CHECK_LAUNCH();
    }
    if (!g.latents && !g.noise_out) return LTX_OK;
    int64_t units = vec ? (g.n_per_batch >> 2) : g.n_per_batch; if (units < 8) units = 8;      // (the scalar rest of an aligned row is at most 6 elements)
    int64_t bx = cdiv64(units, 256); if (bx > (1 << 20)) bx = 1 << 20;
    const dim3 grid((unsigned)bx, (unsigned)g.B);
    if (bf) hipLaunchKernelGGL(guidance_apply_ex_kernel<bf16_t>, grid, dim3(256), 0, s, g, a.rescale_form, resc ? 1 : 0, vec, need ? scal : nullptr);
    else hipLaunchKernelGGL(guidance_apply_ex_kernel<float>, grid, dim3(256), 0, s, g, a.rescale_form, resc ? 1 : 0, vec, need ? scal : nullptr);
    LTX_CHECK_LAUNCH(); return LTX_OK;
}
int ltx_launch_cond_apply(float* latents, const float* cond, int Fc, const unsigned char* hold_dev, int B, int F, int64_t frame_elems, hipStream_t s) {
    if (!latents || !cond || !hold_dev || B < 1 || F < 1 || Fc < 1 || frame_elems < 1) LTX_FAIL(LTX_ERR_ARG, "cond_apply: bad argument");
    if ((int64_t)B * F > 65535) LTX_FAIL(LTX_ERR_ARG, "cond_apply: too many frames");
    const int vec = frame_elems % 4 == 0 && !((uintptr_t)latents & 15) && !((uintptr_t)cond & 15);
    int64_t bx = cdiv64(vec ? frame_elems >> 2 : frame_elems, 256); if (bx > 256) bx = 256;
    hipLaunchKernelGGL(cond_apply_kernel, dim3((unsigned)bx, (unsigned)(B * F)), dim3(256), 0, s, latents, cond, Fc, hold_dev, F, frame_elems, vec);
    LTX_CHECK_LAUNCH(); return LTX_OK;
}
namespace {
// the x extent of the two keyframe kernels: one thread per unit of a group, refused where a grid cannot hold it
int cond_grid_x(int64_t group_elems, int vec, unsigned* bx) {
    const int64_t n = cdiv64(vec ? group_elems >> 2 : group_elems, 256);
    if (n > 0x7fffffffLL) LTX_FAIL(LTX_ERR_ARG, "keyframe conditioning: group too large");
    *bx = (unsigned)n; return LTX_OK;
}
}  // namespace
int ltx_launch_cond_place(float* latents, const CondPlaceEntry* entries, int n, int B, int G, int64_t group_elems, hipStream_t s) {
    if (!latents || (n > 0 && !entries) || n < 0 || B < 1 || B > 65535 || G < 1 || group_elems < 1) LTX_FAIL(LTX_ERR_ARG, "cond_place: bad argument");
    int vec = group_elems % 4 == 0 && !((uintptr_t)latents & 15);
    for (int e = 0; e < n; ++e) {
        if (!entries[e].src || entries[e].group < 0 || entries[e].group >= G || !(entries[e].strength >= 0.0f && entries[e].strength <= 1.0f))
            LTX_FAIL(LTX_ERR_ARG, "cond_place: bad table entry " + std::to_string(e));
        vec = vec && !((uintptr_t)entries[e].src & 15) && entries[e].src_batch_stride % 4 == 0;
    }
    unsigned bx = 0; LTX_TRY(cond_grid_x(group_elems, vec, &bx));
    CondPlaceTab tab;
    for (int e0 = 0; e0 < n; ) {
        int m = 0;
        for (; e0 < n && m < LTX_COND_TAB; ++e0) {
            if (entries[e0].strength == 0.0f) continue;             // the noise's bits stay
            tab.group[m] = entries[e0].group; tab.strength[m] = entries[e0].strength; tab.src[m] = entries[e0].src; tab.src_batch_stride[m] = entries[e0].src_batch_stride; ++m;
        }
        if (!m) continue;
        hipLaunchKernelGGL(cond_place_kernel, dim3(bx, (unsigned)m, (unsigned)B), dim3(256), 0, s, latents, tab, G, group_elems, vec);
        LTX_CHECK_LAUNCH();
    }
    return LTX_OK;
}
int ltx_launch_cond_noise(float* latents, const float* clean, const float* noise, const int* groups, int n, int B, int G, int64_t group_elems, float k, hipStream_t s) {
    if (!latents || !clean || !noise || (n > 0 && !groups) || n < 0 || B < 1 || B > 65535 || G < 1 || group_elems < 1) LTX_FAIL(LTX_ERR_ARG, "cond_noise: bad argument");
    for (int e = 0; e < n; ++e) if (groups[e] < 0 || groups[e] >= G) LTX_FAIL(LTX_ERR_ARG, "cond_noise: group " + std::to_string(groups[e]) + " outside the sequence");
    const int vec = group_elems % 4 == 0 && !((uintptr_t)latents & 15) && !((uintptr_t)clean & 15) && !((uintptr_t)noise & 15);
    unsigned bx = 0; LTX_TRY(cond_grid_x(group_elems, vec, &bx));
    CondGroupTab tab;
    for (int e0 = 0; e0 < n; e0 += LTX_COND_TAB) {
        const int m = n - e0 < LTX_COND_TAB ? n - e0 : LTX_COND_TAB;
        for (int e = 0; e < m; ++e) tab.group[e] = groups[e0 + e];
        hipLaunchKernelGGL(cond_noise_kernel, dim3(bx, (unsigned)m, (unsigned)B), dim3(256), 0, s, latents, clean, noise, tab, G, group_elems, k, vec);
        LTX_CHECK_LAUNCH();
    }
    return LTX_OK;
}
int ltx_launch_group_gather(float* dst, int64_t dst_stride, const float* src, int64_t src_stride, const int* idx_host, int c0, int nc, int nl, int ngroups, int width, hipStream_t s) {
    if (!dst || !src || !idx_host || nc < 1 || nl < 1 || ngroups < 1 || width < 4 || width % 4 || dst_stride % 4 || src_stride % 4 || ((uintptr_t)dst & 15) || ((uintptr_t)src & 15))
        LTX_FAIL(LTX_ERR_ARG, "group_gather: bad argument");
    for (int g0 = 0; g0 < ngroups; g0 += 128) {
        GroupIdx gi; const int ng = ngroups - g0 < 128 ? ngroups - g0 : 128;
        bool any = false;
        for (int g = 0; g < 128; ++g) { gi.v[g] = g < ng ? idx_host[g0 + g] : -1; any = any || (g < ng && gi.v[g] >= c0 && gi.v[g] < c0 + nc); }
        if (!any) continue;
        hipLaunchKernelGGL(group_gather_kernel, grid_for((int64_t)nl * ng * (width / 4)), dim3(256), 0, s, dst, dst_stride, src, src_stride, gi, g0, ng, c0, nc, nl, width / 4);
        LTX_CHECK_LAUNCH();
    }
    return LTX_OK;
}
int ltx_launch_denorm_mix(const float* lat, const float* mean, const float* std_dev, float inv_sf, const float* noise,
                          const TimeVec& nscale, void* out, int dtype, int B, int64_t S, int C, hipStream_t s) {
    hipLaunchKernelGGL(denorm_mix_kernel, grid_for((int64_t)B * S * C), dim3(256), 0, s, lat, mean, std_dev, inv_sf, noise, nscale, out, dtype, B, S, C);
    LTX_CHECK_LAUNCH(); return LTX_OK;
}
int ltx_launch_ncthw_to_cl(const void* x, int xdt, void* y, int ydt, int B, int C, int64_t S, hipStream_t s) {
    hipLaunchKernelGGL(ncthw_to_cl_kernel, grid_for((int64_t)B * S * C), dim3(256), 0, s, x, xdt, y, ydt, B, C, S);
    LTX_CHECK_LAUNCH(); return LTX_OK;
}
int ltx_launch_blend(const BlendArgs& a, hipStream_t s) {
    if (a.blend <= 0 || a.et <= 0 || a.eh <= 0 || a.ew <= 0) return LTX_OK;
    BlendArgs b = a;
    b.inv_blend = 1.0f / (float)a.blend;
    hipLaunchKernelGGL(blend_kernel, grid_for((int64_t)a.BC * a.et * a.eh * a.ew), dim3(256), 0, s, b);
    LTX_CHECK_LAUNCH(); return LTX_OK;
}
int ltx_launch_copy_window(const float* src, int t, int h, int w, float* dst, int T, int H, int W, int BC,
                           int st, int sh, int sw, int ot, int oh, int ow, hipStream_t s) {
    hipLaunchKernelGGL(copy_window_kernel, grid_for((int64_t)BC * st * sh * sw), dim3(256), 0, s, src, t, h, w, dst, T, H, W, BC, st, sh, sw, ot, oh, ow);
    LTX_CHECK_LAUNCH(); return LTX_OK;
}
int ltx_launch_postprocess(float* x, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(postprocess_kernel, grid_for(n), dim3(256), 0, s, x, n);
    LTX_CHECK_LAUNCH(); return LTX_OK;
}
