// The latent upsampler and the two-pass pipeline call (include/ltxhip_upsampler.h; parity reference tests/latent_upsampler_ref.py).
//
// Layout: activations are channels-last in the model dtype like the VAE's, but carry one all-zero GUARD FRAME at each end of T:
// [B, F + 2, H, W, C].  The tuned conv kernels replicate-pad T by clamping the frame index (pad_t = 1); over a tensor whose first
// and last frame are zero the clamp reads zeros, so the replicate-padded conv over F + 2 frames IS the zero-padded conv on frames
// 1 .. F - without a change to any conv kernel.  The conv's output in the two guard frames is garbage (it saw frame 1 / F twice):
// every kernel that follows a conv here (GroupNorm apply, pixel shuffle) writes zeros there before the next conv reads them.
// Cost: 2 / (F + 2) extra conv work.
//   GroupNorm      two kernels, no atomics: per-(sample, slab of voxels) partials (n, mean, M2) over the non-guard frames - each lane
//                  keeps one 16-byte channel chunk, sums shifted by its first value, lanes of a group merged through LDS in a fixed
//                  order - then an elementwise pass that merges the slabs (Chan's formula, fixed order) in its prologue and applies
//                  normalise + affine (+ residual) (+ SiLU), zeros to the guard frames
//   pixel shuffle  upsampler.0 (a per-frame Conv2d) runs as a 27-tap conv whose off-centre temporal taps are zero (3x the work on one
//                  conv out of 4 n + 3), output channels permuted at load so that a sub-pixel's channels are contiguous; one kernel
//                  moves 16-byte chunks to (2h + p1, 2w + p2) and zeroes the guards
//   the temporal and spatiotemporal kinds (ltxhip_upsampler_st.h): upsampler.0 is a true Conv3d there, and its shuffle crosses T with a
//                  dropped first frame.  The conv's epilogue (EPI_D2S_G, kernels.h) writes the guarded [B, Fo + 2, Ho, Wo, mid] tensor
//                  directly - value, zero (the output's guard frames) or nothing per conv voxel and sub-pixel - so there is neither a
//                  shuffle kernel nor a zeroing pass; the spatial kind keeps its kernels (and its bits)
//   token side     unpack + de-normalise into the guarded layout, normalise + pack out of it, AdaIN (slab partials, merge, apply),
//                  re-noise
#include <algorithm>
#include <cstring>
#include <set>
#include "conv3d.h"
#include "../host/weight_list.h"
#include "../../include/ltxhip_upsampler_st.h"
#include "../../include/ltxhip_weights.h"
#include "../../include/ltxhip_guidance.h"

namespace {

struct Stat { float n, mean, m2; };
// Chan et al.: statistics of the union of two disjoint sets
__host__ __device__ __forceinline__ void stat_merge(Stat& a, const Stat& b) {
    if (b.n == 0.f) return;
    if (a.n == 0.f) { a = b; return; }
    const float n = a.n + b.n, d = b.mean - a.mean;
    a.mean += d * (b.n / n);
    a.m2 += b.m2 + d * d * (a.n * b.n / n);
    a.n = n;
}
// sums of (x - k) and (x - k)^2 with k one of the values: no cancellation beyond the spread of the data
__device__ __forceinline__ Stat stat_from_shifted(float cnt, float k, float s1, float s2) {
    Stat r{cnt, 0.f, 0.f};
    if (cnt > 0.f) { r.mean = k + s1 / cnt; r.m2 = fmaxf(s2 - s1 * s1 / cnt, 0.f); }
    return r;
}

__device__ __forceinline__ float ld_el(const void* p, int dt, int64_t i) { return dt == LTX_DT_BF16 ? (float)reinterpret_cast<const bf16_t*>(p)[i] : reinterpret_cast<const float*>(p)[i]; }
__device__ __forceinline__ void st_el(void* p, int dt, int64_t i, float v) { if (dt == LTX_DT_BF16) reinterpret_cast<bf16_t*>(p)[i] = (bf16_t)v; else reinterpret_cast<float*>(p)[i] = v; }

inline dim3 up_grid(int64_t n) { return dim3(ltx_grid1d(n, 65536)); }
#define UP_STRIDE(i, n) for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

// ------------------------------------------------------------------------------------------------ GroupNorm
struct GnGeom {
    int B, F, HW, C, groups, g;      // g: guard frames at each end (0 / 1)
    int nslab, SL;                   // slabs per sample, voxel rows per slab
    __host__ __device__ int64_t V() const { return (int64_t)F * HW; }
};
constexpr int kGnMaxThreads = 1024;

// vector path: blockDim.x = R * CPR (CPR = chunks per voxel row), thread = (row r of the iteration, chunk cc)
template <typename T>
__global__ void gn_stats_vec_kernel(const T* __restrict__ x, GnGeom q, float* __restrict__ part) {
    constexpr int CH = ElemTraits<T>::CHUNK;
    __shared__ Stat sh[kGnMaxThreads];
    const int CPR = q.C / CH, R = blockDim.x / CPR;
    const int tid = threadIdx.x, cc = tid % CPR, r0 = tid / CPR;
    const int slab = blockIdx.x, b = blockIdx.y;
    const int64_t V = q.V();
    const int64_t v0 = (int64_t)slab * q.SL, v1 = v0 + q.SL < V ? v0 + q.SL : V;
    const T* base = x + ((int64_t)b * (q.F + 2 * q.g) + q.g) * q.HW * q.C + (int64_t)cc * CH;
    float k = 0.f, s1 = 0.f, s2 = 0.f, cnt = 0.f;
    for (int64_t v = v0 + r0; v < v1; v += R) {
        Chunk16 c; c.u = *reinterpret_cast<const u32x4*>(base + v * q.C);
        float f[CH]; chunk_to_f32<T>(c, f);
        if (cnt == 0.f) k = f[0];
#pragma unroll
        for (int i = 0; i < CH; ++i) { const float d = f[i] - k; s1 += d; s2 += d * d; }
        cnt += (float)CH;
    }
    sh[tid] = stat_from_shifted(cnt, k, s1, s2);
    __syncthreads();
    const int cpgc = (q.C / q.groups) / CH;      // chunks per group
    for (int g = tid; g < q.groups; g += blockDim.x) {
        Stat a{0.f, 0.f, 0.f};
        for (int r = 0; r < R; ++r)
            for (int j = 0; j < cpgc; ++j) stat_merge(a, sh[r * CPR + g * cpgc + j]);
        float* o = part + (((int64_t)b * q.nslab + slab) * q.groups + g) * 3;
        o[0] = a.n; o[1] = a.mean; o[2] = a.m2;
    }
}

// plain path: one block per (slab, sample, group), 256 threads over the slab's rows x channels of the group
__global__ void gn_stats_plain_kernel(const void* __restrict__ x, int dt, GnGeom q, float* __restrict__ part) {
    __shared__ Stat sh[256];
    const int tid = threadIdx.x, slab = blockIdx.x, b = blockIdx.y, g = blockIdx.z;
    const int cpg = q.C / q.groups;
    const int64_t V = q.V();
    const int64_t v0 = (int64_t)slab * q.SL, v1 = v0 + q.SL < V ? v0 + q.SL : V;
    const int64_t base = ((int64_t)b * (q.F + 2 * q.g) + q.g) * q.HW * q.C + (int64_t)g * cpg;
    const int64_t ne = (v1 - v0) * cpg;
    float k = 0.f, s1 = 0.f, s2 = 0.f, cnt = 0.f;
    for (int64_t e = tid; e < ne; e += 256) {
        const float f = ld_el(x, dt, base + (v0 + e / cpg) * q.C + e % cpg);
        if (cnt == 0.f) k = f;
        const float d = f - k; s1 += d; s2 += d * d; cnt += 1.f;
    }
    sh[tid] = stat_from_shifted(cnt, k, s1, s2);
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {      // fixed tree
        if (tid < w) stat_merge(sh[tid], sh[tid + w]);
        __syncthreads();
    }
    if (tid == 0) {
        float* o = part + (((int64_t)b * q.nslab + slab) * q.groups + g) * 3;
        o[0] = sh[0].n; o[1] = sh[0].mean; o[2] = sh[0].m2;
    }
}

// the apply kernels' prologue: slabs of sample b merged per group in a fixed order -> mean / rstd in LDS (groups <= 256, 256 threads)
__device__ __forceinline__ void gn_finish_stats(const float* __restrict__ part, const GnGeom& q, int b, float eps, Stat* sh, float* smean, float* srstd) {
    const int tid = threadIdx.x;
    const int J = q.groups <= 32 ? 8 : (q.groups <= 128 ? 2 : 1);
    if (tid < q.groups * J) {
        const int g = tid / J, j = tid % J;
        Stat a{0.f, 0.f, 0.f};
        for (int sl = j; sl < q.nslab; sl += J) {
            const float* o = part + (((int64_t)b * q.nslab + sl) * q.groups + g) * 3;
            stat_merge(a, Stat{o[0], o[1], o[2]});
        }
        sh[tid] = a;
    }
    __syncthreads();
    if (tid < q.groups) {
        Stat a = sh[tid * J];
        for (int j = 1; j < J; ++j) stat_merge(a, sh[tid * J + j]);
        smean[tid] = a.mean;
        srstd[tid] = 1.0f / sqrtf(a.m2 / a.n + eps);
    }
    __syncthreads();
}

constexpr int kGnChunksPerBlock = 256 * 8;
template <typename T>
__global__ void gn_apply_vec_kernel(const T* x, T* y, const T* resid, const T* __restrict__ gamma,
                                    const T* __restrict__ beta, GnGeom q, const float* __restrict__ part, float eps, int act) {
    constexpr int CH = ElemTraits<T>::CHUNK;
    __shared__ Stat sh[256];
    __shared__ float smean[256], srstd[256];
    const int b = blockIdx.y;
    gn_finish_stats(part, q, b, eps, sh, smean, srstd);
    const int CPR = q.C / CH, cpg = q.C / q.groups, Ft = q.F + 2 * q.g;
    const int64_t TC = (int64_t)Ft * q.HW * CPR;
    const int64_t c0 = (int64_t)blockIdx.x * kGnChunksPerBlock;
    const int64_t c1 = c0 + kGnChunksPerBlock < TC ? c0 + kGnChunksPerBlock : TC;
    const int64_t sbase = (int64_t)b * Ft * q.HW * q.C;
    for (int64_t idx = c0 + threadIdx.x; idx < c1; idx += 256) {
        const int64_t row = idx / CPR; const int cc = (int)(idx - row * CPR);
        const int frame = (int)(row / q.HW);
        const int64_t off = sbase + idx * CH;
        Chunk16 o;
        if (q.g && (frame == 0 || frame == Ft - 1)) { o.u = (u32x4){0u, 0u, 0u, 0u}; }
        else {
            Chunk16 cx, cg, cb; cx.u = *reinterpret_cast<const u32x4*>(x + off);
            cg.u = *reinterpret_cast<const u32x4*>(gamma + cc * CH); cb.u = *reinterpret_cast<const u32x4*>(beta + cc * CH);
            float f[CH], ga[CH], be[CH], rr[CH];
            chunk_to_f32<T>(cx, f); chunk_to_f32<T>(cg, ga); chunk_to_f32<T>(cb, be);
            if (resid) { Chunk16 cr; cr.u = *reinterpret_cast<const u32x4*>(resid + off); chunk_to_f32<T>(cr, rr); }
            const int g = (cc * CH) / cpg;
            const float m = smean[g], rs = srstd[g];
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                float v = (f[i] - m) * rs * ga[i] + be[i];
                if (resid) v += rr[i];
                if (act) v = silu_f(v);
                f[i] = v;
            }
            f32_to_chunk<T>(f, o);
        }
        *reinterpret_cast<u32x4*>(y + off) = o.u;
    }
}

__global__ void gn_apply_plain_kernel(const void* x, void* y, const void* resid, const void* __restrict__ gamma,
                                      const void* __restrict__ beta, int dt, GnGeom q, const float* __restrict__ part, float eps, int act) {
    __shared__ Stat sh[256];
    __shared__ float smean[256], srstd[256];
    const int b = blockIdx.y;
    gn_finish_stats(part, q, b, eps, sh, smean, srstd);
    const int cpg = q.C / q.groups, Ft = q.F + 2 * q.g;
    const int64_t TE = (int64_t)Ft * q.HW * q.C;
    const int64_t per = (int64_t)kGnChunksPerBlock * 4;
    const int64_t e0 = (int64_t)blockIdx.x * per, e1 = e0 + per < TE ? e0 + per : TE;
    const int64_t sbase = (int64_t)b * TE;
    for (int64_t idx = e0 + threadIdx.x; idx < e1; idx += 256) {
        const int64_t row = idx / q.C; const int c = (int)(idx - row * q.C);
        const int frame = (int)(row / q.HW);
        float v = 0.f;
        if (!(q.g && (frame == 0 || frame == Ft - 1))) {
            const int g = c / cpg;
            v = (ld_el(x, dt, sbase + idx) - smean[g]) * srstd[g] * ld_el(gamma, dt, c) + ld_el(beta, dt, c);
            if (resid) v += ld_el(resid, dt, sbase + idx);
            if (act) v = silu_f(v);
        }
        st_el(y, dt, sbase + idx, v);
    }
}

bool gn_geom(int B, int F, int H, int W, int C, int groups, int guards, GnGeom* q) {
    if (B < 1 || F < 1 || H < 1 || W < 1 || C < 1 || groups < 1 || groups > 256 || C % groups != 0) return false;
    if ((int64_t)H * W > 2147483647LL / 4 || (int64_t)F * H * W > (1LL << 40)) return false;
    q->B = B; q->F = F; q->HW = H * W; q->C = C; q->groups = groups; q->g = guards ? 1 : 0;
    const int64_t V = q->V();
    int64_t SL = cdiv64(V, 256); if (SL < 8) SL = 8;
    if (SL > 2147483647LL) return false;
    q->SL = (int)SL; q->nslab = (int)cdiv64(V, SL);
    return true;
}
size_t gn_part_bytes(const GnGeom& q) { return (size_t)q.B * q.nslab * q.groups * 3 * sizeof(float); }
bool gn_vec_ok(const GnGeom& q, int dt) {
    const int CH = dt == LTX_DT_BF16 ? 8 : 4;
    const int cpg = q.C / q.groups;
    return cpg % CH == 0 && q.C / CH <= kGnMaxThreads;
}

// part: >= gn_part_bytes(q) bytes of device memory
int gn_launch(int dt, const void* x, void* y, const void* resid, const void* gamma, const void* beta, const GnGeom& q, float eps, int act,
              float* part, hipStream_t s) {
    const int Ft = q.F + 2 * q.g;
    if (q.B > 65535) LTX_FAIL(LTX_ERR_ARG, "groupnorm: batch beyond 65535");
    // measurement hook (ltx_prof_report kind 4): x read by both kernels, the residual read and y written (guard frames: written only)
    void* tok = nullptr;
    ltx_prof_begin(LTX_PROF_ROWNORM, (double)q.B * q.HW * q.C * (dt == LTX_DT_BF16 ? 2 : 4) * (2.0 * q.F + (resid ? q.F : 0) + Ft), s, &tok);
    if (gn_vec_ok(q, dt)) {
        const int CH = dt == LTX_DT_BF16 ? 8 : 4, CPR = q.C / CH;
        const int R = CPR >= 256 ? 1 : 256 / CPR;
        const dim3 g1((unsigned)q.nslab, (unsigned)q.B), blk((unsigned)(R * CPR));
        const int64_t TC = (int64_t)Ft * q.HW * CPR;
        const dim3 g2((unsigned)cdiv64(TC, kGnChunksPerBlock), (unsigned)q.B);
        if (dt == LTX_DT_BF16) {
            hipLaunchKernelGGL(gn_stats_vec_kernel<bf16_t>, g1, blk, 0, s, (const bf16_t*)x, q, part);
            hipLaunchKernelGGL(gn_apply_vec_kernel<bf16_t>, g2, dim3(256), 0, s, (const bf16_t*)x, (bf16_t*)y, (const bf16_t*)resid, (const bf16_t*)gamma, (const bf16_t*)beta, q, part, eps, act);
        } else {
            hipLaunchKernelGGL(gn_stats_vec_kernel<float>, g1, blk, 0, s, (const float*)x, q, part);
            hipLaunchKernelGGL(gn_apply_vec_kernel<float>, g2, dim3(256), 0, s, (const float*)x, (float*)y, (const float*)resid, (const float*)gamma, (const float*)beta, q, part, eps, act);
        }
    } else {
        const dim3 g1((unsigned)q.nslab, (unsigned)q.B, (unsigned)q.groups);
        const int64_t TE = (int64_t)Ft * q.HW * q.C;
        const dim3 g2((unsigned)cdiv64(TE, (int64_t)kGnChunksPerBlock * 4), (unsigned)q.B);
        hipLaunchKernelGGL(gn_stats_plain_kernel, g1, dim3(256), 0, s, x, dt, q, part);
        hipLaunchKernelGGL(gn_apply_plain_kernel, g2, dim3(256), 0, s, x, y, resid, gamma, beta, dt, q, part, eps, act);
    }
    ltx_prof_end(tok, s);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}

// ------------------------------------------------------------------------------------------------ layout kernels
// upsampler.0's [O = 4 Cf, I, 3, 3] -> [27][n'][I], n' = s * Cf + c for source channel c * 4 + s; taps off the centre frame are zero
__global__ void pack_conv2d_kernel(const void* src, int sdt, void* dst, int ddt, int O, int I, int Cf) {
    const int64_t n = (int64_t)27 * O * I;
    UP_STRIDE(idx, n) {
        const int i = (int)(idx % I); const int64_t r = idx / I; const int np = (int)(r % O); const int tap = (int)(r / O);
        const int sub = np / Cf, c = np - sub * Cf, o = c * 4 + sub;
        const float v = tap / 9 == 1 ? ld_el(src, sdt, ((int64_t)o * I + i) * 9 + tap % 9) : 0.f;
        st_el(dst, ddt, idx, v);
    }
}

// y [B, Ft, 2H, 2W, C] <- x [B, Ft, H, W, 4C] (channel s * C + c, s = p1 * 2 + p2), guard frames of y zero; 16-byte chunks
template <typename T>
__global__ void pixel_shuffle_kernel(const T* __restrict__ x, T* __restrict__ y, int B, int Ft, int H, int W, int C) {
    constexpr int CH = ElemTraits<T>::CHUNK;
    const int CPR = C / CH;
    const int64_t n = (int64_t)B * Ft * (2 * H) * (2 * W) * CPR;
    UP_STRIDE(idx, n) {
        const int cc = (int)(idx % CPR); int64_t r = idx / CPR;
        const int wo = (int)(r % (2 * W)); r /= 2 * W; const int ho = (int)(r % (2 * H)); r /= 2 * H;
        const int t = (int)(r % Ft); const int64_t b = r / Ft;
        u32x4 v = (u32x4){0u, 0u, 0u, 0u};
        if (t != 0 && t != Ft - 1) {
            const int sub = (ho & 1) * 2 + (wo & 1);
            v = *reinterpret_cast<const u32x4*>(x + ((((b * Ft + t) * H + (ho >> 1)) * W + (wo >> 1)) * 4 + sub) * (int64_t)C + (int64_t)cc * CH);
        }
        *reinterpret_cast<u32x4*>(y + idx * CH) = v;
    }
}

// tokens [B, F*HW, C] f32 (normalised) -> guarded channels-last [B, F + 2, HW, C]: de-normalised as ltx_vae_prepare_latents, guards zero
__global__ void tokens_to_guarded_kernel(const float* __restrict__ tok, const float* __restrict__ mean, const float* __restrict__ sd, float inv_sf,
                                         void* __restrict__ out, int dt, int B, int F, int64_t HW, int C) {
    const int64_t n = (int64_t)B * (F + 2) * HW * C;
    UP_STRIDE(idx, n) {
        const int c = (int)(idx % C); int64_t r = idx / C; const int64_t hw = r % HW; r /= HW; const int t = (int)(r % (F + 2)); const int64_t b = r / (F + 2);
        float x = 0.f;
        if (t != 0 && t != F + 1) x = tok[((b * F + (t - 1)) * HW + hw) * C + c] * sd[c] * inv_sf + mean[c];
        st_el(out, dt, idx, x);
    }
}
// frames 1 .. F of guarded channels-last [B, F + 2, HW, C] -> tokens [B, F*HW, C] f32, normalised as ltx_vae_encode_tokens
__global__ void guarded_to_tokens_kernel(const void* __restrict__ z, int dt, const float* __restrict__ mean, const float* __restrict__ sd, float sf,
                                         float* __restrict__ tok, int B, int F, int64_t HW, int C) {
    const int64_t n = (int64_t)B * F * HW * C;
    UP_STRIDE(idx, n) {
        const int c = (int)(idx % C); int64_t r = idx / C; const int64_t hw = r % HW; r /= HW; const int f = (int)(r % F); const int64_t b = r / F;
        const float v = ld_el(z, dt, ((b * (F + 2) + f + 1) * HW + hw) * C + c);
        tok[idx] = (v - mean[c]) * sf / sd[c];
    }
}
// NCTHW [B, C, F, HW] (io dtype) <-> guarded channels-last [B, F + 2, HW, C] (model dtype)
__global__ void ncthw_to_guarded_kernel(const void* __restrict__ x, int xdt, void* __restrict__ out, int dt, int B, int F, int64_t HW, int C) {
    const int64_t n = (int64_t)B * (F + 2) * HW * C;
    UP_STRIDE(idx, n) {
        const int c = (int)(idx % C); int64_t r = idx / C; const int64_t hw = r % HW; r /= HW; const int t = (int)(r % (F + 2)); const int64_t b = r / (F + 2);
        float v = 0.f;
        if (t != 0 && t != F + 1) v = ld_el(x, xdt, ((b * C + c) * F + (t - 1)) * HW + hw);
        st_el(out, dt, idx, v);
    }
}
__global__ void guarded_to_ncthw_kernel(const void* __restrict__ z, int dt, void* __restrict__ out, int odt, int B, int F, int64_t HW, int C) {
    const int64_t n = (int64_t)B * C * F * HW;
    UP_STRIDE(idx, n) {
        const int64_t hw = idx % HW; int64_t r = idx / HW; const int f = (int)(r % F); r /= F; const int c = (int)(r % C); const int64_t b = r / C;
        st_el(out, odt, idx, ld_el(z, dt, ((b * (F + 2) + f + 1) * HW + hw) * C + c));
    }
}

// ------------------------------------------------------------------------------------------------ AdaIN / re-noise
constexpr int kAdaSlab = 64;      // tokens per slab
// partials per (sample, tensor, slab, channel): blockDim.x = R * C, thread = (token r of the iteration, channel c): the reduction axis
// runs across tokens at stride C, a wave reads consecutive channels of one token
__global__ void adain_stats_kernel(const float* __restrict__ x, const float* __restrict__ ref, int S, int S_ref, int C, int NSL, float* __restrict__ part) {
    __shared__ Stat sh[kGnMaxThreads];
    const int which = blockIdx.y, b = blockIdx.z, slab = blockIdx.x;
    const int Sn = which ? S_ref : S;
    const int64_t t0 = (int64_t)slab * kAdaSlab;
    if (t0 >= Sn) return;
    const int64_t t1 = t0 + kAdaSlab < Sn ? t0 + kAdaSlab : Sn;
    const float* p = (which ? ref : x) + (int64_t)b * Sn * C;
    const int tid = threadIdx.x, c = tid % C, r0 = tid / C, R = blockDim.x / C;
    float k = 0.f, s1 = 0.f, s2 = 0.f, cnt = 0.f;
    for (int64_t t = t0 + r0; t < t1; t += R) {
        const float f = p[t * C + c];
        if (cnt == 0.f) k = f;
        const float d = f - k; s1 += d; s2 += d * d; cnt += 1.f;
    }
    sh[tid] = stat_from_shifted(cnt, k, s1, s2);
    __syncthreads();
    if (tid < C) {
        Stat a = sh[tid];
        for (int r = 1; r < R; ++r) stat_merge(a, sh[r * C + tid]);
        float* o = part + ((((int64_t)b * 2 + which) * NSL + slab) * C + tid) * 3;
        o[0] = a.n; o[1] = a.mean; o[2] = a.m2;
    }
}
// slabs merged in ascending order -> stats[(b * C + c) * 4] = mean_x, std_x, mean_ref, std_ref (unbiased)
__global__ void adain_merge_kernel(const float* __restrict__ part, int B, int S, int S_ref, int C, int NSL, float* __restrict__ stats) {
    const int64_t n = (int64_t)B * C;
    UP_STRIDE(idx, n) {
        const int c = (int)(idx % C); const int64_t b = idx / C;
        for (int which = 0; which < 2; ++which) {
            const int ns = ((which ? S_ref : S) + kAdaSlab - 1) / kAdaSlab;
            Stat a{0.f, 0.f, 0.f};
            for (int sl = 0; sl < ns; ++sl) {
                const float* o = part + (((b * 2 + which) * NSL + sl) * C + c) * 3;
                stat_merge(a, Stat{o[0], o[1], o[2]});
            }
            stats[idx * 4 + which * 2] = a.mean;
            stats[idx * 4 + which * 2 + 1] = sqrtf(a.m2 / (a.n - 1.0f));
        }
    }
}
__global__ void adain_apply_kernel(float* __restrict__ x, const float* __restrict__ stats, int B, int64_t S, int C, float factor) {
    const int64_t n = (int64_t)B * S * C;
    UP_STRIDE(idx, n) {
        const int c = (int)(idx % C); const int64_t b = idx / ((int64_t)S * C);
        const float* st = stats + (b * C + c) * 4;
        const float v = x[idx];
        const float o = (v - st[0]) / st[1] * st[3] + st[2];
        x[idx] = v + factor * (o - v);
    }
}
__global__ void renoise_kernel(float* __restrict__ x, const float* __restrict__ noise, float sigma, int64_t n) {
    UP_STRIDE(idx, n) x[idx] = (1.0f - sigma) * x[idx] + sigma * noise[idx];
}

// ------------------------------------------------------------------------------------------------ the model
struct UpNorm { void* w = nullptr; void* b = nullptr; };
struct UpRes { ConvW c1, c2; UpNorm n1, n2; };

std::vector<std::string> up_keys(const ltx_upsampler_config& c) {
    std::vector<std::string> k;
    auto both = [&](const std::string& p) { k.push_back(p + ".weight"); k.push_back(p + ".bias"); };
    both("initial_conv"); both("initial_norm");
    for (const char* stage : {"res_blocks", "post_upsample_res_blocks"})
        for (int i = 0; i < c.num_blocks_per_stage; ++i)
            for (const char* m : {"conv1", "norm1", "conv2", "norm2"}) both(std::string(stage) + "." + std::to_string(i) + "." + m);
    both("upsampler.0"); both("final_conv");
    return k;
}

int check_cfg(const ltx_upsampler_config* c, const char* who) {
    if (!c) LTX_FAIL(LTX_ERR_ARG, std::string(who) + ": null config");
    if (c->in_channels < 8 || c->in_channels % 8 != 0 || c->in_channels > 4096) LTX_FAIL(LTX_ERR_ARG, std::string(who) + ": in_channels must be a multiple of 8");
    if (c->mid_channels < 32 || c->mid_channels % 32 != 0 || c->mid_channels > 4096) LTX_FAIL(LTX_ERR_ARG, std::string(who) + ": mid_channels must be a multiple of 32 (the GroupNorm groups)");
    if (c->num_blocks_per_stage < 0 || c->num_blocks_per_stage > 16) LTX_FAIL(LTX_ERR_ARG, std::string(who) + ": num_blocks_per_stage must be 0 .. 16");
    return LTX_OK;
}

}  // namespace

struct ltx_upsampler {
    ltx_upsampler_config cfg{};
    int sp = 1, tm = 0;              // the kind: spatial / temporal factor 2 (ltxhip_upsampler_st.h); (1, 0) is the spatial kind of ltxhip_upsampler.h
    int dtype = LTX_DT_BF16, device = 0;
    int Fo(int F) const { return tm ? 2 * F - 1 : F; }
    int So(int X) const { return sp ? 2 * X : X; }
    ConvW initial_conv, up, final_conv;
    UpNorm initial_norm;
    std::vector<UpRes> res, post;
    std::vector<void*> owned;
    DevBuf zin, X, Cb, Nb, part, zout;
    void free_all() {
        for (void* p : owned) if (p) (void)hipFree(p);
        owned.clear();
        DevBuf* bs[] = {&zin, &X, &Cb, &Nb, &part, &zout};
        for (DevBuf* b : bs) b->release();
    }
};

namespace {

constexpr int kGroups = 32;
constexpr float kGnEps = 1e-5f;

const ltx_weight* find_shaped(const WeightMap& wm, const std::string& name, std::initializer_list<int64_t> shape, int* rc) {
    const ltx_weight* w = wm.find(name);
    if (!w) { ltx_set_error("missing weight '" + name + "'"); *rc = LTX_ERR_MISSING_WEIGHT; return nullptr; }
    bool ok = w->ndim == (int)shape.size();
    int d = 0;
    for (int64_t e : shape) { if (ok && w->shape[d] != e) ok = false; ++d; }
    if (!ok) {
        std::string want, got;
        for (int64_t e : shape) want += (want.empty() ? "" : ",") + std::to_string(e);
        for (int i = 0; i < w->ndim && i < 5; ++i) got += (got.empty() ? "" : ",") + std::to_string(w->shape[i]);
        ltx_set_error("weight '" + name + "': shape [" + got + "] where the config implies [" + want + "]"); *rc = LTX_ERR_ARG; return nullptr;
    }
    if (!w->data) { ltx_set_error("weight '" + name + "': null data"); *rc = LTX_ERR_ARG; return nullptr; }
    *rc = LTX_OK;
    return w;
}

int pack_conv2d(const void* src, int sdt, void* dst, int ddt, int cout, int cin) {      // conv_upload's pack step for upsampler.0
    hipLaunchKernelGGL(pack_conv2d_kernel, up_grid((int64_t)27 * cout * cin), dim3(256), 0, 0, src, sdt, dst, ddt, cout, cin, cout / 4);
    return LTX_OK;
}

// conv2d = 1: the spatial kind's upsampler.0, [cout, cin, 3, 3] -> the 27-tap form with the sub-pixel permutation (Cf = cout / 4);
// conv2d = 2: the other kinds' upsampler.0, a Conv3d whose output channels take the same permutation (Cf = cin, nsub = cout / cin)
int load_conv(ltx_upsampler* u, const WeightMap& wm, const std::string& prefix, int cin, int cout, int conv2d, ConvW* c) {
    int rc = LTX_OK;
    const ltx_weight* w = conv2d == 1 ? find_shaped(wm, prefix + ".weight", {cout, cin, 3, 3}, &rc) : find_shaped(wm, prefix + ".weight", {cout, cin, 3, 3, 3}, &rc);
    if (!w) return rc;
    const ltx_weight* b = find_shaped(wm, prefix + ".bias", {cout}, &rc);
    if (!b) return rc;
    if (conv2d == 1) return conv_upload(u->dtype, u->owned, w, b, cin, cout, LTX_PERM_D2S, cout / 4, c, pack_conv2d);
    if (conv2d == 2) return conv_upload(u->dtype, u->owned, w, b, cin, cout, LTX_PERM_D2S, cin, c);
    return conv_upload(u->dtype, u->owned, w, b, cin, cout, LTX_PERM_NONE, 0, c);
}
int load_norm(ltx_upsampler* u, const WeightMap& wm, const std::string& prefix, int ch, UpNorm* n) {
    int rc = LTX_OK;
    if (!find_shaped(wm, prefix + ".weight", {ch}, &rc)) return rc;
    if (!find_shaped(wm, prefix + ".bias", {ch}, &rc)) return rc;
    LTX_TRY(ltx_load_tensor(wm, prefix + ".weight", ch, u->dtype, &n->w)); u->owned.push_back(n->w);
    LTX_TRY(ltx_load_tensor(wm, prefix + ".bias", ch, u->dtype, &n->b)); u->owned.push_back(n->b);
    return LTX_OK;
}
int load_res(ltx_upsampler* u, const WeightMap& wm, const std::string& prefix, int ch, UpRes* r) {
    LTX_TRY(load_conv(u, wm, prefix + ".conv1", ch, ch, 0, &r->c1)); LTX_TRY(load_norm(u, wm, prefix + ".norm1", ch, &r->n1));
    LTX_TRY(load_conv(u, wm, prefix + ".conv2", ch, ch, 0, &r->c2)); LTX_TRY(load_norm(u, wm, prefix + ".norm2", ch, &r->n2));
    return LTX_OK;
}
int up_build(ltx_upsampler* u, const ltx_weight* weights, size_t n) {
    const ltx_upsampler_config& c = u->cfg;
    WeightMap wm(weights, n);
    LTX_TRY(load_conv(u, wm, "initial_conv", c.in_channels, c.mid_channels, 0, &u->initial_conv));
    LTX_TRY(load_norm(u, wm, "initial_norm", c.mid_channels, &u->initial_norm));
    u->res.resize(c.num_blocks_per_stage); u->post.resize(c.num_blocks_per_stage);
    for (int i = 0; i < c.num_blocks_per_stage; ++i) LTX_TRY(load_res(u, wm, "res_blocks." + std::to_string(i), c.mid_channels, &u->res[i]));
    if (u->sp && !u->tm) LTX_TRY(load_conv(u, wm, "upsampler.0", c.mid_channels, 4 * c.mid_channels, 1, &u->up));
    else LTX_TRY(load_conv(u, wm, "upsampler.0", c.mid_channels, (u->sp ? 8 : 2) * c.mid_channels, 2, &u->up));
    for (int i = 0; i < c.num_blocks_per_stage; ++i) LTX_TRY(load_res(u, wm, "post_upsample_res_blocks." + std::to_string(i), c.mid_channels, &u->post[i]));
    LTX_TRY(load_conv(u, wm, "final_conv", c.mid_channels, c.in_channels, 0, &u->final_conv));
    return LTX_OK;
}

// (Dims::T of the calls below is F + 2: the guard frames are frames to the conv, which runs with pad_t = 1)
int up_gn(ltx_upsampler* u, const UpNorm& n, const void* x, void* y, const void* resid, const Dims& d, int ch, hipStream_t s) {
    GnGeom q;
    if (!gn_geom(d.B, d.T - 2, d.H, d.W, ch, kGroups, 1, &q)) LTX_FAIL(LTX_ERR_ARG, "ltx_upsampler: bad GroupNorm geometry");
    return gn_launch(u->dtype, x, y, resid, n.w, n.b, q, kGnEps, 1, u->part.as<float>(), s);
}
// norm2 has no activation of its own: silu(norm2(h) + r) is the kernel's residual form
int up_res(ltx_upsampler* u, const UpRes& r, const Dims& d, int ch, hipStream_t s) {
    LTX_TRY(conv3d(u->dtype, 1, r.c1, u->X.p, u->Cb.p, d, EPI_BIAS, nullptr, 0, s));
    LTX_TRY(up_gn(u, r.n1, u->Cb.p, u->Cb.p, nullptr, d, ch, s));
    LTX_TRY(conv3d(u->dtype, 1, r.c2, u->Cb.p, u->Nb.p, d, EPI_BIAS, nullptr, 0, s));
    return up_gn(u, r.n2, u->Nb.p, u->X.p, u->X.p, d, ch, s);
}

int up_ensure(ltx_upsampler* u, int B, int F, int H, int W) {
    const ltx_upsampler_config& c = u->cfg;
    const size_t esz = ltx_dt_size(u->dtype);
    const int64_t hi = (int64_t)B * (u->Fo(F) + 2) * u->So(H) * u->So(W);
    const size_t act = (size_t)hi * std::max(c.mid_channels, c.in_channels) * esz;
    LTX_TRY(u->X.ensure(act)); LTX_TRY(u->Cb.ensure(act)); LTX_TRY(u->Nb.ensure(act));
    LTX_TRY(u->zin.ensure((size_t)B * (F + 2) * H * W * c.in_channels * esz));
    GnGeom q;
    if (!gn_geom(B, u->Fo(F), u->So(H), u->So(W), c.mid_channels, kGroups, 1, &q)) LTX_FAIL(LTX_ERR_ARG, "ltx_upsampler: bad geometry");
    size_t pb = gn_part_bytes(q);
    if (gn_geom(B, F, H, W, c.mid_channels, kGroups, 1, &q)) pb = std::max(pb, gn_part_bytes(q));
    return u->part.ensure(pb);
}

// zin [B, F + 2, H, W, in_channels] (guards zero) -> Cb [B, Fo + 2, Ho, Wo, in_channels] (guards: garbage, not read by the callers)
int up_forward_cl(ltx_upsampler* u, int B, int F, int H, int W, hipStream_t s) {
    const ltx_upsampler_config& c = u->cfg;
    const int mid = c.mid_channels;
    Dims d{B, F + 2, H, W};
    LTX_TRY(conv3d(u->dtype, 1, u->initial_conv, u->zin.p, u->Cb.p, d, EPI_BIAS, nullptr, 0, s));
    LTX_TRY(up_gn(u, u->initial_norm, u->Cb.p, u->X.p, nullptr, d, mid, s));
    for (auto& r : u->res) LTX_TRY(up_res(u, r, d, mid, s));
    if (u->tm) {
        // conv + shuffle + dropped frame + zero guards in one launch, into the buffer that becomes the activation
        LTX_TRY(conv3d(u->dtype, 1, u->up, u->X.p, u->Nb.p, d, EPI_D2S_G, nullptr, 0, s));
        std::swap(u->X, u->Nb);
        d.T = u->Fo(F) + 2;
    } else {
    LTX_TRY(conv3d(u->dtype, 1, u->up, u->X.p, u->Cb.p, d, EPI_BIAS, nullptr, 0, s));
    {
        const int64_t n = d.vox() * 4 * (mid / (u->dtype == LTX_DT_BF16 ? 8 : 4));
        if (u->dtype == LTX_DT_BF16) hipLaunchKernelGGL(pixel_shuffle_kernel<bf16_t>, up_grid(n), dim3(256), 0, s, (const bf16_t*)u->Cb.p, (bf16_t*)u->X.p, B, d.T, H, W, mid);
        else hipLaunchKernelGGL(pixel_shuffle_kernel<float>, up_grid(n), dim3(256), 0, s, (const float*)u->Cb.p, (float*)u->X.p, B, d.T, H, W, mid);
        LTX_CHECK_LAUNCH();
    }
    }
    d.H = u->So(H); d.W = u->So(W);
    for (auto& r : u->post) LTX_TRY(up_res(u, r, d, mid, s));
    return conv3d(u->dtype, 1, u->final_conv, u->X.p, u->Cb.p, d, EPI_BIAS, nullptr, 0, s);
}

int check_shape(const char* who, const ltx_upsampler* u, int B, int F, int H, int W) {
    if (!u) LTX_FAIL(LTX_ERR_ARG, std::string(who) + ": null handle");
    if (B < 1 || F < 1 || H < 1 || W < 1) LTX_FAIL(LTX_ERR_ARG, std::string(who) + ": bad shape");
    if (F > (1 << 29) || H > (1 << 29) || W > (1 << 29)) LTX_FAIL(LTX_ERR_ARG, std::string(who) + ": shape too large");
    if ((int64_t)B * (u->Fo(F) + 2) * u->So(H) * u->So(W) * std::max(u->cfg.mid_channels, u->cfg.in_channels) > (1LL << 40)) LTX_FAIL(LTX_ERR_ARG, std::string(who) + ": shape too large");
    return LTX_OK;
}

thread_local float t_ms_timing[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};

}  // namespace

extern "C" void ltx_upsampler_config_default(ltx_upsampler_config* cfg) {
    if (!cfg) return;
    cfg->in_channels = 128; cfg->mid_channels = 512; cfg->num_blocks_per_stage = 4;
}

namespace {
// the one constructor: (sp, tm) = (1, 0) the spatial kind
int up_create(const char* who, const ltx_upsampler_config* cfg, int sp, int tm, const ltx_weight* weights, size_t n_weights,
              ltx_dtype model_dtype, int device, ltx_upsampler** out) {
    if (!out) LTX_FAIL(LTX_ERR_ARG, std::string(who) + ": null output");
    *out = nullptr;
    LTX_TRY(check_cfg(cfg, who));
    if (!weights && n_weights) LTX_FAIL(LTX_ERR_ARG, std::string(who) + ": null weights");
    HIP_TRY(hipSetDevice(device));
    ltx_upsampler* u = new ltx_upsampler();
    u->cfg = *cfg; u->sp = sp; u->tm = tm; u->dtype = model_dtype == LTX_BF16 ? LTX_DT_BF16 : LTX_DT_F32; u->device = device;
    const int rc = up_build(u, weights, n_weights);
    if (rc != LTX_OK) { u->free_all(); delete u; return rc; }
    *out = u;
    return LTX_OK;
}
int up_create_from_file(const char* who, const ltx_upsampler_config* cfg, int sp, int tm, const char* path, ltx_dtype model_dtype, int device, ltx_upsampler** out) {
    if (!out) LTX_FAIL(LTX_ERR_ARG, std::string(who) + ": null output");
    *out = nullptr;
    if (!path) LTX_FAIL(LTX_ERR_ARG, std::string(who) + ": null path");
    LTX_TRY(check_cfg(cfg, who));
    const std::vector<std::string> keys = up_keys(*cfg);
    const std::set<std::string> wanted(keys.begin(), keys.end());
    ltx_safetensors* st = nullptr;
    LTX_TRY(ltx_safetensors_open(path, &st));
    std::vector<ltx_weight> ws;      // not one of the model's tensors: ignored, as ltx_upsampler_create does
    int rc = ltx_safetensors_weight_list(st, who, [&](const char* name) { return wanted.count(name) != 0; }, &ws);
    if (rc == LTX_OK) rc = up_create(who, cfg, sp, tm, ws.data(), ws.size(), model_dtype, device, out);
    ltx_safetensors_close(st);
    return rc;
}
// -> the three-field config and the flags; both flags 0 (or a value other than 0 / 1) is refused
int split_st_cfg(const char* who, const ltx_upsampler_st_config* c, ltx_upsampler_config* base) {
    if (!c) LTX_FAIL(LTX_ERR_ARG, std::string(who) + ": null config");
    if ((c->spatial_upsample != 0 && c->spatial_upsample != 1) || (c->temporal_upsample != 0 && c->temporal_upsample != 1))
        LTX_FAIL(LTX_ERR_ARG, std::string(who) + ": spatial_upsample and temporal_upsample are 0 or 1");
    if (!c->spatial_upsample && !c->temporal_upsample) LTX_FAIL(LTX_ERR_ARG, std::string(who) + ": spatial_upsample or temporal_upsample must be set");
    base->in_channels = c->in_channels; base->mid_channels = c->mid_channels; base->num_blocks_per_stage = c->num_blocks_per_stage;
    return LTX_OK;
}
}  // namespace

extern "C" int ltx_upsampler_create(const ltx_upsampler_config* cfg, const ltx_weight* weights, size_t n_weights,
                                    ltx_dtype model_dtype, int device, ltx_upsampler** out) {
    return up_create("ltx_upsampler_create", cfg, 1, 0, weights, n_weights, model_dtype, device, out);
}

extern "C" void ltx_upsampler_st_config_default(ltx_upsampler_st_config* cfg) {
    if (!cfg) return;
    cfg->in_channels = 128; cfg->mid_channels = 512; cfg->num_blocks_per_stage = 4; cfg->spatial_upsample = 1; cfg->temporal_upsample = 0;
}
extern "C" int ltx_upsampler_create_st(const ltx_upsampler_st_config* cfg, const ltx_weight* weights, size_t n_weights,
                                       ltx_dtype model_dtype, int device, ltx_upsampler** out) {
    if (out) *out = nullptr;
    ltx_upsampler_config base;
    LTX_TRY(split_st_cfg("ltx_upsampler_create_st", cfg, &base));
    if (!cfg->temporal_upsample) return ltx_upsampler_create(&base, weights, n_weights, model_dtype, device, out);
    return up_create("ltx_upsampler_create_st", &base, cfg->spatial_upsample, 1, weights, n_weights, model_dtype, device, out);
}
extern "C" int ltx_upsampler_create_from_file_st(const ltx_upsampler_st_config* cfg, const char* path, ltx_dtype model_dtype, int device, ltx_upsampler** out) {
    if (out) *out = nullptr;
    ltx_upsampler_config base;
    LTX_TRY(split_st_cfg("ltx_upsampler_create_from_file_st", cfg, &base));
    if (!cfg->temporal_upsample) return ltx_upsampler_create_from_file(&base, path, model_dtype, device, out);
    return up_create_from_file("ltx_upsampler_create_from_file_st", &base, cfg->spatial_upsample, 1, path, model_dtype, device, out);
}
extern "C" int ltx_upsampler_get_st_config(const ltx_upsampler* u, ltx_upsampler_st_config* out) {
    if (!u || !out) LTX_FAIL(LTX_ERR_ARG, "ltx_upsampler_get_st_config: null argument");
    out->in_channels = u->cfg.in_channels; out->mid_channels = u->cfg.mid_channels; out->num_blocks_per_stage = u->cfg.num_blocks_per_stage;
    out->spatial_upsample = u->sp; out->temporal_upsample = u->tm;
    return LTX_OK;
}
extern "C" int ltx_upsampler_out_shape(const ltx_upsampler* u, int F, int H, int W, int* Fo, int* Ho, int* Wo) {
    if (!u || !Fo || !Ho || !Wo) LTX_FAIL(LTX_ERR_ARG, "ltx_upsampler_out_shape: null argument");
    if (F < 1 || H < 1 || W < 1 || F > (1 << 29) || H > (1 << 29) || W > (1 << 29)) LTX_FAIL(LTX_ERR_ARG, "ltx_upsampler_out_shape: bad shape");
    *Fo = u->Fo(F); *Ho = u->So(H); *Wo = u->So(W);
    return LTX_OK;
}

extern "C" int ltx_upsampler_create_from_file(const ltx_upsampler_config* cfg, const char* path, ltx_dtype model_dtype, int device, ltx_upsampler** out) {
    return up_create_from_file("ltx_upsampler_create_from_file", cfg, 1, 0, path, model_dtype, device, out);
}

extern "C" void ltx_upsampler_destroy(ltx_upsampler* u) {
    if (!u) return;
    (void)hipSetDevice(u->device); (void)hipDeviceSynchronize();
    u->free_all(); delete u;
}
extern "C" int ltx_upsampler_get_config(const ltx_upsampler* u, ltx_upsampler_config* out) {
    if (!u || !out) LTX_FAIL(LTX_ERR_ARG, "ltx_upsampler_get_config: null argument");
    *out = u->cfg; return LTX_OK;
}

extern "C" int ltx_upsampler_forward(ltx_upsampler* u, const void* latents, ltx_dtype io_dtype, int B, int F, int H, int W, void* out, ltx_stream stream) {
    LTX_TRY(check_shape("ltx_upsampler_forward", u, B, F, H, W));
    if (!latents || !out) LTX_FAIL(LTX_ERR_ARG, "ltx_upsampler_forward: null tensor");
    HIP_TRY(hipSetDevice(u->device));
    hipStream_t s = (hipStream_t)stream;
    LTX_TRY(up_ensure(u, B, F, H, W));
    const int C = u->cfg.in_channels, iodt = io_dtype == LTX_BF16 ? LTX_DT_BF16 : LTX_DT_F32;
    const int64_t HW = (int64_t)H * W;
    hipLaunchKernelGGL(ncthw_to_guarded_kernel, up_grid((int64_t)B * (F + 2) * HW * C), dim3(256), 0, s, latents, iodt, u->zin.p, u->dtype, B, F, HW, C);
    LTX_CHECK_LAUNCH();
    LTX_TRY(up_forward_cl(u, B, F, H, W, s));
    const int Fo = u->Fo(F); const int64_t HWo = (int64_t)u->So(H) * u->So(W);
    hipLaunchKernelGGL(guarded_to_ncthw_kernel, up_grid((int64_t)B * Fo * HWo * C), dim3(256), 0, s, (const void*)u->Cb.p, u->dtype, out, iodt, B, Fo, HWo, C);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}

extern "C" int ltx_latent_upsample_tokens(ltx_upsampler* u, const ltx_vae* vae, const float* tokens_lo, int B, int F, int H, int W,
                                          float* tokens_hi, ltx_stream stream) {
    LTX_TRY(check_shape("ltx_latent_upsample_tokens", u, B, F, H, W));
    if (!vae || !tokens_lo || !tokens_hi) LTX_FAIL(LTX_ERR_ARG, "ltx_latent_upsample_tokens: null argument");
    ltx_vae_config vc; LTX_TRY(ltx_vae_get_config(vae, &vc));
    if (vc.latent_channels != u->cfg.in_channels) LTX_FAIL(LTX_ERR_ARG, "ltx_latent_upsample_tokens: upsampler and VAE disagree on the latent channels");
    const float* mean = ltx_vae_latents_mean(vae); const float* sd = ltx_vae_latents_std(vae);
    if (!mean || !sd) LTX_FAIL(LTX_ERR_ARG, "ltx_latent_upsample_tokens: the VAE has no latent statistics");
    HIP_TRY(hipSetDevice(u->device));
    hipStream_t s = (hipStream_t)stream;
    LTX_TRY(up_ensure(u, B, F, H, W));
    const int C = u->cfg.in_channels; const int64_t HW = (int64_t)H * W;
    hipLaunchKernelGGL(tokens_to_guarded_kernel, up_grid((int64_t)B * (F + 2) * HW * C), dim3(256), 0, s, tokens_lo, mean, sd, 1.0f / vc.scaling_factor,
                       u->zin.p, u->dtype, B, F, HW, C);
    LTX_CHECK_LAUNCH();
    LTX_TRY(up_forward_cl(u, B, F, H, W, s));
    const int Fo = u->Fo(F); const int64_t HWo = (int64_t)u->So(H) * u->So(W);
    hipLaunchKernelGGL(guarded_to_tokens_kernel, up_grid((int64_t)B * Fo * HWo * C), dim3(256), 0, s, (const void*)u->Cb.p, u->dtype, mean, sd, vc.scaling_factor,
                       tokens_hi, B, Fo, HWo, C);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}

extern "C" int ltx_upsampler_warmup(ltx_upsampler* u, int B, int F, int H, int W, ltx_stream stream) {
    LTX_TRY(check_shape("ltx_upsampler_warmup", u, B, F, H, W));
    HIP_TRY(hipSetDevice(u->device));
    hipStream_t s = (hipStream_t)stream;
    LTX_TRY(up_ensure(u, B, F, H, W));
    HIP_TRY(hipMemsetAsync(u->zin.p, 0, (size_t)B * (F + 2) * H * W * u->cfg.in_channels * ltx_dt_size(u->dtype), s));
    const int rc = up_forward_cl(u, B, F, H, W, s);
    HIP_TRY(hipStreamSynchronize(s));
    return rc;
}

extern "C" int ltx_latent_adain(float* tokens, const float* ref_tokens, int B, int S, int S_ref, int C, float factor, ltx_stream stream) {
    if (!tokens || !ref_tokens) LTX_FAIL(LTX_ERR_ARG, "ltx_latent_adain: null tensor");
    if (S < 2 || S_ref < 2) LTX_FAIL(LTX_ERR_ARG, "ltx_latent_adain: the unbiased std needs at least 2 tokens");
    if (B < 1 || B > 65535 || C < 1 || C > kGnMaxThreads) LTX_FAIL(LTX_ERR_ARG, "ltx_latent_adain: bad shape (1 <= C <= 1024)");
    hipStream_t s = (hipStream_t)stream;
    const int NSL = (int)cdiv64(std::max(S, S_ref), kAdaSlab);
    DevBuf part, stats;
    struct Rel { DevBuf* a; DevBuf* b; ~Rel() { a->release(); b->release(); } } rel{&part, &stats};
    LTX_TRY(part.ensure((size_t)B * 2 * NSL * C * 3 * sizeof(float)));
    LTX_TRY(stats.ensure((size_t)B * C * 4 * sizeof(float)));
    const int R = C >= 256 ? 1 : 256 / C;
    hipLaunchKernelGGL(adain_stats_kernel, dim3((unsigned)NSL, 2, (unsigned)B), dim3((unsigned)(R * C)), 0, s, (const float*)tokens, ref_tokens, S, S_ref, C, NSL, part.as<float>());
    hipLaunchKernelGGL(adain_merge_kernel, up_grid((int64_t)B * C), dim3(256), 0, s, (const float*)part.p, B, S, S_ref, C, NSL, stats.as<float>());
    hipLaunchKernelGGL(adain_apply_kernel, up_grid((int64_t)B * S * C), dim3(256), 0, s, tokens, (const float*)stats.p, B, (int64_t)S, C, factor);
    LTX_CHECK_LAUNCH();
    HIP_TRY(hipStreamSynchronize(s));      // (the two temporaries are freed here)
    return LTX_OK;
}

extern "C" int ltx_latent_renoise(float* tokens, const float* noise, float sigma, size_t n, ltx_stream stream) {
    if (!tokens || !noise) LTX_FAIL(LTX_ERR_ARG, "ltx_latent_renoise: null tensor");
    if (!(sigma >= 0.0f && sigma <= 1.0f)) LTX_FAIL(LTX_ERR_ARG, "ltx_latent_renoise: sigma must lie in [0, 1]");
    if (n == 0) return LTX_OK;
    hipLaunchKernelGGL(renoise_kernel, up_grid((int64_t)n), dim3(256), 0, (hipStream_t)stream, tokens, noise, sigma, (int64_t)n);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}

// the first sigma of the schedule the denoise loop itself builds (ltx_pipeline_schedule, host/pipeline.hip)
extern "C" int ltx_pipeline_first_sigma(const ltx_pipeline_params* p, int S, float* sigma0) {
    if (!p || !sigma0) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_first_sigma: null argument");
    if (S < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_first_sigma: bad token count");
    std::vector<float> sig; std::vector<int64_t> ts;
    LTX_TRY(ltx_pipeline_schedule(p, S, &sig, &ts));
    *sigma0 = sig[0];
    return LTX_OK;
}

extern "C" int ltx_pipeline_multiscale_last_timing(float ms[9]) {
    if (!ms) LTX_FAIL(LTX_ERR_ARG, "null output");
    for (int i = 0; i < 9; ++i) ms[i] = t_ms_timing[i];
    return LTX_OK;
}

// one pass of the two: under its guidance schedule (include/ltxhip_guidance.h) or, without one, on its params' scalars
static int multiscale_pass(ltx_dit* dit, ltx_vae* vae, const ltx_pipeline_params* p, const ltx_guidance_schedule* sched, float* latents,
                           const float* prompt_embeds, const float* prompt_mask, const float* neg_embeds, const float* neg_mask,
                           const float* decode_noise, int B, int K, float* out_video, ltx_stream stream) {
    if (sched) return ltx_pipeline_call_sched(dit, vae, p, sched, nullptr, latents, prompt_embeds, prompt_mask, neg_embeds, neg_mask, decode_noise, B, K, out_video, stream);
    return ltx_pipeline_call(dit, vae, p, latents, prompt_embeds, prompt_mask, neg_embeds, neg_mask, decode_noise, B, K, out_video, stream);
}

extern "C" int ltx_pipeline_call_multiscale(ltx_dit* dit, ltx_vae* vae, ltx_upsampler* up,
                                            const ltx_pipeline_params* p_first, const ltx_pipeline_params* p_second, float adain_factor,
                                            float* latents_lo, const float* noise_hi,
                                            const float* prompt_embeds, const float* prompt_mask, const float* neg_embeds, const float* neg_mask,
                                            const float* decode_noise, int B, int K, float* latents_hi_out, float* out_video, ltx_stream stream) {
    return ltx_pipeline_call_multiscale_sched(dit, vae, up, p_first, p_second, nullptr, nullptr, adain_factor, latents_lo, noise_hi, prompt_embeds, prompt_mask,
                                              neg_embeds, neg_mask, decode_noise, B, K, latents_hi_out, out_video, stream);
}

extern "C" int ltx_pipeline_call_multiscale_sched(ltx_dit* dit, ltx_vae* vae, ltx_upsampler* up,
                                                  const ltx_pipeline_params* p_first, const ltx_pipeline_params* p_second,
                                                  const ltx_guidance_schedule* sched_first, const ltx_guidance_schedule* sched_second, float adain_factor,
                                                  float* latents_lo, const float* noise_hi,
                                                  const float* prompt_embeds, const float* prompt_mask, const float* neg_embeds, const float* neg_mask,
                                                  const float* decode_noise, int B, int K, float* latents_hi_out, float* out_video, ltx_stream stream) {
    if (!dit || !vae || !up || !p_first || !p_second || !latents_lo || !noise_hi || !latents_hi_out) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_multiscale: null argument");
    if (B < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_multiscale: bad batch");
    // the geometry rule follows the handle's kind (ltxhip_upsampler_st.h)
    if (up->sp) {
        if (p_second->height != 2 * p_first->height || p_second->width != 2 * p_first->width)
            LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_multiscale: the second pass must run at exactly twice the first pass's height and width");
    } else if (p_second->height != p_first->height || p_second->width != p_first->width)
        LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_multiscale: with a temporal upsampler both passes must have the same height and width");
    if (up->tm) {
        if (p_first->num_frames < 1 || p_first->num_frames > (1 << 29) || p_second->num_frames != 2 * p_first->num_frames - 1)
            LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_multiscale: with a temporal or spatiotemporal upsampler the second pass must have 2 * num_frames - 1 frames of the first");
    } else if (p_second->num_frames != p_first->num_frames) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_multiscale: both passes must have the same num_frames");
    if (p_first->height % 32 != 0 || p_first->width % 32 != 0) LTX_FAIL(LTX_ERR_ARG, "`height` and `width` must be divisible by 32");
    ltx_vae_config vc; LTX_TRY(ltx_vae_get_config(vae, &vc));
    ltx_dit_config dc; LTX_TRY(ltx_dit_get_config(dit, &dc));
    if (vc.spatial_compression_ratio < 1 || vc.temporal_compression_ratio < 1 || p_first->num_frames < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_multiscale: bad geometry");
    const int F = (p_first->num_frames - 1) / vc.temporal_compression_ratio + 1;
    const int H = p_first->height / vc.spatial_compression_ratio, W = p_first->width / vc.spatial_compression_ratio;
    if (H < 1 || W < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_multiscale: bad geometry");
    const int C = dc.in_channels;
    if (C != up->cfg.in_channels) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_multiscale: upsampler and transformer disagree on the latent channels");
    const int64_t S = (int64_t)F * H * W;
    const int Fo = up->Fo(F), Ho = up->So(H), Wo = up->So(W);
    const int64_t S_hi = (int64_t)Fo * Ho * Wo;      // 4 S for the spatial kind
    if (4 * S > 2147483647LL || S_hi > 2147483647LL) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_multiscale: too many tokens");
    // the second pass derives its own latent grid from p_second: it must be the one the upsampler writes
    if (up->tm && ((p_second->num_frames - 1) / vc.temporal_compression_ratio + 1 != Fo ||p_second->height / vc.spatial_compression_ratio != Ho ||
        p_second->width / vc.spatial_compression_ratio != Wo))
        LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_multiscale: the second pass's latent grid is not the upsampler's output (num_frames - 1 must be a multiple of the VAE's temporal compression)");
    float sigma0 = 0.f;
    LTX_TRY(ltx_pipeline_first_sigma(p_second, (int)S_hi, &sigma0));

    ltx_pipeline_params p1 = *p_first;
    p1.output_latent = 1;
    LTX_TRY(multiscale_pass(dit, vae, &p1, sched_first, latents_lo, prompt_embeds, prompt_mask, neg_embeds, neg_mask, nullptr, B, K, nullptr, stream));
    LTX_TRY(ltx_pipeline_last_timing(t_ms_timing));
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    struct Ev { hipEvent_t* a; hipEvent_t* b; ~Ev() { if (*a) (void)hipEventDestroy(*a); if (*b) (void)hipEventDestroy(*b); } } evs{&e0, &e1};
    HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0, s));
    LTX_TRY(ltx_latent_upsample_tokens(up, vae, latents_lo, B, F, H, W, latents_hi_out, stream));
    LTX_TRY(ltx_latent_adain(latents_hi_out, latents_lo, B, (int)S_hi, (int)S, C, adain_factor, stream));
    LTX_TRY(ltx_latent_renoise(latents_hi_out, noise_hi, sigma0, (size_t)B * S_hi * C, stream));
    HIP_TRY(hipEventRecord(e1, s));
    HIP_TRY(hipEventSynchronize(e1));
    HIP_TRY(hipEventElapsedTime(&t_ms_timing[4], e0, e1));
    LTX_TRY(multiscale_pass(dit, vae, p_second, sched_second, latents_hi_out, prompt_embeds, prompt_mask, neg_embeds, neg_mask, decode_noise, B, K, out_video, stream));
    return ltx_pipeline_last_timing(t_ms_timing + 5);
}

extern "C" int ltx_op_groupnorm(const void* x, void* y, const void* resid, const void* weight, const void* bias,
                                int B, int F, int H, int W, int C, int groups, float eps, int flags, int dtype, ltx_stream stream) {
    if (!x || !y || !weight || !bias) LTX_FAIL(LTX_ERR_ARG, "ltx_op_groupnorm: null tensor");
    if (flags & ~(LTX_GN_SILU | LTX_GN_GUARDS)) LTX_FAIL(LTX_ERR_ARG, "ltx_op_groupnorm: unknown flag");
    if (dtype != LTX_F32 && dtype != LTX_BF16) LTX_FAIL(LTX_ERR_ARG, "ltx_op_groupnorm: bad dtype");
    GnGeom q;
    if (!gn_geom(B, F, H, W, C, groups, (flags & LTX_GN_GUARDS) != 0, &q)) LTX_FAIL(LTX_ERR_ARG, "ltx_op_groupnorm: bad shape (C a multiple of groups, groups <= 256)");
    const int dt = dtype == LTX_BF16 ? LTX_DT_BF16 : LTX_DT_F32;
    if (gn_vec_ok(q, dt) && ((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)resid) | ((uintptr_t)weight) | ((uintptr_t)bias)) & 15))
        LTX_FAIL(LTX_ERR_ARG, "ltx_op_groupnorm: tensors must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    DevBuf part;
    struct Rel { DevBuf* a; ~Rel() { a->release(); } } rel{&part};
    LTX_TRY(part.ensure(gn_part_bytes(q)));
    LTX_TRY(gn_launch(dt, x, y, resid, weight, bias, q, eps, (flags & LTX_GN_SILU) != 0, part.as<float>(), s));
    HIP_TRY(hipStreamSynchronize(s));      // (the partials are freed here)
    return LTX_OK;
}

// the spatial kind's stand-alone shuffle pass as an op (ltxhip_upsampler_st.h): what EPI_D2S_G folds into the conv, for measurements
extern "C" int ltx_op_pixel_shuffle_guarded(const void* x, void* y, int B, int F, int H, int W, int C, int dtype, ltx_stream stream) {
    if (!x || !y) LTX_FAIL(LTX_ERR_ARG, "ltx_op_pixel_shuffle_guarded: null tensor");
    if (dtype != LTX_F32 && dtype != LTX_BF16) LTX_FAIL(LTX_ERR_ARG, "ltx_op_pixel_shuffle_guarded: bad dtype");
    const int ch = dtype == LTX_BF16 ? 8 : 4;
    if (B < 1 || F < 1 || H < 1 || W < 1 || C < ch || C % ch != 0 || F > (1 << 29) || H > (1 << 29) || W > (1 << 29) ||
        (int64_t)B * (F + 2) * (2 * H) * (2 * W) * C > (1LL << 40))
        LTX_FAIL(LTX_ERR_ARG, "ltx_op_pixel_shuffle_guarded: bad shape (C a multiple of the 16-byte chunk)");
    if ((((uintptr_t)x) | ((uintptr_t)y)) & 15) LTX_FAIL(LTX_ERR_ARG, "ltx_op_pixel_shuffle_guarded: tensors must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)B * (F + 2) * H * W * 4 * (C / ch);
    if (dtype == LTX_BF16) hipLaunchKernelGGL(pixel_shuffle_kernel<bf16_t>, up_grid(n), dim3(256), 0, s, (const bf16_t*)x, (bf16_t*)y, B, F + 2, H, W, C);
    else hipLaunchKernelGGL(pixel_shuffle_kernel<float>, up_grid(n), dim3(256), 0, s, (const float*)x, (float*)y, B, F + 2, H, W, C);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}
