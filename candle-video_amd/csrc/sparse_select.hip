// Device-built block maps for the block-sparse self-attention (include/ltxhip_sparse_dynamic.h states the arithmetic; attn_sparse.hip
// walks the maps): the pooled means of q' and k, and the selection of key tiles per (batch row, head, 128-query block).
//
//  pool_qk       : ONE launch, one HBM pass over q and k (kmean's scheme, quant_qk_i8.hip).  Grid (NQB + NKT, ceil(heads * hd / 8 / 64), B):
//                  a block is one wave, its lanes own 64 consecutive 16-byte chunks of the heads * hd row of ONE 128-query block (x < NQB)
//                  or ONE 64-key tile - a lane owns exactly one chunk, so every load is issued before the first store.  The block's rows are
//                  added in ascending order into eight f32 registers, sixteen loads in flight; a row past the block adds +0.  One division
//                  by float(rows), two 16-byte stores to qbar / kbar [b][head][block][d].  No atomics: the order is a function of S alone.
//  sparse_select : ONE launch, one wave per map row (b, h, qb), four waves (four consecutive qb of one head) per workgroup.
//                  LDS: one chunk of 64 tiles x hd f32 of the head's kbar (16 / 32 KiB; 16-byte units XOR-swizzled by row & 15, so the
//                  ds_read_b128 of sixteen lanes that each walk their own row hit 64 distinct banks), staged once per workgroup and chunk by
//                  all 256 threads; behind it one strip of ceil64(NKT) f32 per wave.  The wave's qbar row sits in registers (hd of them,
//                  the same in every lane).  Lane l owns tiles l, l + 64, ...:
//                    1. per chunk s^ = FMA chain over d ascending -> the wave's strip; the lane keeps a running maximum, one butterfly at
//                       the end (a maximum does not depend on the order);
//                    2. p^ = w_kt * exp2(s^ - max) over the strip in place (v_exp_f32), zeros from NKT up to the strip's end;
//                    3. the rank loop, four owned tiles a pass (static registers): for j = 0 .. NKT - 1 every lane reads p^_j from the SAME
//                       LDS address (four j a ds_read_b128: a broadcast, no bank conflict), adds it to T - so T is the plain ascending sum,
//                       the same in every lane, no butterfly - and to before_i of each owned tile that j precedes.  NKT^2 compares per row;
//                    4. one ballot of (before_i < mass * T) per owned chunk = two map words; mass >= 1, the diagonal and the keep words
//                       (constant address space: scalar loads) are OR-ed in as wave-uniform 64-bit masks, bits at or above NKT cleared;
//                       lanes 0 and 1 store the two words, the popcounts add up to count.
//                  No matrix instruction: the pooled product is NQB x NKT x hd per head, 128 x 64 = 8192 times below the attention's, and the
//                  selection needs f32 scores in a stated order that a reference can bound.
// Dynamic LDS: 64 * hd * 4 + 4 * ceil64(NKT) * 4 bytes, 64 KiB at hd 128 and NKT 2048 - the limit S <= 131072.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int PQ_INFLIGHT = 16;

struct PoolArgs { const bf16_t* q; const bf16_t* k; float* qbar; float* kbar; int S, heads, hd, ldq, ldk, nqb, nkt; };

__global__ __launch_bounds__(64) void pool_qk_kernel(const PoolArgs a) {
    const int c = blockIdx.y * 64 + threadIdx.x, b = blockIdx.z, nch = a.heads * a.hd / 8;
    if (c >= nch) return;
    const bool isq = (int)blockIdx.x < a.nqb;
    const int blk = isq ? (int)blockIdx.x : (int)blockIdx.x - a.nqb, rows = isq ? 128 : 64, ld = isq ? a.ldq : a.ldk, nblk = isq ? a.nqb : a.nkt;
    const int r0 = blk * rows, nr = min(rows, a.S - r0);
    const bf16_t* src = (isq ? a.q : a.k) + ((int64_t)b * a.S + r0) * ld + c * 8;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (int j0 = 0; j0 < nr; j0 += PQ_INFLIGHT) {
        Chunk16 v[PQ_INFLIGHT];
#pragma unroll
        for (int i = 0; i < PQ_INFLIGHT; ++i) {
            v[i].u = (u32x4){0u, 0u, 0u, 0u};                          // a row past the block adds +0: the sum is unchanged
            if (j0 + i < nr) v[i].u = *reinterpret_cast<const u32x4*>(src + (int64_t)(j0 + i) * ld);
        }
#pragma unroll
        for (int i = 0; i < PQ_INFLIGHT; ++i) {
            float f[8]; chunk_to_f32<bf16_t>(v[i], f);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += f[e];
        }
    }
    const float n = (float)nr;
    const int head = c * 8 / a.hd, d = c * 8 % a.hd;
    float* dst = (isq ? a.qbar : a.kbar) + (((int64_t)b * a.heads + head) * nblk + blk) * a.hd + d;
    *reinterpret_cast<f32x4*>(dst) = (f32x4){acc[0] / n, acc[1] / n, acc[2] / n, acc[3] / n};
    *reinterpret_cast<f32x4*>(dst + 4) = (f32x4){acc[4] / n, acc[5] / n, acc[6] / n, acc[7] / n};
}

typedef const __attribute__((address_space(4))) uint32_t* keep_ptr;

struct SelectArgs { const float* qbar; const float* kbar; const uint32_t* keep; uint32_t* map; uint32_t* count; int S, heads, nqb, nkt, nw, keep_heads; float mass; };

template <int HD>
__global__ __launch_bounds__(256) void sparse_select_kernel(const SelectArgs a) {
    constexpr int UPR = HD / 4;                                          // 16-byte units per kbar row
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nkt64 = (a.nkt + 63) & ~63, nchunk = nkt64 >> 6;
    float* const kt_s = reinterpret_cast<float*>(smem);
    float* const strip = reinterpret_cast<float*>(smem + 64 * HD * 4) + wave * nkt64;
    int b, h, qb;
    {
        const int ngrp = (a.nqb + 3) >> 2;
        int L = blockIdx.x;
        qb = (L % ngrp) * 4 + wave; L /= ngrp;
        h = L % a.heads; b = L / a.heads;
    }
    const bool active = qb < a.nqb;                                      // a wave behind the last row walks row NQB - 1 again (the barriers stay uniform) and stores nothing
    if (!active) qb = a.nqb - 1;
    float qr[HD];
    {
        const float* qp = a.qbar + (((int64_t)b * a.heads + h) * a.nqb + qb) * HD;
#pragma unroll
        for (int u = 0; u < UPR; ++u) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(qp + 4 * u);
#pragma unroll
            for (int e = 0; e < 4; ++e) qr[4 * u + e] = v[e];
        }
    }
    // ---- 1. pooled scores, chunk by chunk through LDS
    const float* kb = a.kbar + ((int64_t)b * a.heads + h) * a.nkt * HD;
    float mx = -INFINITY;
    for (int c = 0; c < nchunk; ++c) {
        const int valid = min(64, a.nkt - c * 64);
        __syncthreads();                                                 // the chunk before this one has been read by every wave
        for (int u = tid; u < 64 * UPR; u += 256) {
            const int row = u / UPR, cu = u % UPR;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (row < valid) v = *reinterpret_cast<const f32x4*>(kb + (int64_t)(c * 64 + row) * HD + cu * 4);
            *reinterpret_cast<f32x4*>(kt_s + row * HD + ((cu ^ (row & 15)) << 2)) = v;
        }
        __syncthreads();
        float s = 0.f;
#pragma unroll
        for (int u = 0; u < UPR; ++u) {
            const f32x4 kv = *reinterpret_cast<const f32x4*>(kt_s + lane * HD + ((u ^ (lane & 15)) << 2));
#pragma unroll
            for (int e = 0; e < 4; ++e) s = __builtin_fmaf(qr[4 * u + e], kv[e], s);
        }
        if (lane >= valid) s = -INFINITY;
        strip[c * 64 + lane] = s;
        mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    // ---- 2. p^ in place (a lane reads back what it wrote)
    for (int c = 0; c < nchunk; ++c) {
        const int i = c * 64 + lane;
        const float w = (i == a.nkt - 1 && (a.S & 63)) ? (float)(a.S & 63) : 64.f;
        strip[i] = i < a.nkt ? w * __builtin_amdgcn_exp2f(strip[i] - mx) : 0.f;
    }
    __syncthreads();
    // ---- 3. and 4.
    const keep_ptr KR = (keep_ptr)(uintptr_t)(a.keep ? a.keep + ((int64_t)(a.keep_heads > 1 ? h : 0) * a.nqb + qb) * a.nw : nullptr);
    uint32_t* MR = a.map + (((int64_t)b * a.heads + h) * a.nqb + qb) * a.nw;
    uint32_t cnt = 0;
    for (int c0 = 0; c0 < nchunk; c0 += 4) {
        float pi[4], bef[4]; int ii[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { ii[u] = (c0 + u) * 64 + lane; pi[u] = c0 + u < nchunk ? strip[ii[u]] : 0.f; bef[u] = 0.f; }
        float T = 0.f;
        for (int j = 0; j < nkt64; j += 4) {
            const f32x4 pj = *reinterpret_cast<const f32x4*>(strip + j);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                T += pj[e];                                              // the strip's tail holds +0
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool pre = pj[e] > pi[u] || (pj[e] == pi[u] && j + e < ii[u]);
                    bef[u] += pre ? pj[e] : 0.f;
                }
            }
        }
        const float thr = a.mass * T;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = c0 + u;
            if (c >= nchunk) break;
            unsigned long long bal = a.mass >= 1.0f ? ~0ull : __ballot(bef[u] < thr);
            if (((2 * qb) >> 6) == c) bal |= 3ull << ((2 * qb) & 63);
            if (KR) { bal |= (unsigned long long)KR[2 * c]; if (2 * c + 1 < a.nw) bal |= (unsigned long long)KR[2 * c + 1] << 32; }
            const int valid = a.nkt - c * 64;
            if (valid < 64) bal &= (1ull << valid) - 1ull;
            cnt += (uint32_t)__builtin_popcountll(bal);
            if (active && lane == 0) MR[2 * c] = (uint32_t)bal;
            if (active && lane == 1 && 2 * c + 1 < a.nw) MR[2 * c + 1] = (uint32_t)(bal >> 32);
        }
    }
    if (active && lane == 0) a.count[((int64_t)b * a.heads + h) * a.nqb + qb] = cnt;
}

}  // namespace

int ltx_launch_pool_qk(const void* q, const void* k, float* qbar, float* kbar, int B, int S, int heads, int hd, int ldq, int ldk, hipStream_t s) {
    if (!q || !k || !qbar || !kbar) LTX_FAIL(LTX_ERR_ARG, "pool_qk: null tensor");
    if (B < 1 || S < 1 || heads < 1) LTX_FAIL(LTX_ERR_ARG, "pool_qk: empty problem");
    if (hd != 64 && hd != 128) LTX_FAIL(LTX_ERR_UNSUPPORTED, "pool_qk: head_dim must be 64 or 128 (got " + std::to_string(hd) + ")");
    const int64_t D = (int64_t)heads * hd;
    if (ldq < D || ldk < D) LTX_FAIL(LTX_ERR_ARG, "pool_qk: ldq and ldk must hold heads * head_dim");
    if (ldq % 8 || ldk % 8 || ((uintptr_t)q & 15) || ((uintptr_t)k & 15) || ((uintptr_t)qbar & 15) || ((uintptr_t)kbar & 15))
        LTX_FAIL(LTX_ERR_ARG, "pool_qk: misaligned pointer (q, k, qbar, kbar: 16 bytes, ldq % 8 == 0, ldk % 8 == 0)");
    if (B > 65535) LTX_FAIL(LTX_ERR_UNSUPPORTED, "pool_qk: more than 65535 batch rows");
    PoolArgs a{reinterpret_cast<const bf16_t*>(q), reinterpret_cast<const bf16_t*>(k), qbar, kbar, S, heads, hd, ldq, ldk, cdiv(S, 128), cdiv(S, 64)};
    const dim3 grid((unsigned)(a.nqb + a.nkt), (unsigned)cdiv((int)(D / 8), 64), (unsigned)B);
    void* tok = nullptr;
    ltx_prof_begin(LTX_PROF_ROWNORM, 4.0 * (double)B * S * D, s, &tok);
    LTX_LAUNCH_TIMED(pool_qk_kernel, grid, dim3(64), 0, s, a);
    ltx_prof_end(tok, s);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}

int ltx_launch_sparse_select(const float* qbar, const float* kbar, const uint32_t* keep, int keep_heads, uint32_t* map, uint32_t* count,
                             int B, int S, int heads, int hd, float mass, hipStream_t s) {
    if (!qbar || !kbar || !map || !count) LTX_FAIL(LTX_ERR_ARG, "sparse_select: null tensor");
    if (B < 1 || S < 1 || heads < 1) LTX_FAIL(LTX_ERR_ARG, "sparse_select: empty problem");
    if (!(mass > 0.f && mass <= 1.f)) LTX_FAIL(LTX_ERR_ARG, "sparse_select: mass must be in (0, 1] (got " + std::to_string(mass) + ")");
    if (hd != 64 && hd != 128) LTX_FAIL(LTX_ERR_UNSUPPORTED, "sparse_select: head_dim must be 64 or 128 (got " + std::to_string(hd) + ")");
    if (S > 131072) LTX_FAIL(LTX_ERR_UNSUPPORTED, "sparse_select: S above 131072 (got " + std::to_string(S) + "): a map row of more than 2048 key tiles");
    if (keep && keep_heads != 1 && keep_heads != heads)
        LTX_FAIL(LTX_ERR_ARG, "sparse_select: keep_heads must be 1 or heads (got " + std::to_string(keep_heads) + " with " + std::to_string(heads) + " heads)");
    if (((uintptr_t)qbar & 15) || ((uintptr_t)kbar & 15) || ((uintptr_t)map & 3) || ((uintptr_t)count & 3) || ((uintptr_t)keep & 3))
        LTX_FAIL(LTX_ERR_ARG, "sparse_select: misaligned pointer (qbar, kbar: 16 bytes; map, count, keep: 4 bytes)");
    SelectArgs a{qbar, kbar, keep, map, count, S, heads, cdiv(S, 128), cdiv(S, 64), 0, keep_heads, mass};
    a.nw = cdiv(a.nkt, 32);
    const int64_t blocks = (int64_t)B * heads * cdiv(a.nqb, 4);
    if (blocks > INT32_MAX) LTX_FAIL(LTX_ERR_UNSUPPORTED, "sparse_select: more than 2^31 workgroups");
    const size_t lds = (size_t)64 * hd * 4 + (size_t)4 * ((a.nkt + 63) & ~63) * 4;
    void* tok = nullptr;
    ltx_prof_begin(LTX_PROF_ROWNORM, 4.0 * (double)B * heads * ((double)a.nqb + a.nkt) * hd, s, &tok);
    if (hd == 64) LTX_LAUNCH_TIMED(sparse_select_kernel<64>, dim3((unsigned)blocks), dim3(256), lds, s, a);
    else LTX_LAUNCH_TIMED(sparse_select_kernel<128>, dim3((unsigned)blocks), dim3(256), lds, s, a);
    ltx_prof_end(tok, s);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}
