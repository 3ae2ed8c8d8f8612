// The operand passes of the int8 Q K^T attention (include/ltxhip_int8_attn.h; attn_i8.hip reads their outputs).  HBM-bound.
//
//  kmean        : mean[b][c] = (1 / Sk) sum_j k[b][j][c], one HBM pass + a finish.  Pass: one block per (64-key block, batch row), a
//                 thread owns 16-byte chunks (8 channels) and adds the block's rows in ascending order into f32 (eight loads in
//                 flight): P_i[c].  Finish: one thread per channel adds the partials in eight interleaved chains, s_j = P_j + P_(j+8) +
//                 P_(j+16) + ... (ascending), and mean = (((s_0 + s_1) + (s_2 + s_3)) + ((s_4 + s_5) + (s_6 + s_7))) / float(Sk).  The
//                 order is a function of Sk alone: no atomics, the result repeats bit for bit and does not depend on D or the grid.
//  quant_qk_i8  : ONE launch, two kinds of blocks.  Q blocks: the row-owning mapping of quant_i8.hip with a row = one (token, head): hd / 8 lanes
//                 hold a row's chunks, consecutive lanes walk the token's heads (coalesced over D), four rows a lane; the scale goes
//                 to qs[b][head][token].  K blocks: one WAVE per (batch row, 64-key block, head) - the group whose maximum gives one
//                 scale - four heads a block: a lane holds hd / 8 chunks of the 64 x hd tile (32 / 64 registers), subtracts the
//                 channel means in f32, the maximum over the valid keys is a wave reduction, int8 out.  Every lane issues all its
//                 loads before its first store.
#include "common.h"
#include "kernels.h"
#include "quant_common.h"

namespace {

constexpr int KM_ROWS = 64;       // keys per partial of kmean = keys per scale block of k8 = attn_i8.hip's KV tile

__global__ __launch_bounds__(256) void kmean_part_kernel(const bf16_t* __restrict__ k, float* __restrict__ part, int Sk, int D, int ldk) {
    const int blk = blockIdx.x, b = blockIdx.y, nblk = gridDim.x, nch = D / 8;
    const int r0 = blk * KM_ROWS, nr = min(KM_ROWS, Sk - r0);
    const bf16_t* kb = k + ((int64_t)b * Sk + r0) * ldk;
    for (int c = threadIdx.x; c < nch; c += 256) {
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        for (int j0 = 0; j0 < nr; j0 += 8) {
            Chunk16 v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                v[i].u = (u32x4){0u, 0u, 0u, 0u};                      // a row past the block adds +0: the sum is unchanged
                if (j0 + i < nr) v[i].u = *reinterpret_cast<const u32x4*>(kb + (int64_t)(j0 + i) * ldk + c * 8);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float f[8]; chunk_to_f32<bf16_t>(v[i], f);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += f[e];
            }
        }
        float* p = part + ((int64_t)b * nblk + blk) * D + c * 8;
        *reinterpret_cast<f32x4*>(p) = (f32x4){acc[0], acc[1], acc[2], acc[3]};
        *reinterpret_cast<f32x4*>(p + 4) = (f32x4){acc[4], acc[5], acc[6], acc[7]};
    }
}

__global__ __launch_bounds__(256) void kmean_finish_kernel(const float* __restrict__ part, float* __restrict__ mean, int nblk, int D, int Sk) {
    const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (c >= D) return;
    const float* p = part + (int64_t)b * nblk * D + c;
    float s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = 0.f;
    for (int i0 = 0; i0 < nblk; i0 += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) if (i0 + j < nblk) s[j] += p[(int64_t)(i0 + j) * D];
    }
    mean[(int64_t)b * D + c] = (((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]))) / (float)Sk;
}

struct QuantQkArgs {
    const bf16_t* q; const bf16_t* k; const float* mean;
    unsigned char* q8; float* qs; unsigned char* k8; float* ks;
    int B, Sq, Sk, heads, ldq, ldk, nqblk, nkb;
};
constexpr int QK_QROWS = 4;       // (token, head) rows a lane of a Q block holds

template <int HD>
__global__ __launch_bounds__(256) void quant_qk_i8_kernel(const QuantQkArgs a) {
    constexpr int CPR = HD / 8;                                         // 16-byte chunks (= lanes) per row
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = a.heads * HD, nch = D / 8;
    if ((int)blockIdx.x < a.nqblk) {
        // ---- Q: chunk g of the [B * Sq, D / 8] chunk matrix; a row's CPR chunks sit in CPR consecutive lanes
        const int64_t total = (int64_t)a.B * a.Sq * nch;
        Chunk16 v[QK_QROWS];
        int64_t g[QK_QROWS];
#pragma unroll
        for (int i = 0; i < QK_QROWS; ++i) {
            g[i] = ((int64_t)blockIdx.x * QK_QROWS + i) * 256 + tid;
            const int64_t gg = g[i] < total ? g[i] : tid % CPR;         // (whole rows are in or out: total % CPR == 0)
            v[i].u = *reinterpret_cast<const u32x4*>(a.q + (gg / nch) * a.ldq + (gg % nch) * 8);
        }
        u32x2 o[QK_QROWS]; float amax[QK_QROWS];
#pragma unroll
        for (int i = 0; i < QK_QROWS; ++i) {
            float f[8]; chunk_to_f32<bf16_t>(v[i], f);
            amax[i] = group_max(absmax8(f, 0.f), CPR);
            o[i] = quant8(f, inv_of(amax[i]));
        }
#pragma unroll
        for (int i = 0; i < QK_QROWS; ++i) {
            if (g[i] >= total) continue;
            const int64_t token = g[i] / nch; const int cc = (int)(g[i] % nch);
            *reinterpret_cast<u32x2*>(a.q8 + token * D + cc * 8) = o[i];
            if (cc % CPR == 0) a.qs[((token / a.Sq) * a.heads + cc / CPR) * a.Sq + token % a.Sq] = amax[i] / 127.0f;
        }
        return;
    }
    // ---- K: wave = (batch row b, key block blk, head): 64 keys x HD channels, lane = chunk c of rows rr, rr + RPI, ...
    constexpr int RPI = 64 / CPR, NI = CPR;                             // rows per load instruction of the wave, loads per lane
    const int hgroups = (a.heads + 3) / 4;
    int id = (int)blockIdx.x - a.nqblk;
    const int head = (id % hgroups) * 4 + wave; id /= hgroups;
    const int blk = id % a.nkb, b = id / a.nkb;
    if (head >= a.heads) return;
    const int c = lane % CPR, rr = lane / CPR, key0 = blk * KM_ROWS;
    Chunk16 v[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        int key = key0 + rr + RPI * i; if (key > a.Sk - 1) key = a.Sk - 1;
        v[i].u = *reinterpret_cast<const u32x4*>(a.k + ((int64_t)b * a.Sk + key) * a.ldk + head * HD + c * 8);
    }
    float mu[8];
    {
        const float* mp = a.mean + (int64_t)b * D + head * HD + c * 8;
        const f32x4 m0 = *reinterpret_cast<const f32x4*>(mp), m1 = *reinterpret_cast<const f32x4*>(mp + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { mu[e] = m0[e]; mu[4 + e] = m1[e]; }
    }
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        float f[8]; chunk_to_f32<bf16_t>(v[i], f);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] -= mu[e];
        if (key0 + rr + RPI * i < a.Sk) amax = absmax8(f, amax);
    }
    amax = wave_max(amax);
    const float inv = inv_of(amax);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int key = key0 + rr + RPI * i;
        float f[8]; chunk_to_f32<bf16_t>(v[i], f);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] -= mu[e];
        const u32x2 o = quant8(f, inv);
        if (key < a.Sk) *reinterpret_cast<u32x2*>(a.k8 + ((int64_t)b * a.Sk + key) * D + head * HD + c * 8) = o;
    }
    if (lane == 0) a.ks[((int64_t)b * a.heads + head) * a.nkb + blk] = amax / 127.0f;
}

}  // namespace

size_t ltx_kmean_ws_bytes(int B, int Sk, int D) { return (size_t)B * (size_t)cdiv(Sk, KM_ROWS) * D * sizeof(float); }

int ltx_kmean_check(const void* k, int B, int Sk, int D, int ldk, const float* mean) {
    if (!k || !mean) LTX_FAIL(LTX_ERR_ARG, "kmean: null tensor");
    if (B < 1 || Sk < 1 || D < 1 || ldk < D) LTX_FAIL(LTX_ERR_ARG, "kmean: B, Sk, D >= 1 and ldk >= D");
    if (D % 8 != 0) LTX_FAIL(LTX_ERR_UNSUPPORTED, "kmean: D must be a multiple of 8");
    if (ldk % 8 != 0 || ((uintptr_t)k & 15) || ((uintptr_t)mean & 3)) LTX_FAIL(LTX_ERR_ARG, "kmean: misaligned pointer (k: 16 bytes, ldk % 8 == 0)");
    if ((int64_t)B * Sk * ldk * 2 >= ((int64_t)1 << 31)) LTX_FAIL(LTX_ERR_UNSUPPORTED, "kmean: an operand of 2 GiB or more");
    return LTX_OK;
}

int ltx_launch_kmean(const void* k, int B, int Sk, int D, int ldk, float* part, float* mean, hipStream_t s) {
    LTX_TRY(ltx_kmean_check(k, B, Sk, D, ldk, mean));
    if (!part || ((uintptr_t)part & 15)) LTX_FAIL(LTX_ERR_ARG, "kmean: null or misaligned workspace");
    const int nblk = cdiv(Sk, KM_ROWS);
    void* tok = nullptr;
    ltx_prof_begin(LTX_PROF_ROWNORM, 2.0 * (double)B * Sk * D, s, &tok);
    hipLaunchKernelGGL(kmean_part_kernel, dim3((unsigned)nblk, (unsigned)B), dim3(256), 0, s, reinterpret_cast<const bf16_t*>(k), part, Sk, D, ldk);
    hipLaunchKernelGGL(kmean_finish_kernel, dim3((unsigned)cdiv(D, 256), (unsigned)B), dim3(256), 0, s, part, mean, nblk, D, Sk);
    ltx_prof_end(tok, s);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}

int ltx_launch_quant_qk_i8(const void* q, const void* k, const float* mean, int B, int Sq, int Sk, int heads, int hd, int ldq, int ldk,
                           void* q8, float* qs, void* k8, float* ks, hipStream_t s) {
    if (!q || !k || !q8 || !k8) LTX_FAIL(LTX_ERR_ARG, "quant_qk_i8: null tensor");
    if (!mean || !qs || !ks) LTX_FAIL(LTX_ERR_ARG, "quant_qk_i8: null scale (mean, qs, ks)");
    if (B < 1 || Sq < 1 || Sk < 1 || heads < 1) LTX_FAIL(LTX_ERR_ARG, "quant_qk_i8: empty problem");
    if (hd != 64 && hd != 128) LTX_FAIL(LTX_ERR_UNSUPPORTED, "quant_qk_i8: head_dim must be 64 or 128");
    const int64_t D = (int64_t)heads * hd, lim = (int64_t)1 << 31;
    if (ldq < D || ldk < D) LTX_FAIL(LTX_ERR_ARG, "quant_qk_i8: ldq and ldk must hold heads * head_dim");
    if (ldq % 8 || ldk % 8 || ((uintptr_t)q & 15) || ((uintptr_t)k & 15) || ((uintptr_t)mean & 15) || ((uintptr_t)q8 & 15) || ((uintptr_t)k8 & 15) || ((uintptr_t)qs & 3) || ((uintptr_t)ks & 3))
        LTX_FAIL(LTX_ERR_ARG, "quant_qk_i8: misaligned pointer (q, k, mean, q8, k8: 16 bytes, ldq % 8 == 0, ldk % 8 == 0)");
    if ((int64_t)B * Sq * ldq * 2 >= lim || (int64_t)B * Sk * ldk * 2 >= lim) LTX_FAIL(LTX_ERR_UNSUPPORTED, "quant_qk_i8: an operand of 2 GiB or more");
    QuantQkArgs a{reinterpret_cast<const bf16_t*>(q), reinterpret_cast<const bf16_t*>(k), mean, reinterpret_cast<unsigned char*>(q8), qs,
                  reinterpret_cast<unsigned char*>(k8), ks, B, Sq, Sk, heads, ldq, ldk, 0, cdiv(Sk, KM_ROWS)};
    a.nqblk = (int)cdiv64((int64_t)B * Sq * (D / 8), 256 * QK_QROWS);
    const unsigned grid = (unsigned)a.nqblk + (unsigned)(B * a.nkb * ((heads + 3) / 4));
    void* tok = nullptr;
    ltx_prof_begin(LTX_PROF_ROWNORM, 3.0 * (double)B * ((double)Sq + Sk) * D, s, &tok);
    if (hd == 64) LTX_LAUNCH_TIMED(quant_qk_i8_kernel<64>, dim3(grid), dim3(256), 0, s, a);
    else LTX_LAUNCH_TIMED(quant_qk_i8_kernel<128>, dim3(grid), dim3(256), 0, s, a);
    ltx_prof_end(tok, s);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}
