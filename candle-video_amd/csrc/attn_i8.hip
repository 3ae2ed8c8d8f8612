// Self-attention with an int8 Q K^T on v_mfma_i32_32x32x32_i8 (include/ltxhip_int8_attn.h states the arithmetic): Q and K arrive
// quantised (quant_qk_i8.hip: q8 per (token, head), k8 per (head, block of 64 keys) after the per-channel mean of K is taken out),
// the score product is an exact int32, P V stays bf16 x bf16 -> f32 as in attention.hip.
//
// Split (attn_bf16_kernel's): workgroup = 4 waves = 128 queries of one head, wave = 32 queries, KV tile = 64 keys = ONE scale block
// of k8, so the score scale of a tile is qs[query] * ks[tile]: one product per lane and tile.  1-D grid, whole heads per XCD where
// heads % 8 == 0.
//
// Score stage.  S^T[key][query] = K8 . Q8^T: A = 32 keys x 32 bytes of head dim, B = 32 queries x 32 bytes, lane (r, h) holds bytes
// 32 ks + 16 h .. + 16 of row r of either operand (both operands use the same byte -> k map, so the sum does not depend on the
// instruction's order of k inside a step).  head_dim 64: two instructions per 32 x 32 block, 128: four - half of 32x32x16_bf16.
// The accumulator's layout is the bf16 kernel's (register i of lane (r, h) = key (i & 3) + 8 (i >> 2) + 4 h, query r): a lane owns
// one query column, the row maximum is 32 registers and one exchange with lane ^ 32, and it is taken on the INTEGERS (the scale of
// a tile is one non-negative factor per lane, so max and scale commute; v_max3_i32).  An int32 accumulator cannot start at -m: the
// running maximum enters where the score is converted, x = fma(float(acc), qs * ks, -m), one v_cvt_f32_i32 and one fma per score,
// then p = exp2(x).  The maximum is exact: O and l are rescaled whenever a lane's maximum moves (no threshold, no first-tile guess).
//
// Staging.  K tile: 64 rows x head_dim BYTES (4 KiB / 8 KiB, half the bf16 tile), V tile: 64 rows x head_dim bf16 (8 / 16 KiB), both
// global -> LDS with buffer_load ... lds (1-KiB pieces, lane-linear LDS image) into a ring of THREE tiles; tile t + 2 is in flight
// while t is multiplied, one barrier per tile.  LDS: head_dim 64: 3 x 12 KiB = 36 KiB, three blocks per CU (108 of 160 KiB);
// head_dim 128: 3 x 24 KiB = 72 KiB, two blocks per CU (144 KiB) - the int8 K tile is what lets the 128 form keep three tiles where
// the bf16 kernel holds two.  A K piece is 16 rows (head_dim 64, one per wave) or 8 rows (128, two per wave); the chunk swizzle of
// the tile (kswz<4> / kswz<8>, attn_common.h: 64-byte rows put four rows on one 256-byte bank line, so the chunk is XOR-ed with
// (row / 4) % 4) is an involution and is applied to the SOURCE chunk.  Rows past Sk are outside the buffer descriptors and read as
// zeros; the last, partial tile masks them again (-inf before the exp, left out of the maximum).  ks[tile] is one scalar load.
// All LDS reads are asm (ds_read_b128, ds_read_b64_tr_b16) with explicit lgkmcnt waits: a plain LDS load makes the wait-count pass
// drain every LDS-DMA in flight.  The ring slot is a scalar added to the lane's base addresses once per tile.
//
// P V stage: attention.hip's - P rounded pairwise to bf16 is the B operand, V^T comes through ds_read_b64_tr_b16, f32 accumulation.
// l is summed in f32 from the unrounded p.  Output: 16-byte stores (store_o_wide) where the rows are aligned; no load follows a store.
//
// Compiler remarks (-Rpass-analysis=kernel-resource-usage, gfx950, this file's flags), designed for and got:
//   attn_i8_kernel<64>:  139 VGPRs, 0 AGPRs, no scratch, no spills, LDS 36864 bytes, occupancy 3 waves per SIMD (three blocks per CU)
//   attn_i8_kernel<128>: 225 VGPRs, 0 AGPRs, no scratch, no spills, LDS 73728 bytes, occupancy 2 waves per SIMD (two blocks per CU)
#include "attn_common.h"
#include "kernels.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

template <int OFF> __device__ __forceinline__ i32x4 ds_read16(uint32_t addr) {
    i32x4 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}
template <int N> __device__ __forceinline__ void lds_wait1(i32x4& a) { asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a) : "n"(N)); }
// s_waitcnt vmcnt(N) alone, as the builtin: the wait-count pass reads it, so it knows the loads in front of the DMA (the Q fragments)
// have landed and adds no vmcnt wait of its own inside the loop
template <int N> __device__ __forceinline__ void vm_wait() { __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8)); }

template <int HD>
__global__ __launch_bounds__(256, HD == 64 ? 3 : 2) void attn_i8_kernel(const AttnI8Args a) {
    constexpr int KROW = HD, VROW = HD * 2;                  // bytes per LDS row
    constexpr int KCPR = KROW / 16, VCPR = VROW / 16;        // 16-byte chunks per row
    constexpr int NKS = HD / 32;                             // k-steps of the int8 MFMA over the head dim
    constexpr int NDB = HD / 32;                             // 32-row d blocks of O^T
    constexpr int K_BYTES = BKV * KROW, TILE_BYTES = BKV * (KROW + VROW), NBUF = 3;
    constexpr int KRPP = 1024 / KROW, VRPP = 1024 / VROW;    // rows per 1-KiB DMA piece
    constexpr int PWK = (BKV / KRPP) / 4, PWV = (BKV / VRPP) / 4;      // pieces per wave and tile: 1 + 2 (head_dim 64), 2 + 4 (128)
    constexpr int INFLIGHT = PWK + PWV;                      // DMA instructions of one tile
    __shared__ __attribute__((aligned(16))) unsigned char smem[NBUF * TILE_BYTES];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    int head, b, qb;
    {
        const int nqb = (a.Sq + BQ - 1) / BQ, per_b = nqb * a.heads;
        int L = blockIdx.x;
        b = L / per_b; L -= b * per_b;
        if (a.xcd_heads) { const int xcd = L & 7, j = L >> 3; head = xcd + 8 * (j / nqb); qb = j % nqb; }
        else { head = L / nqb; qb = L - head * nqb; }
    }
    const int D = a.heads * HD, nt = (a.Sk + BKV - 1) / BKV;
    const int q0 = qb * BQ + wave * 32;
    const unsigned char* K8 = reinterpret_cast<const unsigned char*>(a.k8) + (int64_t)b * a.Sk * D + head * HD;
    const bf16_t* V = reinterpret_cast<const bf16_t*>(a.v) + (int64_t)b * a.Sk * a.ldv + head * HD;
    // ks is read-only for the whole launch: through the constant address space the per-tile scale is ONE scalar load (a plain load is
    // a vector load here - the kernel also writes memory - and the wait for it would drain the LDS-DMA of the tiles in flight)
    const __attribute__((address_space(4))) float* KS = (const __attribute__((address_space(4))) float*)(uintptr_t)(a.ks + ((int64_t)b * a.heads + head) * nt);

    // Q^T operand fragments and the query's scale, once per wave
    i32x4 qf[NKS];
    float qs;
    {
        int qr = q0 + r; if (qr > a.Sq - 1) qr = a.Sq - 1;
        const unsigned char* qp = reinterpret_cast<const unsigned char*>(a.q8) + ((int64_t)b * a.Sq + qr) * D + head * HD + 16 * h;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) qf[ks] = *reinterpret_cast<const i32x4*>(qp + 32 * ks);
        qs = a.qs[((int64_t)b * a.heads + head) * a.Sq + qr];
    }

    // ---- DMA staging: lane -> row lane / CPR of the piece, physical chunk lane % CPR, which holds the logical chunk swz(row, .)
    __amdgpu_buffer_rsrc_t rk_rsrc, rv_rsrc;
    uint32_t k_voff[PWK], v_voff[PWV];
    {
        const uint32_t k_bytes = (uint32_t)(a.Sk - 1) * (uint32_t)D + HD;
        const uint32_t v_bytes = (uint32_t)(a.Sk - 1) * (uint32_t)a.ldv * 2u + HD * 2u;
        rk_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(K8), 0, (int)k_bytes, 0x00020000);
        rv_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(V), 0, (int)v_bytes, 0x00020000);
#pragma unroll
        for (int j = 0; j < PWK; ++j) {
            const int row = (wave * PWK + j) * KRPP + lane / KCPR, pc = lane % KCPR;
            k_voff[j] = (uint32_t)row * (uint32_t)D + (uint32_t)kswz<KCPR>(row, pc) * 16u;
        }
#pragma unroll
        for (int j = 0; j < PWV; ++j) {
            const int row = (wave * PWV + j) * VRPP + lane / VCPR, pc = lane % VCPR;
            v_voff[j] = (uint32_t)row * (uint32_t)a.ldv * 2u + (uint32_t)vswz<VCPR>(row, pc) * 16u;
        }
    }
    auto dma_tile = [&](int t, int buf) {
        unsigned char* Ks = smem + buf * TILE_BYTES;
        unsigned char* Vs = Ks + K_BYTES;
        const uint32_t ko = (uint32_t)t * BKV * (uint32_t)D, vo = (uint32_t)t * BKV * (uint32_t)a.ldv * 2u;
#pragma unroll
        for (int j = 0; j < PWK; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rk_rsrc, (__attribute__((address_space(3))) void*)(Ks + (wave * PWK + j) * 1024), 16, (int)k_voff[j], (int)ko, 0, 0);
#pragma unroll
        for (int j = 0; j < PWV; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rv_rsrc, (__attribute__((address_space(3))) void*)(Vs + (wave * PWV + j) * 1024), 16, (int)v_voff[j], (int)vo, 0, 0);
    };
    dma_tile(0, 0);
    if (nt > 1) { dma_tile(1, 1); vm_wait<INFLIGHT>(); } else vm_wait<0>();
    __builtin_amdgcn_s_barrier();

    // lane parts of the LDS read addresses: rows r and r + 32 swizzle alike (32 rows are a whole number of swizzle periods), so the
    // key block, the V row offsets and the k-step sit in the instructions' immediates; the ring slot is added per tile
    const uint32_t smem_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    uint32_t k_base[NKS], tr_base[NDB];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) k_base[ks] = smem_base + r * KROW + kswz<KCPR>(r, 2 * ks + h) * 16;
    {
        // tr-read lane geometry (attention.hip): 16-lane group g = lane >> 4 -> (h = g >> 1, d-half = g & 1)
        const int trq = (lane & 15) >> 2, trp = lane & 3, trdh = (lane >> 4) & 1;
#pragma unroll
        for (int d = 0; d < NDB; ++d) {
            const int row = 4 * h + trq, cv = d * 4 + trdh * 2 + (trp >> 1);
            tr_base[d] = smem_base + K_BYTES + row * VROW + vswz<VCPR>(row, cv) * 16 + (trp & 1) * 8;
        }
    }

    f32x16 acc_o[NDB];
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc_o[d][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    auto tile_body = [&](int t, auto masked_tag) {
        constexpr bool MASKED = decltype(masked_tag)::value;
        const int buf = t % NBUF;
        if (t + 2 < nt) dma_tile(t + 2, (t + 2) % NBUF);
        const float sc = qs * KS[t];                                    // the tile's score scale for this lane's query (log2 units)
        const uint32_t slot = (uint32_t)buf * TILE_BYTES;

        // ---- S^T = K8 . Q8^T: all operand reads of the tile issued, each MFMA waits for its own
        constexpr int NRD = 2 * NKS;
        i32x4 kf[NRD];
        static_for<0, NRD>([&](auto n_tag) {
            constexpr int n = decltype(n_tag)::value, kb = n / NKS, ks = n % NKS;
            kf[n] = ds_read16<kb * 32 * KROW>(k_base[ks] + slot);
        });
        i32x16 sacc[2];
        static_for<0, NRD>([&](auto n_tag) {
            constexpr int n = decltype(n_tag)::value, kb = n / NKS, ks = n % NKS;
            lds_wait1<NRD - 1 - n>(kf[n]);
            if constexpr (ks == 0) {
#pragma unroll
                for (int i = 0; i < 16; ++i) sacc[kb][i] = 0;
            }
            sacc[kb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(kf[n], qf[ks], sacc[kb], 0, 0, 0);
        });
        // V^T operands: a rolling window of four MFMA operands (16 registers), the first four issued ahead of the softmax
        constexpr int NSTEP = NDB * 4;                                  // step n = d*4 + kb*2 + s
        u32x2 vr[4][2];
        auto issue = [&](auto n_tag) {
            constexpr int n = decltype(n_tag)::value, d = n >> 2, j = n & 3;
            constexpr int imm = ((j >> 1) * 32 + (j & 1) * 16) * VROW;
            vr[j][0] = ds_tr_read<imm>(tr_base[d] + slot);
            vr[j][1] = ds_tr_read<imm + 8 * VROW>(tr_base[d] + slot);
        };
        static_for<0, 4>([&](auto n_tag) { issue(n_tag); });

        // ---- tile maximum per query column, on the integers; keys past Sk (last tile) are left out
        if constexpr (MASKED) {
            const int kv0 = t * BKV;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (kv0 + kb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h >= a.Sk) sacc[kb][i] = INT32_MIN;
        }
        int mi = max(sacc[0][0], sacc[1][0]);
#pragma unroll
        for (int i = 1; i < 16; ++i) mi = max(max(mi, sacc[0][i]), sacc[1][i]);
        {
            auto sw = __builtin_amdgcn_permlane32_swap((unsigned)mi, (unsigned)mi, false, false);
            mi = max((int)sw[0], (int)sw[1]);
        }
        const float mt = (float)mi * sc;                                // the largest score of the tile as the convert step forms it
        if (!__all(mt <= m_run)) {                                      // some query's maximum moves: rescale (alpha = 1 for the others)
            const float m_new = fmaxf(m_run, mt);
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);  // first tile: exp2(-inf) = 0 on zeros
            m_run = m_new;
            l_run *= alpha;
#pragma unroll
            for (int d = 0; d < NDB; ++d)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc_o[d][i] *= alpha;
        }
        // ---- p = exp2(float(acc) * sc - m): convert + fma + exp per score; P rounded pairwise to bf16 is the P V operand
        const float nm = -m_run;
        float ls = 0.f;
        bf16x8 pf[2][2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                float x = __builtin_fmaf((float)sacc[kb][i], sc, nm);
                if constexpr (MASKED) { if (sacc[kb][i] == INT32_MIN) x = -INFINITY; }
                const float p = __builtin_amdgcn_exp2f(x);
                ls += p;
                pf[kb][i >> 3][i & 7] = (bf16_t)p;
            }
        l_run += ls;
        // ---- O^T += V^T . P^T
        static_for<0, NSTEP>([&](auto n_tag) {
            constexpr int n = decltype(n_tag)::value, d = n >> 2, j = n & 3;
            constexpr int after = (NSTEP - 1 - n < 3 ? NSTEP - 1 - n : 3) * 2;
            lds_wait<after>(vr[j][0], vr[j][1]);
            union { u32x2 u[2]; bf16x8 v; } cvt;
            cvt.u[0] = vr[j][0]; cvt.u[1] = vr[j][1];
            acc_o[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cvt.v, pf[j >> 1][j & 1], acc_o[d], 0, 0, 0);
            if constexpr (n + 4 < NSTEP) issue(std::integral_constant<int, n + 4>{});
        });
        // tile t + 1 must have landed for every wave; tile t + 2's pieces may stay in flight
        if (t + 2 < nt) vm_wait<INFLIGHT>(); else vm_wait<0>();
        __builtin_amdgcn_s_barrier();
    };
    for (int t = 0; t < nt - 1; ++t) tile_body(t, std::false_type{});
    if (a.Sk % BKV) tile_body(nt - 1, std::true_type{}); else tile_body(nt - 1, std::false_type{});

    const float l_tot = l_run + __shfl_xor(l_run, 32);
    const float inv = 1.0f / l_tot;
    const int qr = q0 + r;
    if (qr < a.Sq) {
        bf16_t* O = reinterpret_cast<bf16_t*>(a.o) + ((int64_t)b * a.Sq + qr) * a.ldo + head * HD;
        if (a.wide_o) store_o_wide<NDB>(acc_o, inv, O, h); else store_o_narrow<NDB>(acc_o, inv, O, h);
    }
}

}  // namespace

int ltx_launch_attention_i8(const AttnI8Args& a, hipStream_t s) {
    if (!a.q8 || !a.qs || !a.k8 || !a.ks || !a.v || !a.o) LTX_FAIL(LTX_ERR_ARG, "attention_i8: null tensor");
    if (a.B < 1 || a.Sq < 1 || a.Sk < 1 || a.heads < 1) LTX_FAIL(LTX_ERR_ARG, "attention_i8: empty problem");
    if (a.hd != 64 && a.hd != 128) LTX_FAIL(LTX_ERR_UNSUPPORTED, "attention_i8: head_dim must be 64 or 128");
    const int64_t D = (int64_t)a.heads * a.hd;
    if (a.ldv < D || a.ldo < D) LTX_FAIL(LTX_ERR_ARG, "attention_i8: ldv and ldo must hold heads * head_dim");
    if (((uintptr_t)a.q8 & 15) || ((uintptr_t)a.k8 & 15) || ((uintptr_t)a.v & 15) || ((uintptr_t)a.o & 7) || ((uintptr_t)a.qs & 3) || ((uintptr_t)a.ks & 3) || a.ldv % 8 || a.ldo % 4)
        LTX_FAIL(LTX_ERR_ARG, "attention_i8: misaligned pointer (q8, k8, v: 16 bytes with ldv % 8 == 0; o: 8 bytes with ldo % 4 == 0)");
    const int64_t lim = (int64_t)1 << 31;
    if ((int64_t)a.B * a.Sq * D >= lim || (int64_t)a.B * a.Sk * D >= lim || (int64_t)a.B * a.Sk * a.ldv * 2 >= lim || (int64_t)a.B * a.Sq * a.ldo * 2 >= lim)
        LTX_FAIL(LTX_ERR_UNSUPPORTED, "attention_i8: an operand of 2 GiB or more");
    AttnI8Args ax = a;
    ax.xcd_heads = a.heads % 8 == 0 ? 1 : 0;
    ax.wide_o = (a.ldo % 8 == 0 && ((uintptr_t)a.o & 15) == 0) ? 1 : 0;
    void* tok = nullptr;
    ltx_prof_begin(LTX_PROF_ATTN_SELF, 4.0 * a.B * a.heads * (double)a.Sq * a.Sk * a.hd, s, &tok);
    const dim3 grid((unsigned)(cdiv(a.Sq, BQ) * a.heads * a.B)), block(256);
    if (a.hd == 64) LTX_LAUNCH_TIMED(attn_i8_kernel<64>, grid, block, 0, s, ax);
    else LTX_LAUNCH_TIMED(attn_i8_kernel<128>, grid, block, 0, s, ax);
    ltx_prof_end(tok, s);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}
