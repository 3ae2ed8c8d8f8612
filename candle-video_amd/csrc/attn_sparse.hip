// Block-sparse self-attention (include/ltxhip_sparse_attn.h states the arithmetic and the map): flash attention whose key loop walks a
// per-query-block LIST of 64-key tiles instead of 0 .. NKT.  q' bf16 prescaled by scale * log2(e), k and v bf16, no key bias.
//
// Split and operand maps (attention.hip's header): workgroup = 4 waves = 128 queries of one head = ONE map row, wave = 32 queries,
// KV tile = 64 keys = one map bit.  Swapped S^T[key][query] = K . Q^T on v_mfma_f32_32x32x16_bf16 with -m as the initial accumulator
// (the PRE form: the accumulator comes out as s - m, p = exp2(acc)), lazy rescale (threshold 2^5, the first listed tile adopts its
// maximum: no guess, no second pass), P rounded pairwise to bf16 stays in registers as the B operand of O^T += V^T . P^T, V^T through
// ds_read_b64_tr_b16, K and V rows chunk-swizzled (attn_common.h).  1-D grid, whole heads per XCD where heads % 8 == 0.
//
// The tile walk.  The row's NW = ceil(NKT / 32) map words are read through the constant address space - one scalar load per word, the
// next word requested while the current one is walked, bits at or above NKT cleared as the last word arrives.  Everything the walk
// touches is wave-uniform, so it compiles to scalar code: s_ff1_i32_b32 finds the lowest set bit, s_and with (word - 1) clears it.  The
// index of the tile that enters the ring is resolved NBUF - 1 list entries ahead of the tile being multiplied and becomes the SCALAR
// offset of its buffer_load ... lds pieces (soffset = kt * 64 * ld * 2): the stride between two staged tiles is data-dependent, the
// per-lane offsets and the LDS image are those of a dense walk, and the ring stays as full as the list allows.  A list of 0 tiles stores
// zeros and never touches the ring; 1 and 2 tiles fill the ring partly (the waits are chosen by what was issued, not by position).
// The ragged last key tile can only be the LAST list entry (ascending order): that entry alone runs the masked body, and only when it
// is tile NKT - 1 and Sk % 64 != 0.  Rows past Sk are outside the buffer descriptors and read as zeros.
//
// Ring: head_dim 64: three 16-KiB tiles (48 KiB, three blocks per CU); head_dim 128: TWO 32-KiB tiles (64 KiB, two blocks per CU) - a
// third tile would take 96 of the CU's 160 KiB and leave one block, i.e. one wave per SIMD, with nothing to overlap the softmax of a
// wave with the MFMAs of another; the register budget (<= 256 at two blocks) is the same either way.
// All LDS reads are asm (ds_read_b128, ds_read_b64_tr_b16) with explicit lgkmcnt waits, as in attn_i8.hip: a plain LDS load makes the
// wait-count pass drain every LDS-DMA in flight.  A scalar load of the walk that is still out only makes such a wait stricter.
//
// Compiler remarks (-Rpass-analysis=kernel-resource-usage, gfx950, this file's flags), designed for and got:
//   attn_sparse_kernel<64>:  165 VGPRs, 0 AGPRs, no scratch, no spills, LDS 49152 bytes, occupancy 3 waves per SIMD (three blocks per CU)
//   attn_sparse_kernel<128>: 244 VGPRs, 0 AGPRs, no scratch, no spills, LDS 65536 bytes, occupancy 2 waves per SIMD (two blocks per CU)
#include "attn_common.h"
#include "kernels.h"

namespace {

template <int OFF> __device__ __forceinline__ u32x4 ds_read16(uint32_t addr) {
    u32x4 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}
template <int N> __device__ __forceinline__ void lds_wait1(u32x4& a) { asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a) : "n"(N)); }
// s_waitcnt vmcnt(N) alone, as the builtin (attn_i8.hip): the wait-count pass reads it and adds no vmcnt wait of its own inside the loop
template <int N> __device__ __forceinline__ void vm_wait() { __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8)); }

typedef const __attribute__((address_space(4))) uint32_t* map_ptr;

template <int HD>
__global__ __launch_bounds__(256, HD == 64 ? 3 : 2) void attn_sparse_kernel(const AttnArgs a, const uint32_t* map, int map_heads, int64_t map_bstride) {
    constexpr int KROW = HD * 2, VROW = HD * 2;              // bytes per LDS row
    constexpr int CPR = KROW / 16;                           // 16-byte chunks per row
    constexpr int NKS = HD / 16;                             // k-steps over the head dim for S^T
    constexpr int NDB = HD / 32;                             // 32-row d blocks of O^T
    constexpr int K_BYTES = BKV * KROW, TILE_BYTES = BKV * (KROW + VROW);
    constexpr int NBUF = HD == 64 ? 3 : 2;
    constexpr int RPP = 1024 / KROW;                         // rows per 1-KiB DMA piece (8 at head_dim 64, 4 at 128)
    constexpr int PW = (BKV / RPP) / 4;                      // pieces per wave per K tile (and per V tile)
    constexpr int INFLIGHT = 2 * PW;                         // DMA instructions of one tile
    __shared__ __attribute__((aligned(16))) unsigned char smem[NBUF * TILE_BYTES];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int nqb = (a.Sq + BQ - 1) / BQ, nt = (a.Sk + BKV - 1) / BKV, nw = (nt + 31) >> 5;
    int head, b, qb;
    {
        const int per_b = nqb * a.heads;
        int L = blockIdx.x;
        b = L / per_b; L -= b * per_b;
        if (a.xcd_heads) { const int xcd = L & 7, j = L >> 3; head = xcd + 8 * (j / nqb); qb = j % nqb; }
        else { head = L / nqb; qb = L - head * nqb; }
    }
    const int q0 = qb * BQ + wave * 32;
    const bf16_t* Q = reinterpret_cast<const bf16_t*>(a.q) + (int64_t)b * a.Sq * a.ldq + head * HD;
    const bf16_t* K = reinterpret_cast<const bf16_t*>(a.k) + (int64_t)b * a.Sk * a.ldk + head * HD;
    const bf16_t* V = reinterpret_cast<const bf16_t*>(a.v) + (int64_t)b * a.Sk * a.ldv + head * HD;

    // ---- the walk over this block's map row: scalar state (word index, the bits left of it, the next word already requested)
    // (map_bstride words between the maps of two batch rows - ltxhip_sparse_dynamic.h; 0: one map for the batch)
    const map_ptr MR = (map_ptr)(uintptr_t)(map + (int64_t)b * map_bstride + ((int64_t)(map_heads > 1 ? head : 0) * nqb + qb) * nw);
    auto map_word = [&](int i) -> uint32_t {
        uint32_t x = MR[i];
        if (i == nw - 1 && (nt & 31)) x &= (1u << (nt & 31)) - 1u;      // bits at or above NKT are not tiles
        return x;
    };
    int wi = 0;
    uint32_t cur = map_word(0), ahead = nw > 1 ? map_word(1) : 0u;
    auto next_tile = [&]() -> int {                          // the next listed tile in ascending order, -1 behind the last
        while (cur == 0u) {
            if (++wi >= nw) { wi = nw; return -1; }
            cur = ahead;
            ahead = wi + 1 < nw ? map_word(wi + 1) : 0u;
        }
        const int kt = wi * 32 + __builtin_ctz(cur);
        cur &= cur - 1u;
        return __builtin_amdgcn_readfirstlane(kt);
    };
    int k0 = next_tile();

    const int qr = q0 + r;
    bf16_t* O = reinterpret_cast<bf16_t*>(a.o) + ((int64_t)b * a.Sq + (qr < a.Sq ? qr : 0)) * a.ldo + head * HD;
    f32x16 acc_o[NDB];
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc_o[d][i] = 0.f;
    if (k0 < 0) {                                            // an empty row (uniform over the block): o = 0, the ring is never touched
        if (qr < a.Sq) { if (a.wide_o) store_o_wide<NDB>(acc_o, 0.f, O, h); else store_o_narrow<NDB>(acc_o, 0.f, O, h); }
        return;
    }

    // Q^T operand fragments (B operand: k = d, col = query)
    bf16x8 qf[NKS];
    {
        const bf16_t* qp = Q + (int64_t)(qr < a.Sq ? qr : a.Sq - 1) * a.ldq + 8 * h;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qp + 16 * ks);
    }

    // ---- DMA staging (attention.hip's geometry): lane -> row lane / CPR of the piece, physical chunk lane % CPR, which holds the
    // logical chunk swz(row, .); the tile enters through the scalar offset
    __amdgpu_buffer_rsrc_t rk_rsrc, rv_rsrc;
    uint32_t k_voff[PW], v_voff[PW];
    {
        const uint32_t k_bytes = (uint32_t)(a.Sk - 1) * (uint32_t)a.ldk * 2u + HD * 2u;
        const uint32_t v_bytes = (uint32_t)(a.Sk - 1) * (uint32_t)a.ldv * 2u + HD * 2u;
        rk_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(K), 0, (int)k_bytes, 0x00020000);
        rv_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(V), 0, (int)v_bytes, 0x00020000);
#pragma unroll
        for (int j = 0; j < PW; ++j) {
            const int row = (wave * PW + j) * RPP + lane / CPR, pc = lane % CPR;
            k_voff[j] = (uint32_t)row * (uint32_t)a.ldk * 2u + (uint32_t)kswz<CPR>(row, pc) * 16u;
            v_voff[j] = (uint32_t)row * (uint32_t)a.ldv * 2u + (uint32_t)vswz<CPR>(row, pc) * 16u;
        }
    }
    auto dma_tile = [&](int kt, int buf) {
        unsigned char* Ks = smem + buf * TILE_BYTES;
        unsigned char* Vs = Ks + K_BYTES;
        const uint32_t ko = (uint32_t)kt * BKV * (uint32_t)a.ldk * 2u, vo = (uint32_t)kt * BKV * (uint32_t)a.ldv * 2u;
#pragma unroll
        for (int j = 0; j < PW; ++j) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rk_rsrc, (__attribute__((address_space(3))) void*)(Ks + (wave * PW + j) * 1024), 16, (int)k_voff[j], (int)ko, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rv_rsrc, (__attribute__((address_space(3))) void*)(Vs + (wave * PW + j) * 1024), 16, (int)v_voff[j], (int)vo, 0, 0);
        }
    };
    // ring prologue: the first listed tile, and - three-tile ring - the second where there is one
    dma_tile(k0, 0);
    int k1 = next_tile();
    if (NBUF == 3 && k1 >= 0) { dma_tile(k1, 1); vm_wait<INFLIGHT>(); } else vm_wait<0>();
    __builtin_amdgcn_s_barrier();

    // lane parts of the LDS read addresses: rows r and r + 32 swizzle alike, so the key block, the V row offsets and the k-step sit in
    // the instructions' immediates; the ring slot is added per tile
    const uint32_t smem_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    uint32_t k_base[NKS], tr_base[NDB];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) k_base[ks] = smem_base + r * KROW + kswz<CPR>(r, 2 * ks + h) * 16;
    {
        // tr-read lane geometry (attention.hip): 16-lane group g = lane >> 4 -> (h = g >> 1, d-half = g & 1)
        const int trq = (lane & 15) >> 2, trp = lane & 3, trdh = (lane >> 4) & 1;
#pragma unroll
        for (int d = 0; d < NDB; ++d) {
            const int row = 4 * h + trq, cv = d * 4 + trdh * 2 + (trp >> 1);
            tr_base[d] = smem_base + K_BYTES + row * VROW + vswz<CPR>(row, cv) * 16 + (trp & 1) * 8;
        }
    }

    float m_run = 0.f, l_run = 0.f;                          // m_run: a placeholder until the first listed tile sets it
    f32x16 minit;                                            // initial accumulator of the S^T chains: -m_run
#pragma unroll
    for (int i = 0; i < 16; ++i) minit[i] = 0.f;
    constexpr float RESCALE_THR = 5.0f;

    // one listed tile, staged in ring slot buf.  first: the row's first listed tile; MASKED: tile NKT - 1 of a ragged Sk
    auto tile_body = [&](int kt, int buf, bool first, auto masked_tag) {
        constexpr bool MASKED = decltype(masked_tag)::value;
        const uint32_t slot = (uint32_t)buf * TILE_BYTES;
        // ---- S^T = K . Q^T (two 32-key blocks), accumulators start at -m_run; a rolling window of eight operand reads
        constexpr int NRD = 2 * NKS, WIN = 8;
        u32x4 kf[WIN];
        auto issue_k = [&](auto n_tag) {
            constexpr int n = decltype(n_tag)::value, kb = n / NKS, ks = n % NKS;
            kf[n % WIN] = ds_read16<kb * 32 * KROW>(k_base[ks] + slot);
        };
        static_for<0, WIN>([&](auto n_tag) { issue_k(n_tag); });
        f32x16 sacc[2];
        static_for<0, NRD>([&](auto n_tag) {
            constexpr int n = decltype(n_tag)::value, kb = n / NKS, ks = n % NKS;
            constexpr int last = n + WIN - 1 < NRD - 1 ? n + WIN - 1 : NRD - 1;      // the youngest read issued so far
            lds_wait1<last - n>(kf[n % WIN]);
            union { u32x4 u; bf16x8 v; } cvt;
            cvt.u = kf[n % WIN];
            if constexpr (ks == 0) sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cvt.v, qf[ks], minit, 0, 0, 0);
            else sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cvt.v, qf[ks], sacc[kb], 0, 0, 0);
            if constexpr (n + WIN < NRD) issue_k(std::integral_constant<int, n + WIN>{});
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

        if constexpr (MASKED) {
            const int kv0 = kt * BKV;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (kv0 + kb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h >= a.Sk) sacc[kb][i] = -INFINITY;
        }
        // ---- tile maximum per query column, RELATIVE to m_run (in-register over 32 scores, then across the two lane halves)
        float mt = fmaxf(sacc[0][0], sacc[1][0]);
#pragma unroll
        for (int i = 1; i < 16; ++i) mt = fmaxf(fmaxf(mt, sacc[0][i]), sacc[1][i]);
        {
            const unsigned mu = __float_as_uint(mt);
            auto sw = __builtin_amdgcn_permlane32_swap(mu, mu, false, false);
            mt = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
        }
        if (first || !__all(mt <= RESCALE_THR)) {                       // first listed tile: adopt its maximum unconditionally
            const float delta = first ? mt : fmaxf(mt, 0.f);
            const float alpha = first ? 1.0f : __builtin_amdgcn_exp2f(-delta);
            m_run += delta;
            l_run *= alpha;
#pragma unroll
            for (int d = 0; d < NDB; ++d)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc_o[d][i] *= alpha;
#pragma unroll
            for (int i = 0; i < 16; ++i) { minit[i] = -m_run; sacc[0][i] -= delta; sacc[1][i] -= delta; }
        }
        // ---- p = exp2(s - m); l from the unrounded p; P rounded pairwise to bf16 is the P V operand
        float ls = 0.f;
        bf16x8 pf[2][2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float p = __builtin_amdgcn_exp2f(sacc[kb][i]);
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
    };

    // ---- the loop over the list: k0 is multiplied, k1 is staged (or in flight), k2 - three-tile ring - enters the ring now
    int buf = 0;
    bool first = true;
    while (k1 >= 0) {
        int k2 = -1;
        if constexpr (NBUF == 3) {
            k2 = next_tile();
            if (k2 >= 0) dma_tile(k2, buf >= 1 ? buf - 1 : 2);          // slot (buf + 2) % 3: read last by the tile before k0, a barrier ago
        } else dma_tile(k1, buf ^ 1);
        tile_body(k0, buf, first, std::false_type{});
        // the next tile must have landed for every wave; with three slots the one after it may stay in flight
        if (NBUF == 3 && k2 >= 0) vm_wait<INFLIGHT>(); else vm_wait<0>();
        __builtin_amdgcn_s_barrier();
        first = false;
        k0 = k1;
        if constexpr (NBUF == 3) { k1 = k2; buf = buf == 2 ? 0 : buf + 1; }
        else { k1 = next_tile(); buf ^= 1; }
    }
    if (k0 == nt - 1 && (a.Sk % BKV)) tile_body(k0, buf, first, std::true_type{}); else tile_body(k0, buf, first, std::false_type{});

    const float l_tot = l_run + __shfl_xor(l_run, 32);
    const float inv = 1.0f / l_tot;
    if (qr < a.Sq) { if (a.wide_o) store_o_wide<NDB>(acc_o, inv, O, h); else store_o_narrow<NDB>(acc_o, inv, O, h); }
}

}  // namespace

int ltx_launch_attention_sparse(const AttnArgs& a, const uint32_t* map, int map_heads, hipStream_t s) { return ltx_launch_attention_sparse_batched(a, map, map_heads, 0, s); }

int ltx_launch_attention_sparse_batched(const AttnArgs& a, const uint32_t* map, int map_heads, int64_t map_bstride, hipStream_t s) {
    if (!a.q || !a.k || !a.v || !a.o || !map) LTX_FAIL(LTX_ERR_ARG, "attention_sparse: null tensor or map");
    if (a.B < 1 || a.Sq < 1 || a.Sk < 1 || a.heads < 1) LTX_FAIL(LTX_ERR_ARG, "attention_sparse: empty problem");
    if (a.hd != 64 && a.hd != 128) LTX_FAIL(LTX_ERR_UNSUPPORTED, "attention_sparse: head_dim must be 64 or 128 (got " + std::to_string(a.hd) + ")");
    if (map_heads != 1 && map_heads != a.heads)
        LTX_FAIL(LTX_ERR_ARG, "attention_sparse: map_heads must be 1 or heads (got " + std::to_string(map_heads) + " with " + std::to_string(a.heads) + " heads)");
    if (map_bstride != 0 && map_bstride < (int64_t)map_heads * cdiv(a.Sq, BQ) * cdiv(cdiv(a.Sk, BKV), 32))
        LTX_FAIL(LTX_ERR_ARG, "attention_sparse: map_batch_stride must be 0 or hold a batch row's map (got " + std::to_string(map_bstride) + " words)");
    if (a.bias || a.bias2d || a.k_count || a.p_out || a.q_rowsq) LTX_FAIL(LTX_ERR_UNSUPPORTED, "attention_sparse: no key bias, key count, row factor or P-only mode");
    const int64_t D = (int64_t)a.heads * a.hd;
    if (a.ldq < D || a.ldk < D || a.ldv < D || a.ldo < D) LTX_FAIL(LTX_ERR_ARG, "attention_sparse: ldq, ldk, ldv and ldo must hold heads * head_dim");
    if (((uintptr_t)a.q & 15) || ((uintptr_t)a.k & 15) || ((uintptr_t)a.v & 15) || ((uintptr_t)a.o & 7) || ((uintptr_t)map & 3) || a.ldq % 8 || a.ldk % 8 || a.ldv % 8 || a.ldo % 4)
        LTX_FAIL(LTX_ERR_ARG, "attention_sparse: misaligned pointer (q, k, v: 16 bytes with row strides % 8 == 0; o: 8 bytes with ldo % 4 == 0; map: 4 bytes)");
    // the 32-bit buffer arithmetic of the tile walk: every row offset of a batch row stays below 2^31 (ltx_attention_q64_fits' rule)
    if (!ltx_attention_q64_fits(a)) LTX_FAIL(LTX_ERR_UNSUPPORTED, "attention_sparse: a row offset of 2 GiB or more");
    AttnArgs ax = a;
    ax.xcd_heads = a.heads % 8 == 0 ? 1 : 0;
    ax.wide_o = (a.ldo % 8 == 0 && ((uintptr_t)a.o & 15) == 0) ? 1 : 0;
    void* tok = nullptr;
    ltx_prof_begin(LTX_PROF_ATTN_SELF, 4.0 * a.B * a.heads * (double)a.Sq * a.Sk * a.hd, s, &tok);      // the dense count: the profiler's rate shows the saving
    const dim3 grid((unsigned)(cdiv(a.Sq, BQ) * a.heads * a.B)), block(256);
    if (a.hd == 64) LTX_LAUNCH_TIMED(attn_sparse_kernel<64>, grid, block, 0, s, ax, map, map_heads, map_bstride);
    else LTX_LAUNCH_TIMED(attn_sparse_kernel<128>, grid, block, 0, s, ax, map, map_heads, map_bstride);
    ltx_prof_end(tok, s);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}
