// int8 x int8 -> int32 MFMA GEMM for the W8A8 linear layers (include/ltxhip_int8.h), gemm_big.hip's structure at one byte per element:
//
//   * tile BM x BN in {256x256, 256x128, 128x128}, K-step 128 int8 (the same 128-B LDS rows), 512 threads = 8 waves as 2(M) x 4(N),
//     each wave (BM/2) x (BN/4) with v_mfma_i32_16x16x64_i8: a lane's operand is 16 bytes = 16 consecutive k, as in bf16;
//   * operands go HBM -> LDS with buffer_load_dwordx4 ... lds; the bank swizzle (16-B chunk ^ ((row>>1)&7)) sits on the per-lane
//     SOURCE address and again on the ds_read_b128 fragment reads; two stages, one vmcnt(0)+barrier per K-step;
//   * the last rows are clamped, the K tail is an out-of-range buffer offset (reads zeros; K % 16 == 0: chunks are whole);
//   * D = Wfrag x Afrag: a lane owns 4 consecutive output columns of one row and calls the shared epilogue<> on
//     (float(acc) * sa[m]) * sw[n]; the raw form stores the int32 accumulators instead (the exact test of the operand map).
// The integer sum is exact, so the tile changes no bit.  No split K: a partly filled last round is left as it is.
#include <atomic>
#include "gemm_common.h"

namespace {

constexpr int ROWB = 128;          // bytes per LDS row (128 int8)
typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int swz_i8(int row, int chunk) { return row * ROWB + ((chunk ^ ((row >> 1) & 7)) << 4); }

extern __shared__ __attribute__((aligned(16))) unsigned char i8_smem[];

struct I8Scales { const float* sa; const float* sw; };

template <int BM, int BN, int EPI>
__global__ __launch_bounds__(512) void gemm_i8_kernel(const GemmArgs g, const I8Scales sc) {
    constexpr int WGM = 2, WGN = 4, NW = 8;
    constexpr int WM = BM / WGM, WN = BN / WGN, FM = WM / 16, FN = WN / 16;
    constexpr int AI = BM / (8 * NW), BI = BN / (8 * NW);        // LDS-DMA instructions per wave per K-step (A, W): 8 rows x 128 B each
    static_assert(BM % (8 * NW) == 0 && BN % (8 * NW) == 0 && WM % 16 == 0 && WN % 16 == 0, "tile/wave layout");
    constexpr int STAGE = (BM + BN) * ROWB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;
    const int ntn = (g.N + BN - 1) / BN;
    // XCD-aware tile order (speed only, bijective for any grid): XCD x gets a contiguous run of tiles
    int bid = blockIdx.x;
    {
        const int nblk = (int)gridDim.x, q = nblk >> 3, r = nblk & 7, x = bid & 7, i = bid >> 3;
        bid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
    }
    const int mt = bid / ntn, nt = bid - mt * ntn;
    const int m0 = mt * BM, n0 = nt * BN;
    const int Kdim = g.K;
    const int nk = (Kdim + 127) / 128;
    constexpr uint32_t OOB = 0x80000000u;                 // >= num_records; the launcher keeps every operand below 2 GiB
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.A), 0, (int)OOB, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.W), 0, (int)OOB, 0x00020000);
    // instruction j of this wave fills LDS rows 8 * (j * NW + wave) .. + 7; lane -> (row in group = lane >> 3, physical chunk = lane & 7)
    const int lr = lane >> 3, pc = lane & 7;
    int a_chunk[AI], b_chunk[BI];
    uint32_t a_off[AI], b_off[BI];
#pragma unroll
    for (int j = 0; j < AI; ++j) {
        const int row = 8 * (j * NW + wave) + lr;
        a_chunk[j] = pc ^ ((row >> 1) & 7);
        int m = m0 + row; if (m > g.M - 1) m = g.M - 1;
        a_off[j] = (uint32_t)m * (uint32_t)g.lda + a_chunk[j] * 16;
    }
#pragma unroll
    for (int j = 0; j < BI; ++j) {
        const int row = 8 * (j * NW + wave) + lr;
        b_chunk[j] = pc ^ ((row >> 1) & 7);
        int n = n0 + row; if (n > g.N - 1) n = g.N - 1;
        b_off[j] = (uint32_t)n * (uint32_t)Kdim + b_chunk[j] * 16;
    }
    auto dma = [&](__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff, unsigned char* lds) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds, 16, (int)voff, (int)soff, 0, 0);
    };
    auto stage = [&](int kt, int buf) {
        unsigned char* As = i8_smem + buf * STAGE; unsigned char* Bs = As + BM * ROWB;
        const uint32_t soff = (uint32_t)kt * 128u;
#pragma unroll
        for (int j = 0; j < AI; ++j) dma(ra, kt * 128 + a_chunk[j] * 16 < Kdim ? a_off[j] : OOB, soff, As + (j * NW + wave) * 1024);
#pragma unroll
        for (int j = 0; j < BI; ++j) dma(rw, kt * 128 + b_chunk[j] * 16 < Kdim ? b_off[j] : OOB, soff, Bs + (j * NW + wave) * 1024);
    };

    i32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = (i32x4){0, 0, 0, 0};

    stage(0, 0);
    __syncthreads();                                   // emits vmcnt(0) for the outstanding LDS-DMA

    const int frow = lane & 15, fq = lane >> 4;
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) stage(kt + 1, buf ^ 1);
        const unsigned char* As = i8_smem + buf * STAGE;
        const unsigned char* Bs = As + BM * ROWB;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {                // 64 k per MFMA: chunk kb * 4 + fq of the row
            i32x4 af[FM], wf[FN];
#pragma unroll
            for (int f = 0; f < FN; ++f) wf[f] = *reinterpret_cast<const i32x4*>(Bs + swz_i8(wn * WN + f * 16 + frow, kb * 4 + fq));
            af[0] = *reinterpret_cast<const i32x4*>(As + swz_i8(wm * WM + frow, kb * 4 + fq));
#pragma unroll
            for (int fm = 0; fm < FM; ++fm) {
                if (fm + 1 < FM) af[fm + 1] = *reinterpret_cast<const i32x4*>(As + swz_i8(wm * WM + (fm + 1) * 16 + frow, kb * 4 + fq));
#pragma unroll
                for (int fn = 0; fn < FN; ++fn) acc[fm][fn] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf[fn], af[fm], acc[fm][fn], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // D = W x A: lane (frow, fq) of fragment (fm, fn) holds row m = .. + frow, columns n = .. + 4 * fq + 0..3
#pragma unroll
    for (int fm = 0; fm < FM; ++fm) {
        const int m = m0 + wm * WM + fm * 16 + frow;
        if (m >= g.M) continue;
        float sam = 0.f;
        if constexpr (EPI != EPI_I8_RAW) sam = sc.sa[m];
#pragma unroll
        for (int fn = 0; fn < FN; ++fn) {
            const int nb = n0 + wn * WN + fn * 16 + 4 * fq;
            if (nb >= g.N) continue;                    // N % 4 == 0: a lane's four columns are inside or outside together
            if constexpr (EPI == EPI_I8_RAW) {
                *reinterpret_cast<i32x4*>(reinterpret_cast<int*>(g.C) + (int64_t)m * g.ldc + nb) = acc[fm][fn];
            } else {
                const f32x4 w4 = *reinterpret_cast<const f32x4*>(sc.sw + nb);
                float v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = ((float)acc[fm][fn][i] * sam) * w4[i];      // the order ltxhip_int8.h states
                epilogue<bf16_t, EPI>(g, m, nb, v);
            }
        }
    }
}

template <int BM, int BN, int EPI>
int launch_i8(const GemmArgs& g, const float* sa, const float* sw, hipStream_t s) {
    constexpr int smem = 2 * (BM + BN) * ROWB;
    static std::atomic<unsigned long long> attr_devs{0};
    auto kern = gemm_i8_kernel<BM, BN, EPI>;
    LTX_TRY(ltx_set_max_dyn_smem(attr_devs, reinterpret_cast<const void*>(kern), smem));
    const dim3 grid((unsigned)(cdiv(g.M, BM) * cdiv(g.N, BN))), block(512);
    const I8Scales sc{sa, sw};
    LTX_LAUNCH_TIMED(kern, grid, block, smem, s, g, sc);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}

template <int BM, int BN>
int launch_i8_epi(const GemmArgs& g, const float* sa, const float* sw, int epi, hipStream_t s) {
    switch (epi) {
        case EPI_BIAS: return launch_i8<BM, BN, EPI_BIAS>(g, sa, sw, s);
        case EPI_GELU: return launch_i8<BM, BN, EPI_GELU>(g, sa, sw, s);
        case EPI_GATE_RESID: return launch_i8<BM, BN, EPI_GATE_RESID>(g, sa, sw, s);
        case EPI_RESID: return launch_i8<BM, BN, EPI_RESID>(g, sa, sw, s);
        case EPI_I8_RAW: return launch_i8<BM, BN, EPI_I8_RAW>(g, sa, sw, s);
    }
    LTX_FAIL(LTX_ERR_ARG, "gemm_i8: epi must be 0..3");
}

}  // namespace

// The shape rule (no measured plans): the largest tile whose grid still gives every CU a block, else 128 x 128.
int ltx_gemm_i8_pick_tile(int M, int N) {
    if (N > 128 && M > 128 && (int64_t)cdiv(M, 256) * cdiv(N, 256) >= 256) return 0;
    if (M > 128 && (int64_t)cdiv(M, 256) * cdiv(N, 128) >= 256) return 1;
    return 2;
}

int ltx_launch_gemm_i8(const GemmArgs& g, const float* sa, const float* sw, int epi, int tile, hipStream_t s) {
    const bool raw = epi == EPI_I8_RAW;
    if (!g.A || !g.W || !g.C) LTX_FAIL(LTX_ERR_ARG, "gemm_i8: null tensor");
    if (!raw && (!sa || !sw)) LTX_FAIL(LTX_ERR_ARG, "gemm_i8: null scale");
    if (!raw && (epi < 0 || epi > 3)) LTX_FAIL(LTX_ERR_ARG, "gemm_i8: epi must be 0..3");
    if (g.M < 1 || g.N < 1 || g.K < 1 || g.lda < g.K) LTX_FAIL(LTX_ERR_ARG, "gemm_i8: M, N, K >= 1 and lda >= K");
    if ((epi == EPI_GATE_RESID || epi == EPI_RESID) && !g.resid) LTX_FAIL(LTX_ERR_ARG, "gemm_i8: residual epilogue needs resid");
    if (epi == EPI_GATE_RESID && (!g.gate || g.rows_per_batch < 1)) LTX_FAIL(LTX_ERR_ARG, "gemm_i8: gated epilogue needs gate");
    if (g.c_seg_shift && epi != EPI_BIAS) LTX_FAIL(LTX_ERR_ARG, "gemm_i8: the segmented output rides on the bias epilogue");
    if (tile < -1 || tile > 2) LTX_FAIL(LTX_ERR_ARG, "gemm_i8: tile must be -1 (shape rule), 0 (256x256), 1 (256x128) or 2 (128x128)");
    if (g.K % 16 != 0) LTX_FAIL(LTX_ERR_UNSUPPORTED, "gemm_i8: K % 16 != 0");
    if (g.K > 131072) LTX_FAIL(LTX_ERR_UNSUPPORTED, "gemm_i8: K too large (at most 131072: the int32 sum must not overflow)");
    if (g.N % 4 != 0 || g.lda % 16 != 0) LTX_FAIL(LTX_ERR_UNSUPPORTED, "gemm_i8: N % 4 != 0 or lda % 16 != 0");
    if ((double)g.M * g.lda >= 2147483648.0 || (double)g.N * g.K >= 2147483648.0) LTX_FAIL(LTX_ERR_UNSUPPORTED, "gemm_i8: an operand of 2 GiB or more (32-bit buffer offsets)");
    const int out_al = raw ? 15 : 7;
    bool misaligned = ((uintptr_t)g.A & 15) || ((uintptr_t)g.W & 15) || ((uintptr_t)g.C & out_al) || g.ldc % 4 != 0;
    if (!raw) {
        misaligned = misaligned || ((uintptr_t)sw & 15) || ((uintptr_t)sa & 3) || ((uintptr_t)g.bias & 7);
        if (g.resid) misaligned = misaligned || ((uintptr_t)g.resid & 7) || g.ldr % 4 != 0;
        if (epi == EPI_GATE_RESID) misaligned = misaligned || ((uintptr_t)g.gate & 15) || g.gate_stride % 4 != 0;
        if (g.c_seg_shift) misaligned = misaligned || (1 << g.c_seg_shift) % 4 != 0 || g.c_seg_stride % 4 != 0;
    }
    if (misaligned) LTX_FAIL(LTX_ERR_ARG, "gemm_i8: misaligned pointer (a_q, w_q, w_scale, gate: 16 bytes; y, resid, bias: 8; leading dimensions % 4)");
    if (tile < 0) tile = ltx_gemm_i8_pick_tile(g.M, g.N);
    void* tok = nullptr;
    ltx_prof_begin(LTX_PROF_GEMM, 2.0 * (double)g.M * g.N * g.K, s, &tok);
    ltx_prof_kernel(LTX_PROFK_GEMM_I8);
    int rc;
    switch (tile) {
        case 0: rc = launch_i8_epi<256, 256>(g, sa, sw, epi, s); break;
        case 1: rc = launch_i8_epi<256, 128>(g, sa, sw, epi, s); break;
        default: rc = launch_i8_epi<128, 128>(g, sa, sw, epi, s); break;
    }
    ltx_prof_end(tok, s);
    return rc;
}
