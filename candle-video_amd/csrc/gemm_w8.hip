// bf16 x fp8 (e4m3) -> f32 MFMA GEMM for the fp8-resident block linears (include/ltxhip_fp8.h), and the two casts.  The weight never
// exists at two bytes in memory: it is staged and kept in LDS as bytes and widened in registers, in front of the bf16 MFMA.
//
//   * tile BM x BN in {256x256, 256x128, 128x128}, 512 threads = 8 waves as 2(M) x 4(N); a wave owns (BM/2) x (BN/4) = FM x FN
//     fragments of v_mfma_f32_16x16x32_bf16 with FM = 8, 8, 4 and FN = 4, 2, 2: tall in M, because the W fragment is the dear one;
//   * K-step 64: A goes HBM -> LDS as 128-byte rows (64 bf16), W as 64-BYTE rows (64 fp8), both by buffer_load_dwordx4 ... lds, two
//     stages, one vmcnt(0) + barrier per K-step.  64-byte W rows were chosen over 128-byte rows staged every other K-step: every
//     K-step then issues the same instructions (no odd / even loop body, no W stage that outlives two A stages) and a stage costs
//     BM * 128 + BN * 64 bytes - 96 KiB for two stages of the largest tile;
//   * bank conflicts.  A: the siblings' swizzle, 16-B chunk ^ ((row >> 1) & 7), ds_read_b128.  W: attn_common.h's 64-byte-row swizzle,
//     chunk ^ ((row >> 2) & 3).  A ds_read_b64 is served 32 lanes = 256 bytes of banks at a time; those 32 lanes are 16 rows x the two
//     halves of ONE logical chunk.  Four rows share a 256-byte line: row & 3 picks the 64-byte quarter, and the four row groups
//     (row >> 2) & 3 get four different XORs, so the 16 rows land on 16 distinct 16-byte slots and their two halves fill each slot:
//     all 64 banks once.  The swizzle sits on the per-lane SOURCE address of the LDS-DMA and again on the fragment reads;
//   * a lane's W operand of one MFMA is 8 consecutive k of one output channel: one ds_read_b64 and four
//     v_cvt_scalef32_pk_bf16_fp8 with scale 1.0 (exact, subnormals included; NaN stays NaN).  A converted fragment is used by all FM
//     MFMAs of its column: 4 FN converts per FM FN MFMAs - one per two MFMAs on the 256-row tiles, one per MFMA on 128 x 128;
//   * the last rows are clamped, the K tail is an out-of-range buffer offset (reads zeros; K % 16 == 0: chunks are whole);
//   * D = Wfrag x Afrag: a lane owns 4 consecutive output columns of one row and calls the shared epilogue<> on acc * sw[n]
//     (sw loaded once per column fragment, in front of the row loop: on gfx950 vmcnt counts the stores of the rows before).
// f32 accumulation in MFMA order; no split K: a partly filled last round is left as it is.
// Measured (tools/fp8_bench.py, profiles/fp8_linear_bench.md): SLOWER than the bf16 route of the same call at every block linear, far
// outside the identical-arm spread - x1.43 .. 1.81 at M = 4992 (against gemm_asm16's generated loops), x1.40 .. 2.23 at M = 384 (against
// the ring tiles); what this kernel buys is the residency (one byte per weight in HBM), not time.  DESIGN section 4 has the table.
// Registers (the compiler's kernel-resource-usage remarks, the same for all four epilogues): 256x256 177 VGPRs, 256x128 104, 128x128 70;
// no AGPRs and no scratch in any instantiation (2 / 4 / 7 waves per SIMD by registers; LDS allows one 256x256 block per CU).
#include <atomic>
#include "gemm_common.h"
#include "attn_common.h"

namespace {

constexpr int AROWB = 128;         // bytes per LDS row of A (64 bf16)
constexpr int WROWB = 64;          // bytes per LDS row of W (64 fp8)
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int swz_a(int row, int chunk) { return row * AROWB + ((chunk ^ ((row >> 1) & 7)) << 4); }
__device__ __forceinline__ int swz_w(int row, int chunk) { return row * WROWB + (kswz<4>(row, chunk) << 4); }

// 8 fp8 -> 8 bf16 (memory order): byte pairs (0,1) (2,3) of each word
__device__ __forceinline__ bf16x8 widen8(u32x2 w) {
    u32x4 r;
    r[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[0], 1.0f, false));
    r[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[0], 1.0f, true));
    r[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[1], 1.0f, false));
    r[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[1], 1.0f, true));
    return __builtin_bit_cast(bf16x8, r);
}

extern __shared__ __attribute__((aligned(16))) unsigned char w8_smem[];

template <int BM, int BN, int EPI>
__global__ __launch_bounds__(512) void gemm_w8_kernel(const GemmArgs g, const float* __restrict__ sw) {
    constexpr int WGM = 2, WGN = 4, NW = 8;
    constexpr int WM = BM / WGM, WN = BN / WGN, FM = WM / 16, FN = WN / 16;
    constexpr int AI = BM / (8 * NW), BI = BN / (16 * NW);       // LDS-DMA instructions per wave per K-step: 8 rows x 128 B (A), 16 rows x 64 B (W)
    static_assert(BM % (8 * NW) == 0 && BN % (16 * NW) == 0 && WM % 16 == 0 && WN % 16 == 0 && FM >= 4, "tile/wave layout");
    constexpr int STAGE = BM * AROWB + BN * WROWB;
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
    const int nk = (Kdim + 63) / 64;
    constexpr uint32_t OOB = 0x80000000u;                 // >= num_records; the launcher keeps every operand below 2 GiB
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.A), 0, (int)OOB, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(g.W), 0, (int)OOB, 0x00020000);
    // A: instruction j of this wave fills LDS rows 8 * (j * NW + wave) .. + 7; lane -> (row = lane >> 3, physical chunk = lane & 7)
    // W: ... rows 16 * (j * NW + wave) .. + 15; lane -> (row = lane >> 2, physical chunk = lane & 3)
    int a_chunk[AI], b_chunk[BI];
    uint32_t a_off[AI], b_off[BI];
#pragma unroll
    for (int j = 0; j < AI; ++j) {
        const int row = 8 * (j * NW + wave) + (lane >> 3);
        a_chunk[j] = (lane & 7) ^ ((row >> 1) & 7);
        int m = m0 + row; if (m > g.M - 1) m = g.M - 1;
        a_off[j] = ((uint32_t)m * (uint32_t)g.lda + a_chunk[j] * 8) * 2u;
    }
#pragma unroll
    for (int j = 0; j < BI; ++j) {
        const int row = 16 * (j * NW + wave) + (lane >> 2);
        b_chunk[j] = kswz<4>(row, lane & 3);
        int n = n0 + row; if (n > g.N - 1) n = g.N - 1;
        b_off[j] = (uint32_t)n * (uint32_t)Kdim + b_chunk[j] * 16;
    }
    auto dma = [&](__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff, unsigned char* lds) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds, 16, (int)voff, (int)soff, 0, 0);
    };
    auto stage = [&](int kt, int buf) {
        unsigned char* As = w8_smem + buf * STAGE; unsigned char* Bs = As + BM * AROWB;
#pragma unroll
        for (int j = 0; j < AI; ++j) dma(ra, kt * 64 + a_chunk[j] * 8 < Kdim ? a_off[j] : OOB, (uint32_t)kt * 128u, As + (j * NW + wave) * 1024);
#pragma unroll
        for (int j = 0; j < BI; ++j) dma(rw, kt * 64 + b_chunk[j] * 16 < Kdim ? b_off[j] : OOB, (uint32_t)kt * 64u, Bs + (j * NW + wave) * 1024);
    };

    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    stage(0, 0);
    __syncthreads();                                   // emits vmcnt(0) for the outstanding LDS-DMA

    const int frow = lane & 15, fq = lane >> 4;
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) stage(kt + 1, buf ^ 1);
        const unsigned char* As = w8_smem + buf * STAGE;
        const unsigned char* Bs = As + BM * AROWB;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {                // 32 k per MFMA; the lane's 8: A chunk kb * 4 + fq, W chunk kb * 2 + (fq >> 1), half fq & 1
            bf16x8 wf[FN], af[FM];
#pragma unroll
            for (int f = 0; f < FN; ++f)
                wf[f] = widen8(*reinterpret_cast<const u32x2*>(Bs + swz_w(wn * WN + f * 16 + frow, kb * 2 + (fq >> 1)) + (fq & 1) * 8));
            af[0] = *reinterpret_cast<const bf16x8*>(As + swz_a(wm * WM + frow, kb * 4 + fq));
#pragma unroll
            for (int fm = 0; fm < FM; ++fm) {
                if (fm + 1 < FM) af[fm + 1] = *reinterpret_cast<const bf16x8*>(As + swz_a(wm * WM + (fm + 1) * 16 + frow, kb * 4 + fq));
#pragma unroll
                for (int fn = 0; fn < FN; ++fn) acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[fn], af[fm], acc[fm][fn], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // D = W x A: lane (frow, fq) of fragment (fm, fn) holds row m = .. + frow, columns n = .. + 4 * fq + 0..3
    f32x4 s4[FN];
#pragma unroll
    for (int fn = 0; fn < FN; ++fn) {
        const int nb = n0 + wn * WN + fn * 16 + 4 * fq;
        s4[fn] = (f32x4){1.f, 1.f, 1.f, 1.f};
        if (sw && nb < g.N) s4[fn] = *reinterpret_cast<const f32x4*>(sw + nb);
    }
#pragma unroll
    for (int fm = 0; fm < FM; ++fm) {
        const int m = m0 + wm * WM + fm * 16 + frow;
        if (m >= g.M) continue;
#pragma unroll
        for (int fn = 0; fn < FN; ++fn) {
            const int nb = n0 + wn * WN + fn * 16 + 4 * fq;
            if (nb >= g.N) continue;                    // N % 4 == 0: a lane's four columns are inside or outside together
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = acc[fm][fn][i] * s4[fn][i];
            epilogue<bf16_t, EPI>(g, m, nb, v);
        }
    }
}

template <int BM, int BN, int EPI>
int launch_w8(const GemmArgs& g, hipStream_t s) {
    constexpr int smem = 2 * (BM * AROWB + BN * WROWB);
    static std::atomic<unsigned long long> attr_devs{0};
    auto kern = gemm_w8_kernel<BM, BN, EPI>;
    LTX_TRY(ltx_set_max_dyn_smem(attr_devs, reinterpret_cast<const void*>(kern), smem));
    const dim3 grid((unsigned)(cdiv(g.M, BM) * cdiv(g.N, BN))), block(512);
    LTX_LAUNCH_TIMED(kern, grid, block, smem, s, g, g.w_scale);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}

template <int BM, int BN>
int launch_w8_epi(const GemmArgs& g, int epi, hipStream_t s) {
    switch (epi) {
        case EPI_BIAS: return launch_w8<BM, BN, EPI_BIAS>(g, s);
        case EPI_GELU: return launch_w8<BM, BN, EPI_GELU>(g, s);
        case EPI_GATE_RESID: return launch_w8<BM, BN, EPI_GATE_RESID>(g, s);
        case EPI_RESID: return launch_w8<BM, BN, EPI_RESID>(g, s);
    }
    LTX_FAIL(LTX_ERR_ARG, "gemm_w8: epi must be 0..3");
}

// ---- the casts: one pass each, 16 elements per thread ----
// f32 -> e4m3fn, round to nearest even, saturating at +-448 (infinities included), NaN -> 0x7F | sign: integer arithmetic and one
// v_rndne_f32, no dependence on the convert instruction's overflow mode
__device__ __forceinline__ unsigned fp8_e4m3_from_f32(float x) {
    uint32_t b = __builtin_bit_cast(uint32_t, x);
    const unsigned sign = (b >> 24) & 0x80u;
    b &= 0x7fffffffu;
    if (b > 0x7f800000u) return sign | 0x7fu;               // NaN
    if (b >= 0x43e00000u) return sign | 0x7eu;              // |x| >= 448 (everything in [448, 464) rounds there anyway)
    if (b < 0x3c800000u) return sign | (unsigned)rintf(__builtin_bit_cast(float, b) * 512.0f);      // below 2^-6, the smallest normal: multiples of 2^-9; 8 is 2^-6 itself, code 0x08
    b += 0x7ffffu + ((b >> 20) & 1u);                       // 23 -> 3 mantissa bits, ties to even (a carry walks into the exponent)
    return sign | ((b >> 20) - (120u << 3));                // re-bias 127 -> 7
}
// x bf16 [rows, D] (row stride ld) -> q fp8 [rows, D] dense: two 16-byte loads, then one 16-byte store
__global__ __launch_bounds__(256) void cast_fp8_kernel(const bf16_t* __restrict__ x, int64_t n16, int D16, int ld, unsigned char* __restrict__ q) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n16) return;
    const int64_t row = i / D16; const int c = (int)(i - row * D16);
    const bf16x8* src = reinterpret_cast<const bf16x8*>(x + row * ld + (int64_t)c * 16);
    const bf16x8 lo = src[0], hi = src[1];
    u32x4 out;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        uint32_t word = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int e = w * 4 + b;
            word |= fp8_e4m3_from_f32((float)(e < 8 ? lo[e] : hi[e - 8])) << (8 * b);
        }
        out[w] = word;
    }
    *reinterpret_cast<u32x4*>(q + i * 16) = out;
}

// q fp8 [n] -> y bf16 or f32 [n]: 8 per thread where both pointers are aligned for it, one per thread in the tail
template <typename T>
__global__ __launch_bounds__(256) void widen_fp8_kernel(const unsigned char* __restrict__ q, int64_t n, T* __restrict__ y, int vec) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i >= n) return;
    if (vec && i + 8 <= n) {
        const u32x2 w = *reinterpret_cast<const u32x2*>(q + i);
        const bf16x8 v = widen8(w);
        if constexpr (sizeof(T) == 2) *reinterpret_cast<bf16x8*>(y + i) = v;
        else {
            f32x4 a = {(float)v[0], (float)v[1], (float)v[2], (float)v[3]}, b = {(float)v[4], (float)v[5], (float)v[6], (float)v[7]};
            *reinterpret_cast<f32x4*>(y + i) = a; *reinterpret_cast<f32x4*>(y + i + 4) = b;
        }
        return;
    }
    for (int64_t j = i; j < n && j < i + 8; ++j) {
        const bf16x2v p = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((uint32_t)q[j], 1.0f, false);
        y[j] = from_f32<T>((float)p[0]);
    }
}

}  // namespace

// The shape rule (no measured plans): the largest tile whose grid still gives every CU a block, else 128 x 128.
int ltx_gemm_w8_pick_tile(int M, int N) {
    if (N > 128 && M > 128 && (int64_t)cdiv(M, 256) * cdiv(N, 256) >= 256) return 0;
    if (M > 128 && (int64_t)cdiv(M, 256) * cdiv(N, 128) >= 256) return 1;
    return 2;
}
const char* ltx_gemm_w8_tile_name(int tile) { return tile == 0 ? "w8:256x256" : (tile == 1 ? "w8:256x128" : "w8:128x128"); }

int ltx_launch_gemm_w8(const GemmArgs& g, int epi, int tile, hipStream_t s) {
    if (!g.A || !g.W || !g.C) LTX_FAIL(LTX_ERR_ARG, "gemm_w8: null tensor");
    if (epi < 0 || epi > 3) LTX_FAIL(LTX_ERR_ARG, "gemm_w8: epi must be 0..3");
    if (g.M < 1 || g.N < 1 || g.K < 1 || g.lda < g.K) LTX_FAIL(LTX_ERR_ARG, "gemm_w8: M, N, K >= 1 and lda >= K");
    if ((epi == EPI_GATE_RESID || epi == EPI_RESID) && !g.resid) LTX_FAIL(LTX_ERR_ARG, "gemm_w8: residual epilogue needs resid");
    if (epi == EPI_GATE_RESID && (!g.gate || g.rows_per_batch < 1)) LTX_FAIL(LTX_ERR_ARG, "gemm_w8: gated epilogue needs gate");
    if (g.c_seg_shift && epi != EPI_BIAS) LTX_FAIL(LTX_ERR_ARG, "gemm_w8: the segmented output rides on the bias epilogue");
    if (tile < -1 || tile > 2) LTX_FAIL(LTX_ERR_ARG, "gemm_w8: tile must be -1 (shape rule), 0 (256x256), 1 (256x128) or 2 (128x128)");
    if (g.conv || g.rowsq || g.C2 || g.rs_sq || g.defer_parts) LTX_FAIL(LTX_ERR_ARG, "gemm_w8: a plain linear call only (no conv, row partials, norm fold or deferred reduction)");
    if (g.K % 16 != 0) LTX_FAIL(LTX_ERR_UNSUPPORTED, "gemm_w8: K % 16 != 0");
    if (g.N % 4 != 0 || g.lda % 8 != 0) LTX_FAIL(LTX_ERR_UNSUPPORTED, "gemm_w8: N % 4 != 0 or lda % 8 != 0");
    if ((double)g.M * g.lda * 2.0 >= 2147483648.0 || (double)g.N * g.K >= 2147483648.0) LTX_FAIL(LTX_ERR_UNSUPPORTED, "gemm_w8: an operand of 2 GiB or more (32-bit buffer offsets)");
    bool misaligned = ((uintptr_t)g.A & 15) || ((uintptr_t)g.W & 15) || ((uintptr_t)g.C & 7) || g.ldc % 4 != 0 || ((uintptr_t)g.w_scale & 15) || ((uintptr_t)g.bias & 7);
    if (g.resid) misaligned = misaligned || ((uintptr_t)g.resid & 7) || g.ldr % 4 != 0;
    if (epi == EPI_GATE_RESID) misaligned = misaligned || ((uintptr_t)g.gate & 15) || g.gate_stride % 4 != 0;
    if (g.c_seg_shift) misaligned = misaligned || (1 << g.c_seg_shift) % 4 != 0 || g.c_seg_stride % 4 != 0;
    if (misaligned) LTX_FAIL(LTX_ERR_ARG, "gemm_w8: misaligned pointer (a, w, w_scale, gate: 16 bytes; y, resid, bias: 8; leading dimensions % 4)");
    if (tile < 0) tile = ltx_gemm_w8_pick_tile(g.M, g.N);
    void* tok = nullptr;
    ltx_prof_begin(LTX_PROF_GEMM, 2.0 * (double)g.M * g.N * g.K, s, &tok);
    ltx_prof_kernel(LTX_PROFK_GEMM_W8);
    int rc;
    switch (tile) {
        case 0: rc = launch_w8_epi<256, 256>(g, epi, s); break;
        case 1: rc = launch_w8_epi<256, 128>(g, epi, s); break;
        default: rc = launch_w8_epi<128, 128>(g, epi, s); break;
    }
    ltx_prof_end(tok, s);
    return rc;
}

int ltx_launch_cast_fp8(const void* x, int64_t rows, int D, int ld, void* q, hipStream_t s) {
    if (!x || !q) LTX_FAIL(LTX_ERR_ARG, "cast_fp8: null tensor");
    if (rows < 1 || D < 16 || D % 16 != 0 || ld < D || ld % 8 != 0) LTX_FAIL(LTX_ERR_ARG, "cast_fp8: rows >= 1, D a multiple of 16, ld >= D a multiple of 8");
    if (((uintptr_t)x & 15) || ((uintptr_t)q & 15)) LTX_FAIL(LTX_ERR_ARG, "cast_fp8: x and q must be 16-byte aligned");
    const int64_t n16 = rows * (D / 16);
    if (cdiv64(n16, 256) > 2147483647) LTX_FAIL(LTX_ERR_UNSUPPORTED, "cast_fp8: tensor too large for one launch");
    hipLaunchKernelGGL(cast_fp8_kernel, dim3((unsigned)cdiv64(n16, 256)), dim3(256), 0, s, reinterpret_cast<const bf16_t*>(x), n16, D / 16, ld, reinterpret_cast<unsigned char*>(q));
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}

int ltx_launch_widen_fp8(const void* q, int64_t n, void* y, int dst_dtype, hipStream_t s) {
    if (!q || !y) LTX_FAIL(LTX_ERR_ARG, "widen_fp8: null tensor");
    if (n < 1) LTX_FAIL(LTX_ERR_ARG, "widen_fp8: empty tensor");
    const int64_t nthr = cdiv64(n, 8);
    if (cdiv64(nthr, 256) > 2147483647) LTX_FAIL(LTX_ERR_UNSUPPORTED, "widen_fp8: tensor too large for one launch");
    const int vec = !((uintptr_t)q & 7) && !((uintptr_t)y & 15);
    const dim3 grid((unsigned)cdiv64(nthr, 256)), block(256);
    if (dst_dtype == LTX_DT_BF16) hipLaunchKernelGGL(widen_fp8_kernel<bf16_t>, grid, block, 0, s, reinterpret_cast<const unsigned char*>(q), n, reinterpret_cast<bf16_t*>(y), vec);
    else hipLaunchKernelGGL(widen_fp8_kernel<float>, grid, block, 0, s, reinterpret_cast<const unsigned char*>(q), n, reinterpret_cast<float*>(y), vec);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}
