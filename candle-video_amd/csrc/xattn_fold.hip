// Cross attention with attn2.to_out folded into the cached text context (dit.hip, text_context).
//   out2 = h + (sum_h P_h V_h) Wo2^T + b = h + sum_h P_h (V_h Wo2_h^T) + b
// V_h Wo2_h^T depends on the prompt and the weights alone, so it is built once per context: vo [L][B][D][H * KP], K-contiguous
// like every weight here, vo[n][h * KP + k] = sum_{d < 64} Wo2[n][64 h + d] * Vc[b, k, 64 h + d] (f32 accumulation, one bf16
// rounding).  The cross kernel then stops at the softmax (AttnArgs::p_out) and to_out runs on P with K = H * KP instead of D.
// This file: the one decision (ltx_xattn_fold_route), KP from the kept-key counts, and the batched build kernel.
#include "common.h"
#include "kernels.h"
#include "options.h"

// H * KP <= kXFoldT * D: the largest ratio at which the folded pair (P-only cross kernel + to_out over H * KP) measured faster
// than the parent pair by more than twice the spread of two identical arms (profiles/xattn_fold_vo_bench.md; docs/lab_notes.md).
// At 2B dims and 4992 tokens: -17 to -18 us per layer at H * KP = D / 2 in every run; at H * KP = D -0.7 to -1.8 us, in one run
// of three below twice the spread, for another 117 MB of vo per batch row - so 1/2.  Option xattn_fold_vo=2 folds up to
// H * KP = D (the tool's arm for this table); beyond D the probabilities no longer fit the attention output's buffer.
static constexpr double kXFoldT = 0.5;

int ltx_xattn_fold_kp(const int* counts, int B) {
    int mx = 1;
    for (int b = 0; b < B; ++b) if (counts[b] > mx) mx = counts[b];
    return (mx + 31) / 32 * 32;
}

bool ltx_xattn_fold_route(int dtype, int head_dim, int heads, int D, int KP, int B, bool compact) {
    if (!ltx_opt().xattn_fold_vo) return false;
    if (dtype != LTX_DT_BF16 || head_dim != 64 || !compact || heads < 1 || D != heads * head_dim || B < 1) return false;
    if (KP < 32 || KP % 32 != 0 || KP > 128) return false;
    // (B > 1: one to_out launch per batch row, its vo is its own - measured at C3's three rows: -42.8 us per layer, same file)
    return (double)heads * KP <= (ltx_opt().xattn_fold_vo >= 2 ? 1.0 : kXFoldT) * D;
}

namespace {
typedef float f32x4v __attribute__((ext_vector_type(4)));

// One block: 256 output rows n of one (layer, batch row, head); a wave owns four 16-row tiles.  MFMA 16x16x32, both operands
// d-contiguous: A = V (row = key, k = d), B = Wo2 (k = d, column = n), so a lane ends with four consecutive keys of one row n.
__global__ __launch_bounds__(256) void xattn_fold_kernel(const XFoldArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int h = blockIdx.y, lb = blockIdx.z, l = lb / a.B, b = lb % a.B;
    const bf16_t* W = reinterpret_cast<const bf16_t*>(a.tab[l].w);
    const bf16_t* V = reinterpret_cast<const bf16_t*>(a.tab[l].v) + (int64_t)b * a.K * a.ldv + h * 64;
    const int HK = a.H * a.KP;
    bf16_t* O = reinterpret_cast<bf16_t*>(a.vo) + (int64_t)lb * a.D * HK + h * a.KP;
    const int n_base = blockIdx.x * 256 + wave * 64;
    bf16x8 wf[4][2];
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = n_base + i * 16 + r;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
            wf[i][ks] = n < a.D ? *reinterpret_cast<const bf16x8*>(W + (int64_t)n * a.D + h * 64 + ks * 32 + q * 8) : zero8;
    }
    for (int kt = 0; kt < a.KP / 16; ++kt) {
        const int key = kt * 16 + r;
        bf16x8 vf[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
            vf[ks] = key < a.K ? *reinterpret_cast<const bf16x8*>(V + (int64_t)key * a.ldv + ks * 32 + q * 8) : zero8;      // keys behind the row's count are zeros in the compacted buffer
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f32x4v acc = {0.f, 0.f, 0.f, 0.f};
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[0], wf[i][0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[1], wf[i][1], acc, 0, 0, 0);
            const int n = n_base + i * 16 + r;
            if (n < a.D) {
                const bf16x4 o4 = {(bf16_t)acc[0], (bf16_t)acc[1], (bf16_t)acc[2], (bf16_t)acc[3]};
                *reinterpret_cast<bf16x4*>(O + (int64_t)n * HK + kt * 16 + q * 4) = o4;
            }
        }
    }
}
}  // namespace

int ltx_launch_xattn_fold(const XFoldArgs& a, hipStream_t s) {
    if (!a.tab || !a.vo || a.L < 1 || a.B < 1 || a.K < 1 || a.H < 1) LTX_FAIL(LTX_ERR_ARG, "xattn_fold: bad argument");
    if (a.D != a.H * 64 || a.KP < 32 || a.KP % 32 != 0 || a.KP > 128 || a.ldv % 8 != 0 || a.ldv < a.D || ((uintptr_t)a.vo & 15))
        LTX_FAIL(LTX_ERR_ARG, "xattn_fold: head_dim 64, KP a multiple of 32 up to 128, 16-byte aligned rows");
    if ((int64_t)a.L * a.B > 65535 || a.H > 65535) LTX_FAIL(LTX_ERR_ARG, "xattn_fold: too many layers x batch rows");
    hipLaunchKernelGGL(xattn_fold_kernel, dim3((unsigned)cdiv(a.D, 256), (unsigned)a.H, (unsigned)(a.L * a.B)), dim3(256), 0, s, a);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}
