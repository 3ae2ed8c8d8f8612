// LoRA merge (include/ltxhip_lora.h): out = round(f32(W0) + sum_i c_i * (B_i A_i)), one pass over the weight.
//
// The adapter switch is a read-modify-write of every targeted weight (2B: 1.9 G parameters) with a rank-r product per output
// element: 2r flops against 4 bytes moved, 64 flop/B at rank 128 - above what the f32 vector pipe sustains against HBM, far below
// the bf16 MFMA ridge.  So the product runs on v_mfma_f32_16x16x32_bf16 and the pass is meant to be bound by the W0 / out streams.
//
// lora_merge_kernel (bf16): 256 threads = 4 waves as 2 (n) x 2 (k), block tile 64 rows x 128 columns of W, wave tile 32 x 64.
//   * operands arrive packed (lora_pack_kernel, once per adapter): A transposed to [K, r_pad], B as [N, r_pad], r_pad = r rounded
//     up to 32 with zeros (exact: a zero product leaves an f32 accumulator as it is).  Both are then read ALONG THE RANK in 16-byte
//     pieces, which is what an MFMA operand fragment is (8 consecutive k-of-the-product values per lane), with no transpose in here.
//   * the MFMA's row index is the weight's COLUMN: D = (A^T slab) x (B slab)^T, a lane owns 4 consecutive columns of one weight
//     row per tile.  Two tiles whose rows interleave in fours (tile t holds columns 8 g' + 4 t + j of a 32-column span) give a lane
//     8 consecutive columns: one 16-byte load of W0 and one 16-byte store of out per (row, span).
//   * per adapter: a fresh accumulator, the rank walked in ascending 32-blocks (staged through LDS 64 ranks at a time), then
//     total = fma(c_i, acc_i, total) in list order; out = rne_bf16(f32(W0) + total).
//   * the lane's four W0 chunks are loaded before the first MFMA, so the pass streams; the store loop holds no load.
//   * N any size, K % 8 == 0: rows / columns beyond the matrix are masked (zeros into LDS, no W0 load, no store).
//   * kOne: the same code compiled for a list of one adapter, where no running total lives through the rank loop: 96 instead of
//     132 registers, four or five blocks per CU instead of three - more W0 bytes in flight for the same stream.
// lora_merge_f32_kernel (parity mode): the same order with plain f32 FMAs, four columns per thread.
#include <cstring>
#include <map>
#include "lora.h"

namespace {

constexpr int BN = 64, BK = 128, RC = 64, LDR = RC + 8;      // LDS rows of 144 bytes: 16-byte aligned, rows 36 banks apart

template <bool kOne>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kOne ? 4 : 3))) void lora_merge_kernel(LoraMergeArgs a) {
    __shared__ __attribute__((aligned(16))) bf16_t As[BK * LDR];      // [column of W][rank]
    __shared__ __attribute__((aligned(16))) bf16_t Bs[BN * LDR];      // [row of W][rank]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_k = (a.K + BK - 1) / BK;
    const int64_t n0 = (int64_t)(blockIdx.x / tiles_k) * BN;
    const int k0 = (int)(blockIdx.x % tiles_k) * BK;
    const int wn = (wave >> 1) * 32, wk = (wave & 1) * 64;
    const int lr = lane & 15, g = lane >> 4;
    const bf16_t* W0 = reinterpret_cast<const bf16_t*>(a.w0);
    bf16_t* out = reinterpret_cast<bf16_t*>(a.out);

    // the lane's chunks: (i, j) -> row n0 + wn + 16 i + lr, columns k0 + wk + 32 j + 8 g .. + 7
    const int64_t nl = n0 + wn + lr; const int kl = k0 + wk + 8 * g;
    Chunk16 w[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            w[i][j].u = (u32x4){0, 0, 0, 0};
            if (nl + 16 * i < a.N && kl + 32 * j < a.K) w[i][j].u = *reinterpret_cast<const u32x4*>(W0 + (nl + 16 * i) * a.K + kl + 32 * j);
        }

    f32x4 tot[2][2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) { tot[i][j][0] = (f32x4){0, 0, 0, 0}; tot[i][j][1] = (f32x4){0, 0, 0, 0}; }

    // As row of (span j, tile t) for this lane's MFMA row lr: column 8 (lr >> 2) + 4 t + (lr & 3) of the span
    const int arow = wk + 8 * (lr >> 2) + (lr & 3);
    const int nad = kOne ? 1 : a.n;                          // (one adapter: the running total is a constant zero until the only fma)
    for (int ad = 0; ad < nad; ++ad) {
        const bf16_t* At = reinterpret_cast<const bf16_t*>(a.At[ad]);
        const bf16_t* Bp = reinterpret_cast<const bf16_t*>(a.Bp[ad]);
        const int rp = a.r_pad[ad];
        f32x4 acc[2][2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) { acc[i][j][0] = (f32x4){0, 0, 0, 0}; acc[i][j][1] = (f32x4){0, 0, 0, 0}; }
        for (int r0 = 0; r0 < rp; r0 += RC) {
            const int rw = rp - r0 < RC ? rp - r0 : RC;      // 32 or 64 ranks in this stage
            __syncthreads();                                  // (the fragments of the stage before are read)
            for (int idx = tid; idx < BK * (RC / 8); idx += 256) {
                const int row = idx >> 3, p = (idx & 7) * 8;
                if (p < rw) {
                    u32x4 v = {0, 0, 0, 0};
                    if (k0 + row < a.K) v = *reinterpret_cast<const u32x4*>(At + (int64_t)(k0 + row) * rp + r0 + p);
                    *reinterpret_cast<u32x4*>(&As[row * LDR + p]) = v;
                }
            }
            for (int idx = tid; idx < BN * (RC / 8); idx += 256) {
                const int row = idx >> 3, p = (idx & 7) * 8;
                if (p < rw) {
                    u32x4 v = {0, 0, 0, 0};
                    if (n0 + row < a.N) v = *reinterpret_cast<const u32x4*>(Bp + (n0 + row) * rp + r0 + p);
                    *reinterpret_cast<u32x4*>(&Bs[row * LDR + p]) = v;
                }
            }
            __syncthreads();
            for (int rs = 0; rs < rw; rs += 32) {
                bf16x8 bf[2], af[2][2];
#pragma unroll
                for (int i = 0; i < 2; ++i) bf[i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(&Bs[(wn + 16 * i + lr) * LDR + rs + 8 * g]));
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int t = 0; t < 2; ++t) af[j][t] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(&As[(arow + 32 * j + 4 * t) * LDR + rs + 8 * g]));
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int t = 0; t < 2; ++t) acc[i][j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[j][t], bf[i], acc[i][j][t], 0, 0, 0);
            }
        }
        const float c = a.coef[ad];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int e = 0; e < 4; ++e) tot[i][j][t][e] = __builtin_fmaf(c, acc[i][j][t][e], tot[i][j][t][e]);
    }

    // D row 4 g + e of tile t is column 8 g + 4 t + e of the span: the lane's 8 consecutive columns are (t, e) in order
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (nl + 16 * i >= a.N || kl + 32 * j >= a.K) continue;
            Chunk16 o;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) o.h[4 * t + e] = (bf16_t)((float)w[i][j].h[4 * t + e] + tot[i][j][t][e]);
            *reinterpret_cast<u32x4*>(out + (nl + 16 * i) * a.K + kl + 32 * j) = o.u;
        }
}

__global__ __launch_bounds__(256) void lora_merge_f32_kernel(LoraMergeArgs a) {
    const float* W0 = reinterpret_cast<const float*>(a.w0);
    float* out = reinterpret_cast<float*>(a.out);
    const int kc = a.K >> 2;
    const int64_t chunks = a.N * kc;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = c / kc; const int k = (int)(c % kc) * 4;
        const f32x4 w = *reinterpret_cast<const f32x4*>(W0 + n * a.K + k);
        float tot[4] = {0.f, 0.f, 0.f, 0.f};
        for (int ad = 0; ad < a.n; ++ad) {
            const int rp = a.r_pad[ad];
            const float* Bp = reinterpret_cast<const float*>(a.Bp[ad]) + n * rp;
            const float* At = reinterpret_cast<const float*>(a.At[ad]) + (int64_t)k * rp;
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int r = 0; r < rp; r += 4) {
                const f32x4 b = *reinterpret_cast<const f32x4*>(Bp + r);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 x = *reinterpret_cast<const f32x4*>(At + (int64_t)j * rp + r);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[j] = __builtin_fmaf(b[e], x[e], acc[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) tot[j] = __builtin_fmaf(a.coef[ad], acc[j], tot[j]);
        }
        const f32x4 o = {w[0] + tot[0], w[1] + tot[1], w[2] + tot[2], w[3] + tot[3]};
        *reinterpret_cast<f32x4*>(out + n * a.K + k) = o;
    }
}

template <typename TD>
__global__ void lora_pack_kernel(const void* src, int sdt, TD* dst, int64_t rows, int r, int r_pad, int transpose) {
    const int64_t total = rows * r_pad;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / r_pad; const int j = (int)(i % r_pad);
        float v = 0.f;
        if (j < r) {
            const int64_t s = transpose ? (int64_t)j * rows + row : row * r + j;
            v = sdt == LTX_DT_BF16 ? (float)reinterpret_cast<const bf16_t*>(src)[s] : reinterpret_cast<const float*>(src)[s];
        }
        dst[i] = from_f32<TD>(v);
    }
}

inline unsigned blocks_for(int64_t n) { return ltx_grid1d(n, 16384); }

}  // namespace

int ltx_launch_lora_pack(const void* src, int sdt, void* dst, int ddt, int64_t rows, int r, int r_pad, int transpose, hipStream_t s) {
    if (!src || !dst || rows < 1 || r < 1 || r_pad < r) LTX_FAIL(LTX_ERR_ARG, "lora_pack: bad argument");
    if (ddt == LTX_DT_BF16) hipLaunchKernelGGL(lora_pack_kernel<bf16_t>, dim3(blocks_for(rows * r_pad)), dim3(256), 0, s, src, sdt, (bf16_t*)dst, rows, r, r_pad, transpose);
    else hipLaunchKernelGGL(lora_pack_kernel<float>, dim3(blocks_for(rows * r_pad)), dim3(256), 0, s, src, sdt, (float*)dst, rows, r, r_pad, transpose);
    LTX_CHECK_LAUNCH(); return LTX_OK;
}

int ltx_launch_lora_merge(const LoraMergeArgs& a, int dtype, hipStream_t s) {
    if (!a.w0 || !a.out || a.N < 1 || a.K < 8 || a.K % 8 != 0) LTX_FAIL(LTX_ERR_ARG, "lora_merge: w0 / out [N, K] with K a multiple of 8");
    if (a.n < 0 || a.n > kLoraMaxAdapters) LTX_FAIL(LTX_ERR_ARG, "lora_merge: at most 8 adapters");
    if (((uintptr_t)a.w0 | (uintptr_t)a.out) & 15) LTX_FAIL(LTX_ERR_ARG, "lora_merge: w0 / out must be 16-byte aligned");
    for (int i = 0; i < a.n; ++i) {
        if (!a.At[i] || !a.Bp[i] || a.r_pad[i] < 32 || a.r_pad[i] % 32 != 0 || a.r_pad[i] > kLoraMaxRank)
            LTX_FAIL(LTX_ERR_ARG, "lora_merge: packed operands with a rank padded to 32..256");
        if (((uintptr_t)a.At[i] | (uintptr_t)a.Bp[i]) & 15) LTX_FAIL(LTX_ERR_ARG, "lora_merge: operands must be 16-byte aligned");
    }
    if (dtype == LTX_DT_BF16) {
        const int64_t blocks = cdiv64(a.N, BN) * cdiv(a.K, BK);
        if (blocks > 0x7fffffffLL) LTX_FAIL(LTX_ERR_UNSUPPORTED, "lora_merge: matrix too large for one launch");
        if (a.n == 1) hipLaunchKernelGGL(lora_merge_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, a);
        else hipLaunchKernelGGL(lora_merge_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, a);
    } else {
        hipLaunchKernelGGL(lora_merge_f32_kernel, dim3(blocks_for(a.N * (a.K / 4))), dim3(256), 0, s, a);
    }
    LTX_CHECK_LAUNCH(); return LTX_OK;
}

extern "C" int ltx_op_lora_merge(const void* w0, void* out, int64_t N, int K, int n, const void* const* A, const void* const* B,
                                 const int* r, const float* coef, int dtype, ltx_stream stream) {
    if (!w0 || !out || w0 == out || N < 1 || K < 8 || K % 8 != 0) LTX_FAIL(LTX_ERR_ARG, "ltx_op_lora_merge: w0 / out [N, K], distinct, K a multiple of 8");
    if (n < 0 || n > kLoraMaxAdapters) LTX_FAIL(LTX_ERR_ARG, "ltx_op_lora_merge: 0..8 adapters");
    if (n > 0 && (!A || !B || !r || !coef)) LTX_FAIL(LTX_ERR_ARG, "ltx_op_lora_merge: null adapter arrays");
    for (int i = 0; i < n; ++i)
        if (!A[i] || !B[i] || r[i] < 1 || r[i] > kLoraMaxRank) LTX_FAIL(LTX_ERR_ARG, "ltx_op_lora_merge: adapter " + std::to_string(i) + ": null tensor or rank outside 1..256");
    const int dt = dtype == 1 ? LTX_DT_BF16 : LTX_DT_F32;
    const size_t esz = ltx_dt_size(dt);
    hipStream_t s = (hipStream_t)stream;
    LoraMergeArgs a; a.w0 = w0; a.out = out; a.N = N; a.K = K; a.n = n;
    std::vector<void*> tmp;
    int rc = LTX_OK;
    for (int i = 0; i < n && rc == LTX_OK; ++i) {
        const int rp = ltx_lora_rank_pad(r[i]);
        void *at = nullptr, *bp = nullptr;
        if (hipMalloc(&at, (size_t)K * rp * esz) != hipSuccess) { (void)hipGetLastError(); ltx_set_error("ltx_op_lora_merge: hipMalloc"); rc = LTX_ERR_HIP; break; }
        tmp.push_back(at);
        if (hipMalloc(&bp, (size_t)N * rp * esz) != hipSuccess) { (void)hipGetLastError(); ltx_set_error("ltx_op_lora_merge: hipMalloc"); rc = LTX_ERR_HIP; break; }
        tmp.push_back(bp);
        rc = ltx_launch_lora_pack(A[i], dt, at, dt, K, r[i], rp, 1, s);
        if (rc == LTX_OK) rc = ltx_launch_lora_pack(B[i], dt, bp, dt, N, r[i], rp, 0, s);
        a.At[i] = at; a.Bp[i] = bp; a.r_pad[i] = rp; a.coef[i] = coef[i];
    }
    if (rc == LTX_OK) rc = ltx_launch_lora_merge(a, dt, s);
    const hipError_t e = hipStreamSynchronize(s);
    for (void* p : tmp) (void)hipFree(p);
    if (rc != LTX_OK) return rc;
    if (e != hipSuccess) { ltx_set_error(std::string("ltx_op_lora_merge: ") + hipGetErrorString(e)); return LTX_ERR_HIP; }
    return LTX_OK;
}

// ---- adapter objects ---------------------------------------------------------------------------------------------------
namespace {

const char* const kLoraTargets[kLoraLinears] = {"attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k",
                                                "attn2.to_v", "attn2.to_out.0", "ff.net.0.proj", "ff.net.2"};

// "transformer_blocks.<i>.<target>" -> (i, which); false: not one of the ten block linears
bool lora_target(const std::string& module, int num_layers, int* block, int* which) {
    static const std::string pre = "transformer_blocks.";
    if (module.compare(0, pre.size(), pre) != 0) return false;
    size_t p = pre.size(), d = p; long idx = 0;
    while (d < module.size() && module[d] >= '0' && module[d] <= '9' && d - p < 6) { idx = idx * 10 + (module[d] - '0'); ++d; }
    if (d == p || d >= module.size() || module[d] != '.' || idx >= num_layers) return false;
    const std::string rest = module.substr(d + 1);
    for (int w = 0; w < kLoraLinears; ++w) if (rest == kLoraTargets[w]) { *block = (int)idx; *which = w; return true; }
    return false;
}

int read_scalar(const ltx_weight* w, const std::string& key, float* out) {
    if (ltx_numel(w) != 1 || !w->data) LTX_FAIL(LTX_ERR_ARG, "ltx_lora_create: '" + key + "' must hold one element");
    unsigned char raw[4] = {0, 0, 0, 0};
    const size_t nb = w->dtype == LTX_BF16 ? 2 : 4;
    if (w->on_device) HIP_TRY(hipMemcpy(raw, w->data, nb, hipMemcpyDeviceToHost));
    else memcpy(raw, w->data, nb);
    uint32_t bits = 0;
    if (w->dtype == LTX_BF16) { uint16_t h; memcpy(&h, raw, 2); bits = (uint32_t)h << 16; } else memcpy(&bits, raw, 4);
    memcpy(out, &bits, 4);
    return LTX_OK;
}

int upload_packed(const ltx_weight* w, int dtype, int64_t rows, int r, int r_pad, int transpose, void** out) {
    const void* src = nullptr; void* tmp = nullptr;
    LTX_TRY(ltx_stage_src(w, &src, &tmp));
    void* p = nullptr;
    if (hipMalloc(&p, (size_t)rows * r_pad * ltx_dt_size(dtype)) != hipSuccess) {
        (void)hipGetLastError(); if (tmp) (void)hipFree(tmp);
        LTX_FAIL(LTX_ERR_HIP, "ltx_lora_create: hipMalloc");
    }
    int rc = ltx_launch_lora_pack(src, w->dtype == LTX_BF16 ? LTX_DT_BF16 : LTX_DT_F32, p, dtype, rows, r, r_pad, transpose, 0);
    const hipError_t e = hipDeviceSynchronize();
    if (tmp) (void)hipFree(tmp);
    if (rc == LTX_OK && e != hipSuccess) { ltx_set_error(std::string("ltx_lora_create: ") + hipGetErrorString(e)); rc = LTX_ERR_HIP; }
    if (rc != LTX_OK) { (void)hipFree(p); return rc; }
    *out = p;
    return LTX_OK;
}

struct LoraTrio { const ltx_weight* t[3] = {nullptr, nullptr, nullptr}; std::string key[3]; int block = 0, which = 0; };

int lora_build(ltx_lora* l, const ltx_weight* tensors, size_t n, int strict, int* n_unmatched) {
    std::map<std::string, LoraTrio> mods;
    int unmatched = 0; std::string first_unmatched;
    for (size_t i = 0; i < n; ++i) {
        if (!tensors[i].name) continue;
        char mod[512]; int role = 0;
        if (ltx_lora_parse_key(tensors[i].name, mod, sizeof(mod), &role) != LTX_OK) continue;      // not an adapter key
        int block = 0, which = 0;
        if (!lora_target(mod, l->cfg.num_layers, &block, &which)) {
            if (!unmatched++) first_unmatched = tensors[i].name;
            continue;
        }
        LoraTrio& tr = mods[mod];
        if (tr.t[role]) LTX_FAIL(LTX_ERR_ARG, std::string("ltx_lora_create: '") + tensors[i].name + "' repeats '" + tr.key[role] + "'");
        tr.t[role] = &tensors[i]; tr.key[role] = tensors[i].name; tr.block = block; tr.which = which;
    }
    if (n_unmatched) *n_unmatched = unmatched;
    if (strict && unmatched) LTX_FAIL(LTX_ERR_UNSUPPORTED, "ltx_lora_create: '" + first_unmatched + "' is not on one of the ten block linears (strict)");
    if (mods.empty()) LTX_FAIL(LTX_ERR_MISSING_WEIGHT, "ltx_lora_create: no adapter tensors for the block linears");
    for (auto& kv : mods) {
        const LoraTrio& tr = kv.second;
        const ltx_weight *A = tr.t[0], *B = tr.t[1];
        if (!A || !B) {
            const std::string& have = A ? tr.key[0] : B ? tr.key[1] : tr.key[2];
            LTX_FAIL(LTX_ERR_ARG, "ltx_lora_create: '" + have + "' has no matching " + (A ? "B / up" : B ? "A / down" : "A / B") + " tensor");
        }
        int out = 0, in = 0;
        ltx_lora_linear_shape(l->cfg, tr.which, &out, &in);
        if (A->ndim != 2 || !A->data || A->shape[1] != in)
            LTX_FAIL(LTX_ERR_ARG, "ltx_lora_create: '" + tr.key[0] + "' must be [r, " + std::to_string(in) + "]");
        if (B->ndim != 2 || !B->data || B->shape[0] != out)
            LTX_FAIL(LTX_ERR_ARG, "ltx_lora_create: '" + tr.key[1] + "' must be [" + std::to_string(out) + ", r]");
        const int64_t r = A->shape[0];
        if (r < 1 || r > kLoraMaxRank) LTX_FAIL(LTX_ERR_ARG, "ltx_lora_create: '" + tr.key[0] + "': rank " + std::to_string(r) + " outside 1..256");
        if (B->shape[1] != r) LTX_FAIL(LTX_ERR_ARG, "ltx_lora_create: '" + tr.key[1] + "': rank " + std::to_string(B->shape[1]) + " does not match its A's " + std::to_string(r));
        LoraEntry e; e.block = tr.block; e.which = tr.which; e.r = (int)r; e.r_pad = ltx_lora_rank_pad((int)r);
        if (tr.t[2]) { float alpha = 0.f; LTX_TRY(read_scalar(tr.t[2], tr.key[2], &alpha)); e.factor = alpha / (float)r; }
        l->entries.push_back(e);                              // (pushed first: a failure below frees what was uploaded)
        LTX_TRY(upload_packed(A, l->dtype, in, (int)r, e.r_pad, 1, &l->entries.back().At));
        LTX_TRY(upload_packed(B, l->dtype, out, (int)r, e.r_pad, 0, &l->entries.back().Bp));
    }
    return LTX_OK;
}

}  // namespace

extern "C" void ltx_lora_destroy(ltx_lora* l) {
    if (!l) return;
    (void)hipSetDevice(l->device);
    (void)hipDeviceSynchronize();
    for (auto& e : l->entries) { if (e.At) (void)hipFree(e.At); if (e.Bp) (void)hipFree(e.Bp); }
    delete l;
}

extern "C" int ltx_lora_create(const ltx_dit* like, const ltx_weight* tensors, size_t n, int strict, ltx_lora** out, int* n_unmatched) {
    if (n_unmatched) *n_unmatched = 0;
    if (!like || !out || (n > 0 && !tensors)) LTX_FAIL(LTX_ERR_ARG, "ltx_lora_create: null argument");
    *out = nullptr;
    ltx_lora* l = new ltx_lora();
    ltx_dit_describe(like, &l->cfg, &l->dtype, &l->device);
    if (hipSetDevice(l->device) != hipSuccess) { (void)hipGetLastError(); delete l; LTX_FAIL(LTX_ERR_HIP, "ltx_lora_create: hipSetDevice"); }
    const int rc = lora_build(l, tensors, n, strict, n_unmatched);
    if (rc != LTX_OK) { ltx_lora_destroy(l); return rc; }
    *out = l;
    return LTX_OK;
}
