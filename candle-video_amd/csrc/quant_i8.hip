// Row-wise symmetric int8 quantisation for the W8A8 linear layers (include/ltxhip_int8.h states the arithmetic; HBM-bound passes).
//
//  quant_rows_i8     : x [rows, D] bf16 -> q int8 [rows, D] + scale f32 [rows].  Activations (attn1.to_out's and ff.net.2's inputs) and
//                      weights (a weight's rows are its output channels).
//  rownorm_quant_i8  : the block's modulated RMS norm, n = h * r * (1 + scale[g]) + shift[g], quantised from its f32 value: the norm
//                      pass in front of q | k | v and ff1 with int8 output (half the bytes written, no bf16 rounding of n).
//
// Mapping: the row-owning one of norm_common.h.  16-byte chunks of 8 bf16, LPR lanes per row (pick_lpr), a lane holds up to NSLOT
// chunks of ONE row in registers between the statistics and the write: one HBM read, one write of 8 bytes per chunk.  Rows wider than
// NSLOT * 64 chunks (the 13B model's ff.net.2 input, D = 16384) take one block per row.  Every load of a lane is issued before its
// first store (vmcnt counts stores on gfx950).  The row maximum is a max: no order of operations to pin; the norm's sum of squares is
// rownorm_kernel's (cached_sqdev, group_sum, rinv_div).
#include "common.h"
#include "kernels.h"
#include "norm_common.h"

namespace {

__device__ __forceinline__ float group_max(float v, int lpr) {
    for (int o = lpr >> 1; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float absmax8(const float* f, float m) {
#pragma unroll
    for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(f[j]));
    return m;
}
// q = clamp(rintf(x * inv), -127, 127), eight of them packed low byte first
__device__ __forceinline__ u32x2 quant8(const float* f, float inv) {
    uint32_t w[2] = {0u, 0u};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float r = fminf(fmaxf(rintf(f[j] * inv), -127.0f), 127.0f);
        w[j >> 2] |= ((uint32_t)(int)r & 255u) << (8 * (j & 3));
    }
    return (u32x2){w[0], w[1]};
}
__device__ __forceinline__ float inv_of(float amax) { return amax > 0.f ? 127.0f / amax : 0.f; }

// one lane group (lpr lanes) per row, 64 / lpr rows per wave, four waves per block
__global__ __launch_bounds__(256) void quant_rows_i8_kernel(const bf16_t* __restrict__ x, unsigned char* __restrict__ q, float* __restrict__ scale,
                                                            int64_t rows, int D, int ld, int lpr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rpw = 64 / lpr, sub = lane % lpr, nch = D / 8;
    const int64_t row = ((int64_t)blockIdx.x * 4 + wave) * rpw + lane / lpr;
    const bool active = row < rows;
    const int64_t rr = active ? row : rows - 1;
    const bf16_t* xr = x + rr * ld;
    Chunk16 v[NSLOT];
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) {
        const int c = sub + i * lpr;
        v[i].u = (u32x4){0u, 0u, 0u, 0u};
        if (c < nch) v[i].u = *reinterpret_cast<const u32x4*>(xr + c * 8);
    }
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) { float f[8]; chunk_to_f32<bf16_t>(v[i], f); amax = absmax8(f, amax); }
    amax = group_max(amax, lpr);
    const float inv = inv_of(amax);
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) {
        const int c = sub + i * lpr;
        float f[8]; chunk_to_f32<bf16_t>(v[i], f);
        const u32x2 o = quant8(f, inv);
        if (active && c < nch) *reinterpret_cast<u32x2*>(q + rr * D + c * 8) = o;
    }
    if (active && sub == 0) scale[row] = amax / 127.0f;
}

// one row per block: 256 threads x NSLOT chunks (rows of up to 2048 chunks)
__global__ __launch_bounds__(256) void quant_rows_i8_block_kernel(const bf16_t* __restrict__ x, unsigned char* __restrict__ q, float* __restrict__ scale, int D, int ld) {
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nch = D / 8;
    const int64_t row = blockIdx.x;
    const bf16_t* xr = x + row * ld;
    Chunk16 v[NSLOT];
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) {
        const int c = tid + i * 256;
        v[i].u = (u32x4){0u, 0u, 0u, 0u};
        if (c < nch) v[i].u = *reinterpret_cast<const u32x4*>(xr + c * 8);
    }
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) { float f[8]; chunk_to_f32<bf16_t>(v[i], f); amax = absmax8(f, amax); }
    amax = group_max(amax, 64);
    if (lane == 0) red[wave] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float inv = inv_of(amax);
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) {
        const int c = tid + i * 256;
        float f[8]; chunk_to_f32<bf16_t>(v[i], f);
        const u32x2 o = quant8(f, inv);
        if (c < nch) *reinterpret_cast<u32x2*>(q + row * D + c * 8) = o;
    }
    if (tid == 0) scale[row] = amax / 127.0f;
}

// rownorm_kernel's WIDE mapping with the finish replaced: the f32 n stays in registers, one more reduction (the row maximum), int8 out
__global__ __launch_bounds__(256) void rownorm_quant_i8_kernel(const RowNormArgs a, float* __restrict__ row_scale, int lpr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rpw = 64 / lpr, sub = lane % lpr, nch = a.D / 8;
    const int64_t row = ((int64_t)blockIdx.x * 4 + wave) * rpw + lane / lpr;
    const bool active = row < a.rows;
    const int64_t rr = active ? row : a.rows - 1;
    const bf16_t* xr = reinterpret_cast<const bf16_t*>(a.x) + rr * a.ldx;
    const int64_t g = rr / a.rows_per_batch;
    const float* sc = a.scale + g * a.mod_stride; const float* sh = a.shift + g * a.mod_stride;
    Chunk16 v[NSLOT];
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) {
        const int c = sub + i * lpr;
        v[i].u = (u32x4){0u, 0u, 0u, 0u};
        if (c < nch) v[i].u = *reinterpret_cast<const u32x4*>(xr + c * 8);
    }
    const float rinv = rinv_div(group_sum(cached_sqdev<bf16_t>(v, 0.f, sub, lpr, nch), lpr), 1.0f / (float)a.D, a.eps);
    float n[NSLOT][8];
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) {
        const int c = sub + i * lpr;
        float f[8]; chunk_to_f32<bf16_t>(v[i], f);
#pragma unroll
        for (int j = 0; j < 8; ++j) n[i][j] = 0.f;
        if (c < nch) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const f32x4 s4 = *reinterpret_cast<const f32x4*>(sc + c * 8 + 4 * h), h4 = *reinterpret_cast<const f32x4*>(sh + c * 8 + 4 * h);
#pragma unroll
                for (int j = 0; j < 4; ++j) n[i][4 * h + j] = (f[4 * h + j] * rinv) * (1.0f + s4[j]) + h4[j];      // rownorm.hip finish_chunk_regs' expression
            }
        }
        amax = absmax8(n[i], amax);
    }
    amax = group_max(amax, lpr);
    const float inv = inv_of(amax);
    unsigned char* qr = reinterpret_cast<unsigned char*>(a.y) + rr * a.D;
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) {
        const int c = sub + i * lpr;
        const u32x2 o = quant8(n[i], inv);
        if (active && c < nch) *reinterpret_cast<u32x2*>(qr + c * 8) = o;
    }
    if (active && sub == 0) row_scale[row] = amax / 127.0f;
}

}  // namespace

int ltx_launch_quant_rows_i8(const void* x, int64_t rows, int D, int ld, void* q, float* scale, hipStream_t s) {
    if (!x || !q) LTX_FAIL(LTX_ERR_ARG, "quant_rows_i8: null tensor");
    if (!scale) LTX_FAIL(LTX_ERR_ARG, "quant_rows_i8: null scale");
    if (rows < 0 || D < 1 || ld < D) LTX_FAIL(LTX_ERR_ARG, "quant_rows_i8: rows >= 0, D >= 1 and ld >= D");
    if (D % 16 != 0 || D > 16384) LTX_FAIL(LTX_ERR_UNSUPPORTED, "quant_rows_i8: D must be a multiple of 16, at most 16384");
    if (ld % 8 != 0 || ((uintptr_t)x & 15) || ((uintptr_t)q & 15) || ((uintptr_t)scale & 3)) LTX_FAIL(LTX_ERR_ARG, "quant_rows_i8: misaligned pointer (x, q: 16 bytes, ld % 8 == 0)");
    if (rows == 0) return LTX_OK;
    if (rows > 2147483647LL) LTX_FAIL(LTX_ERR_UNSUPPORTED, "quant_rows_i8: too many rows");
    const int nch = D / 8, lpr = pick_lpr(nch);
    void* tok = nullptr;
    ltx_prof_begin(LTX_PROF_ROWNORM, 3.0 * (double)rows * D, s, &tok);
    ltx_prof_kernel(LTX_PROFK_QUANT_ROWS_I8);
    if (nch <= NSLOT * lpr)
        LTX_LAUNCH_TIMED(quant_rows_i8_kernel, dim3((unsigned)cdiv64(rows, (int64_t)4 * (64 / lpr))), dim3(256), 0, s, reinterpret_cast<const bf16_t*>(x),
                         reinterpret_cast<unsigned char*>(q), scale, rows, D, ld, lpr);
    else
        LTX_LAUNCH_TIMED(quant_rows_i8_block_kernel, dim3((unsigned)rows), dim3(256), 0, s, reinterpret_cast<const bf16_t*>(x), reinterpret_cast<unsigned char*>(q), scale, D, ld);
    ltx_prof_end(tok, s);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}

int ltx_launch_rownorm_quant_i8(const RowNormArgs& a, float* row_scale, hipStream_t s) {
    if (!a.x || !a.y) LTX_FAIL(LTX_ERR_ARG, "rownorm_quant_i8: null tensor");
    if (!row_scale || !a.scale || !a.shift) LTX_FAIL(LTX_ERR_ARG, "rownorm_quant_i8: null scale (row_scale, and the modulation's scale and shift)");
    if (a.rows < 0 || a.D < 1 || a.ldx < a.D || a.rows_per_batch < 1 || a.mod_stride < a.D) LTX_FAIL(LTX_ERR_ARG, "rownorm_quant_i8: rows >= 0, ld >= D >= 1, rows_per_batch >= 1, mod_stride >= D");
    if (a.D % 16 != 0 || a.D > 4096) LTX_FAIL(LTX_ERR_UNSUPPORTED, "rownorm_quant_i8: D must be a multiple of 16, at most 4096");
    if (a.kind != 0 || a.weight || a.act || a.presum || a.parts) LTX_FAIL(LTX_ERR_UNSUPPORTED, "rownorm_quant_i8: the modulated RMS norm only");
    if (a.ldx % 8 != 0 || a.mod_stride % 4 != 0 || ((uintptr_t)a.x & 15) || ((uintptr_t)a.y & 15) || ((uintptr_t)a.scale & 15) || ((uintptr_t)a.shift & 15) || ((uintptr_t)row_scale & 3))
        LTX_FAIL(LTX_ERR_ARG, "rownorm_quant_i8: misaligned pointer (h, q, shift, scale: 16 bytes, ld % 8 == 0, mod_stride % 4 == 0)");
    if (a.rows == 0) return LTX_OK;
    if (a.rows > 2147483647LL) LTX_FAIL(LTX_ERR_UNSUPPORTED, "rownorm_quant_i8: too many rows");
    const int lpr = pick_lpr(a.D / 8);
    void* tok = nullptr;
    ltx_prof_begin(LTX_PROF_ROWNORM, 3.0 * (double)a.rows * a.D, s, &tok);
    ltx_prof_kernel(LTX_PROFK_ROWNORM_QUANT_I8);
    LTX_LAUNCH_TIMED(rownorm_quant_i8_kernel, dim3((unsigned)cdiv64(a.rows, (int64_t)4 * (64 / lpr))), dim3(256), 0, s, a, row_scale, lpr);
    ltx_prof_end(tok, s);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}
