// Hadamard rotation fused into the two int8 quantise passes of the W8A8 linears (include/ltxhip_int8_rot.h states the arithmetic).
//
//  hadamard_quant_rows_i8     : x [rows, D] bf16 -> q int8 [rows, D] of H x, scale[row] = (amax / 127) * out_scale.  Weights (out_scale
//                               = 1 / K) and the inputs of attn1.to_out and ff.net.2 (out_scale = 1).
//  rownorm_hadamard_quant_i8  : rownorm_quant_i8's modulated RMS norm; the f32 n is rotated in registers before the row maximum.
//
// H x is the unnormalised Walsh-Hadamard transform in Sylvester order, log2 D butterfly stages over the bits of the element index in
// ASCENDING order, every output one rounded f32 add or subtract: the stage order alone fixes the bits.  The rotated f32 row never goes
// to memory.
//
// Mapping: the row-owning one of quant_i8.hip (norm_common.h).  A lane holds NS chunks c = sub + i * lpr of 8 consecutive elements, so
// the element index is  chunk bits [0, 3) | lane bits [3, 3 + log2 lpr) | slot bits above  and ascending order is
//   1. three register stages inside each chunk,
//   2. the lane stages, by xor distance (the cost of the pass: 8 NS values per lane and stage):
//        1, 2   DPP quad_perm, folded into the add:                                  2 VALU per value
//        4      ds_swizzle bit mode (xor 4): the one distance no single DPP control reaches;  1 LDS-crossbar op + 2 VALU
//        8      DPP row_ror:8 (a rotation by half a row of 16 IS xor 8):                      2 VALU
//        16, 32 v_permlane16_swap / v_permlane32_swap on a PAIR of a lane's values: the swap turns the lane stage into a register stage
//               between the two (x' + y', x' - y'), a second swap puts the results back:      2 swaps + 2 VALU per PAIR, no select
//      (a partner's value is subtracted FROM on lanes with the bit set: partner - v == (-v) + partner, the negation is a sign-bit xor)
//   3. rows past 4096 columns take one row per block (c = tid + i * 256): the lane bits continue into two WAVE bits, both stages behind
//      one barrier per slot - each thread reads the four waves' values of its (lane, slot) from a double-buffered LDS strip and computes
//      stage 9 then stage 10 for its own wave (3 adds),
//   4. register stages across the slots.
// NS is a template parameter (1, 2, 4, 8): D is a power of two, so every slot of every lane is full and n[NS][8] never leaves the
// registers.  Every lane of a wave runs every exchange (rows past the end clamp to the last row and skip only the stores).  Every load
// of a lane is issued before its first store.  No matrix instruction: it would round the f32 operand or leave the summation order open.
#include <string>
#include "common.h"
#include "kernels.h"
#include "norm_common.h"
#include "quant_common.h"

namespace {

__device__ __forceinline__ float neg_if(float v, uint32_t signbit) { return __uint_as_float(__float_as_uint(v) ^ signbit); }

template <int CTRL>
__device__ __forceinline__ float dpp_of(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true)); }

// one lane stage on one value: v + partner on lanes with the bit clear, partner - v on lanes with it set (sign: 0x80000000 there, else 0)
template <int DIST>
__device__ __forceinline__ float lane_stage(float v, uint32_t sign) {
    float p;
    if (DIST == 1) p = dpp_of<0xB1>(v);                                                     // quad_perm:[1,0,3,2]
    else if (DIST == 2) p = dpp_of<0x4E>(v);                                                // quad_perm:[2,3,0,1]
    else if (DIST == 4) p = __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x101F));      // bit mode: and 0x1f, or 0, xor 4
    else p = dpp_of<0x128>(v);                                                              // row_ror:8
    return neg_if(v, sign) + p;
}

// the lane stage of distance 16 (WIDE = false) or 32 (true) on a pair of the lane's values
template <bool WIDE>
__device__ __forceinline__ void lanes_swap(float& a, float& b) {      // a's odd rows of 16 (WIDE: upper half) <-> b's even rows (lower half)
#if defined(__HIP_DEVICE_COMPILE__)
    const auto r = WIDE ? __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false)
                        : __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    a = __uint_as_float(r[0]); b = __uint_as_float(r[1]);
#endif
}
template <bool WIDE>
__device__ __forceinline__ void swap_stage(float& x, float& y) {
    lanes_swap<WIDE>(x, y);                        // x' = x on lanes with the bit clear, y of the partner below on the others; y' the other two
    float s = x + y, d = x - y;
    lanes_swap<WIDE>(s, d);
    x = s; y = d;
}

// stages 0 .. 2 (inside each chunk) and the lane stages of a row's lpr lanes
template <int NS>
__device__ __forceinline__ void fwht_chunk_lanes(float (&n)[NS][8], int lane, int lpr) {
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int h = 1; h < 8; h <<= 1)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (!(j & h)) { const float a = n[i][j], b = n[i][j + h]; n[i][j] = a + b; n[i][j + h] = a - b; }
    const uint32_t s1 = (uint32_t)(lane & 1) << 31, s2 = (uint32_t)(lane & 2) << 30, s4 = (uint32_t)(lane & 4) << 29, s8 = (uint32_t)(lane & 8) << 28;
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) n[i][j] = lane_stage<1>(n[i][j], s1);
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) n[i][j] = lane_stage<2>(n[i][j], s2);
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) n[i][j] = lane_stage<4>(n[i][j], s4);
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) n[i][j] = lane_stage<8>(n[i][j], s8);
    if (lpr > 16) {                                // uniform over the launch: every lane of the wave takes the swaps
#pragma unroll
        for (int i = 0; i < NS; ++i)
#pragma unroll
            for (int j = 0; j < 8; j += 2) swap_stage<false>(n[i][j], n[i][j + 1]);
    }
    if (lpr > 32) {
#pragma unroll
        for (int i = 0; i < NS; ++i)
#pragma unroll
            for (int j = 0; j < 8; j += 2) swap_stage<true>(n[i][j], n[i][j + 1]);
    }
}

// the stages over the slot bits
template <int NS>
__device__ __forceinline__ void fwht_slots(float (&n)[NS][8]) {
#pragma unroll
    for (int h = 1; h < NS; h <<= 1)
#pragma unroll
        for (int i = 0; i < NS; ++i)
            if (!(i & h)) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { const float a = n[i][j], b = n[i + h][j]; n[i][j] = a + b; n[i + h][j] = a - b; }
            }
}

// the two wave stages of the one-row-per-block form.  strip: [2][4][64][8] f32 of LDS used for nothing else
template <int NS>
__device__ __forceinline__ void fwht_waves(float (&n)[NS][8], float* strip, int lane, int wave) {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        float* buf = strip + (i & 1) * (4 * 64 * 8);               // double-buffered: one barrier per slot (a writer of slot i + 2 is past barrier i + 1)
        f32x4* mine = reinterpret_cast<f32x4*>(buf + (wave * 64 + lane) * 8);
        mine[0] = (f32x4){n[i][0], n[i][1], n[i][2], n[i][3]}; mine[1] = (f32x4){n[i][4], n[i][5], n[i][6], n[i][7]};
        __syncthreads();
        float w[4][8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const f32x4* src = reinterpret_cast<const f32x4*>(buf + (k * 64 + lane) * 8);
            const f32x4 lo = src[0], hi = src[1];
#pragma unroll
            for (int j = 0; j < 4; ++j) { w[k][j] = lo[j]; w[k][4 + j] = hi[j]; }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            // stage 9 (wave bit 0) for this wave's pair and for the pair two waves away, then stage 10 (wave bit 1)
            const float p = (wave & 1) ? w[0][j] - w[1][j] : w[0][j] + w[1][j];
            const float r = (wave & 1) ? w[2][j] - w[3][j] : w[2][j] + w[3][j];
            n[i][j] = (wave & 2) ? p - r : p + r;
        }
    }
}

template <int NS>
__device__ __forceinline__ float absmax_of(const float (&n)[NS][8]) {
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < NS; ++i) amax = absmax8(n[i], amax);
    return amax;
}

// one lane group (lpr lanes) per row, 64 / lpr rows per wave, four waves per block; D = 8 * NS * lpr
template <int NS>
__global__ __launch_bounds__(256) void hadamard_quant_rows_i8_kernel(const bf16_t* __restrict__ x, unsigned char* __restrict__ q, float* __restrict__ scale,
                                                                     int64_t rows, int D, int ld, int lpr, float out_scale) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rpw = 64 / lpr, sub = lane % lpr;
    const int64_t row = ((int64_t)blockIdx.x * 4 + wave) * rpw + lane / lpr;
    const bool active = row < rows;
    const int64_t rr = active ? row : rows - 1;
    const bf16_t* xr = x + rr * ld;
    Chunk16 v[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) v[i].u = *reinterpret_cast<const u32x4*>(xr + (sub + i * lpr) * 8);
    float n[NS][8];
#pragma unroll
    for (int i = 0; i < NS; ++i) chunk_to_f32<bf16_t>(v[i], n[i]);
    fwht_chunk_lanes<NS>(n, lane, lpr);
    fwht_slots<NS>(n);
    const float amax = group_max(absmax_of<NS>(n), lpr);
    const float inv = inv_of(amax);
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const u32x2 o = quant8(n[i], inv);
        if (active) *reinterpret_cast<u32x2*>(q + rr * D + (sub + i * lpr) * 8) = o;
    }
    if (active && sub == 0) scale[row] = (amax / 127.0f) * out_scale;
}

// one row per block: 256 threads x NS chunks, D = 2048 * NS (NS = 4, 8)
template <int NS>
__global__ __launch_bounds__(256) void hadamard_quant_rows_i8_block_kernel(const bf16_t* __restrict__ x, unsigned char* __restrict__ q, float* __restrict__ scale,
                                                                           int D, int ld, float out_scale) {
    __shared__ __attribute__((aligned(16))) float strip[2 * 4 * 64 * 8];
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = blockIdx.x;
    const bf16_t* xr = x + row * ld;
    Chunk16 v[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) v[i].u = *reinterpret_cast<const u32x4*>(xr + (tid + i * 256) * 8);
    float n[NS][8];
#pragma unroll
    for (int i = 0; i < NS; ++i) chunk_to_f32<bf16_t>(v[i], n[i]);
    fwht_chunk_lanes<NS>(n, lane, 64);
    fwht_waves<NS>(n, strip, lane, wave);
    fwht_slots<NS>(n);
    float amax = group_max(absmax_of<NS>(n), 64);
    if (lane == 0) red[wave] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float inv = inv_of(amax);
#pragma unroll
    for (int i = 0; i < NS; ++i) *reinterpret_cast<u32x2*>(q + row * D + (tid + i * 256) * 8) = quant8(n[i], inv);
    if (tid == 0) scale[row] = (amax / 127.0f) * out_scale;
}

// rownorm_quant_i8_kernel with the rotation between the norm's expression and the row maximum
template <int NS>
__global__ __launch_bounds__(256) void rownorm_hadamard_quant_i8_kernel(const RowNormArgs a, float* __restrict__ row_scale, int lpr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rpw = 64 / lpr, sub = lane % lpr, nch = a.D / 8;
    const int64_t row = ((int64_t)blockIdx.x * 4 + wave) * rpw + lane / lpr;
    const bool active = row < a.rows;
    const int64_t rr = active ? row : a.rows - 1;
    const bf16_t* xr = reinterpret_cast<const bf16_t*>(a.x) + rr * a.ldx;
    const int64_t g = rr / a.rows_per_batch;
    const float* sc = a.scale + g * a.mod_stride; const float* sh = a.shift + g * a.mod_stride;
    Chunk16 v[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) v[i].u = *reinterpret_cast<const u32x4*>(xr + (sub + i * lpr) * 8);
    const float rinv = rinv_div(group_sum(cached_sqdev<bf16_t>(v, 0.f, sub, lpr, nch), lpr), 1.0f / (float)a.D, a.eps);
    float n[NS][8];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int c = sub + i * lpr;
        float f[8]; chunk_to_f32<bf16_t>(v[i], f);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const f32x4 s4 = *reinterpret_cast<const f32x4*>(sc + c * 8 + 4 * h), h4 = *reinterpret_cast<const f32x4*>(sh + c * 8 + 4 * h);
#pragma unroll
            for (int j = 0; j < 4; ++j) n[i][4 * h + j] = (f[4 * h + j] * rinv) * (1.0f + s4[j]) + h4[j];      // rownorm.hip finish_chunk_regs' expression
        }
    }
    fwht_chunk_lanes<NS>(n, lane, lpr);
    fwht_slots<NS>(n);
    const float amax = group_max(absmax_of<NS>(n), lpr);
    const float inv = inv_of(amax);
    unsigned char* qr = reinterpret_cast<unsigned char*>(a.y) + rr * a.D;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const u32x2 o = quant8(n[i], inv);
        if (active) *reinterpret_cast<u32x2*>(qr + (sub + i * lpr) * 8) = o;
    }
    if (active && sub == 0) row_scale[row] = amax / 127.0f;
}

bool rot_width(int D, int hi) { return D >= 128 && D <= hi && (D & (D - 1)) == 0; }

}  // namespace

int ltx_launch_hadamard_quant_rows_i8(const void* x, int64_t rows, int D, int ld, float out_scale, void* q, float* scale, hipStream_t s) {
    if (!x || !q) LTX_FAIL(LTX_ERR_ARG, "hadamard_quant_rows_i8: null tensor");
    if (!scale) LTX_FAIL(LTX_ERR_ARG, "hadamard_quant_rows_i8: null scale");
    if (rows < 0 || D < 1 || ld < D) LTX_FAIL(LTX_ERR_ARG, "hadamard_quant_rows_i8: rows >= 0, D >= 1 and ld >= D");
    if (!(out_scale > 0.f) || out_scale > 3.0e38f) LTX_FAIL(LTX_ERR_ARG, "hadamard_quant_rows_i8: out_scale must be positive and finite");
    if (!rot_width(D, 16384)) LTX_FAIL(LTX_ERR_UNSUPPORTED, "hadamard_quant_rows_i8: D must be a power of two, 128 .. 16384 (got " + std::to_string(D) + ")");
    if (ld % 8 != 0 || ((uintptr_t)x & 15) || ((uintptr_t)q & 15) || ((uintptr_t)scale & 3)) LTX_FAIL(LTX_ERR_ARG, "hadamard_quant_rows_i8: misaligned pointer (x, q: 16 bytes, ld % 8 == 0)");
    if (rows == 0) return LTX_OK;
    if (rows > 2147483647LL) LTX_FAIL(LTX_ERR_UNSUPPORTED, "hadamard_quant_rows_i8: too many rows");
    const int nch = D / 8, lpr = pick_lpr(nch), ns = nch / lpr;      // ns: 1, 2, 4, 8 (row-owning) or 16, 32 (one row per block, 4 or 8 slots of 256 chunks)
    const bf16_t* xp = reinterpret_cast<const bf16_t*>(x); unsigned char* qp = reinterpret_cast<unsigned char*>(q);
    const dim3 grid((unsigned)cdiv64(rows, (int64_t)4 * (64 / lpr)));
    void* tok = nullptr;
    ltx_prof_begin(LTX_PROF_ROWNORM, 3.0 * (double)rows * D, s, &tok);
    ltx_prof_kernel(LTX_PROFK_HADAMARD_QUANT_ROWS_I8);
    switch (ns) {
        case 1: LTX_LAUNCH_TIMED(hadamard_quant_rows_i8_kernel<1>, grid, dim3(256), 0, s, xp, qp, scale, rows, D, ld, lpr, out_scale); break;
        case 2: LTX_LAUNCH_TIMED(hadamard_quant_rows_i8_kernel<2>, grid, dim3(256), 0, s, xp, qp, scale, rows, D, ld, lpr, out_scale); break;
        case 4: LTX_LAUNCH_TIMED(hadamard_quant_rows_i8_kernel<4>, grid, dim3(256), 0, s, xp, qp, scale, rows, D, ld, lpr, out_scale); break;
        case 8: LTX_LAUNCH_TIMED(hadamard_quant_rows_i8_kernel<8>, grid, dim3(256), 0, s, xp, qp, scale, rows, D, ld, lpr, out_scale); break;
        case 16: LTX_LAUNCH_TIMED(hadamard_quant_rows_i8_block_kernel<4>, dim3((unsigned)rows), dim3(256), 0, s, xp, qp, scale, D, ld, out_scale); break;
        default: LTX_LAUNCH_TIMED(hadamard_quant_rows_i8_block_kernel<8>, dim3((unsigned)rows), dim3(256), 0, s, xp, qp, scale, D, ld, out_scale); break;
    }
    ltx_prof_end(tok, s);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}

int ltx_launch_rownorm_hadamard_quant_i8(const RowNormArgs& a, float* row_scale, hipStream_t s) {
    if (!a.x || !a.y) LTX_FAIL(LTX_ERR_ARG, "rownorm_hadamard_quant_i8: null tensor");
    if (!row_scale || !a.scale || !a.shift) LTX_FAIL(LTX_ERR_ARG, "rownorm_hadamard_quant_i8: null scale (row_scale, and the modulation's scale and shift)");
    if (a.rows < 0 || a.D < 1 || a.ldx < a.D || a.rows_per_batch < 1 || a.mod_stride < a.D) LTX_FAIL(LTX_ERR_ARG, "rownorm_hadamard_quant_i8: rows >= 0, ld >= D >= 1, rows_per_batch >= 1, mod_stride >= D");
    if (!rot_width(a.D, 4096)) LTX_FAIL(LTX_ERR_UNSUPPORTED, "rownorm_hadamard_quant_i8: D must be a power of two, 128 .. 4096 (got " + std::to_string(a.D) + ")");
    if (a.kind != 0 || a.weight || a.act || a.presum || a.parts) LTX_FAIL(LTX_ERR_UNSUPPORTED, "rownorm_hadamard_quant_i8: the modulated RMS norm only");
    if (a.ldx % 8 != 0 || a.mod_stride % 4 != 0 || ((uintptr_t)a.x & 15) || ((uintptr_t)a.y & 15) || ((uintptr_t)a.scale & 15) || ((uintptr_t)a.shift & 15) || ((uintptr_t)row_scale & 3))
        LTX_FAIL(LTX_ERR_ARG, "rownorm_hadamard_quant_i8: misaligned pointer (h, q, shift, scale: 16 bytes, ld % 8 == 0, mod_stride % 4 == 0)");
    if (a.rows == 0) return LTX_OK;
    if (a.rows > 2147483647LL) LTX_FAIL(LTX_ERR_UNSUPPORTED, "rownorm_hadamard_quant_i8: too many rows");
    const int nch = a.D / 8, lpr = pick_lpr(nch), ns = nch / lpr;
    const dim3 grid((unsigned)cdiv64(a.rows, (int64_t)4 * (64 / lpr)));
    void* tok = nullptr;
    ltx_prof_begin(LTX_PROF_ROWNORM, 3.0 * (double)a.rows * a.D, s, &tok);
    ltx_prof_kernel(LTX_PROFK_ROWNORM_HADAMARD_QUANT_I8);
    switch (ns) {
        case 1: LTX_LAUNCH_TIMED(rownorm_hadamard_quant_i8_kernel<1>, grid, dim3(256), 0, s, a, row_scale, lpr); break;
        case 2: LTX_LAUNCH_TIMED(rownorm_hadamard_quant_i8_kernel<2>, grid, dim3(256), 0, s, a, row_scale, lpr); break;
        case 4: LTX_LAUNCH_TIMED(rownorm_hadamard_quant_i8_kernel<4>, grid, dim3(256), 0, s, a, row_scale, lpr); break;
        default: LTX_LAUNCH_TIMED(rownorm_hadamard_quant_i8_kernel<8>, grid, dim3(256), 0, s, a, row_scale, lpr); break;
    }
    ltx_prof_end(tok, s);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}
