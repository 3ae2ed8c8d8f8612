// Pieces the tiled attention kernels share (attention.hip: bf16 Q K^T; attn_i8.hip: int8 Q K^T): the tile sizes, the LDS chunk
// swizzles, the transpose read of V^T with its explicit wait, and the O^T store.  Everything here is internal to a translation unit.
#pragma once
#include <type_traits>
#include "common.h"

namespace {

constexpr int BQ = 128, BKV = 64;

typedef float f32x2 __attribute__((ext_vector_type(2)));
// Transpose read issued OUTSIDE the compiler's memory model: for the builtin form the wait-count pass cannot tell the
// read from the LDS-DMA writes of the other ring slots and drains vmcnt to 0 before the first one, which serialises
// the K/V prefetch with the softmax.  The asm form is waited for explicitly (lds_wait ties the registers).
template <int OFF> __device__ __forceinline__ u32x2 ds_tr_read(uint32_t addr) {
    u32x2 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}
template <int N> __device__ __forceinline__ void lds_wait(u32x2& a, u32x2& b) {
    asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N));
}
template <int I, int N, typename F> __device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) { f(std::integral_constant<int, I>{}); static_for<I + 1, N>(f); }
}

// K rows of CPR 16-byte chunks: the 32-row ds_read_b128 operand read (one logical chunk per row) is served 16 lanes - 256 bytes
// of banks - at a time, and 16 / CPR rows share one 256-byte line: XOR-ing the chunk with (row / (16 / CPR)) % CPR sends the 16
// rows of a group to 16 distinct 16-byte bank groups.  CPR = 16 (256-byte rows): c ^ (row % 16); 8 (128-byte rows): c ^ ((row / 2) % 8);
// 4 (the 64-byte int8 rows of attn_i8.hip at head_dim 64): four rows per line, c ^ ((row / 4) % 4).
template <int CPR> __device__ __forceinline__ int kswz(int row, int c) {
    if constexpr (CPR >= 4) { constexpr int RPB = 16 / CPR; return c ^ ((row / RPB) % CPR); }
    else return c;
}
template <int CPR> __device__ __forceinline__ int vswz(int row, int c) {
    if constexpr (CPR == 8) return c ^ (((row >> 1) & 1) << 2);
    else if constexpr (CPR == 16) return c ^ ((row & 3) << 2);
    else return c;
}

// O^T accumulators -> bf16 rows with 16-byte stores.  A lane holds, per 32-wide d block, four groups of 4 consecutive
// columns at 8*g4 + 4*h; lanes l and l^32 (h = 0 / 1) exchange one packed group per pair with v_permlane32_swap so
// that each ends up with 8 consecutive columns: four 16-byte stores per lane instead of eight 8-byte ones.
template <int NDB>
__device__ __forceinline__ void store_o_wide(const f32x16 (&acc_o)[NDB], float inv, bf16_t* O, int h) {
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            union { bf16x4 v; unsigned u[2]; } a, b;
            a.v = (bf16x4){(bf16_t)(acc_o[d][8 * k + 0] * inv), (bf16_t)(acc_o[d][8 * k + 1] * inv), (bf16_t)(acc_o[d][8 * k + 2] * inv), (bf16_t)(acc_o[d][8 * k + 3] * inv)};
            b.v = (bf16x4){(bf16_t)(acc_o[d][8 * k + 4] * inv), (bf16_t)(acc_o[d][8 * k + 5] * inv), (bf16_t)(acc_o[d][8 * k + 6] * inv), (bf16_t)(acc_o[d][8 * k + 7] * inv)};
            const auto s0 = __builtin_amdgcn_permlane32_swap(a.u[0], b.u[0], false, false);
            const auto s1 = __builtin_amdgcn_permlane32_swap(a.u[1], b.u[1], false, false);
            const u32x4 o = {s0[0], s1[0], s0[1], s1[1]};
            *reinterpret_cast<u32x4*>(O + d * 32 + 16 * k + 8 * h) = o;
        }
}
// the same rows with 8-byte stores (an output that is not 16-byte aligned)
template <int NDB>
__device__ __forceinline__ void store_o_narrow(const f32x16 (&acc_o)[NDB], float inv, bf16_t* O, int h) {
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const bf16x4 o4 = {(bf16_t)(acc_o[d][4 * g4 + 0] * inv), (bf16_t)(acc_o[d][4 * g4 + 1] * inv),
                               (bf16_t)(acc_o[d][4 * g4 + 2] * inv), (bf16_t)(acc_o[d][4 * g4 + 3] * inv)};
            *reinterpret_cast<bf16x4*>(O + d * 32 + 8 * g4 + 4 * h) = o4;
        }
}

}  // namespace
