// The quantisation rule of include/ltxhip_int8.h as device helpers, shared by quant_i8.hip (rows of the W8A8 linears) and
// quant_qk_i8.hip (the operands of the int8 Q K^T attention).
#pragma once
#include "common.h"

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

}  // namespace
