// What the row-norm kernels (rownorm.hip) and the q/k pass (qknorm_rope.hip) share: the lane mapping's constants, the two
// reductions, the row statistics of a 16-byte chunk and the three forms of 1 / rms.  The ORDER of additions and the form of
// 1 / rms decide the bits; each is written once here and differs between kernels only where a comment says so.
#pragma once
#include "common.h"

constexpr int NSLOT = 8;                                     // chunks (WIDE) or rows (NARROW) a lane holds in registers

// lanes per row: the power of two >= the row's 16-byte chunks, <= 64
inline int pick_lpr(int nch) {
    int lpr = 1;
    while (lpr < nch && lpr < 64) lpr <<= 1;
    return lpr;
}

// butterfly over the lpr lanes of a row
__device__ __forceinline__ float group_sum(float v, int lpr) {
    for (int o = lpr >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The one-row-per-block kernels' sum over 256 threads, N values at a time behind one barrier: lane butterfly, then the four wave
// sums in WAVE ORDER.  red: a [N][4] LDS array used for nothing else.
template <int N>
__device__ __forceinline__ void block_sum(float (&t)[N], float (*red)[4], int lane, int wave) {
#pragma unroll
    for (int n = 0; n < N; ++n) {
        t[n] = group_sum(t[n], 64);
        if (lane == 0) red[n][wave] = t[n];
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < N; ++n) t[n] = ((red[n][0] + red[n][1]) + red[n][2]) + red[n][3];
}
__device__ __forceinline__ float block_sum(float t, float (*red)[4], int lane, int wave) {
    float one[1] = {t};
    block_sum<1>(one, red, lane, wave);
    return one[0];
}

// ---- row statistics: ONE chunk added to the caller's RUNNING scalar (passed in, returned), element by element in ascending order (never a per-chunk
// subtotal: the order of additions runs across a lane's chunks).  A chunk outside the row holds zeros: the plain sums may take it,
// the squared deviations may not (0 - mean is not zero) - their callers guard with c < nch.
template <typename T>
__device__ __forceinline__ float add_sum(const Chunk16& v, float s) {                       // LayerNorm's mean
    constexpr int CH = ElemTraits<T>::CHUNK;
    float f[CH]; chunk_to_f32<T>(v, f);
#pragma unroll
    for (int j = 0; j < CH; ++j) s += f[j];
    return s;
}
template <typename T>
__device__ __forceinline__ float add_sqdev(const Chunk16& v, float mean, float ss) {        // row norms: (f - mean)^2, mean = 0 for RMS
    constexpr int CH = ElemTraits<T>::CHUNK;
    float f[CH]; chunk_to_f32<T>(v, f);
#pragma unroll
    for (int j = 0; j < CH; ++j) { const float d = f[j] - mean; ss += d * d; }
    return ss;
}
template <typename T>
__device__ __forceinline__ float add_sq(const Chunk16& v, float ss) {                       // q/k pass: f * f
    constexpr int CH = ElemTraits<T>::CHUNK;
    float f[CH]; chunk_to_f32<T>(v, f);
#pragma unroll
    for (int j = 0; j < CH; ++j) ss += f[j] * f[j];
    return ss;
}
// the same over a lane's N cached chunks (chunk i of the lane is row chunk c0 + i * step)
template <typename T, int N>
__device__ __forceinline__ float cached_sum(const Chunk16 (&v)[N]) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < N; ++i) s = add_sum<T>(v[i], s);
    return s;
}
template <typename T, int N>
__device__ __forceinline__ float cached_sqdev(const Chunk16 (&v)[N], float mean, int c0, int step, int nch) {
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < N; ++i) if (c0 + i * step < nch) ss = add_sqdev<T>(v[i], mean, ss);
    return ss;
}
template <typename T, int N>
__device__ __forceinline__ float cached_sq(const Chunk16 (&v)[N]) {
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < N; ++i) ss = add_sq<T>(v[i], ss);
    return ss;
}

// ---- 1 / rms: three forms, different in the last bits ON PURPOSE (each kernel keeps the one its results were recorded with)
// every row-norm kernel but the narrow mapping, and both presum kernels
__device__ __forceinline__ float rinv_div(float ss, float invD, float eps) { return 1.0f / sqrtf(ss * invD + eps); }
// rownorm_kernel's NARROW mapping (the VAE's voxel rows): the hardware reciprocal square root
__device__ __forceinline__ float rinv_rsq(float ss, float invD, float eps) { return __builtin_amdgcn_rsqf(ss * invD + eps); }
// the three q/k kernels: a division by D, and the output scale as the numerator
__device__ __forceinline__ float rinv_qk(float ss, int D, float eps, float oscale) { return oscale / sqrtf(ss / (float)D + eps); }
