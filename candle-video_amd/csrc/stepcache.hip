// The step cache's two kernels (include/ltxhip_stepcache.h; the cache object and the cached forward: dit.hip).
//
//  step_measure  : one HBM pass over h and prev [rows, D].  Per row the RMS norm of block 0 (the WIDE mapping of rownorm.hip: LPR lanes
//                  per row, the row in registers, cached_sqdev -> group_sum -> rinv_div) and the AdaLN modulate
//                  m = round_T(n * (1 + scale_g) + shift_g), g = row / rows_per_batch; sum |m - prev| and sum |prev| in f64; m replaces prev.
//                  Every lane issues all its loads of h and prev, then the modulation operands chunk by chunk, and only then its
//                  stores (gfx950 counts stores in vmcnt: a store in front of a load makes the load's wait a wait for the store).
//                  One f64 pair per block in a workspace, no atomics; step_measure_finish adds the pairs in one fixed tree (the
//                  scheme of the _ex guidance step, elementwise.hip): results repeat bit for bit.
//  step_residual : r = h - r in place, one 16-byte chunk per thread.
#include "common.h"
#include "kernels.h"
#include "norm_common.h"

namespace {

// the block's sum of NV doubles per thread: lanes by shuffles, the four waves through LDS in wave order; valid in threads 0 .. NV-1
template <int NV>
__device__ __forceinline__ double block_sum_f64(double (&acc)[NV], double (*sh)[NV]) {
#pragma unroll
    for (int q = 0; q < NV; ++q)
        for (int o = 32; o > 0; o >>= 1) acc[q] += __shfl_down(acc[q], o, 64);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) sh[threadIdx.x >> 6][q] = acc[q];
    }
    __syncthreads();
    const int q = threadIdx.x < NV ? threadIdx.x : 0;
    return ((sh[0][q] + sh[1][q]) + sh[2][q]) + sh[3][q];
}

template <typename T, int NS, bool FIRST>
__global__ __launch_bounds__(256) void step_measure_kernel(const StepMeasureArgs a, int lpr) {
    constexpr int CH = ElemTraits<T>::CHUNK;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rpw = 64 / lpr, sub = lane % lpr, nch = a.D / CH;
    const float invD = 1.0f / (float)a.D;
    const int64_t row = ((int64_t)blockIdx.x * 4 + wave) * rpw + lane / lpr;
    const bool active = row < a.rows;
    const int64_t rr = active ? row : a.rows - 1;             // (a row past the end reads the last one and neither counts nor stores)
    const T* x = reinterpret_cast<const T*>(a.h) + rr * a.D;
    T* pv = reinterpret_cast<T*>(a.prev) + rr * a.D;
    const int64_t g = rr / a.rows_per_batch;
    const float* sc = a.scale + g * a.mod_stride; const float* sh = a.shift + g * a.mod_stride;
    Chunk16 v[NS], q[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int c = sub + i * lpr;
        v[i].u = (u32x4){0u, 0u, 0u, 0u}; q[i].u = (u32x4){0u, 0u, 0u, 0u};
        if (c < nch) {
            v[i].u = *reinterpret_cast<const u32x4*>(x + c * CH);
            if (!FIRST) q[i].u = *reinterpret_cast<const u32x4*>(pv + c * CH);
        }
    }
    const float rinv = rinv_div(group_sum(cached_sqdev<T>(v, 0.f, sub, lpr, nch), lpr), invD, a.eps);
    double acc[2] = {0.0, 0.0};
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int c = sub + i * lpr;
        if (c >= nch) continue;
        float f[CH], scv[CH], shv[CH];
        chunk_to_f32<T>(v[i], f);
#pragma unroll
        for (int k = 0; k < CH / 4; ++k) {
            const f32x4 a4 = *reinterpret_cast<const f32x4*>(sc + c * CH + 4 * k), b4 = *reinterpret_cast<const f32x4*>(sh + c * CH + 4 * k);
#pragma unroll
            for (int j = 0; j < 4; ++j) { scv[4 * k + j] = a4[j]; shv[4 * k + j] = b4[j]; }
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) { const float n = f[j] * rinv; f[j] = n * (1.0f + scv[j]) + shv[j]; }      // rownorm.hip's finish_chunk_regs, mean 0
        f32_to_chunk<T>(f, v[i]);
        if (!FIRST && active) {
            float mf[CH], pf[CH];
            chunk_to_f32<T>(v[i], mf); chunk_to_f32<T>(q[i], pf);
#pragma unroll
            for (int j = 0; j < CH; ++j) { acc[0] += fabs((double)mf[j] - (double)pf[j]); acc[1] += fabs((double)pf[j]); }
        }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int c = sub + i * lpr;
        if (c < nch && active) *reinterpret_cast<u32x4*>(pv + c * CH) = v[i].u;
    }
    __shared__ double red[4][2];
    const double t = block_sum_f64<2>(acc, red);
    if (threadIdx.x < 2) a.part[(int64_t)blockIdx.x * 2 + threadIdx.x] = t;
}

// one block: thread k adds the pairs k, k + 256, ... in ascending order, then the tree above
__global__ __launch_bounds__(256) void step_measure_finish_kernel(const double* __restrict__ part, int64_t nblk, double* __restrict__ sums) {
    double acc[2] = {0.0, 0.0};
    for (int64_t k = threadIdx.x; k < nblk; k += 256) { acc[0] += part[2 * k]; acc[1] += part[2 * k + 1]; }
    __shared__ double red[4][2];
    const double t = block_sum_f64<2>(acc, red);
    if (threadIdx.x < 2) sums[threadIdx.x] = t;
}

template <typename T>
__global__ __launch_bounds__(256) void step_residual_kernel(const T* __restrict__ h, T* __restrict__ r, int64_t nchunks) {
    constexpr int CH = ElemTraits<T>::CHUNK;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nchunks) return;
    Chunk16 hv, rv;
    hv.u = *reinterpret_cast<const u32x4*>(h + i * CH); rv.u = *reinterpret_cast<const u32x4*>(r + i * CH);
    float hf[CH], rf[CH];
    chunk_to_f32<T>(hv, hf); chunk_to_f32<T>(rv, rf);
#pragma unroll
    for (int j = 0; j < CH; ++j) rf[j] = hf[j] - rf[j];
    f32_to_chunk<T>(rf, rv);
    *reinterpret_cast<u32x4*>(r + i * CH) = rv.u;
}

// slots per lane the row needs under the WIDE mapping (8 or 16); 0: D is not served
int measure_slots(int D, int dtype) {
    if (D < 128 || D % 128 != 0) return 0;
    const int nch = D / (dtype == LTX_DT_BF16 ? 8 : 4), per_lane = cdiv(nch, pick_lpr(nch));
    return per_lane <= 8 ? 8 : per_lane <= 16 ? 16 : 0;
}
int measure_rows_per_block(int D, int dtype) { return 4 * (64 / pick_lpr(D / (dtype == LTX_DT_BF16 ? 8 : 4))); }

template <typename T, int NS>
void launch_measure(const StepMeasureArgs& a, int lpr, unsigned blocks, hipStream_t s) {
    if (a.first) hipLaunchKernelGGL((step_measure_kernel<T, NS, true>), dim3(blocks), dim3(256), 0, s, a, lpr);
    else hipLaunchKernelGGL((step_measure_kernel<T, NS, false>), dim3(blocks), dim3(256), 0, s, a, lpr);
}
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int64_t ltx_step_measure_blocks(int64_t rows, int D, int dtype) {
    if (rows < 1 || !measure_slots(D, dtype)) return 0;
    return cdiv64(rows, measure_rows_per_block(D, dtype));
}

int ltx_launch_step_measure(const StepMeasureArgs& a, int dtype, hipStream_t s) {
    if (!a.h || !a.prev || !a.shift || !a.scale || !a.part) LTX_FAIL(LTX_ERR_ARG, "step_measure: null tensor");
    if (a.rows < 1 || a.rows_per_batch < 1) LTX_FAIL(LTX_ERR_ARG, "step_measure: rows and rows_per_batch must be at least 1");
    const int ns = measure_slots(a.D, dtype);
    if (!ns) LTX_FAIL(LTX_ERR_UNSUPPORTED, "step_measure: D = " + std::to_string(a.D) + " is not served (a multiple of 128, at most " + (dtype == LTX_DT_BF16 ? "8192 in bf16)" : "4096 in f32)"));
    if (a.mod_stride % 4 != 0 || !aligned16(a.h) || !aligned16(a.prev) || !aligned16(a.shift) || !aligned16(a.scale) || !aligned16(a.part))
        LTX_FAIL(LTX_ERR_ARG, "step_measure: tensors must be 16-byte aligned and mod_stride a multiple of 4");
    const int64_t blocks = ltx_step_measure_blocks(a.rows, a.D, dtype);
    if (blocks > 0x7fffffff) LTX_FAIL(LTX_ERR_UNSUPPORTED, "step_measure: too many rows for one launch");
    const int lpr = pick_lpr(a.D / (dtype == LTX_DT_BF16 ? 8 : 4));
    if (dtype == LTX_DT_BF16) { if (ns == 8) launch_measure<bf16_t, 8>(a, lpr, (unsigned)blocks, s); else launch_measure<bf16_t, 16>(a, lpr, (unsigned)blocks, s); }
    else { if (ns == 8) launch_measure<float, 8>(a, lpr, (unsigned)blocks, s); else launch_measure<float, 16>(a, lpr, (unsigned)blocks, s); }
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}

int ltx_launch_step_measure_finish(const double* part, int64_t nblk, double* sums, hipStream_t s) {
    if (!part || !sums || nblk < 1) LTX_FAIL(LTX_ERR_ARG, "step_measure_finish: bad argument");
    hipLaunchKernelGGL(step_measure_finish_kernel, dim3(1), dim3(256), 0, s, part, nblk, sums);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}

int ltx_launch_step_residual(const void* h, void* r, int64_t rows, int D, int dtype, hipStream_t s) {
    if (!h || !r || rows < 1 || D < 1) LTX_FAIL(LTX_ERR_ARG, "step_residual: bad argument");
    const int ch = dtype == LTX_DT_BF16 ? 8 : 4;
    if (D % ch != 0 || !aligned16(h) || !aligned16(r)) LTX_FAIL(LTX_ERR_ARG, "step_residual: rows must be a multiple of 16 bytes and the tensors 16-byte aligned");
    const int64_t nchunks = rows * (D / ch), blocks = cdiv64(nchunks, 256);
    if (blocks > 0x7fffffff) LTX_FAIL(LTX_ERR_UNSUPPORTED, "step_residual: too many elements for one launch");
    if (dtype == LTX_DT_BF16) hipLaunchKernelGGL(step_residual_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, s, reinterpret_cast<const bf16_t*>(h), reinterpret_cast<bf16_t*>(r), nchunks);
    else hipLaunchKernelGGL(step_residual_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s, reinterpret_cast<const float*>(h), reinterpret_cast<float*>(r), nchunks);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}
