// Row-wise normalisation kernels (HBM-bound; algorithmic bytes = read x once + write y once).
//
//  rownorm      : y = act( norm(x) [*w] * (1+scale_b) + shift_b )
//                 RMS  = RmsNorm::forward (ltx_transformer.rs:99-119; f32 statistics) fused with the
//                        AdaLN modulate of LtxVideoTransformerBlock::forward (:874-889, :912-927),
//                        and rmsnorm_channels_first + maybe_apply_scale_shift + SiLU of the VAE
//                        resnet (vae.rs:148-153, 711-739, 755-800) on channels-last rows.
//                 LN   = LayerNormNoParams (ltx_transformer.rs:72-79) + final modulation (:1149-1161).
//  (the q/k pass and the rotary tables: qknorm_rope.hip)
//
// Mapping: LPR lanes per row (pick_lpr), 64/LPR rows per wave, 4 waves per block; every lane moves 16 B per access.  The row
// lives in registers between the statistics pass and the write pass (one HBM read, one HBM write), and every lane issues all of
// its loads before the first reduction (memory-level parallelism instead of a dependent loop):
//   WIDE   rows (> LPR chunks): up to NSLOT chunks of ONE row per lane;
//   NARROW rows (<= LPR chunks, e.g. the VAE's 128..1024-channel voxels): NSLOT different rows per
//          lane group, one chunk each.
// Rows that do not fit NSLOT chunks per lane fall back to a re-reading variant (second read hits L2).
// Every kernel is the same four pieces (norm_common.h and below): the row statistics (add_sum / add_sqdev, reduced by group_sum or
// block_sum), one of the forms of 1 / rms (rinv_div; rinv_rsq for NARROW), the chunk's operands (load_chunk_operands) and its
// finish (finish_chunk_regs; finish_chunk = both).  The presum kernels take the statistic from presum_load / presum_rinv instead.
#include <type_traits>
#include "common.h"
#include "kernels.h"
#include "gemm_common.h"
#include "norm_common.h"
#include "options.h"

namespace {

// The finish of a chunk, operands (weight, scale, shift of ONE chunk) in registers: (f - mean) * rinv [* w] [* (1 + scale) + shift]
// [silu], rounded and stored at dst.  NT: streaming store.
template <typename T, bool NT = false>
__device__ __forceinline__ void finish_chunk_regs(const float* f_in, float mean, float rinv, bool has_w, bool has_mod, bool silu,
                                                  const float* wv, const float* scv, const float* shv, T* dst, bool active) {
    constexpr int CH = ElemTraits<T>::CHUNK;
    float f[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        float n = (f_in[i] - mean) * rinv;
        if (has_w) n *= wv[i];
        if (has_mod) n = n * (1.0f + scv[i]) + shv[i];
        if (silu) n = silu_f(n);
        f[i] = n;
    }
    Chunk16 o; f32_to_chunk<T>(f, o);
    if (active) {
        if constexpr (NT) __builtin_nontemporal_store(o.u, reinterpret_cast<u32x4*>(dst));
        else *reinterpret_cast<u32x4*>(dst) = o.u;
    }
}

template <typename T, bool NT = false>
__device__ __forceinline__ void finish_chunk_regs(const Chunk16& v, float mean, float rinv, bool has_w, bool has_mod, bool silu,
                                                  const float* wv, const float* scv, const float* shv, T* dst, bool active) {
    float f[ElemTraits<T>::CHUNK]; chunk_to_f32<T>(v, f);
    finish_chunk_regs<T, NT>(f, mean, rinv, has_w, has_mod, silu, wv, scv, shv, dst, active);
}

// the operands of chunk c for batch element b: the weight's, and scale / shift from b's rows
template <typename T>
__device__ __forceinline__ void load_chunk_operands(const RowNormArgs& a, int c, int64_t b, float* wv, float* scv, float* shv) {
    constexpr int CH = ElemTraits<T>::CHUNK;
    const T* w = reinterpret_cast<const T*>(a.weight);
    if (w) { Chunk16 wc; wc.u = *reinterpret_cast<const u32x4*>(w + c * CH); chunk_to_f32<T>(wc, wv); }
    if (a.scale) {
        const float* sc = a.scale + b * a.mod_stride; const float* sh = a.shift + b * a.mod_stride;
#pragma unroll
        for (int q = 0; q < CH / 4; ++q) {
            f32x4 a4 = *reinterpret_cast<const f32x4*>(sc + c * CH + 4 * q), b4 = *reinterpret_cast<const f32x4*>(sh + c * CH + 4 * q);
#pragma unroll
            for (int i = 0; i < 4; ++i) { scv[4 * q + i] = a4[i]; shv[4 * q + i] = b4[i]; }
        }
    }
}

// Load the chunk's operands, finish it.  The mappings that keep a lane on one chunk for several rows (NARROW, the presum kernels)
// load once, call finish_chunk_regs per row and load again only for a row of another batch element: 64 B of modulation per 16 B
// of data through the L1/TA path otherwise.
template <typename T>
__device__ __forceinline__ void finish_chunk(const RowNormArgs& a, const float* f_in, float mean, float rinv, int c, int64_t b, T* y, bool active) {
    constexpr int CH = ElemTraits<T>::CHUNK;
    float wv[CH], scv[CH], shv[CH];
    load_chunk_operands<T>(a, c, b, wv, scv, shv);
    finish_chunk_regs<T>(f_in, mean, rinv, a.weight != nullptr, a.scale != nullptr, a.act == 1, wv, scv, shv, y + c * CH, active);
}

template <typename T>
__device__ __forceinline__ void finish_chunk(const RowNormArgs& a, const Chunk16& v, float mean, float rinv, int c, int64_t b, T* y, bool active) {
    float f[ElemTraits<T>::CHUNK]; chunk_to_f32<T>(v, f);
    finish_chunk<T>(a, f, mean, rinv, c, b, y, active);
}

// RowNormArgs::presum: n partial sums of squares per row, written by the GEMM before it.
// up to 16 of a row's, loaded without a branch: a group of four past n re-reads the last one and is zeroed
__device__ __forceinline__ void presum_load(const float* presum, int64_t row, int n, f32x4 (&t)[4]) {
    const float* ps = presum + row * n;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const bool in = 4 * q < n;
        const f32x4 u = *reinterpret_cast<const f32x4*>(ps + (in ? 4 * q : n - 4));
        t[q] = in ? u : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
}
// 1 / rms from them, added in ascending order (groups past n add 0.0f, which changes no bit of a non-negative sum).  PAST16: rows
// of more than 16 partials (wider than the DiT's) take the rest from memory in a loop.
template <bool PAST16>
__device__ __forceinline__ float presum_rinv(const float* presum, int64_t row, int n, const f32x4 (&t)[4], int D, float eps) {
    float ss = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) { ss += t[q][0]; ss += t[q][1]; ss += t[q][2]; ss += t[q][3]; }
    if (PAST16 && n > 16) {
        const float* ps = presum + row * n;                   // (formed here, behind the test: it would stay live from the loads on)
        for (int g4 = 16; g4 < n; g4 += 4) {
            const f32x4 u = *reinterpret_cast<const f32x4*>(ps + g4);
            ss += u[0]; ss += u[1]; ss += u[2]; ss += u[3];
        }
    }
    return rinv_div(ss, 1.0f / (float)D, eps);
}

// RowNormArgs::parts: chunk c of a row that arrives as the K-range sums of the linear layer before it - finished with the layer's
// epilogue expression (gemm_common.h epilogue<>: v = sum + bias, then resid + gate * v or v + resid), rounded to T, written back
// as the new residual stream and returned for the norm.  Ranges added in part order: ((p0 + p1) + p2) + ... (gemm_big.hip).
// NP > 0: the number of ranges known at compile time (four: the shape rule's cut of K >= 8192 at <= 512 rows) - every range's loads are
// issued before the first add, 8 x 16 bytes in flight per chunk instead of one dependent pair at a time (this pass is pure latency at
// 384 rows: 14.6 us -> see docs/lab_notes.md R5.13); NP == 0: a.nparts at run time.  Same order of additions either way.
template <typename T, int NP = 0>
__device__ __forceinline__ Chunk16 deferred_chunk(const RowNormArgs& a, int64_t row, int64_t b, int c, bool active) {
    constexpr int CH = ElemTraits<T>::CHUNK;
    float v[CH];
    const float* pp = a.parts + row * a.D + c * CH;
    if constexpr (NP > 0) {
        f32x4 t[NP][CH / 4];
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int q = 0; q < CH / 4; ++q) t[p][q] = *reinterpret_cast<const f32x4*>(pp + (int64_t)p * a.part_stride + 4 * q);
#pragma unroll
        for (int q = 0; q < CH / 4; ++q) {
            f32x4 acc = t[0][q];
#pragma unroll
            for (int p = 1; p < NP; ++p) acc += t[p][q];
            v[4 * q] = acc[0]; v[4 * q + 1] = acc[1]; v[4 * q + 2] = acc[2]; v[4 * q + 3] = acc[3];
        }
    } else {
#pragma unroll
        for (int q = 0; q < CH / 4; ++q) { const f32x4 t = *reinterpret_cast<const f32x4*>(pp + 4 * q); v[4 * q] = t[0]; v[4 * q + 1] = t[1]; v[4 * q + 2] = t[2]; v[4 * q + 3] = t[3]; }
        for (int p = 1; p < a.nparts; ++p) {
            const float* pq = pp + (int64_t)p * a.part_stride;
#pragma unroll
            for (int q = 0; q < CH / 4; ++q) { const f32x4 t = *reinterpret_cast<const f32x4*>(pq + 4 * q); v[4 * q] += t[0]; v[4 * q + 1] += t[1]; v[4 * q + 2] += t[2]; v[4 * q + 3] += t[3]; }
        }
    }
    if (a.d_bias) {
        Chunk16 bc; bc.u = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(a.d_bias) + c * CH);
        float bf[CH]; chunk_to_f32<T>(bc, bf);
#pragma unroll
        for (int i = 0; i < CH; ++i) v[i] += bf[i];
    }
    Chunk16 rc; rc.u = *reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(a.x) + row * a.ldx + c * CH);
    float r[CH]; chunk_to_f32<T>(rc, r);
    if (a.d_gate) {
        const float* gp = a.d_gate + b * a.d_gate_stride + c * CH;
#pragma unroll
        for (int q = 0; q < CH / 4; ++q) {
            const f32x4 gt = *reinterpret_cast<const f32x4*>(gp + 4 * q);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[4 * q + i] = __builtin_fmaf(gt[i], v[4 * q + i], r[4 * q + i]);      // gemm_common.h epilogue<>: one rounding
        }
    } else {
#pragma unroll
        for (int i = 0; i < CH; ++i) v[i] += r[i];
    }
    Chunk16 o; f32_to_chunk<T>(v, o);
    if (active) *reinterpret_cast<u32x4*>(reinterpret_cast<T*>(a.x_out) + row * a.ldx + c * CH) = o.u;
    return o;
}

// MODE 0: WIDE (row cached in registers), 1: NARROW (NSLOT rows per lane group), 2: re-read fallback; DEFER (MODE 0): RowNormArgs::parts
template <typename T, int MODE, int DEFER = 0>          // DEFER: 0 no; 1: RowNormArgs::parts, a.nparts ranges; 4: four ranges (unrolled)
__global__ __launch_bounds__(256) void rownorm_kernel(const RowNormArgs a, int lpr) {
    constexpr int CH = ElemTraits<T>::CHUNK;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rpw = 64 / lpr;
    const int sub = lane % lpr;
    const int nch = a.D / CH;
    const float invD = 1.0f / (float)a.D;
    if constexpr (MODE == 1) {
        // a wave owns a contiguous block of NSLOT*rpw rows; slot i of a lane group is row0 + i*rpw.  Addresses advance by a
        // constant stride (no per-row 64-bit multiply), rows past the end are predicated off instead of clamped.
        const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * (rpw * NSLOT) + lane / lpr;
        const bool has = sub < nch;
        const T* xp = reinterpret_cast<const T*>(a.x) + row0 * a.ldx + sub * CH;
        T* yp = reinterpret_cast<T*>(a.y) + row0 * a.ldy;
        const int64_t xs = (int64_t)rpw * a.ldx, ys = (int64_t)rpw * a.ldy;
        Chunk16 v[NSLOT];
#pragma unroll
        for (int i = 0; i < NSLOT; ++i) {
            v[i].u = (u32x4){0u, 0u, 0u, 0u};
            if (has && row0 + i * rpw < a.rows) v[i].u = *reinterpret_cast<const u32x4*>(xp + i * xs);
        }
        // per-channel operands of this lane's chunk, for the batch of its first row (reloaded only if a row crosses a batch)
        float wv[CH], scv[CH], shv[CH];
        const int64_t b0 = (row0 < a.rows ? row0 : a.rows - 1) / a.rows_per_batch;      // ONE 64-bit division per lane
        const int64_t b0_end = (b0 + 1) * a.rows_per_batch;                               // first row of the next batch
        if (has) load_chunk_operands<T>(a, sub, b0, wv, scv, shv);
#pragma unroll
        for (int i = 0; i < NSLOT; ++i) {
            const int64_t row = row0 + (int64_t)i * rpw;
            const bool active = row < a.rows;
            // (this loop keeps the parent's text - the row expanded once, the sums written out: through add_sum / add_sqdev and
            // the chunk form of the finish the same arithmetic was scheduled 3 - 6 % slower on the VAE's rows, 92.9 against 87.7 us)
            float f[CH]; chunk_to_f32<T>(v[i], f);
            float mean = 0.f;
            if (a.kind == 1) {
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < CH; ++j) s += f[j];
                mean = group_sum(s, lpr) * invD;
            }
            float ss = 0.f;
            if (has) {
#pragma unroll
                for (int j = 0; j < CH; ++j) { float d = f[j] - mean; ss += d * d; }
            }
            ss = group_sum(ss, lpr);
            const float rinv = rinv_rsq(ss, invD, a.eps);
            if (has) {
                if (row < b0_end) finish_chunk_regs<T>(f, mean, rinv, a.weight != nullptr, a.scale != nullptr, a.act == 1, wv, scv, shv, yp + i * ys + sub * CH, active);
                else if (active) finish_chunk<T>(a, f, mean, rinv, sub, row / a.rows_per_batch, yp + i * ys, active);      // a row of a later batch (rare)
            }
        }
    } else {
        const int64_t row = ((int64_t)blockIdx.x * 4 + wave) * rpw + lane / lpr;
        const bool active = row < a.rows;
        const int64_t rr = active ? row : a.rows - 1;
        const T* x = reinterpret_cast<const T*>(a.x) + rr * a.ldx;
        T* y = reinterpret_cast<T*>(a.y) + rr * a.ldy;
        const int64_t b = rr / a.rows_per_batch;
        auto chunk = [&](int c) { Chunk16 v; v.u = *reinterpret_cast<const u32x4*>(x + c * CH); return v; };
        if constexpr (MODE == 0) {
            Chunk16 v[NSLOT];
#pragma unroll
            for (int i = 0; i < NSLOT; ++i) {
                int c = sub + i * lpr;
                v[i].u = (u32x4){0u, 0u, 0u, 0u};
                if constexpr (DEFER != 0) { if (c < nch) v[i] = deferred_chunk<T, DEFER == 4 ? 4 : 0>(a, rr, b, c, active); }
                else if (c < nch) v[i] = chunk(c);
            }
            float mean = 0.f;
            if (a.kind == 1) mean = group_sum(cached_sum<T>(v), lpr) * invD;
            const float rinv = rinv_div(group_sum(cached_sqdev<T>(v, mean, sub, lpr, nch), lpr), invD, a.eps);
#pragma unroll
            for (int i = 0; i < NSLOT; ++i) {
                int c = sub + i * lpr;
                if (c < nch) finish_chunk<T>(a, v[i], mean, rinv, c, b, y, active);
            }
        } else {
            float mean = 0.f;
            if (a.kind == 1) {
                float s = 0.f;
                for (int c = sub; c < nch; c += lpr) s = add_sum<T>(chunk(c), s);
                mean = group_sum(s, lpr) * invD;
            }
            float ss = 0.f;
            for (int c = sub; c < nch; c += lpr) ss = add_sqdev<T>(chunk(c), mean, ss);
            const float rinv = rinv_div(group_sum(ss, lpr), invD, a.eps);
            for (int c = sub; c < nch; c += lpr) finish_chunk<T>(a, chunk(c), mean, rinv, c, b, y, active);
        }
    }
}

#ifdef LTX_EXPERIMENTS
// Wide rows, several per wave, software-pipelined (round 4; measured negative, lab notes R4.4).  The one-row-per-wave form (MODE 0
// above) has every wave of the launch resident at once and therefore in the same phase: the chip first reads the whole matrix, then
// writes the whole result - 41 MB of the DiT's [4992, 2048] pass take 12.7 us where a pure elementwise map of the same bytes takes
// 6.6 us (tools/archive/norm_probe.py).  Here a wave walks R rows (row = wave + k * waves) with the loads of the next PD rows in
// flight while it reduces, modulates and stores the current one, so reads and writes overlap; each lane keeps the modulation
// operands of its NS chunks in registers when all rows of the wave share a batch element (they do for B = 1; otherwise they are
// re-loaded per row).  Per row the statistics and the finish are MODE 0's calls.
template <typename T, int NS, int R, int PD>
__global__ __launch_bounds__(256) void rownorm_rows_kernel(const RowNormArgs a, int total_waves) {
    constexpr int CH = ElemTraits<T>::CHUNK;
    static_assert(PD >= 1 && PD < R, "prefetch depth");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w0 = (int64_t)blockIdx.x * 4 + wave;
    const int nch = a.D / CH;
    const float invD = 1.0f / (float)a.D;
    auto row_of = [&](int k) { return w0 + (int64_t)k * total_waves; };
    Chunk16 v[PD + 1][NS];
    auto load_row = [&](int k, Chunk16 (&dst)[NS]) {
        const int64_t row = row_of(k);
        const bool in = row < a.rows;
        const T* x = reinterpret_cast<const T*>(a.x) + (in ? row : a.rows - 1) * a.ldx;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int c = lane + i * 64;
            dst[i].u = (u32x4){0u, 0u, 0u, 0u};
            if (in && c < nch) dst[i].u = *reinterpret_cast<const u32x4*>(x + c * CH);
        }
    };
    // operands of this lane's chunks for the batch element of the wave's first row
    const int64_t b_first = (row_of(0) < a.rows ? row_of(0) : a.rows - 1) / a.rows_per_batch;
    const int64_t last_row = row_of(R - 1) < a.rows ? row_of(R - 1) : a.rows - 1;
    const bool one_batch = last_row / a.rows_per_batch == b_first;
    float wv[NS][CH], scv[NS][CH], shv[NS][CH];
#pragma unroll
    for (int i = 0; i < NS; ++i)
        if (lane + i * 64 < nch) load_chunk_operands<T>(a, lane + i * 64, b_first, wv[i], scv[i], shv[i]);
#pragma unroll
    for (int k = 0; k < PD; ++k) load_row(k, v[k]);
#pragma unroll
    for (int k = 0; k < R; ++k) {
        if (k + PD < R) load_row(k + PD, v[(k + PD) % (PD + 1)]);
        Chunk16 (&cur)[NS] = v[k % (PD + 1)];
        const int64_t row = row_of(k);
        const bool active = row < a.rows;
        float mean = 0.f;
        if (a.kind == 1) mean = group_sum(cached_sum<T>(cur), 64) * invD;
        const float rinv = rinv_div(group_sum(cached_sqdev<T>(cur, mean, lane, 64, nch), 64), invD, a.eps);
        T* y = reinterpret_cast<T*>(a.y) + (active ? row : a.rows - 1) * a.ldy;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int c = lane + i * 64;
            if (c >= nch) continue;
            asm volatile("" : "+v"(cur[i].u));              // (keeps the f32 expansion of the statistics from living on: registers)
            if (!one_batch && active) load_chunk_operands<T>(a, c, row / a.rows_per_batch, wv[i], scv[i], shv[i]);
            finish_chunk_regs<T>(cur[i], mean, rinv, a.weight != nullptr, a.scale != nullptr, a.act == 1, wv[i], scv[i], shv[i], y + c * CH, active);
        }
    }
}
#endif

// RMS norm (+ weight, modulation, activation) of rows whose sums of squares are already known (RowNormArgs::presum, the
// by-product of the GEMM that wrote x): one thread per 16-byte chunk, no reduction, no wave waiting for a row - where the
// one-row-per-wave kernel takes 12.6 us for the DiT's [4992, 2048] pass, a pure map of the same bytes takes 6.5 us
// (tools/archive/norm_probe.py).  1 / rms: presum_rinv.
template <typename T, int R, bool WIDE, bool NT = false>       // WIDE: nch >= 64 (a wave lies inside one row group); NT: streaming hints on x and y
__global__ __launch_bounds__(256) void rownorm_presum_kernel(const RowNormArgs a, int nch, int rpb) {
    // block = rpb * R whole rows: thread (sub, c) owns 16-byte chunk c of rows row0 + sub * R .. + R - 1 (nch a power of two
    // <= 256, rpb = 256 / nch).  What bounds the row-reducing kernel is not its reduction but the vector-memory instruction
    // count: 64 B of f32 modulation operands per 16 B of data, re-loaded for every row (9 - 20 loads per 16 B chunk).  Here a
    // thread loads its chunk's operands ONCE for R rows, all R data chunks are in flight together, and 1 / rms comes from the
    // R lanes of each wave that sum the rows' partials (broadcast with readlane): 4 R + 8 memory instructions per R chunks.
    constexpr int CH = ElemTraits<T>::CHUNK;
    const int lane = threadIdx.x & 63;
    const int sub = threadIdx.x / nch, c = threadIdx.x - sub * nch;
    const int64_t row0 = ((int64_t)blockIdx.x * rpb + sub) * R;
    if (row0 >= a.rows) return;
    // Every load of the block is issued before anything waits: the R data chunks first, then the rows' partials (all of them at
    // once - a loop of "load 16 bytes, wait, add" paid one memory latency per four partials, four in a row at D = 2048, before the
    // data loads were even issued: 10.4 us per [4992, 2048] pass against 6.5 for a plain map of the same bytes), then the operands.
    Chunk16 v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t row = row0 + r < a.rows ? row0 + r : a.rows - 1;
        const u32x4* xp = reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(a.x) + row * a.ldx + c * CH);
        if constexpr (NT) v[r].u = __builtin_nontemporal_load(xp); else v[r].u = *xp;
    }
    // 1 / rms of the R rows of this thread: lanes 0 .. R-1 of the wave each sum one row's partials (a wave lies inside one sub
    // when nch >= 64; for narrower rows every lane does its own rows' sums).
    float rinv[R];
    auto in_rows = [&](int64_t row) { return row < a.rows ? row : a.rows - 1; };
    f32x4 pt[WIDE ? 1 : R][4];
    if constexpr (WIDE) { if (lane < R) presum_load(a.presum, in_rows(row0 + lane), a.presum_n, pt[0]); }
    else {
#pragma unroll
        for (int r = 0; r < R; ++r) presum_load(a.presum, in_rows(row0 + r), a.presum_n, pt[r]);
    }
    const uint32_t b0 = (uint32_t)row0 / (uint32_t)a.rows_per_batch;
    const int64_t last = row0 + R - 1 < a.rows ? row0 + R - 1 : a.rows - 1;
    const bool one_batch = (uint32_t)last / (uint32_t)a.rows_per_batch == b0;
    float wv[CH], scv[CH], shv[CH];
    load_chunk_operands<T>(a, c, b0, wv, scv, shv);
    if constexpr (WIDE) {
        float mine = 0.f;
        if (lane < R) mine = presum_rinv<true>(a.presum, in_rows(row0 + lane), a.presum_n, pt[0], a.D, a.eps);
#pragma unroll
        for (int r = 0; r < R; ++r) rinv[r] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine), r));
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r) rinv[r] = presum_rinv<true>(a.presum, in_rows(row0 + r), a.presum_n, pt[r], a.D, a.eps);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t row = row0 + r;
        const bool active = row < a.rows;
        T* y = reinterpret_cast<T*>(a.y) + (active ? row : a.rows - 1) * a.ldy;
        if (!one_batch && active && r > 0) load_chunk_operands<T>(a, c, (uint32_t)row / (uint32_t)a.rows_per_batch, wv, scv, shv);      // (rare: the row's own batch element)
        finish_chunk_regs<T, NT>(v[r], 0.f, rinv[r], a.weight != nullptr, a.scale != nullptr, a.act == 1, wv, scv, shv, y + c * CH, active);
    }
}

// The DiT's case of the map above with nothing left to decide at run time: bf16, a row of nch chunks
// (nch = 64 / 128 / 256), modulation present, no weight, no activation, groups of R rows inside one batch element, no ragged tail,
// at most 16 partials.  rownorm_presum_kernel serves every combination and runs ~550 instructions per wave at 20 000 waves per
// pass - as many issue cycles as the pass has memory time (a bare copy of the same bytes in the same geometry: 7.5 us; that
// kernel: 10.4-11.6, tools/archive/norm_diag.py).  The same presum_load / presum_rinv / finish_chunk_regs: same bits
// (tests/test_gpu_q2fold.py).
template <int R>
__global__ __launch_bounds__(256) void rownorm_presum_lean_kernel(const RowNormArgs a, int nch, int rpb) {
    const int lane = threadIdx.x & 63;
    const int sub = threadIdx.x / nch, c = threadIdx.x - sub * nch;
    const uint32_t row0 = ((uint32_t)blockIdx.x * (uint32_t)rpb + (uint32_t)sub) * R;
    const bf16_t* x = reinterpret_cast<const bf16_t*>(a.x) + (int64_t)row0 * a.ldx + c * 8;
    Chunk16 v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) v[r].u = *reinterpret_cast<const u32x4*>(x + (int64_t)r * a.ldx);
    f32x4 pt[4];
    if (lane < R) presum_load(a.presum, row0 + lane, a.presum_n, pt);
    const uint32_t b = row0 / (uint32_t)a.rows_per_batch;
    const float* sc = a.scale + (int64_t)b * a.mod_stride + c * 8; const float* sh = a.shift + (int64_t)b * a.mod_stride + c * 8;
    const f32x4 s0 = *reinterpret_cast<const f32x4*>(sc), s1 = *reinterpret_cast<const f32x4*>(sc + 4);
    const f32x4 h0 = *reinterpret_cast<const f32x4*>(sh), h1 = *reinterpret_cast<const f32x4*>(sh + 4);
    float mine = 0.f;
    if (lane < R) mine = presum_rinv<false>(a.presum, row0 + lane, a.presum_n, pt, a.D, a.eps);
    const float scv[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
    const float shv[8] = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
    bf16_t* y = reinterpret_cast<bf16_t*>(a.y) + (int64_t)row0 * a.ldy + c * 8;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float rinv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine), r));
        finish_chunk_regs<bf16_t>(v[r], 0.f, rinv, false, true, false, nullptr, scv, shv, y + (int64_t)r * a.ldy, true);
    }
}

#ifdef LTX_NORM_DIAG
// Diagnosis only (tools/norm_diag.py): what a streaming pass over [rows, D] bf16 costs in this library's launch geometry.
// var 0: copy, one 16-byte chunk per thread, consecutive threads consecutive chunks (grid = chunks / 256)
// var 1: the same, four chunks per thread 4 KiB apart (the presum kernel's pattern), var 2: four chunks per thread 256 x 16 B apart (a block's chunks contiguous)
__global__ __launch_bounds__(256) void norm_diag_kernel(const u32x4* __restrict__ x, u32x4* __restrict__ y, int64_t nchunks, int var, int rowchunks) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (var == 0) { if (t < nchunks) y[t] = x[t]; return; }
    u32x4 v[4];
    if (var == 1) {
        const int64_t row0 = (t / rowchunks) * 4, c = t % rowchunks;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = x[(row0 + r) * rowchunks + c];
#pragma unroll
        for (int r = 0; r < 4; ++r) y[(row0 + r) * rowchunks + c] = v[r];
    } else {
        const int64_t base = (int64_t)blockIdx.x * 1024 + threadIdx.x;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = x[base + r * 256];
#pragma unroll
        for (int r = 0; r < 4; ++r) y[base + r * 256] = v[r];
    }
}
extern "C" int ltx_dbg_norm_diag(const void* x, void* y, long long nchunks, int var, int rowchunks, void* stream) {
    const unsigned grid = (unsigned)(var == 0 ? (nchunks + 255) / 256 : nchunks / 1024);
    hipLaunchKernelGGL(norm_diag_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const u32x4*)x, (u32x4*)y, (int64_t)nchunks, var, rowchunks);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
#endif

// Canonical per-row partial sums of squares (GemmArgs::rowsq) of a stored matrix: one f32 per (row, 128-column group) =
// sequential sum over the group's 32 four-column leaves (ltx_rowsq_leaf), ascending.  The stand-alone form of what
// gemm_asm16's epilogue writes as a by-product - same order, same bits.  A wave takes 64 (row, group) pairs: in step c lane L
// would read leaf c of pair L (uncoalesced), so the roles are transposed through LDS: each half-wave reads ONE pair's 256
// contiguous bytes (bf16) per step, writes its 32 leaves, and after 32 steps every lane sums one pair's leaves in order.
template <typename T>
__global__ __launch_bounds__(256) void rowsq_kernel(const T* x, int64_t rows, int N, int ld, float* out) {
    __shared__ float leaves[4][64][33];                    // [wave][pair][leaf] (+1: conflict-free column reads)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, cg = lane & 31;
    const int ng = (N + 127) / 128;
    const int64_t npairs = rows * ng;
    const int64_t p0 = ((int64_t)blockIdx.x * 4 + wave) * 64;
#pragma unroll 4
    for (int st = 0; st < 32; ++st) {
        const int64_t pr = p0 + 2 * st + half;
        float leaf = 0.f;
        if (pr < npairs) {
            const int64_t row = pr / ng; const int g = (int)(pr - row * ng);
            const int n = g * 128 + 4 * cg;
            if (n < N) {                                   // N % 4 == 0: a leaf is inside or outside as a whole
                if constexpr (std::is_same<T, float>::value) leaf = ltx_rowsq_leaf(*reinterpret_cast<const f32x4*>(x + row * ld + n));
                else leaf = ltx_rowsq_leaf(*reinterpret_cast<const bf16x4*>(x + row * ld + n));
            }
        }
        leaves[wave][2 * st + half][cg] = leaf;
    }
    __syncthreads();
    const int64_t pr = p0 + lane;
    if (pr < npairs) {
        float s = leaves[wave][lane][0];
#pragma unroll
        for (int c = 1; c < 32; ++c) s += leaves[wave][lane][c];
        out[pr] = s;
    }
}

// Few rows (C1's 384 tokens, the 128 text rows of T5): ONE ROW PER BLOCK, a chunk (two beyond 2048 columns) per thread.  With a wave per
// row such a pass is 384 waves on 256 CUs, each walking a dependent chain of four chunks (and, finishing deferred K ranges, 1 KiB of
// loads per lane): pure latency - 7.0 us plain, 14.6 us with four ranges.  Four waves per row quarter the chain and put 4 x the loads
// in flight.  Row statistic: block_sum - the plain and the deferred form share it, so finishing the ranges here returns the bits of
// in-launch reduction + this norm (tests/test_gpu_defer.py).
template <typename T, int DEFER>          // DEFER: 0 no; 1: a.nparts ranges; 4: four ranges (unrolled)
__global__ __launch_bounds__(256) void rownorm_block_kernel(const RowNormArgs a) {
    constexpr int CH = ElemTraits<T>::CHUNK, NC = 2;
    __shared__ float red[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = blockIdx.x;
    const int nch = a.D / CH;
    const float invD = 1.0f / (float)a.D;
    const T* x = reinterpret_cast<const T*>(a.x) + row * a.ldx;
    T* y = reinterpret_cast<T*>(a.y) + row * a.ldy;
    const int64_t b = row / a.rows_per_batch;
    Chunk16 v[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = tid + i * 256;
        v[i].u = (u32x4){0u, 0u, 0u, 0u};
        if (c < nch) {
            if constexpr (DEFER != 0) v[i] = deferred_chunk<T, DEFER == 4 ? 4 : 0>(a, row, b, c, true);
            else v[i].u = *reinterpret_cast<const u32x4*>(x + c * CH);
        }
    }
    float mean = 0.f;
    if (a.kind == 1) mean = block_sum(cached_sum<T>(v), red, lane, wave) * invD;
    const float rinv = rinv_div(block_sum(cached_sqdev<T>(v, mean, tid, 256, nch), red + 1, lane, wave), invD, a.eps);
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = tid + i * 256;
        if (c < nch) finish_chunk<T>(a, v[i], mean, rinv, c, b, y, true);
    }
}
// The launches of ltx_rownorm_route's answers: nothing is decided here.
template <typename T>
void launch_rownorm_t(const RowNormArgs& a, const NormDecision& d, int lpr, int nch, hipStream_t s) {
    const int rpw = 64 / lpr;
    const dim3 block_grid((unsigned)a.rows);                                     // one row per block
    const dim3 wave_grid((unsigned)cdiv64(a.rows, (int64_t)4 * rpw));            // rpw rows per wave
    switch (d.route) {
    case NORM_NARROW: {                                                          // NSLOT rows per lane group
        const int64_t rows_per_block = (int64_t)4 * rpw * NSLOT;
        LTX_LAUNCH_TIMED((rownorm_kernel<T, 1>), dim3((unsigned)cdiv64(a.rows, rows_per_block)), dim3(256), 0, s, a, lpr);
        break;
    }
    case NORM_BLOCK: LTX_LAUNCH_TIMED((rownorm_block_kernel<T, 0>), block_grid, dim3(256), 0, s, a); break;
    case NORM_BLOCK_DEFER: LTX_LAUNCH_TIMED((rownorm_block_kernel<T, 1>), block_grid, dim3(256), 0, s, a); break;
    case NORM_BLOCK_DEFER4: LTX_LAUNCH_TIMED((rownorm_block_kernel<T, 4>), block_grid, dim3(256), 0, s, a); break;
    // (measured and left out, round 3: four rows per wave with the scale / shift operands cached in registers - 312 blocks
    // instead of 1248 - ran the DiT's 4992 x 2048 rows in 15.9 us against 12.8 us: the pass is bound by how many row loads are
    // in flight across the chip, not by the operand traffic through the vector-memory path)
#ifdef LTX_EXPERIMENTS     // x_rownorm_rows=1: four rows per wave, two in flight; measured 17.3 us against 12.7 us (lab notes R4.4)
    case NORM_WIDE_ROWS: {
        constexpr int R = 4;
        const int waves = (int)cdiv64(a.rows, R);
        const int blocks = (waves + 3) / 4;
        LTX_LAUNCH_TIMED((rownorm_rows_kernel<T, 4, R, 2>), dim3((unsigned)blocks), dim3(256), 0, s, a, blocks * 4);
        break;
    }
#endif
    case NORM_WIDE_DEFER4: LTX_LAUNCH_TIMED((rownorm_kernel<T, 0, 4>), wave_grid, dim3(256), 0, s, a, lpr); break;
    case NORM_WIDE_DEFER: LTX_LAUNCH_TIMED((rownorm_kernel<T, 0, 1>), wave_grid, dim3(256), 0, s, a, lpr); break;
    case NORM_WIDE: {
        int shm = 0;
#ifdef LTX_EXPERIMENTS
        // x_rownorm_occ=n: at most n blocks per CU, by asking for 160 KiB / n of LDS the kernel never touches - several
        // generations of blocks instead of one, so that the stores of one overlap the loads of the next
        { const int n = ltx_exp("rownorm_occ", 0); if (n >= 1 && n <= 8) shm = 163840 / n - 1024; }
        if (shm > 65536) {
            static std::atomic<unsigned long long> occ_devs{0};
            (void)ltx_set_max_dyn_smem(occ_devs, reinterpret_cast<const void*>(&rownorm_kernel<T, 0>), 163840);
        }
#endif
        LTX_LAUNCH_TIMED((rownorm_kernel<T, 0>), wave_grid, dim3(256), shm, s, a, lpr);
        break;
    }
    case NORM_REREAD: LTX_LAUNCH_TIMED((rownorm_kernel<T, 2>), wave_grid, dim3(256), 0, s, a, lpr); break;
    default: break;                                                              // (the presum routes: launch_presum)
    }
}

template <typename T, int R>
void launch_presum_r(const RowNormArgs& a, const NormDecision& d, int nch, int rpb, hipStream_t s) {
    const dim3 grid((unsigned)cdiv64(a.rows, (int64_t)rpb * R));
    if (d.presum_wide) LTX_LAUNCH_TIMED((rownorm_presum_kernel<T, R, true>), grid, dim3(256), 0, s, a, nch, rpb);
    else LTX_LAUNCH_TIMED((rownorm_presum_kernel<T, R, false>), grid, dim3(256), 0, s, a, nch, rpb);
}

void launch_presum(const RowNormArgs& a, const NormDecision& d, int dtype, int nch, hipStream_t s) {
    const int rpb = 256 / nch;
    const dim3 grid4((unsigned)cdiv64(a.rows, (int64_t)rpb * 4));
    if (d.route == NORM_PRESUM_LEAN) LTX_LAUNCH_TIMED((rownorm_presum_lean_kernel<4>), grid4, dim3(256), 0, s, a, nch, rpb);
    else if (dtype != LTX_DT_BF16) launch_presum_r<float, 4>(a, d, nch, rpb, s);
#ifdef LTX_EXPERIMENTS     // x_norm_nt, x_norm_presum_r = 2 / 8: measured, not faster (the shipped decision never sets presum_nt or another presum_r)
    else if (d.presum_nt) LTX_LAUNCH_TIMED((rownorm_presum_kernel<bf16_t, 4, true, true>), grid4, dim3(256), 0, s, a, nch, rpb);
    else if (d.presum_r == 2) launch_presum_r<bf16_t, 2>(a, d, nch, rpb, s);
    else if (d.presum_r == 8) launch_presum_r<bf16_t, 8>(a, d, nch, rpb, s);
#endif
    else launch_presum_r<bf16_t, 4>(a, d, nch, rpb, s);
}

NormDecision refuse_norm(const char* why) { NormDecision d; d.route = NORM_REFUSED; d.why = why; return d; }

}  // namespace

NormRouteArgs ltx_rownorm_route_args(const RowNormArgs& a, int dtype) {
    NormRouteArgs r;
    r.dtype = dtype; r.rows = a.rows; r.D = a.D; r.kind = a.kind;
    r.scale = a.scale != nullptr; r.shift = a.shift != nullptr; r.weight = a.weight != nullptr; r.act = a.act; r.rows_per_batch = a.rows_per_batch;
    r.presum = a.presum != nullptr; r.presum_n = a.presum_n; r.parts = a.parts != nullptr; r.nparts = a.nparts;
    return r;
}

// The one place where a row-norm call's kernel is chosen (kernels.h).  Shape thresholds, in this order:
//   narrow : the row fits one chunk per lane of its lane group (nch <= lpr) and there are >= 2048 * (64 / lpr) rows
//   block  : at most 512 rows of 65 .. 512 chunks
//   wide   : the row fits NSLOT chunks per lane;  reread: it does not
NormDecision ltx_rownorm_route(const NormRouteArgs& r) {
    NormDecision d;
    const int ch = r.dtype == LTX_DT_BF16 ? 8 : 4;
    if (r.D < ch || r.D % ch != 0) return refuse_norm("rownorm: D/ld must be multiples of the 16-byte chunk");
    if (r.scale != r.shift) return refuse_norm("rownorm: scale and shift go together");
    const int nch = r.D / ch, lpr = pick_lpr(nch), rpw = 64 / lpr;
    const bool narrow = nch <= lpr && r.rows >= (int64_t)rpw * NSLOT * 4 * 64;           // narrow rows, enough of them
    const bool block_rows = r.rows <= 512 && nch > 64 && nch <= 512;                      // few wide rows: one row per block
    const bool cached = nch <= NSLOT * lpr;
    if (r.parts && (r.presum || narrow || (!cached && !block_rows) || r.nparts < 1 || r.nparts > 16 || r.D % 8))
        return refuse_norm("rownorm: deferred rows need whole-row lanes (D of at most 64 x 8 chunks), 1..16 parts of [rows, D] f32 and an output for the finished rows");
    if (r.presum && (r.kind != 0 || r.presum_n < 4 || r.presum_n % 4 != 0 || nch > 256 || (nch & (nch - 1)) || r.rows >= 2147483647LL || r.rows_per_batch >= 2147483647LL))
        return refuse_norm("rownorm: presum serves RMS rows of a power-of-two number (<= 256) of 16-byte chunks with a multiple of 4 partials");
    if (r.presum) {
        const int rpb = 256 / nch;
        int R = 4;                                           // rows per thread (LTX_NORM_PRESUM_R = 2 / 4 / 8: tuning aid; bf16)
        if (r.dtype == LTX_DT_BF16) { const int v = ltx_exp("norm_presum_r", 4); if (v == 2 || v == 4 || v == 8) R = v; }
        const bool wide = nch >= 64;
        // the DiT's case on the kernel that has nothing to decide (LTX_NORM_LEAN=0: the general one; same bits)
        const bool lean_on = ltx_opt().norm_lean != 0, nt = ltx_exp("norm_nt", 0) != 0;
        const bool lean = lean_on && r.dtype == LTX_DT_BF16 && wide && R == 4 && r.scale && !r.weight && r.act == 0 && r.presum_n <= 16 &&
                          r.rows % ((int64_t)rpb * 4) == 0 && r.rows_per_batch % 4 == 0 && !nt;
        d.route = lean ? NORM_PRESUM_LEAN : NORM_PRESUM;
        d.presum_r = R; d.presum_wide = wide; d.presum_nt = r.dtype == LTX_DT_BF16 && R == 4 && wide && nt;
        return d;
    }
    if (narrow) d.route = NORM_NARROW;
    else if (block_rows) d.route = !r.parts ? NORM_BLOCK : (r.nparts == 4 ? NORM_BLOCK_DEFER4 : NORM_BLOCK_DEFER);
#ifdef LTX_EXPERIMENTS
    // wide rows (one wave per row, <= 4 chunks per lane), enough of them: four rows per wave, two in flight
    else if (lpr == 64 && nch <= 4 * 64 && r.rows >= 2048 && ltx_exp("rownorm_rows", 0) == 1) d.route = NORM_WIDE_ROWS;
#endif
    else if (r.parts) d.route = r.nparts == 4 ? NORM_WIDE_DEFER4 : NORM_WIDE_DEFER;      // (checked above: the row fits the lanes)
    else d.route = cached ? NORM_WIDE : NORM_REREAD;
    return d;
}

const char* ltx_rownorm_route_name(NormRoute r) {
    static const char* const names[] = {"refused", "narrow", "block", "wide", "reread", "presum", "presum_lean",
                                        "wide_defer", "wide_defer4", "block_defer", "block_defer4", "wide_rows"};
    return names[r];
}

int ltx_launch_rownorm(const RowNormArgs& a, int dtype, hipStream_t s) {
    const int ch = dtype == LTX_DT_BF16 ? 8 : 4;
    if (a.rows <= 0) return LTX_OK;
    if (a.D % ch != 0 || a.ldx % ch != 0 || a.ldy % ch != 0) LTX_FAIL(LTX_ERR_ARG, "rownorm: D/ld must be multiples of the 16-byte chunk");
    // (every argument check sits in front of ltx_prof_begin: a failure after it would leave the timing record open)
    const NormDecision d = ltx_rownorm_route(ltx_rownorm_route_args(a, dtype));
    if (d.route == NORM_REFUSED) LTX_FAIL(LTX_ERR_ARG, d.why);
    if (a.parts && (!a.x_out || a.part_stride < a.rows * a.D || ((uintptr_t)a.parts & 15) || (a.d_gate && (((uintptr_t)a.d_gate & 15) || a.d_gate_stride % 4))))
        LTX_FAIL(LTX_ERR_ARG, "rownorm: deferred rows need whole-row lanes (D of at most 64 x 8 chunks), 1..16 parts of [rows, D] f32 and an output for the finished rows");
    const int nch = a.D / ch, lpr = pick_lpr(nch);
    void* tok = nullptr;
    ltx_prof_begin(LTX_PROF_ROWNORM, 2.0 * (double)a.rows * a.D * (dtype == LTX_DT_BF16 ? 2 : 4), s, &tok);
    if (d.route == NORM_PRESUM || d.route == NORM_PRESUM_LEAN) launch_presum(a, d, dtype, nch, s);
    else if (dtype == LTX_DT_BF16) launch_rownorm_t<bf16_t>(a, d, lpr, nch, s);
    else launch_rownorm_t<float>(a, d, lpr, nch, s);
    ltx_prof_end(tok, s);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}
int ltx_launch_rowsq(const void* x, int dtype, int64_t rows, int N, int ld, float* out, hipStream_t s) {
    if (rows <= 0 || N <= 0) return LTX_OK;
    if (!x || !out || N % 4 != 0 || ld % 4 != 0 || ((uintptr_t)x & 7)) LTX_FAIL(LTX_ERR_ARG, "rowsq: N and ld must be multiples of 4 and x 8-byte aligned");
    const int64_t npairs = rows * ((N + 127) / 128);
    dim3 grid((unsigned)cdiv64(npairs, 256)), block(256);
    if (dtype == LTX_DT_BF16) hipLaunchKernelGGL(rowsq_kernel<bf16_t>, grid, block, 0, s, reinterpret_cast<const bf16_t*>(x), rows, N, ld, out);
    else hipLaunchKernelGGL(rowsq_kernel<float>, grid, block, 0, s, reinterpret_cast<const float*>(x), rows, N, ld, out);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}

// cvec[b][n] = sum_k shift[b][k] * W[n][k] + bias[n] (norm fold, kernels.h): one wave per output column, lanes over 16-byte
// chunks of the weight row, f32 throughout, a fixed order of additions (per lane ascending k, then the lanes' sums by halving).
// Reads W once: a step's 2 x num_layers launches stream the q|k|v and ff1 weights at the HBM rate - once per distinct timestep.
namespace {
__global__ __launch_bounds__(256) void shift_gemv_kernel(const bf16_t* __restrict__ W, const bf16_t* __restrict__ bias, const float* __restrict__ shift, int shift_stride,
                                                          int B, int N, int K, float* __restrict__ out, int out_stride) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x * 4 + wave;
    if (n >= N) return;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const bf16_t* wr = W + (int64_t)n * K;
    for (int c = lane; c < K / 8; c += 64) {
        const bf16x8 w = *reinterpret_cast<const bf16x8*>(wr + c * 8);
        float wf[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) wf[i] = (float)w[i];
        for (int b = 0; b < B; ++b) {
            const float* sp = shift + (int64_t)b * shift_stride + c * 8;
            const f32x4 s0 = *reinterpret_cast<const f32x4*>(sp), s1 = *reinterpret_cast<const f32x4*>(sp + 4);
            float a = acc[b];
#pragma unroll
            for (int i = 0; i < 4; ++i) a = __builtin_fmaf(wf[i], s0[i], a);
#pragma unroll
            for (int i = 0; i < 4; ++i) a = __builtin_fmaf(wf[4 + i], s1[i], a);
            acc[b] = a;
        }
    }
    const float bn = bias ? (float)bias[n] : 0.f;
    for (int b = 0; b < B; ++b) {
        float a = acc[b];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off);
        if (lane == 0) out[(int64_t)b * out_stride + n] = a + bn;
    }
}
}  // namespace

int ltx_launch_shift_gemv(const void* W, const void* bias, const float* shift, int shift_stride, int B, int N, int K, float* cvec, int cvec_stride, hipStream_t s) {
    if (!W || !shift || !cvec || B < 1 || B > 8 || N < 1 || K < 8 || K % 8 || shift_stride % 4 || ((uintptr_t)W & 15) || ((uintptr_t)shift & 15))
        LTX_FAIL(LTX_ERR_ARG, "shift_gemv: bf16 weights [N, K] with K % 8 == 0, f32 shift rows 16-byte aligned, 1..8 batch rows");
    hipLaunchKernelGGL(shift_gemv_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, reinterpret_cast<const bf16_t*>(W), reinterpret_cast<const bf16_t*>(bias),
                       shift, shift_stride, B, N, K, cvec, cvec_stride);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}
