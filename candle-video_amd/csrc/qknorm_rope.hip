// The q/k pass of self- and cross-attention, and the rotary tables it reads.
//
//  qknorm_rope  : q/k RMSNorm with weight over the FULL inner dim (ltx_transformer.rs:671-672)
//                 fused with apply_rotary_emb (:314-339), in place, for 1 or 2 segments of a fused
//                 QKV row.
//  rope_table   : LtxVideoRotaryPosEmbed::forward (:436-524) -> half-width cos/sin tables.
//
// Three kernels (ltx_qknorm_route picks; the lane mapping is rownorm.hip's WIDE one, norm_common.h) around one arithmetic: the row
// statistic is add_sq in ascending chunk order, 1 / rms is rinv_qk, and a chunk is finished by qk_finish (the general kernel, the
// only one that serves f32, by its own copy of that text: see there).
#include "common.h"
#include "kernels.h"
#include "norm_common.h"
#include "options.h"

namespace {

// The epilogue of chunk c of a segment x: * rinv * w [* wb], the rotation of its pairs (2p, 2p + 1) by (co[p], si[p]), rounded and
// stored.  w, wb: the segment's weight rows; wb (a consumer's weight folded in, QkNormRopeArgs::w0b) may be null; co, si: the
// chunk's CH / 2 table entries in registers.
template <typename T>
__device__ __forceinline__ void qk_finish(Chunk16 v, float rinv, int c, const T* w, const T* wb, bool rope, const Chunk16& co, const Chunk16& si, T* x, bool active) {
    constexpr int CH = ElemTraits<T>::CHUNK;
    float f[CH]; chunk_to_f32<T>(v, f);
    Chunk16 wc; wc.u = *reinterpret_cast<const u32x4*>(w + c * CH);
    float wv[CH]; chunk_to_f32<T>(wc, wv);
#pragma unroll
    for (int j = 0; j < CH; ++j) f[j] = f[j] * rinv * wv[j];
    if (wb) {
        Chunk16 wc2; wc2.u = *reinterpret_cast<const u32x4*>(wb + c * CH);
        float wv2[CH]; chunk_to_f32<T>(wc2, wv2);
#pragma unroll
        for (int j = 0; j < CH; ++j) f[j] *= wv2[j];
    }
    if (rope) {
#pragma unroll
        for (int p = 0; p < CH / 2; ++p) {
            const float re = f[2 * p], im = f[2 * p + 1];
            f[2 * p] = re * co.f[p] - im * si.f[p];          // x*cos + (-x_imag)*sin
            f[2 * p + 1] = im * co.f[p] + re * si.f[p];      // x*cos + ( x_real)*sin
        }
    }
    Chunk16 o; f32_to_chunk<T>(f, o);
    if (active) *reinterpret_cast<u32x4*>(x + c * CH) = o.u;
}

// CACHED: the (<= NSLOT chunks per lane) segment stays in registers between the two passes
template <typename T, bool CACHED>
__global__ __launch_bounds__(256) void qknorm_rope_kernel(const QkNormRopeArgs a, int lpr) {
    constexpr int CH = ElemTraits<T>::CHUNK;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rpw = 64 / lpr;
    const int64_t row = ((int64_t)blockIdx.x * 4 + wave) * rpw + lane / lpr;
    const int sub = lane % lpr;
    const bool active = row < a.rows;
    const int64_t rr = active ? row : a.rows - 1;
    const int nch = a.D / CH;
    const float* cs = a.cos ? a.cos + rr * (a.D / 2) : nullptr;
    const float* sn = a.sin ? a.sin + rr * (a.D / 2) : nullptr;
    // (this kernel keeps its own text of qk_finish: its f32 results carry the multiply-add contractions the compiler chose for
    // THIS text - f[2p+1] as fma(im, co, re * si) in one pair and fma(re, si, im * co) in the other - and through the shared
    // function it chooses others; the bf16 kernels round to the same bits either way)
    auto finish = [&](Chunk16 v, int c, float rinv, const T* w, const T* wb, T* x) {
        float f[CH]; chunk_to_f32<T>(v, f);
        Chunk16 wc; wc.u = *reinterpret_cast<const u32x4*>(w + c * CH);
        float wv[CH]; chunk_to_f32<T>(wc, wv);
#pragma unroll
        for (int i = 0; i < CH; ++i) f[i] = f[i] * rinv * wv[i];
        if (wb) {                                          // a consumer's weight folded in (QkNormRopeArgs::w0b)
            Chunk16 wc2; wc2.u = *reinterpret_cast<const u32x4*>(wb + c * CH);
            float wv2[CH]; chunk_to_f32<T>(wc2, wv2);
#pragma unroll
            for (int i = 0; i < CH; ++i) f[i] *= wv2[i];
        }
        if (cs) {
            float co[CH / 2], si[CH / 2];
            if constexpr (CH == 8) {
                f32x4 c4 = *reinterpret_cast<const f32x4*>(cs + c * 4), s4 = *reinterpret_cast<const f32x4*>(sn + c * 4);
#pragma unroll
                for (int p = 0; p < 4; ++p) { co[p] = c4[p]; si[p] = s4[p]; }
            } else {
#pragma unroll
                for (int p = 0; p < CH / 2; ++p) { co[p] = cs[c * (CH / 2) + p]; si[p] = sn[c * (CH / 2) + p]; }
            }
#pragma unroll
            for (int p = 0; p < CH / 2; ++p) {
                float re = f[2 * p], im = f[2 * p + 1];
                f[2 * p] = re * co[p] - im * si[p];          // x*cos + (-x_imag)*sin
                f[2 * p + 1] = im * co[p] + re * si[p];      // x*cos + ( x_real)*sin
            }
        }
        Chunk16 o; f32_to_chunk<T>(f, o);
        if (active) *reinterpret_cast<u32x4*>(x + c * CH) = o.u;
    };
    for (int seg = 0; seg < a.nseg; ++seg) {
        T* x = reinterpret_cast<T*>(a.x) + rr * a.ld + (int64_t)seg * (a.seg_stride ? a.seg_stride : a.D);
        const T* w = reinterpret_cast<const T*>(seg == 0 ? a.w0 : a.w1);
        const T* wb = seg == 0 ? reinterpret_cast<const T*>(a.w0b) : nullptr;
        const float oscale = seg == 0 ? a.out_scale0 : 1.0f;
        if constexpr (CACHED) {
            Chunk16 v[NSLOT];
#pragma unroll
            for (int i = 0; i < NSLOT; ++i) {
                int c = sub + i * lpr;
                v[i].u = (u32x4){0u, 0u, 0u, 0u};
                if (c < nch) v[i].u = *reinterpret_cast<const u32x4*>(x + c * CH);
            }
            const float rinv = rinv_qk(group_sum(cached_sq<T>(v), lpr), a.D, a.eps, oscale);
#pragma unroll
            for (int i = 0; i < NSLOT; ++i) { int c = sub + i * lpr; if (c < nch) finish(v[i], c, rinv, w, wb, x); }
        } else {
            float ss = 0.f;
            for (int c = sub; c < nch; c += lpr) { Chunk16 v; v.u = *reinterpret_cast<const u32x4*>(x + c * CH); ss = add_sq<T>(v, ss); }
            const float rinv = rinv_qk(group_sum(ss, lpr), a.D, a.eps, oscale);
            for (int c = sub; c < nch; c += lpr) { Chunk16 v; v.u = *reinterpret_cast<const u32x4*>(x + c * CH); finish(v, c, rinv, w, wb, x); }
        }
    }
}

// Fast path of the kernel above for rows of <= NS*lpr chunks (the DiT's 2048-wide q/k: 4 chunks per lane): the cos/sin
// chunks of a lane are loaded ONCE and reused by both segments (q and k share the table), and the loads of every
// segment are issued before the first reduction (memory-level parallelism; the slow kernel read the tables twice and
// serialised the segments).
template <typename T, int NS, int OCC = 5>      // OCC: blocks per CU the register allocation must allow (NS = 4: 94 registers, five)
__global__ __launch_bounds__(256, OCC) void qknorm_rope_fused_kernel(const QkNormRopeArgs a, int lpr) {
    constexpr int CH = ElemTraits<T>::CHUNK;
    static_assert(CH == 8, "bf16 rows only");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rpw = 64 / lpr;
    const int64_t row = ((int64_t)blockIdx.x * 4 + wave) * rpw + lane / lpr;
    const int sub = lane % lpr;
    const bool active = row < a.rows;
    const int64_t rr = active ? row : a.rows - 1;
    const int nch = a.D / CH;
    const bool rope = a.cos != nullptr;
    const float* cs = rope ? a.cos + rr * (a.D / 2) : nullptr;
    const float* sn = rope ? a.sin + rr * (a.D / 2) : nullptr;
    T* x0 = reinterpret_cast<T*>(a.x) + rr * a.ld;
    const int64_t sst = a.seg_stride ? a.seg_stride : a.D;
    Chunk16 v[2][NS];
    Chunk16 co[NS], si[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int c = sub + i * lpr;
        const bool in = c < nch;
        v[0][i].u = (u32x4){0u, 0u, 0u, 0u}; v[1][i].u = (u32x4){0u, 0u, 0u, 0u};
        if (in) v[0][i].u = *reinterpret_cast<const u32x4*>(x0 + c * CH);
        if (in && a.nseg == 2) v[1][i].u = *reinterpret_cast<const u32x4*>(x0 + sst + c * CH);
        if (in && rope) { co[i].u = *reinterpret_cast<const u32x4*>(cs + c * 4); si[i].u = *reinterpret_cast<const u32x4*>(sn + c * 4); }
    }
    // both row statistics first, then chunk-major: chunk i of q and of k are finished together with ONE copy of its cos / sin
    // in registers, which then die (seg-major order kept all four table chunks and both rows alive: 118 VGPRs = 4 waves per SIMD
    // = 4096 wave slots for the DiT's 4992 row-waves, i.e. a second, mostly empty round; chunk-major fits 5 per SIMD)
    float rinv[2] = {0.f, 0.f};
#pragma unroll
    for (int seg = 0; seg < 2; ++seg) {
        if (seg >= a.nseg) break;
        rinv[seg] = rinv_qk(group_sum(cached_sq<T>(v[seg]), lpr), a.D, a.eps, seg == 0 ? a.out_scale0 : 1.0f);
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int c = sub + i * lpr;
        if (c >= nch) continue;
#pragma unroll
        for (int seg = 0; seg < 2; ++seg) {
            if (seg >= a.nseg) break;
            const T* w = reinterpret_cast<const T*>(seg == 0 ? a.w0 : a.w1);
            const T* wb = seg == 0 ? reinterpret_cast<const T*>(a.w0b) : nullptr;
            // (opaque copy: without it the f32 expansion of all eight chunks made for the row statistics is kept alive - 64 registers)
            asm volatile("" : "+v"(v[seg][i].u));
            qk_finish<T>(v[seg][i], rinv[seg], c, w, wb, rope, co[i], si[i], x0 + seg * sst, active);
            __builtin_amdgcn_sched_barrier(0);             // one (chunk, segment) at a time: the scheduler's interleave of all eight costs 30 registers
        }
    }
}

// Few rows (C1's 384 tokens; the text rows of the cached cross-attention keys): one row per block, a chunk (two beyond 2048 columns)
// per thread and segment - the arithmetic of qknorm_rope_fused_kernel, the row statistics summed by block_sum (as in
// rownorm_block_kernel): 6.6 -> ~4 us per launch at 384 rows.
template <typename T>
__global__ __launch_bounds__(256) void qknorm_rope_block_kernel(const QkNormRopeArgs a) {
    constexpr int CH = ElemTraits<T>::CHUNK, NC = 2;
    static_assert(CH == 8, "bf16 rows only");
    __shared__ float red[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = blockIdx.x;
    const int nch = a.D / CH;
    const bool rope = a.cos != nullptr;
    const float* cs = rope ? a.cos + row * (a.D / 2) : nullptr;
    const float* sn = rope ? a.sin + row * (a.D / 2) : nullptr;
    T* x0 = reinterpret_cast<T*>(a.x) + row * a.ld;
    const int64_t sst = a.seg_stride ? a.seg_stride : a.D;
    Chunk16 v[2][NC];
    Chunk16 co[NC], si[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = tid + i * 256;
        const bool in = c < nch;
        v[0][i].u = (u32x4){0u, 0u, 0u, 0u}; v[1][i].u = (u32x4){0u, 0u, 0u, 0u};
        if (in) v[0][i].u = *reinterpret_cast<const u32x4*>(x0 + c * CH);
        if (in && a.nseg == 2) v[1][i].u = *reinterpret_cast<const u32x4*>(x0 + sst + c * CH);
        if (in && rope) { co[i].u = *reinterpret_cast<const u32x4*>(cs + c * 4); si[i].u = *reinterpret_cast<const u32x4*>(sn + c * 4); }
    }
    float ss[2] = {cached_sq<T>(v[0]), cached_sq<T>(v[1])};
    block_sum<2>(ss, red, lane, wave);
    const float rinv[2] = {rinv_qk(ss[0], a.D, a.eps, a.out_scale0), rinv_qk(ss[1], a.D, a.eps, 1.0f)};
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = tid + i * 256;
        if (c >= nch) continue;
#pragma unroll
        for (int seg = 0; seg < 2; ++seg) {
            if (seg >= a.nseg) break;
            const T* w = reinterpret_cast<const T*>(seg == 0 ? a.w0 : a.w1);
            const T* wb = seg == 0 ? reinterpret_cast<const T*>(a.w0b) : nullptr;
            qk_finish<T>(v[seg][i], rinv[seg], c, w, wb, rope, co[i], si[i], x0 + seg * sst, true);
        }
    }
}

__global__ void rope_table_kernel(const RopeTableArgs a) {
    const int half = a.D / 2;
    const int64_t S = (int64_t)a.F * a.H * a.W;
    const int64_t total = (int64_t)a.B * S * half;
    const int rem_pairs = (a.D % 6) / 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int p = (int)(i % half);
        const int64_t row = i / half;
        float co = 1.0f, si = 0.0f;
        if (p >= rem_pairs) {
            const int fi = p - rem_pairs;
            const int step = fi / 3, ax = fi - step * 3;
            float g;
            if (a.use_coords) {
                g = a.coords[row * 3 + ax] * a.gscale[ax];
            } else {
                const int64_t s = row % S;
                const int w = (int)(s % a.W); const int64_t t1 = s / a.W;
                const int h = (int)(t1 % a.H); const int f = (int)(t1 / a.H);
                const float idx = ax == 0 ? (float)f : (ax == 1 ? (float)h : (float)w);
                g = idx * a.gscale[ax];
            }
            const float ang = a.freqs[step] * (g * 2.0f - 1.0f);
            co = cosf(ang); si = sinf(ang);
        }
        a.cos[i] = co; a.sin[i] = si;
    }
}

}  // namespace

// The one place where the q/k pass's kernel is chosen (kernels.h).
QkNormRoute ltx_qknorm_route(int dtype, int64_t rows, int D, const char** why) {
    const int ch = dtype == LTX_DT_BF16 ? 8 : 4;
    if (D < ch || D % ch != 0) { if (why) *why = "qknorm: D/ld must be multiples of the 16-byte chunk"; return QKNORM_REFUSED; }
    const int nch = D / ch, lpr = pick_lpr(nch);
    const bool cached = nch <= NSLOT * lpr;
    if (dtype == LTX_DT_BF16) {
        if (rows <= 512 && nch > 64 && nch <= 512) return QKNORM_BLOCK;              // few wide rows: one row per block
        if (nch <= 4 * lpr) return QKNORM_FUSED4;
        // the 13B model's 4096-wide rows: eight chunks per lane, the table still read once for q and k (LTX_QKNORM_FUSED8=0: the two-pass kernel)
        if (nch <= 8 * lpr && ltx_exp("qknorm_fused8", 1)) return QKNORM_FUSED8;
    }
    return cached ? QKNORM_CACHED : QKNORM_REREAD;
}

const char* ltx_qknorm_route_name(QkNormRoute r) {
    static const char* const names[] = {"refused", "block", "fused4", "fused8", "cached", "reread"};
    return names[r];
}

int ltx_launch_qknorm_rope(const QkNormRopeArgs& a, int dtype, hipStream_t s) {
    const int ch = dtype == LTX_DT_BF16 ? 8 : 4;
    if (a.rows <= 0) return LTX_OK;
    if (a.D % ch != 0 || a.ld % ch != 0) LTX_FAIL(LTX_ERR_ARG, "qknorm: D/ld must be multiples of the 16-byte chunk");
    if (a.nseg < 1 || a.nseg > 2 || !a.w0 || (a.nseg == 2 && !a.w1)) LTX_FAIL(LTX_ERR_ARG, "qknorm: bad segments/weights");
    const char* why = nullptr;
    const QkNormRoute route = ltx_qknorm_route(dtype, a.rows, a.D, &why);
    if (route == QKNORM_REFUSED) LTX_FAIL(LTX_ERR_ARG, why);
    const int nch = a.D / ch, lpr = pick_lpr(nch);
    const int64_t rows_per_block = 4 * (64 / lpr);
    dim3 grid((unsigned)cdiv64(a.rows, rows_per_block)), block(256);
    const bool bf16 = dtype == LTX_DT_BF16;
    switch (route) {
    case QKNORM_BLOCK: hipLaunchKernelGGL((qknorm_rope_block_kernel<bf16_t>), dim3((unsigned)a.rows), block, 0, s, a); break;
    case QKNORM_FUSED4: hipLaunchKernelGGL((qknorm_rope_fused_kernel<bf16_t, 4>), grid, block, 0, s, a, lpr); break;
    case QKNORM_FUSED8: hipLaunchKernelGGL((qknorm_rope_fused_kernel<bf16_t, 8, 2>), grid, block, 0, s, a, lpr); break;
    case QKNORM_CACHED:
        if (bf16) hipLaunchKernelGGL((qknorm_rope_kernel<bf16_t, true>), grid, block, 0, s, a, lpr);
        else hipLaunchKernelGGL((qknorm_rope_kernel<float, true>), grid, block, 0, s, a, lpr);
        break;
    default:
        if (bf16) hipLaunchKernelGGL((qknorm_rope_kernel<bf16_t, false>), grid, block, 0, s, a, lpr);
        else hipLaunchKernelGGL((qknorm_rope_kernel<float, false>), grid, block, 0, s, a, lpr);
        break;
    }
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}

int ltx_launch_rope_table(const RopeTableArgs& a, hipStream_t s) {
    if (a.D % 2 != 0 || a.D < 6) LTX_FAIL(LTX_ERR_ARG, "rope: dim must be even and >= 6");
    const int64_t total = (int64_t)a.B * a.F * a.H * a.W * (a.D / 2);
    int64_t blocks = cdiv64(total, 256); if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(rope_table_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    LTX_CHECK_LAUNCH();
    return LTX_OK;
}
