// Block maps of the sparse self-attention (include/ltxhip_sparse_attn.h, "the block map" and "the window map") as host data: sizes,
// the window builder, the density and the empty-row check of a map for Sq = Sk = S.  Nothing here touches the device or includes
// HIP; csrc/capi_ops.hip exports the three functions and csrc/dit.hip checks a map with them before it is uploaded.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>

inline int64_t sparse_map_nqb(int64_t S) { return (S + 127) / 128; }
inline int64_t sparse_map_nkt(int64_t S) { return (S + 63) / 64; }
inline int64_t sparse_map_nw(int64_t S) { return (sparse_map_nkt(S) + 31) / 32; }
inline size_t sparse_map_words(int64_t S) { return S < 1 ? 0 : (size_t)(sparse_map_nqb(S) * sparse_map_nw(S)); }

// set bits of row `row` below NKT
inline int64_t sparse_map_row_count(const uint32_t* map, int64_t row, int64_t S) {
    const int64_t nkt = sparse_map_nkt(S), nw = sparse_map_nw(S);
    int64_t n = 0;
    for (int64_t w = 0; w < nw; ++w) {
        uint32_t x = map[row * nw + w];
        if (w == nw - 1 && (nkt & 31)) x &= (1u << (nkt & 31)) - 1u;
        n += __builtin_popcount(x);
    }
    return n;
}
// the first row of `rows` with no tile listed, -1 where every row has one
inline int64_t sparse_map_empty_row(const uint32_t* map, int64_t rows, int64_t S) {
    for (int64_t r = 0; r < rows; ++r) if (sparse_map_row_count(map, r, S) == 0) return r;
    return -1;
}
inline double sparse_map_density(const uint32_t* map, int64_t S) {
    if (!map || S < 1) return -1.0;
    int64_t n = 0;
    for (int64_t r = 0; r < sparse_map_nqb(S); ++r) n += sparse_map_row_count(map, r, S);
    return (double)n / ((double)sparse_map_nqb(S) * (double)sparse_map_nkt(S));
}

// The window map.  For a query token (f, h, w) the keys inside its window are, per (f', h') of the clipped box, ONE run of consecutive
// tokens (the clipped columns), i.e. a run of key tiles: S * (2 wf + 1) * (2 wh + 1) runs in all.  false + *err: the refusal.
inline bool sparse_window_map_build(int F, int H, int W, int wf, int wh, int ww, int sink_frames, uint32_t* map, size_t words, std::string* err) {
    auto fail = [&](const std::string& m) { if (err) *err = m; return false; };
    if (F < 1 || H < 1 || W < 1) return fail("sparse window map: F, H and W must be >= 1 (got " + std::to_string(F) + ", " + std::to_string(H) + ", " + std::to_string(W) + ")");
    if (wf < 0 || wh < 0 || ww < 0 || sink_frames < 0)
        return fail("sparse window map: the window (" + std::to_string(wf) + ", " + std::to_string(wh) + ", " + std::to_string(ww) + ") and sink_frames (" + std::to_string(sink_frames) + ") must be >= 0");
    const int64_t S = (int64_t)F * H * W;
    if (!map) return fail("sparse window map: null map");
    if (words != sparse_map_words(S)) return fail("sparse window map: " + std::to_string(words) + " words for a map of " + std::to_string(sparse_map_words(S)) + " (S " + std::to_string(S) + ")");
    const int64_t nw = sparse_map_nw(S);
    std::fill(map, map + words, 0u);
    auto set_run = [&](int64_t qb, int64_t t0, int64_t t1) {      // key tokens [t0, t1] -> their tiles
        for (int64_t kt = t0 / 64; kt <= t1 / 64; ++kt) map[qb * nw + (kt >> 5)] |= 1u << (kt & 31);
    };
    const int64_t sink_tokens = (int64_t)std::min(sink_frames, F) * H * W;
    for (int64_t qb = 0; qb < sparse_map_nqb(S); ++qb) {
        if (sink_tokens > 0) set_run(qb, 0, sink_tokens - 1);
        for (int64_t t = qb * 128; t < std::min<int64_t>(qb * 128 + 128, S); ++t) {
            const int w = (int)(t % W), h = (int)((t / W) % H), f = (int)(t / ((int64_t)W * H));
            const int w0 = std::max(0, w - std::min(ww, W)), w1 = std::min(W - 1, w + std::min(ww, W));
            for (int ff = std::max(0, f - std::min(wf, F)); ff <= std::min(F - 1, f + std::min(wf, F)); ++ff)
                for (int hh = std::max(0, h - std::min(wh, H)); hh <= std::min(H - 1, h + std::min(wh, H)); ++hh) {
                    const int64_t row0 = ((int64_t)ff * H + hh) * W;
                    set_run(qb, row0 + w0, row0 + w1);
                }
        }
    }
    return true;
}
