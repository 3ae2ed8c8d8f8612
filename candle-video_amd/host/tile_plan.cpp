// Tile plans of the VAE's tiled decode and encode (host/tile_plan.h).  The integer arithmetic is the reference's, including
// where each side divides by the compression ratio: decode tiles count in latents and blends in samples, encode tiles count
// in samples and blends in latents.
#include <algorithm>
#include "tile_plan.h"
#include "../csrc/errors.h"

std::vector<TileSpan> tile_spans(int N, int tile, int stride, int extra) {
    std::vector<TileSpan> v;
    if (stride < 1) return v;
    for (int i = 0; i < N; i += stride) v.push_back({i, std::min(i + tile + extra, N)});
    return v;
}

VaeTilePlan::Frames VaeTilePlan::frames(int li, int phys) const {
    Frames f{0, phys, 0};
    if (drop == kFirstOfTile0) { f.skip = li == 0 ? 1 : 0; f.len = phys - f.skip; }
    else if (li > 0 && phys > 1) f.len = phys - 1;
    // result_row: the first tile keeps stride + 1 frames, later tiles `stride` (vae.rs:2410-2434, :2338-2347)
    f.keep = std::min(li > 0 ? keep_t : keep_t + 1, f.len);
    return f;
}

int vae_decode_tile_plan(int r, int tr, const ltx_tiling* tl, int F, int H, int W, VaeTilePlan* p) {
    *p = VaeTilePlan();
    p->oT = (F - 1) * tr + 1; p->oH = H * r; p->oW = W * r;
    p->windows = {{0, F}}; p->rows = {{0, H}}; p->cols = {{0, W}};
    if (!tl || (!tl->use_framewise_decoding && !tl->use_tiling)) return LTX_OK;
    if (r < 1 || tr < 1) LTX_FAIL(LTX_ERR_ARG, "tiling: compression ratios must be >= 1");
    const bool framewise = tl->use_framewise_decoding && F > tl->tile_sample_min_num_frames / tr;
    p->window_tiled = tl->use_tiling && (W > tl->tile_sample_min_width / r || H > tl->tile_sample_min_height / r);
    p->mode = framewise ? VaeTilePlan::kTemporal : p->window_tiled ? VaeTilePlan::kSpatial : VaeTilePlan::kDirect;
    if (framewise) {                     // temporal_tiled_decode (vae.rs:2358-2434)
        const int stride_t = tl->tile_sample_stride_num_frames / tr;
        if (stride_t < 1) LTX_FAIL(LTX_ERR_ARG, "tiling: temporal stride must be >= one latent frame");
        p->windows = tile_spans(F, tl->tile_sample_min_num_frames / tr, stride_t, 1);
        p->blend_t = std::max(tl->tile_sample_min_num_frames - tl->tile_sample_stride_num_frames, 0);
        p->keep_t = tl->tile_sample_stride_num_frames;
    }
    if (p->window_tiled) {               // tiled_decode (vae.rs:2225-2290)
        const int stride_h = tl->tile_sample_stride_height / r, stride_w = tl->tile_sample_stride_width / r;
        if (stride_h < 1 || stride_w < 1) LTX_FAIL(LTX_ERR_ARG, "tiling: stride must be >= one latent");
        p->rows = tile_spans(H, tl->tile_sample_min_height / r, stride_h, 0);
        p->cols = tile_spans(W, tl->tile_sample_min_width / r, stride_w, 0);
        p->blend_h = std::max(tl->tile_sample_min_height - tl->tile_sample_stride_height, 0);
        p->blend_w = std::max(tl->tile_sample_min_width - tl->tile_sample_stride_width, 0);
        p->keep_h = tl->tile_sample_stride_height; p->keep_w = tl->tile_sample_stride_width;
    }
    return LTX_OK;
}

int vae_encode_tile_plan(int r, int tr, const ltx_tiling* tl, const ltx_encode_tiling* et, int F, int H, int W, VaeTilePlan* p) {
    *p = VaeTilePlan();
    p->drop = VaeTilePlan::kFirstOfTile0;
    p->windows = {{0, F}}; p->rows = {{0, H}}; p->cols = {{0, W}};
    const bool framewise = tl && et && et->use_framewise_encoding && F > tl->tile_sample_min_num_frames;      // undivided (vae.rs:2021)
    p->window_tiled = tl && tl->use_tiling && (H > tl->tile_sample_min_height || W > tl->tile_sample_min_width);
    p->mode = framewise ? VaeTilePlan::kTemporal : p->window_tiled ? VaeTilePlan::kSpatial : VaeTilePlan::kDirect;
    if (p->mode == VaeTilePlan::kDirect) return LTX_OK;
    if (r < 1 || tr < 1 || H % r != 0 || W % r != 0) LTX_FAIL(LTX_ERR_ARG, "input not divisible by patch sizes (tiled encode: height and width must be multiples of the compression ratio)");
    p->oH = H / r; p->oW = W / r; p->oT = (F - 1) / tr + 1;                                                    // vae.rs:2162-2163, 2298
    if (framewise) {                     // temporal_tiled_encode (vae.rs:2294-2357)
        if (tl->tile_sample_stride_num_frames < tr) LTX_FAIL(LTX_ERR_ARG, "tiling: temporal stride must be >= one latent frame");
        p->windows = tile_spans(F, tl->tile_sample_min_num_frames, tl->tile_sample_stride_num_frames, 1);
        p->keep_t = tl->tile_sample_stride_num_frames / tr;
        p->blend_t = std::max(tl->tile_sample_min_num_frames / tr - p->keep_t, 0);
    }
    if (p->window_tiled) {               // tiled_encode (vae.rs:2158-2223)
        if (tl->tile_sample_stride_height < r || tl->tile_sample_stride_width < r) LTX_FAIL(LTX_ERR_ARG, "tiling: stride must be >= one latent");
        p->rows = tile_spans(H, tl->tile_sample_min_height, tl->tile_sample_stride_height, 0);
        p->cols = tile_spans(W, tl->tile_sample_min_width, tl->tile_sample_stride_width, 0);
        p->keep_h = tl->tile_sample_stride_height / r; p->keep_w = tl->tile_sample_stride_width / r;
        p->blend_h = std::max(tl->tile_sample_min_height / r - p->keep_h, 0);
        p->blend_w = std::max(tl->tile_sample_min_width / r - p->keep_w, 0);
    }
    return LTX_OK;
}
