// The VAE's tiling scheme (vae.rs:2158-2434) as data: a pure function of the compression ratios, the tiling fields and the
// shape.  csrc/vae.hip walks a plan (assemble_spatial, place_temporal, batched_leaf_decode); nothing here touches the device,
// so the geometry is tested on the CPU (tests/test_tile_plan_cpu.py).
#pragma once
#include <vector>
#include "../../include/ltxhip_encoder.h"

struct TileSpan { int i0, i1; };
// [(i, min(i + tile + extra, N)) for i in range(0, N, stride)]; extra = 1 on the temporal axis (the "+ 1" of vae.rs:2382 / :2309)
std::vector<TileSpan> tile_spans(int N, int tile, int stride, int extra);

struct VaeTilePlan {
    enum Mode { kDirect, kSpatial, kTemporal };
    enum Drop { kLastOfLaterTiles, kFirstOfTile0 };
    Mode mode = kDirect;                       // decode_z / encode_z dispatch (vae.rs:2037-2066, :2017-2035)
    bool window_tiled = false;                 // the (temporal) windows are spatially tiled
    std::vector<TileSpan> windows, rows, cols; // input units: latents on the decode side, samples on the encode side; one full span where not tiled
    // what the blends and the copy windows consume, in OUTPUT units (decode: samples, encode: latents)
    int blend_t = 0, blend_h = 0, blend_w = 0, keep_t = 0, keep_h = 0, keep_w = 0;
    int oT = 0, oH = 0, oW = 0;                // output dims (a direct encode: 0, the encoder's block structure decides)
    // decode: tiles li > 0 lose their LAST frame when longer than 1 (vae.rs:2400-2404); encode: tile 0 loses its FIRST (:2322-2327)
    Drop drop = kLastOfLaterTiles;
    // temporal window li, `phys` output frames as produced: frames to skip at its start, its logical length, frames it gives the result
    struct Frames { int skip, len, keep; };
    Frames frames(int li, int phys) const;
};

// r, tr: spatial / temporal compression ratio.  Both return LTX_OK or refuse (LTX_ERR_ARG + ltx_last_error) before any work.
int vae_decode_tile_plan(int r, int tr, const ltx_tiling* tl, int F, int H, int W, VaeTilePlan* plan);      // latent F, H, W
int vae_encode_tile_plan(int r, int tr, const ltx_tiling* tl, const ltx_encode_tiling* et, int F, int H, int W, VaeTilePlan* plan);   // sample F, H, W
