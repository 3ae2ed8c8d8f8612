// Host sanitizer driver of the VAE tile plan (candle-video_amd/host/tile_plan.cpp built with ASan + UBSan, LTX_HOST_ONLY).
// stdin, one case per line:   dec|enc r tr use_tiling use_framewise min_h min_w min_f stride_h stride_w stride_f F H W
// stdout, one JSON line per case: the whole plan, or the return code and ltx_last_error().  `frames` lists, per temporal window,
// VaeTilePlan::frames at the window's nominal output length (decode (n - 1) * tr + 1, encode (n - 1) / tr + 1).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../candle-video_amd/host/tile_plan.h"

static void spans(const char* name, const std::vector<TileSpan>& v) {
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s[%d, %d]", i ? ", " : "", v[i].i0, v[i].i1);
    printf("], ");
}

int main() {
    char line[512];
    int n_cases = 0;
    while (fgets(line, sizeof line, stdin)) {
        char side[8] = {0};
        int r, tr, F, H, W;
        ltx_tiling tl;
        ltx_encode_tiling et;
        const int got = sscanf(line, "%7s %d %d %d %d %d %d %d %d %d %d %d %d %d", side, &r, &tr, &tl.use_tiling, &tl.use_framewise_decoding,
                               &tl.tile_sample_min_height, &tl.tile_sample_min_width, &tl.tile_sample_min_num_frames,
                               &tl.tile_sample_stride_height, &tl.tile_sample_stride_width, &tl.tile_sample_stride_num_frames, &F, &H, &W);
        if (got <= 0) continue;
        const bool enc = !strcmp(side, "enc");
        if (got != 14 || (!enc && strcmp(side, "dec"))) { fprintf(stderr, "bad case line: %s", line); return 2; }
        VaeTilePlan p;
        int rc;
        if (enc) { et.use_framewise_encoding = tl.use_framewise_decoding; tl.use_framewise_decoding = 0; rc = vae_encode_tile_plan(r, tr, &tl, &et, F, H, W, &p); }
        else rc = vae_decode_tile_plan(r, tr, &tl, F, H, W, &p);
        ++n_cases;
        if (rc != 0) {
            std::string msg;
            for (const char* c = ltx_last_error(); *c; ++c) { if (*c == '"' || *c == '\\') msg += '\\'; msg += *c; }
            printf("{\"ok\": 0, \"rc\": %d, \"error\": \"%s\"}\n", rc, msg.c_str());
            continue;
        }
        static const char* modes[] = {"direct", "spatial", "temporal"};
        printf("{\"ok\": 1, \"mode\": \"%s\", \"window_tiled\": %s, ", modes[p.mode], p.window_tiled ? "true" : "false");
        spans("windows", p.windows); spans("rows", p.rows); spans("cols", p.cols);
        printf("\"blend\": [%d, %d, %d], \"keep\": [%d, %d, %d], \"out\": [%d, %d, %d], ", p.blend_t, p.blend_h, p.blend_w, p.keep_t, p.keep_h, p.keep_w, p.oT, p.oH, p.oW);
        printf("\"drop\": \"%s\", \"frames\": [", p.drop == VaeTilePlan::kFirstOfTile0 ? "first_of_tile0" : "last_of_later_tiles");
        for (size_t li = 0; li < p.windows.size(); ++li) {
            const int n = p.windows[li].i1 - p.windows[li].i0;
            const VaeTilePlan::Frames f = p.frames((int)li, enc ? (n - 1) / tr + 1 : (n - 1) * tr + 1);
            printf("%s[%d, %d, %d]", li ? ", " : "", f.skip, f.len, f.keep);
        }
        printf("]}\n");
    }
    printf("tile plan host sanitizer driver: clean (%d cases)\n", n_cases);
    return 0;
}
