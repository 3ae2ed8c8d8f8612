// Host sanitizer driver of the keyframe layout (candle-video_amd/host/cond_plan.h, header only, built with ASan + UBSan).
// argv: num_frames h w ts_ratio sp_ratio frame_rate  then per item: cond_frames frame_index strength
// stdout: one JSON line - E, G, the groups table [item, frame, strength bits], the coordinates as f32 bit patterns, and the
// update predicate / model timestep of every group on the probe steps (sigma, t) = (1, 1000), (0.8, 800), (0.5, 500).
// A refusal: the message on stderr, exit code 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../candle-video_amd/host/cond_plan.h"

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(int argc, char** argv) {
    if (argc < 7 || (argc - 7) % 3 != 0) { fprintf(stderr, "usage: num_frames h w ts_ratio sp_ratio frame_rate [cond_frames frame_index strength]...\n"); return 2; }
    const int num_frames = atoi(argv[1]), h = atoi(argv[2]), w = atoi(argv[3]), ts = atoi(argv[4]), sp = atoi(argv[5]), fr = atoi(argv[6]);
    std::vector<CondItemGeom> items;
    for (int a = 7; a < argc; a += 3) items.push_back({atoi(argv[a]), atoi(argv[a + 1]), strtof(argv[a + 2], nullptr)});
    CondPlan p;
    std::string err;
    if (!cond_plan_build(items.empty() ? nullptr : items.data(), (int)items.size(), num_frames, h, w, ts, sp, fr, &p, &err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return 1;
    }
    printf("{\"E\": %d, \"G\": %d, \"Fl\": %d, \"hw\": %d, \"groups\": [", p.E, p.G, p.Fl, p.hw);
    for (int g = 0; g < p.G; ++g) printf("%s[%d, %d, %u]", g ? ", " : "", p.groups[g].item, p.groups[g].frame, bits(p.groups[g].strength));
    printf("], \"coords\": [");
    for (size_t i = 0; i < p.coords.size(); ++i) printf("%s%u", i ? ", " : "", bits(p.coords[i]));
    printf("], \"steps\": [");
    const float probe[3][2] = {{1.0f, 1000.0f}, {0.8f, 800.0f}, {0.5f, 500.0f}};
    for (int i = 0; i < 3; ++i) {
        printf("%s[", i ? ", " : "");
        for (int g = 0; g < p.G; ++g)
            printf("%s[%d, %u]", g ? ", " : "", cond_group_updates(probe[i][0], p.groups[g].strength) ? 1 : 0, bits(cond_group_timestep(probe[i][1], p.groups[g].strength)));
        printf("]");
    }
    printf("]}\n");
    return 0;
}
