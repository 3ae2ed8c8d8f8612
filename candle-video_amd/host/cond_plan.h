// The layout of a keyframe-conditioned sequence (include/ltxhip_keyframes.h, "the rule") as data: a pure function of the items'
// geometry, the video's geometry, the compression ratios and the frame rate.  host/pipeline.hip walks a plan (coordinates, the
// place table, the per-step holds); nothing here touches the device or includes HIP, so the layout and every refusal are tested on
// the CPU by a stand-alone program (tests/host/cond_plan_main.cpp, tests/test_cond_plan_cpu.py).
#pragma once
#include <cmath>
#include <string>
#include <vector>

struct CondItemGeom { int cond_frames, frame_index; float strength; };      // ltx_cond_item without its tokens
struct CondGroup { int item = -1, frame = 0; float strength = 0.0f; };      // item -1: no item wrote the group (strength 0)
struct CondPlan {
    int E = 0, G = 0, Fl = 0, hw = 0;       // extra groups, all groups (E + F'), grid frames F', tokens of a group (h * w)
    std::vector<CondGroup> groups;          // [G]: the E extra groups in item order, then the grid frames in pack order
    std::vector<float> coords;              // [G * hw, 3] of one batch row: (seconds, pixel row, pixel column)
};

// group g is updated on a step of sigma `sig` iff (double)sig - 1e-6 < 1 - (double)strength; otherwise it keeps its bits
inline bool cond_group_updates(float sig, float strength) { return (double)sig - 1e-6 < 1.0 - (double)strength; }
// what the model sees for a group on a step of scheduler timestep t (f32 arithmetic)
inline float cond_group_timestep(float t, float strength) { return std::fmin(t, 1000.0f * (1.0f - strength)); }
// a hard hold, the groups that image_cond_noise_scale perturbs
inline bool cond_group_is_hard(float strength) { return (double)strength >= 1.0 - 1e-6; }

// false + *err: the refusal, naming the item and the value.  num_frames: pixel frames of the video; h, w: the latent plane.
inline bool cond_plan_build(const CondItemGeom* items, int n_items, int num_frames, int h, int w, int ts_ratio, int sp_ratio, int frame_rate,
                            CondPlan* plan, std::string* err) {
    auto fail = [&](const std::string& m) { if (err) *err = m; return false; };
    if (!plan) return fail("conditioning layout: null output");
    if (n_items < 0) return fail("conditioning layout: n_items is negative (" + std::to_string(n_items) + ")");
    if (n_items > 0 && !items) return fail("conditioning layout: items is null with n_items " + std::to_string(n_items));
    if (num_frames < 1 || h < 1 || w < 1 || ts_ratio < 1 || sp_ratio < 1 || frame_rate < 1)
        return fail("conditioning layout: num_frames, height, width, the compression ratios and frame_rate must be >= 1");
    const int Fl = (num_frames - 1) / ts_ratio + 1, hw = h * w;
    struct Extra { int item, frame; };
    std::vector<Extra> extra;
    std::vector<CondGroup> grid((size_t)Fl);
    for (int i = 0; i < n_items; ++i) {
        const CondItemGeom& it = items[i];
        const std::string at = "conditioning item " + std::to_string(i) + ": ";
        if (!(it.strength >= 0.0f && it.strength <= 1.0f)) return fail(at + "strength " + std::to_string(it.strength) + " lies outside [0, 1]");
        if (it.cond_frames < 1) return fail(at + "cond_frames " + std::to_string(it.cond_frames) + " must be >= 1");
        if (it.frame_index < 0) return fail(at + "frame_index " + std::to_string(it.frame_index) + " is negative");
        const int n = it.frame_index, Fc = it.cond_frames;
        int first_grid_k = 0, grid0 = 0;          // latent frames k >= first_grid_k go to grid frame grid0 + k
        if (n > 0) {
            if (n % ts_ratio != 0) return fail(at + "frame_index " + std::to_string(n) + " is not a multiple of " + std::to_string(ts_ratio));
            if (n >= num_frames) return fail(at + "frame_index " + std::to_string(n) + " lies beyond the video's " + std::to_string(num_frames) + " frames");
            grid0 = n / ts_ratio;
            if (Fc >= 2 && grid0 + Fc - 1 > Fl - 1)
                return fail(at + "a clip of " + std::to_string(Fc) + " latent frames at frame_index " + std::to_string(n) + " ends at latent frame " +
                            std::to_string(grid0 + Fc - 1) + ", beyond the last one (" + std::to_string(Fl - 1) + ")");
            first_grid_k = Fc < 2 ? Fc : 2;
            for (int k = 0; k < first_grid_k; ++k) extra.push_back({i, k});
        } else if (Fc > Fl) {
            return fail(at + "cond_frames " + std::to_string(Fc) + " exceeds the video's " + std::to_string(Fl) + " latent frames");
        }
        for (int k = first_grid_k; k < Fc; ++k) { CondGroup& g = grid[(size_t)(grid0 + k)]; g.item = i; g.frame = k; g.strength = it.strength; }
    }
    plan->E = (int)extra.size(); plan->G = plan->E + Fl; plan->Fl = Fl; plan->hw = hw;
    plan->groups.clear();
    for (const Extra& e : extra) { CondGroup g; g.item = e.item; g.frame = e.frame; g.strength = items[e.item].strength; plan->groups.push_back(g); }
    plan->groups.insert(plan->groups.end(), grid.begin(), grid.end());
    // coordinates: the grid's as ltx_build_video_coords writes them; an extra group made from latent frame k of an item at n lies
    // at (max(ts_ratio * k - (ts_ratio - 1), 0) + n) / frame_rate seconds, on the spatial coordinates of a grid frame
    const float inv_fr = (float)(1.0 / (double)frame_rate);
    plan->coords.assign((size_t)plan->G * hw * 3, 0.0f);
    size_t o = 0;
    for (int g = 0; g < plan->G; ++g) {
        float sec;
        if (g < plan->E) {
            const float vf = (float)plan->groups[(size_t)g].frame * (float)ts_ratio + (1.0f - (float)ts_ratio);
            sec = (std::fmax(vf, 0.0f) + (float)items[plan->groups[(size_t)g].item].frame_index) * inv_fr;
        } else {
            const float vf = (float)(g - plan->E) * (float)ts_ratio + (1.0f - (float)ts_ratio);
            sec = std::fmin(std::fmax(vf, 0.0f), 1000.0f) * inv_fr;
        }
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) { plan->coords[o++] = sec; plan->coords[o++] = (float)y * (float)sp_ratio; plan->coords[o++] = (float)x * (float)sp_ratio; }
    }
    return true;
}
