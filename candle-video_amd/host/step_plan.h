// The guidance branches of every denoise step as data: a pure function of the number of steps and batch rows, each step's
// (guidance_scale, stg_scale, rescale) and perturbed-block list, and the guidance_batch option.  host/pipeline.hip walks a plan (one
// forward dispatch, one skip mask, one mix per step); nothing here touches the device or includes HIP, so every decision is tested on
// the CPU by a stand-alone program (tests/host/step_plan_main.cpp, tests/test_step_plan_cpu.py).
// The branches lie in three fixed slots of B rows each, in the reference's call order: slot 0 negative prompt (iff g > 1), slot 1 prompt
// (always), slot 2 prompt with the step's blocks perturbed (iff s > 0): a step's branches are the contiguous run [slot0, slot0 + nbr).
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

struct StepGuide { float g = 1.0f, s = 0.0f, r = 0.0f; const int* skip = nullptr; int n_skip = 0; };     // what one step is asked to do
struct StepEntry {
    StepGuide guide;                // (skip / n_skip: the blocks slot 2 perturbs; n_skip 0 unless stg)
    bool cfg = false, stg = false;
    int nbr = 1;                    // forwards' worth of branches
    bool batched = false;           // the branches as ONE forward of `rows` rows: more than one, at most 8 rows, the option on
    int slot0 = 1, rows = 0;        // the step's slots [slot0, slot0 + nbr), rows = nbr * B
};
enum StepMix { STEP_MIX_CLASSIC = 0, STEP_MIX_EX = 1 };     // ltx_launch_guidance_step (+ its stats workspace) / ltx_launch_guidance_step_ex
struct StepPlan {
    std::vector<StepEntry> steps;   // [N]
    bool any_cfg = false, any_stg = false, any_batched = false;
    StepMix mix = STEP_MIX_CLASSIC;
    int cfg_star = 0, rescale_form = 0;     // of the _ex mix (rescale_form: ltx_rescale_form, 0 = LTX_RESCALE_CFG)
    // the model handle's permanent skip list in front of the loop: set_skip false leaves it as it is
    bool set_skip = false; const int* perm_skip = nullptr; int n_perm_skip = 0;
};

inline void step_plan_fill(const StepGuide* guides, int N, int B, bool guidance_batch, StepPlan* plan) {
    plan->steps.assign((size_t)(N > 0 ? N : 0), StepEntry());
    plan->any_cfg = plan->any_stg = plan->any_batched = false;
    for (int i = 0; i < N; ++i) {
        StepEntry& e = plan->steps[(size_t)i];
        e.guide = guides[i];
        e.cfg = e.guide.g > 1.0f; e.stg = e.guide.s > 0.0f;
        if (!e.stg) { e.guide.skip = nullptr; e.guide.n_skip = 0; }
        e.nbr = 1 + (e.cfg ? 1 : 0) + (e.stg ? 1 : 0);
        e.slot0 = e.cfg ? 0 : 1; e.rows = e.nbr * B;
        e.batched = guidance_batch && e.nbr > 1 && e.rows <= 8;
        plan->any_cfg = plan->any_cfg || e.cfg; plan->any_stg = plan->any_stg || e.stg; plan->any_batched = plan->any_batched || e.batched;
    }
}

// The unscheduled call: one guide on every step, the classic mix.  A list given (non-null, of any length) is the handle's permanent
// list iff STG is off and clears it otherwise; no list leaves the handle alone.
inline void step_plan_constant(int N, int B, const StepGuide& guide, bool guidance_batch, StepPlan* plan) {
    const std::vector<StepGuide> all((size_t)(N > 0 ? N : 0), guide);
    step_plan_fill(all.data(), N, B, guidance_batch, plan);
    plan->mix = STEP_MIX_CLASSIC; plan->cfg_star = plan->rescale_form = 0;
    const bool stg = guide.s > 0.0f;
    plan->set_skip = guide.skip != nullptr; plan->perm_skip = stg ? nullptr : guide.skip; plan->n_perm_skip = stg ? 0 : guide.n_skip;
}

// A schedule resolved to one guide per step.  The same values on every step, no CFG-star, the reference's rescale form: the constant
// plan on those values, with the classic mix and its bits.  (A constant s == 0 perturbs nothing and skips nothing: its list is not
// handed on, and the handle's own list is cleared by an empty one.)  Otherwise the _ex mix, and no block is skipped for good.
inline void step_plan_scheduled(const StepGuide* guides, int N, int B, int cfg_star, int rescale_form, bool guidance_batch, StepPlan* plan) {
    bool constant = N >= 1 && !cfg_star && rescale_form == 0;
    for (int i = 1; i < N && constant; ++i) {
        const StepGuide &a = guides[0], &b = guides[i];
        constant = b.g == a.g && b.s == a.s && b.r == a.r;
        if (constant && a.s > 0.0f) constant = b.n_skip == a.n_skip && (a.n_skip == 0 || !std::memcmp(b.skip, a.skip, sizeof(int) * (size_t)a.n_skip));
    }
    if (constant) {
        static const int none = 0;
        StepGuide g = guides[0];
        if (!(g.s > 0.0f && g.n_skip > 0)) { g.skip = &none; g.n_skip = 0; }
        step_plan_constant(N, B, g, guidance_batch, plan);
        return;
    }
    step_plan_fill(guides, N, B, guidance_batch, plan);
    plan->mix = STEP_MIX_EX; plan->cfg_star = cfg_star; plan->rescale_form = rescale_form;
    plan->set_skip = true; plan->perm_skip = nullptr; plan->n_perm_skip = 0;
}

// out [L, rows] = 0, then 1 on the listed blocks for rows [row0, row0 + B); an index outside [0, L) is dropped
inline void step_skip_rows(int L, int rows, int row0, int B, const int* list, int n, std::vector<float>* out) {
    out->assign((size_t)L * (size_t)rows, 0.0f);
    for (int k = 0; k < n; ++k)
        for (int b = 0; b < B && list[k] >= 0 && list[k] < L; ++b) (*out)[(size_t)list[k] * (size_t)rows + (size_t)(row0 + b)] = 1.0f;
}
