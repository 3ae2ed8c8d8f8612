// The step cache's policy as data (include/ltxhip_stepcache.h): whether denoise step i of N runs the transformer blocks or re-uses the
// cached block residual, from the raw distance num / den of block 0's modulated input to the one of the step before.  A pure function
// of its arguments and of two words of state; nothing here touches the device or includes HIP, so every decision is tested on the CPU
// by a stand-alone program (tests/host/step_cache_main.cpp, tests/test_step_cache_policy_cpu.py) against tests/step_cache_ref.py.
#pragma once
#include <cmath>

struct StepCacheState {
    double acc = 0.0;               // the rescaled distances added up since the last computed step
    bool have_prev = false;         // a measurement exists: the next one has something to be a distance from
};
struct StepCachePolicy {            // the fields of ltx_step_cache_params
    float thresh = 0.0f;
    float coeff[5] = {0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
    const unsigned char* pattern = nullptr; int n_pattern = 0;      // per step: 0 decide, 1 compute, 2 reuse (steps past the end: 0)
};

// what is wrong with a caller's parameters (null: nothing)
inline const char* step_cache_policy_error(const StepCachePolicy& p) {
    if (!std::isfinite(p.thresh) || p.thresh < 0.0f) return "rel_l1_thresh must be finite and >= 0";
    for (int k = 0; k < 5; ++k) if (!std::isfinite(p.coeff[k])) return "non-finite coefficient";
    if (p.n_pattern < 0 || (p.n_pattern > 0 && !p.pattern)) return "pattern is null with n_pattern > 0, or n_pattern is negative";
    for (int i = 0; i < p.n_pattern; ++i) if (p.pattern[i] > 2) return "pattern values are 0 (decide), 1 (compute) or 2 (reuse)";
    return nullptr;
}

// (((c0 x + c1) x + c2) x + c3) x + c4 by Horner in f64 from the f32 coefficients
inline double step_cache_poly(const float c[5], double x) {
    return ((((double)c[0] * x + (double)c[1]) * x + (double)c[2]) * x + (double)c[3]) * x + (double)c[4];
}

// The invalid-row rule, written once: a reuse whose cache rows do not all hold a residual computes, and acc = 0.  The library learns
// which rows a step reads after the measurement (ltx_step_cache_require), so it applies the rule there; -> the decision that stands.
inline int step_cache_demote(StepCacheState* st, int reuse, bool rows_valid) {
    if (reuse && !rows_valid) { st->acc = 0.0; reuse = 0; }
    return reuse;
}

// The decision of step i of N after its measurement (num, den).  rows_valid: every cache row the step would read holds a residual.
// -> 1 reuse, 0 compute.  The state afterwards: a measurement exists; acc as the rule leaves it.
inline int step_cache_decide(StepCacheState* st, const StepCachePolicy& p, int i, int N, double num, double den, bool rows_valid) {
    const bool had = st->have_prev;
    st->have_prev = true;
    const int forced = p.pattern && i >= 0 && i < p.n_pattern ? (int)p.pattern[i] : 0;
    int reuse;
    if (forced == 1) { st->acc = 0.0; reuse = 0; }
    else if (forced == 2) reuse = 1;                             // (acc stays)
    else {
        const double d = den == 0.0 ? 0.0 : num / den;
        if (!had || i == 0 || i == N - 1 || den == 0.0 || !std::isfinite(d)) { st->acc = 0.0; reuse = 0; }
        else {
            st->acc += step_cache_poly(p.coeff, d);
            reuse = st->acc < (double)p.thresh ? 1 : 0;
            if (!reuse) st->acc = 0.0;
        }
    }
    return step_cache_demote(st, reuse, rows_valid);
}
