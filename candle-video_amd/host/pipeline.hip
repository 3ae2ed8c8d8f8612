// Host side of the drop-in: LtxPipeline::call control flow, FlowMatchEulerDiscreteScheduler scalar
// math, PCG32 latent generator and video_coords — C++ restatement above the kernel C ABI.
// Reference: src/models/ltx_video/t2v_pipeline.rs (:627-1073), scheduler.rs (:172-207, 274-412, 495-595,
// 646-668), src/utils/deterministic_rng.rs (:11-81), examples/ltx-video/main.rs (:567-646).
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "../csrc/model_util.h"
#include "../csrc/options.h"
#include "../../include/ltxhip_cond.h"
#include "../../include/ltxhip_guidance.h"
#include "../../include/ltxhip_keyframes.h"
#include "../../include/ltxhip_stepcache.h"
#include "cond_plan.h"
#include "step_plan.h"

// calculate_shift (t2v_pipeline.rs:159-169), f32 arithmetic
extern "C" float ltx_calculate_shift(int seq_len, int base_seq_len, int max_seq_len, float base_shift, float max_shift) {
    float m = (max_shift - base_shift) / (float)(max_seq_len - base_seq_len);
    float b = base_shift - m * (float)base_seq_len;
    return (float)seq_len * m + b;
}

// set_timesteps with explicit sigmas (scheduler.rs:320-412) + i64 truncation of the trait wrapper (:658-659)
extern "C" int ltx_sched_set_timesteps(const float* sigmas_in, int n, float mu, int use_mu, float shift,
                                       float shift_terminal, int use_shift_terminal, float* sigmas_out, int64_t* timesteps_out) {
    if (!sigmas_in || n < 1 || !sigmas_out) LTX_FAIL(LTX_ERR_ARG, "ltx_sched_set_timesteps: bad argument");
    std::vector<float> s(sigmas_in, sigmas_in + n);
    if (use_mu) {                                   // time_shift_scalar, exponential (:172-179), sigma = 1
        const float emu = std::exp(mu);
        for (float& v : s) { float base = std::pow(1.0f / v - 1.0f, 1.0f); v = emu / (emu + base); }
    } else {
        for (float& v : s) v = shift * v / (1.0f + (shift - 1.0f) * v);
    }
    if (use_shift_terminal) {                       // stretch_shift_to_terminal_vec (:188-207)
        const float one_minus_last = 1.0f - s[n - 1];
        const float denom = 1.0f - shift_terminal;
        if (std::fabs(denom) < 1e-12f) LTX_FAIL(LTX_ERR_ARG, "shift_terminal too close to 1.0");
        const float scale = one_minus_last / denom;
        for (float& v : s) v = 1.0f - ((1.0f - v) / scale);
    }
    for (int i = 0; i < n; ++i) {
        sigmas_out[i] = s[i];
        if (timesteps_out) timesteps_out[i] = (int64_t)(s[i] * 1000.0f);
    }
    sigmas_out[n] = 0.0f;                           // terminal sigma (:398)
    return LTX_OK;
}

namespace {
// Regularised incomplete beta function I_x(a, b) (continued fraction, modified Lentz) and its inverse by bisection + Newton, f64:
// what statrs' Beta::inverse_cdf / scipy.stats.beta.ppf compute (scheduler.rs:247-272 calls the former).
double betacf(double a, double b, double x) {
    const double tiny = 1e-300;
    double c = 1.0, d = 1.0 - (a + b) * x / (a + 1.0);
    if (std::fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 500; ++m) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((a + m2 - 1.0) * (a + m2));
        d = 1.0 + aa * d; if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d; h *= d * c;
        aa = -(a + m) * (a + b + m) * x / ((a + m2) * (a + m2 + 1.0));
        d = 1.0 + aa * d; if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (std::fabs(del - 1.0) < 1e-16) break;
    }
    return h;
}
double betai(double a, double b, double x) {
    if (x <= 0.0) return 0.0;
    if (x >= 1.0) return 1.0;
    const double lbt = std::lgamma(a + b) - std::lgamma(a) - std::lgamma(b) + a * std::log(x) + b * std::log1p(-x);
    if (x < (a + 1.0) / (a + b + 2.0)) return std::exp(lbt) * betacf(a, b, x) / a;
    return 1.0 - std::exp(lbt) * betacf(b, a, 1.0 - x) / b;
}
double beta_ppf(double p, double a, double b) {
    if (p <= 0.0) return 0.0;
    if (p >= 1.0) return 1.0;
    double lo = 0.0, hi = 1.0, x = 0.5;
    for (int it = 0; it < 200; ++it) {
        const double f = betai(a, b, x) - p;
        if (f > 0.0) hi = x; else lo = x;
        // Newton step from the density; kept only if it stays inside the bracket
        const double lpdf = std::lgamma(a + b) - std::lgamma(a) - std::lgamma(b) + (a - 1.0) * std::log(x) + (b - 1.0) * std::log1p(-x);
        double xn = x - f / std::exp(lpdf);
        if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);
        if (std::fabs(xn - x) < 1e-15) { x = xn; break; }
        x = xn;
    }
    return x;
}
std::vector<float> linspace_f32(float start, float end, int steps) {     // scheduler.rs:209-220
    std::vector<float> v((size_t)(steps > 0 ? steps : 0));
    if (steps == 1) v[0] = start;
    else for (int i = 0; i < steps; ++i) v[i] = start + (end - start) * (float)i / (float)(steps - 1);
    return v;
}
}  // namespace

extern "C" int ltx_sched_set_timesteps_ex(const float* sigmas_in, int n, float mu, int use_mu, float shift,
                                          float shift_terminal, int use_shift_terminal, int sigma_kind, int invert_sigmas,
                                          float* sigmas_out, int64_t* timesteps_out) {
    if (sigma_kind < 0 || sigma_kind > 3) LTX_FAIL(LTX_ERR_ARG, "ltx_sched_set_timesteps_ex: sigma_kind must be 0 (none), 1 (karras), 2 (exponential) or 3 (beta)");
    LTX_TRY(ltx_sched_set_timesteps(sigmas_in, n, mu, use_mu, shift, shift_terminal, use_shift_terminal, sigmas_out, timesteps_out));
    std::vector<float> s(sigmas_out, sigmas_out + n);
    const float smin = s[n - 1], smax = s[0];
    if (sigma_kind == 1) {                           // convert_to_karras (:222-235)
        const float rho = 7.0f, mn = std::pow(smin, 1.0f / rho), mx = std::pow(smax, 1.0f / rho);
        const std::vector<float> ramp = linspace_f32(0.0f, 1.0f, n);
        for (int i = 0; i < n; ++i) s[i] = std::pow(mx + ramp[i] * (mn - mx), rho);
    } else if (sigma_kind == 2) {                    // convert_to_exponential (:237-245)
        const std::vector<float> logs = linspace_f32(std::log(smax), std::log(smin), n);
        for (int i = 0; i < n; ++i) s[i] = std::exp(logs[i]);
    } else if (sigma_kind == 3) {                    // convert_to_beta (:247-272), alpha = beta = 0.6 (:369)
        const std::vector<float> lin = linspace_f32(0.0f, 1.0f, n);
        for (int i = 0; i < n; ++i) {
            const double t = 1.0 - (double)lin[i];
            s[i] = (float)((double)smin + beta_ppf(t, 0.6, 0.6) * (double)(smax - smin));
        }
    }
    for (int i = 0; i < n; ++i) {
        if (invert_sigmas) s[i] = 1.0f - s[i];
        sigmas_out[i] = s[i];
        if (timesteps_out) timesteps_out[i] = (int64_t)(s[i] * 1000.0f);
    }
    sigmas_out[n] = invert_sigmas ? 1.0f : 0.0f;     // terminal sigma (:389-399)
    return LTX_OK;
}

// ---- PCG32 (deterministic_rng.rs) ----
namespace {
struct Pcg32 {
    uint64_t state, inc;
    Pcg32(uint64_t seed, uint64_t inc_) : state(0), inc((inc_ << 1) | 1) { next_u32(); state += seed; next_u32(); }
    uint32_t next_u32() {
        uint64_t old = state;
        state = old * 6364136223846793005ULL + inc;
        uint32_t xorshifted = (uint32_t)(((old >> 18) ^ old) >> 27);
        uint32_t rot = (uint32_t)(old >> 59);
        return (xorshifted >> rot) | (xorshifted << ((0u - rot) & 31));
    }
    float next_f32() { return (float)(next_u32() >> 8) * 5.9604645e-8f; }
    void next_gaussian(float& z0, float& z1) {
        float u1;
        do { u1 = next_f32(); } while (!(u1 > 1e-7f));
        float u2 = next_f32();
        float mag = std::sqrt(-2.0f * std::log(u1));
        const float two_pi_u2 = 2.0f * 3.14159265358979323846f * u2;
        z0 = mag * std::cos(two_pi_u2); z1 = mag * std::sin(two_pi_u2);
    }
};
}  // namespace

extern "C" int ltx_pcg32_randn(uint64_t seed, uint64_t inc, size_t n, float* out) {
    if (!out) LTX_FAIL(LTX_ERR_ARG, "ltx_pcg32_randn: null output");
    Pcg32 r(seed, inc);
    for (size_t i = 0; i < n; i += 2) {
        float a, b; r.next_gaussian(a, b);
        out[i] = a; if (i + 1 < n) out[i + 1] = b;
    }
    return LTX_OK;
}

// the integer stream itself (deterministic_rng.rs:23-35): bit-exact by construction, pinned to the published PCG32 vectors
extern "C" int ltx_pcg32_u32(uint64_t seed, uint64_t inc, size_t n, uint32_t* out) {
    if (!out) LTX_FAIL(LTX_ERR_ARG, "ltx_pcg32_u32: null output");
    Pcg32 r(seed, inc);
    for (size_t i = 0; i < n; ++i) out[i] = r.next_u32();
    return LTX_OK;
}

// ---- device memory for hosts that have no HIP bindings of their own (the Rust shim, rust/hip_backend.rs) ----
extern "C" int ltx_device_alloc(size_t bytes, int device, void** out) {
    if (!out) LTX_FAIL(LTX_ERR_ARG, "ltx_device_alloc: null output");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMalloc(out, bytes ? bytes : 1));
    return LTX_OK;
}
extern "C" int ltx_device_free(void* p) { if (p) HIP_TRY(hipFree(p)); return LTX_OK; }
extern "C" int ltx_memcpy_h2d(void* dst_device, const void* src_host, size_t bytes, ltx_stream stream) {
    HIP_TRY(hipMemcpyAsync(dst_device, src_host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return LTX_OK;
}
extern "C" int ltx_memcpy_d2h(void* dst_host, const void* src_device, size_t bytes, ltx_stream stream) {
    HIP_TRY(hipMemcpyAsync(dst_host, src_device, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return LTX_OK;
}
extern "C" int ltx_stream_synchronize(ltx_stream stream) { HIP_TRY(hipStreamSynchronize((hipStream_t)stream)); return LTX_OK; }

// video_coords (t2v_pipeline.rs:798-847): f' = clamp(8f-7, 0, 1000)/frame_rate ; h' = 32h ; w' = 32w
extern "C" int ltx_build_video_coords(int F, int H, int W, int frame_rate, int ts_ratio, int sp_ratio, float* out) {
    if (!out || F < 1 || H < 1 || W < 1 || frame_rate < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_build_video_coords: bad argument");
    const float inv_fr = (float)(1.0 / (double)frame_rate);
    size_t i = 0;
    for (int f = 0; f < F; ++f)
        for (int h = 0; h < H; ++h)
            for (int w = 0; w < W; ++w) {
                float vf = (float)f * (float)ts_ratio + (1.0f - (float)ts_ratio);
                vf = std::fmin(std::fmax(vf, 0.0f), 1000.0f) * inv_fr;
                out[i++] = vf; out[i++] = (float)h * (float)sp_ratio; out[i++] = (float)w * (float)sp_ratio;
            }
    return LTX_OK;
}

// The one fill of a mix's arguments, for the five C entries below and the denoise loop.  step_noise: the stochastic update on
// (sigma, sigma_next), null: Euler with dt; hold: the held frames, null: none; stats: the classic mix's workspace (the _ex mix has its own).
static GuidanceArgs guidance_args(const void* text, const void* uncond, const void* perturbed, ltx_dtype pred_dtype, float* latents, float* noise_pred_out,
                                  int B, int64_t n, float guidance_scale, float guidance_rescale, float stg_scale, float dt, float sigma, float sigma_next,
                                  const float* step_noise, void* stats_ws, const unsigned char* hold, int num_frames, int64_t frame_elems) {
    GuidanceArgs a;
    a.text = text; a.uncond = uncond; a.pert = perturbed; a.pred_dtype = pred_dtype == LTX_BF16 ? LTX_DT_BF16 : LTX_DT_F32;
    a.latents = latents; a.noise_out = noise_pred_out; a.B = B; a.n_per_batch = n;
    a.guidance_scale = guidance_scale; a.guidance_rescale = guidance_rescale; a.stg_scale = stg_scale;
    if (step_noise) { a.sigma = sigma; a.sigma_next = sigma_next; a.step_noise = step_noise; } else a.dt = dt;
    a.stats = reinterpret_cast<double*>(stats_ws);
    if (hold) { a.hold = hold; a.num_frames = num_frames; a.frame_elems = frame_elems; }
    return a;
}

extern "C" int ltx_guidance_step(const void* text, const void* uncond, const void* perturbed, ltx_dtype pred_dtype,
                                 float* latents, float* noise_pred_out, int B, int64_t n,
                                 float guidance_scale, float guidance_rescale, float stg_scale, float dt,
                                 void* stats_ws, ltx_stream stream) {
    return ltx_launch_guidance_step(guidance_args(text, uncond, perturbed, pred_dtype, latents, noise_pred_out, B, n, guidance_scale, guidance_rescale, stg_scale,
                                                  dt, 0.0f, 0.0f, nullptr, stats_ws, nullptr, 1, 0), (hipStream_t)stream);
}

extern "C" int ltx_guidance_step_stochastic(const void* text, const void* uncond, const void* perturbed, ltx_dtype pred_dtype,
                                            float* latents, float* noise_pred_out, int B, int64_t n,
                                            float guidance_scale, float guidance_rescale, float stg_scale,
                                            float sigma, float sigma_next, const float* step_noise,
                                            void* stats_ws, ltx_stream stream) {
    if (!step_noise || !latents) LTX_FAIL(LTX_ERR_ARG, "ltx_guidance_step_stochastic: latents and step_noise are required");
    return ltx_launch_guidance_step(guidance_args(text, uncond, perturbed, pred_dtype, latents, noise_pred_out, B, n, guidance_scale, guidance_rescale, stg_scale,
                                                  0.0f, sigma, sigma_next, step_noise, stats_ws, nullptr, 1, 0), (hipStream_t)stream);
}

// ---- held frames (include/ltxhip_cond.h) ----
extern "C" int ltx_guidance_step_held(const void* text, const void* uncond, const void* perturbed, ltx_dtype pred_dtype,
                                      float* latents, float* noise_pred_out, int B, int64_t n,
                                      float guidance_scale, float guidance_rescale, float stg_scale, float dt,
                                      void* stats_ws, const unsigned char* hold, int num_frames, int64_t frame_elems, ltx_stream stream) {
    if (!hold) LTX_FAIL(LTX_ERR_ARG, "ltx_guidance_step_held: hold is required");
    return ltx_launch_guidance_step_held(guidance_args(text, uncond, perturbed, pred_dtype, latents, noise_pred_out, B, n, guidance_scale, guidance_rescale, stg_scale,
                                                       dt, 0.0f, 0.0f, nullptr, stats_ws, hold, num_frames, frame_elems), (hipStream_t)stream);
}

extern "C" int ltx_guidance_step_stochastic_held(const void* text, const void* uncond, const void* perturbed, ltx_dtype pred_dtype,
                                                 float* latents, float* noise_pred_out, int B, int64_t n,
                                                 float guidance_scale, float guidance_rescale, float stg_scale,
                                                 float sigma, float sigma_next, const float* step_noise,
                                                 void* stats_ws, const unsigned char* hold, int num_frames, int64_t frame_elems, ltx_stream stream) {
    if (!step_noise || !latents) LTX_FAIL(LTX_ERR_ARG, "ltx_guidance_step_stochastic_held: latents and step_noise are required");
    if (!hold) LTX_FAIL(LTX_ERR_ARG, "ltx_guidance_step_stochastic_held: hold is required");
    return ltx_launch_guidance_step_held(guidance_args(text, uncond, perturbed, pred_dtype, latents, noise_pred_out, B, n, guidance_scale, guidance_rescale, stg_scale,
                                                       0.0f, sigma, sigma_next, step_noise, stats_ws, hold, num_frames, frame_elems), (hipStream_t)stream);
}

// ---- per-step guidance schedules, CFG-star, the two rescale forms (include/ltxhip_guidance.h) ----
// the argument checks every entry point of a schedule shares; num_layers < 0: the model is not known (the host-only resolve)
static int guidance_schedule_check(const ltx_guidance_schedule* sc, int num_layers) {
    if (!sc) LTX_FAIL(LTX_ERR_ARG, "guidance schedule: null schedule");
    if (sc->n < 1 || sc->n > 64) LTX_FAIL(LTX_ERR_ARG, "guidance schedule: n must be 1..64, got " + std::to_string(sc->n));
    if (!sc->guidance_scale || !sc->stg_scale || !sc->rescale || !sc->skip_offsets) LTX_FAIL(LTX_ERR_ARG, "guidance schedule: guidance_scale, stg_scale, rescale and skip_offsets are required");
    if (sc->rescale_form != LTX_RESCALE_CFG && sc->rescale_form != LTX_RESCALE_MIX)
        LTX_FAIL(LTX_ERR_ARG, "guidance schedule: unknown rescale_form " + std::to_string(sc->rescale_form) + " (0 = LTX_RESCALE_CFG, 1 = LTX_RESCALE_MIX)");
    if (sc->cfg_star != 0 && sc->cfg_star != 1) LTX_FAIL(LTX_ERR_ARG, "guidance schedule: cfg_star must be 0 or 1");
    if (sc->skip_offsets[0] != 0) LTX_FAIL(LTX_ERR_ARG, "guidance schedule: skip_offsets must start at 0");
    for (int j = 0; j < sc->n; ++j) {
        const std::string at = " in entry " + std::to_string(j);
        if (!std::isfinite(sc->guidance_scale[j]) || !std::isfinite(sc->stg_scale[j]) || !std::isfinite(sc->rescale[j])) LTX_FAIL(LTX_ERR_ARG, "guidance schedule: non-finite scale" + at);
        if (sc->guidance_timesteps && !std::isfinite(sc->guidance_timesteps[j])) LTX_FAIL(LTX_ERR_ARG, "guidance schedule: non-finite guidance_timesteps value" + at);
        if (sc->stg_scale[j] < 0.0f) LTX_FAIL(LTX_ERR_ARG, "guidance schedule: negative stg_scale" + at);
        if (sc->skip_offsets[j + 1] < sc->skip_offsets[j]) LTX_FAIL(LTX_ERR_ARG, "guidance schedule: skip_offsets decrease" + at);
        if (sc->skip_offsets[j + 1] > sc->skip_offsets[j] && !sc->skip_blocks) LTX_FAIL(LTX_ERR_ARG, "guidance schedule: skip_blocks is null but a block list is not empty" + at);
        for (int k = sc->skip_offsets[j]; k < sc->skip_offsets[j + 1]; ++k)
            if (sc->skip_blocks[k] < 0 || (num_layers >= 0 && sc->skip_blocks[k] >= num_layers))
                LTX_FAIL(LTX_ERR_ARG, "guidance schedule: block index " + std::to_string(sc->skip_blocks[k]) + " outside the model" + at);
    }
    return LTX_OK;
}

extern "C" int ltx_guidance_schedule_resolve(const ltx_guidance_schedule* sched, const float* sigmas, int N, int* entry_of_step) {
    LTX_TRY(guidance_schedule_check(sched, -1));
    if (!sigmas || !entry_of_step || N < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_guidance_schedule_resolve: sigmas, entry_of_step and N >= 1 are required");
    if (!sched->guidance_timesteps) {
        if (sched->n != 1 && sched->n != N)
            LTX_FAIL(LTX_ERR_ARG, "guidance schedule: without guidance_timesteps n must be 1 or the number of steps (" + std::to_string(N) + "), got " + std::to_string(sched->n));
        for (int i = 0; i < N; ++i) entry_of_step[i] = sched->n == 1 ? 0 : i;
        return LTX_OK;
    }
    for (int i = 0; i < N; ++i) {
        int best = 0; double dbest = std::fabs((double)sched->guidance_timesteps[0] - (double)sigmas[i]);
        for (int j = 1; j < sched->n; ++j) {
            const double d = std::fabs((double)sched->guidance_timesteps[j] - (double)sigmas[i]);
            if (d < dbest) { dbest = d; best = j; }      // (strictly: the first minimum wins a tie)
        }
        entry_of_step[i] = best;
    }
    return LTX_OK;
}

extern "C" size_t ltx_guidance_ws_bytes(int B, int64_t n) { return ltx_guidance_ex_ws_bytes(B, n); }

extern "C" int ltx_guidance_step_ex(const void* text, const void* uncond, const void* perturbed, ltx_dtype pred_dtype,
                                    float* latents, float* noise_pred_out, int B, int64_t n,
                                    float guidance_scale, float guidance_rescale, float stg_scale, int cfg_star, int rescale_form,
                                    float dt, float sigma, float sigma_next, const float* step_noise,
                                    const unsigned char* hold, int num_frames, int64_t frame_elems,
                                    void* ws, float* scalars_out, ltx_stream stream) {
    if (!std::isfinite(guidance_scale) || !std::isfinite(guidance_rescale) || !std::isfinite(stg_scale)) LTX_FAIL(LTX_ERR_ARG, "ltx_guidance_step_ex: non-finite scale");
    if (stg_scale < 0.0f) LTX_FAIL(LTX_ERR_ARG, "ltx_guidance_step_ex: negative stg_scale");
    if (pred_dtype != LTX_F32 && pred_dtype != LTX_BF16) LTX_FAIL(LTX_ERR_ARG, "ltx_guidance_step_ex: bad dtype");
    GuidanceExArgs a;
    a.g = guidance_args(text, uncond, perturbed, pred_dtype, latents, noise_pred_out, B, n, guidance_scale, guidance_rescale, stg_scale,
                        dt, sigma, sigma_next, step_noise, nullptr, hold, num_frames, frame_elems);
    a.cfg_star = cfg_star; a.rescale_form = rescale_form; a.ws = ws; a.scalars_out = scalars_out;
    return ltx_launch_guidance_step_ex(a, (hipStream_t)stream);
}

extern "C" int ltx_cond_apply(float* latents, const float* cond_tokens, int cond_frames, const unsigned char* hold,
                              int B, int num_frames, int tokens_per_frame, int channels, ltx_stream stream) {
    if (!hold) LTX_FAIL(LTX_ERR_ARG, "ltx_cond_apply: hold is required");
    if (!latents || !cond_tokens || B < 1 || num_frames < 1 || cond_frames < 1 || tokens_per_frame < 1 || channels < 1)
        LTX_FAIL(LTX_ERR_ARG, "ltx_cond_apply: bad argument");
    bool any = false;
    for (int b = 0; b < B; ++b)
        for (int f = 0; f < num_frames; ++f)
            if (hold[(size_t)b * num_frames + f]) {
                if (f >= cond_frames) LTX_FAIL(LTX_ERR_ARG, "ltx_cond_apply: held frame " + std::to_string(f) + " lies beyond the " + std::to_string(cond_frames) + " conditioning frame(s)");
                any = true;
            }
    if (!any) return LTX_OK;
    hipStream_t s = (hipStream_t)stream;
    const size_t nh = (size_t)B * num_frames;
    unsigned char* hd = nullptr;
    HIP_TRY(hipMalloc((void**)&hd, nh));
    struct Free { void* p; ~Free() { (void)hipFree(p); } } guard{hd};
    HIP_TRY(hipMemcpyAsync(hd, hold, nh, hipMemcpyHostToDevice, s));
    LTX_TRY(ltx_launch_cond_apply(latents, cond_tokens, cond_frames, hd, B, num_frames, (int64_t)tokens_per_frame * channels, s));
    HIP_TRY(hipStreamSynchronize(s));                        // (hold is the caller's host memory and hd is freed here)
    return LTX_OK;
}

// ---- LtxPipeline::call ----
static thread_local float g_timing[4] = {0, 0, 0, 0};
extern "C" int ltx_pipeline_last_timing(float ms[4]) {
    if (!ms) LTX_FAIL(LTX_ERR_ARG, "null output");
    for (int i = 0; i < 4; ++i) ms[i] = g_timing[i];
    return LTX_OK;
}

static thread_local int t_steps[2] = {0, 0};
extern "C" int ltx_pipeline_last_steps(int* executed, int* requested) {
    if (executed) *executed = t_steps[0];
    if (requested) *requested = t_steps[1];
    return LTX_OK;
}

namespace {
// Device scratch of the denoise loop, kept per (thread, device) across calls: per-call hipMalloc/hipFree (an implicit
// device sync each) and the coords rebuild + blocking upload cost ~1 ms per video for nothing.
struct PipeCache {
    DevBuf stats, coords, hold, gws;
    DevBuf kf_coords, kf_clean, kf_grid;                // a keyframe call: its own coordinates (never the geometry-keyed ones), the placed latents, the stripped grid
    DevBuf g_lat, g_emb, g_mask, g_pred, g_coords;      // the branch slots of a step (BranchBatch below): inputs of a batched forward / every prediction
    int coords_key[6] = {-1, -1, -1, -1, -1, -1};      // B, F, H, W, frame_rate, ratios packed
};
PipeCache& pipe_cache(int device) {
    thread_local std::map<int, PipeCache> caches;
    return caches[device];
}
struct PipeScratch {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<hipEvent_t> step_ev;        // three per denoise step (start, after the forwards, after the update); every
                                            // event is owned exactly once and pushed here the moment it exists
    int new_event(hipEvent_t* out) {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreate(&e));
        step_ev.push_back(e); *out = e;
        return LTX_OK;
    }
    ~PipeScratch() {
        for (auto e : ev) if (e) (void)hipEventDestroy(e);
        for (auto e : step_ev) (void)hipEventDestroy(e);
    }
};
}  // namespace

// The schedule of one call at S latent tokens (t2v_pipeline.rs:750-791): N + 1 sigmas and N truncated timesteps.  The one place that
// builds it: the denoise loop below and ltx_pipeline_first_sigma (the re-noise in front of a second pass, csrc/upsampler.hip) both ask here.
int ltx_pipeline_schedule(const ltx_pipeline_params* p, int S, std::vector<float>* sig, std::vector<int64_t>* ts) {
    const int N = p->num_inference_steps;
    if (N < 1) LTX_FAIL(LTX_ERR_ARG, "num_inference_steps must be >= 1");
    std::vector<float> sig_in(N);
    sig->assign(N + 1, 0.0f); ts->assign(N, 0);
    const bool custom = p->sigmas != nullptr;
    for (int i = 0; i < N; ++i)
        sig_in[i] = custom ? p->sigmas[i] : (N == 1 ? 1.0f : 1.0f + (1.0f / (float)N - 1.0f) * (float)i / (float)(N - 1));
    const float mu = custom ? 0.0f : ltx_calculate_shift(S, 256, 4096, 0.5f, 1.15f);      // static default cfg (scheduler.rs:638-639)
    return ltx_sched_set_timesteps(sig_in.data(), N, mu, 1, 1.0f, p->shift_terminal, p->use_shift_terminal, sig->data(), ts->data());
}

// A conditioned run (include/ltxhip_cond.h, ltxhip_keyframes.h): the sequence is G groups of h * w tokens per batch row, E extra ones
// in front of the F' grid frames.  ltx_pipeline_call_cond fills it with the grid alone and one hold row; a keyframe call with its layout.
struct CondRun {
    int G = 0, E = 0;
    std::vector<float> tcap;                 // [B, G]: the model sees min(t_i, tcap) for the group's tokens
    std::vector<unsigned char> hold;         // [hold_rows, B, G], 1 = the group keeps its bits on the step; one row: the same on every step
    int hold_rows = 1;
    const float* coords = nullptr;           // HOST [G * h * w, 3] of one batch row; null: the grid's (E == 0), cached by geometry
    std::vector<CondPlaceEntry> place;       // placement in front of the loop (empty: the latents arrive placed)
    float noise_scale = 0.0f; const float* cond_noise = nullptr;      // noised holds: c and DEVICE [steps, B, G * h * w * C]
    std::vector<int> hard;                   // ... and the groups they cover
};

// The latent geometry of a call (t2v_pipeline.rs:743-745): the VAE's compression ratios, (8, 32) without one.  A ratio below 1 leaves
// its extents 0 (the callers that take a ratio from outside refuse it).
struct LatentGeom { int ts_ratio = 8, sp_ratio = 32, F = 0, H = 0, W = 0; };
static int latent_geom(ltx_vae* vae, const ltx_pipeline_params* p, LatentGeom* g) {
    if (vae) { ltx_vae_config vc; LTX_TRY(ltx_vae_get_config(vae, &vc)); g->ts_ratio = vc.temporal_compression_ratio; g->sp_ratio = vc.spatial_compression_ratio; }
    if (g->ts_ratio >= 1) g->F = (p->num_frames - 1) / g->ts_ratio + 1;
    if (g->sp_ratio >= 1) { g->H = p->height / g->sp_ratio; g->W = p->width / g->sp_ratio; }
    return LTX_OK;
}
static bool any_held(const unsigned char* hold, int B, int F) {
    for (size_t j = 0; j < (size_t)B * (F > 0 ? F : 0); ++j) if (hold[j]) return true;
    return false;
}

// what every pipeline entry hands through to the loop
struct PipeIO { float* latents; const float *prompt_embeds, *prompt_mask, *neg_embeds, *neg_mask, *decode_noise; int B, K; float* out_video; ltx_stream stream; };

// The branch slots of host/step_plan.h on the device, B rows each: slot 0 negative prompt, slot 1 prompt, slot 2 prompt (perturbed).
// Every prediction lies in its slot of g_pred, whichever way its forward ran.  A step whose branches run as ONE forward (:860-940: up to
// three B-row forwards on the same latents) reads the slots [slot0, slot0 + nbr) of g_lat / g_emb / g_mask / g_coords: branch rows are
// independent, every plan of a GEMM shape returns the same bits, and a row that skips a layer keeps its row partials (dit.hip) - so each
// branch's prediction is, bit for bit, the separate forward's WHERE B * S and nbr * B * S rows take the same kernels and K partition
// (above 512 rows per branch: C2 / C3 / C5; at a few hundred tokens the split-K factor, the one-row-per-block norms and the deferred ff2
// depend on the row count and the two forms agree to rounding only: tests/test_gpu_c3.py), at 2.5 instead of 3 rounds of the chip per
// attention launch and fewer one-round grids (one C3 step 61.8 -> 58.1 ms).  guidance_batch=0: the reference's three calls.
// The DiT's text context is keyed by (embeddings, mask, rows): one key for an unscheduled call, at most the four it keeps under a
// schedule (DESIGN.md enumerates them).  Every pointer is fixed in front of the loop (rope_key compares the coordinates' in the caching scope).
struct BranchBatch {
    PipeCache& pc; int B; int64_t n; size_t emb_n, mask_n, coords_n;         // elements of one slot
    const float* src_emb[3]; const float* src_mask[3];                       // the caller's tensors of each slot
    float* pred(int slot) const { return pc.g_pred.as<float>() + (size_t)slot * B * n; }
    const float* emb(int slot) const { return pc.g_emb.as<float>() + (size_t)slot * emb_n; }
    const float* mask(int slot) const { return pc.g_mask.as<float>() + (size_t)slot * mask_n; }
    const float* coords(int slot) const { return pc.g_coords.as<float>() + (size_t)slot * coords_n; }
    // sizes the buffers; with a batched step in the plan, the inputs of the slots some step runs (coords: DEVICE [B, S, 3])
    int stage(const StepPlan& plan, const float* coords_dev, hipStream_t s) {
        LTX_TRY(pc.g_pred.ensure((size_t)3 * B * n * sizeof(float)));
        if (!plan.any_batched) return LTX_OK;
        LTX_TRY(pc.g_lat.ensure((size_t)3 * B * n * sizeof(float))); LTX_TRY(pc.g_emb.ensure(3 * emb_n * sizeof(float)));
        LTX_TRY(pc.g_mask.ensure(3 * mask_n * sizeof(float))); LTX_TRY(pc.g_coords.ensure(3 * coords_n * sizeof(float)));
        const bool present[3] = {plan.any_cfg, true, plan.any_stg};
        for (int k = 0; k < 3; ++k) {
            if (!present[k]) continue;
            HIP_TRY(hipMemcpyAsync(pc.g_emb.as<float>() + (size_t)k * emb_n, src_emb[k], emb_n * sizeof(float), hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(pc.g_mask.as<float>() + (size_t)k * mask_n, src_mask[k], mask_n * sizeof(float), hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(pc.g_coords.as<float>() + (size_t)k * coords_n, coords_dev, coords_n * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        return LTX_OK;
    }
};

// The step cache of a call (include/ltxhip_stepcache.h): the caller's parameters and where the decisions go.  Null in pipeline_run: not
// one launch or wait of the loop changes.
struct PipeStepCache { const ltx_step_cache_params* params; unsigned char* reused_out; float* distance_out; };

// cr: null - no conditioning; plan: the branches, scales and perturbed blocks of every step (host/step_plan.h); scd: the step cache or null
static int pipeline_run(ltx_dit* dit, ltx_vae* vae, const ltx_pipeline_params* p, const CondRun* cr, const StepPlan& plan, const PipeIO& io,
                        const PipeStepCache* scd = nullptr) {
    float* const latents = io.latents; const int B = io.B, K = io.K;
    if (!dit || !p || !latents || !io.prompt_embeds || !io.prompt_mask) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call: null argument");
    if (!p->output_latent && (!vae || !io.out_video)) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call: decode requested without vae/out_video");
    // check_inputs (:313-365)
    if (p->height % 32 != 0 || p->width % 32 != 0) LTX_FAIL(LTX_ERR_ARG, "`height` and `width` must be divisible by 32");
    if (p->num_inference_steps < 1) LTX_FAIL(LTX_ERR_ARG, "num_inference_steps must be >= 1");
    // :304-310: whether ANY step has the branch (the steps decide for themselves below)
    if (plan.any_cfg && (!io.neg_embeds || !io.neg_mask)) LTX_FAIL(LTX_ERR_ARG, "classifier-free guidance needs negative embeddings and mask");
    if (p->stochastic_sampling && !p->step_noise) LTX_FAIL(LTX_ERR_ARG, "stochastic_sampling needs step_noise [steps,B,S*C]");
    hipStream_t s = (hipStream_t)io.stream;
    ltx_dit_config dc; LTX_TRY(ltx_dit_get_config(dit, &dc));
    LatentGeom lg; LTX_TRY(latent_geom(vae, p, &lg));
    const int F = lg.F, H = lg.H, W = lg.W;
    const int G = cr ? cr->G : F, E = cr ? cr->E : 0;                      // groups of the sequence the model sees; the grid is its last F
    const int S = G * H * W, C = dc.in_channels, L = dc.num_layers;
    const int64_t n = (int64_t)S * C;
    if (cr && (G != E + F || cr->tcap.size() != (size_t)B * G || cr->hold.size() != (size_t)cr->hold_rows * B * G ||
               (cr->hold_rows != 1 && cr->hold_rows != p->num_inference_steps) || (E > 0 && !cr->coords)))
        LTX_FAIL(LTX_ERR_ARG, "pipeline: inconsistent conditioning description");

    // skip blocks: permanent iff STG is off (:691-697); a schedule never skips a block for good
    if (plan.set_skip) LTX_TRY(ltx_dit_set_skip_blocks(dit, plan.perm_skip, plan.n_perm_skip));
    // sigmas / mu / timesteps (:750-791)
    const int N = p->num_inference_steps;
    std::vector<float> sig; std::vector<int64_t> ts;
    LTX_TRY(ltx_pipeline_schedule(p, F * H * W, &sig, &ts));      // (the grid's tokens, with or without extra groups)

    PipeScratch sc;
    int cur_dev = 0; HIP_TRY(hipGetDevice(&cur_dev));
    PipeCache& pc = pipe_cache(cur_dev);
    const bool classic = plan.mix == STEP_MIX_CLASSIC;
    LTX_TRY(pc.stats.ensure(64 * B));
    if (!classic) LTX_TRY(pc.gws.ensure(ltx_guidance_ex_ws_bytes(B, n)));
    if (cr) {                                        // device copy for the update kernels (the model's per-group timesteps are built on the host)
        LTX_TRY(pc.hold.ensure(cr->hold.size()));
        HIP_TRY(hipMemcpyAsync(pc.hold.p, cr->hold.data(), cr->hold.size(), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));            // (once per call, in front of the loop)
    }
    auto upload_coords = [&](DevBuf& buf, const float* row) -> int {      // one batch row's HOST [S, 3] -> DEVICE [B, S, 3]
        std::vector<float> all((size_t)B * S * 3);
        for (int b = 0; b < B; ++b) std::memcpy(all.data() + (size_t)b * S * 3, row, sizeof(float) * S * 3);
        LTX_TRY(buf.ensure(all.size() * sizeof(float)));
        HIP_TRY(hipMemcpyAsync(buf.p, all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        return LTX_OK;
    };
    const int key[6] = {B, F, H, W, p->frame_rate, lg.ts_ratio * 1000 + lg.sp_ratio};
    if (cr && cr->coords) {
        // a layout's own coordinates: a buffer of their own, written on every call - the geometry-keyed one below is neither read nor
        // re-keyed, and the pointer is stable for the whole call (the DiT's rope_key compares it inside the caching scope)
        LTX_TRY(upload_coords(pc.kf_coords, cr->coords));
    } else if (std::memcmp(key, pc.coords_key, sizeof(key)) != 0) {      // video_coords [B,S,3] (:798-847): rebuilt only when the geometry changes
        std::vector<float> vc((size_t)S * 3);
        LTX_TRY(ltx_build_video_coords(F, H, W, p->frame_rate, lg.ts_ratio, lg.sp_ratio, vc.data()));
        LTX_TRY(upload_coords(pc.coords, vc.data()));
        std::memcpy(pc.coords_key, key, sizeof(key));
    }
    const float* coords = (cr && cr->coords ? pc.kf_coords : pc.coords).as<float>();
    BranchBatch bb{pc, B, n, (size_t)B * K * dc.caption_channels, (size_t)B * K, (size_t)B * S * 3,
                   {io.neg_embeds, io.prompt_embeds, io.prompt_embeds}, {io.neg_mask, io.prompt_mask, io.prompt_mask}};
    LTX_TRY(bb.stage(plan, coords, s));
    for (auto& e : sc.ev) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(sc.ev[0], s));
    const int64_t group_elems = (int64_t)H * W * C;
    const bool noised = cr && cr->noise_scale > 0.0f && !cr->hard.empty();
    if (cr && !cr->place.empty()) LTX_TRY(ltx_launch_cond_place(latents, cr->place.data(), (int)cr->place.size(), B, G, group_elems, s));
    if (noised) {                                    // what placement wrote, for the noised holds of every step
        LTX_TRY(pc.kf_clean.ensure((size_t)B * n * sizeof(float)));
        HIP_TRY(hipMemcpyAsync(pc.kf_clean.p, latents, (size_t)B * n * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    struct CtxScope { ltx_dit* d; ~CtxScope() { (void)ltx_dit_context_cache(d, 0); } } ctx_scope{dit};
    LTX_TRY(ltx_dit_context_cache(dit, 1));     // embeddings/masks are step-invariant inside one call
    // the step cache: 3 * B rows, one set per branch slot of host/step_plan.h; it lives for this call
    struct CacheScope { ltx_step_cache* c = nullptr; ~CacheScope() { ltx_step_cache_destroy(c); } } cache;
    if (scd) {
        LTX_TRY(ltx_step_cache_create(dit, 3 * B, &cache.c));
        for (int i = 0; i < N; ++i) { if (scd->reused_out) scd->reused_out[i] = 0; if (scd->distance_out) scd->distance_out[i] = 0.0f; }
    }
    // denoising loop (:860-994)
    const bool hooked = p->interrupt != nullptr || p->on_step != nullptr;
    bool stopped = false; int steps_run = 0;
    std::vector<float> tframes;                             // held frames: the step's timesteps per (row of the forward, latent frame)
    std::vector<float> slm;                                 // the step's skip mask [L, rows of the forward] (:911-923)
    std::vector<hipEvent_t> done_ev;                        // e2 of every executed step (owned by sc.step_ev)
    for (int i = 0; i < N; ++i) {
        // interrupt / per-step hook (:861-865).  The loop only ENQUEUES work: the host stays at most one step ahead of the device
        // here, so that a flag raised while step k runs skips from step k + 2 on at the latest
        if (hooked) {
            if (done_ev.size() >= 2) HIP_TRY(hipEventSynchronize(done_ev[done_ev.size() - 2]));
            if (!stopped && p->on_step && p->on_step(p->on_step_user, i, N, ts[i]) != 0) stopped = true;
            if (stopped || (p->interrupt && *p->interrupt)) continue;
        }
        ++steps_run;
        float tvals[8]; for (int b = 0; b < 8; ++b) tvals[b] = (float)ts[i];       // Tensor::full(t as f32, (b,))
        hipEvent_t e0, e1, e2;
        LTX_TRY(sc.new_event(&e0)); LTX_TRY(sc.new_event(&e1)); LTX_TRY(sc.new_event(&e2));
        HIP_TRY(hipEventRecord(e0, s));
        const StepEntry& st = plan.steps[(size_t)i];        // the branches of THIS step (uncond iff g > 1, perturbed iff s > 0)
        const int frows = st.batched ? st.rows : B;         // rows of one forward of this step
        if (cr) {                                    // held frames: the model sees timestep 0 for their tokens and t_i for the rest, in every guidance branch
            tframes.resize((size_t)frows * G);
            for (size_t r = 0; r < tframes.size() / ((size_t)B * G); ++r)
                for (size_t j = 0; j < (size_t)B * G; ++j) tframes[r * B * G + j] = std::fmin((float)ts[i], cr->tcap[j]);
        }
        if (noised) {
            const float kn = (float)((double)cr->noise_scale * (double)sig[i] * (double)sig[i]);
            LTX_TRY(ltx_launch_cond_noise(latents, pc.kf_clean.as<float>(), cr->cond_noise + (size_t)i * B * n, cr->hard.data(), (int)cr->hard.size(), B, G, group_elems, kn, s));
        }
        const unsigned char* hold_i = cr ? pc.hold.as<unsigned char>() + (cr->hold_rows > 1 ? (size_t)i * B * G : 0) : nullptr;
        int reuse = 0;
        if (scd) {                                   // one measurement of the B videos and one decision for every branch of the step
            float dist = 0.0f;
            LTX_TRY(ltx_step_cache_decide(cache.c, dit, latents, cr ? tframes.data() : tvals, cr ? G : 0, B, S, cr ? G : F, H, W, LTX_F32, i, N, scd->params, &reuse, &dist, s));
            LTX_TRY(ltx_step_cache_require(cache.c, dit, st.slot0 * B, st.nbr * B, S, &reuse));      // (a branch the steps before did not run)
            if (scd->reused_out) scd->reused_out[i] = (unsigned char)reuse;
            if (scd->distance_out) scd->distance_out[i] = dist;
        }
        auto forward = [&](const void* x, const void* emb, const float* mk, int rows, const float* vc, const float* skip, void* pred, int slot) -> int {
            if (scd) return ltx_dit_forward_cached(dit, cache.c, slot * B, reuse, cr ? G : 0, x, emb, cr ? tframes.data() : tvals, mk, rows, S, K, cr ? G : F, H, W, nullptr, vc, skip, LTX_F32, pred, s);
            if (cr) return ltx_dit_forward_frames(dit, x, emb, tframes.data(), mk, rows, S, K, G, H, W, nullptr, vc, skip, LTX_F32, pred, s);
            return ltx_dit_forward(dit, x, emb, tvals, mk, rows, S, K, F, H, W, nullptr, vc, skip, LTX_F32, pred, s);
        };
        if (st.stg) step_skip_rows(L, frows, st.batched ? (st.nbr - 1) * B : 0, B, st.guide.skip, st.guide.n_skip, &slm);      // (the perturbed branch: the last rows)
        if (st.batched) {
            for (int r = 0; r < st.nbr; ++r) HIP_TRY(hipMemcpyAsync(pc.g_lat.as<float>() + (size_t)r * B * n, latents, (size_t)B * n * sizeof(float), hipMemcpyDeviceToDevice, s));
            LTX_TRY(forward(pc.g_lat.p, bb.emb(st.slot0), bb.mask(st.slot0), st.rows, bb.coords(st.slot0), st.stg ? slm.data() : nullptr, bb.pred(st.slot0), st.slot0));
        } else {
            for (int k = st.slot0; k < st.slot0 + st.nbr; ++k) LTX_TRY(forward(latents, bb.src_emb[k], bb.src_mask[k], B, coords, k == 2 ? slm.data() : nullptr, bb.pred(k), k));
        }
        HIP_TRY(hipEventRecord(e1, s));
        // guidance mix (:941-962) on the branches that ran + scheduler.step (:987; scheduler.rs:544-581): dt = sigma_next - sigma; held groups keep their bits
        GuidanceExArgs ge;
        ge.g = guidance_args(bb.pred(1), st.cfg ? bb.pred(0) : nullptr, st.stg ? bb.pred(2) : nullptr, LTX_F32, latents, nullptr, B, n,
                             st.guide.g, st.guide.r, st.guide.s, sig[i + 1] - sig[i], sig[i], sig[i + 1],
                             p->stochastic_sampling ? p->step_noise + (size_t)i * B * n : nullptr, classic ? pc.stats.p : nullptr, hold_i, G, group_elems);
        if (classic) LTX_TRY(ltx_launch_guidance_step(ge.g, s));
        else {                                       // the mix of include/ltxhip_guidance.h
            ge.cfg_star = plan.cfg_star; ge.rescale_form = plan.rescale_form; ge.ws = pc.gws.p;
            LTX_TRY(ltx_launch_guidance_step_ex(ge, s));
        }
        HIP_TRY(hipEventRecord(e2, s));
        done_ev.push_back(e2);
    }
    t_steps[0] = steps_run; t_steps[1] = N;
    HIP_TRY(hipEventRecord(sc.ev[1], s));
    if (!p->output_latent) {
        // unpack + denormalize + noise mix + decode + postprocess (:1002-1070)
        float tdec[8], nsc[8];
        for (int b = 0; b < 8; ++b) { tdec[b] = p->decode_timestep; nsc[b] = p->decode_noise_scale; }
        ltx_vae_config vc; LTX_TRY(ltx_vae_get_config(vae, &vc));
        const bool tc = vc.timestep_conditioning != 0;
        // the extra groups are dropped: an offset for one batch row, one strided copy of the grid tokens for more
        const float* grid = latents + (size_t)E * group_elems;
        if (E > 0 && B > 1) {
            const size_t row = (size_t)F * group_elems * sizeof(float);
            LTX_TRY(pc.kf_grid.ensure((size_t)B * row));
            HIP_TRY(hipMemcpy2DAsync(pc.kf_grid.p, row, grid, (size_t)n * sizeof(float), row, (size_t)B, hipMemcpyDeviceToDevice, s));
            grid = pc.kf_grid.as<float>();
        }
        LTX_TRY(ltx_vae_decode_tokens(vae, grid, tc ? io.decode_noise : nullptr, nsc, tc ? tdec : nullptr, B, F, H, W, p->tiling, p->postprocess, io.out_video, s));
    }
    HIP_TRY(hipEventRecord(sc.ev[2], s));
    HIP_TRY(hipStreamSynchronize(s));
    float dit_ms = 0, gs_ms = 0, t = 0;
    for (size_t i = 0; i + 3 <= sc.step_ev.size(); i += 3) {
        HIP_TRY(hipEventElapsedTime(&t, sc.step_ev[i], sc.step_ev[i + 1])); dit_ms += t;
        HIP_TRY(hipEventElapsedTime(&t, sc.step_ev[i + 1], sc.step_ev[i + 2])); gs_ms += t;
    }
    g_timing[0] = dit_ms; g_timing[1] = gs_ms;
    HIP_TRY(hipEventElapsedTime(&g_timing[2], sc.ev[1], sc.ev[2]));
    HIP_TRY(hipEventElapsedTime(&g_timing[3], sc.ev[0], sc.ev[2]));
    return LTX_OK;
}

// the unscheduled call: the constant plan of the scalars of `p`
static int pipeline_run_params(ltx_dit* dit, ltx_vae* vae, const ltx_pipeline_params* p, const CondRun* cr, const PipeIO& io, const PipeStepCache* scd = nullptr) {
    StepPlan plan;
    if (p) {
        StepGuide g; g.g = p->guidance_scale; g.s = p->stg_scale; g.r = p->guidance_rescale;
        g.skip = p->skip_block_list; g.n_skip = p->skip_block_list ? p->n_skip_blocks : 0;
        step_plan_constant(p->num_inference_steps, io.B, g, ltx_opt().guidance_batch != 0, &plan);
    }
    return pipeline_run(dit, vae, p, cr, plan, io, scd);
}

extern "C" int ltx_pipeline_call(ltx_dit* dit, ltx_vae* vae, const ltx_pipeline_params* p,
                                 float* latents, const float* prompt_embeds, const float* prompt_mask,
                                 const float* neg_embeds, const float* neg_mask, const float* decode_noise,
                                 int B, int K, float* out_video, ltx_stream stream) {
    return pipeline_run_params(dit, vae, p, nullptr, {latents, prompt_embeds, prompt_mask, neg_embeds, neg_mask, decode_noise, B, K, out_video, stream});
}

// the held frames of include/ltxhip_cond.h as a conditioned run: the grid alone, one hold row, timestep 0 on a held frame
static void cond_run_from_hold(const unsigned char* hold, int B, int F, CondRun* cr) {
    cr->G = F; cr->E = 0; cr->hold_rows = 1;
    cr->hold.assign(hold, hold + (size_t)B * F);
    cr->tcap.resize((size_t)B * F);
    for (size_t j = 0; j < cr->tcap.size(); ++j) cr->tcap[j] = hold[j] ? 0.0f : INFINITY;
}

extern "C" int ltx_pipeline_call_cond(ltx_dit* dit, ltx_vae* vae, const ltx_pipeline_params* p, const ltx_conditioning* cond,
                                      float* latents, const float* prompt_embeds, const float* prompt_mask,
                                      const float* neg_embeds, const float* neg_mask, const float* decode_noise,
                                      int B, int K, float* out_video, ltx_stream stream) {
    if (!cond || !cond->hold) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_cond: conditioning with a hold mask is required");
    if (!p || B < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_cond: null argument");
    LatentGeom lg; LTX_TRY(latent_geom(vae, p, &lg));
    const bool any = any_held(cond->hold, B, lg.F);
    CondRun cr;
    if (any) cond_run_from_hold(cond->hold, B, lg.F, &cr);
    // nothing held: ltx_pipeline_call itself
    return pipeline_run_params(dit, vae, p, any ? &cr : nullptr, {latents, prompt_embeds, prompt_mask, neg_embeds, neg_mask, decode_noise, B, K, out_video, stream});
}

// ---- the pipeline calls under a guidance schedule (include/ltxhip_guidance.h) ----
// cr: the conditioned run or null; sig: the call's sigmas (ltx_pipeline_schedule at the grid's tokens)
static int pipeline_run_sched(ltx_dit* dit, ltx_vae* vae, const ltx_pipeline_params* p, const ltx_guidance_schedule* sched, const CondRun* cr,
                              const std::vector<float>& sig, const PipeIO& io, const PipeStepCache* scd = nullptr) {
    const int N = p->num_inference_steps;
    std::vector<int> entry((size_t)N, 0);
    LTX_TRY(ltx_guidance_schedule_resolve(sched, sig.data(), N, entry.data()));
    std::vector<StepGuide> guides((size_t)N);
    for (int i = 0; i < N; ++i) {
        const int j = entry[(size_t)i];
        StepGuide& g = guides[(size_t)i];
        g.g = sched->guidance_scale[j]; g.s = sched->stg_scale[j]; g.r = sched->rescale[j];
        g.n_skip = sched->skip_offsets[j + 1] - sched->skip_offsets[j];
        g.skip = g.n_skip > 0 ? sched->skip_blocks + sched->skip_offsets[j] : nullptr;
    }
    StepPlan plan;
    step_plan_scheduled(guides.data(), N, io.B, sched->cfg_star, sched->rescale_form, ltx_opt().guidance_batch != 0, &plan);
    return pipeline_run(dit, vae, p, cr, plan, io, scd);
}

extern "C" int ltx_pipeline_call_sched(ltx_dit* dit, ltx_vae* vae, const ltx_pipeline_params* p, const ltx_guidance_schedule* sched,
                                       const ltx_conditioning* cond, float* latents, const float* prompt_embeds, const float* prompt_mask,
                                       const float* neg_embeds, const float* neg_mask, const float* decode_noise,
                                       int B, int K, float* out_video, ltx_stream stream) {
    if (!dit || !p || !sched || B < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_sched: null argument");
    if (cond && !cond->hold) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_sched: conditioning without a hold mask");
    ltx_dit_config dc; LTX_TRY(ltx_dit_get_config(dit, &dc));
    LTX_TRY(guidance_schedule_check(sched, dc.num_layers));
    // the sigmas the denoise loop will run (the same geometry rule and the same builder)
    LatentGeom lg; LTX_TRY(latent_geom(vae, p, &lg));
    if (lg.ts_ratio < 1 || lg.sp_ratio < 1 || p->num_frames < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_sched: bad geometry");
    std::vector<float> sig; std::vector<int64_t> ts;
    LTX_TRY(ltx_pipeline_schedule(p, lg.F * lg.H * lg.W, &sig, &ts));
    const bool any = cond && any_held(cond->hold, B, lg.F);
    CondRun cr;
    if (any) cond_run_from_hold(cond->hold, B, lg.F, &cr);
    return pipeline_run_sched(dit, vae, p, sched, any ? &cr : nullptr, sig, {latents, prompt_embeds, prompt_mask, neg_embeds, neg_mask, decode_noise, B, K, out_video, stream});
}

// ---- the step cache (include/ltxhip_stepcache.h): ltx_pipeline_call / _cond / _sched with one decision per step ----
extern "C" int ltx_pipeline_call_cached(ltx_dit* dit, ltx_vae* vae, const ltx_pipeline_params* p, const ltx_guidance_schedule* sched,
                                        const ltx_conditioning* cond, const ltx_step_cache_params* cache_params,
                                        float* latents, const float* prompt_embeds, const float* prompt_mask,
                                        const float* neg_embeds, const float* neg_mask, const float* decode_noise,
                                        int B, int K, float* out_video, ltx_stream stream,
                                        unsigned char* reused_out, float* distance_out) {
    if (!dit || !p || B < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_cached: null argument");
    if (cond && !cond->hold) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_cached: conditioning without a hold mask");
    LTX_TRY(ltx_step_cache_params_check(cache_params, "ltx_pipeline_call_cached"));
    LatentGeom lg; LTX_TRY(latent_geom(vae, p, &lg));
    if (lg.ts_ratio < 1 || lg.sp_ratio < 1 || p->num_frames < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_cached: bad geometry");
    const bool any = cond && any_held(cond->hold, B, lg.F);
    CondRun cr;
    if (any) cond_run_from_hold(cond->hold, B, lg.F, &cr);
    const PipeStepCache scd{cache_params, reused_out, distance_out};
    const PipeIO io{latents, prompt_embeds, prompt_mask, neg_embeds, neg_mask, decode_noise, B, K, out_video, stream};
    if (!sched) return pipeline_run_params(dit, vae, p, any ? &cr : nullptr, io, &scd);
    ltx_dit_config dc; LTX_TRY(ltx_dit_get_config(dit, &dc));
    LTX_TRY(guidance_schedule_check(sched, dc.num_layers));
    std::vector<float> sig; std::vector<int64_t> ts;
    LTX_TRY(ltx_pipeline_schedule(p, lg.F * lg.H * lg.W, &sig, &ts));
    return pipeline_run_sched(dit, vae, p, sched, any ? &cr : nullptr, sig, io, &scd);
}

// ---- keyframe conditioning (include/ltxhip_keyframes.h): the layout is host/cond_plan.h's, these entries hand it on ----
static int cond_plan_from_items(const ltx_cond_item* items, int n_items, int height, int width, int num_frames, int frame_rate, int ts_ratio, int sp_ratio, CondPlan* plan) {
    if (n_items > 0 && !items) LTX_FAIL(LTX_ERR_ARG, "conditioning layout: items is null with n_items " + std::to_string(n_items));
    if (sp_ratio < 1 || height < sp_ratio || width < sp_ratio) LTX_FAIL(LTX_ERR_ARG, "conditioning layout: height and width must hold one latent at least");
    std::vector<CondItemGeom> geo((size_t)(n_items > 0 ? n_items : 0));
    for (int i = 0; i < n_items; ++i) geo[(size_t)i] = {items[i].cond_frames, items[i].frame_index, items[i].strength};
    std::string err;
    if (!cond_plan_build(geo.data(), n_items, num_frames, height / sp_ratio, width / sp_ratio, ts_ratio, sp_ratio, frame_rate, plan, &err)) LTX_FAIL(LTX_ERR_ARG, err);
    return LTX_OK;
}

extern "C" int ltx_cond_layout(const ltx_cond_item* items, int n_items, int height, int width, int num_frames, int frame_rate,
                               int ts_ratio, int sp_ratio, int* E, int* G, ltx_cond_group* groups, int max_groups, float* coords) {
    CondPlan plan;
    LTX_TRY(cond_plan_from_items(items, n_items, height, width, num_frames, frame_rate, ts_ratio, sp_ratio, &plan));
    if ((groups || coords) && plan.G > max_groups)
        LTX_FAIL(LTX_ERR_ARG, "ltx_cond_layout: the layout has " + std::to_string(plan.G) + " groups, the output holds " + std::to_string(max_groups));
    if (E) *E = plan.E;
    if (G) *G = plan.G;
    if (groups) for (int g = 0; g < plan.G; ++g) groups[g] = {plan.groups[(size_t)g].item, plan.groups[(size_t)g].frame, plan.groups[(size_t)g].strength};
    if (coords) std::memcpy(coords, plan.coords.data(), plan.coords.size() * sizeof(float));
    return LTX_OK;
}

// the place table of a groups table: one entry per group an item owns (the launch leaves out strength 0)
static int cond_place_entries(const ltx_cond_item* items, int n_items, const ltx_cond_group* groups, int G, int64_t group_elems, std::vector<CondPlaceEntry>* out) {
    out->clear();
    for (int g = 0; g < G; ++g) {
        const ltx_cond_group& e = groups[g];
        if (e.item < 0) continue;
        if (e.item >= n_items || !items[e.item].tokens || e.item_frame < 0 || e.item_frame >= items[e.item].cond_frames || !(e.strength >= 0.0f && e.strength <= 1.0f))
            LTX_FAIL(LTX_ERR_ARG, "conditioning: group " + std::to_string(g) + " names item " + std::to_string(e.item) + ", frame " + std::to_string(e.item_frame) +
                                  ", strength " + std::to_string(e.strength) + ": no such frame of the items given, tokens missing, or strength outside [0, 1]");
        CondPlaceEntry pe; pe.group = g; pe.strength = e.strength;
        pe.src = items[e.item].tokens + (int64_t)e.item_frame * group_elems; pe.src_batch_stride = (int64_t)items[e.item].cond_frames * group_elems;
        out->push_back(pe);
    }
    return LTX_OK;
}

extern "C" int ltx_cond_place(float* latents, const ltx_cond_item* items, int n_items, const ltx_cond_group* groups, int G,
                              int B, int tokens_per_group, int channels, ltx_stream stream) {
    if (!latents || !groups || G < 1 || B < 1 || tokens_per_group < 1 || channels < 1 || n_items < 0 || (n_items > 0 && !items)) LTX_FAIL(LTX_ERR_ARG, "ltx_cond_place: bad argument");
    std::vector<CondPlaceEntry> place;
    LTX_TRY(cond_place_entries(items, n_items, groups, G, (int64_t)tokens_per_group * channels, &place));
    return ltx_launch_cond_place(latents, place.data(), (int)place.size(), B, G, (int64_t)tokens_per_group * channels, (hipStream_t)stream);
}

extern "C" int ltx_cond_noise(float* latents, const float* clean, const float* noise, const ltx_cond_group* groups, int G,
                              int B, int tokens_per_group, int channels, float scale, float sigma, ltx_stream stream) {
    if (!latents || !clean || !noise || !groups || G < 1 || B < 1 || tokens_per_group < 1 || channels < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_cond_noise: bad argument");
    if (!(scale > 0.0f) || !std::isfinite(scale) || !std::isfinite(sigma)) LTX_FAIL(LTX_ERR_ARG, "ltx_cond_noise: scale must be > 0 and sigma finite, got " + std::to_string(scale) + ", " + std::to_string(sigma));
    std::vector<int> hard;
    for (int g = 0; g < G; ++g) if (groups[g].item >= 0 && cond_group_is_hard(groups[g].strength)) hard.push_back(g);
    if (hard.empty()) return LTX_OK;
    const float k = (float)((double)scale * (double)sigma * (double)sigma);
    return ltx_launch_cond_noise(latents, clean, noise, hard.data(), (int)hard.size(), B, G, (int64_t)tokens_per_group * channels, k, (hipStream_t)stream);
}

extern "C" int ltx_cond_step_hold(const ltx_cond_group* groups, int G, float sigma, float timestep, unsigned char* hold_out, float* timesteps_out) {
    if (!groups || G < 1 || !hold_out) LTX_FAIL(LTX_ERR_ARG, "ltx_cond_step_hold: groups, G >= 1 and hold_out are required");
    for (int g = 0; g < G; ++g) {
        hold_out[g] = cond_group_updates(sigma, groups[g].strength) ? 0 : 1;
        if (timesteps_out) timesteps_out[g] = cond_group_timestep(timestep, groups[g].strength);
    }
    return LTX_OK;
}

extern "C" int ltx_pipeline_call_keyframes(ltx_dit* dit, ltx_vae* vae, const ltx_pipeline_params* p, const ltx_guidance_schedule* sched,
                                           const ltx_cond_item* items, int n_items, float image_cond_noise_scale, const float* cond_noise,
                                           float* latents, const float* prompt_embeds, const float* prompt_mask,
                                           const float* neg_embeds, const float* neg_mask, const float* decode_noise,
                                           int B, int K, float* out_video, ltx_stream stream) {
    if (!dit || !p || B < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_keyframes: null argument");
    if (n_items < 0 || (n_items > 0 && !items)) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_keyframes: items is null with n_items " + std::to_string(n_items));
    if (!(image_cond_noise_scale >= 0.0f) || !std::isfinite(image_cond_noise_scale)) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_keyframes: image_cond_noise_scale must be >= 0, got " + std::to_string(image_cond_noise_scale));
    if (image_cond_noise_scale > 0.0f && !cond_noise) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_keyframes: image_cond_noise_scale " + std::to_string(image_cond_noise_scale) + " needs cond_noise [steps, B, S_ext*C]");
    ltx_dit_config dc; LTX_TRY(ltx_dit_get_config(dit, &dc));
    if (sched) LTX_TRY(guidance_schedule_check(sched, dc.num_layers));
    LatentGeom lg; LTX_TRY(latent_geom(vae, p, &lg));
    CondPlan plan;
    LTX_TRY(cond_plan_from_items(items, n_items, p->height, p->width, p->num_frames, p->frame_rate, lg.ts_ratio, lg.sp_ratio, &plan));
    std::vector<float> sig; std::vector<int64_t> ts;
    LTX_TRY(ltx_pipeline_schedule(p, plan.Fl * plan.hw, &sig, &ts));
    const int N = p->num_inference_steps, G = plan.G;
    bool any = false;
    for (const CondGroup& g : plan.groups) any = any || g.item >= 0;
    CondRun cr;
    if (any) {
        for (int i = 0; i < n_items; ++i) if (!items[i].tokens) LTX_FAIL(LTX_ERR_ARG, "ltx_pipeline_call_keyframes: conditioning item " + std::to_string(i) + " has no tokens");
        std::vector<ltx_cond_group> groups((size_t)G);
        for (int g = 0; g < G; ++g) groups[(size_t)g] = {plan.groups[(size_t)g].item, plan.groups[(size_t)g].frame, plan.groups[(size_t)g].strength};
        LTX_TRY(cond_place_entries(items, n_items, groups.data(), G, (int64_t)plan.hw * dc.in_channels, &cr.place));
        cr.G = G; cr.E = plan.E; cr.hold_rows = N;
        cr.tcap.resize((size_t)B * G); cr.hold.resize((size_t)N * B * G);
        for (int b = 0; b < B; ++b)
            for (int g = 0; g < G; ++g) {
                const float sg = plan.groups[(size_t)g].strength;
                cr.tcap[(size_t)b * G + g] = 1000.0f * (1.0f - sg);
                for (int i = 0; i < N; ++i) cr.hold[((size_t)i * B + b) * G + g] = cond_group_updates(sig[i], sg) ? 0 : 1;
            }
        if (plan.E > 0) cr.coords = plan.coords.data();          // (E == 0: the grid's own, as ltx_pipeline_call_cond uses them)
        if (image_cond_noise_scale > 0.0f) {
            cr.noise_scale = image_cond_noise_scale; cr.cond_noise = cond_noise;
            for (int g = 0; g < G; ++g) if (plan.groups[(size_t)g].item >= 0 && cond_group_is_hard(plan.groups[(size_t)g].strength)) cr.hard.push_back(g);
        }
    }
    // no item owns a group: ltx_pipeline_call (or _sched) itself
    const PipeIO io{latents, prompt_embeds, prompt_mask, neg_embeds, neg_mask, decode_noise, B, K, out_video, stream};
    if (sched) return pipeline_run_sched(dit, vae, p, sched, any ? &cr : nullptr, sig, io);
    return pipeline_run_params(dit, vae, p, any ? &cr : nullptr, io);
}

// ---- warm-up: everything a first call would otherwise do inside the caller's forward --------------------------------
// Runs one DiT forward and one decode of the given geometry on scratch buffers: GEMM plans are measured (or taken from a
// loaded plan file), workspaces are sized, code objects are loaded.  Afterwards calls of this geometry enqueue work only.
extern "C" int ltx_warmup(ltx_dit* dit, ltx_vae* vae, int B, int F, int H, int W, int K, ltx_stream stream) {
    if (B < 1 || B > 8 || F < 1 || H < 1 || W < 1 || K < 1) LTX_FAIL(LTX_ERR_ARG, "ltx_warmup: bad geometry");
    hipStream_t s = (hipStream_t)stream;
    const int S = F * H * W;
    float tvals[8] = {500.f, 500.f, 500.f, 500.f, 500.f, 500.f, 500.f, 500.f};
    if (dit) {
        ltx_dit_config dc; LTX_TRY(ltx_dit_get_config(dit, &dc));
        struct Tmp { DevBuf b; ~Tmp() { b.release(); } void* p() const { return b.p; } int ensure(size_t n) { return b.ensure(n); } } x, enc, out;
        LTX_TRY(x.ensure((size_t)B * S * dc.in_channels * sizeof(float)));
        LTX_TRY(enc.ensure((size_t)B * K * dc.caption_channels * sizeof(float)));
        LTX_TRY(out.ensure((size_t)B * S * dc.out_channels * sizeof(float)));
        HIP_TRY(hipMemsetAsync(x.p(), 0, (size_t)B * S * dc.in_channels * sizeof(float), s));
        HIP_TRY(hipMemsetAsync(enc.p(), 0, (size_t)B * K * dc.caption_channels * sizeof(float), s));
        LTX_TRY(ltx_dit_forward(dit, x.p(), enc.p(), tvals, nullptr, B, S, K, F, H, W, nullptr, nullptr, nullptr, LTX_F32, out.p(), s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (vae) {
        ltx_vae_config vc; LTX_TRY(ltx_vae_get_config(vae, &vc));
        const int To = (F - 1) * vc.temporal_compression_ratio + 1, Ho = H * vc.spatial_compression_ratio, Wo = W * vc.spatial_compression_ratio;
        struct Tmp { DevBuf b; ~Tmp() { b.release(); } void* p() const { return b.p; } int ensure(size_t n) { return b.ensure(n); } } z, vid;
        LTX_TRY(z.ensure((size_t)B * S * vc.latent_channels * sizeof(float)));
        LTX_TRY(vid.ensure((size_t)B * 3 * To * Ho * Wo * sizeof(float)));
        HIP_TRY(hipMemsetAsync(z.p(), 0, (size_t)B * S * vc.latent_channels * sizeof(float), s));
        LTX_TRY(ltx_vae_decode_tokens(vae, reinterpret_cast<const float*>(z.p()), nullptr, tvals, vc.timestep_conditioning ? tvals : nullptr, B, F, H, W, nullptr, 0,
                                      reinterpret_cast<float*>(vid.p()), s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return LTX_OK;
}
