// Host sanitizer driver of the step cache's policy (candle-video_amd/host/step_cache.h, header only, built with ASan + UBSan).
// stdin, numbers as the bit patterns of their types (no decimal round trip):
//   trace <thresh u32> <c0 .. c4 u32> <have_prev 0|1> <acc u64> <n_pattern> <pattern bytes ...> <n_steps_lines>
//   then per line:  <i> <N> <num u64> <den u64> <rows_valid 0|1>
//   check <thresh u32> <c0 .. c4 u32> <n_pattern> <pattern bytes ...> <null_pattern 0|1>          the parameter check alone
// stdout: per step line "<reuse> <acc u64> <have_prev>"; per check line "ok" or the message.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../candle-video_amd/host/step_cache.h"

static float f32_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static double f64_of(uint64_t u) { double d; memcpy(&d, &u, 8); return d; }
static uint64_t bits_of(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }

static bool read_policy(StepCachePolicy* p) {
    uint32_t u[6];
    for (uint32_t& v : u) if (scanf("%" SCNu32, &v) != 1) return false;
    p->thresh = f32_of(u[0]);
    for (int k = 0; k < 5; ++k) p->coeff[k] = f32_of(u[k + 1]);
    return true;
}
static bool read_pattern(std::vector<unsigned char>* pat, int* n) {
    if (scanf("%d", n) != 1) return false;
    pat->assign((size_t)(*n > 0 ? *n : 0), 0);
    for (unsigned char& b : *pat) { int v; if (scanf("%d", &v) != 1) return false; b = (unsigned char)v; }
    return true;
}

int main() {
    char word[16];
    while (scanf("%15s", word) == 1) {
        StepCachePolicy p;
        std::vector<unsigned char> pat;      // sized exactly: a read past n_pattern is a sanitizer finding
        if (!strcmp(word, "check")) {
            int n = 0, null_pattern = 0;
            if (!read_policy(&p) || !read_pattern(&pat, &n) || scanf("%d", &null_pattern) != 1) return 2;
            p.pattern = null_pattern || pat.empty() ? nullptr : pat.data(); p.n_pattern = n;
            const char* why = step_cache_policy_error(p);
            printf("%s\n", why ? why : "ok");
            continue;
        }
        if (strcmp(word, "trace")) return 2;
        StepCacheState st;
        int have = 0, n = 0, lines = 0;
        uint64_t acc = 0;
        if (!read_policy(&p) || scanf("%d %" SCNu64, &have, &acc) != 2 || !read_pattern(&pat, &n) || scanf("%d", &lines) != 1) return 2;
        st.have_prev = have != 0; st.acc = f64_of(acc);
        p.pattern = pat.empty() ? nullptr : pat.data(); p.n_pattern = n;
        for (int l = 0; l < lines; ++l) {
            int i = 0, N = 0, valid = 0;
            uint64_t num = 0, den = 0;
            if (scanf("%d %d %" SCNu64 " %" SCNu64 " %d", &i, &N, &num, &den, &valid) != 5) return 2;
            const int reuse = step_cache_decide(&st, p, i, N, f64_of(num), f64_of(den), valid != 0);
            printf("%d %" PRIu64 " %d\n", reuse, bits_of(st.acc), st.have_prev ? 1 : 0);
        }
    }
    return 0;
}
