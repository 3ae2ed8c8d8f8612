/* ABI guard of include/ltxhip_stepcache.h, a sibling of cabi_layout_guidance.c: compiled as C99 by tests/test_step_cache_cabi_cpu.py
 * (which proves the header is plain C), prints the layout of ltx_step_cache_params as JSON; the test compares it with the mirrors of
 * candle-video_amd/ltxhip/__init__.py and of rust/ltxhip-sys/src/lib.rs. */
#include <stddef.h>
#include <stdio.h>
#include "ltxhip_stepcache.h"

#define FIELD(f) printf("\"%s\": %zu%s", #f, offsetof(ltx_step_cache_params, f), last ? "" : ", ")

int main(void) {
    int last = 0;
    struct probe { char c; ltx_step_cache_params s; };
    printf("{\"ltx_step_cache_params\": {\"size\": %zu, \"align\": %zu, \"coeff_bytes\": %zu, \"fields\": {", sizeof(ltx_step_cache_params),
           offsetof(struct probe, s), sizeof(((ltx_step_cache_params*)0)->coeff));
    FIELD(rel_l1_thresh); FIELD(coeff); FIELD(pattern);
    last = 1; FIELD(n_pattern);
    printf("}}}\n");
    return 0;
}
