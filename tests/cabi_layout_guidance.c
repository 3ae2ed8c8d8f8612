/* ABI guard of include/ltxhip_guidance.h, a sibling of cabi_layout_stg.c: compiled as C99 by tests/test_guidance_sched_cabi_cpu.py
 * (which proves the header is plain C), prints the layout of ltx_guidance_schedule and the values of ltx_rescale_form as JSON; the
 * test compares them with the mirrors of candle-video_amd/ltxhip/__init__.py and of rust/ltxhip-sys/src/lib.rs. */
#include <stddef.h>
#include <stdio.h>
#include "ltxhip_guidance.h"

#define FIELD(f) printf("\"%s\": %zu%s", #f, offsetof(ltx_guidance_schedule, f), last ? "" : ", ")

int main(void) {
    int last = 0;
    struct probe { char c; ltx_guidance_schedule s; };
    printf("{\"ltx_guidance_schedule\": {\"size\": %zu, \"align\": %zu, \"fields\": {", sizeof(ltx_guidance_schedule), offsetof(struct probe, s));
    FIELD(n); FIELD(guidance_scale); FIELD(stg_scale); FIELD(rescale); FIELD(skip_blocks); FIELD(skip_offsets); FIELD(guidance_timesteps); FIELD(cfg_star);
    last = 1; FIELD(rescale_form);
    printf("}}, \"ltx_rescale_form\": {\"size\": %zu, \"values\": {\"LTX_RESCALE_CFG\": %d, \"LTX_RESCALE_MIX\": %d}}}\n",
           sizeof(ltx_rescale_form), (int)LTX_RESCALE_CFG, (int)LTX_RESCALE_MIX);
    return 0;
}
