/* ABI layout guard of include/ltxhip_upsampler.h, a sibling of cabi_layout_cond.c: compiled as C99 by
 * tests/test_latent_upsampler_ref_cpu.py, prints sizeof / alignment / offsetof of the struct as JSON; the test compares them with the
 * ctypes mirror (candle-video_amd/ltxhip/__init__.py) and the UPSAMPLER_LAYOUT_* constant of rust/ltxhip-sys/src/lib.rs. */
#include <stddef.h>
#include <stdio.h>
#include "ltxhip_upsampler.h"

#define ALIGN_OF(T) offsetof(struct { char c; T x; }, x)

int main(void) {
    printf("{\"ltx_upsampler_config\": {\"size\": %zu, \"align\": %zu, \"fields\": {\"in_channels\": %zu, \"mid_channels\": %zu, \"num_blocks_per_stage\": %zu}}}\n",
           sizeof(ltx_upsampler_config), ALIGN_OF(ltx_upsampler_config), offsetof(ltx_upsampler_config, in_channels),
           offsetof(ltx_upsampler_config, mid_channels), offsetof(ltx_upsampler_config, num_blocks_per_stage));
    return 0;
}
