/* ABI layout guard of include/ltxhip_upsampler_st.h, a sibling of cabi_layout_upsampler.c: compiled as C99 by
 * tests/test_latent_upsampler_st_ref_cpu.py, prints sizeof / alignment / offsetof of the struct as JSON; the test compares them with
 * the ctypes mirror (candle-video_amd/ltxhip/__init__.py) and the UPSAMPLER_ST_LAYOUT_* constant of rust/ltxhip-sys/src/lib.rs. */
#include <stddef.h>
#include <stdio.h>
#include "ltxhip_upsampler_st.h"

#define ALIGN_OF(T) offsetof(struct { char c; T x; }, x)

int main(void) {
    printf("{\"ltx_upsampler_st_config\": {\"size\": %zu, \"align\": %zu, \"fields\": {\"in_channels\": %zu, \"mid_channels\": %zu, "
           "\"num_blocks_per_stage\": %zu, \"spatial_upsample\": %zu, \"temporal_upsample\": %zu}}}\n",
           sizeof(ltx_upsampler_st_config), ALIGN_OF(ltx_upsampler_st_config), offsetof(ltx_upsampler_st_config, in_channels),
           offsetof(ltx_upsampler_st_config, mid_channels), offsetof(ltx_upsampler_st_config, num_blocks_per_stage),
           offsetof(ltx_upsampler_st_config, spatial_upsample), offsetof(ltx_upsampler_st_config, temporal_upsample));
    return 0;
}
