/* ABI guard of include/ltxhip_stg.h, a sibling of cabi_layout_cond.c: compiled as C99 by tests/test_stg_cabi_cpu.py (which proves
 * the header is plain C), prints the size of the enum and the value of every enumerator as JSON; the test compares them with the
 * constants of candle-video_amd/ltxhip/__init__.py and of rust/ltxhip-sys/src/lib.rs. */
#include <stdio.h>
#include "ltxhip_stg.h"

int main(void) {
    printf("{\"ltx_stg_mode\": {\"size\": %zu, \"values\": {\"LTX_STG_TRANSFORMER_BLOCK\": %d, \"LTX_STG_ATTENTION_SKIP\": %d, \"LTX_STG_ATTENTION_VALUES\": %d}}}\n",
           sizeof(ltx_stg_mode), (int)LTX_STG_TRANSFORMER_BLOCK, (int)LTX_STG_ATTENTION_SKIP, (int)LTX_STG_ATTENTION_VALUES);
    return 0;
}
