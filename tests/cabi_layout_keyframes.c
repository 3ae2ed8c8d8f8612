/* ABI layout guard of include/ltxhip_keyframes.h, a sibling of cabi_layout.c: compiled as C99 by tests/test_keyframes_ref_cpu.py,
 * prints sizeof / alignment / offsetof of the two structs as JSON; the test compares them with the ctypes mirrors
 * (candle-video_amd/ltxhip/__init__.py) and the KEYFRAMES_LAYOUT_* constants of rust/ltxhip-sys/src/lib.rs. */
#include <stddef.h>
#include <stdio.h>
#include "ltxhip_keyframes.h"

#define ALIGN_OF(T) offsetof(struct { char c; T x; }, x)

int main(void) {
    printf("{\"ltx_cond_item\": {\"size\": %zu, \"align\": %zu, \"fields\": {\"tokens\": %zu, \"cond_frames\": %zu, \"frame_index\": %zu, \"strength\": %zu}}, ",
           sizeof(ltx_cond_item), ALIGN_OF(ltx_cond_item), offsetof(ltx_cond_item, tokens), offsetof(ltx_cond_item, cond_frames),
           offsetof(ltx_cond_item, frame_index), offsetof(ltx_cond_item, strength));
    printf("\"ltx_cond_group\": {\"size\": %zu, \"align\": %zu, \"fields\": {\"item\": %zu, \"item_frame\": %zu, \"strength\": %zu}}}\n",
           sizeof(ltx_cond_group), ALIGN_OF(ltx_cond_group), offsetof(ltx_cond_group, item), offsetof(ltx_cond_group, item_frame),
           offsetof(ltx_cond_group, strength));
    return 0;
}
