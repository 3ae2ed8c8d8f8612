/* ABI layout guard of include/ltxhip_cond.h, the sibling of cabi_layout.c: compiled as C99 by tests/test_dit_frames_ref_cpu.py,
 * prints sizeof / alignment / offsetof of the struct as JSON; the test compares them with the ctypes mirror
 * (candle-video_amd/ltxhip/__init__.py) and the COND_LAYOUT_* constant of rust/ltxhip-sys/src/lib.rs. */
#include <stddef.h>
#include <stdio.h>
#include "ltxhip_cond.h"

#define ALIGN_OF(T) offsetof(struct { char c; T x; }, x)

int main(void) {
    printf("{\"ltx_conditioning\": {\"size\": %zu, \"align\": %zu, \"fields\": {\"hold\": %zu}}}\n",
           sizeof(ltx_conditioning), ALIGN_OF(ltx_conditioning), offsetof(ltx_conditioning, hold));
    return 0;
}
