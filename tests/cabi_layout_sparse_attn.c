/* ABI guard of include/ltxhip_sparse_attn.h, a sibling of cabi_layout_stg.c: compiled as C99 by tests/test_sparse_map_cpu.py (which
 * proves the header is plain C) and linked against the library; prints the sizes of the types that cross the boundary and what the
 * three host functions give for a 3 x 8 x 13 grid as JSON; the test compares them with the ctypes mirror's answers. */
#include <stdio.h>
#include "ltxhip_sparse_attn.h"

int main(void) {
    uint32_t map[3];
    const size_t words = ltx_sparse_map_words(3 * 8 * 13);
    const int rc = words == 3 ? ltx_sparse_window_map(3, 8, 13, 0, 0, 0, 0, map, words) : -1;
    printf("{\"sizes\": {\"word\": %zu, \"size_t\": %zu, \"S\": %zu}, \"words\": %zu, \"rc\": %d, \"map\": [%u, %u, %u], \"density\": %.17g}\n",
           sizeof(map[0]), sizeof(size_t), sizeof(int64_t), words, rc, (unsigned)map[0], (unsigned)map[1], (unsigned)map[2],
           ltx_sparse_map_density(map, 3 * 8 * 13));
    return 0;
}
