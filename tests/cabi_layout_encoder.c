/* ABI layout guard of include/ltxhip_encoder.h, the sibling of cabi_layout.c: compiled as C99 by
 * tests/test_vae_encoder_ref_cpu.py, prints sizeof / alignment / offsetof of the structs as JSON; the test compares them with the
 * ctypes mirrors (candle-video_amd/ltxhip/__init__.py) and the ENCODER_LAYOUT_* constants of rust/ltxhip-sys/src/lib.rs. */
#include <stddef.h>
#include <stdio.h>
#include "ltxhip_encoder.h"
#include "ltxhip_weights.h"

#define ALIGN_OF(T) offsetof(struct { char c; T x; }, x)
#define BEGIN(T) printf("%s\"%s\": {\"size\": %zu, \"align\": %zu, \"fields\": {", first ? "" : ", ", #T, sizeof(T), ALIGN_OF(T)); first = 0; ff = 1
#define F(T, f) printf("%s\"%s\": %zu", ff ? "" : ", ", #f, offsetof(T, f)); ff = 0
#define END() printf("}}")

int main(void) {
    int first = 1, ff = 1;
    printf("{");
    BEGIN(ltx_vae_encoder_config); F(ltx_vae_encoder_config, in_channels); F(ltx_vae_encoder_config, latent_channels); F(ltx_vae_encoder_config, n_blocks);
        F(ltx_vae_encoder_config, block_out_channels); F(ltx_vae_encoder_config, layers_per_block); F(ltx_vae_encoder_config, spatiotemporal_scaling);
        F(ltx_vae_encoder_config, downsample_types); F(ltx_vae_encoder_config, patch_size); F(ltx_vae_encoder_config, patch_size_t); F(ltx_vae_encoder_config, is_causal);
        F(ltx_vae_encoder_config, spatial_compression_ratio); F(ltx_vae_encoder_config, temporal_compression_ratio); END();
    BEGIN(ltx_encode_tiling); F(ltx_encode_tiling, use_framewise_encoding); END();
    printf("}\n");
    return 0;
}
