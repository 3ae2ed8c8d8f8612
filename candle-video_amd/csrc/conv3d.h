// The one description of a model's 3x3x3 channels-last conv (conv3d.hip): its weights, how they are packed and uploaded, and how a
// call becomes GEMM launches.  Used by the VAE decoder and encoder (vae.hip), the latent upsampler (upsampler.hip) and the conv ops
// (capi_ops.hip); every function takes the model dtype and pad_t (frames of left temporal replicate padding: 2 causal, 1 not).
#pragma once
#include "model_util.h"

struct ConvW {
    void* w = nullptr;   // [27][N][Cin] model dtype (N possibly permuted)
    void* b = nullptr;   // [N]
    int cin = 0, cout = 0;
    int st = 1, sh = 1, sw = 1, group = 1;   // EPI_S2D (encoder downsampler convs): strides and residual group size (vae.rs:516)
    int nsub = 8;        // depth-to-space convs: output channels per final channel, 8 = (2, 2, 2), 4 = (1, 2, 2); EPI_D2S_G also 2 = (2, 1, 1)
};
struct Dims { int B, T, H, W; int64_t vox() const { return (int64_t)B * T * H * W; } };
struct PostNorm { int on = 0; float eps = 0.f; int act = 0; int mod_stride = 0; const float* scale = nullptr; const float* shift = nullptr; };

// conv weight repack [O,I,kt,kh,kw] -> [tap][n'][I] with output-channel permutation
enum { LTX_PERM_NONE = 0, LTX_PERM_D2S = 1, LTX_PERM_UNPATCH = 2 };
int ltx_pack_conv(const void* src_dev, int sdt, void* dst, int ddt, int O, int I, int ntaps, int mode, int Cf, hipStream_t s);

// Allocate c->w / c->b (recorded in `owned`), stage w and b (found and checked by the caller), pack, synchronise, free the staging
// copy.  pack_w: the weight's pack step where it is not ltx_pack_conv's (the upsampler's per-frame Conv2d); the bias always is.
typedef int (*ConvPackFn)(const void* src_dev, int sdt, void* dst, int ddt, int cout, int cin);
int conv_upload(int dtype, std::vector<void*>& owned, const ltx_weight* w, const ltx_weight* b, int cin, int cout, int mode, int Cf, ConvW* c,
                ConvPackFn pack_w = nullptr);

// The launch-side description of the conv over all of d (operand pointers A / C / resid left to the caller), with the EPI_D2S /
// EPI_S2D / EPI_D2S_G geometry (the last one: d.T counts the two guard frames) and, with pn, the fused output norm
GemmArgs conv_args(const ConvW& cw, const Dims& d, int pad_t, int epi, const PostNorm* pn = nullptr);
int conv_chunk(int dtype, const ConvW& cw, const Dims& d);      // samples per launch
bool fuse_norm2(int dtype, int pad_t, const ConvW& cw, const Dims& d_all, int ch);
int conv3d(int dtype, int pad_t, const ConvW& cw, const void* x, void* y, const Dims& d, int epi, const void* resid, int post, hipStream_t s, const PostNorm* pn = nullptr);
// The ops' form: w / bias in the checkpoint layout (dtype wdt) are packed into two temporaries for this one call (cw carries the
// shape fields), and s is synchronised before they are released
int conv3d_unpacked(int dtype, int pad_t, ConvW cw, const void* w, const void* bias, int wdt, int mode, const void* x, void* y, const Dims& d, int epi,
                    const void* resid, int post, hipStream_t s, const PostNorm* pn = nullptr);
