"""Parity reference of the LoRA merge (include/ltxhip_lora.h).  The reference project has no LoRA support, so like
tests/dit_frames_ref.py this restates the published rule:

    W_eff = W0 + sum_i c_i * (B_i A_i),   c_i = scale_i * alpha_i / r_i   (alpha absent: c_i = scale_i)

`merge` evaluates it in f64 on the values ROUNDED TO THE MODEL DTYPE (what the engine stores) and returns the error bars that
follow from the engine's arithmetic, with no measured constant:

    mag   = |W0| + sum_i |c_i| * (|B_i| |A_i|)
    gamma = (R_pad + 4) * 2^-24 * mag,   R_pad = the ranks, each rounded up to 32, summed
            (exact products, at most R_pad f32 accumulations, one fma per adapter, one final add: (R_pad + 4) roundings of 2^-24)
    f32  mode: |out - E| <= gamma
    bf16 mode: |out - E| <= 1/2 max(ulp_bf16(E), ulp_bf16(out)) + gamma          (+ the one rounding of the stored result)

Everything here is device-agnostic torch: the GPU tests evaluate it where their tensors live."""
import math

import torch

TARGETS = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v", "attn2.to_out.0",
           "ff.net.0.proj", "ff.net.2")


def coef(scale, alpha, r):
    """c_i as the engine forms it: f32(scale) * (f32(alpha) / f32(r)); alpha None = factor 1"""
    s = torch.tensor(float(scale), dtype=torch.float32)
    if alpha is None:
        return float(s)
    return float(s * (torch.tensor(float(alpha), dtype=torch.float32) / torch.tensor(float(r), dtype=torch.float32)))


def rank_pad(r):
    return (r + 31) // 32 * 32


def merge(W0, adapters, dtype=torch.bfloat16):
    """adapters: [(A [r, in], B [out, r], c), ...] -> (E f64, gamma f64)"""
    W = W0.to(dtype).double()
    E = W.clone(); mag = W.abs()
    R = 0
    for A, B, c in adapters:
        A = A.to(dtype).double(); B = B.to(dtype).double()
        E += float(c) * (B @ A)
        mag += abs(float(c)) * (B.abs() @ A.abs())
        R += rank_pad(A.shape[0])
    return E, (R + 4) * 2.0 ** -24 * mag


def ulp_bf16(x):
    """spacing of bf16 at |x| (f64 in, f64 out); 0 at 0"""
    _, ex = torch.frexp(x.double().abs())                # |x| = m 2^ex, m in [0.5, 1): the binade starts at 2^(ex - 1), 8 significant bits
    u = torch.ldexp(torch.ones_like(x, dtype=torch.float64), ex - 8)
    return torch.where(x == 0, torch.zeros_like(u), u)


def bar(out, E, gamma, dtype):
    if dtype == torch.float32:
        return gamma
    return 0.5 * torch.maximum(ulp_bf16(E), ulp_bf16(out.double())) + gamma


def worst(out, E, gamma, dtype):
    """(number of elements beyond the bar, largest error / bar)"""
    err = (out.double() - E).abs()
    b = bar(out, E, gamma, dtype)
    ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return int((err > b).sum()), float(ratio.max())


def merge_f32acc(W0, adapters, dtype=torch.bfloat16):
    """the engine's order restated with f32 accumulation: acc_i = B_i A_i in f32, total = fma(c_i, acc_i, total), out = round(W0 + total)"""
    W = W0.to(dtype).float()
    total = torch.zeros_like(W)
    for A, B, c in adapters:
        acc = B.to(dtype).float() @ A.to(dtype).float()
        total = torch.addcmul(total, acc, torch.tensor(float(c), dtype=torch.float32, device=W.device))
    return (W + total).to(dtype)


def lora_delta_forward(x, W0, A, B, c):
    """the definition of LoRA on one linear: y = x W0^T + c * ((x A^T) B^T)"""
    import torch.nn.functional as F
    return F.linear(x, W0) + c * F.linear(F.linear(x, A), B)


def fused_rows(which, D):
    """(name of the fused weight or None, first row) of target `which` inside the engine's fused q|k|v (attn1) and k|v (attn2) weights"""
    return {0: ("qkv1", 0), 1: ("qkv1", D), 2: ("qkv1", 2 * D), 5: ("kv2", 0), 6: ("kv2", D)}.get(which, (None, 0))


def synth_adapter(cfg_dims, targets, rank, seed, alpha=None, dtype=torch.float32):
    """tensors of one adapter: targets = [(block, which), ...]; A ~ N(0, 1/r), B ~ 0.05 N(0, 1); names in the lora_A / lora_B spelling"""
    D, cross = cfg_dims
    g = torch.Generator().manual_seed(seed)
    out = {}
    for block, which in targets:
        o = 4 * D if which == 8 else D
        i = 4 * D if which == 9 else cross if which in (5, 6) else D
        name = f"transformer_blocks.{block}.{TARGETS[which]}"
        out[name + ".lora_A.weight"] = (torch.randn(rank, i, generator=g) / math.sqrt(rank)).to(dtype)
        out[name + ".lora_B.weight"] = (0.05 * torch.randn(o, rank, generator=g)).to(dtype)
        if alpha is not None:
            out[name + ".alpha"] = torch.tensor(float(alpha))
    return out


def merged_weights(w, adapters, dtype):
    """checkpoint dict `w` (Diffusers names) with every targeted linear replaced by merge()'s E (f64 -> f32); adapters:
    [(tensors, scale), ...] with tensors in the lora_A / lora_B (+ .alpha) spelling.  Returns (weights, {name: (E, gamma)})."""
    per = {}
    for tensors, scale in adapters:
        for k in tensors:
            if k.endswith(".lora_A.weight"):
                mod = k[: -len(".lora_A.weight")]
                A, B = tensors[k], tensors[mod + ".lora_B.weight"]
                al = tensors.get(mod + ".alpha")
                per.setdefault(mod, []).append((A, B, coef(scale, None if al is None else float(al), A.shape[0])))
    out = dict(w); bars = {}
    for mod, ads in per.items():
        E, gamma = merge(w[mod + ".weight"], ads, dtype)
        out[mod + ".weight"] = E.float()
        bars[mod] = (E, gamma)
    return out, bars
