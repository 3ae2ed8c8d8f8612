"""Torch restatement of include/ltxhip_int8_attn.h: the mean of K, the two quantisations (f32, the engine's operations: bit-equal
given the same mean), attention in f64 on the quantised operands, and a context manager that runs the oracle's attn1 through them.
q is the prescaled query q' = bf16(q * scale * log2(e)); scores are in log2 units.  Tensors are [B, S, heads * hd]."""
import contextlib
import math

import torch

import ltx_oracle as O
from int8_ref import quant_rows

LOG2E = 1.4426950408889634


def kmean64(k):
    return k.double().mean(1)


def quant_qk(q, k, mean, heads):
    """-> q8 int8 [B, Sq, D], qs f32 [B, heads, Sq], k8 int8 [B, Sk, D], ks f32 [B, heads, ceil(Sk / 64)]; mean f32 [B, D]"""
    B, Sq, D = q.shape
    Sk, hd = k.shape[1], D // heads
    q8, qs = quant_rows(q.float().reshape(B, Sq, heads, hd))
    kc = k.float() - mean.float()[:, None, :]
    nkb = (Sk + 63) // 64
    kp = torch.cat([kc, kc.new_zeros(B, nkb * 64 - Sk, D)], 1).reshape(B, nkb, 64, heads, hd)      # zero rows leave the block's amax alone
    amax = kp.abs().amax(dim=(2, 4), keepdim=True)
    c127 = torch.tensor(127.0, dtype=torch.float32, device=k.device)
    inv = torch.where(amax > 0, c127 / amax, torch.zeros_like(amax))
    k8 = torch.clamp(torch.round(kp * inv), -127, 127).to(torch.int8).reshape(B, nkb * 64, D)[:, :Sk]
    return q8.reshape(B, Sq, D), qs.permute(0, 2, 1).contiguous(), k8.contiguous(), (amax / c127).reshape(B, nkb, heads).permute(0, 2, 1).contiguous()


def _heads(x, heads):
    B, S, D = x.shape
    return x.reshape(B, S, heads, D // heads).transpose(1, 2).double()


def softmax2_v(s, v, heads):
    """softmax over keys of ln2 * s [B, heads, Sq, Sk] (f64), times v -> [B, Sq, D] f64"""
    p = torch.softmax(s * math.log(2.0), -1)
    return (p @ _heads(v, heads)).transpose(1, 2).reshape(v.shape[0], s.shape[2], v.shape[2])


def attention64(q8, qs, k8, ks, v, heads):
    """f64 attention on the quantised operands: s = acc * qs[i] * ks[j / 64]"""
    acc = _heads(q8, heads) @ _heads(k8, heads).transpose(-1, -2)
    sk = ks.double().repeat_interleave(64, -1)[..., :k8.shape[1]]
    return softmax2_v(acc * qs.double()[..., None] * sk[:, :, None, :], v, heads)


def exact64(q, k, v, heads):
    """unquantised attention of the same bf16 inputs"""
    return softmax2_v(_heads(q, heads) @ _heads(k, heads).transpose(-1, -2), v, heads)


def chain64(q, k, v, heads, smooth=True):
    """the whole definition on the CPU; smooth=False leaves the mean of K in (what the header rules out)"""
    mean = kmean64(k).float() if smooth else torch.zeros(k.shape[0], k.shape[2])
    return attention64(*quant_qk(q, k, mean.to(k.device), heads), v, heads)


@contextlib.contextmanager
def int8_attention(block_flags=None):
    """inside the context ltx_oracle.attention computes attn1 of every block (or of the blocks with a truthy flag) by chain64 on the
    tensors the engine stores in bf16: q' = bf16(q * scale * log2(e)), k, v.  Linears go through O.linear, so int8_ref.w8a8 composes."""
    plain = O.attention

    def attention(p, prefix, heads, hidden, enc, mask_bias, rope):
        l = int(prefix.split(".")[-3]) if prefix.endswith("attn1.") else -1
        if l < 0 or (block_flags is not None and not block_flags[l]):
            return plain(p, prefix, heads, hidden, enc, mask_bias, rope)
        q, k, v = [O.linear(hidden, p[prefix + f"to_{n}.weight"], p.get(prefix + f"to_{n}.bias")) for n in "qkv"]
        q = O.apply_rotary_emb(O.rms_norm(q, p[prefix + "norm_q.weight"], 1e-5), *rope)
        k = O.apply_rotary_emb(O.rms_norm(k, p[prefix + "norm_k.weight"], 1e-5), *rope)
        qp = (q.float() * ((q.shape[-1] // heads) ** -0.5 * LOG2E)).bfloat16()
        out = chain64(qp, k.bfloat16(), v.bfloat16(), heads).to(q.dtype)
        return O.linear(out, p[prefix + "to_out.0.weight"], p.get(prefix + "to_out.0.bias"))

    O.attention = attention
    try:
        yield
    finally:
        O.attention = plain
