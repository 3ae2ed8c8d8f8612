"""Torch restatement of include/ltxhip_sparse_attn.h: block maps packed to / expanded from their uint32 words (held as int32), f64
softmax over the map expanded to elements, and a context manager that runs the oracle's attn1 through it.  q is the prescaled query
q' = bf16(q * scale * log2(e)); scores are in log2 units.  Tensors are [B, S, heads * hd]."""
import contextlib
import math

import torch

import ltx_oracle as O
from int8_attn_ref import LOG2E, _heads


def pack(bits):
    """bool [..., NQB, NKT] -> int32 [..., NQB, ceil(NKT / 32)]: key tile kt is bit kt & 31 of word kt >> 5"""
    nw = (bits.shape[-1] + 31) // 32
    b = torch.zeros(*bits.shape[:-1], nw * 32, dtype=torch.int64)
    b[..., :bits.shape[-1]] = bits
    w = (b.reshape(*bits.shape[:-1], nw, 32) << torch.arange(32)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def expand(map, Sq, Sk):
    """int32 [..., NQB, NW] -> bool [..., Sq, Sk]; bits at or above ceil(Sk / 64) drop out"""
    bits = ((map.cpu().to(torch.int64)[..., None] >> torch.arange(32)) & 1).bool().flatten(-2)[..., :(Sk + 63) // 64]
    return bits.repeat_interleave(128, -2)[..., :Sq, :].repeat_interleave(64, -1)[..., :Sk]


def attention64(q, k, v, map, heads):
    """f64 attention over the attended keys alone; a query with none gets zeros.  map [NQB, NW] or [heads, NQB, NW]"""
    keep = expand(map, q.shape[1], k.shape[1]).to(q.device)
    s = (_heads(q, heads) @ _heads(k, heads).transpose(-1, -2)).masked_fill(~keep, float("-inf"))
    p = torch.nan_to_num(torch.softmax(s * math.log(2.0), -1), nan=0.0)      # a row of -inf alone: no key, zeros
    return (p @ _heads(v, heads)).transpose(1, 2).reshape(q.shape)


@contextlib.contextmanager
def sparse_attention(map, block_flags=None):
    """inside the context ltx_oracle.attention computes attn1 of every block (or of the blocks with a truthy flag) by attention64 on the
    tensors the engine stores in bf16: q' = bf16(q * scale * log2(e)), k, v"""
    plain = O.attention

    def attention(p, prefix, heads, hidden, enc, mask_bias, rope):
        l = int(prefix.split(".")[-3]) if prefix.endswith("attn1.") else -1
        if l < 0 or (block_flags is not None and not block_flags[l]):
            return plain(p, prefix, heads, hidden, enc, mask_bias, rope)
        q, k, v = [O.linear(hidden, p[prefix + f"to_{n}.weight"], p.get(prefix + f"to_{n}.bias")) for n in "qkv"]
        q = O.apply_rotary_emb(O.rms_norm(q, p[prefix + "norm_q.weight"], 1e-5), *rope)
        k = O.apply_rotary_emb(O.rms_norm(k, p[prefix + "norm_k.weight"], 1e-5), *rope)
        qp = (q.float() * ((q.shape[-1] // heads) ** -0.5 * LOG2E)).bfloat16()
        out = attention64(qp, k.bfloat16(), v.bfloat16(), map, heads).to(q.dtype)
        return O.linear(out, p[prefix + "to_out.0.weight"], p.get(prefix + "to_out.0.bias"))

    O.attention = attention
    try:
        yield
    finally:
        O.attention = plain
