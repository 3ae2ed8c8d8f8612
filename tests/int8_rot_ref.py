"""Torch restatement of include/ltxhip_int8_rot.h beside int8_ref.py: the staged Walsh-Hadamard transform (every output of a stage is
ONE rounded add or subtract of two of the stage's inputs, so an f32 input gives the engine's bits), the rotated quantise, and the
oracle's block linears in W8A8 with the named kinds rotated.

Error bar of the norm + rotate + quantise pass against the f64 value H n64 (u = 2^-24).  The engine rotates its f32 n, |n - n64| <=
gamma_n elementwise (int8_ref.rownorm64); an output of H is a signed sum of ALL D inputs, so that error reaches it as at most G = sum_e
gamma_n[e].  The rotation's own roundings: a stage's output v carries at most u |v| and reaches a final output with coefficient +-1;
over the log2 D stages the bar takes R = log2(D) u max|H n64| per row.  Quantising the f32 H n is int8_ref's:
  |q s - H n64| <= s / 2 + G + R + 4 u amax   and   |s - amax64 / 127| <= (G + R + 2 u amax64) / 127,   amax64 = max|H n64|."""
import contextlib
import math

import torch

import int8_ref as R
import ltx_oracle as O


def fwht(x):
    D = x.shape[-1]
    assert D & (D - 1) == 0
    lead = x.shape[:-1]
    h = 1
    while h < D:
        v = x.reshape(*lead, D // (2 * h), 2, h)
        a, b = v[..., 0, :], v[..., 1, :]
        x = torch.stack((a + b, a - b), dim=-2).reshape(*lead, D)
        h *= 2
    return x


def hadamard_quant_rows(x, out_scale=1.0):
    """x [..., D] -> (q int8 of H x, scale f32 = (amax / 127) * out_scale)"""
    q, s = R.quant_rows(fwht(x.float()))
    return q, s * torch.tensor(out_scale, dtype=torch.float32, device=s.device)


def rot_bars(n64, gamma_n):
    """-> (H n64, G + R per row, amax64 per row)"""
    Hn = fwht(n64)
    amax = Hn.abs().amax(-1)
    return Hn, gamma_n.sum(-1) + math.log2(n64.shape[-1]) * R.U * amax, amax


def outlier_rows(rows, K, seed, gain=60.0, count=4):
    """Gaussian rows with `count` random columns scaled by `gain` (the few large channels a per-row scale cannot afford)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, K, generator=g)
    x[:, torch.randperm(K, generator=g)[:count]] *= gain
    return x


def linear_w8a8_rot(x, w, b, round_input):
    """int8_ref.linear_w8a8 with both operands rotated along K and the weight scales times 1 / K"""
    xin = x.bfloat16().float() if round_input else x.float()
    lead = xin.shape[:-1]
    K = xin.shape[-1]
    qa, sa = hadamard_quant_rows(xin.reshape(-1, K))
    qw, sw = hadamard_quant_rows(w.bfloat16().float(), 1.0 / K)
    y = R.acc_i8(qa, qw) * sa.double()[:, None] * sw.double()[None, :]
    if b is not None:
        y = y + b.double()[None, :]
    return y.to(x.dtype).reshape(*lead, w.shape[0])


@contextlib.contextmanager
def w8a8_rot(weights, mask=R.I8_ALL, rot=R.I8_ALL):
    """int8_ref.w8a8 with the kinds of `rot` rotated"""
    table = {}
    l = 0
    while f"transformer_blocks.{l}.attn1.to_q.weight" in weights:
        for name, bit, rnd in R._KINDS:
            if mask & bit:
                table[id(weights[f"transformer_blocks.{l}.{name}.weight"])] = (rnd, bool(rot & bit))
        l += 1
    plain = O.linear

    def linear(x, w, b):
        hit = table.get(id(w))
        if hit is None:
            return plain(x, w, b)
        return (linear_w8a8_rot if hit[1] else R.linear_w8a8)(x, w, b, hit[0])

    O.linear = linear
    try:
        yield
    finally:
        O.linear = plain
