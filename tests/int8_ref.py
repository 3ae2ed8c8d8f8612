"""Torch restatement of include/ltxhip_int8.h: symmetric int8 rows, the exact integer product, the norm + quantise pass, and a
context manager that runs the oracle's block linears in W8A8.  Device-agnostic torch: the GPU tests evaluate it where their tensors live.

    quant_rows(x)        amax = max|x|, inv = 127 / amax (f32, IEEE division; 0 for a zero row), q = clamp(rint(x * inv), -127, 127)
                         (round half to even), scale = amax / 127 (f32)
    gemm_i8(...)         acc = qa qw^T as an f64 product of the integers (exact: |acc| <= 127^2 K < 2^53), then IN F64 the value the
                         engine rounds: E = epi(acc * sa[m] * sw[n] + bias[n])

Error bars, from the arithmetic alone (u = 2^-24, one f32 rounding):
  the engine forms v = (f32(acc) * sa) * sw + bias in f32: the int32 -> f32 conversion, two products and the sum are four roundings,
      gamma_v = u * (3 |acc sa sw| + |v|)
  epi 0 (bias): gamma = gamma_v.   epi 3 (v + resid): gamma = gamma_v + u |E|.   epi 2 (fma(gate, v, resid)): gamma = |gate| gamma_v + u |E|.
  epi 1 (GELU-tanh as x / (1 + exp2(x (A + B x^2)))): the derivative is at most 1.13, the exponent a = x (A + B x^2) carries three
      roundings that the exponential turns into a relative error of 3 u |a| ln 2, exp2 and the reciprocal are 1-ulp hardware
      approximations and three more operations follow:  gamma = 1.13 gamma_v + u (8 + 3 |a|) |E|
  the stored result is one bf16 rounding of the f32 value:  |out - E| <= 1/2 max(ulp_bf16(E), ulp_bf16(out)) + gamma     (lora_ref.bar)
  norm + quantise (rownorm_gamma): the sum of squares is at most D / 64 + 7 sequential f32 additions per lane and six butterfly steps;
      times 1 / D, plus eps, square root (which halves the relative error), reciprocal: r carries (D / 128 + 7) u.  t = h r (1 + scale)
      adds three roundings, n = t + shift one more:  gamma_n = u ((D / 128 + 10) |t| + |n|).  Quantising the f32 n: inv, the product and
      scale are one rounding each of values bounded by amax:  |q s - n64| <= s / 2 + gamma_n + 4 u amax
      and  |s - amax64 / 127| <= (max gamma_n + 2 u amax64) / 127."""
import contextlib
import math

import torch

import ltx_oracle as O
from lora_ref import ulp_bf16

I8_QKV, I8_TO_OUT, I8_FF1, I8_FF2, I8_ALL = 1, 2, 4, 8, 15
U = 2.0 ** -24
GELU_A = -2.0 * 0.7978845608028654 * 1.4426950408889634
GELU_B = GELU_A * 0.044715


def quant_rows(x):
    """x [..., D] (any float dtype; evaluated in f32) -> (q int8 [..., D], scale f32 [...])"""
    xf = x.float()
    amax = xf.abs().amax(-1, keepdim=True)
    c127 = torch.tensor(127.0, dtype=torch.float32, device=xf.device)
    inv = torch.where(amax > 0, c127 / amax, torch.zeros_like(amax))
    q = torch.clamp(torch.round(xf * inv), -127, 127).to(torch.int8)       # torch.round: half to even
    return q, (amax / c127).squeeze(-1)


def acc_i8(qa, qw):
    """the exact integer product [M, N] as f64"""
    return qa.double() @ qw.double().t()


def gelu64(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def gemm_i8(qa, sa, qw, sw, bias=None, epi=0, resid=None, gate=None, rows_per_batch=1):
    """(E f64 [M, N], gamma f64 [M, N]) of the epilogue `epi` on the exact product (module docstring)"""
    acc = acc_i8(qa, qw)
    sc = acc * sa.double()[:, None] * sw.double()[None, :]
    v = sc + (bias.double()[None, :] if bias is not None else 0.0)
    gv = U * (3.0 * sc.abs() + v.abs())
    if epi == 0:
        return v, gv
    if epi == 1:
        E = gelu64(v)
        a = (v * (GELU_A + GELU_B * v * v)).abs()
        return E, 1.13 * gv + U * (8.0 + 3.0 * a) * E.abs()
    r = resid.double()
    if epi == 3:
        E = v + r
        return E, gv + U * E.abs()
    g = gate.double()[torch.arange(qa.shape[0], device=qa.device) // rows_per_batch]
    E = r + g * v
    return E, g.abs() * gv + U * E.abs()


def bar_bf16(out, E, gamma):
    return 0.5 * torch.maximum(ulp_bf16(E), ulp_bf16(out.double())) + gamma


def rownorm64(h, shift, scale, rows_per_batch, eps):
    """(n f64 [rows, D], gamma_n) of n = h r (1 + scale[g]) + shift[g], g = row / rows_per_batch; h bf16 values, f32 tables [groups, D]"""
    hd = h.double()
    D = hd.shape[-1]
    g = torch.arange(hd.shape[0], device=h.device) // rows_per_batch
    r = 1.0 / torch.sqrt((hd * hd).sum(-1, keepdim=True) / D + eps)
    t = hd * r * (1.0 + scale.double()[g])
    n = t + shift.double()[g]
    return n, U * ((D / 128.0 + 10.0) * t.abs() + n.abs())


def rownorm_quant(h, shift, scale, rows_per_batch, eps):
    """the engine's order in f32 (the statistics' sum order aside): -> (q, row_scale)"""
    hf = h.float()
    D = hf.shape[-1]
    g = torch.arange(hf.shape[0], device=h.device) // rows_per_batch
    r = 1.0 / torch.sqrt((hf * hf).sum(-1, keepdim=True) * torch.tensor(1.0 / D, dtype=torch.float32, device=h.device) + eps)
    n = (hf * r) * (1.0 + scale.float()[g]) + shift.float()[g]
    return quant_rows(n)


# ---- the oracle's block linears in W8A8 ----
_KINDS = (("attn1.to_q", I8_QKV, False), ("attn1.to_k", I8_QKV, False), ("attn1.to_v", I8_QKV, False), ("attn1.to_out.0", I8_TO_OUT, True),
          ("ff.net.0.proj", I8_FF1, False), ("ff.net.2", I8_FF2, True))


def linear_w8a8(x, w, b, round_input):
    """one quantised layer on the oracle's tensors: x quantised per row (after a bf16 rounding where the engine stores the tensor in
    bf16), w from its bf16 rounding per output channel, the exact product scaled in f64 and returned in x's dtype"""
    xin = x.bfloat16().float() if round_input else x.float()
    lead = xin.shape[:-1]
    qa, sa = quant_rows(xin.reshape(-1, xin.shape[-1]))
    qw, sw = quant_rows(w.bfloat16().float())
    y = acc_i8(qa, qw) * sa.double()[:, None] * sw.double()[None, :]
    if b is not None:
        y = y + b.double()[None, :]
    return y.to(x.dtype).reshape(*lead, w.shape[0])


@contextlib.contextmanager
def w8a8(weights, mask=I8_ALL, block_masks=None):
    """inside the context ltx_oracle.linear runs the block linears that `mask` (and-ed with block_masks[l] where given) names in W8A8;
    the weight tensors of `weights` (the dict handed to the oracle's forward) are recognised by identity.  Yields a dict whose
    "hits" counts the substituted calls."""
    table = {}
    l = 0
    while f"transformer_blocks.{l}.attn1.to_q.weight" in weights:
        m = mask & (block_masks[l] if block_masks is not None else I8_ALL)
        for name, bit, rnd in _KINDS:
            if m & bit:
                table[id(weights[f"transformer_blocks.{l}.{name}.weight"])] = rnd
        l += 1
    stats = {"hits": 0}
    plain = O.linear

    def linear(x, w, b):
        rnd = table.get(id(w))
        if rnd is None:
            return plain(x, w, b)
        stats["hits"] += 1
        return linear_w8a8(x, w, b, rnd)

    O.linear = linear
    try:
        yield stats
    finally:
        O.linear = plain
