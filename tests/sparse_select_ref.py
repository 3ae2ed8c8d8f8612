"""Plain f64 torch restatement of include/ltxhip_sparse_dynamic.h: the pooled means of q' and k, and the selection of key tiles per
(batch row, head, 128-query block) with, per map row, the MARGIN by which the reference's own choice holds.  q, k are [B, S, heads * hd];
maps are bool [B, heads, NQB, NKT] (sparse_attn_ref.pack makes the words).

The bound tau (u = 2^-24, A = the row's largest sum_d |qbar_d kbar_d|, every figure a relative error):
  s^ is an FMA chain of hd terms: |ds| <= hd u A; x = s^ - max carries two of them and one rounding of |x| <= 2 A: |dx| <= (2 hd + 2) u A;
  p^ = w exp2(x): ln 2 |dx| from x, 4 u for v_exp_f32 (1 ulp of f32), u for the product:  e_p = ln 2 (2 hd + 2) u A + 5 u
      (a p^ flushed to zero is off by less than 2^-120 of T >= 1: nothing);
  T and before_i are ascending sums of at most NKT non-negative terms: e_p from the terms and NKT u from the additions, relative to T;
  mass * T adds one rounding.  The comparison before_i < mass T can differ only where |before_i - mass T| / T <= 2 (e_p + NKT u) + u,
  and two tiles can trade places in the order only where their relative gap is <= 2 e_p - smaller than the first.  So
      tau = 2 (e_p + NKT u) + u
  and a row whose margin (below) is at least tau must come out of the kernel exactly as it does here."""
import math

import torch


def _blocks(x, heads, rows):
    """[B, S, heads * hd] -> f64 block means [B, heads, ceil(S / rows), hd]"""
    B, S, D = x.shape
    n = (S + rows - 1) // rows
    pad = torch.zeros(B, n * rows, D, dtype=torch.float64)
    pad[:, :S] = x.double().cpu()
    cnt = torch.full((n,), float(rows), dtype=torch.float64); cnt[-1] = S - (n - 1) * rows
    return (pad.reshape(B, n, rows, heads, D // heads).sum(2) / cnt[None, :, None, None]).transpose(1, 2)


def pool64(q, k, heads):
    return _blocks(q, heads, 128), _blocks(k, heads, 64)


def tau(hd, nkt, A):
    u = 2.0 ** -24
    return 2.0 * (math.log(2.0) * (2 * hd + 2) * u * A + 5 * u + nkt * u) + u


def select64(qbar, kbar, S, mass, keep=None):
    """qbar [B, heads, NQB, hd], kbar [B, heads, NKT, hd] (the f32 means the kernel read) -> (bits bool [B, heads, NQB, NKT], forced bool
    of the same shape: the diagonal and keep, margin f64 [B, heads, NQB], tau f64 [B, heads, NQB]); keep bool [NQB, NKT] or [heads, NQB, NKT]"""
    qbar, kbar = qbar.double().cpu(), kbar.double().cpu()
    nqb, nkt, hd = qbar.shape[2], kbar.shape[2], qbar.shape[3]
    s = qbar @ kbar.transpose(-1, -2)
    A = (qbar.abs() @ kbar.abs().transpose(-1, -2)).amax(-1)
    w = torch.full((nkt,), 64.0, dtype=torch.float64); w[-1] = S - 64 * (nkt - 1)
    p = w * torch.exp2(s - s.amax(-1, keepdim=True))
    T = p.sum(-1, keepdim=True)
    ps, order = torch.sort(p, dim=-1, descending=True, stable=True)      # ties: the lower tile first
    before_sorted = ps.cumsum(-1) - ps
    before = torch.empty_like(p).scatter_(-1, order, before_sorted)
    by_mass = (before < mass * T) | (mass >= 1.0)
    forced = torch.zeros_like(by_mass)
    for qb in range(nqb):
        forced[..., qb, 2 * qb:2 * qb + 2] = True
    if keep is not None:
        forced |= keep.bool()
    # the margin: the relative gap between the last tile the mass takes and the first it leaves, and the nearest before_i to mass T
    n_sel = (before_sorted < mass * T).sum(-1, keepdim=True)             # the selection is a prefix of the sorted order
    last = ps.gather(-1, (n_sel - 1).clamp(min=0))
    first_out = torch.where(n_sel < nkt, ps.gather(-1, n_sel.clamp(max=nkt - 1)), torch.zeros_like(last))
    gap = torch.where(n_sel < nkt, (last - first_out) / last, torch.full_like(last, math.inf))[..., 0]
    near = ((before - mass * T).abs() / T).amin(-1)
    margin = torch.minimum(gap, near) if mass < 1.0 else torch.full_like(near, math.inf)
    return by_mass | forced, forced, margin, tau(hd, nkt, A)
