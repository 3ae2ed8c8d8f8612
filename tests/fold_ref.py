"""Torch-CPU reference of the DiT's norm fold (GemmArgs::C2 / ::rs_sq, candle-video_amd/csrc/kernels.h) and of the three small
launchers around it, in float64.  Not a test module (tests/test_fold_ref_cpu.py pins it against the unfolded block expression,
tests/test_gpu_fold_ops.py compares the HIP kernels against it).  No HIP here.

LtxVideoTransformerBlock::forward (ltx_transformer.rs:847-851, 905-909) normalises h and modulates it in front of the q|k|v and
ff1 projections: y = h * r * (1 + sc) + sh, r_m = 1 / sqrt(mean(h_m^2) + eps).  Times W^T that is
    r_m * ((h (.) (1 + sc)) W^T) + (sh W^T + b)
so the layer that writes h (a residual epilogue) also stores C2 = h (.) (1 + sc) and the row partials of h (fold_out_ref), a
GEMV per timestep gives cvec = sh W^T + b (shift_gemv_ref), and the projection finishes with r_m and cvec (fold_in_ref).

dtype = torch.bfloat16 places the roundings where the kernels place them (C stored in bf16, C2 one f32 multiply of the stored C
and one bf16 rounding - reproducible on the CPU bit for bit); dtype = torch.float64 rounds nothing: the algebra alone."""
import math
from typing import Optional, Tuple

import torch
from torch import Tensor


def batch_rows(v: Tensor, M: int, rows_per_batch: int) -> Tensor:
    """v [batch, n] -> [M, n]: row m takes v[b(m)], b(m) = m // rows_per_batch"""
    return v[torch.arange(M) // rows_per_batch]


def gelu_tanh(x: Tensor) -> Tensor:
    """gelu_approximate (ltx_transformer.rs:214-226) in x's dtype"""
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x)))


def resid_epilogue_ref(x: Tensor, w: Tensor, bias: Optional[Tensor], resid: Tensor, gate: Optional[Tensor], epi: int, rows_per_batch: int) -> Tensor:
    """epi 2: resid + gate[b(m)] * (x W^T + bias) (ltx_transformer.rs:900, :934); epi 3: resid + (x W^T + bias) (:909).  float64."""
    lin = x.double() @ w.double().T
    if bias is not None:
        lin = lin + bias.double()
    if epi == 2:
        return resid.double() + batch_rows(gate.double(), x.shape[0], rows_per_batch)[:, :w.shape[0]] * lin
    assert epi == 3, epi
    return resid.double() + lin


def rowsq_ref(stored: Tensor) -> Tensor:
    """per-row sums of squares of a stored matrix, one per 128-column group (the last one may be narrower): [M, ceil(N / 128)] f64"""
    M, N = stored.shape
    ng = (N + 127) // 128
    sq = torch.zeros(M, ng * 128, dtype=torch.float64)
    sq[:, :N] = stored.double() ** 2
    return sq.view(M, ng, 128).sum(-1)


def mod_scale_ref(stored: Tensor, scale: Tensor, rows_per_batch: int) -> Tensor:
    """C2 of kernels.h: T(float(stored) * (1.0f + scale[b(m)])) - float32 arithmetic on the values as stored, one rounding to T
    (float64 input: exact, no rounding)"""
    M, N = stored.shape
    if stored.dtype == torch.float64:
        return stored * (1.0 + batch_rows(scale.double(), M, rows_per_batch)[:, :N])
    one_plus = 1.0 + batch_rows(scale.float(), M, rows_per_batch)[:, :N]          # f32: one rounding
    return (stored.float() * one_plus).to(stored.dtype)                           # f32 product, then the rounding to T


def fold_out_ref(x: Tensor, w: Tensor, bias: Optional[Tensor], resid: Tensor, gate: Optional[Tensor], scale2: Tensor, epi: int, rows_per_batch: int,
                 dtype=torch.bfloat16, stored: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """Producer side -> (C float64 before any rounding, C2, rowsq float64 of C as stored).  `stored`: the C a kernel stored (C2
    and rowsq are functions of the STORED values); default C rounded to dtype through float32, as an f32 accumulator is."""
    C = resid_epilogue_ref(x, w, bias, resid, gate, epi, rows_per_batch)
    if stored is None:
        stored = C if dtype == torch.float64 else C.float().to(dtype)
    return C, mod_scale_ref(stored, scale2, rows_per_batch), rowsq_ref(stored)


def row_rinv_ref(rs_sq: Tensor, rs_D: int, eps: float) -> Tensor:
    """r_m = 1 / sqrt(sum_g rs_sq[m, g] / rs_D + eps) in float64"""
    return 1.0 / torch.sqrt(rs_sq.double().sum(-1) / rs_D + eps)


def fold_in_ref(a: Tensor, w: Tensor, rs_sq: Tensor, rs_D: int, eps: float, cvec: Tensor, epi: int, rows_per_batch: int) -> Tensor:
    """Consumer side: epi(r_m * (A W^T) + cvec[b(m)]), epi 0 none / 1 GELU-tanh.  float64."""
    M, N = a.shape[0], w.shape[0]
    out = row_rinv_ref(rs_sq, rs_D, eps)[:, None] * (a.double() @ w.double().T) + batch_rows(cvec.double(), M, rows_per_batch)[:, :N]
    if epi == 1:
        return gelu_tanh(out)
    assert epi == 0, epi
    return out


def shift_gemv_ref(w: Tensor, bias: Optional[Tensor], shift: Tensor) -> Tensor:
    """cvec[b][n] = sum_k shift[b][k] * w[n][k] + bias[n] (shift [B, >= K]: the first K columns).  float64."""
    K = w.shape[1]
    out = shift.double()[:, :K] @ w.double().T
    return out if bias is None else out + bias.double()


def scale_cols_ref(w: Tensor, scale: Tensor) -> Tensor:
    """w[n][k] * (1 + scale[k]): float32 arithmetic, one rounding to w's dtype (float64 input: exact)"""
    if w.dtype == torch.float64:
        return w * (1.0 + scale.double())[None, :]
    return (w.float() * (1.0 + scale.float())[None, :]).to(w.dtype)
