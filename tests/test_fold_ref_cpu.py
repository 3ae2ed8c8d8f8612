"""CPU suite: tests/fold_ref.py (the float64 reference of the norm fold) proved against the unfolded block expression before it
judges a kernel, and ltx_op_linear_fold_ok (host code: no device needed) on a table of shapes.

The unfolded expression is LtxVideoTransformerBlock::forward's linear(rms_norm(h) * (1 + sc) + sh) (ltx_transformer.rs:847-851).
oracle/ltx_oracle.py's rms_norm keeps its statistics in float32 whatever it is given (as the reference does), so it cannot carry
a 1e-12 bar: the bar is held against the oracle's expression evaluated in float64 (rms_norm_f64 below, the same lines), and
the oracle's own function is held to what float32 allows."""
import pytest
import torch

import fold_ref as R
import ltx_oracle as O


def rms_norm_f64(x, eps):
    """ltx_oracle.rms_norm without its float32 cast: (x * x).sum(-1) * (1 / D), (ms + eps).sqrt(), x / denom"""
    ms = (x * x).sum(-1, keepdim=True) * (1.0 / x.shape[-1])
    return x / (ms + eps).sqrt()


def rel_max(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("epi_out,epi_in", [(3, 0), (2, 1)])
@pytest.mark.parametrize("M,rpb,D,N,Kp", [(22, 11, 256, 24, 40), (21, 7, 384, 36, 16), (9, 9, 130, 8, 8)])
def test_fold_composition_equals_the_unfolded_block_expression(epi_out, epi_in, M, rpb, D, N, Kp):
    """fold_out_ref -> rowsq -> shift_gemv_ref -> fold_in_ref in float64 (no rounding) against linear(rms_norm(h) (1 + sc) + sh):
    <= 1e-12 relative.  D = 130: a last partial group narrower than 128 columns."""
    g = torch.Generator().manual_seed(M + D + N)
    B = M // rpb
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, wp, bp, resid, gate = rnd(M, Kp), rnd(D, Kp) / Kp ** 0.5, rnd(D) * 0.1, rnd(M, D), rnd(B, D)
    sc, sh = rnd(B, D) * 0.3, rnd(B, D) * 0.5
    w, b = rnd(N, D) / D ** 0.5, rnd(N) * 0.1
    eps = 1e-6
    h, h2, rowsq = R.fold_out_ref(x, wp, bp, resid, gate, sc, epi_out, rpb, dtype=torch.float64)
    assert rowsq.shape == (M, (D + 127) // 128)
    cvec = R.shift_gemv_ref(w, b, sh)
    got = R.fold_in_ref(h2, w, rowsq, D, eps, cvec, epi_in, rpb)
    # the unfolded form, on the same h
    want_h = resid + (R.batch_rows(gate, M, rpb) if epi_out == 2 else 1.0) * (x @ wp.T + bp)
    assert torch.equal(h, want_h)
    y = rms_norm_f64(want_h, eps) * (1.0 + R.batch_rows(sc, M, rpb)) + R.batch_rows(sh, M, rpb)
    want = O.linear(y, w, b)
    if epi_in == 1:
        want = R.gelu_tanh(want)
    assert rel_max(got, want) <= 1e-12, rel_max(got, want)
    # ... and the oracle's own functions (float32 statistics / float32 GELU): as close as float32 allows
    y32 = O.rms_norm(want_h, None, eps) * (1.0 + R.batch_rows(sc, M, rpb)) + R.batch_rows(sh, M, rpb)
    want32 = O.linear(y32, w, b)
    if epi_in == 1:
        want32 = O.gelu_approximate(want32)
    assert rel_max(got, want32.double()) <= 2e-6, rel_max(got, want32.double())


def test_bf16_mode_rounds_where_the_kernels_round():
    g = torch.Generator().manual_seed(3)
    M, rpb, D, Kp = 12, 6, 256, 16
    x, wp, bp = torch.randn(M, Kp, generator=g).bfloat16(), torch.randn(D, Kp, generator=g).bfloat16(), torch.randn(D, generator=g).bfloat16()
    resid, sc = torch.randn(M, D, generator=g).bfloat16(), torch.randn(2, D, generator=g) * 0.3
    C, C2, rowsq = R.fold_out_ref(x, wp, bp, resid, None, sc, 3, rpb)
    stored = C.float().bfloat16()
    assert C2.dtype == torch.bfloat16
    # one f32 multiply of the stored value and one rounding, per element
    m, n = 7, 200
    assert float(C2[m, n]) == float((torch.tensor(float(stored[m, n]), dtype=torch.float32) * (torch.tensor(1.0, dtype=torch.float32) + sc[1, n])).bfloat16())
    assert torch.equal(rowsq, R.rowsq_ref(stored)) and abs(float(rowsq[m, 1]) - float((stored[m, 128:].double() ** 2).sum())) < 1e-12
    # a given stored matrix overrides the default rounding (the GPU tests pass the kernel's own output)
    other = (stored.float() * 1.5).bfloat16()
    _, C2b, rowsqb = R.fold_out_ref(x, wp, bp, resid, None, sc, 3, rpb, stored=other)
    assert torch.equal(C2b, R.mod_scale_ref(other, sc, rpb)) and torch.equal(rowsqb, R.rowsq_ref(other))
    w = torch.randn(8, 16, generator=g).bfloat16(); s = torch.randn(16, generator=g)
    assert torch.equal(R.scale_cols_ref(w, s), (w.float() * (1.0 + s)).bfloat16())


# (M, N, K, epi, consumer, rs_n, vec_stride, rows_per_batch) -> served?   Default options; shape rules: more than 512 rows, an unsplit
# shape (M * N > 8 388 608 above 1536 rows: ltx_gemm_split_factor), K % 64 == 0, N % 8 == 0, 4 .. 16 partials in fours, batch
# elements of at least 320 rows, 16-byte aligned vector rows
FOLD_OK_TABLE = [
    ((2200, 4096, 2048, 0, 1, 16, 4096, 1100), True),
    ((2200, 4096, 2048, 1, 1, 16, 4096, 1100), True),
    ((2199, 4096, 512, 0, 1, 4, 4096, 733), True),
    ((2199, 4096, 1024, 1, 1, 8, 4096, 733), True),
    ((2199, 4096, 1536, 0, 1, 12, 4096, 733), True),
    ((2240, 4096, 2048, 0, 1, 16, 4096, 320), True),
    ((2200, 4104, 2048, 0, 1, 16, 4104, 1100), True),
    ((1100, 4096, 2048, 0, 1, 16, 4096, 1100), True),
    ((733, 4096, 512, 0, 1, 4, 4096, 733), True),
    ((2200, 4096, 2048, 0, 1, 20, 4096, 1100), False),        # more than 16 partials
    ((2200, 4096, 2048, 0, 1, 6, 4096, 1100), False),         # not in fours
    ((2200, 4096, 2048, 0, 1, 0, 4096, 1100), False),
    ((2233, 4096, 2048, 0, 1, 16, 4096, 319), False),         # a tile could straddle two boundaries
    ((512, 4096, 2048, 0, 1, 16, 4096, 512), False),          # the small-M tiles' rows
    ((2200, 4096, 2048, 2, 1, 16, 4096, 1100), False),        # the row scale rides on bias / GELU only
    ((2200, 4096, 2048, 0, 1, 16, 4102, 1100), False),        # cvec rows not 16-byte aligned
    ((2200, 4100, 2048, 0, 1, 16, 4100, 1100), False),        # N % 8
    ((2200, 4096, 2080, 0, 1, 16, 4096, 1100), False),        # K % 64
    ((2200, 2048, 2048, 0, 1, 16, 2048, 1100), False),        # a split-K shape (M * N below the rule)
    ((4110, 2048, 2048, 2, 0, 0, 2048, 2055), True),
    ((4110, 2048, 2048, 3, 0, 0, 2048, 2055), True),
    ((4110, 2048, 512, 3, 0, 0, 2048, 2055), True),
    ((4110, 2048, 8192, 2, 0, 0, 12288, 2055), True),
    ((16400, 512, 512, 3, 0, 0, 512, 8200), True),
    ((4110, 2048, 2048, 0, 0, 0, 2048, 2055), False),         # the second output rides on the residual epilogues only
    ((4110, 2048, 2048, 1, 0, 0, 2048, 2055), False),
    ((4096, 2048, 2048, 3, 0, 0, 2048, 2048), False),         # M * N == 8 388 608: still split
    ((512, 2048, 2048, 3, 0, 0, 2048, 512), False),
    ((4110, 2048, 2048, 3, 0, 0, 2048, 319), False),
    ((4110, 2048, 2048, 3, 0, 0, 2050, 2055), False),
]


@pytest.fixture(scope="module")
def hip():
    import ltxhip
    return ltxhip


def test_linear_fold_ok_answers_by_shape(hip):
    for args, want in FOLD_OK_TABLE:
        assert hip.ops.linear_fold_ok(*args) is want, (args, want)


def test_linear_fold_ok_stands_down_when_the_call_is_routed_elsewhere(hip):
    """gemm_off=big hands every GEMM to the 128 x 128 kernel, gemm_off=asm16 takes the one-wave-per-SIMD tiles out of the plans,
    gemm_wide_epi=0 their epilogue: no fold in any of them."""
    served = [a for a, want in FOLD_OK_TABLE if want]
    for opts in (dict(gemm_off="big"), dict(gemm_off="asm16"), dict(gemm_wide_epi="0")):
        with hip.options(**opts):
            for args in served:
                assert not hip.ops.linear_fold_ok(*args), (opts, args)
    for args in served:
        assert hip.ops.linear_fold_ok(*args), args
