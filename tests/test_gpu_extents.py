"""GPU suite: what an op may touch.  Every case runs one C entry of include/ltxhip_ops.h (and the int8 / fp8 / stg /
step-cache headers) on operands laid into the arena of tests/extents.py, four times: twice on the tame filler (the control: the op
repeats its bits), once with NaN and once with +Inf in every byte around the operands.  Per case:
  1. control    the two tame runs are bit-equal
  2. filler     the tame, NaN and Inf runs are bit-equal: no byte outside the documented operands reaches the result
  3. guards     Arena.verify() after every run: no filler byte and no input changed, every output element written
  4. value      the bar the op's own suite uses against its f32 / f64 reference (imported, not restated); nothing NaN or Inf
  5. route      where the library has a decision step, the kernel family the case is meant for served it
B = 2 wherever the entry has a batch.  Strided operands come `fused` (column slices of one wider buffer, as the DiT passes q | k | v)
and `padded` (ld = cols + 8, filler in the gap).  Shapes are the smallest that leave a ragged tile on every axis the kernel tiles:
M = BM + 8, N = BN + 8, K = two K steps + 16 for the GEMM tiles.
Refusals asserted instead of a run: attention_compact on strided k / v (it demands dense rows)."""
import math

import pytest
import torch

import extents as E
import fp8_ref as F
import int8_ref as R
import int8_attn_ref as A8
import ltx_oracle as O
import test_gpu_norm_kernels as NK
from conftest import rel_l2
from test_gpu_fold_ops import check_floor
from test_gpu_gemm_route import KERNEL_OF, family
from test_gpu_ops import check, cl, ncthw, ref_attention

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
LOG2E = 1.4426950408889634
CASES = {}


@pytest.fixture(scope="module")
def hip():
    import ltxhip
    assert torch.cuda.is_available()
    return ltxhip


def case(name, capacity=48 << 20, **opts):
    def deco(fn):
        assert name not in CASES, name
        CASES[name] = (fn, opts, capacity)
        return fn
    return deco


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape, scale=1.0, dt=BF16):
    return (torch.randn(*shape, generator=g) * scale).to(dt)


def dtc(hip, dt):
    return hip._dt(dt)


def routed(st, got, want):
    """assertion 5 on a probe's answer"""
    assert got == want, ("route", got, want)
    st["routed"] = True


def launch(hip, st, kernel, call):
    """run `call` (a C entry: the return code is checked); with `kernel`, the ONE GEMM kernel that counts a launch must be it"""
    if kernel is None:
        hip._check(call())
        return
    hip.prof_enable(True)
    try:
        hip._check(call())
        torch.cuda.synchronize()
        counts = {k: sum(hip.prof_report_kernel(cls, i)[2] for cls in (0, 1)) for i, k in enumerate(hip.PROF_KERNELS)}
    finally:
        hip.prof_enable(False)
    assert {k for k, c in counts.items() if c} == {kernel}, (kernel, counts)
    st["routed"] = True


def stream(hip):
    return hip._stream()


# ================================================================== GEMM families through ltx_op_linear (bf16)
def linear_inputs(M, N, K, dt, seed, rpb):
    g = gen(seed)
    x, w, b = randn(g, M, K, dt=dt), randn(g, N, K, scale=K ** -0.5, dt=dt), randn(g, N, scale=0.1, dt=dt)
    r = randn(g, M, N, dt=dt); gate = randn(g, -(-M // rpb), N, dt=F32)
    return x, w, b, r, gate


def linear_want(x, w, b, r, gate, epi, rpb):
    lin = x.double() @ w.double().T + (b.double() if b is not None else 0)
    rows = torch.arange(x.shape[0]) // rpb
    if epi == 0:
        return lin.float()
    return (r.double() + (gate.double()[rows] * lin if epi == 2 else lin)).float()


def linear_case(name, M, N, K, fam, epi=0, dt=BF16, packed=False, rpb=None, capacity=48 << 20, **opts):
    """rpb: rows per batch of the gate (epilogue 2): a boundary inside the first tile"""
    rpb = rpb or max(M // 2 - 3, 1)

    @case(name, capacity, **opts)
    def fn(hip, A, st):
        x, w, b, r, gate = linear_inputs(M, N, K, dt, M + N + K + epi, rpb)
        px, _ = A.place(x, name="x"); pw, _ = A.place(w, name="w"); pb, _ = A.place(b, name="bias")
        pr = pg = None
        if epi >= 2:
            pr, _ = A.place(r, name="resid")
        if epi == 2:
            pg, _ = A.place(gate, name="gate")
        py, y = A.place(torch.empty(M, N, dtype=dt), role="out", name="y")
        route = hip.ops.gemm_route(M, N, K, epi=epi, dtype=dt)
        routed(st, family(route) if fam in KERNEL_OF else route, fam)
        st["note"] = route
        if packed:
            wp = hip.ops.ring_pack(w.to(DEV)).cpu()
            pwp, _ = A.place(wp, name="w_packed")
            call = lambda: hip.lib.ltx_op_linear_packed(px, pw, pwp, pb, py, M, N, K, epi, pr, pg, rpb, stream(hip))
        else:
            call = lambda: hip.lib.ltx_op_linear(px, pw, pb, py, M, N, K, dtc(hip, dt), epi, pr, pg, rpb, stream(hip))
        A.arm()
        launch(hip, st, KERNEL_OF[fam], call)
        st["check"] = lambda o: check(o["y"], linear_want(x, w, b, r, gate, epi, rpb), dt)
        return {"y": y}
    return fn


# the one-wave-per-SIMD family serves more than 512 rows, unsplit shapes and K % 64 == 0 only (gemm_route sends K = 512 + 16 to 160x128): the
# nearest ragged shape it serves has K = 512 + 64.  N = 1032 leaves 8 live columns in the last 256-wide tile
linear_case("linear asm16 epi0", 2304 + 8, 1024 + 8, 512 + 64, "asm16", 0, gemm_plan="asm16")
linear_case("linear asm16 epi2", 2304 + 8, 1024 + 8, 512 + 64, "asm16", 2, gemm_plan="asm16")
linear_case("linear asm16 epi3", 2304 + 8, 1024 + 8, 512 + 64, "asm16", 3, gemm_plan="asm16")
for _epi in (0, 2, 3):
    linear_case(f"linear ring epi{_epi}", 72, 40, 144, "ring", _epi)                       # ring:64x32
    linear_case(f"linear ring packed epi{_epi}", 72, 40, 144, "ring", _epi, packed=True)
    linear_case(f"linear gemm128 epi{_epi}", 136, 136, 144, "gemm128", _epi, gemm_off="big")
    linear_case(f"linear f32 (130, 96, 72) epi{_epi}", 130, 96, 72, "gemm128", _epi, dt=F32)
linear_case("linear ring M=1", 1, 40, 144, "ring", 0)
linear_case("linear gemm128 M=1", 1, 136, 144, "gemm128", 0, gemm_off="big")
for _tile in ("256x256", "192x256", "128x256", "256x128", "192x128", "160x128", "128x128", "192x64", "160x256w16", "p8:256", "p8:128"):
    _bm, _bn = (128, int(_tile[3:])) if _tile.startswith("p8") else [int(v[:3]) for v in _tile.split("x")]
    for _epi in (0, 2, 3):
        linear_case(f"linear {_tile} epi{_epi}", _bm + 8, _bn + 8, 144, "p8" if _tile.startswith("p8") else "big", _epi, gemm_plan=_tile)
# the tail split-K of gemm_big (test_gpu_ops.test_gemm_tail_split_k's shapes: the split is active for every tile there)
for _tile in ("192x128", "160x128", "128x128", "256x256", "192x64", "160x256w16"):
    linear_case(f"linear {_tile} split-K", 1500, 56 if _tile == "192x64" else 600, 2048, "big", 2, rpb=750, gemm_plan=_tile)


@case("linear_segmented (77, 192, 64, seg 64)")
def _segmented(hip, A, st):
    M, N, K, seg = 77, 192, 64, 64
    x, w, b, _, _ = linear_inputs(M, N, K, BF16, 5, M)
    px, _ = A.place(x, name="x"); pw, _ = A.place(w, name="w"); pb, _ = A.place(b, name="bias")
    py, y = A.place(torch.empty(N // seg * M, seg, dtype=BF16), role="out", name="y")        # three dense [M, seg] matrices
    routed(st, family(hip.ops.gemm_route(M, N, K)), "ring")
    A.arm()
    launch(hip, st, KERNEL_OF["ring"], lambda: hip.lib.ltx_op_linear_segmented(px, pw, pb, py, M, N, K, seg, 1, stream(hip)))
    want = linear_want(x, w, b, None, None, 0, M)
    st["check"] = lambda o: check(o["y"].view(N // seg, M, seg).permute(1, 0, 2).reshape(M, N), want, BF16)
    return {"y": y}


@case("linear_rowsq (72, 136, 144)")
def _linear_rowsq(hip, A, st):
    M, N, K = 72, 136, 144
    x, w, b, _, _ = linear_inputs(M, N, K, BF16, 6, M)
    px, _ = A.place(x, name="x"); pw, _ = A.place(w, name="w"); pb, _ = A.place(b, name="bias")
    py, y = A.place(torch.empty(M, N, dtype=BF16), role="out", name="y")
    ps, rs = A.place(torch.empty(M, 2, dtype=F32), role="out", name="rowsq")                   # ceil(N / 128) partial columns
    routed(st, family(hip.ops.gemm_route(M, N, K)), "ring")
    A.arm()
    launch(hip, st, KERNEL_OF["ring"], lambda: hip.lib.ltx_op_linear_rowsq(px, pw, pb, py, ps, M, N, K, 1, 0, None, None, 1, stream(hip)))
    
    def value(o):
        check(o["y"], linear_want(x, w, b, None, None, 0, M), BF16)
        yd = o["y"].double()
        want = torch.stack([(yd[:, :128] ** 2).sum(-1), (yd[:, 128:] ** 2).sum(-1)], -1)
        assert rel_l2(o["rowsq"], want.float()) < 1e-6                                         # test_gpu_fold_ops' bar for the partials
    st["check"] = value
    return {"y": y, "rowsq": rs}


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
def test_rowsq_with_a_row_stride(hip, dt):
    """ltx_op_rowsq on [rows, N] with ld = N + 8 and as a column slice of a wider buffer: ceil(N / 128) partials per row"""
    rows, N = 37, 264

    def body(fused):
        def run(A):
            g = gen(11)
            x, other = randn(g, rows, N, dt=dt), randn(g, rows, 128, dt=dt)
            if fused:
                (_, _), (px, xv) = A.place_fused([other, x], ["in", "in"], names=["left", "x"])
            else:
                px, xv = A.place(x, ld=N + 8, name="x")
            ps, rs = A.place(torch.empty(rows, 3, dtype=F32), role="out", name="rowsq")
            A.arm()
            hip._check(hip.lib.ltx_op_rowsq(px, rows, N, xv.stride(0), ps, dtc(hip, dt), stream(hip)))
            run.x = x
            return {"rowsq": rs}
        out = E.filler_passes(run, DEV)
        xd = run.x.double()
        want = torch.stack([(xd[:, i:i + 128] ** 2).sum(-1) for i in (0, 128, 256)], -1)
        assert torch.isfinite(out["rowsq"]).all() and rel_l2(out["rowsq"], want.float()) < 1e-6
    body(False); body(True)


@case("linear_deferred + rownorm_deferred (40, 136, 8192)")
def _deferred(hip, A, st):
    M, N, K = 40, 136, 8192                  # (the shape rule leaves the K ranges un-reduced from K = 8192 up, in steps of 64)
    P = hip.lib.ltx_op_linear_split_factor(M, N, K)
    x, w, b, r, gate = linear_inputs(M, N, K, BF16, 7, 20)
    sc, sh = randn(gen(8), 2, N, scale=0.3, dt=F32), randn(gen(9), 2, N, scale=0.3, dt=F32)
    px, _ = A.place(x, name="x"); pw, _ = A.place(w, name="w"); pb, _ = A.place(b, name="bias"); pr, _ = A.place(r, name="resid")
    pg, _ = A.place(gate, name="gate"); psc, _ = A.place(sc, name="scale"); psh, _ = A.place(sh, name="shift")
    pp, parts = A.place(torch.empty(P * M, N, dtype=F32), role="out", name="parts")          # written by the first entry, read by the second
    ph, h = A.place(torch.empty(M, N, dtype=BF16), role="out", name="h_out"); py, y = A.place(torch.empty(M, N, dtype=BF16), role="out", name="y")
    assert P >= 2, P
    routed(st, hip.ops.norm_route(M, N, BF16, kind=0, scale=True, rows_per_batch=20, nparts=P), "wide_defer4")
    A.arm()
    launch(hip, st, KERNEL_OF["ring"], lambda: hip.lib.ltx_op_linear_deferred(px, pw, pp, M, N, K, stream(hip)))
    hip._check(hip.lib.ltx_op_rownorm_deferred(pp, P, pb, pr, pg, N, ph, py, M, N, 0, 1e-6, psc, psh, 20, N, 1, stream(hip)))

    def value(o):
        want_h = linear_want(x, w, b, r, gate, 2, 20)
        check(o["h_out"], want_h, BF16)
        c = dict(presum_n=0, kind=0, rpb=20, act=0)
        ref = NK.rownorm_formula(c, dict(x=o["h_out"], weight=None, scale=sc, shift=sh, presum=None))
        NK.assert_close(o["y"], ref, "bf16", NK.FLOOR["rownorm"], "rownorm_deferred")
        check(o["parts"].view(P, M, N).sum(0), (x.double() @ w.double().T).float(), F32)
    st["check"] = value
    return {"parts": parts, "h_out": h, "y": y}


@case("shift_gemv (B 2, N 136, K 144, strides > N, K)")
def _shift_gemv(hip, A, st):
    B, N, K = 2, 136, 144
    g = gen(12)
    w, b, shift = randn(g, N, K, scale=K ** -0.5), randn(g, N, scale=0.1), randn(g, B, K, dt=F32)
    pw, _ = A.place(w, name="w"); pb, _ = A.place(b, name="bias"); psh, sv = A.place(shift, ld=K + 8, name="shift")
    pc, cv = A.place(torch.empty(B, N, dtype=F32), ld=N + 8, role="out", name="cvec")
    A.arm()
    hip._check(hip.lib.ltx_op_shift_gemv(pw, pb, psh, K + 8, B, N, K, pc, N + 8, stream(hip)))
    st["no_route"] = "ltx_op_shift_gemv has one kernel and no decision step"
    st["check"] = lambda o: check(o["cvec"], (shift.double() @ w.double().T + b.double()).float(), F32)
    return {"cvec": cv}


# ================================================================== quantised GEMMs
def quant_gemm_case(kind, tile, epi, seg=0, w_scale=True):
    M, N, K = 264, 136 if not seg else 256, 144

    @case(f"{kind} tile {tile} epi{epi}" + (" segmented" if seg else "") + ("" if w_scale else " no w_scale"))
    def fn(hip, A, st):
        g = gen(300 + epi + tile)
        rpb = 104
        if kind == "gemm_w8":
            a = randn(g, M, K); w = F.cast(torch.randn(N, K, generator=g) / K ** 0.5)
        else:
            a = torch.randint(-127, 128, (M, K), generator=g).to(torch.int8); w = torch.randint(-127, 128, (N, K), generator=g).to(torch.int8)
        sa = torch.rand(M, generator=g) * 0.02 + 0.002
        sw = (torch.rand(N, generator=g) * 0.004 + 0.0005) if kind == "gemm_i8" else (torch.rand(N, generator=g) + 0.5)
        bias, resid, gate = randn(g, N, scale=0.1), randn(g, M, N), randn(g, -(-M // rpb), N, dt=F32)
        pa, _ = A.place(a, name="a"); pw, _ = A.place(w, name="w"); psw, _ = A.place(sw, name="w_scale"); pb, _ = A.place(bias, name="bias")
        pr = pg = None
        if epi >= 2:
            pr, _ = A.place(resid, name="resid")
        if epi == 2:
            pg, _ = A.place(gate, name="gate")
        nseg = N // seg if seg else 1
        py, y = A.place(torch.empty(nseg * M, N // nseg, dtype=BF16), role="out", name="y")
        if kind == "gemm_i8":
            psa, _ = A.place(sa, name="a_scale")
            call = lambda: hip.lib.ltx_op_gemm_i8(pa, psa, pw, psw, pb, py, M, N, K, epi, pr, pg, rpb, seg, tile, stream(hip))
            kernel = "gemm_i8_kernel"
        else:
            call = lambda: hip.lib.ltx_op_gemm_w8(pa, pw, psw if w_scale else None, pb, py, M, N, K, epi, pr, pg, rpb, seg, tile, stream(hip))
            kernel = "gemm_w8_kernel"
        A.arm()
        launch(hip, st, kernel, call)

        def value(o):
            got = o["y"].view(nseg, M, N // nseg).permute(1, 0, 2).reshape(M, N) if seg else o["y"]
            rows = torch.arange(M) // rpb
            if kind == "gemm_i8":
                import lora_ref
                Eref, gamma = R.gemm_i8(a, sa, w, sw, bias.float(), epi, resid if epi >= 2 else None, gate if epi == 2 else None, rpb)
                assert torch.isfinite(got.float()).all() and lora_ref.worst(got, Eref, gamma, BF16)[0] == 0       # test_gpu_int8's derived bar
            else:
                v = a.double() @ F.widen64(w).t() * (sw.double() if w_scale else 1.0) + bias.double()
                want = [v, None, resid.double() + gate.double()[rows] * v, resid.double() + v][epi]
                check_floor(got, want.float(), st["name"])                                                          # test_gpu_fp8's bar
        st["check"] = value
        return {"y": y}
    return fn


for _tile in (0, 1, 2):
    for _epi in (0, 2):
        quant_gemm_case("gemm_i8", _tile, _epi)
        quant_gemm_case("gemm_w8", _tile, _epi)
    quant_gemm_case("gemm_i8", _tile, 0, seg=128)
    quant_gemm_case("gemm_w8", _tile, 0, w_scale=False)


@pytest.mark.parametrize("tile", [0, 1, 2])
def test_gemm_i8_raw(hip, tile):
    """the int32 accumulators: bit-equal to the integer product (test_gpu_int8's check), inside the arena"""
    M, N, K = 264, 136, 144

    def run(A):
        g = gen(40 + tile)
        a = torch.randint(-127, 128, (M, K), generator=g).to(torch.int8); w = torch.randint(-127, 128, (N, K), generator=g).to(torch.int8)
        pa, _ = A.place(a, name="a"); pw, _ = A.place(w, name="w"); pacc, acc = A.place(torch.empty(M, N, dtype=torch.int32), role="out", name="acc")
        A.arm()
        st = {}
        launch(hip, st, "gemm_i8_kernel", lambda: hip.lib.ltx_op_gemm_i8_raw(pa, pw, pacc, M, N, K, tile, stream(hip)))
        run.want = (a.double() @ w.double().T).to(torch.int32)
        return {"acc": acc}
    out = E.filler_passes(run, DEV)
    assert torch.equal(out["acc"], run.want)


# ================================================================== row passes
def rownorm_case(route, dt, rows, D, kind, weight, mod, act=0, wide_mod=False, presum_n=0):
    name = f"rownorm {route} {'bf16' if dt == BF16 else 'f32'} {rows}x{D} k{kind}" + (" w" if weight else "") + (" mod" if mod else "") + (" stride" if wide_mod else "") + \
        (" silu" if act else "") + (f" presum{presum_n}" if presum_n else "")

    @case(name)
    def fn(hip, A, st):
        rpb = -(-rows // 2)
        c = dict(dtype="bf16" if dt == BF16 else "f32", rows=rows, D=D, kind=kind, rpb=rpb, mod=mod, act=act, weight=weight, presum_n=presum_n)
        inp = NK.rownorm_inputs(c, rows + D + kind)
        routed(st, NK.rownorm_route(hip, c), route)
        px, _ = A.place(inp["x"], name="x"); py, y = A.place(torch.empty(rows, D, dtype=dt), role="out", name="y")
        pw = A.place(inp["weight"], name="weight")[0] if weight else None
        psc = psh = None; ms = 0
        if mod:
            if wide_mod:                                                                        # column slices of one [B, 2 D + 8] table
                (psh, _), (psc, _) = A.place_fused([inp["shift"], inp["scale"]], ["in", "in"], pad=8, names=["shift", "scale"]); ms = 2 * D + 8
            else:
                psc, _ = A.place(inp["scale"], name="scale"); psh, _ = A.place(inp["shift"], name="shift"); ms = D
        A.arm()
        if presum_n:
            pps, _ = A.place(inp["presum"], name="presum"); A.arm()
            hip._check(hip.lib.ltx_op_rownorm_presum(px, py, rows, D, NK.EPS_NORM, pw, psc, psh, rpb, ms, act, pps, presum_n, dtc(hip, dt), stream(hip)))
        else:
            hip._check(hip.lib.ltx_op_rownorm(px, py, rows, D, kind, NK.EPS_NORM, pw, psc, psh, rpb, ms, act, dtc(hip, dt), stream(hip)))
        st["check"] = lambda o: NK.assert_close(o["y"], NK.rownorm_formula(c, inp), c["dtype"], NK.FLOOR["presum" if presum_n else "rownorm"], name)
        return {"y": y}
    return fn


# (rows, D) of test_gpu_norm_kernels.py's tables, rows cut to the smallest that leave a partial block / wave on the same route
for _dt in (BF16, F32):
    rownorm_case("narrow", _dt, 2048 + 5 if _dt == BF16 else 4096 + 2, 512 if _dt == BF16 else 128, 0, False, True, act=1)
    rownorm_case("narrow", _dt, 2048 + 5 if _dt == BF16 else 4096 + 2, 512 if _dt == BF16 else 128, 1, True, True, wide_mod=True)
    rownorm_case("wide", _dt, 513, 2048, 0, False, True, wide_mod=True)
    rownorm_case("wide", _dt, 513, 2048, 1, True, False)
    rownorm_case("block", _dt, 3, 1536 if _dt == BF16 else 2048, 0, True, True, act=1)
    rownorm_case("block", _dt, 3, 1536 if _dt == BF16 else 2048, 1, False, True, wide_mod=True)
rownorm_case("reread", BF16, 9, 4104, 0, False, False)
rownorm_case("reread", BF16, 9, 4104, 1, True, True, wide_mod=True)
rownorm_case("reread", F32, 3, 2052, 1, False, True)
rownorm_case("presum", BF16, 37, 256, 0, True, True, act=1, presum_n=8)
rownorm_case("presum", F32, 10, 1024, 0, False, True, wide_mod=True, presum_n=8)
rownorm_case("presum", BF16, 37, 256, 0, False, True, presum_n=8)
rownorm_case("presum", BF16, 4 * 6 + 3, 2048, 0, True, True, act=1, wide_mod=True, presum_n=16)
rownorm_case("presum", BF16, 27, 2048, 0, False, False, presum_n=16)
rownorm_case("presum", BF16, 37, 256, 0, True, True, act=1, presum_n=32)
rownorm_case("presum", BF16, 13, 1024, 0, False, True, wide_mod=True, presum_n=4)
rownorm_case("presum", F32, 10, 1024, 0, True, True, act=1, presum_n=8)
for _rows, _D in ((32, 512), (16, 1024), (8, 2048)):
    rownorm_case("presum_lean", BF16, _rows, _D, 0, False, True, presum_n=_D // 128)


def qknorm_case(route, dt, rows, D, layout, segs):
    @case(f"qknorm_rope{'_segs' if segs else ''} {route} {'bf16' if dt == BF16 else 'f32'} {rows}x{D} {layout}")
    def fn(hip, A, st):
        """in place on q (and k) of one q | k | v row (fused, ld = 3 D) or on ld = D + 8; the rope tables end exactly at row `rows`"""
        g = gen(rows + D)
        c = dict(dtype="bf16" if dt == BF16 else "f32", rows=rows, D=D, cfg="x", rope=1)
        q, k, v = [NK._rows(g, rows, 1, D).to(dt) for _ in range(3)]
        w0, w1 = (1 + 0.5 * torch.randn(D, generator=g)).to(dt), (1 + 0.5 * torch.randn(D, generator=g)).to(dt)
        ang = torch.rand(rows, D // 2, generator=g, dtype=torch.float64) * (2 * math.pi)
        cos, sin = torch.cos(ang).float(), torch.sin(ang).float()
        routed(st, hip.ops.qknorm_route(rows, D, dt), route)
        if layout == "fused":
            (pq, qv), (_, kv), (_, vv) = A.place_fused([q, k, v], ["inout", "inout" if segs else "in", "in"], names=["q", "k", "v"]); ld = 3 * D
        else:
            pq, qv = A.place(q, ld=D + 8, role="inout", name="q"); ld = D + 8; kv = None
        pw0, _ = A.place(w0, name="w0"); pw1, _ = A.place(w1, name="w1"); pc, _ = A.place(cos, name="cos"); ps, _ = A.place(sin, name="sin")
        A.arm()
        two = segs and layout == "fused"
        if segs:
            hip._check(hip.lib.ltx_op_qknorm_rope_segs(pq, rows, D, ld, 2 if two else 1, 0, pw0, pw1 if two else None, None, NK.EPS_QK, pc, ps, 0.125 * LOG2E, dtc(hip, dt), stream(hip)))
        else:
            hip._check(hip.lib.ltx_op_qknorm_rope(pq, rows, D, ld, pw0, NK.EPS_QK, pc, ps, dtc(hip, dt), stream(hip)))

        def value(o):
            def formula(x, w, s):
                xd = x.double()
                y = xd / torch.sqrt((xd * xd).sum(-1, keepdim=True) / D + NK.EPS_QK) * w.double()
                re, im = y[:, 0::2], y[:, 1::2]
                return torch.stack((re * cos.double() - im * sin.double(), im * cos.double() + re * sin.double()), dim=-1).reshape(x.shape) * s
            NK.assert_close(o["q"], formula(q, w0, 0.125 * LOG2E if segs else 1.0), c["dtype"], NK.FLOOR["qknorm"], "q")
            if two:
                NK.assert_close(o["k"], formula(k, w1, 1.0), c["dtype"], NK.FLOOR["qknorm"], "k")
        st["check"] = value
        return {"q": qv, "k": kv} if two else {"q": qv}
    return fn


for _route, _dt, _rows, _D in (("fused4", BF16, 130, 128), ("fused8", BF16, 513, 2056), ("block", BF16, 3, 520), ("reread", BF16, 6, 4104), ("cached", F32, 9, 72)):
    for _layout in ("fused", "padded"):
        qknorm_case(_route, _dt, _rows, _D, _layout, False)
        qknorm_case(_route, _dt, _rows, _D, _layout, True)


def simple(name, capacity=48 << 20, **opts):
    """a case of an entry without a decision step"""
    def deco(fn):
        def wrapped(hip, A, st):
            st["no_route"] = "the entry has one kernel and no decision step"
            return fn(hip, A, st)
        return case(name, capacity, **opts)(wrapped)
    return deco


@simple("quant_rows_i8 (37 x 144) fused and padded")
def _quant_rows(hip, A, st):
    rows, D = 37, 144
    g = gen(7)
    x, x2, other = randn(g, rows, D), randn(g, rows, D), randn(g, rows, 64)
    x[1] = 0
    px, xv = A.place(x, ld=D + 8, name="x")
    (_, _), (px2, x2v) = A.place_fused([other, x2], ["in", "in"], names=["left", "x2"])
    pq, q = A.place(torch.empty(rows, D, dtype=torch.int8), role="out", name="q"); ps, s = A.place(torch.empty(1, rows, dtype=F32), role="out", name="scale")
    pq2, q2 = A.place(torch.empty(rows, D, dtype=torch.int8), role="out", name="q2"); ps2, s2 = A.place(torch.empty(1, rows, dtype=F32), role="out", name="scale2")
    A.arm()
    hip._check(hip.lib.ltx_op_quant_rows_i8(px, rows, D, D + 8, pq, ps, stream(hip)))
    hip._check(hip.lib.ltx_op_quant_rows_i8(px2, rows, D, D + 64, pq2, ps2, stream(hip)))

    def value(o):
        for a, qq, ss in ((x, "q", "scale"), (x2, "q2", "scale2")):
            qr, sr = R.quant_rows(a)
            assert torch.equal(o[qq], qr) and torch.equal(o[ss].reshape(-1), sr)                # bit for bit (test_gpu_int8)
    st["check"] = value
    return {"q": q, "scale": s, "q2": q2, "scale2": s2}


@simple("rownorm_quant_i8 (40 x 256, ld > D, table slices)")
def _rownorm_quant(hip, A, st):
    rows, D, rpb = 40, 256, 20
    g = gen(9)
    h = randn(g, rows, D, scale=3.0); shift, scale = randn(g, 2, D, dt=F32), randn(g, 2, D, scale=0.3, dt=F32)
    ph, _ = A.place(h, ld=D + 8, name="h")
    (psh, _), (psc, _) = A.place_fused([shift, scale], ["in", "in"], pad=8, names=["shift", "scale"])
    pq, q = A.place(torch.empty(rows, D, dtype=torch.int8), role="out", name="q"); ps, s = A.place(torch.empty(1, rows, dtype=F32), role="out", name="row_scale")
    A.arm()
    hip._check(hip.lib.ltx_op_rownorm_quant_i8(ph, rows, D, D + 8, 1e-6, psh, psc, 2 * D + 8, rpb, pq, ps, stream(hip)))

    def value(o):                                                                               # test_gpu_int8's bar
        n, gn = R.rownorm64(h, shift, scale, rpb, 1e-6)
        amax = n.abs().amax(-1); sd = o["row_scale"].reshape(-1).double()
        err = (o["q"].double() * sd[:, None] - n).abs()
        assert bool((err <= sd[:, None] / 2 + gn + 4 * R.U * amax[:, None]).all())
        assert bool(((sd - amax / 127).abs() <= (gn.amax(-1) + 2 * R.U * amax) / 127).all())
    st["check"] = value
    return {"q": q, "row_scale": s}


@simple("cast_fp8 (37 x 144, ld > D) and widen_fp8 (n = 763)")
def _fp8(hip, A, st):
    rows, D = 37, 144
    x = randn(gen(3), rows, D, scale=20.0)
    codes = torch.arange(256, dtype=torch.uint8).repeat(3)[:-5]
    px, _ = A.place(x, ld=D + 8, name="x"); pq, q = A.place(torch.empty(rows, D, dtype=torch.uint8).view(F.F8), role="out", name="q")
    pc, _ = A.place(codes.view(F.F8), name="codes")
    pyb, yb = A.place(torch.empty(1, 763, dtype=BF16), role="out", name="wide_bf16"); pyf, yf = A.place(torch.empty(1, 763, dtype=F32), role="out", name="wide_f32")
    A.arm()
    hip._check(hip.lib.ltx_op_cast_fp8(px, rows, D, D + 8, pq, stream(hip)))
    hip._check(hip.lib.ltx_op_widen_fp8(pc, 763, 1, pyb, stream(hip)))
    hip._check(hip.lib.ltx_op_widen_fp8(pc, 763, 0, pyf, stream(hip)))
    st["finite"] = False                                                                        # the NaN codes widen to NaN: by contract

    def value(o):                                                                               # bit-equal to tests/fp8_ref.py (test_gpu_fp8)
        assert torch.equal(F.codes(o["q"]), F.codes(F.cast(x)))
        for k, dt in (("wide_bf16", BF16), ("wide_f32", F32)):
            ref = codes.view(F.F8).to(dt); y = o[k].reshape(-1); fin = ~torch.isnan(ref.float())
            assert torch.equal(y[fin], ref[fin]) and bool(torch.isnan(y[~fin].float()).all())
    st["check"] = value
    return {"q": q, "wide_bf16": yb, "wide_f32": yf}


@simple("mod_scale (B 2 x 19 rows, D 136, scale stride > D) and scale_cols (37 x 136)")
def _mod_scale(hip, A, st):
    import fold_ref
    B, rpb, D = 2, 19, 136
    g = gen(4)
    h, scale = randn(g, B * rpb, D), randn(g, B, D, scale=0.3, dt=F32)
    w, sc1 = randn(g, 37, D), randn(g, 1, D, scale=0.3, dt=F32)
    ph, _ = A.place(h, name="h"); ps, _ = A.place(scale, ld=D + 8, name="scale"); py, y = A.place(torch.empty(B * rpb, D, dtype=BF16), role="out", name="y")
    pw, _ = A.place(w, name="w"); ps1, _ = A.place(sc1, name="scale_cols.scale"); po, out = A.place(torch.empty(37, D, dtype=BF16), role="out", name="out")
    A.arm()
    hip._check(hip.lib.ltx_op_mod_scale(ph, ps, D + 8, py, B, rpb, D, 1, stream(hip)))
    hip._check(hip.lib.ltx_op_scale_cols(pw, ps1, po, 37, D, 1, stream(hip)))

    def value(o):                                                                               # bit-equal to tests/fold_ref.py (test_gpu_fold_ops)
        assert torch.equal(o["y"], fold_ref.mod_scale_ref(h, scale, rpb)) and torch.equal(o["out"], fold_ref.scale_cols_ref(w, sc1[0]))
    st["check"] = value
    return {"y": y, "out": out}


@simple("stg_fill (B 2, S 19, D 136, ldd and lds > D)")
def _stg_fill(hip, A, st):
    import ctypes as C
    B, S, D = 2, 19, 136
    g = gen(5)
    dst, src, q, k = randn(g, B * S, D), randn(g, B * S, D), randn(g, B * S, D), randn(g, B * S, D)
    (_, _), (_, _), (pd, dv) = A.place_fused([q, k, dst], ["in", "in", "inout"], names=["q", "k", "dst"])       # the v segment of q | k | v
    ps, _ = A.place(src, ld=D + 8, name="src")
    A.arm()
    hip._check(hip.lib.ltx_op_stg_fill(pd, 3 * D, ps, D + 8, (C.c_ubyte * 2)(0, 1), B, S, D, 1, stream(hip)))
    st["check"] = lambda o: (assert_equal(o["dst"][:S], dst[:S]), assert_equal(o["dst"][S:], src[S:]))
    return {"dst": dv}


def assert_equal(a, b):
    assert E.same_bits(a.contiguous(), b.contiguous())


@simple("step_residual (105 x 136) bf16 and f32")
def _step_residual(hip, A, st):
    g = gen(5)
    outs = {}
    wants = {}
    calls = []
    for dt, nm in ((BF16, "bf16"), (F32, "f32")):
        h, r = randn(g, 105, 136, dt=dt), randn(g, 105, 136, dt=dt)
        ph, _ = A.place(h, name="h " + nm); pr, rv = A.place(r, role="inout", name="r " + nm)
        outs[nm] = rv; wants[nm] = (h.float() - r.float()).to(dt)
        calls.append((ph, pr, dtc(hip, dt)))
    A.arm()
    for ph, pr, d in calls:
        hip._check(hip.lib.ltx_op_step_residual(ph, pr, 105, 136, d, stream(hip)))
    st["check"] = lambda o: [assert_equal(o[k], wants[k]) for k in wants]
    return outs


@simple("step_measure (B 2 x 21 rows, D 256, table slices, workspace in the arena)")
def _step_measure(hip, A, st):
    import step_cache_ref as SC
    rows, D, rpb = 42, 256, 21
    g = gen(6)
    h, prev = randn(g, rows, D), randn(g, rows, D)
    shift, scale = randn(g, 2, D, dt=F32), randn(g, 2, D, scale=0.3, dt=F32)
    nws = max(int(hip.lib.ltx_op_step_measure_ws_bytes(rows, D, 1)), 16)
    ph, _ = A.place(h, name="h"); pp, pv = A.place(prev, role="inout", name="prev")
    (psh, _), (psc, _) = A.place_fused([shift, scale], ["in", "in"], pad=8, names=["shift", "scale"])
    pws, _ = A.place(torch.zeros(1, nws, dtype=torch.uint8), role="inout", name="ws"); psum, sums = A.place(torch.empty(1, 2, dtype=torch.float64), role="out", name="sums")
    A.arm()
    hip._check(hip.lib.ltx_op_step_measure(ph, pp, psh, psc, 2 * D + 8, rows, D, rpb, 1e-6, 1, 0, pws, psum, stream(hip)))

    def value(o):                                                                               # test_gpu_step_cache's bounds
        c = dict(presum_n=0, kind=0, rpb=rpb, act=0)
        m = NK.rownorm_formula(c, dict(x=h, weight=None, scale=scale, shift=shift, presum=None))
        NK.assert_close(o["prev"], m, "bf16", NK.FLOOR["rownorm"], "step_measure m")
        md = o["prev"].double()
        bound = 4 * 2.0 ** -8 * float(md.abs().sum())
        assert abs(float(o["sums"][0, 0]) - float((md - prev.double()).abs().sum())) <= bound
        assert abs(float(o["sums"][0, 1]) - float(prev.double().abs().sum())) <= bound
    st["check"] = value
    return {"prev": pv, "sums": sums}


@simple("timestep_embedding (n 3, both flavours) and blend (dim 2, 3, 4)")
def _embed_blend(hip, A, st):
    import ctypes as C
    ts, tv = [1000.0, 500.0, 0.05], [0.05, 0.025, 1.0]
    pe, e0 = A.place(torch.empty(3, 256, dtype=F32), role="out", name="dit embedding"); pv, e1 = A.place(torch.empty(3, 256, dtype=BF16), role="out", name="vae embedding")
    g = gen(8)
    a = torch.randn(6, 3, 5, 7, generator=g); bs = [torch.randn(6, 3, 5, 7, generator=g) for _ in range(3)]
    pa, _ = A.place(a.reshape(6 * 3 * 5, 7), name="a")
    pbs = [A.place(b.reshape(6 * 3 * 5, 7), role="inout", name=f"b dim {d}") for d, b in zip((2, 3, 4), bs)]
    A.arm()
    hip._check(hip.lib.ltx_op_timestep_embedding((C.c_float * 3)(*ts), 3, 0, 1.0, 0, pe, stream(hip)))
    hip._check(hip.lib.ltx_op_timestep_embedding((C.c_float * 3)(*tv), 3, 1, 1000.0, 1, pv, stream(hip)))
    for d, (pb, _) in zip((2, 3, 4), pbs):
        hip._check(hip.lib.ltx_op_blend(pa, pb, 6, 3, 5, 7, 3, 5, 7, d, 2, stream(hip)))

    def value(o):                                                                               # test_gpu_ops' bars
        t = torch.tensor(ts)
        assert (o["dit"] - O.get_timestep_embedding(t)).abs().max() <= 2e-4
        tb = torch.tensor(tv).bfloat16()
        want_b = O.vae_timestep_embedding((tb * torch.tensor(1000.0).bfloat16()).float()).bfloat16()
        assert (o["vae"].float() - want_b.float()).abs().max() <= 2 ** -7
        for d, b in zip((2, 3, 4), bs):
            assert (o[f"b{d}"].view(1, 6, 3, 5, 7) - O._blend(a[None], b[None], 2, d)).abs().max() < 1e-6
    st["check"] = value
    return dict({"dit": e0, "vae": e1}, **{f"b{d}": v for d, (_, v) in zip((2, 3, 4), pbs)})


# ================================================================== attention
XKV = 128          # the short-key-set kernel holds at most 128 keys (csrc/attention.hip)


def attention_path(hd, Sk, dt, prescaled, off, ldo):
    """the dispatch of ltx_launch_attention (csrc/attention.hip) restated: which kernel a case is MEANT to reach"""
    off = set((off or "").split("+"))
    if dt == F32:
        return "f32"
    if hd == 64 and Sk <= XKV and "cross" not in off:
        return "cross64"
    if prescaled and hd == 64:
        return "q64" if "q64" not in off else ("pipe64" if "pipe" not in off else "generic")
    if prescaled and hd == 128:                                      # ltx_attention_q128_fits: Sk >= 128, ldo % 8 == 0
        return "q128" if ("q128" not in off and Sk >= 128 and ldo % 8 == 0) else "generic"
    return "generic"


def attention_case(name, hd, heads, Sq, Sk, path, dt=BF16, biased=False, layout="fused", ldo_extra=0, prescaled=False, **opts):
    """q | k | v as column slices of one buffer (Sq == Sk) or each on ld = D + 8; o a column slice of a wider buffer whose ldo % 8 is
    0 (ldo_extra 0: D + 8) or 4 (ldo_extra 4: D + 12, the narrow-store path: wide_o is decided from ldo).
    path: the kernel the case is meant for.  Evidence asserted per case: one launch counted in the profiler's attention class (self
    where Sq == Sk and no bias, else cross), and the exact-max counters of ltx_attention_fallback_counts - only the q64 loop raises
    counts[0], only the exact pass gated behind the q128 loop raises counts[1], and a prescaled case's late key 16 x the query forces
    that overflow: "q64" wants counts[0] > 0, "q128" counts == (0, 1), every other path (0, 0).  The pipe64, generic, cross64 and f32
    kernels have no counter of their own: for them the restated dispatch above and the zero counters are what can be asserted."""
    @case(name + f" -> {path}", **opts)
    def fn(hip, A, st):
        B, D = 2, hd * heads
        ldo = D + 8 + ldo_extra
        assert attention_path(hd, Sk, dt, prescaled, opts.get("attn_off"), ldo) == path, name
        g = gen(hd + Sq + Sk)
        q, k, v = randn(g, B, Sq, D, dt=dt), randn(g, B, Sk, D, dt=dt), randn(g, B, Sk, D, dt=dt)
        k[0, Sk - 3] = (q[0, 5].float() * (16.0 if prescaled else 6.0)).to(dt)                  # a late dominant key in the ragged last tile
        sc = hd ** -0.5
        if prescaled:
            q = (q.float() * (sc * LOG2E)).to(dt)
        bias = None
        if biased:
            bias = torch.zeros(B, Sk); bias[:, Sk // 3 + 1:] = -10000.0; bias[0, 0] = -1.5
        if layout == "fused" and Sq == Sk:
            (pq, _), (pk, _), (pv, _) = A.place_fused([q, k, v], ["in"] * 3, names=["q", "k", "v"]); ldq = ldk = ldv = 3 * D
        elif layout == "fused":
            pq, _ = A.place(q, name="q"); (pk, _), (pv, _) = A.place_fused([k, v], ["in"] * 2, names=["k", "v"]); ldq, ldk, ldv = D, 2 * D, 2 * D
        else:
            pq, _ = A.place(q, ld=D + 8, name="q"); pk, _ = A.place(k, ld=D + 8, name="k"); pv, _ = A.place(v, ld=D + 8, name="v"); ldq = ldk = ldv = D + 8
        left = torch.zeros(B * Sq, 8 + ldo_extra, dtype=dt)
        (po, ov), (_, _) = A.place_fused([torch.empty(B * Sq, D, dtype=dt), left], ["out", "in"], names=["o", "beside o"])
        pb = A.place(bias, name="key_bias")[0] if biased else None
        A.arm()
        hip.attention_fallback_counts(reset=True)
        hip.prof_enable(True)
        try:
            if prescaled:
                hip._check(hip.lib.ltx_op_attention_prescaled(pq, pk, pv, po, B, Sq, Sk, heads, hd, ldq, ldk, ldv, ldo, stream(hip)))
            else:
                hip._check(hip.lib.ltx_op_attention(pq, pk, pv, po, B, Sq, Sk, heads, hd, ldq, ldk, ldv, ldo, sc, pb, dtc(hip, dt), stream(hip)))
            torch.cuda.synchronize()
            launches = (hip.prof_report(2)[2], hip.prof_report(3)[2])
        finally:
            hip.prof_enable(False)
        fb = tuple(hip.attention_fallback_counts())
        st["note"] = f"attention launches (self, cross) {launches}, exact-max counters {fb}"
        assert launches == ((0, 1) if biased or Sq != Sk else (1, 0)), (name, launches)
        if path == "q64":
            assert fb[0] > 0 and fb[1] == 0, (name, fb)
        else:
            assert fb == ((0, 1) if path == "q128" else (0, 0)), (name, path, fb)
        st["routed"] = True
        ref = ref_attention(q, k, v, heads, math.log(2.0) if prescaled else sc, bias)
        st["check"] = lambda o: check(o["o"].view(B, Sq, D), ref, dt)
        return {"o": ov}
    return fn


for _hd in (16, 32, 64, 128):
    for _Sq in (200, 70):
        attention_case(f"attention bf16 hd{_hd} ({_Sq}, 333) fused ldo%8=0", _hd, 2, _Sq, 333, "generic")
        attention_case(f"attention bf16 hd{_hd} ({_Sq}, 333) padded ldo%8=4", _hd, 2, _Sq, 333, "generic", layout="padded", ldo_extra=4)
for _Sq in (200, 70):
    attention_case(f"attention f32 hd64 ({_Sq}, 333) fused", 64, 2, _Sq, 333, "f32", dt=F32)
    attention_case(f"attention f32 hd64 ({_Sq}, 333) padded ldo%8=4", 64, 2, _Sq, 333, "f32", dt=F32, layout="padded", ldo_extra=4)
attention_case("attention bf16 hd64 self (333, 333) q|k|v slices", 64, 2, 333, 333, "generic")
for _Sk in (10, 100, 128):
    attention_case(f"attention short keys Sk {_Sk} with a key bias fused", 64, 3, 70, _Sk, "cross64", biased=True)
    attention_case(f"attention short keys Sk {_Sk} with a key bias padded ldo%8=4", 64, 3, 70, _Sk, "cross64", biased=True, layout="padded", ldo_extra=4)
# attention_prescaled at the smallest shape each loop is given, plus a ragged last tile on both axes.  head_dim 64: the dispatch hands
# Sk <= 128 to the short-key-set kernel and ltx_attention_q64_fits bounds only the 2^31 offsets, so the q64 loop's floor is Sk = 129;
# head_dim 128: ltx_attention_q128_fits wants Sk >= 128 (two key tiles).  Sk = 128 + 5 serves both: two full 64-key tiles and five
# keys; Sq = 64 + 6 leaves a ragged query tile under the 64- and the 128-row tiles.  The q128 predicate also wants ldo % 8 == 0:
# the ldo % 8 == 4 case of head_dim 128 is MEANT to miss the loop and is named "generic"
for _hd, _arms in ((64, ((None, "q64"), ("q64", "pipe64"), ("pipe+q64", "generic"))), (128, ((None, "q128"), ("q128", "generic")))):
    for _off, _path in _arms:
        _o = {} if _off is None else {"attn_off": _off}
        attention_case(f"attention_prescaled hd{_hd} (70, 133) fused attn_off={_off}", _hd, 2, 70, 133, _path, prescaled=True, **_o)
        attention_case(f"attention_prescaled hd{_hd} (133, 133) q|k|v slices attn_off={_off}", _hd, 2, 133, 133, _path, prescaled=True, **_o)
        attention_case(f"attention_prescaled hd{_hd} (70, 133) padded ldo%8=4 attn_off={_off}", _hd, 2, 70, 133, "generic" if _hd == 128 else _path, prescaled=True,
                       layout="padded", ldo_extra=4, **_o)


@simple("kmean and quant_qk_i8 (B 2, Sq 100, Sk 100, hd 64) on q | k | v slices")
def _quant_qk(hip, A, st):
    B, Sq, Sk, heads, hd = 2, 100, 100, 2, 64
    D = heads * hd
    g = gen(13)
    q, k, v = randn(g, B, Sq, D), randn(g, B, Sk, D) + 1.0, randn(g, B, Sk, D)
    (pq, _), (pk, _), (_, _) = A.place_fused([q, k, v], ["in"] * 3, names=["q", "k", "v"])
    pm, mean = A.place(torch.empty(B, D, dtype=F32), role="out", name="mean")
    pq8, q8 = A.place(torch.empty(B * Sq, D, dtype=torch.int8), role="out", name="q8"); pk8, k8 = A.place(torch.empty(B * Sk, D, dtype=torch.int8), role="out", name="k8")
    pqs, qs = A.place(torch.empty(B * heads, Sq, dtype=F32), role="out", name="qs"); pks, ks = A.place(torch.empty(B * heads, (Sk + 63) // 64, dtype=F32), role="out", name="ks")
    A.arm()
    hip._check(hip.lib.ltx_op_kmean(pk, B, Sk, D, 3 * D, pm, stream(hip)))
    hip._check(hip.lib.ltx_op_quant_qk_i8(pq, pk, pm, B, Sq, Sk, heads, hd, 3 * D, 3 * D, pq8, pqs, pk8, pks, stream(hip)))

    def value(o):                                                                               # test_gpu_int8_attn: the sum bound; bit for bit
        err = (o["mean"].double() - A8.kmean64(k)).abs()
        assert bool((err <= Sk * 2.0 ** -24 * k.double().abs().amax(1)).all())
        want = A8.quant_qk(q, k, o["mean"], heads)
        got = (o["q8"].view(B, Sq, D), o["qs"].view(B, heads, Sq), o["k8"].view(B, Sk, D), o["ks"].view(B, heads, -1))
        for nm, a, b in zip(("q8", "qs", "k8", "ks"), got, want):
            assert a.shape == b.shape and torch.equal(a, b.cpu()), nm
    st["check"] = value
    return {"mean": mean, "q8": q8, "qs": qs, "k8": k8, "ks": ks}


def cross_case(kind, layout):
    """the short-key-set kernel's three other entries (bf16, head_dim 64, Sk <= 128, a scattered key bias, B = 2 with different counts)"""
    @simple(f"{kind} (B 2, Sq 70, Sk 100) {layout}")
    def fn(hip, A, st):
        import lora_ref
        B, Sq, Sk, heads, hd = 2, 70, 100, 8, 64                                                # D = 512: four row partials, the fewest the kernel takes
        D = heads * hd
        g = gen(21)
        q, k, v = randn(g, B, Sq, D, scale=1.7), randn(g, B, Sk, D), randn(g, B, Sk, D)
        bias = torch.full((B, Sk), -10000.0)
        kept = [torch.arange(0, Sk, 3), torch.arange(1, Sk, 7)]                                 # 34 and 15 keys kept: KP = 64
        for b in range(B):
            bias[b, kept[b]] = 0.0
        bias[0, 3] = -2.5
        counts = [len(kept[0]), len(kept[1])]
        KP = hip.ops.xattn_fold_kp(counts)
        xd = q.double().view(B * Sq, D)
        rs = (xd * xd).view(B * Sq, 4, 128).sum(-1).float()
        rinv = 1.0 / torch.sqrt(xd.pow(2).sum(-1, keepdim=True) / D + 1e-5)
        with_rs = kind != "attention_compact"
        if layout == "fused":
            pq, _ = A.place(q, name="q"); (pk, _), (pv, _) = A.place_fused([k, v], ["in"] * 2, names=["k", "v"]); ldq, ldk, ldv = D, 2 * D, 2 * D
        elif layout == "padded q, dense k and v":
            pq, _ = A.place(q, ld=D + 8, name="q"); pk, _ = A.place(k, name="k"); pv, _ = A.place(v, name="v"); ldq, ldk, ldv = D + 8, D, D
        else:
            pq, _ = A.place(q, ld=D + 8, name="q"); pk, _ = A.place(k, ld=D + 8, name="k"); pv, _ = A.place(v, ld=D + 8, name="v"); ldq = ldk = ldv = D + 8
        pb, _ = A.place(bias, name="key_bias"); prs, _ = A.place(rs, name="q_rowsq")
        pcnt, cnt = A.place(torch.empty(1, B, dtype=torch.int32), role="out", name="counts_out") if kind != "attention_rowsq" else (None, None)
        sc = 0.125
        qn = (q.double() * rinv.view(B, Sq, 1)) if with_rs else q.double()
        ref = ref_attention(qn.float(), k, v, heads, sc, bias)
        if kind == "attention_probs":
            pk, _ = A.place(k, name="k dense")                                                  # the entry takes no strides: dense q and k
            pp, p = A.place(torch.empty(B * Sq, heads * KP, dtype=BF16), role="out", name="p")
            A.arm()
            hip._check(hip.lib.ltx_op_attention_probs(pq, pk, pp, B, Sq, Sk, heads, KP, sc, pb, prs, 4, 1e-5, pcnt, stream(hip)))

            def value(o):                                                                       # test_gpu_xattn_fold_vo's bar
                assert o["counts"].reshape(-1).tolist() == counts
                pd = o["p"].double().view(B, Sq, heads, KP)
                for b, c in enumerate(counts):
                    qh = qn[b].view(Sq, heads, 64); kh = k[b, kept[b]].double().view(c, heads, 64)
                    s = torch.einsum("shd,khd->shk", qh, kh) * sc
                    if b == 0:
                        s[:, :, 1] -= 2.5                                                       # key 3 is the second kept key of row 0
                    Eref = torch.softmax(s, -1)
                    ds = 68 * 2.0 ** -24 * sc * LOG2E * float(torch.einsum("shd,khd->shk", qh.abs(), kh.abs()).max())
                    got = pd[b, :, :, :c]
                    bar = 0.5 * torch.maximum(lora_ref.ulp_bf16(Eref), lora_ref.ulp_bf16(got)) + Eref * (2 * ds + 2.0 ** -20)
                    assert int(((got - Eref).abs() > bar).sum()) == 0, (b, float(((got - Eref).abs() / bar.clamp_min(1e-300)).max()))
                    assert torch.count_nonzero(pd[b, :, :, c:]) == 0, "the KP padding columns are exact zeros"
            st["check"] = value
            return {"p": p, "counts": cnt}
        (po, ov), (_, _) = A.place_fused([torch.empty(B * Sq, D, dtype=BF16), torch.zeros(B * Sq, 8, dtype=BF16)], ["out", "in"], names=["o", "beside o"])
        A.arm()
        if kind == "attention_compact" and ldk != D:                                            # REFUSAL: the entry demands dense k / v rows (it compacts them)
            with pytest.raises(hip.LtxError, match="dense k / v rows"):
                hip._check(hip.lib.ltx_op_attention_compact(pq, pk, pv, po, B, Sq, Sk, heads, hd, ldq, ldk, ldv, D + 8, sc, pb, None, 0, D, 1e-5, pcnt, stream(hip)))
            A.refused = True
            st["check"] = lambda o: None
            return {}
        if kind == "attention_rowsq":
            hip._check(hip.lib.ltx_op_attention_rowsq(pq, pk, pv, po, B, Sq, Sk, heads, hd, ldq, ldk, ldv, D + 8, sc, pb, prs, 4, D, 1e-5, stream(hip)))
        else:
            hip._check(hip.lib.ltx_op_attention_compact(pq, pk, pv, po, B, Sq, Sk, heads, hd, ldq, ldk, ldv, D + 8, sc, pb, None, 0, D, 1e-5, pcnt, stream(hip)))

        def value(o):                                                                           # test_gpu_xattn_compact / test_gpu_q2fold: rel-L2 <= 5e-3
            e = rel_l2(o["o"].float().view(B, Sq, D), ref)
            assert e <= 5e-3, e
            if kind == "attention_compact":
                assert o["counts"].reshape(-1).tolist() == counts
        st["check"] = value
        return {"o": ov, "counts": cnt} if kind == "attention_compact" else {"o": ov}
    return fn


for _layout in ("fused", "padded"):
    cross_case("attention_rowsq", _layout)
cross_case("attention_compact", "padded q, dense k and v")
cross_case("attention_compact", "fused")                  # refused: asserted as a refusal
cross_case("attention_probs", "fused")


@simple("attention_i8 (B 2, Sq 70, Sk 100, hd 64), v a slice of k | v, o beside other columns")
def _attention_i8(hip, A, st):
    from test_gpu_int8_attn import TOL
    B, Sq, Sk, heads, hd = 2, 70, 100, 2, 64
    D = heads * hd
    g = gen(23)
    q, k, v = randn(g, B, Sq, D, scale=0.4), randn(g, B, Sk, D), randn(g, B, Sk, D)
    q8, qs, k8, ks = A8.quant_qk(q, k, A8.kmean64(k).float(), heads)
    pq8, _ = A.place(q8, name="q8"); pqs, _ = A.place(qs.reshape(B * heads, Sq), name="qs"); pk8, _ = A.place(k8, name="k8"); pks, _ = A.place(ks.reshape(B * heads, -1), name="ks")
    (_, _), (pv, _) = A.place_fused([k, v], ["in"] * 2, names=["k", "v"])
    (po, ov), (_, _) = A.place_fused([torch.empty(B * Sq, D, dtype=BF16), torch.zeros(B * Sq, 12, dtype=BF16)], ["out", "in"], names=["o", "beside o"])      # ldo % 8 == 4
    A.arm()
    hip._check(hip.lib.ltx_op_attention_i8(pq8, pqs, pk8, pks, pv, po, B, Sq, Sk, heads, hd, 2 * D, D + 12, stream(hip)))
    want = A8.attention64(q8, qs, k8, ks, v, heads).float()

    def value(o):
        e = rel_l2(o["o"].float().view(B, Sq, D), want)
        assert e <= TOL, e
    st["check"] = value
    return {"o": ov}


# ================================================================== block-sparse attention and its device-built maps
def sparse_qkv(g, B, Sq, Sk, D, hd):
    return randn(g, B, Sq, D, scale=3.0 * LOG2E * hd ** -0.5), randn(g, B, Sk, D), randn(g, B, Sk, D)


def sparse_attention_case(hd):
    @simple(f"attention_sparse hd{hd} (B 2, Sq 200, Sk 300, heads 3) per-head map, k | v slices, o on ld = D + 8 and D + 4")
    def fn(hip, A, st):
        """key tile 3 is in no row of any head: its k and v rows are operands the kernel must not need.  o is stored twice: beside
        eight other columns (16-byte stores) and beside four (ldo % 8 == 4: the 8-byte stores)"""
        import sparse_attn_ref as SP
        from test_gpu_int8_attn import TOL
        from test_gpu_sparse_attn import random_bits
        B, Sq, Sk, heads = 2, 200, 300, 3
        D = heads * hd
        q, k, v = sparse_qkv(gen(31 + hd), B, Sq, Sk, D, hd)
        bits = random_bits((heads, 2, 5), 6)
        bits[:, 0, 3] = bits[:, 1, 3] = False
        assert bool(bits.any(-1).all()) and not bool(bits[..., 3].any())
        map = SP.pack(bits)
        pq, _ = A.place(q, name="q"); (pk, _), (pv, _) = A.place_fused([k, v], ["in"] * 2, names=["k", "v"])
        pm, _ = A.place(map.view(1, -1), name="map")
        outs = {}
        calls = []
        for extra in (8, 4):
            (po, ov), (_, _) = A.place_fused([torch.empty(B * Sq, D, dtype=BF16), torch.zeros(B * Sq, extra, dtype=BF16)], ["out", "in"], names=[f"o ld D+{extra}", "beside o"])
            outs[f"o{extra}"] = ov; calls.append((po, D + extra))
        A.arm()
        for po, ldo in calls:
            hip._check(hip.lib.ltx_op_attention_sparse(pq, pk, pv, po, pm, heads, B, Sq, Sk, heads, hd, D, 2 * D, 2 * D, ldo, stream(hip)))
        ref = SP.attention64(q, k, v, map, heads).float()

        def value(o):                                                                           # test_gpu_sparse_attn's bar
            assert E.same_bits(o["o8"], o["o4"]), "the 8-byte stores differ from the 16-byte stores"
            e = rel_l2(o["o8"].float().view(B, Sq, D), ref)
            assert e <= TOL, e
        st["check"] = value
        return outs
    return fn


def sparse_batched_case(hd):
    @simple(f"attention_sparse_batched hd{hd} (B 2, S 300, heads 3) q | k | v slices, map_batch_stride > a row's map")
    def fn(hip, A, st):
        """the two batch rows' maps lie five filler words apart"""
        import sparse_attn_ref as SP
        from test_gpu_int8_attn import TOL
        from test_gpu_sparse_attn import random_bits
        B, S, heads = 2, 300, 3
        D = heads * hd
        q, k, v = sparse_qkv(gen(37 + hd), B, S, S, D, hd)
        bits = random_bits((B, heads, 3, 5), 7)
        map = SP.pack(bits)
        words = heads * 3
        assert not torch.equal(map[0], map[1])
        (pq, _), (pk, _), (pv, _) = A.place_fused([q, k, v], ["in"] * 3, names=["q", "k", "v"])
        pm, _ = A.place(map.view(B, words), ld=words + 5, name="maps")
        (po, ov), (_, _) = A.place_fused([torch.empty(B * S, D, dtype=BF16), torch.zeros(B * S, 8, dtype=BF16)], ["out", "in"], names=["o", "beside o"])
        A.arm()
        hip._check(hip.lib.ltx_op_attention_sparse_batched(pq, pk, pv, po, pm, heads, words + 5, B, S, S, heads, hd, 3 * D, 3 * D, 3 * D, D + 8, stream(hip)))
        ref = torch.cat([SP.attention64(q[b:b + 1], k[b:b + 1], v[b:b + 1], map[b], heads) for b in range(B)]).float()

        def value(o):
            e = rel_l2(o["o"].float().view(B, S, D), ref)
            assert e <= TOL, e
        st["check"] = value
        return {"o": ov}
    return fn


@simple("pool_qk (B 2, S 193, heads 9, hd 64) on q | k | v slices: 72 16-byte chunks a row, k's last beside v's first")
def _pool_qk(hip, A, st):
    import test_gpu_sparse_select as TSS
    B, S, heads, hd = 2, 193, 9, 64
    D = heads * hd
    g = gen(41)
    q, k, v = randn(g, B, S, D), randn(g, B, S, D), randn(g, B, S, D)
    (pq, _), (pk, _), (_, _) = A.place_fused([q, k, v], ["in"] * 3, names=["q", "k", "v"])
    pqb, qbar = A.place(torch.empty(B * heads * 2, hd, dtype=F32), role="out", name="qbar"); pkb, kbar = A.place(torch.empty(B * heads * 4, hd, dtype=F32), role="out", name="kbar")
    A.arm()
    hip._check(hip.lib.ltx_op_pool_qk(pq, pk, pqb, pkb, B, S, heads, hd, 3 * D, 3 * D, stream(hip)))
    st["check"] = lambda o: TSS.pooled_inside_the_bound(q, k, heads, o["qbar"].view(B, heads, 2, hd), o["kbar"].view(B, heads, 4, hd), st["name"])
    return {"qbar": qbar, "kbar": kbar}


def sparse_select_case(hd):
    @simple(f"sparse_select hd{hd} (B 2, 4097 tokens, heads 4) with a keep map: three words a row")
    def fn(hip, A, st):
        """65 tiles: NW = 3 is odd, so the last ballot of a row stores ONE word.  Every word and count written, nothing behind a row's
        third word.  The keep map holds tiles 0 and 32 in every row, so no map word can be the arena's never-written value (bit 31
        alone); word 2 holds bit 0 or nothing"""
        import sparse_attn_ref as SP
        import test_gpu_sparse_select as TSS
        S, (B, heads) = 4097, TSS.WIDE[4097]
        qbar, kbar = [x.cpu() for x in TSS.ranked_world(S, hd)]
        keep = torch.zeros(33, 65, dtype=torch.bool)
        keep[:, 0] = keep[:, 32] = keep[::4, 64] = True
        pqb, _ = A.place(qbar, name="qbar"); pkb, _ = A.place(kbar, name="kbar"); pkeep, _ = A.place(SP.pack(keep), name="keep")
        pm, map = A.place(torch.empty(B * heads * 33, 3, dtype=torch.int32), role="out", name="map")
        pc, count = A.place(torch.empty(1, B * heads * 33, dtype=torch.int32), role="out", name="count")
        A.arm()
        hip._check(hip.lib.ltx_op_sparse_select(pqb, pkb, pkeep, 1, pm, pc, B, S, heads, hd, 0.5, stream(hip)))
        st["check"] = lambda o: TSS.selection_matches(o["map"].view(B, heads, 33, 3), o["count"].view(B, heads, 33), qbar, kbar, S, 0.5, keep, st["name"])
        return {"map": map, "count": count}
    return fn


for _hd in (64, 128):
    sparse_attention_case(_hd)
    sparse_batched_case(_hd)
    sparse_select_case(_hd)


# ================================================================== convolutions (channels-last, B = 2)
def conv_case(name, Cin, Cout, fam, dt=BF16, causal=False, resid=False, kind="conv", T=2, H=5, W=6, **opts):
    @case(name, **opts)
    def fn(hip, A, st):
        B = 2
        g = gen(Cin + Cout + T)
        x, w, b = randn(g, B, Cin, T, H, W, dt=dt), randn(g, Cout, Cin, 3, 3, 3, scale=(27 * Cin) ** -0.5, dt=dt), randn(g, Cout, scale=0.1, dt=dt)
        r = randn(g, B, Cout, T, H, W, dt=dt)
        px, _ = A.place(cl(x).reshape(-1, Cin), name="x"); pw, _ = A.place(w.reshape(Cout, -1), name="w"); pb, _ = A.place(b, name="bias")
        pr = A.place(cl(r).reshape(-1, Cout), name="resid")[0] if resid else None
        epi = {"conv": 3 if resid else 0, "up": 4, "out": 5}[kind]
        route = hip.ops.gemm_route(B * T * H * W, Cout, Cin, 1, 27, B, T, H, W, epi=epi, dtype=dt)
        st["note"] = route
        routed(st, route if fam.startswith("halo:") else family(route), fam)
        ref = O.causal_conv3d(x.float(), w.float(), b.float(), causal)
        if kind == "conv":
            py, y = A.place(torch.empty(B * T * H * W, Cout, dtype=dt), role="out", name="y")
            call = lambda: hip.lib.ltx_op_conv3d(px, pw, pb, dtc(hip, dt), py, pr, B, T, H, W, Cin, Cout, int(causal), dtc(hip, dt), stream(hip))
            want = ref + (r.float() if resid else 0)
            st["check"] = lambda o: check(ncthw(o["y"].view(B, T, H, W, Cout)), want, dt)
        elif kind == "up":
            py, y = A.place(torch.empty(B * (2 * T - 1) * 2 * H * 2 * W, Cout // 8, dtype=dt), role="out", name="y")
            call = lambda: hip.lib.ltx_op_upsample3d(px, pw, pb, dtc(hip, dt), py, B, T, H, W, Cin, Cout, int(causal), 1, dtc(hip, dt), stream(hip))
            want = O.upsampler({"conv.conv.weight": w.float(), "conv.conv.bias": b.float()}, "", x.float(), Cout // 8, causal)
            st["check"] = lambda o: check(ncthw(o["y"].view(B, 2 * T - 1, 2 * H, 2 * W, Cout // 8)), want, dt)
        else:
            py, y = A.place(torch.empty(B * (Cout // 16) * T * 4 * H, 4 * W, dtype=F32), role="out", name="y")
            call = lambda: hip.lib.ltx_op_conv_out_unpatchify(px, pw, pb, dtc(hip, dt), py, B, T, H, W, Cin, Cout, int(causal), 0, dtc(hip, dt), stream(hip))
            want = O.unpatchify(ref, 4, 1)
            st["check"] = lambda o: check(o["y"].view(B, Cout // 16, T, 4 * H, 4 * W), want, dt)
        A.arm()
        launch(hip, st, KERNEL_OF["halo" if fam.startswith("halo") else fam], call)
        return {"y": y}
    return fn


for _causal in (False, True):
    _c = " causal" if _causal else ""
    conv_case(f"conv3d halo:128 (64 -> 128){_c}", 64, 128, "halo:128", causal=_causal, gemm_plan="halo:128", gemm_splitk="0")
    conv_case(f"conv3d halo:256 (64 -> 256){_c}", 64, 256, "halo:256", causal=_causal, gemm_plan="halo:256", gemm_splitk="0")
    conv_case(f"conv3d per-tap tile (64 -> 128){_c}", 64, 128, "big", causal=_causal, gemm_off="halo", gemm_splitk="0")
    conv_case(f"conv3d f32 (16 -> 40){_c}", 16, 40, "gemm128", dt=F32, causal=_causal)
conv_case("conv3d halo:128 with resid", 64, 128, "halo:128", resid=True, gemm_plan="halo:128", gemm_splitk="0")
conv_case("upsample3d halo:128 (64 -> 128)", 64, 128, "halo:128", kind="up", gemm_plan="halo:128", gemm_splitk="0")
conv_case("conv_out_unpatchify (128 -> 48) halo:64", 128, 48, "halo:64", kind="out", gemm_splitk="0")


# ================================================================== the norm fold's two GEMM sides
FOLD = (648, 324, 520, 512)        # M, rows_per_batch, N, K: the smallest the fold serves (more than 512 rows, batch elements of at least
                                   # 320 rows, an asm16 shape) with a ragged last tile in M (648 = 4 x 160 + 8) and N (520 = 2 x 256 + 8)


def fold_out_case(epi):
    @case(f"linear_fold_out epi{epi} (648, 520, 512), scale2 stride > N", gemm_plan="asm16:160x256")
    def fn(hip, A, st):
        import fold_ref
        M, rpb, N, K = FOLD
        x, w, b, r, gate = linear_inputs(M, N, K, BF16, 70 + epi, rpb)
        scale2 = randn(gen(71), 2, N, scale=0.3, dt=F32) + torch.tensor([0.5, -0.4])[:, None]
        px, _ = A.place(x, name="x"); pw, _ = A.place(w, name="w"); pb, _ = A.place(b, name="bias"); pr, _ = A.place(r, name="resid")
        pg = A.place(gate, name="gate")[0] if epi == 2 else None
        ps2, _ = A.place(scale2, ld=N + 8, name="scale2")
        py, y = A.place(torch.empty(M, N, dtype=BF16), role="out", name="y"); py2, y2 = A.place(torch.empty(M, N, dtype=BF16), role="out", name="y2")
        prs, rs = A.place(torch.empty(M, (N + 127) // 128, dtype=F32), role="out", name="rowsq")      # ceil(N / 128) partial columns
        assert hip.ops.linear_fold_ok(M, N, K, epi, False, 0, N + 8, rpb)
        routed(st, family(hip.ops.gemm_route(M, N, K, epi=epi, fold_out=True)), "asm16")
        A.arm()
        launch(hip, st, KERNEL_OF["asm16"], lambda: hip.lib.ltx_op_linear_fold_out(px, pw, pb, py, py2, prs, ps2, N + 8, M, N, K, epi, pr, pg, rpb, stream(hip)))

        def value(o):                                                                           # test_gpu_fold_ops' producer bars
            check_floor(o["y"], linear_want(x, w, b, r, gate, epi, rpb), st["name"])
            assert E.same_bits(o["y2"], fold_ref.mod_scale_ref(o["y"], scale2, rpb)), "y2 is not bf16(f32(y as stored) * (1 + scale2))"
            assert rel_l2(o["rowsq"], fold_ref.rowsq_ref(o["y"]).float()) < 1e-6
        st["check"] = value
        return {"y": y, "y2": y2, "rowsq": rs}
    return fn


def fold_in_case(epi):
    @case(f"linear_fold_in epi{epi} (648, 520, 512), cvec stride > N", gemm_plan="asm16:160x256")
    def fn(hip, A, st):
        import fold_ref
        M, rpb, N, K = FOLD
        g = gen(80 + epi)
        h = (torch.randn(M, K, generator=g) * torch.exp(0.5 * torch.randn(M, 1, generator=g))).bfloat16()
        a = fold_ref.mod_scale_ref(h, torch.randn(2, K, generator=g) * 0.3, rpb)
        w = randn(g, N, K, scale=K ** -0.5)
        cvec = torch.randn(2, N, generator=g) * 0.1 + torch.tensor([3.0, -3.0])[:, None]
        rsq = fold_ref.rowsq_ref(h).float()
        pa, _ = A.place(a, name="x"); pw, _ = A.place(w, name="w"); prs, _ = A.place(rsq, name="rs_sq"); pc, _ = A.place(cvec, ld=N + 8, name="cvec")
        py, y = A.place(torch.empty(M, N, dtype=BF16), role="out", name="y")
        assert hip.ops.linear_fold_ok(M, N, K, epi, True, K // 128, N + 8, rpb)
        routed(st, family(hip.ops.gemm_route(M, N, K, epi=epi, fold_in=True)), "asm16")
        A.arm()
        launch(hip, st, KERNEL_OF["asm16"], lambda: hip.lib.ltx_op_linear_fold_in(pa, pw, py, prs, K // 128, K, 1e-6, pc, N + 8, M, N, K, epi, rpb, stream(hip)))
        ref = fold_ref.fold_in_ref(a, w, rsq, K, 1e-6, cvec, epi, rpb).float()
        st["check"] = lambda o: check_floor(o["y"], ref, st["name"])                            # test_gpu_fold_ops' consumer bar
        return {"y": y}
    return fn


for _epi in (2, 3):
    fold_out_case(_epi)
for _epi in (0, 1):
    fold_in_case(_epi)


# ================================================================== conv3d_norm, conv3d_shuffle
def conv_norm_case(Cout, causal):
    @case(f"conv3d_norm halo:{Cout} (64 -> {Cout}){' causal' if causal else ''}, table slices of [B, 4 Cout]", gemm_splitk="0")
    def fn(hip, A, st):
        import test_gpu_conv_norm as CN
        B, T, H, W, Cin, eps, act = 2, 2, 5, 6, 64, 1e-6, 1
        g = gen(Cout + causal)
        x, w, b = randn(g, B, Cin, T, H, W), randn(g, Cout, Cin, 3, 3, 3, scale=(27 * Cin) ** -0.5), randn(g, Cout, scale=0.1)
        table = 0.3 * torch.randn(B, 4 * Cout, generator=g)
        parts = [table[:, i * Cout:(i + 1) * Cout].contiguous() for i in range(4)]
        scale, shift = CN.slices(table, Cout)
        px, _ = A.place(cl(x).reshape(-1, Cin), name="x"); pw, _ = A.place(w.reshape(Cout, -1), name="w"); pb, _ = A.place(b, name="bias")
        (_, _), (_, _), (psh, _), (psc, _) = A.place_fused(parts, ["in"] * 4, names=["table 0", "table 1", "shift", "scale"])
        py, y = A.place(torch.empty(B * T * H * W, Cout, dtype=BF16), role="out", name="y")
        routed(st, hip.ops.gemm_route(B * T * H * W, Cout, Cin, 1, 27, B, T, H, W, pn=True), f"halo:{Cout}")
        A.arm()
        launch(hip, st, KERNEL_OF["halo"], lambda: hip.lib.ltx_op_conv3d_norm(px, pw, pb, 1, py, psc, psh, 4 * Cout, eps, act, B, T, H, W, Cin, Cout, int(causal), 1, stream(hip)))

        def value(o):                                                                           # test_gpu_conv_norm: twice the reference's own floor
            c = CN.conv_f64(x, w, b, causal)
            exact = CN.norm_f64(c, scale, shift, eps, act)
            floor = rel_l2(CN.norm_f64(c.float().bfloat16(), scale, shift, eps, act).float().bfloat16(), exact)
            e = rel_l2(o["y"].float().view(B, T, H, W, Cout), exact)
            assert e <= 2 * floor, (e, floor)
        st["check"] = value
        return {"y": y}
    return fn


for _Cout in (128, 256):
    for _causal in (False, True):
        conv_norm_case(_Cout, _causal)


def shuffle_case(st_, ss, dt, fam, **opts):
    @case(f"conv3d_shuffle ({st_}, {ss}) {'bf16' if dt == BF16 else 'f32'} w32 -> {fam}", **opts)
    def fn(hip, A, st):
        import test_gpu_latent_upsampler_st as ST
        from conftest import rel_max
        x, w, b, want = ST._op_case("w32", st_, ss)                                             # B 2, F 3, H 5, W 7, 32 -> 32 channels
        B, Fo, Ho, Wo, Cf = want.shape
        _, F_, H, W, Cin, _ = ST.OP_CASES["w32"]
        O_ = w.shape[0]
        z = torch.zeros_like(x[:, :, :1])
        xg = torch.cat([z, x, z], 2).permute(0, 2, 3, 4, 1).contiguous().to(dt)                  # zero guard frames in front and behind
        px, _ = A.place(xg.reshape(-1, Cin), name="x"); pw, _ = A.place(w.to(dt).reshape(O_, -1), name="w"); pb, _ = A.place(b.to(dt), name="bias")
        py, y = A.place(torch.empty(B * (Fo + 2) * Ho * Wo, Cf, dtype=dt), role="out", name="y")
        route = ST._route(hip, "w32", st_, ss, dt)
        st["note"] = route
        routed(st, family(route), fam)
        A.arm()
        launch(hip, st, KERNEL_OF[fam], lambda: hip.lib.ltx_op_conv3d_shuffle(px, pw, pb, dtc(hip, dt), py, B, F_, H, W, Cin, O_, st_, ss, dtc(hip, dt), stream(hip)))

        def value(o):                                                                           # test_gpu_latent_upsampler_st's checks
            yy = o["y"].view(B, Fo + 2, Ho, Wo, Cf)
            assert bool((yy[:, 0] == 0).all()) and bool((yy[:, Fo + 1] == 0).all()), "the guard frames are written as exact zeros"
            if dt == F32:
                assert rel_max(yy[:, 1:Fo + 1], want) <= 1e-3
            else:
                check_floor(yy[:, 1:Fo + 1], want, st["name"])
        st["check"] = value
        return {"y": y}
    return fn


for _f in ((2, 1), (2, 2), (1, 2)):
    shuffle_case(*_f, BF16, "big", gemm_splitk="0")
    shuffle_case(*_f, F32, "gemm128")


# ================================================================== the one body
@pytest.mark.parametrize("name", list(CASES))
def test_extents(hip, name):
    fn, opts, capacity = CASES[name]
    st = {"name": name}

    def run(A):
        with hip.options(gemm_tune="0", **opts):
            return fn(hip, A, st)
    first = E.filler_passes(run, DEV, capacity)
    print(f"{name}: {st.get('note', '')}")
    if st.get("finite", True):
        for k, v in first.items():
            if v.is_floating_point():
                assert torch.isfinite(v.float()).all(), (name, k)
    st["check"](first)
    assert st.get("routed") is True or st.get("no_route"), f"{name}: neither a route assertion nor a stated reason why the entry has none"
