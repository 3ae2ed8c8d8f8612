"""GPU suite: the norm fold's two GEMM epilogue sides (GemmArgs::C2 / ::rs_sq in gemm_asm16_kernel's wide epilogue) and the three
small launchers around them (shift_gemv, mod_scale, scale_cols), each as ONE kernel against tests/fold_ref.py (float64).

tests/test_gpu_normfold.py sees the fold through a three-layer forward, where a wrong batch row's cvec on the rows of a straddling
tile, a dropped group of row partials or a mis-rounded second output are diluted below its bars.  Here:
  consumer  out = epi(r_m * acc + cvec[b(m)]): one f32 fma and one bf16 rounding on the accumulator -> the rounding floor of
            tests/test_gpu_tight.py (<= 2 bf16 ulp above 2^-6 of the rms, rel-L2 <= 3e-3), the three tile heights bit-equal, and the
            rows of the first / last batch element bit-equal to a call that has only that batch element (no straddling tile)
  producer  y bit-equal to the launch without the second output, rowsq bit-equal to the stand-alone pass, y2 bit-equal to the f32
            expression on the stored y (and to ops.mod_scale), y on the rounding floor
Shapes: the smallest the one-wave-per-SIMD family serves (more than 512 rows, an unsplit shape: M * N > 8 388 608 above 1536
rows), batch boundaries that cut a tile for every tile height, partial last tiles, ragged N, D = 512 .. 2048 (4 .. 16 partials),
batch elements of the admitted minimum of 320 rows."""
import math

import pytest
import torch

import fold_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILES = ["asm16:256x256", "asm16:320x256", "asm16:160x256"]
EPS = 1e-6
ERR_ARG = "rc=1"                   # LTX_ERR_ARG


@pytest.fixture(scope="module")
def hip():
    import ltxhip
    assert torch.cuda.is_available()
    torch.set_num_threads(16)
    return ltxhip


def ulp_distance(a_bf16: torch.Tensor, b_bf16: torch.Tensor) -> torch.Tensor:
    """distance in representable bf16 values (sign-magnitude bits mapped to a monotonic integer line)"""
    def line(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (line(a_bf16) - line(b_bf16)).abs()


def check_floor(got_bf16, ref_f32, what, max_ulp=2, l2=3e-3):
    """tests/test_gpu_tight.py's bar"""
    got = got_bf16.cpu()
    assert torch.isfinite(got.float()).all(), what
    e = rel_l2(got.float(), ref_f32)
    d = ulp_distance(got, ref_f32.bfloat16())
    big = ref_f32.abs() > ref_f32.pow(2).mean().sqrt() * 2.0 ** -6
    worst = int(d[big].max()) if big.any() else 0
    frac1 = float((d[big] >= 1).float().mean()) if big.any() else 0.0
    assert e <= l2, (what, "rel-L2", e)
    assert worst <= max_ulp, (what, "max ulp", worst)
    return e, worst, frac1


def floor_stats(got_bf16, ref_f32):
    """check_floor's two figures without its bars"""
    got = got_bf16.cpu()
    d = ulp_distance(got, ref_f32.bfloat16())
    big = ref_f32.abs() > ref_f32.pow(2).mean().sqrt() * 2.0 ** -6
    return rel_l2(got.float(), ref_f32), int(d[big].max())


# ------------------------------------------------------------------ consumer side
#        name      M     rows_per_batch  K = D   N    synthetic partials
CONSUMER = {
    "a":     (2200, 1100, 2048, 4096, False),       # the boundary cuts a tile of every height; every last tile is partial
    "a_syn": (2200, 1100, 2048, 4096, True),        # partials that are no sums of squares: every group decides some rows
    "b512":  (2199, 733, 512, 4096, False),         # 4 / 8 / 12 partials per row: the re-read of the last group
    "b1024": (2199, 733, 1024, 4096, False),
    "b1536": (2199, 733, 1536, 4096, False),
    "c":     (2240, 320, 2048, 4096, False),        # the admitted minimum: aligned on the 320-row tile, cutting the other two
    "d":     (2200, 1100, 2048, 4104, False),       # ragged N: the last column tile holds 8 live columns
}
OFFSETS = [3.0, -3.0, 0.0, 2.0, -2.0, 1.0, -1.0]    # cvec rows far apart: a wrong batch row is hundreds of ulps
_cases = {}


def consumer_case(hip, name):
    """inputs (CPU and device), the row partials and the f64 accumulator of a case: built once, shared, never written"""
    if name in _cases:
        return _cases[name]
    M, rpb, K, N, syn = CONSUMER[name]
    B = M // rpb
    g = torch.Generator().manual_seed(sum(map(ord, name)) + M + K + N)
    h = (torch.randn(M, K, generator=g) * torch.exp(0.5 * torch.randn(M, 1, generator=g))).bfloat16()      # rows of different rms
    sc = torch.randn(B, K, generator=g) * 0.3
    a = R.mod_scale_ref(h, sc, rpb)                                         # the A operand the producer would have left
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16()
    cvec = torch.randn(B, N, generator=g) * 0.1 + torch.tensor(OFFSETS[:B])[:, None]
    if syn:
        n = K // 128
        lead = (torch.arange(M)[:, None] % n) == torch.arange(n)[None, :]   # group m % n carries the row: dropped, doubled or swapped for another row's, it shows
        rs = (0.5 + torch.rand(M, n, generator=g)) * torch.where(lead, 1000.0, 1.0) * (K / 1000.0)
        rs_dev = rs.to(DEV)
    else:
        rs_dev = hip.ops.rowsq(h.to(DEV))
        rs = rs_dev.cpu()
        assert rel_l2(rs, R.rowsq_ref(h).float()) < 1e-6                    # (the partials themselves: tests/test_gpu_ops.py)
    c = dict(M=M, rpb=rpb, K=K, N=N, B=B, a=a.to(DEV), w=w.to(DEV), rs=rs_dev, cvec=cvec.to(DEV),
             ref_lin=R.fold_in_ref(a, w, rs, K, EPS, cvec, 0, rpb), out={})
    _cases[name] = c
    return c


def consumer_run(hip, c, tile, epi):
    key = (tile, epi)
    if key not in c["out"]:
        with hip.options(gemm_plan=tile):
            c["out"][key] = hip.ops.linear_fold_in(c["a"], c["w"], c["rs"], c["cvec"], epi=epi, rows_per_batch=c["rpb"], rs_D=c["K"], eps=EPS)
    return c["out"][key]


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("epi", [0, 1])
@pytest.mark.parametrize("name", list(CONSUMER))
def test_consumer_side_on_the_rounding_floor_and_bit_equal_across_tiles(hip, name, epi, tile):
    c = consumer_case(hip, name)
    M, rpb, K, N = c["M"], c["rpb"], c["K"], c["N"]
    assert hip.ops.linear_fold_ok(M, N, K, epi, True, K // 128, N, rpb), "the case is not one the fold serves"
    got = consumer_run(hip, c, tile, epi)
    ref = (c["ref_lin"] if epi == 0 else R.gelu_tanh(c["ref_lin"])).float()
    e, worst, frac = check_floor(got, ref, (name, epi, tile))
    # rows 256 .. 319 of a 320-row tile take their 1 / rms from the four-lane chain, the others from the per-thread sum: each range on its own
    hi = (torch.arange(M) % 320) >= 256
    _, worst_lo, _ = check_floor(got[~hi.to(DEV)], ref[~hi], (name, epi, tile, "tile rows 0..255"))
    _, worst_hi, _ = check_floor(got[hi.to(DEV)], ref[hi], (name, epi, tile, "tile rows 256..319"))
    print(f"fold_in {name} epi {epi} {tile}: rel-L2 {e:.2e}  max ulp {worst} (rows 0..255 of a 320-row tile {worst_lo}, rows 256..319 {worst_hi})  off by >= 1 ulp {100 * frac:.2f} %")
    # the same accumulation chain and the same fma whatever the tile height
    assert torch.equal(got, consumer_run(hip, c, TILES[0], epi)), "tiles differ"


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name", ["a", "b512", "b1536", "c", "d"])
def test_consumer_rows_of_a_batch_element_keep_the_bits_of_a_one_batch_call(hip, name, tile):
    """The per-row choice between the two batch elements' cvec in a tile that the boundary cuts, against calls no boundary cuts: the
    first and the last batch element ALONE (their rows, their partials, their cvec row).  Case c's batch elements are 320 rows - below
    the 512 this kernel family starts at - so there the one-batch call keeps all rows and takes the one cvec row for all of them."""
    c = consumer_case(hip, name)
    M, rpb, K, N, B = c["M"], c["rpb"], c["K"], c["N"], c["B"]
    for epi in (0, 1):
        got = consumer_run(hip, c, tile, epi)
        for b in (0, B - 1):
            rows = slice(b * rpb, (b + 1) * rpb)
            with hip.options(gemm_plan=tile):
                if rpb > 512:
                    assert hip.ops.linear_fold_ok(rpb, N, K, epi, True, K // 128, N, rpb)
                    alone = hip.ops.linear_fold_in(c["a"][rows], c["w"], c["rs"][rows], c["cvec"][b:b + 1], epi=epi, rows_per_batch=rpb, rs_D=K, eps=EPS)
                else:
                    assert hip.ops.linear_fold_ok(M, N, K, epi, True, K // 128, N, M)
                    alone = hip.ops.linear_fold_in(c["a"], c["w"], c["rs"], c["cvec"][b:b + 1], epi=epi, rows_per_batch=M, rs_D=K, eps=EPS)[rows]
            assert torch.equal(got[rows], alone), (name, tile, epi, "batch element", b)
        assert not torch.equal(got[:rpb], got[rpb:2 * rpb])


# ------------------------------------------------------------------ producer side
#           M      rows_per_batch  N = D   K
PRODUCER = {
    "k2048": (4110, 2055, 2048, 2048),              # the 160-row tile requests its residual inside the K loop (K / 64 >= 12)
    "k512":  (4110, 2055, 2048, 512),               # ... and here it does not
    "k8192": (4110, 2055, 2048, 8192),              # ff2's K
    "d512":  (16400, 8200, 512, 512),               # the smallest D
}
_pcases = {}


def producer_case(name):
    if name in _pcases:
        return _pcases[name]
    M, rpb, N, K = PRODUCER[name]
    B = M // rpb
    g = torch.Generator().manual_seed(sum(map(ord, name)) + M + K + N)
    x = torch.randn(M, K, generator=g).bfloat16(); w = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16(); b = (torch.randn(N, generator=g) * 0.1).bfloat16()
    resid = torch.randn(M, N, generator=g).bfloat16(); gate = torch.randn(B, N, generator=g)
    scale2 = torch.randn(B, N + 64, generator=g) * 0.3 + torch.tensor([0.5, -0.4])[:, None]      # rows that differ per batch element; a row stride wider than N
    c = dict(M=M, rpb=rpb, N=N, K=K, cpu=(x, w, b, resid, gate, scale2), dev=tuple(t.to(DEV) for t in (x, w, b, resid, gate, scale2)),
             lin=x.double() @ w.double().T + b.double(), out={})
    _pcases[name] = c
    return c


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("epi", [2, 3])
@pytest.mark.parametrize("name", list(PRODUCER))
def test_producer_side_second_output_and_partials_bit_exact(hip, name, epi, tile):
    c = producer_case(name)
    M, rpb, N, K = c["M"], c["rpb"], c["N"], c["K"]
    x, w, b, resid, gate, scale2 = c["dev"]
    assert hip.ops.linear_fold_ok(M, N, K, epi, False, 0, N + 64, rpb), "the case is not one the fold serves"
    with hip.options(gemm_plan=tile):
        y, y2, rs = hip.ops.linear_fold_out(x, w, b, scale2, epi, resid, gate if epi == 2 else None, rpb)
        y_plain, rs_plain = hip.ops.linear_rowsq(x, w, b, epi=epi, resid=resid, gate=gate if epi == 2 else None, rows_per_batch=rpb)
    torch.cuda.synchronize()
    assert torch.equal(y, y_plain) and torch.equal(rs, rs_plain), "the second output disturbs the first"
    assert torch.equal(rs, hip.ops.rowsq(y)), "row partials differ from the stand-alone pass on the stored rows"
    want2 = R.mod_scale_ref(y.cpu(), c["cpu"][5], rpb)                      # bf16(f32(y as stored) * (1.0f + scale2[b(m)]))
    bad = (y2.cpu().view(torch.int16) != want2.view(torch.int16)).nonzero()
    assert bad.numel() == 0, ("second output", len(bad), bad[:4].tolist())
    assert torch.equal(hip.ops.mod_scale(y, scale2, rpb), y2), "ops.mod_scale and the epilogue's second output differ"
    # the three tile heights agree - among them the 160-row tile's residual-prefetch instantiation (k2048, k8192) and the 256- / 320-row
    # tiles, which read the residual in the epilogue
    first = c["out"].setdefault(epi, (y, y2, rs))
    assert all(torch.equal(p, q) for p, q in zip((y, y2, rs), first)), "tiles differ"
    g64 = R.batch_rows(c["cpu"][4].double(), M, rpb)
    want = c["cpu"][3].double() + (g64 * c["lin"] if epi == 2 else c["lin"])
    e, worst, frac = check_floor(y, want.float(), (name, epi, tile))
    print(f"fold_out {name} epi {epi} {tile}: rel-L2 {e:.2e}  max ulp {worst}  off by >= 1 ulp {100 * frac:.2f} %")


def test_producer_reference_epilogue_is_fold_ref(hip):
    """(the float64 epilogue the producer test assembles from its cached x W^T + b is fold_ref's)"""
    c = producer_case("k512")
    x, w, b, resid, gate, scale2 = c["cpu"]
    for epi in (2, 3):
        want = resid.double() + (R.batch_rows(gate.double(), c["M"], c["rpb"]) * c["lin"] if epi == 2 else c["lin"])
        assert torch.equal(R.resid_epilogue_ref(x, w, b, resid, gate, epi, c["rpb"]), want)


# ------------------------------------------------------------------ producer -> shift_gemv -> consumer
def test_chain_against_the_unfolded_block_expression(hip):
    """out2's epilogue -> shift_gemv -> the projection, against float64 linear(rms_norm(h) (1 + sc) + sh) on the stored h; beside it
    the unfolded arm (ops.rownorm, then ops.linear) against the same reference.  The fold rounds h (1 + sc) where the pass rounds
    the modulated, normalised row - one bf16 rounding in another place: its worst ulp may exceed the pass's by 1, its rel-L2 by 10 %
    (tests/test_gpu_normfold.py's bar).  Both arms are printed; docs/lab_notes.md, "Norm fold, kernel-level tests and the routing guard",
    keeps the figures."""
    M, rpb, D, N = 4110, 2055, 2048, 4096
    g = torch.Generator().manual_seed(4110)
    x = torch.randn(M, D, generator=g).bfloat16(); wp = (torch.randn(D, D, generator=g) / math.sqrt(D)).bfloat16(); bp = (torch.randn(D, generator=g) * 0.1).bfloat16()
    resid = (torch.randn(M, D, generator=g) * torch.exp(0.5 * torch.randn(M, 1, generator=g))).bfloat16()
    sc, sh = torch.randn(2, D, generator=g) * 0.3, torch.randn(2, D, generator=g) * 0.5
    w = (torch.randn(N, D, generator=g) / math.sqrt(D)).bfloat16(); b = (torch.randn(N, generator=g) * 0.1).bfloat16()
    assert hip.ops.linear_fold_ok(M, D, D, 3, False, 0, D, rpb) and hip.ops.linear_fold_ok(M, N, D, 0, True, D // 128, N, rpb)
    dv = lambda t: t.to(DEV)
    h, h2, rs = hip.ops.linear_fold_out(dv(x), dv(wp), dv(bp), dv(sc), 3, dv(resid), None, rpb)
    cvec = hip.ops.shift_gemv(dv(w), dv(b), dv(sh))
    fold = hip.ops.linear_fold_in(h2, dv(w), rs, cvec, epi=0, rows_per_batch=rpb, rs_D=D, eps=EPS)
    passed = hip.ops.linear(hip.ops.rownorm(h, kind=0, eps=EPS, scale=dv(sc), shift=dv(sh), rows_per_batch=rpb), dv(w), dv(b))
    h64 = h.cpu().double()
    y = h64 / ((h64 * h64).sum(-1, keepdim=True) * (1.0 / D) + EPS).sqrt() * (1.0 + R.batch_rows(sc.double(), M, rpb)) + R.batch_rows(sh.double(), M, rpb)
    ref = (y @ w.double().T + b.double()).float()
    e_pass, u_pass = floor_stats(passed, ref)
    e_fold, u_fold = floor_stats(fold, ref)
    print(f"chain M {M} D {D} N {N}: fold rel-L2 {e_fold:.3e} max ulp {u_fold}   pass rel-L2 {e_pass:.3e} max ulp {u_pass}")
    check_floor(fold, ref, "chain, fold arm", max_ulp=u_pass + 1)
    assert e_fold <= 1.1 * e_pass, (e_fold, e_pass)


# ------------------------------------------------------------------ the small launchers
@pytest.mark.parametrize("K", [8, 512, 2048, 1544])
def test_shift_gemv_against_f64_within_the_f32_chain_bound(hip, K):
    """|err| <= (K / 64 + 16) 2^-24 sum_k |s w| + 2^-23 |ref|: an f32 fma chain of K / 64 steps per lane, the six shuffle adds and the
    bias (a dropped 8-column chunk is orders of magnitude above it); B = 1, 3, 8 rows, N = 6144, 4104, 5, with and without a bias, and
    a shift row stride wider than K."""
    g = torch.Generator().manual_seed(K)
    for N in (6144, 4104, 5):
        w = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16(); bias = torch.randn(N, generator=g).bfloat16()
        for B in (1, 3, 8):
            for stride, bs in ((K, bias), (K + 8, bias), (K, None)):
                shift = torch.randn(B, stride, generator=g)
                got = hip.ops.shift_gemv(w.to(DEV), bs.to(DEV) if bs is not None else None, shift.to(DEV), K=K).cpu().double()
                ref = R.shift_gemv_ref(w, bs, shift)
                bound = (K / 64 + 16) * 2.0 ** -24 * (shift.double()[:, :K].abs() @ w.double().abs().T) + 2.0 ** -23 * ref.abs()
                over = ((got - ref).abs() - bound).max()
                assert got.shape == (B, N) and float(over) <= 0.0, (N, B, stride, bs is not None, float(over), float(((got - ref).abs() / bound).max()))
    # an output row stride wider than N: the columns past N stay untouched
    w = (torch.randn(12, K, generator=g) / math.sqrt(K)).bfloat16(); shift = torch.randn(2, K, generator=g)
    wide = hip.ops.shift_gemv(w.to(DEV), None, shift.to(DEV), out_stride=16).cpu()
    assert torch.equal(wide[:, 12:], torch.zeros(2, 4)) and torch.equal(wide[:, :12], hip.ops.shift_gemv(w.to(DEV), None, shift.to(DEV)).cpu())


@pytest.mark.parametrize("N,K", [(2047, 2048), (2049, 2048), (4097, 2048), (524287, 8), (524289, 8), (3, 8)])
def test_scale_cols_bit_exact_around_the_grid_span(hip, N, K):
    """bf16(f32(W) * (1.0f + scale[k])) where N * K sits just below / just above a multiple of the launch's span (elementwise.hip's
    grid_for: at most 16384 blocks of 256 threads = 4 194 304 elements per sweep of the grid-stride loop)"""
    assert N == 3 or min(N * K % 4194304, -N * K % 4194304) <= 2048
    g = torch.Generator().manual_seed(N + K)
    w = torch.randn(N, K, generator=g).bfloat16(); s = torch.randn(K, generator=g) * 0.3
    got = hip.ops.scale_cols(w.to(DEV), s.to(DEV)).cpu()
    assert torch.equal(got.view(torch.int16), R.scale_cols_ref(w, s).view(torch.int16))


# ------------------------------------------------------------------ refusals
def test_calls_the_fold_does_not_serve_are_refused_before_any_launch(hip):
    M, rpb, K, N = 2200, 1100, 2048, 4096
    z = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt, device=DEV)
    f = lambda *s: z(*s, dt=torch.float32)
    hip.prof_enable(True)
    try:
        for what, call in [
            ("20 partials", lambda: hip.ops.linear_fold_in(z(M, K), z(N, K), f(M, 20), f(2, N), rows_per_batch=rpb)),
            ("6 partials", lambda: hip.ops.linear_fold_in(z(M, K), z(N, K), f(M, 6), f(2, N), rows_per_batch=rpb)),
            ("319-row batch elements", lambda: hip.ops.linear_fold_in(z(2233, K), z(N, K), f(2233, 16), f(7, N), rows_per_batch=319)),
            ("consumer of 512 rows", lambda: hip.ops.linear_fold_in(z(512, K), z(N, K), f(512, 16), f(1, N), rows_per_batch=512)),
            ("producer epi 0", lambda: hip.ops.linear_fold_out(z(4110, K), z(K, K), z(K), f(2, K), 0, z(4110, K), None, 2055)),
            ("producer of 512 rows", lambda: hip.ops.linear_fold_out(z(512, K), z(K, K), z(K), f(1, K), 3, z(512, K), None, 512)),
        ]:
            with pytest.raises(hip.LtxError, match=ERR_ARG):
                call()
        # the A/B arm that hands every GEMM to the 128 x 128 kernel, which reads neither rs_sq / cvec nor C2: an error, not numbers
        with hip.options(gemm_off="big"):
            assert not hip.ops.linear_fold_ok(M, N, K, 0, True, 16, N, rpb)
            with pytest.raises(hip.LtxError, match=ERR_ARG):
                hip.ops.linear_fold_in(z(M, K), z(N, K), f(M, 16), f(2, N), rows_per_batch=rpb)
            with pytest.raises(hip.LtxError, match=ERR_ARG):
                hip.ops.linear_fold_out(z(4110, K), z(K, K), z(K), f(2, K), 3, z(4110, K), None, 2055)
        torch.cuda.synchronize()
        assert hip.prof_report(0)[2] == 0, "a refused call launched a GEMM"
    finally:
        hip.prof_enable(False)
    # (and the same consumer call is served once nothing stands in its way)
    assert hip.ops.linear_fold_ok(M, N, K, 0, True, 16, N, rpb)
