"""GPU suite: the 3x3x3 conv that finishes with the resnet's norm2 inside its epilogue (conv_halo.hip, GemmArgs::pn_on;
ops.conv3d_norm), at op level: y = act(c * rsqrt(mean_n(c^2) + eps) * (1 + scale[b]) + shift[b]) on the conv's bf16 rows c.

All cases are bf16, inputs seeded randn rounded to bf16, weights scaled by (27 Cin)^-0.5, bias by 0.1; scale / shift are f32
0.3 * randn, different per batch row, and are passed as column slices of one [B, 4N] table (shift = table[:, 2N:3N], scale =
table[:, 3N:4N], row stride 4N: the decoder's layout).  Cases (Cin, N, B, T, H, W, causal), all routed to halo:<N>:
    ragged   (64, 128, 2, 2, 20, 37, False)   ragged patches both ways, two batch rows, modulation, SiLU
    exact    (128, 256, 2, 3, 16, 16, True)   exact patches, causal padding, 32 chunks per row
    encoder  (192, 128, 1, 1, 5, 7, True)     one partial patch, Cin != N, no modulation, eps = 1e-8 (the encoder's call)
    act0     (64, 256, 1, 2, 33, 18, False)   act = 0 with modulation
    zero     (64, 128, 1, 1, 16, 17, False)   w = 0, bias = 0: every conv row is exactly zero

Comparison (a), the epilogue alone.  X = ops.conv3d on the halo-staged kernel (gemm_plan=halo:<N>; with gemm_splitk=0, because
the shape rule cuts K for outputs this small and a forced plan is not honoured for a split shape - the test asserts that the
probe names halo:<N> for that call): the bits the fused call normalises.  Reference in float64 from X, rounded once to bf16.  Bar:
at most 2 bf16 ulp where the reference magnitude is above 2^-6 of the tensor's rms, everything finite, and the mask may leave
out at most 3 % of the elements (it leaves out 1.4 - 1.8 %, see below).  One ulp is the reference's own (an f32 evaluation of the
formula is within 1 ulp of the f64 one inside the mask), the second is for the kernel's approximate rsq and exp.  With the two batch
rows of scale / shift exchanged in the reference the same bar must FAIL: a test that cannot tell the rows apart proves nothing.
The unfused pair the VAE runs under vae_fuse_norm=0 - ops.rownorm on the same X - is held to the same bar against the same
reference; the two are not compared with each other (the row statistics are summed in another order).

Comparison (b), the whole fused call, float64 end to end (conv of the bf16 inputs + bias, norm, modulation, SiLU, nothing
rounded): rel-L2 at most TWICE the floor of the reference itself - the same pipeline with the conv result rounded once to bf16
before the norm and the result rounded to bf16, against the unrounded one; the factor covers the kernel's f32 accumulation order
flipping isolated conv roundings.  The floor is computed from the reference alone, each run; measured (CPU, these seeds):
    case      floor (b)    bar = 2 x    excluded by the mask of (a), on the f64 reference of the unrounded conv
    ragged    2.53e-03     5.05e-03     1.67 %
    exact     2.51e-03     5.02e-03     1.68 %
    encoder   2.58e-03     5.15e-03     1.32 %
    act0      2.29e-03     4.58e-03     1.39 %
(two roundings of about 1.7e-3 each, plus what SiLU adds near its minimum).  Measured on an MI355X: comparison (a) max 1 ulp in the
three cases with modulation and 0 in the encoder's, for the fused call and for conv3d + rownorm alike; comparison (b) rel-L2
2.527e-03 / 2.510e-03 / 2.577e-03 / 2.290e-03 - the floor itself to three digits; zero rows 0 ulp from bf16(silu(shift)).

The zero case: with modulation the output is bf16(silu(shift[b][c])) to 1 ulp on every element, without it exactly 0, finite in
both at eps = 1e-8, where rsqrt(eps) = 1e4 multiplies an exact zero.

Also: the same call twice gives the same bits; row 1 of a two-row call equals the call on row 1 alone (nothing in a tile crosses
batch rows); f32 tensors, 12 voxels and 64 output channels raise LtxError instead of returning un-normalised data."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from test_gpu_tight import ulp_distance

pytestmark = pytest.mark.gpu
DEV = "cuda"

#        name       Cin  N   B  T  H   W  causal mod    eps   act
CASES = {"ragged": (64, 128, 2, 2, 20, 37, False, True, 1e-6, 1),
         "exact": (128, 256, 2, 3, 16, 16, True, True, 1e-6, 1),
         "encoder": (192, 128, 1, 1, 5, 7, True, False, 1e-8, 1),
         "act0": (64, 256, 1, 2, 33, 18, False, True, 1e-6, 0)}
ZERO = (64, 128, 1, 1, 16, 17, False)
MAX_ULP, MASK_LOG2, MAX_EXCLUDED = 2, -6, 0.03


@pytest.fixture(scope="module")
def hip():
    import ltxhip
    assert torch.cuda.is_available()
    torch.set_num_threads(16)
    return ltxhip


def cl(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


def make_inputs(name):
    Cin, N, B, T, H, W, causal, mod, eps, act = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    x = torch.randn(B, Cin, T, H, W, generator=g).bfloat16()
    w = (torch.randn(N, Cin, 3, 3, 3, generator=g) * (27 * Cin) ** -0.5).bfloat16()
    b = (torch.randn(N, generator=g) * 0.1).bfloat16()
    table = 0.3 * torch.randn(B, 4 * N, generator=g)            # the decoder's [B, 4N] modulation table: shift | scale are its last two quarters
    return x, w, b, (table if mod else None)


def slices(table, N):
    """(scale, shift) as the decoder passes them: column slices of the table, row stride 4N"""
    return (None, None) if table is None else (table[:, 3 * N:4 * N], table[:, 2 * N:3 * N])


def conv_f64(x, w, b, causal):
    """LtxVideoCausalConv3d in float64 on channels-first x: replicate padding in time (two frames in front when causal, else one
    on each side), zero padding in the plane; channels-last result [B, T, H, W, N]"""
    x = x.double()
    front, back = (2, 0) if causal else (1, 1)
    xp = torch.cat([x[:, :, :1]] * front + [x] + [x[:, :, -1:]] * back, 2)
    return cl(F.conv3d(xp, w.double(), b.double(), padding=(0, 1, 1)))


def norm_f64(c, scale, shift, eps, act):
    """the epilogue on rows c [B, T, H, W, N], float64, nothing rounded"""
    c = c.double()
    n = c * torch.rsqrt(c.pow(2).mean(-1, keepdim=True) + eps)
    if scale is not None:
        n = n * (1.0 + scale.double()[:, None, None, None, :]) + shift.double()[:, None, None, None, :]
    return n * torch.sigmoid(n) if act == 1 else n


def mask_of(ref):
    return ref.abs() > ref.pow(2).mean().sqrt() * 2.0 ** MASK_LOG2


def worst_ulp(got_bf16, ref_f64):
    """(max ulp distance inside the mask, share of elements the mask leaves out)"""
    big = mask_of(ref_f64)
    d = ulp_distance(got_bf16, ref_f64.float().bfloat16())
    return int(d[big].max()), 1.0 - float(big.float().mean())


def reference_floor(name):
    """comparison (b)'s references from the inputs alone: (unrounded f64 result, its floor - the same pipeline with the conv rounded
    once to bf16 before the norm and the result rounded to bf16, rel-L2 against the unrounded one)"""
    Cin, N, B, T, H, W, causal, mod, eps, act = CASES[name]
    x, w, b, table = make_inputs(name)
    scale, shift = slices(table, N)
    c = conv_f64(x, w, b, causal)
    exact = norm_f64(c, scale, shift, eps, act)
    rounded = norm_f64(c.float().bfloat16(), scale, shift, eps, act).float().bfloat16()
    return exact, rel_l2(rounded, exact)


@pytest.fixture(scope="module")
def runs(hip):
    """per case, computed once and shared (nothing below modifies it): inputs, the plain conv X on the halo-staged kernel, the fused
    result y, the references of both comparisons"""
    out = {}
    for name, (Cin, N, B, T, H, W, causal, mod, eps, act) in CASES.items():
        x, w, b, table = make_inputs(name)
        xd, wd, bd = cl(x).to(DEV), w.to(DEV), b.to(DEV)
        td = table.to(DEV) if mod else None
        scale_d, shift_d = slices(td, N)
        route = dict(M=B * T * H * W, N=N, K=Cin, conv=1, ntaps=27, B=B, T=T, H=H, W=W)
        assert hip.ops.gemm_route(pn=True, **route) == f"halo:{N}"
        with hip.options(gemm_splitk="0", gemm_plan=f"halo:{N}"):
            assert hip.ops.gemm_route(**route) == f"halo:{N}"            # X really comes from the kernel whose epilogue is under test
            X = hip.ops.conv3d(xd, wd, bd, causal)
        y = hip.ops.conv3d_norm(xd, wd, bd, causal, eps=eps, act=act, scale=scale_d, shift=shift_d)
        torch.cuda.synchronize()
        scale, shift = slices(table, N)
        exact, floor = reference_floor(name)
        out[name] = dict(dev=(xd, wd, bd, scale_d, shift_d), X=X, y=y.cpu(), ref_a=norm_f64(X.cpu(), scale, shift, eps, act), exact=exact, floor=floor,
                         scale=scale, shift=shift)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_epilogue_alone_to_two_ulp(hip, runs, name):
    Cin, N, B, T, H, W, causal, mod, eps, act = CASES[name]
    r = runs[name]
    assert torch.isfinite(r["y"].float()).all()
    worst, excluded = worst_ulp(r["y"], r["ref_a"])
    print(f"{name}: fused vs f64 epilogue of X: max ulp {worst} inside the mask, mask leaves out {100 * excluded:.2f} %")
    assert excluded <= MAX_EXCLUDED, excluded
    assert worst <= MAX_ULP, worst
    if mod and B == 2:          # the reference with the two modulation rows exchanged must miss the bar
        perm = norm_f64(r["X"].cpu(), r["scale"].flip(0), r["shift"].flip(0), eps, act)
        assert int(ulp_distance(r["y"], perm.float().bfloat16())[mask_of(perm)].max()) > MAX_ULP


@pytest.mark.parametrize("name", list(CASES))
def test_unfused_pair_meets_the_same_bar(hip, runs, name):
    """ops.conv3d + ops.rownorm (RMS, same eps, modulation and activation): what the VAE runs under vae_fuse_norm=0"""
    Cin, N, B, T, H, W, causal, mod, eps, act = CASES[name]
    r = runs[name]
    sc, sh = (r["dev"][3].contiguous(), r["dev"][4].contiguous()) if mod else (None, None)
    got = hip.ops.rownorm(r["X"].reshape(-1, N), kind=0, eps=eps, scale=sc, shift=sh, rows_per_batch=T * H * W, act=act).reshape(B, T, H, W, N).cpu()
    assert torch.isfinite(got.float()).all()
    worst, _ = worst_ulp(got, r["ref_a"])
    print(f"{name}: conv3d + rownorm vs f64 epilogue of X: max ulp {worst} inside the mask")
    assert worst <= MAX_ULP, worst


@pytest.mark.parametrize("name", list(CASES))
def test_whole_fused_call_to_twice_the_reference_floor(hip, runs, name):
    r = runs[name]
    e = rel_l2(r["y"].float(), r["exact"])
    print(f"{name}: fused vs f64 end to end: rel-L2 {e:.3e}, floor of the reference {r['floor']:.3e}, bar {2 * r['floor']:.3e}")
    assert 1.5e-3 <= r["floor"] <= 3.5e-3, r["floor"]          # two bf16 roundings of ~1.7e-3 each: the floor itself is sane
    assert e <= 2 * r["floor"], (e, r["floor"])


def test_all_zero_rows(hip):
    """w = 0, bias = 0: every conv row is exactly zero, so r = rsqrt(eps) (1e4 at the encoder's eps) multiplies 0"""
    Cin, N, B, T, H, W, causal = ZERO
    g = torch.Generator().manual_seed(77)
    x = cl(torch.randn(B, Cin, T, H, W, generator=g).bfloat16()).to(DEV)
    w, b = torch.zeros(N, Cin, 3, 3, 3, dtype=torch.bfloat16, device=DEV), torch.zeros(N, dtype=torch.bfloat16, device=DEV)
    table = 0.3 * torch.randn(B, 4 * N, generator=g)
    scale, shift = slices(table.to(DEV), N)
    assert hip.ops.gemm_route(B * T * H * W, N, Cin, conv=1, ntaps=27, B=B, T=T, H=H, W=W, pn=True) == f"halo:{N}"
    for eps in (1e-8, 1e-6):
        plain = hip.ops.conv3d_norm(x, w, b, causal, eps=eps, act=1).cpu()
        assert torch.isfinite(plain.float()).all() and not plain.float().any(), eps          # exactly zero (either sign)
        got = hip.ops.conv3d_norm(x, w, b, causal, eps=eps, act=1, scale=scale, shift=shift).cpu()
        assert torch.isfinite(got.float()).all()
        sh = table[:, 2 * N:3 * N].double()
        want = (sh * torch.sigmoid(sh))[:, None, None, None, :].expand(B, T, H, W, N).float().bfloat16()
        d = int(ulp_distance(got, want).max())
        print(f"zero rows, eps {eps:g}: max ulp to bf16(silu(shift)) {d}")
        assert d <= 1, (eps, d)


def test_same_bits_twice_and_per_batch_row(hip, runs):
    for name, (Cin, N, B, T, H, W, causal, mod, eps, act) in CASES.items():
        xd, wd, bd, sc, sh = runs[name]["dev"]
        again = hip.ops.conv3d_norm(xd, wd, bd, causal, eps=eps, act=act, scale=sc, shift=sh).cpu()
        assert torch.equal(again, runs[name]["y"]), name
        if B == 2:              # row 1 alone, with ITS modulation row: nothing in a tile crosses batch rows
            one = hip.ops.conv3d_norm(xd[1:2], wd, bd, causal, eps=eps, act=act, scale=sc[1:2], shift=sh[1:2]).cpu()
            assert torch.equal(one[0], runs[name]["y"][1]), name
            assert not torch.equal(one[0], runs[name]["y"][0])


def test_calls_the_kernel_does_not_serve_are_refused(hip):
    """before the dispatch refused them, the first two returned the conv WITHOUT the norm and return code 0"""
    g = torch.Generator().manual_seed(5)

    def call(dt, Cin, N, B, T, H, W):
        x = cl(torch.randn(B, Cin, T, H, W, generator=g)).to(dt).to(DEV)
        w = (torch.randn(N, Cin, 3, 3, 3, generator=g) * (27 * Cin) ** -0.5).to(dt).to(DEV)
        return hip.ops.conv3d_norm(x, w, torch.zeros(N, dtype=dt, device=DEV))

    for args in ((torch.float32, 64, 128, 1, 1, 16, 17), (torch.bfloat16, 64, 128, 1, 1, 3, 4), (torch.bfloat16, 64, 64, 1, 1, 16, 17)):
        with pytest.raises(hip.LtxError):
            call(*args)
    assert call(torch.bfloat16, 64, 128, 1, 1, 16, 17).shape == (1, 1, 16, 17, 128)          # the served neighbour of all three
    x = cl(torch.randn(1, 64, 1, 16, 17, generator=g)).bfloat16().to(DEV)
    w = torch.zeros(128, 64, 3, 3, 3, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(hip.LtxError):          # half a modulation
        hip.ops.conv3d_norm(x, w, torch.zeros(128, dtype=torch.bfloat16, device=DEV), scale=torch.zeros(1, 128, device=DEV))
