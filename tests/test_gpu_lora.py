"""GPU suite: LoRA adapters merged into the DiT's weights on the device (include/ltxhip_lora.h, csrc/lora.hip).

The reference project has no LoRA support; the parity reference is tests/lora_ref.py (pinned to the definition of LoRA by
tests/test_lora_cpu.py).  Bars, derived there from the engine's arithmetic:
  f32 mode  |out - E| <= gamma;   bf16 mode  |out - E| <= 1/2 max(ulp_bf16(E), ulp_bf16(out)) + gamma,
  gamma = (R_pad + 4) 2^-24 (|W0| + sum |c_i| |B_i||A_i|);  an all-integer case must come out bit-equal.
Forwards on merged weights: the project's bars against the oracle run on lora_ref's merged weights (bf16 rel-L2 <= 2e-2 against
bf16-rounded weights and inputs, f32 rel-max <= 1e-3), and - the test that every weight-derived cache was invalidated - bit-equality
with a fresh handle created from the weights read back."""
import os
import subprocess
import sys

import pytest
import torch

import lora_ref as R
import ltx_oracle as O
from conftest import rel_l2, rel_max
from test_gpu_normfold import CFGD
from tools_cfg import PIPE_DIT_CFG

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
D = 2048


@pytest.fixture(scope="module")
def hip():
    import ltxhip
    assert torch.cuda.is_available()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return ltxhip


# ---------------------------------------------------------------- 1. the kernel
SHAPES = [(2048, 2048), (8192, 2048), (2048, 8192), (136, 264), (16, 8)]
RANKS = (1, 4, 16, 33, 64, 128, 256)
# one, two and three adapters of different rank; a negative and a zero coefficient among them
MULTI = [((16, 33), (0.75, -1.25)), ((64, 128, 4), (1.0, -0.5, 0.0))]


def _adapter(N, K, r, g):
    return torch.randn(r, K, generator=g) / r ** 0.5, 0.05 * torch.randn(N, r, generator=g)


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("N,K", SHAPES)
def test_merge_kernel_inside_the_derived_bars_and_repeatable(hip, N, K, dt):
    g = torch.Generator().manual_seed(1000 + N + K)
    W0 = (0.02 * torch.randn(N, K, generator=g)).to(DEV)
    cases = [((r,), (1.0 if r != 4 else -2.0,)) for r in RANKS] + MULTI
    for ranks, coefs in cases:
        ads = [(*(t.to(DEV) for t in _adapter(N, K, r, g)), c) for r, c in zip(ranks, coefs)]
        out = hip.ops.lora_merge(W0.to(dt), [(A.to(dt), B.to(dt), c) for A, B, c in ads])
        again = hip.ops.lora_merge(W0.to(dt), [(A.to(dt), B.to(dt), c) for A, B, c in ads])
        torch.cuda.synchronize()
        assert out.dtype == dt and torch.isfinite(out.float()).all()
        assert torch.equal(out, again), (ranks, "not repeatable")
        E, gamma = R.merge(W0, ads, dt)                       # f64, evaluated on the device the tensors live on
        bad, ratio = R.worst(out, E, gamma, dt)
        print({"N": N, "K": K, "dtype": str(dt), "ranks": ranks, "coefs": coefs, "beyond_bar": bad, "worst_error_over_bar": round(ratio, 4)})
        assert bad == 0, (ranks, coefs, bad, ratio)
        assert not torch.equal(out, W0.to(dt)) or all(c == 0.0 for c in coefs)
    # no adapters: a copy
    assert torch.equal(hip.ops.lora_merge(W0.to(dt), []), W0.to(dt))


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
def test_merge_kernel_exact_integers_come_out_bit_equal(hip, dt):
    """W0 integers in [-8, 8], A and B in {-1, 0, 1}, r = 16, coefficient 2: every intermediate is exact, |E| <= 40 is a bf16 number"""
    g = torch.Generator().manual_seed(7)
    for N, K in ((136, 264), (64, 128), (200, 1032)):
        W0 = torch.randint(-8, 9, (N, K), generator=g).double()
        A = torch.randint(-1, 2, (16, K), generator=g).double(); B = torch.randint(-1, 2, (N, 16), generator=g).double()
        want = W0 + 2.0 * (B @ A)
        assert want.abs().max() <= 40
        out = hip.ops.lora_merge(W0.to(dt).to(DEV), [(A.to(dt).to(DEV), B.to(dt).to(DEV), 2.0)])
        assert torch.equal(out.double().cpu(), want), (N, K, int((out.double().cpu() != want).sum()))


# ---------------------------------------------------------------- adapters of the handle tests
# a: all ten linears of layer 0, and attn1.to_k / attn2.to_v of layer 2 (row ranges inside the fused weights); rank 16, alpha 8
# b: rank 33 on ff.net.2 of layers 0 (on top of a) and 1, no alpha
A_TARGETS = [(0, w) for w in range(10)] + [(2, 1), (2, 6)]
B_TARGETS = [(0, 9), (1, 9)]
SCALES = (0.8, -1.1)


@pytest.fixture(scope="module")
def case(hip):
    cfg = O.DitConfig(**CFGD)
    w = O.synth_weights(O.dit_weight_shapes(cfg), seed=71)
    ta = R.synth_adapter((D, D), A_TARGETS, 16, seed=81, alpha=8.0)
    tb = R.synth_adapter((D, D), B_TARGETS, 33, seed=82)
    merged, bars = R.merged_weights(w, [(ta, SCALES[0]), (tb, SCALES[1])], BF16)
    merged32, _ = R.merged_weights(w, [(ta, SCALES[0]), (tb, SCALES[1])], F32)
    return dict(cfg=cfg, w=w, ta=ta, tb=tb, merged=merged, merged32=merged32, bars=bars)


def _model(hip, w, dt=BF16, cfgd=CFGD):
    return hip.LtxVideoTransformer3DModel(hip.LtxVideoTransformer3DModelConfig(**cfgd), {k: v.to(DEV) for k, v in w.items()}, dt)


def _loras(hip, model, case):
    dev = lambda t: {k: v.to(DEV) for k, v in t.items()}
    return [hip.LtxLora.from_tensors(model, dev(case["ta"]), strict=True), hip.LtxLora.from_tensors(model, dev(case["tb"]), strict=True)]


def _read_all(model, L=3):
    out = {(b, wh): model.read_linear(b, wh) for b in range(L) for wh in range(10)}
    torch.cuda.synchronize()
    return out


def _name(b, wh):
    return f"transformer_blocks.{b}.{R.TARGETS[wh]}"


def _weights_from_readback(w, lin):
    w2 = {k: v.to(DEV) for k, v in w.items()}
    for (b, wh), t in lin.items():
        w2[_name(b, wh) + ".weight"] = t
    return w2


# ---------------------------------------------------------------- 2. handle state
def test_handle_weights_follow_the_adapter_list_and_nothing_else(hip, case):
    w = case["w"]
    model = _model(hip, w)
    la, lb = _loras(hip, model, case)
    assert la.n_unmatched == 0 and model.adapter_count() == 0
    base = _read_all(model)
    for (b, wh), t in base.items():
        assert torch.equal(t.cpu(), w[_name(b, wh) + ".weight"].bfloat16()), (b, wh)
    model.set_adapters([la], [SCALES[0]])
    assert model.adapter_count() == 1
    only_a = _read_all(model)
    model.set_adapters([la, lb], SCALES)
    assert model.adapter_count() == 2
    both = _read_all(model)
    targeted = set(A_TARGETS) | set(B_TARGETS)
    for (b, wh), t in both.items():
        if (b, wh) in targeted:
            E, gamma = case["bars"][_name(b, wh)]
            bad, ratio = R.worst(t.cpu(), E, gamma, BF16)
            print({"linear": _name(b, wh), "beyond_bar": bad, "worst_error_over_bar": round(ratio, 4)})
            assert bad == 0, (b, wh, bad, ratio)
            assert not torch.equal(t, base[(b, wh)])
        else:
            assert torch.equal(t, base[(b, wh)]), (b, wh)          # untargeted linears, untargeted rows of a fused weight: the base bits
    assert not torch.equal(only_a[(0, 9)], both[(0, 9)]) and torch.equal(only_a[(0, 3)], both[(0, 3)]) and torch.equal(only_a[(1, 9)], base[(1, 9)])
    # no history: [a] then [a, b] is a fresh handle set to [a, b]
    fresh = _model(hip, w)
    fa, fb = _loras(hip, fresh, case)
    fresh.set_adapters([la, lb], SCALES)                        # (an adapter serves any handle of equal configuration)
    got = _read_all(fresh)
    for k in both:
        assert torch.equal(got[k], both[k]), k
    fresh.set_adapters([fa, fb], SCALES)
    got = _read_all(fresh)
    for k in both:
        assert torch.equal(got[k], both[k]), k
    # n = 0: the base, bit for bit
    model.set_adapters([])
    assert model.adapter_count() == 0
    for k, t in _read_all(model).items():
        assert torch.equal(t, base[k]), k


# ---------------------------------------------------------------- 3. forward and caches
def _inputs(F, H, W, seed=72, K=128):
    g = torch.Generator().manual_seed(seed)
    S = F * H * W
    hidden = torch.randn(1, S, 128, generator=g); enc = torch.randn(1, K, 4096, generator=g)
    mask = torch.zeros(1, K); mask[:, :40] = 1
    return hidden, enc, mask, torch.tensor([896.0]), O.build_video_coords(1, F, H, W)


@pytest.fixture(scope="module")
def oracle(case):
    """O.dit_forward on lora_ref's merged weights, once per geometry: (bf16-rounded weights and inputs, plain f32)"""
    out = {}
    for geo in ((13, 16, 24), (4, 8, 12)):
        hidden, enc, mask, t, coords = _inputs(*geo)
        wr = {k: v.bfloat16().float() for k, v in case["merged"].items()}
        out[geo] = (O.dit_forward(wr, case["cfg"], hidden.bfloat16().float(), enc.bfloat16().float(), t, mask, *geo, None, coords, None),
                    O.dit_forward(case["merged32"], case["cfg"], hidden, enc, t, mask, *geo, None, coords, None))
    return out


def _forward_case(hip, case, geo, want=None, dt=BF16):
    """inside ONE open context_cache scope with the same enc pointer: base forward, set_adapters, forward, clear, forward"""
    hidden, enc, mask, t, coords = _inputs(*geo)
    io = dt
    args = (hidden.to(DEV).to(io), enc.to(DEV).to(io).contiguous(), t, mask.to(DEV), *geo, None, coords.to(DEV), None)
    model = _model(hip, case["w"], dt)
    loras = _loras(hip, model, case)
    model.context_cache(True)
    y0 = model.forward(*args).float().cpu()
    model.set_adapters(loras, SCALES)
    y1 = model.forward(*args).float().cpu()
    lin = _read_all(model)
    model.set_adapters([])
    y2 = model.forward(*args).float().cpu()
    model.context_cache(False)
    assert torch.isfinite(y1).all()
    assert torch.equal(y2, y0), "clearing the adapters did not restore the base forward"
    assert not torch.equal(y1, y0)
    fresh = _model(hip, _weights_from_readback(case["w"], lin), dt)
    yf = fresh.forward(*args).float().cpu()
    assert torch.equal(y1, yf), "a weight-derived cache survived set_adapters: rel-L2 %.3e to a fresh handle on the same weights" % rel_l2(y1, yf)
    if want is not None:
        e = rel_l2(y1, want) if dt == BF16 else rel_max(y1, want)
        print({"geometry": geo, "dtype": str(dt), "vs_oracle_on_merged_weights": round(e, 6), "adapters_moved_the_output_by": round(rel_l2(y1, y0), 4)})
        assert e <= (2e-2 if dt == BF16 else 1e-3), e
    return y1


@pytest.mark.parametrize("nf", ["0", "1", "2"])
def test_forward_after_set_adapters_is_a_fresh_handle_on_the_merged_weights(hip, case, oracle, nf):
    """4992 rows at timestep 896, where the norm fold is live: norm_fold 2 reads the per-timestep scaled weight copies, 1 and 2 the
    shift . W^T + b vectors, all of them the cross-attention K/V of the open context scope"""
    with hip.options(norm_fold=nf):
        _forward_case(hip, case, (13, 16, 24), oracle[(13, 16, 24)][0])


def test_forward_f32_handle(hip, case, oracle):
    _forward_case(hip, case, (13, 16, 24), oracle[(13, 16, 24)][1], F32)


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
def test_forward_at_384_rows(hip, case, oracle, dt):
    """(4, 8, 12): the small-M (ring) tiles, deferred ff2, one-row-per-block norms"""
    _forward_case(hip, case, (4, 8, 12), oracle[(4, 8, 12)][0 if dt == BF16 else 1], dt)


def _child_384():
    """entry of the child process below"""
    import ltxhip
    cfg = O.DitConfig(**CFGD)
    c = dict(cfg=cfg, w=O.synth_weights(O.dit_weight_shapes(cfg), seed=71), ta=R.synth_adapter((D, D), A_TARGETS, 16, seed=81, alpha=8.0),
             tb=R.synth_adapter((D, D), B_TARGETS, 33, seed=82))
    _forward_case(ltxhip, c, (4, 8, 12))
    print("child-ok experiments=%d" % int(ltxhip.has_experiments()))


def test_forward_at_384_rows_with_packed_ring_weights_in_a_child_process():
    """LTX_RING_PACK=1 / x_ring_pack=1: small-M calls read a tile-contiguous second copy of the weights (LinearW::wp), built on the
    first call - another function of the weights that set_adapters has to drop.  The copy exists in experiment builds only
    (ltx_has_experiments); the shipped library ignores the switch and the child repeats the 384-row case."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, LTX_RING_PACK="1", LTX_OPTIONS="x_ring_pack=1")
    code = "import sys; sys.path.insert(0, %r); import conftest, test_gpu_lora as T; T._child_384()" % here
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "child-ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


# ---------------------------------------------------------------- 4. pipeline
def test_pipeline_call_runs_on_the_adapted_handle(hip, case):
    """C1 geometry (256 x 384 x 25 -> 384 tokens, 128 text tokens) on the three-layer model, 2 steps with CFG: adapters are handle
    state, so ltx_pipeline_call needs no argument for them - it equals the call on a fresh handle built from the read-back weights"""
    F, H, W = 4, 8, 12
    lat = O.pack_latents(O.Pcg32(42, 1442695040888963407).randn((1, 128, F, H, W))).to(DEV)
    g = torch.Generator().manual_seed(42)
    pe = torch.randn(1, 128, 4096, generator=g).to(DEV); ne = torch.randn(1, 128, 4096, generator=g).to(DEV)
    pm = torch.zeros(1, 128); pm[:, :32] = 1; nm = torch.zeros(1, 128); nm[:, :20] = 1
    call = hip.PipelineCall(height=256, width=384, num_frames=25, num_inference_steps=2, sigmas=[1.0, 0.6], guidance_scale=3.0, output_latent=True)
    run = lambda m: hip.LtxPipeline(m, None).call(call, lat, pe, pm.to(DEV), ne, nm.to(DEV))[0].float().cpu()
    model = _model(hip, case["w"])
    base = run(model)
    model.set_adapters(_loras(hip, model, case), SCALES)
    got = run(model)
    fresh = _model(hip, _weights_from_readback(case["w"], _read_all(model)))
    assert torch.isfinite(got).all() and not torch.equal(got, base)
    assert torch.equal(got, run(fresh))
    model.set_adapters([])
    assert torch.equal(run(model), base)


# ---------------------------------------------------------------- 5. files and errors
TINY_D = PIPE_DIT_CFG["num_attention_heads"] * PIPE_DIT_CFG["attention_head_dim"]
TINY_TARGETS = [(0, 0), (0, 2), (0, 5), (1, 8), (2, 9), (2, 3)]
SPELLINGS = ((".lora_A.weight", ".lora_B.weight"), (".lora_down.weight", ".lora_up.weight"), (".lora.down.weight", ".lora.up.weight"))


def _respell(tensors, spelling, prefix=""):
    out = {}
    for k, v in tensors.items():
        k = k.replace(".lora_A.weight", spelling[0]).replace(".lora_B.weight", spelling[1])
        out[prefix + k] = v.contiguous()
    return out


def _tiny(hip, heads=None):
    cfgd = dict(PIPE_DIT_CFG)
    if heads:
        cfgd.update(num_attention_heads=heads, cross_attention_dim=heads * cfgd["attention_head_dim"])
    w = O.synth_weights(O.dit_weight_shapes(O.DitConfig(**cfgd)), seed=11)
    return _model(hip, w, BF16, cfgd), w


def test_adapter_files_in_every_spelling_give_the_same_weights(hip, tmp_path):
    from safetensors.torch import save_file
    model, w = _tiny(hip)
    plain = R.synth_adapter((TINY_D, TINY_D), TINY_TARGETS, 4, seed=91)
    with_alpha = R.synth_adapter((TINY_D, TINY_D), TINY_TARGETS, 4, seed=91, alpha=2.0)
    results = {}
    for alpha, tensors in ((False, plain), (True, with_alpha)):
        for i, (sp, prefix) in enumerate(zip(SPELLINGS, ("", "transformer.", "diffusion_model."))):
            path = str(tmp_path / f"adapter_{int(alpha)}_{i}.safetensors")
            t = _respell(tensors, sp, prefix)
            if i == 1:
                t = {k: (v.bfloat16() if not k.endswith(".alpha") else v) for k, v in t.items()}        # a BF16 payload too
            save_file(t, path)
            lora = hip.LtxLora.from_file(model, path, strict=True)
            assert lora.n_unmatched == 0
            model.set_adapters([lora], [1.5])
            results[(alpha, i)] = _read_all(model)
    model.set_adapters([])
    for alpha in (False, True):
        for i in (1, 2):
            for k in results[(alpha, 0)]:
                assert torch.equal(results[(alpha, i)][k], results[(alpha, 0)][k]), (alpha, i, k)
    # the file path is the tensor path; alpha / r = 0.5 halves the coefficient
    model.set_adapters([hip.LtxLora.from_tensors(model, {k: v.to(DEV) for k, v in plain.items()})], [0.75])
    half = _read_all(model)
    for b, wh in TINY_TARGETS:
        assert torch.equal(half[(b, wh)], results[(True, 0)][(b, wh)]) and not torch.equal(half[(b, wh)], results[(False, 0)][(b, wh)])
        E, gamma = R.merge(w[_name(b, wh) + ".weight"], [(plain[_name(b, wh) + ".lora_A.weight"], plain[_name(b, wh) + ".lora_B.weight"], R.coef(1.5, None, 4))], BF16)
        assert R.worst(results[(False, 0)][(b, wh)].cpu(), E, gamma, BF16)[0] == 0


def test_errors_name_the_key_and_leave_the_handle_unchanged(hip, tmp_path):
    from safetensors.torch import save_file
    model, w = _tiny(hip)
    good = R.synth_adapter((TINY_D, TINY_D), TINY_TARGETS, 4, seed=92)
    dev = lambda t: {k: v.to(DEV) for k, v in t.items()}
    lora = hip.LtxLora.from_tensors(model, dev(good))
    model.set_adapters([lora], [1.0])
    before = _read_all(model)

    def unchanged():
        assert model.adapter_count() == 1
        for k, t in _read_all(model).items():
            assert torch.equal(t, before[k]), k

    # adapter keys on something that is not a block linear: counted, refused under strict (first such key named)
    extra = dict(good)
    extra["proj_in.lora_A.weight"] = torch.zeros(4, 8); extra["proj_in.lora_B.weight"] = torch.zeros(TINY_D, 4)
    extra["transformer_blocks.7.attn1.to_q.lora_A.weight"] = torch.zeros(4, TINY_D)      # a block the config does not have
    extra["transformer_blocks.0.attn1.norm_q.alpha"] = torch.tensor(1.0)
    extra["transformer_blocks.0.attn1.to_q.weight"] = torch.zeros(TINY_D, TINY_D)         # not an adapter key at all: ignored
    assert hip.LtxLora.from_tensors(model, extra).n_unmatched == 4
    with pytest.raises(hip.LtxError, match=r"rc=4\].*'proj_in\.lora_A\.weight'"):
        hip.LtxLora.from_tensors(model, extra, strict=True)
    path = str(tmp_path / "unmatched.safetensors")
    save_file({"diffusion_model." + k: v.contiguous() for k, v in extra.items()}, path)
    assert hip.LtxLora.from_file(model, path).n_unmatched == 4
    with pytest.raises(hip.LtxError, match=r"rc=4\].*proj_in\.lora_A\.weight"):
        hip.LtxLora.from_file(model, path, strict=True)
    # an A without its B
    lone = {k: v for k, v in good.items() if k != "transformer_blocks.1.ff.net.0.proj.lora_B.weight"}
    with pytest.raises(hip.LtxError, match=r"rc=1\].*'transformer_blocks\.1\.ff\.net\.0\.proj\.lora_A\.weight' has no matching B"):
        hip.LtxLora.from_tensors(model, lone)
    # a wrong in / out, a rank mismatch inside the pair
    bad_in = dict(good); bad_in["transformer_blocks.2.ff.net.2.lora_A.weight"] = torch.zeros(4, TINY_D)          # ff.net.2 reads 4 D
    with pytest.raises(hip.LtxError, match=r"rc=1\].*'transformer_blocks\.2\.ff\.net\.2\.lora_A\.weight' must be \[r, %d\]" % (4 * TINY_D)):
        hip.LtxLora.from_tensors(model, bad_in)
    bad_out = dict(good); bad_out["transformer_blocks.0.attn1.to_q.lora_B.weight"] = torch.zeros(TINY_D + 8, 4)
    with pytest.raises(hip.LtxError, match=r"rc=1\].*'transformer_blocks\.0\.attn1\.to_q\.lora_B\.weight' must be \[%d, r\]" % TINY_D):
        hip.LtxLora.from_tensors(model, bad_out)
    bad_r = dict(good); bad_r["transformer_blocks.0.attn1.to_q.lora_B.weight"] = torch.zeros(TINY_D, 5)
    with pytest.raises(hip.LtxError, match=r"rc=1\].*'transformer_blocks\.0\.attn1\.to_q\.lora_B\.weight': rank 5 does not match"):
        hip.LtxLora.from_tensors(model, bad_r)
    # rank 257
    big = {"transformer_blocks.0.attn1.to_q.lora_A.weight": torch.zeros(257, TINY_D), "transformer_blocks.0.attn1.to_q.lora_B.weight": torch.zeros(TINY_D, 257)}
    with pytest.raises(hip.LtxError, match=r"rc=1\].*'transformer_blocks\.0\.attn1\.to_q\.lora_A\.weight': rank 257"):
        hip.LtxLora.from_tensors(model, big)
    ok256 = {k: torch.zeros(256, TINY_D) if "lora_A" in k else torch.zeros(TINY_D, 256) for k in big}
    assert hip.LtxLora.from_tensors(model, ok256).n_unmatched == 0
    unchanged()
    # n = 9
    with pytest.raises(hip.LtxError, match=r"rc=1\].*9 adapters"):
        model.set_adapters([lora] * 9, [1.0] * 9)
    unchanged()
    # an adapter built for another width
    wide, _ = _tiny(hip, heads=4)
    other = hip.LtxLora.from_tensors(wide, dev(R.synth_adapter((2 * TINY_D, 2 * TINY_D), [(0, 0)], 4, seed=93)))
    with pytest.raises(hip.LtxError, match=r"rc=1\].*adapter 1 was built for another configuration"):
        model.set_adapters([lora, other], [1.0, 1.0])
    unchanged()
    # and one built for another model dtype
    f32_model = _model(hip, w, F32, PIPE_DIT_CFG)
    with pytest.raises(hip.LtxError, match=r"rc=1\].*another configuration"):
        f32_model.set_adapters([lora], [1.0])
    assert f32_model.adapter_count() == 0
    # a file payload that is neither F32 nor BF16
    path = str(tmp_path / "f16.safetensors")
    save_file({k: v.half() for k, v in good.items()}, path)
    with pytest.raises(hip.LtxError, match=r"rc=4\].*is F16"):
        hip.LtxLora.from_file(model, path)
    unchanged()
