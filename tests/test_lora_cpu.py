"""CPU suite: the host half of include/ltxhip_lora.h (exported and bound symbols, the adapter key parser) and tests/lora_ref.py
pinned to the DEFINITION of LoRA rather than to itself: a merged linear equals the base linear plus the low-rank branch, including
the row ranges an adapter addresses inside the engine's fused q|k|v and k|v weights."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import lora_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LTX_ERR_ARG = 1


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ltx_[a-z0-9_]+)\s*\(", src)))


def test_lora_symbols_are_exported_and_bound():
    import ltxhip
    lib = ctypes.CDLL(os.path.join(ROOT, "candle-video_amd", "libltxhip.so"))
    names = _declared("ltxhip_lora.h")
    assert len(names) == 8 and set(names) == set(ltxhip.LORA_SYMBOLS)
    for n in names:
        assert hasattr(lib, n), n
    for attr in ("set_adapters", "adapter_count", "read_linear"):
        assert hasattr(ltxhip.LtxVideoTransformer3DModel, attr)
    assert hasattr(ltxhip.LtxLora, "from_file") and hasattr(ltxhip.LtxLora, "from_tensors") and hasattr(ltxhip.ops, "lora_merge")
    assert tuple(ltxhip.LORA_TARGETS) == R.TARGETS
    rust = open(os.path.join(ROOT, "rust", "ltxhip-sys", "src", "lib.rs")).read()
    assert set(names) <= set(re.findall(r"pub fn (ltx_\w+)\(", rust))


PREFIXES = ("", "transformer.", "diffusion_model.", "model.diffusion_model.")
SUFFIXES = ((".lora_A.weight", 0), (".lora_B.weight", 1), (".lora_down.weight", 0), (".lora_up.weight", 1), (".lora.down.weight", 0), (".lora.up.weight", 1),
            (".alpha", 2))


def test_parse_key_every_prefix_and_suffix():
    import ltxhip
    for mod in ("transformer_blocks.27.attn1.to_out.0", "transformer_blocks.0.ff.net.0.proj", "transformer_blocks.3.attn2.to_k"):
        for p in PREFIXES:
            for s, role in SUFFIXES:
                assert ltxhip.lora_parse_key(p + mod + s) == (mod, role), (p, mod, s)
    # only ONE prefix goes
    assert ltxhip.lora_parse_key("transformer.transformer.x.lora_A.weight") == ("transformer.x", 0)


def test_parse_key_official_layout_names_resolve_as_checkpoints_do():
    import ltxhip
    assert ltxhip.lora_parse_key("model.diffusion_model.patchify_proj.lora_A.weight") == ("proj_in", 0)
    assert ltxhip.lora_parse_key("diffusion_model.adaln_single.linear.lora_up.weight") == ("time_embed.linear", 1)
    assert ltxhip.lora_parse_key("transformer_blocks.2.attn1.q_norm.alpha") == ("transformer_blocks.2.attn1.norm_q", 2)
    buf = ctypes.create_string_buffer(1024)
    for key in ("transformer_blocks.1.attn2.k_norm.lora.down.weight", "transformer_blocks.1.ff.net.2.lora_B.weight"):
        ltxhip.lib.ltx_weights_remap_key(key.rsplit(".lora", 1)[0].encode(), buf, 1024)
        assert ltxhip.lora_parse_key(key)[0] == buf.value.decode()


def test_parse_key_refuses_what_is_not_an_adapter_key():
    import ltxhip
    L = ltxhip.lib
    buf = ctypes.create_string_buffer(256); role = ctypes.c_int(7)
    for key in ("transformer_blocks.0.attn1.to_q.weight", "transformer_blocks.0.attn1.to_q.bias", "transformer_blocks.0.attn1.to_q.lora_A", "lora_A.weight.x",
                "transformer_blocks.0.scale_shift_table", "", ".alpha", "transformer..alpha"):
        assert L.ltx_lora_parse_key(key.encode(), buf, 256, ctypes.byref(role)) == LTX_ERR_ARG, key
        assert role.value == 7
    assert b"not an adapter tensor name" in L.ltx_last_error() or b"names no module" in L.ltx_last_error()
    assert L.ltx_lora_parse_key(None, buf, 256, ctypes.byref(role)) == LTX_ERR_ARG
    assert L.ltx_lora_parse_key(b"a.alpha", None, 256, ctypes.byref(role)) == LTX_ERR_ARG
    small = ctypes.create_string_buffer(4)
    assert L.ltx_lora_parse_key(b"transformer_blocks.0.attn1.to_q.alpha", small, 4, ctypes.byref(role)) == LTX_ERR_ARG
    assert b"too small" in L.ltx_last_error()
    with pytest.raises(ltxhip.LtxError, match="rc=1"):
        ltxhip.lora_parse_key("proj_out.weight")


def test_host_argument_errors_need_no_device():
    import ltxhip
    L = ltxhip.lib
    one = ctypes.c_void_p(8)
    out = ctypes.c_void_p()
    assert L.ltx_lora_create(None, None, 0, 0, ctypes.byref(out), None) == LTX_ERR_ARG
    assert L.ltx_lora_create_from_file(None, b"x.safetensors", 0, ctypes.byref(out), None) == LTX_ERR_ARG
    assert L.ltx_dit_set_adapters(None, None, None, 0, None) == LTX_ERR_ARG
    assert L.ltx_dit_read_linear(None, 0, 0, one, None) == LTX_ERR_ARG
    assert L.ltx_dit_adapter_count(None) == 0
    L.ltx_lora_destroy(None)
    r = (ctypes.c_int * 1)(16); c = (ctypes.c_float * 1)(1.0); p = (ctypes.c_void_p * 1)(8)
    assert L.ltx_op_lora_merge(one, one, 16, 8, 0, None, None, None, None, 1, None) == LTX_ERR_ARG           # out aliases w0
    assert L.ltx_op_lora_merge(one, ctypes.c_void_p(16), 16, 12, 0, None, None, None, None, 1, None) == LTX_ERR_ARG      # K % 8
    assert L.ltx_op_lora_merge(one, ctypes.c_void_p(16), 16, 8, 9, p, p, r, c, 1, None) == LTX_ERR_ARG
    r[0] = 257
    assert L.ltx_op_lora_merge(one, ctypes.c_void_p(16), 16, 8, 1, p, p, r, c, 1, None) == LTX_ERR_ARG
    assert b"1..256" in L.ltx_last_error()


def test_merge_is_the_definition_of_lora_on_one_linear():
    g = torch.Generator().manual_seed(3)
    out_f, in_f, r = 24, 40, 5
    W0 = torch.randn(out_f, in_f, generator=g, dtype=torch.float64)
    A = torch.randn(r, in_f, generator=g, dtype=torch.float64); B = torch.randn(out_f, r, generator=g, dtype=torch.float64)
    A2 = torch.randn(3, in_f, generator=g, dtype=torch.float64); B2 = torch.randn(out_f, 3, generator=g, dtype=torch.float64)
    x = torch.randn(7, in_f, generator=g, dtype=torch.float64)
    c, c2 = R.coef(0.75, 8.0, r), R.coef(-1.5, None, 3)
    assert c == 0.75 * (8.0 / 5.0) or abs(c - 1.2) < 1e-6
    E, gamma = R.merge(W0, [(A, B, c), (A2, B2, c2)], torch.float64)
    want = F.linear(x, W0) + c * F.linear(F.linear(x, A), B) + c2 * F.linear(F.linear(x, A2), B2)
    assert (F.linear(x, E) - want).abs().max() <= 1e-10
    assert torch.allclose(R.lora_delta_forward(x, W0, A, B, c), F.linear(x, R.merge(W0, [(A, B, c)], torch.float64)[0]), rtol=0, atol=1e-10)
    assert (gamma > 0).all() and gamma.shape == W0.shape


def test_merge_inside_the_fused_weights_addresses_the_adapters_rows():
    """to_k / to_v inside q|k|v and to_v inside k|v: merging the row range of the fused matrix is merging the separate linear"""
    g = torch.Generator().manual_seed(4)
    D, r = 16, 3
    x = torch.randn(5, D, generator=g, dtype=torch.float64)
    sep = {n: torch.randn(D, D, generator=g, dtype=torch.float64) for n in ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn2.to_k", "attn2.to_v")}
    fused = {"qkv1": torch.cat([sep["attn1.to_q"], sep["attn1.to_k"], sep["attn1.to_v"]]), "kv2": torch.cat([sep["attn2.to_k"], sep["attn2.to_v"]])}
    for which in (1, 2, 6):
        name, row = R.fused_rows(which, D)
        A = torch.randn(r, D, generator=g, dtype=torch.float64); B = torch.randn(D, r, generator=g, dtype=torch.float64)
        c = R.coef(1.25, 2.0, r)
        Wf = fused[name].clone()
        Wf[row:row + D] = R.merge(Wf[row:row + D], [(A, B, c)], torch.float64)[0]
        y = F.linear(x, Wf)
        target = R.TARGETS[which]
        for n, w in sep.items():
            if n.split(".")[0] != target.split(".")[0]:
                continue
            nm, rw = R.fused_rows(R.TARGETS.index(n), D)
            want = R.lora_delta_forward(x, w, A, B, c) if n == target else F.linear(x, w)
            assert (y[:, rw:rw + D] - want).abs().max() <= 1e-10, (which, n)
    assert R.fused_rows(3, D) == (None, 0) and R.fused_rows(0, D) == ("qkv1", 0) and R.fused_rows(5, D) == ("kv2", 0)


@pytest.mark.parametrize("N,K,ranks", [(136, 264, (1, 33)), (512, 256, (16,)), (96, 1024, (64, 128, 4))])
def test_f32_accumulate_restatement_is_inside_the_bars(N, K, ranks):
    """the bars are derived, not measured: the engine's arithmetic restated in torch (f32 accumulation, one fma per adapter, one
    rounding of the result) must never leave them"""
    g = torch.Generator().manual_seed(5)
    W0 = 0.02 * torch.randn(N, K, generator=g)
    ads = [(torch.randn(r, K, generator=g) / r ** 0.5, 0.05 * torch.randn(N, r, generator=g), s) for r, s in zip(ranks, (1.0, -0.5, 0.75))]
    for dt in (torch.bfloat16, torch.float32):
        E, gamma = R.merge(W0, ads, dt)
        bad, ratio = R.worst(R.merge_f32acc(W0, ads, dt), E, gamma, dt)
        assert bad == 0 and ratio <= 1.0, (dt, bad, ratio)
    # and the bar is not vacuous: an error of one bf16 ulp is caught
    E, gamma = R.merge(W0, ads, torch.bfloat16)
    off = R.merge_f32acc(W0, ads, torch.bfloat16).double() + 1.01 * R.ulp_bf16(E)
    assert R.worst(off, E, gamma, torch.bfloat16)[0] > 0
    assert float(R.ulp_bf16(torch.tensor([1.0, 1.5, 2.0, 0.0, -0.75], dtype=torch.float64)).sub(torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 0.0, 2.0 ** -8], dtype=torch.float64)).abs().max()) == 0.0


@pytest.mark.skipif(__import__("shutil").which("g++") is None, reason="needs g++")
def test_key_parser_is_clean_under_asan_and_ubsan():
    """host/lora.cpp built for the host alone with AddressSanitizer + UBSan and driven by a stand-alone program
    (tests/host/lora_asan_main.cpp): exact-fit and too-small buffers, long keys, names the remapper lengthens"""
    import subprocess
    pkg = os.path.join(ROOT, "candle-video_amd")
    b = subprocess.run(["make", "-C", pkg, "asan_lora"], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(pkg, "build", "asan", "ltx_lora_asan")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert "lora host sanitizer driver: clean" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr
