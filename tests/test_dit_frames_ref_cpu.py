"""CPU suite: pins tests/dit_frames_ref.py (per-frame timesteps, held conditioning frames) against the oracle where the two must
coincide, and checks the host half of include/ltxhip_cond.h: exported and bound symbols, the layout of ltx_conditioning against
its ctypes mirror and the Rust constant, and the argument errors that need no device."""
import ctypes
import json
import os
import re
import subprocess

import torch

import dit_frames_ref as R
import ltx_oracle as O
from tools_cfg import PIPE_DIT_CFG, VAE_CFG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LTX_ERR_ARG = 1


def _dit(seed=11):
    cfg = O.DitConfig(**PIPE_DIT_CFG)
    return cfg, O.synth_weights(O.dit_weight_shapes(cfg), seed=seed)


def _dit_inputs(B, F, H, W, K=16, seed=5):
    g = torch.Generator().manual_seed(seed)
    hidden = torch.randn(B, F * H * W, 8, generator=g); enc = torch.randn(B, K, 32, generator=g)
    mask = torch.zeros(B, K); mask[:, :9] = 1
    return hidden, enc, mask, O.build_video_coords(B, F, H, W)


def test_equal_frame_timesteps_are_the_oracle_forward_bit_for_bit():
    cfg, w = _dit()
    B, F, H, W = 2, 3, 2, 3
    hidden, enc, mask, coords = _dit_inputs(B, F, H, W)
    t = torch.tensor([896.0, 100.0])
    slm = torch.zeros(cfg.num_layers, B); slm[1, 1] = 1.0
    for kw in (dict(), dict(skip_layer_mask=slm), dict(skip_block_list=[2])):
        want = O.dit_forward(w, cfg, hidden, enc, t, mask, F, H, W, None, coords, **kw)
        got = R.dit_forward_frames(w, cfg, hidden, enc, t.reshape(B, 1).expand(B, F).contiguous(), mask, F, H, W, None, coords, **kw)
        assert torch.equal(got, want), kw
    # without coords (the grid's own RoPE positions) as well
    assert torch.equal(R.dit_forward_frames(w, cfg, hidden, enc, t.reshape(B, 1).expand(B, F).contiguous(), mask, F, H, W),
                       O.dit_forward(w, cfg, hidden, enc, t, mask, F, H, W))


def test_a_frame_sees_its_own_timestep():
    """Modulation is per token, but attention mixes tokens: the check is on the first block's modulated input, which is local.
    A forward whose frame f alone differs must agree with the uniform forwards on NO frame exactly (attention), while a model
    with zeroed attention output projections makes frames independent: frame f then equals the uniform forward at ITS timestep."""
    cfg, w = _dit()
    w = dict(w)
    for k in list(w):
        if "to_out.0" in k:
            w[k] = torch.zeros_like(w[k])                                          # frames no longer interact
    B, F, H, W = 1, 3, 2, 3
    hidden, enc, mask, coords = _dit_inputs(B, F, H, W)
    tf = torch.tensor([[0.0, 640.0, 896.0]])
    got = R.dit_forward_frames(w, cfg, hidden, enc, tf, mask, F, H, W, None, coords)
    for f in range(F):
        uni = O.dit_forward(w, cfg, hidden, enc, tf[:, f], mask, F, H, W, None, coords)
        sl = slice(f * H * W, (f + 1) * H * W)
        assert torch.allclose(got[:, sl], uni[:, sl], rtol=1e-5, atol=1e-6), f
        other = slice(((f + 1) % F) * H * W, ((f + 1) % F + 1) * H * W)
        assert not torch.allclose(got[:, other], uni[:, other], rtol=1e-3, atol=1e-4)


def _pipe_case(do_cfg=True):
    dcfg, dw = _dit()
    vcfg = O.VaeConfig(**VAE_CFG)
    vw = O.synth_weights(O.vae_decoder_weight_shapes(vcfg), seed=12)
    g = torch.Generator().manual_seed(13)
    F, H, W = 2, 2, 3
    lat = O.pack_latents(O.Pcg32(42, 1442695040888963407).randn((1, 8, F, H, W)))
    pe = torch.randn(1, 16, 32, generator=g); pm = torch.zeros(1, 16); pm[:, :9] = 1
    ne = torch.randn(1, 16, 32, generator=g); nm = torch.zeros(1, 16); nm[:, :5] = 1
    args = O.PipelineArgs(height=64, width=96, num_frames=9, num_inference_steps=2, sigmas=[1.0, 0.6],
                          guidance_scale=3.0 if do_cfg else 1.0, guidance_rescale=0.7 if do_cfg else 0.0,
                          stg_scale=1.0 if do_cfg else 0.0, skip_block_list=[1] if do_cfg else None)
    mean, std = torch.zeros(8), torch.ones(8)
    return dcfg, dw, vcfg, vw, mean, std, args, lat, pe, pm, ne, nm, (F, H, W)


def test_hold_all_zero_is_the_oracle_pipeline_bit_for_bit():
    for do_cfg in (False, True):
        dcfg, dw, vcfg, vw, mean, std, args, lat, pe, pm, ne, nm, (F, H, W) = _pipe_case(do_cfg)
        want = O.pipeline_call(dw, dcfg, vw, vcfg, mean, std, args, lat, pe, pm, ne, nm, None, torch.float32)
        got = R.pipeline_call_cond(dw, dcfg, vw, vcfg, mean, std, args, lat, torch.zeros(1, F), pe, pm, ne, nm, None, torch.float32)
        assert torch.equal(got, want), do_cfg


def test_hold_all_one_leaves_the_latents_unchanged_and_a_held_frame_keeps_its_bits():
    dcfg, dw, vcfg, vw, mean, std, args, lat, pe, pm, ne, nm, (F, H, W) = _pipe_case(True)
    args.output_latent = True
    out = R.pipeline_call_cond(dw, dcfg, vw, vcfg, mean, std, args, lat, torch.ones(1, F), pe, pm, ne, nm, None, torch.float32)
    assert torch.equal(out, lat)
    out = R.pipeline_call_cond(dw, dcfg, vw, vcfg, mean, std, args, lat, torch.tensor([[1, 0]]), pe, pm, ne, nm, None, torch.float32)
    hw = H * W
    assert torch.equal(out[:, :hw], lat[:, :hw]) and not torch.equal(out[:, hw:], lat[:, hw:])
    free = O.pipeline_call(dw, dcfg, vw, vcfg, mean, std, args, lat, pe, pm, ne, nm, None, torch.float32)
    assert not torch.allclose(out[:, hw:], free[:, hw:], rtol=1e-4, atol=1e-5)     # the free frame saw a frame at timestep 0


# ---- host half of the C ABI ----

def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ltx_[a-z0-9_]+)\s*\(", src)))


def test_cond_symbols_are_exported_and_bound():
    import ltxhip
    lib = ctypes.CDLL(os.path.join(ROOT, "candle-video_amd", "libltxhip.so"))
    names = _declared("ltxhip_cond.h")
    assert len(names) == 5 and set(names) == set(ltxhip.COND_SYMBOLS)
    for n in names:
        assert hasattr(lib, n), n
    for attr in ("forward_frames",):
        assert hasattr(ltxhip.LtxVideoTransformer3DModel, attr)
    assert hasattr(ltxhip.ops, "guidance_step") and hasattr(ltxhip, "cond_apply")
    rust = open(os.path.join(ROOT, "rust", "ltxhip-sys", "src", "lib.rs")).read()
    assert set(names) <= set(re.findall(r"pub fn (ltx_\w+)\(", rust))


def test_conditioning_layout_matches_ctypes_and_rust(tmp_path):
    import ltxhip
    exe = str(tmp_path / "cabi_layout_cond")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cabi_layout_cond.c"), "-o", exe], check=True)
    c = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)["ltx_conditioning"]
    cls = ltxhip.ConditioningC
    assert (ctypes.sizeof(cls), ctypes.alignment(cls)) == (c["size"], c["align"])
    assert [f[0] for f in cls._fields_] == list(c["fields"]) and cls.hold.offset == c["fields"]["hold"]
    src = open(os.path.join(ROOT, "rust", "ltxhip-sys", "src", "lib.rs")).read()
    m = re.search(r"pub const COND_LAYOUT_LTX_CONDITIONING: \(usize, usize\) = \((\d+), (\d+)\);", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (c["size"], c["align"])
    body = re.search(r"pub struct ltx_conditioning \{(.*?)\n\}", src, re.S).group(1)
    assert re.findall(r"pub (\w+):", body) == list(c["fields"])


def test_argument_errors_without_a_device():
    import ltxhip
    L = ltxhip.lib
    one = ctypes.c_void_p(16)                                   # a non-null pointer that is never dereferenced: every call fails on its arguments
    t = (ctypes.c_float * 6)(*[0.0] * 6)
    # S != F' * h * w, with and without video_coords
    assert L.ltx_dit_forward_frames(one, one, one, t, None, 1, 35, 4, 3, 3, 4, None, None, None, 0, one, None) == LTX_ERR_ARG
    assert b"num_frames*height*width" in L.ltx_last_error()
    assert L.ltx_dit_forward_frames(one, one, one, t, None, 1, 35, 4, 3, 3, 4, None, one, None, 0, one, None) == LTX_ERR_ARG
    assert L.ltx_dit_forward_frames(None, one, one, t, None, 1, 36, 4, 3, 3, 4, None, None, None, 0, one, None) == LTX_ERR_ARG
    assert L.ltx_dit_forward_frames(one, one, one, None, None, 1, 36, 4, 3, 3, 4, None, None, None, 0, one, None) == LTX_ERR_ARG
    # a held frame beyond the conditioning frames; a null hold
    hold = (ctypes.c_ubyte * 4)(1, 0, 1, 0)
    assert L.ltx_cond_apply(one, one, 2, hold, 1, 4, 6, 8, None) == LTX_ERR_ARG
    assert b"held frame 2" in L.ltx_last_error()
    assert L.ltx_cond_apply(one, one, 2, None, 1, 4, 6, 8, None) == LTX_ERR_ARG
    assert L.ltx_cond_apply(None, one, 2, hold, 1, 4, 6, 8, None) == LTX_ERR_ARG
    nothing = (ctypes.c_ubyte * 4)(0, 0, 0, 0)
    assert L.ltx_cond_apply(one, one, 2, nothing, 1, 4, 6, 8, None) == 0          # nothing held: nothing to copy, no device touched
    z = ctypes.c_float(0.0)
    assert L.ltx_guidance_step_held(one, None, None, 0, one, None, 1, ctypes.c_int64(48), z, z, z, z, None, None, 4, ctypes.c_int64(12), None) == LTX_ERR_ARG
    assert L.ltx_guidance_step_held(one, None, None, 0, one, None, 1, ctypes.c_int64(48), z, z, z, z, None, one, 4, ctypes.c_int64(11), None) == LTX_ERR_ARG
    assert L.ltx_guidance_step_stochastic_held(one, None, None, 0, one, None, 1, ctypes.c_int64(48), z, z, z, z, z, one, None, None, 4, ctypes.c_int64(12), None) == LTX_ERR_ARG
    p = ltxhip.PipelineParamsC(); L.ltx_pipeline_params_default(ctypes.byref(p))
    assert L.ltx_pipeline_call_cond(one, None, ctypes.byref(p), None, one, one, one, None, None, None, 1, 4, None, None) == LTX_ERR_ARG
    cond = ltxhip.ConditioningC()
    assert L.ltx_pipeline_call_cond(one, None, ctypes.byref(p), ctypes.byref(cond), one, one, one, None, None, None, 1, 4, None, None) == LTX_ERR_ARG
    assert b"hold" in L.ltx_last_error()
    # the Python side refuses the same before any pointer is taken
    import pytest
    with pytest.raises(ltxhip.LtxError, match="2 x 3"):
        ltxhip._hold_host([[1, 0, 0]], 2, 3)
