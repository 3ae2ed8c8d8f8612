"""CPU suite: pins tests/keyframes_ref.py (keyframe conditioning, include/ltxhip_keyframes.h) where it must coincide with what is
already pinned - no items: the oracle's pipeline; one image at frame 0 at full strength: tests/dit_frames_ref.py's held pipeline - and
checks the update predicate and the model timestep on a table.  The host half of the header: exported, bound and declared symbols,
the layout of ltx_cond_item / ltx_cond_group against the ctypes mirrors and the Rust constants, the host entries against the
reference, and the argument errors that need no device."""
import ctypes
import json
import os
import re
import subprocess

import pytest
import torch

import dit_frames_ref as RF
import keyframes_ref as KR
import ltx_oracle as O
from tools_cfg import PIPE_DIT_CFG, VAE_CFG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LTX_OK, LTX_ERR_ARG = 0, 1


def _pipe_case(do_cfg=True):
    dcfg = O.DitConfig(**PIPE_DIT_CFG)
    dw = O.synth_weights(O.dit_weight_shapes(dcfg), seed=11)
    vcfg = O.VaeConfig(**VAE_CFG)
    vw = O.synth_weights(O.vae_decoder_weight_shapes(vcfg), seed=12)
    g = torch.Generator().manual_seed(13)
    F, H, W = 2, 2, 3
    lat = O.pack_latents(O.Pcg32(42, 1442695040888963407).randn((1, 8, F, H, W)))
    pe = torch.randn(1, 16, 32, generator=g); pm = torch.zeros(1, 16); pm[:, :9] = 1
    ne = torch.randn(1, 16, 32, generator=g); nm = torch.zeros(1, 16); nm[:, :5] = 1
    img = torch.randn(1, H * W, 8, generator=g)
    args = O.PipelineArgs(height=64, width=96, num_frames=9, num_inference_steps=2, sigmas=[1.0, 0.6],
                          guidance_scale=3.0 if do_cfg else 1.0, guidance_rescale=0.7 if do_cfg else 0.0,
                          stg_scale=1.0 if do_cfg else 0.0, skip_block_list=[1] if do_cfg else None)
    return dcfg, dw, vcfg, vw, torch.zeros(8), torch.ones(8), args, lat, pe, pm, ne, nm, img, (F, H, W)


def test_no_items_is_the_oracle_pipeline_bit_for_bit():
    for do_cfg in (False, True):
        dcfg, dw, vcfg, vw, mean, std, args, lat, pe, pm, ne, nm, _, _ = _pipe_case(do_cfg)
        want = O.pipeline_call(dw, dcfg, vw, vcfg, mean, std, args, lat, pe, pm, ne, nm, None, torch.float32)
        got = KR.pipeline_call_keyframes(dw, dcfg, vw, vcfg, mean, std, args, lat, [], pe, pm, ne, nm, None, torch.float32)
        assert torch.equal(got, want), do_cfg


def test_one_image_at_frame_0_at_full_strength_is_the_held_pipeline_bit_for_bit():
    for do_cfg in (False, True):
        dcfg, dw, vcfg, vw, mean, std, args, lat, pe, pm, ne, nm, img, (F, H, W) = _pipe_case(do_cfg)
        items = [KR.Item(img, 1, 0, 1.0)]
        placed = lat.clone(); placed[:, :H * W] = img
        for out_lat in (False, True):
            args.output_latent = out_lat
            want = RF.pipeline_call_cond(dw, dcfg, vw, vcfg, mean, std, args, placed, torch.tensor([[1, 0]]), pe, pm, ne, nm, None, torch.float32)
            got = KR.pipeline_call_keyframes(dw, dcfg, vw, vcfg, mean, std, args, lat, items, pe, pm, ne, nm, None, torch.float32)
            assert torch.equal(got, want), (do_cfg, out_lat)


def test_update_predicate_and_model_timestep_on_a_table():
    """(sigma, strength) -> (updated, what the model sees at t = trunc(1000 sigma)); edges: s = 0, s = 1, sig == 1 - s"""
    # the predicate is (double)sig - 1e-6 < 1 - (double)s: AT sig == 1 - s the left side is smaller by 1e-6 and the group IS updated
    table = [
        (1.0, 0.0, True, 1000.0), (0.5, 0.0, True, 500.0), (0.0, 0.0, True, 0.0),          # s = 0: always updated, the model sees t
        (1.0, 1.0, False, 0.0), (0.5, 1.0, False, 0.0), (0.025, 1.0, False, 0.0),          # s = 1: held on every step of a schedule, the model sees 0
        (0.0, 1.0, True, 0.0),                                                             # ... sig == 1 - s == 0, the terminal sigma, is the edge again
        (1.0, 0.25, False, 750.0), (0.8, 0.25, False, 750.0),
        (0.75, 0.25, True, 750.0),                                                         # sig == 1 - s
        (0.7499, 0.25, True, 749.0), (0.5, 0.25, True, 500.0),
        (0.5, 0.5, True, 500.0), (0.51, 0.5, False, 500.0), (0.499, 0.5, True, 499.0),
    ]
    for sig, s, upd, tm in table:
        t = int(KR.f32(sig) * 1000.0)
        assert KR.updates(sig, s) == upd, (sig, s)
        assert KR.model_timestep(float(t), s) == tm, (sig, s)
    # a hair above the edge stays frozen: the slack is 1e-6, not more
    assert not KR.updates(0.75 + 2e-6, 0.25) and KR.updates(0.75 + 5e-7, 0.25)
    assert KR.is_hard(1.0) and not KR.is_hard(0.999)


def test_layout_placement_noise_and_strip_of_the_reference():
    hw, C, B = 6, 8, 2
    g = torch.Generator().manual_seed(3)
    img = torch.randn(B, hw, C, generator=g); clip = torch.randn(B, 3 * hw, C, generator=g)
    items = [KR.Item(img, 1, 0, 1.0), KR.Item(img, 1, 24, 0.3), KR.Item(clip, 3, 8, 1.0)]
    lay = KR.layout(items, 25, 2, 3)
    assert (lay.E, lay.G, lay.Fl) == (3, 7, 4)
    assert [(i, k) for i, k, _ in lay.groups] == [(1, 0), (2, 0), (2, 1), (0, 0), (-1, 0), (-1, 0), (2, 2)]
    sec = lay.coords[::hw, 0] * 25
    assert torch.allclose(sec, torch.tensor([24.0, 8.0, 9.0, 0.0, 1.0, 9.0, 17.0]))
    assert torch.equal(lay.coords[:hw, 1:], lay.coords[3 * hw:4 * hw, 1:])
    noise = torch.randn(B, lay.G * hw, C, generator=g)
    lat = KR.place(noise, items, lay)
    assert torch.equal(lat[:, 3 * hw:4 * hw], img) and torch.equal(lat[:, 6 * hw:], clip[:, 2 * hw:]) and torch.equal(lat[:, 4 * hw:6 * hw], noise[:, 4 * hw:6 * hw])
    assert torch.allclose(lat[:, :hw], noise[:, :hw] + 0.3 * (img - noise[:, :hw]), atol=1e-6)
    nz = torch.randn(B, lay.G * hw, C, generator=g)
    out = KR.noised(lat, nz, lay, 0.15, 0.8)
    assert torch.equal(out[:, :hw], lat[:, :hw]) and torch.equal(out[:, 4 * hw:6 * hw], lat[:, 4 * hw:6 * hw])
    assert torch.allclose(out[:, 3 * hw:4 * hw], img + 0.15 * 0.64 * nz[:, 3 * hw:4 * hw], atol=1e-6)
    assert torch.equal(KR.strip(lat, lay), lat[:, 3 * hw:])
    # a later item owns the group where two meet
    both = KR.layout([KR.Item(clip, 3, 0, 1.0), KR.Item(img, 1, 0, 0.5)], 25, 2, 3)
    assert [(i, k, s) for i, k, s in both.groups] == [(1, 0, 0.5), (0, 1, 1.0), (0, 2, 1.0), (-1, 0, 0.0)]


# ---- host half of the C ABI ----
def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ltx_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def hip():
    import ltxhip
    return ltxhip


def test_symbols_are_exported_bound_and_declared(hip):
    lib = ctypes.CDLL(os.path.join(ROOT, "candle-video_amd", "libltxhip.so"))
    names = _declared("ltxhip_keyframes.h")
    assert names == ["ltx_cond_layout", "ltx_cond_noise", "ltx_cond_place", "ltx_cond_step_hold", "ltx_pipeline_call_keyframes"]
    assert names == hip.KEYFRAME_SYMBOLS
    for n in names:
        assert hasattr(lib, n), n
    for attr in ("cond_layout", "cond_place", "cond_noise", "cond_step_hold", "ConditioningItem"):
        assert hasattr(hip, attr), attr
    rust = open(os.path.join(ROOT, "rust", "ltxhip-sys", "src", "lib.rs")).read()
    assert set(names) <= set(re.findall(r"pub fn (ltx_\w+)\(", rust))
    for h in ("ltxhip.h", "ltxhip_ops.h", "ltxhip_cond.h", "ltxhip_guidance.h", "ltxhip_upsampler.h"):
        assert not set(names) & set(_declared(h)), h


def test_header_is_plain_c_and_the_layout_matches_the_mirrors(hip, tmp_path):
    exe = str(tmp_path / "cabi_layout_keyframes")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cabi_layout_keyframes.c"), "-o", exe], check=True)
    c = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)
    rust = open(os.path.join(ROOT, "rust", "ltxhip-sys", "src", "lib.rs")).read()
    for name, cls in (("ltx_cond_item", hip.CondItemC), ("ltx_cond_group", hip.CondGroupC)):
        st = c[name]
        assert ctypes.sizeof(cls) == st["size"] and ctypes.alignment(cls) == st["align"]
        assert [f for f, _ in cls._fields_] == list(st["fields"])
        for f, off in st["fields"].items():
            assert getattr(cls, f).offset == off, f
        assert re.search(r"pub const KEYFRAMES_LAYOUT_%s: \(usize, usize\) = \(%d, %d\);" % (name.upper(), st["size"], st["align"]), rust), name
        body = re.search(r"pub struct %s \{(.*?)\n\}" % name, rust, re.S).group(1)
        assert re.findall(r"pub (\w+):", body) == list(st["fields"])


def test_host_entries_agree_with_the_reference(hip):
    items = [hip.ConditioningItem(None, 0, 1.0, 1), hip.ConditioningItem(None, 24, 0.3, 1), hip.ConditioningItem(None, 8, 1.0, 3)]
    ref = KR.layout([KR.Item(None, 1, 0, 1.0), KR.Item(None, 1, 24, 0.3), KR.Item(None, 3, 8, 1.0)], 25, 4, 6)
    lay = hip.cond_layout(items, 128, 192, 25)
    assert (lay.E, lay.G, lay.hw) == (ref.E, ref.G, ref.hw) and lay.groups == ref.groups
    assert torch.equal(lay.coords.view(torch.int32), ref.coords.view(torch.int32))
    for sig, t in ((1.0, 1000.0), (0.8, 800.0), (0.7, 700.0), (0.5, 500.0), (0.0, 0.0)):
        hold, tm = hip.cond_step_hold(lay, sig, t)
        assert hold == [0 if KR.updates(sig, s) else 1 for _, _, s in ref.groups]
        assert tm == [KR.model_timestep(t, s) for _, _, s in ref.groups]
    plain = hip.cond_layout([], 128, 192, 25)
    assert (plain.E, plain.G) == (0, 4) and torch.equal(plain.coords, O.build_video_coords(1, 4, 4, 6)[0])


def test_argument_errors_without_a_device(hip):
    L = hip.lib
    err = lambda: L.ltx_last_error().decode()
    one = ctypes.c_void_p(4096)                                         # non-null, aligned, never dereferenced: every call fails on its arguments
    f = ctypes.c_float
    E, G = ctypes.c_int(0), ctypes.c_int(0)

    def lay(items, n=None, num_frames=25):
        arr = (hip.CondItemC * max(len(items), 1))(*[hip.CondItemC(None, fc, fi, s) for fc, fi, s in items])
        return L.ltx_cond_layout(arr if items else None, len(items) if n is None else n, 128, 192, num_frames, 25, 8, 32, ctypes.byref(E), ctypes.byref(G), None, 0, None)
    assert lay([(1, 12, 1.0)]) == LTX_ERR_ARG and "item 0" in err() and "12" in err() and "multiple of 8" in err()
    assert lay([(1, 0, 1.0), (1, 32, 1.0)]) == LTX_ERR_ARG and "item 1" in err() and "32" in err()
    assert lay([(3, 16, 1.0)]) == LTX_ERR_ARG and "item 0" in err() and "clip" in err()
    assert lay([(1, 8, 1.5)]) == LTX_ERR_ARG and "strength" in err() and "1.5" in err()
    assert lay([(1, 8, float("nan"))]) == LTX_ERR_ARG and "strength" in err()
    assert lay([(1, 8, -0.1)]) == LTX_ERR_ARG and "strength" in err()
    assert lay([(5, 0, 1.0)]) == LTX_ERR_ARG and "cond_frames 5" in err()
    assert lay([(0, 0, 1.0)]) == LTX_ERR_ARG and lay([(1, -8, 1.0)]) == LTX_ERR_ARG
    assert lay([], n=2) == LTX_ERR_ARG and "items is null" in err()
    assert lay([(1, 24, 1.0), (3, 8, 0.5)]) == LTX_OK and (E.value, G.value) == (3, 7)
    groups = (hip.CondGroupC * 7)()
    arr = (hip.CondItemC * 1)(hip.CondItemC(None, 1, 24, 1.0))
    assert L.ltx_cond_layout(arr, 1, 128, 192, 25, 25, 8, 32, None, None, groups, 4, None) == LTX_ERR_ARG and "5 groups" in err()
    # place / noise / step_hold
    g1 = (hip.CondGroupC * 2)(hip.CondGroupC(0, 1, 1.0), hip.CondGroupC(-1, 0, 0.0))
    tok = (hip.CondItemC * 1)(hip.CondItemC(ctypes.cast(one, ctypes.POINTER(ctypes.c_float)), 1, 0, 1.0))
    assert L.ltx_cond_place(one, tok, 1, g1, 2, 1, 6, 8, None) == LTX_ERR_ARG and "group 0" in err()      # frame 1 of a one-frame item
    assert L.ltx_cond_place(None, tok, 1, g1, 2, 1, 6, 8, None) == LTX_ERR_ARG
    assert L.ltx_cond_place(one, None, 1, g1, 2, 1, 6, 8, None) == LTX_ERR_ARG
    assert L.ltx_cond_noise(one, one, one, g1, 2, 1, 6, 8, f(0.0), f(0.5), None) == LTX_ERR_ARG and "scale" in err()
    assert L.ltx_cond_noise(one, None, one, g1, 2, 1, 6, 8, f(0.1), f(0.5), None) == LTX_ERR_ARG
    g0 = (hip.CondGroupC * 2)(hip.CondGroupC(0, 0, 0.5), hip.CondGroupC(-1, 0, 0.0))
    assert L.ltx_cond_noise(one, one, one, g0, 2, 1, 6, 8, f(0.1), f(0.5), None) == LTX_OK                 # no hard hold: no launch, no device touched
    assert L.ltx_cond_step_hold(g0, 2, f(0.5), f(500.0), None, None) == LTX_ERR_ARG
    # the pipeline call: what it refuses before it touches the model
    p = hip.PipelineParamsC(); L.ltx_pipeline_params_default(ctypes.byref(p))
    call = lambda items, n, c, cn: L.ltx_pipeline_call_keyframes(one, None, ctypes.byref(p), None, items, n, f(c), cn, one, one, one, None, None, None, 1, 4, None, None)
    assert call(None, 2, 0.0, None) == LTX_ERR_ARG and "items is null" in err()
    assert call(tok, 1, 0.15, None) == LTX_ERR_ARG and "cond_noise" in err()
    assert call(tok, 1, -1.0, None) == LTX_ERR_ARG and "image_cond_noise_scale" in err()
    assert L.ltx_pipeline_call_keyframes(None, None, ctypes.byref(p), None, tok, 1, f(0.0), None, one, one, one, None, None, None, 1, 4, None, None) == LTX_ERR_ARG
