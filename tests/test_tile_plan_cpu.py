"""CPU suite: the VAE tile plan (candle-video_amd/host/tile_plan.cpp), the geometry that csrc/vae.hip's tiled decode and encode walk.

The plan is built for the host alone with AddressSanitizer + UBSan and driven by a stand-alone program (tests/host/tile_plan_main.cpp),
one run for all cases.  Every integer of it is then compared
  * decode: with `ltxhip.sharded`, which tests/test_sharded_cpu.py pins bit for bit against the oracle's `vae_decode`: `_mode`,
    `leaf_crops`, and - because the blend and keep extents of `_assemble_spatial` / `assemble` are locals - what those two functions
    DO with labelled leaves: the extents they hand to `blend`, and which leaf and frame every output sample comes from;
  * encode: with the loops of tests/vae_encoder_ref.py's `tiled_encode` / `temporal_tiled_encode`, restated below as comprehensions."""
import json
import os
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LTX_ERR_ARG = 1
FIELDS = ("r", "tr", "tiling", "framewise", "min_h", "min_w", "min_f", "stride_h", "stride_w", "stride_f", "F", "H", "W")


def _case(side, r, tr, tiling, framewise, mins, strides, shape):
    return dict(zip(("side",) + FIELDS, (side, r, tr, int(tiling), int(framewise)) + tuple(mins) + tuple(strides) + tuple(shape)))


DEFAULTS = ((512, 512, 16), (384, 384, 8))
T64 = ((64, 64, 16), (32, 32, 8))
CASES = [
    # decode; shapes are latent F, H, W
    _case("dec", 32, 8, 1, 1, *DEFAULTS, (13, 16, 24)),                     # the reference's defaults at the headline size
    _case("dec", 32, 8, 1, 0, *T64, (2, 5, 6)),                             # test_vae_tiled_decode_fixture, spatial only
    _case("dec", 32, 8, 1, 1, *T64, (4, 5, 6)),                             # ... and framewise + spatial (16 / 8 frames)
    _case("dec", 16, 2, 1, 1, (64, 64, 4), (32, 32, 2), (5, 6, 7)),         # test_vae_spatial_only_tiled_decode: tr = 2, 4 / 2 frames
    _case("dec", 16, 4, 1, 1, (64, 64, 8), (32, 32, 4), (4, 6, 7)),         # test_vae_noise_injection's tiled part
    _case("dec", 16, 2, 0, 1, (64, 64, 4), (32, 32, 2), (5, 3, 4)),         # framewise without use_tiling
    _case("dec", 16, 4, 1, 0, (64, 64, 8), (32, 32, 4), (9, 6, 7)),         # use_tiling without framewise, many frames
    _case("dec", 16, 4, 1, 1, (64, 64, 8), (48, 48, 4), (4, 7, 10)),        # ragged: last tile (1 latent = 16 samples) narrower than the blend (16)... and than the stride
    _case("dec", 16, 4, 1, 1, (64, 80, 8), (48, 32, 4), (5, 5, 9)),         # ragged, different extents per axis
    _case("dec", 16, 4, 1, 1, (64, 64, 8), (64, 64, 8), (7, 9, 9)),         # stride == min: blend 0
    _case("dec", 16, 4, 1, 1, (32, 32, 4), (64, 48, 8), (7, 9, 9)),         # stride > min: blend clamped to 0, gaps between tiles
    _case("dec", 16, 4, 1, 1, (64, 64, 8), (32, 32, 4), (2, 6, 7)),         # F at the framewise threshold (8 / 4 = 2): spatial
    _case("dec", 16, 4, 1, 1, (64, 64, 8), (32, 32, 4), (3, 6, 7)),         # one past it: temporal
    _case("dec", 16, 4, 0, 1, (64, 64, 8), (32, 32, 8), (5, 3, 4)),         # windows (0,3) (2,5) (4,5): the last is one frame, kept whole
    _case("dec", 16, 4, 1, 1, (64, 64, 8), (32, 32, 4), (3, 4, 4)),         # framewise, plane at the spatial threshold: windows not tiled
    _case("dec", 16, 4, 1, 1, (64, 64, 8), (32, 32, 4), (2, 4, 4)),         # everything at its threshold: direct
    _case("dec", 16, 4, 0, 0, (64, 64, 8), (32, 32, 4), (9, 9, 9)),         # both switches off: direct
    # encode; shapes are sample F, H, W
    _case("enc", 32, 8, 1, 0, *DEFAULTS, (9, 640, 768)),                    # test_spatial_tiled_encode_c4_tile_parameters
    _case("enc", 32, 8, 0, 1, *T64, (33, 64, 64)),                          # test_temporal_tiled_encode, framewise only
    _case("enc", 32, 8, 1, 1, *T64, (33, 96, 96)),                          # ... and framewise + spatial
    _case("enc", 32, 8, 1, 1, *DEFAULTS, (97, 512, 768)),                   # defaults at the headline size
    _case("enc", 16, 4, 1, 0, (64, 64, 8), (48, 48, 4), (9, 112, 160)),     # ragged: last tile one latent wide
    _case("enc", 16, 4, 1, 1, (64, 80, 8), (48, 32, 4), (17, 80, 144)),     # ragged, different extents per axis
    _case("enc", 16, 4, 1, 1, (64, 64, 8), (64, 64, 8), (25, 144, 144)),    # stride == min: blend 0
    _case("enc", 16, 4, 1, 1, (32, 32, 4), (64, 48, 8), (25, 144, 144)),    # stride > min: clamped to 0
    _case("enc", 16, 4, 1, 1, (64, 64, 8), (32, 32, 4), (8, 96, 96)),       # F at the UNDIVIDED threshold (8 samples): spatial
    _case("enc", 16, 4, 1, 1, (64, 64, 8), (32, 32, 4), (9, 96, 96)),       # one past it: temporal
    _case("enc", 16, 2, 1, 1, (64, 64, 4), (32, 32, 2), (9, 96, 112)),      # tr = 2
    _case("enc", 16, 4, 0, 1, (64, 64, 0), (32, 32, 4), (9, 64, 64)),       # tile 0 is one sample frame = one latent frame: nothing left after its drop
    _case("enc", 16, 4, 0, 1, (64, 64, 8), (32, 32, 8), (17, 64, 64)),      # last window (16, 17) is one frame
    _case("enc", 16, 4, 1, 1, (64, 64, 8), (32, 32, 4), (9, 64, 64)),       # framewise, plane at the spatial threshold: windows not tiled
    _case("enc", 16, 4, 1, 1, (64, 64, 8), (32, 32, 4), (8, 64, 64)),       # direct
    _case("enc", 16, 4, 1, 1, (64, 64, 8), (32, 32, 4), (8, 50, 50)),       # direct: H % r is not this path's business
]
STRIDE = "tiling: stride must be >= one latent"
TSTRIDE = "tiling: temporal stride must be >= one latent frame"
DIVIS = "input not divisible by patch sizes (tiled encode: height and width must be multiples of the compression ratio)"
REFUSALS = [
    (_case("dec", 16, 4, 1, 0, (64, 64, 8), (8, 32, 4), (2, 6, 7)), STRIDE),
    (_case("dec", 16, 4, 1, 0, (64, 64, 8), (32, 15, 4), (2, 6, 7)), STRIDE),
    (_case("dec", 16, 4, 1, 1, (64, 64, 8), (32, 0, 4), (5, 6, 7)), STRIDE),            # framewise + spatial: the leaves' refusal
    (_case("dec", 16, 4, 0, 1, (64, 64, 8), (32, 32, 3), (5, 6, 7)), TSTRIDE),
    (_case("dec", 16, 4, 1, 1, (64, 64, 8), (8, 8, 3), (5, 6, 7)), TSTRIDE),            # both wrong: the temporal one is met first
    (_case("dec", 0, 4, 1, 0, (64, 64, 8), (32, 32, 4), (2, 6, 7)), "tiling: compression ratios must be >= 1"),
    (_case("enc", 16, 4, 1, 0, (64, 64, 8), (15, 32, 4), (9, 96, 96)), STRIDE),
    (_case("enc", 16, 4, 1, 1, (64, 64, 8), (32, 8, 4), (9, 96, 96)), STRIDE),
    (_case("enc", 16, 4, 0, 1, (64, 64, 8), (32, 32, 3), (9, 64, 64)), TSTRIDE),
    (_case("enc", 16, 4, 1, 0, (64, 64, 8), (32, 32, 4), (9, 100, 96)), DIVIS),
    (_case("enc", 16, 4, 0, 1, (64, 64, 8), (32, 32, 4), (9, 64, 72)), DIVIS),
    (_case("enc", 0, 4, 1, 0, (64, 64, 8), (32, 32, 4), (9, 96, 96)), DIVIS),
    (_case("enc", 16, 0, 1, 0, (64, 64, 8), (32, 32, 4), (9, 96, 96)), DIVIS),
    (_case("enc", 16, 4, 1, 1, (64, 64, 8), (8, 8, 3), (9, 100, 96)), DIVIS),           # everything wrong: divisibility is met first
]


@pytest.fixture(scope="module")
def plans():
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    pkg = os.path.join(ROOT, "candle-video_amd")
    b = subprocess.run(["make", "-C", pkg, "asan_tile_plan"], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    cases = CASES + [c for c, _ in REFUSALS]
    text = "".join(" ".join([c["side"]] + [str(c[k]) for k in FIELDS]) + "\n" for c in cases)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(pkg, "build", "asan", "ltx_tile_plan_asan")], input=text, capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == f"tile plan host sanitizer driver: clean ({len(cases)} cases)"
    out = [json.loads(l) for l in lines[:-1]]
    assert len(out) == len(cases)
    return out


def test_driver_is_clean_under_asan_and_ubsan_and_refuses_what_the_walks_refused(plans):
    for (c, msg), p in zip(REFUSALS, plans[len(CASES):]):
        assert p == {"ok": 0, "rc": LTX_ERR_ARG, "error": msg}, (c, p)
    assert all(p["ok"] == 1 for p in plans[:len(CASES)])


def _labelled_leaf(k, t, h, w):
    """a decoded leaf whose every sample says which leaf (k) and which of its frames it is"""
    assert k < 512 and t <= 64
    return ((k * 64 + torch.arange(t, dtype=torch.int16)).view(1, 1, t, 1, 1)).expand(1, 1, t, h, w)


def _walk(p, c):
    """What a walk of plan `p` assembles from labelled leaves, and the blend extents it uses per axis: the steps of csrc/vae.hip's
    assemble_spatial / place_temporal on integers (windows x rows x cols, keep-corner copies, the plan's frame drop)."""
    r, tr = c["r"], c["tr"]
    oT, oH, oW = p["out"]
    bt, bh, bw = p["blend"]
    kt, kh, kw = p["keep"]
    out = torch.full((1, 1, oT, oH, oW), -1, dtype=torch.int16)
    used = {2: [], 3: [], 4: []}
    k = ot = 0
    for li, (t0, t1) in enumerate(p["windows"]):
        phys = (t1 - t0 - 1) * tr + 1
        win = torch.full((1, 1, phys, oH, oW), -1, dtype=torch.int16)
        oy = 0
        for ri, (h0, h1) in enumerate(p["rows"]):
            ox = 0
            for ci, (w0, w1) in enumerate(p["cols"]):
                th, tw = (h1 - h0) * r, (w1 - w0) * r
                if ri > 0: used[3].append(bh)
                if ci > 0: used[4].append(bw)
                hs, ws = min(kh, th) if kh else th, min(kw, tw) if kw else tw
                ch, cw = min(hs, oH - oy), min(ws, oW - ox)
                if ch > 0 and cw > 0:
                    win[..., oy:oy + ch, ox:ox + cw] = _labelled_leaf(k, phys, th, tw)[..., :ch, :cw]
                k += 1; ox += ws
            oy += hs
        if p["mode"] != "temporal":
            return win, used
        skip, length, keep = p["frames"][li]
        if li > 0: used[2].append(bt)
        n = min(keep, oT - ot)
        if n > 0:
            out[:, :, ot:ot + n] = win[:, :, skip:skip + n]
        ot += keep
    return out, used


def test_decode_plans_equal_the_sharded_restatement(plans):
    from ltxhip import sharded as S
    for c, p in zip(CASES, plans):
        if c["side"] != "dec":
            continue
        tl = S.Tiling(bool(c["tiling"]), bool(c["framewise"]), c["min_h"], c["min_w"], c["min_f"], c["stride_h"], c["stride_w"], c["stride_f"], c["r"], c["tr"])
        F, H, W, r, tr = c["F"], c["H"], c["W"], c["r"], c["tr"]
        assert p["mode"] == S._mode(tl, F, H, W), c
        if p["mode"] != "direct":
            assert p["window_tiled"] == S._temporal_is_tiled(tl, H, W), c
        assert p["drop"] == "last_of_later_tiles"
        crops = [(t0, t1, h0, h1, w0, w1) for t0, t1 in p["windows"] for h0, h1 in p["rows"] for w0, w1 in p["cols"]]
        assert crops == S.leaf_crops(tl, F, H, W), c                          # window x row x col order
        assert p["out"] == [(F - 1) * tr + 1, H * r, W * r]
        # extents: run sharded's own assembly on labelled leaves, with a `blend` that records what it is asked for
        asked = {2: [], 3: [], 4: []}
        def blend(a, b, extent, dim):
            asked[dim].append(extent)
            return b
        leaves = [_labelled_leaf(k, (t1 - t0 - 1) * tr + 1, (h1 - h0) * r, (w1 - w0) * r) for k, (t0, t1, h0, h1, w0, w1) in enumerate(crops)]
        want = S.assemble(tl, F, H, W, leaves, blend)
        got, used = _walk(p, c)
        assert used == asked, (c, used, asked)
        # (a stride beyond the tile leaves the reference's concatenation short of the output: the walk leaves those samples unwritten)
        wt, wh, ww = want.shape[2:]
        assert torch.equal(got[:, :, :wt, :wh, :ww], want), c
        assert (got[:, :, wt:] == -1).all() and (got[:, :, :, wh:] == -1).all() and (got[..., ww:] == -1).all(), c
        assert (wt, wh, ww) == tuple(got.shape[2:]) or any(c["stride_" + a] > c["min_" + a] for a in "hwf"), c
        if p["mode"] == "temporal":                                          # the "longer than 1" rule, where a case has such a window
            for li, ((t0, t1), (skip, length, keep)) in enumerate(zip(p["windows"], p["frames"])):
                phys = (t1 - t0 - 1) * tr + 1
                assert skip == 0 and length == (phys - 1 if li > 0 and phys > 1 else phys) and keep == min(c["stride_f"] + (li == 0), length), (c, li)
    one = plans[CASES.index(_case("dec", 16, 4, 0, 1, (64, 64, 8), (32, 32, 8), (5, 3, 4)))]
    assert one["windows"][-1] == [4, 5] and one["frames"][-1] == [0, 1, 1]     # a one-frame last window keeps its frame


def _encode_expect(c):
    """tests/vae_encoder_ref.py: encode_z's dispatch, tiled_encode's and temporal_tiled_encode's loops and extents"""
    r, tr, F, H, W = c["r"], c["tr"], c["F"], c["H"], c["W"]
    framewise = bool(c["framewise"]) and F > c["min_f"]
    tiled = bool(c["tiling"]) and (H > c["min_h"] or W > c["min_w"])
    e = dict(ok=1, mode="temporal" if framewise else "spatial" if tiled else "direct", window_tiled=tiled, drop="first_of_tile0",
             windows=[[0, F]], rows=[[0, H]], cols=[[0, W]], blend=[0, 0, 0], keep=[0, 0, 0], out=[0, 0, 0])
    if e["mode"] != "direct":
        e["out"] = [(F - 1) // tr + 1, H // r, W // r]
    if framewise:
        ls_t = c["stride_f"] // tr
        e["windows"] = [[i, min(i + c["min_f"] + 1, F)] for i in range(0, F, c["stride_f"])]
        e["blend"][0], e["keep"][0] = max(c["min_f"] // tr - ls_t, 0), ls_t
    if tiled:
        ls_h, ls_w = c["stride_h"] // r, c["stride_w"] // r
        e["rows"] = [[i, min(i + c["min_h"], H)] for i in range(0, H, c["stride_h"])]
        e["cols"] = [[j, min(j + c["min_w"], W)] for j in range(0, W, c["stride_w"])]
        e["blend"][1:], e["keep"][1:] = [max(c["min_h"] // r - ls_h, 0), max(c["min_w"] // r - ls_w, 0)], [ls_h, ls_w]
    lens = [(t1 - t0 - 1) // tr + 1 - (li == 0) for li, (t0, t1) in enumerate(e["windows"])]      # "if i == 0: tile = tile[:, :, 1:]"
    e["frames"] = [[int(li == 0), n, min(e["keep"][0] + (li == 0), n)] for li, n in enumerate(lens)]
    return e


def test_encode_plans_equal_the_reference_loops(plans):
    n = 0
    for c, p in zip(CASES, plans):
        if c["side"] == "enc":
            assert p == _encode_expect(c), (c, p, _encode_expect(c)); n += 1
    assert n == 16
    zero = plans[CASES.index(_case("enc", 16, 4, 0, 1, (64, 64, 0), (32, 32, 4), (9, 64, 64)))]
    assert zero["windows"][0] == [0, 1] and zero["frames"][0] == [1, 0, 0]     # tile 0 has nothing left after its drop
