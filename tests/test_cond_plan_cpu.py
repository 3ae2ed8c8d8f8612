"""CPU suite: the keyframe layout (candle-video_amd/host/cond_plan.h), the data that host/pipeline.hip's keyframe call walks.

The header is built for the host alone with AddressSanitizer + UBSan into a stand-alone program (tests/host/cond_plan_main.cpp), one
run per case.  Every integer and every coordinate (as f32 bits) it prints is compared with tests/keyframes_ref.py; every refusal must
end the program with its message, which names the item and the value."""
import json
import os
import shutil
import subprocess

import pytest
import torch

import keyframes_ref as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM = dict(num_frames=25, h=4, w=6, ts=8, sp=32, fr=25)           # latent grid 4 x 4 x 6
PROBES = ((1.0, 1000.0), (0.8, 800.0), (0.5, 500.0))

# name -> [(cond_frames, frame_index, strength)]
CASES = {
    "no items": [],
    "image at frame 0": [(1, 0, 1.0)],
    "keyframe at the last frame": [(1, 24, 1.0)],
    "first and last frame": [(1, 0, 1.0), (1, 24, 1.0)],
    "two keyframes": [(1, 8, 0.25), (1, 16, 1.0)],
    "clip at 8 with three latent frames": [(3, 8, 1.0)],          # E = 2 and one grid frame (latent frame 3)
    "clip of two latent frames at 16": [(2, 16, 0.5)],            # E = 2, no grid frame
    "clip at 0 fills the grid": [(4, 0, 0.7)],
    "overlap: a clip, then an image on its first frame": [(3, 0, 1.0), (1, 0, 0.5)],
    "overlap: a keyframe clip's grid frame, then a clip from 0": [(3, 8, 1.0), (4, 0, 0.3)],
    "overlap: strength 0 takes a group back": [(2, 0, 1.0), (1, 0, 0.0)],
    "the same keyframe twice": [(1, 16, 1.0), (1, 16, 0.5)],      # two extra groups at one time coordinate
}
OTHER_GEOM = [
    (dict(num_frames=17, h=2, w=3, ts=4, sp=16, fr=30), [(1, 0, 1.0), (1, 12, 0.5), (3, 4, 1.0)]),   # other ratios and frame rate: F' = 5
    (dict(num_frames=1, h=1, w=1, ts=8, sp=32, fr=25), [(1, 0, 1.0)]),
]
REFUSALS = [
    ([(1, 12, 1.0)], ["item 0", "frame_index 12", "multiple of 8"]),
    ([(1, 0, 1.0), (1, 32, 1.0)], ["item 1", "frame_index 32", "25 frames"]),
    ([(1, 25, 1.0)], ["item 0", "frame_index 25"]),
    ([(3, 16, 1.0)], ["item 0", "clip of 3", "frame_index 16", "latent frame 4"]),
    ([(3, 24, 1.0)], ["item 0", "clip of 3"]),
    ([(5, 0, 1.0)], ["item 0", "cond_frames 5", "4 latent frames"]),
    ([(1, 8, 1.5)], ["item 0", "strength 1.5"]),
    ([(1, 0, 1.0), (1, 8, -0.25)], ["item 1", "strength -0.25"]),
    ([(1, 8, float("nan"))], ["item 0", "strength"]),
    ([(0, 0, 1.0)], ["item 0", "cond_frames 0"]),
    ([(1, -8, 1.0)], ["item 0", "frame_index -8"]),
]


@pytest.fixture(scope="module")
def exe():
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    pkg = os.path.join(ROOT, "candle-video_amd")
    b = subprocess.run(["make", "-C", pkg, "asan_cond_plan"], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    return os.path.join(pkg, "build", "asan", "ltx_cond_plan_asan")


def _run(exe, geom, items):
    argv = [exe] + [str(geom[k]) for k in ("num_frames", "h", "w", "ts", "sp", "fr")] + [repr(v) if isinstance(v, float) else str(v) for it in items for v in it]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run(argv, capture_output=True, text=True, env=env, timeout=60)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    return r


def _bits(x: float) -> int:
    return int(torch.tensor(x, dtype=torch.float32).view(torch.int32)) & 0xFFFFFFFF


def _check(exe, geom, items, name):
    r = _run(exe, geom, items)
    assert r.returncode == 0, (name, r.stderr[-2000:])
    p = json.loads(r.stdout)
    ref = KR.layout([KR.Item(None, fc, n, s) for fc, n, s in items], geom["num_frames"], geom["h"], geom["w"], geom["ts"], geom["sp"], geom["fr"])
    assert (p["E"], p["G"], p["Fl"], p["hw"]) == (ref.E, ref.G, ref.Fl, ref.hw), name
    assert p["groups"] == [[i, k, _bits(s)] for i, k, s in ref.groups], name
    want = (ref.coords.reshape(-1).view(torch.int32).to(torch.int64) & 0xFFFFFFFF).tolist()
    assert p["coords"] == want, name
    for (sig, t), row in zip(PROBES, p["steps"]):
        assert row == [[int(KR.updates(sig, s)), _bits(KR.model_timestep(t, s))] for _, _, s in ref.groups], (name, sig)
    return p


def test_layouts_and_coordinates_equal_the_reference(exe):
    for name, items in CASES.items():
        _check(exe, GEOM, items, name)
    for geom, items in OTHER_GEOM:
        _check(exe, geom, items, str(geom))


def test_the_named_cases_lay_out_as_the_rule_says(exe):
    last = _check(exe, GEOM, CASES["keyframe at the last frame"], "last")
    assert (last["E"], last["G"]) == (1, 5) and last["groups"][0][:2] == [0, 0] and all(g[0] == -1 for g in last["groups"][1:])
    assert last["coords"][0] == _bits(float(torch.tensor(24.0) * torch.tensor(1.0 / 25)))       # 24 / 25 s, in front of the grid's 0 s
    two = _check(exe, GEOM, CASES["two keyframes"], "two")
    assert (two["E"], two["G"]) == (2, 6) and [g[:2] for g in two["groups"][:2]] == [[0, 0], [1, 0]]
    clip = _check(exe, GEOM, CASES["clip at 8 with three latent frames"], "clip")
    assert (clip["E"], clip["G"]) == (2, 6)
    assert [g[:2] for g in clip["groups"]] == [[0, 0], [0, 1], [-1, 0], [-1, 0], [-1, 0], [0, 2]]   # latent frame 2 -> grid frame 8/8 + 2 = 3
    hw3 = 24 * 3
    assert [clip["coords"][g * hw3] for g in (0, 1)] == [_bits(float(torch.tensor(8.0) * torch.tensor(1.0 / 25))), _bits(float(torch.tensor(9.0) * torch.tensor(1.0 / 25)))]
    over = _check(exe, GEOM, CASES["overlap: a clip, then an image on its first frame"], "overlap")
    assert [g[:2] for g in over["groups"]] == [[1, 0], [0, 1], [0, 2], [-1, 0]] and over["groups"][0][2] == _bits(0.5)
    back = _check(exe, GEOM, CASES["overlap: strength 0 takes a group back"], "back")
    assert back["groups"][0] == [1, 0, 0] and back["steps"][0][0][0] == 1                            # strength 0: updated from the first step


def test_every_refusal_exits_with_its_message(exe):
    for items, words in REFUSALS:
        r = _run(exe, GEOM, items)
        assert r.returncode == 1 and r.stdout == "", (items, r.returncode, r.stdout[:200])
        for w in words:
            assert w in r.stderr, (items, w, r.stderr)
        with pytest.raises(ValueError):
            KR.layout([KR.Item(None, fc, n, s) for fc, n, s in items], 25, 4, 6)
    bad = _run(exe, dict(GEOM, fr=0), [])
    assert bad.returncode == 1 and "frame_rate" in bad.stderr
