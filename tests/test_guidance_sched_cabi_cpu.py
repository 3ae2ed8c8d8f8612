"""CPU suite: the host half of include/ltxhip_guidance.h - the header is plain C, its symbols are exported, bound by the ctypes mirror
and declared by the Rust crate, the struct and the enum have the layout the mirrors use, ltx_guidance_schedule_resolve agrees with
tests/guidance_sched_ref.py, and every argument error that needs no device is reported with a message.  No kernel is launched here."""
import ctypes
import json
import os
import random
import re
import subprocess

import pytest

import guidance_sched_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LTX_OK, LTX_ERR_ARG = 0, 1


@pytest.fixture(scope="module")
def hip():
    import ltxhip
    return ltxhip


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ltx_[a-z0-9_]+)\s*\(", src)))


def test_symbols_are_exported_bound_and_declared(hip):
    lib = ctypes.CDLL(os.path.join(ROOT, "candle-video_amd", "libltxhip.so"))
    names = _declared("ltxhip_guidance.h")
    assert names == ["ltx_guidance_schedule_resolve", "ltx_guidance_step_ex", "ltx_guidance_ws_bytes", "ltx_pipeline_call_multiscale_sched", "ltx_pipeline_call_sched"]
    assert names == hip.GUIDANCE_SYMBOLS
    for n in names:
        assert hasattr(lib, n), n
    assert hasattr(hip, "GuidanceSchedule") and hasattr(hip, "guidance_combine_ex") and hasattr(hip, "guidance_step_ex")
    rust = open(os.path.join(ROOT, "rust", "ltxhip-sys", "src", "lib.rs")).read()
    assert set(names) <= set(re.findall(r"pub fn (ltx_\w+)\(", rust))
    for h in ("ltxhip.h", "ltxhip_ops.h", "ltxhip_cond.h", "ltxhip_stg.h", "ltxhip_upsampler.h"):
        assert not set(names) & set(_declared(h)), h


def test_header_is_plain_c_and_the_layout_matches_the_mirrors(hip, tmp_path):
    exe = str(tmp_path / "cabi_layout_guidance")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cabi_layout_guidance.c"), "-o", exe], check=True)
    c = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)
    st, en = c["ltx_guidance_schedule"], c["ltx_rescale_form"]
    cls = hip.GuidanceScheduleC
    assert ctypes.sizeof(cls) == st["size"] and ctypes.alignment(cls) == st["align"]
    assert [f for f, _ in cls._fields_] == list(st["fields"])
    for f, off in st["fields"].items():
        assert getattr(cls, f).offset == off, f
    assert en["size"] == ctypes.sizeof(ctypes.c_int) and en["values"] == {"LTX_RESCALE_CFG": 0, "LTX_RESCALE_MIX": 1}
    assert (hip.LTX_RESCALE_CFG, hip.LTX_RESCALE_MIX) == (0, 1) and hip.RESCALE_FORMS == R.FORMS
    rust = open(os.path.join(ROOT, "rust", "ltxhip-sys", "src", "lib.rs")).read()
    for name, v in en["values"].items():
        assert re.search(r"pub const %s: c_int = %d;" % (name, v), rust), name
    assert re.search(r"pub const GUIDANCE_LAYOUT_LTX_GUIDANCE_SCHEDULE: \(usize, usize\) = \(%d, %d\);" % (st["size"], st["align"]), rust)
    assert "size_of::<ltx_guidance_schedule>() == GUIDANCE_LAYOUT_LTX_GUIDANCE_SCHEDULE.0" in rust
    body = re.search(r"pub struct ltx_guidance_schedule \{(.*?)\n\}", rust, re.S).group(1)
    assert re.findall(r"pub (\w+):", body) == list(st["fields"])


def sched(hip, n=4, **kw):
    d = dict(guidance_scale=[1.0, 3.0, 1.0, 8.0][:n], stg_scale=[0.0, 0.0, 1.0, 4.0][:n], rescale=[1.0, 1.0, 0.5, 0.5][:n],
             skip_block_list=[[], [], [1], [0, 2]][:n], guidance_timesteps=[1.0, 0.75, 0.5, 0.25][:n])
    d.update(kw)
    return hip.GuidanceSchedule(**d)


def test_resolve_agrees_with_the_reference(hip):
    s = sched(hip)
    for sig in ([1.0, 0.9, 0.8, 0.6, 0.3, 0.0], [0.875, 0.625, 0.375], [5.0, -1.0], [0.5]):
        assert s.resolve(sig) == R.resolve(s, sig), sig
    assert s.resolve([0.875, 0.625, 0.375]) == [0, 1, 2]               # ties: the first minimum
    assert sched(hip, guidance_timesteps=[0.25, 0.5, 0.75, 1.0]).resolve([0.875, 0.625, 0.375]) == [2, 1, 0]
    assert sched(hip, 1, guidance_timesteps=None).resolve([1.0, 0.5, 0.2]) == [0, 0, 0]
    assert sched(hip, 3, guidance_timesteps=None).resolve([1.0, 0.5, 0.2]) == [0, 1, 2]
    rnd = random.Random(7)
    for _ in range(50):
        n, N = rnd.randint(1, 64), rnd.randint(1, 40)
        gt = [rnd.choice([rnd.random(), rnd.randint(0, 8) / 8.0]) for _ in range(n)]
        sig = [rnd.choice([rnd.random(), rnd.randint(0, 16) / 16.0]) for _ in range(N)]
        s = hip.GuidanceSchedule([1.0] * n, [0.0] * n, [0.0] * n, None, gt)
        assert s.resolve(sig) == R.resolve(s, sig)


def test_error_cases_report_why(hip):
    err = lambda: hip.lib.ltx_last_error().decode()
    sig = [1.0, 0.5, 0.2]
    cases = [(dict(guidance_scale=[1.0, float("inf"), 1.0, 8.0]), "non-finite"), (dict(rescale=[1.0, 1.0, float("nan"), 0.5]), "non-finite"),
             (dict(stg_scale=[0.0, float("nan"), 1.0, 4.0]), "non-finite"), (dict(guidance_timesteps=[1.0, float("inf"), 0.5, 0.25]), "non-finite"),
             (dict(stg_scale=[0.0, -0.5, 1.0, 4.0]), "negative stg_scale"), (dict(rescale_form=2), "unknown rescale_form"),
             (dict(rescale_form=-1), "unknown rescale_form"), (dict(skip_block_list=[[], [], [-1], []]), "outside the model")]
    for kw, why in cases:
        with pytest.raises(hip.LtxError, match=why):
            sched(hip, **kw).resolve(sig)
        with pytest.raises(ValueError):
            R.resolve(sched(hip, **kw), sig) if "skip_block_list" not in kw else R.check(sched(hip, **kw), 3)
    for n in (2, 4):
        with pytest.raises(hip.LtxError, match="n must be 1 or the number of steps"):
            sched(hip, n, guidance_timesteps=None).resolve(sig)
    with pytest.raises(hip.LtxError, match="1..64"):
        hip.GuidanceSchedule([], [], []).resolve(sig)
    with pytest.raises(hip.LtxError, match="1..64"):
        hip.GuidanceSchedule([1.0] * 65, [0.0] * 65, [0.0] * 65).resolve(sig)
    with pytest.raises(hip.LtxError, match="one value per entry"):
        hip.GuidanceSchedule([1.0, 2.0], [0.0], [0.0, 0.0]).resolve(sig)
    with pytest.raises(hip.LtxError, match="unknown rescale_form"):
        sched(hip, rescale_form="both").resolve(sig)
    # the raw entry: null pieces
    keep = []
    c = sched(hip).to_c(keep)
    out = (ctypes.c_int * 3)(7, 7, 7)
    sg = (ctypes.c_float * 3)(*sig)
    L = hip.lib
    assert L.ltx_guidance_schedule_resolve(None, sg, 3, out) == LTX_ERR_ARG and err()
    assert L.ltx_guidance_schedule_resolve(ctypes.byref(c), None, 3, out) == LTX_ERR_ARG and err()
    assert L.ltx_guidance_schedule_resolve(ctypes.byref(c), sg, 0, out) == LTX_ERR_ARG and err()
    assert L.ltx_guidance_schedule_resolve(ctypes.byref(c), sg, 3, None) == LTX_ERR_ARG and err()
    c.cfg_star = 2
    assert L.ltx_guidance_schedule_resolve(ctypes.byref(c), sg, 3, out) == LTX_ERR_ARG and "cfg_star" in err()
    assert list(out) == [7, 7, 7]                                       # a refused call writes nothing
    c.cfg_star = 1
    assert L.ltx_guidance_schedule_resolve(ctypes.byref(c), sg, 3, out) == LTX_OK and list(out) == [0, 2, 3]


def test_workspace_size(hip):
    ws = lambda B, n: int(hip.lib.ltx_guidance_ws_bytes(B, ctypes.c_int64(n)))
    assert ws(0, 10) == 0 and ws(1, 0) == 0
    for B, n in ((1, 1), (3, 1025), (3, 72 * 128 + 3), (1, 4992 * 128), (8, 1 << 30)):
        blocks = min(max(-(-n // 2048), 1), 256)
        assert ws(B, n) % 16 == 0 and ws(B, n) >= B * blocks * 9 * 8 + B * 8, (B, n)
    assert ws(1, 4992 * 128) <= 32 * 1024                               # a few KB: partials, never a copy of the predictions


def test_argument_errors_without_a_device(hip):
    L = hip.lib
    err = lambda: L.ltx_last_error().decode()
    one = ctypes.c_void_p(4096)                                         # non-null, aligned, never dereferenced: every call fails on its arguments
    f = ctypes.c_float

    def step(text=one, B=1, n=64, g=3.0, r=0.5, s=1.0, star=0, form=0, ws=one, lat=one, out=None, nz=None, hold=None, nf=1, fe=64, dtype=0):
        return L.ltx_guidance_step_ex(text, one, one, dtype, lat, out, B, ctypes.c_int64(n), f(g), f(r), f(s), star, form, f(-0.1), f(0.0), f(0.0), nz,
                                      hold, nf, ctypes.c_int64(fe), ws, None, None)
    assert step(g=float("inf")) == LTX_ERR_ARG and "non-finite" in err()
    assert step(r=float("nan")) == LTX_ERR_ARG and "non-finite" in err()
    assert step(s=-1.0) == LTX_ERR_ARG and "negative stg_scale" in err()
    assert step(form=2) == LTX_ERR_ARG and "unknown rescale_form" in err()
    assert step(star=3) == LTX_ERR_ARG and "cfg_star" in err()
    assert step(text=None) == LTX_ERR_ARG and err()
    assert step(B=0) == LTX_ERR_ARG and err()
    assert step(n=0) == LTX_ERR_ARG and err()
    assert step(ws=None) == LTX_ERR_ARG and "workspace" in err()
    assert step(ws=ctypes.c_void_p(4104)) == LTX_ERR_ARG and "workspace" in err()
    assert step(lat=None) == LTX_ERR_ARG and "nothing to write" in err()
    assert step(lat=None, out=one, nz=one) == LTX_ERR_ARG and "stochastic" in err()
    assert step(hold=one, nf=3, fe=20) == LTX_ERR_ARG and "num_frames * frame_elems" in err()
    assert step(dtype=5) == LTX_ERR_ARG and err()
    keep = []
    c = sched(hip).to_c(keep)
    p = hip.PipelineParamsC(); L.ltx_pipeline_params_default(ctypes.byref(p))
    assert L.ltx_pipeline_call_sched(None, None, ctypes.byref(p), ctypes.byref(c), None, one, one, one, None, None, None, 1, 128, None, None) == LTX_ERR_ARG and err()
    assert L.ltx_pipeline_call_multiscale_sched(None, None, None, ctypes.byref(p), ctypes.byref(p), ctypes.byref(c), None, f(1.0), one, one, one, one, None, None, None,
                                                1, 128, one, None, None) == LTX_ERR_ARG and err()
