"""CPU suite: the host half of include/ltxhip_stepcache.h - the header is plain C, its symbols are exported, bound by the ctypes mirror
and declared by the Rust crate, the struct has the layout the mirrors use, and every argument error that needs no device is reported
with a message.  No kernel is launched here."""
import ctypes
import json
import os
import re
import subprocess

import pytest

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
    names = _declared("ltxhip_stepcache.h")
    assert names == ["ltx_dit_forward_cached", "ltx_op_step_measure", "ltx_op_step_measure_ws_bytes", "ltx_op_step_residual", "ltx_pipeline_call_cached",
                     "ltx_step_cache_create", "ltx_step_cache_decide", "ltx_step_cache_destroy", "ltx_step_cache_params_default",
                     "ltx_step_cache_read_residual", "ltx_step_cache_require", "ltx_step_cache_reset"]
    assert names == hip.STEPCACHE_SYMBOLS
    for n in names:
        assert hasattr(lib, n), n
    for n in ("StepCache", "StepCacheParams", "dit_forward_cached", "pipeline_call_cached"):
        assert hasattr(hip, n), n
    rust = open(os.path.join(ROOT, "rust", "ltxhip-sys", "src", "lib.rs")).read()
    assert set(names) <= set(re.findall(r"pub fn (ltx_\w+)\(", rust))
    for h in ("ltxhip.h", "ltxhip_ops.h", "ltxhip_cond.h", "ltxhip_stg.h", "ltxhip_upsampler.h", "ltxhip_upsampler_st.h", "ltxhip_guidance.h", "ltxhip_keyframes.h",
              "ltxhip_lora.h", "ltxhip_encoder.h"):
        assert not set(names) & set(_declared(h)), h


def test_header_is_plain_c_and_the_layout_matches_the_mirrors(hip, tmp_path):
    exe = str(tmp_path / "cabi_layout_stepcache")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cabi_layout_stepcache.c"), "-o", exe], check=True)
    st = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)["ltx_step_cache_params"]
    cls = hip.StepCacheParamsC
    assert ctypes.sizeof(cls) == st["size"] and ctypes.alignment(cls) == st["align"]
    assert [f for f, _ in cls._fields_] == list(st["fields"])
    for f, off in st["fields"].items():
        assert getattr(cls, f).offset == off, f
    assert cls.coeff.size == st["coeff_bytes"] == 5 * 4
    rust = open(os.path.join(ROOT, "rust", "ltxhip-sys", "src", "lib.rs")).read()
    assert re.search(r"pub const STEPCACHE_LAYOUT_LTX_STEP_CACHE_PARAMS: \(usize, usize\) = \(%d, %d\);" % (st["size"], st["align"]), rust)
    assert "size_of::<ltx_step_cache_params>() == STEPCACHE_LAYOUT_LTX_STEP_CACHE_PARAMS.0" in rust
    body = re.search(r"pub struct ltx_step_cache_params \{(.*?)\n\}", rust, re.S).group(1)
    assert re.findall(r"pub (\w+):", body) == list(st["fields"]) and "[c_float; 5]" in body


def test_the_default_parameters_never_reuse(hip):
    p = hip.StepCacheParamsC()
    p.rel_l1_thresh = 7.0; p.n_pattern = 3
    hip.lib.ltx_step_cache_params_default(ctypes.byref(p))
    assert p.rel_l1_thresh == 0.0 and list(p.coeff) == [0.0, 0.0, 0.0, 1.0, 0.0] and not p.pattern and p.n_pattern == 0
    hip.lib.ltx_step_cache_params_default(None)                         # (a null pointer is left alone)
    d = hip.StepCacheParams()
    keep = []
    c = d.to_c(keep)
    assert (c.rel_l1_thresh, list(c.coeff), c.n_pattern) == (0.0, [0.0, 0.0, 0.0, 1.0, 0.0], 0)
    c = hip.StepCacheParams(0.25, (1, 2, 3, 4, 5), [0, 1, 2]).to_c(keep)
    assert (c.rel_l1_thresh, list(c.coeff), c.n_pattern, [c.pattern[i] for i in range(3)]) == (0.25, [1.0, 2.0, 3.0, 4.0, 5.0], 3, [0, 1, 2])
    with pytest.raises(hip.LtxError, match="five values"):
        hip.StepCacheParams(0.1, (1, 2, 3)).to_c(keep)


def test_argument_errors_without_a_device(hip):
    L = hip.lib
    err = lambda: L.ltx_last_error().decode()
    one = ctypes.c_void_p(4096)                                         # non-null, aligned, never dereferenced: every call fails on its arguments
    f, i64 = ctypes.c_float, ctypes.c_int64
    out = ctypes.c_void_p(1)
    assert L.ltx_step_cache_create(None, 3, ctypes.byref(out)) == LTX_ERR_ARG and "null" in err()
    assert L.ltx_step_cache_create(one, 3, None) == LTX_ERR_ARG and "null" in err()
    assert L.ltx_step_cache_reset(None) == LTX_ERR_ARG and "null" in err()
    L.ltx_step_cache_destroy(None)                                      # (a null handle is left alone)
    keep = []
    ok = hip.StepCacheParams(0.1).to_c(keep)
    reuse, dist = ctypes.c_int(7), f(7.0)

    def decide(cache=None, dit=None, hidden=one, t=one, params=ok, r=reuse):
        return L.ltx_step_cache_decide(cache, dit, hidden, t, 0, 1, 72, 3, 4, 6, 0, 1, 6, ctypes.byref(params) if params is not None else None,
                                       ctypes.byref(r) if r is not None else None, ctypes.byref(dist), None)
    assert decide() == LTX_ERR_ARG and "null" in err()
    assert decide(cache=one, dit=one, hidden=None) == LTX_ERR_ARG and "null" in err()
    assert decide(cache=one, dit=one, r=None) == LTX_ERR_ARG and "null" in err()
    assert (reuse.value, dist.value) == (7, 7.0)                        # a refused call writes nothing
    r = ctypes.c_int(1)
    assert L.ltx_step_cache_require(None, one, 0, 1, 72, ctypes.byref(r)) == LTX_ERR_ARG and "null" in err()
    assert L.ltx_step_cache_require(one, one, 0, 1, 72, None) == LTX_ERR_ARG and "null" in err()
    assert L.ltx_dit_forward_cached(None, None, 0, 0, 0, one, one, one, None, 1, 72, 128, 3, 4, 6, None, None, None, 0, one, None) == LTX_ERR_ARG and "null" in err()
    assert L.ltx_dit_forward_cached(one, one, 0, 0, 0, one, None, one, None, 1, 72, 128, 3, 4, 6, None, None, None, 0, one, None) == LTX_ERR_ARG and "null" in err()   # enc is needed unless the step re-uses
    assert L.ltx_step_cache_read_residual(None, 0, one, None) == LTX_ERR_ARG and "null" in err()
    # the pipeline entry: its own arguments and the parameters, before anything touches the device
    p = hip.PipelineParamsC(); L.ltx_pipeline_params_default(ctypes.byref(p))

    def call(dit=one, params=ok, cond=None, B=1):
        return L.ltx_pipeline_call_cached(dit, None, ctypes.byref(p), None, cond, ctypes.byref(params) if params is not None else None, one, one, one, None, None, None,
                                          B, 128, None, None, None, None)
    assert call(dit=None) == LTX_ERR_ARG and "null" in err()
    assert call(B=0) == LTX_ERR_ARG and err()
    assert call(params=None) == LTX_ERR_ARG and "null step cache parameters" in err()
    assert call(cond=ctypes.byref(hip.ConditioningC(None))) == LTX_ERR_ARG and "hold mask" in err()
    bad = [(hip.StepCacheParams(-0.5), "rel_l1_thresh"), (hip.StepCacheParams(float("nan")), "rel_l1_thresh"), (hip.StepCacheParams(float("inf")), "rel_l1_thresh"),
           (hip.StepCacheParams(0.1, (0, 0, float("nan"), 1, 0)), "non-finite coefficient"), (hip.StepCacheParams(0.1, pattern=[0, 3]), "0 \\(decide\\), 1 \\(compute\\) or 2 \\(reuse\\)")]
    for sp, why in bad:
        c = sp.to_c(keep)
        assert call(params=c) == LTX_ERR_ARG and re.search(why, err()), (why, err())
    c = hip.StepCacheParams(0.1).to_c(keep); c.n_pattern = 4
    assert call(params=c) == LTX_ERR_ARG and "pattern is null" in err()
    c.n_pattern = -1
    assert call(params=c) == LTX_ERR_ARG and "negative" in err()
    # the kernels' entries
    assert int(L.ltx_op_step_measure_ws_bytes(i64(105), 128, 0)) == 16 * -(-105 // 8) and int(L.ltx_op_step_measure_ws_bytes(i64(105), 128, 1)) == 16 * -(-105 // 16)
    assert int(L.ltx_op_step_measure_ws_bytes(i64(4992), 2048, 1)) == 16 * 1248 and int(L.ltx_op_step_measure_ws_bytes(i64(10), 2048, 0)) == 16 * 3
    for D in (0, 64, 192, 2056, 16384):
        assert int(L.ltx_op_step_measure_ws_bytes(i64(10), D, 1)) == 0, D
    assert int(L.ltx_op_step_measure_ws_bytes(i64(0), 128, 1)) == 0 and int(L.ltx_op_step_measure_ws_bytes(i64(10), 8192, 0)) == 0

    def measure(h=one, prev=one, sh=one, sc=one, ms=128, rows=10, D=128, rpb=5, dtype=0, ws=one, sums=one):
        return L.ltx_op_step_measure(h, prev, sh, sc, ms, i64(rows), D, i64(rpb), f(1e-6), dtype, 0, ws, sums, None)
    assert measure(h=None) == LTX_ERR_ARG and "null" in err()
    assert measure(sums=None) == LTX_ERR_ARG and "null" in err()
    assert measure(dtype=3) == LTX_ERR_ARG and "dtype" in err()
    assert measure(rows=0) == LTX_ERR_ARG and err()
    assert measure(rpb=0) == LTX_ERR_ARG and err()
    assert measure(ms=64) == LTX_ERR_ARG and "mod_stride" in err()
    for D in (192, 2056):
        assert measure(D=D, ms=4096) == 4 and "multiple of 128" in err(), D            # LTX_ERR_UNSUPPORTED
    assert measure(D=8192, ms=8192, dtype=0) == 4 and "4096 in f32" in err()
    assert measure(prev=ctypes.c_void_p(4104)) == LTX_ERR_ARG and "aligned" in err()
    assert measure(ms=130, D=128) == LTX_ERR_ARG and "mod_stride" in err()
    assert L.ltx_op_step_residual(None, one, i64(4), 128, 0, None) == LTX_ERR_ARG and err()
    assert L.ltx_op_step_residual(one, one, i64(4), 130, 1, None) == LTX_ERR_ARG and "16 bytes" in err()
    assert L.ltx_op_step_residual(one, ctypes.c_void_p(4100), i64(4), 128, 0, None) == LTX_ERR_ARG and "aligned" in err()
    assert L.ltx_op_step_residual(one, one, i64(4), 128, 2, None) == LTX_ERR_ARG and "dtype" in err()
