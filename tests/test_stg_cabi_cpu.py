"""CPU suite: the host half of include/ltxhip_stg.h - the header is plain C, its symbols are exported, bound by the ctypes mirror and
declared by the Rust crate, the enum has the values the mirrors use, the mode names of the published configs parse, and every
argument error that needs no device is reported with a message.  No kernel is launched here."""
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
    names = _declared("ltxhip_stg.h")
    assert names == ["ltx_dit_get_stg_mode", "ltx_dit_set_stg_mode", "ltx_op_stg_fill", "ltx_stg_mode_from_name"]
    assert names == hip.STG_SYMBOLS
    for n in names:
        assert hasattr(lib, n), n
    assert hasattr(hip.LtxVideoTransformer3DModel, "set_stg_mode") and isinstance(hip.LtxVideoTransformer3DModel.stg_mode, property)
    assert hasattr(hip.ops, "stg_fill")
    rust = open(os.path.join(ROOT, "rust", "ltxhip-sys", "src", "lib.rs")).read()
    assert set(names) <= set(re.findall(r"pub fn (ltx_\w+)\(", rust))
    shim = open(os.path.join(ROOT, "rust", "hip_backend.rs")).read()
    assert "pub fn set_stg_mode" in shim and "sys::ltx_dit_set_stg_mode(" in shim
    # the headers that existed before declare none of the new names
    for h in ("ltxhip.h", "ltxhip_ops.h", "ltxhip_cond.h"):
        assert not set(names) & set(_declared(h)), h


def test_header_is_plain_c_and_the_enum_matches_the_mirrors(hip, tmp_path):
    exe = str(tmp_path / "cabi_layout_stg")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cabi_layout_stg.c"), "-o", exe], check=True)
    c = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)["ltx_stg_mode"]
    assert c["size"] == ctypes.sizeof(ctypes.c_int)                         # the mirrors pass the enum as a C int
    assert c["values"] == {"LTX_STG_TRANSFORMER_BLOCK": 0, "LTX_STG_ATTENTION_SKIP": 1, "LTX_STG_ATTENTION_VALUES": 2}
    assert (hip.LTX_STG_TRANSFORMER_BLOCK, hip.LTX_STG_ATTENTION_SKIP, hip.LTX_STG_ATTENTION_VALUES) == (0, 1, 2)
    rust = open(os.path.join(ROOT, "rust", "ltxhip-sys", "src", "lib.rs")).read()
    for name, v in c["values"].items():
        assert re.search(r"pub const %s: c_int = %d;" % (name, v), rust), name


def test_mode_names_of_the_published_configs(hip):
    L = hip.lib
    for value, name in enumerate(("transformer_block", "attention_skip", "attention_values")):
        out = ctypes.c_int(-1)
        assert L.ltx_stg_mode_from_name(name.encode(), ctypes.byref(out)) == LTX_OK and out.value == value
        assert hip.stg_mode_from_name(name) == value and hip.STG_MODES[value] == name


def test_refused_names_report_why(hip):
    L = hip.lib
    err = lambda: L.ltx_last_error().decode()
    out = ctypes.c_int(7)
    assert L.ltx_stg_mode_from_name(b"residual", ctypes.byref(out)) == LTX_ERR_ARG and "residual" in err() and "not offered" in err()
    assert L.ltx_stg_mode_from_name(b"attention_value", ctypes.byref(out)) == LTX_ERR_ARG and "attention_value" in err()
    assert L.ltx_stg_mode_from_name(b"", ctypes.byref(out)) == LTX_ERR_ARG and err()
    assert L.ltx_stg_mode_from_name(b"Attention_Skip", ctypes.byref(out)) == LTX_ERR_ARG and err()      # the configs' spelling only
    assert L.ltx_stg_mode_from_name(None, ctypes.byref(out)) == LTX_ERR_ARG and err()
    assert L.ltx_stg_mode_from_name(b"attention_skip", None) == LTX_ERR_ARG and err()
    assert out.value == 7                                                    # a refused call writes nothing
    with pytest.raises(hip.LtxError, match="residual"):
        hip.stg_mode_from_name("residual")


def test_argument_errors_without_a_device(hip):
    L = hip.lib
    err = lambda: L.ltx_last_error().decode()
    one = ctypes.c_void_p(4096)                                              # non-null, 16-byte aligned, never dereferenced: every call fails on its arguments
    odd = ctypes.c_void_p(4104)
    rows = (ctypes.c_ubyte * 3)(0, 0, 1)
    out = ctypes.c_int(0)
    assert L.ltx_dit_set_stg_mode(None, 1) == LTX_ERR_ARG and err()
    assert L.ltx_dit_get_stg_mode(None, ctypes.byref(out)) == LTX_ERR_ARG and err()
    assert L.ltx_op_stg_fill(None, 2048, one, 2048, rows, 3, 72, 2048, 1, None) == LTX_ERR_ARG and err()
    assert L.ltx_op_stg_fill(one, 2048, one, 2048, None, 3, 72, 2048, 1, None) == LTX_ERR_ARG and err()
    assert L.ltx_op_stg_fill(one, 2048, one, 2048, rows, 0, 72, 2048, 1, None) == LTX_ERR_ARG and err()
    # 16-byte accesses: a row length, a leading dimension or a pointer that is no multiple of the vector is refused
    assert L.ltx_op_stg_fill(one, 2052, one, 2052, rows, 3, 72, 2052, 1, None) == LTX_ERR_ARG and "16 bytes" in err()      # bf16: 4104 bytes a row
    assert L.ltx_op_stg_fill(one, 2050, one, 2050, rows, 3, 72, 2050, 0, None) == LTX_ERR_ARG and "16 bytes" in err()      # f32: 8200 bytes a row
    assert L.ltx_op_stg_fill(one, 2048, one, 2052, rows, 3, 72, 2048, 1, None) == LTX_ERR_ARG and "16 bytes" in err()
    assert L.ltx_op_stg_fill(odd, 2048, one, 2048, rows, 3, 72, 2048, 1, None) == LTX_ERR_ARG and "16 bytes" in err()
    assert L.ltx_op_stg_fill(one, 1024, one, 2048, rows, 3, 72, 2048, 1, None) == LTX_ERR_ARG and err()                    # a leading dimension below the row length
    # no row selected: nothing to launch, nothing read through the pointers
    none = (ctypes.c_ubyte * 3)(0, 0, 0)
    assert L.ltx_op_stg_fill(one, 2048, one, 2048, none, 3, 72, 2048, 1, None) == LTX_OK
