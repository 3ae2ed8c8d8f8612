"""CPU suite: the host half of include/ltxhip_int8_rot.h - its symbols are exported, bound by the ctypes mirror and declared by the
Rust crate, and every refusal that needs no device comes back with the documented code and a message.  No kernel is launched here."""
import ctypes
import os
import re
import subprocess

import pytest

from test_int8_cabi_cpu import LTX_ERR_ARG, LTX_ERR_UNSUPPORTED, ROOT, _declared


@pytest.fixture(scope="module")
def hip():
    import ltxhip
    return ltxhip


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "ltxhip_int8_rot.h"\nint main(void) { return (int)sizeof(&ltx_op_hadamard_quant_rows_i8) == 0; }\n')
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)


def test_symbols_are_exported_bound_and_declared(hip):
    lib = ctypes.CDLL(os.path.join(ROOT, "candle-video_amd", "libltxhip.so"))
    names = _declared("ltxhip_int8_rot.h")
    assert names == ["ltx_dit_get_int8_rotation", "ltx_dit_set_int8_rotation", "ltx_op_hadamard_quant_rows_i8", "ltx_op_rownorm_hadamard_quant_i8"]
    assert names == hip.INT8_ROT_SYMBOLS and not set(names) & (set(hip.EXPORTED_SYMBOLS) | set(hip.INT8_SYMBOLS) | set(hip.INT8_ATTN_SYMBOLS))
    for n in names:
        assert hasattr(lib, n) and getattr(hip.lib, n).restype is ctypes.c_int, n
    assert all(hasattr(hip.ops, n) for n in ("hadamard_quant_rows_i8", "rownorm_hadamard_quant_i8"))
    assert hasattr(hip.LtxVideoTransformer3DModel, "set_int8_rotation") and hasattr(hip.LtxVideoTransformer3DModel, "int8_rotation")
    rust = open(os.path.join(ROOT, "rust", "ltxhip-sys", "src", "lib.rs")).read()
    assert set(names) <= set(re.findall(r"pub fn (ltx_\w+)\(", rust))
    assert "pub fn set_int8_rotation" in open(os.path.join(ROOT, "rust", "hip_backend.rs")).read()


def test_argument_errors_without_a_device(hip):
    L = hip.lib
    err = lambda: L.ltx_last_error().decode()
    one, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)             # non-null, never dereferenced: every call fails on its arguments
    assert L.ltx_dit_set_int8_rotation(None, 1, None) == LTX_ERR_ARG and "null" in err()
    assert L.ltx_dit_get_int8_rotation(one, None) == LTX_ERR_ARG and "null" in err()

    def rows(x=one, D=2048, ld=2048, c=1.0, q=one, s=one):
        return L.ltx_op_hadamard_quant_rows_i8(x, 5, D, ld, c, q, s, None)
    assert rows(x=None) == LTX_ERR_ARG and "null tensor" in err()
    assert rows(s=None) == LTX_ERR_ARG and "null scale" in err()
    assert rows(q=odd) == LTX_ERR_ARG and "misaligned" in err()
    assert rows(c=0.0) == LTX_ERR_ARG and "out_scale" in err()
    for D in (64, 1536, 32768):
        assert rows(D=D, ld=32768) == LTX_ERR_UNSUPPORTED and f"got {D}" in err()

    def norm(h=one, D=2048, shift=one, stride=2048, rpb=5):
        return L.ltx_op_rownorm_hadamard_quant_i8(h, 5, D, D, 1e-6, shift, one, stride, rpb, one, one, None)
    assert norm(h=None) == LTX_ERR_ARG and "null tensor" in err()
    assert norm(shift=odd) == LTX_ERR_ARG and "misaligned" in err()
    assert norm(D=8192, stride=8192) == LTX_ERR_UNSUPPORTED and "got 8192" in err()
