"""CPU suite: the host half of include/ltxhip_int8.h - the header is plain C, its symbols are exported, bound by the ctypes mirror and
declared by the Rust crate, and every argument error that needs no device is refused with the documented code and a message.  No
kernel is launched here."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LTX_OK, LTX_ERR_ARG, LTX_ERR_UNSUPPORTED = 0, 1, 4


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
    names = _declared("ltxhip_int8.h")
    assert names == ["ltx_dit_get_int8_linears", "ltx_dit_set_int8_linears", "ltx_op_gemm_i8", "ltx_op_gemm_i8_raw", "ltx_op_quant_rows_i8", "ltx_op_rownorm_quant_i8"]
    assert names == hip.INT8_SYMBOLS and not set(names) & set(hip.EXPORTED_SYMBOLS)
    for n in names:
        assert hasattr(lib, n), n
        assert getattr(hip.lib, n).argtypes is not None and getattr(hip.lib, n).restype is ctypes.c_int, n
    for n in ("quant_rows_i8", "rownorm_quant_i8", "gemm_i8", "gemm_i8_raw"):
        assert hasattr(hip.ops, n), n
    assert hasattr(hip.LtxVideoTransformer3DModel, "set_int8_linears") and hasattr(hip.LtxVideoTransformer3DModel, "int8_linears")
    rust = open(os.path.join(ROOT, "rust", "ltxhip-sys", "src", "lib.rs")).read()
    assert set(names) <= set(re.findall(r"pub fn (ltx_\w+)\(", rust))
    assert "pub fn set_int8_linears" in open(os.path.join(ROOT, "rust", "hip_backend.rs")).read()
    for h in ("ltxhip.h", "ltxhip_ops.h", "ltxhip_cond.h", "ltxhip_stg.h", "ltxhip_upsampler.h", "ltxhip_upsampler_st.h", "ltxhip_guidance.h", "ltxhip_keyframes.h",
              "ltxhip_lora.h", "ltxhip_encoder.h", "ltxhip_stepcache.h"):
        assert not set(names) & set(_declared(h)), h
    assert (hip.LTX_I8_QKV, hip.LTX_I8_TO_OUT, hip.LTX_I8_FF1, hip.LTX_I8_FF2, hip.LTX_I8_ALL) == (1, 2, 4, 8, 15)
    for bit, name in zip((1, 2, 4, 8), ("QKV", "TO_OUT", "FF1", "FF2")):
        assert re.search(r"LTX_I8_%s = %d\b" % (name, bit), open(os.path.join(ROOT, "include", "ltxhip_int8.h")).read())
        assert re.search(r"pub const LTX_I8_%s: u8 = %d;" % (name, bit), rust)


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "use_int8.c"
    src.write_text('#include "ltxhip_int8.h"\nint main(void) { return (LTX_I8_QKV | LTX_I8_TO_OUT | LTX_I8_FF1 | LTX_I8_FF2) == LTX_I8_ALL ? 0 : 1; }\n')
    exe = str(tmp_path / "use_int8")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    assert subprocess.run([exe]).returncode == 0


def test_mask_names(hip):
    assert hip.int8_mask("all") == 15 and hip.int8_mask(("qkv", "ff2")) == 9 and hip.int8_mask("none") == 0 and hip.int8_mask(None) == 0 and hip.int8_mask(6) == 6
    with pytest.raises(hip.LtxError, match="unknown name"):
        hip.int8_mask("attn2")
    with pytest.raises(hip.LtxError, match="outside"):
        hip.int8_mask(16)


def test_argument_errors_without_a_device(hip):
    L = hip.lib
    err = lambda: L.ltx_last_error().decode()
    one = ctypes.c_void_p(4096)                                         # non-null, aligned, never dereferenced: every call fails on its arguments
    odd = ctypes.c_void_p(4100)
    f, i64 = ctypes.c_float, ctypes.c_int64
    assert L.ltx_dit_set_int8_linears(None, None, 15, None) == LTX_ERR_ARG and "null" in err()
    assert L.ltx_dit_get_int8_linears(None, one) == LTX_ERR_ARG and "null" in err()
    assert L.ltx_dit_get_int8_linears(one, None) == LTX_ERR_ARG and "null" in err()

    def quant(x=one, rows=4, D=64, ld=64, q=one, s=one):
        return L.ltx_op_quant_rows_i8(x, i64(rows), D, ld, q, s, None)
    assert quant(x=None) == LTX_ERR_ARG and "null" in err()
    assert quant(s=None) == LTX_ERR_ARG and "null scale" in err()
    assert quant(D=24, ld=24) == LTX_ERR_UNSUPPORTED and "multiple of 16" in err()
    assert quant(D=16400, ld=16400) == LTX_ERR_UNSUPPORTED and "16384" in err()
    assert quant(x=odd) == LTX_ERR_ARG and "misaligned" in err()
    assert quant(ld=68) == LTX_ERR_ARG and "misaligned" in err()
    assert quant(ld=32) == LTX_ERR_ARG and err()
    assert quant(rows=0) == LTX_OK

    def norm(h=one, rows=4, D=64, ld=64, sh=one, sc=one, ms=64, rpb=2, q=one, rs=one):
        return L.ltx_op_rownorm_quant_i8(h, i64(rows), D, ld, f(1e-6), sh, sc, ms, i64(rpb), q, rs, None)
    assert norm(h=None) == LTX_ERR_ARG and "null" in err()
    assert norm(rs=None) == LTX_ERR_ARG and "null scale" in err()
    assert norm(sc=None) == LTX_ERR_ARG and "null scale" in err()
    assert norm(D=8, ld=8, ms=8) == LTX_ERR_UNSUPPORTED and "multiple of 16" in err()
    assert norm(D=8192, ld=8192, ms=8192) == LTX_ERR_UNSUPPORTED and "4096" in err()
    assert norm(rpb=0) == LTX_ERR_ARG and err()
    assert norm(ms=32) == LTX_ERR_ARG and "mod_stride" in err()
    assert norm(sh=odd) == LTX_ERR_ARG and "misaligned" in err()
    assert norm(rows=0) == LTX_OK

    def gemm(a=one, sa=one, w=one, sw=one, bias=None, y=one, M=16, N=16, K=16, epi=0, resid=None, gate=None, rpb=1, seg=0, tile=-1):
        return L.ltx_op_gemm_i8(a, sa, w, sw, bias, y, M, N, K, epi, resid, gate, rpb, seg, tile, None)
    assert gemm(a=None) == LTX_ERR_ARG and "null tensor" in err()
    assert gemm(sa=None) == LTX_ERR_ARG and "null scale" in err()
    assert gemm(sw=None) == LTX_ERR_ARG and "null scale" in err()
    assert gemm(K=24) == LTX_ERR_UNSUPPORTED and "K % 16" in err()
    assert gemm(K=131072 + 16) == LTX_ERR_UNSUPPORTED and "K too large" in err()
    assert gemm(N=18) == LTX_ERR_UNSUPPORTED and "N % 4" in err()
    assert gemm(a=odd) == LTX_ERR_ARG and "misaligned" in err()
    assert gemm(sw=odd) == LTX_ERR_ARG and "misaligned" in err()
    assert gemm(y=ctypes.c_void_p(4098)) == LTX_ERR_ARG and "misaligned" in err()
    assert gemm(epi=4) == LTX_ERR_ARG and "epi" in err()
    assert gemm(epi=3) == LTX_ERR_ARG and "resid" in err()
    assert gemm(epi=2, resid=one) == LTX_ERR_ARG and "gate" in err()
    assert gemm(epi=2, resid=one, gate=odd) == LTX_ERR_ARG and "misaligned" in err()
    assert gemm(seg=6) == LTX_ERR_ARG and "seg_width" in err()
    assert gemm(seg=8, epi=1) == LTX_ERR_ARG and "seg_width" in err()
    assert gemm(tile=3) == LTX_ERR_ARG and "tile" in err()
    assert gemm(M=0) == LTX_ERR_ARG and err()
    assert gemm(M=1 << 20, K=4096) == LTX_ERR_UNSUPPORTED and "2 GiB" in err()
    raw = lambda **kw: L.ltx_op_gemm_i8_raw(kw.get("a", one), kw.get("w", one), kw.get("acc", one), 16, 16, kw.get("K", 16), kw.get("tile", -1), None)
    assert raw(acc=None) == LTX_ERR_ARG and "null" in err()
    assert raw(K=8) == LTX_ERR_UNSUPPORTED and "K % 16" in err()
    assert raw(acc=ctypes.c_void_p(4104)) == LTX_ERR_ARG and "misaligned" in err()
