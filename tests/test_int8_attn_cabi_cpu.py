"""CPU suite: the host half of include/ltxhip_int8_attn.h - its symbols are exported, bound by the ctypes mirror and declared by the
Rust crate, and every refusal that needs no device comes back with the documented code and a message.  No kernel is launched here."""
import ctypes
import os
import re

import pytest

from test_int8_cabi_cpu import LTX_ERR_ARG, LTX_ERR_UNSUPPORTED, ROOT, _declared


@pytest.fixture(scope="module")
def hip():
    import ltxhip
    return ltxhip


def test_symbols_are_exported_bound_and_declared(hip):
    lib = ctypes.CDLL(os.path.join(ROOT, "candle-video_amd", "libltxhip.so"))
    names = _declared("ltxhip_int8_attn.h")
    assert names == ["ltx_dit_get_int8_attention", "ltx_dit_set_int8_attention", "ltx_op_attention_i8", "ltx_op_kmean", "ltx_op_quant_qk_i8"]
    assert names == hip.INT8_ATTN_SYMBOLS and not set(names) & (set(hip.EXPORTED_SYMBOLS) | set(hip.INT8_SYMBOLS))
    for n in names:
        assert hasattr(lib, n) and getattr(hip.lib, n).restype is ctypes.c_int, n
    assert all(hasattr(hip.ops, n) for n in ("kmean", "quant_qk_i8", "attention_i8"))
    assert hasattr(hip.LtxVideoTransformer3DModel, "set_int8_attention") and hasattr(hip.LtxVideoTransformer3DModel, "int8_attention")
    rust = open(os.path.join(ROOT, "rust", "ltxhip-sys", "src", "lib.rs")).read()
    assert set(names) <= set(re.findall(r"pub fn (ltx_\w+)\(", rust))
    assert "pub fn set_int8_attention" in open(os.path.join(ROOT, "rust", "hip_backend.rs")).read()


def test_argument_errors_without_a_device(hip):
    L = hip.lib
    err = lambda: L.ltx_last_error().decode()
    one, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)             # non-null, never dereferenced: every call fails on its arguments
    assert L.ltx_dit_set_int8_attention(None, None, 1, None) == LTX_ERR_ARG and "null" in err()
    assert L.ltx_dit_get_int8_attention(one, None) == LTX_ERR_ARG and "null" in err()

    def kmean(k=one, Sk=70, D=128, ldk=128, mean=one):
        return L.ltx_op_kmean(k, 1, Sk, D, ldk, mean, None)
    assert kmean(k=None) == LTX_ERR_ARG and "null" in err()
    assert kmean(k=odd) == LTX_ERR_ARG and "misaligned" in err()
    assert kmean(ldk=132) == LTX_ERR_ARG and "misaligned" in err()
    assert kmean(D=12, ldk=16) == LTX_ERR_UNSUPPORTED and "multiple of 8" in err()
    assert kmean(Sk=1 << 20, D=1024, ldk=1024) == LTX_ERR_UNSUPPORTED and "2 GiB" in err()

    def quant(q=one, k=one, mean=one, hd=64, ldq=128, q8=one, qs=one, Sq=70):
        return L.ltx_op_quant_qk_i8(q, k, mean, 1, Sq, 70, 2, hd, ldq, 128, q8, qs, one, one, None)
    assert quant(q=None) == LTX_ERR_ARG and "null tensor" in err()
    assert quant(qs=None) == LTX_ERR_ARG and "null scale" in err()
    assert quant(hd=32) == LTX_ERR_UNSUPPORTED and "64 or 128" in err()
    assert quant(mean=odd) == LTX_ERR_ARG and "misaligned" in err()
    assert quant(ldq=64) == LTX_ERR_ARG and "ldq" in err()
    assert quant(Sq=1 << 23) == LTX_ERR_UNSUPPORTED and "2 GiB" in err()

    def attn(q8=one, ks=one, v=one, o=one, hd=64, heads=2, ldv=128, Sk=70):
        return L.ltx_op_attention_i8(q8, one, one, ks, v, o, 1, 70, Sk, heads, hd, ldv, heads * hd, None)
    assert attn(ks=None) == LTX_ERR_ARG and "null" in err()
    assert attn(hd=96) == LTX_ERR_UNSUPPORTED and "64 or 128" in err()
    assert attn(v=odd) == LTX_ERR_ARG and "misaligned" in err()
    assert attn(o=ctypes.c_void_p(4098)) == LTX_ERR_ARG and "misaligned" in err()
    assert attn(ldv=64) == LTX_ERR_ARG and "ldv" in err()
    assert attn(Sk=1 << 24) == LTX_ERR_UNSUPPORTED and "2 GiB" in err()
