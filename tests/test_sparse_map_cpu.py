"""CPU suite: the host half of include/ltxhip_sparse_attn.h - the window-map builder through the library against a brute-force numpy
expansion, the density, the symbols (exported, bound by the ctypes mirror, declared by the Rust crate), the header as plain C, and
every refusal that needs no device.  No kernel is launched here."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import sparse_attn_ref as SP
from test_int8_cabi_cpu import LTX_ERR_ARG, LTX_ERR_UNSUPPORTED, ROOT, _declared


@pytest.fixture(scope="module")
def hip():
    import ltxhip
    return ltxhip


def brute(F, H, W, wf, wh, ww, sink):
    """bool [NQB, NKT] from the definition: every (query token, key token) pair"""
    f, h, w = np.unravel_index(np.arange(F * H * W), (F, H, W))
    near = (abs(f[:, None] - f) <= wf) & (abs(h[:, None] - h) <= wh) & (abs(w[:, None] - w) <= ww) | (f < sink)[None, :]
    S, nqb, nkt = F * H * W, (F * H * W + 127) // 128, (F * H * W + 63) // 64
    pad = np.zeros((nqb * 128, nkt * 64), bool); pad[:S, :S] = near
    return pad.reshape(nqb, 128, nkt, 64).any(axis=(1, 3))


@pytest.mark.parametrize("sink", [0, 1])
@pytest.mark.parametrize("window", [(0, 0, 0), (1, 4, 6), "full"])
@pytest.mark.parametrize("F,H,W", [(3, 8, 13), (4, 16, 26), (13, 16, 24)])
def test_window_map_is_the_brute_force_expansion(hip, F, H, W, window, sink):
    wf, wh, ww = (F, H, W) if window == "full" else window
    S = F * H * W
    map = hip.sparse_window_map(F, H, W, wf, wh, ww, sink)
    want = brute(F, H, W, wf, wh, ww, sink)
    assert map.shape == (want.shape[0], (want.shape[1] + 31) // 32) and map.numel() == hip.lib.ltx_sparse_map_words(S)
    assert np.array_equal(SP.expand(map, S, S).numpy()[::128, ::64], want) and np.array_equal(SP.pack(SP.torch.from_numpy(want)).numpy(), map.numpy())
    assert want.diagonal().all() if want.shape[0] == want.shape[1] else want.any(1).all()      # every row has its diagonal
    assert hip.sparse_map_density(map, S) == pytest.approx(want.mean(), abs=1e-12) and (window != "full" or want.all())


def test_symbols_are_exported_bound_and_declared_and_the_header_is_plain_c(hip, tmp_path):
    lib = ctypes.CDLL(os.path.join(ROOT, "candle-video_amd", "libltxhip.so"))
    names = _declared("ltxhip_sparse_attn.h")
    assert names == ["ltx_dit_get_sparse_attention", "ltx_dit_set_sparse_attention", "ltx_op_attention_sparse", "ltx_sparse_map_density", "ltx_sparse_map_words", "ltx_sparse_window_map"]
    assert names == hip.SPARSE_ATTN_SYMBOLS and not set(names) & (set(hip.EXPORTED_SYMBOLS) | set(hip.INT8_ATTN_SYMBOLS))
    assert all(hasattr(lib, n) for n in names) and hasattr(hip.ops, "attention_sparse")
    assert hasattr(hip.LtxVideoTransformer3DModel, "set_sparse_attention") and hasattr(hip.LtxVideoTransformer3DModel, "sparse_attention")
    rust = open(os.path.join(ROOT, "rust", "ltxhip-sys", "src", "lib.rs")).read()
    assert set(names) <= set(re.findall(r"pub fn (ltx_\w+)\(", rust))
    assert "pub fn set_sparse_attention" in open(os.path.join(ROOT, "rust", "hip_backend.rs")).read()
    exe, pkg = str(tmp_path / "cabi_layout_sparse_attn"), os.path.join(ROOT, "candle-video_amd")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cabi_layout_sparse_attn.c"), "-o", exe, "-L", pkg, "-lltxhip", "-Wl,-rpath," + pkg], check=True)
    c = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)
    map = hip.sparse_window_map(3, 8, 13, 0, 0, 0)
    assert c["sizes"] == {"word": 4, "size_t": ctypes.sizeof(ctypes.c_size_t), "S": 8} and c["words"] == map.numel() == 3 and c["rc"] == 0
    assert c["map"] == map.flatten().tolist() == [3, 12, 16] and c["density"] == hip.sparse_map_density(map, 312) == 1 / 3


def test_argument_errors_without_a_device(hip):
    L = hip.lib
    err = lambda: L.ltx_last_error().decode()
    one, buf = ctypes.c_void_p(4096), (ctypes.c_uint32 * 3)()           # `one`: non-null, never dereferenced - every call fails on its arguments
    assert L.ltx_sparse_window_map(3, 8, 13, 0, 0, 0, 0, buf, 4) == LTX_ERR_ARG and "4 words for a map of 3" in err()
    assert L.ltx_sparse_window_map(3, 8, 13, 0, -1, 0, 0, buf, 3) == LTX_ERR_ARG and "(0, -1, 0)" in err()
    assert L.ltx_sparse_map_words(0) == 0 and L.ltx_sparse_map_density(None, 312) == -1.0
    assert L.ltx_dit_set_sparse_attention(None, buf, 1, 312, None, None) == LTX_ERR_ARG and "null" in err()

    def attn(q=one, map=one, mh=1, hd=64, ldk=128, Sk=70):
        return L.ltx_op_attention_sparse(q, one, one, one, map, mh, 1, 70, Sk, 2, hd, 2 * hd, ldk, 2 * hd, 2 * hd, None)
    assert attn(map=None) == LTX_ERR_ARG and "null" in err()
    assert attn(hd=96) == LTX_ERR_UNSUPPORTED and "64 or 128 (got 96)" in err()
    assert attn(mh=3) == LTX_ERR_ARG and "got 3 with 2 heads" in err()
    assert attn(q=ctypes.c_void_p(4100)) == LTX_ERR_ARG and "misaligned" in err()
    assert attn(ldk=64) == LTX_ERR_ARG and "ldk" in err()
    assert attn(Sk=1 << 23) == LTX_ERR_UNSUPPORTED and "2 GiB" in err()
