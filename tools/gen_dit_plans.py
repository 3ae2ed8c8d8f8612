"""Writes tests/golden/dit_plans.json: the decisions of the DiT forward (ltxhip.ops.dit_plan, the read-only probe of csrc/dit.hip's
ltx_dit_plan) for a fixed table of model dims and call shapes under a fixed list of option settings.  No GPU is needed (nothing is
launched or measured).

The committed file was recorded ONCE, on the decision code as it stood inside dit_forward_b8 (moved verbatim into ltx_dit_plan,
before the GEMM argument builders replaced its hand-written fit-test arguments; see docs/lab_notes.md);
tests/test_dit_plan_cpu.py holds every later plan to it.  Run this tool again only when a rule of the forward is changed on purpose.

    python tools/gen_dit_plans.py [out.json]
"""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "candle-video_amd"))

# (heads, head_dim): the 2B and 13B models, the reduced dims of the GPU tests (D = 512, 256, 32), a D that is no power of two (1536)
DIMS = [[32, 64], [32, 128], [8, 64], [4, 64], [2, 16], [24, 64]]
# rows of one batch row -> its latent frames (G = F in a per-frame call): C1's 384 and the headline's 4992 tokens, the 512 / 513
# threshold between the small-M and the large tiles, a plane below every tile, the largest preset
ROWS = {"48": 2, "384": 4, "512": 8, "513": 3, "4992": 13, "17556": 21}
BATCH = [1, 2, 3, 8]
TEXT = [8, 128, 256]
DTYPES = ["bf16", "f32"]
T0 = {"gemm_tune": "0"}
SETTINGS = {"default": T0, "norm_fold=0": dict(T0, norm_fold="0"), "norm_fold=1": dict(T0, norm_fold="1"), "norm_presum=0": dict(T0, norm_presum="0"),
            "norm_presum=2": dict(T0, norm_presum="2"), "q2_fold=2": dict(T0, q2_fold="2"), "ff2_defer=0": dict(T0, ff2_defer="0"),
            "dense_qkv=0": dict(T0, dense_qkv="0"), "off=big": dict(T0, gemm_off="big"), "off=asm16": dict(T0, gemm_off="asm16"),
            "wide_epi=0": dict(T0, gemm_wide_epi="0")}
DECISIONS = ("fold_q2", "presum", "nfold", "defer_ff2", "ff2_parts", "dense_qkv", "fold_q")


def shapes(rows, batch, text):
    """the call shapes of one (setting, dims) row of the table, in the order its codes are written"""
    return [dict(S=int(s), B=b, G=g, K=k, dtype=dt, skip_mask=sk)
            for s, b, per_frame, k, dt, sk in itertools.product(rows, batch, (False, True), text, DTYPES, (False, True))
            for g in [rows[s] if per_frame else 1]]


def code(plan):
    """one plan's decisions as two hex digits (bit i: DECISIONS[i]; ff2_parts: the bit says 4, else 1)"""
    assert plan["ff2_parts"] in (1, 4), plan
    return "%02x" % sum((plan[k] == 4 if k == "ff2_parts" else bool(plan[k])) << i for i, k in enumerate(DECISIONS))


def decode(c):
    v = int(c, 16)
    return {k: (4 if v >> i & 1 else 1) if k == "ff2_parts" else bool(v >> i & 1) for i, k in enumerate(DECISIONS)}


def probe(hip, dims, shape):
    import torch
    kw = dict(shape)
    kw["dtype"] = torch.float32 if kw.pop("dtype") == "f32" else torch.bfloat16
    return hip.ops.dit_plan(dims[0], dims[1], **kw)


def plans(hip, dims, rows, batch, text, settings):
    """{setting: {"heads x head_dim": codes of shapes(...) joined}}"""
    out = {}
    for sname, opts in settings.items():
        with hip.options(**opts):
            out[sname] = {f"{d[0]}x{d[1]}": "".join(code(probe(hip, d, sh)) for sh in shapes(rows, batch, text)) for d in dims}
    return out


if __name__ == "__main__":
    import ltxhip
    table = {"dims": DIMS, "rows": ROWS, "batch": BATCH, "text": TEXT, "settings": SETTINGS}
    table["plans"] = plans(ltxhip, DIMS, ROWS, BATCH, TEXT, SETTINGS)
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "dit_plans.json")
    with open(dst, "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    codes = [s[i:i + 2] for per in table["plans"].values() for s in per.values() for i in range(0, len(s), 2)]
    print(f"{dst}: {len(codes)} plans, {len(set(codes))} distinct")
