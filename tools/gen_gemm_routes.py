"""Writes tests/golden/gemm_routes.json: the answers of the read-only dispatch probe (ltxhip.ops.gemm_route) for a fixed
table of GEMM / conv calls under a fixed list of option settings.  No GPU is needed (nothing is launched or measured).

The committed file was recorded ONCE, on the commit that added the probe to the dispatcher as it was before the plan-table /
route refactor (see docs/lab_notes.md for the hash); tests/test_gemm_routes_cpu.py holds every later dispatcher to it.  Run this
tool again only on that commit (to check the record) or when a rule of the dispatch is changed on purpose.

    python tools/gen_gemm_routes.py [out.json]
"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "candle-video_amd"))

BIAS, GELU, GATE_RESID, RESID, D2S, UNPATCH, S2D = range(7)


def lin(M, N, K, epi=BIAS, **kw):
    return dict(M=M, N=N, K=K, epi=epi, **kw)


def conv(C, N, B, T, H, W, epi=BIAS, **kw):
    return dict(M=B * T * H * W, N=N, K=C, conv=1, ntaps=27, B=B, T=T, H=H, W=W, epi=epi, **kw)


S, D = 4992, 2048          # the 2B headline: 13 x 16 x 24 latent tokens of 2048 channels
CALLS = {
    # DiT, 2B headline, each with its real epilogue; then the norm-fold forms of the same calls
    "dit.qkv": lin(S, 3 * D, D), "dit.to_out": lin(S, D, D, GATE_RESID), "dit.q2": lin(S, D, D), "dit.out2": lin(S, D, D, RESID),
    "dit.ff1": lin(S, 4 * D, D, GELU), "dit.ff2": lin(S, D, 4 * D, GATE_RESID),
    "dit.qkv.fold_in": lin(S, 3 * D, D, fold_in=True), "dit.q2.fold_in": lin(S, D, D, fold_in=True), "dit.ff1.fold_in": lin(S, 4 * D, D, GELU, fold_in=True),
    "dit.to_out.fold_out": lin(S, D, D, GATE_RESID, fold_out=True), "dit.out2.fold_out": lin(S, D, D, RESID, fold_out=True),
    "dit.ff2.fold_out": lin(S, D, 4 * D, GATE_RESID, fold_out=True),
    # C1's DiT: 4 x 8 x 12 = 384 tokens
    "c1.qkv": lin(384, 3 * D, D), "c1.to_out": lin(384, D, D, GATE_RESID), "c1.ff1": lin(384, 4 * D, D, GELU), "c1.ff2": lin(384, D, 4 * D, GATE_RESID),
    "c1.ff2.defer": lin(384, D, 4 * D, defer=True), "c1.qkv.fold_in": lin(384, 3 * D, D, fold_in=True), "c1.to_out.fold_out": lin(384, D, D, GATE_RESID, fold_out=True),
    "dit.to_out.defer": lin(S, D, D, defer=True),
    # small linear layers: 128 text rows, the timestep MLPs; T5-XXL's wo
    "text.kv": lin(128, 2 * D, D), "text.caption": lin(128, D, 4096, GELU), "time.in": lin(1, D, 256), "time.ada": lin(1, 6 * D, D),
    "t5.wo": lin(128, 4096, 10240, RESID), "t5.wo.defer": lin(128, 4096, 10240, defer=True),
    # VAE decode at C2's stage shapes (latent 13 x 16 x 24)
    "vae.mid1024": conv(1024, 1024, 1, 13, 16, 24), "vae.mid1024.resid": conv(1024, 1024, 1, 13, 16, 24, RESID),
    "vae.up1024": conv(1024, 4096, 1, 13, 16, 24, D2S), "vae.c512": conv(512, 512, 1, 25, 32, 48, RESID), "vae.up512": conv(512, 2048, 1, 25, 32, 48, D2S),
    "vae.c256": conv(256, 256, 1, 49, 64, 96), "vae.up256": conv(256, 1024, 1, 49, 64, 96, D2S), "vae.c128": conv(128, 128, 1, 97, 128, 192, RESID),
    "vae.conv_out": conv(128, 48, 1, 97, 128, 192, UNPATCH),
    "vae.c128.pn": conv(128, 128, 1, 97, 128, 192, pn=True), "vae.c256.pn": conv(256, 256, 1, 49, 64, 96, pn=True),
    # C1's mid block (384 voxels), an edge tile of the tiled decode (48 voxels), a batch of leaf tiles
    "c1.mid1024": conv(1024, 1024, 1, 4, 8, 12), "c1.mid1024.resid": conv(1024, 1024, 1, 4, 8, 12, RESID), "tile.edge1024": conv(1024, 1024, 1, 1, 6, 8),
    "tile.batch512": conv(512, 512, 4, 5, 16, 16, RESID),
    # VAE encode: a space-to-depth downsampler
    "enc.down128": conv(128, 64, 1, 9, 64, 96, S2D), "enc.c256": conv(256, 256, 1, 5, 32, 48),
    # f32, and a linear layer whose activation passes the 2 GiB the 32-bit offsets reach
    "f32.linear": lin(256, 256, 256, dtype="f32"), "f32.conv": conv(128, 128, 1, 2, 16, 32, dtype="f32"), "huge.linear": lin(600000, D, D),
    # shapes between the families' floors
    "mid.linear1024": lin(1024, 256, 256), "mid.linear2048": lin(2048, 256, 256), "mid.linear2304": lin(2304, 1024, 512), "mid.linear1536": lin(1536, D, D, RESID),
}

T0 = {"gemm_tune": "0"}
SETTINGS = {"default": T0, "splitk=0": dict(T0, gemm_splitk="0")}
for fam in ("asm16", "ring", "p8", "halo", "halo_out", "big"):
    SETTINGS["off=" + fam] = dict(T0, gemm_off=fam)
for name in ("256x128", "p8:256", "halo:128", "halo:256", "asm16:160x256", "asm16c:256x256", "ring:96x96", "asm16", "ring"):
    SETTINGS["plan=" + name] = dict(T0, gemm_plan=name)
# a plan file (gemm_tune stays on; only the calls whose key the file names are probed: the plan cache is the process's)
PLAN_FILE = ["4992 6144 2048 0 0 0 0 0 160x256w16", "384 8192 2048 0 0 0 0 0 ring:64x128", "4992 1024 1024 1 27 13 16 24 asm16c:256x256",
             "384 2048 8192 3 0 0 0 0 ring:128x64"]
PLAN_FILE_CALLS = ["dit.qkv", "dit.qkv.fold_in", "c1.ff1", "vae.mid1024", "vae.mid1024.resid", "c1.ff2.defer"]


def probe(hip, call):
    import torch
    kw = dict(call)
    kw["dtype"] = torch.float32 if kw.pop("dtype", "bf16") == "f32" else torch.bfloat16
    try:
        return hip.ops.gemm_route(**kw)
    except hip.LtxError:
        return "refused"


def routes(hip, calls, settings, plan_file, plan_file_calls):
    out = {}
    for sname, opts in settings.items():
        with hip.options(**opts):
            out[sname] = {c: probe(hip, calls[c]) for c in calls}
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "plans.txt")
        with open(p, "w") as f:
            f.write("\n".join(plan_file) + "\n")
        hip.plan_load(p)
    with hip.options(gemm_tune="1", gemm_off="", gemm_plan="", gemm_splitk="1"):
        out["plan_file"] = {c: probe(hip, calls[c]) for c in plan_file_calls}
    return out


if __name__ == "__main__":
    import ltxhip
    table = {"calls": CALLS, "settings": SETTINGS, "plan_file": PLAN_FILE, "plan_file_calls": PLAN_FILE_CALLS}
    table["routes"] = routes(ltxhip, CALLS, SETTINGS, PLAN_FILE, PLAN_FILE_CALLS)
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "gemm_routes.json")
    with open(dst, "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    n = sum(len(v) for v in table["routes"].values())
    print(f"{dst}: {n} routes, {len(set(r for v in table['routes'].values() for r in v.values()))} distinct")
