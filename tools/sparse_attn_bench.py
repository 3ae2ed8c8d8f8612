#!/usr/bin/env python
"""Cost of the block-sparse self-attention (include/ltxhip_sparse_attn.h) beside the dense launch it replaces, at the two production
shapes (B = 1: S = 4992 = 13 x 16 x 24 with 32 heads x 64, S = 17556 = 21 x 22 x 38 with 32 heads x 128).

Arms, ALTERNATING inside one timed loop after a warm-up of every arm (tools/int8_attn_bench.py's protocol: device events around every
call, the median over rounds of the mean per call): ops.attention_prescaled (the dense launch the DiT uses today), ops.attention_sparse
with the FULL map (the price of the plain loop) and with window maps wf in {1, 2, 3} over the full spatial extent, sink_frames in {0, 1}.
Per arm: the map's density, the time, time / (dense time x density) - 1 would be a loop as good as the dense one that skips for
free - and the break-even density, density x dense time / time: what a map must stay under for this loop to beat the dense launch
if its time per listed tile holds.  Then one forward at 13 x 16 x 24 tokens with every block flagged (wf = 1) beside the plain one.
The dynamic arm (include/ltxhip_sparse_dynamic.h), same protocol with a second identical dense arm for the spread: ops.pool_qk,
ops.sparse_select and the batched sparse launch on the selected per-head map each on their own, and the chain of the three, for mass in
{0.5, 0.8, 0.95}, with the density the selection lands at; the forward with every block building its maps beside the two above.
Writes profiles/sparse_attn_bench.json and .md (or --out).  Needs the GPU; nothing is measured without one."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("candle-video_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import torch

from int8_bench import timed

SHAPES = (((13, 16, 24), 32, 64), ((21, 22, 38), 32, 128))
LOG2E = 1.4426950408889634
MASSES = (0.5, 0.8, 0.95)


def case(hip, geo, heads, hd, iters):
    F, H, W = geo
    S, D = F * H * W, heads * hd
    g = torch.Generator().manual_seed(S)
    q = (torch.randn(1, S, D, generator=g) * (3.0 * LOG2E * hd ** -0.5)).bfloat16().cuda()
    k, v = torch.randn(1, S, D, generator=g).bfloat16().cuda(), torch.randn(1, S, D, generator=g).bfloat16().cuda()
    maps = {"full": hip.sparse_window_map(F, H, W, F, H, W)}
    for wf in (1, 2, 3):
        for sink in (0, 1):
            maps[f"wf{wf}_sink{sink}"] = hip.sparse_window_map(F, H, W, wf, H, W, sink)
    dens = {n: hip.sparse_map_density(m, S) for n, m in maps.items()}
    dev = {n: m.cuda() for n, m in maps.items()}
    arms = {"dense": lambda: hip.ops.attention_prescaled(q, k, v, heads)}
    for n in maps:
        arms[n] = lambda n=n: hip.ops.attention_sparse(q, k, v, dev[n], heads)
    for _ in range(3):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ms = dict(zip(arms, timed(list(arms.values()), iters)))
    rows = [dict(S=S, heads=heads, head_dim=hd, arm="dense", density=1.0, ms=ms["dense"], over_dense_x_density=1.0, break_even_density=1.0)]
    for n in maps:
        rows.append(dict(S=S, heads=heads, head_dim=hd, arm=n, density=dens[n], ms=ms[n], over_dense_x_density=ms[n] / (ms["dense"] * dens[n]),
                         break_even_density=dens[n] * ms["dense"] / ms[n]))
    return rows


def dynamic(hip, geo, heads, hd, iters):
    F, H, W = geo
    S, D = F * H * W, heads * hd
    g = torch.Generator().manual_seed(S)
    q = (torch.randn(1, S, D, generator=g) * (3.0 * LOG2E * hd ** -0.5)).bfloat16().cuda()
    k, v = torch.randn(1, S, D, generator=g).bfloat16().cuda(), torch.randn(1, S, D, generator=g).bfloat16().cuda()
    qbar, kbar = hip.ops.pool_qk(q, k, heads)
    nkt = (S + 63) // 64
    arms = {"dense": lambda: hip.ops.attention_prescaled(q, k, v, heads), "dense_again": lambda: hip.ops.attention_prescaled(q, k, v, heads),
            "pool_qk": lambda: hip.ops.pool_qk(q, k, heads)}
    dens = {}
    for mass in MASSES:
        map, count = hip.ops.sparse_select(qbar, kbar, S, mass)
        dens[mass] = float(count.sum()) / (count.numel() * nkt)
        arms[f"select_{mass}"] = lambda mass=mass: hip.ops.sparse_select(qbar, kbar, S, mass)
        arms[f"sparse_{mass}"] = lambda map=map: hip.ops.attention_sparse_batched(q, k, v, map, heads)
        arms[f"chain_{mass}"] = lambda mass=mass: hip.ops.attention_sparse_batched(q, k, v, hip.ops.sparse_select(*hip.ops.pool_qk(q, k, heads), S, mass)[0], heads)
    for _ in range(3):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ms = dict(zip(arms, timed(list(arms.values()), iters)))
    base = dict(S=S, heads=heads, head_dim=hd, dense_ms=ms["dense"], dense_again_ms=ms["dense_again"], pool_qk_ms=ms["pool_qk"])
    return [dict(base, mass=mass, density=dens[mass], select_ms=ms[f"select_{mass}"], sparse_ms=ms[f"sparse_{mass}"], chain_ms=ms[f"chain_{mass}"],
                 map_building_over_dense=(ms["pool_qk"] + ms[f"select_{mass}"]) / ms["dense"]) for mass in MASSES]


def forward(hip, F, H, W, L, iters):
    import ltx_oracle as O
    from test_gpu_normfold import CFGD
    cfgd = dict(CFGD, num_layers=L)
    w = O.synth_weights(O.dit_weight_shapes(O.DitConfig(**cfgd)), seed=71)
    m = hip.LtxVideoTransformer3DModel(hip.LtxVideoTransformer3DModelConfig(**cfgd), {k: v.cuda() for k, v in w.items()}, torch.bfloat16)
    del w
    g = torch.Generator().manual_seed(2)
    S = F * H * W
    x = torch.randn(1, S, 128, generator=g).cuda(); enc = torch.randn(1, 128, 4096, generator=g).cuda()
    mask = torch.zeros(1, 128); mask[:, :40] = 1; mask = mask.cuda()
    coords = O.build_video_coords(1, F, H, W).cuda()
    run = lambda: m.forward(x, enc, [896.0], mask, F, H, W, None, coords, None)
    m.context_cache(True)
    out = dict(S=S, layers=L, iters=iters)
    map = hip.sparse_window_map(F, H, W, 1, H, W)
    for name, mp in (("plain_forward_ms", None), ("sparse_wf1_forward_ms", map)):
        m.set_sparse_attention(mp, S)
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        out[name] = timed([run], iters)[0]
    m.set_sparse_attention(None)
    out["density"] = hip.sparse_map_density(map, S)
    for mass in MASSES:                                                 # every block builds its maps; the density is the mean over the blocks
        m.set_sparse_attention_dynamic(mass)
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        out[f"dynamic_{mass}_forward_ms"] = timed([run], iters)[0]
        out[f"dynamic_{mass}_density"] = sum(m.sparse_dynamic_density()) / L
    m.set_sparse_attention_dynamic(0)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_attn_bench"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sparse_attn_bench: no GPU - nothing is measured without one")
    import ltxhip
    rows = [r for geo, heads, hd in SHAPES for r in case(ltxhip, geo, heads, hd, a.iters)]
    dyn = [r for geo, heads, hd in SHAPES for r in dynamic(ltxhip, geo, heads, hd, a.iters)]
    fwd = forward(ltxhip, 13, 16, 24, a.layers, max(a.iters // 2, 3))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out + ".json", "w") as f:
        json.dump(dict(kernel=rows, dynamic=dyn, forward=fwd), f, indent=1)
    cols = list(rows[0])
    fmt = lambda x: f"{x:.4g}" if isinstance(x, float) else str(x)
    with open(a.out + ".md", "w") as f:
        f.write("# Block-sparse self-attention beside the dense launch (tools/sparse_attn_bench.py, MI355X, device events, B = 1)\n\n")
        f.write("| " + " | ".join(cols) + " |\n|" + "---|" * len(cols) + "\n")
        for r in rows:
            f.write("| " + " | ".join(fmt(r[c]) for c in cols) + " |\n")
        f.write("\nDevice-built maps (pool_qk -> sparse_select -> the batched sparse launch; gaussian q and k):\n\n")
        f.write("| " + " | ".join(dyn[0]) + " |\n|" + "---|" * len(dyn[0]) + "\n")
        for r in dyn:
            f.write("| " + " | ".join(fmt(v) for v in r.values()) + " |\n")
        f.write("\nOne forward, every block flagged (wf = 1, full spatial extent; then device-built maps per mass): " + ", ".join(f"{k} {fmt(v)}" for k, v in fwd.items()) + "\n")
    print(json.dumps(dict(kernel=rows, dynamic=dyn, forward=fwd)))


if __name__ == "__main__":
    main()
