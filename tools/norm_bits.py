"""The bits of every row-norm and q/k-norm kernel (candle-video_amd/csrc/rownorm.hip, qknorm_rope.hip) over the op-level cases.
    python tools/norm_bits.py --out profiles/norm_bits_<name>.json
Run on two builds of the library (LTXHIP_LIB names a variant build), the two files must be identical entry for entry: a change
to the kernels' text that is meant to move no bit moved none.  Nothing is asserted here but that each case reaches the kernel it
names (ops.norm_route / ops.qknorm_route) and that a call repeated gives its own bits.

The cases: ROWNORM_CASES and QKNORM_CASES of tests/test_gpu_norm_kernels.py with that file's inputs (every route of both decision
steps at the smallest shape that reaches its edges), and the deferred routes - wide_defer, wide_defer4, block_defer, block_defer4 -
at the sizes of tests/test_gpu_defer.py: 1, 3 and 4 K ranges of random f32 sums, with gate and bias and without.
Each entry is the SHA-256 of the output's bytes: y; for a deferred case the finished rows x_out, then y; for a q/k case the whole
buffer, guard rows and untouched columns included."""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "candle-video_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ltxhip                               # noqa: E402
import test_gpu_norm_kernels as K           # noqa: E402

DEV = "cuda"
# (rows, D, batch elements): one row per block at 64 < D / 8 <= 512 and <= 512 rows, one wave per row otherwise
DEFER_SHAPES = {"block": [(384, 2048, 2), (301, 1032, 1)], "wide": [(96, 512, 2), (513, 1024, 1)]}


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def twice(call):
    a, b = call(), call()
    assert a == b, "a repeated call gave other bits"
    return a


def rownorm(res):
    for i, c in enumerate(K.ROWNORM_CASES):
        assert K.rownorm_route(ltxhip, c) == c["route"], c["id"]
        inp = K.rownorm_inputs(c, i)

        def call():
            y = K.run_rownorm(ltxhip, c, inp)
            torch.cuda.synchronize()
            return sha(y)
        res["rownorm/" + c["id"]] = twice(call)


def deferred(res):
    seed = 0
    for family, shapes in DEFER_SHAPES.items():
        for rows, D, nb in shapes:
            for P in (1, 3, 4):
                for full in (True, False):             # gate + bias and RMS; neither and LayerNorm
                    seed += 1
                    route = f"{family}_defer4" if P == 4 else f"{family}_defer"
                    kind, rpb = (0 if full else 1), rows // nb
                    assert ltxhip.ops.norm_route(rows, D, torch.bfloat16, kind=kind, scale=True, rows_per_batch=rpb, nparts=P) == route, (route, rows, D, P)
                    g = torch.Generator().manual_seed(9000 + seed)
                    parts = torch.randn(P, rows, D, generator=g).to(DEV)
                    h0 = torch.randn(rows, D, generator=g).bfloat16().to(DEV)
                    bias = torch.randn(D, generator=g).bfloat16().to(DEV) if full else None
                    gate = torch.randn(nb, D, generator=g).to(DEV) if full else None
                    scale, shift = (0.1 * torch.randn(nb, D, generator=g)).to(DEV), (0.1 * torch.randn(nb, D, generator=g)).to(DEV)

                    def call():
                        h, y = ltxhip.ops.rownorm_deferred(parts, bias, h0, gate, kind=kind, eps=1e-6, scale=scale, shift=shift, rows_per_batch=rpb)
                        torch.cuda.synchronize()
                        return sha(h, y)
                    res[f"deferred/{route}-{rows}x{D}-p{P}-k{kind}-rpb{rpb}-{'gate-bias' if full else 'plain'}"] = twice(call)


def qknorm(res):
    for i, c in enumerate(K.QKNORM_CASES):
        assert K.qknorm_route(ltxhip, c) == c["route"], c["id"]
        inp = K.qknorm_inputs(c, i)
        _, _, ld, nseg, seg_stride, _ = K.qk_layout(c)

        def call():
            buf = inp["buf"].to(DEV)
            ltxhip.ops.qknorm_rope_segs(buf, c["rows"], c["D"], ld, nseg, seg_stride, K.dv(inp["w0"]), K.dv(inp["w1"]), K.dv(inp["w0b"]), K.EPS_QK,
                                        K.dv(inp["cos"]), K.dv(inp["sin"]), inp["out_scale0"])
            torch.cuda.synchronize()
            return sha(buf)
        res["qknorm/" + c["id"]] = twice(call)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("norm_bits.py needs a GPU")
    res = {}
    rownorm(res)
    deferred(res)
    qknorm(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=0, sort_keys=True) + "\n")
    print(json.dumps({"entries": len(res), "out": a.out, "sha_of_all": hashlib.sha256(json.dumps(res, sort_keys=True).encode()).hexdigest()}))


if __name__ == "__main__":
    main()
