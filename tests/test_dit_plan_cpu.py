"""CPU suite: the decisions of the DiT forward (ops.dit_plan, the read-only probe of csrc/dit.hip's ltx_dit_plan) against
tests/golden/dit_plans.json - the answers recorded on the decision code as it stood inside the forward, with its hand-written
fit-test arguments, BEFORE the GEMM argument builders served both the fit tests and the launches (tools/gen_dit_plans.py,
docs/lab_notes.md).  2B, 13B, the GPU tests' reduced dims and a D that is no power of two; 48 .. 17556 rows per batch row, 1 .. 8
rows, one timestep per row or per frame, 8 .. 256 text tokens, both dtypes, with and without a skip-layer mask; under the default
options and every option the decisions read.  Nothing is launched.

The second half holds what the block loop relies on: the norm fold only over the row partials, no deferred ff2 where the partials
are wanted from its epilogue, and a plan that says fold only where the GEMM dispatch agrees (ops.linear_fold_ok) for the four
calls that carry the fold's operands."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "dit_plans.json")))
BIAS, GELU, GATE_RESID, RESID = range(4)


@pytest.fixture(scope="module")
def G():
    import gen_dit_plans
    return gen_dit_plans


@pytest.fixture(scope="module")
def probed(G):
    import ltxhip
    return ltxhip, G.plans(ltxhip, GOLDEN["dims"], GOLDEN["rows"], GOLDEN["batch"], GOLDEN["text"], GOLDEN["settings"])


def entries(G, table):
    """(setting, (heads, head_dim), shape, decisions) of every plan of a table"""
    shapes = G.shapes(GOLDEN["rows"], GOLDEN["batch"], GOLDEN["text"])
    for s, per in table.items():
        for d in GOLDEN["dims"]:
            codes = per[f"{d[0]}x{d[1]}"]
            assert len(codes) == 2 * len(shapes)
            for i, sh in enumerate(shapes):
                yield s, d, sh, G.decode(codes[2 * i:2 * i + 2])


def test_table_covers_the_decisions(G):
    rows = list(entries(G, GOLDEN["plans"]))
    assert len(rows) >= 30000
    for k in G.DECISIONS:
        assert {p[k] for _, _, _, p in rows} == ({1, 4} if k == "ff2_parts" else {False, True}), k


def test_plans_equal_the_recorded_table(probed):
    _, got = probed
    wrong = [(s, d) for s, per in GOLDEN["plans"].items() for d, want in per.items() if got[s][d] != want]
    assert not wrong, f"plans moved under (setting, dims): {wrong}"


def test_sizes(probed, G):
    hip, _ = probed
    for d in GOLDEN["dims"]:
        for sh in G.shapes(GOLDEN["rows"], GOLDEN["batch"], GOLDEN["text"])[::37]:
            p, D = G.probe(hip, d, sh), d[0] * d[1]
            assert (p["M"], p["MK"], p["NB"], p["Sg"]) == (sh["B"] * sh["S"], sh["B"] * sh["K"], sh["B"] * sh["G"], sh["S"] // sh["G"])
            assert (p["seg"], p["ldqkv"]) == ((p["M"] * D, D) if p["dense_qkv"] else (D, 3 * D))


def test_decisions_imply_what_the_block_loop_assumes(probed, G):
    _, got = probed
    for s, d, sh, p in entries(G, got):
        assert not p["nfold"] or p["presum"], (s, d, sh)
        assert not p["defer_ff2"] or not p["presum"], (s, d, sh)
        assert (p["ff2_parts"] > 1) == p["defer_ff2"], (s, d, sh)
        assert not p["nfold"] or p["dense_qkv"], (s, d, sh)


def test_a_plan_that_folds_agrees_with_the_dispatch(probed, G):
    hip, got = probed
    checked = set()
    for s, d, sh, p in entries(G, got):
        D, M, Sg = d[0] * d[1], sh["B"] * sh["S"], sh["S"] // sh["G"]
        if not p["nfold"] or (s, D, M, Sg) in checked:
            continue
        checked.add((s, D, M, Sg))
        with hip.options(**GOLDEN["settings"][s]):
            assert hip.ops.linear_fold_ok(M, D, D, RESID, False, 0, 6 * D, Sg), (s, d, sh, "o2")
            assert hip.ops.linear_fold_ok(M, D, 4 * D, GATE_RESID, False, 0, 6 * D, Sg), (s, d, sh, "ff2")
            assert hip.ops.linear_fold_ok(M, 3 * D, D, BIAS, True, D // 128, 3 * D, Sg), (s, d, sh, "qkv1")
            assert hip.ops.linear_fold_ok(M, 4 * D, D, GELU, True, D // 128, 4 * D, Sg), (s, d, sh, "ff1")
    assert len(checked) >= 20
