"""CPU suite: where the GEMM dispatch sends a call (ops.gemm_route, the read-only probe of csrc/gemm.hip's gemm_route) against
tests/golden/gemm_routes.json - the answers recorded on the dispatcher as it was BEFORE the plan table / route refactor
(tools/gen_gemm_routes.py, docs/lab_notes.md).  Every linear layer and conv of the DiT, the VAE and T5 is in the table, under
the default options, each gemm_off family, forced plans, gemm_splitk=0 and a loaded plan file: the kernel, tile and K partition
that serve a call must not move.  Nothing is launched or measured.

The second half holds the invariant whose absence let norm-fold / deferred-parts operands reach a kernel that ignores them: a
call that carries such operands is routed to the one family that honours them (asm16 tiles / ring tiles) or refused - never to
gemm128 or asm32 - and the fit tests the callers ask first (ops.linear_fold_ok, the deferred launch's own check) agree with the
route.  (A flagged call is restricted to its family, so it may go to asm16 / ring where the SAME shape without the operands is
served by another plan - a forced gemm_big tile, a plan file's choice, the static model between 512 and 2048 rows; the reverse
holds wherever the plain call is left to gemm128 / asm32.)"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_routes.json")))


@pytest.fixture(scope="module")
def probed():
    import ltxhip
    import gen_gemm_routes as G
    return ltxhip, G.routes(ltxhip, GOLDEN["calls"], GOLDEN["settings"], GOLDEN["plan_file"], GOLDEN["plan_file_calls"])


def entries():
    return [(s, c) for s, per in GOLDEN["routes"].items() for c in per]


def test_table_covers_the_dispatch():
    names = {r for per in GOLDEN["routes"].values() for r in per.values()}
    assert len(entries()) >= 300
    for fam in ("gemm128", "refused", "p8:", "halo:128", "halo:256", "halo:64", "asm16:", "asm16c:", "ring:", "256x128"):
        assert any(n.startswith(fam) for n in names), fam


def test_routes_equal_the_recorded_table(probed):
    _, got = probed
    wrong = [(s, c, got[s][c], want) for s, c in entries() for want in [GOLDEN["routes"][s][c]] if got[s][c] != want]
    assert not wrong, f"{len(wrong)} routes moved (setting, call, now, recorded): {wrong[:12]}"


def test_flagged_calls_reach_their_family_or_are_refused(probed):
    hip, got = probed
    for s, c in entries():
        call, route = GOLDEN["calls"][c], got[s][c]
        if call.get("fold_in") or call.get("fold_out"):
            assert route == "refused" or route.startswith("asm16:"), (s, c, route)
        if call.get("defer"):
            assert route == "refused" or route.startswith("ring:"), (s, c, route)


def test_fit_tests_agree_with_the_route(probed):
    hip, got = probed
    for sname, opts in GOLDEN["settings"].items():
        with hip.options(**opts):
            for c, call in GOLDEN["calls"].items():
                route = got[sname][c]
                if call.get("fold_in") or call.get("fold_out"):
                    ok = hip.ops.linear_fold_ok(call["M"], call["N"], call["K"], call["epi"], bool(call.get("fold_in")), rs_n=16 if call.get("fold_in") else 0)
                    assert ok == route.startswith("asm16:"), (sname, c, route, ok)
                elif not call.get("conv") and not call.get("defer") and call.get("dtype", "bf16") == "bf16" and route in ("gemm128", "asm32"):
                    # a shape left to a kernel that reads neither field: no fold, no deferral, whatever the epilogue
                    for consumer, epi in ((True, 0), (True, 1), (False, 2), (False, 3)):
                        assert not hip.ops.linear_fold_ok(call["M"], call["N"], call["K"], epi, consumer, rs_n=16 if consumer else 0), (sname, c)
                    with pytest.raises(hip.LtxError):
                        hip.ops.gemm_route(call["M"], call["N"], call["K"], defer=True)
