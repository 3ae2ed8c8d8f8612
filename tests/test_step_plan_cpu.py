"""CPU suite: the denoise loop's step plan (candle-video_amd/host/step_plan.h), the data that host/pipeline.hip's loop walks.

The header is built for the host alone with AddressSanitizer + UBSan into a stand-alone program (tests/host/step_plan_main.cpp), one
run per case.  Every integer it prints is compared with tests/step_plan_ref.py."""
import json
import os
import shutil
import subprocess

import pytest

import step_plan_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPOSITIONS = [(1.0, 0.0), (3.0, 0.0), (1.0, 1.0), (3.0, 1.0)]                      # text, + uncond, + perturbed, all three
# the schedule of tests/test_gpu_guidance_sched.py resolved over six steps: it visits all four compositions
FOUR = [(1.0, 0.0, 1.0, []), (3.0, 0.0, 0.5, []), (3.0, 0.0, 0.5, []), (1.0, 1.0, 0.5, [1]), (1.0, 1.0, 0.5, [1]), (8.0, 4.0, 0.7, [0, 2])]


@pytest.fixture(scope="module")
def exe():
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    pkg = os.path.join(ROOT, "candle-video_amd")
    b = subprocess.run(["make", "-C", pkg, "asan_step_plan"], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    return os.path.join(pkg, "build", "asan", "ltx_step_plan_asan")


def _run(exe, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=60)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (args, r.stderr[-2000:])
    return json.loads(r.stdout)


def _list(k):
    return "-" if k is None else ("e" if len(k) == 0 else ",".join(str(v) for v in k))


def _guide(g, s, r, k):
    return [repr(g), repr(s), repr(r), _list(k)]


def constant(exe, N, B, gb, g, s, r, k):
    got = _run(exe, ["plan", B, gb, "const", N] + _guide(g, s, r, k))
    assert got == R.plan([(g, s, r, k)] * N, B, gb), (N, B, gb, g, s, r, k)
    return got


def scheduled(exe, B, gb, guides, cfg_star=0, form=0):
    got = _run(exe, ["plan", B, gb, "sched", cfg_star, form, len(guides)] + [a for gd in guides for a in _guide(*gd)])
    assert got == R.plan(guides, B, gb, True, cfg_star, form), (B, gb, guides, cfg_star, form)
    return got


def test_every_composition_option_and_batch_size(exe):
    for B in (1, 2, 3, 4, 5):
        for gb in (0, 1):
            for g, s in COMPOSITIONS:
                for k in (None, [], [1], [0, 2]):
                    constant(exe, 3, B, gb, g, s, 0.7, k)
            for star, form in ((0, 0), (1, 1)):
                scheduled(exe, B, gb, FOUR, star, form)


def test_the_eight_row_edge(exe):
    at8 = constant(exe, 2, 4, 1, 3.0, 0.0, 0.7, None)                                 # two branches of four rows: exactly 8
    assert at8["steps"][0] == [1, 0, 2, 1, 0, 8, []] and at8["any_batched"] == 1
    at9 = constant(exe, 2, 3, 1, 3.0, 1.0, 0.7, [1])                                  # three of three: 9 rows run separately
    assert at9["steps"][0] == [1, 1, 3, 0, 0, 9, [1]] and at9["any_batched"] == 0
    for g, s in COMPOSITIONS:
        assert constant(exe, 2, 5, 1, g, s, 0.7, [1])["any_batched"] == 0              # B = 5 is never batched
    assert constant(exe, 2, 4, 0, 3.0, 0.0, 0.7, None)["any_batched"] == 0             # the option off
    mixed = scheduled(exe, 3, 1, FOUR)                                                # per step: two branches fit, three do not
    assert [st[3] for st in mixed["steps"]] == [0, 1, 1, 1, 1, 0] and mixed["any_batched"] == 1


def test_slots_are_a_contiguous_run(exe):
    p = scheduled(exe, 2, 1, FOUR, 1, 1)
    assert [(st[4], st[2]) for st in p["steps"]] == [(1, 1), (0, 2), (0, 2), (1, 2), (1, 2), (0, 3)]
    assert [st[6] for st in p["steps"]] == [[], [], [], [1], [1], [0, 2]]
    assert (p["any_cfg"], p["any_stg"], p["mix"], p["cfg_star"], p["rescale_form"], p["handle"], p["handle_null"]) == (1, 1, 1, 1, 1, [], 1)
    # STG only, unscheduled: slots 1-2, the same layout a schedule uses
    assert constant(exe, 1, 2, 1, 1.0, 1.0, 0.0, [1])["steps"][0] == [0, 1, 2, 1, 1, 4, [1]]


def test_the_handles_permanent_list(exe):
    assert constant(exe, 2, 1, 1, 3.0, 0.0, 0.7, [1])["handle"] == [1]                 # STG off: the list skips for good
    on = constant(exe, 2, 1, 1, 3.0, 1.0, 0.7, [1])
    assert (on["handle"], on["handle_null"]) == ([], 1)                               # STG on: cleared, the list perturbs slot 2
    assert constant(exe, 2, 1, 1, 3.0, 1.0, 0.7, None)["handle"] is None               # no list: the handle is left alone
    assert constant(exe, 2, 1, 1, 1.0, 0.0, 0.0, [])["handle"] == []


def test_constant_schedules(exe):
    for g, s, k in ((3.0, 1.0, [1]), (3.0, 0.0, []), (1.0, 0.0, []), (3.0, 1.0, [])):
        for N in (1, 6):
            p = scheduled(exe, 2, 1, [(g, s, 0.7, k)] * N)
            assert p["mix"] == 0 and p["handle"] == [] and p["handle_null"] == int(s > 0)
            un = constant(exe, N, 2, 1, g, s, 0.7, k if s > 0 else [])
            assert p["steps"] == un["steps"]
        assert scheduled(exe, 2, 1, [(g, s, 0.7, k)] * 3, 1, 0)["mix"] == 1              # the same values with CFG-star
        assert scheduled(exe, 2, 1, [(g, s, 0.7, k)] * 3, 0, 1)["mix"] == 1              # ... or LTX_RESCALE_MIX: the _ex mix
    # s == 0: the lists are not compared, none is handed on, and the handle is cleared through an empty list
    p = scheduled(exe, 1, 1, [(3.0, 0.0, 0.5, [1]), (3.0, 0.0, 0.5, [2])])
    assert p["mix"] == 0 and p["steps"][0][6] == [] and (p["handle"], p["handle_null"]) == ([], 0)
    # s > 0: another list, another rescale or another scale is another step
    assert scheduled(exe, 1, 1, [(3.0, 1.0, 0.5, [1]), (3.0, 1.0, 0.5, [2])])["mix"] == 1
    assert scheduled(exe, 1, 1, [(3.0, 1.0, 0.5, [1]), (3.0, 1.0, 0.6, [1])])["mix"] == 1
    assert scheduled(exe, 1, 1, [(3.0, 1.0, 0.5, [1]), (3.0, 1.0, 0.5, [1, 2])])["mix"] == 1


def test_step_skip_rows(exe):
    cases = [(3, 2, 0, 2, [1]), (3, 6, 4, 2, [0, 2]), (3, 4, 2, 2, [1]), (3, 9, 6, 3, [0, 1, 2]), (3, 2, 0, 2, []), (3, 2, 0, 2, None),
             (3, 4, 2, 2, [3]), (3, 4, 2, 2, [-1, 1, 7]), (1, 1, 0, 1, [0])]            # 3, -1 and 7 lie outside the model: dropped
    for L, rows, row0, B, k in cases:
        assert _run(exe, ["rows", L, rows, row0, B, _list(k)]) == R.skip_rows(L, rows, row0, B, k), (L, rows, row0, B, k)
    assert _run(exe, ["rows", 3, 4, 2, 2, "-1,1,7"]) == [[0, 0, 0, 0], [0, 0, 1, 1], [0, 0, 0, 0]]
