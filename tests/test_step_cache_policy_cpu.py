"""CPU suite: the step cache's policy (candle-video_amd/host/step_cache.h), the rule ltx_step_cache_decide applies to a measurement.

The header is built for the host alone with AddressSanitizer + UBSan into a stand-alone program (tests/host/step_cache_main.cpp);
nothing is preloaded.  Numbers travel as bit patterns.  Every decision and every accumulator it prints is compared, integer for
integer and bit for bit, with tests/step_cache_ref.py's `policy` - whose arithmetic is Python's: IEEE doubles, Horner as written."""
import os
import random
import shutil
import struct
import subprocess

import pytest

import step_cache_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    pkg = os.path.join(ROOT, "candle-video_amd")
    b = subprocess.run(["make", "-C", pkg, "asan_step_cache"], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    return os.path.join(pkg, "build", "asan", "ltx_step_cache_asan")


def u32(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def u64(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def _run(exe, text):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=120)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


def trace_text(params, have, acc, steps):
    pat = list(params.pattern or [])
    head = ["trace", u32(params.rel_l1_thresh)] + [u32(c) for c in params.coeff] + [int(have), u64(acc), len(pat)] + pat + [len(steps)]
    return " ".join(str(v) for v in head) + "\n" + "".join(f"{i} {N} {u64(num)} {u64(den)} {int(valid)}\n" for i, N, num, den, valid in steps)


def expect(params, have, acc, steps):
    st = R.Policy(acc=acc, have_prev=have)
    out = []
    for i, N, num, den, valid in steps:
        reuse = R.policy(st, params, i, N, num, den, valid)
        out.append(f"{int(reuse)} {R.acc_bits(st.acc)} {int(st.have_prev)}")
    return out


def check(exe, cases):
    got = _run(exe, "".join(trace_text(*c) for c in cases))
    want = [line for c in cases for line in expect(*c)]
    assert got == want


SPECIAL = [0.0, -0.0, 1e-300, 1e300, float("inf"), float("-inf"), float("nan"), 0.03, 1.0]
COEFFS = [(0.0, 0.0, 0.0, 1.0, 0.0), (17.5, -9.25, 1.75, 0.625, 0.0078125),      # (an arbitrary quartic, nobody's fit)
          (0.1, -0.2, 0.3, 0.5, 0.0), (0.0, 0.0, 0.0, 0.0, 0.25)]


def test_random_traces_agree_bit_for_bit(exe):
    rnd = random.Random(1729)
    cases = []
    for k in range(400):
        N = rnd.randint(1, 12)
        coeff = rnd.choice(COEFFS) if k % 3 else tuple(rnd.uniform(-2, 2) for _ in range(5))
        pat = None
        if rnd.random() < 0.5:
            pat = [rnd.choice([0, 0, 0, 1, 2]) for _ in range(rnd.randint(1, N + 2))]      # shorter, equal and longer than the call
        params = R.Params(rnd.choice([0.0, 0.05, 0.3, 1.0, 1e9]), coeff, pat)
        steps = []
        for i in range(N):
            den = rnd.choice(SPECIAL) if rnd.random() < 0.1 else rnd.uniform(1.0, 1e6)
            num = rnd.choice(SPECIAL) if rnd.random() < 0.1 else den * rnd.choice([rnd.uniform(0, 0.1), rnd.uniform(0, 2)])
            steps.append((i, N, num, den, rnd.random() > 0.15))
        cases.append((params, rnd.random() < 0.2, rnd.choice([0.0, 0.01, 0.7]), steps))
    assert sum(len(c[3]) for c in cases) > 2000
    want = [line for c in cases for line in expect(*c)]
    assert any(l.startswith("1 ") for l in want) and any(l.startswith("0 ") for l in want)
    check(exe, cases)


def test_every_reset_case(exe):
    """each reason to compute, alone, from a state that would otherwise re-use: acc comes back as 0"""
    p = R.Params(1.0, COEFFS[0], None)
    ok = (2, 6, 1.0, 100.0, True)                                       # d = 0.01: re-used from (have, acc = 0.5)
    st = R.Policy(acc=0.5, have_prev=True)
    assert R.policy(st, p, *ok) and st.acc == 0.5 + 0.01
    resets = {"no previous measurement": (False, (2, 6, 1.0, 100.0, True)), "i == 0": (True, (0, 6, 1.0, 100.0, True)),
              "i == N - 1": (True, (5, 6, 1.0, 100.0, True)), "den == 0": (True, (2, 6, 1.0, 0.0, True)), "den == -0": (True, (2, 6, 1.0, -0.0, True)),
              "0 / 0": (True, (2, 6, 0.0, 0.0, True)), "d = inf": (True, (2, 6, float("inf"), 100.0, True)), "d = nan": (True, (2, 6, float("nan"), 100.0, True)),
              "den = nan": (True, (2, 6, 1.0, float("nan"), True)), "an invalid row": (True, (2, 6, 1.0, 100.0, False)),
              "threshold reached": (True, (2, 6, 60.0, 100.0, True)), "N == 1": (True, (0, 1, 1.0, 100.0, True))}
    cases = []
    for why, (have, step) in resets.items():
        st = R.Policy(acc=0.5, have_prev=have)
        assert not R.policy(st, p, *step) and st.acc == 0.0 and st.have_prev, why
        cases.append((p, have, 0.5, [step, ok]))                         # ... and the step after starts from 0
    check(exe, cases)


def test_pattern_semantics(exe):
    p = R.Params(0.05, COEFFS[0], [0, 2, 1, 2, 0, 0])
    steps = [(i, 8, 4.0, 100.0, True) for i in range(8)]               # d = 0.04 on every step
    st = R.Policy()
    got = [(R.policy(st, p, *s), st.acc) for s in steps]
    #       first    forced reuse  forced compute  forced reuse  0.04 < 0.05  0.08: compute  past the pattern  last step
    assert got == [(False, 0.0), (True, 0.0), (False, 0.0), (True, 0.0), (True, 0.04), (False, 0.0), (True, 0.04), (False, 0.0)]
    st = R.Policy(acc=0.03, have_prev=True)
    assert R.policy(st, R.Params(0.05, COEFFS[0], [2]), 0, 4, 1.0, 1.0, True) and st.acc == 0.03          # a forced reuse leaves acc, even on step 0
    assert not R.policy(st, R.Params(0.05, COEFFS[0], [2]), 0, 4, 1.0, 1.0, False) and st.acc == 0.0      # ... but not without a residual
    check(exe, [(p, False, 0.0, steps), (R.Params(0.05, COEFFS[0], [2]), True, 0.03, [(0, 4, 1.0, 1.0, True), (0, 4, 1.0, 1.0, False)]),
                (R.Params(0.05, COEFFS[0], [1, 1, 1]), True, 0.04, [(1, 4, 0.0, 1.0, True)])])


def test_the_default_never_reuses(exe):
    p = R.Params()
    steps = [(i, 9, 0.0, 5.0, True) for i in range(9)]                 # not even at distance 0: acc < 0 is false
    assert all(l.startswith("0 ") for l in expect(p, False, 0.0, steps))
    check(exe, [(p, False, 0.0, steps)])


def test_parameter_check(exe):
    def line(thresh, coeff, pat, null=0):
        return " ".join(str(v) for v in ["check", u32(thresh)] + [u32(c) for c in coeff] + [len(pat)] + list(pat) + [null]) + "\n"
    got = _run(exe, line(0.1, COEFFS[0], []) + line(-0.1, COEFFS[0], []) + line(float("nan"), COEFFS[0], []) + line(float("inf"), COEFFS[0], []) +
               line(0.1, (0.0, float("inf"), 0.0, 1.0, 0.0), []) + line(0.1, COEFFS[0], [0, 1, 2]) + line(0.1, COEFFS[0], [0, 3]) + line(0.1, COEFFS[0], [0, 1], 1))
    assert got[0] == "ok" and got[5] == "ok"
    assert "rel_l1_thresh" in got[1] and "rel_l1_thresh" in got[2] and "rel_l1_thresh" in got[3]
    assert "coefficient" in got[4] and "0 (decide), 1 (compute) or 2 (reuse)" in got[6] and "null" in got[7]
