"""CPU unit test of the LM step driver's host policy (instantsfm_amd/csrc/lm_policy.h, used by csrc/ba_step.h lm_step
and csrc/ba_solve.h): the TrustRegion update bitwise against a restatement of the oracle's (oracle/ba_oracle.c
ora_step, "pypose TrustRegion.update"), the accept rule, the whole decision table after a k_tl_cgp launch that did not
converge, the CG launch counts and the PCG error texts.  tests/cpp/lm_policy_test.cpp answers one query per line and
prints doubles as %a, so every comparison is exact."""
import itertools
import math
import os
import shutil
import struct
import subprocess
from types import SimpleNamespace

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# insfm_ba_default_desc (TrustRegion(1e4, 1e10, 1e-6, 2, 1/16, 0.25, 0.5, 1e-3))
PRODUCT = SimpleNamespace(rmax=1e10, rmin=1e-6, up=2.0, down0=1.0 / 16.0, factor=0.25, high=0.5, low=1e-3)
HALF = SimpleNamespace(**{**vars(PRODUCT), "factor": 0.5})


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("lm_policy") / "lm_policy_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe,
                    os.path.join(REPO, "tests", "cpp", "lm_policy_test.cpp")], check=True)

    def run(queries):
        out = subprocess.run([exe], input="".join(q + "\n" for q in queries), check=True, capture_output=True,
                             text=True, timeout=60).stdout.splitlines()
        assert len(out) == len(queries)
        return out
    return run


def hx(x):
    return x.hex() if isinstance(x, float) else str(x)


def same_bits(a, b):
    return (math.isnan(a) and math.isnan(b)) or struct.pack("<d", a) == struct.pack("<d", b)


def clampd(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)


def ora_tr_update(damping, down, quality, o):
    """oracle/ba_oracle.c ora_step: pypose TrustRegion.update"""
    radius = 1.0 / damping
    if quality > o.high:
        radius = o.up * radius
        down = o.down0
    elif quality > o.low:
        down = o.down0
    else:
        radius = radius * down
        down = down * o.factor
    radius = clampd(radius, o.rmin, o.rmax)
    return 1.0 / radius, down


def tr_query(damping, down, quality, o):
    return "tr " + " ".join(hx(float(v)) for v in (damping, down, quality, o.rmax, o.rmin, o.up, o.down0, o.factor,
                                                  o.high, o.low))


def parse2(line):
    a, b = line.split()
    return float.fromhex(a), float.fromhex(b)


QUALITIES = [0.9, 0.5, 0.25, 1e-3, 1e-4, -3.0, math.inf, -math.inf, math.nan]


@pytest.mark.parametrize("opts", [PRODUCT, HALF], ids=["product", "tr_factor_half"])
def test_tr_update_bitwise(ask, opts):
    # dampings: the start (1 / 1e4), mid-run values, one whose shrunk radius falls below tr_min (1e5 -> 6.25e-7) and
    # one whose grown radius exceeds tr_max (1e-10 -> 2e10); downs: fresh and compounded
    cases = [(dmp, down, q) for dmp in (1e-4, 0.37, 3.0, 1e5, 1e6, 1e-10, 7e-11)
             for down in (opts.down0, opts.down0 * opts.factor ** 3) for q in QUALITIES]
    out = ask([tr_query(dmp, down, q, opts) for dmp, down, q in cases])
    hit_min = hit_max = False
    for (dmp, down, q), line in zip(cases, out):
        got, want = parse2(line), ora_tr_update(dmp, down, q, opts)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), (dmp, down, q, got, want)
        hit_min |= got[0] == 1.0 / opts.rmin
        hit_max |= got[0] == 1.0 / opts.rmax
    assert hit_min and hit_max
    # NaN takes the shrink branch: the radius shrinks by `down`, `down` compounds
    nan_dmp, nan_down = parse2(ask([tr_query(0.37, opts.down0, math.nan, opts)])[0])
    assert nan_dmp == 1.0 / ((1.0 / 0.37) * opts.down0) and nan_down == opts.down0 * opts.factor


@pytest.mark.parametrize("opts", [PRODUCT, HALF], ids=["product", "tr_factor_half"])
def test_tr_update_forty_shrinks_then_one_good_trial(ask, opts):
    dmp, down = 1e-4, opts.down0
    for k in range(40):
        got = parse2(ask([tr_query(dmp, down, -1.0, opts)])[0])
        want = ora_tr_update(dmp, down, -1.0, opts)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), k
        assert got[1] == opts.down0 * opts.factor ** (k + 1)  # (powers of two: exact)
        dmp, down = got
    assert dmp == 1.0 / opts.rmin
    got = parse2(ask([tr_query(dmp, down, 0.9, opts)])[0])
    assert got == ora_tr_update(dmp, down, 0.9, opts) and got[1] == opts.down0 and got[0] < dmp


def test_gain_quality_bitwise(ask):
    cases = [(10.0, 9.0, 0.7, 0.5), (1.0, 1.0, 0.3, 0.1), (3.0, 4.5, 1e-9, 2e-9), (1.0, 0.5, 0.0, 0.0),
             (0.1, 0.3, -0.2, 0.1)]
    out = ask(["gq " + " ".join(hx(v) for v in c) for c in cases])
    for (last, new, gp, gc), line in zip(cases, out):
        assert same_bits(float.fromhex(line), (last - new) / (gp + gc) if gp + gc else math.inf)


def test_trial_verdict(ask):
    q = ["verdict 0 0x1p+0 0x1p+0 0 30",   # last == loss_new accepts
         "verdict 0 0x1p+0 0x1p+1 30 30",  # worse, no rejects left: accepts
         "verdict 0 0x1p+0 0x1p+1 29 30",  # worse, rejects left
         "verdict 0 0x1p+1 0x1p+0 0 30",   # better
         "verdict 1 0x1p+1 0x1p+0 0 30", "verdict 1 0x1p+0 0x1p+1 0 30", "verdict 1 0x1p+0 0x1p+1 30 30",
         "verdict 0 0x1p+0 nan 0 30"]      # a NaN loss is not "worse": accepted, as the oracle's `last < loss_new`
    assert ask(q) == ["accept", "accept", "reject", "accept", "fail", "fail", "fail", "accept"]


def cgp_rule(status, not_spd, multi, any_rank_abort, cgp_lost, adef2):
    """The ordered rule of lm_step after a k_tl_cgp launch, written out from its specification."""
    if not_spd:
        return "fail_step"
    if multi and any_rank_abort:
        return "repeat_collective"
    if status == 4 and cgp_lost:
        return "repeat_launch_path"
    if status == 2 and adef2:
        return "repeat_additive"
    if status != 1:
        return "fail_step" if status == 2 else "device_error"
    return "converged"


def test_cgp_next_whole_table(ask):
    rows = list(itertools.product((0, 1, 2, 3, 4), *([(0, 1)] * 5)))
    assert len(rows) == 160
    out = ask(["next " + " ".join(map(str, r)) for r in rows])
    assert out == [cgp_rule(*r) for r in rows]
    assert set(out) == {"converged", "fail_step", "repeat_collective", "repeat_launch_path", "repeat_additive",
                        "device_error"}


def test_launch_counts(ask):
    assert ask(["batch 16 100 1 2", "batch 0 100 1 2", "batch 50 1 1 2"]) == ["14", "3", "3"]
    assert ask(["barriers 0 0", "barriers 0 7", "barriers 1 0", "barriers 1 7"]) == ["2", "9", "3", "17"]


def test_pcg_status_messages(ask):
    """The texts of the two sites (cg_tail: coarse count or -1 = off; lm_step's late k_tl_cgp status: -2)."""
    assert ask(["msg 2 7 3", "msg 4 0 -1", "msg 0 502 1", "msg 3 9 -1", "msg 2 2 -2", "msg 4 5 -2"]) == [
        "PCG breakdown at iteration 7 (status 2, coarse 3)",
        "PCG timed out (a k_tl_cgp grid barrier or a cross-rank exchange of the partitioned CG) at iteration 0 "
        "(status 4, coarse off)",
        "PCG did not finish at iteration 502 (status 0, coarse 1)",
        "PCG did not finish at iteration 9 (status 3, coarse off)",
        "PCG breakdown at iteration 2 (status 2)",
        "PCG timed out (a k_tl_cgp grid barrier) at iteration 5 (status 4)",
    ]
