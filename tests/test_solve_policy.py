"""CPU unit test of the host decisions of one linear solve (instantsfm_amd/csrc/solve_policy.h, executed by
csrc/ba_solve.h run_solve and csrc/ba_step.h repeat_trial): plan_solve over its whole input space against a restatement
of the conditions run_solve, run_tl_setup and run_tl_cg held before the decisions moved (each with the line of
csrc/ba_solve.h at commit 020b1aa it restates), named rows literally, the three repeat recipes as exact step sets,
k_tl_cgp's flag word and insfm_ba_cg_info's path code.  tests/cpp/solve_policy_test.cpp answers one query per line
and prints doubles as %a, so every comparison is exact."""
import itertools
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BOOLS = ("optimize_poses", "tlon", "prog_host", "cgp", "u_late", "rank0", "has_points", "keep_S", "flags_dirty",
         "prep_valid", "tl_fresh", "async_status")
CMIN, CMAX, F = 1e-6, 1e32, 1.0001  # insfm_ba_default_desc's clamps; the first trial's factor at the start damping


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("solve_policy") / "solve_policy_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe,
                    os.path.join(REPO, "tests", "cpp", "solve_policy_test.cpp")], check=True)

    def run(queries):
        out = subprocess.run([exe], input="".join(q + "\n" for q in queries), check=True, capture_output=True,
                             text=True, timeout=120).stdout.splitlines()
        assert len(out) == len(queries)
        return out
    return run


def facts(**kw):
    s = dict(kind=0, optimize_poses=1, tlon=1, prog_host=1, cgp=1, u_late=0, rank0=1, has_points=1, keep_S=0,
             flags_dirty=0, prep_valid=0, prep_f=0.0, tl_solves=0, tl_fresh=0, async_status=1, clamp_min=CMIN,
             clamp_max=CMAX, f=F)
    assert set(kw) <= set(s), kw
    s.update(kw)
    return s


def plan_query(s):
    return "plan " + " ".join(
        str(int(s[k])) for k in ("kind", "optimize_poses", "tlon", "prog_host", "cgp", "u_late", "rank0", "has_points",
                                 "keep_S", "flags_dirty", "prep_valid")) + " " + float(s["prep_f"]).hex() + \
        f" {s['tl_solves']} {int(s['tl_fresh'])} {int(s['async_status'])} " + \
        " ".join(float(s[k]).hex() for k in ("clamp_min", "clamp_max", "f"))


FIELDS = ("prepared", "zero_words", "sf", "smin", "smax", "sdiag", "add_U_in_factor", "scale", "basis_by_factor", "cg",
          "dc_by_cgp", "slot", "use", "defer_chain", "must_wait_fact")


def parse_plan(line):
    t = line.split()
    assert len(t) == len(FIELDS), line
    p = {}
    for name, v in zip(FIELDS, t):
        p[name] = float.fromhex(v) if name in ("sf", "smin", "smax") else v if name == "cg" else int(v)
    return p


def parent_plan(s):
    """What run_solve / run_tl_setup / run_tl_cg computed between their launches (csrc/ba_solve.h at 020b1aa)."""
    gpk = s["kind"] == 1                                                       # L752  gpk = h->kind == 1
    p = {}
    p["prepared"] = int(bool(s["prep_valid"] and s["prep_f"] == s["f"] and s["kind"] == 0))  # L742
    p["zero_words"] = int(bool(s["flags_dirty"] or not s["has_points"] or s["kind"] == 1))   # L746
    p["sf"] = 1.0 if gpk else s["f"]                                           # L756
    p["smin"] = -1.0e308 if gpk else s["clamp_min"]                            # L757
    p["smax"] = 1.0e308 if gpk else s["clamp_max"]                             # L757
    p["sdiag"] = 1 if gpk else (0 if s["u_late"] else int(bool(s["rank0"])))   # L758
    p["add_U_in_factor"] = int(bool(s["u_late"] and not gpk))                  # L807  ul
    p["scale"] = int(not (s["tlon"] and s["cgp"] and s["tl_solves"] > 0 and s["tl_fresh"] and not s["keep_S"]))  # L811
    p["basis_by_factor"] = int(bool(s["tlon"] and s["cgp"] and not gpk))       # L813
    if not s["optimize_poses"]:                                                # L773  if (h->d.optimize_poses)
        cg = "none"
    elif not (s["tlon"] and s["prog_host"]):                                   # L828  ? run_tl_cg : run_bj_cg
        cg = "block_jacobi"
    elif not s["cgp"]:                                                         # L510 / L528  h->cgp_nb ? ... : ...
        cg = "launch_path"
    else:
        cg = "persistent_async" if s["async_status"] else "persistent"        # L543  h->cgp_nb && h->cg_async
    p["cg"] = cg
    # L499  h->dc_by_cgp = h->cgp_nb != 0, set where run_tl_cg runs (L773, L828); false on a handle it never runs on
    p["dc_by_cgp"] = int(bool(s["optimize_poses"] and s["tlon"] and s["prog_host"] and s["cgp"]))
    slot = s["tl_solves"] & 1                                                  # L262
    use = slot ^ 1 if (s["tl_solves"] > 0 and s["tl_fresh"]) else slot         # L266
    p["slot"], p["use"] = slot, use
    p["defer_chain"] = int(bool(s["cgp"] and use != slot))                     # L270  cgp_defer
    p["must_wait_fact"] = int(use == slot)                                     # L278  use == slot || hipEventQuery(...)
    return p


def test_plan_solve_whole_table(ask):
    rows = []
    for kind in (0, 1):
        for bits in itertools.product((0, 1), repeat=len(BOOLS)):
            for tl_solves in (0, 1, 2):
                for prep_f in (F, 2.0 * F):
                    rows.append(facts(kind=kind, tl_solves=tl_solves, prep_f=prep_f, **dict(zip(BOOLS, bits))))
    assert len(rows) == 2 * 2 ** 12 * 3 * 2
    out = ask([plan_query(s) for s in rows])
    seen = set()
    for s, line in zip(rows, out):
        got, want = parse_plan(line), parent_plan(s)
        assert got == want, (s, got, want)
        seen.add(got["cg"])
    assert seen == {"none", "block_jacobi", "launch_path", "persistent", "persistent_async"}


def plan_of(ask, **kw):
    return parse_plan(ask([plan_query(facts(**kw))])[0])


def test_first_solve_uses_its_own_slot(ask):
    p = plan_of(ask, tl_solves=0, tl_fresh=1)
    assert (p["slot"], p["use"], p["defer_chain"], p["must_wait_fact"], p["scale"]) == (0, 0, 0, 1, 1)


@pytest.mark.parametrize("tl_solves,slot", [(1, 1), (2, 0), (7, 1)])
def test_first_solve_after_a_linearization_lags(ask, tl_solves, slot):
    p = plan_of(ask, tl_solves=tl_solves, tl_fresh=1)
    assert (p["slot"], p["use"], p["defer_chain"], p["must_wait_fact"], p["scale"]) == (slot, slot ^ 1, 1, 0, 0)
    assert p["cg"] == "persistent_async" and p["dc_by_cgp"] == 1 and p["basis_by_factor"] == 1
    assert plan_of(ask, tl_solves=tl_solves, tl_fresh=1, keep_S=1)["scale"] == 1
    # the launch path lags too, but issues its chain at once and keeps the scaled copy
    q = plan_of(ask, tl_solves=tl_solves, tl_fresh=1, cgp=0)
    assert (q["use"], q["defer_chain"], q["must_wait_fact"], q["scale"], q["cg"]) == (slot ^ 1, 0, 0, 1, "launch_path")


def test_retried_trial_waits_for_its_own_slot(ask):
    p = plan_of(ask, tl_solves=3, tl_fresh=0, flags_dirty=1)
    assert (p["slot"], p["use"], p["defer_chain"], p["must_wait_fact"], p["scale"]) == (1, 1, 0, 1, 1)
    assert p["prepared"] == 0 and p["zero_words"] == 1


def test_prepared_needs_the_prepared_factor(ask):
    assert plan_of(ask, prep_valid=1, prep_f=F)["prepared"] == 1
    assert plan_of(ask, prep_valid=1, prep_f=2.0)["prepared"] == 0
    assert plan_of(ask, prep_valid=0, prep_f=F)["prepared"] == 0
    assert plan_of(ask, prep_valid=1, prep_f=F, kind=1)["prepared"] == 0


def test_global_positioning(ask):
    for dirty, pts in itertools.product((0, 1), repeat=2):
        p = plan_of(ask, kind=1, flags_dirty=dirty, has_points=pts, u_late=1, rank0=0, cgp=0)
        assert p["sf"] == 1.0 and p["smin"] == -1.0e308 and p["smax"] == 1.0e308 and p["sdiag"] == 1
        assert p["zero_words"] == 1 and p["add_U_in_factor"] == 0 and p["basis_by_factor"] == 0
    b = plan_of(ask, kind=0)
    assert (b["sf"], b["smin"], b["smax"], b["sdiag"], b["zero_words"]) == (F, CMIN, CMAX, 1, 0)
    assert plan_of(ask, kind=0, rank0=0)["sdiag"] == 0
    assert plan_of(ask, kind=0, has_points=0)["zero_words"] == 1


def test_points_only_solve_runs_no_cg(ask):
    for tlon, prog, cgp in itertools.product((0, 1), repeat=3):
        p = plan_of(ask, optimize_poses=0, tlon=tlon, prog_host=prog, cgp=cgp)
        assert p["cg"] == "none" and p["dc_by_cgp"] == 0


def test_u_late(ask):
    p = plan_of(ask, u_late=1)
    assert p["sdiag"] == 0 and p["add_U_in_factor"] == 1
    p = plan_of(ask, u_late=0)
    assert p["sdiag"] == 1 and p["add_U_in_factor"] == 0


def test_no_progress_word_means_block_jacobi_chunks(ask):
    assert plan_of(ask, tlon=1, prog_host=0)["cg"] == "block_jacobi"
    assert plan_of(ask, tlon=1, prog_host=0, cgp=0)["cg"] == "block_jacobi"
    assert plan_of(ask, tlon=0, prog_host=1, cgp=0)["cg"] == "block_jacobi"
    assert plan_of(ask, async_status=0)["cg"] == "persistent"


def test_repeat_recipes(ask):
    """The seven steps in their one order: leave_persistent zero_status factorize ensure_sn basis reissue_chain
    run_cg (cgp_collective_fallback, relaunch_on_launch_path, adef2_fallback + refactor_for_cgp before they merged)."""
    q = [f"recipe {how} {bbf}" for how in ("repeat_collective", "repeat_launch_path", "repeat_additive")
         for bbf in (0, 1)]
    collective = "leave_persistent zero_status factorize ensure_sn basis reissue_chain run_cg"
    launch_path = "zero_status ensure_sn basis reissue_chain run_cg"
    assert ask(q) == [collective, collective, launch_path, launch_path,
                      "zero_status factorize basis run_cg | additive",
                      "zero_status factorize run_cg | additive | with_cams"]
    others = ("converged", "fail_step", "device_error")
    assert ask([f"recipe {how} {bbf}" for how in others for bbf in (0, 1)]) == ["invalid"] * 6


def test_cgp_flag_word(ask):
    assert ask(["bits"]) == ["1 2 4 8"]  # (k_tl_cgp tests these bits of its `oseg` argument)
    rows = list(itertools.product((0, 1), repeat=4))
    assert len(rows) == 16
    out = ask(["flags " + " ".join(map(str, r)) for r in rows])
    assert out == [str(seg * 1 + fault * 2 + brk * 4 + basis * 8) for seg, fault, brk, basis in rows]
    assert sorted(map(int, out)) == list(range(16))


def test_cg_path_code(ask):
    """include/insfm_ba.h insfm_ba_cg_info: 0 launch path / block-Jacobi, 1 persistent, 2 its fixed-order form, 3
    row-partitioned, 4 / 5 = 1 / 2 as A-DEF2."""
    rows = list(itertools.product((0, 1), (0, 64, 128), (0, 1), (0, 1)))
    out = ask(["path " + " ".join(map(str, r)) for r in rows])
    for (xpart, nb, det, adef2), got in zip(rows, out):
        want = 3 if xpart else 0 if nb == 0 else {(0, 0): 1, (1, 0): 2, (0, 1): 4, (1, 1): 5}[(det, adef2)]
        assert int(got) == want, (xpart, nb, det, adef2)
    assert set(map(int, out)) == {0, 1, 2, 3, 4, 5}
