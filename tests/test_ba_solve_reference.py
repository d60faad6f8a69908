"""tests/ba_solve_reference.py held to an all-at-once solve of the full damped system, and the C oracle
(oracle/ba_oracle.c prep_points / ora_schur / ora_pcg / backsub / ora_step's gain ratio) held to that reference item
by item on the scenes of tests/ba_edge_scene.py.  CPU only.

test_gpu_parity.py and test_gpu_ragged.py compare the HIP path's Schur build and solve with the oracle, which restates
the same closed forms and runs the same PCG to the same iteration, under one global max norm.  Here the yardstick is
the longdouble block elimination of ba_solve_reference.py (per-observation autograd rows, generic 3x3 point pivots, a
refined direct solve), the `clamps` scene reaches the diagonal clamp from both sides, and every track, camera, entry of
b, block of S~ and part of dc is compared on its own scale (ba_checks.py).  test_gpu_ba_solve.py asks the same of the
kernels with the bounds computed here.

Measured (x86-64, gcc; worst item over f = F1 / F2 and the preconditioners, pcg_tol 1e-12; dc against the direct solution):

  scene    models      | Y       V       g_p     U       g_c     b       S~      dc      dp      | widest bound
  dense    0 2 3 4 6   | 1.6e-13 1.0e-13 2.9e-13 1.9e-14 3.6e-14 6.2e-15 2.8e-14 1.5e-09 3.7e-14 | Y 1.4e-12, g_p 1.6e-12, dc 1.2e-8
  banded   2           | 1.3e-13 6.3e-14 7.9e-14 1.1e-14 2.0e-14 7.4e-15 9.0e-15 1.3e-09 3.6e-14 | Y 1.3e-12, dc 1.02e-8
  wide     4 6 9       | 7.9e-15 4.7e-15 2.5e-14 1.2e-15 8.8e-15 1.9e-15 1.2e-15 1.3e-09 6.9e-15 | dc 1.05e-8
  clamps   2 4         | 7.7e-14 3.3e-14 7.1e-13 7.0e-15 4.9e-13 3.0e-13 3.6e-11 4.4e-10 5.0e-14 | Y 1.5e-12, g_p 1.1e-12

  Widened bounds are 8x the oracle's plain-versus-fma spread on single tracks (Y, g_p: residuals of 1 px left from
  projections of 1000 px) and, for dc, 8x the oracle's own distance from the direct solution (FULL_OPENCV on the dense
  scene with precond 1 at F1: 1.5e-9; block-Jacobi on the banded scene and OPENCV on the wide scene at F1: 1.3e-9).
  On `clamps` at F1 the planted point's cancellation (30 against 30 down to a depth of 0.025) shows in g_c, b and S~,
  inside their tolerances.  True residual |b - S dc| / (1e-5 |b|) of the oracle's dc at the product's pcg_tol 1e-5:
  0.19 .. 0.99 over all cases -- the updated residual the PCG stops on is the true one.
  Gain ratio of the first step, reference vs oracle to 1e-10: clamps 1.477206 / 1.480324, uniform 1.635047, dense
  1.640297, banded 1.641097; all above tr_high = 0.5 by more than 10 %, accepted on the first trial.
  The reference against the all-at-once solve of the full damped system: dc 6e-17 .. 1e-12, dp 1e-18 .. 9e-15 (cond x 1e-19).

Mutation checks (clamps, model 4, f = F1, precond 1): one observation's contribution left out of one off-diagonal
block moves that block of S~ alone (4.6e-4) and nothing else but dc; the clamp skipped on one camera entry below
clamp_min moves only blocks of S~ in that camera's row and column (9.8e-3); the undamped V in the elimination moves b
(9.6e-2), S~ (1.8e-2) and dp (4.5e-1) and leaves Y, V, g_p, U, g_c alone.  The file takes about 50 s.
"""
import numpy as np
import pytest

import ba_checks as K
import ba_edge_scene as E
import ba_solve_reference as B
from gp_reference import LD
from oracle import oracle as O

# (scene, model, preconditioners): the cases of test_gpu_ba_solve.py; precond 2 is the A-DEF2 form of the persistent CG
CASES = ([("dense", m, (0, 1)) for m in (0, 2, 3, 4, 6)] + [("banded", 2, (0, 1, 2))]
         + [("wide", m, (0, 1)) for m in (4, 6, 9)] + [("clamps", m, (0, 1)) for m in E.CLAMP_MODELS])


@pytest.mark.parametrize("name,model", [("clamps", 2), ("clamps", 4), ("uniform", 2)])
def test_reference_block_elimination_matches_full_system(name, model):
    """Point pivots, the refined camera solve and the back-substitution against a refined dense solve of the whole
    damped (C D + 3 P) system, on the per-item scales of ba_checks.  Both solves end with a longdouble residual of
    1e-19 |b|, so they agree to cond x 1e-19, not to 1e-17: the gauge directions are held by the damping alone
    (cond ~ 1e6 at f = 1 + 1e-4).  Held to 1e-10, two decades inside the 1e-8 that dc and dp are checked to.
    model_decrease against 2 g.d - d^T H d of the reference's own undamped blocks: 1e-15 relative."""
    for f in E.F_VALUES:
        sys_ = E.system(name, model, f)
        H, g = sys_.full()
        x, resid = B.refined_solve(H, g)
        C, D = sys_.gc.shape
        dc, dp = x[:C * D].reshape(C, D), x[C * D:].reshape(-1, 3)
        back = sys_.backsub(sys_.dc)
        top = np.abs(sys_.dc)
        scale = np.concatenate([np.broadcast_to(top[:, 0:3].max(axis=1, keepdims=True), (C, 3)),
                                np.broadcast_to(top[:, 3:6].max(axis=1, keepdims=True), (C, 3)),
                                np.broadcast_to(top[:, 6:].max(axis=0, keepdims=True), (C, D - 6))], axis=1)
        e_dc = float(np.max(np.abs(dc - sys_.dc) / scale))
        e_dp = float(np.max(np.abs(dp - back["dp"]).max(axis=1) / back["dp_abs"].max(axis=1)))
        md, qd = sys_.model_decrease(sys_.dc, back["dp"]), sys_.quadratic_decrease(sys_.dc, back["dp"])
        e_md = float(abs(md - qd) / abs(md))
        print(f"{name} model {model} f {f}: full-system residual {resid:.1e}, reduced {sys_.dc_resid:.1e}; dc {e_dc:.1e} "
              f"dp {e_dp:.1e}; model decrease {float(md):.6e} vs quadratic form {e_md:.1e}")
        assert resid < 1e-17 and sys_.dc_resid < 1e-17
        assert e_dc < 1e-10 and e_dp < 1e-10 and e_md < 1e-15 and md > 0


@pytest.mark.parametrize("model", E.CLAMP_MODELS)
def test_clamps_scene_reaches_its_classes(model):
    for f in E.F_VALUES:
        print(f"clamps model {model} f {f}:", E.check_clamps(E.system("clamps", model, f)))


@pytest.mark.parametrize("name,model,preconds", CASES)
def test_oracle_matches_reference_per_item(name, model, preconds):
    """prep_points / ora_schur / ora_pcg / backsub at pcg_tol 1e-12 against the reference, every item on its own scale
    (dc: its distance from the direct solution is printed; it is what the HIP path's dc bound is made of); then the
    true residual of the oracle's dc at the product's pcg_tol 1e-5."""
    pat = K.pattern(name, model)
    for precond in preconds:
        for f in E.F_VALUES:
            sys_ = E.system(name, model, f)
            assert sys_.spd and sys_.dc_resid < 1e-17
            bnd, plain, it, own = K.oracle_bounds(name, model, precond, f)
            K.report(f"{name} model {model} precond {precond} f {f} ({it} iterations, direct residual {sys_.dc_resid:.1e}) "
                     f"oracle vs reference", own, bnd)
            fig = K.oracle_true_residual(name, model, precond, f)
            print(f"  true residual of the oracle's dc at pcg_tol 1e-5: {fig:.3f}")
            assert np.isfinite(fig)
            for k in ("b", "dc"):                                # the camera that sees nothing: exactly nothing
                empty = np.bincount(E.problem(name, model).cam_idx, minlength=sys_.gc.shape[0]) == 0
                assert np.all(plain[k][empty] == 0.0) and np.all(sys_.dc[empty] == 0)
    assert pat[1].size == K.oracle_for(name, model).nnzb()


def _flagged(name, model, f, mutate):
    sys_ = E.system(name, model, f, mutate=mutate)
    bnd, plain, _, _ = K.oracle_bounds(name, model, 1, f)
    ref = K.reference(sys_, K.pattern(name, model), plain["dc"], E.system(name, model, E.F1))
    errs = K.errors(plain, ref)
    print(f"mutation {mutate}:", {k: f"{float(v.max()):.2e}" for k, v in errs.items()})
    return sys_, errs, {k: np.flatnonzero(~(errs[k] <= bnd[k])) for k in errs}


def test_mutation_dropped_pair_is_caught_at_its_block():
    """one observation's contribution left out of one off-diagonal block: that block of S~ and no other, no other
    quantity but dc (the solution of the changed system)"""
    name, model, f = "clamps", 4, E.F1
    sys_, errs, bad = _flagged(name, model, f, ("drop_pair", 100))
    i, j = sorted(sys_.mutated)
    rp, col = K.pattern(name, model)
    block = int(rp[i] + np.flatnonzero(col[rp[i]:rp[i + 1]] == j)[0])
    assert list(bad["St"]) == [block], (bad["St"], block)
    assert errs["St"][block] > 1e-6
    for k in ("Y", "V", "gp", "U", "gc", "b", "dp"):
        assert bad[k].size == 0, (k, bad[k])
    assert bad["dc"].size > 0


def test_mutation_skipped_clamp_is_caught_in_its_camera():
    """the clamp skipped on one camera entry below clamp_min: blocks of S~ in that camera's row and column, nowhere
    else; b (which no camera diagonal enters) and the point side stay"""
    name, model, f = "clamps", 4, E.F1
    base = E.system(name, model, f)
    c, k = (int(v) for v in np.argwhere(base.below_c)[5])
    sys_, errs, bad = _flagged(name, model, f, ("no_clamp_c", (c, k)))
    rp, col = K.pattern(name, model)
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    assert bad["St"].size > 0 and errs["St"].max() > 1e-6
    assert np.all((rows[bad["St"]] == c) | (col[bad["St"]] == c)), (c, rows[bad["St"]], col[bad["St"]])
    for q in ("Y", "V", "gp", "U", "gc", "b", "dp"):
        assert bad[q].size == 0, (q, bad[q])
    assert bad["dc"].size > 0


def test_mutation_undamped_v_is_caught():
    """the undamped V in the elimination: b, S~ and dp leave their bounds almost everywhere; the linearization's own
    sums and the records (which the reference takes from the damped block's Cholesky factor) stay"""
    sys_, errs, bad = _flagged("clamps", 4, E.F1, "undamped_V")
    for k in ("b", "St", "dp", "dc"):
        assert errs[k].max() > 1e-6, (k, errs[k].max())
    assert bad["dp"].size > 0.9 * errs["dp"].size and bad["St"].size > 0.5 * errs["St"].size
    for k in ("Y", "V", "gp", "U", "gc"):
        assert bad[k].size == 0, (k, bad[k])


@pytest.mark.parametrize("name,model,precond", [("clamps", 2, 1), ("clamps", 4, 1), ("uniform", 2, 1), ("dense", 2, 1),
                                                ("banded", 2, 2)])
def test_oracle_gain_ratio_matches_reference(name, model, precond):
    """One LM step of the oracle: its gain ratio against (loss_before - loss_after) / model_decrease from the reference
    at the oracle's own dc, dp (1e-10 relative); the step is accepted on the first trial, the ratio lies at least 10 %
    away from tr_high and tr_low, and the new damping is tr_update of the reference's ratio -- what
    test_gpu_ba_solve.py::test_step_gain_and_radius relies on for these seeds."""
    prob = E.problem(name, model)
    ora = K.oracle_for(name, model, precond=precond)
    cams, pts = prob.cams_init.copy(), prob.points_init.copy()
    loss = ora.step(cams, pts)
    st = ora.stats()
    assert st["trials"] == 1 and st["failed"] == 0 and st["damp_factor"] == E.F1
    q, before, after = K.reference_quality(name, model, E.F1, cams, pts, ora.get(O.DC), ora.get(O.DP))
    print(f"{name} model {model}: gain ratio {q:.6f} (oracle {ora.quality():.6f}), loss {before:.6e} -> {after:.6e}")
    K.check_gain_margin(q, before, after)
    assert abs(loss - after) / after < K.COST_TOL
    assert abs(ora.quality() - q) / abs(q) < 1e-10
    assert st["damping"] == K.tr_update(1.0 / K.TR["tr_radius"], K.TR["tr_down"], q)[0]


def test_tr_update_restatement():
    """the three branches and both ends of the radius clamp of the Python restatement of lm_policy.h tr_update"""
    assert K.tr_update(1e-4, 1 / 16, 0.9) == (1.0 / 2e4, 1 / 16)
    assert K.tr_update(1e-4, 1 / 64, 0.1) == (1e-4, 1 / 16)
    assert K.tr_update(1e-4, 1 / 16, 1e-4) == (1.0 / (1e4 / 16), 1 / 64)
    assert K.tr_update(1e-4, 1 / 16, float("nan")) == (1.0 / (1e4 / 16), 1 / 64)
    assert K.tr_update(1e-10, 1 / 16, 0.9)[0] == 1e-10 and K.tr_update(1.0 / 2e-6, 1 / 16, 0.0)[0] == 1e6


def test_longdouble_is_wider_than_double():
    """the reference's claims rest on an 80-bit (or wider) long double"""
    assert np.finfo(LD).eps < 1e-18
