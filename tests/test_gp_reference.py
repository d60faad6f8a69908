"""tests/gp_reference.py held to the all-at-once dense solve, and the C oracle (oracle/ba_oracle.c ora_gp_*) held to
gp_reference.py item by item on the edge scenes of tests/gp_edge_scene.py.  CPU only.

The oracle restates the kernels' closed forms, so GPU-versus-oracle parity (test_gpu_gp.py, test_gpu_ragged.py) cannot
see an error both share; test_oracle_gp.py checks the oracle against a dense float64 solve on one uniform scene at
1e-5 .. 1e-7, with a global norm.  Here the yardstick is the 50-digit block elimination of gp_reference.py (forward
residual + mpmath.diff only), the scenes reach every clamp, Huber branch and loop edge (gp_edge_scene.check_*), and every
track, camera, observation and block is compared on its own scale (gp_checks.py).

Measured (x86-64, gcc; worst item over precond 0 / 1 and f = 1.001 / 1.5, pcg_tol 1e-12):

  scene  | W       V       g'_p    U'      g'_c    b       S~      dc      dp      ds      loss    sum r^2 | widened
  edges  | 5.3e-16 5.8e-16 2.0e-16 6.7e-16 1.8e-16 1.5e-16 8.2e-16 2.6e-12 2.3e-15 2.3e-15 1.9e-15 3.4e-15 | none
  counts | 9.0e-16 5.6e-16 2.3e-14 3.3e-15 2.2e-14 4.1e-15 2.9e-15 3.8e-12 1.7e-14 3.0e-14 1.5e-15 2.0e-15 | none

  (the oracle's plain-versus-fma spread stays below every tolerance on every item, so no bound is widened.)
  True residual |b - S dc| / (1e-5 |b|) of the oracle's dc at the product's pcg_tol 1e-5, per (precond, f) =
  (0, 1.001), (0, 1.5), (1, 1.001), (1, 1.5): edges 0.883 0.712 0.619 0.326, counts 0.247 0.075 0.640 0.347 -- the
  updated residual the PCG stops on is the true one.

Mutation check (test_mutated_reference_is_caught, edges, f = 1.5, precond 1): with f left out of the scale pivots the
same comparison gives W 3.3e-01, V 1.8e-01, g'_p 1.6e-01, b 8.4e-02, S~ 4.9e-01, dc 6.5e-01; with the sign of the
scale-gradient term of g'_p flipped, g'_p 7.4e-01, b 1.3e-01, dc 5.5e-01, dp 6.8e-01 while W, V and S~ stay at 5.3e-16,
5.8e-16 and 8.2e-16.  The file takes about 28 s.
"""
import numpy as np
import pytest

import gp_checks as K
import gp_edge_scene as E
import gp_reference as G
from instantsfm_amd.synth import make_gp_problem
from test_oracle_gp import dense_gp_step

SCENES = ("edges", "counts")
CHECK = dict(edges=E.check_edges, counts=E.check_counts)


@pytest.mark.parametrize("depth_frac", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("f", [1.5, 1.001])
def test_reference_block_elimination_matches_full_system(depth_frac, f):
    """Scale pivots, then point pivots, then the dense camera solve (mpmath and longdouble) against
    test_oracle_gp.dense_gp_step, which solves the whole damped system at once in float64: 1e-9 of the largest step.
    The oracle at pcg_tol 1e-13 agrees with the reference as well (1e-8, the project's bound for solve outputs)."""
    p = make_gp_problem(12, 60, track_len=5, seed=3, depth_frac=depth_frac, init="perturbed", init_sigma=0.3)
    obs = G.observations(p, p.cams_init, p.points_init, p.scales_init, 0.1)
    dc_d, dp_d, ds_d = dense_gp_step(p, p.cams_init, p.points_init, p.scales_init, f)
    got, it = K.oracle_solve(p, f, pcg_tol=1e-13, precond=1, cluster_size=4)
    for kind in ("mp", "ld"):
        red = G.reduce(obs, f, kind=kind)
        back = red.backsub(red.dc)
        fig = {}
        for name, ref, dense, ora in (("dc", red.dc, dc_d, got["dc"]), ("dp", back["dp"], dp_d, got["dp"]),
                                      ("ds", back["ds"], ds_d, got["ds"])):
            hi = G.split(ref)[0]
            scale = max(np.abs(dense).max(), 1e-300)
            fig[name] = (float(np.abs(hi - dense).max() / scale), float(np.abs(hi - ora.reshape(hi.shape)).max() / scale))
        print(f"depth_frac {depth_frac} f {f} {kind}: (vs dense, vs oracle at 1e-13, {it} iterations)", fig)
        for name, (d, o) in fig.items():
            assert d < 1e-9 and o < 1e-8, (kind, name, d, o)
        assert np.all(G.split(back["ds"])[0][p.sfree == 0] == 0.0)


@pytest.mark.parametrize("name", SCENES)
def test_scene_reaches_its_classes(name):
    """every branch class and loop boundary the scene exists for, asserted from the reference's branch report"""
    for f in E.F_VALUES:
        CHECK[name](E.problem(name), E.observed(name), E.reduced(name, f))


@pytest.mark.parametrize("name", SCENES)
def test_oracle_cost_matches_reference(name):
    prob, obs = E.problem(name), E.observed(name)
    loss, rmse = K.oracle_for(prob).cost(prob.cams_init, prob.points_init, prob.scales_init)
    err = K.cost_errors(loss, rmse * rmse * prob.n_obs, obs)
    print(f"{name} oracle cost vs reference", err)
    assert err["loss"] < K.COST_TOL and err["sq"] < K.COST_TOL


@pytest.mark.parametrize("f", E.F_VALUES)
@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("name", SCENES)
def test_oracle_matches_reference_per_item(name, precond, f):
    """ora_gp_linearize / gp_prep / ora_schur / ora_pcg / backsub / gp_scale_steps at pcg_tol 1e-12 against the reference,
    every item on its own scale; then the true residual of the oracle's dc at the product's pcg_tol 1e-5."""
    prob, red = E.problem(name), E.reduced(name, f)
    bnd, plain, it = K.oracle_bounds(name, precond, f)
    ref = K.reference(red, K.pattern(K.oracle_for(prob)), plain["dc"])
    K.report(f"{name} precond {precond} f {f} ({it} iterations) oracle vs reference", K.item_errors(plain, ref), bnd)
    assert np.all(plain["ds"][prob.sfree == 0] == 0.0)
    fig = K.oracle_true_residual(name, precond, f)
    print(f"{name} precond {precond} f {f}: true residual of the oracle's dc at pcg_tol 1e-5: {fig:.3f}")
    assert np.isfinite(fig)


@pytest.mark.parametrize("mutate,must_move,must_stay", [("hss_no_f", ("W", "V", "gp"), ()),
                                                        ("gp_sign", ("gp", "b"), ("W", "V", "St"))])
def test_mutated_reference_is_caught(mutate, must_move, must_stay):
    """The comparison once more with a deliberate change planted in the reference: f left out of the scale pivots, or
    the sign of the scale-gradient term of g'_p flipped.  The quantities the change reaches leave their bounds by many
    decades (so the comparison would catch the same slip in the oracle or the kernels); the others do not move."""
    f = 1.5
    prob, red = E.problem("edges"), E.reduced("edges", f, mutate=mutate)
    plain, _ = K.oracle_solve(prob, f, precond=1, pcg_tol=1e-12)
    ref = K.reference(red, K.pattern(K.oracle_for(prob)), plain["dc"])
    errs = K.item_errors(plain, ref)
    worst = {k: float(np.max(v)) for k, v in errs.items()}
    print(f"mutation {mutate}:", {k: f"{v:.2e}" for k, v in worst.items()})
    for k in must_move:
        assert worst[k] > 1e-3, (k, worst[k])
    for k in must_stay:
        assert worst[k] < K.TOL[k], (k, worst[k])


def test_tight_pcg_survives_summation_order_on_the_offset_scene():
    """The edges scene sits 1e3 from the origin and is a few units across.  With the two-level preconditioner's scale
    column taken about the origin (c_i) that column nearly lines up with the translation columns, the coarse matrix is
    ill-conditioned, and at pcg_tol 1e-12, precond 1, f = 1.5 the PCG broke down (`den <= 0`) in 4 of 11 summation
    orders of the Schur build (iterations 12, 13, 14 in the others) -- on the MI355X the atomic k_schur_gp failed the
    same solve from run to run.  With the column taken about the cluster's first camera (c_i - c_first, the same span)
    every order converges in the same number of iterations."""
    prob = E.problem("edges")
    its = []
    for seed in range(12):
        ora = K.oracle_for(prob, precond=1, pcg_tol=1e-12, order_seed=seed, order_mode=3 if seed else 0)
        ora.linearize(prob.cams_init, prob.points_init, prob.scales_init)
        its.append(ora.solve(1.5))
    print("PCG iterations per summation order:", its)
    assert min(its) > 0 and max(its) - min(its) <= 1, its
