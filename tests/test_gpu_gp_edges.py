"""The global-positioning kernels of csrc/ba_gp.h (k_gp_lin, k_gp_lin_cams, k_gp_prep_points, k_gp_prep_cams,
k_schur_gp, k_schur<3, ORD>, k_gp_backsub, k_gp_cost) branch by branch against the 50-digit reference of
tests/gp_reference.py, on the edge scenes of tests/gp_edge_scene.py.  Needs an MI355X.

test_gpu_gp.py and test_gpu_ragged.py compare these kernels with oracle/ba_oracle.c, which restates their closed forms,
on scenes that never reach a clamp, a second round of the per-camera loops or |r| == 0, and under a global norm.  Here
 * the yardstick shares no formula with the kernels (forward residual, mpmath.diff, generic block elimination), and
   test_gp_reference.py holds the oracle to it on the CPU;
 * the scenes reach gp_hss's clamp and the diagonal clamps of k_gp_prep_points / k_gp_prep_cams from both sides, every
   Huber branch, cameras with 0, 1, 255 .. 769 observations and tracks of 1 .. 17 (asserted by gp_edge_scene.check_*);
 * every track, camera, observation and block is compared on its own scale (gp_checks.py), the W records and S~ included.
Both Schur kernels (deterministic False: k_schur_gp, True: k_schur<3, ORD>), precond 0 and 1, f = 1.001 and 1.5.

Bounds: the project's tolerances per item, widened per item to 8x the oracle's plain-versus-fma spread only where that
is larger (gp_checks.bounds).  The true residual |b - S dc| / (1e-5 |b|) at the product's pcg_tol has no derivable
bound: it is held at or below 2 x max(1, the oracle's figure) (gp_checks.oracle_true_residual).

Measured on the MI355X (worst item over both Schur modes, both preconditioners and both f):

  scene  | W       V       g'_p    b       S~      dc      dp      ds      cost    step loss | true residual
  edges  | 5.7e-16 3.2e-16 2.0e-16 8.1e-17 8.6e-16 2.4e-12 4.3e-16 9.9e-16 7.4e-17 4.8e-17   | the oracle's to 3 digits
  counts | 5.4e-16 3.4e-16 1.7e-14 8.5e-16 1.5e-15 3.7e-12 1.2e-14 2.5e-14 1.1e-16 2.5e-17   | the oracle's to 3 digits

with the oracle's PCG iteration counts throughout and no bound widened.

What the file found.  insfm_ba_debug_get(h, 0) copied N*D*3 doubles for a global-positioning handle where
insfm_ba_debug.h documents [N,4] records (a host buffer of the documented size was overrun).  And on the offset scene the
two-level PCG at pcg_tol 1e-12 (precond 1, f = 1.5) broke down from run to run in the atomic Schur mode: the coarse
basis scaled about the world origin, so its scale column nearly lined up with the translations; it now scales about a
point of the cluster (ba_twolevel.h tl_basis_entry; test_gp_reference.py keeps the case on the CPU).

The reference is cached per process (gp_edge_scene.observed / reduced); the module prints its total host time (6.5 s
for the 26 tests on the MI355X host).
"""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import gp_checks as K  # noqa: E402
import gp_edge_scene as E  # noqa: E402
import gp_reference as G  # noqa: E402
from instantsfm_amd.engine import GlobalPositioner  # noqa: E402
from test_gpu_gp import DEV, dev  # noqa: E402

SCENES = ("edges", "counts")
CHECK = dict(edges=E.check_edges, counts=E.check_counts)


@pytest.fixture(scope="module", autouse=True)
def host_time():
    t0 = time.perf_counter()
    yield
    print(f"\ntest_gpu_gp_edges.py: {time.perf_counter() - t0:.1f} s host time in all")


def engine(prob, **kw):
    return GlobalPositioner(prob.trans, prob.cam_idx, prob.pt_idx, prob.fcam, prob.sfree, prob.n_cams, prob.n_points,
                            device=DEV, huber_delta=E.DELTA, clamp_min=E.CLAMP_MIN, **kw)


def params(prob):
    return dev(prob.cams_init), dev(prob.points_init), dev(prob.scales_init)


def gpu_solve(eng, prob, f, nb):
    """linearize at the scene's initial parameters, solve for damping factor f: gp_checks' `got`, PCG iterations"""
    N, P, C = prob.n_obs, prob.n_points, prob.n_cams
    eng.debug_linearize(*params(prob))
    it = eng.debug_solve(f)
    assert eng.nnzb() == nb
    got = dict(W=G.expand_w(eng.debug_get(0, (N, 4))), V=G.sym6(eng.debug_get(1, (P, 6))), gp=eng.debug_get(2, (P, 3)),
               b=eng.debug_get(6, (C, 3)), St=eng.debug_get(5, (nb, 3, 3)), dc=eng.debug_get(7, (C, 3)),
               dp=eng.debug_get(8, (P, 3)), ds=eng.debug_ds())
    for k, a in got.items():
        assert np.all(np.isfinite(a)), k
    return got, it


def raw_buffers(eng, prob, nb):
    N, P, C = prob.n_obs, prob.n_points, prob.n_cams
    return [eng.debug_get(0, (N, 4)), eng.debug_get(1, (P, 6)), eng.debug_get(2, (P, 3)), eng.debug_get(5, (nb, 3, 3)),
            eng.debug_get(6, (C, 3)), eng.debug_get(7, (C, 3)), eng.debug_get(8, (P, 3)), eng.debug_ds()]


@pytest.mark.parametrize("name", SCENES)
def test_cost(name):
    """k_gp_cost: Huber loss and sum |r|^2 against the reference, 1e-12"""
    prob, obs = E.problem(name), E.observed(name)
    CHECK[name](prob, obs, E.reduced(name, E.F_VALUES[0]))
    eng = engine(prob)
    loss, rmse = eng.cost(*params(prob))
    assert np.isfinite(loss) and np.isfinite(rmse)
    err = K.cost_errors(loss, rmse * rmse * prob.n_obs, obs)
    print(f"{name} cost vs reference", {k: f"{v:.2e}" for k, v in err.items()})
    assert err["loss"] < K.COST_TOL and err["sq"] < K.COST_TOL
    eng.close()


@pytest.mark.parametrize("f", E.F_VALUES)
@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name", SCENES)
def test_linear_system_per_item(name, det, precond, f):
    """debug_linearize + debug_solve at pcg_tol 1e-12: the W records (expanded), V, g'_p per track, b per camera, S~
    per block, dc against the reference's direct solution, dp and ds against the reference's back-substitution of the
    GPU's own dc; ds exactly 0 on fixed scales.  Then the true residual of dc at the product's pcg_tol 1e-5."""
    prob, red = E.problem(name), E.reduced(name, f)
    CHECK[name](prob, E.observed(name), red)
    pat = K.pattern(K.oracle_for(prob))
    nb = pat[1].size
    bnd, _, it_o = K.oracle_bounds(name, precond, f)
    eng = engine(prob, deterministic=det, precond=precond, pcg_tol=1e-12)
    got, it = gpu_solve(eng, prob, f, nb)
    eng.close()
    K.report(f"{name} det {det} precond {precond} f {f} (PCG {it} / oracle {it_o})",
             K.item_errors(got, K.reference(red, pat, got["dc"])), bnd)
    assert np.all(got["ds"][prob.sfree == 0] == 0.0)
    eng = engine(prob, deterministic=det, precond=precond)
    got, it = gpu_solve(eng, prob, f, nb)
    eng.close()
    fig, fig_o = K.true_residual(red, got["dc"], 1e-5), K.oracle_true_residual(name, precond, f)
    print(f"  pcg_tol 1e-5: {it} iterations, true residual / (tol |b|) {fig:.3f} (oracle {fig_o:.3f})")
    assert fig <= 2.0 * max(1.0, fig_o), (fig, fig_o)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name", SCENES)
def test_step(name, det):
    """One LM step: the returned loss is the reference cost at the returned parameters (1e-12); fixed scales and the
    camera that sees nothing are bitwise unchanged; everything stays finite."""
    prob = E.problem(name)
    eng = engine(prob, deterministic=det)
    c, p, s = params(prob)
    loss, st = eng.step(c, p, s)
    eng.close()
    c, p, s = c.cpu().numpy(), p.cpu().numpy(), s.cpu().numpy()
    assert st["failed"] == 0 and np.isfinite(loss)
    assert np.all(np.isfinite(c)) and np.all(np.isfinite(p)) and np.all(np.isfinite(s))
    (hi, lo), _ = G.cost_at(prob, c, p, s, E.DELTA)
    err = abs((loss - hi) - lo) / hi
    print(f"{name} det {det} step: trials {st['trials']} PCG {st['pcg_iters']} loss {loss:.6e} vs reference {err:.2e}")
    assert err < K.COST_TOL
    fixed = prob.sfree == 0
    assert fixed.any() and np.array_equal(s[fixed], prob.scales_init[fixed])
    assert not np.array_equal(s[~fixed], prob.scales_init[~fixed])
    empty = np.bincount(prob.cam_idx, minlength=prob.n_cams) == 0
    assert empty.sum() == 1 and np.array_equal(c[empty], prob.cams_init[empty])
    assert not np.array_equal(c[~empty], prob.cams_init[~empty])


@pytest.mark.parametrize("name", SCENES)
def test_deterministic_handles_repeat_bitwise(name):
    prob = E.problem(name)
    nb = K.pattern(K.oracle_for(prob))[1].size
    runs = []
    for _ in range(2):
        eng = engine(prob, deterministic=True, pcg_tol=1e-12)
        gpu_solve(eng, prob, E.F_VALUES[0], nb)
        runs.append(raw_buffers(eng, prob, nb))
        eng.close()
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("det", [False, True])
def test_nan_point_fails_the_step_and_leaves_the_buffers(det):
    """INSFM_BA_ESOLVER's contract (include/insfm_ba.h), as test_solver_failure_leaves_caller_buffers_unchanged: one
    NaN point coordinate makes its point block indefinite; the step reports solver_failed and leaves the caller's
    three buffers bytewise unchanged; after a reset the next step with clean input succeeds."""
    prob = E.problem("edges")
    eng = engine(prob, deterministic=det)
    pts = prob.points_init.copy()
    pts[5, 1] = np.nan
    c, p, s = dev(prob.cams_init), dev(pts), dev(prob.scales_init)
    loss, st = eng.step(c, p, s)
    assert st["failed"] == 1, st
    assert c.cpu().numpy().tobytes() == prob.cams_init.tobytes() and p.cpu().numpy().tobytes() == pts.tobytes()
    assert s.cpu().numpy().tobytes() == prob.scales_init.tobytes()
    eng.reset()
    c, p, s = params(prob)
    loss, st = eng.step(c, p, s)
    assert st["failed"] == 0 and np.isfinite(loss), st
    (hi, lo), _ = G.cost_at(prob, c.cpu().numpy(), p.cpu().numpy(), s.cpu().numpy(), E.DELTA)
    assert abs((loss - hi) - lo) / hi < K.COST_TOL
    eng.close()
