"""The middle of a bundle-adjustment trial on the HIP path -- point preparation, k_schur (FIRST, RETRY, atomic, ORD,
rows split into chunks), k_cg_factor / k_cg_factor_basis / k_cg_scale, the CG paths (launch-path block-Jacobi and
two-level, k_tl_cgp paths 1, 2, 4, 5), k_cg_finish, k_backsub_rc with its gain parts and update_cams_block -- item by
item against the longdouble reference of tests/ba_solve_reference.py.  Needs an MI355X.

test_gpu_parity.py::test_solve_parity and test_gpu_ragged.py::test_ragged_solve_parity compare these stages with
oracle/ba_oracle.c, which restates the same closed forms and runs the same PCG to the same iteration, under one global
max norm.  Here
 * the yardstick shares no formula with the kernels (per-observation autograd rows, generic 3x3 point pivots over the
   dense system's blocks, a refined direct solve; no Y Y^T form), and test_ba_solve_reference.py holds the oracle to it;
 * every track, camera, entry of b, block of S~ and part of dc is held to its own scale (ba_checks.py), so the focal
   and distortion entries of b and dc are not hidden under the pose entries;
 * dc (pcg_tol 1e-12) is compared with the DIRECT solution, and the true residual |b - S dc| / (1e-5 |b|) of the
   product's solve is taken with the reference's S and b;
 * the `clamps` scene reaches the diagonal clamp from both sides on cameras and points (ba_edge_scene.check_clamps);
 * one step()'s loss, gain ratio and new damping are checked against the reference's model decrease
   sum |r~|^2 - |r~ + J~ d|^2, which names no U, V or g.
On the k_tl_cgp paths debug_get(5) hands out the scaled S~ as on the launch path (the handle forms the row-contiguous
copy on request), so S~ is compared there as well.

Bounds: the project's tolerances per item (records, V, g_p 1e-12; U, g_c, b 1e-10; S~ 1e-9; dp 1e-8), widened per item
to 8x the oracle's plain-versus-fma spread only where that is larger; dc: max(1e-8, 8x the oracle's own distance from
the direct solution on that item); true residual: at most 2 x max(1, the oracle's figure); PCG iterations at the
product's pcg_tol equal to the oracle's on the launch path (FULL_OPENCV on the wide scene excepted: its near-dependent
distortion columns, test_gpu_wide.py), within one on k_tl_cgp (as test_ragged_banded_solve_and_step).

The oracle's figures on the CPU (test_ba_solve_reference.py; worst item over f = F1 / F2 and the preconditioners) -- the
scale the kernels are expected on, as in test_gpu_wide.py and test_gpu_gp_edges.py:

  scene    models      | Y       V       g_p     U       g_c     b       S~      dc*     dp      | true residual
  dense    0 2 3 4 6   | 1.6e-13 1.0e-13 2.9e-13 1.9e-14 3.6e-14 6.2e-15 2.8e-14 1.5e-09 3.7e-14 | 0.37 .. 0.97
  banded   2           | 1.3e-13 6.3e-14 7.9e-14 1.1e-14 2.0e-14 7.4e-15 9.0e-15 1.3e-09 3.6e-14 | 0.36 .. 0.99
  wide     4 6 9       | 7.9e-15 4.7e-15 2.5e-14 1.2e-15 8.8e-15 1.9e-15 1.2e-15 1.3e-09 6.9e-15 | 0.50 .. 0.94
  clamps   2 4         | 7.7e-14 3.3e-14 7.1e-13 7.0e-15 4.9e-13 3.0e-13 3.6e-11 4.4e-10 5.0e-14 | 0.19 .. 0.80
  (dc*: dc against the direct solution; step loss against the reference cost: 1.6e-16 .. 2.1e-15)

Widened bounds (all from the oracle alone): Y per track up to 1.5e-12 and g_p per track up to 1.6e-12 on single tracks
(8x the plain-versus-fma spread: residuals of 1 px left from projections of 1000 px); dc up to 1.2e-8 (dense model 6,
precond 1, F1), 1.02e-8 (banded, precond 0, F1) and 1.05e-8 (wide model 4 / 6, F1): 8x the oracle's own distance from
the direct solution.  Everything else stands at the project's tolerances.

Measured on the MI355X (worst item over both Schur modes, the preconditioners and both f; 40 tests, 25 s host time):

  scene    | Y       V       g_p     U       g_c     b       S~      dc*     dp      step loss | true residual
  dense    | 1.8e-13 1.0e-13 2.9e-13 2.1e-14 5.7e-14 1.1e-14 1.3e-14 2.1e-09 6.5e-14 1.3e-15   | the oracle's to 3 digits
  banded   | 1.6e-13 1.2e-13 1.2e-13 2.8e-14 2.8e-14 9.4e-15 3.7e-15 5.1e-10 5.1e-14 2.5e-15   | the oracle's to 3 digits
  wide     | 1.6e-14 6.6e-15 3.8e-14 2.1e-15 1.7e-14 4.0e-15 9.8e-16 3.8e-10 1.1e-14 -         | the oracle's to 3 digits
  clamps   | 1.8e-13 5.2e-14 7.1e-13 1.1e-14 4.9e-13 8.1e-15 1.0e-13 3.4e-10 3.5e-14 1.5e-15   | the oracle's to 3 digits

with the oracle's PCG iteration counts at pcg_tol 1e-5 in every case (k_tl_cgp included), points-only dp at 1.1e-13
(dense) and 6.4e-14 (clamps), the gain ratios of the CPU table and stats["damping"] = 5e-5 = tr_update of them.  No item
came near a widened bound (Y 1.8e-13 under 1.2e-12 .. 1.5e-12; dc 2.1e-9 under 1e-8), and on `clamps` the kernels' b and
S~ (8.1e-15, 1.0e-13) sit below the oracle's (3.0e-13, 3.6e-11).  What the file found: nothing -- no defect in the Schur
build, the CG paths or the back-substitution on these scenes.

The reference is cached per process (ba_edge_scene.system keeps the last few; the cases walk scene by scene and model by
model, F1 then F2); the module prints its worst figures per scene and its total host time.
"""
import functools
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import ba_checks as K  # noqa: E402
import ba_edge_scene as E  # noqa: E402
import ba_solve_reference as B  # noqa: E402
from instantsfm_amd import _capi  # noqa: E402
from instantsfm_amd.engine import CGP_PATHS, BundleAdjuster, effective_precond  # noqa: E402
from test_create_plan import LIN_THREADS  # noqa: E402
from test_gpu_parity import DEV, dev  # noqa: E402
from test_gpu_ragged import check_dense_scene, check_split_rows  # noqa: E402

# (scene, model, deterministic, precond), scene by scene and model by model (the reference is cached per scene, model, f)
CASES = ([("dense", m, det, pc) for m in (0, 2, 3, 4, 6) for det in (False, True) for pc in ((1, 0) if m == 2 else (1,))]
         + [("banded", 2, det, pc) for det in (False, True) for pc in (1, 2)]
         + [("wide", m, False, 1) for m in (4, 6, 9)]
         + [("clamps", m, det, pc) for m in E.CLAMP_MODELS for det in (False, True) for pc in (0, 1)])
BANDED_PATH = {(False, 1): 1, (True, 1): 2, (False, 2): 4, (True, 2): 5}
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def host_time():
    t0 = time.perf_counter()
    yield
    for name, fig in WORST.items():
        print(f"\n{name} worst per item:", {k: f"{v:.1e}" for k, v in fig.items()})
    print(f"\ntest_gpu_ba_solve.py: {time.perf_counter() - t0:.1f} s host time in all")


def stop_on_device_error(test):
    """a HIP error ends the session: nothing more is started on a device that has reported one"""
    @functools.wraps(test)
    def run(*args, **kw):
        try:
            return test(*args, **kw)
        except RuntimeError as e:
            if getattr(e, "code", None) == _capi.INSFM_BA_EHIP or "HIP error" in str(e) or "illegal memory" in str(e):
                pytest.exit(f"device error in {test.__name__}{args}: {e}", returncode=3)
            raise
    return run


def note(name, figures):
    w = WORST.setdefault(name, {})
    for k, v in figures.items():
        w[k] = max(w.get(k, 0.0), float(v))


def engine(name, model, **kw):
    p, s = E.problem(name, model), E.settings(name, model)
    return BundleAdjuster(p.model, p.uv, p.cam_idx, p.pt_idx, p.pp, p.n_cams, p.n_points, device=DEV, **dict(s, **kw))


def check_scene(name, model, eng, det):
    """the property each scene is here for, and the CG path the handle runs"""
    prob, path = E.problem(name, model), eng.cg_info()[0]
    if name == "dense":
        check_dense_scene(prob, 2 * LIN_THREADS if model == 2 else LIN_THREADS)
        check_split_rows(prob, K.oracle_for(name, model), eng.D, det)
        assert path == 0, eng.cg_info()
    elif name == "clamps":
        E.check_clamps(E.system(name, model, E.F1))
    elif name == "wide":
        assert path == 0, eng.cg_info()
    return path


def linearized(eng, prob):
    N, P, C, D = prob.n_obs, prob.n_points, prob.n_cams, eng.D
    eng.debug_linearize(dev(prob.cams_init), dev(prob.points_init))
    return dict(Y=eng.debug_get(0, (N, 3, D)).transpose(0, 2, 1), V=eng.debug_get(1, (P, 6)), gp=eng.debug_get(2, (P, 3)),
                U=eng.debug_get(3, (C, D, D)), gc=eng.debug_get(4, (C, D)))


def solved(eng, prob, f, nb):
    P, C, D = prob.n_points, prob.n_cams, eng.D
    it = eng.debug_solve(f)
    assert eng.nnzb() == nb
    got = dict(b=eng.debug_get(6, (C, D)), St=eng.debug_get(5, (nb, D, D)), dc=eng.debug_get(7, (C, D)),
               dp=eng.debug_get(8, (P, 3)))
    for k, a in got.items():
        assert np.all(np.isfinite(a)), k
    return got, it


@pytest.mark.parametrize("name,model,det,precond", CASES)
@stop_on_device_error
def test_linear_system_per_item(name, model, det, precond):
    """debug_linearize at the scene's initial parameters, debug_solve(F1) and then debug_solve(F2) on the same
    linearization (k_schur's RETRY form) at pcg_tol 1e-12: Y, V, g_p per track, U per camera, g_c and b per entry, S~
    per block, dc per camera part and intrinsics column against the direct solution, dp per track against the
    reference's back-substitution of the GPU's own dc.  Then the same two solves at the product's pcg_tol 1e-5: the
    true residual with the reference's S and b, and the PCG iteration count against the oracle's."""
    prob, pat = E.problem(name, model), K.pattern(name, model)
    nb = pat[1].size
    eng = engine(name, model, deterministic=det, precond=precond, pcg_tol=1e-12)
    path = check_scene(name, model, eng, det)
    if name == "banded":
        assert path == BANDED_PATH[det, precond], eng.cg_info()
    pc = effective_precond(precond, path)
    got = linearized(eng, prob)
    records = E.system(name, model, E.F1)
    for f in E.F_VALUES:
        sys_ = E.system(name, model, f)
        bnd, _, it_o, own = K.oracle_bounds(name, model, pc, f)
        sol, it = solved(eng, prob, f, nb)
        errs = K.errors(dict(got if f == E.F1 else {}, **sol), K.reference(sys_, pat, sol["dc"], records))
        note(name, K.report(f"{name} model {model} det {det} precond {precond} path {path} f {f} (PCG {it} / oracle {it_o}; "
                            f"oracle dc vs direct {own['dc'].max():.1e})", errs, bnd))
        empty = np.bincount(prob.cam_idx, minlength=prob.n_cams) == 0
        assert np.all(sol["b"][empty] == 0.0) and np.all(sol["dc"][empty] == 0.0)
    eng.close()
    eng = engine(name, model, deterministic=det, precond=precond)
    eng.debug_linearize(dev(prob.cams_init), dev(prob.points_init))
    for f in E.F_VALUES:
        sol, it = solved(eng, prob, f, nb)
        fig = K.true_residual(E.system(name, model, f), sol["dc"], 1e-5)
        fig_o, it_o = K.oracle_at_tolerance(name, model, pc, f)
        print(f"  pcg_tol 1e-5 f {f}: {it} iterations (oracle {it_o}), true residual / (tol |b|) {fig:.3f} (oracle {fig_o:.3f})")
        note(name, dict(true_residual=fig))
        assert fig <= 2.0 * max(1.0, fig_o), (fig, fig_o)
        if path in CGP_PATHS:
            assert abs(it - it_o) <= 1, (it, it_o)
        elif not (name == "wide" and model == 6):
            assert it == it_o, (it, it_o)
    eng.close()


@pytest.mark.parametrize("name,model", [("dense", 2)] + [("clamps", m) for m in E.CLAMP_MODELS])
@stop_on_device_error
def test_points_only(name, model):
    """optimize_poses=False: dp per track is the reference's V_d^-1 g_p (1e-8 on the track's sum of |terms|), for F1 and
    the retried F2; one step() returns the reference cost at the returned points and leaves the cameras bitwise."""
    prob = E.problem(name, model)
    eng = engine(name, model, optimize_poses=False)
    eng.debug_linearize(dev(prob.cams_init), dev(prob.points_init))
    for f in E.F_VALUES:
        eng.debug_solve(f)
        dp = eng.debug_get(8, (prob.n_points, 3))
        back = E.system(name, model, f).backsub(None)
        hi, lo = B.hi_lo(back["dp"])
        err = (np.abs((dp.astype(B.LD) - hi) - lo).max(axis=1) / back["dp_abs"].max(axis=1)).astype(np.float64)
        print(f"{name} model {model} points only f {f}: dp per track {err.max():.2e}")
        note(name, dict(dp_points_only=err.max()))
        assert np.all(err <= K.TOL["dp"]), (np.flatnonzero(err > K.TOL["dp"])[:8], err.max())
    eng.close()
    eng = engine(name, model, optimize_poses=False)
    c, p = dev(prob.cams_init), dev(prob.points_init)
    loss, st = eng.step(c, p)
    eng.close()
    assert st["failed"] == 0 and c.cpu().numpy().tobytes() == prob.cams_init.tobytes()
    assert not np.array_equal(p.cpu().numpy(), prob.points_init)
    ref = float(B.cost(prob, prob.cams_init, p.cpu().numpy(), E.settings(name, model)["huber_delta"]))
    print(f"  step loss vs reference {abs(loss - ref) / ref:.2e}")
    assert abs(loss - ref) / ref < K.COST_TOL


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name,model", [("clamps", 2), ("clamps", 4), ("dense", 2), ("banded", 2)])
@stop_on_device_error
def test_step_gain_and_radius(name, model, det):
    """One step() with the product defaults: the returned loss is the reference cost at the returned parameters (1e-12);
    the step (dc, dp) of debug_get(7) / (8) is the parameter change (points and intrinsics, to the rounding of the
    update); stats["damping"] is lm_policy.h's tr_update of the gain ratio (loss_before - loss) / model_decrease(dc, dp)
    taken from the reference.  The ratio is at least 10 % away from tr_high and tr_low and the step is accepted on the
    first trial (test_ba_solve_reference.py shows the same from the oracle on the CPU)."""
    prob = E.problem(name, model)
    C, P = prob.n_cams, prob.n_points
    eng = engine(name, model, deterministic=det)
    c, p = dev(prob.cams_init), dev(prob.points_init)
    loss, st = eng.step(c, p)
    dc, dp = eng.debug_get(7, (C, eng.D)), eng.debug_get(8, (P, 3))
    eng.close()
    cams, pts = c.cpu().numpy(), p.cpu().numpy()
    assert st["trials"] == 1 and st["failed"] == 0 and st["rejects"] == 0, st
    eps = np.finfo(np.float64).eps
    assert np.all(np.abs((pts - prob.points_init) - dp) <= 2 * eps * np.maximum(np.abs(pts), np.abs(prob.points_init)))
    assert np.all(np.abs((cams[:, 7:] - prob.cams_init[:, 7:]) - dc[:, 6:])
                  <= 2 * eps * np.maximum(np.abs(cams[:, 7:]), np.abs(prob.cams_init[:, 7:])))
    q, before, after = K.reference_quality(name, model, E.F1, cams, pts, dc, dp)
    K.check_gain_margin(q, before, after)
    e_loss, e_before = abs(loss - after) / after, abs(st["loss_before"] - before) / before
    damping = K.tr_update(1.0 / K.TR["tr_radius"], K.TR["tr_down"], q)[0]
    print(f"{name} model {model} det {det}: PCG {st['pcg_iters']}, gain ratio {q:.6f}, loss vs reference {e_loss:.2e}, "
          f"loss before {e_before:.2e}, damping {st['damping']:.6e} (tr_update {damping:.6e})")
    note(name, dict(step_loss=e_loss))
    assert e_loss < K.COST_TOL and e_before < K.COST_TOL
    assert st["damping"] == damping


@pytest.mark.parametrize("model", E.CLAMP_MODELS)
@stop_on_device_error
def test_deterministic_repeat_bitwise(model):
    """two deterministic handles: the same bytes for S~, b, dc and dp, first trial and retried trial"""
    prob = E.problem("clamps", model)
    nb = K.pattern("clamps", model)[1].size
    runs = []
    for _ in range(2):
        eng = engine("clamps", model, deterministic=True, precond=1, pcg_tol=1e-12)
        eng.debug_linearize(dev(prob.cams_init), dev(prob.points_init))
        out = []
        for f in E.F_VALUES:
            sol, _ = solved(eng, prob, f, nb)
            out += [sol[k] for k in ("St", "b", "dc", "dp")]
        runs.append(out)
        eng.close()
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
