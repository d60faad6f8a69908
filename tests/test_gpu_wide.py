"""HIP path vs an independent high-precision reference and vs the C oracle on wide-field, strongly distorted scenes
and on on-axis fisheye scenes (tests/wide_scene.py).  Needs an MI355X.

The scenes of test_gpu_parity.py / test_gpu_ragged.py start from zero distortion on a narrow field (r2 <= 0.15), where
every term of distort<M>'s Jd that carries radp, p1, p2, Np, Dp, iD2 or hp multiplies a coefficient that is exactly 0:
a kernel with `2.0 * p1 * v` for `6.0 * p1 * v`, or a wrong sign in dr[5..7], passes them.  And the oracle's distort()
mirrors the kernel's line for line, so an error both share is invisible to GPU-vs-oracle parity.  Here
 * the scenes reach r2 ~ 1.5 with every distortion coefficient moving Jp and Jc's pose columns by more than 1e-4
   (wide_scene.check_wide, conditions a-e), and the on-axis scenes put observations at r2 == 0, next to 0 and on both
   sides of fisheye_g's switch at r2 = 1e-3;
 * the yardstick is tests/ba_reference.py (forward model + torch.autograd, mpmath at 50 digits near the axis,
   numpy.longdouble sums), which shares no Jacobian code with the kernel or the oracle; tests/test_ba_reference.py
   holds the oracle to it on the CPU;
 * arrays are compared column by column (colrel; U on rows and columns, urel), so a focal column of ~0.3 is not
   hidden under a rotation column of 1e4 as it is under the global rel() norm -- which is asserted as well.
Each test first asserts the scene property it exists for.

Bounds.  The global rel() norm keeps the project's tolerances: records, V, g_p 1e-12; U, g_c 1e-10;
cost 1e-12; steps: equal PCG iterations and trials, loss 1e-10, parameters 1e-9.  The column-wise norm is stricter, so
its bound is computed in the test from the oracle alone (wide_scene.parity_bounds): the larger of the project's
tolerance and 8x the spread between the oracle's plain and fused-multiply-add builds on the same scene in the same
norm (8x: the margin test_gpu_ragged.py documents).  Measured on the CPU (x86-64, gcc), largest over the models:

  scene | Y       V       g_p     U       g_c     loss    rmse    | bounds
  wide  | 1.2e-14 9.7e-15 2.3e-14 1.7e-15 9.3e-15 8.9e-16 5.7e-16 | the project's tolerances throughout
  axis  | 8.4e-14 1.0e-13 1.8e-13 8.8e-15 1.8e-13 8.1e-15 4.3e-15 | g_p 1.4e-12 (models 5, 9: 1.1e-12 / 1.4e-12), else same

(the axis scenes linearize at the ground-truth geometry, so their residuals are the 0.5 px noise left after
cancelling projections of ~1000 px: two decades more relative rounding in r~, g_p and g_c than on the wide scenes).
The per-track figures of the axis scene get their bound the same way from the per-track spread.
On the MI355X the kernels land on the same scale as that spread (worst column, wide: Y 1.2e-14, g_p 2.3e-14; axis:
g_p 2.5e-13, g_c 3.2e-13; two LM steps: loss 9.7e-15, parameters 2.1e-13); every test prints its figures.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import ba_reference as R  # noqa: E402
import wide_scene as WS  # noqa: E402
from instantsfm_amd.engine import LM_DEFAULTS, BundleAdjuster, effective_precond  # noqa: E402
from oracle import oracle as O  # noqa: E402
from test_gpu_parity import DEV, dev, rel  # noqa: E402

REL_TOL = dict(Y=1e-12, V=1e-12, gp=1e-12, U=1e-10, gc=1e-10)


def report(tag, figures, bounds):
    """print every figure, then hold each to its bound (as test_gpu_ragged.report)"""
    print(tag, {k: f"{v:.2e}" for k, v in figures.items()})
    for k, v in figures.items():
        assert v < bounds[k], (tag, k, v, bounds[k])


@pytest.fixture(scope="module")
def scenes():
    """(family, model) -> (problem, Huber radius, reference, oracle linearization, bounds), built once per module"""
    cache = {}

    def get(family, model):
        if (family, model) not in cache:
            if family == "wide":
                prob, delta = WS.wide_problem(model), WS.HUBER_DELTA
                ref = WS.reference_linearization(prob, delta)
            else:
                prob, delta = WS.axis_problem(model), 1.0
                ref = WS.reference_linearization(prob, delta, WS.axis_special(prob))
            ora = WS.oracle_linearization(prob, delta)
            bounds, spread = WS.parity_bounds(prob, delta, ora)
            print(f"{family} model {model} oracle plain-vs-fma spread", {k: f"{v:.2e}" for k, v in spread.items()})
            cache[family, model] = prob, delta, ref, ora, bounds
        return cache[family, model]
    return get


def engine(prob, delta, **kw):
    return BundleAdjuster(prob.model, prob.uv, prob.cam_idx, prob.pt_idx, prob.pp, prob.n_cams, prob.n_points,
                          device=DEV, huber_delta=delta, **kw)


def gpu_linearization(eng, prob):
    N, P, C, D = prob.n_obs, prob.n_points, prob.n_cams, eng.D
    eng.debug_linearize(dev(prob.cams_init), dev(prob.points_init))
    got = dict(Y=eng.debug_get(0, (N, 3, D)).transpose(0, 2, 1), V=eng.debug_get(1, (P, 6)), gp=eng.debug_get(2, (P, 3)),
               U=eng.debug_get(3, (C, D, D)), gc=eng.debug_get(4, (C, D)))
    for k, a in got.items():
        assert np.all(np.isfinite(a)), k
    return got


def check_linearization(tag, got, ref, ora, bounds):
    """column-wise against the reference and against the oracle, then the global norm at the project's tolerances"""
    report(f"{tag} vs reference (columns)", WS.compare(got, ref), bounds)
    report(f"{tag} vs oracle (columns)", WS.compare(got, ora), bounds)
    report(f"{tag} vs oracle (global)", {k: rel(got[k], ora[k]) for k in REL_TOL}, REL_TOL)
    report(f"{tag} vs reference (global)", {k: rel(got[k], np.asarray(ref[k], dtype=np.float64)) for k in REL_TOL}, REL_TOL)


def check_cost(tag, eng, prob, ref, ora, bounds):
    lg, rg = eng.cost(dev(prob.cams_init), dev(prob.points_init))
    assert np.isfinite(lg) and np.isfinite(rg)
    cb = dict(loss=bounds["loss"], rmse=bounds["rmse"])
    report(f"{tag} cost vs reference", dict(loss=abs(lg - ref["loss"]) / ref["loss"], rmse=abs(rg - ref["rmse"]) / ref["rmse"]), cb)
    report(f"{tag} cost vs oracle", dict(loss=abs(lg - ora["loss"]) / ora["loss"], rmse=abs(rg - ora["rmse"]) / ora["rmse"]), cb)


def check_wide_scene(prob, ref):
    """what the wide scene is for: r2 up to 1..2, distortion away from 0 at the linearization point, both Huber
    branches (conditions a-e in full are asserted when the scene is built)"""
    _, r2 = WS.normalized(prob)
    assert 1.0 <= r2.max() <= 2.0 and np.mean(r2 > 0.5) >= 0.05
    nf = R.N_FOCAL[prob.model]
    used = np.array(WS.GT_DIST[prob.model]) != 0
    assert np.all(prob.cams_init[:, 7 + nf:][:, used] != 0)
    assert 0.005 <= ref["beyond"].mean() <= 0.05


@pytest.mark.parametrize("model", R.MODELS)
def test_wide_linearize(scenes, model):
    """k_lin_points / k_lin_cams (eval_obs<M, true>, distort<M>) at cams_init / points_init of the wide scene: the
    records Y, V, g_p, U, g_c against the longdouble reference assembly and against the oracle."""
    prob, delta, ref, ora, bounds = scenes("wide", model)
    check_wide_scene(prob, ref)
    eng = engine(prob, delta, deterministic=True)
    check_linearization(f"wide model {model}", gpu_linearization(eng, prob), ref, ora, bounds)
    eng.close()


@pytest.mark.parametrize("model", R.MODELS)
def test_wide_cost(scenes, model):
    """k_cost (eval_obs<M, false>) on the wide scene: loss and RMSE against the longdouble reference and the oracle."""
    prob, delta, ref, ora, bounds = scenes("wide", model)
    check_wide_scene(prob, ref)
    eng = engine(prob, delta)
    check_cost(f"wide model {model}", eng, prob, ref, ora, bounds)
    eng.close()


@pytest.mark.parametrize("model", (3, 4, 5, 8, 9))
def test_wide_step(scenes, model):
    """Two LM steps on the wide scene in lockstep with OracleBA.step, as test_step_parity: equal PCG iterations and
    trials, loss 1e-10, parameters 1e-9.  For these models the first check of the trial path (k_backsub_rc, k_cost,
    the retraction) away from k = 0.  FULL_OPENCV is left out of solves: its distortion columns k1..k3 and k4..k6 are
    near-dependent (cond(S) ~ 5e13, test_oracle.py::test_pcg_rounding_sensitivity_lives_in_the_near_null_space), so the
    last bits of S decide the PCG's path; test_wide_linearize and test_wide_cost cover its kernels."""
    prob, delta, ref, _, _ = scenes("wide", model)
    check_wide_scene(prob, ref)
    eng = engine(prob, delta, precond=1)
    ora = O.OracleBA(prob.model, prob.uv, prob.cam_idx, prob.pt_idx, prob.pp, prob.n_cams, prob.n_points,
                     huber_delta=delta, precond=effective_precond(1, eng.cg_info()[0]),
                     cluster_size=LM_DEFAULTS["cluster_size"])
    cg, pg = dev(prob.cams_init), dev(prob.points_init)
    co, po = prob.cams_init.copy(), prob.points_init.copy()
    for s in range(2):
        lg, st = eng.step(cg, pg)
        lo = ora.step(co, po)
        so = ora.stats()
        print(f"wide model {model} step {s}: trials {st['trials']} / {so['trials']}, PCG {st['pcg_iters']} / {so['pcg_iters']}")
        assert st["pcg_iters"] == so["pcg_iters"] and st["trials"] == so["trials"], (s, st, so)
        assert st["failed"] == so["failed"] == 0
        report(f"wide model {model} step {s}", dict(loss=abs(lg - lo) / lo, cams=rel(cg.cpu().numpy(), co),
                                                    pts=rel(pg.cpu().numpy(), po)), dict(loss=1e-10, cams=1e-9, pts=1e-9))
    nf = R.N_FOCAL[model]
    assert np.all(np.abs(co[:, 7 + nf]) > 1e-2)   # the steps stayed at strong distortion
    eng.close()


def per_track(got, exp, prob, tracks):
    """worst rel() of the Y records and of V over `tracks`, each track on its own"""
    ptr = np.searchsorted(prob.pt_idx, np.arange(prob.n_points + 1))
    worst = dict(Y=0.0, V=0.0)
    for p in tracks:
        a, b = ptr[p], ptr[p + 1]
        worst = dict(Y=max(worst["Y"], rel(got["Y"][a:b], np.asarray(exp["Y"][a:b], dtype=np.float64))),
                     V=max(worst["V"], rel(got["V"][p], np.asarray(exp["V"][p], dtype=np.float64))))
    return worst


@pytest.mark.parametrize("model", WS.AXIS_MODELS)
def test_axis_linearize_and_cost(scenes, model):
    """fisheye_g's three branches (r2 == 0, the series below 1e-3, the closed form above) on the hand-built on-axis
    scene: the comparisons of test_wide_linearize and test_wide_cost, then on their own the records and V of every
    track with an r2 == 0 observation and of every track with an observation next to the 1e-3 switch.  Everything the
    kernels return is finite (the reference's atan(r)/r is NaN at r2 == 0)."""
    prob, delta, ref, ora, bounds = scenes("axis", model)
    _, r2 = WS.normalized(prob)
    classes = WS.axis_classes(r2)
    assert all(m.sum() >= 8 for m in classes.values()), {k: int(m.sum()) for k, m in classes.items()}
    assert R.v_cond(ref["V"]).max() < 1e6 and 0 < ref["beyond"].sum() < prob.n_obs
    assert np.all(prob.cams_init[:, 7 + R.N_FOCAL[model]] != 0)
    eng = engine(prob, delta, deterministic=True)
    got = gpu_linearization(eng, prob)
    check_linearization(f"axis model {model}", got, ref, ora, bounds)
    check_cost(f"axis model {model}", eng, prob, ref, ora, bounds)
    fma = WS.oracle_linearization(prob, delta, variant="fma")
    for name in ("zero", "below", "above"):
        tracks = np.unique(prob.pt_idx[classes[name]])
        assert tracks.size >= 8
        spread = per_track(fma, ora, prob, tracks)
        tb = {k: max(1e-12, 8.0 * v) for k, v in spread.items()}
        print(f"axis model {model} {name} tracks: oracle plain-vs-fma spread", {k: f"{v:.2e}" for k, v in spread.items()})
        report(f"axis model {model} {name} tracks vs reference", per_track(got, ref, prob, tracks), tb)
        report(f"axis model {model} {name} tracks vs oracle", per_track(got, ora, prob, tracks), tb)
    eng.close()
