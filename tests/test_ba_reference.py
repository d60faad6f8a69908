"""The independent reference (ba_reference.py: forward model + torch.autograd / mpmath, longdouble assembly) against
the C oracle on wide-field, strongly distorted scenes and on on-axis fisheye scenes (wide_scene.py).  CPU only.

The oracle's analytic Jacobians were pinned only by finite differences (test_oracle.py: 1e-5 at |k1| <= 0.06); here
they are held to the reference where every distortion term carries weight (r2 up to ~1.5, every coefficient moving
the Jacobians by more than 1e-4, scene condition d), column by column (colrel), so a small column -- a focal or a
high-order distortion column next to rotation columns of 1e4 -- is held to its own size.

Bounds, none taken from the code under test:
 * per observation (r, Jc, Jp): 1e-12, the project's tolerance for residual / Jacobian products.
   float64 rounding is 1.1e-16; the worst amplification is the residual's cancellation (projections of ~2000 px
   against a column maximum of >= 5 px: 4e-14 per rounding), and a Jacobian entry is a sum of a few dozen products.
 * sums (W, V, g_p, U, g_c, cost): wide_scene.parity_bounds -- the project's tolerance or 8x the oracle's own
   plain-vs-fma spread on the scene, whichever is larger.
"""
import numpy as np
import pytest

import ba_reference as R
import wide_scene as WS
from oracle import oracle as O

OBS_TOL = 1e-12


@pytest.fixture(scope="module")
def wide():
    cache = {}

    def get(model):
        if model not in cache:
            cache[model] = WS.wide_problem(model)
        return cache[model]
    return get


@pytest.fixture(scope="module")
def axis():
    cache = {}

    def get(model):
        if model not in cache:
            prob = WS.axis_problem(model)
            cache[model] = prob, WS.reference_linearization(prob, 1.0, WS.axis_special(prob))
        return cache[model]
    return get


def report(tag, figures, bounds):
    print(tag, {k: f"{v:.2e}" for k, v in figures.items()})
    for k, v in figures.items():
        assert v < bounds[k], (tag, k, v, bounds[k])


def check_against_oracle(tag, prob, ref, delta):
    X, cam, pp = prob.points_init[prob.pt_idx], prob.cams_init[prob.cam_idx], prob.pp[prob.cam_idx]
    r, Jc, Jp = O.evaluate(prob.model, X, cam, pp, prob.uv)
    assert np.all(np.isfinite(r)) and np.all(np.isfinite(Jc)) and np.all(np.isfinite(Jp))
    report(f"{tag} per observation", dict(r=R.colrel(r, ref["r"]), Jc=R.colrel(Jc, ref["Jc"]), Jp=R.colrel(Jp, ref["Jp"])),
           dict(r=OBS_TOL, Jc=OBS_TOL, Jp=OBS_TOL))
    ora = WS.oracle_linearization(prob, delta)
    bounds, spread = WS.parity_bounds(prob, delta, ora)
    print(f"{tag} plain-vs-fma spread", {k: f"{v:.2e}" for k, v in spread.items()})
    fig = WS.compare(ora, ref)
    fig["W"] = WS.yrel(ora["W"], ref["W"])
    report(f"{tag} sums", fig, dict(bounds, W=bounds["Y"]))


@pytest.mark.parametrize("model", R.MODELS)
def test_wide_scene_conditions(wide, model):
    """conditions (a)-(e) of wide_scene.py, every model"""
    fig = WS.check_wide(wide(model))
    print(model, fig)
    assert set(fig["coefficient_effect"]) == set(range(len(WS.GT_DIST[model]))) - ({3} if model == 5 else set())
    prob = wide(model)
    assert (prob.n_cams, prob.n_points, prob.n_obs) == (24, 600, 6000) and np.all(np.diff(prob.pt_idx) >= 0)
    nf = R.N_FOCAL[model]
    assert np.all(prob.cams_init[:, 7 + nf:][:, np.array(WS.GT_DIST[model]) != 0] != 0)  # initial distortion is not 0


@pytest.mark.parametrize("model", WS.AXIS_MODELS)
def test_axis_scene_classes(axis, model):
    """every r2 class has >= 8 observations, every track >= 2 oblique ones and a well-conditioned undamped V_p"""
    prob, ref = axis(model)
    _, r2 = WS.normalized(prob)
    counts = {k: int(m.sum()) for k, m in WS.axis_classes(r2).items()}
    cond = R.v_cond(ref["V"])
    print(model, counts, f"cond(V) <= {cond.max():.2e}")
    assert prob.n_cams <= 16 and prob.n_points <= 64 and min(counts.values()) >= 8
    assert np.bincount(prob.pt_idx[prob.cam_idx >= 8], minlength=prob.n_points).min() >= 2
    assert cond.max() < 1e6
    assert np.all(prob.cams_init[:, -1 if model != 5 else -2] != 0)
    assert 0 < ref["beyond"].sum() < prob.n_obs   # both Huber branches


def test_colrel_holds_every_column_to_its_own_size():
    """the norms themselves: an error of 1e-7 of a small column is under 1e-11 in the global max norm and 1e-7 in colrel;
    a column that is exactly zero must stay exactly zero; a NaN is never under a bound"""
    rng = np.random.default_rng(0)
    exp = rng.normal(size=(50, 2, 4)) * np.array([1e4, 1e4, 0.3, 0.0])
    got = exp.copy()
    got[7, 1, 2] += 0.3e-7
    assert np.max(np.abs(got - exp)) / np.max(np.abs(exp)) < 1e-11
    assert 1e-9 < R.colrel(got, exp) < 1e-6 and R.colrel(exp, exp) == 0.0
    assert R.colrel(got, exp, axis=1) < 1e-11      # along the other axis the large columns set the scale again
    got = exp.copy()
    got[3, 0, 3] = 1e-300
    assert R.colrel(got, exp) == float("inf")
    got[3, 0, 3] = np.nan
    assert R.colrel(got, exp) == float("inf")
    J = rng.normal(size=(30, 2, 4)) * np.array([1e4, 1e2, 0.3, 0.0])
    U = np.einsum("nad,nae->de", J, J)[None]
    got = U.copy()
    got[0, 2, 2] *= 1 + 1e-7
    assert np.max(np.abs(got - U)) / np.max(np.abs(U)) < 1e-12 and 1e-8 < R.urel(got, U) < 1e-6
    got = U.copy()
    got[0, 0, 3] = 1e-300
    assert R.urel(got, U) == float("inf") and R.urel(U, U) == 0.0


def test_y_from_whitens_by_the_damped_point_block():
    """Y_o R_p^T = W_o with R_p R_p^T = V_p, its diagonal clamped to [clamp_min, clamp_max] and multiplied by f"""
    rng = np.random.default_rng(1)
    Jp = rng.normal(size=(12, 2, 3))
    Jp[8:] *= 1e-4                       # point 2: a diagonal below clamp_min
    pt_idx = np.repeat(np.arange(3), 4)
    W = rng.normal(size=(12, 7, 3))
    full = np.zeros((3, 3, 3))
    np.add.at(full, pt_idx, np.einsum("naj,nak->njk", Jp, Jp))
    V = np.stack([full[:, 0, 0], full[:, 0, 1], full[:, 0, 2], full[:, 1, 1], full[:, 1, 2], full[:, 2, 2]], axis=1)
    f = 1.0 + 1e-4
    Y = R.y_from(W, V, pt_idx, f, clamp_min=1e-6)
    assert full[2, 0, 0] < 1e-6 < full[0, 0, 0]
    for p in range(3):
        damped = full[p].copy()
        damped[np.diag_indices(3)] = np.clip(np.diag(damped), 1e-6, 1e32) * f
        for o in np.flatnonzero(pt_idx == p):
            # Y = W R^-T  =>  Y Y^T = W (R R^T)^-1 W^T
            assert np.allclose(Y[o] @ Y[o].T, W[o] @ np.linalg.inv(damped) @ W[o].T, rtol=1e-9, atol=0)


def test_projection_restatement_matches_projection_ref():
    """project() against oracle/projection_ref.reproject on the wide scenes: the same forward model"""
    from oracle.projection_ref import reproject
    for model in R.MODELS:
        prob = WS.wide_problem(model)
        args = (prob.points_init[prob.pt_idx], prob.cams_init[prob.cam_idx], prob.pp[prob.cam_idx])
        assert R.colrel(R.project(model, *args).numpy(), reproject(model, *args)) < 1e-14


def test_autograd_and_mpmath_paths_agree():
    """where both paths work (r2 ~ 1e-3 .. 1, 16 wide-field observations) they give the same Jacobians"""
    for model in (4, 5, 6):
        prob = WS.wide_problem(model)
        sel = np.arange(0, prob.n_obs, prob.n_obs // 16)[:16]
        args = tuple(a[sel] for a in (prob.points_init[prob.pt_idx], prob.cams_init[prob.cam_idx],
                                      prob.pp[prob.cam_idx], prob.uv))
        ra, Jca, Jpa = R.residual_jacobians(model, *args)
        rm, Jcm, Jpm = R.mp_residual_jacobians(model, *args)
        report(f"model {model} autograd vs mpmath", dict(r=R.colrel(ra, rm), Jc=R.colrel(Jca, Jcm), Jp=R.colrel(Jpa, Jpm)),
               dict(r=OBS_TOL, Jc=OBS_TOL, Jp=OBS_TOL))


@pytest.mark.parametrize("model", R.MODELS)
def test_oracle_matches_reference_wide(wide, model):
    """O.evaluate and OracleBA.linearize / .cost against the reference on the wide scene"""
    prob = wide(model)
    ref = WS.reference_linearization(prob, WS.HUBER_DELTA)
    assert 1.0 <= WS.normalized(prob)[1].max() <= 2.0
    assert 0.005 <= ref["beyond"].mean() <= 0.05
    check_against_oracle(f"wide model {model}", prob, ref, WS.HUBER_DELTA)


@pytest.mark.parametrize("model", WS.AXIS_MODELS)
def test_oracle_matches_reference_axis(axis, model):
    """the same on the on-axis scene, the reference's class observations (r2 == 0, next to 0, next to the 1e-3 switch
    of fisheye_g) evaluated in mpmath"""
    prob, ref = axis(model)
    assert WS.axis_special(prob).sum() >= 40
    for k in ("r", "Jc", "Jp", "W", "V", "gp", "U", "gc"):
        assert np.all(np.isfinite(np.asarray(ref[k], dtype=np.float64))), k
    check_against_oracle(f"axis model {model}", prob, ref, 1.0)
    # the class observations on their own, so that the oblique ones cannot set the scale
    sel = WS.axis_special(prob)
    X, cam, pp = prob.points_init[prob.pt_idx][sel], prob.cams_init[prob.cam_idx][sel], prob.pp[prob.cam_idx][sel]
    r, Jc, Jp = O.evaluate(model, X, cam, pp, prob.uv[sel])
    report(f"axis model {model} class observations",
           dict(r=R.colrel(r, ref["r"][sel]), Jc=R.colrel(Jc, ref["Jc"][sel]), Jp=R.colrel(Jp, ref["Jp"][sel])),
           dict(r=OBS_TOL, Jc=OBS_TOL, Jp=OBS_TOL))
