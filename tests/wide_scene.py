"""Wide-field, strongly distorted BA scenes and hand-built on-axis fisheye scenes -- what synth.make_problem (ring of
30 around a ball of 8: r2 <= 0.15; initial distortion 0) never produces.  Test helper only; used by
test_ba_reference.py and test_gpu_wide.py.

wide_problem(model, seed): make_problem's recipe (ring cameras looking at the origin, points uniform in a ball, 10
observations per track, 0.5 px noise, 1 % outliers of 5..20 px per coordinate, track-major order, the same initial
perturbations of poses, points and focals), 24 cameras and 600 points, with
 * the ring at RING = 10.5 around the ball of BALL = 8, so the largest r2 is between 1 and 2,
 * strong ground-truth distortion (GT_DIST) and initial distortion = ground truth * (1 + N(0, 0.03^2)), not 0.
The tests linearize at the initial values with Huber radius HUBER_DELTA = 30 px: the initial perturbations put the
typical residual near 8 px, and the 0.5 px noise alone leaves exp(-2) = 13.5 % of the residuals beyond the product's
default radius of 1 px, so no radius of 1 px can put "a few per cent" of the observations in the outer branch.
check_wide() asserts, from the independent reference (ba_reference.py) alone:
 a. every observation has camera-frame depth > 1;
 b. max r2 in [1, 2] and at least 5 % of the observations at r2 > 0.5;
 c. FULL_OPENCV's denominator 1 + k4 r2 + k5 r4 + k6 r6 > 0.5 everywhere;
 d. every distortion coefficient matters: with coefficient j alone set to 0 the reference's Jp, and the pose columns of
    Jc, move by more than 1e-4 in colrel (OPENCV_FISHEYE's k4, which the model ignores, excepted);
 e. between 0.5 % and 5 % of the observations lie beyond the Huber radius, so both weight branches run.

axis_problem(model), fisheye models 5, 8, 9: 8 cameras with q = (0, 0, 0, 1) and t = (-X_x, -X_y, t_z) for a point
X each, whose observation of X has p_x = p_y = 0 exactly (r2 == 0 bit for bit), four more points per such camera
offset so that r2 falls in (0, 1e-10], [1e-7, 1e-5], [0.9e-3, 1e-3) and [1e-3, 1.1e-3] (fisheye_g switches from the
series to the closed form at 1e-3), and 6 oblique cameras that see every point.  Poses and points are exact: the
initial values are the constructed ones, only the observations carry noise.
"""
import numpy as np

import ba_reference as R
from instantsfm_amd.scene.defs import num_intrinsics
from instantsfm_amd.synth import (BAProblem, _FOCAL_COUNT, _project, _quat_from_matrix, _quat_from_rotvec, _quat_mul)

N_CAMS, N_POINTS, TRACK_LEN = 24, 600, 10
RING, BALL = 10.5, 8.0
HUBER_DELTA = 30.0
FOCALS = {1: [1000.0], 2: [1000.0, 1010.0]}
# k1 k2 p1 p2 k3 k4 k5 k6 (models 2, 3, 4, 6 take prefixes); the fisheye models have their own
_OPENCV = [-0.12, 0.03, 2e-3, -3e-3, 4e-3, 0.05, -0.02, 3e-3]
GT_DIST = {0: [], 1: [], 2: _OPENCV[:1], 3: _OPENCV[:2], 4: _OPENCV[:4], 6: _OPENCV[:8],
           5: [-0.05, 0.01, -2e-3, 0.0], 8: [-0.05], 9: [-0.05, 0.01]}
AXIS_MODELS = (5, 8, 9)
# the r2 each class point is placed at: zero {0}, tiny (0,1e-10], small [1e-7,1e-5], below [.9e-3,1e-3), above [1e-3,1.1e-3]
_AXIS_R2 = (0.0, 2.5e-11, 1e-6, 0.95e-3, 1.05e-3)


def gt_intrinsics(model):
    return np.array(FOCALS[_FOCAL_COUNT[model]] + GT_DIST[model])


def _look_at(centers, target=np.zeros(3)):
    """world-to-camera rotations of cameras at `centers` looking at `target`, z up (make_problem's frame)"""
    zax = target - centers
    zax = zax / np.linalg.norm(zax, axis=1, keepdims=True)
    xax = np.cross(zax, np.array([0.0, 0.0, 1.0]))
    xax /= np.linalg.norm(xax, axis=1, keepdims=True)
    return np.stack([xax, np.cross(zax, xax), zax], axis=1)


def wide_problem(model, seed=0):
    rng = np.random.default_rng([seed, 21])
    C, P, L = N_CAMS, N_POINTS, TRACK_LEN
    ni, nf = num_intrinsics(model), _FOCAL_COUNT[model]
    ang = 2 * np.pi * np.arange(C) / C
    centers = np.stack([RING * np.cos(ang), RING * np.sin(ang), rng.uniform(-2, 2, C)], axis=1)
    Rw2c = _look_at(centers)
    t = -np.einsum('cij,cj->ci', Rw2c, centers)
    q = _quat_from_matrix(Rw2c)
    intr = np.tile(gt_intrinsics(model), (C, 1))
    cams_gt = np.concatenate([t, q, intr], axis=1)
    pp = np.tile(np.array([1000.0, 750.0]), (C, 1))
    d = rng.normal(size=(P, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    points_gt = d * (BALL * rng.uniform(0, 1, (P, 1)) ** (1.0 / 3.0))
    cams_of = np.sort(np.argsort(rng.uniform(size=(P, C)), axis=1)[:, :L], axis=1)
    cam_idx = cams_of.reshape(-1).astype(np.int32)
    pt_idx = np.repeat(np.arange(P, dtype=np.int32), L)
    uv, _ = _project(model, points_gt[pt_idx], cams_gt[cam_idx], pp[cam_idx])
    uv = uv + rng.normal(0, 0.5, uv.shape)
    n_out = int(round(0.01 * uv.shape[0]))
    which = rng.choice(uv.shape[0], n_out, replace=False)
    uv[which] += rng.choice([-1.0, 1.0], (n_out, 2)) * rng.uniform(5, 20, (n_out, 2))
    q0 = _quat_mul(_quat_from_rotvec(rng.normal(0, 0.002, (C, 3))), q)
    t0 = t + rng.normal(0, 0.05, (C, 3))
    intr0 = intr.copy()
    intr0[:, :nf] *= 1 + rng.normal(0, 0.005, (C, 1))
    intr0[:, nf:] *= 1 + rng.normal(0, 0.03, (C, ni - nf))
    cams_init = np.concatenate([t0, q0, intr0], axis=1)
    points_init = points_gt + rng.normal(0, 0.05, (P, 3))
    prob = BAProblem(model, cams_gt, cams_init, pp, points_gt, points_init, np.ascontiguousarray(uv), cam_idx, pt_idx)
    check_wide(prob)
    return prob


def normalized(prob, cams=None, pts=None):
    """(depth [N], r2 [N]) of every observation at (cams, pts), default the initial values; plain float64 arithmetic
    in the kernel's operation order, so r2 == 0 here is r2 == 0 there"""
    cams = prob.cams_init if cams is None else cams
    pts = prob.points_init if pts is None else pts
    c, X = cams[prob.cam_idx], pts[prob.pt_idx]
    qv, w = c[:, 3:6], c[:, 6:7]
    c1 = np.cross(qv, X)
    pc = X + 2.0 * (w * c1 + np.cross(qv, c1)) + c[:, :3]
    u, v = pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2]
    return pc[:, 2], u * u + v * v


def wide_figures(prob, coefficients=True):
    """the figures conditions (a)-(e) are about, at the initial values, from the reference alone"""
    depth, r2 = normalized(prob)
    model, nf = prob.model, _FOCAL_COUNT[prob.model]
    fig = dict(min_depth=float(depth.min()), max_r2=float(r2.max()), frac_r2_half=float(np.mean(r2 > 0.5)))
    if model == 6:
        k4, k5, k6 = (prob.cams_init[prob.cam_idx, 7 + nf + j] for j in (5, 6, 7))
        fig["min_denominator"] = float(np.min(1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3))
    args = (prob.points_init[prob.pt_idx], prob.cams_init[prob.cam_idx], prob.pp[prob.cam_idx], prob.uv)
    r, Jc, Jp = R.residual_jacobians(model, *args)
    fig["frac_beyond"] = float(np.mean(np.sqrt(np.sum(r * r, axis=1)) >= HUBER_DELTA))
    if coefficients:
        fig["coefficient_effect"] = {}
        for j in range(len(GT_DIST[model])):
            if model == 5 and j == 3:
                continue
            cam0 = args[1].copy()
            cam0[:, 7 + nf + j] = 0.0
            _, Jc0, Jp0 = R.residual_jacobians(model, args[0], cam0, args[2], args[3])
            fig["coefficient_effect"][j] = (R.colrel(Jp0, Jp), R.colrel(Jc0[:, :, :6], Jc[:, :, :6]))
    return fig


def check_wide(prob, coefficients=True):
    fig = wide_figures(prob, coefficients)
    assert fig["min_depth"] > 1.0, fig                                            # a
    assert 1.0 <= fig["max_r2"] <= 2.0 and fig["frac_r2_half"] >= 0.05, fig        # b
    assert fig.get("min_denominator", 1.0) > 0.5, fig                              # c
    for j, (ep, ec) in fig.get("coefficient_effect", {}).items():                  # d
        assert ep > 1e-4 and ec > 1e-4, (prob.model, j, ep, ec)
    assert 0.005 <= fig["frac_beyond"] <= 0.05, fig                                # e
    return fig


def axis_classes(r2):
    """class name -> mask over observations"""
    return dict(zero=r2 == 0.0, tiny=(r2 > 0) & (r2 <= 1e-10), small=(r2 >= 1e-7) & (r2 <= 1e-5),
                below=(r2 >= 0.9e-3) & (r2 < 1e-3), above=(r2 >= 1e-3) & (r2 <= 1.1e-3))


def axis_problem(model, seed=0):
    assert model in AXIS_MODELS
    rng = np.random.default_rng([seed, 22])
    K, n_obl = 8, 6
    C = K + n_obl
    # targets X_j: a loose cluster around the origin; axis camera j looks down +z at X_j from depth 9 + 0.3 j
    targets = rng.uniform(-2.0, 2.0, (K, 3))
    depth = 9.0 + 0.3 * np.arange(K)
    t_axis = np.stack([-targets[:, 0], -targets[:, 1], depth - targets[:, 2]], axis=1)
    q_axis = np.tile([0.0, 0.0, 0.0, 1.0], (K, 1))
    # points: class k of camera j is X_j moved in its own image plane by depth * sqrt(r2_k) in a direction of its own
    pts, owner, cls = [], [], []
    for j in range(K):
        for k, r2 in enumerate(_AXIS_R2):
            a = rng.uniform(0, 2 * np.pi)
            off = depth[j] * np.sqrt(r2)
            pts.append(targets[j] + np.array([off * np.cos(a), off * np.sin(a), 0.0]))
            owner.append(j)
            cls.append(k)
    points = np.array(pts)
    owner = np.array(owner)
    P = points.shape[0]
    # oblique cameras: on a cone around the z axis behind the axis cameras' side, looking at the cluster
    ang = 2 * np.pi * np.arange(n_obl) / n_obl + 0.2
    centers = np.stack([7.0 * np.cos(ang), 7.0 * np.sin(ang), -9.0 + rng.uniform(-1, 1, n_obl)], axis=1)
    Rw2c = _look_at(centers)
    t_obl = -np.einsum('cij,cj->ci', Rw2c, centers)
    q_obl = _quat_from_matrix(Rw2c)
    intr = np.tile(gt_intrinsics(model), (C, 1))
    cams = np.concatenate([np.concatenate([t_axis, t_obl]), np.concatenate([q_axis, q_obl]), intr], axis=1)
    pp = np.tile(np.array([1000.0, 750.0]), (C, 1))
    # track p: its owner's axis camera, every axis camera for the on-axis points (at an ordinary r2), all oblique ones
    cam_idx, pt_idx = [], []
    for p in range(P):
        seen = set(range(K, C)) | {int(owner[p])}
        if cls[p] == 0:
            seen |= set(range(K))
        cam_idx += sorted(seen)
        pt_idx += [p] * len(seen)
    cam_idx, pt_idx = np.array(cam_idx, dtype=np.int32), np.array(pt_idx, dtype=np.int32)
    prob = BAProblem(model, cams.copy(), cams, pp, points.copy(), points, None, cam_idx, pt_idx)
    depth_o, r2 = normalized(prob)
    # observations: the model's own projection (the on-axis limit where r2 == 0) + 0.5 px noise
    on = r2 == 0.0
    uv = np.empty((cam_idx.size, 2))
    uv[~on], _ = _project(model, points[pt_idx[~on]], cams[cam_idx[~on]], pp[cam_idx[~on]])
    uv[on] = pp[cam_idx[on]]
    prob.uv = np.ascontiguousarray(uv + rng.normal(0, 0.5, uv.shape))
    assert C <= 16 and P <= 64 and depth_o.min() > 1.0
    for name, mask in axis_classes(r2).items():
        assert mask.sum() >= 8, (name, int(mask.sum()))
    oblique = np.bincount(pt_idx[cam_idx >= K], minlength=P)
    assert oblique.min() >= 2
    return prob


def axis_special(prob):
    """mask of the observations in one of the five classes (the ones the mpmath path evaluates)"""
    _, r2 = normalized(prob)
    return np.any(list(axis_classes(r2).values()), axis=0)


# ------------------------------------------------------------------------------------------------------------
# parity bounds: the project's tolerance or 8x the oracle's own rounding spread, whichever is larger
# ------------------------------------------------------------------------------------------------------------
F1 = 1.0 + 1e-4     # the first trial's damping factor, which the stored records Y are prepared for
TOLERANCE = dict(Y=1e-12, V=1e-12, gp=1e-12, U=1e-10, gc=1e-10, loss=1e-12, rmse=1e-12)


def yrel(got, exp):
    """colrel of records [N, D, 3] along the camera-parameter axis and along the point axis"""
    return max(R.colrel(got, exp, axis=1), R.colrel(got, exp, axis=2))


def compare(got, exp):
    """column-wise figures of one linearization against another: dicts with Y [N,D,3], V, gp, U, gc (and loss, rmse)"""
    fig = dict(Y=yrel(got["Y"], exp["Y"]), V=R.colrel(got["V"], exp["V"]), gp=R.colrel(got["gp"], exp["gp"]),
               U=R.urel(got["U"], exp["U"]), gc=R.colrel(got["gc"], exp["gc"]))
    for k in ("loss", "rmse"):
        if k in got and k in exp:
            fig[k] = abs(got[k] - exp[k]) / abs(exp[k])
    return fig


def oracle_linearization(prob, delta, variant=""):
    """the C oracle's linearization and cost at the initial values, as the dict compare() takes"""
    from oracle import oracle as O
    ora = O.OracleBA(prob.model, prob.uv, prob.cam_idx, prob.pt_idx, prob.pp, prob.n_cams, prob.n_points,
                     variant=variant, huber_delta=delta)
    ora.linearize(prob.cams_init, prob.points_init)
    W, V = ora.get(O.W), ora.get(O.V)
    loss, rmse = ora.cost(prob.cams_init, prob.points_init)
    return dict(W=W, Y=R.y_from(W, V, prob.pt_idx, F1), V=V, gp=ora.get(O.GP), U=ora.get(O.U), gc=ora.get(O.GC),
                loss=loss, rmse=rmse)


def reference_linearization(prob, delta, mp_mask=None):
    """the independent reference's, same layout (plus the per-observation r, Jc, Jp and the `beyond` mask)"""
    r, Jc, Jp = R.reference_obs(prob, prob.cams_init, prob.points_init, mp_mask)
    out = R.assemble(r, Jc, Jp, prob.cam_idx, prob.pt_idx, prob.n_cams, prob.n_points, delta)
    out.update(r=r, Jc=Jc, Jp=Jp, Y=R.y_from(out["W"], out["V"], prob.pt_idx, F1))
    return out


def parity_bounds(prob, delta, plain=None):
    """(bounds, spreads): per quantity the spread between the oracle's plain and fused-multiply-add builds on this
    scene, in the column-wise norms, and the bound max(project tolerance, 8 x spread) -- the margin over the oracle's
    own rounding that test_gpu_ragged.py documents.  Nothing here comes from the code under test."""
    plain = oracle_linearization(prob, delta) if plain is None else plain
    spread = compare(oracle_linearization(prob, delta, variant="fma"), plain)
    return {k: max(TOLERANCE[k], 8.0 * v) for k, v in spread.items()}, spread
