"""Seeded edge inputs for the between-round passes (csrc/passes.hip), shared by test_passes_reference.py (oracle vs
the 50-digit reference, CPU) and test_gpu_passes_edges.py (kernels vs both).  Test helper only.

Every builder asserts, with tests/passes_reference.py or exact rational arithmetic, that its rows reach the branch or
sit on the threshold they were built for; nothing here reads oracle/passes.py or the kernel.  Builders are cached:
the 50-digit reference of a case is computed once per process.
"""
from fractions import Fraction
from functools import lru_cache
import math

import mpmath as mp
import numpy as np

import passes_reference as PR

SIZES = (255, 256, 257)      # one block less one, one block, one block and one item
N_BIG = 3001                 # 12 blocks, the last one partial
MAX_NONFINITE = 0.01         # asserted cap on the share of non-finite rows per case
MAX_NEAR = 0.01              # asserted cap on the share of rows too close to a threshold to decide

# About 5x the magnitudes of camera_models_golden.npz, signs mixed, chosen so that each forward model stays monotone
# out to r^2 = 1.5 (theta = 70 degrees for the fisheye models): the inverse the kernels iterate for exists.
WIDE_PARAMS = {
    0: [900.0, 500.0, 400.0],
    1: [900.0, 950.0, 500.0, 400.0],
    2: [900.0, 500.0, 400.0, 0.25],
    3: [900.0, 500.0, 400.0, -0.25, 0.05],
    4: [900.0, 950.0, 500.0, 400.0, 0.25, -0.05, -0.005, 0.01],
    5: [900.0, 950.0, 500.0, 400.0, -0.1, 0.02, -0.005, 0.0025],
    6: [900.0, 950.0, 500.0, 400.0, -0.25, 0.05, 0.005, -0.01, 0.015, 0.1, -0.02, 0.003],
    7: [900.0, 950.0, 500.0, 400.0, 0.9],
    8: [900.0, 500.0, 400.0, -0.15],
    9: [900.0, 500.0, 400.0, 0.15, -0.03],
    10: [900.0, 950.0, 500.0, 400.0, 0.1, -0.02, -0.005, 0.01, 0.005, 0.0025, 0.001, -0.0015],
}
FOV_SMALL = [900.0, 950.0, 500.0, 400.0, 0.005]   # omega^2 = 2.5e-5 < 1e-4: the first FOV branch
ICDIST_PARAMS = [500.0, 320.0, 240.0, -0.3]       # models 2 and 8: focal 500, k = -0.3
IDENT = np.eye(4)


def pp_of(model, p):
    return (p[1], p[2]) if model in PR.SINGLE_FOCAL else (p[2], p[3])


def fl(x):
    """round a Fraction to the nearest double (float() of a Fraction is correctly rounded)"""
    return float(x)


def up(x):
    return float(np.nextafter(x, np.inf))


def down(x):
    return float(np.nextafter(x, -np.inf))


def _wide_points(rng, model, n):
    """camera-frame points whose normalized radius reaches sqrt(1.5) (tan 70 deg for the fisheye models)"""
    rmax = np.tan(np.deg2rad(70.0)) if model in PR.FISHEYE else np.sqrt(1.5)
    r = rmax * np.sqrt(rng.uniform(0.0004, 1.0, n))
    r[0] = rmax                                    # the rim itself
    a = rng.uniform(0, 2 * np.pi, n)
    z = rng.uniform(0.5, 5.0, n)
    return np.stack([r * np.cos(a) * z, r * np.sin(a) * z, z], 1)


def project(model, p, X):
    """Camera.cam2img of the 50-digit reference, rounded to float64 [n, 2]"""
    out = np.zeros((len(X), 2))
    with mp.workdps(PR.MP_DPS):
        pm = [mp.mpf(z) for z in p]
        for i, x in enumerate(X):
            px, py, _ = PR.cam2img(model, pm, *(mp.mpf(float(z)) for z in x))
            out[i] = float(px), float(py)
    return out


def _nonfinite_ok(ref_rows):
    bad = ~np.isfinite(ref_rows).reshape(len(ref_rows), -1).all(1)
    assert bad.mean() < MAX_NONFINITE, bad.mean()
    return bad


# ------------------------------------------------------------------------------------------------------------
# k_undistort
# ------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def undistort_wide(model, f32):
    """One camera of `model`, wide-field features, then the principal point and the pixel beside it."""
    rng = np.random.default_rng(100 + model)
    p = WIDE_PARAMS[model]
    n = SIZES[model % 3] if model in (4, 5, 7) and not f32 else 129
    xy = project(model, p, _wide_points(rng, model, n - 2))
    cx, cy = pp_of(model, p)
    xy = np.concatenate([xy, [[cx, cy], [cx + 1.0, cy]]])
    if f32:
        xy = xy.astype(np.float32)
    case = dict(cam_model=[model], cam_params=[p], feat_cam=np.zeros(n, np.int32), xy=xy, pp_row=n - 2)
    ref = PR.undistort_ref([model], [p], case["feat_cam"], xy)
    bad = _nonfinite_ok(ref["ray_hi"])
    # wide rows are finite; only the principal point of a fisheye model is 0/0
    assert not bad[:n - 2].any() and not bad[n - 1]
    assert bad[n - 2] == (model in PR.FISHEYE)
    if model != 7:   # the undistorted radius the features reach (FOV's img2cam is not the inverse of its cam2img)
        assert np.nanmax((ref["uv_hi"] ** 2).sum(1)) > 1.2
    case["ref"] = ref
    return case


@lru_cache(maxsize=None)
def undistort_single():
    """n = 1"""
    p = WIDE_PARAMS[4]
    xy = np.array([[1310.5, 955.25]])
    fc = np.zeros(1, np.int32)
    ref = PR.undistort_ref([4], [p], fc, xy)
    assert np.isfinite(ref["ray_hi"]).all()
    return dict(cam_model=[4], cam_params=[p], feat_cam=fc, xy=xy, ref=ref)


@lru_cache(maxsize=None)
def undistort_icdist(f32):
    """Model 2 and model 8, focal 500, k = -0.3: r0^2 = 4 leaves the loop in iteration 1, r0^2 just under 3 in
    iteration 2 (the first iterate is large); both return the K-normalized input (2.0 and 1.7303)."""
    f, cx, cy, _ = ICDIST_PARAMS
    xy = np.array([[cx + 2.0 * f, cy], [cx + 1.7303 * f, cy]] * 2)
    if f32:
        xy = xy.astype(np.float32)
    fc = np.array([0, 0, 1, 1], np.int32)
    ref = PR.undistort_ref([2, 8], [ICDIST_PARAMS] * 2, fc, xy)
    assert list(ref["branch"]) == [1, 2, 1, 2], ref["branch"]
    x0 = (xy[:, 0].astype(np.float64) - cx) / f
    assert x0[0] ** 2 == 4.0 and 2.9 < x0[1] ** 2 < 3.0
    assert np.allclose(ref["uv_hi"][:2, 0], [2.0, 1.7303], rtol=1e-6) and np.isfinite(ref["ray_hi"]).all()
    return dict(cam_model=[2, 8], cam_params=[ICDIST_PARAMS] * 2, feat_cam=fc, xy=xy, ref=ref)


@lru_cache(maxsize=None)
def undistort_fov(f32):
    """Two FOV cameras: omega = 0.005 (first branch) and omega = 0.9 with the pixel (0, 0), pixels with u^2 + v^2
    just under 1e-4 (second branch) and ordinary pixels (general branch).  The float32 case also holds (0.01, 0):
    float32(0.01)^2 rounds to float32(1e-4), which numpy compares in float32 (not < 1e-4: general branch) while the
    50-digit square is below 1e-4; the two branches agree to 1e-9 there, so either is within the float32 bound."""
    rng = np.random.default_rng(7)
    a = np.concatenate([[[0.0, 0.0], [0.004, -0.003]], rng.uniform([0, 0], [1000, 800], (20, 2))])
    b = np.concatenate([[[0.0, 0.0], [0.007, 0.007], [-0.0099, 0.0], [0.0, 0.0099]], rng.uniform([0, 0], [1000, 800], (20, 2)),
                        rng.uniform(-1.5, 1.5, (6, 2))])
    if f32:
        b = np.concatenate([b, [[0.01, 0.0]]])
    xy = np.concatenate([a, b])
    fc = np.concatenate([np.zeros(len(a)), np.ones(len(b))]).astype(np.int32)
    order = rng.permutation(len(xy))
    xy, fc = xy[order], fc[order]
    if f32:
        xy = xy.astype(np.float32)
    params = [FOV_SMALL, WIDE_PARAMS[7]]
    ref = PR.undistort_ref([7, 7], params, fc, xy)
    assert set(ref["branch"][fc == 0]) == {1} and set(ref["branch"][fc == 1]) == {2, 3}
    assert (ref["branch"] == 2).sum() >= 4 and np.isfinite(ref["ray_hi"]).all()
    r2 = (xy.astype(np.float64) ** 2).sum(1)
    m = (fc == 1) & (ref["branch"] == 2)
    assert r2[m].max() > 9.7e-5 and r2[m].min() == 0.0     # just under 1e-4, and the origin itself
    return dict(cam_model=[7, 7], cam_params=params, feat_cam=fc, xy=xy, ref=ref)


def _multi_cameras(rng):
    """13 cameras: one of each model in shuffled order and a second fisheye and FOV camera with their own intrinsics"""
    models = [int(m) for m in rng.permutation(11)] + [5, 7]
    params = []
    for j, m in enumerate(models):
        p = list(WIDE_PARAMS[m])
        if j >= 11:
            p[0] *= 0.8
            p[2 if m not in PR.SINGLE_FOCAL else 1] += 37.5
        params.append(p)
    return models, params


@lru_cache(maxsize=None)
def undistort_multi(f32):
    """One call over 13 cameras with the features interleaved among them."""
    rng = np.random.default_rng(11)
    models, params = _multi_cameras(rng)
    n = 257 if f32 else 769
    fc = rng.integers(0, len(models), n).astype(np.int32)
    fc[:len(models)] = np.arange(len(models))             # every camera is used
    xy = np.zeros((n, 2))
    for c, (m, p) in enumerate(zip(models, params)):
        sel = np.flatnonzero(fc == c)
        xy[sel] = project(m, p, _wide_points(rng, m, len(sel)))
    if f32:
        xy = xy.astype(np.float32)
    assert sorted(set(models)) == list(range(11)) and models[:11] != sorted(models[:11])
    ref = PR.undistort_ref(models, params, fc, xy)
    assert np.isfinite(ref["ray_hi"]).all()
    return dict(cam_model=models, cam_params=params, feat_cam=fc, xy=xy, ref=ref)


# ------------------------------------------------------------------------------------------------------------
# k_filter_reproj_pixel (Camera.cam2img)
# ------------------------------------------------------------------------------------------------------------
PIXEL_THR = 1.0


def _pixel_case(obs_img, obs_track, feats, img_cam, cam_model, cam_params, w2c, xyz, thr=PIXEL_THR):
    n = len(obs_img)
    case = dict(obs_img=np.asarray(obs_img, np.int32), obs_track=np.asarray(obs_track, np.int32),
                obs_feat=np.arange(n, dtype=np.int64), feats=feats, img_cam=np.asarray(img_cam, np.int32),
                cam_model=list(cam_model), cam_params=[list(p) for p in cam_params], w2c=np.asarray(w2c), xyz=xyz, thr=thr)
    case["ref"] = PR.filter_reproj_pixel_ref(case["obs_img"], case["obs_track"], case["obs_feat"], feats, img_cam,
                                             cam_model, cam_params, w2c, xyz)
    return case


def near_threshold(value, cond, thr, eps=PR.EPS64):
    """rows whose reference quantity lies within its own bound of the threshold (undecidable in float64)"""
    with np.errstate(invalid="ignore"):
        return np.abs(value - thr) <= PR.bound(cond, value, eps)


@lru_cache(maxsize=None)
def pixel_wide(model, f32):
    """world2cam = I, one image per camera: wide-field points with noisy features around the threshold, then the
    cam2img edges: on-axis (the fisheye clamp), depth exactly 1e-10 and the next double above, a negative depth, and
    depth -1e-10 on the axis (0/0: the one non-finite row).  Model 7 uses two cameras (omega = 0.9 and 0.005) and
    points with r^2 below 1e-4.  Every model is built with float32 and with float64 features."""
    rng = np.random.default_rng(200 + model + 50 * f32)
    cams = [WIDE_PARAMS[model]] + ([FOV_SMALL] if model == 7 else [])
    n = SIZES[model % 3] if model in (4, 5, 7) and not f32 else 131
    n_edge = 5 + (4 if model == 7 else 0)
    X = _wide_points(rng, model, n - n_edge)
    img = rng.integers(0, len(cams), n).astype(np.int32)
    cx, cy = pp_of(model, cams[0])
    edge = [[0.0, 0.0, 2.0], [0.0, 0.0, 1e-10], [0.0, 0.0, up(1e-10)], [0.3, 0.2, -2.0], [0.0, 0.0, -1e-10]]
    if model == 7:
        edge += [[0.005, 0.003, 1.0], [0.0, 0.0099, 1.0], [0.011, 0.0, 1.0], [0.0, 0.0, 3.0]]
        img[n - n_edge:] = [0, 0, 0, 0, 0, 0, 0, 0, 1]
    X = np.concatenate([X, edge])
    feats = np.zeros((n, 2))
    for c, p in enumerate(cams):
        sel = np.flatnonzero(img == c)
        feats[sel] = project(model, p, X[sel])
    feats[:n - n_edge] += rng.normal(0, 0.6, (n - n_edge, 2))
    feats[n - n_edge + 4] = [cx, cy]                       # the 0/0 row: any finite feature
    feats[n - n_edge + 3] = [cx, cy]
    if f32:
        feats = feats.astype(np.float32)
    case = _pixel_case(img, np.arange(n), feats, np.arange(len(cams)), [model] * len(cams), cams,
                       np.tile(IDENT, (len(cams), 1, 1)), X)
    ref, e0 = case["ref"], n - n_edge
    bad = _nonfinite_ok(ref["err_hi"])
    assert list(np.flatnonzero(bad)) == [e0 + 4] and np.isnan(ref["err_hi"][e0 + 4])
    assert ref["depth"][e0 + 1] == 1e-10 and ref["depth"][e0 + 2] == up(1e-10) and ref["depth"][e0 + 3] < 0
    assert ref["err_hi"][e0 + 2] < 1e-6 and ref["err_hi"][e0] < 1e-6      # on the feature: valid iff the depth passes
    if model in PR.FISHEYE:
        assert ref["branch"][e0] == 4 and (ref["branch"][:e0] == 0).all()  # the clamp, only on the axis
    if model == 7:
        assert list(ref["branch"][e0 + 5:]) == [2, 2, 3, 1] and ref["branch"][e0] == 2
    near = near_threshold(ref["err_hi"], ref["cond"], PIXEL_THR)
    assert near.mean() <= MAX_NEAR
    good = np.isfinite(ref["err_hi"])
    assert 0.1 < (ref["err_hi"][good] < PIXEL_THR).mean() < 0.9          # both outcomes
    case.update(near=near, f32=f32, edge0=e0)
    return case


def _poses(rng, m):
    from scipy.spatial.transform import Rotation
    w2c = np.tile(IDENT, (m, 1, 1))
    w2c[:, :3, :3] = Rotation.from_rotvec(rng.normal(0, 0.2, (m, 3))).as_matrix()
    w2c[:, :3, 3] = rng.normal(0, 0.3, (m, 3))
    return w2c


@lru_cache(maxsize=None)
def pixel_multi(f32):
    """13 cameras (every model), 26 posed images, 513 observations interleaved among them."""
    rng = np.random.default_rng(12)
    models, params = _multi_cameras(rng)
    m = 2 * len(models)
    img_cam = rng.permutation(np.arange(m) % len(models)).astype(np.int32)
    w2c = _poses(rng, m)
    n = 513
    img = rng.integers(0, m, n).astype(np.int32)
    img[:m] = np.arange(m)
    xyz, feats = np.zeros((n, 3)), np.zeros((n, 2))
    for i in range(m):
        sel = np.flatnonzero(img == i)
        c = img_cam[i]
        pc = _wide_points(rng, models[c], len(sel)) * 0.6
        xyz[sel] = (pc - w2c[i, :3, 3]) @ w2c[i, :3, :3]                  # R^T (pc - t)
        feats[sel] = project(models[c], params[c], np.einsum("jk,ik->ij", w2c[i, :3, :3], xyz[sel]) + w2c[i, :3, 3])
    feats = feats + rng.normal(0, 0.6, (n, 2))
    if f32:
        feats = feats.astype(np.float32)
    case = _pixel_case(img, np.arange(n), feats, img_cam, models, params, w2c, xyz)
    ref = case["ref"]
    assert np.isfinite(ref["err_hi"]).all() and (ref["depth"] > 0.1).all()
    near = near_threshold(ref["err_hi"], ref["cond"], PIXEL_THR)
    assert near.mean() <= MAX_NEAR and 0.1 < (ref["err_hi"] < PIXEL_THR).mean() < 0.9
    case.update(near=near, f32=f32)
    return case


# ------------------------------------------------------------------------------------------------------------
# k_filter_reproj, k_filter_angle: general scenes with the depth edges
# ------------------------------------------------------------------------------------------------------------
REPROJ_THR = 1e-2
ANGLE_COS = float(np.cos(np.deg2rad(1.0)))


def _obs_scene(seed, n, noise):
    rng = np.random.default_rng(seed)
    m, t = 40, 500
    w2c = _poses(rng, m)
    w2c[:, :3, 3] += [0, 0, 6.0]
    xyz = rng.normal(0, 1.5, (t, 3))
    img = rng.integers(0, m, n).astype(np.int32)
    trk = rng.integers(0, t, n).astype(np.int32)
    pc = np.einsum("ijk,ik->ij", w2c[img, :3, :3], xyz[trk]) + w2c[img, :3, 3]
    rays = pc / np.linalg.norm(pc, axis=1, keepdims=True) + rng.normal(0, noise, (n, 3))
    return w2c, xyz, img, trk, rays


def _depth_rows(w2c, xyz, img, trk, rays, depths):
    """append one identity image and, per depth z, a point (0, 0, z) seen along the ray (0, 0, 1)"""
    k = len(depths)
    w2c = np.concatenate([w2c, IDENT[None]])
    pts = np.array([[0.0, 0.0, z] for z in depths])
    img = np.concatenate([img, np.full(k, len(w2c) - 1)]).astype(np.int32)
    trk = np.concatenate([trk, len(xyz) + np.arange(k)]).astype(np.int32)
    return w2c, np.concatenate([xyz, pts]), img, trk, np.concatenate([rays, np.tile([0.0, 0.0, 1.0], (k, 1))])


@lru_cache(maxsize=None)
def reproj_scene():
    """1025 observations for k_filter_reproj; the last four: depth exactly 1e-10 (invalid: the test is >), the next
    double above (valid), a point behind the camera, and depth -1e-10 on the axis (0/0: the one non-finite row)."""
    w2c, xyz, img, trk, rays = _obs_scene(21, 1025 - 4, 5e-3)
    # at depth z the error against the ray (0, 0, 1) is 0, so validity is the depth test alone
    w2c, xyz, img, trk, rays = _depth_rows(w2c, xyz, img, trk, rays, [1e-10, up(1e-10), -2.0, -1e-10])
    n = len(img)
    ref = PR.filter_reproj_normalized_ref(img, trk, np.arange(n), w2c, xyz, rays)
    bad = _nonfinite_ok(ref["err_hi"])
    assert list(np.flatnonzero(bad)) == [n - 1]
    assert list(ref["depth"][-4:]) == [1e-10, up(1e-10), -2.0, -1e-10] and (ref["err_hi"][-4:-1] == 0).all()
    near = near_threshold(ref["err_hi"], ref["cond"], REPROJ_THR)
    assert near.mean() <= MAX_NEAR and 0.1 < (ref["err_hi"][~bad] < REPROJ_THR).mean() < 0.9
    assert (np.abs(ref["depth"][:-4]) > 0.1).all()
    return dict(obs_img=img, obs_track=trk, obs_ray=np.arange(n), w2c=w2c, xyz=xyz, rays=rays, thr=REPROJ_THR, ref=ref,
                near=near)


@lru_cache(maxsize=None)
def angle_scene():
    """3001 observations for k_filter_angle (threshold cos 1 deg); the last five are the depth edges on the ray
    (0, 0, 1): behind the camera (-2 and -1e-12), the double just below 1e-10 (invalid: p2 < 1e-10 leaves early),
    1e-10 itself and the double just above (both go on to the angle test and pass it)."""
    w2c, xyz, img, trk, rays = _obs_scene(22, N_BIG - 5, 1e-2)
    w2c, xyz, img, trk, rays = _depth_rows(w2c, xyz, img, trk, rays, [-2.0, -1e-12, down(1e-10), 1e-10, up(1e-10)])
    n = len(img)
    ref = PR.filter_angle_ref(img, trk, np.arange(n), w2c, xyz, rays)
    assert np.isfinite(ref["cos_hi"]).all()
    assert list(ref["depth"][-5:]) == [-2.0, -1e-12, down(1e-10), 1e-10, up(1e-10)]
    assert (ref["cos_hi"][-3:] == 1.0).all() and (ref["cos_hi"][-5:-3] == -1.0).all()
    near = near_threshold(ref["cos_hi"], ref["cond"], ANGLE_COS)
    assert near.mean() <= MAX_NEAR and 0.1 < (ref["cos_hi"] > ANGLE_COS).mean() < 0.9
    assert (np.abs(ref["depth"][:-5]) > 0.1).all()
    return dict(obs_img=img, obs_track=trk, obs_ray=np.arange(n), w2c=w2c, xyz=xyz, rays=rays, thr=ANGLE_COS, ref=ref,
                near=near)


# ------------------------------------------------------------------------------------------------------------
# threshold equality: world2cam = I and zeros placed so that every sum is exact in any order
# ------------------------------------------------------------------------------------------------------------
def F(x):
    return Fraction(float(x))


@lru_cache(maxsize=None)
def eq_angle():
    """pt = (0, 0, 2): ||pt|| = sqrt(0 + 0 + 4) = 2 and pt / ||pt|| = (0, 0, 1) exactly, so the dot product with the
    ray (s, 0, c) is 0 s + 0 0 + 1 c = c.  Row 0: c = cos_thres (invalid, the test is >); row 1: the next double up."""
    c = ANGLE_COS
    rays = np.array([[0.5, 0.0, c], [0.5, 0.0, up(c)]])
    xyz = np.array([[0.0, 0.0, 2.0]])
    for r, want in zip(rays, (c, up(c))):
        unit = [F(0) / 2, F(0) / 2, F(2) / 2]
        assert F(2) * F(2) == 4 and unit == [0, 0, 1]
        assert unit[0] * F(r[0]) + unit[1] * F(r[1]) + unit[2] * F(r[2]) == F(want)
    return dict(obs_img=np.zeros(2, np.int32), obs_track=np.zeros(2, np.int32), obs_ray=np.arange(2), w2c=IDENT[None],
                xyz=xyz, rays=rays, thr=c, expect=np.array([False, True]))


@lru_cache(maxsize=None)
def eq_reproj():
    """pt = (0, 0, 1): both reprojected coordinates are 0 / (1 + 1e-10) = 0.  The ray (e, 0, rz) with rz = the double
    nearest 1 - 1e-10 has fl(rz + 1e-10) = 1, so its reprojection is (e / 1, 0 / 1) and the error is
    sqrt((0 - e)^2 + 0) = e exactly (e^2 is rounded, but sqrt of the rounded square of a double returns it).
    Row 0: e = max_err (invalid, the test is <); row 1: the next double down (valid)."""
    thr = REPROJ_THR
    rz = 1.0 - 1e-10
    assert fl(F(rz) + F(1e-10)) == 1.0
    rays = np.array([[thr, 0.0, rz], [down(thr), 0.0, rz]])
    with mp.workdps(60):
        for r in rays:
            d0 = fl(F(0) / (F(1) + F(1e-10))) - fl(F(r[0]) / 1)
            sq = fl(F(d0) * F(d0) + 0)
            assert float(mp.sqrt(mp.mpf(sq))) == abs(r[0])
    return dict(obs_img=np.zeros(2, np.int32), obs_track=np.zeros(2, np.int32), obs_ray=np.arange(2), w2c=IDENT[None],
                xyz=np.array([[0.0, 0.0, 1.0]]), rays=rays, thr=thr, expect=np.array([False, True]),
                err=np.abs(rays[:, 0]))


@lru_cache(maxsize=None)
def eq_pixel():
    """PINHOLE with the principal point at the origin: pt = (0, 0, 1) projects to 0 f + 0 = 0, the feature (-e, 0)
    gives the error sqrt((0 + e)^2 + 0) = e.  Row 0: e = max_err = 3 (invalid); row 1: the next double down."""
    thr = 3.0
    feats = np.array([[-thr, 0.0], [-down(thr), 0.0]])
    with mp.workdps(60):
        for ft in feats:
            d0 = F(0) * 900 + 0 - F(ft[0])
            assert float(mp.sqrt(mp.mpf(fl(d0 * d0)))) == -ft[0] and fl(d0) == -ft[0]
    return dict(obs_img=np.zeros(2, np.int32), obs_track=np.zeros(2, np.int32), obs_feat=np.arange(2, dtype=np.int64),
                feats=feats, img_cam=np.zeros(1, np.int32), cam_model=[1], cam_params=[[900.0, 950.0, 0.0, 0.0]],
                w2c=IDENT[None], xyz=np.array([[0.0, 0.0, 1.0]]), thr=thr, expect=np.array([False, True]),
                err=-feats[:, 0])


@lru_cache(maxsize=None)
def eq_cand():
    """PINHOLE, identity pose (t = 0, q = (0, 0, 0, 1)), principal point at the origin: a point on the axis projects
    to 0 and the feature (e, 0) gives the error e; the rotated depth is the point's z.  Rows: error = thr (valid, the
    test is <=), the next double above (invalid), depth exactly 1e-7 (invalid, the test is >), the next double above
    (valid)."""
    thr = 3.0
    rows = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 900.0, 950.0]])
    feats = np.array([[thr, 0.0], [up(thr), 0.0], [0.0, 0.0], [0.0, 0.0]])
    xyz = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1e-7], [0.0, 0.0, up(1e-7)]])
    trk = np.array([0, 0, 1, 2], np.int32)
    ref = PR.reproj_candidates_ref(1, np.zeros(4, np.int32), trk, np.arange(4), feats, rows, np.zeros((1, 2)), xyz)
    assert list(ref["err_hi"]) == [thr, up(thr), 0.0, 0.0] and (ref["err_lo"] == 0).all()
    assert list(ref["depth"]) == [1.0, 1.0, 1e-7, up(1e-7)]
    return dict(model=1, cand_img=np.zeros(4, np.int32), cand_track=trk, cand_feat=np.arange(4, dtype=np.int64),
                feats=feats, rows=rows, pps=np.zeros((1, 2)), xyz=xyz, thr=thr,
                expect=np.array([True, False, False, True]), err=feats[:, 0])


# ------------------------------------------------------------------------------------------------------------
# k_filter_tri_angle
# ------------------------------------------------------------------------------------------------------------
def _fl_unit(X, c):
    """(X - c) / (||X - c|| + 1e-10) in correctly rounded double steps (Fractions; sqrt through mpmath)"""
    v = [fl(F(X[a]) - F(c[a])) for a in range(3)]
    s = fl(F(fl(F(fl(F(v[0]) * F(v[0]))) + F(fl(F(v[1]) * F(v[1]))))) + F(fl(F(v[2]) * F(v[2]))))
    with mp.workdps(60):
        nrm = fl(F(float(mp.sqrt(mp.mpf(s)))) + F(1e-10))
    return [fl(F(z) / F(nrm)) for z in v]


def _fl_dot(a, b):
    """a . b for vectors whose third components are zero: the sum has two terms, one rounding, any order"""
    assert a[2] == 0 and b[2] == 0
    return fl(F(fl(F(a[0]) * F(b[0]))) + F(fl(F(a[1]) * F(b[1]))))


TRI_DEG = 2.0
TRI_COS = float(np.cos(np.deg2rad(TRI_DEG)))   # what FilterTracksTriangulationAngle compares with


@lru_cache(maxsize=None)
def tri_scene():
    """Tracks for k_filter_tri_angle, the point at the origin unless said otherwise; `remove` is the expected mask of
    the named tracks (asserted outright), the random tracks behind them go through the reference.
      0: no observation (all() of nothing: removed)      1: one observation (its own cosine ~ 1: removed)
      2, 3, 4: two observations whose cosine is exactly the threshold (kept: the test is >), one ulp below (kept),
               one ulp above (removed); the directions lie in the plane z = 0 and one of them is the x axis
      5: a duplicated image id in a narrow track (removed)
      6: the point exactly at one camera's centre (direction 0, cosine 0: kept)
      7: 200 observations, only the pair of the last two fails (kept)      8: 200 observations, all pass (removed)
    """
    rng = np.random.default_rng(31)
    centers, obs, ptr, xyz = [], [], [0], []

    def add(cs, X=(0.0, 0.0, 0.0), ids=None):
        base = len(centers)
        centers.extend([list(map(float, c)) for c in cs])
        obs.extend([base + i for i in (ids if ids is not None else range(len(cs)))])
        ptr.append(len(obs))
        xyz.append(list(map(float, X)))

    add([])
    add([[-1.0, 0.5, 0.25]])
    # the pair: a = unit(-c_a) with c_a = (-2, 0, 0), b = unit(-c_b) with c_b = -p (1, tan 2 deg, 0) for three distances p
    ca = [-2.0, 0.0, 0.0]
    a = _fl_unit([0.0] * 3, ca)
    thr = TRI_COS

    def dotf(p, q):                # the same double sequence in plain float arithmetic, to search with
        return a[0] * (p / (math.sqrt(p * p + q * q + 0.0) + 1e-10))

    lo, hi = 0.99 * math.tan(math.radians(TRI_DEG)), math.tan(math.radians(TRI_DEG))
    assert dotf(1.0, lo) > thr > dotf(1.0, hi)             # 1e-10 in both norms puts the exact 2 deg pair below thr
    while up(lo) < hi:
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if dotf(1.0, mid) > thr else (lo, mid)
    q0 = lo
    found = {}
    for k in range(-4000, 4000):   # the same direction at other distances: 1e-10 in the norm moves the cosine by
        p = 1.0 + k * 2.0 ** -23   # about a tenth of an ulp per step
        d = dotf(p, fl(F(p) * F(q0)))
        for sgn, want in ((-1, down(thr)), (0, thr), (1, up(thr))):
            if d == want:
                found.setdefault(sgn, p)
        if len(found) == 3:
            break
    assert set(found) == {-1, 0, 1}, found
    for p, want in ((found[0], thr), (found[-1], down(thr)), (found[1], up(thr))):
        cb = [-p, -fl(F(p) * F(q0)), 0.0]
        b = _fl_unit([0.0] * 3, cb)
        assert _fl_dot(a, b) == want and _fl_dot(a, a) > thr and _fl_dot(b, b) > thr
        add([ca, cb])
    narrow = [[-5.0, 0.01 * i, 0.0] for i in range(3)]
    add(narrow, ids=[0, 1, 1, 2, 0])
    add([[1.0, 2.0, 3.0], [-4.0, 2.0, 3.0], [-4.0, 2.05, 3.0]], X=(1.0, 2.0, 3.0))

    def fan(angles_deg):
        ang = np.deg2rad(np.asarray(angles_deg))
        dist = rng.uniform(4.0, 9.0, len(ang))
        return np.stack([-dist * np.cos(ang), -dist * np.sin(ang), rng.uniform(-0.01, 0.01, len(ang))], 1)

    add(fan(np.concatenate([rng.uniform(-0.3, 0.3, 198), [1.05, -1.05]])))
    add(fan(rng.uniform(-0.5, 0.5, 200)))
    n_named = len(xyz)
    for _ in range(300):                                   # random short tracks: more than one block of tracks
        L = int(rng.integers(2, 9))
        X = rng.normal(0, 1.0, 3)
        spread = rng.choice([0.02, 0.2, 2.0])
        add(X + [0, 0, -6.0] + rng.normal(0, spread, (L, 3)), X=X)
    centers, xyz = np.array(centers), np.array(xyz)
    ptr, obs = np.array(ptr, np.int64), np.array(obs, np.int32)
    ref = PR.tri_angle_ref(ptr, obs, centers, xyz)
    rem = np.zeros(len(xyz), bool)
    near = np.zeros(len(xyz), bool)
    for t, (cosm, cond) in enumerate(ref):
        rem[t] = bool(np.all(cosm > thr))
        near[t] = bool(np.any(np.abs(cosm - thr) <= PR.bound(cond, cosm)))
    expect = np.array([True, True, False, False, True, True, False, False, True])
    # what the named tracks were built for, from the 50-digit cosines: 2..4 sit on the threshold by construction
    assert list(near[:n_named]) == [False, False, True, True, True, False, False, False, False]
    decided = [0, 1, 5, 6, 7, 8]
    assert np.array_equal(rem[decided], expect[decided])
    c7 = ref[7][0]
    fails = np.argwhere(np.triu(c7 <= thr))
    assert fails.tolist() == [[198, 199]]                  # only the last pair
    assert ref[6][0][0, 1] == 0.0 and len(ref[0][0]) == 0 and ref[1][0].shape == (1, 1)
    assert near[n_named:].mean() <= MAX_NEAR and 0.1 < rem[n_named:].mean() < 0.9
    assert len(xyz) > 256
    return dict(track_ptr=ptr, obs_img=obs, centers=centers, xyz=xyz, thr=thr, ref=ref, remove=rem, near=near,
                expect=expect, n_named=n_named)


# ------------------------------------------------------------------------------------------------------------
# k_reproj_candidates
# ------------------------------------------------------------------------------------------------------------
CAND_MODELS = (0, 1, 2, 3, 4, 5, 6, 8, 9)
CAND_THR = 3.0
PP_IDX = {0: [1, 2], 2: [1, 2], 3: [1, 2], 8: [1, 2], 9: [1, 2]}


@lru_cache(maxsize=None)
def cand_scene(model, f32):
    """Every observation of a small make_retri_scene as a candidate (float32 or float64 features), then one identity-pose image with a point at depth exactly 1e-7 (invalid) and at the next double above
    (valid), each with its feature on its own projection."""
    from scipy.spatial.transform import Rotation
    from instantsfm_amd.synth import make_retri_scene
    cameras, images, tracks, tracks_orig = make_retri_scene(model=model, n_cams=12, n_points=10, seed=40 + model,
                                                            point_sigma=0.02,
                                                            features_dtype=np.float32 if f32 else np.float64)
    ppi = PP_IDX.get(model, [2, 3])
    rows, pps = [], []
    for im in images:
        prm = [float(z) for z in cameras[im.cam_id].params]
        w = np.asarray(im.world2cam, dtype=np.float64)
        rows.append(list(w[:3, 3]) + list(Rotation.from_matrix(w[:3, :3]).as_quat()) + [z for j, z in enumerate(prm) if j not in ppi])
        pps.append([prm[j] for j in ppi])
    prm0 = [float(z) for z in cameras[0].params]
    rows.append([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0] + [z for j, z in enumerate(prm0) if j not in ppi])
    pps.append([prm0[j] for j in ppi])
    rows, pps = np.array(rows), np.array(pps)
    keys = list(tracks.keys())
    xyz = [np.asarray(tracks[k].xyz, dtype=np.float64) for k in keys]
    foff = np.concatenate([[0], np.cumsum([len(im.features) for im in images])])
    feats = np.concatenate([np.asarray(im.features).reshape(-1, 2) for im in images])
    ci, ct, cf = [], [], []
    for k, o in tracks_orig.items():
        if k in tracks:
            for i, f in np.asarray(o).reshape(-1, 2).tolist():
                ci.append(i)
                ct.append(keys.index(k))
                cf.append(foff[i] + f)
    n0 = len(ci)
    edge = np.array([[1e-8, 0.0, 1e-7], [1e-8, 0.0, up(1e-7)]])
    fe = project(model, prm0, edge)        # cam2img adds 1e-10 to the depth: off by 1e-3 relative here, far inside thr
    for j in range(2):
        ci.append(len(images))
        ct.append(len(xyz))
        cf.append(len(feats) + j)
        xyz.append(edge[j])
    feats = np.concatenate([feats, fe.astype(feats.dtype)])
    ci, ct, cf, xyz = np.array(ci, np.int32), np.array(ct, np.int32), np.array(cf, np.int64), np.array(xyz)
    ref = PR.reproj_candidates_ref(model, ci, ct, cf, feats, rows, pps, xyz)
    assert np.isfinite(ref["err_hi"]).all()
    assert list(ref["depth"][n0:]) == [1e-7, up(1e-7)] and (ref["err_hi"][n0:] < 0.5).all()
    near = near_threshold(ref["err_hi"], ref["cond"], CAND_THR)
    assert near.mean() <= MAX_NEAR and (np.abs(ref["depth"][:n0] - 1e-7) > 1e-3).all()
    assert (ref["err_hi"] <= CAND_THR).any() and (ref["err_hi"] > CAND_THR).any()
    return dict(model=model, cand_img=ci, cand_track=ct, cand_feat=cf, feats=feats, rows=rows, pps=pps, xyz=xyz,
                thr=CAND_THR, ref=ref, near=near, f32=f32, n0=n0, scene=(cameras, images, tracks, tracks_orig))
