"""Checkers, oracle adaptors and case lists shared by test_passes_reference.py (CPU: oracle/passes.py against the
50-digit reference) and test_gpu_passes_edges.py (MI355X: the kernels against both).  Test helper only.

Rules (ISSUE "Test pass kernels branch by branch"):
  * float64 arithmetic: |got - reference| <= 16 x (conditioning figure + eps |value|) per item, the conditioning
    figure from the reference alone (passes_reference.bound); a reference NaN / inf must be met by a NaN / inf;
  * float32 features in k_undistort: Camera.img2cam (oracle) equals the reference's float32-path value within one
    float32 ulp of the value (of the factor for FOV); rays (oracle and kernel) equal the rays of that float32-path
    value within F32_ULPS float32 ulps propagated; against the 50-digit value the bound uses float32's eps;
  * masks are equal except where the reference quantity lies within the same bound of the threshold; the scenes
    assert from the reference alone that this is at most 1 % of a case; the equality items are asserted outright.
Each check prints the worst observed ratio to its bound ("passes-ratio ..." lines, pytest -s).
"""
from types import SimpleNamespace

import numpy as np

from oracle import passes as OP
from oracle import projection_ref as OPR

import passes_edge_scene as S
import passes_reference as PR

EXACT_UNDISTORT = (0, 1, 2, 3, 4, 6)   # no transcendental function on the img2cam path
EXACT_CAM2IMG = (0, 1, 2, 3, 4)        # model 6 calls pow() in cam2img


def report(who, kernel, group, ratio, extra=""):
    print(f"passes-ratio {who:6s} {kernel:22s} {group:24s} worst {ratio:.3g} {extra}")


def held(got, hi, lo, cond, eps=PR.EPS64, floor=0.0):
    """Assert `got` within bound(cond, value) of the reference (hi + lo) on every finite row and non-finite of the
    same kind elsewhere.  Returns (worst ratio to the bound, bound)."""
    got = np.asarray(got, dtype=np.float64)
    hi, lo = np.asarray(hi), np.asarray(lo)
    cond = np.asarray(cond, dtype=np.float64)
    if hi.ndim == 2:
        cond = cond[:, None]
    nan, inf = np.isnan(hi), np.isinf(hi)
    assert np.array_equal(np.isnan(got), nan), "NaN rows differ from the reference's"
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], hi[inf]), "inf rows differ"
    ok = ~(nan | inf)
    b = np.maximum(PR.bound(np.where(np.isfinite(cond), cond, 0.0), np.where(ok, hi, 0.0), eps), floor) * np.ones_like(hi)
    err = PR.err_to(np.where(ok, got, 0.0), np.where(ok, hi, 0.0), np.where(ok, lo, 0.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(ok & (b > 0), err / np.where(b > 0, b, 1.0), np.where(ok & (err > 0), np.inf, 0.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, f"worst ratio to the bound {worst:.3g} at {np.unravel_index(np.argmax(ratio), ratio.shape)}"
    return worst, b


def masks_agree(got, want, near, forced=()):
    """equal outside `near`; the items in `forced` are never excluded"""
    near = np.array(near, dtype=bool)
    near[list(forced)] = False
    assert near.mean() <= S.MAX_NEAR or near.sum() <= len(forced)
    assert np.array_equal(np.asarray(got, bool)[~near], np.asarray(want, bool)[~near])


# ---------------------------------------------------------------------------------------------------------------
# oracle adaptors: the scenes are plain arrays, oracle/passes.py takes scene objects
# ---------------------------------------------------------------------------------------------------------------
def oracle_undistort(case):
    xy = case["xy"]
    n = len(xy)
    uv, rays = np.zeros((n, 2)), np.zeros((n, 3))
    for c, (m, p) in enumerate(zip(case["cam_model"], case["cam_params"])):
        sel = np.flatnonzero(case["feat_cam"] == c)
        if len(sel):
            with np.errstate(all="ignore"):
                uv[sel] = OP.img2cam(m, np.asarray(p), xy[sel])
                rays[sel] = OP.undistort_rays(m, np.asarray(p), xy[sel])
    return uv, rays


def _one_track_per_obs(case, key):
    img = case["obs_img"]
    return {i: SimpleNamespace(xyz=np.asarray(case["xyz"][case["obs_track"][i]], dtype=np.float64),
                               observations=np.array([[img[i], case[key][i]]], dtype=np.int64)) for i in range(len(img))}


def oracle_pixel(case, thr=None):
    cams = [SimpleNamespace(model_id=SimpleNamespace(value=m), params=np.asarray(p)) for m, p in
            zip(case["cam_model"], case["cam_params"])]
    imgs = [SimpleNamespace(world2cam=w, cam_id=int(c), features=case["feats"]) for w, c in zip(case["w2c"], case["img_cam"])]
    with np.errstate(all="ignore"):
        v, _, _, err = OP.filter_reproj_pixel(cams, imgs, _one_track_per_obs(case, "obs_feat"), case["thr"] if thr is None else thr)
    return v, err


def oracle_reproj(case):
    imgs = [SimpleNamespace(world2cam=w, features_undist=case["rays"]) for w in case["w2c"]]
    with np.errstate(all="ignore"):
        v, _, _, err = OP.filter_reproj_normalized(imgs, _one_track_per_obs(case, "obs_ray"), case["thr"])
    return v, err


def oracle_angle(case):
    imgs = [SimpleNamespace(world2cam=w, features_undist=case["rays"]) for w in case["w2c"]]
    assert case["thr"] == S.ANGLE_COS                     # the cosine filter_angle computes from 1 degree
    v, _, _ = OP.filter_angle(imgs, _one_track_per_obs(case, "obs_ray"), 1.0)
    return v


def oracle_tri(case):
    ptr, obs = case["track_ptr"], case["obs_img"]
    imgs = [SimpleNamespace(center=lambda c=c: c) for c in case["centers"]]
    tracks = {t: SimpleNamespace(xyz=case["xyz"][t], observations=np.stack([obs[ptr[t]:ptr[t + 1]], np.zeros(ptr[t + 1] - ptr[t], np.int64)], 1).astype(np.int64))
              for t in range(len(ptr) - 1)}
    assert case["thr"] == S.TRI_COS
    gone = OP.filter_tri_angle(imgs, tracks, S.TRI_DEG)
    rem = np.zeros(len(tracks), bool)
    rem[gone] = True
    return rem


def oracle_cand(case):
    """OP.complete_candidates on the scene objects for the scene's own candidates (same order: every observation of
    every track of tracks_orig that is still in tracks); the two appended depth-edge rows, which belong to no scene
    object, through the same projection_ref calls that function ends with."""
    n0 = case.get("n0", 0)
    valid, err = np.zeros(len(case["cand_img"]), bool), np.zeros(len(case["cand_img"]))
    if n0:
        cameras, images, tracks, tracks_orig = case["scene"]
        with np.errstate(all="ignore"):
            obs, rows, ok, e = OP.complete_candidates(cameras, images, tracks, tracks_orig, case["thr"])
        assert np.array_equal(obs[:, 0], case["cand_img"][:n0]) and np.array_equal(rows, case["cand_track"][:n0])
        valid[:n0], err[:n0] = ok, e
    rows, X = case["rows"][case["cand_img"][n0:]], case["xyz"][case["cand_track"][n0:]]
    uv = case["feats"][case["cand_feat"][n0:]].astype(np.float64)
    with np.errstate(all="ignore"):
        z = OPR.rotate_quat(X, rows[:, :7])[:, 2]
        err[n0:] = np.linalg.norm(OPR.reproject(case["model"], X, rows, case["pps"][case["cand_img"][n0:]]) - uv, axis=-1)
    valid[n0:] = (err[n0:] <= case["thr"]) & (z > 1e-7)
    return valid, err


# ---------------------------------------------------------------------------------------------------------------
# checks shared with test_gpu_passes_edges.py
# ---------------------------------------------------------------------------------------------------------------
def f32_uv_tolerance(case):
    """one float32 ulp of the float32-path value; for FOV, of the factor (uv = float64 base x float32 factor)"""
    ref = case["ref"]
    uv32 = ref["uv32"]
    tol = np.spacing(np.abs(uv32).astype(np.float32)).astype(np.float64)
    fac = ref["factor32"]
    fov = np.isfinite(fac)
    if fov.any():
        rel = np.spacing(np.abs(fac[fov]).astype(np.float32)).astype(np.float64) / np.abs(fac[fov])
        tol[fov] = np.abs(uv32[fov]) * rel[:, None] + 4 * PR.EPS64 * np.abs(uv32[fov])
    return tol


def f32_arith_models(case):
    """per row: does img2cam have a float32 step for float32 features (all models but the two pinholes)"""
    return ~np.isin(np.asarray(case["cam_model"])[case["feat_cam"]], (0, 1))


# Float32 path, rays against the rays of the stepwise float32 value.  Both sides run the same float32 steps on the
# same float32 inputs and differ only in the float32 transcendental functions and in where they round: sin and cos (or
# tan) are each within 1.5 ulp of the true value in numpy and within 1 ulp in the HIP device library (their documented
# maxima), so two functions differ by at most 5 ulps together; the three float32 roundings after them (two products,
# one quotient; for the FOV first branch four operations against the kernel's single rounding) add at most 1.5 ulp a
# side.  5 + 3 = 8 float32 ulps of the value, none for the models without a transcendental function.
F32_ULPS = 8.0


def check_rays_f32_path(who, name, case, rays):
    """rays of float32 features against [uv32, 1] / ||.|| (float64, as undistort_process): |d ray| <= |du| + |dv|
    since the normalization's Jacobian has norm <= 1, plus 16 eps64 for the float64 normalization itself"""
    ref, narrow = case["ref"], f32_arith_models(case)
    uv32 = ref["uv32"]
    ok = narrow & np.isfinite(uv32).all(1)
    if not ok.any():
        return
    want = np.hstack([uv32, np.ones((len(uv32), 1))])
    want = want / np.linalg.norm(want, axis=1, keepdims=True)
    tol = F32_ULPS * f32_uv_tolerance(case).sum(1) + 16 * PR.EPS64
    d = np.abs(np.asarray(rays)[ok] - want[ok]).max(1)
    assert np.isfinite(np.asarray(rays)[ok]).all() and (d <= tol[ok]).all(), float((d / tol[ok]).max())
    report(who, "k_undistort rays f32path", name, float((d / tol[ok]).max()), f"(ratio to {F32_ULPS:g} float32 ulps)")


def check_rays(who, name, case, rays):
    ref = case["ref"]
    f32 = case["xy"].dtype == np.float32
    worst, b = held(rays, ref["ray_hi"], ref["ray_lo"], ref["cond_ray"], PR.EPS32 if f32 else PR.EPS64)
    report(who, "k_undistort rays", name, worst, f"nonfinite rows {int((~np.isfinite(ref['ray_hi'])).any(1).sum())}/{len(rays)}")
    if f32:
        check_rays_f32_path(who, name, case, rays)
    return b


UNDISTORT_CASES = ([("wide", m, f) for f in (False, True) for m in range(11)] +
                   [("icdist", None, f) for f in (False, True)] + [("fov", None, f) for f in (False, True)] +
                   [("multi", None, f) for f in (False, True)] + [("single", None, False)])


def undistort_case(kind, model, f32):
    if kind == "wide":
        return S.undistort_wide(model, f32)
    if kind == "single":
        return S.undistort_single()
    return {"icdist": S.undistort_icdist, "fov": S.undistort_fov, "multi": S.undistort_multi}[kind](f32)


def case_id(c):
    return f"{c[0]}{'' if c[1] is None else c[1]}-{'f32' if c[2] else 'f64'}"


def cand_id(c):
    return f"m{c[0]}-{'f32' if c[1] else 'f64'}"


PIXEL_CASES = [("wide", m, f) for f in (False, True) for m in range(11)] + [("multi", None, f) for f in (False, True)]
CAND_CASES = [(m, f) for f in (False, True) for m in S.CAND_MODELS]


def pixel_case(kind, model, f32):
    return S.pixel_wide(model, f32) if kind == "wide" else S.pixel_multi(f32)


def ref_valid_pixel(case):
    ref = case["ref"]
    with np.errstate(invalid="ignore"):
        return (ref["depth"] > 1e-10) & (ref["err_hi"] < case["thr"])


def check_pixel(who, name, case, valid, err):
    ref = case["ref"]
    worst, b = held(err, ref["err_hi"], ref["err_lo"], ref["cond"])
    masks_agree(valid, ref_valid_pixel(case), case["near"])
    if "edge0" in case:                      # on-axis valid; depth 1e-10 not, the next double is; behind; 0/0
        assert list(valid[case["edge0"]:case["edge0"] + 5]) == [True, False, True, False, False]
    report(who, "k_filter_reproj_pixel", name, worst, f"near threshold {int(case['near'].sum())}/{len(err)}")
    return b


def check_reproj(who, case, valid, err):
    ref = case["ref"]
    worst, b = held(err, ref["err_hi"], ref["err_lo"], ref["cond"])
    with np.errstate(invalid="ignore"):
        want = (ref["depth"] > 1e-10) & (ref["err_hi"] < case["thr"])
    masks_agree(valid, want, case["near"])
    assert list(valid[-4:]) == [False, True, False, False]   # depth 1e-10, the next double, behind, 0/0
    report(who, "k_filter_reproj", "scene", worst, f"near threshold {int(case['near'].sum())}/{len(err)}")
    return b


def check_angle(who, case, valid):
    ref = case["ref"]
    want = (ref["depth"] >= 1e-10) & (ref["cos_hi"] > case["thr"])      # the reference skips pt[2] < EPSILON
    masks_agree(valid, want, case["near"])
    assert list(valid[-5:]) == [False, False, False, True, True]  # behind twice, just below 1e-10, 1e-10, just above
    report(who, "k_filter_angle", "scene", 0.0, f"mask only; near threshold {int(case['near'].sum())}/{len(valid)}")


def check_tri(who, case, remove):
    nn = case["n_named"]
    assert np.array_equal(remove[:nn], case["expect"]), remove[:nn]      # the named tracks outright
    masks_agree(remove[nn:], case["remove"][nn:], case["near"][nn:])
    report(who, "k_filter_tri_angle", "scene", 0.0, f"mask only; near threshold {int(case['near'][nn:].sum())}/{len(remove) - nn}")


def ref_valid_cand(case):
    ref = case["ref"]
    return (ref["err_hi"] <= case["thr"]) & (ref["depth"] > 1e-7)


def check_cand(who, case, valid, err):
    ref = case["ref"]
    worst, b = held(err, ref["err_hi"], ref["err_lo"], ref["cond"])
    masks_agree(valid, ref_valid_cand(case), case["near"])
    assert list(valid[case["n0"]:]) == [False, True]                     # depth exactly 1e-7, the next double above
    report(who, "k_reproj_candidates", f"model {case['model']} {'f32' if case['f32'] else 'f64'}", worst)
    return b


# ---------------------------------------------------------------------------------------------------------------
