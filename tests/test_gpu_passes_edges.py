"""The pass kernels of csrc/passes.hip branch by branch, on the edge scenes of tests/passes_edge_scene.py, held to both
checkers: the independent 50-digit reference (tests/passes_reference.py) and the CPU restatement (oracle/passes.py).
Needs an MI355X.

  * rows of models without a transcendental function on the path: bit-equal to the oracle (img2cam: 0, 1, 2, 3, 4, 6;
    cam2img: 0 .. 4 -- model 6 calls pow() there);
  * every other row: within 16 x (conditioning figure + eps |value|) of the 50-digit reference and within
    max(1e-13, that bound) of the oracle;
  * a row is non-finite wherever the reference's is, NaN for NaN; no row is skipped (the scenes assert that fewer
    than 1 % of a case's rows are non-finite);
  * masks equal the reference's except within the bound of the threshold (at most 1 % of a case, asserted by the
    scenes from the reference alone); the equality items are asserted outright;
  * float32 features in k_undistort: the rays also equal the rays of the reference's stepwise float32-path value
    within 8 float32 ulps propagated (passes_checks.check_rays_f32_path);
  * every cam2img and candidate case runs with float32 and with float64 features;
  * two runs of every kernel return identical bytes.
The 50-digit references are built in this process by the cached scene builders: the whole file takes 17 s on
the MI355X host (about 30 s on a slower one), 1.1 s for the largest single case; the kernels take milliseconds.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

from instantsfm_amd import _capi, passes  # noqa: E402

import passes_edge_scene as S  # noqa: E402
import passes_reference as PR  # noqa: E402
import passes_checks as T  # noqa: E402


def twice(fn):
    """run a kernel wrapper twice: identical bytes"""
    a, b = fn(), fn()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert x.tobytes() == y.tobytes(), "two runs differ"
    return a


def close_to_oracle(got, want, bound):
    """|kernel - oracle| <= max(1e-13, bound) on finite rows, the same non-finite kind elsewhere"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    ok = np.isfinite(want)
    d = np.abs(np.where(ok, got, 0.0) - np.where(ok, want, 0.0))
    lim = np.maximum(1e-13, bound)
    assert (d <= lim).all(), float((d / lim).max())


# ---------------------------------------------------------------------------------------------------------------
# k_undistort
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.UNDISTORT_CASES, ids=T.case_id)
def test_undistort(case):
    c = T.undistort_case(*case)
    rays = twice(lambda: passes.undistort(c["xy"], c["feat_cam"], np.asarray(c["cam_model"], np.int32), c["cam_params"]))
    assert rays.shape == (len(c["xy"]), 3)
    _, orays = T.oracle_undistort(c)
    b = T.check_rays("gpu", T.case_id(case), c, rays)                 # against the 50-digit reference, every row
    exact = np.isin(np.asarray(c["cam_model"])[c["feat_cam"]], T.EXACT_UNDISTORT)
    np.testing.assert_array_equal(rays[exact], orays[exact])
    close_to_oracle(rays[~exact], orays[~exact], b[~exact])


# ---------------------------------------------------------------------------------------------------------------
# k_filter_reproj_pixel
# ---------------------------------------------------------------------------------------------------------------
def gpu_pixel(c, thr=None):
    return passes.filter_reproj_pixel(c["obs_img"], c["obs_track"], c["obs_feat"], c["feats"], c["img_cam"],
                                      np.asarray(c["cam_model"], np.int32), c["cam_params"], c["w2c"], c["xyz"],
                                      c["thr"] if thr is None else thr, with_err=True)


@pytest.mark.parametrize("case", T.PIXEL_CASES, ids=T.case_id)
def test_filter_reproj_pixel(case):
    c = T.pixel_case(*case)
    v, err = twice(lambda: gpu_pixel(c))
    b = T.check_pixel("gpu", T.case_id(case), c, v, err)
    ov, oerr = T.oracle_pixel(c)
    if case[0] == "wide" and case[1] in T.EXACT_CAM2IMG:      # world2cam = I: the point is exact in any sum order
        np.testing.assert_array_equal(err, oerr)
        np.testing.assert_array_equal(v, ov)
    else:                                                     # transcendental models; posed images (einsum's order)
        close_to_oracle(err, oerr, b)
        near = c["near"]
        assert np.array_equal(v[~near], ov[~near])
    assert np.array_equal(passes.filter_reproj_pixel(c["obs_img"], c["obs_track"], c["obs_feat"], c["feats"], c["img_cam"],
                                                     np.asarray(c["cam_model"], np.int32), c["cam_params"], c["w2c"],
                                                     c["xyz"], c["thr"]), v)          # the call without err


# ---------------------------------------------------------------------------------------------------------------
# k_filter_reproj, k_filter_angle, k_filter_tri_angle
# ---------------------------------------------------------------------------------------------------------------
def gpu_reproj(c):
    return passes.filter_reproj_normalized(c["obs_img"], c["obs_track"], c["obs_ray"], c["w2c"], c["xyz"], c["rays"],
                                           c["thr"], with_err=True)


def gpu_angle(c):
    return passes.filter_angle(c["obs_img"], c["obs_track"], c["obs_ray"], c["w2c"], c["xyz"], c["rays"], c["thr"])


def gpu_tri(c):
    return passes.filter_tri_angle(c["track_ptr"], c["obs_img"], c["centers"], c["xyz"], c["thr"])


def test_filter_reproj_normalized():
    c = S.reproj_scene()
    v, err = twice(lambda: gpu_reproj(c))
    b = T.check_reproj("gpu", c, v, err)
    ov, oerr = T.oracle_reproj(c)
    close_to_oracle(err, oerr, b)
    assert np.array_equal(v[~c["near"]], ov[~c["near"]])


def test_filter_angle():
    c = S.angle_scene()
    v = twice(lambda: gpu_angle(c))
    T.check_angle("gpu", c, v)
    ov = T.oracle_angle(c)
    assert np.array_equal(v[~c["near"]], ov[~c["near"]])


def test_filter_tri_angle():
    c = S.tri_scene()
    rem = twice(lambda: gpu_tri(c))
    T.check_tri("gpu", c, rem)
    orem = T.oracle_tri(c)
    keep = ~c["near"]
    keep[:c["n_named"]] = True                                # the named tracks are never excluded
    assert np.array_equal(rem[keep], orem[keep])


# ---------------------------------------------------------------------------------------------------------------
# k_reproj_candidates
# ---------------------------------------------------------------------------------------------------------------
def gpu_cand(c, model=None):
    return passes.reproj_candidates(c["model"] if model is None else model, c["cand_img"], c["cand_track"], c["cand_feat"],
                                    c["feats"], c["rows"], c["pps"], c["xyz"], c["thr"], with_err=True)


@pytest.mark.parametrize("case", T.CAND_CASES, ids=T.cand_id)
def test_reproj_candidates(case):
    c = S.cand_scene(*case)
    v, err = twice(lambda: gpu_cand(c))
    b = T.check_cand("gpu", c, v, err)
    ov, oerr = T.oracle_cand(c)
    close_to_oracle(err, oerr, b)
    assert np.array_equal(v[~c["near"]], ov[~c["near"]])


@pytest.mark.parametrize("model", [7, 10])
def test_reproj_candidates_unsupported_model(model):
    c = S.eq_cand()
    with pytest.raises(_capi.BAError) as e:
        gpu_cand(c, model)
    assert e.value.code == _capi.INSFM_BA_EINVAL


@pytest.mark.parametrize("model,rc", [(1, _capi.INSFM_BA_OK), (9, _capi.INSFM_BA_OK), (7, _capi.INSFM_BA_EINVAL),
                                      (10, _capi.INSFM_BA_EINVAL)])
def test_reproj_candidates_empty(model, rc):
    """n = 0: a supported model returns OK, an unsupported one still EINVAL, and neither output is written"""
    L = _capi.load()
    dev = torch.device("cuda:0")
    valid = torch.full((8,), 0xAB, dtype=torch.uint8, device=dev)
    err = torch.full((8,), -7.5, dtype=torch.float64, device=dev)
    buf = torch.zeros(64, dtype=torch.float64, device=dev)
    p = ctypes.c_void_p(buf.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for ptr in (p, None):                                     # with buffers, and with the null pointers n = 0 allows
        got = L.insfm_reproj_candidates(0, model, ptr, ptr, ptr, ptr, 0, ptr, ptr, ptr, 3.0,
                                        ctypes.c_void_p(valid.data_ptr()), ctypes.c_void_p(err.data_ptr()), stream)
        assert got == rc
    torch.cuda.synchronize(dev)
    assert (valid.cpu().numpy() == 0xAB).all() and (err.cpu().numpy() == -7.5).all()
    v, e = passes.reproj_candidates(model if rc == 0 else 1, np.zeros(0), np.zeros(0), np.zeros(0), np.zeros((0, 2)),
                                    np.zeros((1, 9)), np.zeros((1, 2)), np.zeros((1, 3)), 3.0, with_err=True)
    assert v.shape == (0,) and e.shape == (0,)


# ---------------------------------------------------------------------------------------------------------------
# threshold equality: asserted outright
# ---------------------------------------------------------------------------------------------------------------
def test_equality_angle():
    c = S.eq_angle()
    assert np.array_equal(twice(lambda: gpu_angle(c)), c["expect"])


def test_equality_reproj():
    c = S.eq_reproj()
    v, err = twice(lambda: gpu_reproj(c))
    assert np.array_equal(err, c["err"]) and np.array_equal(v, c["expect"])


def test_equality_pixel():
    c = S.eq_pixel()
    v, err = twice(lambda: gpu_pixel(c))
    assert np.array_equal(err, c["err"]) and np.array_equal(v, c["expect"])


def test_equality_candidates():
    c = S.eq_cand()
    v, err = twice(lambda: gpu_cand(c))
    assert np.array_equal(err, c["err"]) and np.array_equal(v, c["expect"])
