"""oracle/passes.py held to the independent 50-digit reference (tests/passes_reference.py) on the edge scenes of
tests/passes_edge_scene.py: wide fields, strong distortion, every FOV branch in both precisions, the icdist exit in
iterations 1 and 2, the fisheye clamp, the depth early-outs, empty and single-observation tracks and both sides of
every comparison sign.  CPU only; the rules and checkers are in tests/passes_checks.py.  Each test prints the worst
observed ratio to the bound ("passes-ratio ..." lines, pytest -s); DESIGN.md section 10 records them.
"""
import numpy as np
import pytest

import passes_edge_scene as S
from passes_checks import (CAND_CASES, PIXEL_CASES, UNDISTORT_CASES, cand_id, case_id, check_angle, check_cand,
                           check_pixel, check_rays, check_reproj, check_tri, f32_arith_models, f32_uv_tolerance, held,
                           oracle_angle, oracle_cand, oracle_pixel, oracle_reproj, oracle_tri, oracle_undistort,
                           pixel_case, report, undistort_case)


@pytest.mark.parametrize("case", UNDISTORT_CASES, ids=case_id)
def test_oracle_undistort(case):
    kind, model, f32 = case
    c = undistort_case(kind, model, f32)
    ref = c["ref"]
    uv, rays = oracle_undistort(c)
    name = case_id(case)
    if not f32:
        worst, _ = held(uv, ref["uv_hi"], ref["uv_lo"], ref["cond_uv"])
        report("oracle", "img2cam", name, worst)
    else:
        narrow = f32_arith_models(c)
        if (~narrow).any():                 # the pinholes compute in float64 whatever the feature type
            worst, _ = held(uv[~narrow], ref["uv_hi"][~narrow], ref["uv_lo"][~narrow], ref["cond_uv"][~narrow])
            report("oracle", "img2cam", name + " (0,1)", worst)
        if narrow.any():
            want, tol = ref["uv32"][narrow], f32_uv_tolerance(c)[narrow]
            assert np.array_equal(np.isnan(uv[narrow]), np.isnan(want))
            ok = ~np.isnan(want)
            d = np.abs(uv[narrow][ok] - want[ok])
            r = np.where(d > 0, d / np.where(tol[ok] > 0, tol[ok], 1.0), 0.0) + np.where((d > 0) & (tol[ok] == 0), np.inf, 0.0)
            assert (d <= tol[ok]).all(), float(r.max())
            report("oracle", "img2cam f32 path", name, float(r.max()) if d.size else 0.0,
                   f"rows that differ {int((uv[narrow] != want)[ok].reshape(-1).sum())}/{ok.sum()} (ratio to one float32 ulp)")
    check_rays("oracle", name, c, rays)


@pytest.mark.parametrize("case", PIXEL_CASES, ids=case_id)
def test_oracle_filter_reproj_pixel(case):
    c = pixel_case(*case)
    v, err = oracle_pixel(c)
    check_pixel("oracle", case_id(case), c, v, err)


def test_oracle_filter_reproj_normalized():
    c = S.reproj_scene()
    check_reproj("oracle", c, *oracle_reproj(c))


def test_oracle_filter_angle():
    c = S.angle_scene()
    check_angle("oracle", c, oracle_angle(c))


def test_oracle_filter_tri_angle():
    c = S.tri_scene()
    check_tri("oracle", c, oracle_tri(c))


@pytest.mark.parametrize("case", CAND_CASES, ids=cand_id)
def test_oracle_reproj_candidates(case):
    c = S.cand_scene(*case)
    check_cand("oracle", c, *oracle_cand(c))


# ---------------------------------------------------------------------------------------------------------------
# threshold equality: asserted outright, never excluded
def test_oracle_equality_angle():
    c = S.eq_angle()
    assert np.array_equal(oracle_angle(c), c["expect"])


def test_oracle_equality_reproj():
    c = S.eq_reproj()
    v, err = oracle_reproj(c)
    assert np.array_equal(err, c["err"]) and np.array_equal(v, c["expect"])


def test_oracle_equality_pixel():
    c = S.eq_pixel()
    v, err = oracle_pixel(c)
    assert np.array_equal(err, c["err"]) and np.array_equal(v, c["expect"])


def test_oracle_equality_candidates():
    c = S.eq_cand()
    v, err = oracle_cand(c)
    assert np.array_equal(err, c["err"]) and np.array_equal(v, c["expect"])
