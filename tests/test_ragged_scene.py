"""The ragged scene generator (tests/ragged_scene.py) itself: deterministic per seed, honours its arguments, and gives
scenes the oracle's LM steps through without a failed step.  Runs without a GPU."""
import numpy as np
import pytest

import ragged_scene as RS
from instantsfm_amd.synth import make_gp_problem, make_problem
from oracle import oracle as O


def _lengths_of(cam_idx, pt_idx, n_points):
    """distinct cameras per track"""
    ptr = RS.track_ptr(pt_idx, n_points)
    return np.array([np.unique(cam_idx[a:b]).size for a, b in zip(ptr[:-1], ptr[1:])])


def test_draw_lengths():
    n = RS.draw_lengths(1500, 139, 5, (128, 129, 135))
    assert np.array_equal(n, RS.draw_lengths(1500, 139, 5, (128, 129, 135)))
    assert not np.array_equal(n, RS.draw_lengths(1500, 139, 6, (128, 129, 135)))
    assert n.size == 1500 and n.min() == 2 and n.max() == 135
    assert all(np.count_nonzero(n == k) >= 1 for k in (128, 129, 135)) and np.count_nonzero(n > 61) == 3
    assert 0.25 < np.mean(n == 2) < 0.35          # the forced 30 % (2 + geometric is at least 3)
    assert 4.0 < np.mean(n[n <= 61]) < 5.5        # 0.3 * 2 + 0.7 * (2 + 4)
    assert RS.draw_lengths(400, 5, 1).max() == 5  # the cap


@pytest.mark.parametrize("model", (2, 0))
def test_dense_scene(model):
    C, planted = RS.dense_shape(model)
    lengths = RS.dense_lengths(model)
    a, b = RS.dense_problem(model), RS.dense_problem(model)
    for k in ("uv", "cam_idx", "pt_idx", "cams_init", "points_init"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    c = RS.dense_problem(model, seed=4)
    assert c.uv.shape != a.uv.shape or not np.array_equal(c.uv, a.uv)
    assert a.n_cams == C and a.n_points == RS.N_POINTS == lengths.size and a.model == model
    assert a.cam_idx.dtype == np.int32 and a.pt_idx.dtype == np.int32 and a.uv.shape == (a.cam_idx.size, 2)
    assert np.all(np.diff(a.pt_idx) >= 0) and np.array_equal(np.unique(a.pt_idx), np.arange(a.n_points))
    assert np.array_equal(_lengths_of(a.cam_idx, a.pt_idx, a.n_points), lengths)
    assert sorted(lengths)[-len(planted):] == sorted(planted)
    # cameras ascend inside a track; a repeat directly follows its original
    same = a.pt_idx[1:] == a.pt_idx[:-1]
    assert np.all(~same | (a.cam_idx[1:] >= a.cam_idx[:-1]))
    seen = np.bincount(a.cam_idx, minlength=C)
    assert seen[7] == 0 and np.all(np.delete(seen, 7) > 0)
    dup = RS.duplicates(a.cam_idx, a.pt_idx)
    n_long = np.repeat(lengths, np.diff(RS.track_ptr(a.pt_idx, a.n_points))) >= 3
    assert dup.sum() > 0 and not np.any(dup & ~n_long)
    assert 0.03 < dup.sum() / np.count_nonzero(n_long & ~dup) < 0.07
    assert np.all(np.abs(a.uv[dup] - a.uv[np.flatnonzero(dup) - 1]).max(axis=1) > 0)  # its own noise
    assert 8000 <= a.n_obs <= 9000
    # geometry and initial values are make_problem's
    base = make_problem(C, RS.N_POINTS, track_len=2, seed=3, model=model)
    for k in ("cams_gt", "cams_init", "pp", "points_gt", "points_init"):
        assert np.array_equal(getattr(a, k), getattr(base, k)), k
    # 0.5 px noise, 1 % outliers
    r, _, _ = O.evaluate(model, a.points_gt[a.pt_idx], a.cams_gt[a.cam_idx], a.pp[a.cam_idx], a.uv, want_jac=False)
    err = np.abs(r).max(axis=1)
    assert 0.005 < np.mean(err > 4.0) < 0.015 and 0.4 < np.std(r[err < 4.0]) < 0.6


def test_banded_scene():
    a = RS.banded_problem()
    assert np.array_equal(a.uv, RS.banded_problem().uv)
    C, w = 200, 30
    assert a.n_cams == C and np.all(np.diff(a.pt_idx) >= 0) and np.all(np.bincount(a.cam_idx, minlength=C) > 0)
    ptr = RS.track_ptr(a.pt_idx, a.n_points)
    lengths = _lengths_of(a.cam_idx, a.pt_idx, a.n_points)
    assert lengths.min() == 2 and sorted(lengths)[-2:] == [60, 61] and RS.duplicates(a.cam_idx, a.pt_idx).sum() > 0
    for s, e in zip(ptr[:-1], ptr[1:]):  # every track inside one window of 2 w + 1 consecutive cameras (mod C)
        c = np.unique(a.cam_idx[s:e])
        gaps = np.diff(np.concatenate([c, [c[0] + C]]))
        assert C - gaps.max() <= 2 * w
    with pytest.raises(ValueError):
        RS.make_ragged_problem(C, [62, 2], 0, window=w)
    with pytest.raises(ValueError):
        RS.make_ragged_problem(20, [1, 2], 0)


def test_gp_scene():
    g = RS.dense_gp_problem(init="perturbed", init_sigma=0.5)
    h = RS.dense_gp_problem(init="perturbed", init_sigma=0.5)
    assert np.array_equal(g.trans, h.trans) and np.array_equal(g.sfree, h.sfree)
    base = make_gp_problem(140, RS.N_POINTS, track_len=2, seed=3, depth_frac=0.3, init="perturbed", init_sigma=0.5)
    for k in ("fcam", "cams_gt", "points_gt", "cams_init", "points_init"):
        assert np.array_equal(getattr(g, k), getattr(base, k)), k
    assert np.array_equal(_lengths_of(g.cam_idx, g.pt_idx, g.n_points), RS.dense_lengths(0))
    assert np.bincount(g.cam_idx, minlength=140)[7] == 0 and RS.duplicates(g.cam_idx, g.pt_idx).sum() > 0
    assert np.all(np.diff(g.pt_idx) >= 0) and g.trans.shape == (g.n_obs, 3) == (g.cam_idx.size, 3)
    assert np.allclose(np.linalg.norm(g.trans, axis=1), 1.0, atol=1e-14)
    assert 0.25 < np.mean(g.sfree == 0) < 0.35
    depth = np.linalg.norm(g.points_gt[g.pt_idx] - g.cams_gt[g.cam_idx], axis=1)
    assert np.array_equal(g.scales_init, np.where(g.sfree == 0, 1.0 / depth, 1.0))
    ang = np.arccos(np.clip(np.sum(g.trans * (g.points_gt[g.pt_idx] - g.cams_gt[g.cam_idx]) / depth[:, None], 1), -1, 1))
    assert np.median(ang) < 0.004 and 0.003 < np.mean(ang > 0.03) < 0.015


def test_lin_runs_helper():
    pt = np.repeat(np.arange(6), [2, 130, 3, 100, 30, 2])
    assert np.array_equal(RS.lin_runs(pt, 6, 128), [0, 1, 2, 4, 6])
    assert np.array_equal(RS.lin_runs(np.repeat(np.arange(300), 1), 300, 128), [0, 128, 256, 300])


@pytest.mark.parametrize("family,model", [("dense", 2), ("dense", 6), ("banded", 2)])
@pytest.mark.parametrize("precond", (1, 2))
def test_oracle_steps_through(family, model, precond):
    p = RS.dense_problem(model) if family == "dense" else RS.banded_problem(model)
    ora = O.OracleBA(p.model, p.uv, p.cam_idx, p.pt_idx, p.pp, p.n_cams, p.n_points, precond=precond)
    c, q = p.cams_init.copy(), p.points_init.copy()
    losses = [ora.cost(c, q)[0]]
    for _ in range(3):
        losses.append(ora.step(c, q))
        st = ora.stats()
        assert st["failed"] == 0 and st["rejects"] == 0, st
    assert np.all(np.diff(losses) < 0)
    if family == "dense":  # the camera that sees nothing is left bit-for-bit alone
        assert np.array_equal(c[7], p.cams_init[7]) and not np.array_equal(c[8], p.cams_init[8])


def test_oracle_gp_steps_through():
    g = RS.dense_gp_problem(init="perturbed", init_sigma=0.5)
    ora = O.OracleGP(g.trans, g.cam_idx, g.pt_idx, g.fcam, g.sfree, g.n_cams, g.n_points, precond=1)
    c, q, s = g.cams_init.copy(), g.points_init.copy(), g.scales_init.copy()
    for _ in range(3):
        ora.step(c, q, s)
        st = ora.stats()
        assert st["failed"] == 0 and st["rejects"] == 0, st
    assert np.array_equal(c[7], g.cams_init[7])
