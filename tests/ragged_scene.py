"""Ragged test scenes: tracks of 2 to several hundred observations, a camera that sees nothing, duplicated
observations -- the shapes synth.make_problem / make_gp_problem never produce (every track `track_len` long, every
camera about equally busy).  Test helper only; used by test_ragged_scene.py, test_create_plan.py and test_gpu_ragged.py.

Geometry, intrinsics, initial perturbations and the noise law (0.5 px Gaussian, 1 % outliers; for global positioning
the angular ray noise) are make_problem's / make_gp_problem's: the base scene is drawn with the same camera count,
len(lengths) points and track_len=2, and only the observations (uv or rays, cam_idx, pt_idx) are replaced.  Every
ring camera sees the whole point ball, so any camera may observe any point.

Observations are track-major (pt_idx nondecreasing); inside a track the cameras ascend and a duplicated observation
(same camera, same track, its own noise) directly follows its original, which is the engine's local order, so debug
records compare with the oracle's index for index.
"""
import dataclasses

import numpy as np

from instantsfm_amd.synth import _project, make_gp_problem, make_problem

# the two scene families of the GPU tests (tests/test_gpu_ragged.py) and of the host plan test
N_POINTS = 1500
DENSE = dict(window=None, empty_cam=7, dup_frac=0.05)
DENSE_CAMS = {2: 270}       # SIMPLE_RADIAL (D = 8); every other model: 140 cameras
DENSE_PLANTED = {2: (127, 128, 129, 256, 257, 260)}
BANDED = dict(n_cams=200, window=30, empty_cam=None, dup_frac=0.05)
BANDED_PLANTED = (60, 61)


def draw_lengths(n_points, cap, seed, planted=()):
    """Track lengths 2 + geometric(0.25), 30 % forced to 2, capped at `cap`; `planted` overwrites the first entries
    and the list is then shuffled.  The minimum is 2."""
    rng = np.random.default_rng([seed, 11])
    n = 2 + rng.geometric(0.25, int(n_points))
    n[rng.uniform(size=n.size) < 0.3] = 2
    n = np.minimum(n, int(cap))
    n[:len(planted)] = planted
    assert n.min() >= 2 and n.max() <= cap
    return rng.permutation(n)


def _tracks(rng, C, lengths, dup_frac, empty_cam, window):
    """(cam_idx, pt_idx, is_dup) of the ragged observation list."""
    allowed = np.array([c for c in range(C) if c != empty_cam])
    cams, pts, dups = [], [], []
    for p, L in enumerate(np.asarray(lengths, dtype=np.int64)):
        if window is None:
            pool = allowed
        else:
            home = int(rng.integers(0, C))
            pool = (home + np.arange(-window, window + 1)) % C
            pool = np.unique(pool[pool != (-1 if empty_cam is None else empty_cam)])
        if L < 2 or L > pool.size:
            raise ValueError(f"track {p}: length {L} outside [2, {pool.size}]")
        c = np.sort(rng.choice(pool, int(L), replace=False))
        rep = np.ones(c.size, dtype=np.int64)
        if dup_frac > 0 and L >= 3:
            rep += rng.uniform(size=c.size) < dup_frac
        d = np.zeros(int(rep.sum()), dtype=bool)
        d[np.cumsum(rep)[rep == 2] - 1] = True  # the second of a repeated pair
        cams.append(np.repeat(c, rep))
        pts.append(np.full(d.size, p))
        dups.append(d)
    return (np.concatenate(cams).astype(np.int32), np.concatenate(pts).astype(np.int32), np.concatenate(dups))


def make_ragged_problem(n_cams, lengths, seed, model=2, dup_frac=0.0, empty_cam=None, window=None, noise_px=0.5,
                        outlier_frac=0.01):
    """BAProblem whose track p has lengths[p] distinct cameras (sorted): drawn uniformly from all cameras except
    `empty_cam` (window=None) or from {h-window..h+window} mod C around a random home camera h; `dup_frac` of the
    observations of tracks of length >= 3 are repeated."""
    base = make_problem(n_cams, len(lengths), track_len=2, seed=seed, model=model)
    rng = np.random.default_rng([seed, 12])
    cam_idx, pt_idx, _ = _tracks(rng, base.n_cams, lengths, dup_frac, empty_cam, window)
    uv, _ = _project(model, base.points_gt[pt_idx], base.cams_gt[cam_idx], base.pp[cam_idx])
    uv = uv + rng.normal(0, noise_px, uv.shape)
    n_out = int(round(outlier_frac * uv.shape[0]))
    if n_out:
        which = rng.choice(uv.shape[0], n_out, replace=False)
        uv[which] += rng.choice([-1.0, 1.0], (n_out, 2)) * rng.uniform(5, 20, (n_out, 2))
    return dataclasses.replace(base, uv=np.ascontiguousarray(uv), cam_idx=cam_idx, pt_idx=pt_idx)


def make_ragged_gp_problem(n_cams, lengths, seed, dup_frac=0.0, empty_cam=None, window=None, depth_frac=0.0,
                           ray_sigma=0.002, outlier_frac=0.01, **base_kw):
    """The GPProblem twin: make_gp_problem's cameras, points, factors and initial values (base_kw: init, init_sigma,
    ...), rays / scale flags / initial scales for the ragged observation list."""
    base = make_gp_problem(n_cams, len(lengths), track_len=2, seed=seed, **base_kw)
    rng = np.random.default_rng([seed, 13])
    cam_idx, pt_idx, _ = _tracks(rng, base.n_cams, lengths, dup_frac, empty_cam, window)
    v = base.points_gt[pt_idx] - base.cams_gt[cam_idx]
    depth = np.linalg.norm(v, axis=1)
    rays = v / depth[:, None]
    n = rays.shape[0]
    sig = np.full(n, ray_sigma)
    n_out = int(round(outlier_frac * n))
    if n_out:
        sig[rng.choice(n, n_out, replace=False)] = rng.uniform(0.05, 0.2, n_out)
    rays = rays + rng.normal(size=rays.shape) * sig[:, None]
    rays /= np.linalg.norm(rays, axis=1, keepdims=True)
    has_depth = rng.uniform(size=n) < depth_frac
    return dataclasses.replace(base, trans=np.ascontiguousarray(rays), cam_idx=cam_idx, pt_idx=pt_idx,
                               sfree=(~has_depth).astype(np.int32),
                               scales_init=np.ascontiguousarray(np.where(has_depth, 1.0 / depth, 1.0)))


def dense_shape(model):
    """(camera count, planted lengths) of the dense family for a camera model."""
    return DENSE_CAMS.get(model, 140), DENSE_PLANTED.get(model, (128, 129, 135))


def dense_lengths(model, seed=5):
    C, planted = dense_shape(model)
    return draw_lengths(N_POINTS, C - 1, seed, planted)  # (one camera sees nothing)


def dense_problem(model=2, seed=3, lengths_seed=5):
    """dense family: any camera but camera 7 may see any point, so every Schur row is nearly full; planted tracks on
    both sides of one and (D = 8) two linearize passes."""
    return make_ragged_problem(dense_shape(model)[0], dense_lengths(model, lengths_seed), seed, model=model, **DENSE)


def dense_gp_problem(seed=3, lengths_seed=5, depth_frac=0.3, **kw):
    return make_ragged_gp_problem(140, dense_lengths(0, lengths_seed), seed, depth_frac=depth_frac, **DENSE, **kw)


def banded_problem(model=2, seed=3, lengths_seed=5):
    """banded family: 200 cameras, tracks inside a window of 61, so rows keep <= 128 neighbours (persistent CG)."""
    kw = dict(BANDED)
    C = kw.pop("n_cams")
    return make_ragged_problem(C, draw_lengths(N_POINTS, 2 * kw["window"] + 1, lengths_seed, BANDED_PLANTED), seed,
                               model=model, **kw)


def track_ptr(pt_idx, n_points):
    """[P + 1] first observation of every track"""
    return np.searchsorted(np.asarray(pt_idx), np.arange(int(n_points) + 1))


def lin_runs(pt_idx, n_points, lin_threads):
    """The track runs k_lin_points / k_backsub_rc take one workgroup each (create_plan.h plan_lin_runs): a run is
    closed before a track that would take it past lin_threads tracks or observations.  Returns the run boundaries."""
    ptr = track_ptr(pt_idx, n_points)
    lb = [0]
    for p in range(int(n_points)):
        if p > lb[-1] and (ptr[p + 1] - ptr[lb[-1]] > lin_threads or p - lb[-1] >= lin_threads):
            lb.append(p)
    if n_points > 0:
        lb.append(int(n_points))
    return np.array(lb)


def duplicates(cam_idx, pt_idx):
    """mask of the observations that repeat their predecessor's (camera, track)"""
    cam_idx, pt_idx = np.asarray(cam_idx), np.asarray(pt_idx)
    d = np.zeros(cam_idx.size, dtype=bool)
    d[1:] = (cam_idx[1:] == cam_idx[:-1]) & (pt_idx[1:] == pt_idx[:-1])
    return d
