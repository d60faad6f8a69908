"""The scenes of the BA Schur-build-and-solve tests (test_ba_solve_reference.py, test_gpu_ba_solve.py), with their
cached references.  Test helper only.

Reused as they are: ragged_scene.dense_problem (rows split into chunks, an empty camera, duplicates, tracks past one
linearize pass; D = 7, 8, 9, 12, 16), ragged_scene.banded_problem (rows of <= 128 neighbours: the persistent CG),
wide_scene.wide_problem (strong distortion, Huber radius 30 px) and synth.make_problem(24, 600) ("uniform", CPU only).

New: `clamps` (models 2 and 4), the one scene whose damped diagonals reach the clamp from both sides.  12 ring cameras,
150 tracks of 2 to 9 cameras (5 % duplicated observations) from ragged_scene.make_ragged_problem, the world turned into
camera 0's initial frame (camera 0 starts at the identity rotation), and one planted track: its point sits PLANT_DEPTH
in front of camera 0 (seen also by cameras 5, 6 and 7 from across the ring).  Its x and y diagonal entries and camera
0's x and y translation entries are then all (focal / depth)^2 = 1.58e9 to within 2e-5 of each other (OPENCV: the y
pair, 1.62e9, 2 % above the x pair) and are the largest diagonal entries of the system, 34x the next one.  CLAMP_MAX
lies just below them and above everything else; CLAMP_MIN lies inside the bulk (camera entries run from 0.15 to 5e7,
point entries from 33 to 7.9e3).  Clamping from above takes something away from a positive semidefinite matrix whose
gauge directions are held up by the damping alone: a cut of 1e-3 already leaves the system indefinite at f = 1 + 1e-4.
So the cut stays inside f - 1: the entries above CLAMP_MAX lose 1.7e-5 .. 3.9e-5 of their size (more than 1e-6, so that
kernel and reference cannot take different branches), which the first trial's f more than restores.  check_clamps()
asserts all of it from the reference's report.  The planted track's projections cancel 30 against 30 down to 0.025, so
its rows of the reference come from mpmath.
"""
import dataclasses

import numpy as np

import ba_solve_reference as B
import ragged_scene as RS
import wide_scene as WS
from instantsfm_amd.synth import _project, _quat_mul, make_problem, quat_to_matrix

F1 = 1.0 + 1e-4     # the first trial's damping factor (1 + 1 / tr_radius): the factor the records are prepared for
F2 = 1.0 + 1.3e-2   # another factor at the same linearization: k_schur's RETRY form
F_VALUES = (F1, F2)

CLAMP_MODELS = (2, 4)
N_CAMS, N_TRACKS, SEED = 12, 150, 7
PLANT_DEPTH, PLANT_UV = 0.025, (0.05, -0.03)
PLANT_CAMS = (0, 5, 6, 7)
CLAMP_MIN = 3.0e3
CLAMP_MAX = {2: 1.58398e9, 4: 1.61582e9}

SETTINGS = dict(dense=dict(huber_delta=1.0), banded=dict(huber_delta=1.0), uniform=dict(huber_delta=1.0),
                wide=dict(huber_delta=WS.HUBER_DELTA))


def settings(name, model):
    """keyword arguments shared by the engine, the oracle and the reference: huber_delta, clamp_min, clamp_max"""
    if name == "clamps":
        return dict(huber_delta=1.0, clamp_min=CLAMP_MIN, clamp_max=CLAMP_MAX[model])
    return dict(SETTINGS[name], clamp_min=1e-6, clamp_max=1e32)


def clamps_problem(model):
    rng = np.random.default_rng([SEED, 31])
    lengths = rng.integers(2, 10, N_TRACKS)
    base = RS.make_ragged_problem(N_CAMS, np.append(lengths, 2), SEED, model=model, dup_frac=0.05)
    keep = base.pt_idx < N_TRACKS
    # turn the world into camera 0's initial frame (X -> Q X, R -> R Q^T, t as it is: every projection stays), so that
    # camera 0 starts at the identity rotation bit for bit and the world axes are its image axes
    q0 = base.cams_init[0, 3:7].copy()
    Q = quat_to_matrix(q0)
    conj = np.concatenate([-q0[:3], q0[3:]])
    cams_gt, cams_init = base.cams_gt.copy(), base.cams_init.copy()
    for cams in (cams_gt, cams_init):
        q = _quat_mul(cams[:, 3:7], conj[None, :])
        cams[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    cams_init[0, 3:7] = (0.0, 0.0, 0.0, 1.0)
    gt, pts = base.points_gt @ Q.T, base.points_init @ Q.T
    # the planted point: (u z, v z, z) in camera 0's frame at its initial pose, X = p_c - t_0
    X = np.array([PLANT_UV[0] * PLANT_DEPTH, PLANT_UV[1] * PLANT_DEPTH, PLANT_DEPTH]) - cams_init[0, 0:3]
    gt[N_TRACKS] = pts[N_TRACKS] = X
    seen = np.array(PLANT_CAMS, dtype=np.int32)
    uv, _ = _project(model, np.tile(X, (seen.size, 1)), cams_init[seen], base.pp[seen])
    uv = uv + rng.normal(0, 0.2, uv.shape)
    return dataclasses.replace(base, cams_gt=cams_gt, cams_init=cams_init, points_gt=np.ascontiguousarray(gt),
                               points_init=np.ascontiguousarray(pts),
                               uv=np.ascontiguousarray(np.concatenate([base.uv[keep], uv])),
                               cam_idx=np.concatenate([base.cam_idx[keep], seen]).astype(np.int32),
                               pt_idx=np.concatenate([base.pt_idx[keep], np.full(seen.size, N_TRACKS)]).astype(np.int32))


_BUILD = dict(dense=RS.dense_problem, banded=RS.banded_problem, wide=WS.wide_problem, clamps=clamps_problem,
              uniform=lambda model: make_problem(24, 600, seed=11, model=model))
_cache = {}
KEEP_SYSTEMS = 3


def problem(name, model):
    if ("problem", name, model) not in _cache:
        _cache["problem", name, model] = _BUILD[name](model)
    return _cache["problem", name, model]


def observed(name, model, point=None):
    """ba_solve_reference.observe at the scene's initial parameters, or at `point` = (tag, cams, pts): another
    linearization point, cached under its tag"""
    key = ("obs", name, model, None if point is None else point[0])
    if key not in _cache:
        p = problem(name, model)
        cams, pts = (p.cams_init, p.points_init) if point is None else point[1:]
        # the planted track's projections cancel 30 against 30 down to a depth of 0.025: those rows come from mpmath
        mask = (p.pt_idx == N_TRACKS) if name == "clamps" else None
        _cache[key] = B.observe(p, cams, pts, settings(name, model)["huber_delta"], mask)
    return _cache[key]


def system(name, model, f, mutate=None, point=None):
    """the reduced reference system for damping factor f at the initial parameters (or at `point`, as observed()),
    cached per process and shared by det, precond and the tests: the last KEEP_SYSTEMS of them, so callers walk the
    cases scene by scene, model by model"""
    key = ("sys", name, model, float(f), mutate, None if point is None else point[0])
    if key in _cache:
        _cache[key] = _cache.pop(key)                  # most recently used last
    else:
        kw = settings(name, model)
        _cache[key] = B.reduce(observed(name, model, point), f, clamp_min=kw["clamp_min"], clamp_max=kw["clamp_max"],
                               mutate=mutate)
        held = [k for k in _cache if k[0] == "sys"]
        for k in held[:-KEEP_SYSTEMS]:                 # a dense S and its |terms| are 160 MB at D = 16: keep a few
            del _cache[k]
    return _cache[key]


def check_clamps(sys_):
    """what the clamps scene is for, from the reference's report: camera-diagonal and point-diagonal entries below
    clamp_min and above clamp_max, plenty strictly between, none within 1e-6 (relative) of a threshold, and the
    clamped system still positive definite"""
    model = {8: 2, 12: 4}[sys_.gc.shape[1]]
    lo, hi = CLAMP_MIN, CLAMP_MAX[model]
    dc, dp = sys_.diag_c.astype(np.float64), sys_.diag_p.astype(np.float64)
    assert sys_.below_c.sum() >= 1 and sys_.below_p.sum() >= 1 and sys_.above_c.sum() >= 1 and sys_.above_p.sum() >= 1
    assert np.array_equal(sys_.below_c, dc < lo) and np.array_equal(sys_.above_p, dp > hi)
    between_c = ~sys_.below_c & ~sys_.above_c
    between_p = ~sys_.below_p & ~sys_.above_p
    assert between_c.sum() >= 24 and between_p.sum() >= 50, (between_c.sum(), between_p.sum())
    every = np.concatenate([dc.ravel(), dp.ravel()])
    for t in (lo, hi):
        assert np.abs(every / t - 1.0).min() > 1e-6, (t, np.abs(every / t - 1.0).min())
    # the cut from above stays inside the first trial's damping, so the damped diagonal is no smaller than the plain one
    assert every.max() / hi - 1.0 < F1 - 1.0
    assert sys_.spd and sys_.spd_points and np.isfinite(sys_.dc_resid)
    lengths = np.bincount(np.asarray(sys_.pt), minlength=dp.shape[0])
    assert lengths.min() >= 2 and 9 <= lengths.max() <= 12
    return dict(below_c=int(sys_.below_c.sum()), above_c=int(sys_.above_c.sum()), below_p=int(sys_.below_p.sum()),
                above_p=int(sys_.above_p.sum()), between_c=int(between_c.sum()), between_p=int(between_p.sum()))
