"""Two seeded global-positioning scenes built for the branches and loop edges of csrc/ba_gp.h.  Test helper only.

edges   19 cameras (two whose sum of squared position-Jacobian entries stays below clamp_min, one that sees nothing),
        64 tracks, the whole scene offset by 1e3 so that X - c cancels three digits.  Observation classes, each with
        both camera factors (1 and 0.5): |r| bit-for-bit 0 (dyadic coordinates and scales), |r| in [0.999, 1) delta,
        in [1, 1.001] delta and at 1e3 delta; free scales whose undamped diagonal is in [0.9, 1) and [1, 1.1] times
        clamp_min, at 1e-2 times it and exactly 0 (X_p == c_i bit for bit); negative scales, free and fixed.  Track
        classes: point diagonal far below clamp_min (scales ~1e-4), and one track on each side of it; all-fixed,
        all-free and mixed tracks of lengths 1, 2, 7, 8, 9, 15, 16 and 17 (the lane-group boundaries of the per-track
        kernels); duplicated observations (the 17-long tracks see one of the 16 regular cameras twice).
counts  12 cameras, 769 tracks: camera k sees the first n_k tracks, n = 0, 1, 255, 256, 257, 511, 512, 513, 768, 769
        (the rounds of the per-camera loops: 256 threads, two records in flight), two more cameras see every track (one
        per camera factor); about 30 % of the scales are fixed.

check_edges / check_counts assert every class from the reference's own report (gp_reference.observations / reduce:
the branch taken, the undamped diagonals), never from the constants the scenes were built with, so a later change of
those constants cannot hollow the scenes out.  Within a track the observations are sorted by camera, so the library's
track order is the caller's order and per-observation records compare index by index.

observed() / reduced() cache the reference per process: test_gp_reference.py and test_gpu_gp_edges.py share them.
"""
import numpy as np

import gp_reference as G
from instantsfm_amd.synth import GPProblem

DELTA = 0.1            # TorchGP's Huber threshold (GLOBAL_POSITIONER_OPTIONS['thres_loss_function'])
CLAMP_MIN = 1e-6       # the LM's diagonal clamp (pypose TrustRegion min=1e-6), LM_DEFAULTS["clamp_min"]
OFFSET = np.array([1000.0, -1000.0, 1000.0])
LENGTHS = (1, 2, 7, 8, 9, 15, 16, 17)
COUNTS = (0, 1, 255, 256, 257, 511, 512, 513, 768, 769)
FACTORS = (1.0, 0.5)
F_VALUES = (1.001, 1.5)
MAGNITUDE = dict(zero=0.0, inside=0.3, in_edge=0.9995, out_edge=1.0005, far=1e3, outside=3.0)   # |r| / delta
DYADIC_SCALES = (1.0, 0.5, 0.25, 0.75, -0.5, 1.5)


def _unit(rng):
    d = rng.normal(size=3)
    return d / np.linalg.norm(d)


def _pack(C, fcam, cams, tracks):
    """tracks: list of (X, [(camera, free, scale, ray)]) -> GPProblem, observations sorted by camera inside a track"""
    trans, cam_idx, pt_idx, sfree, scales, pts = [], [], [], [], [], []
    for p, (X, obs) in enumerate(tracks):
        pts.append(X)
        for c, free, s, t in sorted(obs, key=lambda q: q[0]):      # (stable: duplicates keep their order)
            trans.append(t); cam_idx.append(c); pt_idx.append(p); sfree.append(int(free)); scales.append(s)
    cams, pts = np.ascontiguousarray(cams, dtype=np.float64), np.ascontiguousarray(pts, dtype=np.float64)
    return GPProblem(np.ascontiguousarray(trans, dtype=np.float64), np.array(cam_idx, np.int32), np.array(pt_idx, np.int32),
                     np.ascontiguousarray(fcam, dtype=np.float64), np.array(sfree, np.int32), cams.copy(), pts.copy(),
                     cams, pts, np.array(scales, np.float64))


def _ray(rng, fcam, cams, X, c, s, kind):
    """the ray that makes the residual of (camera c, point X, scale s) a vector of length MAGNITUDE[kind] * delta"""
    e = X - cams[c]
    if kind == "zero":
        return s * e              # exact for dyadic s and e: the residual is bit-for-bit 0
    return s * e + _unit(rng) * (MAGNITUDE[kind] * DELTA / fcam[c])


def edges_problem(seed=11):
    rng = np.random.default_rng(seed)
    C, REG = 19, 16                # cameras 0..15 regular, 16 / 17 tiny (factor 1 / 0.5), 18 sees nothing
    fcam = np.where(np.arange(C) % 2 == 0, 1.0, 0.5)
    cams = OFFSET + rng.permutation(65 ** 3)[:C, None] // np.array([1, 65, 65 * 65]) % 65 / 8.0 - 4.0   # dyadic, distinct
    tracks = []
    kinds = ("inside", "zero", "in_edge", "out_edge", "far", "outside", "inside")
    count = [0]

    def point(jitter):
        X = OFFSET + rng.integers(-16, 17, 3) / 8.0
        return X + rng.normal(0, 0.05, 3) if jitter else X

    def generic(cam_list, free_list, jitter):
        X = point(jitter)
        obs = []
        for c, free in zip(cam_list, free_list):
            kind = kinds[count[0] % len(kinds)]
            count[0] += 1
            if jitter and kind == "zero":
                kind = "inside"
            s = DYADIC_SCALES[int(rng.integers(len(DYADIC_SCALES)))]
            obs.append((int(c), bool(free), s, _ray(rng, fcam, cams, X, c, s, kind)))
        tracks.append((X, obs))

    # all-fixed, all-free and mixed tracks at the lane-group boundaries; 17 observations on 16 cameras: one twice
    for L in LENGTHS:
        for mode in ("fixed", "free", "mixed"):
            if L == 1 and mode == "mixed":
                continue
            cl = np.sort(rng.permutation(REG)[:min(L, REG)])
            if L > REG:
                cl = np.sort(np.concatenate([cl, rng.integers(0, REG, L - REG)]))
            fl = dict(fixed=np.zeros(L, bool), free=np.ones(L, bool), mixed=np.arange(L) % 3 != 1)[mode]
            generic(cl, fl, jitter=(len(tracks) % 2 == 1))
    # free scales around the clamp: the point sits next to (or on) camera c
    for target in (0.95, 1.05, 1e-2, 0.0):
        for c in (2, 3):
            X = cams[c] + _unit(rng) * (np.sqrt(target * CLAMP_MIN) / fcam[c])
            obs = [(c, True, 1.0, 1.0 * (X - cams[c]) + _unit(rng) * (0.3 * DELTA / fcam[c]))]
            for c2, free in ((int(rng.integers(4, 10)), False), (int(rng.integers(10, 16)), True)):
                obs.append((c2, free, 0.5, _ray(rng, fcam, cams, X, c2, 0.5, "inside")))
            tracks.append((X, obs))
    # tracks (and cameras 16, 17) whose position diagonal stays far below clamp_min: scales around 1e-4
    for L in (2, 3, 5, 8, 9, 4):
        X = point(True)
        cl = [16, 17] + list(rng.permutation(REG)[:L - 2])
        obs = []
        for k, c in enumerate(cl):
            s = (1e-4 if k % 3 else -1e-4) * (1.0 + 0.5 * rng.uniform())
            kind = ("inside", "outside", "in_edge", "out_edge")[k % 4]
            obs.append((int(c), k % 2 == 0, s, _ray(rng, fcam, cams, X, c, s, kind)))
        tracks.append((X, obs))
    # one track on each side of clamp_min: four inside observations with (f s)^2 = target * clamp_min / 4
    for target in (0.95, 1.05):
        X = point(True)
        obs = []
        for k, c in enumerate(np.sort(rng.permutation(REG)[:4])):
            s = np.sqrt(target * CLAMP_MIN / 4.0) / fcam[c]
            obs.append((int(c), k % 2 == 0, s, _ray(rng, fcam, cams, X, c, s, "inside")))
        tracks.append((X, obs))
    # filler: short mixed tracks that tie the regular cameras together; the last sees one camera twice
    while len(tracks) < 64:
        L = int(rng.integers(3, 7))
        cl = np.sort(rng.permutation(REG)[:L])
        if len(tracks) == 63:
            cl[1] = cl[0]
        generic(cl, rng.uniform(size=L) < 0.6, jitter=True)
    return _pack(C, fcam, cams, tracks)


def counts_problem(seed=12):
    rng = np.random.default_rng(seed)
    C, P = 12, 769
    n_seen = list(COUNTS) + [P, P]
    fcam = np.where(np.arange(C) % 2 == 0, 1.0, 0.5)          # cameras 10 / 11: factor 1 / 0.5
    ang = 2 * np.pi * np.arange(C) / C
    centers = np.stack([30 * np.cos(ang), 30 * np.sin(ang), rng.uniform(-2, 2, C)], axis=1)
    d = rng.normal(size=(P, 3))
    points = d / np.linalg.norm(d, axis=1, keepdims=True) * (8.0 * rng.uniform(0, 1, (P, 1)) ** (1.0 / 3.0))
    tracks = []
    for p in range(P):
        obs = []
        for c in range(C):
            if p >= n_seen[c]:
                continue
            v = points[p] - centers[c]
            depth = np.linalg.norm(v)
            ray = v / depth + rng.normal(size=3) * (0.1 if rng.uniform() < 0.15 else 0.002)
            fixed = rng.uniform() < 0.3
            obs.append((c, not fixed, (1.0 if fixed else 1.0 + rng.normal(0, 0.003)) / depth, ray / np.linalg.norm(ray)))
        tracks.append((points[p] + rng.normal(0, 0.05, 3), obs))
    return _pack(C, fcam, centers + rng.normal(0, 0.05, (C, 3)), tracks)


# ------------------------------------------------------------------------------------------------------------
# the cached reference
# ------------------------------------------------------------------------------------------------------------
_BUILD = dict(edges=edges_problem, counts=counts_problem)
_KIND = dict(edges="mp", counts="ld")         # counts: longdouble sums over the mp per-observation terms
_cache = {}


def problem(name):
    if ("problem", name) not in _cache:
        _cache["problem", name] = _BUILD[name]()
    return _cache["problem", name]


def observed(name):
    """gp_reference.observations at the scene's initial parameters"""
    if ("obs", name) not in _cache:
        p = problem(name)
        _cache["obs", name] = G.observations(p, p.cams_init, p.points_init, p.scales_init, DELTA)
    return _cache["obs", name]


def reduced(name, f, mutate=None):
    key = ("red", name, float(f), mutate)
    if key not in _cache:
        _cache[key] = G.reduce(observed(name), f, clamp_min=CLAMP_MIN, kind=_KIND[name], mutate=mutate)
    return _cache[key]


def track_ptr(prob):
    return np.searchsorted(prob.pt_idx, np.arange(prob.n_points + 1))


# ------------------------------------------------------------------------------------------------------------
# what the scenes are for, asserted from the reference's report
# ------------------------------------------------------------------------------------------------------------
def _f64(a):
    return G.split(a)[0]


def _sorted_by_camera(prob):
    same = prob.pt_idx[1:] == prob.pt_idx[:-1]
    return bool(np.all(np.diff(prob.pt_idx) >= 0) and np.all(prob.cam_idx[1:][same] >= prob.cam_idx[:-1][same]))


def check_edges(prob, obs, red):
    """every class of the edges scene, from obs (branch, |r|) and red (undamped diagonals, clamp flags)"""
    assert _sorted_by_camera(prob)
    fac = prob.fcam[prob.cam_idx]
    free = obs.free

    def both(mask):
        return all(np.any(mask & (fac == v)) for v in FACTORS)

    rs = _f64(obs.rs) / obs.delta
    assert both(obs.huber == G.ZERO) and np.all(_f64(obs.rs)[obs.huber == G.ZERO] == 0.0)
    assert both((obs.huber == G.INSIDE) & (rs >= 0.999) & (rs < 1.0))
    assert both((obs.huber == G.OUTSIDE) & (rs >= 1.0) & (rs <= 1.001))
    assert both((obs.huber == G.OUTSIDE) & (np.abs(rs / 1e3 - 1.0) < 1e-9))
    assert both(free & (obs.huber == G.OUTSIDE)) and both(~free & (obs.huber == G.OUTSIDE))
    q = _f64(red.sdiag) / CLAMP_MIN                  # a free scale's undamped diagonal over clamp_min
    assert both(free & red.hss_clamped & (q >= 0.9) & (q < 1.0))
    assert both(free & ~red.hss_clamped & (q >= 1.0) & (q <= 1.1))
    assert both(free & red.hss_clamped & (q > 0.5e-2) & (q < 2e-2))
    assert both(free & red.hss_clamped & (q == 0.0))
    coincide = np.all(prob.points_init[prob.pt_idx] == prob.cams_init[prob.cam_idx], axis=1)
    assert np.array_equal(coincide, free & (q == 0.0))
    assert both(free & (prob.scales_init < 0)) and both(~free & (prob.scales_init < 0))
    # tracks
    dp = _f64(red.diag_p)[:, 0] / CLAMP_MIN
    assert np.sum(red.clamped_p & (dp < 0.3)) >= 6 and np.array_equal(red.clamped_p, dp < 1.0)
    assert np.sum((dp >= 0.9) & (dp < 1.0)) == 1 and np.sum((dp >= 1.0) & (dp <= 1.1)) == 1
    ptr = track_ptr(prob)
    seen = set()
    for p in range(prob.n_points):
        fr = free[ptr[p]:ptr[p + 1]]
        seen.add((fr.size, "free" if fr.all() else ("mixed" if fr.any() else "fixed")))
    for L in LENGTHS:
        for mode in ("fixed", "free") + (("mixed",) if L > 1 else ()):
            assert (L, mode) in seen, (L, mode)
    dup = (prob.cam_idx[1:] == prob.cam_idx[:-1]) & (prob.pt_idx[1:] == prob.pt_idx[:-1])
    assert dup.sum() >= 3
    # cameras: two with a clamped diagonal that do see something (one per factor), one that sees nothing
    n_obs = np.bincount(prob.cam_idx, minlength=prob.n_cams)
    dc = _f64(red.diag_c)[:, 0] / CLAMP_MIN
    assert np.array_equal(red.clamped_c, dc < 1.0)
    for v in FACTORS:
        assert np.any(red.clamped_c & (n_obs >= 4) & (prob.fcam == v))
    assert np.sum(n_obs == 0) == 1 and np.sum(~red.clamped_c) >= 16
    # the offset: every position is ~1e3 from the origin while the scene itself is a few units across
    assert np.abs(prob.cams_init).min() > 900 and np.abs(prob.points_init).min() > 900
    assert np.ptp(prob.points_init, axis=0).max() < 20


def check_counts(prob, obs, red):
    assert _sorted_by_camera(prob)
    n_obs = np.bincount(prob.cam_idx, minlength=prob.n_cams)
    assert prob.n_cams == 12 and prob.n_points == 769
    assert tuple(n_obs[:10]) == COUNTS and n_obs[10] == n_obs[11] == 769 and prob.fcam[10] != prob.fcam[11]
    for c in range(10):                                  # camera k sees the FIRST n_k tracks
        assert np.array_equal(np.sort(prob.pt_idx[prob.cam_idx == c]), np.arange(COUNTS[c]))
    assert 0.25 < np.mean(~obs.free) < 0.35
    assert 0.01 < np.mean(obs.huber == G.OUTSIDE) < 0.5 and not np.any(obs.huber == G.ZERO)
    assert not red.hss_clamped.any() and not red.clamped_p.any()
    assert np.array_equal(red.clamped_c, n_obs == 0)
