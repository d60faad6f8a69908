"""Scenes for the image-pair inlier tests (ImagePairInliersCount): named, seeded sets of image pairs with synthetic
two-view geometry.  tools/gen_golden.py --only inliers runs the reference on the same scenes and records what it does
(tests/golden/pair_inliers_golden.npz), so this file is the single definition of their inputs.

Every pair owns its two images (2p, 2p + 1) and one PINHOLE-like camera per image (SIMPLE_PINHOLE, pp = (1000, 750)).
Pixel features are the projections of random points (0.5 px noise, a share of random wrong partners) plus a few
unmatched ones, shuffled; ``features_undist`` are the unit rays of the stored pixels through the camera.  ``scene``
asserts that no comparison the scoring makes on these inputs is within 1e-9 (relative, pair_inliers.host_scores'
margin) of flipping, and moves on to the next seed otherwise: exact equality of inlier sets between two float64
implementations is only meaningful away from rounding.  That is a condition on the inputs, not a tolerance on results.
"""
import functools
import os
from dataclasses import dataclass

import numpy as np

from instantsfm_amd import pair_inliers as PI
from instantsfm_amd import synth as S
from instantsfm_amd.config.colmap import INLIER_THRESHOLD_OPTIONS as OPTIONS
from instantsfm_amd.scene import defs as D

PP = np.array([1000.0, 750.0])
SIZE = np.array([2000.0, 1500.0])
MIN_MARGIN = 1e-9
E, F, H = 2, 3, 4                      # ConfigurationType values of the three scored kinds
SPECIAL_SIZES = (0, 1, 63, 64, 65, 129, 5000)
NAMES = ("general_f32", "general_f64", "f_cases", "e_cases")


@dataclass
class Scene:
    xy: list        # per image [n, 2] pixel features
    rays: list      # per image [n, 3] features_undist
    focal: list     # per image (= per camera) focal length
    pairs: list     # dicts: i1, i2, config, valid, matches [m, 2] uint32, F, H, rotation, translation, inliers


def _K(f):
    return np.array([[f, 0, PP[0]], [0, f, PP[1]], [0, 0, 1.0]])


def _hom(x):
    return np.concatenate([x, np.ones((x.shape[0], 1))], axis=1)


def two_view(rng, n, f1=1000.0, f2=1000.0, t=None, planar=False, noise=0.5, outliers=0.2, behind=0, far=0, center=0,
             shift=0.0, rot_sigma=0.08):
    """n matched pixels of two views: image 2 sees x2 ~ R x1 + t (|t| = 1, depths 4-12, R a random rotation of
    ``rot_sigma`` radians per axis).  ``planar`` puts the points
    on one plane; the first ``behind`` points lie behind both cameras, the next ``far`` at depth 500, the first
    ``center`` within 30 px of the principal point; ``shift`` moves every x2 that far off its epipolar line (planar:
    off its position).  Returns (x1, x2, geometry)."""
    q = S._quat_from_rotvec(rng.normal(0, rot_sigma, 3))
    R = S.quat_to_matrix(q)
    t = rng.normal(size=3) * [1, 1, 0.3] if t is None else np.asarray(t, dtype=np.float64)
    t = t / np.linalg.norm(t)
    x1 = rng.uniform([200, 150], [1800, 1350], (n, 2))
    x1[:center] = PP + rng.uniform(-30, 30, (center, 2))
    r1 = _hom((x1 - PP) / f1)
    normal, dist = np.array([0.1, -0.05, 1.0]) / np.linalg.norm([0.1, -0.05, 1.0]), 8.0
    if planar:
        z = dist / (r1 @ normal)
    else:
        z = rng.uniform(4, 12, n)
        z[:behind] *= -1
        z[behind:behind + far] = 500.0
    X2 = (r1 * z[:, None]) @ R.T + t
    x2 = X2[:, :2] / X2[:, 2:] * f2 + PP
    x1 = x1 + rng.normal(0, noise, x1.shape)
    x2 = x2 + rng.normal(0, noise, x2.shape)
    out = rng.uniform(size=n) < outliers
    x2[out] = rng.uniform([0, 0], SIZE, (int(out.sum()), 2))
    Emat = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
    Fmat = np.linalg.inv(_K(f2)).T @ Emat @ np.linalg.inv(_K(f1))
    Hmat = _K(f2) @ (R + np.outer(t, normal) / dist) @ np.linalg.inv(_K(f1))
    if shift:
        line = _hom(x1) @ Fmat.T
        x2 = x2 + shift * (np.array([[1.0, 0.0]]) if planar else line[:, :2] / np.linalg.norm(line[:, :2], axis=1,
                                                                                             keepdims=True))
    return x1, x2, dict(F=Fmat, H=Hmat, rotation=q, translation=t, focal=(f1, f2))


class _Builder:
    def __init__(self, rng, dtype=np.float32, ray_dtype=np.float64):
        self.rng, self.dtype, self.ray_dtype = rng, dtype, ray_dtype
        self.sc = Scene([], [], [], [])

    def add(self, config, x1, x2, geo, valid=True, inliers=None, extra=4):
        """Store the matched pixels as two new images (with ``extra`` unmatched features each, shuffled) and the pair
        with its matches in random order."""
        rng, n = self.rng, x1.shape[0]
        cols = []
        for x, f in ((x1, geo['focal'][0]), (x2, geo['focal'][1])):
            feats = np.concatenate([x, rng.uniform([0, 0], SIZE, (extra, 2))]).astype(self.dtype)
            slot = rng.permutation(n + extra)
            stored = np.empty_like(feats)
            stored[slot] = feats
            r = _hom((stored.astype(np.float64) - PP) / f)
            self.sc.xy.append(stored)
            self.sc.rays.append((r / np.linalg.norm(r, axis=1, keepdims=True)).astype(self.ray_dtype))
            self.sc.focal.append(float(f))
            cols.append(slot[:n])
        order = rng.permutation(n)
        i1 = len(self.sc.xy) - 2
        self.sc.pairs.append(dict(i1=i1, i2=i1 + 1, config=int(config), valid=bool(valid),
                                  matches=np.stack(cols, 1)[order].astype(np.uint32), F=geo['F'], H=geo['H'],
                                  rotation=geo['rotation'], translation=geo['translation'], inliers=inliers))

    def add_kind(self, config, n, **kw):
        f1, f2 = self.rng.uniform(800, 1300, 2)
        x1, x2, geo = two_view(self.rng, n, f1=f1, f2=f2, planar=config >= H, **kw)
        self.add(config, x1, x2, geo)


def _general(seed, n_pairs, dtype, ray_dtype, sizes):
    """Pairs of 15-40 matches, kinds H (configs 4, 5, 6), F, E and skipped ones (configs 0, 1, 7, 8 on valid pairs)
    interleaved at random; among them, per kind, one pair of each of ``sizes``, an all-inlier and a no-inlier pair."""
    rng = np.random.default_rng(seed)
    b = _Builder(rng, dtype, ray_dtype)
    todo = [(c, dict(n=n)) for c in (E, F, H) for n in sizes]
    todo += [(c, dict(n=30, noise=0.0, outliers=0.0)) for c in (E, F, H)]
    todo += [(c, dict(n=30, shift=50.0)) for c in (E, F, H)]
    where = dict(zip(sorted(rng.choice(n_pairs, len(todo), replace=False).tolist()), todo))
    for p in range(n_pairs):
        if p in where:
            config, kw = where[p]
            b.add_kind(config, **kw)
            continue
        config = int(rng.choice([E, E, E, F, F, 4, 5, 6, 0, 1, 7, 8]))
        b.add_kind(config, int(rng.integers(15, 41)))
    return b.sc


def _reflect_through_epipole(x2, Fmat):
    """x2 mirrored through the epipole of image 2: on the same epipolar line, opposite orientation."""
    e2 = np.linalg.svd(Fmat.T)[2][-1]
    return 2 * e2[:2] / e2[2] - x2


def _f_cases(seed):
    rng = np.random.default_rng(seed)
    b = _Builder(rng)
    # 0, 1: one geometry under F and -F -- every orientation vote flips, so one of the two has a negative majority
    x1, x2, geo = two_view(rng, 40, t=[1, 0.2, 0.5])
    b.add(F, x1, x2, geo)
    b.add(F, x1, x2, dict(geo, F=-geo['F']))
    # 2: an exact tie -- 12 exact matches and their mirror images through the epipole
    x1, x2, geo = two_view(rng, 13, t=[1, 0.2, 0.5], noise=0.0, outliers=0.0)
    mirrored = _reflect_through_epipole(x2, geo['F'])
    b.add(F, np.concatenate([x1[:12], x1[:12]]), np.concatenate([x2[:12], mirrored[:12]]), geo,
          inliers=np.array([5, 3, 1]))
    # 3: the same with one more mirrored match: the majority is on the mirrored side
    b.add(F, np.concatenate([x1[:12], x1]), np.concatenate([x2[:12], mirrored]), geo)
    # 4: no pre-inlier at all (every x2 50 px off its line); pre-set inliers must survive
    x1, x2, geo = two_view(rng, 25, shift=50.0, outliers=0.0)
    b.add(F, x1, x2, geo, inliers=np.array([2, 7]))
    # 5: first column of F zero -- every signum is exactly 0 and counts as negative
    x1 = rng.uniform([200, 150], [1800, 1350], (20, 2))
    F0 = rng.normal(size=(3, 3)) * [0.0, 1e-3, 1.0]
    line = _hom(x1) @ F0.T                                  # x2 on its line: (u, -(l0 u + l2) / l1)
    u = rng.uniform(0, 2000, 20)
    x2 = np.stack([u, -(line[:, 0] * u + line[:, 2]) / line[:, 1]], 1)
    b.add(F, x1, x2, dict(geo, F=F0))
    # 6: the epipole fallback -- F scaled so that no component of cross(F[0], F[1]) exceeds 1e-6
    x1, x2, geo = two_view(rng, 35)
    scale = 1e-4 / np.sqrt(np.abs(np.cross(geo['F'][0], geo['F'][1])).max())
    b.add(F, x1, x2, dict(geo, F=geo['F'] * scale))
    # 7: a zero F -- every r2 is 0 / 0
    b.add(F, x1, x2, dict(geo, F=np.zeros((3, 3))), inliers=np.array([1, 2, 3]))
    return b.sc


def _e_cases(seed):
    rng = np.random.default_rng(seed)
    b = _Builder(rng)
    # 0: translation pointing backwards (epipole12[2] < 0)
    x1, x2, geo = two_view(rng, 40, t=[0.3, 0.1, -1.0])
    b.add(E, x1, x2, geo)
    # 1: cheirality -- 10 points behind both cameras, 6 beyond the maximal depth
    x1, x2, geo = two_view(rng, 45, behind=10, far=6, outliers=0.1)
    b.add(E, x1, x2, geo)
    # 2: forward motion, 12 points within 3 degrees of the epipole
    x1, x2, geo = two_view(rng, 45, t=[0.0, 0.0, 1.0], center=12, outliers=0.1, rot_sigma=0.01)
    b.add(E, x1, x2, geo)
    # 3: two cameras of different focal length
    x1, x2, geo = two_view(rng, 40, f1=800.0, f2=1300.0)
    b.add(E, x1, x2, geo)
    # 4: the wrong sign of t: every match fails check_cheirality
    x1, x2, geo = two_view(rng, 30)
    b.add(E, x1, x2, dict(geo, translation=-geo['translation']))
    # 5, 6: an invalid pair and a valid pair of config UNDEFINED, each with pre-set inliers that must survive
    b.add(E, x1, x2, geo, valid=False, inliers=np.array([4, 2, 9]))
    b.add(0, x1, x2, geo, inliers=np.array([8, 1]))
    # 7: a homography pair with its own focal lengths
    x1, x2, geo = two_view(rng, 33, f1=900.0, f2=1100.0, planar=True)
    b.add(6, x1, x2, geo)
    return b.sc


def build(name, seed):
    if name == "general_f32":
        return _general(seed, 2000, np.float32, np.float64, SPECIAL_SIZES)
    if name == "general_f64":
        return _general(seed, 150, np.float64, np.float32, (0, 1, 64, 65))
    if name == "f_cases":
        return _f_cases(seed)
    if name == "e_cases":
        return _e_cases(seed)
    raise KeyError(name)


def as_objects(sc, defs=D):
    """(view_graph, cameras, images) of a scene in the classes of ``defs`` (this package's, or the reference's)."""
    cameras = [defs.Camera(id=i, model_id=defs.CameraModelId.SIMPLE_PINHOLE, width=2000, height=1500,
                           params=np.array([f, PP[0], PP[1]])) for i, f in enumerate(sc.focal)]
    images = [defs.Image(id=i, cam_id=i, is_registered=True, features=xy.copy(), features_undist=rays.copy())
              for i, (xy, rays) in enumerate(zip(sc.xy, sc.rays))]
    vg = defs.ViewGraph()
    for p in sc.pairs:
        pair = defs.ImagePair(image_id1=p['i1'], image_id2=p['i2'], is_valid=p['valid'], F=p['F'].copy(),
                              H=p['H'].copy(), rotation=p['rotation'].copy(), translation=p['translation'].copy(),
                              inliers=None if p['inliers'] is None else p['inliers'].copy(),
                              config=defs.ConfigurationType(p['config']))
        pair.matches = p['matches'].copy()
        vg.image_pairs[defs.Ids2PairId(p['i1'], p['i2'])] = pair
    return vg, cameras, images


@functools.lru_cache(maxsize=None)
def scene(name):
    """The named scene: the first seed (name's index, then + 100, + 200 ...) whose margins are all >= MIN_MARGIN."""
    for attempt in range(20):
        sc = build(name, NAMES.index(name) + 100 * attempt)
        if host(sc)[1][4].min() >= MIN_MARGIN:
            return sc
    raise AssertionError(f"no seed of scene {name} keeps every comparison {MIN_MARGIN} away from rounding")


def host(sc):
    """(flat arrays, host_scores result) of a scene."""
    flat = PI.flatten(*as_objects(sc), OPTIONS)
    return flat, PI.host_scores(flat)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The scene's flat arrays and host result, computed once and shared by the tests (treat as read-only)."""
    return host(scene(name))


def score_bound(flat):
    """|score - reference| allowed per pair: 1e-10 * n_matches * thr^2.  Each of the n terms is at most thr^2; a
    Sampson term's rounding error in these coordinate ranges is about 1e-12 * thr^2 (eps * pixel extent * 2 thr), so
    the bound leaves about 100x headroom."""
    return 1e-10 * np.diff(flat.pair_ptr) * flat.pair_geom[:, 9]


@functools.lru_cache(maxsize=None)
def golden(name):
    """What the reference did on the scene (tools/gen_golden.py --only inliers), per valid pair in view-graph order:
    dict of score, assigned, count, and inliers (concatenated)."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_inliers_golden.npz")
    with np.load(path) as z:
        return {k: z[f"{name}_{k}"] for k in ("score", "assigned", "count", "inliers")}


def check_against_golden(name, flat, idx, count, score, touched):
    """Inliers and the assigned flags exact, scores within score_bound; returns the largest |delta| / bound."""
    g = golden(name)
    assert np.array_equal(np.asarray(touched).astype(bool), g["assigned"])
    assert np.array_equal(count, g["count"])
    assert np.array_equal(idx, g["inliers"].astype(np.int32))
    bound = score_bound(flat)
    delta = np.abs(score - g["score"])
    assert (delta <= bound).all(), (delta - bound).max()
    return float(np.where(bound > 0, delta / np.where(bound > 0, bound, 1), 0.0).max())


# ---------------------------------------------------------------------------------------------------------------------
# the mapper scene (tests/mapper_scene.py) with ground-truth two-view geometry
# ---------------------------------------------------------------------------------------------------------------------
def true_matches(view_graph, images, seed=0, **size):
    """Per pair (view-graph order) a bool array: the match joins two observations of one point.  The database's
    keypoints are the float32 observations of synth.make_problem, so each is looked up by its coordinates."""
    prob = S.make_problem(size['n_images'], size['n_points'], track_len=size['track_len'], seed=seed,
                          window=size['window'])
    uv = prob.uv.astype(np.float32)
    point_of = [dict() for _ in images]
    for c, p, xy in zip(prob.cam_idx.tolist(), prob.pt_idx.tolist(), uv):
        point_of[c][xy.tobytes()] = p
    out = []
    for pair in view_graph.image_pairs.values():
        f1, f2 = images[pair.image_id1].features, images[pair.image_id2].features
        a = [point_of[pair.image_id1].get(f1[i].tobytes(), -1) for i in pair.matches[:, 0]]
        b = [point_of[pair.image_id2].get(f2[j].tobytes(), -2) for j in pair.matches[:, 1]]
        out.append(np.array(a) == np.array(b))
    return out
