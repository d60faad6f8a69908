"""Small view graphs for the rotation-averaging tests: ring graphs over random ground-truth rotations.

Image i is paired with i + 1 .. i + reach (mod n).  A pair's rotation is the ground-truth relative rotation times a
N(0, sigma^2) rotation vector; ``outlier_frac`` of the pairs that are not chain pairs (i, i + 1) carry a random rotation
instead.  Every pair has its own inlier count, so the maximum spanning tree is unique.

  ring12     12 images, reach 3: the smallest graph with cycles and outliers
  ring32/33  one Gauss-Jordan tile exactly, and one image over
  ring70     70 images, reach 4: three tiles, 280 pairs (more than one 256-thread block)
  partial    14 images, two of them unregistered (their pairs invalid) and one more invalid pair
  no_pairs   3 images, only image 0 registered, no valid pair: only the gauge row acts
  root0      12 images, image 0 unregistered: the spanning-tree walk starts at image 0 whatever its state, so nothing
             is initialised and the solve starts from the identity rotations.  Its ground-truth rotations stay within
             ``spread`` of the identity so that this start is not near an angle of pi anywhere.

``solve_inputs(name)`` are the dense arrays the package's host code hands to insfm_rotavg_solve for the scene;
``expected(name)`` is the restatement's result on them (computed once, shared by the tests).
"""
import functools

import numpy as np
from scipy.spatial.transform import Rotation as R

import rotavg_reference as REF
from instantsfm_amd.config.colmap import L1_SOLVER_OPTIONS, ROTATION_ESTIMATOR_OPTIONS
from instantsfm_amd.processors.rotation_averaging import RotationEstimator
from instantsfm_amd.scene.defs import Ids2PairId, Image, ImagePair, ViewGraph

RO, LO = dict(ROTATION_ESTIMATOR_OPTIONS), dict(L1_SOLVER_OPTIONS)

SPECS = {
    "ring12": dict(n=12, reach=3, seed=1),
    "ring32": dict(n=32, reach=3, seed=2),
    "ring33": dict(n=33, reach=3, seed=3),
    "ring70": dict(n=70, reach=4, seed=4),
    "partial": dict(n=14, reach=3, seed=5, unregistered=(5, 9), invalid=((2, 4),)),
    "no_pairs": dict(n=3, reach=1, seed=6, unregistered=(1, 2)),
    "root0": dict(n=12, reach=3, seed=7, unregistered=(0,), spread_deg=25.0),
}
NAMES = tuple(SPECS)
MIN_GAP = 1e-6


def scene(name, sigma_deg=0.7, outlier_frac=0.12):
    """A fresh (view_graph, images, ground-truth rotations [n, 3, 3])."""
    spec = SPECS[name]
    n, reach, seed = spec["n"], spec["reach"], spec["seed"]
    rng = np.random.default_rng([seed, 11])
    if "spread_deg" in spec:
        gt = R.from_rotvec(rng.normal(0, np.deg2rad(spec["spread_deg"]) / np.sqrt(3), (n, 3))).as_matrix()
    else:
        gt = R.random(n, random_state=seed).as_matrix()
    chain = {}
    for i in range(n):
        for d in range(1, reach + 1):
            a, b = sorted((i, (i + d) % n))
            if a != b:
                chain.setdefault((a, b), d == 1)
    edges = [(a, b, c) for (a, b), c in chain.items()]
    counts = 30 + rng.permutation(len(edges))
    images = [Image(id=i, is_registered=i not in spec.get("unregistered", ())) for i in range(n)]
    vg = ViewGraph()
    for (a, b, chain), count in zip(edges, counts.tolist()):
        rel = gt[b] @ gt[a].T
        if not chain and rng.uniform() < outlier_frac:
            rel = R.random(random_state=int(rng.integers(1 << 30))).as_matrix()
        else:
            rel = R.from_rotvec(rng.normal(0, np.deg2rad(sigma_deg), 3)).as_matrix() @ rel
        q = R.from_matrix(rel).as_quat()
        valid = images[a].is_registered and images[b].is_registered and (a, b) not in spec.get("invalid", ())
        vg.image_pairs[Ids2PairId(a, b)] = ImagePair(image_id1=a, image_id2=b, is_valid=valid, rotation=q,
                                                     translation=rng.normal(size=3), inliers=np.arange(count))
    vg.num_images, vg.num_pairs = n, len(edges)
    return vg, images, gt


def solve_inputs(name):
    """(n, pair_i, pair_j, quat, rot, fixed, fixed_rot) after the package's host initialisation of the scene."""
    vg, images, _ = scene(name)
    est = RotationEstimator(device=None)
    est.InitializeFromMaximumSpanningTree(vg, images)
    est.SetupLinearSystem(vg, images)
    f = est.flat
    return (f.n, f.pair_i, f.pair_j, f.quat, est.rotation_estimated[:3 * f.n].reshape(f.n, 3).copy(),
            f.id2idx[est.fixed_camera_id], np.array(est.fixed_camera_rotation))


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement on ``solve_inputs(name)``: (ok, rot, info, smallest decision gap).  Treat as read-only."""
    ok, rot, info, gap = REF.solve_with_gap(*solve_inputs(name), RO, LO)
    rot.setflags(write=False)
    info.setflags(write=False)
    return ok, rot, info, gap


def angle_between(rot_a, rot_b):
    """Per image, the angle of R_a^T R_b in radians."""
    a, b = np.array(rot_a), np.array(rot_b)  # (copies: scipy takes no read-only array)
    return (R.from_rotvec(a).inv() * R.from_rotvec(b)).magnitude()
