"""Rotation averaging without a GPU: the spanning tree, the flattening, the scene helpers, FilterRotations' host path,
the C ABI's argument checks and the mapper keyword (with the device stage replaced by the numpy / scipy restatement of
tests/rotavg_reference.py)."""
import contextlib
import ctypes
import io
import itertools
import os
import re

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as R

import rotavg_reference as REF
import rotavg_scene as RS
from instantsfm_amd import _capi
from instantsfm_amd import rotavg as RA
from instantsfm_amd.controllers import global_mapper
from instantsfm_amd.controllers.config import Config
from instantsfm_amd.processors.relpose_filter import FilterRotations
from instantsfm_amd.processors.rotation_averaging import RotationEstimator
from instantsfm_amd.scene.defs import Ids2PairId, Image, ImagePair, ViewGraph
from instantsfm_amd.utils.tree import MaximumSpanningTree

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------
# the spanning tree
# ---------------------------------------------------------------------------------------------------------------------
def _usable(vg, images):
    return [(p.image_id1, p.image_id2, len(p.inliers)) for p in vg.image_pairs.values()
            if p.is_valid and images[p.image_id1].is_registered and images[p.image_id2].is_registered]


def _tree_edges(parents):
    return {tuple(sorted((i, p))) for i, p in enumerate(parents) if p not in (-1, i)}


def _path_min_weight(tree, weight, a, b):
    """The lightest edge on the tree path from a to b."""
    adj = {}
    for u, v in tree:
        adj.setdefault(u, []).append(v)
        adj.setdefault(v, []).append(u)
    best = {a: np.inf}
    stack = [a]
    while stack:
        cur = stack.pop()
        for nb in adj.get(cur, ()):
            if nb not in best:
                best[nb] = min(best[cur], weight[tuple(sorted((cur, nb)))])
                stack.append(nb)
    return best[b]


@pytest.mark.parametrize("name", RS.NAMES)
def test_maximum_spanning_tree_is_maximal(name):
    """The parents describe a tree over everything image 0 reaches, and no left-out pair is heavier than the lightest
    pair on the tree path between its images (the cycle property, which only a maximum spanning tree has)."""
    vg, images, _ = RS.scene(name)
    parents, root = MaximumSpanningTree(vg, images)
    assert root == 0 and parents[0] == 0 and len(parents) == len(images)
    usable = _usable(vg, images)
    weight = {tuple(sorted((a, b))): w for a, b, w in usable}
    tree = _tree_edges(parents)
    assert tree <= set(weight)
    if not images[0].is_registered:
        assert tree == set() and parents[1:] == [-1] * (len(images) - 1)
        return
    reached = {i for i, p in enumerate(parents) if p != -1}
    assert reached == {i for i, im in enumerate(images) if im.is_registered} and len(tree) == len(reached) - 1
    for a, b, w in usable:
        if tuple(sorted((a, b))) not in tree:
            assert w < _path_min_weight(tree, weight, a, b)
    assert parents == REF.maximum_spanning_parents(vg, images)


def _graph(n, weighted_pairs):
    vg = ViewGraph()
    for a, b, w in weighted_pairs:
        vg.image_pairs[Ids2PairId(a, b)] = ImagePair(image_id1=a, image_id2=b, inliers=list(range(w)))
    return vg, [Image(id=i, is_registered=True) for i in range(n)]


def test_maximum_spanning_tree_against_enumeration():
    """Every spanning tree of a 5-image, 8-pair graph enumerated: none is heavier."""
    pairs = [(0, 1, 5), (1, 2, 9), (2, 3, 4), (3, 4, 8), (0, 4, 7), (0, 2, 6), (1, 3, 3), (2, 4, 10)]
    vg, images = _graph(5, pairs)
    parents, _ = MaximumSpanningTree(vg, images)
    weight = {(a, b): w for a, b, w in pairs}
    got = sum(weight[e] for e in _tree_edges(parents))
    best = 0
    for subset in itertools.combinations(pairs, 4):
        label = list(range(5))
        for a, b, _ in subset:
            label = [label[b] if x == label[a] else x for x in label]
        if len(set(label)) == 1:
            best = max(best, sum(w for _, _, w in subset))
    assert got == best == 34


def test_maximum_spanning_tree_tie_rule():
    """Equal weights: the pair that comes first in the view graph wins.  In a triangle of equal pairs the first two
    listed form the tree, whichever they are."""
    for order in itertools.permutations([(0, 1), (0, 2), (1, 2)]):
        vg, images = _graph(3, [(a, b, 40) for a, b in order])
        parents, _ = MaximumSpanningTree(vg, images)
        assert _tree_edges(parents) == set(order[:2]), order
    # an invalid pair and a pair of an unregistered image do not count
    vg, images = _graph(4, [(0, 1, 40), (1, 2, 40), (0, 2, 90), (2, 3, 50)])
    vg.image_pairs[Ids2PairId(0, 2)].is_valid = False
    images[3].is_registered = False
    assert MaximumSpanningTree(vg, images)[0] == [0, 0, 1, -1]
    assert "networkx" not in open(os.path.join(REPO, "instantsfm_amd", "utils", "tree.py")).read().replace(
        "without networkx", "")


def test_package_does_not_import_networkx():
    for root, _, files in os.walk(os.path.join(REPO, "instantsfm_amd")):
        for f in files:
            if f.endswith(".py"):
                assert not re.search(r"^\s*(import|from)\s+networkx", open(os.path.join(root, f)).read(), re.M), f


# ---------------------------------------------------------------------------------------------------------------------
# flatten and the scene helpers
# ---------------------------------------------------------------------------------------------------------------------
def test_flatten_orders_and_maps():
    vg, images, _ = RS.scene("partial")
    flat = RA.flatten(vg, images)
    assert flat.image_ids == [i for i in range(14) if i not in (5, 9)]
    assert flat.id2idx == {image_id: k for k, image_id in enumerate(flat.image_ids)}
    valid = [(k, p) for k, p in vg.image_pairs.items() if p.is_valid]
    assert flat.keys == [k for k, _ in valid] and all(a is b for a, (_, b) in zip(flat.pairs, valid))
    assert 0 < len(valid) < len(vg.image_pairs) - 1 and not vg.image_pairs[Ids2PairId(2, 4)].is_valid
    assert flat.pair_i.dtype == flat.pair_j.dtype == np.int32 and flat.quat.shape == (len(valid), 4)
    assert flat.pair_i.tolist() == [flat.id2idx[p.image_id1] for _, p in valid]
    assert flat.pair_j.tolist() == [flat.id2idx[p.image_id2] for _, p in valid]
    assert np.array_equal(flat.quat, np.array([p.rotation for _, p in valid]))
    assert flat.n == 12 and flat.n_pairs == len(valid)
    # a valid pair of an unregistered image is the reference's KeyError
    vg.image_pairs[Ids2PairId(4, 5)].is_valid = True
    with pytest.raises(KeyError):
        RA.flatten(vg, images)
    empty = RA.flatten(ViewGraph(), [Image(id=0, is_registered=True)])
    assert empty.n == 1 and empty.n_pairs == 0 and empty.quat.shape == (0, 4)


def test_axis_angle_and_cam1to2_match_scipy():
    rng = np.random.default_rng(3)
    vectors = [np.zeros(3), np.array([1e-9, 0, 0]), np.array([0, 1e-4, -1e-4]), np.array([0.5, -0.2, 0.1]),
               np.array([0, 0, 3.0]), np.array([2.0, -2.0, 1.0]) / 3 * (np.pi - 1e-2)]
    vectors += list(R.random(40, random_state=5).as_rotvec())
    for v in vectors:
        M = R.from_rotvec(v).as_matrix()
        image = Image(world2cam=np.eye(4))
        image.world2cam[:3, :3] = M
        assert np.abs(image.axis_angle() - R.from_matrix(M).as_rotvec()).max() <= 1e-12
        pair = ImagePair()
        pose = np.eye(4)
        pose[:3, :3], pose[:3, 3] = M, rng.normal(size=3)
        pair.set_cam1to2(pose)
        q = R.from_matrix(M).as_quat()
        assert min(np.abs(pair.rotation - q).max(), np.abs(pair.rotation + q).max()) <= 1e-12
        assert np.array_equal(pair.translation, pose[:3, 3])
        assert np.abs(pair.get_cam1to2() - pose).max() <= 1e-12
        # an unnormalised quaternion is normalised, as Rotation.from_quat does
        pair.rotation = 3.0 * q
        assert np.abs(pair.get_cam1to2()[:3, :3] - M).max() <= 1e-12
    assert np.array_equal(ImagePair(translation=np.ones(3)).get_cam1to2()[3], [0, 0, 0, 1])


def test_initialisation_matches_restatement():
    """InitializeFromMaximumSpanningTree + SetupLinearSystem against the restatement's walk: the same rotations."""
    for name in RS.NAMES:
        n, pi, pj, quat, rot, fixed, fixed_rot = RS.solve_inputs(name)
        vg, images, _ = RS.scene(name)
        est = REF.Estimator()
        est.estimate(vg, images, dict(RS.RO, max_num_l1_iterations=0, max_num_irls_iterations=0), RS.LO)
        want = np.array([R.from_matrix(im.world2cam[:3, :3]).as_rotvec() for im in images if im.is_registered])
        assert RS.angle_between(rot, want).max() <= 1e-12, name
        assert fixed == 0 and np.abs(fixed_rot - rot[0]).max() == 0
    # the root-0 quirk: image 0 is not registered, so nothing was initialised
    assert not np.any(RS.solve_inputs("root0")[4])


def test_restatement_matches_recorded_reference(golden_dir):
    """tests/golden/rotavg_golden.npz (tools/gen_golden.py --only rotavg): the reference's own RotationEstimator on
    ``ring12``, its sparse Cholesky answered by a dense one.  The scene is still the recorded one, the restatement runs
    the same number of ADMM and IRLS iterations and ends at the same rotations.  Both sides solve the same dense
    systems in float64 along the same iteration, so they differ by rounding only: 1e-10 rad, the bound the GPU tests
    hold the device to."""
    g = np.load(os.path.join(golden_dir, "rotavg_golden.npz"))
    vg, images, _ = RS.scene("ring12")
    pairs = list(vg.image_pairs.values())
    assert np.array_equal(g["pair_i"], [p.image_id1 for p in pairs])
    assert np.array_equal(g["pair_j"], [p.image_id2 for p in pairs])
    assert np.array_equal(g["quat"], np.array([p.rotation for p in pairs]))
    assert np.array_equal(g["n_inliers"], [len(p.inliers) for p in pairs])
    est = REF.Estimator()
    assert est.estimate(vg, images, RS.RO, RS.LO) and est.gap > RS.MIN_GAP
    n_l1 = int(est.info[REF.INFO_L1_ITERS])
    assert est.info[REF.INFO_ADMM:REF.INFO_ADMM + n_l1].tolist() == g["admm"].tolist() and n_l1 == len(g["admm"])
    assert int(est.info[REF.INFO_IRLS_ITERS]) == int(g["irls"])
    got = np.array([im.world2cam[:3, :3] for im in images])
    angle = R.from_matrix(np.einsum('nji,njk->nik', got, g["rotations"])).magnitude().max()
    print(f"restatement against the recorded reference: {angle:.3g} rad")
    assert angle <= 1e-10
    # and the scene-level restatement agrees with the array-level one the GPU tests compare with
    assert est.info.tolist() == RS.expected("ring12")[2].tolist()


# ---------------------------------------------------------------------------------------------------------------------
# FilterRotations on the host
# ---------------------------------------------------------------------------------------------------------------------
def _solved_scene(name):
    vg, images, _ = RS.scene(name)
    ok, rot, _, _ = RS.expected(name)
    ids = [i for i, im in enumerate(images) if im.is_registered]
    matrices = R.from_rotvec(np.array(rot)).as_matrix()    # (a copy: scipy takes no read-only array)
    for k, i in enumerate(ids):
        images[i].world2cam[:3, :3] = matrices[k]
    return vg, images


@pytest.mark.parametrize("name", ["ring12", "ring70", "partial"])
def test_filter_rotations_host_path(name, capsys):
    vg, images = _solved_scene(name)
    vg2, images2 = _solved_scene(name)
    before = [p.is_valid for p in vg.image_pairs.values()]
    angles = REF.filter_rotations(vg2, images2, 5.0)
    FilterRotations(vg, images, 5.0, device="cpu")
    flags, want = [p.is_valid for p in vg.image_pairs.values()], [p.is_valid for p in vg2.image_pairs.values()]
    assert flags == want and flags != before               # the outlier pairs went
    assert capsys.readouterr().out == f"Filtered {before.count(True) - flags.count(True)} relative rotation " \
                                      "with angle > 5.0 degrees\n"
    pairs = [p for p, was in zip(vg.image_pairs.values(), before) if was]
    got = RA.host_pair_errors([p.image_id1 for p in pairs], [p.image_id2 for p in pairs],
                              [p.rotation for p in pairs], [im.world2cam[:3, :3] for im in images])
    assert np.abs(got - angles).max() <= 1e-9 and angles.min() > 1e-3
    FilterRotations(vg, images, 5.0, device=None)           # nothing more to drop
    assert [p.is_valid for p in vg.image_pairs.values()] == flags


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI's argument checks
# ---------------------------------------------------------------------------------------------------------------------
def _options(**kw):
    o = RA.make_options(RS.RO, RS.LO)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


SOLVE_CASES = {
    "negative_n": dict(n=-1), "zero_n": dict(n=0), "negative_pairs": dict(n_pairs=-1), "too_many_pairs": dict(n_pairs=2 ** 30),
    "n_over_limit": dict(n=RA.MAX_IMAGES + 1), "null_pair_i": dict(pair_i=None), "null_pair_j": dict(pair_j=None),
    "null_quat": dict(quat=None), "null_rot": dict(rot=None), "null_fixed_rot": dict(fixed_rot=None),
    "null_options": dict(opt=None), "null_info": dict(info=None), "fixed_negative": dict(fixed=-1),
    "fixed_out_of_range": dict(fixed=4), "nan_sigma": dict(opt=_options(irls_loss_parameter_sigma=float("nan"))),
    "inf_rho": dict(opt=_options(rho=float("inf"))), "zero_rho": dict(opt=_options(rho=0.0)),
    "nan_alpha": dict(opt=_options(alpha=float("nan"))), "nan_tolerance": dict(opt=_options(absolute_tolerance=float("nan"))),
    "inf_threshold": dict(opt=_options(l1_step_convergence_threshold=float("inf"))),
    "negative_iterations": dict(opt=_options(max_num_irls_iterations=-1)),
}


@pytest.mark.parametrize("case", sorted(SOLVE_CASES))
def test_solve_rejects_bad_arguments_without_gpu(case):
    """Sizes, missing pointers, the fixed index and the options are refused before the device is touched (the buffers
    here are host memory: a call that got past these checks could not succeed), and nothing is written."""
    L = _capi.load()
    buf = np.zeros(64)
    p = ctypes.c_void_p(buf.ctypes.data)
    info = (ctypes.c_int32 * RA.INFO_LEN)(*([-7] * RA.INFO_LEN))
    a = dict(n=4, n_pairs=3, pair_i=p, pair_j=p, quat=p, rot=p, fixed=0, fixed_rot=p, opt=_options(), info=info)
    a.update(SOLVE_CASES[case])
    opt = ctypes.byref(a["opt"]) if a["opt"] is not None else None
    rc = L.insfm_rotavg_solve(a["n"], a["n_pairs"], a["pair_i"], a["pair_j"], a["quat"], a["rot"], a["fixed"],
                              a["fixed_rot"], opt, a["info"], None)
    assert rc == _capi.INSFM_BA_EINVAL
    assert not buf.any() and list(info) == [-7] * RA.INFO_LEN


def test_stage_entry_points_reject_bad_arguments_without_gpu():
    L = _capi.load()
    buf = np.zeros(64)
    p = ctypes.c_void_p(buf.ctypes.data)
    E = _capi.INSFM_BA_EINVAL
    assert L.insfm_rotavg_residuals(-1, 0, p, p, p, p, 0, p, p, None) == E
    assert L.insfm_rotavg_residuals(4, 2, p, p, p, None, 0, p, p, None) == E
    assert L.insfm_rotavg_residuals(4, 2, p, p, p, p, 4, p, p, None) == E
    assert L.insfm_rotavg_residuals(4, 2, p, None, p, p, 0, p, p, None) == E
    assert L.insfm_rotavg_residuals(4, 2, p, p, p, p, 0, p, None, None) == E
    assert L.insfm_rotavg_update(-1, p, p, None) == E
    assert L.insfm_rotavg_update(3, None, p, None) == E
    assert L.insfm_rotavg_update(3, p, None, None) == E
    assert L.insfm_rotavg_update(RA.MAX_IMAGES + 1, p, p, None) == E
    assert L.insfm_rotavg_update(0, None, None, None) == 0
    assert L.insfm_rotavg_system(4, -1, p, p, None, 0, p, None, None) == E
    assert L.insfm_rotavg_system(4, 2, p, p, None, 0, None, None, None) == E
    assert L.insfm_rotavg_system(4, 2, None, p, None, 0, p, None, None) == E
    assert L.insfm_rotavg_system(4, 2, p, p, None, 5, p, None, None) == E
    assert L.insfm_rotavg_system(RA.MAX_IMAGES + 1, 2, p, p, None, 0, p, None, None) == E
    assert L.insfm_rotavg_pair_errors(-1, 0, p, p, p, p, p, None) == E
    assert L.insfm_rotavg_pair_errors(0, 2, p, p, p, p, p, None) == E
    assert L.insfm_rotavg_pair_errors(4, 2, p, p, None, p, p, None) == E
    assert L.insfm_rotavg_pair_errors(4, 2, p, p, p, p, None, None) == E
    assert L.insfm_rotavg_pair_errors(4, 0, None, None, None, None, None, None) == 0
    assert not buf.any()


def test_python_error_names_the_limit():
    n = RA.MAX_IMAGES + 1
    with pytest.raises(ValueError, match=str(RA.MAX_IMAGES)):
        RA.solve(n, [], [], np.zeros((0, 4)), np.zeros((n, 3)), 0, np.zeros(3), RS.RO, RS.LO)
    header = open(os.path.join(REPO, "include", "insfm_rotavg.h")).read()
    assert f"#define INSFM_ROTAVG_MAX_IMAGES {RA.MAX_IMAGES}\n" in header and RA.MAX_IMAGES >= 4096
    assert f"#define INSFM_ROTAVG_INFO_LEN {RA.INFO_LEN}\n" in header


# ---------------------------------------------------------------------------------------------------------------------
# the processor and the mapper keyword, with the device stage replaced by the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RS.NAMES)
def test_estimator_plumbing(name, monkeypatch):
    """RotationEstimator with ``rotavg.solve`` replaced by the restatement against the restatement's own
    EstimateRotations: the same rotations, twice on one instance (the fixed image and its rotation persist)."""
    monkeypatch.setattr(RA, "solve", REF.solve)
    vg, images, _ = RS.scene(name)
    vg2, images2, _ = RS.scene(name)
    est, ref = RotationEstimator(), REF.Estimator()
    for call in range(2):
        with contextlib.redirect_stdout(io.StringIO()):
            assert est.EstimateRotations(vg, images, RS.RO, RS.LO) is True
        assert ref.estimate(vg2, images2, RS.RO, RS.LO)
        got = np.array([im.world2cam[:3, :3] for im in images])
        want = np.array([im.world2cam[:3, :3] for im in images2])
        assert np.abs(got - want).max() <= 1e-12, (name, call)
        assert est.info.tolist() == ref.info.tolist()
        assert est.fixed_camera_id == ref.fixed_camera_id == (1 if name == "root0" else 0)
        assert np.array_equal(est.fixed_camera_rotation, ref.fixed_camera_rotation)
        for im, registered in zip(images, [im.is_registered for im in images2]):
            assert registered or np.array_equal(im.world2cam, np.eye(4))
        # the second call starts from a graph without its worst pairs, like the mapper's
        FilterRotations(vg, images, 5.0, device="cpu")
        REF.filter_rotations(vg2, images2, 5.0)


def test_estimator_reports_failure(monkeypatch):
    """A NaN step or weight: False, and the images keep what the initialisation gave them."""
    def failing(n, pair_i, pair_j, quat, rot, *a, **kw):
        info = np.zeros(RA.INFO_LEN, np.int32)
        info[RA.INFO_FAILED] = RA.FAILED_IRLS
        return False, rot, info
    monkeypatch.setattr(RA, "solve", failing)
    vg, images, _ = RS.scene("ring12")
    want = RS.solve_inputs("ring12")[4]
    with contextlib.redirect_stdout(io.StringIO()) as out:
        assert RotationEstimator().EstimateRotations(vg, images, RS.RO, RS.LO) is False
    assert out.getvalue() == "nan weight!\n"
    got = np.array([im.axis_angle() for im in images])
    assert RS.angle_between(got, want).max() <= 1e-12


def test_mapper_keyword_runs_the_stage(monkeypatch):
    """SolveGlobalMapper(rotation_averaging=True) with the device calls replaced: estimate, filter, largest component,
    twice, before track establishment; the timing and trace entries; the switch still refuses."""
    monkeypatch.setattr(RA, "solve", REF.solve)
    monkeypatch.setattr(RA, "device_pair_errors", lambda pi, pj, q, Rw, device: (0, RA.host_pair_errors(pi, pj, q, Rw)))
    vg, images, gt = RS.scene("ring70")
    cfg = Config.for_ba_half()
    cfg.OPTIONS['skip_track_establishment'] = True     # the mapper stops right after the stage (tracks unbound)
    T = {}
    with contextlib.redirect_stdout(io.StringIO()) as out, pytest.raises(UnboundLocalError):
        global_mapper.SolveGlobalMapper(vg, {}, images, cfg, timings=T, rotation_averaging=True)
    assert out.getvalue().count("relative rotation with angle > 10.0 degrees") == 2
    assert "70 / 70 images are within the connected component." in out.getvalue()
    n_valid = sum(p.is_valid for p in vg.image_pairs.values())
    assert T['trace'] == [('rotation_averaging', 70, n_valid, None)] and 200 < n_valid < 280
    assert T['rotation_averaging_s'] > 0

    vg2, images2, _ = RS.scene("ring70")
    ref = REF.Estimator()
    for _ in range(2):
        assert ref.estimate(vg2, images2, cfg.ROTATION_ESTIMATOR_OPTIONS, cfg.L1_SOLVER_OPTIONS)
        REF.filter_rotations(vg2, images2, 10.0)
    assert [p.is_valid for p in vg.image_pairs.values()] == [p.is_valid for p in vg2.image_pairs.values()]
    got = np.array([im.world2cam[:3, :3] for im in images])
    assert np.abs(got - np.array([im.world2cam[:3, :3] for im in images2])).max() <= 1e-12
    # Up to the gauge the rotations are the ground truth's, to the noise of the pairs: a chain of k pairs with 0.7 deg
    # of noise per axis drifts by about 0.7 sqrt(3 k) deg, 7 deg half-way round the 70-ring, and the three longer
    # pairs per image tighten that several times; the outlier pairs are random rotations, 126 deg on average.
    rel = np.einsum('nji,njk->nik', gt, got)            # R_gt^T R_est: the world's gauge, the same for every image
    assert np.rad2deg(R.from_matrix(np.einsum('nij,kj->nik', rel, rel[0])).magnitude().max()) < 3.5

    cfg.OPTIONS['skip_rotation_averaging'] = False
    with pytest.raises(NotImplementedError):
        global_mapper.SolveGlobalMapper(vg, {}, images, cfg, rotation_averaging=True)


def test_mapper_raises_where_the_reference_exits(monkeypatch):
    monkeypatch.setattr(RA, "solve", REF.solve)
    vg, images, _ = RS.scene("no_pairs")
    cfg = Config.for_ba_half()
    with contextlib.redirect_stdout(io.StringIO()), pytest.raises(RuntimeError, match="largest connected component"):
        global_mapper.SolveGlobalMapper(vg, {}, images, cfg, device="cpu", rotation_averaging=True)
