"""Image-pair inlier scoring without a GPU: the numpy host path (pair_inliers.host_scores) and the processor on
``device="cpu"`` against what the reference's ImagePairInliersCount did on the scenes of tests/pair_scene.py
(tests/golden/pair_inliers_golden.npz, tools/gen_golden.py --only inliers), the two view-graph filters on hand-counted
cases, and the C ABI's argument checks."""
import contextlib
import ctypes
import io

import numpy as np
import pytest

import pair_scene as PS
from instantsfm_amd import _capi
from instantsfm_amd import pair_inliers as PI
from instantsfm_amd.processors.image_pair_inliers import ImagePairInliersCount
from instantsfm_amd.processors.relpose_filter import FilterInlierNum, FilterInlierRatio
from instantsfm_amd.scene.defs import ConfigurationType, Ids2PairId, ImagePair, ViewGraph


@pytest.mark.parametrize("name", PS.NAMES)
def test_host_scores_match_reference(name):
    flat, (idx, count, score, touched, margin) = PS.expected(name)
    assert margin.shape == (flat.n_matches,) and margin.min() >= PS.MIN_MARGIN
    ratio = PS.check_against_golden(name, flat, idx, count, score, touched)
    print(f"{name}: largest |score - reference| / bound = {ratio:.3g}")
    # every pair's inliers are ascending local indices
    for part, n in zip(np.split(idx, np.cumsum(count)[:-1]), np.diff(flat.pair_ptr)):
        assert (np.diff(part) > 0).all() and (part.size == 0 or (part[0] >= 0 and part[-1] < n))


def test_general_scene_covers_the_sizes_and_kinds():
    flat, (idx, count, score, touched, _) = PS.expected("general_f32")
    n = np.diff(flat.pair_ptr)
    assert flat.xy.dtype == np.float32 and flat.rays.dtype == np.float64
    flat64 = PS.expected("general_f64")[0]
    assert flat64.xy.dtype == np.float64 and flat64.rays.dtype == np.float32
    for kind in (PI.HOMOGRAPHY, PI.FUNDAMENTAL, PI.ESSENTIAL):
        sel = flat.pair_kind == kind
        assert set(PS.SPECIAL_SIZES) <= set(n[sel].tolist())
        assert (count[sel & (n == 30)] == 30).any() and (count[sel & (n == 30)] == 0).any()  # all / no inliers
    assert (flat.pair_kind == PI.SKIP).sum() > 100 and not touched[flat.pair_kind == PI.SKIP].any()


def test_fundamental_cases_are_what_they_claim():
    flat, (idx, count, score, touched, _) = PS.expected("f_cases")
    sc = PS.scene("f_cases")
    parts = np.split(idx, np.cumsum(count)[:-1])
    # F and -F: the same majority, so one of the two votes was mostly negative
    # (the two pairs store the same pixels in their own random order: compare the inliers' image-1 coordinates)
    first = [np.sort(sc.xy[sc.pairs[p]['i1']][sc.pairs[p]['matches'][parts[p], 0], 0]) for p in (0, 1)]
    assert count[0] == count[1] > 20 and np.array_equal(first[0], first[1]) and score[0] == pytest.approx(score[1])
    assert touched.tolist() == [1, 1, 0, 1, 0, 1, 1, 0]
    assert count[2] == 0 and score[2] == 0                       # the tie: 12 against 12
    assert count[3] == 13 and score[3] == pytest.approx(12 * 16.0, abs=1e-6)   # 13 mirrored in, 12 others at thr^2
    assert count[5] == 20                                        # signum exactly 0 counts as negative
    F6 = sc.pairs[6]['F']
    assert np.abs(np.cross(F6[0], F6[1])).max() <= 1e-6
    assert np.array_equal(flat.pair_geom[6, 10:13], np.cross(F6[1], F6[2])) and count[6] > 20
    assert count[7] == 0 and not np.any(flat.pair_geom[7, :9])   # zero F: 0 / 0, no pre-inlier


def test_essential_cases_are_what_they_claim():
    flat, (idx, count, score, touched, _) = PS.expected("e_cases")
    sc = PS.scene("e_cases")
    n = np.diff(flat.pair_ptr)
    assert sc.pairs[0]['translation'][2] < 0 and flat.pair_geom[0, 12] > 0 and count[0] > 25
    assert 0 < count[1] <= n[1] - 16                             # 10 behind the cameras, 6 too far
    assert 0 < count[2] <= n[2] - 12                             # 12 within 3 degrees of the epipole
    f1, f2 = sc.focal[sc.pairs[3]['i1']], sc.focal[sc.pairs[3]['i2']]
    assert f1 != f2 and flat.pair_geom[3, 9] == (0.5 * (1 / f1 + 1 / f2)) ** 2 and count[3] > 25
    assert count[4] == 0 and touched[4] == 1 and score[4] == pytest.approx(n[4] * flat.pair_geom[4, 9], rel=1e-12)
    assert len(flat.pairs) == len(sc.pairs) - 1                  # the invalid pair is not visited
    assert flat.pair_kind[5] == PI.SKIP and touched[5] == 0


@pytest.mark.parametrize("name", PS.NAMES)
def test_processor_on_cpu(name):
    sc = PS.scene(name)
    vg, cameras, images = PS.as_objects(sc)
    before = {k: p.inliers for k, p in vg.image_pairs.items()}
    scores = {}
    assert ImagePairInliersCount(vg, cameras, images, PS.OPTIONS, device="cpu", scores=scores) is None
    valid = [(k, p) for k, p in vg.image_pairs.items() if p.is_valid]
    assert list(scores) == [k for k, _ in valid]
    g = PS.golden(name)
    want = np.split(g["inliers"].astype(np.int64), np.cumsum(g["count"])[:-1])
    bound = PS.score_bound(PS.expected(name)[0])
    for (k, p), assigned, w, s, b in zip(valid, g["assigned"], want, g["score"], bound):
        if assigned:
            assert isinstance(p.inliers, np.ndarray) and p.inliers.dtype == np.int64 and np.array_equal(p.inliers, w)
        else:
            assert p.inliers is before[k]
        assert abs(scores[k] - s) <= b
    for (k, p), spec in zip(vg.image_pairs.items(), sc.pairs):
        if not p.is_valid:
            assert p.inliers is before[k] and np.array_equal(p.inliers, spec['inliers'])
        elif spec['inliers'] is not None and not g["assigned"][[kk for kk, _ in valid].index(k)]:
            assert np.array_equal(p.inliers, spec['inliers'])    # pre-set inliers survive where nothing is assigned


def test_empty_view_graph():
    flat = PI.flatten(ViewGraph(), [], [], PS.OPTIONS)
    idx, count, score, touched, margin = PI.host_scores(flat)
    assert flat.n_pairs == 0 and idx.size == count.size == score.size == touched.size == margin.size == 0
    ImagePairInliersCount(ViewGraph(), [], [], PS.OPTIONS, device="cpu")


@pytest.mark.parametrize("column", [0, 1])
def test_match_outside_its_image_raises_index_error(column):
    vg, cameras, images = PS.as_objects(PS.scene("f_cases"))
    pair = list(vg.image_pairs.values())[3]
    image = images[pair.image_id1 if column == 0 else pair.image_id2]
    pair.matches[5, column] = len(image.features)
    with pytest.raises(IndexError):
        ImagePairInliersCount(vg, cameras, images, PS.OPTIONS, device="cpu")


def _graph(rows):
    """A view graph of pairs (valid, inliers, matches)."""
    vg = ViewGraph()
    for i, (valid, n_inl, n_match) in enumerate(rows):
        p = ImagePair(image_id1=i, image_id2=i + 1, is_valid=valid, inliers=np.arange(n_inl))
        p.matches = np.zeros((n_match, 2), np.uint32)
        vg.image_pairs[Ids2PairId(i, i + 1)] = p
    return vg


def test_filter_inlier_num_is_exclusive_at_the_minimum():
    vg = _graph([(True, 29, 100), (True, 30, 100), (True, 31, 100), (False, 0, 100), (True, 0, 0)])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        FilterInlierNum(vg, 30)
    assert [p.is_valid for p in vg.image_pairs.values()] == [False, True, True, False, False]
    assert out.getvalue() == "Filtered 2 relative pose with inlier number < 30\n"   # (the invalid pair is not counted)
    vg.image_pairs[Ids2PairId(1, 2)].inliers = [1, 2, 3]                            # a plain list counts by its length
    with contextlib.redirect_stdout(io.StringIO()):
        FilterInlierNum(vg, 4)
    assert [p.is_valid for p in vg.image_pairs.values()] == [False, False, True, False, False]


def test_filter_inlier_ratio_is_exclusive_at_the_minimum():
    vg = _graph([(True, 24, 100), (True, 25, 100), (True, 1, 4), (True, 0, 7), (False, 0, 0), (True, 26, 100)])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        FilterInlierRatio(vg, 0.25)
    assert [p.is_valid for p in vg.image_pairs.values()] == [False, True, True, False, False, True]
    assert out.getvalue() == "Filtered 2 relative pose with inlier ratio < 0.25\n"
    with pytest.raises(ZeroDivisionError):                                          # len(inliers) / 0 in the reference
        FilterInlierRatio(_graph([(True, 0, 0)]), 0.25)


def test_kind_of_every_configuration():
    vg = ViewGraph()
    for c in ConfigurationType:
        p = ImagePair(image_id1=0, image_id2=1, config=c)
        p.matches = np.zeros((0, 2), np.uint32)
        vg.image_pairs[c.value] = p
    cams, ims = PS.as_objects(PS.scene("e_cases"))[1:]
    kinds = PI.flatten(vg, cams, ims, PS.OPTIONS).pair_kind.tolist()
    assert kinds == [0, 0, PI.ESSENTIAL, PI.FUNDAMENTAL, PI.HOMOGRAPHY, PI.HOMOGRAPHY, PI.HOMOGRAPHY, 0, 0]


@pytest.mark.parametrize("case", ["negative_pairs", "negative_matches", "too_many_matches", "negative_features",
                                  "null_pair_ptr", "null_kind", "null_geom", "null_count", "null_matches", "null_xy",
                                  "null_idx", "no_features"])
def test_abi_rejects_bad_inputs_without_gpu(case):
    """Sizes and missing pointers are refused before the device is touched (the buffers here are host memory: a call
    that got past the checks could not succeed)."""
    L = _capi.load()
    buf = np.zeros(64)
    p = ctypes.c_void_p(buf.ctypes.data)
    a = dict(n_pairs=1, pair_ptr=p, n_matches=2, match_a=p, match_b=p, n_features=4, xy=p, xy_f32=0, rays=None,
             rays_f32=0, kind=p, geom=p, idx=p, count=p, score=p, touched=p)
    a.update({"negative_pairs": dict(n_pairs=-1), "negative_matches": dict(n_matches=-1),
              "too_many_matches": dict(n_matches=2 ** 31), "negative_features": dict(n_features=-1),
              "null_pair_ptr": dict(pair_ptr=None), "null_kind": dict(kind=None), "null_geom": dict(geom=None),
              "null_count": dict(count=None), "null_matches": dict(match_b=None), "null_xy": dict(xy=None),
              "null_idx": dict(idx=None), "no_features": dict(n_features=0)}[case])
    rc = L.insfm_pair_inliers(a["n_pairs"], a["pair_ptr"], a["n_matches"], a["match_a"], a["match_b"], a["n_features"],
                              a["xy"], a["xy_f32"], a["rays"], a["rays_f32"], a["kind"], a["geom"], a["idx"],
                              a["count"], a["score"], a["touched"], None)
    assert rc == _capi.INSFM_BA_EINVAL
    assert not buf.any()


def test_abi_empty_call_without_gpu():
    assert _capi.load().insfm_pair_inliers(0, None, 0, None, None, 0, None, 0, None, 0, None, None, None, None, None,
                                           None, None) == 0


def test_mapper_scene_host_path_separates_true_from_wrong(tmp_path):
    """The 40-image mapper scene (tests/mapper_scene.py) with ground-truth two-view geometry and intrinsics
    (synth.ground_truth_two_view) and the default thresholds, on the host path: the scoring must keep at least 90 % of
    the true matches and at most 10 % of the wrong ones for the GPU mapper test to mean anything."""
    import mapper_scene as MS
    from instantsfm_amd.synth import ground_truth_two_view
    from oracle import mapper as OM
    scene = MS.make_db(tmp_path / "db.db", seed=0)
    vg, cams, ims, cfg = MS.load(tmp_path / "db.db", scene, seed=0)
    ground_truth_two_view(vg, cams, ims, scene)
    OM.undistort_images(cams, ims)
    ImagePairInliersCount(vg, cams, ims, cfg.INLIER_THRESHOLD_OPTIONS, device="cpu")
    true = PS.true_matches(vg, ims, seed=0, **MS.SMALL)
    kept_true = kept_wrong = n_true = n_wrong = 0
    for pair, t in zip(vg.image_pairs.values(), true):
        keep = np.zeros(len(pair.matches), bool)
        keep[pair.inliers] = True
        n_true, n_wrong = n_true + int(t.sum()), n_wrong + int((~t).sum())
        kept_true, kept_wrong = kept_true + int((keep & t).sum()), kept_wrong + int((keep & ~t).sum())
    print(f"true matches kept {kept_true} / {n_true}, wrong matches kept {kept_wrong} / {n_wrong}")
    assert n_wrong > 100 and kept_true >= 0.9 * n_true and kept_wrong <= 0.1 * n_wrong
