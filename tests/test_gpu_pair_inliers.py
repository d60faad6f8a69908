"""Image-pair inlier scoring on the GPU (csrc/pair_inliers.hip, insfm_pair_inliers): the raw call against the numpy
host path on the scenes of tests/pair_scene.py, the processor against the reference's recorded results, and the mapper
with ``pair_inliers=True`` against the host-scored pipeline.  Needs an MI355X."""
import contextlib
import dataclasses
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import mapper_scene as MS  # noqa: E402
import pair_scene as PS  # noqa: E402
from instantsfm_amd import _capi  # noqa: E402
from instantsfm_amd import pair_inliers as PI  # noqa: E402
from instantsfm_amd.controllers import global_mapper  # noqa: E402
from instantsfm_amd.controllers.global_mapper import SolveGlobalMapper  # noqa: E402
from instantsfm_amd.processors.image_pair_inliers import ImagePairInliersCount  # noqa: E402
from instantsfm_amd.processors.relpose_filter import FilterInlierNum, FilterInlierRatio  # noqa: E402
from instantsfm_amd.scene.defs import ViewGraph  # noqa: E402
from instantsfm_amd.synth import ground_truth_two_view  # noqa: E402
from oracle import mapper as OM  # noqa: E402

FILL = -7


@pytest.mark.parametrize("name", PS.NAMES)
def test_device_call_matches_host_path(name):
    """Inliers, counts and touched exact; scores within 1e-10 * n_matches * thr^2 (pair_scene.score_bound); buffer
    entries past each pair's count still hold the fill value; a second run returns the same bytes."""
    flat, (idx, count, score, touched, _) = PS.expected(name)
    rc, d_idx, d_count, d_score, d_touched = PI.device_call(flat, fill=FILL)
    assert rc == 0
    assert np.array_equal(d_count, count) and np.array_equal(d_touched, touched)
    local = np.arange(flat.n_matches) - np.repeat(flat.pair_ptr[:-1], np.diff(flat.pair_ptr))
    written = local < np.repeat(count, np.diff(flat.pair_ptr))
    assert np.array_equal(d_idx[written], idx)
    assert (d_idx[~written] == FILL).all()
    delta, bound = np.abs(d_score - score), PS.score_bound(flat)
    ratio = np.where(bound > 0, delta / np.where(bound > 0, bound, 1), 0).max()
    print(f"{name}: largest |score - host| / bound = {ratio:.3g}")
    assert (delta <= bound).all(), (delta - bound).max()
    again = PI.device_call(flat, fill=FILL)
    assert again[0] == 0
    for a, b in zip(again[1:], (d_idx, d_count, d_score, d_touched)):
        assert a.tobytes() == b.tobytes()


def test_empty_calls():
    empty = PI.flatten(ViewGraph(), [], [], PS.OPTIONS)
    rc, idx, count, score, touched = PI.device_call(empty, fill=FILL)
    assert rc == 0 and idx.size == count.size == score.size == touched.size == 0
    # pairs without a single match
    flat = PS.expected("e_cases")[0]
    none = dataclasses.replace(flat, pair_ptr=np.zeros(flat.n_pairs + 1, np.int64), match_a=np.zeros(0, np.int32),
                               match_b=np.zeros(0, np.int32))
    rc, idx, count, score, touched = PI.device_call(none, fill=FILL)
    assert rc == 0 and idx.size == 0 and not count.any() and not score.any()
    assert np.array_equal(touched, np.isin(flat.pair_kind, (PI.HOMOGRAPHY, PI.ESSENTIAL)).astype(np.int32))


@pytest.mark.parametrize("case", ["ptr_decreasing", "ptr_negative", "ptr_past_matches", "kind_4", "kind_negative",
                                  "feature_past_end", "feature_negative", "essential_without_rays"])
def test_invalid_input_is_refused_and_nothing_written(case):
    flat = PS.expected("e_cases")[0]
    ptr, a, b, kind = flat.pair_ptr.copy(), flat.match_a.copy(), flat.match_b.copy(), flat.pair_kind.copy()
    rays = flat.rays
    if case == "ptr_decreasing":
        ptr[2] = ptr[1] - 1
    elif case == "ptr_negative":
        ptr[0] = -1
    elif case == "ptr_past_matches":
        ptr[-1] += 1
    elif case == "kind_4":
        kind[1] = 4
    elif case == "kind_negative":
        kind[3] = -1
    elif case == "feature_past_end":
        a[17] = flat.xy.shape[0]
    elif case == "feature_negative":
        b[40] = -1
    elif case == "essential_without_rays":
        rays = None
    bad = dataclasses.replace(flat, pair_ptr=ptr, match_a=a, match_b=b, pair_kind=kind, rays=rays)
    rc, idx, count, score, touched = PI.device_call(bad, fill=FILL)
    assert rc == _capi.INSFM_BA_EINVAL
    assert (idx == FILL).all() and (count == FILL).all() and (score == FILL).all() and (touched == FILL).all()
    with pytest.raises(_capi.BAError):
        PI.score(bad)


@pytest.mark.parametrize("name", PS.NAMES)
def test_processor_matches_reference_and_cpu_device(name):
    sc = PS.scene(name)
    vg, cameras, images = PS.as_objects(sc)
    vg2, cameras2, images2 = PS.as_objects(sc)
    before = {k: p.inliers for k, p in vg.image_pairs.items()}
    scores, scores2 = {}, {}
    ImagePairInliersCount(vg, cameras, images, PS.OPTIONS, device="cuda:0", scores=scores)
    ImagePairInliersCount(vg2, cameras2, images2, PS.OPTIONS, device="cpu", scores=scores2)
    g = PS.golden(name)
    want = np.split(g["inliers"].astype(np.int64), np.cumsum(g["count"])[:-1])
    bound = PS.score_bound(PS.expected(name)[0])
    valid = [k for k, p in vg.image_pairs.items() if p.is_valid]
    assert list(scores) == list(scores2) == valid
    for k, assigned, w, s, b in zip(valid, g["assigned"], want, g["score"], bound):
        p, p2 = vg.image_pairs[k], vg2.image_pairs[k]
        if assigned:
            assert isinstance(p.inliers, np.ndarray) and p.inliers.dtype == np.int64
            assert np.array_equal(p.inliers, w) and np.array_equal(p2.inliers, w)
        else:
            assert p.inliers is before[k]
        assert abs(scores[k] - s) <= b and abs(scores[k] - scores2[k]) <= b
    for k, p in vg.image_pairs.items():
        if not p.is_valid:
            assert p.inliers is before[k]


def _prepared(path, scene, seed):
    vg, cams, ims, cfg = MS.load(path, scene, seed=seed)
    ground_truth_two_view(vg, cams, ims, scene)
    return vg, cams, ims, cfg


def test_mapper_scores_its_own_inliers(tmp_path, monkeypatch):
    """SolveGlobalMapper(pair_inliers=True) on the 40-image mapper scene with ground-truth two-view geometry and
    intrinsics (synth.ground_truth_two_view) and the default thresholds (E 1 px, F 4 px, 30 inliers, ratio 0.25).

    On the host path (tests/test_pair_inliers.py, seed 0) the scoring keeps 24731 of the 26488 true matches (93 %) and
    1 of the 267 wrong ones.  After the stage every pair's inliers and validity and every image's ``is_registered``
    equal what the host path gives on a fresh copy; the trace starts with ``pair_inliers``; the remaining stages match
    oracle.mapper.solve_global_mapper run on that host-scored copy within test_gpu_mapper.py's bounds (counts exact,
    GP loss 1e-6 relative, BA RMSE 1e-4 px, camera centres 1e-4)."""
    scene = MS.make_db(tmp_path / "db.db", seed=0)
    # the host-scored copy: the same stage on the CPU restatements
    vg2, cams2, ims2, cfg2 = _prepared(tmp_path / "db.db", scene, 0)
    with contextlib.redirect_stdout(io.StringIO()):
        OM.undistort_images(cams2, ims2)
        ImagePairInliersCount(vg2, cams2, ims2, cfg2.INLIER_THRESHOLD_OPTIONS, device="cpu")
        FilterInlierNum(vg2, cfg2.INLIER_THRESHOLD_OPTIONS['min_inlier_num'])
        FilterInlierRatio(vg2, cfg2.INLIER_THRESHOLD_OPTIONS['min_inlier_ratio'])
        vg2.keep_largest_connected_component(ims2)
    stage = dict(inliers={k: np.array(p.inliers) for k, p in vg2.image_pairs.items()},
                 valid={k: p.is_valid for k, p in vg2.image_pairs.items()},
                 registered=[im.is_registered for im in ims2])
    n_valid = sum(stage['valid'].values())
    assert 0 < n_valid < len(vg2.image_pairs) and sum(stage['registered']) > 30   # the filters removed some pairs

    vg, cams, ims, cfg = _prepared(tmp_path / "db.db", scene, 0)
    after_stage = {}

    class RecordingTrackEngine(global_mapper.TrackEngine):   # (constructed right after the stage)
        def __init__(self, view_graph, images, device="cuda:0"):
            after_stage['registered'] = [im.is_registered for im in images]
            super().__init__(view_graph, images, device=device)
    monkeypatch.setattr(global_mapper, "TrackEngine", RecordingTrackEngine)
    np.random.seed(0)
    T = {}
    with contextlib.redirect_stdout(io.StringIO()):
        cams, ims, tracks = SolveGlobalMapper(vg, cams, ims, cfg, timings=T, pair_inliers=True)
    assert after_stage['registered'] == stage['registered']
    for k, p in vg.image_pairs.items():
        assert p.is_valid == stage['valid'][k]
        assert np.array_equal(p.inliers, stage['inliers'][k]), k
    got = T['trace']
    assert got[0] == ('pair_inliers', n_valid, sum(len(stage['inliers'][k]) for k, v in stage['valid'].items() if v),
                      None)
    assert T['pair_inliers_s'] > 0
    assert np.asarray(vg.image_pairs[next(iter(vg.image_pairs))].inliers).dtype == np.int64

    np.random.seed(0)
    ref = []
    with contextlib.redirect_stdout(io.StringIO()):
        _, _, tracks2 = OM.solve_global_mapper(vg2, cams2, ims2, cfg2, trace=ref)
    assert [im.is_registered for im in ims] == [im.is_registered for im in ims2]
    assert [g[0] for g in got[1:]] == [r[0] for r in ref]
    for g, r in zip(got[1:], ref):
        assert g[1:3] == r[1:3], (g, r)
        if g[0] == 'gp':
            assert abs(g[3] - r[3]) <= 1e-6 * abs(r[3]), (g, r)
        elif g[3] is not None:
            assert abs(g[3] - r[3]) <= 1e-4, (g, r)
    assert list(tracks.keys()) == list(tracks2.keys())
    C = np.array([im.center() for im in ims])
    C2 = np.array([im.center() for im in ims2])
    assert np.abs(C - C2).max() <= 1e-4, np.abs(C - C2).max()


def test_mapper_without_the_stage_is_unchanged(tmp_path):
    """``pair_inliers=False`` (the default): today's trace -- no ``pair_inliers`` entry, the caller's inliers used."""
    scene = MS.make_db(tmp_path / "db.db", seed=0)
    traces = []
    for kw in ({}, dict(pair_inliers=False)):
        vg, cams, ims, cfg = MS.load(tmp_path / "db.db", scene, seed=0)
        cfg.OPTIONS['skip_bundle_adjustment'] = cfg.OPTIONS['skip_retriangulation'] = True
        np.random.seed(0)
        T = {}
        with contextlib.redirect_stdout(io.StringIO()):
            SolveGlobalMapper(vg, cams, ims, cfg, timings=T, **kw)
        assert 'pair_inliers_s' not in T
        assert all(len(p.inliers) == len(p.matches) for p in vg.image_pairs.values())
        traces.append(T['trace'])
    assert [t[0] for t in traces[0]] == ['tracks', 'gp', 'gp_filtered']
    # (the GP loss of two identical runs differs in the last bits: compared to test_gpu_mapper.py's 1e-6 relative)
    assert [t[:3] for t in traces[0]] == [t[:3] for t in traces[1]]
    assert abs(traces[0][1][3] - traces[1][1][3]) <= 1e-6 * abs(traces[0][1][3])
