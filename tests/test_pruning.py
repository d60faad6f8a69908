"""Pruning on the CPU: the host path of the co-visibility pair counts (instantsfm_amd/covis.py) and the host policy of
PruneWeaklyConnectedImages / EstablishStrongClusters against what the reference did on the same scenes
(tools/gen_golden.py --only pruning, tests/golden/pruning_golden.npz), and the mapper's switch."""
import contextlib
import io
import os

import numpy as np
import pytest

import pruning_scene as PS
from instantsfm_amd import covis
from instantsfm_amd.controllers.config import OUT_OF_SCOPE_STAGES, Config
from instantsfm_amd.controllers.global_mapper import SolveGlobalMapper
from instantsfm_amd.processors import reconstruction_pruning as RP
from instantsfm_amd.utils.union_find import UnionFind


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "pruning_golden.npz")) as z:
        return dict(z)


def golden_scene(golden, name):
    """The committed inputs; they are also what pruning_scene builds today."""
    M, ptr, img = PS.scene(name)
    assert M == int(golden[f"{name}_M"])
    np.testing.assert_array_equal(ptr, golden[f"{name}_track_ptr"])
    np.testing.assert_array_equal(img, golden[f"{name}_obs_img"])
    return M, ptr, img


def prune(M, ptr, img, device):
    images, tracks = PS.as_objects(M, ptr, img)
    with contextlib.redirect_stdout(io.StringIO()):
        RP.PruneWeaklyConnectedImages(images, tracks, device=device)
    return np.array([im.is_registered for im in images]), np.array([im.cluster_id for im in images])


def cluster(M, lo, hi, count, threshold):
    images = PS.as_objects(M, np.zeros(1, np.int64), np.zeros(0, np.int32))[0]
    with contextlib.redirect_stdout(io.StringIO()):
        RP.EstablishStrongClusters(RP.visibility_graph(lo, hi, count), images, threshold, 2)
    return np.array([im.is_registered for im in images]), np.array([im.cluster_id for im in images])


@pytest.mark.parametrize("name", PS.names())
def test_host_pair_list_matches_reference(golden, name):
    """Ids (image_id1 is the larger), weights and dict order."""
    M, ptr, img = golden_scene(golden, name)
    lo, hi, count = covis.covis_pairs(ptr, img, min_count=5, device="cpu")
    assert (lo < hi).all()
    np.testing.assert_array_equal(np.stack([hi, lo, count], 1), golden[f"{name}_pairs"])
    vg = RP.visibility_graph(lo, hi, count)
    got = [(p.image_id1, p.image_id2, p.weight) for p in vg.image_pairs.values()]
    assert got == [tuple(r) for r in golden[f"{name}_pairs"].tolist()]


@pytest.mark.parametrize("name", PS.names())
def test_processor_on_host_path_matches_reference(golden, name):
    M, ptr, img = golden_scene(golden, name)
    count = covis.covis_pairs(ptr, img, device="cpu")[2]
    with contextlib.redirect_stdout(io.StringIO()):
        assert RP.strong_cluster_threshold(count) == int(golden[f"{name}_threshold"])
    reg, cl = prune(M, ptr, img, "cpu")
    np.testing.assert_array_equal(reg, golden[f"{name}_registered"])
    np.testing.assert_array_equal(cl, golden[f"{name}_cluster"])


def test_hand_built_scene(golden):
    """The two images with 3 shared tracks are unregistered and the satellite group is cluster 1."""
    reg, cl = golden["hand_registered"], golden["hand_cluster"]
    assert reg.tolist() == [True] * 15 + [False] * 2
    assert cl.tolist() == [0] * 10 + [1] * 5 + [-1] * 2


def test_golden_scenes_cover_every_kind(golden):
    """The fixture choice: at least 5 committed seeds unregister an image, 5 give several clusters, and in at least
    one (here: 5) taking the pairs in key order instead of first-occurrence order changes the outcome."""
    unreg = clusters = order = 0
    for s in PS.SEEDS:
        reg, cl = golden[f"{s}_registered"], golden[f"{s}_cluster"]
        unreg += not reg.all()
        clusters += cl.max() > 0
        pairs = golden[f"{s}_pairs"]
        by_key = np.lexsort((pairs[:, 0], pairs[:, 1]))
        assert sorted(by_key.tolist()) == list(range(len(pairs)))
        p = pairs[by_key]
        reg2, cl2 = cluster(int(golden[f"{s}_M"]), p[:, 1], p[:, 0], p[:, 2], int(golden[f"{s}_threshold"]))
        order += not (np.array_equal(reg, reg2) and np.array_equal(cl, cl2))
        # (and in dict order the same call reproduces the reference)
        reg3, cl3 = cluster(int(golden[f"{s}_M"]), pairs[:, 1], pairs[:, 0], pairs[:, 2], int(golden[f"{s}_threshold"]))
        assert np.array_equal(reg, reg3) and np.array_equal(cl, cl3)
    assert unreg >= 5 and clusters >= 5 and order >= 5, (unreg, clusters, order)


def test_empty_visibility_graph_raises_index_error():
    """No pair reaches 5: the reference indexes pair_count[0] of an empty array."""
    rows = [[0, 1, 2]] * 4 + [[3, 4]] * 50 + [[5]] * 3
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    img = np.concatenate(rows)
    assert len(covis.covis_pairs(ptr, img, device="cpu")[0]) == 0
    with pytest.raises(IndexError):
        prune(6, ptr, img, "cpu")
    with pytest.raises(IndexError):
        prune(6, np.zeros(1, np.int64), np.zeros(0, np.int32), "cpu")


def test_host_pairs_small_example():
    """Ordinals by hand: track 0 (rows 5,3,5,9) enumerates (5,3) (5,5) (5,9) (3,5) (3,9) (5,9); track 1 has two rows and
    is skipped; track 2 (7,3,9) continues at ordinal 6."""
    ptr = np.array([0, 4, 6, 9])
    img = np.array([5, 3, 5, 9, 1, 2, 7, 3, 9])
    lo, hi, count, first, total = covis.host_pairs(ptr, img, min_count=1)
    assert total == 9
    assert list(zip(lo.tolist(), hi.tolist(), count.tolist(), first.tolist())) == [
        (3, 5, 2, 0), (5, 9, 2, 2), (3, 9, 2, 4), (3, 7, 1, 6), (7, 9, 1, 7)]
    lo, hi, count, first, _ = covis.host_pairs(ptr, img, min_count=2)
    assert list(zip(lo.tolist(), hi.tolist())) == [(3, 5), (5, 9), (3, 9)]
    with pytest.raises(ValueError):
        covis.host_pairs(np.array([0, 4, 3]), img)


def test_union_find_direction():
    """Union(x, y) hangs x's root under y's root."""
    uf = UnionFind()
    uf.Union(5, 2)
    assert uf.Find(5) == 2 and uf.Find(2) == 2
    uf.Union(2, 9)
    assert uf.Find(5) == 9
    uf.Union(7, 5)
    assert uf.Find(7) == 9 and uf.Find(11) == 11


def test_mapper_accepts_the_pruning_switch():
    """for_ba_half() leaves pruning off (the reference default); with pruning=True the mapper passes its stage check
    (and then fails on the empty scene handed to it here, not with NotImplementedError)."""
    assert Config.for_ba_half().OPTIONS['skip_pruning'] is True
    assert 'skip_pruning' not in OUT_OF_SCOPE_STAGES and len(OUT_OF_SCOPE_STAGES) == 4
    cfg = Config.for_ba_half(pruning=True)
    assert cfg.OPTIONS['skip_pruning'] is False
    with pytest.raises(Exception) as e:
        SolveGlobalMapper(None, [], [], cfg)
    assert not isinstance(e.value, NotImplementedError), e.value
