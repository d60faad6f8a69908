"""PruneWeaklyConnectedImages / EstablishStrongClusters -- drop-in for
``instantsfm/processors/reconstruction_pruning.py`` (reference :109-210).

The visibility graph -- how many track-row pairs every two images share (:173-191), the reference's Python double loop
over every track -- is counted on the MI355X (``instantsfm_amd.covis``, csrc/covis.hip) and arrives in the insertion
order of the reference's dict.  Everything after it works on at most M(M-1)/2 pairs and depends on iteration order
(threshold, union-find direction, component discovery, cluster ranking), so it stays on the host and follows the
reference statement by statement.  Side effects are the reference's: ``image.is_registered`` and ``image.cluster_id``.
"""
import numpy as np

from ..covis import covis_pairs
from ..scene.defs import ImagePair, Ids2PairId, ViewGraph
from ..utils.union_find import UnionFind
from .track_filter import collect_tracks


def EstablishStrongClusters(view_graph: ViewGraph, images, threshold, min_num_images):
    """:109-170.  Images joined by pairs of weight > threshold form the initial clusters; for at most 10 rounds, two
    clusters joined by two or more pairs of weight >= 0.75 * threshold merge; pairs across the final clusters become
    invalid and the remaining components are numbered by size."""
    view_graph.keep_largest_connected_component(images)

    def valid_pairs():
        return (pair for pair in view_graph.image_pairs.values() if pair.is_valid)

    uf = UnionFind()
    for pair in valid_pairs():
        if pair.weight > threshold:
            uf.Union(pair.image_id1, pair.image_id2)

    iteration = 0
    merged = True
    while merged:
        merged = False
        iteration += 1
        if iteration > 10:
            break
        num_pairs = {}  # root -> {other root -> weaker pairs between the two}, both in order of first sight
        for pair in valid_pairs():
            if pair.weight < 0.75 * threshold:
                continue
            root1, root2 = uf.Find(pair.image_id1), uf.Find(pair.image_id2)
            if root1 == root2:
                continue
            row1, row2 = num_pairs.setdefault(root1, {}), num_pairs.setdefault(root2, {})
            row1[root2] = row1.get(root2, 0) + 1
            row2[root1] = row2.get(root1, 0) + 1
        for root1, counter in num_pairs.items():
            for root2, count in counter.items():
                if root1 > root2 and count >= 2:
                    merged = True
                    uf.Union(root1, root2)

    for pair in valid_pairs():
        if uf.Find(pair.image_id1) != uf.Find(pair.image_id2):
            pair.is_valid = False
    num_comp = view_graph.mark_connected_components(images)
    print(f"Clustering take {iteration} iterations. Images are grouped into {num_comp} clusters after strong-clustering")


def _track_rows(tracks):
    """(track_ptr [T+1] int64, image of every observation row) over the tracks in dict order."""
    got = collect_tracks(tracks) if tracks else None
    if got is not None:
        counts, allobs = got[0], got[1]
    else:
        obs = [np.asarray(t.observations).reshape(-1, 2) for t in tracks.values()]
        counts = np.array([o.shape[0] for o in obs], dtype=np.int64)
        allobs = np.concatenate(obs) if obs else np.zeros((0, 2), np.int64)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), allobs[:, 0].astype(np.int32)


def visibility_graph(lo, hi, count):
    """:205-208: one ImagePair per counted image pair, in the given order.  ``PairId2Ids`` hands the larger id back
    first, so ``image_id1`` is the larger one."""
    view_graph = ViewGraph()
    for a, b, c in zip(lo.tolist(), hi.tolist(), count.tolist()):
        view_graph.image_pairs[Ids2PairId(a, b)] = ImagePair(image_id1=b, image_id2=a, weight=c)
    return view_graph


def strong_cluster_threshold(count):
    """:194-209: median minus median absolute deviation of the pair counts, both taken as sorted[len // 2], at least
    20.  IndexError on an empty graph, as in the reference."""
    pair_count = np.sort(np.asarray(count, dtype=np.int64))
    median_count = pair_count[len(pair_count) // 2]
    pair_count_diff = np.sort(np.abs(pair_count - median_count))
    median_count_diff = pair_count_diff[len(pair_count_diff) // 2]
    print(f"Threshold for Strong Clustering: {median_count - median_count_diff}")
    return max(median_count - median_count_diff, 20)


def PruneWeaklyConnectedImages(images, tracks, min_num_images=2, device="cuda:0"):
    """:172-210.  ``device="cpu"`` counts the pairs with numpy instead of the HIP kernels (same list, same order)."""
    track_ptr, obs_img = _track_rows(tracks)
    lo, hi, count = covis_pairs(track_ptr, obs_img, min_count=5, device=device)
    print(f"Established visibility graph with {len(count)} pairs")
    threshold = strong_cluster_threshold(count)
    EstablishStrongClusters(visibility_graph(lo, hi, count), images, threshold, min_num_images)
