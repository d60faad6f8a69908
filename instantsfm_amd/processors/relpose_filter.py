"""FilterRotations / FilterInlierNum / FilterInlierRatio -- drop-ins for ``instantsfm/processors/relpose_filter.py``
(reference :5-43), the view-graph filters after rotation averaging and after ImagePairInliersCount.  The inlier filters
are host code: one pass collects the valid pairs' inlier and match counts, the comparison is vectorised.
``FilterRotations`` computes every pair's angle in one ``insfm_rotavg_pair_errors`` call (csrc/rotavg.hip), or in numpy
for ``device`` ``"cpu"`` / ``None``.  The printed lines are the reference's.
"""
import numpy as np

from .. import rotavg as RA
from ..scene.defs import ViewGraph


def _valid_counts(view_graph):
    pairs = [pair for pair in view_graph.image_pairs.values() if pair.is_valid]
    n_inl = np.array([len(pair.inliers) for pair in pairs], dtype=np.int64)
    n_match = np.array([len(pair.matches) for pair in pairs], dtype=np.int64)
    return pairs, n_inl, n_match


def _invalidate(pairs, drop):
    for k in np.flatnonzero(drop).tolist():
        pairs[k].is_valid = False
    return int(np.count_nonzero(drop))


def FilterRotations(view_graph: ViewGraph, images, max_angle, device="cuda:0"):
    """relpose_filter.py:5-23: a valid pair between two registered images whose rotation differs from the images'
    relative rotation by more than ``max_angle`` degrees becomes invalid (a NaN angle leaves it valid, as the
    reference's comparison does)."""
    pairs = [pair for pair in view_graph.image_pairs.values()
             if pair.is_valid and images[pair.image_id1].is_registered and images[pair.image_id2].is_registered]
    pair_i = np.array([pair.image_id1 for pair in pairs], dtype=np.int32)
    pair_j = np.array([pair.image_id2 for pair in pairs], dtype=np.int32)
    quat = np.array([np.asarray(pair.rotation, dtype=np.float64) for pair in pairs]).reshape(-1, 4)
    world2cam = np.array([image.world2cam[:3, :3] for image in images], dtype=np.float64).reshape(-1, 3, 3)
    angle = RA.pair_errors(pair_i, pair_j, quat, world2cam, device=device)
    with np.errstate(invalid="ignore"):
        num_invalid = _invalidate(pairs, angle > max_angle)
    print('Filtered', num_invalid, 'relative rotation with angle >', max_angle, 'degrees')


def FilterInlierNum(view_graph: ViewGraph, min_inlier_num):
    """relpose_filter.py:25-33: a valid pair with fewer than ``min_inlier_num`` inliers becomes invalid."""
    pairs, n_inl, _ = _valid_counts(view_graph)
    num_invalid = _invalidate(pairs, n_inl < min_inlier_num)
    print('Filtered', num_invalid, 'relative pose with inlier number <', min_inlier_num)


def FilterInlierRatio(view_graph: ViewGraph, min_inlier_ratio):
    """relpose_filter.py:35-43: a valid pair whose inliers are less than ``min_inlier_ratio`` of its matches becomes
    invalid.  A valid pair without matches raises ZeroDivisionError, as the reference's division does."""
    pairs, n_inl, n_match = _valid_counts(view_graph)
    if (n_match == 0).any():
        raise ZeroDivisionError("division by zero")
    num_invalid = _invalidate(pairs, n_inl / n_match < min_inlier_ratio)
    print('Filtered', num_invalid, 'relative pose with inlier ratio <', min_inlier_ratio)
