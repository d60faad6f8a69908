"""FilterInlierNum / FilterInlierRatio -- drop-ins for ``instantsfm/processors/relpose_filter.py`` (reference :25-43),
the view-graph filters after ImagePairInliersCount.  Host code: one pass collects the valid pairs' inlier and match
counts, the comparison is vectorised, the printed lines are the reference's.  ``FilterRotations`` (:5-23) belongs to
rotation averaging and is not part of this build.
"""
import numpy as np

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
