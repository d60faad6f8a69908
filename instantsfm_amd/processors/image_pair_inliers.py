"""ImagePairInliersCount -- drop-in for ``instantsfm/processors/image_pair_inliers.py`` (reference :1-133).

The reference walks every match of every valid pair in Python (``score_error_homography`` / ``_fundamental`` /
``_essential``); here the view graph is flattened once on the host (``pair_inliers.flatten``) and every match is
evaluated in csrc/pair_inliers.hip (``insfm_pair_inliers``), one wave per pair.  ``pair.inliers`` is assigned exactly
where the reference assigns it -- not for a pair of another configuration, nor for an UNCALIBRATED pair whose
orientation vote ties -- as an int64 array of ascending match indices.  CALIBRATED pairs read ``features_undist``
(``UndistortImages`` first) and ``pair.rotation`` / ``pair.translation``.
"""
import numpy as np

from .. import pair_inliers as PI
from ..scene.defs import ViewGraph


def ImagePairInliersCount(view_graph: ViewGraph, cameras, images, INLIER_THRESHOLD_OPTIONS, device="cuda:0",
                          scores=None):
    """image_pair_inliers.py:127-133.  ``scores`` (optional dict) receives what the reference's ``score_error``
    returns for every valid pair, under the pair's view-graph key.  ``device="cpu"`` runs the numpy host path."""
    flat = PI.flatten(view_graph, cameras, images, INLIER_THRESHOLD_OPTIONS)
    idx, count, score, touched = PI.score(flat, device)
    parts = np.split(idx.astype(np.int64), np.cumsum(count)[:-1]) if flat.n_pairs else []
    for pair, inl, t in zip(flat.pairs, parts, touched.tolist()):
        if t:
            pair.inliers = inl
    if scores is not None:
        scores.update(zip(flat.keys, score.tolist()))
