"""RotationEstimator -- drop-in for ``instantsfm/processors/rotation_averaging.py`` (reference :12-195).

The reference runs ComputeResiduals and UpdateGlobalRotations as Python loops over scipy rotations, once per L1 and
IRLS iteration, and refactors a sparse matrix per IRLS iteration.  Here the spanning-tree initialisation (:16-39, a walk
of n - 1 3x3 products) stays on the host and everything from SetupLinearSystem's arrays on is one
``insfm_rotavg_solve`` call (``rotavg.solve``, csrc/rotavg.hip): the system is (B^T W B) (x) I3, inverted densely on
the device.  At most ``rotavg.MAX_IMAGES`` registered images.

Same return value and side effects as the reference: True and ``image.world2cam[:3, :3]`` of every registered image
set, or False (a NaN step or weight) with the images as the initialisation left them.  ``fixed_camera_id`` and the
rotation it is held at are chosen on the first call and kept for later calls on the same instance.  A system that
cannot be solved (an image without a path of valid pairs to the fixed one) raises ``BAError``.
"""
from collections import deque

import numpy as np

from .. import rotavg as RA
from ..scene.defs import Ids2PairId, ViewGraph
from ..utils.rotation import quat_to_matrix, rotvec_to_matrix
from ..utils.tree import MaximumSpanningTree


class RotationEstimator:
    def __init__(self, device="cuda:0"):
        self.fixed_camera_id = -1
        self.fixed_camera_rotation = None
        self.device = device
        self.info = None           # insfm_rotavg_solve's info of the last call (iteration counts)

    def InitializeFromMaximumSpanningTree(self, view_graph: ViewGraph, images):
        """:16-39.  (``children[parent]`` with parent -1 lands in the last image's list, as in the reference; such an
        entry is reached only if the last image is reachable, and is then skipped by the ``parents[current] == -1``
        test.)"""
        parents, root = MaximumSpanningTree(view_graph, images)
        children = [[] for _ in range(len(images))]
        for idx, parent in enumerate(parents):
            if idx != root:
                children[parent].append(idx)
        queue = deque([root])
        while queue:
            current = queue.popleft()
            queue.extend(children[current])
            if current == root or parents[current] == -1:
                continue
            pair = view_graph.image_pairs[Ids2PairId(current, parents[current])]
            pair_rotation = quat_to_matrix(pair.rotation)
            parent_rotation = images[parents[current]].world2cam[:3, :3]
            if pair.image_id1 == current:
                images[current].world2cam[:3, :3] = np.linalg.inv(pair_rotation) @ parent_rotation
            else:
                images[current].world2cam[:3, :3] = pair_rotation @ parent_rotation

    def SetupLinearSystem(self, view_graph: ViewGraph, images):
        """:41-82: the dense arrays instead of the sparse matrix."""
        self.flat = RA.flatten(view_graph, images)
        self.images = {image_id: images[image_id] for image_id in self.flat.image_ids}
        self.image_pairs = dict(zip(self.flat.keys, self.flat.pairs))
        self.image_id2idx = {image_id: 3 * k for image_id, k in self.flat.id2idx.items()}
        self.rotation_estimated = np.zeros(len(images) * 3)
        for image_id, k in self.flat.id2idx.items():
            self.rotation_estimated[3 * k:3 * k + 3] = images[image_id].axis_angle()
        if self.fixed_camera_id == -1:
            self.fixed_camera_id = self.flat.image_ids[0]
            self.fixed_camera_rotation = self.images[self.fixed_camera_id].axis_angle()

    def EstimateRotations(self, view_graph: ViewGraph, images, ROTATION_ESTIMATOR_OPTIONS, L1_SOLVER_OPTIONS):
        """:177-195."""
        self.InitializeFromMaximumSpanningTree(view_graph, images)
        self.SetupLinearSystem(view_graph, images)
        flat, n = self.flat, self.flat.n
        fixed = flat.id2idx[self.fixed_camera_id]  # (KeyError when the fixed image is no longer registered, as :76)
        ok, rot, self.info = RA.solve(n, flat.pair_i, flat.pair_j, flat.quat, self.rotation_estimated[:3 * n],
                                      fixed, self.fixed_camera_rotation, ROTATION_ESTIMATOR_OPTIONS,
                                      L1_SOLVER_OPTIONS, device=self.device)
        if not ok:
            print('nan error' if self.info[RA.INFO_FAILED] == RA.FAILED_L1 else 'nan weight!')
            return False
        self.rotation_estimated[:3 * n] = np.asarray(rot).reshape(-1)
        matrices = rotvec_to_matrix(np.asarray(rot).reshape(n, 3))
        for k, image_id in enumerate(flat.image_ids):
            images[image_id].world2cam[:3, :3] = matrices[k]
        view_graph.image_pairs.update(self.image_pairs)
        return True
