"""Rotation averaging restated in numpy / scipy for the tests: RotationEstimator (processors/rotation_averaging.py:12-195)
with L1Solver (utils/l1_solver.py:5-43), statement by statement, on scipy ``Rotation`` objects and the dense
(B^T W B) (x) I3 system solved by ``scipy.linalg.cho_solve`` (the reference's sparse Cholesky is not installed
here).  Written from the algorithm; nothing here is used by the package.

``solve`` works on the dense arrays of ``instantsfm_amd.rotavg.flatten`` and has ``rotavg.solve``'s signature, so a test
can put it in its place.  ``solve_with_gap`` also returns the smallest relative gap |a - b| / max(|a|, |b|) over every
convergence comparison ``a < b`` made on the way: how far the iteration counts are from depending on rounding.
``Estimator`` is the whole EstimateRotations, spanning-tree initialisation included.
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve
from scipy.spatial.transform import Rotation as R

INFO_LEN = 16
INFO_L1_ITERS, INFO_ADMM, INFO_IRLS_ITERS, INFO_FAILED = 0, 1, 11, 12


class _Gaps:
    def __init__(self):
        self.smallest = np.inf

    def less(self, a, b):
        scale = max(abs(a), abs(b))
        if scale > 0 and np.isfinite(scale):
            self.smallest = min(self.smallest, abs(a - b) / scale)
        return a < b


def incidence(n, pair_i, pair_j, fixed):
    """B: one row per pair (-1 at image 1, +1 at image 2) and the gauge row."""
    P = len(pair_i)
    B = np.zeros((P + 1, n))
    B[np.arange(P), np.asarray(pair_i, int)] = -1.0
    B[np.arange(P), np.asarray(pair_j, int)] = 1.0
    B[P, fixed] = 1.0
    return B


def residuals(pair_i, pair_j, R_rel, rot, fixed, fixed_rot):
    """ComputeResiduals (:84-98): [P + 1, 3]."""
    P = len(pair_i)
    res = np.zeros((P + 1, 3))
    for k in range(P):
        R1 = R.from_rotvec(rot[pair_i[k]]).as_matrix()
        R2 = R.from_rotvec(rot[pair_j[k]]).as_matrix()
        res[k] = -R.from_matrix(R2.T @ R_rel[k] @ R1).as_rotvec()
    res[P] = R.from_matrix(R.from_rotvec(fixed_rot).as_matrix().T @ R.from_rotvec(rot[fixed]).as_matrix()).as_rotvec()
    return res


def update(rot, step):
    """UpdateGlobalRotations (:163-168)."""
    out = np.empty_like(rot)
    for a in range(rot.shape[0]):
        out[a] = R.from_matrix(R.from_rotvec(rot[a]).as_matrix() @ R.from_rotvec(-step[a]).as_matrix()).as_rotvec()
    return out


def _shrinkage(v, kappa):
    return np.maximum(0, v - kappa) - np.maximum(0, -v - kappa)


def _l1_solve(B, chol, rhs, max_iterations, lo, gaps):
    """L1Solver.solve (l1_solver.py:11-39) on [rows, 3] arrays (the three coordinates share B).  Returns x and the
    number of iterations run."""
    n, m = B.shape[1], B.shape[0]
    x, z, u = np.zeros((n, 3)), np.zeros((m, 3)), np.zeros((m, 3))
    rhs_norm = np.linalg.norm(rhs)
    primal_abs = np.sqrt(3 * m) * lo['absolute_tolerance']
    dual_abs = np.sqrt(3 * n) * lo['absolute_tolerance']
    count = 0
    for _ in range(max_iterations):
        count += 1
        x = cho_solve(chol, B.T @ (rhs + z - u))
        a_times_x = B @ x
        ax_hat = lo['alpha'] * a_times_x + (1.0 - lo['alpha']) * (z + rhs)
        z_old = z.copy()
        z = _shrinkage(ax_hat - rhs + u, 1.0 / lo['rho'])
        u = u + ax_hat - z - rhs
        r_norm = np.linalg.norm(a_times_x - z - rhs)
        s_norm = np.linalg.norm(-lo['rho'] * B.T @ (z - z_old))
        max_norm = max(np.linalg.norm(a_times_x), np.linalg.norm(z), rhs_norm)
        primal_eps = primal_abs + lo['relative_tolerance'] * max_norm
        dual_eps = dual_abs + lo['relative_tolerance'] * np.linalg.norm(lo['rho'] * B.T @ u)
        first, second = gaps.less(r_norm, primal_eps), gaps.less(s_norm, dual_eps)
        if first and second:
            break
    return x, count


def solve_with_gap(n, pair_i, pair_j, quat, rot, fixed, fixed_rot, ro, lo):
    """(ok, rot [n, 3], info [INFO_LEN], smallest decision gap)."""
    pair_i, pair_j = np.asarray(pair_i, int), np.asarray(pair_j, int)
    P = len(pair_i)
    R_rel = R.from_quat(np.asarray(quat, float).reshape(-1, 4)).as_matrix() if P else np.zeros((0, 3, 3))
    rot = np.array(rot, dtype=np.float64).reshape(n, 3)
    start = rot.copy()
    fixed_rot = np.asarray(fixed_rot, float)
    B = incidence(n, pair_i, pair_j, fixed)
    gaps = _Gaps()
    info = np.zeros(INFO_LEN, np.int32)
    n_avg = lambda step: np.linalg.norm(step, axis=1).sum() / n   # ComputeAverageStepSize (:170-175)

    if ro['max_num_l1_iterations'] > 0:                           # SolveL1Regression (:100-124)
        res = residuals(pair_i, pair_j, R_rel, rot, fixed, fixed_rot)
        chol = cho_factor(B.T @ B)
        iteration, curr_norm, cap = 0, 0.0, 10
        while iteration < ro['max_num_l1_iterations']:
            last_norm = curr_norm
            step, count = _l1_solve(B, chol, res, cap, lo, gaps)
            if iteration < 10:
                info[INFO_ADMM + iteration] = count
            info[INFO_L1_ITERS] = iteration + 1
            if np.any(np.isnan(step)):
                info[INFO_FAILED] = 1
                return False, start, info, gaps.smallest
            curr_norm = np.linalg.norm(step)
            rot = update(rot, step)
            res = residuals(pair_i, pair_j, R_rel, rot, fixed, fixed_rot)
            iteration += 1
            first = gaps.less(n_avg(step), ro['l1_step_convergence_threshold'])
            second = gaps.less(np.abs(last_norm - curr_norm), 1e-6)
            if first or second:
                break
            cap = min(cap * 2, 100)

    if ro['max_num_irls_iterations'] > 0:                         # SolveIRLS (:126-161)
        sigma = np.deg2rad(ro['irls_loss_parameter_sigma'])
        res = residuals(pair_i, pair_j, R_rel, rot, fixed, fixed_rot)
        for it in range(ro['max_num_irls_iterations']):
            info[INFO_IRLS_ITERS] = it + 1
            weights = np.ones(P + 1)
            weights[:P] = sigma ** 2 / (np.sum(res[:P] ** 2, axis=1) + sigma ** 2) ** 2
            if np.any(np.isnan(weights)):
                info[INFO_FAILED] = 2
                return False, start, info, gaps.smallest
            at_weight = B.T * weights
            step = cho_solve(cho_factor(at_weight @ B), at_weight @ res)
            rot = update(rot, step)
            res = residuals(pair_i, pair_j, R_rel, rot, fixed, fixed_rot)
            if gaps.less(n_avg(step), ro['irls_step_convergence_threshold']):
                break
    return True, rot, info, gaps.smallest


def solve(n, pair_i, pair_j, quat, rot, fixed, fixed_rot, ROTATION_ESTIMATOR_OPTIONS, L1_SOLVER_OPTIONS, device=None):
    """``instantsfm_amd.rotavg.solve``'s signature and return value."""
    return solve_with_gap(n, pair_i, pair_j, quat, rot, fixed, fixed_rot, ROTATION_ESTIMATOR_OPTIONS,
                          L1_SOLVER_OPTIONS)[:3]


def maximum_spanning_parents(view_graph, images):
    """utils/tree.py:25-47: the edges heaviest first (of equally heavy ones the earliest pair of the view graph), each
    kept when it joins two components (tracked by relabelling, no union-find), then the parents from a walk from
    image 0."""
    n = len(images)
    edges = [(len(p.inliers), -order, p.image_id1, p.image_id2)
             for order, p in enumerate(view_graph.image_pairs.values())
             if p.is_valid and images[p.image_id1].is_registered and images[p.image_id2].is_registered]
    label = list(range(n))
    adj = [[] for _ in range(n)]
    for _, _, u, v in sorted(edges, reverse=True):
        if label[u] != label[v]:
            old, new = label[u], label[v]
            label = [new if x == old else x for x in label]
            adj[u].append(v)
            adj[v].append(u)
    parents = [-1] * n
    parents[0] = 0
    stack = [0]
    while stack:
        cur = stack.pop()
        for nb in adj[cur]:
            if parents[nb] == -1:
                parents[nb] = cur
                stack.append(nb)
    return parents


class Estimator:
    """EstimateRotations (:177-195) on the scene classes, with the fixed image kept across calls."""

    def __init__(self):
        self.fixed_camera_id = -1
        self.fixed_camera_rotation = None
        self.info = None
        self.gap = np.inf

    def estimate(self, view_graph, images, ro, lo):
        parents = maximum_spanning_parents(view_graph, images)
        depth_order = sorted((i for i in range(len(images)) if parents[i] not in (-1, i)),
                             key=lambda i: self._depth(parents, i))
        lookup = {(p.image_id1, p.image_id2): p for p in view_graph.image_pairs.values()}
        for cur in depth_order:                                   # InitializeFromMaximumSpanningTree (:16-39)
            par = parents[cur]
            pair = lookup.get((cur, par)) or lookup[(par, cur)]
            Rp = R.from_quat(pair.rotation).as_matrix()
            parent_R = images[par].world2cam[:3, :3]
            images[cur].world2cam[:3, :3] = (np.linalg.inv(Rp) if pair.image_id1 == cur else Rp) @ parent_R
        ids = [i for i, im in enumerate(images) if im.is_registered]
        idx = {i: k for k, i in enumerate(ids)}
        pairs = [p for p in view_graph.image_pairs.values() if p.is_valid]
        rot = np.array([R.from_matrix(images[i].world2cam[:3, :3]).as_rotvec() for i in ids]).reshape(-1, 3)
        if self.fixed_camera_id == -1:
            self.fixed_camera_id = ids[0]
            self.fixed_camera_rotation = rot[0].copy()
        ok, rot, self.info, gap = solve_with_gap(
            len(ids), [idx[p.image_id1] for p in pairs], [idx[p.image_id2] for p in pairs],
            np.array([p.rotation for p in pairs], float).reshape(-1, 4), rot, idx[self.fixed_camera_id],
            self.fixed_camera_rotation, ro, lo)
        self.gap = min(self.gap, gap)
        if ok:
            for k, i in enumerate(ids):
                images[i].world2cam[:3, :3] = R.from_rotvec(rot[k]).as_matrix()
        return ok

    @staticmethod
    def _depth(parents, i):
        d = 0
        while parents[i] != i:
            i, d = parents[i], d + 1
        return d


def filter_rotations(view_graph, images, max_angle):
    """FilterRotations (relpose_filter.py:5-23) as the direct loop; returns the angles of the pairs it looked at."""
    angles = []
    for pair in view_graph.image_pairs.values():
        if not pair.is_valid:
            continue
        image1, image2 = images[pair.image_id1], images[pair.image_id2]
        if image1.is_registered and image2.is_registered:
            pose1 = image2.world2cam @ np.linalg.inv(image1.world2cam)
            rotation_matrix = np.linalg.inv(pose1[:3, :3]) @ R.from_quat(pair.rotation).as_matrix()
            cos_r = np.clip((np.trace(rotation_matrix) - 1) / 2, -1.0, 1.0)
            angle = np.rad2deg(np.arccos(cos_r))
            angles.append(angle)
            if angle > max_angle:
                pair.is_valid = False
    return np.array(angles)
