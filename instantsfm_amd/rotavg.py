"""Rotation averaging (include/insfm_rotavg.h): numpy in, numpy out, csrc/rotavg.hip in between.

``flatten`` turns the view graph into the library's arrays the way ``RotationEstimator.SetupLinearSystem``
(processors/rotation_averaging.py:42-52) numbers things: the registered images in image order get the dense indices
0 .. n-1, the valid pairs in view-graph order the rows 0 .. P-1.  ``solve`` runs SolveL1Regression and SolveIRLS on the
device; ``residuals``, ``update`` and ``system`` are its three stages on their own; ``pair_errors`` is FilterRotations'
angle, on the device or -- for ``device`` ``"cpu"`` / ``None`` -- in numpy (``host_pair_errors``).  The ``device_*``
functions are one raw library call each and return the return code with the buffers.
"""
import ctypes
from dataclasses import dataclass

import numpy as np

from . import _capi
from .utils.rotation import quat_to_matrix

MAX_IMAGES = 8192        # INSFM_ROTAVG_MAX_IMAGES: three n x n float64 buffers per call, 1.5 GiB at the limit
INFO_LEN = 16
INFO_L1_ITERS, INFO_ADMM, INFO_IRLS_ITERS, INFO_FAILED = 0, 1, 11, 12
FAILED_L1, FAILED_IRLS = 1, 2


@dataclass
class Flat:
    """The pair arrays of one insfm_rotavg_* call and what they describe."""
    pairs: list              # the valid ImagePair objects, in view-graph order
    keys: list               # their view-graph keys
    pair_i: np.ndarray       # int32 [P] dense index of image_id1
    pair_j: np.ndarray       # int32 [P] dense index of image_id2
    quat: np.ndarray         # float64 [P, 4] pair.rotation (xyzw)
    image_ids: list          # dense index -> image id (position in ``images``)
    id2idx: dict             # image id -> dense index

    @property
    def n(self):
        return len(self.image_ids)

    @property
    def n_pairs(self):
        return int(self.pair_i.shape[0])


def flatten(view_graph, images):
    """The valid pairs of ``view_graph`` (view-graph order) over the registered images (image order).  A valid pair
    that touches an unregistered image raises KeyError, as the reference's ``image_id2idx[image_id1]`` does."""
    image_ids = [image_id for image_id, image in enumerate(images) if image.is_registered]
    id2idx = {image_id: k for k, image_id in enumerate(image_ids)}
    pairs, keys = [], []
    for key, pair in view_graph.image_pairs.items():
        if pair.is_valid:
            pairs.append(pair)
            keys.append(key)
    pair_i = np.array([id2idx[pair.image_id1] for pair in pairs], dtype=np.int32)
    pair_j = np.array([id2idx[pair.image_id2] for pair in pairs], dtype=np.int32)
    quat = np.array([np.asarray(pair.rotation, dtype=np.float64) for pair in pairs], dtype=np.float64).reshape(-1, 4)
    return Flat(pairs, keys, pair_i, pair_j, quat, image_ids, id2idx)


def make_options(ROTATION_ESTIMATOR_OPTIONS, L1_SOLVER_OPTIONS):
    """insfm_rotavg_options from the two option tables (sigma goes from degrees to radians, as :129 does)."""
    ro, lo = ROTATION_ESTIMATOR_OPTIONS, L1_SOLVER_OPTIONS
    return _capi.RotavgOptions(
        int(ro['max_num_l1_iterations']), int(ro['max_num_irls_iterations']),
        float(ro['l1_step_convergence_threshold']), float(ro['irls_step_convergence_threshold']),
        float(np.deg2rad(ro['irls_loss_parameter_sigma'])),
        float(lo['rho']), float(lo['alpha']), float(lo['absolute_tolerance']), float(lo['relative_tolerance']))


def _check_n(n):
    if n > MAX_IMAGES:
        raise ValueError(f"rotation averaging holds dense {n} x {n} float64 buffers; this build supports at most "
                         f"{MAX_IMAGES} registered images (INSFM_ROTAVG_MAX_IMAGES)")


class _Call:
    """Device copies of the pair arrays for one library call."""

    def __init__(self, device, pair_i, pair_j, quat=None):
        from .engine import _require_gpu
        from .passes import _dev, _p, _stream
        self.dev = _require_gpu(device)
        self.lib = _capi.load()
        self.p, self.stream = _p, _stream(self.dev)
        self._dev = _dev
        self.P = int(np.asarray(pair_i).shape[0])
        self.pi = self.up(pair_i, np.int32)
        self.pj = self.up(pair_j, np.int32)
        self.quat = self.up(np.asarray(quat, np.float64).reshape(-1, 4), np.float64, 4) if quat is not None else None

    def up(self, a, dt, width=1):
        a = np.ascontiguousarray(a, dtype=dt)
        return self._dev(a if a.size else np.zeros((1, width) if width > 1 else 1, dt), self.dev)


def device_solve(n, pair_i, pair_j, quat, rot, fixed, fixed_rot, options, device="cuda:0"):
    """One insfm_rotavg_solve call: (return code, rot [n, 3], info [INFO_LEN]).  ``options`` is a
    ``_capi.RotavgOptions`` (``make_options``)."""
    c = _Call(device, pair_i, pair_j, quat)
    d_rot = c.up(np.asarray(rot, np.float64).reshape(n, 3), np.float64, 3)
    d_fix = c.up(np.asarray(fixed_rot, np.float64).reshape(3), np.float64)
    info = (ctypes.c_int32 * INFO_LEN)(*([-1] * INFO_LEN))
    rc = c.lib.insfm_rotavg_solve(n, c.P, c.p(c.pi), c.p(c.pj), c.p(c.quat), c.p(d_rot), int(fixed), c.p(d_fix),
                                  ctypes.byref(options), info, c.stream)
    return rc, d_rot.cpu().numpy()[:n], np.array(info[:], dtype=np.int32)


def solve(n, pair_i, pair_j, quat, rot, fixed, fixed_rot, ROTATION_ESTIMATOR_OPTIONS, L1_SOLVER_OPTIONS,
          device="cuda:0"):
    """SolveL1Regression + SolveIRLS: (ok, rot [n, 3], info).  ``ok`` is False after a NaN step or weight (the
    reference's ``return False``; ``rot`` is then the input).  Raises ValueError above MAX_IMAGES and BAError for every
    other refusal, a singular system (INSFM_BA_ESOLVER) included."""
    _check_n(n)
    rc, out, info = device_solve(n, pair_i, pair_j, quat, rot, fixed, fixed_rot,
                                 make_options(ROTATION_ESTIMATOR_OPTIONS, L1_SOLVER_OPTIONS), device)
    if rc != 0:
        raise _capi.BAError(rc, "insfm_rotavg_solve" + (": the system is singular (an image has no path of valid "
                                                          "pairs to the fixed image)"
                                                          if rc == _capi.INSFM_BA_ESOLVER else ""))
    return int(info[INFO_FAILED]) == 0, out, info


def device_residuals(n, pair_i, pair_j, quat, rot, fixed, fixed_rot, device="cuda:0", fill=np.nan):
    """One insfm_rotavg_residuals call: (return code, res [P + 1, 3])."""
    import torch
    c = _Call(device, pair_i, pair_j, quat)
    d_rot = c.up(np.asarray(rot, np.float64).reshape(n, 3), np.float64, 3)
    d_fix = c.up(np.asarray(fixed_rot, np.float64).reshape(3), np.float64)
    res = torch.full((c.P + 1, 3), fill, dtype=torch.float64, device=c.dev)
    rc = c.lib.insfm_rotavg_residuals(n, c.P, c.p(c.pi), c.p(c.pj), c.p(c.quat), c.p(d_rot), int(fixed), c.p(d_fix),
                                      c.p(res), c.stream)
    return rc, res.cpu().numpy()


def device_update(rot, step, device="cuda:0"):
    """One insfm_rotavg_update call: (return code, rot [n, 3])."""
    c = _Call(device, np.zeros(0, np.int32), np.zeros(0, np.int32))
    rot = np.asarray(rot, np.float64).reshape(-1, 3)
    n = rot.shape[0]
    d_rot = c.up(rot, np.float64, 3)
    d_step = c.up(np.asarray(step, np.float64).reshape(n, 3), np.float64, 3)
    rc = c.lib.insfm_rotavg_update(n, c.p(d_rot), c.p(d_step), c.stream)
    return rc, d_rot.cpu().numpy()[:n]


def device_system(n, pair_i, pair_j, weights, fixed, inverse=False, device="cuda:0", fill=np.nan):
    """One insfm_rotavg_system call: (return code, M [n, n], inverse [n, n] or None)."""
    import torch
    c = _Call(device, pair_i, pair_j)
    d_w = c.up(weights, np.float64) if weights is not None else None
    M = torch.full((n, n), fill, dtype=torch.float64, device=c.dev)
    inv = torch.full((n, n), fill, dtype=torch.float64, device=c.dev) if inverse else None
    rc = c.lib.insfm_rotavg_system(n, c.P, c.p(c.pi), c.p(c.pj), c.p(d_w), int(fixed), c.p(M), c.p(inv), c.stream)
    return rc, M.cpu().numpy(), (inv.cpu().numpy() if inverse else None)


def device_pair_errors(pair_i, pair_j, quat, world2cam, device="cuda:0", fill=np.nan):
    """One insfm_rotavg_pair_errors call: (return code, angle_deg [P]).  ``world2cam`` [n, 3, 3]."""
    import torch
    c = _Call(device, pair_i, pair_j, quat)
    Rw = np.asarray(world2cam, np.float64).reshape(-1, 9)
    d_R = c.up(Rw, np.float64, 9)
    ang = torch.full((max(c.P, 1),), fill, dtype=torch.float64, device=c.dev)
    rc = c.lib.insfm_rotavg_pair_errors(Rw.shape[0], c.P, c.p(c.pi), c.p(c.pj), c.p(c.quat), c.p(d_R), c.p(ang),
                                        c.stream)
    return rc, ang.cpu().numpy()[:c.P]


def host_pair_errors(pair_i, pair_j, quat, world2cam):
    """relpose_filter.py:13-19 in numpy: degrees(acos(clip((trace((R_j R_i^T)^T R_rel) - 1) / 2, -1, 1)))."""
    P = int(np.asarray(pair_i).shape[0])
    if P == 0:
        return np.zeros(0)
    Rw = np.asarray(world2cam, np.float64).reshape(-1, 3, 3)
    R1, R2 = Rw[np.asarray(pair_i)], Rw[np.asarray(pair_j)]
    Rr = quat_to_matrix(np.asarray(quat, np.float64).reshape(-1, 4))
    trace = np.einsum('pac,pbc,pab->p', R2, R1, Rr)
    return np.rad2deg(np.arccos(np.clip((trace - 1) / 2, -1.0, 1.0)))


def pair_errors(pair_i, pair_j, quat, world2cam, device="cuda:0"):
    """The pairs' rotation errors in degrees: the device path, or the host path for ``device`` ``"cpu"`` / ``None``."""
    if device is None or str(device) == "cpu":
        return host_pair_errors(pair_i, pair_j, quat, world2cam)
    rc, ang = device_pair_errors(pair_i, pair_j, quat, world2cam, device)
    if rc != 0:
        raise _capi.BAError(rc, "insfm_rotavg_pair_errors")
    return ang
