"""Rotation conversions in numpy (no scipy in the package code): what ``scipy.spatial.transform.Rotation`` does in
``from_matrix`` / ``from_quat`` / ``from_rotvec`` and ``as_matrix`` / ``as_quat(canonical=False)`` / ``as_rotvec``, for
one rotation or a batch (leading axes).  Quaternions are xyzw.  The series branches and their 1e-3 threshold are
scipy's; csrc/rotavg.hip uses the same maps on the device.
"""
import numpy as np

_SMALL = 1e-3


def quat_to_matrix(q):
    """``Rotation.from_quat(q).as_matrix()``: the quaternion is normalised first."""
    q = np.asarray(q, dtype=np.float64)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    x, y, z, w = np.moveaxis(q, -1, 0)
    return np.stack([
        np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
        np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
        np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def matrix_to_quat(R):
    """``Rotation.from_matrix(R).as_quat(canonical=False)`` for proper rotation matrices: the largest of the three
    diagonal entries and the trace picks the component that is computed from a sum, the others follow from the
    off-diagonal sums and differences."""
    R = np.asarray(R, dtype=np.float64)
    lead = R.shape[:-2]
    M = R.reshape(-1, 3, 3)
    out = np.empty((M.shape[0], 4))
    trace = M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2]
    choice = np.argmax(np.stack([M[:, 0, 0], M[:, 1, 1], M[:, 2, 2], trace], 1), axis=1)
    for n, (m, c) in enumerate(zip(M, choice.tolist())):
        if c == 3:
            out[n] = (m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1], 1 + trace[n])
        else:
            i, j, k = c, (c + 1) % 3, (c + 2) % 3
            out[n, i] = 1 - trace[n] + 2 * m[i, i]
            out[n, j] = m[j, i] + m[i, j]
            out[n, k] = m[k, i] + m[i, k]
            out[n, 3] = m[k, j] - m[j, k]
    out /= np.linalg.norm(out, axis=1, keepdims=True)
    return out.reshape(lead + (4,))


def rotvec_to_quat(v):
    """``Rotation.from_rotvec(v).as_quat()``."""
    v = np.asarray(v, dtype=np.float64)
    a = np.linalg.norm(v, axis=-1, keepdims=True)
    a2 = a * a
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(a <= _SMALL, 0.5 - a2 / 48 + a2 * a2 / 3840, np.sin(a / 2) / a)
    return np.concatenate([s * v, np.cos(a / 2)], axis=-1)


def quat_to_rotvec(q):
    """``Rotation.from_quat(q).as_rotvec()``: angle in [0, pi] (the quaternion is negated when w < 0)."""
    q = np.asarray(q, dtype=np.float64)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    q = np.where(q[..., 3:4] < 0, -q, q)
    nv = np.linalg.norm(q[..., :3], axis=-1, keepdims=True)
    a = 2 * np.arctan2(nv, q[..., 3:4])
    a2 = a * a
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(a <= _SMALL, 2 + a2 / 12 + 7 * a2 * a2 / 2880, a / np.sin(a / 2))
    return s * q[..., :3]


def rotvec_to_matrix(v):
    return quat_to_matrix(rotvec_to_quat(v))


def matrix_to_rotvec(R):
    return quat_to_rotvec(matrix_to_quat(R))
