"""Image-pair inlier scoring (include/insfm_pairs.h): the per-match tests of ImagePairInliersCount
(processors/image_pair_inliers.py:7-133, utils/two_view_geometry.py:24-57) -- numpy in, numpy out, one HIP kernel in
between.

``flatten`` turns the view graph into the library's arrays: a CSR over the matches of the valid pairs (in view-graph
order), global feature numbers like ``track_establishment.flatten_matches``, the concatenated pixel features and rays,
and per pair its kind and 32 float64 constants (matrix, squared threshold, epipoles, relative pose), all computed on
the host in float64.  ``score`` runs them on the device; ``device="cpu"`` or ``None`` asks for ``host_scores``, the
vectorised numpy restatement (the CPU tests' subject and the GPU tests' expected values).  ``device_call`` is one raw
library call that returns whole buffers.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _capi
from .scene.defs import ConfigurationType

SKIP, HOMOGRAPHY, FUNDAMENTAL, ESSENTIAL = 0, 1, 2, 3   # pair_kind (insfm_pairs.h)
GEOM_STRIDE = 32
EPSILON = 1e-10                                           # two_view_geometry.py:4
MAX_MATCHES = 2 ** 31
_HOST_CHUNK = 1 << 19                                     # matches per host_scores block (bounds its temporaries)

_KIND = {ConfigurationType.PLANAR: HOMOGRAPHY, ConfigurationType.PANORAMIC: HOMOGRAPHY,
         ConfigurationType.PLANAR_OR_PANORAMIC: HOMOGRAPHY, ConfigurationType.UNCALIBRATED: FUNDAMENTAL,
         ConfigurationType.CALIBRATED: ESSENTIAL}


@dataclass
class Flat:
    """The arrays of one insfm_pair_inliers call (insfm_pairs.h) and the pairs they describe."""
    pairs: list                  # the valid ImagePair objects, in view-graph order (row p of the per-pair arrays)
    keys: list                   # their view-graph keys
    pair_ptr: np.ndarray         # int64 [P+1]
    match_a: np.ndarray          # int32 [M]
    match_b: np.ndarray          # int32 [M]
    xy: np.ndarray               # [NF, 2] float32 or float64
    rays: Optional[np.ndarray]   # [NF, 3] float32 or float64; None when no pair is ESSENTIAL
    pair_kind: np.ndarray        # int32 [P]
    pair_geom: np.ndarray        # float64 [P, 32]

    @property
    def n_pairs(self):
        return int(self.pair_kind.shape[0])

    @property
    def n_matches(self):
        return int(self.match_a.shape[0])


def pair_constants(kind, thr, M=None, rotation=None, translation=None):
    """One row of pair_geom (insfm_pairs.h): ``M`` is H or F; an ESSENTIAL pair gives ``rotation`` (xyzw) and
    ``translation`` (x2 ~ R x1 + t) instead and E = [t]x R is formed here (E_from_motion, two_view_geometry.py:7-13)."""
    g = np.zeros(GEOM_STRIDE)
    g[9] = float(thr) ** 2
    if kind == ESSENTIAL:
        from scipy.spatial.transform import Rotation
        t = np.asarray(translation, dtype=np.float64).reshape(3)
        R = Rotation.from_quat(np.asarray(rotation, dtype=np.float64)).as_matrix()
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        g[0:9] = (tx @ R).reshape(-1)
        e12, e21 = t, R @ -t                                               # image_pair_inliers.py:74-79
        g[10:13] = -e12 if e12[2] < 0 else e12
        g[13:16] = -e21 if e21[2] < 0 else e21
        g[16:25] = R.reshape(-1)
        g[25:28] = t
        g[28] = np.cos(np.deg2rad(3)) + 1e-6                               # :87-88
        g[29] = 1 + 1e-6
        g[30], g[31] = 1e-2, 100.                                          # check_cheirality's depths (:97)
    elif kind in (HOMOGRAPHY, FUNDAMENTAL):
        M = np.asarray(M, dtype=np.float64).reshape(3, 3)
        g[0:9] = M.reshape(-1)
        if kind == FUNDAMENTAL:                                            # :29-33
            with np.errstate(invalid="ignore"):
                epipole = np.cross(M[0], M[1])
                if not np.any(np.abs(epipole) > 1e-6):
                    epipole = np.cross(M[1], M[2])
            g[10:13] = epipole
    return g


def flatten(view_graph, cameras, images, options):
    """The valid pairs of ``view_graph`` as the arrays of insfm_pair_inliers (a ``Flat``).  ``options`` is
    INLIER_THRESHOLD_OPTIONS.  A match that names a feature outside its image raises IndexError, as the reference's
    ``image.features[pair.matches[:, 0]]`` does."""
    nfeat = np.array([len(im.features) for im in images], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(nfeat)]).astype(np.int64)
    if off[-1] >= MAX_MATCHES:
        raise ValueError("too many features for 32-bit feature numbering")
    pairs, keys, kinds, geoms, a_parts, b_parts, counts = [], [], [], [], [], [], []
    for key, pair in view_graph.image_pairs.items():
        if not pair.is_valid:
            continue
        kind = _KIND.get(pair.config, SKIP)
        i1, i2 = int(pair.image_id1), int(pair.image_id2)
        if kind == SKIP:
            m = np.zeros((0, 2), np.int64)
            g = np.zeros(GEOM_STRIDE)
        else:
            m = np.asarray(pair.matches).reshape(-1, 2).astype(np.int64, copy=False)
            if m.size and (m[:, 0].max() >= nfeat[i1] or m[:, 1].max() >= nfeat[i2] or m.min() < 0):
                raise IndexError(f"match of pair ({i1}, {i2}) refers to a feature outside its image")
            if kind == HOMOGRAPHY:
                g = pair_constants(kind, options['max_epipolar_error_H'], pair.H)
            elif kind == FUNDAMENTAL:
                g = pair_constants(kind, options['max_epipolar_error_F'], pair.F)
            else:
                cam1, cam2 = cameras[images[i1].cam_id], cameras[images[i2].cam_id]
                thr = options['max_epipolar_error_E'] * 0.5 * (1. / cam1.focal() + 1. / cam2.focal())   # :81-85
                g = pair_constants(kind, thr, rotation=pair.rotation, translation=pair.translation)
                for i in (i1, i2):
                    if m.size and len(images[i].features_undist) != nfeat[i]:
                        raise IndexError(f"image {i} has no features_undist (run UndistortImages first)")
        pairs.append(pair)
        keys.append(key)
        kinds.append(kind)
        geoms.append(g)
        a_parts.append(off[i1] + m[:, 0])
        b_parts.append(off[i2] + m[:, 1])
        counts.append(m.shape[0])
    P = len(pairs)
    pair_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    if pair_ptr[-1] >= MAX_MATCHES:
        raise ValueError("too many matches for one call (2^31 or more)")
    ma = (np.concatenate(a_parts) if P else np.zeros(0)).astype(np.int32)
    mb = (np.concatenate(b_parts) if P else np.zeros(0)).astype(np.int32)
    feats = [np.asarray(im.features).reshape(-1, 2) for im in images]
    f32 = all(f.dtype == np.float32 for f in feats if f.size)
    xy = (np.concatenate([f.astype(np.float32 if f32 else np.float64, copy=False) for f in feats]) if feats
          else np.zeros((0, 2)))
    rays = None
    if ESSENTIAL in kinds:
        und = [np.asarray(im.features_undist) for im in images]
        und = [u.reshape(-1, 3) if u.size and u.shape[0] == n else np.full((int(n), 3), np.nan)
               for u, n in zip(und, nfeat)]
        r32 = all(u.dtype == np.float32 for u in und if u.size)
        rays = np.concatenate([u.astype(np.float32 if r32 else np.float64, copy=False) for u in und])
    return Flat(pairs, keys, pair_ptr, ma, mb, np.ascontiguousarray(xy), rays, np.array(kinds, np.int32),
                np.array(geoms, np.float64).reshape(P, GEOM_STRIDE))


# ---------------------------------------------------------------------------------------------------------------------
# host path
# ---------------------------------------------------------------------------------------------------------------------
def _margin(lhs, rhs, mag):
    """|lhs - rhs| over the summed magnitudes of the terms forming both sides; inf where the comparison cannot flip
    under rounding: a NaN side (every comparison with it is false) or all terms exactly zero."""
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.abs(lhs - rhs) / mag
    return np.where(np.isnan(m), np.inf, m)


def _sampson(g, x1, x2):
    """two_view_geometry.py:24-34 on [n, 3] points; g[:, 0:9] is the matrix."""
    E = g[:, 0:9].reshape(-1, 3, 3)
    Ex1 = np.einsum('nij,nj->ni', E, x1) / (x1[:, 2:3] + EPSILON)
    Etx2 = np.einsum('nji,nj->ni', E, x2) / (x2[:, 2:3] + EPSILON)
    C = np.einsum('ni,ni->n', x2, Ex1)
    return C ** 2 / (Ex1[:, 0] ** 2 + Ex1[:, 1] ** 2 + Etx2[:, 0] ** 2 + Etx2[:, 1] ** 2)


def _block(flat, p0, p1):
    """host_scores on the pairs p0 .. p1: (inlier mask [m], per-match score term [m], margin [m], touched [pairs])."""
    lo, hi = int(flat.pair_ptr[p0]), int(flat.pair_ptr[p1])
    n = np.diff(flat.pair_ptr[p0:p1 + 1])
    pid = np.repeat(np.arange(p1 - p0), n)
    kind = flat.pair_kind[p0:p1][pid]
    geom = flat.pair_geom[p0:p1]
    ma, mb = flat.match_a[lo:hi], flat.match_b[lo:hi]
    inl = np.zeros(hi - lo, bool)
    term = np.zeros(hi - lo)
    margin = np.full(hi - lo, np.inf)
    touched = np.isin(flat.pair_kind[p0:p1], (HOMOGRAPHY, ESSENTIAL))
    one = np.ones((1, 1))

    def pix(idx):
        a = flat.xy[idx].astype(np.float64)
        return np.concatenate([a, np.broadcast_to(one, (a.shape[0], 1))], axis=1)

    sel = np.flatnonzero(kind == HOMOGRAPHY)
    if sel.size:                                                           # score_error_homography (:7-26)
        g = geom[pid[sel]]
        x1, x2 = pix(ma[sel]), pix(mb[sel])
        Hx1 = np.einsum('nij,nj->ni', g[:, 0:9].reshape(-1, 3, 3), x1)
        r2 = np.sum((Hx1[:, :2] / (Hx1[:, 2:3] + EPSILON) - x2[:, :2]) ** 2, axis=1)
        ok = r2 < g[:, 9]
        inl[sel] = ok
        term[sel] = np.where(ok, r2, g[:, 9])
        margin[sel] = _margin(r2, g[:, 9], np.abs(r2) + g[:, 9])

    sel = np.flatnonzero(kind == FUNDAMENTAL)
    if sel.size:                                                           # score_error_fundamental (:28-68)
        q = pid[sel]
        g = geom[q]
        x1, x2 = pix(ma[sel]), pix(mb[sel])
        r2 = _sampson(g, x1, x2)
        pre = r2 < g[:, 9]
        mg = _margin(r2, g[:, 9], np.abs(r2) + g[:, 9])
        t1 = np.stack([g[:, 0] * x2[:, 0], g[:, 3] * x2[:, 1], g[:, 6]], 1)      # get_orientation_signum (:49-52)
        t2 = np.stack([g[:, 11], -g[:, 12] * x1[:, 1]], 1)
        s1, s2 = t1[:, 0] + t1[:, 1] + t1[:, 2], t2[:, 0] + t2[:, 1]
        sig = s1 * s2
        # (the product's sign flips iff a factor's does; a factor whose terms are all exactly zero is exact)
        mag1, mag2 = np.abs(t1).sum(1), np.abs(t2).sum(1)
        msig = np.minimum(np.where(mag1 > 0, _margin(s1, 0.0, np.where(mag1 > 0, mag1, 1.0)), np.inf),
                          np.where(mag2 > 0, _margin(s2, 0.0, np.where(mag2 > 0, mag2, 1.0)), np.inf))
        margin[sel] = np.where(pre, np.minimum(mg, msig), mg)
        pos = pre & (sig > 0)
        n_pos = np.bincount(q[pos], minlength=p1 - p0)
        n_neg = np.bincount(q[pre], minlength=p1 - p0) - n_pos
        voted = n_pos != n_neg
        touched |= voted & (flat.pair_kind[p0:p1] == FUNDAMENTAL)
        ok = pre & voted[q] & ((sig > 0) == (n_pos > n_neg)[q])
        inl[sel] = ok
        term[sel] = np.where(ok, r2, np.where(pre & voted[q], g[:, 9], 0.0))

    sel = np.flatnonzero(kind == ESSENTIAL)
    if sel.size:                                                           # score_error_essential (:70-116)
        g = geom[pid[sel]]
        x1, x2 = flat.rays[ma[sel]].astype(np.float64), flat.rays[mb[sel]].astype(np.float64)
        r2 = _sampson(g, x1, x2)
        thr2 = g[:, 9]
        stage = r2 < thr2
        mg = _margin(r2, thr2, np.abs(r2) + thr2)
        R, t = g[:, 16:25].reshape(-1, 3, 3), g[:, 25:28]
        Rx1 = np.einsum('nij,nj->ni', R, x1)                               # check_cheirality (:36-47)
        ta, tb1, tb2 = -Rx1 * x2, -Rx1 * t, t * x2
        a, b1, b2 = ta.sum(1), tb1.sum(1), tb2.sum(1)
        l1, l2 = b1 - a * b2, -a * b1 + b2
        dmin, dmax = g[:, 30] * (1 - a ** 2), g[:, 31] * (1 - a ** 2)
        with np.errstate(invalid="ignore"):
            cheir = (l1 > dmin) & (l2 > dmin) & (l1 < dmax) & (l2 < dmax)
        A, B1, B2 = np.abs(ta).sum(1), np.abs(tb1).sum(1), np.abs(tb2).sum(1)
        m1, m2 = B1 + A * B2, A * B1 + B2
        mc = np.minimum.reduce([_margin(l1, dmin, m1 + np.abs(dmin)), _margin(l2, dmin, m2 + np.abs(dmin)),
                                _margin(l1, dmax, m1 + np.abs(dmax)), _margin(l2, dmax, m2 + np.abs(dmax))])
        mg = np.where(stage, np.minimum(mg, mc), mg)
        stage = stage & cheir
        Rtx2 = np.einsum('nji,nj->ni', R, x2)                              # inv(R) x2 (:101)
        tang = x1 * Rtx2
        ang = tang.sum(1)
        mg = np.where(stage, np.minimum(mg, _margin(ang, g[:, 29], np.abs(tang).sum(1) + g[:, 29])), mg)
        with np.errstate(invalid="ignore"):
            stage = stage & ~(ang > g[:, 29])
            te1, te2 = x1 * g[:, 13:16], x2 * g[:, 10:13]                  # :106-108
            d1, d2 = te1.sum(1), te2.sum(1)
            me = np.minimum(_margin(d1, g[:, 28], np.abs(te1).sum(1) + g[:, 28]),
                            _margin(d2, g[:, 28], np.abs(te2).sum(1) + g[:, 28]))
            mg = np.where(stage, np.minimum(mg, me), mg)
            ok = stage & ~((d1 > g[:, 28]) | (d2 > g[:, 28]))
        inl[sel] = ok
        term[sel] = np.where(ok, r2, thr2)
        margin[sel] = mg
    return inl, term, margin, touched, pid


def host_scores(flat):
    """The numpy host path: (inlier_idx [total inliers] -- every pair's ascending local match indices, concatenated in
    pair order --, inlier_count [P], score [P], touched [P], margin [M]).

    ``margin`` is, per match, the smallest margin of the comparisons evaluated for it: |lhs - rhs| over the summed
    magnitudes of the terms forming both sides (``_margin``).  Every comparison of a stage the match reached counts
    (all four of check_cheirality, both epipole tests); an F pair's orientation vote counts for its pre-inliers.  It
    tells how far the inputs are from a rounding-dependent outcome; it is not part of the result."""
    P, M = flat.n_pairs, flat.n_matches
    count = np.zeros(P, np.int32)
    score = np.zeros(P)
    touched = np.zeros(P, np.int32)
    margin = np.full(M, np.inf)
    idx_parts = []
    p0 = 0
    while p0 < P:
        p1 = int(np.searchsorted(flat.pair_ptr, flat.pair_ptr[p0] + _HOST_CHUNK, side="right")) - 1
        p1 = min(max(p1, p0 + 1), P)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            inl, term, mg, tch, pid = _block(flat, p0, p1)
        lo = int(flat.pair_ptr[p0])
        margin[lo:lo + mg.size] = mg
        count[p0:p1] = np.bincount(pid[inl], minlength=p1 - p0)
        score[p0:p1] = np.bincount(pid, weights=term, minlength=p1 - p0)
        touched[p0:p1] = tch
        local = np.arange(lo, lo + mg.size) - flat.pair_ptr[p0:p1][pid]
        idx_parts.append(local[inl])
        p0 = p1
    idx = np.concatenate(idx_parts).astype(np.int32) if idx_parts else np.zeros(0, np.int32)
    return idx, count, score, touched, margin


# ---------------------------------------------------------------------------------------------------------------------
# device path
# ---------------------------------------------------------------------------------------------------------------------
def device_call(flat, device="cuda:0", fill=-1):
    """One insfm_pair_inliers call: (return code, inlier_idx [M], inlier_count [P], score [P], touched [P]).  The
    output buffers come back whole, pre-filled with ``fill``."""
    import torch

    from .engine import _require_gpu
    from .passes import _dev, _p, _stream
    dev = _require_gpu(device)
    lib = _capi.load()
    P, M = flat.n_pairs, flat.n_matches
    xy = np.asarray(flat.xy)
    xy_f32 = xy.dtype == np.float32
    xy = xy.astype(np.float32 if xy_f32 else np.float64, copy=False).reshape(-1, 2)
    nf = xy.shape[0]
    rays, rays_f32 = flat.rays, False
    if rays is not None:
        rays = np.asarray(rays)
        rays_f32 = rays.dtype == np.float32
        rays = rays.astype(np.float32 if rays_f32 else np.float64, copy=False).reshape(-1, 3)

    def up(a, dt, width=1):
        a = np.ascontiguousarray(a, dtype=dt)
        return _dev(a if a.size else np.zeros((1, width) if width > 1 else 1, dt), dev)

    d_ptr, d_a, d_b = up(flat.pair_ptr, np.int64), up(flat.match_a, np.int32), up(flat.match_b, np.int32)
    d_xy = up(xy, xy.dtype, 2)
    d_rays = up(rays, rays.dtype, 3) if rays is not None else None
    d_kind, d_geom = up(flat.pair_kind, np.int32), up(flat.pair_geom, np.float64, GEOM_STRIDE)
    idx = torch.full((max(M, 1),), fill, dtype=torch.int32, device=dev)
    count = torch.full((max(P, 1),), fill, dtype=torch.int32, device=dev)
    score = torch.full((max(P, 1),), float(fill), dtype=torch.float64, device=dev)
    touched = torch.full((max(P, 1),), fill, dtype=torch.int32, device=dev)
    rc = lib.insfm_pair_inliers(P, _p(d_ptr), M, _p(d_a), _p(d_b), nf, _p(d_xy), int(xy_f32), _p(d_rays),
                                int(rays_f32), _p(d_kind), _p(d_geom), _p(idx), _p(count), _p(score), _p(touched),
                                _stream(dev))
    return (rc, idx.cpu().numpy()[:M], count.cpu().numpy()[:P], score.cpu().numpy()[:P], touched.cpu().numpy()[:P])


def score(flat, device="cuda:0"):
    """(inlier_idx, inlier_count, score, touched) of ``flat`` like ``host_scores`` (without the margins): the device
    path, or the host path for ``device`` ``"cpu"`` / ``None``."""
    if device is None or str(device) == "cpu":
        return host_scores(flat)[:4]
    rc, idx, count, sc, touched = device_call(flat, device)
    if rc != 0:
        raise _capi.BAError(rc, "insfm_pair_inliers")
    keep = np.arange(flat.n_matches) - np.repeat(flat.pair_ptr[:-1], np.diff(flat.pair_ptr)) \
        < np.repeat(count, np.diff(flat.pair_ptr))
    return idx[keep], count, sc, touched
