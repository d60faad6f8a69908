#!/usr/bin/env python3
"""Time the image-pair inlier scoring ("Pair inliers") on a config-5-sized view graph.

The view graph is ``synth.make_match_graph``'s (500 images, ~8M matches by default); every pair gets a random relative
pose and, from it and one shared pinhole camera, its E, F and a plane-induced H; ``--kinds`` sets the shares of
CALIBRATED / UNCALIBRATED / PLANAR pairs.  The keypoints are random, so at the mapper's thresholds almost no match is
an inlier; ``--thr-scale`` multiplies the three thresholds (about 300 lets half of the matches pass r2 < thr^2, so the
cheirality / epipole checks and the index compaction run for them).
  * ``insfm_pair_inliers`` (csrc/pair_inliers.hip) on device-resident inputs, timed with device events around the call;
  * the whole wrapper (``pair_inliers.score``: upload, call, download) on a host clock;
  * the numpy host path (``pair_inliers.host_scores``), once.
The device figures are the best of ``--repeats`` after one warm-up, plus the mean over ``--window`` back-to-back calls
in one event window (the inputs stay resident and warm in both).  Needs an MI355X.
Usage:  python tools/bench_inliers.py [--images 500] [--points 600000] [--thr-scale 1] [--repeats 5] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from instantsfm_amd import _capi  # noqa: E402
from instantsfm_amd import pair_inliers as PI  # noqa: E402
from instantsfm_amd.config.colmap import INLIER_THRESHOLD_OPTIONS  # noqa: E402
from instantsfm_amd.scene.defs import Camera, CameraModelId, ConfigurationType  # noqa: E402
from instantsfm_amd.synth import _quat_from_rotvec, make_match_graph, quat_to_matrix  # noqa: E402

FOCAL, PP = 1000.0, (1000.0, 750.0)


def synthetic_geometry(view_graph, images, shares, seed=0):
    """Random relative poses (rotation N(0, 0.1^2) rad per axis, unit translation) and the E / F / H they give with
    the shared camera; unit rays of the keypoints as ``features_undist``."""
    rng = np.random.default_rng(seed)
    K = np.array([[FOCAL, 0, PP[0]], [0, FOCAL, PP[1]], [0, 0, 1.0]])
    Kinv = np.linalg.inv(K)
    configs = [ConfigurationType.CALIBRATED, ConfigurationType.UNCALIBRATED, ConfigurationType.PLANAR]
    n = len(view_graph.image_pairs)
    q = _quat_from_rotvec(rng.normal(0, 0.1, (n, 3)))
    R = quat_to_matrix(q)
    t = rng.normal(size=(n, 3))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    which = rng.choice(3, n, p=np.asarray(shares) / np.sum(shares))
    normal = np.array([0.0, 0.0, 1.0])
    for k, pair in enumerate(view_graph.image_pairs.values()):
        tx = np.array([[0, -t[k, 2], t[k, 1]], [t[k, 2], 0, -t[k, 0]], [-t[k, 1], t[k, 0], 0]])
        pair.rotation, pair.translation = q[k], t[k]
        pair.E = tx @ R[k]
        pair.F = Kinv.T @ pair.E @ Kinv
        pair.H = K @ (R[k] + np.outer(t[k], normal) / 8.0) @ Kinv
        pair.config = configs[which[k]]
    for im in images:
        r = np.concatenate([(im.features.astype(np.float64) - PP) / FOCAL, np.ones((len(im.features), 1))], axis=1)
        im.features_undist = r / np.linalg.norm(r, axis=1, keepdims=True)
    return [Camera(id=0, model_id=CameraModelId.SIMPLE_PINHOLE, width=2000, height=1500,
                   params=np.array([FOCAL, PP[0], PP[1]]))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=500)
    ap.add_argument("--points", type=int, default=600_000)
    ap.add_argument("--kinds", type=float, nargs=3, default=(0.8, 0.1, 0.1), metavar=("E", "F", "H"))
    ap.add_argument("--thr-scale", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=int, default=200, help="calls in the one-window mean (call_mean_ms)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    from instantsfm_amd.engine import _require_gpu
    from instantsfm_amd.passes import _dev, _p, _stream
    dev = _require_gpu("cuda:0")
    lib = _capi.load()

    vg, images = make_match_graph(n_images=args.images, n_points=args.points)
    cameras = synthetic_geometry(vg, images, args.kinds)
    options = dict(INLIER_THRESHOLD_OPTIONS)
    for key in ("max_epipolar_error_E", "max_epipolar_error_F", "max_epipolar_error_H"):
        options[key] *= args.thr_scale
    t0 = time.perf_counter()
    flat = PI.flatten(vg, cameras, images, options)
    flatten_ms = (time.perf_counter() - t0) * 1e3
    P, M = flat.n_pairs, flat.n_matches

    t0 = time.perf_counter()
    idx, count, score, touched, _ = PI.host_scores(flat)
    numpy_ms = (time.perf_counter() - t0) * 1e3

    d = [_dev(flat.pair_ptr, dev), _dev(flat.match_a, dev), _dev(flat.match_b, dev), _dev(flat.xy, dev),
         _dev(flat.rays, dev), _dev(flat.pair_kind, dev), _dev(flat.pair_geom, dev)]
    out = [torch.empty(M, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.int32, device=dev),
           torch.empty(P, dtype=torch.float64, device=dev), torch.empty(P, dtype=torch.int32, device=dev)]

    def call():
        rc = lib.insfm_pair_inliers(P, _p(d[0]), M, _p(d[1]), _p(d[2]), flat.xy.shape[0], _p(d[3]),
                                    int(flat.xy.dtype == np.float32), _p(d[4]), int(flat.rays.dtype == np.float32),
                                    _p(d[5]), _p(d[6]), *[_p(t) for t in out], _stream(dev))
        assert rc == 0, rc

    call()
    g_idx, g_count, g_score, g_touched = PI.score(flat)
    assert np.array_equal(g_idx, idx) and np.array_equal(g_count, count) and np.array_equal(g_touched, touched)
    assert (np.abs(g_score - score) <= 1e-10 * np.diff(flat.pair_ptr) * flat.pair_geom[:, 9]).all()
    call_ms = float("inf")
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        call_ms = min(call_ms, e0.elapsed_time(e1))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.window):
        call()
    e1.record()
    e1.synchronize()
    call_mean_ms = e0.elapsed_time(e1) / args.window
    wrapper_ms = float("inf")
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        PI.score(flat)
        wrapper_ms = min(wrapper_ms, (time.perf_counter() - t0) * 1e3)
    kinds = np.bincount(flat.pair_kind, minlength=4).tolist()
    res = dict(images=args.images, pairs=P, matches=M, features=int(flat.xy.shape[0]), kinds_skip_h_f_e=kinds,
               thr_scale=args.thr_scale, inliers=int(count.sum()), flatten_ms=flatten_ms, call_ms=call_ms,
               call_mean_ms=call_mean_ms, wrapper_ms=wrapper_ms, numpy_ms=numpy_ms,
               call_matches_per_s=M / (call_mean_ms * 1e-3), numpy_matches_per_s=M / (numpy_ms * 1e-3))
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
