#!/usr/bin/env python3
"""Time rotation averaging ("Rotation averaging") on the view graph of a synthetic mapper scene.

The view graph is ``synth.write_mapper_database``'s (a ring of images, each paired with its neighbours up to ``reach``
apart, read back through ReadColmapDatabase); every pair's rotation is the ground-truth relative rotation times a
N(0, sigma^2) rotation vector, ``--outliers`` of the pairs carry a random rotation instead, and the inliers are all of
the pair's matches.  Per size it reports, as wall time around calls that wait for their work (best of ``--repeats``
after one warm-up):
  * ``system_ms``   insfm_rotavg_system without the inverse: validation, the per-image CSR and M = B^T W B;
  * ``inverse_ms``  the same call with the inverse, minus ``system_ms``: the Gauss-Jordan chain (and a second build);
  * ``l1_ms``       insfm_rotavg_solve with the IRLS phase off, and ``admm_iter_us`` = (l1_ms - system_ms - inverse_ms)
                    over the ADMM iterations run: five launches and one 48-byte copy each;
  * ``irls_ms``     insfm_rotavg_solve with the L1 phase off, from the L1 result, and ``irls_iter_ms`` per iteration:
                    weights, build, inverse, one product, update, residuals, one copy;
  * ``solve_ms``    the whole solve, ``estimate_ms`` RotationEstimator.EstimateRotations around it (spanning tree,
                    flattening, upload, solve, write-back), and the iteration counts.
Needs an MI355X.
Usage:  python tools/bench_rotavg.py [--images 100 300 1000] [--reach 3] [--sigma-deg 0.5] [--outliers 0.1] [--json f]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from instantsfm_amd import rotavg as RA  # noqa: E402
from instantsfm_amd.config.colmap import L1_SOLVER_OPTIONS, ROTATION_ESTIMATOR_OPTIONS  # noqa: E402
from instantsfm_amd.controllers.data_reader import ReadColmapDatabase  # noqa: E402
from instantsfm_amd.processors.rotation_averaging import RotationEstimator  # noqa: E402
from instantsfm_amd.synth import _quat_from_matrix, _quat_from_rotvec, quat_to_matrix, write_mapper_database  # noqa: E402


def make_scene(n_images, reach, sigma_deg, outliers, seed=0):
    """(view_graph, images) with noisy relative rotations; the images carry no rotations."""
    rng = np.random.default_rng([seed, 13])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "db.db")
        scene = write_mapper_database(path, n_images=n_images, n_points=40 * n_images, track_len=6, window=2 * reach,
                                      reach=reach, seed=seed, images_per_camera=50, distractors=10)
        with contextlib.redirect_stdout(io.StringIO()):
            vg, _, images, _ = ReadColmapDatabase(path)
    for pair in vg.image_pairs.values():
        rel = scene.rot_gt[pair.image_id2] @ scene.rot_gt[pair.image_id1].T
        if rng.uniform() < outliers and abs(pair.image_id1 - pair.image_id2) != 1:
            rel = quat_to_matrix(_quat_from_rotvec(rng.normal(0, 1.5, 3)))
        else:
            rel = quat_to_matrix(_quat_from_rotvec(rng.normal(0, np.deg2rad(sigma_deg), 3))) @ rel
        pair.rotation = _quat_from_matrix(rel)
        pair.inliers = np.arange(len(pair.matches))
    for im in images:
        im.is_registered = True
        im.world2cam = np.eye(4)
    return vg, images


def best_ms(fn, repeats):
    fn()
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def bench(n_images, args):
    import torch
    from instantsfm_amd import _capi
    from instantsfm_amd.engine import _require_gpu
    from instantsfm_amd.passes import _dev, _p, _stream
    dev = _require_gpu("cuda:0")
    lib = _capi.load()
    vg, images = make_scene(n_images, args.reach, args.sigma_deg, args.outliers)
    est = RotationEstimator()
    t0 = time.perf_counter()
    est.InitializeFromMaximumSpanningTree(vg, images)
    est.SetupLinearSystem(vg, images)
    host_ms = (time.perf_counter() - t0) * 1e3
    f = est.flat
    n, P = f.n, f.n_pairs
    rot0 = est.rotation_estimated[:3 * n].reshape(n, 3).copy()
    fixed = f.id2idx[est.fixed_camera_id]
    d_pi, d_pj, d_q = _dev(f.pair_i, dev), _dev(f.pair_j, dev), _dev(f.quat, dev)
    d_fix = _dev(np.array(est.fixed_camera_rotation), dev)
    d_rot0 = _dev(rot0, dev)
    M = torch.empty((n, n), dtype=torch.float64, device=dev)
    inv = torch.empty((n, n), dtype=torch.float64, device=dev)
    stream = _stream(dev)
    import ctypes
    info = (ctypes.c_int32 * RA.INFO_LEN)()

    def system(with_inverse):
        rc = lib.insfm_rotavg_system(n, P, _p(d_pi), _p(d_pj), None, fixed, _p(M), _p(inv) if with_inverse else None,
                                     stream)
        assert rc == 0, rc

    def solve(start, l1, irls):
        ro = dict(ROTATION_ESTIMATOR_OPTIONS)
        if not l1:
            ro['max_num_l1_iterations'] = 0
        if not irls:
            ro['max_num_irls_iterations'] = 0
        opt = RA.make_options(ro, L1_SOLVER_OPTIONS)
        rot = start.clone()

        def call():
            rot.copy_(start)
            rc = lib.insfm_rotavg_solve(n, P, _p(d_pi), _p(d_pj), _p(d_q), _p(rot), fixed, _p(d_fix),
                                        ctypes.byref(opt), info, stream)
            assert rc == 0 and info[RA.INFO_FAILED] == 0, (rc, list(info))
        return call, rot

    system_ms = best_ms(lambda: system(False), args.repeats)
    inverse_ms = best_ms(lambda: system(True), args.repeats) - system_ms
    call, rot_l1 = solve(d_rot0, True, False)
    l1_ms = best_ms(call, args.repeats)
    l1_iters, admm = int(info[RA.INFO_L1_ITERS]), [int(v) for v in info[RA.INFO_ADMM:RA.INFO_ADMM + 10] if v]
    call, _ = solve(rot_l1.clone(), False, True)
    irls_ms = best_ms(call, args.repeats)
    irls_iters = int(info[RA.INFO_IRLS_ITERS])
    call, _ = solve(d_rot0, True, True)
    solve_ms = best_ms(call, args.repeats)
    counts = (int(info[RA.INFO_L1_ITERS]), int(info[RA.INFO_IRLS_ITERS]))

    def estimate():
        vg2, images2 = make_scene(n_images, args.reach, args.sigma_deg, args.outliers)
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            assert RotationEstimator().EstimateRotations(vg2, images2, ROTATION_ESTIMATOR_OPTIONS, L1_SOLVER_OPTIONS)
        return (time.perf_counter() - t0) * 1e3
    estimate()
    estimate_ms = min(estimate() for _ in range(2))
    return dict(images=n, pairs=P, host_init_ms=host_ms, system_ms=system_ms, inverse_ms=inverse_ms, l1_ms=l1_ms,
                l1_iterations=l1_iters, admm_iterations=admm,
                admm_iter_us=1e3 * (l1_ms - system_ms - inverse_ms) / max(1, sum(admm)),
                irls_ms=irls_ms, irls_iterations=irls_iters, irls_iter_ms=irls_ms / max(1, irls_iters),
                solve_ms=solve_ms, solve_l1_irls_iterations=counts, estimate_ms=estimate_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=(100, 300, 1000))
    ap.add_argument("--reach", type=int, default=3)
    ap.add_argument("--sigma-deg", type=float, default=0.5)
    ap.add_argument("--outliers", type=float, default=0.1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    lines = []
    for n_images in args.images:
        lines.append(json.dumps(bench(n_images, args)))
        print(lines[-1], flush=True)
    if args.json:
        with open(args.json, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
