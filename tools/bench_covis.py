#!/usr/bin/env python3
"""Time the co-visibility pair counts of pruning ("Pruning") on the bench scene's tracks.

Three ways to get the pair list of PruneWeaklyConnectedImages (reconstruction_pruning.py:173-191):
  * ``insfm_covis_pairs`` (csrc/covis.hip) on device-resident inputs, timed with device events around the call, and
    the whole wrapper (``covis.covis_pairs``: upload, call, download, sort by first occurrence) on a host clock;
  * the numpy host path (``covis.host_pairs``);
  * the reference-style Python double loop over every track -- only at ``--loop-config`` (config 3 takes minutes).
Each figure is the best of ``--repeats`` after one warm-up.  The workspace figure is the high-water mark of the
device's default memory pool (where the call's stream-ordered scratch comes from) over one call.  Needs an MI355X.
Usage:  python tools/bench_covis.py [--config 3] [--loop-config 2] [--repeats 5] [--json out.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from instantsfm_amd import _capi, covis  # noqa: E402
from instantsfm_amd.scene.defs import Ids2PairId  # noqa: E402
from instantsfm_amd.synth import make_config  # noqa: E402

USED_MEM_HIGH = 0x8  # hipMemPoolAttrUsedMemHigh


def scene_tracks(cfg):
    prob = make_config(cfg)
    length = len(prob.cam_idx) // prob.points_gt.shape[0]
    return np.arange(prob.points_gt.shape[0] + 1, dtype=np.int64) * length, prob.cam_idx.astype(np.int32)


def double_loop(track_ptr, obs_img, min_count=5):
    """The reference's loops over plain Python ints (its numpy scalars are slower still)."""
    count = {}
    img = obs_img.tolist()
    for t in range(len(track_ptr) - 1):
        row = img[track_ptr[t]:track_ptr[t + 1]]
        if len(row) <= 2:
            continue
        for i in range(len(row)):
            for j in range(i + 1, len(row)):
                if row[i] == row[j]:
                    continue
                pair_id = Ids2PairId(row[i], row[j])
                if pair_id not in count:
                    count[pair_id] = 1
                else:
                    count[pair_id] += 1
    return {k: c for k, c in count.items() if c >= min_count}


def best_of(fn, repeats):
    fn()
    best = float("inf")
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t)
    return best * 1e3


def pool_high_water(dev_index, fn):
    """Bytes the default memory pool had in use at most while fn ran (None when the runtime does not report it)."""
    hip = ctypes.CDLL("libamdhip64.so")
    pool = ctypes.c_void_p()
    if hip.hipDeviceGetDefaultMemPool(ctypes.byref(pool), dev_index) != 0:
        return None
    zero = ctypes.c_uint64(0)
    if hip.hipMemPoolSetAttribute(pool, USED_MEM_HIGH, ctypes.byref(zero)) != 0:
        return None
    fn()
    high = ctypes.c_uint64(0)
    if hip.hipMemPoolGetAttribute(pool, USED_MEM_HIGH, ctypes.byref(high)) != 0:
        return None
    return int(high.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--loop-config", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    from instantsfm_amd.engine import _require_gpu
    from instantsfm_amd.passes import _dev, _p, _stream
    dev = _require_gpu("cuda:0")
    lib = _capi.load()

    ptr, img = scene_tracks(args.config)
    lo, hi, cnt, first, total = covis.host_pairs(ptr, img)
    m = int(img.max()) + 1
    cap = min(total, m * (m - 1) // 2)
    d_ptr, d_img = _dev(ptr, dev), _dev(img, dev)
    out = [torch.empty(cap, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.int32, torch.int64)]
    counts = (ctypes.c_int64 * 2)(0, 0)

    def call():
        rc = lib.insfm_covis_pairs(len(ptr) - 1, _p(d_ptr), _p(d_img), 5, cap, *[_p(t) for t in out], counts,
                                   _stream(dev))
        assert rc == 0, rc

    call()
    assert (counts[0], counts[1]) == (len(lo), total)
    glo, ghi, gcnt = covis.covis_pairs(ptr, img)
    assert np.array_equal(glo, lo) and np.array_equal(ghi, hi) and np.array_equal(gcnt, cnt)
    call_ms = float("inf")
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        call_ms = min(call_ms, e0.elapsed_time(e1))
    res = dict(config=args.config, tracks=len(ptr) - 1, rows=int(ptr[-1]), images=m, ordinals=total, pairs=len(lo),
               call_ms=call_ms, wrapper_ms=best_of(lambda: covis.covis_pairs(ptr, img), args.repeats),
               numpy_ms=best_of(lambda: covis.host_pairs(ptr, img), args.repeats),
               workspace_bytes=pool_high_water(dev.index or 0, call))

    lptr, limg = scene_tracks(args.loop_config)
    ref = double_loop(lptr.tolist(), limg)
    llo, lhi, lcnt = covis.covis_pairs(lptr, limg)
    assert list(ref.items()) == [(Ids2PairId(a, b), c) for a, b, c in zip(llo.tolist(), lhi.tolist(), lcnt.tolist())]
    res.update(loop_config=args.loop_config, loop_ordinals=covis.pair_ordinals(lptr)[1],
               loop_ms=best_of(lambda: double_loop(lptr.tolist(), limg), args.repeats),
               loop_config_wrapper_ms=best_of(lambda: covis.covis_pairs(lptr, limg), args.repeats),
               loop_config_numpy_ms=best_of(lambda: covis.host_pairs(lptr, limg), args.repeats))
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
