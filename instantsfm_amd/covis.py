"""Co-visibility pair counts (include/insfm_covis.h): the visibility graph of PruneWeaklyConnectedImages
(reconstruction_pruning.py:173-191) from the tracks' CSR arrays -- numpy in, numpy out, HIP kernels in between.

``covis_pairs`` returns the image pairs seen at least ``min_count`` times in the insertion order of the reference's
``image_observation_count`` dict (order of first occurrence in its track / i / j loops), which is what every later
step of the stage iterates in.  ``device="cpu"`` or ``None`` asks for the numpy host path explicitly (the CPU tests
and the GPU tests' expected values); a scene with 2^31 or more pair ordinals, which the library refuses, takes it too.
"""
import ctypes

import numpy as np

from . import _capi

MAX_ORDINALS = 2 ** 31  # hipcub item counts are int (insfm_covis.h)


def _csr(track_ptr, obs_img):
    ptr = np.ascontiguousarray(track_ptr, dtype=np.int64).reshape(-1)
    img = np.ascontiguousarray(obs_img, dtype=np.int32).reshape(-1)
    if ptr.size == 0:
        ptr = np.zeros(1, np.int64)
    if ptr[0] < 0 or ptr[-1] > img.size or (np.diff(ptr) < 0).any():
        raise ValueError("track_ptr must be non-decreasing and within obs_img")
    return ptr, img


def pair_ordinals(track_ptr):
    """(first ordinal of each track [T], ordinals in all): L(L-1)/2 per track of L > 2 rows, in track order."""
    L = np.diff(np.asarray(track_ptr, dtype=np.int64))
    n = np.where(L > 2, L * (L - 1) // 2, 0)
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    return off[:-1], int(off[-1])


def host_pairs(track_ptr, obs_img, min_count=5):
    """The host path: (lo, hi, count, first ordinal) sorted by first ordinal, and the ordinal total.  Tracks are taken
    one length at a time; inside a length the (i < j) pairs come from ``np.triu_indices`` (i-major, like the loops)."""
    ptr, img = _csr(track_ptr, obs_img)
    off, total = pair_ordinals(ptr)
    L = np.diff(ptr)
    keys = np.empty(total, np.int64)
    for length in np.unique(L[L > 2]).tolist():
        t = np.flatnonzero(L == length)
        rows = img[ptr[t][:, None] + np.arange(length)].astype(np.int64)  # [tracks, length]
        i, j = np.triu_indices(length, 1)
        a, b = rows[:, i], rows[:, j]
        k = (np.minimum(a, b) << 32) | (np.maximum(a, b) & 0xffffffff)
        k[a == b] = -1
        keys[off[t][:, None] + np.arange(i.size)] = k
    ordinal = np.flatnonzero(keys != -1)
    uniq, idx, cnt = np.unique(keys[ordinal], return_index=True, return_counts=True)
    first = ordinal[idx]
    sel = cnt >= min_count
    uniq, first, cnt = uniq[sel], first[sel], cnt[sel]
    order = np.argsort(first, kind="stable")
    uniq, first, cnt = uniq[order], first[order], cnt[order]
    lo = (uniq >> 32).astype(np.int32)
    hi = (uniq & 0xffffffff).astype(np.uint32).view(np.int32)
    return lo, hi, cnt.astype(np.int32), first.astype(np.int64), total


def device_call(track_ptr, obs_img, min_count, capacity, device="cuda:0", fill=-1):
    """One insfm_covis_pairs call: (return code, pair_lo, pair_hi, pair_count, pair_first, counts).  The four output
    buffers come back whole (``capacity`` entries, pre-filled with ``fill``), in the library's order."""
    import torch

    from .engine import _require_gpu
    from .passes import _dev, _p, _stream
    dev = _require_gpu(device)
    lib = _capi.load()
    ptr, img = _csr(track_ptr, obs_img)
    nt = ptr.size - 1
    cap = int(capacity)
    d_ptr = _dev(ptr, dev)
    d_img = _dev(img if img.size else np.zeros(1, np.int32), dev)
    out = [torch.full((max(cap, 1),), fill, dtype=dt, device=dev)
           for dt in (torch.int32, torch.int32, torch.int32, torch.int64)]
    counts = (ctypes.c_int64 * 2)(0, 0)
    rc = lib.insfm_covis_pairs(nt, _p(d_ptr), _p(d_img), int(min_count), cap, *[_p(t) for t in out], counts,
                               _stream(dev))
    return (rc, *[t.cpu().numpy()[:cap] for t in out], (int(counts[0]), int(counts[1])))


def covis_pairs(track_ptr, obs_img, min_count=5, device="cuda:0"):
    """(lo, hi, count) of every image pair (lo < hi) that shares at least ``min_count`` track-row pairs, sorted by the
    pair's first occurrence."""
    if device is None or str(device) == "cpu":
        return host_pairs(track_ptr, obs_img, min_count)[:3]
    ptr, img = _csr(track_ptr, obs_img)
    total = pair_ordinals(ptr)[1]
    m = int(img.max()) + 1 if img.size and img.min() >= 0 else 0
    capacity = min(total, m * (m - 1) // 2) if m else total
    rc, lo, hi, cnt, first, counts = device_call(ptr, img, min_count, capacity, device)
    if rc == _capi.INSFM_BA_EINVAL and counts[1] >= MAX_ORDINALS:
        return host_pairs(ptr, img, min_count)[:3]
    if rc != 0:
        raise _capi.BAError(rc, "insfm_covis_pairs")
    n = counts[0]
    order = np.argsort(first[:n], kind="stable")
    return lo[:n][order], hi[:n][order], cnt[:n][order]
