"""CPU test of the host planning of insfm_ba_create (instantsfm_amd/csrc/create_plan.h): every index array the
kernels assume, computed by tests/cpp/create_plan_test.cpp from synthetic scenes and checked here against their
defining properties, a brute-force count over the tracks and the oracle's clusters.  Each scene runs with a host pool
of 1 and of 5 threads; the two plans must be identical."""
import functools
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import ragged_scene as RS
from instantsfm_amd.shard import shard_ranges
from instantsfm_amd.synth import make_problem
from oracle import oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_NI = {0: 1, 1: 2, 2: 2, 3: 3, 4: 6, 5: 6, 6: 10, 8: 2, 9: 3}
# the device-side constants create passes to the plan (ba_schur.h, ba_lin.h, ba_twolevel.h, ba_cgp.h); the properties below
# hold for any values
LDS_BUDGET, LDS_TARGET, LDS_TARGET_DET = 96 * 1024, 96 * 1024, 52 * 1024
SCHUR_WAVES, DET_WAVES, SCHUR_CHUNK = 8, 4, 4
LIN_THREADS, COARSE_MAX, SEG_MAX, PAD_SLOT, X_CHUNKS = 128, 768, 40, -2 ** 31, 4


def _scene(prob, cam_idx=None, pt_idx=None, K=0, p0=0, p1=None, det=False, oracle=False, tight_lds=False):
    return dict(prob=prob, cam_idx=np.ascontiguousarray(prob.cam_idx if cam_idx is None else cam_idx, dtype=np.int32),
                pt_idx=np.ascontiguousarray(prob.pt_idx if pt_idx is None else pt_idx, dtype=np.int32),
                K=K, p0=p0, p1=prob.n_points if p1 is None else p1, det=det, oracle=oracle, tight_lds=tight_lds)


@functools.lru_cache(maxsize=None)
def _scenes():
    """name -> scene; built on first use, so that collecting the module stays cheap"""
    out = {}
    small = make_problem(24, 900, seed=9)
    out["one_cluster"] = _scene(small)
    prob = make_problem(40, 1500, seed=9)
    dup = np.flatnonzero(np.random.default_rng(9).random(prob.n_obs) < 0.05)  # same camera, same track, twice
    idx = np.sort(np.concatenate([np.arange(prob.n_obs), dup]), kind="stable")
    out["duplicates"] = _scene(prob, prob.cam_idx[idx], prob.pt_idx[idx], tight_lds=True)
    prob = make_problem(30, 800, seed=4)
    keep = prob.cam_idx != 7  # camera 7 sees nothing
    out["empty_camera"] = _scene(prob, prob.cam_idx[keep], prob.pt_idx[keep])
    prob = make_problem(150, 6000, seed=8)
    perm = np.random.default_rng(3).permutation(prob.n_cams).astype(np.int32)
    for K in (4, 16, 32):
        out[f"clusters_K{K}"] = _scene(prob, K=K, oracle=True)
        out[f"clusters_K{K}_perm"] = _scene(prob, perm[prob.cam_idx], K=K, oracle=True)
    prob6 = make_problem(150, 6000, seed=8, model=6)
    for K in (2, 3):  # the coarse dimension cap grows the target
        out[f"model6_K{K}"] = _scene(prob6, K=K, oracle=True)
    for world in (2, 4):
        for r, (a, b) in enumerate(shard_ranges(small.pt_idx, small.n_points, world)):
            out[f"shard_{r}_of_{world}"] = _scene(small, p0=int(a), p1=int(b), det=True)
    out["shard_empty"] = _scene(small, p0=450, p1=450, det=True)
    # band graphs (track p: L consecutive cameras, listed in descending order) on either side of the padding rule:
    # 30 rows of at most 2 (L - 1) neighbours, the end rows shorter -- L = 5: 240 slots for 220 (padded, with pad slots
    # inside rows in cluster order), L = 6: 300 for 270 (more than 10 % over: not padded)
    for L, name in ((5, "band_padded"), (6, "band_unpadded")):
        pt = np.repeat(np.arange(600), L)
        cam = (pt % (30 - L + 1)) + np.tile(np.arange(L)[::-1], 600)
        out[name] = _scene(types.SimpleNamespace(n_cams=30, n_points=600, model=2), cam, pt, K=4)
    # ragged scenes (tests/ragged_scene.py; the GPU runs them in test_gpu_ragged.py) at the product's cluster target:
    # tracks of 2..275 observations, duplicates, a camera that sees nothing and rows of ~269 upper blocks (dense, in
    # the atomic and the deterministic form of the Schur limits); tracks inside a window of 61 cameras (banded)
    dense = RS.dense_problem(2)
    out["ragged_dense"] = _scene(dense, K=24, oracle=True)
    out["ragged_dense_det"] = _scene(dense, K=24, det=True)
    out["ragged_banded"] = _scene(RS.banded_problem(2), K=24, oracle=True)
    return out


NAMES = sorted(["one_cluster", "duplicates", "empty_camera", "shard_empty", "band_padded", "band_unpadded",
                "ragged_dense", "ragged_dense_det", "ragged_banded",
                *(f"clusters_K{K}{p}" for K in (4, 16, 32) for p in ("", "_perm")), *(f"model6_K{K}" for K in (2, 3)),
                *(f"shard_{r}_of_{w}" for w in (2, 4) for r in range(w))])


def _pair_counts(sc):
    """[C, C] number of (observation of i, observation of j) pairs sharing a track, i != j: the brute force."""
    key = id(sc["cam_idx"])
    if key not in _pair_counts.cache:
        C = sc["prob"].n_cams
        W = np.zeros((C, C), dtype=np.int64)
        cam, pt = sc["cam_idx"], sc["pt_idx"]
        cuts = np.flatnonzero(np.diff(pt)) + 1
        for c in np.split(cam, cuts):
            u, n = np.unique(c, return_counts=True)
            W[np.ix_(u, u)] += np.outer(n, n)
        np.fill_diagonal(W, 0)
        _pair_counts.cache[key] = W
    return _pair_counts.cache[key]


_pair_counts.cache = {}


def _limits(sc, C, D):
    waves = DET_WAVES if sc["det"] else SCHUR_WAVES
    ws, bs = 4 * D + 1, D * D + (8 if (D * D) % 16 == 0 else 0)
    budget, target = LDS_BUDGET, (LDS_TARGET_DET if sc["det"] else LDS_TARGET)
    if sc["tight_lds"]:  # room for 10 blocks only: long rows are split
        budget = target = 8 * (D + 12) + 4 * C + 8 * waves * (64 // D) * ws + 64 + 8 * bs * 10 + 8
    return budget, target, waves, ws, bs


def schur_cap(limits, C, D):
    """blocks per Schur row chunk (create_plan.h plan_schur_work) under _limits' (budget, target, waves, ws, bs)"""
    _, target, waves, ws, _bs = limits
    fixed = 8 * (D + 12) + 4 * C + 8 * waves * (64 // D) * ws + 64
    return (target - fixed) // (8 * _bs)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    path = str(tmp_path_factory.mktemp("plan") / "create_plan_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-o", path,
                    os.path.join(REPO, "tests", "cpp", "create_plan_test.cpp")], check=True)
    return path


_plans = {}


@pytest.fixture
def plan(exe, tmp_path, request):
    """(scene, plan) of the scene named by the test's `name` parameter; run once per scene with pools of 1 and 5."""
    name = request.getfixturevalue("name")
    assert sorted(_scenes()) == NAMES
    sc = _scenes()[name]
    if name not in _plans:
        prob = sc["prob"]
        C, P, N, D = prob.n_cams, prob.n_points, sc["cam_idx"].size, 6 + MODEL_NI[prob.model]
        W = _pair_counts(sc)
        up = np.triu(W, 1)
        ri, ci = np.nonzero(up)  # row-major: per row the columns ascending, like k_pattern's compaction
        budget, target, waves, ws, bs = _limits(sc, C, D)
        hdr = [C, P, N, sc["p0"], sc["p1"], D, 1, sc["K"], X_CHUNKS, SCHUR_CHUNK * SCHUR_WAVES * (64 // D), budget, target,
               waves, ws, bs, LIN_THREADS, COARSE_MAX, SEG_MAX, PAD_SLOT, ri.size]
        np.concatenate([np.array(hdr, dtype=np.int64), sc["cam_idx"], sc["pt_idx"], np.bincount(ri, minlength=C), ci,
                        up[ri, ci]]).astype(np.int32).tofile(tmp_path / "in.bin")
        outs = []
        for pool in (1, 5):
            res = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / f"out{pool}.bin"), str(pool)],
                                 check=True, capture_output=True, text=True, timeout=60)
            outs.append((res.stdout, (tmp_path / f"out{pool}.bin").read_bytes()))
        assert outs[0] == outs[1], f"{name}: the plan depends on the pool size"
        data, pl, at = np.frombuffer(outs[0][1], dtype=np.int32), {}, 0
        for kind, key, val in (ln.split() for ln in outs[0][0].splitlines()):
            if kind == "scalar":
                pl[key] = int(val)
            else:
                pl[key] = data[at:at + int(val)]
                at += int(val)
        assert at == data.size
        pl.update(C=C, P=P, N=N, D=D, Pl=sc["p1"] - sc["p0"], limits=(budget, target, waves, ws, bs), hdr=hdr)
        _plans[name] = pl
    return sc, _plans[name]


def _rows(ptr):
    """row index of every entry of a CSR-style pointer array"""
    return np.repeat(np.arange(ptr.size - 1), np.diff(ptr))


@pytest.mark.parametrize("name", NAMES)
def test_track_order(plan, name):
    sc, pl = plan
    cam, pt = sc["cam_idx"], sc["pt_idx"]
    o0, Nl, Pl = pl["o0"], pl["Nl"], pl["Pl"]
    assert pl["check"] == 0
    assert np.array_equal(pl["gptr"], np.searchsorted(pt, np.arange(pl["P"] + 1)))
    assert o0 == pl["gptr"][sc["p0"]] and Nl == pl["gptr"][sc["p1"]] - o0
    assert np.array_equal(pl["lptr"], pl["gptr"][sc["p0"]:sc["p1"] + 1] - o0)
    lsrc, lcam, lptl, lust, key = (pl[k] for k in ("lsrc", "lcam", "lptl", "lust", "key"))
    assert np.array_equal(np.sort(lsrc), np.arange(o0, o0 + Nl))  # a permutation of the shard's observations
    assert np.array_equal(lptl, _rows(pl["lptr"])) and np.array_equal(lptl, pt[lsrc] - sc["p0"])
    assert np.array_equal(lcam, cam[lsrc])
    same = lptl[1:] == lptl[:-1]
    # within a track: cameras nondecreasing, equal cameras in input order
    assert np.all(~same | (lcam[:-1] < lcam[1:]) | ((lcam[:-1] == lcam[1:]) & (lsrc[:-1] < lsrc[1:])))
    # the upper partners of o are the contiguous tail [lust[o], track end): lust = start of o's camera run
    start = np.ones(Nl, dtype=bool)
    start[1:] = ~same | (lcam[1:] != lcam[:-1])
    assert np.array_equal(lust, np.maximum.accumulate(np.where(start, np.arange(Nl), 0)))
    assert np.array_equal(key, pl["lptr"][lptl + 1] - lust)


@pytest.mark.parametrize("name", NAMES)
def test_camera_major_lists(plan, name):
    sc, pl = plan
    cptr, cobs, key, lcam, chunk = pl["cptr"], pl["cobs"], pl["key"], pl["lcam"], pl["hdr"][9]
    assert cptr.size == pl["C"] + 1 and cptr[0] == 0 and cptr[-1] == pl["Nl"]
    assert np.array_equal(np.sort(cobs), np.arange(pl["Nl"]))
    crow = _rows(cptr)
    assert np.array_equal(lcam[cobs], crow)  # grouped by camera
    cid = (np.arange(pl["Nl"]) - cptr[crow]) // chunk
    # a chunk holds the observations point order puts there ...
    assert np.array_equal(cobs[np.lexsort((cobs, cid, crow))], np.argsort(lcam, kind="stable"))
    # ... by nonincreasing partner count, ties in point order
    same = (crow[1:] == crow[:-1]) & (cid[1:] == cid[:-1])
    ka, kb = key[cobs[:-1]], key[cobs[1:]]
    assert np.all(~same | (ka > kb) | ((ka == kb) & (cobs[:-1] < cobs[1:])))


@pytest.mark.parametrize("name", NAMES)
def test_block_pattern_and_graph(plan, name):
    sc, pl = plan
    C, W = pl["C"], _pair_counts(sc)
    rptr, cols, brow = pl["rptr"], pl["cols"], pl["brow"]
    assert np.array_equal(pl["gcptr"], np.concatenate([[0], np.cumsum(np.bincount(sc["cam_idx"], minlength=C))]))
    assert np.array_equal(brow, _rows(rptr))
    assert np.array_equal(cols[rptr[:-1]], np.arange(C))  # every row starts with its diagonal
    inner = np.ones(cols.size, dtype=bool)
    inner[rptr[:-1]] = False
    assert np.all(np.diff(cols)[inner[1:]] > 0)  # and is ascending
    A = np.zeros((C, C), dtype=bool)
    A[brow, cols] = True
    assert np.array_equal(A, (np.triu(W, 1) > 0) | np.eye(C, dtype=bool))  # the upper blocks: the co-visible pairs
    gptr, gnb, gw = pl["g_ptr"], pl["g_nb"], pl["g_w"]
    grow = _rows(gptr)
    G = np.zeros((C, C), dtype=np.int64)
    G[grow, gnb] = gw
    assert gw.size == np.count_nonzero(W) and np.array_equal(G, W) and np.all(gw > 0)
    assert np.all((np.diff(gnb) > 0) | (grow[1:] != grow[:-1]))
    # the assembly from the device-style upper lists gives the same pattern and graph
    for k in ("rptr", "cols", "g_ptr", "g_nb", "g_w"):
        assert np.array_equal(pl["dev_" + k], pl[k]), k
    assert np.array_equal(pl["dev_upw"], W[brow, cols])
    # lower transpose: per column the upper blocks in it, rows ascending
    lop, locol, loblk = pl["lop"], pl["locol"], pl["loblk"]
    n_lo = cols.size - C
    assert lop[-1] == n_lo
    lcol = _rows(lop)
    assert np.array_equal(cols[loblk[:n_lo]], lcol) and np.array_equal(brow[loblk[:n_lo]], locol[:n_lo])
    assert np.all((np.diff(locol[:n_lo]) > 0) | (lcol[1:] != lcol[:-1]))


@pytest.mark.parametrize("name", NAMES)
def test_clusters(plan, name):
    sc, pl = plan
    prob, lab = sc["prob"], pl["lab"]
    assert pl["coarse_ok"] == 1 and pl["nc"] * (pl["D"] + 1) <= COARSE_MAX
    assert lab.size == pl["C"] and np.array_equal(np.unique(lab), np.arange(pl["nc"]))
    if name == "one_cluster":
        assert pl["nc"] == 1
    if sc["oracle"]:
        ora = O.OracleBA(prob.model, prob.uv, sc["cam_idx"], sc["pt_idx"], prob.pp, prob.n_cams, prob.n_points,
                         cluster_size=sc["K"])
        lo, no = ora.clusters()
        assert pl["nc"] == no and np.array_equal(lab, lo)


@pytest.mark.parametrize("name", NAMES)
def test_neighbour_lists(plan, name):
    sc, pl = plan
    C, rptr, cols, brow, lab = pl["C"], pl["rptr"], pl["cols"], pl["brow"], pl["lab"]
    nptr, nj, pup, plo, n_nbr = pl["nptr"], pl["nj"], pl["pup"], pl["plo"], pl["n_nbr"]
    off = np.ones(cols.size, dtype=bool)
    off[rptr[:-1]] = False
    e = np.flatnonzero(off)
    r, c = brow[e], cols[e]
    assert np.array_equal(nj[pup[e]], c) and np.all((nptr[r] <= pup[e]) & (pup[e] < nptr[r + 1]))
    assert np.array_equal(nj[plo[e]], r) and np.all((nptr[c] <= plo[e]) & (plo[e] < nptr[c + 1]))
    used = np.concatenate([pup[e], plo[e]])
    assert np.unique(used).size == used.size == 2 * e.size  # all slots distinct
    assert np.all(pup[rptr[:-1]] == 0) and np.all(plo[rptr[:-1]] == 0)
    assert nptr[-1] == n_nbr and nj.size == max(n_nbr, 1)
    # padding: to equal-length rows exactly when that costs at most 10 % more slots
    longest = int((np.bincount(r, minlength=C) + np.bincount(c, minlength=C)).max())
    nn = 2 * e.size
    padded = longest > 0 and nn > 0 and C * longest * 10 <= nn * 11
    assert pl["nbr_stride"] == (longest if padded else 0)
    assert n_nbr == (C * longest if padded else nn)
    if padded:
        assert np.array_equal(nptr, np.arange(C + 1) * longest)
    pad = np.setdiff1d(np.arange(n_nbr), used)
    assert np.array_equal(nj[pad], _rows(nptr)[pad])  # pad slots hold the row itself
    if name.startswith("band_"):  # the two sides of the rule
        assert padded == (name == "band_padded") and (pad.size > 0) == padded
    # with a coarse space every row is in cluster order: what in_order reports
    nrow = _rows(nptr)
    ln = lab[nj[:n_nbr]]
    assert np.all((np.diff(ln) >= 0) | (nrow[1:] != nrow[:-1]))
    assert pl["in_order"] == 1 and np.array_equal(pl["sperm"][:n_nbr], np.arange(n_nbr))
    assert pl["maxlen"] == np.diff(nptr).max()
    assert pl["nb"] == (64 if pl["maxlen"] <= 64 else 128 if pl["maxlen"] <= 128 else 0)
    assert pl["nb_wide"] == (128 if pl["maxlen"] <= 128 else 0)
    assert pl["cgp_ok"] == int(pl["nb"] > 0 and pl["maxseg"] <= SEG_MAX)
    if name.startswith("ragged_"):  # dense: launch-path CG; banded: rows of 65..128 neighbours on the persistent CG
        assert (pl["nb"], pl["cgp_ok"]) == ((128, 1) if name == "ragged_banded" else (0, 0))
    # slot source list of k_tl_cgp
    src = pl["src"]
    assert np.array_equal(src[pup[e]], e) and np.array_equal(src[plo[e]], ~e)
    assert src.size == max(n_nbr, 1) and np.all(src[pad] == PAD_SLOT)


@pytest.mark.parametrize("name", NAMES)
def test_schur_work_and_exchange_chunks(plan, name):
    sc, pl = plan
    C, D, rptr = pl["C"], pl["D"], pl["rptr"]
    budget, target, waves, ws, bs = pl["limits"]
    work = pl["work"].reshape(-1, 4)
    row, kb, ke = work[:, 0], work[:, 1], work[:, 2]
    assert pl["fits"] == 1 and np.all(work[:, 3] == 0)
    first = np.ones(row.size, dtype=bool)
    first[1:] = row[1:] != row[:-1]
    last = np.roll(first, -1)
    # the items tile each row's block range in order
    assert np.array_equal(row[first], np.arange(C))
    assert np.array_equal(kb[first], rptr[:-1]) and np.array_equal(ke[last], rptr[1:])
    assert np.all(kb[1:][~first[1:]] == ke[:-1][~first[1:]]) and np.all(ke > kb)
    fixed = 8 * (D + 12) + 4 * C + 8 * waves * (64 // D) * ws + 64
    assert pl["cap"] == (target - fixed) // (8 * bs) == schur_cap(pl["limits"], C, D)
    assert np.all(ke - kb <= pl["cap"]) and pl["max_chunk"] == (ke - kb).max()
    assert pl["schur_lds"] <= budget and pl["schur_lds"] % 16 == 0
    if sc["tight_lds"]:
        assert pl["cap"] == 10 and row.size > C  # long rows were split
    if name.startswith("ragged_dense"):  # at the shipped limits: nearly every row is longer than a chunk
        assert not sc["tight_lds"] and np.diff(rptr).max() - 1 > pl["cap"] and row.size > C
        assert np.count_nonzero(np.bincount(row, minlength=C) > 1) > C // 3
        assert np.bincount(row, minlength=C)[7] == 1  # the camera that sees nothing: one item, its diagonal block
    xr, xw = pl["xr"], pl["xw"]
    assert xr.size == xw.size <= X_CHUNKS + 1
    assert xr[0] == 0 and xr[-1] == C and np.all(np.diff(xr) > 0)
    assert xw[0] == 0 and xw[-1] == row.size and np.all(np.diff(xw) > 0)
    assert np.array_equal(xw, np.searchsorted(row, xr, side="left"))  # the first work item of each boundary row


@pytest.mark.parametrize("name", NAMES)
def test_linearize_runs(plan, name):
    sc, pl = plan
    lb, lptr, Pl = pl["lb"], pl["lptr"], pl["Pl"]
    if Pl == 0:
        assert np.array_equal(lb, [0])
        return
    assert lb[0] == 0 and lb[-1] == Pl and np.all(np.diff(lb) > 0)
    tracks, obs = np.diff(lb), lptr[lb[1:]] - lptr[lb[:-1]]
    assert np.all(tracks <= LIN_THREADS) and np.all((obs <= LIN_THREADS) | (tracks == 1))
    if name.startswith("ragged_dense"):
        assert np.any((tracks == 1) & (obs > LIN_THREADS)) and np.any((tracks == 1) & (obs > 2 * LIN_THREADS))
        # a run closed by the observation limit: the next track would not have fitted, the track limit was not reached
        nxt = lptr[lb[1:-1] + 1] - lptr[lb[1:-1]]
        assert np.any((tracks[:-1] < LIN_THREADS) & (tracks[:-1] > 1) & (obs[:-1] + nxt > LIN_THREADS))
    if name == "ragged_banded":  # unequal tracks: no run reaches the track limit, every run is closed by observations
        assert np.all(tracks < LIN_THREADS) and np.unique(tracks).size > 3


@pytest.mark.parametrize("name", NAMES)
def test_coarse_segments(plan, name):
    sc, pl = plan
    C, nc, lab, nptr, nj, n_nbr = pl["C"], pl["nc"], pl["lab"], pl["nptr"], pl["nj"], pl["n_nbr"]
    clp, clc, sperm, rsp = pl["clp"], pl["clc"], pl["sperm"], pl["rsp"]
    segs = pl["segs"].reshape(-1, 4)
    assert np.array_equal(clc, np.argsort(lab, kind="stable")) and np.array_equal(clp, np.searchsorted(lab[clc], np.arange(nc + 1)))
    assert np.array_equal(pl["cpos"][clc], np.arange(C))
    size = np.diff(clp)
    assert pl["maxmem"] == size.max() and np.array_equal(pl["alone"], (size[lab] < 2).astype(np.int32))
    nrow = _rows(nptr)
    assert np.array_equal(np.sort(sperm[:n_nbr]), np.arange(n_nbr)) and np.array_equal(nrow[sperm[:n_nbr]], nrow)
    # each row's segments partition its sperm-ordered slots by neighbour cluster, with exactly one own-cluster segment
    srow = _rows(rsp)
    scl, qb, qe, own = segs.T
    first = np.ones(srow.size, dtype=bool)
    first[1:] = srow[1:] != srow[:-1]
    assert rsp[-1] == srow.size and np.all(np.diff(rsp) >= 1) and pl["maxseg"] == np.diff(rsp).max()
    assert np.all(qb[first] == 0) and np.array_equal(qe[np.roll(first, -1)], np.diff(nptr))
    assert np.all(qb[1:][~first[1:]] == qe[:-1][~first[1:]])
    assert np.all((np.diff(scl) > 0) | first[1:])
    assert np.array_equal(own, (scl == lab[srow]).astype(np.int32)) and np.array_equal(np.bincount(srow[own == 1]), np.ones(C))
    assert np.all((qe > qb) | (own == 1))
    slot_seg = np.repeat(np.arange(srow.size), qe - qb)  # the segment of every slot, in (row, sperm) order
    assert slot_seg.size == n_nbr and np.array_equal(lab[nj[sperm[:n_nbr]]], scl[slot_seg])
    # E source lists: every segment once, under its (row cluster, column cluster) pair, rows ascending
    eptr, eseg = pl["eptr"], pl["eseg"]
    assert eptr.size == nc * nc + 1 and eptr[-1] == srow.size == eseg.size
    assert np.array_equal(np.sort(eseg), np.arange(srow.size))
    pair = _rows(eptr)
    assert np.array_equal(pair, lab[srow[eseg]] * nc + scl[eseg])
    assert np.all((np.diff(srow[eseg]) > 0) | (pair[1:] != pair[:-1]))
