"""Pruning on the HIP path: insfm_covis_pairs (csrc/covis.hip) against the numpy host path (instantsfm_amd/covis.py)
and the reference's recorded pair lists (tests/golden/pruning_golden.npz), the processor on cuda:0, and the mapper's
last stage.  Every comparison is exact: the work is integer counting.  Needs an MI355X."""
import contextlib
import io
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import mapper_scene as MS  # noqa: E402
import pruning_scene as PS  # noqa: E402
from instantsfm_amd import _capi, covis  # noqa: E402
from instantsfm_amd.controllers.config import Config  # noqa: E402
from instantsfm_amd.controllers.global_mapper import SolveGlobalMapper  # noqa: E402
from instantsfm_amd.processors import reconstruction_pruning as RP  # noqa: E402
from oracle import mapper as OM  # noqa: E402

FILL = -7


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "pruning_golden.npz")) as z:
        return dict(z)


def csr(rows):
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return ptr, (np.concatenate(rows) if len(rows) and ptr[-1] else np.zeros(0)).astype(np.int32)


def check_against_host(ptr, img, min_count=5):
    """One library call with room for every ordinal; its output reordered by pair_first must be the host path's, the
    rest of the buffers untouched.  Returns the host list."""
    lo, hi, count, first, total = covis.host_pairs(ptr, img, min_count)
    rc, glo, ghi, gcount, gfirst, counts = covis.device_call(ptr, img, min_count, max(total, 1), fill=FILL)
    assert rc == 0
    assert counts == (len(lo), total)
    n = counts[0]
    order = np.argsort(gfirst[:n], kind="stable")
    np.testing.assert_array_equal(gfirst[:n][order], first)
    np.testing.assert_array_equal(glo[:n][order], lo)
    np.testing.assert_array_equal(ghi[:n][order], hi)
    np.testing.assert_array_equal(gcount[:n][order], count)
    for a in (glo, ghi, gcount, gfirst):
        assert (a[n:] == FILL).all()
    return lo, hi, count


@pytest.fixture(scope="module")
def ragged():
    """20k tracks over 300 images: lengths 0-12 drawn at random, plus 64, 65, 257 and one of 300 rows that sees every
    image once (44,850 ordinals), placed among them."""
    rng = np.random.default_rng(5)
    rows = [rng.integers(0, 300, int(n)) for n in rng.integers(0, 13, 20_000)]
    for at, n in ((17, 64), (5_000, 65), (12_345, 257)):
        rows[at] = rng.integers(0, 300, n)
    rows[19_999] = rng.permutation(300)
    return csr(rows)


@pytest.mark.parametrize("name", PS.names())
def test_kernel_matches_host_path_and_reference(golden, name):
    M, ptr, img = PS.scene(name)
    lo, hi, count = check_against_host(ptr, img)
    np.testing.assert_array_equal(np.stack([hi, lo, count], 1), golden[f"{name}_pairs"])
    wlo, whi, wcount = covis.covis_pairs(ptr, img)  # the wrapper: capacity min(ordinals, M(M-1)/2), sorted
    np.testing.assert_array_equal(np.stack([whi, wlo, wcount], 1), golden[f"{name}_pairs"])


def test_no_tracks():
    rc, lo, hi, count, first, counts = covis.device_call(np.zeros(1, np.int64), np.zeros(0, np.int32), 5, 4, fill=FILL)
    assert rc == 0 and counts == (0, 0) and (lo == FILL).all() and (first == FILL).all()
    assert [len(a) for a in covis.covis_pairs(np.zeros(1, np.int64), np.zeros(0, np.int32))] == [0, 0, 0]


def test_only_short_tracks_give_no_ordinals():
    ptr, img = csr([[], [3], [1, 2], [], [2, 1], [4], [1, 2]] * 50)
    assert covis.host_pairs(ptr, img, 1)[4] == 0
    assert len(check_against_host(ptr, img, 1)[0]) == 0


def test_three_row_tracks():
    rng = np.random.default_rng(0)
    ptr, img = csr([rng.integers(0, 6, 3) for _ in range(1000)])
    assert len(check_against_host(ptr, img)[0]) == 15


def test_track_of_one_image():
    ptr, img = csr([[7] * 6])
    assert covis.host_pairs(ptr, img, 1)[4] == 15
    assert len(check_against_host(ptr, img, 1)[0]) == 0
    ptr, img = csr([[7] * 6, [1, 2, 3], [7] * 3, [2, 1, 3]])
    assert len(check_against_host(ptr, img, 2)[0]) == 3


def sorted_keys(ptr, img):
    """What the radix sort of csrc/covis.hip leaves: (lo << 32) | hi of every ordinal, all ones for a pair of one image."""
    keys = [(min(a, b) << 32 | max(a, b)) if a != b else 2 ** 64 - 1
            for s, e in zip(ptr[:-1], ptr[1:]) for i, a in enumerate(img[s:e].tolist()) for b in img[s + i + 1:e].tolist()
            if e - s > 2]
    return sorted(keys)


def block_edge_scenes():
    """Ordinal totals of 3, 255, 256 and 257 (3 per 3-row track, 10 per 5-row track): one element, and the 256-thread
    block edge of the run segmentation.  The last two have 257: in one the run of (3, 9) starts exactly at sorted
    position 256, in the other it lies on positions 255 | 256."""
    rng = np.random.default_rng(7)
    few = lambda n, rows: [rng.integers(0, 7, rows) for _ in range(n)]  # noqa: E731
    fives = [[0, 1, 2, 3, 4], [0, 1, 2, 3, 9]]
    scenes = [(3, csr([[4, 2, 7]])), (255, csr(few(85, 3))), (256, csr(few(82, 3) + few(1, 5))),
              (257, csr([[0, 1, 2]] * 79 + fives)), (257, csr([[0, 1, 2]] * 78 + [[3, 9, 0]] + fives))]
    starts_at_256, straddles = sorted_keys(*scenes[3][1]), sorted_keys(*scenes[4][1])
    assert starts_at_256[255] != starts_at_256[256] == (3 << 32 | 9)
    assert straddles[254] != straddles[255] == straddles[256] == (3 << 32 | 9)
    return scenes


@pytest.mark.parametrize("min_count", [5, 1])
def test_long_and_ragged_tracks(ragged, min_count):
    for total, (p, im) in block_edge_scenes():
        assert len(sorted_keys(p, im)) == covis.host_pairs(p, im, min_count)[4] == total
        check_against_host(p, im, min_count)
    ptr, img = ragged
    L = np.diff(ptr)
    assert {64, 65, 257, 300} <= set(L.tolist()) and (L == 0).any()
    lo, hi, count = check_against_host(ptr, img, min_count)
    assert len(lo) > 40_000 if min_count == 1 else 0 < len(lo) < 44_850
    wlo, whi, wcount = covis.covis_pairs(ptr, img, min_count)
    assert np.array_equal(wlo, lo) and np.array_equal(whi, hi) and np.array_equal(wcount, count)


def test_count_threshold_is_inclusive():
    """A pair seen exactly 4 times is dropped at min_count 5, one seen exactly 5 times is kept."""
    ptr, img = csr([[10, 11, 40 + k] for k in range(4)] + [[21, 50 + k, 20] for k in range(5)])
    lo, hi, count = check_against_host(ptr, img, 5)
    assert (lo.tolist(), hi.tolist(), count.tolist()) == ([20], [21], [5])
    assert (10, 11, 4) in zip(*[a.tolist() for a in check_against_host(ptr, img, 4)])


def test_image_ids_above_16_bits():
    big = [65_535, 65_536, 70_000, 1 << 20, (1 << 24) + 1, 2 ** 31 - 1]
    rng = np.random.default_rng(1)
    ptr, img = csr([rng.choice(big, 4) for _ in range(300)] + [[65_536, 1, 65_537]] * 6)
    lo, hi, count = check_against_host(ptr, img)
    assert hi.max() == 2 ** 31 - 1 and (65_536, 65_537) in zip(lo.tolist(), hi.tolist())


def test_capacity_one_short_writes_nothing(ragged):
    ptr, img = ragged
    n = len(covis.host_pairs(ptr, img, 5)[0])
    rc, lo, hi, count, first, counts = covis.device_call(ptr, img, 5, n - 1, fill=FILL)
    assert rc == _capi.INSFM_BA_EINVAL and counts[0] == 0
    for a in (lo, hi, count, first):
        assert len(a) == n - 1 and (a == FILL).all()
    rc, lo, hi, count, first, counts = covis.device_call(ptr, img, 5, n, fill=FILL)
    assert rc == 0 and counts[0] == n and (lo != FILL).all()


def test_two_runs_are_byte_identical(ragged):
    ptr, img = ragged
    total = covis.pair_ordinals(ptr)[1]
    a = covis.device_call(ptr, img, 2, total, fill=FILL)
    b = covis.device_call(ptr, img, 2, total, fill=FILL)
    assert a[0] == b[0] == 0 and a[5] == b[5]
    for x, y in zip(a[1:5], b[1:5]):
        assert x.tobytes() == y.tobytes()


def _prune(M, ptr, img, device):
    images, tracks = PS.as_objects(M, ptr, img)
    with contextlib.redirect_stdout(io.StringIO()):
        RP.PruneWeaklyConnectedImages(images, tracks, device=device)
    return np.array([im.is_registered for im in images]), np.array([im.cluster_id for im in images])


@pytest.mark.parametrize("name", PS.names())
def test_processor_on_gpu_matches_reference_and_host(golden, name):
    M, ptr, img = PS.scene(name)
    reg, cl = _prune(M, ptr, img, "cuda:0")
    np.testing.assert_array_equal(reg, golden[f"{name}_registered"])
    np.testing.assert_array_equal(cl, golden[f"{name}_cluster"])
    reg2, cl2 = _prune(M, ptr, img, "cpu")
    assert np.array_equal(reg, reg2) and np.array_equal(cl, cl2)


def test_mapper_runs_pruning_last(tmp_path):
    """SolveGlobalMapper with for_ba_half(pruning=True): the stages before pruning are the run without it (same stage
    list, same track / observation counts; the LM figures of two runs of the same kernels within the bounds
    test_gpu_mapper.py holds GPU and CPU pipelines to -- floating-point atomics may reorder sums between runs), the
    last trace entry is 'pruned', and the flags and cluster ids are what the host path gives on the returned tracks.
    The CPU pipeline's tracks say beforehand that this scene's visibility graph is not empty."""
    scene = MS.make_db(tmp_path / "db.db", seed=0)
    vg0, cams0, ims0, cfg0 = MS.load(tmp_path / "db.db", scene, seed=0)
    np.random.seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        _, _, cpu_tracks = OM.solve_global_mapper(vg0, cams0, ims0, cfg0, trace=[])
    assert len(covis.covis_pairs(*RP._track_rows(cpu_tracks), device="cpu")[0]) > 0

    runs = []
    for pruning in (False, True):
        vg, cams, ims, cfg = MS.load(tmp_path / "db.db", scene, seed=0)
        cfg = Config.for_ba_half(cfg.feature_name, pruning=pruning)
        np.random.seed(0)
        T = {}
        with contextlib.redirect_stdout(io.StringIO()):
            _, ims, tracks = SolveGlobalMapper(vg, cams, ims, cfg, timings=T)
        runs.append((T, ims, tracks))
    (T0, _, tracks0), (T1, ims1, tracks1) = runs
    plain, pruned = T0['trace'], T1['trace']
    assert plain[-1][0] == 'retri_filtered' and 'pruning_s' not in T0
    assert pruned[-1] == ('pruned',) + pruned[-2][1:3] + (None,) and T1['pruning_s'] > 0
    assert [p[0] for p in pruned[:-1]] == [p[0] for p in plain]
    for g, r in zip(pruned[:-1], plain):
        assert g[1:3] == r[1:3], (g, r)
        if g[0] == 'gp':
            assert abs(g[3] - r[3]) <= 1e-6 * abs(r[3]), (g, r)
        elif g[3] is not None:
            assert abs(g[3] - r[3]) <= 1e-4, (g, r)
    assert list(tracks1.keys()) == list(tracks0.keys())

    expect = [type(im)(id=im.id, is_registered=True) for im in ims1]
    with contextlib.redirect_stdout(io.StringIO()):
        RP.PruneWeaklyConnectedImages(expect, tracks1, device="cpu")
    assert [im.is_registered for im in ims1] == [im.is_registered for im in expect]
    assert [im.cluster_id for im in ims1] == [im.cluster_id for im in expect]
    assert any(im.cluster_id == 0 for im in ims1)
