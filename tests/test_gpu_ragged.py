"""HIP path vs the C oracle on ragged scenes (tests/ragged_scene.py): tracks of 2 to 275 observations, duplicated
observations, a camera that sees nothing and Schur rows longer than a row chunk.  Needs an MI355X.

The uniform scenes of test_gpu_parity.py / test_gpu_gp.py (every track 10 long, every camera equally busy) never run
 * k_lin_points' / k_backsub_rc's pass loop over one track longer than the workgroup, nor runs of unequal tracks
   closed by the observation limit,
 * k_schur on a row split into chunks at the product's block sizes (only the first chunk adds U and b), in the atomic,
   the deterministic (ORD) and the retried-trial (RETRY) form, nor with very unequal partner counts inside a wave,
   nor the form a multi-rank run launches (rank 0 adds U and g_c in k_schur, one launch per exchange range),
 * block dimensions 7 and 9 beyond the linearization,
 * the persistent CG on rows of unequal length,
 * global positioning on any of the above.
Each test asserts the scene properties it was written for (longest track, empty camera, duplicates, rows longer than
the chunk cap, CG path), so a later change of constants cannot hollow it out silently.

Tolerances (as on the uniform scenes): records, V, g_p 1e-12; U, g_c, b 1e-10; S~ 1e-9; dc, dp 1e-8;
parameters after a step 1e-9; loss 1e-10; cost 1e-12.  The oracle's own plain-vs-fma rounding spread on these scenes
is at least ~8x below each of them.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import ragged_scene as RS  # noqa: E402
import test_gpu_gp as GPT  # noqa: E402
from oracle import oracle as O  # noqa: E402
from test_create_plan import LIN_THREADS, _limits, schur_cap  # noqa: E402
from test_gpu_parity import MODELS, dev, engines, rel, y_records  # noqa: E402

F1 = 1.0 + 1e-4     # the first trial's damping factor (1 + 1 / tr_radius): the factor the records are prepared for
F2 = 1.0 + 1.3e-2   # another factor at the same linearization: k_schur's RETRY form (Y M_p)


@pytest.fixture(scope="module")
def scenes():
    """(family, model) -> problem, built once per module"""
    cache = {}

    def get(family, model=2):
        if (family, model) not in cache:
            cache[family, model] = {"dense": RS.dense_problem, "banded": RS.banded_problem,
                                    "gp": lambda m: RS.dense_gp_problem(init="perturbed", init_sigma=0.5)}[family](model)
        return cache[family, model]
    return get


def track_lengths(prob):
    ptr = RS.track_ptr(prob.pt_idx, prob.n_points)
    return np.array([np.unique(prob.cam_idx[a:b]).size for a, b in zip(ptr[:-1], ptr[1:])])


def check_dense_scene(prob, long_track):
    """what the dense family is for: a track past `long_track` linearize passes' worth of observations, a camera
    without observations, duplicated observations"""
    assert track_lengths(prob).max() > long_track
    assert np.count_nonzero(np.bincount(prob.cam_idx, minlength=prob.n_cams) == 0) == 1
    assert RS.duplicates(prob.cam_idx, prob.pt_idx).sum() >= 1


def check_split_rows(prob, ora, D, det):
    """the longest Schur row has more upper blocks than a row chunk holds at the shipped limits (plan_schur_work), so
    k_schur runs rows in several chunks -- except D = 7 in the atomic form, whose chunk (206 blocks) holds a whole row
    of the 140-camera scene (it splits in deterministic mode, cap 112)"""
    rp, _ = ora.pattern()
    longest = int(np.diff(rp).max()) - 1
    cap = schur_cap(_limits(dict(det=det, tight_lds=False), prob.n_cams, D), prob.n_cams, D)
    assert (longest > cap) == (not (D == 7 and not det)), (longest, cap, D, det)
    return longest, cap


def report(tag, figures, bounds):
    """print every figure, then hold each to its bound"""
    print(tag, {k: f"{v:.2e}" for k, v in figures.items()})
    for k, v in figures.items():
        assert v < bounds[k], (tag, k, v, bounds[k])


@pytest.mark.parametrize("model", MODELS)
def test_ragged_linearize_parity(scenes, model):
    """Y records, V, g_p, U, g_c on the dense scene, and on their own the records and V of every planted long track
    (the pass loop over one track) and of the first and the last track of every k_lin_points run (so that a fault
    confined to one track cannot hide under the global max norm)."""
    prob = scenes("dense", model)
    eng, ora = engines(prob, deterministic=True)
    N, P, C, D = prob.n_obs, prob.n_points, prob.n_cams, eng.D
    planted = RS.dense_shape(model)[1]
    check_dense_scene(prob, 2 * LIN_THREADS if model == 2 else LIN_THREADS)
    check_split_rows(prob, ora, D, True)
    assert eng.cg_info()[0] == 0, eng.cg_info()
    eng.debug_linearize(dev(prob.cams_init), dev(prob.points_init))
    ora.linearize(prob.cams_init, prob.points_init)
    Yg, Yo = eng.debug_get(0, (N, 3, D)).transpose(0, 2, 1), y_records(ora, prob.pt_idx, F1)
    Vg, Vo = eng.debug_get(1, (P, 6)), ora.get(O.V)
    report(f"model {model}", dict(Y=rel(Yg, Yo), V=rel(Vg, Vo), gp=rel(eng.debug_get(2, (P, 3)), ora.get(O.GP)),
                                  U=rel(eng.debug_get(3, (C, D, D)), ora.get(O.U)),
                                  gc=rel(eng.debug_get(4, (C, D)), ora.get(O.GC))),
           dict(Y=1e-12, V=1e-12, gp=1e-12, U=1e-10, gc=1e-10))
    ptr = RS.track_ptr(prob.pt_idx, P)
    lb = RS.lin_runs(prob.pt_idx, P, LIN_THREADS)
    runs_t, runs_o = np.diff(lb), ptr[lb[1:]] - ptr[lb[:-1]]
    long_tracks = np.flatnonzero(track_lengths(prob) >= min(planted))
    assert long_tracks.size == len(planted)
    # the runs the scene is for: single tracks of more than one (D = 8: two) passes, and runs of unequal tracks
    assert np.count_nonzero((runs_t == 1) & (runs_o > (2 if model == 2 else 1) * LIN_THREADS)) >= 2
    assert np.any((runs_t > 1) & (runs_t < LIN_THREADS))
    worst = dict(Y=0.0, V=0.0)
    for p in np.unique(np.concatenate([long_tracks, lb[:-1], lb[1:] - 1])):
        a, b = ptr[p], ptr[p + 1]
        fy, fv = rel(Yg[a:b], Yo[a:b]), rel(Vg[p], Vo[p])
        assert fy < 1e-12 and fv < 1e-12, (int(p), int(b - a), fy, fv)
        worst = dict(Y=max(worst["Y"], fy), V=max(worst["V"], fv))
    report(f"model {model} per track", worst, dict(Y=1e-12, V=1e-12))
    eng.close()


@pytest.mark.parametrize("model", (0, 2, 3, 4, 6))
@pytest.mark.parametrize("det", (False, True))
@pytest.mark.parametrize("precond", (0, 1))
def test_ragged_solve_parity(scenes, model, det, precond):
    """One linearization of the dense scene, then the first trial's solve and a retried one (k_schur RETRY) on rows
    split into chunks: same block count and PCG iterations, b, S~, dc, dp; in deterministic mode a second handle
    gives bitwise the same S~, b and dc."""
    prob = scenes("dense", model)
    eng, ora = engines(prob, deterministic=det, precond=precond)
    C, P, D = prob.n_cams, prob.n_points, eng.D
    check_dense_scene(prob, 2 * LIN_THREADS if model == 2 else LIN_THREADS)
    longest, cap = check_split_rows(prob, ora, D, det)
    assert eng.cg_info()[0] == 0, eng.cg_info()  # rows of more than 128 neighbours (or D != 8): the launch-path CG
    nb = eng.nnzb()
    assert nb == ora.nnzb()
    twin = engines(prob, deterministic=True, precond=precond)[0] if det else None
    for h in (eng, twin):
        if h is not None:
            h.debug_linearize(dev(prob.cams_init), dev(prob.points_init))
    ora.linearize(prob.cams_init, prob.points_init)
    for f in (F1, F2):
        it_g, it_o = eng.debug_solve(f), ora.solve(f)
        print(f"model {model} det {det} precond {precond} f {f}: longest row {longest} cap {cap}, PCG {it_g} / {it_o}")
        assert it_g == it_o
        got = [eng.debug_get(5, (nb, D, D)), eng.debug_get(6, (C, D)), eng.debug_get(7, (C, D)), eng.debug_get(8, (P, 3))]
        report(f"  f {f}", dict(b=rel(got[1], ora.get(O.B)), S=rel(got[0], ora.get(O.S)), dc=rel(got[2], ora.get(O.DC)),
                                dp=rel(got[3], ora.get(O.DP))), dict(b=1e-10, S=1e-9, dc=1e-8, dp=1e-8))
        if twin is not None:
            assert twin.debug_solve(f) == it_g
            for k, which in enumerate((5, 6, 7)):
                assert np.array_equal(twin.debug_get(which, got[k].shape), got[k]), (f, which)
    for h in (eng, twin):
        if h is not None:
            h.close()


@pytest.fixture
def group_of_one():
    """a gloo process group of this process alone (loopback), for a handle with the all-reduce callbacks forced on"""
    import socket
    import torch.distributed as dist
    assert not dist.is_initialized()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        yield
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("model,det,chunks", [(2, False, 4), (2, True, 4), (4, True, 1), (6, False, 4)])
def test_ragged_exchange_form_solve_parity(scenes, group_of_one, model, det, chunks):
    """The form of the Schur build every rank of a multi-rank run launches, on split rows.  A single-rank handle's
    k_schur adds neither U nor g_c (k_cg_factor adds them behind k_lin_cams), so there a later chunk of a row that
    added them again would go unnoticed; with the all-reduce callbacks on (force_exchange, a group of one) rank 0's
    k_schur adds U' and g_c itself -- in the row's first chunk only -- and, with exchange_chunks > 1, is launched once
    per range of work items, whose boundaries must fall on the first chunk of a row.  Same checks and bounds as
    test_ragged_solve_parity, first trial and retried trial."""
    prob = scenes("dense", model)
    eng, ora = engines(prob, deterministic=det, precond=1, force_exchange=True, exchange_chunks=chunks)
    C, P, D = prob.n_cams, prob.n_points, eng.D
    check_dense_scene(prob, 2 * LIN_THREADS if model == 2 else LIN_THREADS)
    longest, cap = check_split_rows(prob, ora, D, det)
    assert eng.cg_info()[0] == 0, eng.cg_info()
    nb = eng.nnzb()
    assert nb == ora.nnzb()
    eng.debug_linearize(dev(prob.cams_init), dev(prob.points_init))
    ora.linearize(prob.cams_init, prob.points_init)
    calls = 0
    for f in (F1, F2):
        it_g, it_o = eng.debug_solve(f), ora.solve(f)
        print(f"exchange form model {model} det {det} chunks {chunks} f {f}: longest row {longest} cap {cap}, "
              f"PCG {it_g} / {it_o}, callbacks {eng.exchange_calls[0]}")
        assert it_g == it_o and not eng._errors
        assert eng.exchange_calls[0] - calls >= chunks  # (chunks > 1: one per row range and one for b)
        calls = eng.exchange_calls[0]
        report(f"  f {f}", dict(b=rel(eng.debug_get(6, (C, D)), ora.get(O.B)), S=rel(eng.debug_get(5, (nb, D, D)), ora.get(O.S)),
                                dc=rel(eng.debug_get(7, (C, D)), ora.get(O.DC)), dp=rel(eng.debug_get(8, (P, 3)), ora.get(O.DP))),
               dict(b=1e-10, S=1e-9, dc=1e-8, dp=1e-8))
    eng.close()


@pytest.mark.parametrize("det", (False, True))
def test_ragged_banded_solve_and_step(scenes, det):
    """The banded scene (model 2, product defaults): rows of at most 128 neighbours, so the persistent A-DEF2 k_tl_cgp
    runs (path 4, deterministic 5) on rows of unequal length.  The reduced system of the first linearization (b, S~),
    then 4 LM steps against the oracle's precond 2 with the bounds of test_adef2_coarse_correction_matches_oracle:
    same trials, PCG iterations within one, loss 1e-8, parameters 1e-7."""
    prob = scenes("banded")
    C, D = prob.n_cams, 8
    lengths = track_lengths(prob)
    assert lengths.min() == 2 and lengths.max() == 61 and RS.duplicates(prob.cam_idx, prob.pt_idx).sum() >= 1
    eng, ora = engines(prob, deterministic=det)
    assert eng.cg_info()[0] == (5 if det else 4), eng.cg_info()
    rp, _ = ora.pattern()
    assert np.unique(np.diff(rp)).size > 10  # ragged rows
    eng.debug_linearize(dev(prob.cams_init), dev(prob.points_init))
    ora.linearize(prob.cams_init, prob.points_init)
    it_g, it_o = eng.debug_solve(F1), ora.solve(F1)
    nb = eng.nnzb()
    assert nb == ora.nnzb() and abs(it_g - it_o) <= 1, (it_g, it_o)
    report(f"banded det {det}", dict(b=rel(eng.debug_get(6, (C, D)), ora.get(O.B)),
                                     S=rel(eng.debug_get(5, (nb, D, D)), ora.get(O.S))), dict(b=1e-10, S=1e-9))
    eng.close()
    eng, ora = engines(prob, deterministic=det)
    cg, pg = dev(prob.cams_init), dev(prob.points_init)
    co, po = prob.cams_init.copy(), prob.points_init.copy()
    for s in range(4):
        lg, st = eng.step(cg, pg)
        lo = ora.step(co, po)
        so = ora.stats()
        print(f"banded det {det} step {s}: loss {abs(lg - lo) / lo:.2e} PCG {st['pcg_iters']} / {so['pcg_iters']}")
        assert st["trials"] == so["trials"] and abs(st["pcg_iters"] - so["pcg_iters"]) <= 1, (s, st, so)
        assert st["failed"] == so["failed"] == 0
        assert abs(lg - lo) / lo < 1e-8, (s, lg, lo)
    report(f"banded det {det} parameters", dict(cams=rel(cg.cpu().numpy(), co), pts=rel(pg.cpu().numpy(), po)),
           dict(cams=1e-7, pts=1e-7))
    eng.close()


@pytest.mark.parametrize("model", (0, 2, 3, 4))
def test_ragged_step_parity(scenes, model):
    """4 LM steps on the dense scene in lockstep with the oracle (precond 1), as test_step_parity.  The camera that sees
    nothing comes back bit-for-bit unchanged, as the oracle leaves it."""
    prob = scenes("dense", model)
    eng, ora = engines(prob, precond=1)
    check_dense_scene(prob, 2 * LIN_THREADS if model == 2 else LIN_THREADS)
    check_split_rows(prob, ora, eng.D, False)
    assert eng.cg_info()[0] == 0, eng.cg_info()
    cg, pg = dev(prob.cams_init), dev(prob.points_init)
    co, po = prob.cams_init.copy(), prob.points_init.copy()
    for s in range(4):
        lg, st = eng.step(cg, pg)
        lo = ora.step(co, po)
        so = ora.stats()
        assert st["pcg_iters"] == so["pcg_iters"] and st["trials"] == so["trials"], (s, st, so)
        assert st["failed"] == so["failed"] == 0
        report(f"model {model} step {s}", dict(loss=abs(lg - lo) / lo, cams=rel(cg.cpu().numpy(), co),
                                               pts=rel(pg.cpu().numpy(), po)), dict(loss=1e-10, cams=1e-9, pts=1e-9))
    empty = int(np.flatnonzero(np.bincount(prob.cam_idx, minlength=prob.n_cams) == 0)[0])
    assert np.array_equal(co[empty], prob.cams_init[empty])
    assert np.array_equal(cg.cpu().numpy()[empty], prob.cams_init[empty])
    assert not np.array_equal(cg.cpu().numpy()[empty + 1], prob.cams_init[empty + 1])
    eng.close()


@pytest.mark.parametrize("family", ("dense", "banded"))
def test_ragged_cost_parity(scenes, family):
    prob = scenes(family)
    eng, ora = engines(prob)
    assert track_lengths(prob).max() > (2 * LIN_THREADS if family == "dense" else 60)
    assert eng.cg_info()[0] == (0 if family == "dense" else 4), eng.cg_info()
    lg, rg = eng.cost(dev(prob.cams_init), dev(prob.points_init))
    lo, ro = ora.cost(prob.cams_init, prob.points_init)
    report(f"cost {family}", dict(loss=abs(lg - lo) / lo, rmse=abs(rg - ro) / ro), dict(loss=1e-12, rmse=1e-12))
    eng.close()


def test_ragged_points_only(scenes):
    """optimize_poses=False on the dense scene: k_lin_points returns before the records (Y null) on runs of one long
    track; 3 steps as test_points_only_mode."""
    prob = scenes("dense")
    eng, ora = engines(prob, optimize_poses=False)
    check_dense_scene(prob, 2 * LIN_THREADS)
    assert eng.cg_info()[0] == 0, eng.cg_info()
    cg, pg = dev(prob.cams_init), dev(prob.points_init)
    co, po = prob.cams_init.copy(), prob.points_init.copy()
    for s in range(3):
        lg, _ = eng.step(cg, pg)
        lo = ora.step(co, po)
        print(f"points only step {s}: loss {abs(lg - lo) / lo:.2e}")
        assert abs(lg - lo) / lo < 1e-10
    assert np.array_equal(cg.cpu().numpy(), prob.cams_init)  # cameras frozen
    ptr = RS.track_ptr(prob.pt_idx, prob.n_points)
    long_tracks = np.flatnonzero(np.diff(ptr) > LIN_THREADS)
    report("points only", dict(pts=rel(pg.cpu().numpy(), po), long=rel(pg.cpu().numpy()[long_tracks], po[long_tracks])),
           dict(pts=1e-9, long=1e-9))
    eng.close()


def check_gp_scene(p, eng):
    """the dense global-positioning scene: a track longer than a linearize pass, a camera without observations,
    duplicates, fixed and free scales.  (D = 3: a row chunk holds 1112 blocks, so no row of 140 cameras is split.)"""
    ptr = RS.track_ptr(p.pt_idx, p.n_points)
    assert np.diff(ptr).max() > LIN_THREADS
    assert np.count_nonzero(np.bincount(p.cam_idx, minlength=p.n_cams) == 0) == 1
    assert RS.duplicates(p.cam_idx, p.pt_idx).sum() >= 1
    assert 0 < np.count_nonzero(p.sfree == 0) < p.n_obs
    assert eng.cg_info()[0] == 0, eng.cg_info()


@pytest.mark.parametrize("precond", (0, 1))
@pytest.mark.parametrize("f", (1.001, 1.5))
@pytest.mark.parametrize("det", (False, True))
def test_ragged_gp_solve_parity(scenes, precond, f, det):
    """test_gp_solve_parity's checks and bounds on the dense ragged scene (140 cameras, 30 % fixed scales), with the
    Schur build of either mode: k_schur_gp, and deterministic mode's k_schur<3, GPW, ORD>."""
    p = scenes("gp")
    eng, ora = GPT.engines(p, precond=precond, deterministic=det)
    check_gp_scene(p, eng)
    eng.debug_linearize(GPT.dev(p.cams_init), GPT.dev(p.points_init), GPT.dev(p.scales_init))
    ora.linearize(p.cams_init, p.points_init, p.scales_init)
    it_g, it_o = eng.debug_solve(f), ora.solve(f)
    assert it_g == it_o
    C, P = p.n_cams, p.n_points
    ds_g, ds_o = eng.debug_ds(), ora.ds()
    report(f"gp precond {precond} f {f} det {det}",
           dict(V=rel(eng.debug_get(1, (P, 6)), ora.get(O.V)), gp=rel(eng.debug_get(2, (P, 3)), ora.get(O.GP)),
                b=rel(eng.debug_get(6, (C, 3)), ora.get(O.B)), dc=rel(eng.debug_get(7, (C, 3)), ora.get(O.DC)),
                dp=rel(eng.debug_get(8, (P, 3)), ora.get(O.DP)), ds=rel(ds_g, ds_o)),
           dict(V=1e-12, gp=1e-12, b=1e-10, dc=1e-8, dp=1e-8, ds=1e-8))
    assert np.all(ds_g[p.sfree == 0] == 0.0)
    eng.close()


@pytest.mark.parametrize("det", (False, True))
def test_ragged_gp_step_parity(scenes, det):
    """test_gp_step_parity's checks and bounds on the dense ragged scene: 5 LM steps in lockstep (precond 1)."""
    p = scenes("gp")
    eng, ora = GPT.engines(p, precond=1, deterministic=det)
    check_gp_scene(p, eng)
    cg, pg, sg = GPT.dev(p.cams_init), GPT.dev(p.points_init), GPT.dev(p.scales_init)
    co, po, so = p.cams_init.copy(), p.points_init.copy(), p.scales_init.copy()
    for s in range(5):
        lg, st = eng.step(cg, pg, sg)
        lo = ora.step(co, po, so)
        sto = ora.stats()
        assert st["pcg_iters"] == sto["pcg_iters"] and st["trials"] == sto["trials"], (s, st, sto)
        report(f"gp det {det} step {s}", dict(loss=abs(lg - lo) / lo, cams=rel(cg.cpu().numpy(), co), pts=rel(pg.cpu().numpy(), po),
                                    scales=rel(sg.cpu().numpy(), so)), dict(loss=1e-10, cams=1e-9, pts=1e-9, scales=1e-9))
    fixed = p.sfree == 0
    assert np.array_equal(sg.cpu().numpy()[fixed], p.scales_init[fixed])
    empty = int(np.flatnonzero(np.bincount(p.cam_idx, minlength=p.n_cams) == 0)[0])
    assert np.array_equal(co[empty], p.cams_init[empty]) and np.array_equal(cg.cpu().numpy()[empty], p.cams_init[empty])
    eng.close()
