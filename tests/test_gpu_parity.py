"""HIP path vs the C oracle (oracle/ba_oracle.c) on the same seeded inputs.  Needs an MI355X.

Tolerances: per-kernel 1e-12 relative for residual/Jacobian products, 1e-10 for block sums, PCG solution
1e-8 at equal iteration count, params after one LM step 1e-9, final RMSE |delta| <= 1e-4 px.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

from instantsfm_amd.engine import LM_DEFAULTS, BundleAdjuster, effective_precond  # noqa: E402
from instantsfm_amd.synth import make_config, make_problem  # noqa: E402
from oracle import oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
MODELS = (0, 1, 2, 3, 4, 5, 6, 8, 9)


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def engines(prob, **kw):
    """The GPU engine with the product defaults (engine.LM_DEFAULTS: precond 2, cluster target 24) unless overridden,
    and the oracle running the preconditioner that engine runs (effective_precond: A-DEF2 on the persistent CG, the
    additive form on the launch path)."""
    eng = BundleAdjuster(prob.model, prob.uv, prob.cam_idx, prob.pt_idx, prob.pp, prob.n_cams, prob.n_points, device=DEV,
                         **kw)
    pc = effective_precond(kw.get("precond", LM_DEFAULTS["precond"]), eng.cg_info()[0])
    ora = O.OracleBA(prob.model, prob.uv, prob.cam_idx, prob.pt_idx, prob.pp, prob.n_cams, prob.n_points,
                     optimize_poses=int(kw.get("optimize_poses", True)), precond=pc,
                     cluster_size=kw.get("cluster_size", LM_DEFAULTS["cluster_size"]), **{k: kw[k] for k in (
                         "tr_factor", "pcg_tol", "clamp_min", "clamp_max") if k in kw})
    return eng, ora


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def y_records(ora, pt_idx, f, clamp_min=1e-6, clamp_max=1e32):
    """The oracle's W_o turned into the GPU's stored records Y_o = W_o R_p^-T, R_p = chol(V_p damped by f)."""
    Wo = ora.get(O.W)                        # [N, D, 3]
    Vp = ora.get(O.V)                        # [P, 6] packed (xx xy xz yy yz zz)
    full = np.empty((Vp.shape[0], 3, 3))
    idx = [(0, 0, 0), (1, 0, 1), (2, 0, 2), (3, 1, 1), (4, 1, 2), (5, 2, 2)]
    for k, a, b in idx:
        full[:, a, b] = full[:, b, a] = Vp[:, k]
    for a in range(3):
        full[:, a, a] = np.clip(full[:, a, a], clamp_min, clamp_max) * f
    R = np.linalg.cholesky(full)
    Ri = np.linalg.inv(R)
    return np.einsum("oak,ojk->oaj", Wo, Ri[np.asarray(pt_idx)])


@pytest.mark.parametrize("model", MODELS)
def test_linearize_parity(model):
    prob = make_problem(24, 600, seed=11, model=model)
    eng, ora = engines(prob, deterministic=True)
    eng.debug_linearize(dev(prob.cams_init), dev(prob.points_init))
    ora.linearize(prob.cams_init, prob.points_init)
    N, P, C, D = prob.n_obs, prob.n_points, prob.n_cams, eng.D
    # the stored records are the symmetric Y_o = W_o L_p (PointPrep in csrc/ba_lin.h): L_p = R_p^-T with R_p the
    # Cholesky factor of the point block damped for the first trial (f = 1 + damping = 1 + 1e-4), stored [o][3][D]
    assert rel(eng.debug_get(0, (N, 3, D)).transpose(0, 2, 1), y_records(ora, prob.pt_idx, 1.0 + 1e-4)) < 1e-12
    assert rel(eng.debug_get(1, (P, 6)), ora.get(O.V)) < 1e-12
    assert rel(eng.debug_get(2, (P, 3)), ora.get(O.GP)) < 1e-12
    assert rel(eng.debug_get(3, (C, D, D)), ora.get(O.U)) < 1e-10
    assert rel(eng.debug_get(4, (C, D)), ora.get(O.GC)) < 1e-10


@pytest.mark.parametrize("model", (2, 4, 6))
@pytest.mark.parametrize("deterministic", (True, False))
@pytest.mark.parametrize("precond,cluster", [(0, 32), (1, 32), (1, 6)])
def test_solve_parity(model, deterministic, precond, cluster):
    prob = make_problem(30, 800, seed=5, model=model)
    eng, ora = engines(prob, deterministic=deterministic, precond=precond, cluster_size=cluster)
    eng.debug_linearize(dev(prob.cams_init), dev(prob.points_init))
    ora.linearize(prob.cams_init, prob.points_init)
    f = 1.0 + 1e-4
    it_g = eng.debug_solve(f)
    it_o = ora.solve(f)
    assert it_g == it_o
    C, P, D = prob.n_cams, prob.n_points, eng.D
    nb = eng.nnzb()
    assert nb == ora.nnzb()
    assert rel(eng.debug_get(6, (C, D)), ora.get(O.B)) < 1e-10
    assert rel(eng.debug_get(5, (nb, D, D)), ora.get(O.S)) < 1e-9   # scaled S~ = L^-1 S L^-T
    assert rel(eng.debug_get(7, (C, D)), ora.get(O.DC)) < 1e-8
    assert rel(eng.debug_get(8, (P, 3)), ora.get(O.DP)) < 1e-8


@pytest.mark.parametrize("cfg,steps,precond", [(1, 6, 1), (2, 2, 1), (2, 2, 0)])
def test_step_parity(cfg, steps, precond):
    prob = make_config(cfg)
    eng, ora = engines(prob, precond=precond)
    cg, pg = dev(prob.cams_init), dev(prob.points_init)
    co, po = prob.cams_init.copy(), prob.points_init.copy()
    for s in range(steps):
        lg, st = eng.step(cg, pg)
        lo = ora.step(co, po)
        so = ora.stats()
        assert st["pcg_iters"] == so["pcg_iters"] and st["trials"] == so["trials"], (s, st, so)
        assert abs(lg - lo) / lo < 1e-10, (s, lg, lo)
        assert rel(cg.cpu().numpy(), co) < 1e-9
        assert rel(pg.cpu().numpy(), po) < 1e-9


@pytest.mark.parametrize("cfg", [1, 2])
def test_converged_rmse_matches_oracle(cfg):
    prob = make_config(cfg)
    eng, ora = engines(prob)
    cg, pg = dev(prob.cams_init), dev(prob.points_init)
    hist = []
    for _ in range(200):
        hist.append(eng.step(cg, pg)[0])
        if len(hist) >= 8:
            a, b = np.mean(hist[-4:]), np.mean(hist[-8:-4])
            if abs((b - a) / b) < 5e-4 or hist[-1] == hist[-2]:
                break
    _, rmse_g = eng.cost(cg, pg)
    _, _, hist_o, rmse_o = O.solve_to_convergence(prob)
    assert len(hist) == len(hist_o)
    assert abs(rmse_g - rmse_o) <= 1e-4, (rmse_g, rmse_o)
    # converged to the noise level of the synthetic scene (0.5 px Gaussian + 1% outliers)
    assert rmse_g < 2.5


def test_points_only_mode():
    prob = make_problem(20, 500, seed=2)
    eng, ora = engines(prob, optimize_poses=False)
    cg, pg = dev(prob.cams_init), dev(prob.points_init)
    co, po = prob.cams_init.copy(), prob.points_init.copy()
    for _ in range(3):
        lg, _ = eng.step(cg, pg)
        lo = ora.step(co, po)
        assert abs(lg - lo) / lo < 1e-10
    assert np.array_equal(cg.cpu().numpy(), prob.cams_init)  # cameras frozen
    assert rel(pg.cpu().numpy(), po) < 1e-9


def test_deterministic_mode_bitwise():
    prob = make_config(1, seed=4)
    out = []
    for _ in range(2):
        eng, _ = engines(prob, deterministic=True)
        cg, pg = dev(prob.cams_init), dev(prob.points_init)
        for _ in range(3):
            eng.step(cg, pg)
        out.append((cg.cpu().numpy(), pg.cpu().numpy()))
        eng.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_deterministic_schur_bitwise_config3():
    """Deterministic mode's k_schur on the full config-3 scene (round 6: four waves per row chunk taking their LDS adds
    in turn, several partner rounds per own round): two handles build bitwise the same S and b and solve to bitwise the
    same camera step; S agrees with the atomic (non-deterministic) build to rounding."""
    prob = make_config(3)
    C, D = prob.n_cams, 8
    out = []
    for det in (True, True, False):
        eng = BundleAdjuster(prob.model, prob.uv, prob.cam_idx, prob.pt_idx, prob.pp, prob.n_cams, prob.n_points,
                             device=DEV, deterministic=det)
        eng.debug_linearize(dev(prob.cams_init), dev(prob.points_init))
        eng.debug_solve(1.0 + 1e-4)
        nb = eng.nnzb()
        out.append((eng.debug_get(5, (nb, D, D)), eng.debug_get(6, (C, D)), eng.debug_get(7, (C, D))))
        eng.close()
    (S1, b1, d1), (S2, b2, d2), (S3, b3, _) = out
    assert np.array_equal(S1, S2) and np.array_equal(b1, b2) and np.array_equal(d1, d2)
    assert np.max(np.abs(S1 - S3)) <= 1e-12 * np.max(np.abs(S3))
    assert np.max(np.abs(b1 - b3)) <= 1e-12 * np.max(np.abs(b3))


def test_cost_matches_oracle():
    prob = make_config(1, seed=7)
    eng, ora = engines(prob)
    lg, rg = eng.cost(dev(prob.cams_init), dev(prob.points_init))
    lo, ro = ora.cost(prob.cams_init, prob.points_init)
    assert abs(lg - lo) / lo < 1e-12 and abs(rg - ro) / ro < 1e-12


def test_config3_first_step_and_properties():
    """Full BASELINE size: one LM step vs the oracle plus size-independent properties."""
    prob = make_config(3)
    eng, ora = engines(prob)
    cg, pg = dev(prob.cams_init), dev(prob.points_init)
    l0, _ = eng.cost(cg, pg)
    lg, st = eng.step(cg, pg)
    assert lg < l0 and st["trials"] == 1
    co, po = prob.cams_init.copy(), prob.points_init.copy()
    lo = ora.step(co, po)
    assert abs(lg - lo) / lo < 1e-10
    assert rel(cg.cpu().numpy(), co) < 1e-8
    assert rel(pg.cpu().numpy(), po) < 1e-8


def test_config3_to_convergence_matches_oracle():
    """Full BASELINE size, every LM step to the reference stop rule (bundle_adjustment.py:134-141), GPU vs oracle:
    the same number of steps, per step the same trials and PCG iterations (two-level PCG under the lag rule) and the
    loss to 1e-9; at the stop step the RMSE to 1e-6 px and the parameters to 1e-6 (relative).  The lagged coarse
    inverse is built from the previous S~, whose last bits differ between the GPU's LDS-atomic Schur build and the
    oracle, so the trajectories agree to the CG tolerance's reach, not bitwise.  The additive coarse correction
    (precond 1, the multi-rank launch path's form); the product default is test_config3_product_default_*."""
    prob = make_config(3)
    eng, ora = engines(prob, precond=1)
    cg, pg = dev(prob.cams_init), dev(prob.points_init)
    co, po = prob.cams_init.copy(), prob.points_init.copy()
    hist = []
    for s in range(40):
        lg, st = eng.step(cg, pg)
        lo = ora.step(co, po)
        so = ora.stats()
        assert (st["trials"], st["pcg_iters"]) == (so["trials"], so["pcg_iters"]), (s, st, so)
        assert abs(lg - lo) / lo < 1e-9, (s, lg, lo)
        hist.append(lg)
        if len(hist) >= 8:
            a, b = np.mean(hist[-4:]), np.mean(hist[-8:-4])
            if abs((b - a) / b) < 5e-4 or hist[-1] == hist[-2]:
                break
    assert 5 <= len(hist) < 40, len(hist)
    _, rmse_g = eng.cost(cg, pg)
    _, rmse_o = ora.cost(co, po)
    assert abs(rmse_g - rmse_o) < 1e-6, (rmse_g, rmse_o)
    assert rel(cg.cpu().numpy(), co) < 1e-6
    assert rel(pg.cpu().numpy(), po) < 1e-6


@pytest.mark.parametrize("model", (2, 4))
def test_torchba_solve_end_to_end(model):
    """TorchBA.Solve on scene objects (reference API, bundle_adjustment.py:44-154) vs the oracle LM on the same
    packed problem: same number of LM steps, same written-back points / poses / intrinsics."""
    from instantsfm_amd.config.colmap import BUNDLE_ADJUSTER_OPTIONS
    from instantsfm_amd.processors.bundle_adjustment import TorchBA, pack, _pose_matrices
    from instantsfm_amd.synth import to_scene
    prob = make_problem(24, 1200, seed=13, model=model)
    cameras, images, tracks = to_scene(prob)
    pk = pack(cameras, images, tracks, BUNDLE_ADJUSTER_OPTIONS)
    ba = TorchBA(device="cuda:0")
    ba.Solve(cameras, images, tracks, BUNDLE_ADJUSTER_OPTIONS, progress=False)
    # (the oracle runs the preconditioner the engine ran: A-DEF2 on the D = 8 persistent CG, else the additive form)
    ora = O.OracleBA(pk.model.value, pk.points_2d, pk.camera_indices, pk.point_indices, pk.camera_pps,
                     pk.camera_params.shape[0], pk.points_3d.shape[0], precond=ba.precond_effective)
    c, p = pk.camera_params.copy(), pk.points_3d.copy()
    hist = []
    for _ in range(BUNDLE_ADJUSTER_OPTIONS['max_num_iterations']):
        hist.append(ora.step(c, p))
        if len(hist) >= 8:
            a, b = np.mean(hist[-4:]), np.mean(hist[-8:-4])
            if abs((b - a) / b) < 5e-4 or hist[-1] == hist[-2]:
                break
    assert len(ba.loss_history) == len(hist)
    assert abs(ba.loss_history[-1] - hist[-1]) / hist[-1] < 1e-9
    xyz = np.stack([tracks[pk.track_keys[i]].xyz for i in pk.unique_points])
    assert rel(xyz, p) < 1e-8
    M = _pose_matrices(c[:, :7])
    for i, image_id in enumerate(pk.unique_cameras):
        assert np.max(np.abs(images[image_id].world2cam - M[i])) < 1e-8 * max(1.0, np.max(np.abs(M[i])))
        full = np.asarray(cameras[images[image_id].cam_id].params)
        rest = [k for k in range(full.size) if k not in pk.pp_indices - 7]
        assert rel(full[rest], c[i, 7:]) < 1e-8


@pytest.mark.parametrize("shuffle", (False, True))
def test_clusters_match_oracle(shuffle):
    """The coarse space is the same on both sides: identical camera clusters (greedy co-visibility aggregation)."""
    prob = make_problem(150, 6000, seed=8)
    cam_idx = prob.cam_idx
    if shuffle:
        perm = np.random.default_rng(3).permutation(prob.n_cams).astype(np.int32)
        cam_idx = perm[cam_idx]
    for K in (4, 16, 32):
        eng = BundleAdjuster(prob.model, prob.uv, cam_idx, prob.pt_idx, prob.pp, prob.n_cams, prob.n_points, device=DEV,
                             cluster_size=K)
        ora = O.OracleBA(prob.model, prob.uv, cam_idx, prob.pt_idx, prob.pp, prob.n_cams, prob.n_points, cluster_size=K)
        lg, ng = eng.clusters()
        lo, no = ora.clusters()
        assert ng == no and np.array_equal(lg, lo), K
        eng.close()


def test_two_level_step_with_coarse_active_and_fewer_iterations():
    """Config 2: the coarse correction is active, matches the oracle's iteration counts and needs far fewer CG
    iterations than block-Jacobi for the same stopping rule; both reach the same loss after 4 steps (1e-6)."""
    prob = make_config(2)
    res = {}
    for pc in (0, 1):
        eng, ora = engines(prob, precond=pc)
        cg = dev(prob.cams_init)
        pg = dev(prob.points_init)
        co, po = prob.cams_init.copy(), prob.points_init.copy()
        its = []
        for _ in range(4):
            lg, st = eng.step(cg, pg)
            lo = ora.step(co, po)
            so = ora.stats()
            assert st["pcg_iters"] == so["pcg_iters"], (pc, st, so)
            assert st["coarse_used"] == so["coarse_used"] == pc
            its.append(st["pcg_iters"])
        res[pc] = (lg, sum(its))
    assert res[1][1] * 2 < res[0][1], res
    assert abs(res[1][0] - res[0][0]) / res[0][0] < 1e-6, res


@pytest.mark.parametrize("model,det", [(2, False), (4, False), (6, False), (6, True)])
def test_repeated_solves_lagged_coarse_inverse(model, det):
    """Consecutive solves on one engine under the lag rule: the first solve after a linearization runs with the coarse
    inverse of the previous solve (factorized on the side stream while that CG ran), retries at the same
    linearization use their own.  Every solve matches the oracle's (same rule): iterations, and dc in residual space
    (||S (dc_gpu - dc_oracle)|| / ||b||), energy norm and max-abs.  The coarse sizes here (m = 45 / 65 / 85) end in a
    partial dense block.

    The bound of each solve is derived in the test, not fitted: the oracle is re-run with the Schur row sums taken in
    other orders (order_seed 1..3: each camera row's observations in a seeded permutation; order_mode 2: the PCG's dot
    products in reverse order).  That is a yardstick of the rounding scale of these solves, not a model of the GPU's
    arithmetic: the oracle builds S = U - W V^-1 W^T from W records, while the GPU sums symmetric records
    Y_o = W_o R_p^-T (R_p the Cholesky factor of the first trial's damped point block) and, on retried trials, applies
    M_p = R_p^T V'^-1 R_p -- the same S in exact arithmetic, with other roundings and another summation order.  The GPU
    must stay within 10x the largest spread of those re-runs from the oracle, or within the fixed tolerances below
    where that spread is smaller (resid 1e-9, energy 1e-6, max-abs 1e-8 for own-E solves and 1e-6 for lagged ones),
    and always under the explicit caps resid 1e-7, energy 1e-4, max-abs 1e-3 (the derived bound alone can
    reach ~7e-4 in max-abs for D = 16).  For FULL_OPENCV (D = 16) at k = 0 the distortion columns k1..k3 and k4..k6
    are exactly dependent, held apart only by the damping (cond(S) ~ 5e13): there the order re-runs alone move a lagged
    solve by ~3e-9 in residual space and ~7e-5 in max-abs, which is the bound's scale."""
    prob = make_problem(30, 800, seed=5, model=model)
    cams, pts = prob.cams_init.copy(), prob.points_init.copy()
    args = (prob.model, prob.uv, prob.cam_idx, prob.pt_idx, prob.pp, prob.n_cams, prob.n_points)
    ref = O.OracleBA(*args)
    ref.linearize(cams, pts)
    seq = [(1, 1 + 1e-4), (1, 1 + 5e-5), (1, 1 + 8e-4), (0, 1 + 1.3e-2), (0, 1.2), (1, 1 + 6e-4)]
    # the oracle and its summation-order re-runs on the same sequence: per solve, the spread of the re-runs
    base = O.OracleBA(*args, cluster_size=6, precond=1)
    pert = [O.OracleBA(*args, cluster_size=6, precond=1, order_seed=sd, order_mode=2) for sd in (1, 2, 3)]
    dc_ora, spread = [], []
    for relin, f in seq:
        if relin:
            for o in [base] + pert:
                o.linearize(cams, pts)
        it = base.solve(f)
        assert all(o.solve(f) == it for o in pert)
        S, b = O.dense_reduced(ref, f)
        dref = base.get(O.DC)
        dc_ora.append(dref)
        ds = [O.solve_differences(S, b, o.get(O.DC), dref) for o in pert]
        spread.append({q: max(d[q] for d in ds) for q in ("resid", "energy", "max")})
    for rep in range(3):
        eng, ora = engines(prob, cluster_size=6, deterministic=det, precond=1)
        for k, (relin, f) in enumerate(seq):
            if relin:
                eng.debug_linearize(dev(cams), dev(pts))
                ora.linearize(cams, pts)
            it_g = eng.debug_solve(f)
            it_o = ora.solve(f)
            assert it_g == it_o, (rep, k, it_g, it_o)
            assert np.array_equal(ora.get(O.DC), dc_ora[k])  # (the oracle is deterministic)
            dc_g = eng.debug_get(7, (prob.n_cams, eng.D))
            S, b = O.dense_reduced(ref, f)
            d = O.solve_differences(S, b, dc_g, dc_ora[k])
            lagged = relin and k > 0
            bound = {"resid": max(1e-9, 10 * spread[k]["resid"]), "energy": max(1e-6, 10 * spread[k]["energy"]),
                     "max": max(1e-6 if lagged else 1e-8, 10 * spread[k]["max"])}
            print(f"model {model} det {det} rep {rep} solve {k}: {d}; order spread {spread[k]}")
            cap = {"resid": 1e-7, "energy": 1e-4, "max": 1e-3}
            for q in ("resid", "energy", "max"):
                assert d[q] < bound[q], (rep, k, q, d, spread[k])
                assert d[q] < cap[q], (rep, k, q, d)
        eng.close()


@pytest.mark.parametrize("model", (4, 6))
def test_high_d_models_to_convergence_match_oracle(model):
    """OPENCV (D = 12) and FULL_OPENCV (D = 16) scenes run to the reference stop rule (bundle_adjustment.py:128-150),
    GPU two-level PCG vs the oracle step by step: the same number of LM steps, the same trials per step, the loss per
    step to 1e-8 and the final RMSE to 1e-6 px (the north_star bar is 1e-4 px)."""
    prob = make_problem(200, 20000, seed=7, model=model)
    eng, ora = engines(prob)
    cg, pg = dev(prob.cams_init), dev(prob.points_init)
    co, po = prob.cams_init.copy(), prob.points_init.copy()
    hist = []
    for s in range(60):
        lg, st = eng.step(cg, pg)
        lo = ora.step(co, po)
        so = ora.stats()
        assert st["trials"] == so["trials"], (s, st, so)
        assert abs(lg - lo) / lo < 1e-8, (s, lg, lo)
        hist.append(lg)
        if len(hist) >= 8:
            a, b = np.mean(hist[-4:]), np.mean(hist[-8:-4])
            if abs((b - a) / b) < 5e-4 or hist[-1] == hist[-2]:
                break
    assert 5 <= len(hist) < 60, len(hist)
    _, rmse_g = eng.cost(cg, pg)
    _, rmse_o = ora.cost(co, po)
    print(f"model {model}: {len(hist)} steps, rmse gpu {rmse_g:.12f} oracle {rmse_o:.12f}")
    assert abs(rmse_g - rmse_o) < 1e-6, (rmse_g, rmse_o)
    assert rmse_g < 2.5


def test_two_level_converges_to_the_block_jacobi_oracle_on_config3():
    """The product default (two-level PCG, the build's preconditioner) against the oracle's block-Jacobi PCG(1e-5) --
    the closest restatement of the reference's PCG(tol=1e-5) (bundle_adjustment.py:117) -- on the full config-3 scene,
    each run to the reference stop rule: the same number of LM steps and final RMSE |delta| <= 1e-4 px (north_star);
    in practice they agree to ~1e-8 px."""
    prob = make_config(3)
    eng = BundleAdjuster(prob.model, prob.uv, prob.cam_idx, prob.pt_idx, prob.pp, prob.n_cams, prob.n_points, device=DEV)
    cg, pg = dev(prob.cams_init), dev(prob.points_init)
    hist = []
    for _ in range(200):
        hist.append(eng.step(cg, pg)[0])
        if len(hist) >= 8:
            a, b = np.mean(hist[-4:]), np.mean(hist[-8:-4])
            if abs((b - a) / b) < 5e-4 or hist[-1] == hist[-2]:
                break
    _, rmse_g = eng.cost(cg, pg)
    eng.close()
    _, _, hist_o, rmse_o = O.solve_to_convergence(prob, precond=0)
    print(f"two-level GPU {len(hist)} steps rmse {rmse_g:.10f}; block-Jacobi oracle {len(hist_o)} steps rmse {rmse_o:.10f}")
    assert len(hist) == len(hist_o)
    assert abs(rmse_g - rmse_o) <= 1e-4, (rmse_g, rmse_o)


def _reject_scene(seed, frac):
    """A config-1-sized scene whose LM takes rejected trials: a fraction of the initial points moved by N(0, 10^2)
    (the oracle's reject counts: seed 21 / 5 % -> steps 5 and 6 reject 2 and 1 trials; seed 23 / 20 % rejects one
    trial at steps 4, 5, 7 and 11, but its conditioning puts GPU and oracle ~4e-9 apart in loss, so it only checks the
    tr_factor knob below)."""
    prob = make_problem(24, 600, seed=seed)
    rng = np.random.default_rng(seed)
    p0 = prob.points_init.copy()
    idx = rng.random(p0.shape[0]) < frac
    p0[idx] += rng.normal(0, 10.0, (int(idx.sum()), 3))
    return prob, p0


@pytest.mark.parametrize("seed,frac,tr_factor,precond", [(21, 0.05, 0.5, 1), (21, 0.05, 0.25, 1), (21, 0.05, 0.25, 2)])
def test_reject_path_parity(seed, frac, tr_factor, precond):
    """BA steps that reject trials (LM reject loop, bundle_adjustment.py:119 reject=30), step by step vs the oracle:
    trials, rejects, damping, loss and the in-place-updated caller buffers (the step reads them as the linearization
    point, retries from them unchanged after a reject and copies the accepted trial back) to 1e-9.  tr_factor (the
    TrustRegion down-multiplier's shrink per consecutive failure) is passed through to both."""
    prob, p0 = _reject_scene(seed, frac)
    # the displaced points make the normal equations ill-conditioned: at the reference's PCG tolerance (1e-5) the
    # iterate carries rounding differences of ~1e-8 into the loss, so the solves run to 1e-9 here (tighter ones
    # reach the rounding floor near convergence and break down on one side or the other) and the comparison
    # is one of the LM logic (reject / retry / copy-back), not of PCG rounding (the reject pattern is the same).
    # precond 2: the A-DEF2 k_tl_cgp with lagged coarse inverses and retries that factor their own
    eng, ora = engines(prob, tr_factor=tr_factor, pcg_tol=1e-9, precond=precond)
    assert eng.cg_info()[0] == (4 if precond == 2 else 1), eng.cg_info()
    cg, pg = dev(prob.cams_init), dev(p0)
    co, po = prob.cams_init.copy(), p0.copy()
    total_rej, multi = 0, 0
    for s in range(12):
        lg, st = eng.step(cg, pg)
        lo = ora.step(co, po)
        so = ora.stats()
        assert (st["trials"], st["rejects"], st["failed"]) == (so["trials"], so["rejects"], so["failed"]), (s, st, so)
        assert abs(st["damping"] - so["damping"]) <= 1e-9 * so["damping"], (s, st, so)
        assert abs(lg - lo) <= 1e-9 * lo, (s, lg, lo)
        assert rel(cg.cpu().numpy(), co) < 1e-9, s
        assert rel(pg.cpu().numpy(), po) < 1e-9, s
        total_rej += st["rejects"]
        multi += st["rejects"] > 0
    assert total_rej > 0 and multi > 0


def test_reject_path_tr_factor_changes_damping():
    """The tr_factor knob is live: with two consecutive rejects (seed 21, step 5), 0.5 and 0.25 give different damping
    sequences (oracle and GPU alike, see test_reject_path_parity)."""
    prob, p0 = _reject_scene(21, 0.05)
    damp = {}
    for trf in (0.5, 0.25):
        ora = O.OracleBA(prob.model, prob.uv, prob.cam_idx, prob.pt_idx, prob.pp, prob.n_cams, prob.n_points,
                         tr_factor=trf)
        c, p = prob.cams_init.copy(), p0.copy()
        damp[trf] = []
        for _ in range(15):
            ora.step(c, p)
            damp[trf].append(ora.stats()["damping"])
    assert damp[0.5] != damp[0.25]


def test_solver_failure_leaves_caller_buffers_unchanged():
    """A trial whose damped point blocks are not positive definite (forced here with an out-of-range diagonal clamp,
    clamp_min = clamp_max = -1) fails the step: the LM reports solver_failed, returns the previous loss and leaves the
    caller's parameter buffers bit-for-bit unchanged -- like the oracle (and the LM's "Linear solver failed. Breaking
    optimization step...")."""
    prob = make_problem(20, 400, seed=2)
    eng, _ = engines(prob, clamp_min=-1.0, clamp_max=-1.0)
    ora = O.OracleBA(prob.model, prob.uv, prob.cam_idx, prob.pt_idx, prob.pp, prob.n_cams, prob.n_points,
                     clamp_min=-1.0, clamp_max=-1.0)
    cg, pg = dev(prob.cams_init), dev(prob.points_init)
    l0, _ = eng.cost(cg, pg)
    lg, st = eng.step(cg, pg)
    assert st["failed"] == 1 and lg == l0, st
    assert np.array_equal(cg.cpu().numpy(), prob.cams_init) and np.array_equal(pg.cpu().numpy(), prob.points_init)
    co, po = prob.cams_init.copy(), prob.points_init.copy()
    lo = ora.step(co, po)
    assert ora.stats()["failed"] == 1 and abs(lo - l0) <= 1e-12 * l0
    assert np.array_equal(co, prob.cams_init) and np.array_equal(po, prob.points_init)


def _spd(m, seed, cond_exp=4.0):
    """B B^T + 1e-3 m I with rows / columns scaled over cond_exp decades (the coarse matrix's wide diagonal)."""
    rng = np.random.default_rng(seed)
    B = rng.normal(size=(m, m))
    sc = 10.0 ** (cond_exp * np.arange(m) / max(1, m - 1))
    return (B @ B.T + 1e-3 * m * np.eye(m)) * sc[:, None] * sc[None, :], sc


@pytest.mark.parametrize("m", [1, 5, 32, 33, 279, 567, 747, 768])
def test_coarse_inverse_matches_numpy(m):
    """The two-level preconditioner's E^-1 (blocked Gauss-Jordan, f64 MFMA; k_gj_pivot / k_gj_update) vs numpy's
    inverse, in the scale-free metric max |D^-1 (E X - I) D|, and a non-positive-definite matrix is reported."""
    import ctypes
    from instantsfm_amd import _capi
    L = _capi.load()
    E, sc = _spd(m, seed=m)
    Ed = dev(E)
    Xd = torch.empty_like(Ed)
    us = ctypes.c_double()
    rc = L.insfm_ba_debug_spd_inverse(m, ctypes.c_void_p(Ed.data_ptr()), ctypes.c_void_p(Xd.data_ptr()), None, 5,
                                      ctypes.byref(us))
    assert rc == 1
    X = Xd.cpu().numpy()
    res = (E @ X - np.eye(m)) * sc[None, :] / sc[:, None]
    assert np.abs(res).max() < 1e-9, np.abs(res).max()
    ref = np.linalg.inv(E)
    assert np.abs((X - ref) * sc[:, None] * sc[None, :]).max() < 1e-8
    # the oracle runs the same steps, pivots and fused multiply-adds
    Xo, oko = O.spd_inverse(E)
    assert oko
    dev_o = np.abs((X - Xo) * sc[:, None] * sc[None, :]).max()
    print(f"m={m}: {us.value:.1f} us per inverse; vs oracle: bitwise {np.array_equal(X, Xo)}, max scaled diff {dev_o:.2e}")
    assert np.array_equal(X, Xo)  # same steps, pivots and fused multiply-adds: bitwise
    if m > 1:
        En = E.copy()
        En[m // 2, m // 2] = -abs(En[m // 2, m // 2])   # not positive definite
        rc = L.insfm_ba_debug_spd_inverse(m, ctypes.c_void_p(dev(En).data_ptr()), ctypes.c_void_p(Xd.data_ptr()),
                                          None, 0, None)
        assert rc == 0


@pytest.mark.timeout(300)
def test_device_block_pattern_matches_host_pass():
    """insfm_ba_create derives the Schur block pattern and the co-visibility graph on the device (k_pattern) on a
    single rank; the host pass (multi-rank, INSFM_DIAG=pattern_host) must give the same result: the same block count,
    the same two-level clusters (which read the graph's weights) and bitwise the same deterministic LM steps, on
    config 2, a scene with duplicated observations, one with a camera that sees nothing and the 24-camera scene of the
    multi-rank tests (tools/dist_check.py --small: one coarse cluster at the default target)."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for diag in ("", "pattern_host"):
        p = subprocess.run([sys.executable, os.path.join(repo, "tools", "pattern_check.py")], capture_output=True,
                           text=True, timeout=140, env=dict(os.environ, INSFM_DIAG=diag), cwd=repo)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        outs.append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]))
    assert outs[0]["env"] == "" and outs[1]["env"] == "pattern_host"
    assert outs[0]["scenes"] == outs[1]["scenes"]
    assert set(outs[0]["scenes"]) == {"config2", "duplicates", "empty_camera", "dist_small"}
    assert outs[0]["scenes"]["dist_small"]["nc"] == 1  # (the default target makes the 24-camera scene one cluster)


@pytest.mark.parametrize("K", (2, 3))
def test_clusters_match_oracle_when_the_cap_grows_the_target(K):
    """FULL_OPENCV (D = 16, 17 coarse columns per cluster) on 150 cameras: a target of K = 2 or 3 gives more than
    768 / 17 clusters, so both sides grow the target in proportion to the excess (rounded up to even) and must arrive
    at the same clusters, within the cap."""
    prob = make_problem(150, 6000, seed=8, model=6)
    eng = BundleAdjuster(prob.model, prob.uv, prob.cam_idx, prob.pt_idx, prob.pp, prob.n_cams, prob.n_points, device=DEV,
                         cluster_size=K)
    ora = O.OracleBA(prob.model, prob.uv, prob.cam_idx, prob.pt_idx, prob.pp, prob.n_cams, prob.n_points, cluster_size=K)
    lg, ng = eng.clusters()
    lo, no = ora.clusters()
    assert ng == no and np.array_equal(lg, lo)
    assert ng * 17 <= 768 and np.bincount(lo).min() >= 2
    eng.close()


@pytest.mark.parametrize("cfg,steps", [(2, 4), (3, 10)])
def test_adef2_coarse_correction_matches_oracle(cfg, steps):
    """precond 2 at the default cluster target (24): k_tl_cgp applies the coarse correction as A-DEF2 (M~^-1 r = r +
    Z~ E^-1 Z~^T (r - S~ r), started from the coarse solution x0 = Z~ E^-1 Z~^T r0; oracle/ba_oracle.c adef2_apply)
    against the oracle's precond 2: PCG iterations per step within one (the k_tl_cgp form sums S~ x, S~ Z~ y and the
    restrictions in another order), losses 1e-8 relative; and at most 0.6x the iterations of the additive form
    (precond 1) at the same target on the same steps (config 3, round 5: 128 against ~280 over 10 steps)."""
    prob = make_config(cfg)
    eng, ora = engines(prob, precond=2)
    assert eng.cg_info()[0] == 4, eng.cg_info()  # the A-DEF2 k_tl_cgp ran
    add = BundleAdjuster(prob.model, prob.uv, prob.cam_idx, prob.pt_idx, prob.pp, prob.n_cams, prob.n_points, device=DEV,
                         precond=1)
    cg, pg = dev(prob.cams_init), dev(prob.points_init)
    ca, pa = dev(prob.cams_init), dev(prob.points_init)
    co, po = prob.cams_init.copy(), prob.points_init.copy()
    it_g, it_o, it_a = [], [], []
    for s in range(steps):
        lg, st = eng.step(cg, pg)
        lo = ora.step(co, po)
        so = ora.stats()
        it_a.append(add.step(ca, pa)[1]["pcg_iters"])
        it_g.append(st["pcg_iters"])
        it_o.append(so["pcg_iters"])
        assert st["trials"] == so["trials"] and abs(st["pcg_iters"] - so["pcg_iters"]) <= 1, (s, st, so)
        assert abs(lg - lo) / lo < 1e-8, (s, lg, lo)
    assert rel(cg.cpu().numpy(), co) < 1e-7
    print(f"config {cfg}: A-DEF2 GPU {it_g} (sum {sum(it_g)}), oracle {it_o} (sum {sum(it_o)}), additive GPU {it_a} "
          f"(sum {sum(it_a)})")
    assert sum(it_g) <= 0.6 * sum(it_a), (it_g, it_a)


def _stop(hist):
    """TorchBA.Solve's stop rule (bundle_adjustment.py:134-141) on a loss history."""
    if len(hist) >= 8:
        a, b = np.mean(hist[-4:]), np.mean(hist[-8:-4])
        return abs((b - a) / b) < 5e-4 or hist[-1] == hist[-2]
    return False


@pytest.fixture(scope="module")
def config3_adef2_oracle():
    """The oracle's precond-2 (A-DEF2, cluster target 24) LM on config 3 to the reference stop rule: per step (loss,
    trials, PCG iterations), the final RMSE and parameters -- shared by the product-default tests below."""
    prob = make_config(3)
    ora = O.OracleBA(prob.model, prob.uv, prob.cam_idx, prob.pt_idx, prob.pp, prob.n_cams, prob.n_points, precond=2,
                     cluster_size=24)
    co, po = prob.cams_init.copy(), prob.points_init.copy()
    traj, hist = [], []
    for _ in range(40):
        lo = ora.step(co, po)
        so = ora.stats()
        traj.append((lo, so["trials"], so["pcg_iters"]))
        hist.append(lo)
        if _stop(hist):
            break
    return prob, traj, ora.cost(co, po)[1], co, po


@pytest.mark.parametrize("det", (False, True))
def test_config3_product_default_to_convergence_matches_oracle(config3_adef2_oracle, det):
    """the configuration TorchBA.Solve and bench.py run (precond 2, cluster target 24) on the full
    config-3 scene against the oracle's precond 2, every LM step to the reference stop rule: the same step count (the
    GPU's own stop rule fires at the oracle's step), per step the same trials, PCG iterations within one and the loss
    to 1e-8; at the stop step the RMSE to 1e-6 px and the parameters to 1e-6.  det: deterministic mode, i.e. the
    fixed-order A-DEF2 k_tl_cgp (path 5) that every rank of a multi-rank run uses."""
    prob, traj, rmse_o, co, po = config3_adef2_oracle
    eng = BundleAdjuster(prob.model, prob.uv, prob.cam_idx, prob.pt_idx, prob.pp, prob.n_cams, prob.n_points, device=DEV,
                         deterministic=det)
    assert eng.cg_info()[0] == (5 if det else 4), eng.cg_info()
    cg, pg = dev(prob.cams_init), dev(prob.points_init)
    hist, its = [], []
    for s, (lo, tro, ito) in enumerate(traj):
        assert not _stop(hist), s  # (the GPU's stop rule has not fired before the oracle's)
        lg, st = eng.step(cg, pg)
        hist.append(lg)
        its.append((st["pcg_iters"], ito))
        assert st["trials"] == tro and abs(st["pcg_iters"] - ito) <= 1, (s, st, ito)
        assert abs(lg - lo) / lo < 1e-8, (s, lg, lo)
    assert _stop(hist) and 5 <= len(hist) < 40, len(hist)
    _, rmse_g = eng.cost(cg, pg)
    print(f"det {det}: {len(hist)} steps, PCG (gpu, oracle) {its}, rmse gpu {rmse_g:.12f} oracle {rmse_o:.12f}")
    assert abs(rmse_g - rmse_o) < 1e-6, (rmse_g, rmse_o)
    assert rel(cg.cpu().numpy(), co) < 1e-6
    assert rel(pg.cpu().numpy(), po) < 1e-6


@pytest.mark.timeout(300)
def test_adef2_breakdown_falls_back_to_additive():
    """an A-DEF2 solve that breaks down (k_tl_cgp status 2; forced by INSFM_DIAG=adef2_breakdown on the
    first A-DEF2 launch of the process) is repeated with the additive coarse correction instead of failing the step.
    tools/adef2_fallback_check.py steps config 2 three times with the fault and, after it, three times on a fresh
    handle without: the faulted step does not fail, its solve matches the oracle's additive (precond 1) solve of the
    first step (same iterations, loss 1e-10), and the run stays within 1e-6 of the unfaulted one."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(repo, "tools", "adef2_fallback_check.py")], capture_output=True,
                       text=True, timeout=280, env=dict(os.environ, INSFM_DIAG="adef2_breakdown"), cwd=repo)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert "A-DEF2 PCG breakdown at iteration 2" in p.stderr, p.stderr[-2000:]
    assert out["cg_path"] == 4 and out["fallbacks"] == [1, 0], out
    assert not any(out["failed"]) and not any(out["failed_ref"]), out
    prob = make_config(2)
    ora = O.OracleBA(prob.model, prob.uv, prob.cam_idx, prob.pt_idx, prob.pp, prob.n_cams, prob.n_points, precond=1)
    co, po = prob.cams_init.copy(), prob.points_init.copy()
    lo = ora.step(co, po)
    assert out["iters"][0] == ora.stats()["pcg_iters"], (out, ora.stats())
    assert abs(out["losses"][0] - lo) / lo < 1e-10, (out["losses"][0], lo)
    for a, b in zip(out["losses"], out["losses_ref"]):
        assert abs(a - b) / b < 1e-6, (out["losses"], out["losses_ref"])
