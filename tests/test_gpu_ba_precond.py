"""The two-level preconditioner and the first CG iterates on the HIP path -- k_tl_basis / k_cg_factor_basis (Z~),
k_tl_erow + k_tl_ereduce (E), the Gauss-Jordan chain behind them (E^-1, per coarse-inverse slot), k_tl_pc / k_tl_pc_cl +
k_tl_pspmv (the launch path's iteration) and k_tl_cgp (paths 1, 2, 4, 5: the in-register coarse solves, the A-DEF2 start,
the segments it writes for the lagged E build) -- item by item against the longdouble reference of
tests/ba_precond_reference.py.  Needs an MI355X.

Every CG path stops with status "done" at it >= maxit and returns its current iterate, so a handle created with
pcg_max_iter = k and pcg_tol = 1e-30 returns x_k as dc; in exact arithmetic x_k is determined by S~, b and M~^-1 alone.
test_gpu_ba_solve.py compares the CONVERGED dc with the direct solution, which any SPD preconditioner reaches; this
file is what sees the preconditioner.  ba_precond_checks.py names the items, scales, sequences and bounds, and
test_ba_precond_reference.py holds the oracle to the same reference and shows, from the reference alone, that every
planted error of the kind this file is for stands at least 100 bounds high.

Cases (one handle per k in 1, 2, 3; k = 0 as well on the A-DEF2 paths 4 and 5, where dc = L^-T Z~ E^-1 Z~^T r0: k_tl_cgp's
setup tags tag0 + maxit + 1 / + 2 stay apart from iteration 0's tag0, the launch advances the tag by maxit + 3, and the
loop leaves at `it >= maxit` before its first exchange; the launch path's hist has maxit + 2 rows):
  dense    models 2, 4 (MC 9, 13), both deterministic values: path 0, effective precond 1; the empty camera 7 is a
           singleton cluster ([I_D | 0], E's unit diagonal entry), asserted from the labels
  banded   model 2, deterministic x precond {1, 2}: k_tl_cgp paths 1, 2, 4, 5, at the default cluster size and at 6:
           33 clusters, m = 297 > 256 (the coarse vector spans several LDS fills per thread), nc (D + 1) <= 768, and
           cluster pairs with no block between them, asserted from the labels and the pattern
  clamps   models 2, 4, cluster size 6: the factors L_i span nine decades (first solve, retry, lagged solve)
  uniform  cluster size 6: the scene of the CPU table
Each handle runs the scene's sequence (linearize at A, solve F1 | linearize at B, solve F1: lagged | solve F2: the
retry | linearize at A, solve F1: reads the retry's slot).  After every solve: debug_solve returned k; dc against the
reference x_k under the E^-1 plan_solve prescribes; Z~ (debug_get 18); the coarse-inverse slot the solve filled
(debug_get 12 / 13) against the reference E^-1 of that system -- on k_tl_cgp the lagged solve's slot is built from the
segments the kernel writes behind the CG, and this is the only per-item check they get; the other slot unchanged bit
for bit.  E itself once per scene (debug_time_kernel(7) rebuilds slot 0's E, debug_get 16).  Deterministic handles:
two runs give the same bytes.

Bounds (ba_precond_checks.bounds; nothing from the HIP path): x_k max(1e-8, 8 x the oracle's own distance from the
reference on that item for the same scene, precond, k and solve); Z~ and E max(1e-9, 8 x the oracle's plain-versus-fma
spread); E^-1 max(8 x the oracle's figure, m eps cond_2 of the equilibrated reference E).

The oracle against the reference on the CPU (worst item over the preconditioners, k and the solves of the sequence):

  scene                    | x_k     Z~      E       E^-1    | coarse residual |Z~^T r0'| / |Z~^T r0| under the lag
  dense 2 / 4              | 1.2e-10 1.1e-13 4.9e-16 1.0e-10 | 1.48, 0.65 / 1.53, 0.66
  banded, cluster size 24  | 1.9e-11 3.1e-13 3.6e-16 4.8e-11 |
  banded, cluster size 6   | 1.5e-10 3.1e-13 2.9e-15 1.1e-10 | 1.59, 0.68
  clamps 2 / 4             | 1.3e-09 2.2e-09 1.0e-09 4.8e-09 | 0.62 / 0.65
  uniform                  | 4.1e-10 1.6e-13 6.4e-16 1.1e-10 | 1.57, 0.62
  (on a solve's own E^-1 the coarse residual is 1e-18 .. 6e-16: A-DEF2 with a lagged E^-1 is no projection, and the
  textbook PCG iterates part from the single-reduction ones there, 4e-4 .. 0.36 at k = 2, 3; the kernels follow the
  recurrence)

Measured on the MI355X (worst item per scene over det, precond, k and the solves; 28 tests, 32 s host time):

  scene                    | x_k     Z~      E       E^-1
  dense 2 / 4              | 1.6e-10 1.4e-13 3.1e-16 1.8e-10
  banded, cluster size 24  | 1.5e-10 8.3e-14 7.2e-17 6.3e-11
  banded, cluster size 6   | 1.8e-10 9.0e-14 1.4e-15 1.2e-10
  clamps 2 / 4             | 3.5e-12 4.1e-12 3.8e-12 9.1e-12
  uniform                  | 4.9e-11 5.3e-14 4.4e-16 1.3e-10

Path codes 0, 1, 2, 4 and 5 were all reached, k = 0 included on 4 and 5.  No x_k item came within 50x of its bound
(1e-8), and on `clamps` the kernels sit two decades below the oracle (as for S~ in test_gpu_ba_solve.py).  What the file
found: nothing -- no defect in the basis, the E build, either coarse-inverse chain, the lag rule's slots, the coarse
corrections or the recurrences on these scenes.
"""
import functools
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no GPU", allow_module_level=True)

import ba_checks as K  # noqa: E402
import ba_edge_scene as E  # noqa: E402
import ba_precond_checks as PC  # noqa: E402
from instantsfm_amd.engine import BundleAdjuster, effective_precond  # noqa: E402
from test_gpu_ba_solve import BANDED_PATH, stop_on_device_error  # noqa: E402
from test_gpu_parity import DEV, dev  # noqa: E402

DEFAULT_CS = 24
# (scene, model, deterministic, precond, cluster size), scene by scene and model by model (the reference is cached)
CASES = ([("dense", m, det, 1, DEFAULT_CS) for m in (2, 4) for det in (False, True)]
         + [("banded", 2, det, pc, cs) for cs in (DEFAULT_CS, 6) for det in (False, True) for pc in (1, 2)]
         + [("clamps", m, det, pc, 6) for m in E.CLAMP_MODELS for det, pc in ((False, 1), (True, 2))]
         + [("uniform", 2, det, pc, 6) for det, pc in ((False, 1), (True, 2))])
SCENES = sorted({(c[0], c[1], c[4]) for c in CASES}, key=[(c[0], c[1], c[4]) for c in CASES].index)
COARSE_MAX = 768
WORST, PATHS = {}, set()


@pytest.fixture(scope="module", autouse=True)
def host_time():
    t0 = time.perf_counter()
    yield
    for name, fig in WORST.items():
        print(f"\n{name} worst per item:", {k: f"{v:.1e}" for k, v in fig.items()})
    print(f"\nCG paths reached: {sorted(PATHS)}")
    print(f"\ntest_gpu_ba_precond.py: {time.perf_counter() - t0:.1f} s host time in all")


def note(name, figures):
    w = WORST.setdefault(name, {})
    for k, v in figures.items():
        w[k] = max(w.get(k, 0.0), float(v))


def engine(name, model, cs, **kw):
    p, s = E.problem(name, model), E.settings(name, model)
    return BundleAdjuster(p.model, p.uv, p.cam_idx, p.pt_idx, p.pp, p.n_cams, p.n_points, device=DEV,
                          **dict(s, cluster_size=cs, **kw))


def check_scene(name, model, cs, eng, det, precond):
    """the CG path the handle runs, and from the labels what the scene is here for"""
    prob, path = E.problem(name, model), eng.cg_info()[0]
    lab, nc = eng.clusters()
    lab_o, nc_o = PC.labels(name, model, cs)
    assert nc == nc_o and np.array_equal(lab, lab_o)
    m = nc * (eng.D + 1)
    assert m <= COARSE_MAX
    sizes = np.bincount(lab, minlength=nc)
    if name == "dense":
        assert path == 0, eng.cg_info()
        empty = np.flatnonzero(np.bincount(prob.cam_idx, minlength=prob.n_cams) == 0)
        assert empty.size == 1 and sizes[lab[empty[0]]] == 1          # the `alone` branch
    elif name == "banded":
        assert path == BANDED_PATH[det, precond], eng.cg_info()
        if cs == 6:
            rp, col = K.pattern(name, model)
            rows = np.repeat(np.arange(prob.n_cams), np.diff(rp))
            linked = np.zeros((nc, nc), dtype=bool)
            linked[lab[rows], lab[col]] = True
            assert m > 256 and not (linked | linked.T).all()          # cluster pairs with no block between them
    PATHS.add(path)
    return path, m


def slots(eng, m):
    return [eng.debug_get(12, (m, m)), eng.debug_get(13, (m, m))]


def run_sequence(name, model, cs, det, precond, k):
    """one handle stopped at iteration k through the scene's sequence: [(dc, Zt, slot bytes before, slots after)]"""
    eng = engine(name, model, cs, deterministic=det, precond=precond, pcg_max_iter=k, pcg_tol=1e-30)
    path, m = check_scene(name, model, cs, eng, det, precond)
    C, D = eng.n_cams, eng.D
    out = []
    for tag, f, fresh in PC.sequence_of(name):
        if fresh:
            eng.debug_linearize(*(dev(a) for a in PC.params(name, model, tag)))
        before = slots(eng, m)
        assert eng.debug_solve(f) == k
        out.append(dict(dc=eng.debug_get(7, (C, D)), Zt=eng.debug_get(18, (C, D, D + 1)), before=before, after=slots(eng, m)))
    eng.close()
    return path, out


@pytest.mark.parametrize("name,model,det,precond,cs", CASES)
@stop_on_device_error
def test_iterates_and_coarse_operators_per_item(name, model, det, precond, cs):
    ref = PC.reference_sequence(name, model, cs)
    seq = PC.sequence_of(name)
    uses, pc = PC.uses(seq), None
    for k in (1, 2, 3, 0):
        if k == 0 and pc != 2:      # the coarse start alone: the A-DEF2 paths (4, 5) only
            break
        path, got = run_sequence(name, model, cs, det, precond, k)
        pc = effective_precond(precond, path)
        assert (pc == 2) == (path in (4, 5))
        check(name, model, cs, det, pc, path, k, ref, uses, got)


def check(name, model, cs, det, pc, path, k, ref, uses, got):
    figs = PC.oracle_figures(name, model, cs, pc, k)
    for i, (r, g, (own, spr)) in enumerate(zip(ref, got, figs)):
        slot = i & 1                                   # solve_policy.h plan_solve: the slot solve i fills
        assert uses[i] == i or (uses[i] & 1) == (slot ^ 1)
        errs = PC.items(dict(dc=g["dc"], Zt=g["Zt"], Einv=g["after"][slot]), r, pc, k)
        note(f"{name} cs {cs}", PC.hold(f"{name} model {model} cs {cs} det {det} precond {pc} path {path} k {k} solve {i} "
                                       f"(oracle x_k {own['x'].max():.1e}, E^-1 {own['Einv'][0]:.1e})",
                                       errs, PC.bounds(own, spr, r)))
        assert g["after"][slot ^ 1].tobytes() == g["before"][slot ^ 1].tobytes(), (i, "the other slot changed")
        assert np.all(np.isfinite(g["after"][slot]))
        empty = np.bincount(E.problem(name, model).cam_idx, minlength=g["dc"].shape[0]) == 0
        assert np.all(g["dc"][empty] == 0.0)


@pytest.mark.parametrize("name,model,cs", SCENES)
@stop_on_device_error
def test_coarse_matrix_per_block(name, model, cs):
    """E before its inversion, per cluster-pair block over the block's sum of |terms|: debug_time_kernel(7) rebuilds
    slot 0's E from the last solve's S~ and Z~ (k_tl_erow + k_tl_ereduce)"""
    r = PC.reference_sequence(name, model, cs)[0]
    _, spr = PC.oracle_figures(name, model, cs, 1, 1)[0]
    tag, f, _ = PC.sequence_of(name)[0]
    eng = engine(name, model, cs, precond=1, pcg_max_iter=1, pcg_tol=1e-30)
    m = eng.clusters()[1] * (eng.D + 1)
    ld = 32 * ((m + 31) // 32)
    eng.debug_linearize(*(dev(a) for a in PC.params(name, model, tag)))
    assert eng.debug_solve(f) == 1
    eng.debug_time_kernel(7, 1)
    Eg = eng.debug_get(16, (ld, ld))[:m, :m]
    eng.close()
    errs = dict(E=PC.e_errors(Eg, r.E, r.E_abs, eng.D + 1).ravel())
    note(f"{name} cs {cs}", PC.hold(f"{name} model {model} cs {cs} E", errs, dict(E=np.maximum(PC.TOL["E"], 8.0 * spr["E"]))))


@pytest.mark.parametrize("name,model,precond,cs", [("banded", 2, 1, 6), ("banded", 2, 2, 6), ("dense", 4, 1, DEFAULT_CS)])
@stop_on_device_error
def test_deterministic_repeat_bitwise(name, model, precond, cs):
    """two deterministic handles stopped at iteration 2: the same bytes for dc, Z~ and every coarse-inverse slot a solve
    has filled (slot 1 is unwritten memory until the second solve), after every solve of the sequence"""
    runs = [run_sequence(name, model, cs, True, precond, 2)[1] for _ in range(2)]
    for i, (a, b) in enumerate(zip(*runs)):
        assert a["dc"].tobytes() == b["dc"].tobytes() and a["Zt"].tobytes() == b["Zt"].tobytes(), i
        for s in ((0,) if i == 0 else (0, 1)):
            assert a["after"][s].tobytes() == b["after"][s].tobytes(), (i, s)
