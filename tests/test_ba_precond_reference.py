"""The C oracle's two-level preconditioner and early CG iterates, item by item against the longdouble reference of
tests/ba_precond_reference.py, and the conditions that make that comparison mean something.  CPU only.

What runs between the block factorization and the converged camera step -- coarse_basis, ora_coarse_setup,
coarse_apply_v, adef2_apply and the pipelined recurrence of ora_pcg, which the HIP kernels k_tl_basis,
k_cg_factor_basis, k_tl_erow, k_tl_ereduce, k_tl_pc, k_tl_pc_cl, k_tl_pspmv and k_tl_cgp restate -- was only ever
compared through PCG iteration counts and LM losses, and a converged CG reaches the direct solution with any SPD
preconditioner.  Here an oracle created with pcg_max_iter = k and pcg_tol = 1e-30 hands out x_k, and ora_get hands out
Z~, E and E^-1 (built and used); ba_precond_checks.py names the items, scales, sequences and bounds.

Scenes: `uniform` (24 cameras, 4 clusters of 6) through the four-solve lag sequence, `clamps` models 2 and 4 (2 clusters
of 6, L_i over nine decades) through first solve, retry and lagged solve.  The reference system at the second
linearization point is asserted positive definite.

From the reference alone:
 * the basis fit J_c G + J_p dX = 0 holds to 1e-12 of the sum of |terms| on every camera (measured 3.5e-16 .. 4.5e-16);
 * textbook PCG and the single-reduction recurrence agree to 1e-15 per item wherever M~ is symmetric (additive with any
   E^-1; A-DEF2 on its own E^-1) and at k = 1 everywhere (measured <= 5.5e-16); under A-DEF2 with a lagged E^-1 they
   part from k = 2 on (uniform 3.8e-2 / 1.4e-2, 5.7e-4 / 1.2e-3; clamps 2.0e-3 .. 6.8e-3) and the oracle follows the
   recurrence;
 * the lagged and the own-E^-1 iterates differ by at least 100 bounds (0.087 .. 23 on the item scale, bounds 1e-8);
 * every planted error (a flipped rho part of a rotation column, a cluster-pair segment left out of E, the other
   slot's E^-1 on the lagged solve and on the retry, one camera left out of the prolongation) moves some compared item
   by at least 100 bounds.
Observation: the coarse residual |Z~^T r_0'| / |Z~^T r_0| behind the A-DEF2 start is 1e-18 .. 6e-16 on a solve's own
E^-1 and 1.57 / 0.62 (uniform), 0.62 / 0.65 (clamps 2 / 4) under the lag: A-DEF2 with a lagged E^-1 is no projection.

The oracle against the reference (worst item; x_k over k = 0..3, both preconditioners, every solve of the sequence):

  scene      | x_k     Z~      E       E^-1 vs its own E (bound 8 m eps cond) | E^-1 vs the reference's E
  uniform 2  | 4.1e-10 1.6e-13 6.4e-16 9.5e-11 (8.5e-10)                      | 1.3e-13 .. 1.1e-10
  clamps 2   | 5.0e-10 1.5e-09 4.3e-10 3.7e-15 (8.8e-13)                      | 6.7e-13 .. 1.7e-09
  clamps 4   | 1.3e-09 2.2e-09 1.0e-09 4.3e-15 (2.7e-12)                      | 1.1e-12 .. 4.8e-09

x_k is held to the project's dc tolerance 1e-8 per item, Z~ and E to max(1e-9, 8 x the plain-versus-fma spread) (on
`clamps` at F1 the spread is 2.0e-9 / 1.6e-9, so those items stand at up to 1.6e-8; the oracle's own S~ is 3.6e-11
there, test_gpu_ba_solve.py).  E^-1: the oracle's inversion is held against its OWN E to 8 m eps cond_2 (Gauss-Jordan
elimination, Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 14.4: residual <= 8 n u |L||U||x|
per column, and | |L||U| | ~ |A| on an equilibrated SPD matrix); against the reference's E the distance of the two
E's enters, | I - A_ref X | <= | I - A_own X | + | A_ref - A_own | | X |, and that sum is the bound.
"""
import time

import numpy as np
import pytest

import ba_precond_checks as PC
from gp_reference import LD

SCENES = (("uniform", 2, 6), ("clamps", 2, 6), ("clamps", 4, 6))
MARGIN = 100.0


@pytest.fixture(scope="module", autouse=True)
def host_time():
    t0 = time.perf_counter()
    yield
    print(f"\ntest_ba_precond_reference.py: {time.perf_counter() - t0:.1f} s in all")


def f64(a):
    return np.asarray(a).astype(np.float64)


def gpu_bounds(name, model, cs, precond, k, i):
    own, spr = PC.oracle_figures(name, model, cs, precond, k)[i]
    return PC.bounds(own, spr, PC.reference_sequence(name, model, cs)[i])


@pytest.mark.parametrize("name,model,cs", SCENES)
def test_reference_conditions(name, model, cs):
    """the basis fit, the agreement of the two recurrences where M~ is symmetric, and the distance between the lagged
    and the own-E^-1 iterates, from the reference alone"""
    ref, seq = PC.reference_sequence(name, model, cs, full=True), PC.sequence_of(name)
    lagged = [i for i, u in enumerate(PC.uses(seq)) if u != i]
    assert lagged and any(not fresh for _, _, fresh in seq)
    for i, r in enumerate(ref):
        assert r.fit.max() < 1e-12 and r.einv_resid < 1e-17, (i, r.fit.max(), r.einv_resid)
        for pc in (1, 2):
            agree = [PC.x_errors(f64(r.x_text[pc][k]), r.x[pc][k]).max() for k in PC.KS]
            print(f"{name} {model} solve {i} precond {pc}: textbook vs single-reduction {['%.1e' % v for v in agree]}, "
                  f"coarse residual behind the start {r.coarse[pc]:.2e}")
            sym = pc == 1 or r.symmetric
            assert all(v <= 1e-15 for v in (agree if sym else agree[:2])), (i, pc, agree)
            if not r.symmetric:
                apart = [PC.x_errors(f64(r.x_own[pc][k]), r.x[pc][k]) for k in PC.KS]
                print(f"    own E^-1 vs the lagged one {['%.1e' % v.max() for v in apart]}")
                for k in (PC.KS if pc == 2 else PC.KS[1:]):
                    assert np.max(apart[k] / gpu_bounds(name, model, cs, pc, k, i)["x"]) >= MARGIN, (i, pc, k)
        if r.symmetric:
            assert r.coarse[2] < 1e-12


@pytest.mark.parametrize("precond", [1, 2])
@pytest.mark.parametrize("name,model,cs", SCENES)
def test_oracle_per_item(name, model, cs, precond):
    """Z~ per camera and column, E per cluster-pair block, E^-1 and x_k (k = 0..3) per camera part and intrinsics
    column, after every solve of the sequence"""
    ref = PC.reference_sequence(name, model, cs)
    uses = PC.uses(PC.sequence_of(name))
    for k in PC.KS:
        got, figs = PC.oracle_sequence(name, model, cs, precond, k), PC.oracle_figures(name, model, cs, precond, k)
        for i, (r, g, (own, spr)) in enumerate(zip(ref, got, figs)):
            bnd = PC.oracle_bounds(spr, r)
            # the inversion against the oracle's own E; against the reference's E the two E's distance enters
            d = LD(1) / np.sqrt(np.diagonal(g["E"]).astype(LD))
            A = (g["E"].astype(LD) * d[:, None]) * d[None, :]
            X = (g["Einv"].astype(LD) / d[:, None]) / d[None, :]
            pure = float(np.linalg.norm(f64(np.eye(r.m, dtype=LD) - A @ X), 2))
            apart = float(np.linalg.norm(f64(r.A - A), 2) * np.linalg.norm(f64(X), 2))
            print(f"  E^-1 against its own E {pure:.2e} (bound {8 * bnd['Einv']:.2e}), E's distance x |X| {apart:.2e}")
            assert pure <= 8.0 * bnd["Einv"], (i, pure, bnd["Einv"])
            bnd["Einv"] = 8.0 * bnd["Einv"] + apart
            PC.hold(f"{name} {model} precond {precond} k {k} solve {i}", own, bnd)
            # the lag rule itself: the E^-1 the CG ran with is, bit for bit, the one solve `uses[i]` built
            assert g["Einv_used"].tobytes() == got[uses[i]]["Einv"].tobytes(), i


@pytest.mark.parametrize("name,model,cs", SCENES)
def test_planted_errors_are_seen(name, model, cs):
    """every mutation moves some compared item by at least 100 times the bound the HIP path is held to"""
    ref, seq = PC.reference_sequence(name, model, cs), PC.sequence_of(name)
    uses = PC.uses(seq)
    lab = ref[0].labels
    D = ref[0].Zt.shape[1]

    def worst(errs, i, pc, k):
        bnd = gpu_bounds(name, model, cs, pc, k, i)
        return max(float(np.max(errs[q] / bnd[q])) for q in errs)

    def x_moves(co, i, einv_used=None, mutate=None):
        out = 0.0
        for pc in (1, 2):
            xs = co.iterates(pc, PC.KS[-1], einv_used, mutate=mutate)[0]
            for k in (PC.KS if pc == 2 else PC.KS[1:]):
                out = max(out, worst(dict(x=PC.x_errors(f64(xs[k]), ref[i].x[pc][k])), i, pc, k))
        return out

    tag, f, _ = seq[0]
    # a flipped rho part of one rotation column: Z~ (and with it every iterate)
    co = PC.coarse(name, model, cs, tag, f, ("rho_sign", 3))
    moved = worst(dict(Zt=PC.zt_errors(f64(co.Zt), ref[0].Zt).ravel()), 0, 1, 1)
    print(f"{name} {model} rho_sign: Z~ moves by {moved:.1e} bounds, x_k by {x_moves(co, 0):.1e}")
    assert moved >= MARGIN and x_moves(co, 0) >= MARGIN
    # one row's segment of an off-diagonal cluster pair left out of E
    assert ref[0].nc > 1
    i0, c0 = 0, (lab[0] + 1) % ref[0].nc        # (Coarse asserts that row i0 has a block into cluster c0)
    co = PC.coarse(name, model, cs, tag, f, ("drop_pair", (i0, c0)))
    moved = worst(dict(E=PC.e_errors(f64(co.E), ref[0].E, ref[0].E_abs, D + 1).ravel()), 0, 1, 1)
    print(f"{name} {model} drop_pair ({i0}, cluster {c0}): E moves by {moved:.1e} bounds")
    assert moved >= MARGIN
    # one camera left out of the prolongation
    co = PC.coarse(name, model, cs, tag, f)
    moved = x_moves(co, 0, mutate=("no_prolong", lab.size // 2))
    print(f"{name} {model} no_prolong: x_k moves by {moved:.1e} bounds")
    assert moved >= MARGIN
    # the other slot's E^-1: the lagged solve on its own, the retry on the stale one
    for i, (tag, f, fresh) in enumerate(seq):
        if i == 0:
            continue
        co = PC.coarse(name, model, cs, tag, f)
        wrong = None if uses[i] != i else ref[i - 1].Einv
        moved = x_moves(co, i, wrong)
        print(f"{name} {model} solve {i} on the other slot's E^-1: x_k moves by {moved:.1e} bounds")
        assert moved >= MARGIN
