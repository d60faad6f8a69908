"""The per-item comparison of one implementation's two-level preconditioner and early CG iterates (the C oracle or the
HIP path) with tests/ba_precond_reference.py, shared by test_ba_precond_reference.py and test_gpu_ba_precond.py.  Test
helper only.

The hook: every CG path stops with status "done" at it >= maxit and returns its current iterate, so a solver created
with pcg_max_iter = k and pcg_tol = 1e-30 returns x_k as dc.  In exact arithmetic x_k is determined by S~, b and M~^-1
alone, so a longdouble CG with its own M~^-1 checks basis, E, E^-1, restriction, prolongation, coarse start and
recurrence together.

A sequence is a list of solves (point, f, fresh): `fresh` = the first solve after a linearization, which under the lag
rule (solve_policy.h plan_solve, ora_pcg) runs on the E^-1 the PREVIOUS solve built; every other solve runs on its own.
  LAG     linearize at A, solve F1 (own E) | linearize at B, solve F1 (lagged: A's E^-1) | solve F2 (the retry, own E) |
          linearize at A again, solve F1 (lagged: reads the retry's slot)
  RETRY   linearize at A, solve F1 | solve F2 | linearize at A again, solve F1 (lagged on the retry's E^-1)
B is the point one oracle LM step from A.  `clamps` runs RETRY: its clamp_max is tuned to the initial point and the
reference system at B is not positive definite there.

Items and scales (errors are max |got - ref| over the item, over the scale):
  Z~     per camera and column      the column's largest reference entry in that camera; a zero column must be exact
  E      per cluster-pair block     the block's largest sum of |terms|; a block without terms must be exactly 0
  E^-1   one figure                 || I - A_ref X ||_2 with A_ref the reference's equilibrated E, X the E^-1 taken to
                                    that scale
  x_k    per camera translation part, rotation part, and per intrinsics column over all cameras (ba_checks' dc norm
         with the reference iterate in place of the direct solution)
Bounds, none from the HIP path:
  x_k    max(1e-8, 8 x the oracle's own distance from the reference on that item: same scene, precond, k, solve)
  Z~, E  max(1e-9, 8 x the oracle's plain-versus-fma spread on that item): the rule and floor of S~
  E^-1   max(8 x the oracle's figure, m eps cond_2(A_ref)): Gauss-Jordan without pivoting on an equilibrated SPD matrix
         (the bound argued in test_gpu_rotavg.py)
"""
import numpy as np

import ba_checks as K
import ba_edge_scene as E
import ba_precond_reference as PR
from gp_reference import LD
from oracle import oracle as O

LAG = (("A", E.F1, True), ("B", E.F1, True), ("B", E.F2, False), ("A", E.F1, True))
RETRY = (("A", E.F1, True), ("A", E.F2, False), ("A", E.F1, True))
KS = (0, 1, 2, 3)
TOL = dict(x=K.TOL["dc"], Zt=K.TOL["St"], E=K.TOL["St"])
EPS = float(np.finfo(np.float64).eps)
_cache = {}


def sequence_of(name):
    return RETRY if name == "clamps" else LAG


def point(name, model, tag):
    """None for A (the scene's initial parameters); ("B", cams, pts) one oracle LM step from A (cached)"""
    if tag == "A":
        return None
    key = ("B", name, model)
    if key not in _cache:
        p = E.problem(name, model)
        cams, pts = p.cams_init.copy(), p.points_init.copy()
        ora = K.oracle_for(name, model)
        ora.step(cams, pts)
        assert ora.stats()["failed"] == 0 and not np.array_equal(cams, p.cams_init)
        _cache[key] = ("B", cams, pts)
    return _cache[key]


def params(name, model, tag):
    p, pt = E.problem(name, model), point(name, model, tag)
    return (p.cams_init, p.points_init) if pt is None else pt[1:]


def labels(name, model, cluster_size):
    key = ("labels", name, model, cluster_size)
    if key not in _cache:
        _cache[key] = K.oracle_for(name, model, cluster_size=cluster_size, precond=1).clusters()
    return _cache[key]


def uses(seq):
    """per solve, the index of the solve whose E^-1 its CG runs on (the lag rule)"""
    return [i - 1 if (fresh and i > 0) else i for i, (_, _, fresh) in enumerate(seq)]


# ------------------------------------------------------------------------------------------------------------
# the reference along a sequence
# ------------------------------------------------------------------------------------------------------------
class Solve:
    """What the reference keeps of one solve of a sequence (the dense S~ is dropped): Zt, E, E_abs, Einv (its own),
    d, A, cond, m, einv_resid, fit, spd; x[precond] [4,C,D] the iterates on the E^-1 the lag rule prescribes (single-
    reduction recurrence), x_text[precond] the same by textbook PCG, x_own[precond] on the solve's own E^-1,
    coarse[precond] the coarse residual behind the start, symmetric = the solve runs on its own E^-1"""
    einv_distance = PR.Coarse.einv_distance


def coarse(name, model, cluster_size, tag, f, mutate=None):
    """the (heavy, uncached) Coarse of one system"""
    sys_ = E.system(name, model, f, point=point(name, model, tag))
    assert sys_.spd, (name, model, tag, f)
    return PR.Coarse(sys_, params(name, model, tag)[1], labels(name, model, cluster_size)[0], mutate)


def keep(co, einv_used, own, full):
    s = Solve()
    for k in ("Zt", "E", "E_abs", "Einv", "d", "A", "cond", "m", "einv_resid", "fit", "labels", "nc"):
        setattr(s, k, getattr(co, k))
    s.symmetric = own
    s.x, s.x_text, s.x_own, s.coarse = {}, {}, {}, {}
    for pc in (1, 2):
        s.x[pc], s.coarse[pc] = co.iterates(pc, KS[-1], einv_used)
        if full:
            s.x_text[pc] = co.iterates(pc, KS[-1], einv_used, recurrence="textbook")[0]
            s.x_own[pc] = s.x[pc] if own else co.iterates(pc, KS[-1])[0]
    return s


def reference_sequence(name, model, cluster_size, full=False):
    """[Solve] along the scene's sequence (cached per scene, model and cluster size; both preconditioners).  full: also
    the textbook iterates and, for a lagged solve, the iterates on its own E^-1 (the CPU tests' conditions)"""
    key = ("seq", name, model, cluster_size)
    if key not in _cache or (full and not _cache[key][0].x_text):
        seq, out = sequence_of(name), []
        first = None        # the sequence comes back to its first system: its Coarse is kept until then
        for i, ((tag, f, _), use) in enumerate(zip(seq, uses(seq))):
            again = i > 0 and (tag, f) == seq[0][:2]
            co = first if again else coarse(name, model, cluster_size, tag, f)
            first = co if i == 0 else first
            out.append(keep(co, None if use == i else out[use].Einv, use == i, full))
            del co
        _cache[key] = out
    return _cache[key]


# ------------------------------------------------------------------------------------------------------------
# items
# ------------------------------------------------------------------------------------------------------------
def _rel(err, scale):
    return np.where(scale > 0, err / np.where(scale > 0, scale, 1), np.where(err == 0, 0.0, np.inf)).astype(np.float64)


def zt_errors(got, ref):
    """[C, MC]: per camera and column"""
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref).max(axis=1)
    return _rel(err, np.abs(ref).max(axis=1))


def e_errors(got, ref, ref_abs, MC):
    """[nc, nc]: per cluster-pair block"""
    nc = ref.shape[0] // MC
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref).reshape(nc, MC, nc, MC).max(axis=(1, 3))
    return _rel(err, ref_abs.reshape(nc, MC, nc, MC).max(axis=(1, 3)))


def x_errors(got, ref):
    """[2 C + D - 6]: per camera translation part, rotation part; per intrinsics column"""
    got = np.asarray(got, dtype=np.float64)
    if not np.all(np.isfinite(got)):
        return np.full(2 * ref.shape[0] + ref.shape[1] - 6, np.inf)
    err, a = np.abs(got.astype(LD) - ref), np.abs(ref)
    return np.concatenate([_rel(err[:, 0:3].max(axis=1), a[:, 0:3].max(axis=1)),
                           _rel(err[:, 3:6].max(axis=1), a[:, 3:6].max(axis=1)),
                           _rel(err[:, 6:].max(axis=0), a[:, 6:].max(axis=0))])


def items(got, ref, precond, k):
    """name -> per-item errors of one implementation's solve `got` (dict with any of dc, Zt, E, Einv) against the
    reference Solve `ref`; dc is x_k of `precond`"""
    out = {}
    if "dc" in got:
        out["x"] = x_errors(got["dc"], ref.x[precond][k])
    if "Zt" in got:
        out["Zt"] = zt_errors(got["Zt"], ref.Zt).ravel()
    if "E" in got:
        out["E"] = e_errors(got["E"], ref.E, ref.E_abs, ref.Zt.shape[2]).ravel()
    if "Einv" in got:
        out["Einv"] = np.array([ref.einv_distance(got["Einv"])])
    return out


def hold(tag, errs, bnd):
    """print the worst figure of every quantity, then hold every item to its bound"""
    worst = {k: float(np.max(v)) for k, v in errs.items()}
    print(tag, {k: f"{v:.2e}" for k, v in worst.items()},
          "widest bound", {k: f"{float(np.max(bnd[k])):.1e}" for k in errs})
    for k in errs:
        bad = np.flatnonzero(~(errs[k] <= bnd[k]))
        assert bad.size == 0, (tag, k, bad[:8], errs[k][bad[:8]], np.broadcast_to(bnd[k], errs[k].shape)[bad[:8]])
    return worst


# ------------------------------------------------------------------------------------------------------------
# the oracle along a sequence
# ------------------------------------------------------------------------------------------------------------
def oracle_sequence(name, model, cluster_size, precond, k, variant=""):
    """[dict(dc, Zt, E, Einv, Einv_used)] per solve of the scene's sequence from one oracle stopped at iteration k"""
    key = ("ora", name, model, cluster_size, precond, k, variant)
    if key not in _cache:
        ora = K.oracle_for(name, model, variant, cluster_size=cluster_size, precond=precond, pcg_max_iter=k, pcg_tol=1e-30)
        out = []
        for tag, f, fresh in sequence_of(name):
            if fresh:
                ora.linearize(*params(name, model, tag))
            assert ora.solve(f) == k
            out.append(dict(dc=ora.get(O.DC), Zt=ora.get(O.ZT), E=ora.get(O.E), Einv=ora.get(O.EINV_BUILT),
                            Einv_used=ora.get(O.EINV_USED)))
        _cache[key] = out
    return _cache[key]


def oracle_figures(name, model, cluster_size, precond, k):
    """per solve: (the oracle's own per-item errors against the reference, the per-item plain-versus-fma spread of Z~
    and E) -- what bounds() is made of (cached)"""
    key = ("fig", name, model, cluster_size, precond, k)
    if key not in _cache:
        ref = reference_sequence(name, model, cluster_size)
        plain = oracle_sequence(name, model, cluster_size, precond, k)
        fma = oracle_sequence(name, model, cluster_size, precond, k, "fma")
        out = []
        for r, a, b in zip(ref, plain, fma):
            own = items(a, r, precond, k)
            MC = r.Zt.shape[2]
            spr = dict(Zt=_rel(np.abs(a["Zt"] - b["Zt"]).max(axis=1), np.abs(r.Zt).max(axis=1).astype(np.float64)).ravel(),
                       E=e_errors(b["E"], a["E"].astype(LD), r.E_abs, MC).ravel())
            out.append((own, spr))
        _cache[key] = out
    return _cache[key]


def einv_floor(ref):
    return ref.m * EPS * ref.cond


def bounds(own, spr, ref):
    """per-item bounds of one solve for the HIP path, from the oracle's figures and the number formats alone"""
    return dict(x=np.maximum(TOL["x"], 8.0 * own["x"]), Zt=np.maximum(TOL["Zt"], 8.0 * spr["Zt"]),
                E=np.maximum(TOL["E"], 8.0 * spr["E"]), Einv=np.maximum(8.0 * own["Einv"], einv_floor(ref)))


def oracle_bounds(spr, ref):
    """what the oracle itself is held to: the project's tolerances, the spread rule for Z~ and E, the Gauss-Jordan
    bound for E^-1"""
    return dict(x=np.float64(TOL["x"]), Zt=np.maximum(TOL["Zt"], 8.0 * spr["Zt"]), E=np.maximum(TOL["E"], 8.0 * spr["E"]),
                Einv=np.float64(einv_floor(ref)))
