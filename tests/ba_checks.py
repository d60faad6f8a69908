"""The per-item comparison of one implementation's BA Schur build and solve (the C oracle or the HIP path) with
tests/ba_solve_reference.py, shared by test_ba_solve_reference.py and test_gpu_ba_solve.py.  Test helper only.

An implementation hands over `got` (float64): Y [N,D,3] the stored records for the first trial's f, V [P,6] and
gp [P,3], U [C,D,D] and gc [C,D] (all undamped, as the linearization leaves them), b [C,D], St [nnzb,D,D] the
block-Jacobi scaled S~ in the order of the upper block pattern, dc [C,D], dp [P,3]; any subset.

Per item, on the item's own scale (errors()):
  Y, V     per track     the track's largest reference entry
  gp, dp   per track     the largest entry of the reference's sum of |terms|
  U        per camera    entry (a, b) over sqrt(max|U_aa| max|U_bb|), ba_reference.urel's scale
  gc, b    per entry     the entry's sum of |terms| (a focal entry of b is held to its own size)
  St       per block     the largest entry of |L_i^-1| S_abs_ij |L_j^-T|
  dc       per camera    translation part and rotation part separately, each over its largest reference entry; then
           per intrinsics column over all cameras, over the column's largest reference entry (ba_reference.colrel)
An entry whose scale is 0 must be exact (the empty camera's b and dc, a column the model ignores).

Bounds (bounds()): the project's tolerances: records, V, g_p 1e-12; U, g_c, b 1e-10; S~ 1e-9; dc, dp
1e-8 -- per item max(tolerance, 8 x the oracle's plain-versus-fma spread on that item in the same norm), as
gp_checks.bounds.  dc is compared with the reference's DIRECT solution at pcg_tol 1e-12; how far a converged PCG stays
from it depends on the conditioning of S~, so its item bound is max(1e-8, 8 x the oracle's own distance on that item
for the same scene, preconditioner and f), measured on the CPU and cached per process.  Nothing here comes from the
HIP path.  The true residual |b - S dc| / (tol |b|) (gp_checks.true_residual on the reference's S and b) at the
product's pcg_tol 1e-5 is held at or below 2 x max(1, the oracle's figure), as gp_checks.oracle_true_residual.
"""
import numpy as np

import ba_edge_scene as E
import ba_reference as R
import ba_solve_reference as B
from gp_checks import true_residual  # noqa: F401  (generic: takes any reference with S and b)
from gp_reference import LD, split
from oracle import oracle as O

TOL = dict(Y=1e-12, V=1e-12, gp=1e-12, U=1e-10, gc=1e-10, b=1e-10, St=1e-9, dc=1e-8, dp=1e-8)
COST_TOL = 1e-12
ORDER = ("Y", "V", "gp", "U", "gc", "b", "St", "dc", "dp")
TR = dict(tr_radius=1e4, tr_max=1e10, tr_min=1e-6, tr_up=2.0, tr_down=0.5 ** 4, tr_factor=0.25, tr_high=0.5, tr_low=1e-3)


def oracle_for(name, model, variant="", **kw):
    p, s = E.problem(name, model), E.settings(name, model)
    return O.OracleBA(p.model, p.uv, p.cam_idx, p.pt_idx, p.pp, p.n_cams, p.n_points, variant=variant, **dict(s, **kw))


def pattern(name, model):
    key = ("pattern", name, model)
    if key not in _cache:
        _cache[key] = oracle_for(name, model).pattern()
    return _cache[key]


def oracle_solve(name, model, f, variant="", **kw):
    """the oracle's `got` for damping factor f at the scene's initial parameters, and its PCG iteration count"""
    p, s = E.problem(name, model), E.settings(name, model)
    ora = oracle_for(name, model, variant, **kw)
    ora.linearize(p.cams_init, p.points_init)
    W, V = ora.get(O.W), ora.get(O.V)
    it = ora.solve(f)
    assert it >= 0
    return dict(Y=R.y_from(W, V, p.pt_idx, E.F1, s["clamp_min"], s["clamp_max"]), V=V, gp=ora.get(O.GP), U=ora.get(O.U),
                gc=ora.get(O.GC), b=ora.get(O.B), St=ora.get(O.S), dc=ora.get(O.DC), dp=ora.get(O.DP)), it


# ------------------------------------------------------------------------------------------------------------
# reference values with their entrywise scales, and the reduction of entrywise figures to items
# ------------------------------------------------------------------------------------------------------------
def _top(a, axes):
    """the largest |entry| over `axes`, broadcast back to a's shape"""
    return np.broadcast_to(np.abs(a).max(axis=axes, keepdims=True), a.shape)


def reference(sys_, pat, dc=None, records=None):
    """name -> (hi, lo, scale), float64 arrays of the quantity's own shape.  dp: the reference's back-substitution of
    the camera step `dc` that the implementation found (None: points-only), so its CG tolerance does not enter;
    `records`: the System at F1 whose records Y are compared (default sys_)."""
    ptr = np.searchsorted(sys_.pt, np.arange(sys_.gp.shape[0] + 1))
    lengths = np.diff(ptr)

    def f64(a):
        return np.asarray(a).astype(np.float64)

    Y = (sys_ if records is None else records).records()
    ytop = np.maximum.reduceat(np.abs(f64(Y)).reshape(Y.shape[0], -1).max(axis=1), ptr[:-1])
    V = np.stack([sys_.V[:, a, b] for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], axis=1)
    d = np.sqrt(np.abs(f64(sys_.diag_c)).max(axis=0))
    St, St_abs = sys_.scaled(pat)
    dstar = f64(sys_.dc)
    dscale = np.concatenate([_top(dstar[:, 0:3], 1), _top(dstar[:, 3:6], 1), _top(dstar[:, 6:], 0)], axis=1)
    back = sys_.backsub(dc)
    out = dict(Y=split(Y) + (np.repeat(ytop, lengths)[:, None, None] * np.ones(Y.shape),),
               V=split(V) + (_top(f64(V), 1),), gp=split(sys_.gp) + (_top(f64(sys_.gp_abs), 1),),
               U=split(sys_.U) + (np.broadcast_to(d[:, None] * d[None, :], sys_.U.shape),),
               gc=split(sys_.gc) + (f64(sys_.gc_abs),), b=split(sys_.b.reshape(sys_.gc.shape)) + (f64(sys_.b_abs).reshape(sys_.gc.shape),),
               St=split(St) + (_top(f64(St_abs), (1, 2)),), dc=split(sys_.dc) + (dscale,),
               dp=split(back["dp"]) + (_top(f64(back["dp_abs"]), 1),))
    out["_ptr"] = ptr
    return out


def _items(name, q, ptr):
    """entrywise figures -> per item"""
    if name == "Y":
        return np.maximum.reduceat(q.reshape(q.shape[0], -1).max(axis=1), ptr[:-1])
    if name in ("gc", "b"):
        return q.reshape(-1)
    if name == "dc":
        return np.concatenate([q[:, 0:3].max(axis=1), q[:, 3:6].max(axis=1), q[:, 6:].max(axis=0)])
    return q.reshape(q.shape[0], -1).max(axis=1)


def errors(got, ref):
    """name -> per-item error array of `got` against reference(...); an entry whose scale is 0 must be exact"""
    out = {}
    for k in (k for k in ORDER if k in got):
        hi, lo, scale = ref[k]
        g = np.asarray(got[k], dtype=np.float64).reshape(hi.shape)
        if not np.all(np.isfinite(g)):
            out[k] = np.full(_items(k, np.zeros(hi.shape), ref["_ptr"]).shape, np.inf)
            continue
        err = np.abs((g.astype(LD) - hi.astype(LD)) - lo.astype(LD))
        q = np.where(scale > 0, err / np.where(scale > 0, scale, 1), np.where(err == 0, 0.0, np.inf)).astype(np.float64)
        out[k] = _items(k, q, ref["_ptr"])
    return out


def spread(plain, fma, ref):
    """per-item distance of the oracle's fused-multiply-add build from its plain build, in errors()' norm"""
    between = {k: (np.asarray(plain[k], dtype=np.float64).reshape(ref[k][0].shape), np.zeros(ref[k][0].shape), ref[k][2])
               for k in ORDER}
    between["_ptr"] = ref["_ptr"]
    return errors(fma, between)


def bounds(spr, dc_distance=None):
    """max(tolerance, 8 x spread) per item; dc: max(1e-8, 8 x the oracle's own distance from the direct solution)"""
    out = {k: np.maximum(TOL[k], 8.0 * spr[k]) for k in spr}
    if dc_distance is not None:
        out["dc"] = np.maximum(TOL["dc"], 8.0 * dc_distance)
    return out


def report(tag, errs, bnd):
    """print the worst figure of every quantity (and how far its bound was widened), then hold every item to its bound"""
    worst = {k: float(np.max(v)) if v.size else 0.0 for k, v in errs.items()}
    print(tag, {k: f"{v:.2e}" for k, v in worst.items()},
          "widest bound", {k: f"{float(np.max(bnd[k])):.1e}" for k in errs if bnd[k].size and np.max(bnd[k]) > TOL[k]})
    for k in errs:
        bad = np.flatnonzero(~(errs[k] <= bnd[k]))
        assert bad.size == 0, (tag, k, bad[:8], errs[k][bad[:8]], bnd[k][bad[:8]])
    return worst


# ------------------------------------------------------------------------------------------------------------
# cached oracle figures
# ------------------------------------------------------------------------------------------------------------
_cache = {}


def oracle_bounds(name, model, precond, f):
    """(bounds, plain `got`, iterations, the oracle's own per-item errors) for one scene, preconditioner and f at
    pcg_tol 1e-12 (cached).  The oracle's precond 2 is the A-DEF2 form the persistent CG runs."""
    key = ("bounds", name, model, precond, float(f))
    if key not in _cache:
        sys_ = E.system(name, model, f)
        plain, it = oracle_solve(name, model, f, precond=precond, pcg_tol=1e-12)
        fma, _ = oracle_solve(name, model, f, variant="fma", precond=precond, pcg_tol=1e-12)
        ref = reference(sys_, pattern(name, model), plain["dc"], E.system(name, model, E.F1))
        own = errors(plain, ref)
        _cache[key] = bounds(spread(plain, fma, ref), own["dc"]), plain, it, own
    return _cache[key]


def oracle_at_tolerance(name, model, precond, f, tol=1e-5):
    """(true_residual() of the oracle's dc, its PCG iterations) at the product's pcg_tol (cached): the HIP path's
    figure is held at or below 2 x max(1, this) -- the factor 2 for the different summation order of a residual that is
    updated, not recomputed"""
    key = ("resid", name, model, precond, float(f), tol)
    if key not in _cache:
        got, it = oracle_solve(name, model, f, precond=precond, pcg_tol=tol)
        _cache[key] = true_residual(E.system(name, model, f), got["dc"], tol), it
    return _cache[key]


def oracle_true_residual(name, model, precond, f, tol=1e-5):
    return oracle_at_tolerance(name, model, precond, f, tol)[0]


# ------------------------------------------------------------------------------------------------------------
# the gain ratio and the trust radius
# ------------------------------------------------------------------------------------------------------------
def tr_update(damping, down, quality, o=TR):
    """lm_policy.h tr_update restated: (damping, down) after a trial of gain ratio `quality`"""
    radius = 1.0 / damping
    radius, down = ((o["tr_up"] * radius, o["tr_down"]) if quality > o["tr_high"] else
                    ((radius, o["tr_down"]) if quality > o["tr_low"] else (radius * down, down * o["tr_factor"])))
    return 1.0 / min(max(radius, o["tr_min"]), o["tr_max"]), down


def reference_quality(name, model, f, cams_new, pts_new, dc, dp):
    """(quality, loss_before, loss_after) from the reference alone: (loss_before - loss_after) / model_decrease(dc, dp),
    the losses by the forward model at the initial and at the returned parameters"""
    p, s = E.problem(name, model), E.settings(name, model)
    sys_ = E.system(name, model, f)
    before, after = sys_.obs.loss, B.cost(p, cams_new, pts_new, s["huber_delta"])
    return float((before - after) / sys_.model_decrease(dc, dp)), float(before), float(after)


def check_gain_margin(quality, before, after, o=TR):
    """the step test's scene property: accepted on the first trial, and the gain ratio at least 10 % away from both
    TrustRegion thresholds, so that no rounding decides the branch"""
    assert after <= before, (before, after)
    for t in (o["tr_high"], o["tr_low"]):
        assert abs(quality / t - 1.0) >= 0.1, (quality, t)
