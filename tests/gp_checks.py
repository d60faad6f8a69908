"""The per-item comparison of one implementation's global-positioning solve (the C oracle or the HIP path) with
tests/gp_reference.py, shared by test_gp_reference.py and test_gpu_gp_edges.py.  Test helper only.

An implementation hands over `got`: W [N,3,3] (camera rows, point columns), V [P,3,3], gp [P,3] = g'_p, b [C,3],
St [nnzb,3,3] = the block-Jacobi scaled S~ in the order of the upper block pattern (rp, col), dc [C,3], dp [P,3], ds [N];
the oracle also U [C,3,3] = U'_c and gc [C,3] = g'_c (the HIP path's debug interface does not hand those out; there they
are covered through b and S~).

Per item means: the error of a track's, camera's, observation's or block's entries over that item's own scale -- its
largest reference entry, or, where the item is a sum that can cancel (g'_p, g'_c, b, S~, dp, ds), the largest entry of the
reference's sum of |terms|.  An item whose scale is 0 (a fixed scale's ds, the empty camera's b and dc) must be exact.

Tolerances are the project's: records, V, g'_p 1e-12; U, g_c, b 1e-10; S~ 1e-9; dc, dp, ds 1e-8; cost 1e-12.
Where float64 cannot deliver that on an item, the item's bound is max(tolerance, 8 x the oracle's plain-versus-fma spread
on that item in the same norm) -- bounds() -- as test_gpu_wide.py does; never anything the code under test returned.
"""
import numpy as np

import gp_edge_scene as E
import gp_reference as G
from oracle import oracle as O

TOL = dict(W=1e-12, V=1e-12, gp=1e-12, U=1e-10, gc=1e-10, b=1e-10, St=1e-9, dc=1e-8, dp=1e-8, ds=1e-8)
COST_TOL = 1e-12
ORDER = ("W", "V", "gp", "U", "gc", "b", "St", "dc", "dp", "ds")


def oracle_for(prob, variant="", **kw):
    return O.OracleGP(prob.trans, prob.cam_idx, prob.pt_idx, prob.fcam, prob.sfree, prob.n_cams, prob.n_points,
                      variant=variant, **kw)


def pattern(ora):
    """(row_ptr, col) of the reduced system's upper blocks, diagonal first in each row"""
    return O.OracleBA.pattern(ora)


def oracle_solve(prob, f, variant="", **kw):
    """the oracle's `got` for damping factor f at the scene's initial parameters, and its PCG iteration count"""
    ora = oracle_for(prob, variant, **kw)
    ora.linearize(prob.cams_init, prob.points_init, prob.scales_init)
    it = ora.solve(f)
    assert it >= 0
    P = prob.n_points
    return dict(W=ora.get(O.W), V=G.sym6(ora.get(O.V)), gp=ora.get(O.GP), U=ora.get(O.U), gc=ora.get(O.GC),
                b=ora.get(O.B), St=ora.get(O.S),
                dc=ora.get(O.DC), dp=ora.get(O.DP).reshape(P, 3), ds=ora.ds()), it


def reference(red, pat, dc):
    """name -> ((hi, lo) value, float64 scale [items]) of the reference for the pattern `pat`; dp and ds for the camera
    step `dc` that the implementation under test found, so its CG tolerance does not enter."""
    rp, col = pat
    C = red.U.shape[0]
    rows = np.repeat(np.arange(C), np.diff(rp))
    back = red.backsub(dc)

    def top(a):                                          # the item's largest |entry|
        a = np.abs(G.split(a)[0])
        return a.reshape(a.shape[0], -1).max(axis=1)

    St, St_abs = red.St[rows, col], red.St_abs[rows, col]
    return dict(W=(G.split(red.W), top(red.W)), V=(G.split(red.V), top(red.V)),
                gp=(G.split(red.gp), top(red.gp_abs)), U=(G.split(red.U), top(red.U)),
                gc=(G.split(red.gc), top(red.gc_abs)), b=(G.split(red.b.reshape(C, 3)), top(red.b_abs.reshape(C, 3))),
                St=(G.split(St), top(St_abs)), dc=(G.split(red.dc), top(red.dc)),
                dp=(G.split(back["dp"]), top(back["dp_abs"])), ds=(G.split(back["ds"]), top(back["ds_abs"])))


def item_errors(got, ref):
    """name -> per-item error array of `got` against reference(...)"""
    out = {}
    for k in (k for k in ORDER if k in got):
        (hi, lo), scale = ref[k]
        g = np.asarray(got[k], dtype=np.float64).reshape(hi.shape)
        out[k] = G.item_err(g, (hi, lo), scale=(scale.reshape((-1,) + (1,) * (hi.ndim - 1)) * np.ones(hi.shape),))
    return out


def spread(plain, fma, ref):
    """per-item distance of the oracle's fused-multiply-add build from its plain build, in item_errors' norm"""
    out = {}
    for k in ORDER:
        (hi, _), scale = ref[k]
        a = np.asarray(plain[k], dtype=np.float64).reshape(hi.shape)
        b = np.asarray(fma[k], dtype=np.float64).reshape(hi.shape)
        d = np.abs(a - b).reshape(hi.shape[0], -1).max(axis=1)
        out[k] = np.where(scale > 0, d / np.where(scale > 0, scale, 1.0), np.where(d == 0, 0.0, np.inf))
    return out


def bounds(spr, tol=TOL):
    return {k: np.maximum(tol[k], 8.0 * spr[k]) for k in ORDER}


def report(tag, errs, bnd):
    """print the worst figure of every quantity (and how far its bound was widened), then hold every item to its bound"""
    worst = {k: float(np.max(v)) if v.size else 0.0 for k, v in errs.items()}
    print(tag, {k: f"{v:.2e}" for k, v in worst.items()},
          "widest bound", {k: f"{float(np.max(b)):.1e}" for k, b in bnd.items() if b.size and np.max(b) > TOL[k]})
    for k in errs:
        bad = np.flatnonzero(~(errs[k] <= bnd[k]))
        assert bad.size == 0, (tag, k, bad[:8], errs[k][bad[:8]], bnd[k][bad[:8]])
    return worst


def true_residual(red, dc, tol):
    """|b - S dc| / (tol |b|) with the reference's S and b (longdouble): at or below 1 when the PCG's stopping rule
    |b - S x| <= tol |b| holds for the true residual, not only for the updated one"""
    L = np.longdouble
    Sh, Sl = G.split(red.S)
    bh, bl = G.split(red.b)
    S, b = Sh.astype(L) + Sl.astype(L), bh.astype(L) + bl.astype(L)
    r = b - S @ np.asarray(dc, dtype=np.float64).reshape(-1).astype(L)
    return float(np.sqrt(np.sum(r * r)) / (L(tol) * np.sqrt(np.sum(b * b))))


def cost_errors(loss, sq, obs):
    """relative errors of a float64 (loss, sum |r|^2) against the reference cost"""
    import mpmath as mp
    with mp.workdps(G.MP_DPS):
        rl, rq = G.cost(obs)
        return dict(loss=float(abs(mp.mpf(float(loss)) - rl) / rl), sq=float(abs(mp.mpf(float(sq)) - rq) / rq))


_oracle_cache = {}


def oracle_bounds(name, precond, f):
    """per-item bounds for scene `name` from the oracle's plain and fused-multiply-add builds at pcg_tol 1e-12 (cached):
    (bounds, plain `got`, iterations)"""
    key = ("bounds", name, precond, float(f))
    if key not in _oracle_cache:
        prob, red = E.problem(name), E.reduced(name, f)
        plain, it = oracle_solve(prob, f, precond=precond, pcg_tol=1e-12)
        fma, _ = oracle_solve(prob, f, variant="fma", precond=precond, pcg_tol=1e-12)
        ref = reference(red, pattern(oracle_for(prob)), plain["dc"])
        _oracle_cache[key] = bounds(spread(plain, fma, ref)), plain, it
    return _oracle_cache[key]


def oracle_true_residual(name, precond, f, tol=1e-5):
    """true_residual() of the oracle's dc at the product's pcg_tol (cached): the HIP path's figure is held at or below
    2 x max(1, this) -- the factor 2 for the different summation order of a residual that is updated, not recomputed"""
    key = ("resid", name, precond, float(f), tol)
    if key not in _oracle_cache:
        got, _ = oracle_solve(E.problem(name), f, precond=precond, pcg_tol=tol)
        _oracle_cache[key] = true_residual(E.reduced(name, f), got["dc"], tol)
    return _oracle_cache[key]
