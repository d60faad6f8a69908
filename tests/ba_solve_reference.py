"""An independent reference for the middle of a bundle-adjustment trial: the damped normal equations, the reduced
camera system, its direct solution, the back-substitution and the model decrease.  Test helper only (CPU, no GPU, no
C oracle).

oracle/ba_oracle.c restates the kernels' own closed forms (prep_points' clamp-then-f, the stored records, S = U - Y Y^T
row by row, the PCG to the same iteration), so a slip both share is invisible to GPU-versus-oracle parity.  This module
takes the per-observation r, Jc, Jp of ba_reference.reference_obs (float64 autograd, mpmath where asked) as exact
inputs and from there on works in numpy.longdouble:

 * observe():  the Triggs-corrected rows r~ = sqrt(w) r, J~ = sqrt(w) J (w = 1 if |r| < delta else delta / |r|);
 * reduce():   W_o, V_p, g_p, U_c, g_c summed as ba_reference.assemble does (with the sums of |terms| next to g_p and
               g_c); the LM's damping as the reference project describes it (diagonal clamped to [clamp_min, clamp_max],
               then multiplied by the cumulative factor f), on the camera blocks and the point blocks alike; generic
               block elimination of the points, one 3x3 pivot per track with a plain cofactor inverse, over the blocks
               of the dense full system: S = U_d - sum_p W V_d^-1 W^T, b = g_c - sum W V_d^-1 g_p (S_abs, b_abs: the
               sums of |terms|); the Y Y^T form appears nowhere;
 * System.scaled(): the block-Jacobi scaled S~_ij = L_i^-1 S_ij L_j^-T, L_i = chol(S_ii), and its |terms| bound;
 * System.records(): Y_o = W_o R_p^-T, R_p = chol(V_d) -- the storage format's definition (insfm_ba_debug.h);
 * System.dc:  the direct solution: float64 Cholesky of the diagonally equilibrated dense S, refined with longdouble
               residuals until the residual stops falling (refined_solve);
 * System.backsub(dc): dp = V_d^-1 (g_p - sum W^T dc) per track with its |terms|; dc=None: points-only, V_d^-1 g_p;
 * System.model_decrease(dc, dp) = sum |r~|^2 - |r~ + J~c dc + J~p dp|^2 over the observations: the undamped
               quadratic's decrease, written without U, V or g;
 * System.full(): the dense damped (C D + 3 P) system, for the reference's own check against an all-at-once solve.

Values are handed out through gp_reference.split as (hi, lo) double-doubles.

Reached (x86-64, 80-bit longdouble): the final residual |b - S dc| is 1e-19 .. 1.1e-18 |b| on every scene of
ba_edge_scene.py (asserted below 1e-17 |b|); block elimination + back-substitution agree with the refined dense solve
of the full system to 6e-17 .. 1e-12 (dc) and 1e-18 .. 9e-15 (dp) on the per-item scales: both solves are as good as
their residual, and the conditioning (gauge directions held by the damping alone) stands between residual and solution
(test_ba_solve_reference.py).

`mutate` plants one deliberate error for the mutation checks: ("drop_pair", o) leaves observation o's contribution out
of the off-diagonal block between its camera and the next other camera of its track; ("no_clamp_c", (c, k)) and
("no_clamp_p", (p, k)) skip the clamp on one diagonal entry; "undamped_V" eliminates with the undamped point blocks.
"""
import numpy as np

import ba_reference as R
from gp_reference import LD, split


class Observed:
    """Triggs-corrected rows at one parameter point, longdouble: rt [N,2], Jc [N,2,D], Jp [N,2,3]; cam, pt [N];
    r [N,2] float64 (raw), beyond [N] bool (|r| >= delta), loss (Huber), n_cams, n_points, D, delta"""


def observe(prob, cams, pts, delta=1.0, mp_mask=None):
    r, Jc, Jp = R.reference_obs(prob, np.asarray(cams), np.asarray(pts), mp_mask)
    out = Observed()
    out.cam, out.pt = np.asarray(prob.cam_idx).astype(np.int64), np.asarray(prob.pt_idx).astype(np.int64)
    out.n_cams, out.n_points, out.D, out.delta, out.r = prob.n_cams, prob.n_points, Jc.shape[2], float(delta), r
    rl, d = r.astype(LD), LD(delta)
    s = np.sum(rl * rl, axis=1)
    rs = np.sqrt(s)
    inside = rs < d
    sw = np.sqrt(np.where(inside, LD(1), d / np.where(inside, LD(1), rs)))
    out.rt, out.Jc, out.Jp = rl * sw[:, None], Jc.astype(LD) * sw[:, None, None], Jp.astype(LD) * sw[:, None, None]
    out.beyond = ~inside
    out.loss = np.sum(np.where(inside, s, LD(2) * d * rs - d * d))
    return out


def cost(prob, cams, pts, delta=1.0):
    """Huber loss at any parameters (the forward model alone), as a longdouble"""
    c, p = np.asarray(prob.cam_idx), np.asarray(prob.pt_idx)
    r = (R.project(prob.model, np.asarray(pts)[p], np.asarray(cams)[c], prob.pp[c]).numpy() - prob.uv).astype(LD)
    s, d = np.sum(r * r, axis=1), LD(delta)
    rs = np.sqrt(s)
    return np.sum(np.where(rs < d, s, LD(2) * d * rs - d * d))


# ------------------------------------------------------------------------------------------------------------
# small dense tools, batched over the leading axis, longdouble
# ------------------------------------------------------------------------------------------------------------
def inv3(A):
    """plain cofactor inverse of 3x3 blocks [n,3,3]; also returns the determinants"""
    c = np.empty_like(A)
    for i in range(3):
        for j in range(3):
            a, b, e, g = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            c[:, j, i] = A[:, a, e] * A[:, b, g] - A[:, a, g] * A[:, b, e]
    det = A[:, 0, 0] * c[:, 0, 0] + A[:, 0, 1] * c[:, 1, 0] + A[:, 0, 2] * c[:, 2, 0]
    return c / det[:, None, None], det


def chol(A):
    """lower Cholesky factors of [n,k,k]; the second result is False where a pivot was not positive"""
    n, k = A.shape[0], A.shape[1]
    L, ok = np.zeros_like(A), np.ones(n, dtype=bool)
    for j in range(k):
        s = A[:, j, j] - np.sum(L[:, j, :j] * L[:, j, :j], axis=1)
        ok &= s > 0
        L[:, j, j] = np.sqrt(np.where(s > 0, s, 1))
        for i in range(j + 1, k):
            L[:, i, j] = (A[:, i, j] - np.sum(L[:, i, :j] * L[:, j, :j], axis=1)) / L[:, j, j]
    return L, ok


def tri_inv(L):
    """inverses of lower triangular [n,k,k] by forward substitution"""
    k = L.shape[1]
    X, eye = np.zeros_like(L), np.eye(k, dtype=L.dtype)
    for i in range(k):
        X[:, i, :] = (eye[i][None, :] - np.einsum("nj,njc->nc", L[:, i, :i], X[:, :i, :])) / L[:, i, i][:, None]
    return X


def refined_solve(A, b, max_rounds=60):
    """x with A x = b for a dense SPD longdouble A: float64 Cholesky of the diagonally equilibrated matrix, then
    iterative refinement with longdouble residuals until the residual norm stops falling.  Returns (x, |b - A x| / |b|)."""
    if not np.all(np.diagonal(A) > 0):
        raise np.linalg.LinAlgError("diagonal not positive")
    d = LD(1) / np.sqrt(np.diagonal(A))
    Lf = np.linalg.cholesky(((A * d[:, None]) * d[None, :]).astype(np.float64))      # raises where A is not SPD
    Li = np.linalg.inv(Lf)

    def solve(v):
        return Li.T @ (Li @ v)

    x, nb = np.zeros(b.shape[0], dtype=LD), np.sqrt(np.sum(b * b))
    best, best_x = None, x
    for _ in range(max_rounds):
        r = b - A @ x
        nr = np.sqrt(np.sum(r * r))
        if best is not None and not nr < best:
            break
        best, best_x = nr, x
        if nr == 0:
            break
        # the correction in two float64 pieces, so that the update itself carries more than 53 bits
        rs = r * d
        hi = rs.astype(np.float64)
        lo = (rs - hi.astype(LD)).astype(np.float64)
        x = x + d * (solve(hi).astype(LD) + solve(lo).astype(LD))
    return best_x, (float(best / nb) if nb > 0 else 0.0)


# ------------------------------------------------------------------------------------------------------------
# the damped system and its reduction
# ------------------------------------------------------------------------------------------------------------
class System:
    """What reduce() returns (longdouble):
    per observation  W [N,D,3];
    per track        V [P,3,3] undamped, Vd damped, Vinv = Vd^-1, gp [P,3], gp_abs, diag_p [P,3] the undamped diagonal;
    per camera       U [C,D,D] undamped, Ud damped, gc [C,D], gc_abs, diag_c [C,D];
    clamp report     below_c / above_c [C,D], below_p / above_p [P,3] bool;
    reduced system   S [CD,CD], S_abs, b [CD], b_abs, spd (every V_d, the dense S), dc [C,D] the direct solution,
                     dc_resid its |b - S dc| / |b|."""

    def scaled(self, pat):
        """(S~ [nnzb,D,D], its |terms| bound) for the upper block pattern pat = (row_ptr, col)"""
        key = (pat[0].tobytes(), pat[1].tobytes())
        if key not in self._scaled:
            C, D = self.U.shape[0], self.U.shape[1]
            rp, col = (np.asarray(a).astype(np.int64) for a in pat)
            rows = np.repeat(np.arange(C), np.diff(rp))
            S4, A4 = self.S.reshape(C, D, C, D), self.S_abs.reshape(C, D, C, D)
            L, ok = chol(np.stack([S4[c, :, c, :] for c in range(C)]))
            assert ok.all()
            Li = tri_inv(L)
            LiT, aLi = np.transpose(Li, (0, 2, 1)), np.abs(Li)
            St = np.matmul(np.matmul(Li[rows], S4[rows, :, col, :]), LiT[col])
            St_abs = np.matmul(np.matmul(aLi[rows], A4[rows, :, col, :]), np.transpose(aLi, (0, 2, 1))[col])
            self._scaled[key] = St, St_abs
        return self._scaled[key]

    def records(self):
        """Y [N,D,3] = W_o R_p^-T, R_p the lower Cholesky factor of the damped point block"""
        Rf, ok = chol(self.Vd)
        assert ok.all()
        return np.einsum("oak,ojk->oaj", self.W, tri_inv(Rf)[self.pt])

    def backsub(self, dc=None):
        """dp [P,3] for the camera step dc [C,D] (None: points-only mode, V_d^-1 g_p) and dp_abs, the |terms| behind it"""
        t, t_abs = self.gp.copy(), self.gp_abs.copy()
        if dc is not None:
            dc = np.asarray(dc).astype(LD).reshape(self.gc.shape)
            np.add.at(t, self.pt, -np.einsum("oak,oa->ok", self.W, dc[self.cam]))
            np.add.at(t_abs, self.pt, np.einsum("oak,oa->ok", np.abs(self.W), np.abs(dc[self.cam])))
        return dict(dp=np.einsum("pjk,pk->pj", self.Vinv, t), dp_abs=np.einsum("pjk,pk->pj", np.abs(self.Vinv), t_abs))

    def model_decrease(self, dc, dp):
        """sum_o |r~|^2 - |r~ + J~c dc + J~p dp|^2 (dc None: cameras fixed)"""
        o = self.obs
        e = o.rt + np.einsum("oak,ok->oa", o.Jp, np.asarray(dp).astype(LD).reshape(-1, 3)[o.pt])
        if dc is not None:
            e = e + np.einsum("oad,od->oa", o.Jc, np.asarray(dc).astype(LD).reshape(self.gc.shape)[o.cam])
        return np.sum(np.sum(o.rt * o.rt, axis=1) - np.sum(e * e, axis=1))

    def quadratic_decrease(self, dc, dp):
        """2 g.d - d^T H d from the undamped blocks (what the kernels' gain parts add up to); used only to check
        model_decrease against the reference's own blocks"""
        dc, dp = np.asarray(dc).astype(LD).reshape(self.gc.shape), np.asarray(dp).astype(LD).reshape(-1, 3)
        lin = np.sum(self.gc * dc) + np.sum(self.gp * dp)
        quad = (np.einsum("ca,cab,cb->", dc, self.U, dc) + np.einsum("pj,pjk,pk->", dp, self.V, dp)
                + 2 * np.einsum("oa,oak,ok->", dc[self.cam], self.W, dp[self.pt]))
        return 2 * lin - quad

    def full(self):
        """(H, g): the dense damped system over [cameras, points]"""
        C, D = self.gc.shape
        P, n = self.gp.shape[0], C * D
        H = np.zeros((n + 3 * P, n + 3 * P), dtype=LD)
        for c in range(C):
            H[c * D:(c + 1) * D, c * D:(c + 1) * D] = self.Ud[c]
        for p in range(P):
            H[n + 3 * p:n + 3 * p + 3, n + 3 * p:n + 3 * p + 3] = self.Vd[p]
        for o in range(self.cam.size):
            c, p = self.cam[o], self.pt[o]
            H[c * D:(c + 1) * D, n + 3 * p:n + 3 * p + 3] += self.W[o]
            H[n + 3 * p:n + 3 * p + 3, c * D:(c + 1) * D] += self.W[o].T
        return H, np.concatenate([self.gc.reshape(-1), self.gp.reshape(-1)])


def reduce(obs, f, clamp_min=1e-6, clamp_max=1e32, mutate=None, solve=True):
    N, C, P, D = obs.cam.size, obs.n_cams, obs.n_points, obs.D
    cam, pt = obs.cam, obs.pt
    kind, arg = (mutate, None) if isinstance(mutate, str) or mutate is None else mutate
    out = System()
    out.obs, out.cam, out.pt, out.f, out._scaled = obs, cam, pt, float(f), {}
    # --- the sums, as ba_reference.assemble builds them
    out.W = np.einsum("nad,nak->ndk", obs.Jc, obs.Jp)
    out.V, out.U = np.zeros((P, 3, 3), dtype=LD), np.zeros((C, D, D), dtype=LD)
    np.add.at(out.V, pt, np.einsum("naj,nak->njk", obs.Jp, obs.Jp))
    np.add.at(out.U, cam, np.einsum("nad,nae->nde", obs.Jc, obs.Jc))
    out.gp, out.gp_abs, out.gc, out.gc_abs = (np.zeros(s, dtype=LD) for s in ((P, 3), (P, 3), (C, D), (C, D)))
    tp, tc = np.einsum("naj,na->naj", obs.Jp, obs.rt), np.einsum("nad,na->nad", obs.Jc, obs.rt)
    np.add.at(out.gp, pt, -tp.sum(axis=1))
    np.add.at(out.gp_abs, pt, np.abs(tp).sum(axis=1))
    np.add.at(out.gc, cam, -tc.sum(axis=1))
    np.add.at(out.gc_abs, cam, np.abs(tc).sum(axis=1))
    # --- damping: A.diagonal().clamp_(clamp_min, clamp_max), then the cumulative factor
    lo, hi, fz = LD(clamp_min), LD(clamp_max), LD(f)
    out.diag_c, out.diag_p = np.diagonal(out.U, axis1=1, axis2=2).copy(), np.diagonal(out.V, axis1=1, axis2=2).copy()
    out.below_c, out.above_c = out.diag_c < lo, out.diag_c > hi
    out.below_p, out.above_p = out.diag_p < lo, out.diag_p > hi
    dc_d, dp_d = np.clip(out.diag_c, lo, hi) * fz, np.clip(out.diag_p, lo, hi) * fz
    if kind == "no_clamp_c":
        dc_d[arg] = out.diag_c[arg] * fz
    if kind == "no_clamp_p":
        dp_d[arg] = out.diag_p[arg] * fz
    out.Ud, out.Vd = out.U.copy(), out.V.copy()
    for k in range(D):
        out.Ud[:, k, k] = dc_d[:, k]
    for k in range(3):
        out.Vd[:, k, k] = dp_d[:, k]
    # --- every point as a 3x3 pivot
    out.Vinv, det = inv3(out.V if kind == "undamped_V" else out.Vd)
    _, okp = chol(out.Vd)
    n = C * D
    S, S_abs = np.zeros((n, n), dtype=LD), np.zeros((n, n), dtype=LD)
    for c in range(C):
        S[c * D:(c + 1) * D, c * D:(c + 1) * D] = out.Ud[c]
    S_abs += np.abs(S)
    b, b_abs = out.gc.reshape(-1).copy(), out.gc_abs.reshape(-1).copy()
    ptr = np.searchsorted(pt, np.arange(P + 1))
    lane = np.arange(D)
    for p in range(P):
        a, e = ptr[p], ptr[p + 1]
        if a == e:
            continue
        uniq, inv = np.unique(cam[a:e], return_inverse=True)
        Wb = np.zeros((uniq.size, D, 3), dtype=LD)
        np.add.at(Wb, inv, out.W[a:e])
        WV = Wb @ out.Vinv[p]
        T = np.einsum("iak,jbk->iajb", WV, Wb).reshape(uniq.size * D, uniq.size * D)
        idx = (uniq[:, None] * D + lane[None, :]).ravel()
        sel = np.ix_(idx, idx)
        S[sel] -= T
        S_abs[sel] += np.abs(T)
        b[idx] -= (WV @ out.gp[p]).ravel()
        b_abs[idx] += (np.abs(WV) @ out.gp_abs[p]).ravel()
    if kind == "drop_pair":
        o = int(arg)
        p, i = pt[o], cam[o]
        j = next(int(c) for c in cam[ptr[p]:ptr[p + 1]] if c != i)
        Wj = out.W[ptr[p]:ptr[p + 1]][cam[ptr[p]:ptr[p + 1]] == j].sum(axis=0)
        T = out.W[o] @ out.Vinv[p] @ Wj.T
        S[i * D:(i + 1) * D, j * D:(j + 1) * D] += T
        S[j * D:(j + 1) * D, i * D:(i + 1) * D] += T.T
        out.mutated = (i, j)
    out.S, out.S_abs, out.b, out.b_abs = S, S_abs, b, b_abs
    out.spd_points = bool(okp.all() and np.all(det > 0))
    if solve:
        try:
            x, out.dc_resid = refined_solve(S, b)
            out.spd = out.spd_points
        except np.linalg.LinAlgError:
            x, out.dc_resid, out.spd = np.full(n, np.nan, dtype=LD), float("inf"), False
        out.dc = x.reshape(C, D)
        if out.spd and mutate is None:
            assert out.dc_resid < 1e-17, out.dc_resid
    return out


def hi_lo(a):
    return split(np.asarray(a))
