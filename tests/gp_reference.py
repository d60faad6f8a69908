"""An independent reference for the global-positioning linearization, reduction, back-substitution and cost
(csrc/ba_gp.h, oracle/ba_oracle.c ora_gp_*).  Test helper only (CPU, mpmath, no C oracle, no GPU).

oracle/ba_oracle.c restates the kernels' own closed forms (the scale elimination W_o = -beta^2 (I - a a^T / h_ss), c2, cg,
the damped h_ss), so a slip both share is invisible to GPU-versus-oracle parity.  This module writes down only

 * the forward residual r_o = f_o (t_o - s_o (X_p - c_i)) (utils/cost_function.py:23-29), forward();
 * the Huber kernel with Triggs weighting as the LM applies it: w = 1 if |r| < delta else delta / |r|, rows of r and J
   multiplied by sqrt(w); loss |r|^2 inside, 2 delta |r| - delta^2 outside;
 * the damped normal equations over [camera positions, points, free scales]: H = J~^T J~ with
   diag <- clip(diag, clamp_min, clamp_max) * f, right-hand side -J~^T r~;
 * block elimination that knows only the sparsity: every free scale as a 1x1 pivot (it touches one camera and one
   point), every point as a 3x3 pivot with a plain cofactor inverse; the dense 3C x 3C camera system is what remains.

Jacobian rows are mpmath.diff of forward() along each of the 7 parameters of an observation; the kernels' a / beta
shorthand appears nowhere.  observations() runs in mpmath at MP_DPS digits.  reduce() runs in mpmath ("mp") or, for the
larger scene, in numpy.longdouble over the mp per-observation terms ("ld", as ba_reference.assemble does).

Values are handed out through split() as (hi, lo) double-doubles: hi the value rounded to float64, lo the rest, so
(got - hi) - lo is the error of a float64 `got` far below the 1e-12 the tests ask for.  item_err() is the per-item
norm the tests share.
"""
import numpy as np
import mpmath as mp

MP_DPS = 50
ZERO, INSIDE, OUTSIDE = 0, 1, 2          # Huber branch of an observation: |r| == 0, |r| < delta, |r| >= delta
LD = np.longdouble


def forward(c, X, s, t, f):
    """r = f (t - s (X - c)) on component lists (any arithmetic)"""
    return [f * (t[k] - s * (X[k] - c[k])) for k in range(3)]


def _m(x):
    return mp.mpf(float(x))


def _obj(shape):
    a = np.empty(shape, dtype=object)
    a[...] = mp.mpf(0)
    return a


class Observations:
    """per-observation terms at one parameter point, mpmath objects in numpy object arrays:
    r [N,3], rs [N] = |r|, w [N] the Huber weight, J [N,3,7] = d r / d [c, X, s] (the s column is 0 where the scale
    is fixed: it is no unknown there), huber [N] the branch (ZERO / INSIDE / OUTSIDE), free [N] bool."""


def observations(prob, cams, pts, scales, delta):
    cams, pts, scales = (np.asarray(a, dtype=np.float64) for a in (cams, pts, scales))
    N = prob.n_obs
    out = Observations()
    out.r, out.rs, out.w, out.J = _obj((N, 3)), _obj(N), _obj(N), _obj((N, 3, 7))
    out.huber = np.zeros(N, dtype=np.int64)
    out.free = np.asarray(prob.sfree).astype(bool).copy()
    out.cam, out.pt = np.asarray(prob.cam_idx).astype(np.int64), np.asarray(prob.pt_idx).astype(np.int64)
    out.n_cams, out.n_points, out.delta = prob.n_cams, prob.n_points, float(delta)
    with mp.workdps(MP_DPS):
        d = _m(delta)
        for o in range(N):
            ci, p = out.cam[o], out.pt[o]
            base = [_m(z) for z in cams[ci]] + [_m(z) for z in pts[p]] + [_m(scales[o])]
            t = [_m(z) for z in prob.trans[o]]
            f = _m(prob.fcam[ci])
            r = forward(base[0:3], base[3:6], base[6], t, f)
            rs = mp.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
            out.r[o], out.rs[o] = r, rs
            out.huber[o] = ZERO if rs == 0 else (INSIDE if rs < d else OUTSIDE)
            out.w[o] = mp.mpf(1) if rs < d else d / rs
            for j in range(7 if out.free[o] else 6):
                for k in range(3):
                    def along(z, j=j, k=k):
                        q = base[:j] + [z] + base[j + 1:]
                        return f * (t[k] - q[6] * (q[3 + k] - q[k]))
                    out.J[o, k, j] = mp.diff(along, base[j])
    return out


def cost(obs):
    """(Huber loss, sum |r|^2) as mpmath numbers"""
    with mp.workdps(MP_DPS):
        d = _m(obs.delta)
        loss, sq = mp.mpf(0), mp.mpf(0)
        for rs in obs.rs:
            sq += rs * rs
            loss += rs * rs if rs < d else 2 * d * rs - d * d
        return loss, sq


def cost_at(prob, cams, pts, scales, delta):
    """(Huber loss, sum |r|^2) at any parameters, as float64 pairs (hi, lo): the forward residual alone"""
    cams, pts, scales = (np.asarray(a, dtype=np.float64) for a in (cams, pts, scales))
    with mp.workdps(MP_DPS):
        d = _m(delta)
        loss, sq = mp.mpf(0), mp.mpf(0)
        for o in range(prob.n_obs):
            ci, p = prob.cam_idx[o], prob.pt_idx[o]
            r = forward([_m(z) for z in cams[ci]], [_m(z) for z in pts[p]], _m(scales[o]), [_m(z) for z in prob.trans[o]],
                        _m(prob.fcam[ci]))
            q = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
            rs = mp.sqrt(q)
            sq += q
            loss += q if rs < d else 2 * d * rs - d * d
        return (float(loss), float(loss - mp.mpf(float(loss)))), (float(sq), float(sq - mp.mpf(float(sq))))


# ------------------------------------------------------------------------------------------------------------
# arithmetic: mpmath objects or numpy.longdouble, behind the same numpy calls
# ------------------------------------------------------------------------------------------------------------
def _to(kind, a):
    """object array of mpf -> array of the working arithmetic"""
    if kind == "mp":
        return a
    flat = a.ravel()
    out = np.empty(flat.size, dtype=LD)
    for i, v in enumerate(flat):
        h = float(v)
        out[i] = LD(h) + LD(float(v - mp.mpf(h)))
    return out.reshape(a.shape)


def _num(kind, x):
    return _m(x) if kind == "mp" else LD(x)


def _zeros(kind, shape):
    return _obj(shape) if kind == "mp" else np.zeros(shape, dtype=LD)


def _sqrt(kind, x):
    return mp.sqrt(x) if kind == "mp" else np.sqrt(x)


def _clip(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)


def _inv3(A, kind):
    """plain cofactor inverse of a 3x3 block"""
    c = _zeros(kind, (3, 3))
    for i in range(3):
        for j in range(3):
            a, b, e, g = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            c[j, i] = A[a, e] * A[b, g] - A[a, g] * A[b, e]
    det = A[0, 0] * c[0, 0] + A[0, 1] * c[1, 0] + A[0, 2] * c[2, 0]
    return c / det


def _solve(A, b):
    """Gaussian elimination with partial pivoting (any arithmetic); A, b are copied"""
    A, b = A.copy(), b.copy()
    n = b.shape[0]
    for k in range(n):
        piv = max(range(k, n), key=lambda i: abs(A[i, k]))
        if piv != k:
            A[[k, piv]] = A[[piv, k]]
            b[[k, piv]] = b[[piv, k]]
        for i in range(k + 1, n):
            m = A[i, k] / A[k, k]
            if m != 0:
                A[i, k:] = A[i, k:] - m * A[k, k:]
                b[i] = b[i] - m * b[k]
    x = b.copy()
    for k in range(n - 1, -1, -1):
        s = x[k]
        for j in range(k + 1, n):
            s = s - A[k, j] * x[j]
        x[k] = s / A[k, k]
    return x


def _chol3(A, kind):
    L = _zeros(kind, (3, 3))
    for i in range(3):
        for j in range(i + 1):
            s = A[i, j]
            for k in range(j):
                s = s - L[i, k] * L[j, k]
            L[i, j] = _sqrt(kind, s) if i == j else s / L[j, j]
    return L


def _abs(a):
    return np.abs(a) if a.dtype != object else np.frompyfunc(abs, 1, 1)(a)


class Reduced:
    """what reduce() returns, arrays in the working arithmetic (split() turns them into double-doubles):
    per observation  W [N,3,3] the reduced camera-point block, sdiag [N] the undamped scale diagonal, hss_clamped [N]
                     (free scales with sdiag below clamp_min), pivot [N] the damped scale diagonal (0 where fixed);
    per track        V [P,3,3], gp [P,3] = g'_p, gp_abs [P,3] = sum |terms| of g'_p, clamped_p [P], diag_p [P,3] the
                     undamped diagonal;
    per camera       U [C,3,3] = U'_c, gc [C,3] = g'_c, gc_abs [C,3], clamped_c [C], diag_c [C,3];
    reduced system   S [3C,3C], b [3C], b_abs [3C] = sum |terms|, St [C,C,3,3] the block-Jacobi scaled
                     S~_ij = L_i^-1 S_ij L_j^-T (S_ii = L_i L_i^T), St_abs the same of sum |terms|, dc [C,3] the direct
                     solution;
    dp(dc) [P,3] and ds(dc) [N]: the back-substitution for a given camera step (backsub(dc) gives both at once)."""

    def backsub(self, dc):
        """dp [P,3], ds [N] for the camera step dc [C,3], with dp_abs / ds_abs, the sums of |terms| behind them"""
        with mp.workdps(MP_DPS):
            kind = self.kind
            dc = _to_work(kind, dc)
            t, t_abs = self.gp.copy(), self.gp_abs.copy()
            for o in range(self.cam.size):
                t[self.pt[o]] = t[self.pt[o]] - self.W[o].T @ dc[self.cam[o]]
                t_abs[self.pt[o]] = t_abs[self.pt[o]] + _abs(self.W[o].T) @ _abs(dc[self.cam[o]])
            dp = np.stack([self.Vinv[p] @ t[p] for p in range(t.shape[0])])
            dp_abs = np.stack([_abs(self.Vinv[p]) @ t_abs[p] for p in range(t.shape[0])])
            ds, ds_abs = _zeros(kind, self.cam.size), _zeros(kind, self.cam.size)
            for o in np.flatnonzero(self.free):
                m, c, p = self.m[o], self.cam[o], self.pt[o]
                ds[o] = (self.gs[o] - m[0:3] @ dc[c] - m[3:6] @ dp[p]) / self.pivot[o]
                ds_abs[o] = (abs(self.gs[o]) + _abs(m[0:3]) @ _abs(dc[c]) + _abs(m[3:6]) @ dp_abs[p]) / self.pivot[o]
            return dict(dp=dp, dp_abs=dp_abs, ds=ds, ds_abs=ds_abs)

    def dp(self, dc):
        return self.backsub(dc)["dp"]

    def ds(self, dc):
        return self.backsub(dc)["ds"]


def _to_work(kind, a):
    a = np.asarray(a)
    if a.dtype == object or a.dtype == LD:
        return a
    if kind == "ld":
        return a.astype(LD)
    out = np.empty(a.shape, dtype=object)
    for idx in np.ndindex(a.shape):
        out[idx] = _m(a[idx])
    return out


def reduce(obs, f, clamp_min=1e-6, clamp_max=1e32, kind="mp", mutate=None):
    """Damped normal equations at damping factor f and their block elimination down to the camera system.
    `mutate` plants a deliberate error for the mutation check: "hss_no_f" leaves f out of the scale pivots,
    "gp_sign" flips the sign of the scale-gradient term in g'_p."""
    with mp.workdps(MP_DPS):
        return _reduce(obs, f, clamp_min, clamp_max, kind, mutate)


def _reduce(obs, f, clamp_min, clamp_max, kind, mutate):
    N, C, P = obs.cam.size, obs.n_cams, obs.n_points
    cam, pt = obs.cam, obs.pt
    fz, lo, hi = _num(kind, f), _num(kind, clamp_min), _num(kind, clamp_max)
    J, r, w = _to(kind, obs.J), _to(kind, obs.r), _to(kind, obs.w)
    Jt = np.transpose(J, (0, 2, 1))
    M = np.stack([w[o] * (Jt[o] @ J[o]) for o in range(N)]) if N else _zeros(kind, (0, 7, 7))
    g = np.stack([-(w[o] * (Jt[o] @ r[o])) for o in range(N)]) if N else _zeros(kind, (0, 7))

    def damp(x):
        return _clip(x, lo, hi) * fz

    out = Reduced()
    out.kind, out.cam, out.pt, out.free = kind, cam, pt, obs.free
    # --- every free scale as a 1x1 pivot: it couples to its own camera and point only
    out.pivot = _zeros(kind, N)
    out.hss_clamped = np.zeros(N, dtype=bool)
    out.m, out.gs, out.sdiag = M[:, 0:6, 6].copy(), g[:, 6].copy(), M[:, 6, 6].copy()
    A = M[:, 0:6, 0:6].copy()              # per-observation [camera, point] block with the scale eliminated
    h = g[:, 0:6].copy()
    h_abs = _abs(h)
    for o in np.flatnonzero(obs.free):
        out.hss_clamped[o] = bool(M[o, 6, 6] < lo)
        out.pivot[o] = _clip(M[o, 6, 6], lo, hi) if mutate == "hss_no_f" else damp(M[o, 6, 6])
        m = out.m[o]
        A[o] = A[o] - np.outer(m, m) / out.pivot[o]
        corr = m * (g[o, 6] / out.pivot[o])
        if mutate == "gp_sign":
            corr = np.concatenate([corr[0:3], -corr[3:6]])
        h[o] = h[o] - corr
        h_abs[o] = h_abs[o] + _abs(corr)
    out.W = A[:, 0:3, 3:6].copy()
    # --- camera and point blocks: the undamped diagonal sums decide the clamp; the scale fill-in comes on top
    dC, dP = _zeros(kind, (C, 3)), _zeros(kind, (P, 3))
    out.U, out.V = _zeros(kind, (C, 3, 3)), _zeros(kind, (P, 3, 3))
    out.gc, out.gp, out.gp_abs = _zeros(kind, (C, 3)), _zeros(kind, (P, 3)), _zeros(kind, (P, 3))
    gc_abs = _zeros(kind, (C, 3))
    for o in range(N):
        ci, p = cam[o], pt[o]
        for k in range(3):
            dC[ci, k] = dC[ci, k] + M[o, k, k]
            dP[p, k] = dP[p, k] + M[o, 3 + k, 3 + k]
        Ao = A[o].copy()
        for k in range(6):
            Ao[k, k] = Ao[k, k] - M[o, k, k]          # the undamped diagonal is put back below, clipped and damped
        out.U[ci] = out.U[ci] + Ao[0:3, 0:3]
        out.V[p] = out.V[p] + Ao[3:6, 3:6]
        out.gc[ci] = out.gc[ci] + h[o, 0:3]
        out.gp[p] = out.gp[p] + h[o, 3:6]
        gc_abs[ci] = gc_abs[ci] + h_abs[o, 0:3]
        out.gp_abs[p] = out.gp_abs[p] + h_abs[o, 3:6]
    out.clamped_c = np.array([any(dC[c, k] < lo for k in range(3)) for c in range(C)], dtype=bool)
    out.clamped_p = np.array([any(dP[p, k] < lo for k in range(3)) for p in range(P)], dtype=bool)
    out.diag_c, out.diag_p, out.gc_abs = dC, dP, gc_abs
    for c in range(C):
        for k in range(3):
            out.U[c, k, k] = out.U[c, k, k] + damp(dC[c, k])
    for p in range(P):
        for k in range(3):
            out.V[p, k, k] = out.V[p, k, k] + damp(dP[p, k])
    # --- every point as a 3x3 pivot
    n = 3 * C
    S, S_abs = _zeros(kind, (n, n)), _zeros(kind, (n, n))
    b, b_abs = out.gc.reshape(-1).copy(), gc_abs.reshape(-1).copy()
    for c in range(C):
        S[3 * c:3 * c + 3, 3 * c:3 * c + 3] = out.U[c]
        S_abs[3 * c:3 * c + 3, 3 * c:3 * c + 3] = _abs(out.U[c])
    ptr = np.searchsorted(pt, np.arange(P + 1))
    out.Vinv = _zeros(kind, (P, 3, 3))
    for p in range(P):
        Vi = _inv3(out.V[p], kind)
        out.Vinv[p] = Vi
        blocks = {}
        for o in range(ptr[p], ptr[p + 1]):
            blocks[cam[o]] = blocks[cam[o]] + out.W[o] if cam[o] in blocks else out.W[o]
        for ci, Wi in blocks.items():
            WV = Wi @ Vi
            t = WV @ out.gp[p]
            b[3 * ci:3 * ci + 3] = b[3 * ci:3 * ci + 3] - t
            b_abs[3 * ci:3 * ci + 3] = b_abs[3 * ci:3 * ci + 3] + _abs(WV) @ out.gp_abs[p]
            for cj, Wj in blocks.items():
                t = WV @ Wj.T
                S[3 * ci:3 * ci + 3, 3 * cj:3 * cj + 3] = S[3 * ci:3 * ci + 3, 3 * cj:3 * cj + 3] - t
                S_abs[3 * ci:3 * ci + 3, 3 * cj:3 * cj + 3] = S_abs[3 * ci:3 * ci + 3, 3 * cj:3 * cj + 3] + _abs(t)
    out.S, out.b, out.b_abs = S, b, b_abs
    out.dc = _solve(S, b).reshape(C, 3)
    # --- block-Jacobi scaling S~_ij = L_i^-1 S_ij L_j^-T
    one = _num(kind, 1.0)
    Li = []
    for c in range(C):
        L = _chol3(S[3 * c:3 * c + 3, 3 * c:3 * c + 3], kind)
        inv = _zeros(kind, (3, 3))
        for j in range(3):                                    # forward substitution, column by column
            for i in range(j, 3):
                s = one if i == j else _num(kind, 0.0)
                for k in range(j, i):
                    s = s - L[i, k] * inv[k, j]
                inv[i, j] = s / L[i, i]
        Li.append(inv)
    out.St, out.St_abs = _zeros(kind, (C, C, 3, 3)), _zeros(kind, (C, C, 3, 3))
    for i in range(C):
        for j in range(C):
            blk = S[3 * i:3 * i + 3, 3 * j:3 * j + 3]
            out.St[i, j] = Li[i] @ blk @ Li[j].T
            out.St_abs[i, j] = _abs(Li[i]) @ S_abs[3 * i:3 * i + 3, 3 * j:3 * j + 3] @ _abs(Li[j].T)
    return out


# ------------------------------------------------------------------------------------------------------------
# double-doubles and the per-item norm
# ------------------------------------------------------------------------------------------------------------
def split(a):
    """array (or scalar) of the working arithmetic -> (hi, lo) float64 arrays, value = hi + lo"""
    a = np.asarray(a)
    if a.dtype == object:
        with mp.workdps(MP_DPS):
            hi = np.array([float(v) for v in a.ravel()], dtype=np.float64).reshape(a.shape)
            lo = np.array([float(v - mp.mpf(h)) for v, h in zip(a.ravel(), hi.ravel())], dtype=np.float64).reshape(a.shape)
        return hi, lo
    hi = a.astype(np.float64)
    return hi, (a.astype(LD) - hi.astype(LD)).astype(np.float64)


def item_err(got, ref, scale=None):
    """Per-item relative error of float64 `got` [items, ...] against the reference `ref` (working arithmetic or a
    (hi, lo) pair): max over the item's entries of |got - ref| divided by the item's own largest |ref| entry -- or,
    where `scale` is given (the reference's sum |terms| of a sum that may cancel), by the largest entry of that.  An
    item whose scale is 0 must be exact: inf otherwise.  Returns a float64 array [items]."""
    hi, lo = ref if isinstance(ref, tuple) else split(ref)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == hi.shape, (got.shape, hi.shape)
    n = hi.shape[0]
    if not np.all(np.isfinite(got)):
        return np.full(n, np.inf)
    err = np.abs((got.astype(LD) - hi.astype(LD)) - lo.astype(LD)).reshape(n, -1).max(axis=1)
    sc = np.abs(hi if scale is None else (scale[0] if isinstance(scale, tuple) else split(scale)[0]))
    sc = sc.reshape(n, -1).max(axis=1).astype(LD)
    out = np.where(sc > 0, err / np.where(sc > 0, sc, 1), np.where(err == 0, 0.0, np.inf))
    return out.astype(np.float64)


def sym6(V):
    """packed [P,6] (xx xy xz yy yz zz) -> full [P,3,3]"""
    V = np.asarray(V)
    full = np.empty((V.shape[0], 3, 3), dtype=V.dtype)
    for k, (a, b) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
        full[:, a, b] = full[:, b, a] = V[:, k]
    return full


def expand_w(rec):
    """the kernel's 32-byte records {u, beta^2} [N,4] -> the 3x3 blocks they stand for (include/insfm_ba_debug.h):
    W_o = -beta^2 (I - u u^T).  This is the storage format's definition, not a formula of the reference."""
    rec = np.asarray(rec, dtype=np.float64)
    u, b2 = rec[:, 0:3], rec[:, 3]
    return -b2[:, None, None] * (np.eye(3)[None] - u[:, :, None] * u[:, None, :])
