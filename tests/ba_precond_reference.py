"""An independent reference for what runs between the block factorization and the converged camera step: the coarse
basis of the two-level preconditioner, its operators E and E^-1, both coarse corrections and the first CG iterates.
Test helper only (CPU, numpy.longdouble, no GPU, no C oracle).

oracle/ba_oracle.c restates the kernels' closed forms (coarse_basis, ora_coarse_setup, coarse_apply_v, adef2_apply and
the pipelined recurrence of ora_pcg), so a slip both share -- a sign in a rotation column, a cluster-pair segment left
out of E, the wrong coarse-inverse slot under the lag rule -- leaves M~ positive definite or nearly so and the solve
converging, perhaps one iteration later.  This module builds on ba_solve_reference.System (S, b) and takes the cluster
labels as input (the clustering is tested elsewhere):

 * basis():   G_i from the property that makes the coarse space worth its cost -- its columns are the camera's response
              to a similarity of the world.  For a camera in a cluster of two or more and k < 7, G_i[0:6, k] is the
              least-squares solution of  J_c,o[:, 0:6] g = -J_p,o dX_k(X_p)  over the camera's observations, with
              dX_k = e_k (translation), e_{k-3} x X (rotation), X (scale): longdouble normal equations (column
              equilibrated, refined with longdouble residuals) of the reference's own J_c and J_p.  No formula for rho
              or phi is written down.  Intrinsic rows are 0 for k < 7, columns 7.. are the unit intrinsic columns, a
              camera alone in its cluster gets [I_D | 0].  fit[c] is the residual of the fit over the sum of |terms|,
              per column the camera's largest residual row over its largest row of |terms| (a single row whose own
              terms nearly vanish holds the rounding of the Jacobian's larger intermediates): the reference's own
              accuracy, 3.5e-16 .. 5.0e-16 on the scenes of ba_edge_scene.py.
 * Coarse:    L_i = chol(S_ii) and S~_ij = L_i^-1 S_ij L_j^-T block by block (System.scaled's way, diagonal blocks I),
              Z~_i = L_i^T G_i, E = Z~^T S~ Z~ with the sum of |terms| next to it (a zero diagonal entry becomes 1),
              E^-1 by a float64 inverse of the symmetrically equilibrated E refined by Newton steps X += X (I - A X) in
              longdouble; einv_resid = max |I - A X| over max | |A| |X| | (asserted below 1e-17).
 * iterates(): x_0 .. x_k mapped back by L^-T, for
                 precond 1 (additive)  u = r + Z~ E^-1 Z~^T r,               x_0 = 0
                 precond 2 (A-DEF2)    u = r + Z~ E^-1 Z~^T (r - S~ r),      x_0 = Z~ E^-1 Z~^T r_0
              with the E^-1 to apply as a separate argument (the lag rule: current Z~, the previous solve's E^-1), by
              textbook PCG and by the single-reduction recurrence as published (Chronopoulos & Gear 1989; Ghysels &
              Vanroose 2014: alpha = gamma / (delta - beta gamma / alpha_prev)).  Where M~ is symmetric the two agree
              (asserted to 1e-15 by the tests); A-DEF2 with a lagged E^-1 is not symmetric, and the recurrence's
              iterates are then the yardstick from k = 2 on (k = 1 is the same step in both forms).

`mutate` plants one deliberate error: ("rho_sign", k) flips the rho part of rotation column k of every fitted G_i;
("drop_pair", (i, c)) leaves row i's contribution to the cluster pair (cluster of i, c) out of E; ("no_prolong", i)
leaves camera i out of the prolongation.  Using the other slot's E^-1 is the caller's `einv_used`.
"""
import numpy as np

import ba_solve_reference as B
from gp_reference import LD

SIM = 7   # similarity columns: 3 translations, 3 rotations, 1 scale


def _solve_normal(A, R):
    """least-squares g [k,c] of A g = R (A [n,k], R [n,c]) by column-equilibrated longdouble normal equations with
    three rounds of refinement on the longdouble residual; the second result is False where A has no full rank"""
    N = A.T @ A
    if not np.all(np.diagonal(N) > 0):
        return None, False
    d = LD(1) / np.sqrt(np.diagonal(N))
    L, ok = B.chol(((N * d[:, None]) * d[None, :])[None])
    if not ok.all() or np.linalg.cond(((N * d[:, None]) * d[None, :]).astype(np.float64)) > 1e14:
        return None, False
    Li = B.tri_inv(L)[0]
    g = np.zeros((A.shape[1], R.shape[1]), dtype=LD)
    for _ in range(4):
        g = g + d[:, None] * (Li.T @ (Li @ (d[:, None] * (A.T @ (R - A @ g)))))
    return g, True


def basis(obs, pts, labels, mutate=None):
    """(G [C,D,D+1], fit [C]) at the parameters `obs` was taken at (pts [P,3]: the points of that linearization)"""
    kind, arg = mutate if mutate is not None else (None, None)
    C, D = obs.n_cams, obs.D
    MC = D + 1
    labels = np.asarray(labels)
    alone = np.bincount(labels)[labels] < 2
    X = np.asarray(pts).astype(LD)[obs.pt]
    dX = np.zeros((X.shape[0], 3, SIM), dtype=LD)
    eye = np.eye(3, dtype=LD)
    for k in range(3):
        dX[:, k, k] = 1
        dX[:, :, 3 + k] = np.cross(eye[k][None, :], X)
    dX[:, :, 6] = X
    rhs = -np.einsum("nak,nkc->nac", obs.Jp, dX)
    G, fit = np.zeros((C, D, MC), dtype=LD), np.zeros(C)
    for c in range(C):
        sel = obs.cam == c
        if alone[c]:
            G[c, :, :D] = np.eye(D, dtype=LD)
            continue
        assert sel.sum() >= 3, f"camera {c} has {sel.sum()} observations and is not alone in its cluster"
        A, R = obs.Jc[sel][:, :, 0:6].reshape(-1, 6), rhs[sel].reshape(-1, SIM)
        g, ok = _solve_normal(A, R)
        assert ok, f"camera {c}: its observations do not determine the six pose columns"
        terms = np.abs(A) @ np.abs(g) + np.abs(R)
        fit[c] = float(np.max(np.abs(A @ g - R).max(axis=0) / terms.max(axis=0)))
        G[c, 0:6, 0:SIM] = g
        for a in range(6, D):
            G[c, a, a + 1] = 1
        if kind == "rho_sign":
            G[c, 0:3, arg] = -G[c, 0:3, arg]
    assert np.all(np.bincount(obs.cam, minlength=C)[~alone] > 0)
    return G, fit


class Coarse:
    """The coarse operators of one System for one clustering (longdouble): labels, nc, m = nc (D + 1), members [nc]
    lists, L / Li [C,D,D], bt [C D] = L^-1 b, St [CD,CD] dense S~ (diagonal blocks I), G, fit, Zt [C,D,MC], Z [CD,m],
    E / E_abs [m,m], d [m] = 1 / sqrt(diag E), A = diag(d) E diag(d), Einv [m,m], einv_resid, cond (2-norm, of A)."""

    def __init__(self, sys_, pts, labels, mutate=None):
        kind, arg = mutate if mutate is not None else (None, None)
        C, D = sys_.gc.shape
        MC, n = D + 1, C * D
        self.labels = labels = np.asarray(labels).astype(np.int64)
        self.nc = nc = int(labels.max()) + 1
        self.m = m = nc * MC
        self.members = [np.flatnonzero(labels == c) for c in range(nc)]
        # --- block-Jacobi scaling, block by block
        S4 = np.ascontiguousarray(sys_.S.reshape(C, D, C, D).transpose(0, 2, 1, 3))
        A4 = np.ascontiguousarray(sys_.S_abs.reshape(C, D, C, D).transpose(0, 2, 1, 3))
        idx = np.arange(C)
        self.L, ok = B.chol(S4[idx, idx])
        assert ok.all()
        self.Li = Li = B.tri_inv(self.L)
        LiT = np.transpose(Li, (0, 2, 1))
        St4 = np.matmul(np.matmul(Li[:, None], S4), LiT[None, :])
        Sa4 = np.matmul(np.matmul(np.abs(Li)[:, None], A4), np.abs(LiT)[None, :])
        St4[idx, idx] = np.eye(D, dtype=LD)
        Sa4[idx, idx] = np.eye(D, dtype=LD)
        self.St = np.ascontiguousarray(St4.transpose(0, 2, 1, 3)).reshape(n, n)
        St_abs = np.ascontiguousarray(Sa4.transpose(0, 2, 1, 3)).reshape(n, n)
        del S4, A4, St4, Sa4
        self.bt = np.einsum("cak,ck->ca", Li, sys_.b.reshape(C, D)).reshape(n)
        # --- basis
        self.G, self.fit = basis(sys_.obs, pts, labels, mutate if kind == "rho_sign" else None)
        self.Zt = np.matmul(np.transpose(self.L, (0, 2, 1)), self.G)
        self.Z = np.zeros((n, m), dtype=LD)
        for i in range(C):
            self.Z[i * D:(i + 1) * D, labels[i] * MC:(labels[i] + 1) * MC] = self.Zt[i]
        # --- E = Z~^T S~ Z~, cluster column block by cluster column block (Z~ is block sparse)
        E, E_abs = np.zeros((m, m), dtype=LD), np.zeros((m, m), dtype=LD)
        rows = [(mem[:, None] * D + np.arange(D)[None, :]).ravel() for mem in self.members]
        aZ = np.abs(self.Z)
        for c in range(nc):
            cs = slice(c * MC, (c + 1) * MC)
            Y = self.St[:, rows[c]] @ self.Z[rows[c], cs]
            Ya = St_abs[:, rows[c]] @ aZ[rows[c], cs]
            E[:, cs], E_abs[:, cs] = self.Z.T @ Y, aZ.T @ Ya
            if kind == "drop_pair" and arg[1] == c:
                i = int(arg[0])
                dropped = self.Zt[i].T @ Y[i * D:(i + 1) * D]
                assert labels[i] != c and np.any(dropped != 0)
        if kind == "drop_pair":
            ci, cs = slice(labels[int(arg[0])] * MC, (labels[int(arg[0])] + 1) * MC), slice(arg[1] * MC, (arg[1] + 1) * MC)
            E[ci, cs] -= dropped
            E[cs, ci] -= dropped.T
        for k in range(m):
            if E[k, k] == 0:
                E[k, k] = E_abs[k, k] = 1
        self.E, self.E_abs = E, E_abs
        # --- E^-1
        self.d = LD(1) / np.sqrt(np.diagonal(E))
        self.A = (E * self.d[:, None]) * self.d[None, :]
        self.cond = float(np.linalg.cond(self.A.astype(np.float64)))
        X, eye = np.linalg.inv(self.A.astype(np.float64)).astype(LD), np.eye(m, dtype=LD)
        best = None
        for _ in range(8):
            Rr = eye - self.A @ X
            res = float(np.max(np.abs(Rr)) / np.max(np.abs(self.A) @ np.abs(X)))
            if best is not None and not res < best[0]:
                break
            best = (res, X)
            X = X + X @ Rr
        self.einv_resid, X = best
        self.Einv = (X * self.d[:, None]) * self.d[None, :]
        if mutate is None:
            assert self.einv_resid < 1e-17, self.einv_resid

    def einv_distance(self, Einv):
        """|| I - A X ||_2 for X = an implementation's E^-1 taken to the equilibrated scale"""
        X = (np.asarray(Einv).astype(LD) / self.d[:, None]) / self.d[None, :]
        return float(np.linalg.norm((np.eye(self.m, dtype=LD) - self.A @ X).astype(np.float64), 2))

    def unscale(self, xt):
        """x = L^-T x~, [C,D]"""
        C, D = self.L.shape[0], self.L.shape[1]
        return np.einsum("cka,ck->ca", self.Li, xt.reshape(C, D))

    def iterates(self, precond, kmax, einv_used=None, recurrence="single", mutate=None):
        """x_0 .. x_kmax [kmax + 1, C, D] of the preconditioned CG on S~ x~ = L^-1 b, mapped back by L^-T.
        recurrence: "textbook" or "single" (the single-reduction form).  Also returns the coarse residual
        |Z~^T r_0'| / |Z~^T (L^-1 b)| behind the start (A-DEF2; 0 in exact arithmetic with the system's own E^-1)."""
        kind, arg = mutate if mutate is not None else (None, None)
        S, Z = self.St, self.Z
        Einv = self.Einv if einv_used is None else np.asarray(einv_used).astype(LD)
        Zp = Z
        if kind == "no_prolong":
            D = self.L.shape[1]
            Zp = Z.copy()
            Zp[int(arg) * D:(int(arg) + 1) * D] = 0

        def Q(r):
            return Zp @ (Einv @ (Z.T @ r))

        if precond == 1:
            def M(r):
                return r + Q(r)
            x = np.zeros_like(self.bt)
        else:
            def M(r):
                return r + Q(r - S @ r)
            x = Q(self.bt)
        r = self.bt - S @ x
        nz = np.sqrt(np.sum((Z.T @ self.bt) ** 2))
        coarse = float(np.sqrt(np.sum((Z.T @ r) ** 2)) / nz) if nz > 0 else 0.0
        xs = [x]
        if recurrence == "textbook":
            z = M(r)
            p, rz = z, r @ z
            for _ in range(kmax):
                Sp = S @ p
                alpha = rz / (p @ Sp)
                x, r = x + alpha * p, r - alpha * Sp
                z = M(r)
                rz, rz0 = r @ z, rz
                p = z + (rz / rz0) * p
                xs.append(x)
        else:
            u = M(r)
            w = S @ u
            p, s = np.zeros_like(u), np.zeros_like(u)
            gam_prev = alpha_prev = None
            for k in range(kmax):
                gam, dlt = r @ u, w @ u
                beta = LD(0) if k == 0 else gam / gam_prev
                alpha = gam / (dlt if k == 0 else dlt - beta * gam / alpha_prev)
                p, s = u + beta * p, w + beta * s
                x, r = x + alpha * p, r - alpha * s
                u = M(r)
                w = S @ u
                gam_prev, alpha_prev = gam, alpha
                xs.append(x)
        return np.stack([self.unscale(v) for v in xs]), coarse
