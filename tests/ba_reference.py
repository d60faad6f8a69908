"""An independent reference for the BA linearization and cost.  Test helper only (CPU, no GPU, no C oracle).

The C oracle's distort() (oracle/ba_oracle.c) mirrors the kernel's distort<M> (csrc/ba_device.h) line for line, so
GPU-versus-oracle parity cannot see a wrong Jacobian coefficient that both share.  This module restates only the
forward model (oracle/projection_ref.reproject, models 0-6, 8, 9) and never writes a Jacobian down:

 * project():            the forward model in torch float64;
 * residual_jacobians(): r [N,2], Jc [N,2,D], Jp [N,2,3] from torch.autograd -- w.r.t. the point and the intrinsics
                         directly, w.r.t. the pose through the 6-vector d of the left retraction Exp([rho, phi]) * pose
                         at d = 0 (the small-angle series of Exp is exact to first order there);
 * mp_residual_jacobians(): the same for chosen observations in mpmath at 50 digits, derivatives from mpmath.diff of
                         the forward model.  atan(r)/r and its autograd derivative lose digits as r -> 0 (0/0 at r = 0);
                         here atan(r)/r at r2 == 0 is its limit 1 (so d/dr2 -> -1/3 comes out of the differences);
 * assemble():           numpy.longdouble sums of the Huber-weighted products W_o, V_p, g_p, U_c, g_c, loss and RMSE;
 * y_from(), colrel(), urel(): the comparison helpers shared by test_ba_reference.py and test_gpu_wide.py.
"""
import numpy as np
import torch

N_INTR = {0: 1, 1: 2, 2: 2, 3: 3, 4: 6, 5: 6, 6: 10, 8: 2, 9: 3}
N_FOCAL = {0: 1, 1: 2, 2: 1, 3: 1, 4: 2, 5: 2, 6: 2, 8: 1, 9: 1}
MODELS = tuple(sorted(N_INTR))
MP_DPS = 50


# ------------------------------------------------------------------------------------------------------------
# forward model, written once for any arithmetic: `ops` supplies cross-free scalar code on lists of components
# ------------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _rotate(qv, w, v):
    """v + 2 w (qv x v) + 2 qv x (qv x v) (rotate_quat without the translation), on component lists"""
    c1 = _cross(qv, v)
    c2 = _cross(qv, c1)
    return [v[i] + 2.0 * (w * c1[i] + c2[i]) for i in range(3)]


def _quat_mul(a, b):
    """Hamilton product, xyzw component lists"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
            aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz]


def _retract(t, q, d):
    """Exp([rho, phi]) * (t, q) with Exp's small-angle series: q_d = [phi (1/2 - th2/48), 1 - th2/8],
    tau = rho + phi x rho / 2 + phi x (phi x rho) / 6.  Only used at d = 0, for its first derivative."""
    rho, phi = d[:3], d[3:]
    th2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]
    s = 0.5 - th2 / 48.0
    qd = [phi[0] * s, phi[1] * s, phi[2] * s, 1.0 - th2 / 8.0]
    c1 = _cross(phi, rho)
    c2 = _cross(phi, c1)
    rt = _rotate(qd[:3], qd[3], t)
    return [rt[i] + rho[i] + c1[i] / 2.0 + c2[i] / 6.0 for i in range(3)], _quat_mul(qd, q)


def _distorted(model, u, v, k, atan_over_r):
    """distorted normalized coordinates of model `model` (cost_function.py:32-177 via projection_ref.reproject)"""
    if model in (0, 1):
        return u, v
    r2 = u * u + v * v
    if model == 2:
        h = 1.0 + k[0] * r2
        return u * h, v * h
    if model == 3:
        h = 1.0 + k[0] * r2 + k[1] * r2 ** 2
        return u * h, v * h
    if model in (4, 6):
        k1, k2, p1, p2 = k[0], k[1], k[2], k[3]
        if model == 4:
            radial = k1 * r2 + k2 * r2 ** 2
        else:
            k3, k4, k5, k6 = k[4], k[5], k[6], k[7]
            radial = (1.0 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1.0 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3) - 1.0
        uvp = u * v
        return (u + u * radial + 2.0 * p1 * uvp + p2 * (r2 + 2.0 * u ** 2),
                v + v * radial + 2.0 * p2 * uvp + p1 * (r2 + 2.0 * v ** 2))
    if model in (5, 8, 9):
        g = atan_over_r(r2)
        if model == 5:
            h = g * (1.0 + k[0] * r2 + k[1] * r2 ** 2 + k[2] * r2 ** 3)      # k4 is not used (cost_function.py:95)
        elif model == 8:
            h = g * (1.0 + k[0] * r2)
        else:
            h = g * (1.0 + k[0] * r2 + k[1] * r2 ** 2)
        return u * h, v * h
    raise NotImplementedError(model)


def _forward(model, X, t, q, intr, pp, atan_over_r):
    """pixel coordinates; every argument a list of components (torch columns or mpmath numbers)"""
    rx = _rotate(q[:3], q[3], X)
    pc = [rx[i] + t[i] for i in range(3)]
    u, v = pc[0] / pc[2], pc[1] / pc[2]
    nf = N_FOCAL[model]
    du, dv = _distorted(model, u, v, intr[nf:], atan_over_r)
    fx, fy = intr[0], intr[nf - 1]
    return du * fx + pp[0], dv * fy + pp[1]


def _cols(a):
    return [a[:, i] for i in range(a.shape[1])]


def _torch_g(r2):
    r = torch.sqrt(r2)
    return torch.atan(r) / r


def project(model, X, cam, pp):
    """pixel coordinates [N, 2] of points X [N, 3] in cameras cam [N, 7 + ni] = [t, q_xyzw, intrinsics-without-pp],
    principal points pp [N, 2]; torch float64 on the CPU.  NaN at r2 == 0 for the fisheye models, as the reference."""
    X, cam, pp = (torch.as_tensor(a, dtype=torch.float64) for a in (X, cam, pp))
    x, y = _forward(model, _cols(X), _cols(cam[:, 0:3]), _cols(cam[:, 3:7]), _cols(cam[:, 7:]), _cols(pp), _torch_g)
    return torch.stack([x, y], dim=1)


def residual_jacobians(model, X, cam, pp, uv):
    """(r [N,2], Jc [N,2,D], Jp [N,2,3]) float64 arrays; Jacobians from torch.autograd alone.  Observations are
    independent of each other, so the gradient of a component summed over them holds every observation's row."""
    X = torch.tensor(np.asarray(X), dtype=torch.float64, requires_grad=True)
    cam = torch.as_tensor(np.asarray(cam), dtype=torch.float64)
    intr = cam[:, 7:].clone().requires_grad_(True)
    d = torch.zeros((X.shape[0], 6), dtype=torch.float64, requires_grad=True)
    pp = torch.as_tensor(np.asarray(pp), dtype=torch.float64)
    t, q = _retract(_cols(cam[:, 0:3]), _cols(cam[:, 3:7]), _cols(d))
    x, y = _forward(model, _cols(X), t, q, _cols(intr), _cols(pp), _torch_g)
    proj = torch.stack([x, y], dim=1)
    Jc, Jp = [], []
    for a in range(2):
        gX, gd, gi = torch.autograd.grad(proj[:, a].sum(), [X, d, intr], retain_graph=True)
        Jp.append(gX)
        Jc.append(torch.cat([gd, gi], dim=1))
    r = proj.detach().numpy() - np.asarray(uv, dtype=np.float64)
    return r, torch.stack(Jc, dim=1).numpy(), torch.stack(Jp, dim=1).numpy()


def mp_residual_jacobians(model, X, cam, pp, uv, dps=MP_DPS):
    """residual_jacobians() in mpmath at `dps` digits: each of the 3 + 6 + ni derivatives is mpmath.diff of the
    forward model along that parameter.  Slow: meant for a few dozen chosen observations."""
    import mpmath as mp
    X, cam, pp, uv = (np.asarray(a, dtype=np.float64) for a in (X, cam, pp, uv))
    n, ni = X.shape[0], N_INTR[model]
    D = 6 + ni
    r, Jc, Jp = np.zeros((n, 2)), np.zeros((n, 2, D)), np.zeros((n, 2, 3))

    def g(r2):
        if r2 == 0:
            return mp.mpf(1)
        s = mp.sqrt(r2)
        return mp.atan(s) / s

    with mp.workdps(dps):
        for i in range(n):
            base = [mp.mpf(float(z)) for z in np.concatenate([X[i], np.zeros(6), cam[i, 7:]])]
            t0, q0, p0 = ([mp.mpf(float(z)) for z in a] for a in (cam[i, 0:3], cam[i, 3:7], pp[i]))

            def f(params, a):
                t, q = _retract(t0, q0, params[3:9])
                return _forward(model, params[0:3], t, q, params[9:], p0, g)[a]

            for a in range(2):
                r[i, a] = float(f(base, a) - mp.mpf(float(uv[i, a])))
                for j in range(3 + D):
                    def along(z, j=j, a=a):
                        return f(base[:j] + [z] + base[j + 1:], a)
                    val = float(mp.diff(along, base[j]))
                    if j < 3:
                        Jp[i, a, j] = val
                    else:
                        Jc[i, a, j - 3] = val
    return r, Jc, Jp


def reference_obs(prob, cams, pts, mp_mask=None):
    """(r, Jc, Jp) of every observation of `prob` at (cams, pts): autograd, and mpmath where mp_mask is set"""
    cam_idx, pt_idx = np.asarray(prob.cam_idx), np.asarray(prob.pt_idx)
    args = (pts[pt_idx], cams[cam_idx], prob.pp[cam_idx], prob.uv)
    r, Jc, Jp = residual_jacobians(prob.model, *args)
    if mp_mask is not None and np.any(mp_mask):
        sel = np.flatnonzero(mp_mask)
        r[sel], Jc[sel], Jp[sel] = mp_residual_jacobians(prob.model, *(a[sel] for a in args))
    return r, Jc, Jp


# ------------------------------------------------------------------------------------------------------------
# assembly in numpy.longdouble
# ------------------------------------------------------------------------------------------------------------
def assemble(r, Jc, Jp, cam_idx, pt_idx, n_cams, n_points, delta=1.0):
    """The Huber-weighted normal-equation blocks (pypose Huber + Triggs corrector: w = 1 if ||r|| < delta else
    delta / ||r||; r~ = sqrt(w) r, J~ = sqrt(w) J) and the cost, summed in longdouble:
    W [N,D,3] = J~c^T J~p, V [P,6] packed (xx xy xz yy yz zz), gp [P,3] = -sum J~p^T r~, U [C,D,D], gc [C,D] =
    -sum J~c^T r~, loss = sum huber(||r||^2), rmse = sqrt(sum ||r||^2 / N), beyond = mask of ||r|| >= delta."""
    L = np.longdouble
    r, Jc, Jp = (np.asarray(a).astype(L) for a in (r, Jc, Jp))
    cam_idx, pt_idx = np.asarray(cam_idx), np.asarray(pt_idx)
    N, D = r.shape[0], Jc.shape[2]
    delta = L(delta)
    s = np.sum(r * r, axis=1)
    rs = np.sqrt(s)
    inside = rs < delta
    sw = np.sqrt(np.where(inside, L(1), delta / np.where(inside, L(1), rs)))
    rt, Jct, Jpt = r * sw[:, None], Jc * sw[:, None, None], Jp * sw[:, None, None]
    W = np.einsum("nad,nak->ndk", Jct, Jpt)
    Vfull = np.zeros((n_points, 3, 3), dtype=L)
    np.add.at(Vfull, pt_idx, np.einsum("naj,nak->njk", Jpt, Jpt))
    gp = np.zeros((n_points, 3), dtype=L)
    np.add.at(gp, pt_idx, -np.einsum("naj,na->nj", Jpt, rt))
    U = np.zeros((n_cams, D, D), dtype=L)
    np.add.at(U, cam_idx, np.einsum("nad,nae->nde", Jct, Jct))
    gc = np.zeros((n_cams, D), dtype=L)
    np.add.at(gc, cam_idx, -np.einsum("nad,na->nd", Jct, rt))
    V = np.stack([Vfull[:, 0, 0], Vfull[:, 0, 1], Vfull[:, 0, 2], Vfull[:, 1, 1], Vfull[:, 1, 2], Vfull[:, 2, 2]], axis=1)
    loss = np.sum(np.where(inside, s, L(2) * delta * rs - delta * delta))
    return dict(W=W, V=V, gp=gp, U=U, gc=gc, loss=float(loss), rmse=float(np.sqrt(np.sum(s) / L(N))), beyond=~inside)


def y_from(W, V, pt_idx, f, clamp_min=1e-6, clamp_max=1e32):
    """What test_gpu_parity.y_records does, from arrays: W_o [N,D,3] and packed V_p [P,6] turned into the GPU's stored
    records Y_o = W_o R_p^-T, R_p = chol(V_p with its diagonal clamped and multiplied by f)."""
    W, V = np.asarray(W, dtype=np.float64), np.asarray(V, dtype=np.float64)
    full = np.empty((V.shape[0], 3, 3))
    for k, (a, b) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
        full[:, a, b] = full[:, b, a] = V[:, k]
    for a in range(3):
        full[:, a, a] = np.clip(full[:, a, a], clamp_min, clamp_max) * f
    Ri = np.linalg.inv(np.linalg.cholesky(full))
    return np.einsum("oak,ojk->oaj", W, Ri[np.asarray(pt_idx)])


def v_cond(V):
    """condition number of every packed 3x3 block of V [P,6]"""
    V = np.asarray(V, dtype=np.float64)
    full = np.empty((V.shape[0], 3, 3))
    for k, (a, b) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
        full[:, a, b] = full[:, b, a] = V[:, k]
    return np.linalg.cond(full)


def colrel(got, exp, axis=-1):
    """max over the columns along `axis` of max|got - exp| / max|exp|, each column scaled by itself, so a column of
    small entries (a focal column ~0.3 next to rotation columns ~1e4) is held to its own size.  A column that is
    exactly zero in exp (the ignored k4 of OPENCV_FISHEYE) must be exactly zero in got: inf otherwise."""
    got = np.moveaxis(np.asarray(got, dtype=np.longdouble), axis, -1)
    exp = np.moveaxis(np.asarray(exp, dtype=np.longdouble), axis, -1)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    got, exp = got.reshape(-1, got.shape[-1]), exp.reshape(-1, exp.shape[-1])
    if not (np.all(np.isfinite(got)) and np.all(np.isfinite(exp))):
        return float("inf")
    err, scale = np.max(np.abs(got - exp), axis=0), np.max(np.abs(exp), axis=0)
    worst = 0.0
    for e, s in zip(err, scale):
        worst = max(worst, (0.0 if e == 0 else float("inf")) if s == 0 else float(e / s))
    return worst


def urel(got, exp):
    """colrel for the camera blocks U [C,D,D] on rows and columns both: entry (a, b) is scaled by
    sqrt(max|U_aa| max|U_bb|); where that scale is zero the entry must be exactly zero."""
    got, exp = np.asarray(got, dtype=np.longdouble), np.asarray(exp, dtype=np.longdouble)
    assert got.shape == exp.shape and got.shape[-1] == got.shape[-2]
    if not (np.all(np.isfinite(got)) and np.all(np.isfinite(exp))):
        return float("inf")
    d = np.sqrt(np.max(np.abs(np.diagonal(exp, axis1=-2, axis2=-1)), axis=0))
    scale = d[:, None] * d[None, :]
    err = np.max(np.abs(got - exp), axis=0)
    if np.any((scale == 0) & (err != 0)):
        return float("inf")
    return float(np.max(err / np.where(scale == 0, 1, scale)))
