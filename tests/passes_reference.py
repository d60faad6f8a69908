"""An independent reference for the between-round passes (csrc/passes.hip, oracle/passes.py).  Test helper only.

oracle/passes.py restates cvUndistortPointsInternal and Camera.cam2img in the kernel's own operation order, so an error
both share is invisible to GPU-versus-oracle parity.  This module writes the same operations down once more, from the
reference project's scene/defs.py (Camera.set_params / img2cam / Distortion / cam2img, fisheye_from_normal,
normal_from_fisheye), processors/track_filter.py, utils/cost_function.py (through ba_reference._forward) and OpenCV's
published undistortPoints algorithm (calib3d, cvUndistortPointsInternal: K-normalize, then `iters` rounds of
x <- (x0 - delta(x)) * icdist(x), leaving with the K-normalized point when icdist < 0; default criteria COUNT 5, no
tilt, R = I, no P), in mpmath at MP_DPS digits.  It is not derived from oracle/passes.py or the kernel.

Every *_ref function returns, per item:
  * the value as a double-double pair (hi, lo): hi = the 50-digit value rounded to float64, lo = the rest, so that
    (got - hi) - lo is the error of a float64 `got` to ~32 digits;
  * `cond`, the conditioning figure: the largest change of the item's own 50-digit output when one input or parameter
    at a time moves up by one ulp of its storage type (float32 for float32 features, float64 for everything else).
    Inputs that are exactly zero are not moved (their ulp is the smallest subnormal; nothing changes at 50 digits).
    It comes from this reference alone;
  * which branch the item took, so a scene can assert that it reaches the branch it was built for.
bound() turns (value, cond) into the acceptance bound the tests use.

Float32 features.  Camera.img2cam keeps part of its arithmetic in float32 when the features are float32: cv2 returns
float32 points and normal_from_fisheye / the FOV factor then run in numpy float32.  img2cam_f32_path() replays those
steps with explicit np.float32 roundings (see the comments there for which operand has which type).
"""
import numpy as np
import mpmath as mp

from ba_reference import _forward, _rotate

MP_DPS = 50
EPSILON = 1e-10            # track_filter.py:3 and the constant of Camera.cam2img, as the double they are
SINGLE_FOCAL = (0, 2, 3, 8, 9)
FISHEYE = (5, 8, 9, 10)
NAN = float("nan")
EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)


def bound(cond, value, eps=EPS64, factor=16.0):
    """16 x (conditioning figure + eps |value|): a handful of rounded operations on the longest path, each at most
    eps/2 relative on a quantity of the output's size or an input-ulp's worth of the output's sensitivity."""
    return factor * (np.asarray(cond, dtype=np.float64) + eps * np.abs(np.asarray(value, dtype=np.float64)))


def _m(x):
    return mp.mpf(float(x))


def _isnan(x):
    return isinstance(x, float) and x != x or (isinstance(x, mp.mpf) and mp.isnan(x))


def _split(vals):
    """list of mpf / nan -> (hi, lo) float lists"""
    hi, lo = [], []
    for v in vals:
        if _isnan(v) or mp.isinf(v):
            hi.append(float(v))
            lo.append(0.0)
        else:
            h = float(v)
            hi.append(h)
            lo.append(float(v - mp.mpf(h)) if np.isfinite(h) else 0.0)
    return hi, lo


def ulp_of(x, f32=False):
    """spacing of x in its storage type, 0.0 for an exact zero (not moved)"""
    if x == 0:
        return 0.0
    return float(np.spacing(np.abs(np.float32(x)))) if f32 else float(np.spacing(abs(float(x))))


def conditioned(fn, inputs, ulps):
    """fn(list of mpf) -> list of mpf (or nan).  Returns (base outputs, cond)."""
    x = [_m(v) for v in inputs]
    base = fn(x)
    if any(_isnan(b) or mp.isinf(b) for b in base):
        return base, NAN
    cond = mp.mpf(0)
    for j, h in enumerate(ulps):
        if h == 0:
            continue
        out = fn(x[:j] + [x[j] + mp.mpf(h)] + x[j + 1:])
        if any(_isnan(o) or mp.isinf(o) for o in out):
            return base, float("inf")
        cond = max(cond, max(abs(o - b) for o, b in zip(out, base)))
    return base, float(cond)


# ------------------------------------------------------------------------------------------------------------
# Camera.set_params / img2cam
# ------------------------------------------------------------------------------------------------------------
def intrinsics(model, p):
    """(fx, fy, cx, cy) of Camera.set_params (defs.py:177-237)"""
    if model in SINGLE_FOCAL:
        return p[0], p[0], p[1], p[2]
    return p[0], p[1], p[2], p[3]


def dist_coeffs(model, p):
    """The cv2 vector (k1,k2,p1,p2,k3,k4,k5,k6,s1,s2,s3,s4) Camera.img2cam builds (defs.py:323-367) from self.k,
    self.p, self.sx as set_params fills them."""
    z = 0 * p[0]
    if model in (2, 8):
        k = [p[3]]
    elif model in (3, 9):
        k = [p[3], p[4]]
    elif model == 4:
        k = [p[4], p[5], p[6], p[7]]
    elif model == 5:                      # self.k = p[4:8]; [k0, k1, 0, 0, k2], the fourth is ignored
        k = [p[4], p[5], z, z, p[6]]
    elif model == 6:                      # self.k = [p4, p5, p8, p9, p10, p11], self.p = [p6, p7]
        k = [p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11]]
    elif model == 10:                     # self.k = [p4, p5, p8, p9], self.p = [p6, p7], self.sx = [p10, p11]
        k = [p[4], p[5], p[6], p[7], p[8], z, z, z, p[10], p[11], z, z]
    else:
        raise NotImplementedError(model)
    return k + [z] * (12 - len(k))


def cv_undistort(u, v, fx, fy, cx, cy, k, iters=5):
    """OpenCV's undistortPoints for one point.  Returns (x, y, exit) with exit = the 1-based iteration in which
    icdist < 0 ended the loop, 0 if all `iters` ran."""
    x = (u - cx) / fx
    y = (v - cy) / fy
    x0, y0 = x, y
    for j in range(iters):
        r2 = x * x + y * y
        den = 1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2
        if den == 0:
            return NAN, NAN, -1
        icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / den
        if icdist < 0:
            return x0, y0, j + 1
        dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
        dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
        x = (x0 - dx) * icdist
        y = (y0 - dy) * icdist
    return x, y, 0


def normal_from_fisheye(x, y):
    """defs.py:250-253: uv sin(theta) / (theta cos(theta)); 0/0 at uv = 0 is NaN there"""
    th = mp.sqrt(x * x + y * y)
    tc = th * mp.cos(th)
    if tc == 0:
        return NAN, NAN
    s = mp.sin(th)
    return x * s / tc, y * s / tc


FOV_EPS = 1e-4  # the literal of defs.py:285,343, a double


def fov_branch(omega2, r2):
    return 1 if omega2 < mp.mpf(FOV_EPS) else (2 if r2 < mp.mpf(FOV_EPS) else 3)


def img2cam(model, p, u, v):
    """Camera.img2cam (defs.py:315-369) of one pixel at working precision.  Returns (x, y, branch): branch is the
    icdist exit for the cv2 models, the FOV branch (1, 2, 3) for model 7, 0 otherwise."""
    fx, fy, cx, cy = intrinsics(model, p)
    if model == 0:
        f = (fx + fy) / 2                 # focal() = mean(focal_length)
        return (u - cx) / f, (v - cy) / f, 0
    if model == 1:
        return (u - cx) / fx, (v - cy) / fy, 0
    if model == 7:                        # r2 of the raw pixel, as written
        omega = p[4]
        r2 = u * u + v * v
        omega2 = omega * omega
        br = fov_branch(omega2, r2)
        if br == 1:
            factor = (omega2 * r2) / 3 - omega2 / 12 + 1
        elif br == 2:
            factor = (omega * (omega2 * r2 + 3)) / (6 * mp.tan(omega / 2))
        else:
            radius = mp.sqrt(r2)
            factor = mp.tan(radius * omega) / (radius * 2 * mp.tan(omega / 2))
        return (u - cx) / fx * factor, (v - cy) / fy * factor, br
    x, y, ex = cv_undistort(u, v, fx, fy, cx, cy, dist_coeffs(model, p))
    if ex >= 0 and model in FISHEYE:
        x, y = normal_from_fisheye(x, y)
    return x, y, ex


def ray_of(x, y):
    """undistort_process (image_undistortion.py:3-6): [x, y, 1] / ||[x, y, 1]||"""
    if _isnan(x) or _isnan(y):
        return [NAN, NAN, NAN]
    n = mp.sqrt(x * x + y * y + 1)
    return [x / n, y / n, 1 / n]


def _f32(x):
    return np.float32(float(x))


def img2cam_f32_path(model, p, u32, v32):
    """What Camera.img2cam returns for a float32 pixel under numpy 2 promotion, from the 50-digit quantities with the
    reference's own float32 roundings put in.  p: float64 parameters; returns (x, y, factor) as Python floats (factor:
    the FOV factor as float32, None for the other models).

    Models 0, 1: (xy - principal_point) / focal: float32 array minus float64 array is float64, so there is no
    float32 step; the value is the 50-digit one at the float32 pixel.
    cv2 models: cv2.undistortPoints computes in double and returns the array's type, float32: one rounding of the
    exact 5-iteration value.  normal_from_fisheye then runs on a float32 array: np.linalg.norm, np.cos, np.sin,
    the products and the quotient are all float32 (no float64 operand anywhere).
    """
    with mp.workdps(MP_DPS):
        pm = [_m(z) for z in p]
        u, v = _m(np.float32(u32)), _m(np.float32(v32))
        if model in (0, 1):
            x, y, _ = img2cam(model, pm, u, v)
            return float(x), float(y), None
        if model == 7:
            fx, fy, cx, cy = intrinsics(model, pm)
            omega = float(p[4])                      # Camera.omega: a Python float (params is a list of floats)
            omega2 = omega ** 2                      # Python float
            xy = np.array([u32, v32], dtype=np.float32)
            r2 = np.float32(np.sum(xy ** 2))         # float32 array ** Python int, summed in float32
            eps = FOV_EPS                            # Python float
            if omega2 < eps:                         # Python floats
                # omega2 (Python float, weak) * r2 (float32 array) -> float32; / 3 (Python int) -> float32;
                # omega2 / 12 is a Python float (weak), so the difference and the sum with 1 stay float32
                t = np.float32(np.float32(omega2) * r2)
                t = np.float32(t / np.float32(3))
                t = np.float32(t - np.float32(omega2 / 12))
                factor = np.float32(t + np.float32(1))
            elif r2 < np.float32(eps):               # float32 array < Python float (weak): compared in float32
                # omega2 * r2[mask] float32; + 3 float32; omega (Python float) * float32 array -> float32;
                # 6 * np.tan(omega / 2): np.tan of a Python float is an np.float64 scalar, so the denominator is
                # np.float64 and float32 array / np.float64 scalar is float64; storing into factor (float32,
                # zeros_like(r2)) rounds once more
                t = np.float32(np.float32(omega2) * r2)
                t = np.float32(t + np.float32(3))
                t = np.float32(np.float32(omega) * t)
                den = float(6 * mp.tan(_m(omega) / 2))             # np.float64 scalar
                factor = np.float32(float(t) / den)                # float64 quotient, stored as float32
            else:
                # radius = np.sqrt(float32 array) float32; radius * omega (Python float) float32; np.tan float32;
                # radius * 2 (Python int) float32; * np.tan(omega / 2) (np.float64 scalar) -> float64;
                # float32 / float64 -> float64, stored as float32
                radius = np.float32(np.sqrt(r2))
                arg = np.float32(radius * np.float32(omega))
                num = np.tan(np.array([arg], dtype=np.float32))[0]  # numpy's own float32 tan (not correctly rounded)
                den = float(np.float32(radius * np.float32(2))) * float(mp.tan(_m(omega) / 2))  # float64 product
                factor = np.float32(float(num) / den)
            # (xy - principal_point) / focal_length: float64 arrays on the right, so float64; * factor (float32
            # array) -> float64
            f = _m(factor)
            return float((u - cx) / fx * f), float((v - cy) / fy * f), float(factor)
        fx, fy, cx, cy = intrinsics(model, pm)
        x, y, ex = cv_undistort(u, v, fx, fy, cx, cy, dist_coeffs(model, pm))
        if ex < 0:
            return NAN, NAN, None
        x32, y32 = _f32(x), _f32(y)
        if model in FISHEYE:
            with np.errstate(all="ignore"):
                th = np.sqrt(np.array([np.float32(np.float32(x32 * x32) + np.float32(y32 * y32))], dtype=np.float32))
                tc = np.float32(th[0] * np.cos(th)[0])       # numpy's own float32 cos and sin, on arrays as there
                s = np.sin(th)[0]
                x32 = np.float32(np.float32(x32 * s) / tc)
                y32 = np.float32(np.float32(y32 * s) / tc)
        return float(x32), float(y32), None


def undistort_ref(cam_model, cam_params, feat_cam, xy):
    """Per feature: Camera.img2cam and the unit ray at 50 digits.  xy float32 or float64 [n, 2].
    dict: uv_hi/uv_lo [n,2], ray_hi/ray_lo [n,3], cond_uv [n], cond_ray [n], branch [n] (see img2cam), and for float32
    features uv32 [n,2] / factor32 [n] (img2cam_f32_path)."""
    xy = np.asarray(xy)
    f32 = xy.dtype == np.float32
    n = xy.shape[0]
    out = dict(uv_hi=np.zeros((n, 2)), uv_lo=np.zeros((n, 2)), ray_hi=np.zeros((n, 3)), ray_lo=np.zeros((n, 3)),
               cond_uv=np.zeros(n), cond_ray=np.zeros(n), branch=np.zeros(n, np.int64))
    if f32:
        out["uv32"] = np.zeros((n, 2))
        out["factor32"] = np.full(n, np.nan)
    with mp.workdps(MP_DPS):
        for i in range(n):
            c = int(feat_cam[i])
            model = int(cam_model[c])
            p = [float(z) for z in cam_params[c]]
            inputs = [float(xy[i, 0]), float(xy[i, 1])] + p
            ulps = [ulp_of(xy[i, 0], f32), ulp_of(xy[i, 1], f32)] + [ulp_of(z) for z in p]
            br = []

            def fn(a, model=model, br=br):
                x, y, b = img2cam(model, a[2:], a[0], a[1])
                br.append(b)
                return [x, y] + ray_of(x, y)

            base, _ = conditioned(fn, inputs, [0.0] * len(ulps))
            out["branch"][i] = br[0]
            if any(_isnan(b) for b in base):
                out["uv_hi"][i], out["ray_hi"][i] = np.nan, np.nan
                out["cond_uv"][i] = out["cond_ray"][i] = np.nan
            else:
                x = [_m(z) for z in inputs]
                cu, cr = mp.mpf(0), mp.mpf(0)
                for j, h in enumerate(ulps):
                    if h == 0:
                        continue
                    o = fn(x[:j] + [x[j] + mp.mpf(h)] + x[j + 1:])
                    if any(_isnan(z) for z in o):
                        cu = cr = mp.inf
                        break
                    cu = max(cu, abs(o[0] - base[0]), abs(o[1] - base[1]))
                    cr = max(cr, *(abs(o[2 + a] - base[2 + a]) for a in range(3)))
                hi, lo = _split(base)
                out["uv_hi"][i], out["uv_lo"][i] = hi[:2], lo[:2]
                out["ray_hi"][i], out["ray_lo"][i] = hi[2:], lo[2:]
                out["cond_uv"][i], out["cond_ray"][i] = float(cu), float(cr)
            if f32:
                x32, y32, fac = img2cam_f32_path(model, p, xy[i, 0], xy[i, 1])
                out["uv32"][i] = x32, y32
                if fac is not None:
                    out["factor32"][i] = fac
    return out


# ------------------------------------------------------------------------------------------------------------
# Camera.cam2img
# ------------------------------------------------------------------------------------------------------------
def cam2img(model, p, X, Y, Z):
    """Camera.cam2img (defs.py:371-412) with Distortion (:255-313) and fisheye_from_normal (:244-248) at working
    precision.  Returns (px, py, branch): branch 1/2/3 = the FOV branch, 4 = the fisheye clamp was active, else 0."""
    fx, fy, cx, cy = intrinsics(model, p)
    f = (fx + fy) / 2
    zz = Z + mp.mpf(EPSILON)
    if zz == 0:
        if X == 0 or Y == 0:
            return NAN, NAN, 0            # 0/0 in one coordinate: the norm of the difference is NaN
        return mp.inf, mp.inf, 0
    u, v = X / zz, Y / zz
    br = 0
    if model in FISHEYE:
        r = mp.sqrt(u * u + v * v)
        if r < mp.mpf(1e-8):
            r, br = mp.mpf(1e-8), 4
        th = mp.atan(r)
        u, v = u * th / r, v * th / r
    r2 = u * u + v * v
    if model == 0:
        return u * f + cx, v * f + cy, br
    if model == 1:
        return u * fx + cx, v * fy + cy, br
    if model in (2, 8):
        k = p[3]
        return (u + u * k * r2) * f + cx, (v + v * k * r2) * f + cy, br
    if model in (3, 9):
        k1, k2 = p[3], p[4]
        return (u + u * k1 * r2 + u * k2 * r2 ** 2) * f + cx, (v + v * k1 * r2 + v * k2 * r2 ** 2) * f + cy, br
    if model in (4, 6, 10):
        p1, p2 = p[6], p[7]               # self.p
        if model == 4:
            radial = p[4] * r2 + p[5] * r2 ** 2
        elif model == 6:                  # self.k = [p4, p5, p8, p9, p10, p11]
            radial = (1 + p[4] * r2 + p[5] * r2 ** 2 + p[8] * r2 ** 3) / (1 + p[9] * r2 + p[10] * r2 ** 2 + p[11] * r2 ** 3) - 1
        else:                             # self.k = [p4, p5, p8, p9]: k[2] = p8, the fourth ignored
            radial = p[4] * r2 + p[5] * r2 ** 2 + p[8] * r2 ** 3
        uv_ = u * v
        du = u * radial + 2 * p1 * uv_ + p2 * (r2 + 2 * u * u)    # self.p[::-1] on the second term
        dv = v * radial + 2 * p2 * uv_ + p1 * (r2 + 2 * v * v)
        if model == 10:
            du, dv = du + p[10] * r2, dv + p[11] * r2
        return (u + du) * fx + cx, (v + dv) * fy + cy, br
    if model == 5:                        # self.k = p[4:8], the fourth ignored
        radial = p[4] * r2 + p[5] * r2 ** 2 + p[6] * r2 ** 3
        return (u + u * radial) * fx + cx, (v + v * radial) * fy + cy, br
    if model == 7:                        # uv = Distortion(uv), not uv + Distortion(uv); the mean focal
        omega = p[4]
        omega2 = omega * omega
        br = fov_branch(omega2, r2)
        if br == 1:
            factor = (omega2 * r2) / 3 - omega2 / 12 + 1
        elif br == 2:
            t = mp.tan(omega / 2)
            factor = (-2 * t * (4 * r2 * t ** 2 - 3)) / (3 * omega)
        else:
            radius = mp.sqrt(r2)
            factor = mp.atan(radius * 2 * mp.tan(omega / 2)) / (radius * omega)
        return u * factor * f + cx, v * factor * f + cy, br
    raise NotImplementedError(model)


def _pc(W, X):
    """world2cam[:3] @ [X, 1]; W: 12 entries row-major (3 x 4)"""
    return [W[4 * r] * X[0] + W[4 * r + 1] * X[1] + W[4 * r + 2] * X[2] + W[4 * r + 3] for r in range(3)]


def _norm2(a, b):
    if _isnan(a) or _isnan(b):
        return NAN
    if mp.isinf(a) or mp.isinf(b):
        return mp.inf
    return mp.sqrt(a * a + b * b)


def _run(fn, inputs, ulps):
    base, cond = conditioned(fn, inputs, ulps)
    hi, lo = _split(base)
    return hi, lo, cond


def _obs_run(W, X, rest, rest_ulps, tail):
    """_run() for an observation: value = tail(world2cam[:3] @ [X, 1], rest).  The camera-frame point is linear in
    every entry of world2cam and of X, so a one-ulp move of one of them is applied to the point itself (W[r][c] + h
    moves pc[r] by h X[c]; X[c] + h moves pc by h W[:, c]) instead of forming the whole product again: the same
    perturbed value, a third of the work.  Returns (hi, lo, cond, depth)."""
    Wm, Xm, Rm = [_m(z) for z in W], [_m(z) for z in X], [_m(z) for z in rest]
    pc = _pc(Wm, Xm)
    base = tail(pc, Rm)
    hi, lo = _split(base)
    depth = float(pc[2])
    if any(_isnan(b) or mp.isinf(b) for b in base):
        return hi, lo, NAN, depth
    moves = []
    for r in range(3):
        for c in range(4):
            h = ulp_of(W[4 * r + c])
            if h:
                d = mp.mpf(h) * (Xm[c] if c < 3 else 1)
                moves.append(([pc[k] + d if k == r else pc[k] for k in range(3)], Rm))
    for c in range(3):
        h = ulp_of(X[c])
        if h:
            moves.append(([pc[k] + mp.mpf(h) * Wm[4 * k + c] for k in range(3)], Rm))
    for j, h in enumerate(rest_ulps):
        if h:
            moves.append((pc, Rm[:j] + [Rm[j] + mp.mpf(h)] + Rm[j + 1:]))
    cond = mp.mpf(0)
    for p2, r2 in moves:
        out = tail(p2, r2)
        if any(_isnan(o) or mp.isinf(o) for o in out):
            return hi, lo, float("inf"), depth
        cond = max(cond, abs(out[0] - base[0]))
    return hi, lo, float(cond), depth


def filter_reproj_pixel_ref(obs_img, obs_track, obs_feat, feats, img_cam, cam_model, cam_params, w2c, xyz):
    """FilterTracksByReprojection's per-observation quantities: err (hi, lo), depth, cond, branch."""
    feats = np.asarray(feats)
    f32 = feats.dtype == np.float32
    w2c = np.asarray(w2c, dtype=np.float64).reshape(-1, 16)
    n = len(obs_img)
    out = dict(err_hi=np.zeros(n), err_lo=np.zeros(n), cond=np.zeros(n), depth=np.zeros(n), branch=np.zeros(n, np.int64))
    with mp.workdps(MP_DPS):
        for i in range(n):
            im = int(obs_img[i])
            c = int(img_cam[im])
            model = int(cam_model[c])
            p = [float(z) for z in cam_params[c]]
            W = [float(z) for z in w2c[im][:12]]
            X = [float(z) for z in xyz[int(obs_track[i])]]
            ft = feats[int(obs_feat[i])]
            rest = [float(ft[0]), float(ft[1])] + p
            ulps = [ulp_of(ft[0], f32), ulp_of(ft[1], f32)] + [ulp_of(z) for z in p]
            br = []

            def tail(pc, a, model=model, br=br):
                px, py, b = cam2img(model, a[2:], *pc)
                br.append(b)
                if _isnan(px) or _isnan(py):
                    return [NAN]
                return [_norm2(px - a[0], py - a[1])]

            hi, lo, cond, depth = _obs_run(W, X, rest, ulps, tail)
            out["err_hi"][i], out["err_lo"][i], out["cond"][i], out["branch"][i] = hi[0], lo[0], cond, br[0]
            out["depth"][i] = depth
    return out


def filter_reproj_normalized_ref(obs_img, obs_track, obs_ray, w2c, xyz, rays):
    """FilterTracksByReprojectionNormalized (track_filter.py:48-55): err (hi, lo), depth, cond."""
    w2c = np.asarray(w2c, dtype=np.float64).reshape(-1, 16)
    n = len(obs_img)
    out = dict(err_hi=np.zeros(n), err_lo=np.zeros(n), cond=np.zeros(n), depth=np.zeros(n))
    with mp.workdps(MP_DPS):
        e = mp.mpf(EPSILON)
        for i in range(n):
            W = [float(z) for z in w2c[int(obs_img[i])][:12]]
            X = [float(z) for z in xyz[int(obs_track[i])]]
            r = [float(z) for z in rays[int(obs_ray[i])]]

            def tail(pc, a):
                pz, rz = pc[2] + e, a[2] + e
                if pz == 0 or rz == 0:
                    return [NAN]
                return [_norm2(pc[0] / pz - a[0] / rz, pc[1] / pz - a[1] / rz)]

            hi, lo, cond, depth = _obs_run(W, X, r, [ulp_of(z) for z in r], tail)
            out["err_hi"][i], out["err_lo"][i], out["cond"][i], out["depth"][i] = hi[0], lo[0], cond, depth
    return out


def filter_angle_ref(obs_img, obs_track, obs_ray, w2c, xyz, rays):
    """FilterTracksByAngle (track_filter.py:13-17): depth, and cos = (pt / ||pt||) . ray (hi, lo) with its cond;
    cos is computed for every observation, the depth test is the caller's."""
    w2c = np.asarray(w2c, dtype=np.float64).reshape(-1, 16)
    n = len(obs_img)
    out = dict(cos_hi=np.zeros(n), cos_lo=np.zeros(n), cond=np.zeros(n), depth=np.zeros(n))
    with mp.workdps(MP_DPS):
        for i in range(n):
            W = [float(z) for z in w2c[int(obs_img[i])][:12]]
            X = [float(z) for z in xyz[int(obs_track[i])]]
            r = [float(z) for z in rays[int(obs_ray[i])]]

            def tail(pc, a):
                nrm = mp.sqrt(pc[0] ** 2 + pc[1] ** 2 + pc[2] ** 2)
                if nrm == 0:
                    return [NAN]
                return [(pc[0] * a[0] + pc[1] * a[1] + pc[2] * a[2]) / nrm]

            hi, lo, cond, depth = _obs_run(W, X, r, [ulp_of(z) for z in r], tail)
            out["cos_hi"][i], out["cos_lo"][i], out["cond"][i], out["depth"][i] = hi[0], lo[0], cond, depth
    return out


def tri_angle_ref(track_ptr, obs_img, centers, xyz):
    """FilterTracksTriangulationAngle (track_filter.py:125-132) per track: the pairwise cosines of the directions
    (xyz - centre) / (norm + EPSILON) over the track's observations (a duplicated image contributes the same
    direction twice, which changes no pair's value).  Returns a list with, per track, (cos [L,L] float64,
    cond [L,L]): cond of pair (i, j) is the largest change of that cosine when one coordinate of the point or of
    either centre moves up one ulp."""
    res = []
    with mp.workdps(MP_DPS):
        e = mp.mpf(EPSILON)

        def unit(X, c):
            v = [X[a] - c[a] for a in range(3)]
            nrm = mp.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2) + e
            return [z / nrm for z in v]

        for t in range(len(track_ptr) - 1):
            ids = [int(obs_img[j]) for j in range(int(track_ptr[t]), int(track_ptr[t + 1]))]
            L = len(ids)
            X = [_m(z) for z in xyz[t]]
            C = [[_m(z) for z in centers[i]] for i in ids]
            U = [unit(X, c) for c in C]
            cosm = np.zeros((L, L))
            Uf = np.array([[float(z) for z in u] for u in U]).reshape(L, 3)
            for i in range(L):
                for j in range(i, L):
                    cosm[i, j] = cosm[j, i] = float(U[i][0] * U[j][0] + U[i][1] * U[j][1] + U[i][2] * U[j][2])
            # first-order changes of every direction: dC[i][a] for its own centre coordinate a, dX[i][a] for the point
            dC = np.zeros((L, 3, 3))
            dX = np.zeros((L, 3, 3))
            for i in range(L):
                for a in range(3):
                    h = ulp_of(float(centers[ids[i]][a]))
                    if h:
                        c2 = list(C[i])
                        c2[a] = c2[a] + mp.mpf(h)
                        dC[i, a] = [float(z - w) for z, w in zip(unit(X, c2), U[i])]
                    h = ulp_of(float(xyz[t][a]))
                    if h:
                        X2 = list(X)
                        X2[a] = X2[a] + mp.mpf(h)
                        dX[i, a] = [float(z - w) for z, w in zip(unit(X2, C[i]), U[i])]
            cond = np.zeros((L, L))
            if L:
                own = np.abs(np.einsum("iak,jk->aij", dC, Uf))          # centre of i moves: |dU_i . U_j|
                cond = np.maximum(own.max(0), own.max(0).T)
                both = np.abs(np.einsum("iak,jk->aij", dX, Uf) + np.einsum("jak,ik->aij", dX, Uf))
                cond = np.maximum(cond, both.max(0))
            res.append((cosm, cond))
    return res


def reproj_candidates_ref(model, cand_img, cand_track, cand_feat, feats, rows, pps, xyz):
    """complete_tracks' candidate test (track_retriangulation.py:58-90): reproject_funcs[model] (cost_function.py,
    through ba_reference._forward) with the image's row [t, q_xyzw, intrinsics without pp] and pp.  err (hi, lo),
    depth (z of the rotated point), cond."""
    feats = np.asarray(feats)
    f32 = feats.dtype == np.float32
    n = len(cand_img)
    out = dict(err_hi=np.zeros(n), err_lo=np.zeros(n), cond=np.zeros(n), depth=np.zeros(n))

    def g(r2):
        if r2 == 0:
            return NAN                    # arctan(r) / r at r = 0: 0/0 in the reference
        s = mp.sqrt(r2)
        return mp.atan(s) / s

    with mp.workdps(MP_DPS):
        for i in range(n):
            im = int(cand_img[i])
            row = [float(z) for z in rows[im]]
            S = len(row)
            pp = [float(z) for z in pps[im]]
            X = [float(z) for z in xyz[int(cand_track[i])]]
            ft = feats[int(cand_feat[i])]
            inputs = row + pp + X + [float(ft[0]), float(ft[1])]
            ulps = [ulp_of(z) for z in row + pp + X] + [ulp_of(ft[0], f32), ulp_of(ft[1], f32)]

            def fn(a, S=S):
                try:
                    x, y = _forward(model, a[S + 2:S + 5], a[0:3], a[3:7], a[7:S], a[S:S + 2], g)
                except (ZeroDivisionError, TypeError):
                    return [NAN]
                if _isnan(x) or _isnan(y):
                    return [NAN]
                return [_norm2(x - a[S + 5], y - a[S + 6])]

            hi, lo, cond = _run(fn, inputs, ulps)
            out["err_hi"][i], out["err_lo"][i], out["cond"][i] = hi[0], lo[0], cond
            a = [_m(z) for z in inputs]
            out["depth"][i] = float(_rotate(a[3:6], a[6], a[S + 2:S + 5])[2] + a[2])
    return out


def err_to(got, hi, lo):
    """|got - (hi + lo)| for finite references (float64 arrays)"""
    return np.abs((np.asarray(got, dtype=np.float64) - hi) - lo)
