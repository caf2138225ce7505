"""EXACT reference of the camera model and of the sums the LM step is made of -- test infrastructure, NOT product code.

Written from the DEFINITION of the model, in mpmath at a fixed precision: Rodrigues through sin / cos of theta (identity at
theta = 0), pinhole divide, two radial terms, OpenCV's tangential term for the 13-parameter rows, one focal length, principal
point; residual = w * (project - uv).  The derivatives are central differences IN MPMATH with a step far below float64
resolution (default: 80 digits, h = 1e-25; truncation ~ h^2 = 1e-50 relative, rounding ~ 1e-80 / h = 1e-55), so none of
the a / b / a2 / b2 series and none of the closed-form derivative formulas of sba_model.hpp or oracle/lm_schur_model.py is
in here: an error shared by those two cannot agree with this file.  Inputs are taken as the exact float64 values they
are; every returned number is rounded to float64 once.

What it pins (tests/test_exact_model_host.py pins this file first; tests/test_gpu_exact_model.py then pins the device):
  exact_blocks   r (M,2), Jc (M,2,NCP), Jp (M,2,3)
  robust_rows    the header's IRLS rule: rows and residual components scaled by sqrt(rho'(z)), z = (r / f_scale)^2
  normal_sums    diagU, g_c, g_p, V, cost, each with the sum of the magnitudes of its terms
  wt_dc          W_p^T dc = sum over the point's observations of Jp^T (Jc dc), with its term magnitudes
  point_step     (V_p + lam diag D_p) dp = -(g_p + W_p^T dc), fixed points exactly zero
  reduced_system S = blockdiag(U_c) - sum W_p V'_p^-1 W_p^T (not damped in the cameras) and rhs = -g_c + sum W_p V'_p^-1 g_p over the
                 free points, V'_p = V_p + lam diag D_p, with d = sqrt(diag U) and the magnitudes of their terms
  tie_matrix     T of delta_c = T delta_s, the shared-intrinsics unknowns in the order of pySBA.py:313
  tied_system    S_s = T^T S T, rhs_s = T^T rhs, diagU_s = T^T diagU, g_s = T^T g_c
  sq_system      the squared-pixel-error variants: rho = w Delta^2, rows J~ = 2 w Delta dDelta/dtheta per camera (cameras only) or
                 J~ = 2 w Delta (dDelta/dX) (x) [X, 1] (one 3 x 4 affine for all points), H = J~^T J~, g = J~^T rho, cost = 0.5 rho . rho
About 1 ms per observation (the seven rotations a camera needs are built once per camera).
"""
from __future__ import annotations

import mpmath as mp
import numpy as np

DPS = 80            # decimal digits of every mpmath evaluation
H_DIGITS = 25       # central-difference step h = 10^-H_DIGITS
ZERO_DIGITS = 30    # a difference quotient below 10^-ZERO_DIGITS of the pixel value is an exact zero of the derivative
SUM_DPS = 50        # products of two float64 values (106 bits) and their sums are exact at this precision


def _mpf(v):
    return v if isinstance(v, mp.mpf) else mp.mpf(float(v))


# ----------------------------------------------------------------------------- the model, from its definition
def rotation(rho):
    """(cos t, sin t, unit axis) of the rotation vector rho, or None for rho = 0 (the identity)."""
    th2 = rho[0] * rho[0] + rho[1] * rho[1] + rho[2] * rho[2]
    if th2 == 0:
        return None
    th = mp.sqrt(th2)
    return mp.cos(th), mp.sin(th), [r / th for r in rho]


def rotate(rot, X):
    """Rodrigues: cos t X + sin t (k x X) + (1 - cos t) (k . X) k."""
    if rot is None:
        return list(X)
    c, s, k = rot
    kx = [k[1] * X[2] - k[2] * X[1], k[2] * X[0] - k[0] * X[2], k[0] * X[1] - k[1] * X[0]]
    kd = k[0] * X[0] + k[1] * X[1] + k[2] * X[2]
    return [c * X[i] + s * kx[i] + (1 - c) * kd * k[i] for i in range(3)]


def pixel(p, intr):
    """Camera-frame point p -> pixel.  intr = [f, k1, k2, cx, cy] or [f, k1, k2, p1, p2, cx, cy]."""
    f, k1, k2 = intr[0], intr[1], intr[2]
    p1, p2 = (intr[3], intr[4]) if len(intr) == 7 else (0, 0)
    cx, cy = intr[-2], intr[-1]
    x, y = p[0] / p[2], p[1] / p[2]
    n = x * x + y * y
    d = 1 + k1 * n + k2 * n * n
    xd = x * d + 2 * p1 * x * y + p2 * (n + 2 * x * x)
    yd = y * d + p1 * (n + 2 * y * y) + 2 * p2 * x * y
    return f * xd + cx, f * yd + cy


def project(cam_row, X):
    """One 11- or 13-parameter camera row and one world point -> (u, v), in mpmath at the CURRENT precision."""
    cam = [_mpf(v) for v in cam_row]
    X = [_mpf(v) for v in X]
    if len(cam) not in (11, 13):
        raise ValueError("camera rows have 11 or 13 parameters")
    P = rotate(rotation(cam[0:3]), X)
    return pixel([P[i] + cam[3 + i] for i in range(3)], cam[6:])


def series_digits(dps=DPS, h_digits=H_DIGITS):
    """Correct decimal digits of (1 - cos h) / h^2 at this precision and step (the rotation term that cancels hardest)."""
    with mp.workdps(dps):
        h = mp.mpf(10) ** -h_digits
        got = (1 - mp.cos(h)) / (h * h)
    with mp.workdps(4 * dps):
        h = mp.mpf(10) ** -h_digits
        ref = (1 - mp.cos(h)) / (h * h)
        err = abs(got - ref) / ref
        return float(-mp.log10(err)) if err != 0 else float(dps)


def _indices(ci, pi):
    return np.asarray(ci).reshape(-1).astype(np.int64), np.asarray(pi).reshape(-1).astype(np.int64)


def _weights(w, M):
    wv = np.ones(M) if w is None else np.asarray(w, dtype=np.float64).reshape(-1)
    return np.full(M, wv[0]) if wv.size == 1 else wv


def exact_residual(cams, pts, uv, ci, pi, w=None, dps=DPS):
    """r (M,2) = w (project - uv) alone."""
    ci, pi = _indices(ci, pi)
    wv = _weights(w, ci.size)
    r = np.zeros((ci.size, 2))
    with mp.workdps(dps):
        rots = {}
        for m in range(ci.size):
            c = int(ci[m])
            if c not in rots:
                cam = [_mpf(v) for v in cams[c]]
                rots[c] = (cam, rotation(cam[0:3]))
            cam, rot = rots[c]
            P = rotate(rot, [_mpf(v) for v in pts[pi[m]]])
            u, v = pixel([P[i] + cam[3 + i] for i in range(3)], cam[6:])
            wm = _mpf(wv[m])
            r[m] = float(wm * (u - _mpf(uv[m, 0]))), float(wm * (v - _mpf(uv[m, 1])))
    return r


def camera_points(cams, pts, ci, pi, dps=DPS):
    """(M,3) camera-frame points R X + t."""
    ci, pi = _indices(ci, pi)
    out = np.zeros((ci.size, 3))
    with mp.workdps(dps):
        for m in range(ci.size):
            cam = [_mpf(v) for v in cams[ci[m]]]
            P = rotate(rotation(cam[0:3]), [_mpf(v) for v in pts[pi[m]]])
            out[m] = [float(P[i] + cam[3 + i]) for i in range(3)]
    return out


def exact_blocks(cams, pts, uv, ci, pi, w=None, dps=DPS, h_digits=H_DIGITS):
    """r (M,2), Jc (M,2,NCP), Jp (M,2,3) of w (project - uv): central differences in mpmath, rounded once to float64."""
    cams = np.asarray(cams, dtype=np.float64)
    pts = np.asarray(pts, dtype=np.float64)
    ci, pi = _indices(ci, pi)
    M, ncp = ci.size, cams.shape[1]
    wv = _weights(w, M)
    r, Jc, Jp = np.zeros((M, 2)), np.zeros((M, 2, ncp)), np.zeros((M, 2, 3))
    with mp.workdps(dps):
        h = mp.mpf(10) ** -h_digits
        inv2h = 1 / (2 * h)
        zero_below = mp.mpf(10) ** -ZERO_DIGITS
        percam = {}
        for m in range(M):
            c = int(ci[m])
            if c not in percam:         # the rotation and its six displaced neighbours depend on the camera alone
                cam = [_mpf(v) for v in cams[c]]
                rots = []
                for k in range(3):
                    ra, rb = list(cam[0:3]), list(cam[0:3])
                    ra[k] += h
                    rb[k] -= h
                    rots.append((rotation(ra), rotation(rb)))
                percam[c] = (cam, rotation(cam[0:3]), rots)
            cam, rot0, rots = percam[c]
            t, intr = cam[3:6], cam[6:]
            X = [_mpf(v) for v in pts[pi[m]]]
            wm = _mpf(wv[m])
            P = rotate(rot0, X)
            p = [P[i] + t[i] for i in range(3)]
            u, v = pixel(p, intr)
            r[m] = float(wm * (u - _mpf(uv[m, 0]))), float(wm * (v - _mpf(uv[m, 1])))
            for k in range(ncp + 3):
                if k < 3:
                    Pa, Pb = rotate(rots[k][0], X), rotate(rots[k][1], X)
                    a = pixel([Pa[i] + t[i] for i in range(3)], intr)
                    b = pixel([Pb[i] + t[i] for i in range(3)], intr)
                elif k < 6:             # p = R X + t: a step in t is the same step in p
                    pa, pb = list(p), list(p)
                    pa[k - 3] += h
                    pb[k - 3] -= h
                    a, b = pixel(pa, intr), pixel(pb, intr)
                elif k < ncp:
                    ia, ib = list(intr), list(intr)
                    ia[k - 6] += h
                    ib[k - 6] -= h
                    a, b = pixel(p, ia), pixel(p, ib)
                else:
                    Xa, Xb = list(X), list(X)
                    Xa[k - ncp] += h
                    Xb[k - ncp] -= h
                    Pa, Pb = rotate(rot0, Xa), rotate(rot0, Xb)
                    a = pixel([Pa[i] + t[i] for i in range(3)], intr)
                    b = pixel([Pb[i] + t[i] for i in range(3)], intr)
                du, dv = wm * (a[0] - b[0]) * inv2h, wm * (a[1] - b[1]) * inv2h
                # an exact zero of the derivative (a point on the optical axis) comes out as the difference's truncation, ~h^2 of
                # the third derivative: anything below 10^-ZERO_DIGITS of the pixel's own size per unit step is that zero
                du = 0.0 if abs(du) < zero_below * abs(u) else float(du)
                dv = 0.0 if abs(dv) < zero_below * abs(v) else float(dv)
                if k < ncp:
                    Jc[m, 0, k], Jc[m, 1, k] = du, dv
                else:
                    Jp[m, 0, k - ncp], Jp[m, 1, k - ncp] = du, dv
    return r, Jc, Jp


# ----------------------------------------------------------------------------- robust loss (scipy's rho, the header's IRLS rows)
def rho_functions(z, loss):
    """(rho(z), rho'(z)) of scipy.optimize.least_squares' losses, from their definitions, in mpmath."""
    z = _mpf(z)
    if loss == "linear":
        return z, mp.mpf(1)
    if loss == "huber":
        return (z, mp.mpf(1)) if z <= 1 else (2 * mp.sqrt(z) - 1, 1 / mp.sqrt(z))
    if loss == "soft_l1":
        return 2 * (mp.sqrt(1 + z) - 1), 1 / mp.sqrt(1 + z)
    if loss == "cauchy":
        return mp.log(1 + z), 1 / (1 + z)
    raise ValueError("loss must be 'linear', 'huber', 'soft_l1' or 'cauchy'")


def robust_rows(r, Jc, Jp, loss, f_scale):
    """Rows and residual components scaled by sqrt(rho'((r / f_scale)^2)).
    Returns r_s, Jc_s, Jp_s, cost_terms (M,2) with cost = 0.5 sum cost_terms (f_scale^2 rho(z); r^2 for the linear loss),
    and the scale (M,2) itself."""
    r = np.asarray(r, dtype=np.float64)
    if loss in (None, "linear") or not f_scale > 0:
        with mp.workdps(SUM_DPS):
            terms = np.array([[float(_mpf(v) ** 2) for v in row] for row in r])
        return r.copy(), Jc.copy(), Jp.copy(), terms, np.ones_like(r)
    rs, Jcs, Jps = r.copy(), Jc.copy(), Jp.copy()
    terms, scale = np.zeros_like(r), np.ones_like(r)
    with mp.workdps(SUM_DPS):
        delta = _mpf(f_scale)
        for m in range(r.shape[0]):
            for k in range(2):
                rho, drho = rho_functions((_mpf(r[m, k]) / delta) ** 2, loss)
                s = mp.sqrt(drho)
                terms[m, k] = float(delta * delta * rho)
                scale[m, k] = float(s)
                if s != 1:
                    rs[m, k] = float(s * _mpf(r[m, k]))
                    Jcs[m, k] = [float(s * _mpf(v)) for v in Jc[m, k]]
                    Jps[m, k] = [float(s * _mpf(v)) for v in Jp[m, k]]
    return rs, Jcs, Jps, terms, scale


# ----------------------------------------------------------------------------- sums of products
def _dot(a, b):
    return float(mp.fdot([_mpf(x) for x in a], [_mpf(y) for y in b]))


def normal_sums(r, Jc, Jp, ci, pi, n_cams, n_pts, cost_terms=None, r_slack=None):
    """diagU (C,NCP), gc (C,NCP), gp (N,3), V (N,3,3) and cost of the given blocks, summed exactly and rounded once, with the
    magnitudes of their terms: gc_mag / gp_mag = sum |J_ij| (|r_i| + r_slack_i), V_mag = sum |J_ij J_ik| (diagU and diag V are
    their own), cost_mag = 0.5 sum |r_i| (|r_i| + r_slack_i) ... for the robust losses 0.5 sum of the cost terms."""
    ci, pi = _indices(ci, pi)
    M, ncp = ci.size, Jc.shape[2]
    slack = np.zeros((M, 2)) if r_slack is None else np.broadcast_to(np.asarray(r_slack, dtype=np.float64).reshape(M, -1), (M, 2))
    ra = np.abs(r) + slack
    out = dict(diagU=np.zeros((n_cams, ncp)), gc=np.zeros((n_cams, ncp)), gc_mag=np.zeros((n_cams, ncp)),
               gp=np.zeros((n_pts, 3)), gp_mag=np.zeros((n_pts, 3)), V=np.zeros((n_pts, 3, 3)), V_mag=np.zeros((n_pts, 3, 3)))
    with mp.workdps(SUM_DPS):
        for c in range(n_cams):
            sel = np.nonzero(ci == c)[0]
            rr, aa = r[sel].ravel(), ra[sel].ravel()
            for k in range(ncp):
                col = Jc[sel, :, k].ravel()
                out["diagU"][c, k] = _dot(col, col)
                out["gc"][c, k] = _dot(col, rr)
                out["gc_mag"][c, k] = _dot(np.abs(col), aa)
        for p in range(n_pts):
            sel = np.nonzero(pi == p)[0]
            rr, aa = r[sel].ravel(), ra[sel].ravel()
            for k in range(3):
                col = Jp[sel, :, k].ravel()
                out["gp"][p, k] = _dot(col, rr)
                out["gp_mag"][p, k] = _dot(np.abs(col), aa)
                for j in range(k, 3):
                    cj = Jp[sel, :, j].ravel()
                    out["V"][p, k, j] = out["V"][p, j, k] = _dot(col, cj)
                    out["V_mag"][p, k, j] = out["V_mag"][p, j, k] = _dot(np.abs(col), np.abs(cj))
        if cost_terms is None:
            out["cost"] = 0.5 * _dot(r.ravel(), r.ravel())
        else:
            out["cost"] = 0.5 * float(mp.fsum([_mpf(v) for v in np.asarray(cost_terms).ravel()]))
        out["cost_mag"] = 0.5 * _dot(np.abs(r).ravel(), ra.ravel())
    return out


def wt_dc(Jc, Jp, ci, pi, dc, n_pts):
    """t (N,3) = sum over each point's observations of Jp^T (Jc dc_cam), and t_mag = sum |Jp|^T (|Jc| |dc_cam|)."""
    ci, pi = _indices(ci, pi)
    dc = np.asarray(dc, dtype=np.float64).reshape(-1, Jc.shape[2])
    t, t_mag = np.zeros((n_pts, 3)), np.zeros((n_pts, 3))
    with mp.workdps(SUM_DPS):
        s = [[mp.fdot([_mpf(x) for x in Jc[m, k]], [_mpf(y) for y in dc[ci[m]]]) for k in range(2)] for m in range(ci.size)]
        sa = [[mp.fdot([_mpf(abs(x)) for x in Jc[m, k]], [_mpf(abs(y)) for y in dc[ci[m]]]) for k in range(2)] for m in range(ci.size)]
        for p in range(n_pts):
            sel = np.nonzero(pi == p)[0]
            for j in range(3):
                t[p, j] = float(mp.fsum([_mpf(Jp[m, k, j]) * s[m][k] for m in sel for k in range(2)]))
                t_mag[p, j] = float(mp.fsum([_mpf(abs(Jp[m, k, j])) * sa[m][k] for m in sel for k in range(2)]))
    return t, t_mag


def damping_diagonal(V):
    """D (N,3) of the FIRST linearisation: diag V with zeros replaced by 1 (ModelEngine.linearize)."""
    d = np.einsum("nii->ni", V)
    return np.where(d > 0, d, 1.0)


def point_step(V, gp, wtdc, lam, D, fixed=None):
    """dp (N,3): (V_p + lam diag D_p) dp = -(g_p + W_p^T dc), solved in mpmath; fixed points get exactly zero."""
    N = V.shape[0]
    dp = np.zeros((N, 3))
    with mp.workdps(SUM_DPS):
        lam = _mpf(lam)
        for p in range(N):
            if fixed is not None and fixed[p]:
                continue
            A = mp.matrix(3, 3)
            for i in range(3):
                for j in range(3):
                    A[i, j] = _mpf(V[p, i, j]) + (lam * _mpf(D[p, i]) if i == j else 0)
            b = mp.matrix([-(_mpf(gp[p, i]) + _mpf(wtdc[p, i])) for i in range(3)])
            x = mp.lu_solve(A, b)
            dp[p] = [float(x[i]) for i in range(3)]
    return dp


# ----------------------------------------------------------------------------- the reduced camera system
def _ld(x):
    """mpf -> np.longdouble (two float64 pieces: 64 mantissa bits survive)."""
    hi = float(x)
    return np.longdouble(hi) + np.longdouble(float(x - mp.mpf(hi)))


def _chol3_inv(A):
    """Inverse of the lower Cholesky factor of a 3 x 3 mpmath matrix (rows of L^-1)."""
    return mp.inverse(mp.cholesky(A))


def reduced_system(Jc, Jp, r, ci, pi, n_cams, n_pts, lam, fixed=None, full_mp=False):
    """The reduced camera system of the given (robust-scaled) blocks, as the exchange buffer holds it (NOT damped in the cameras):
        S   = blockdiag(U_c) - sum over free p of W_p V'_p^-1 W_p^T,    V'_p = V_p + lam diag D_p,  D_p = diag V_p (zeros -> 1)
        rhs = -g_c + sum over free p of W_p V'_p^-1 g_p
    (fixed points contribute nothing to the sums; their observations still count in U and g_c).  U, g_c, V, g_p, D, the W blocks
    Jc^T Jp, the 3 x 3 Cholesky factor of V'_p, Z = W L^-T, x_p = V'^-1 g_p and the whole of rhs are formed in mpmath; the sum
    S -= Z_i Z_j^T alone runs in np.longdouble.  Its terms are bounded by Cauchy-Schwarz: sum_p |Z_i| |Z_j|^T <= d_i d_j because
    sum_p Z_i Z_i^T <= U_ii, so a sum of N three-term products in longdouble stays below (N + 3) 2^-63 d_i d_j, 0.03 eps64 d_i d_j
    at 50 points (tests/test_exact_model_host.py holds it to 0.1 against full_mp=True, which forms V'^-1 by mpmath's LU inverse,
    W V'^-1 W^T as it stands and every sum in mpmath: in common are only the sums of products of float64 values U, V, g and
    W = Jc^T Jp, which are exact at this precision).
    Returns dict: S (n,n) float64 and S_ld, the same before its one rounding, rhs (n,), d = sqrt(diag U) with zeros replaced by 1,
    S_mag = sum |Jc_i||Jc_j| + sum |W||V'^-1||W^T|,
    G (M,ncp,3) = |W_m| |V'^-1| per observation (rhs_mag = gc scale + sum_m G_m gp scale), share (C,C) bool: the two cameras
    see a common free point."""
    if np.finfo(np.longdouble).eps > 2e-19:
        raise RuntimeError("reduced_system needs an extended-precision np.longdouble (64 mantissa bits)")
    ci, pi = _indices(ci, pi)
    M, ncp = ci.size, Jc.shape[2]
    n = n_cams * ncp
    free = np.ones(n_pts, bool) if fixed is None else ~np.asarray(fixed, bool)
    S = np.zeros((n, n), dtype=np.longdouble)
    S_mag = np.zeros((n, n))
    rhs, d = np.zeros(n), np.ones(n)
    G = np.zeros((M, ncp, 3))
    share = np.eye(n_cams, dtype=bool)
    with mp.workdps(SUM_DPS):
        lam = _mpf(lam)
        mJc = [[[_mpf(v) for v in Jc[m, k]] for k in range(2)] for m in range(M)]
        mJp = [[[_mpf(v) for v in Jp[m, k]] for k in range(2)] for m in range(M)]
        mr = [[_mpf(v) for v in r[m]] for m in range(M)]
        acc = [[mp.mpf(0)] * ncp for _ in range(n_cams)]           # rhs, in mpmath throughout
        Sx = mp.zeros(n, n) if full_mp else None
        for c in range(n_cams):
            sel = np.nonzero(ci == c)[0]
            o = c * ncp
            for a in range(ncp):
                ca = [mJc[m][k][a] for m in sel for k in range(2)]
                acc[c][a] = -mp.fdot(ca, [mr[m][k] for m in sel for k in range(2)])
                for b in range(a, ncp):
                    u = mp.fdot(ca, [mJc[m][k][b] for m in sel for k in range(2)])
                    S[o + a, o + b] = S[o + b, o + a] = _ld(u)
                    if full_mp:
                        Sx[o + a, o + b] = Sx[o + b, o + a] = u
                    if a == b and u > 0:
                        d[o + a] = float(mp.sqrt(u))
            A = np.abs(Jc[sel]).reshape(-1, ncp)
            S_mag[o:o + ncp, o:o + ncp] = A.T @ A
        for p in np.nonzero(free)[0]:
            sel = np.nonzero(pi == p)[0]
            if sel.size == 0:
                continue
            V = mp.matrix(3, 3)
            g = [mp.mpf(0)] * 3
            for i in range(3):
                ci_ = [mJp[m][k][i] for m in sel for k in range(2)]
                g[i] = mp.fdot(ci_, [mr[m][k] for m in sel for k in range(2)])
                for j in range(i, 3):
                    V[i, j] = V[j, i] = mp.fdot(ci_, [mJp[m][k][j] for m in sel for k in range(2)])
            for i in range(3):
                V[i, i] += lam * (V[i, i] if V[i, i] > 0 else 1)
            cams_p = sorted(set(int(c) for c in ci[sel]))
            W = {c: [[mp.mpf(0)] * 3 for _ in range(ncp)] for c in cams_p}      # one block per camera, duplicates summed
            for m in sel:
                Wc = W[int(ci[m])]
                for a in range(ncp):
                    for j in range(3):
                        Wc[a][j] += mJc[m][0][a] * mJp[m][0][j] + mJc[m][1][a] * mJp[m][1][j]
            rows = np.concatenate([c * ncp + np.arange(ncp) for c in cams_p])
            Vinv = mp.inverse(V)
            Vinv_abs = np.array([[abs(float(Vinv[i, j])) for j in range(3)] for i in range(3)])
            Wabs = np.array([[[abs(float(v)) for v in row] for row in W[c]] for c in cams_p])          # (k, ncp, 3)
            GW = Wabs @ Vinv_abs
            S_mag[np.ix_(rows, rows)] += GW.reshape(-1, 3) @ Wabs.reshape(-1, 3).T
            for m in sel:                                   # |W_m| |V'^-1| of the observation's own block
                G[m] = np.abs(np.einsum("ka,kj->aj", Jc[m], Jp[m])) @ Vinv_abs
            share[np.ix_(cams_p, cams_p)] = True
            if full_mp:
                x = Vinv * mp.matrix(g)
                Wm = mp.matrix([row for c in cams_p for row in W[c]])
                P = Wm * Vinv * Wm.T
                for a, ra in enumerate(rows):
                    for b, rb in enumerate(rows):
                        Sx[int(ra), int(rb)] -= P[a, b]
            else:
                Li = _chol3_inv(V)                          # V' = L L^T: V'^-1 = Li^T Li, Z = W Li^T
                x = Li.T * (Li * mp.matrix(g))
                Z = np.array([[_ld(mp.fdot(row, [Li[j, i] for i in range(3)])) for j in range(3)] for c in cams_p for row in W[c]],
                             dtype=np.longdouble)
                S[np.ix_(rows, rows)] -= Z @ Z.T
            for c in cams_p:
                for a in range(ncp):
                    acc[c][a] += mp.fdot(W[c][a], [x[j] for j in range(3)])
        if full_mp:
            for a in range(n):
                for b in range(n):
                    S[a, b] = _ld(Sx[a, b])
        rhs[:] = [float(v) for row in acc for v in row]
    S = 0.5 * (S + S.T)
    return dict(S=S.astype(np.float64), S_ld=S, rhs=rhs, d=d, S_mag=S_mag, G=G, share=share)


# ----------------------------------------------------------------------------- shared intrinsics (SBA_MODE_SHARED_INTR)
def tie_matrix(n_cams, ncp):
    """T (C ncp, n_tied) of zeros and ones, delta_c = T delta_s, written as the reference unpacks its parameter vector (pySBA.py:313,
    fun_sharedcam): x = [f k1 k2 | 6 extrinsics per camera | the per-camera tail], tail = cx cy, or p1 p2 cx cy with 13 parameters;
    a camera row is [extrinsics, shared, tail]."""
    pc = ncp - 9
    n_tied = 3 + (6 + pc) * n_cams
    x = np.arange(n_tied)
    shared, extr, tail = x[:3], x[3:3 + 6 * n_cams].reshape(n_cams, 6), x[3 + 6 * n_cams:].reshape(n_cams, pc)
    col = np.concatenate((extr, np.tile(shared, (n_cams, 1)), tail), axis=1).ravel()
    T = np.zeros((n_cams * ncp, n_tied))
    T[np.arange(n_cams * ncp), col] = 1.0
    return T


def tied_system(T, S_ld, rhs, diagU, gc, full_mp=False):
    """S_s = T^T S T (np.longdouble from the longdouble S, and rounded once), rhs_s, diagU_s, g_s = T^T of the float64 vectors, summed
    in longdouble and rounded once.  A tied entry sums at most C^2 entries of S, each below d_i d_j, so the longdouble sum stays below
    C^2 2^-64 of sum d_i d_j; full_mp sums the same entries in mpmath (tests/test_exact_model_host.py holds the two together)."""
    L = np.longdouble
    Tl = T.astype(L)
    vec = lambda v: (Tl.T @ np.asarray(v, dtype=L).ravel())      # noqa: E731
    if full_mp:
        n, nt = T.shape
        cols = [np.nonzero(T[:, a])[0] for a in range(nt)]
        Ss = np.zeros((nt, nt), dtype=L)
        with mp.workdps(SUM_DPS):
            def mpl(v):
                hi = float(v)
                return mp.mpf(hi) + mp.mpf(float(v - L(hi)))
            Sm = [[mpl(S_ld[i, j]) for j in range(n)] for i in range(n)]
            for a in range(nt):
                for b in range(a, nt):
                    Ss[a, b] = Ss[b, a] = _ld(mp.fsum([Sm[i][j] for i in cols[a] for j in cols[b]]))
    else:
        Ss = Tl.T @ np.asarray(S_ld, dtype=L) @ Tl
        Ss = 0.5 * (Ss + Ss.T)
    rhs_s, dU_s, g_s = vec(rhs), vec(diagU), vec(gc)
    return dict(S=Ss.astype(np.float64), S_ld=Ss, rhs=rhs_s.astype(np.float64), rhs_ld=rhs_s, diagU=dU_s.astype(np.float64),
                g=g_s.astype(np.float64))


# ----------------------------------------------------------------------------- the squared-pixel-error variants
def sq_system(delta, Jc, Jp, w, ci, pi, pts, n_cams, kind, full_mp=False, row_factor=2):
    """delta (M,2), Jc (M,2,NCP), Jp (M,2,3): the UNWEIGHTED exact pixel error and its derivatives (exact_blocks with w = 1).
    kind 'cams' (SBA_MODE_CAMS_ONLY_SQ): one group per camera, P = NCP parameters, row J~ = 2 w Delta dDelta/dcam.
    kind 'affine' (SBA_MODE_TRANSFORM_SQ): one group, P = 12, theta = reshape(3, 4) at the identity, J~[4 a + l] = 2 w Delta dDelta/dX_a [X, 1]_l.
    rho = w Delta^2 per pixel component.  The rows [J~ | rho] are formed in mpmath; their products are summed in np.longdouble from the
    longdouble roundings of the rows (each product within 3 x 2^-64 of itself, each sum of R rows within R 2^-64 of h_i h_j by
    Cauchy-Schwarz); full_mp forms every sum in mpmath.  Returns H (G,P,P), g (G,P), cost, h = sqrt(diag H) (G,P), rho (M,2)."""
    ci, pi = _indices(ci, pi)
    M = ci.size
    wv = _weights(w, M)
    P = Jc.shape[2] if kind == "cams" else 12
    G = n_cams if kind == "cams" else 1
    L = np.longdouble
    rows_mp = []
    with mp.workdps(SUM_DPS):
        for m in range(M):
            Xh = [_mpf(v) for v in pts[pi[m]]] + [mp.mpf(1)]
            for k in range(2):
                d = _mpf(delta[m, k])
                f = row_factor * _mpf(wv[m]) * d
                if kind == "cams":
                    row = [f * _mpf(v) for v in Jc[m, k]]
                else:
                    row = [f * _mpf(Jp[m, k, a]) * Xh[l] for a in range(3) for l in range(4)]
                rows_mp.append(row + [_mpf(wv[m]) * d * d])
        grp = np.repeat(ci if kind == "cams" else np.zeros(M, np.int64), 2)
        Q = np.zeros((G, P + 1, P + 1), dtype=L)
        if full_mp:
            for g_ in range(G):
                sel = np.nonzero(grp == g_)[0]
                for i in range(P + 1):
                    ri = [rows_mp[r][i] for r in sel]
                    for j in range(i, P + 1):
                        Q[g_, i, j] = Q[g_, j, i] = _ld(mp.fdot(ri, [rows_mp[r][j] for r in sel]))
        else:
            R = np.array([[_ld(v) for v in row] for row in rows_mp], dtype=L)
            for g_ in range(G):
                Rg = R[grp == g_]
                Q[g_] = Rg.T @ Rg
        rho = np.array([float(row[-1]) for row in rows_mp]).reshape(M, 2)
    H = Q[:, :P, :P]
    cost = 0.5 * np.sum(Q[:, P, P])
    h = np.sqrt(np.einsum("gii->gi", H)).astype(np.float64)
    return dict(H=H.astype(np.float64), H_ld=H, g=Q[:, :P, P].astype(np.float64), g_ld=Q[:, :P, P], cost=float(cost), cost_ld=cost,
                h=np.where(h > 0, h, 1.0), rho=rho)


def affine_points(theta, pts):
    """theta (12,) = reshape(3, 4) applied to [X, 1], in mpmath at the CURRENT precision: a list of rows of mpf (exact_residual takes them)."""
    th = [_mpf(v) for v in np.ravel(theta)]
    out = []
    for X in pts:
        Xh = [_mpf(v) for v in X] + [mp.mpf(1)]
        out.append([mp.fdot(th[4 * a:4 * a + 4], Xh) for a in range(3)])
    return out
