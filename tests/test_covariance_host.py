"""CPU: the covariance entry point is exported, declared and fails loudly without a device; the numpy oracles the GPU tests
(tests/test_gpu_covariance.py) compare against are checked here -- the similarity-gauge null vectors of include/sba_hip.h
against the oracle's undamped reduced camera system, and the pseudo-inverse against a minimal-constraint inverse on the
intrinsics (the gauge-independence the GPU tests rely on).

The free-gauge reference of the GPU tests is P (S + alpha Q Q^T)^-1 P by a Cholesky factorisation, not an eigh pseudo-inverse
dropping 7 eigenpairs: in raw units S has a condition number near 1e14 on the complement of the gauge (focal length against
distance on these rigs), so eigh does not separate the gauge from the weakest true direction (eigen-gap ~20 on the 4 x 60 rig)
and its pseudo-inverse is off by several per cent, while the Cholesky route is insensitive to the diagonal scaling that
causes most of that condition number.  Its independence from the analytic Q comes from two other checks: S Q ~ 0 below,
and the intrinsic blocks against a minimal-constraint inverse that knows nothing of Q."""
import ctypes
import os
import re

import numpy as np
import pytest

from lasercalib_amd import _native
from lasercalib_amd.synth import make_rig
from oracle import lm_schur_model as lsm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- numpy oracles (also used by the GPU tests)
def huber_scale(res, f_scale):
    """sqrt(rho') per residual component of scipy's Huber loss (the IRLS row scaling of the engine, sba_model.hpp)."""
    a = np.abs(res)
    return np.sqrt(np.where(a <= f_scale, 1.0, f_scale / np.maximum(a, 1e-300)))


def oracle_blocks(cams, pts, uv, ci, pi, w=None, huber=None):
    """Residual (M,2) and Jacobian blocks Jc (M,2,11), Jp (M,2,3) of the problem the engine solves (weights, Huber IRLS)."""
    w = np.ones(ci.shape[0]) if w is None else w
    res, Jc, Jp = lsm.residual_jacobian(cams, pts, uv, ci, pi, w)
    res = res.reshape(-1, 2)
    if huber is not None:
        s = huber_scale(res, huber)
        res, Jc, Jp = res * s, Jc * s[:, :, None], Jp * s[:, :, None]
    return res, Jc, Jp


def oracle_S(cams, pts, uv, ci, pi, w=None, huber=None, drop=None, fixed=None):
    """The undamped reduced camera system (lam = 0) of oracle/lm_schur_model.py; drop: points left out entirely; fixed:
    anchored points (their observations stay in U, they are no unknowns)."""
    res, Jc, Jp = oracle_blocks(cams, pts, uv, ci, pi, w, huber)
    if fixed is not None:
        Jp = Jp * (~fixed[pi])[:, None, None]
    keep = np.ones(ci.shape[0], bool) if drop is None else ~np.isin(pi, drop)
    C, N = cams.shape[0], pts.shape[0]
    U, gc, V, gp, W = lsm.normal_blocks(res[keep], Jc[keep], Jp[keep], ci[keep], pi[keep], C, N)
    if drop is not None:
        V[drop] = np.eye(3)
    if fixed is not None:
        V[fixed] = np.eye(3)
    S, _rhs, Vinv = lsm.reduced_system(U, gc, V, gp, W, ci[keep], pi[keep], 0.0, np.zeros((N, 3)))
    return S, V, W, keep


def gauge_basis(cams):
    """The 7 similarity null vectors on the camera rows (n x 7, orthonormal): d rvec = -J_r^-1 omega, d t = -R tau + s t."""
    C, P = cams.shape
    Q = np.zeros((C * P, 7))
    for c in range(C):
        r = cams[c, 0:3]
        th2 = float(r @ r)
        th = np.sqrt(th2)
        K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
        if th2 < 1e-8:
            a, b, beta, cs = 1 - th2 / 6, 0.5 - th2 / 24, 1 / 12 + th2 / 720, 1 - th2 / 2
        else:
            a, b, cs = np.sin(th) / th, (1 - np.cos(th)) / th2, np.cos(th)
            beta = 1 / th2 - (1 + np.cos(th)) / (2 * th * np.sin(th))
        R = cs * np.eye(3) + a * K + b * np.outer(r, r)
        Jri = np.eye(3) + 0.5 * K + beta * K @ K
        Q[c * P:c * P + 3, 0:3] = -Jri
        Q[c * P + 3:c * P + 6, 3:6] = -R
        Q[c * P + 3:c * P + 6, 6] = cams[c, 3:6]
    q, _ = np.linalg.qr(Q)
    return q


def minimal_constraint_inverse(S, P):
    """Inverse of S with camera 0's pose and camera 1's x translation removed, zero-padded: a generalised inverse of S that
    agrees with S^+ on every functional orthogonal to the gauge (the intrinsic blocks)."""
    drop = list(range(6)) + [P + 3]
    keep = np.setdiff1d(np.arange(S.shape[0]), drop)
    out = np.zeros_like(S)
    out[np.ix_(keep, keep)] = np.linalg.inv(S[np.ix_(keep, keep)])
    return out


def fd_blocks(cams, pts, uv, ci, pi):
    """Residual (M,2) and central-difference Jacobian blocks Jc (M,2,P), Jp (M,2,3) of the 13-parameter model of
    oracle/sba_oracle_tangential.py (its project is vectorised over observation rows: one evaluation per parameter column)."""
    from oracle import sba_oracle_tangential as ot
    rows, X = cams[ci].copy(), pts[pi].copy()
    res = ot.project(X, rows) - uv
    P = cams.shape[1]
    Jc, Jp = np.empty((ci.size, 2, P)), np.empty((ci.size, 2, 3))
    for k in range(P):
        h = 1e-6 * (1.0 + np.abs(rows[:, k]))
        up, dn = rows.copy(), rows.copy()
        up[:, k] += h
        dn[:, k] -= h
        Jc[:, :, k] = (ot.project(X, up) - ot.project(X, dn)) / (2 * h)[:, None]
    for k in range(3):
        h = 1e-6 * (1.0 + np.abs(X[:, k]))
        up, dn = X.copy(), X.copy()
        up[:, k] += h
        dn[:, k] -= h
        Jp[:, :, k] = (ot.project(up, rows) - ot.project(dn, rows)) / (2 * h)[:, None]
    return res, Jc, Jp


def generic_S(Jc, Jp, ci, pi, C, N, fixed=None):
    """The undamped reduced camera system for any camera row length, with duplicate (point, camera) observations summed:
    S = U - sum_p W_p V_p^-1 W_p^T.  Returns S, V (N,3,3) and W_p per point (dict: point -> (cams, (k*P, 3)))."""
    P = Jc.shape[2]
    free = np.ones(N, bool) if fixed is None else ~fixed
    U = np.zeros((C, P, P))
    V = np.zeros((N, 3, 3))
    np.add.at(U, ci, np.einsum("mri,mrj->mij", Jc, Jc))
    np.add.at(V, pi, np.einsum("mri,mrj->mij", Jp, Jp))
    Wo = np.einsum("mri,mrj->mij", Jc, Jp)
    S = np.zeros((C * P, C * P))
    for c in range(C):
        S[c * P:(c + 1) * P, c * P:(c + 1) * P] = U[c]
    order = np.argsort(pi, kind="stable")
    start = np.searchsorted(pi[order], np.arange(N + 1))
    Wp = {}
    for p in range(N):
        idx = order[start[p]:start[p + 1]]
        if idx.size == 0 or not free[p]:
            continue
        cams = np.unique(ci[idx])
        W = np.zeros((cams.size, P, 3))
        np.add.at(W, np.searchsorted(cams, ci[idx]), Wo[idx])
        W = W.reshape(-1, 3)
        rows = (cams[:, None] * P + np.arange(P)[None, :]).ravel()
        S[np.ix_(rows, rows)] -= W @ np.linalg.solve(V[p], W.T)
        Wp[p] = (cams, W)
    return S, V, Wp


# ----------------------------------------------------------------------------- the ABI
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _native.load()


def test_covariance_symbol_exported_and_declared(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sba_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+sba_covariance\s*\(", text)
    assert "sba_covariance" in _native.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "sba_covariance")


def test_covariance_struct_layouts():
    assert ctypes.sizeof(_native.CovOpts) == 32
    assert ctypes.sizeof(_native.CovReport) == 80


def test_covariance_without_device_fails_loudly(lib):
    if lib.sba_device_count() > 0:
        pytest.skip("a GPU is visible; the no-device path is exercised on the CPU-only container")
    from lasercalib_amd.pySBA import PySBA
    rig = make_rig(3, 30)
    sba = PySBA(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"])
    with pytest.raises(_native.SbaError, match="no HIP device"):
        sba.covariance()


# ----------------------------------------------------------------------------- the oracles
@pytest.mark.parametrize("C,N,vis", [(4, 60, 1.0), (9, 120, 0.7)])
def test_gauge_basis_spans_the_null_space_of_the_oracle_S(C, N, vis):
    rig = make_rig(C, N, seed=3, visibility=vis)
    cams, pts = rig["cams_true"], rig["pts_true"]
    S, *_ = oracle_S(cams, pts, rig["points_2d"], rig["camera_ind"], rig["point_ind"])
    Q = gauge_basis(cams)
    np.testing.assert_allclose(Q.T @ Q, np.eye(7), atol=1e-12)
    rel = np.linalg.norm(S @ Q) / (np.linalg.norm(S) * np.linalg.norm(Q))
    assert rel < 1e-10, rel


def test_intrinsics_do_not_depend_on_the_gauge():
    rig = make_rig(5, 80, seed=4)
    cams, pts = rig["cams_true"], rig["pts_true"]
    S, *_ = oracle_S(cams, pts, rig["points_2d"], rig["camera_ind"], rig["point_ind"])
    Sm = minimal_constraint_inverse(S, 11)
    Q = gauge_basis(cams)
    P = np.eye(S.shape[0]) - Q @ Q.T
    Sr = P @ np.linalg.inv(S + np.mean(np.diag(S)) * Q @ Q.T) @ P       # the library's recipe
    assert np.linalg.norm(S @ Sr @ S - S) <= 1e-6 * np.linalg.norm(S)    # a generalised inverse ...
    assert np.linalg.norm(Sr @ Q) <= 1e-8 * np.linalg.norm(Sr)            # ... with the minimum-norm datum
    for c in range(5):
        i = slice(c * 11 + 6, c * 11 + 11)
        ref = Sm[i, i]
        assert np.linalg.norm(Sr[i, i] - ref) <= 1e-6 * np.linalg.norm(ref)


def test_generic_oracle_matches_the_schur_model_and_the_13_parameter_gauge():
    rig = make_rig(5, 80, seed=6, visibility=0.8)
    cams, pts = rig["cams_true"], rig["pts_true"]
    ci, pi = rig["camera_ind"], rig["point_ind"]
    S, *_ = oracle_S(cams, pts, rig["points_2d"], ci, pi)
    _r, Jc, Jp = oracle_blocks(cams, pts, rig["points_2d"], ci, pi)
    Sg, _V, _W = generic_S(Jc, Jp, ci, pi, 5, 80)
    assert np.linalg.norm(Sg - S) <= 1e-12 * np.linalg.norm(S)
    # 13-parameter rows, central differences: the same similarity gauge (intrinsics, p1 and p2 included, do not move)
    rig = make_rig(5, 80, seed=6, visibility=0.8, tangential=True)
    cams, pts = rig["cams_true"], rig["pts_true"]
    _r, Jc, Jp = fd_blocks(cams, pts, rig["points_2d"], rig["camera_ind"], rig["point_ind"])
    S13, _V, _W = generic_S(Jc, Jp, rig["camera_ind"], rig["point_ind"], 5, 80)
    Q = gauge_basis(cams)
    rel = np.linalg.norm(S13 @ Q) / (np.linalg.norm(S13) * np.linalg.norm(Q))
    assert rel < 1e-8, rel      # central-difference error: 2e-9 measured
