"""GPU tests of sba_covariance (include/sba_hip.h): the Gauss-Newton covariance of the cameras and points at the optimum.

Oracles (numpy, tests/test_covariance_host.py): the dense Jacobian of oracle/lm_schur_model.py (FD Jacobian of
oracle/sba_oracle_tangential.py for 13 parameters) for the anchored case, and the undamped reduced camera system
reduced_system(lam=0) for the free gauge.  The synthetic rigs are ill-conditioned in raw units (condition ~1e14 of S on the
complement of the gauge, ~1e9 after Jacobi scaling: focal length against distance), so every comparison is relative to the
block's norm and the oracle inverts with a Cholesky factorisation, which is insensitive to diagonal scaling (why not an eigh
pseudo-inverse: tests/test_covariance_host.py).  For 13-parameter rows the oracle S is built (generic_S) from the handle's
analytic Jacobian blocks, which are checked here against central differences of oracle/sba_oracle_tangential.py.
"""
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sl

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lasercalib_amd import _native  # noqa: E402
from lasercalib_amd.synth import make_rig  # noqa: E402
from test_covariance_host import (fd_blocks, gauge_basis, generic_S, minimal_constraint_inverse, oracle_blocks,  # noqa: E402
                                  oracle_S)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert _native.device_count() > 0, "no HIP device visible: GPU tests must run on the MI355X box"


def _solved(rig, dtype="f64", fixed=None, huber=None, cams=None, pts=None):
    prob = _native.Problem(rig["cams0"] if cams is None else cams, rig["pts0"] if pts is None else pts, rig["points_2d"],
                           rig["camera_ind"], rig["point_ind"], dtype=dtype)
    if fixed is not None:
        prob.set_fixed_points(fixed)
    if huber is not None:
        prob.set_robust_loss("huber", huber)
    prob.solve_lm(prob.make_opts(ftol=1e-12 if dtype == "f64" else 1e-8, xtol=1e-12, gtol=1e-12, max_nfev=400))
    return prob


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _chol_inv(A):
    return sl.cho_solve(sl.cho_factor(A, lower=True), np.eye(A.shape[0]))


def _blocks(X, C, P):
    return np.stack([X[c * P:(c + 1) * P, c * P:(c + 1) * P] for c in range(C)])


def _oracle_points(Xc, V, W, ci, pi, N, P):
    """Sigma_pp = V^-1 + V^-1 W^T Sigma_cc W V^-1, W_p (n x 3) summed over the point's observations."""
    out = np.empty((N, 3, 3))
    for p in range(N):
        idx = np.nonzero(pi == p)[0]
        Wp = np.zeros((Xc.shape[0], 3))
        for o in idx:
            Wp[ci[o] * P:(ci[o] + 1) * P] += W[o]
        Vi = np.linalg.inv(V[p])
        out[p] = Vi + Vi @ Wp.T @ Xc @ Wp @ Vi
    return out


# ----------------------------------------------------------------------------- 1. anchored: against inv(J^T J) of the dense Jacobian
def test_anchored_matches_dense_inverse():
    C, N = 5, 80
    rig = make_rig(C, N, seed=11)
    fixed = np.zeros(N, bool)
    fixed[np.random.default_rng(2).choice(N, 12, replace=False)] = True
    pts0 = rig["pts0"].copy()
    pts0[fixed] = rig["pts_true"][fixed]
    prob = _solved(rig, fixed=fixed, pts=pts0)
    cams, pts = prob.get_params()
    cov = prob.covariance(scale=False, full=True)
    prob.close()
    assert cov.gauge_rank == 0 and cov.info == 0 and cov.n_points_anchored == 12 and cov.gauge_residual == 0.0
    ci, pi = rig["camera_ind"], rig["point_ind"]
    _res, Jc, Jp = oracle_blocks(cams, pts, rig["points_2d"], ci, pi)
    free = np.nonzero(~fixed)[0]
    col = -np.ones(N, int)
    col[free] = np.arange(free.size)
    n = 11 * C
    J = np.zeros((2 * ci.size, n + 3 * free.size))
    for o in range(ci.size):
        J[2 * o:2 * o + 2, ci[o] * 11:(ci[o] + 1) * 11] = Jc[o]
        if col[pi[o]] >= 0:
            J[2 * o:2 * o + 2, n + 3 * col[pi[o]]:n + 3 * col[pi[o]] + 3] = Jp[o]
    Sig = _chol_inv(J.T @ J)
    e_c = max(_rel(cov.cameras[c], Sig[c * 11:(c + 1) * 11, c * 11:(c + 1) * 11]) for c in range(C))
    e_f = _rel(cov.cameras_full, Sig[:n, :n])
    e_p = max(_rel(cov.points[p], Sig[n + 3 * col[p]:n + 3 * col[p] + 3, n + 3 * col[p]:n + 3 * col[p] + 3]) for p in free)
    print(f"anchored 5 x 80: camera blocks {e_c:.2e}, full {e_f:.2e}, points {e_p:.2e}")
    assert e_c <= 1e-7 and e_p <= 1e-7
    assert np.all(cov.points[fixed] == 0.0)


# ----------------------------------------------------------------------------- 2. free gauge against the oracle S
@pytest.mark.parametrize("C,N,vis,minc", [(4, 60, 1.0, 2), (16, 200, 0.7, 2), (17, 250, 0.6, 4)])
def test_free_gauge_against_oracle(C, N, vis, minc):
    rig = make_rig(C, N, seed=5, visibility=vis, min_cams_per_point=minc)
    prob = _solved(rig)
    cams, pts = prob.get_params()
    cov = prob.covariance(scale=False, full=True)
    prob.close()
    assert cov.gauge_rank == 7 and cov.info == 0 and cov.n_points_degenerate == 0
    assert cov.gauge_residual <= 1e-10, cov.gauge_residual
    ci, pi = rig["camera_ind"], rig["point_ind"]
    S, V, W, _keep = oracle_S(cams, pts, rig["points_2d"], ci, pi)
    Q = gauge_basis(cams)
    P = np.eye(S.shape[0]) - Q @ Q.T
    X = P @ _chol_inv(S + np.mean(np.diag(S)) * Q @ Q.T) @ P
    e_c = max(_rel(cov.cameras[c], X[c * 11:(c + 1) * 11, c * 11:(c + 1) * 11]) for c in range(C))
    assert np.allclose(cov.cameras, _blocks(cov.cameras_full, C, 11))
    # intrinsics against an inverse that knows nothing of Q (gauge independence)
    Xm = minimal_constraint_inverse(S, 11)
    e_i = max(_rel(cov.cameras[c][6:, 6:], Xm[c * 11 + 6:(c + 1) * 11, c * 11 + 6:(c + 1) * 11]) for c in range(C))
    ref_p = _oracle_points(X, V, W, ci, pi, N, 11)
    e_p = max(_rel(cov.points[p], ref_p[p]) for p in range(N))
    print(f"free {C} x {N}: camera blocks {e_c:.2e}, intrinsics vs minimal constraint {e_i:.2e}, points {e_p:.2e}, "
          f"gauge residual {cov.gauge_residual:.1e}")
    assert e_c <= 1e-6 and e_i <= 1e-6 and e_p <= 1e-6


# ----------------------------------------------------------------------------- 3. large systems: the multi-workgroup factorisation
def _device_S(prob, rig, C, N, fixed=None):
    """generic_S from the handle's own analytic Jacobian blocks at its current parameters."""
    _r, Jc, Jp = prob.residual_jacobian()
    return generic_S(Jc, Jp, rig["camera_ind"], rig["point_ind"], C, N, fixed), Jc, Jp


@pytest.mark.parametrize("C,N,tang", [(64, 2000, False), (128, 1500, False), (128, 1000, True)])
def test_large_intrinsics_against_minimal_constraint_inverse(C, N, tang):
    """(128, 1000, 13 parameters) is n = 1664, the largest system: 52 tile columns, all 7 row blocks of k_cov_inv."""
    rig = make_rig(C, N, seed=7, visibility=0.1 if tang else 0.3, tangential=tang)
    P = 13 if tang else 11
    with _native.Problem(rig["cams_true"], rig["pts_true"], rig["points_2d"], rig["camera_ind"], rig["point_ind"]) as prob:
        cov = prob.covariance(scale=False, points=False)
        cams, pts = prob.get_params()
        if tang:
            (S, _V, _W), _Jc, _Jp = _device_S(prob, rig, C, N)
    assert cov.gauge_rank == 7 and cov.info == 0 and cov.gauge_residual <= 1e-10
    if not tang:
        S, *_ = oracle_S(cams, pts, rig["points_2d"], rig["camera_ind"], rig["point_ind"])
    Xm = minimal_constraint_inverse(S, P)
    e_i = max(_rel(cov.cameras[c][6:, 6:], Xm[c * P + 6:(c + 1) * P, c * P + 6:(c + 1) * P]) for c in range(C))
    print(f"large {C} x {N} ({P} p): intrinsics vs minimal constraint {e_i:.2e}, gauge residual {cov.gauge_residual:.1e}, "
          f"device {cov.seconds_device * 1e3:.2f} ms")
    assert e_i <= 1e-6


def test_tangential_free_gauge():
    C, N = 8, 200
    rig = make_rig(C, N, seed=53, visibility=0.8, tangential=True)
    prob = _solved(rig)
    cams, pts = prob.get_params()
    cov = prob.covariance(scale=False, full=True)
    (S, V, Wp), Jc, Jp = _device_S(prob, rig, C, N)
    prob.close()
    ci, pi = rig["camera_ind"], rig["point_ind"]
    _r, Jc_fd, Jp_fd = fd_blocks(cams, pts, rig["points_2d"], ci, pi)
    e_j = max(_rel(Jc, Jc_fd), _rel(Jp, Jp_fd))
    assert cov.gauge_rank == 7 and cov.info == 0 and cov.gauge_residual <= 1e-10, cov.gauge_residual
    Q = gauge_basis(cams)
    Pm = np.eye(S.shape[0]) - Q @ Q.T
    X = Pm @ _chol_inv(S + np.mean(np.diag(S)) * Q @ Q.T) @ Pm
    e_c = max(_rel(cov.cameras[c], X[c * 13:(c + 1) * 13, c * 13:(c + 1) * 13]) for c in range(C))
    Xm = minimal_constraint_inverse(S, 13)
    e_i = max(_rel(cov.cameras[c][6:, 6:], Xm[c * 13 + 6:(c + 1) * 13, c * 13 + 6:(c + 1) * 13]) for c in range(C))
    e_p = max(_rel(cov.points[p], _generic_point(X, V, Wp, p, 13)) for p in range(N))
    print(f"tangential free {C} x {N}: Jacobian vs central differences {e_j:.1e}, camera blocks {e_c:.2e}, intrinsics {e_i:.2e}, "
          f"points {e_p:.2e}, gauge residual {cov.gauge_residual:.1e}")
    assert e_j <= 1e-6 and e_c <= 1e-6 and e_i <= 1e-6 and e_p <= 1e-6


def _generic_point(X, V, Wp, p, P):
    cams, W = Wp[p]
    rows = (cams[:, None] * P + np.arange(P)[None, :]).ravel()
    Vi = np.linalg.inv(V[p])
    return Vi + Vi @ W.T @ X[np.ix_(rows, rows)] @ W @ Vi


def test_tangential_anchored_against_fd_jacobian():
    from oracle import sba_oracle_tangential as ot
    C, N = 4, 60
    rig = make_rig(C, N, seed=13, tangential=True)
    fixed = np.zeros(N, bool)
    fixed[:8] = True
    pts0 = rig["pts0"].copy()
    pts0[fixed] = rig["pts_true"][fixed]
    prob = _solved(rig, fixed=fixed, pts=pts0)
    cams, pts = prob.get_params()
    cov = prob.covariance(scale=False)
    prob.close()
    ci, pi = rig["camera_ind"], rig["point_ind"]
    x = np.hstack([cams.ravel(), pts.ravel()])
    J = ot.fd_jacobian(x, C, N, ci, pi, rig["points_2d"], np.ones((ci.size, 1))).toarray()
    keep = np.r_[np.arange(13 * C), 13 * C + np.nonzero(np.repeat(~fixed, 3))[0]]
    Sig = _chol_inv(J[:, keep].T @ J[:, keep])
    e_c = max(_rel(cov.cameras[c], Sig[c * 13:(c + 1) * 13, c * 13:(c + 1) * 13]) for c in range(C))
    print(f"tangential anchored: camera blocks vs FD {e_c:.2e}")
    assert cov.gauge_rank == 0 and e_c <= 1e-4


# ----------------------------------------------------------------------------- 4. f32 handles
def test_f32_handle_matches_f64():
    """The covariance is computed in float64 for either dtype; at the same parameters the two handles differ only by the
    f32 observation list (pixel coordinates rounded to f32).  Measured spread on the MI355X: 9.1e-7 relative on both the
    intrinsic and the point standard deviations; the bar is 1e-5."""
    rig = make_rig(16, 300, seed=17, visibility=0.8)
    p64 = _solved(rig, "f64")
    cams, pts = p64.get_params()
    c64 = p64.covariance()
    p64.close()
    with _native.Problem(cams, pts, rig["points_2d"], rig["camera_ind"], rig["point_ind"], dtype="f32") as p32:
        c32 = p32.covariance()
    ei = np.max(np.abs(c32.camera_std()[:, 6:] / c64.camera_std()[:, 6:] - 1))
    ep = np.max(np.abs(c32.point_std() / c64.point_std() - 1))
    print(f"f32 vs f64 handle: intrinsic std {ei:.2e}, point std {ep:.2e}")
    assert ei <= 1e-5 and ep <= 1e-5


# ----------------------------------------------------------------------------- 5. Huber, 6. cams_fixed, 7. scaling, 8. sigma^2
def test_huber_against_irls_scaled_rows():
    C, N = 6, 150
    rig = make_rig(C, N, seed=19, noise_px=1.0)
    fixed = np.zeros(N, bool)
    fixed[:10] = True
    pts0 = rig["pts0"].copy()
    pts0[fixed] = rig["pts_true"][fixed]
    prob = _solved(rig, fixed=fixed, huber=1.0, pts=pts0)
    cams, pts = prob.get_params()
    cov = prob.covariance(scale=False)
    prob.close()
    ci, pi = rig["camera_ind"], rig["point_ind"]
    S, V, W, _ = oracle_S(cams, pts, rig["points_2d"], ci, pi, huber=1.0, fixed=fixed)
    X = _chol_inv(S)
    e_c = max(_rel(cov.cameras[c], X[c * 11:(c + 1) * 11, c * 11:(c + 1) * 11]) for c in range(C))
    ref_p = _oracle_points(X, V, W, ci, pi, N, 11)
    e_p = max(_rel(cov.points[p], ref_p[p]) for p in range(10, N))
    print(f"huber: camera blocks {e_c:.2e}, points {e_p:.2e}")
    assert e_c <= 1e-6 and e_p <= 1e-6


def test_cams_fixed_and_scaling():
    rig = make_rig(8, 200, seed=23, visibility=0.8)
    prob = _solved(rig)
    cams, pts = prob.get_params()
    _r, cost = prob.residual()
    unscaled = prob.covariance(scale=False)
    scaled = prob.covariance(scale=True)
    fixedc = prob.covariance(scale=False, cams_fixed=True)
    prob.close()
    n = 8 * 11
    assert scaled.dof == 2 * rig["camera_ind"].size - (n + 3 * 200 - 7) == unscaled.dof
    np.testing.assert_allclose(scaled.sigma2, 2 * cost / scaled.dof, rtol=1e-9)
    np.testing.assert_allclose(scaled.cameras, unscaled.cameras * scaled.sigma2, rtol=1e-12)
    np.testing.assert_allclose(scaled.points, unscaled.points * scaled.sigma2, rtol=1e-12)
    # noise_px = 0.3 per component
    assert abs(scaled.sigma2 / 0.09 - 1) <= 0.1, scaled.sigma2
    # cameras held: Sigma_pp = V_p^-1
    _S, V, _W, _ = oracle_S(cams, pts, rig["points_2d"], rig["camera_ind"], rig["point_ind"])
    e = max(_rel(fixedc.points[p], np.linalg.inv(V[p])) for p in range(200))
    assert fixedc.gauge_rank == 0 and fixedc.dof == 2 * rig["camera_ind"].size - 600 and e <= 1e-9, e


# ----------------------------------------------------------------------------- 9. no side effects
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("C,N", [(16, 400), (64, 600)])
def test_covariance_leaves_the_handle_as_it_was(C, N, dtype):
    rig = make_rig(C, N, seed=29, visibility=0.6 if C > 16 else 1.0)
    args = (rig["points_2d"], rig["camera_ind"], rig["point_ind"])
    opts = dict(ftol=1e-6, max_iter=6)
    with _native.Problem(rig["cams0"], rig["pts0"], *args, dtype=dtype) as a:
        before = a.get_params()
        a.covariance()
        after = a.get_params()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        ca, pa, ra, _ = a.solve_lm(a.make_opts(**opts))
    with _native.Problem(rig["cams0"], rig["pts0"], *args, dtype=dtype) as b:
        cb, pb, rb, _ = b.solve_lm(b.make_opts(**opts))
    assert np.array_equal(ca, cb) and np.array_equal(pa, pb) and ra.cost == rb.cost


# ----------------------------------------------------------------------------- 10. degenerate points, 11. multi-rank handle
def test_single_view_point_is_nan_and_leaves_S_alone():
    rig = make_rig(6, 120, seed=37)
    prob = _solved(rig)
    cams, pts = prob.get_params()
    base = prob.covariance(scale=False)
    prob.close()
    # one more point, seen by camera 2 only
    Xn = np.array([[10.0, -20.0, 50.0]])
    from lasercalib_amd.synth import _project_np
    uv = np.vstack([rig["points_2d"], _project_np(Xn, cams[[2]])])
    ci = np.r_[rig["camera_ind"], 2]
    pi = np.r_[rig["point_ind"], 120]
    with _native.Problem(cams, np.vstack([pts, Xn]), uv, ci, pi) as p2:
        cov = p2.covariance(scale=False)
    assert cov.n_points_degenerate == 1 and np.all(np.isnan(cov.points[120]))
    assert np.all(np.isfinite(cov.points[:120]))
    assert _rel(cov.cameras, base.cameras) <= 1e-9


def test_multi_rank_handle_is_unsupported():
    rig = make_rig(4, 60, seed=41)
    with _native.Problem(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"]) as prob:
        h = prob.ipc_export(1)
        prob.ipc_attach(0, [h])
        with pytest.raises(_native.SbaError, match="status -6"):
            prob.covariance()


def test_pysba_covariance_and_uncertainty_table():
    from lasercalib_amd.pySBA import PySBA
    from lasercalib_amd import report
    rig = make_rig(5, 150, seed=43)
    sba = PySBA(rig["cams0"].copy(), rig["pts0"].copy(), rig["points_2d"], rig["camera_ind"], rig["point_ind"])
    sba.bundleAdjust(1e-8)
    cov = sba.covariance()
    assert cov.cameras.shape == (5, 11, 11) and cov.points.shape == (150, 3, 3) and cov.gauge_rank == 7
    assert cov.camera_std().shape == (5, 11) and cov.point_std().shape == (150, 3)
    assert np.all(np.isfinite(cov.camera_std()[:, 6:])) and np.all(cov.point_std() > 0)
    text = report.camera_uncertainty_table(sba, cov)
    assert len(text.splitlines()) == 6 and "+-" in text


# ----------------------------------------------------------------------------- unsorted observations with duplicates
def test_shuffled_observations_with_duplicates():
    C, N = 6, 150
    rig = make_rig(C, N, seed=59, visibility=0.8)
    rng = np.random.default_rng(5)
    M = rig["camera_ind"].size
    order = np.r_[rng.permutation(M), rng.choice(M, 25, replace=False)]      # shuffled, 25 observations twice
    uv, ci, pi = rig["points_2d"][order], rig["camera_ind"][order], rig["point_ind"][order]
    with _native.Problem(rig["cams_true"], rig["pts_true"], uv, ci, pi) as prob:
        cov = prob.covariance(scale=False)
    _r, Jc, Jp = oracle_blocks(rig["cams_true"], rig["pts_true"], uv, ci, pi)
    S, V, Wp = generic_S(Jc, Jp, ci, pi, C, N)
    Q = gauge_basis(rig["cams_true"])
    Pm = np.eye(S.shape[0]) - Q @ Q.T
    X = Pm @ _chol_inv(S + np.mean(np.diag(S)) * Q @ Q.T) @ Pm
    e_c = max(_rel(cov.cameras[c], X[c * 11:(c + 1) * 11, c * 11:(c + 1) * 11]) for c in range(C))
    e_p = max(_rel(cov.points[p], _generic_point(X, V, Wp, p, 11)) for p in range(N))
    print(f"shuffled + duplicates: camera blocks {e_c:.2e}, points {e_p:.2e}")
    assert cov.gauge_residual <= 1e-10 and e_c <= 1e-6 and e_p <= 1e-6


# ----------------------------------------------------------------------------- anchors that do not fix the datum
@pytest.mark.parametrize("case", ["one", "two", "collinear"])
def test_anchors_that_do_not_fix_the_datum_are_refused(case):
    rig = make_rig(4, 60, seed=61)
    pts = rig["pts_true"].copy()
    fixed = np.zeros(60, bool)
    fixed[:{"one": 1, "two": 2, "collinear": 4}[case]] = True
    if case == "collinear":
        pts[:4] = pts[0] + np.outer(np.arange(4.0), [10.0, -5.0, 2.0])
    with _native.Problem(rig["cams_true"], pts, rig["points_2d"], rig["camera_ind"], rig["point_ind"]) as prob:
        prob.set_fixed_points(fixed)
        with pytest.raises(_native.SbaError, match="status -1: sba_covariance: .*(datum)"):
            prob.covariance()
        ok = prob.covariance(cams_fixed=True)          # points-only covariance needs no datum
        assert ok.gauge_rank == 0 and ok.info == 0


# ----------------------------------------------------------------------------- 8b. calibrated: predicted against resampled variance
def test_predicted_focal_variance_matches_resampling():
    """Anchored solves of one rig with fresh pixel noise (sigma 0.3 px, fixed seeds): the sample variance of every camera's
    focal length lies within [0.6, 1.6] x the predicted sigma^2 (Sigma_cc)_ff.

    160 solves, not 40: the sample variance of K draws scatters by sqrt(2 / (K - 1)) -- 0.23 at K = 40, so a band of
    [0.6, 1.6] over four cameras is crossed by chance about one draw in ten (this seed's first 40 gave 0.70 0.87 0.92 0.59 on the
    device, reproduced to 1e-2 by the linearised estimator (J^T J)^-1 J^T e in numpy, whose 1000-draw ratios are 0.95 .. 1.06).
    At K = 160 the scatter is 0.11 and the band is more than 3.5 of it either side."""
    C, N = 4, 60
    rig = make_rig(C, N, seed=67, noise_px=0.0, perturb=False)
    args = (rig["camera_ind"], rig["point_ind"])
    fixed = np.zeros(N, bool)
    fixed[np.random.default_rng(3).choice(N, 8, replace=False)] = True
    with _native.Problem(rig["cams_true"], rig["pts_true"], rig["points_2d"], *args) as prob:
        prob.set_fixed_points(fixed)
        pred = 0.09 * prob.covariance(scale=False, points=False).cameras[:, 6, 6]
    rng = np.random.default_rng(71)
    fs = []
    for _ in range(160):
        uv = rig["points_2d"] + rng.normal(0.0, 0.3, rig["points_2d"].shape)
        with _native.Problem(rig["cams_true"], rig["pts_true"], uv, *args) as p:
            p.set_fixed_points(fixed)
            cams, _pts, rep, _ = p.solve_lm(p.make_opts(ftol=1e-12, xtol=1e-12, gtol=1e-12))
        fs.append(cams[:, 6])
    ratio = np.var(np.array(fs), axis=0, ddof=1) / pred
    print(f"resampled / predicted variance of f: {np.array2string(ratio, precision=2)}")
    assert np.all((ratio >= 0.6) & (ratio <= 1.6)), ratio
