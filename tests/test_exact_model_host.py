"""oracle/exact_model.py pinned before it pins anything else, and the numpy float64 models pinned by it (CPU only).

The exact reference evaluates the camera model from its definition in mpmath and differentiates it by central differences
far below float64 resolution; it shares no series and no derivative formula with sba_model.hpp or oracle/lm_schur_model.py.
Here it is checked against itself at twice the precision, against the exact-rational OpenCV vectors (F8), against the
reference's finite-difference Jacobian (F3) and against the closed form at zero rotation.  Then it checks the numpy models
per column kind, the model's damped point step, and scipy's own robust-loss functions.  Last, the numpy model's error
ratios on the cases of tests/test_gpu_exact_model.py are recomputed: they are where that file's K constants come from
(oracle/exact_cases.py: K = 16 x the largest ratio, not below 16), so the constants' origin is executable.  The reference of the reduced camera system (exact_model.reduced_system) is held to
0.1 eps64 d_i d_j of a full-mpmath evaluation, and numpy's float64 and LAPACK's float32 Cholesky solves of the model's own
systems are held to the a-priori backward-error bound the GPU file's part (e) uses, with what that bar can see worked out.
  The last part does the same for the other four modes (tests/test_gpu_exact_variants.py): the tie matrix
against the reference's unpacking, the tied and the squared-variant sums against full-mpmath evaluations, the model's ratios that set the new K,
and a planted error for every new bar.

Mutation check of this file (scratch copy): the coefficient 1/30 of a2_s in lm_schur_model.rodrigues_coeffs changed to 1/31
fails test_numpy_model_per_column_kind[edge11] on the rotation kinds (the cameras below the series switch).
"""
import json
import os
from fractions import Fraction

import mpmath as mp
import numpy as np
import pytest

from lasercalib_amd.synth import make_rig
from oracle import exact_cases as xc
from oracle import exact_model as ex
from oracle import lm_schur_model as model
from oracle import sba_oracle_tangential as orc13

EPS64 = xc.EPS["f64"]
_J_TOL = {"f64": 1e-6}          # tests/test_gpu_parity.py: the finite differences' own accuracy, relative to the largest entry


def test_precision_doubling_changes_no_bit():
    """Twice the digits and twice the digits of h: every returned float64 is the same, on the rig with all the edges."""
    assert ex.series_digits() >= 20.0                    # (1 - cos h) / h^2 keeps at least 20 correct digits
    for name in ("edge11", "edge13"):
        c = xc.case(name)
        r, Jc, Jp, _ = xc._blocks(name)
        r2, Jc2, Jp2 = ex.exact_blocks(c.cams, c.pts, c.uv, c.ci, c.pi, c.w, dps=2 * ex.DPS, h_digits=2 * ex.H_DIGITS)
        assert np.array_equal(r, r2) and np.array_equal(Jc, Jc2) and np.array_equal(Jp, Jp2)


def test_projection_against_exact_rational_opencv_vectors():
    """F8: OpenCV's published model in exact rational arithmetic, exact rotations.  Equal after rounding, to 1 ulp.
    (The vectors' quarter and half turns are exact; their rotation VECTORS are stored as float64(pi / 2), 6e-17 short of it,
    which alone moves a pixel by 1.5 ulp: the turn is handed over as pi / 2 at the working precision.)"""
    d = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "f8_opencv_tangential.json")))
    turns = {"identity": (0, 0), "quarter_z": (2, 0.5), "quarter_x": (0, 0.5), "half_y": (1, 1.0)}      # axis, multiple of pi
    for row in d["rows"]:
        with mp.workdps(ex.DPS):
            cam = [mp.mpf(v) for v in row["camera"]]
            axis, mult = turns[row["rotation"]]
            assert abs(row["camera"][axis] - mult * np.pi) <= 1e-15 and sum(v != 0 for v in row["camera"][:3]) == (mult != 0)
            cam[axis] = mp.pi * mp.mpf(mult)
            got = [float(v) for v in ex.project(cam, row["point"])]
        want = [float(Fraction(s)) for s in row["uv_exact"]]
        for a, b in zip(got, want):
            assert abs(a - b) <= np.spacing(abs(b)), (row["rotation"], a, b)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_blocks_against_reference_finite_differences(golden, tag):
    """F3, the reference's own scipy 3-point Jacobian: agreement at the finite differences' accuracy."""
    from scipy.sparse import csr_matrix
    g = golden("f3_jacobian.npz")
    C, N = g[f"{tag}_shape"]
    x0, ci, pi = g[f"{tag}_x0"], g[f"{tag}_ci"], g[f"{tag}_pi"]
    _, Jc, Jp = ex.exact_blocks(x0[:11 * C].reshape(C, 11), x0[11 * C:].reshape(N, 3), g[f"{tag}_uv"], ci, pi, 1.0)
    J = model.jacobian_csr(Jc, Jp, ci, pi, C, N)
    Jref = csr_matrix((g[f"{tag}_J_data"], g[f"{tag}_J_indices"], g[f"{tag}_J_indptr"]), shape=J.shape)
    assert abs(J - Jref).max() <= _J_TOL["f64"] * abs(Jref).max()


def test_zero_rotation_block_is_the_closed_form():
    """At rho = 0, dP/drho = -[X]x: the rotation block is A (-[X]x) with A = d r / d t, the exact translation block."""
    c = xc.case("edge11")
    _, Jc, _, _ = xc._blocks("edge11")
    sel = np.nonzero(c.ci == 0)[0]
    assert np.all(c.cams[0, 0:3] == 0.0) and sel.size == c.N
    for m in sel:
        X = c.pts[c.pi[m]]
        Xx = np.array([[0.0, -X[2], X[1]], [X[2], 0.0, -X[0]], [-X[1], X[0], 0.0]])
        A = Jc[m, :, 3:6]
        bound = 8 * EPS64 * (np.abs(A) @ np.abs(Xx))         # two products and one sum per entry, rounded inputs
        assert np.all(np.abs(Jc[m, :, 0:3] - A @ (-Xx)) <= bound)


def _kind_ratios(J, Jx):
    return np.array([np.max(np.abs(J[:, :, k] - Jx[:, :, k])) / max(np.max(np.abs(Jx[:, :, k])), 1e-300) for k in range(Jx.shape[2])])


@pytest.mark.parametrize("name", ["edge11", "edge13", "m9x40", "t5x30"])
def test_numpy_model_per_column_kind(name):
    """lm_schur_model.residual_jacobian: every column kind within 64 eps64 of that kind's largest exact entry (observed: at
    most 10.4 eps64 on the rotation columns of the edge rig, 0 for cx and cy); the residual within 1e-11 px."""
    c = xc.case(name)
    r, Jc, Jp, _ = xc._blocks(name)
    r_m, Jc_m, Jp_m = model.residual_jacobian(c.cams, c.pts, c.uv, c.ci, c.pi, c.w)
    assert np.max(np.abs(r_m - r)) <= 1e-11
    kc, kp = _kind_ratios(Jc_m, Jc), _kind_ratios(Jp_m, Jp)
    assert np.all(kc <= 64 * EPS64) and np.all(kp <= 64 * EPS64), (kc / EPS64, kp / EPS64)
    assert np.array_equal(Jc_m[:, :, c.ncp - 2:], Jc[:, :, c.ncp - 2:])               # cx, cy columns: w and 0 exactly
    if name == "edge11":      # the cameras on either side of the series switch, each on its own
        for cam in (0, 1, 2):
            s = c.ci == cam
            assert np.all(_kind_ratios(Jc_m[s], Jc[s]) <= 64 * EPS64), cam


@pytest.mark.parametrize("name", ["edge13", "t5x30"])
def test_tangential_oracle_finite_differences_per_column_kind(name):
    """oracle/sba_oracle_tangential.fd_jacobian (scipy 3-point) at its own accuracy, but per column kind."""
    c = xc.case(name)
    _, Jc, Jp, _ = xc._blocks(name)
    x0 = np.hstack((c.cams.ravel(), c.pts.ravel()))
    Jfd = orc13.fd_jacobian(x0, c.C, c.N, c.ci, c.pi, c.uv, c.w.reshape(-1, 1)).tocsc()
    J = model.jacobian_csr(Jc, Jp, c.ci, c.pi, c.C, c.N).tocsc()
    kind = np.concatenate([np.tile(np.arange(13), c.C), 13 + np.tile(np.arange(3), c.N)])
    for k in range(16):
        cols = np.nonzero(kind == k)[0]
        assert abs(J[:, cols] - Jfd[:, cols]).max() <= _J_TOL["f64"] * abs(J[:, cols]).max(), k


@pytest.mark.parametrize("C,N,vis,lam", [(16, 40, 1.0, 1e-4), (9, 50, 0.6, 1e-4), (24, 20, 0.8, 1e-4), (5, 30, 0.8, 1e-2)])
def test_point_step_against_model_engine(C, N, vis, lam):
    """exact_model.point_step fed the exact blocks and the MODEL'S camera step against ModelEngine.solve_trial's dp.
    Observed: relative <= 1.3e-13 with cond(V') <= 13.  cond(V') <= 1e3 is what the GPU cases rely on."""
    rig = make_rig(C, N, seed=7 + C, visibility=vis, min_cams_per_point=2)
    cams, pts, uv = xc.f32(rig["cams0"]), xc.f32(rig["pts0"]), xc.f32(rig["points_2d"])
    ci, pi = rig["camera_ind"], rig["point_ind"]
    w = xc.f32(np.random.default_rng(0).uniform(0.5, 1.5, ci.size))
    eng = model.ModelEngine(cams, pts, uv, ci, pi, w=w)
    eng.lam = lam
    eng.linearize()
    sc = eng.solve_trial(eng.form_reduced())
    eng.decide(sc[None, :], 1)
    assert eng.accepted and 0.5 < eng.rho < 1.5
    r, Jc, Jp = ex.exact_blocks(cams, pts, uv, ci, pi, w)
    s = ex.normal_sums(r, Jc, Jp, ci, pi, C, N)
    D = ex.damping_diagonal(s["V"])
    t, _ = ex.wt_dc(Jc, Jp, ci, pi, eng.dc, N)
    dp = ex.point_step(s["V"], s["gp"], t, lam, D)
    Vd = s["V"] + lam * D[:, :, None] * np.eye(3)[None]
    assert max(np.linalg.cond(Vd[p]) for p in range(N)) <= 1e3
    rel = np.linalg.norm(dp - eng.dp, axis=1) / np.linalg.norm(dp, axis=1)
    assert np.max(rel) <= 1e-11, np.max(rel)
    fixed = np.arange(N) % 3 == 0
    assert np.all(ex.point_step(s["V"], s["gp"], t, lam, D, fixed)[fixed] == 0.0)


@pytest.mark.parametrize("loss", ["huber", "soft_l1", "cauchy"])
def test_robust_rows_against_scipy_rho(loss):
    """Value and first derivative of rho against scipy.optimize.least_squares' own functions, below, at and above z = 1;
    rows and residual scaled by sqrt(rho'), the cost terms f_scale^2 rho."""
    from scipy.optimize._lsq.least_squares import IMPLEMENTED_LOSSES
    f_scale = 1.5
    r = np.array([[0.3, -1.2], [1.5, -1.5], [4.0, 40.0], [1.4999, 1.5001]]) * 1.0
    z = (r / f_scale) ** 2
    rho = np.empty((3,) + z.shape)
    IMPLEMENTED_LOSSES[loss](z.copy(), rho, cost_only=False)
    Jc = np.arange(r.size * 11, dtype=np.float64).reshape(r.shape[0], 2, 11) + 1.0
    Jp = np.arange(r.size * 3, dtype=np.float64).reshape(r.shape[0], 2, 3) - 2.5
    rs, Jcs, Jps, terms, scale = ex.robust_rows(r, Jc, Jp, loss, f_scale)
    for m in range(r.shape[0]):
        for k in range(2):
            with mp.workdps(ex.SUM_DPS):
                v, d = (float(x) for x in ex.rho_functions(z[m, k], loss))
            # (scipy's soft_l1 is 2 (sqrt(1 + z) - 1), a difference of values of size sqrt(1 + z): its own rounding sets the bar)
            assert abs(v - rho[0, m, k]) <= 4 * EPS64 * max(abs(v), np.sqrt(1 + z[m, k])) and abs(d - rho[1, m, k]) <= 4 * EPS64 * abs(d)
    assert np.allclose(terms, f_scale ** 2 * rho[0], rtol=8 * EPS64, atol=8 * EPS64 * f_scale ** 2)
    assert np.allclose(scale, np.sqrt(rho[1]), rtol=8 * EPS64, atol=0)
    assert np.allclose(rs, r * np.sqrt(rho[1]), rtol=8 * EPS64, atol=0)
    assert np.allclose(Jcs, Jc * np.sqrt(rho[1])[:, :, None], rtol=8 * EPS64, atol=0)
    assert np.allclose(Jps, Jp * np.sqrt(rho[1])[:, :, None], rtol=8 * EPS64, atol=0)
    if loss == "huber":
        assert np.all(scale[z <= 1] == 1.0) and np.all(scale[z > 1] < 1.0)           # both branches
    lin = ex.robust_rows(r, Jc, Jp, "linear", 0.0)
    assert np.array_equal(lin[0], r) and np.array_equal(lin[1], Jc) and np.allclose(lin[3], r * r, rtol=2 * EPS64, atol=0)


_QUANTITIES = ("blocks", "diagU", "gc", "gp", "cost", "gmax", "dp", "s_cost", "s_pred", "s_dx2", "s_x2", "s_gmax", "S", "rhs")


@pytest.mark.parametrize("name", xc.ALL_CASES)
def test_numpy_model_ratios_stay_under_K_over_16(name):
    """Where K comes from: the numpy float64 model on the GPU file's own cases, error / (eps64 * scale) per quantity, must
    stay under K / 16.  (Sums (b) are compared on the base cases; under the Huber loss diagU is not a plain sum of squares
    of exactly known rows -- the row scale carries the residual's cancellation -- and is compared nowhere.)"""
    q = xc.model_quantities(name)
    assert q["rho"] > 0.25, q["rho"]                         # the trial is one the LM control accepts
    R = xc.ratios(name, q, EPS64)
    assert R["cond"] <= 1e3 and R["fixed_zero"]
    assert R["r_abs"] <= 1e-11
    for k in _QUANTITIES:
        if name in xc.VARIANT_CASES and k in ("diagU", "gc", "gp", "cost", "gmax"):
            continue
        assert R[k] <= xc.K[k] / 16.0, (k, R[k], xc.K[k] / 16.0)
    if xc.case(name).loss == "linear":
        assert R["S"] <= xc.K["S_lin"] / 16.0, (R["S"], xc.K["S_lin"] / 16.0)
    assert R["S_outside"] == 0.0
    if "huber" in name:                                      # both branches of the loss are taken, on the exact residuals
        z = xc.exact(name).r ** 2
        assert np.sum(z > 1.0) >= 12 and np.sum(z <= 1.0) >= 12


def test_reduced_system_reference_against_full_mpmath():
    """exact_model.reduced_system sums S in np.longdouble from mpmath factors; on the smallest case (t5x30, n = 65) it must agree
    with the evaluation that forms V'^-1 by mpmath's inverse and every sum in mpmath to 0.1 eps64 d_i d_j (observed: 1e-3), and the
    right-hand sides, both in mpmath throughout, bit for bit.  The float64 S is the longdouble one rounded."""
    E = xc.exact("t5x30")
    c = E.case
    X = xc.reduced("t5x30")
    F = ex.reduced_system(E.Jcs, E.Jps, E.rs, c.ci, c.pi, c.C, c.N, xc.LAMBDA0, c.fixed, full_mp=True)
    n = c.C * c.ncp
    assert X.S.shape == (n, n) == (65, 65)
    dd = np.outer(X.d, X.d)
    assert np.max(np.abs((X.S_ld - F["S_ld"]).astype(np.float64)) / dd) <= 0.1 * EPS64
    assert np.array_equal(X.rhs, F["rhs"]) and np.array_equal(X.S, X.S_ld.astype(np.float64)) and np.array_equal(X.S, X.S.T)
    dU = np.sqrt(E.diagU).ravel()                                            # d is the root of the exact diag U, rounded once
    assert np.all(np.abs(X.d - dU) <= np.spacing(dU))
    # Cauchy-Schwarz, the reason d_i d_j is the scale: no entry of S and no term sum exceeds it by more than the damping allows
    assert np.max(np.abs(X.S) / dd) <= 1.0 and np.all(np.abs(X.S) <= X.S_mag * (1 + 8 * EPS64))


def test_reduced_system_of_fixed_points_and_damping():
    """Fixed points leave the Schur sums but stay in U and g_c; the damping lam D_p sits inside V' (S moves with lam)."""
    E = xc.exact("t5x30")
    c = E.case
    fixed = (np.arange(c.N) % 5) == 1
    args = (E.Jcs, E.Jps, E.rs, c.ci, c.pi, c.C, c.N)
    A = xc.reduced("t5x30")
    Fx = ex.reduced_system(*args, xc.LAMBDA0, fixed)
    keep = ~fixed[c.pi]
    sub = ex.reduced_system(E.Jcs[keep], E.Jps[keep], E.rs[keep], c.ci[keep], c.pi[keep], c.C, c.N, xc.LAMBDA0)
    dd = np.outer(A.d, A.d)
    # (U - Schur over the free points) = (system of the free points' observations alone) + (U and g_c of the fixed points' observations)
    s = ex.normal_sums(E.rs[~keep], E.Jcs[~keep], E.Jps[~keep], c.ci[~keep], c.pi[~keep], c.C, c.N)
    assert np.max(np.abs(np.diag(Fx["S"]) - np.diag(sub["S"]) - s["diagU"].ravel()) / np.diag(dd)) <= 4 * EPS64
    assert np.max(np.abs(Fx["rhs"] - sub["rhs"] + s["gc"].ravel()) / xc.rhs_scale("t5x30", EPS64)) <= 4 * EPS64
    assert np.max(np.abs(Fx["S"] - A.S) / dd) > 1e-3                            # the fixed points' Schur terms are gone
    undamped = ex.reduced_system(*args, 0.0)
    assert np.max(np.abs(undamped["S"] - A.S) / dd) > 1e-4                      # lam = 1e-2 inside V' is visible at 1e-4 d_i d_j


@pytest.mark.parametrize("name", xc.ALL_CASES)
def test_numpy_cholesky_solves_stay_under_the_a_priori_bound(name):
    """The bar of the GPU file's part (e) on the host: dc of numpy's float64 Cholesky (the model's) and of LAPACK's float32
    Cholesky with triangular solves, each as a solution of the model's own damped system, under solve_bound(n, eps) (Higham Thm
    10.3 / 10.4; the f32 run also narrows A and rhs: eps32).  Observed: at most 92 eps64 (t16x12) of 197 .. 1124, and 0.25 eps32.
    The longdouble evaluation of the residual stays below 1 % of either bar."""
    from scipy.linalg import cholesky, solve_triangular
    q = xc.model_quantities(name)
    n = q["S"].shape[0]
    R = xc.ratios(name, {k: q[k] for k in ("S", "rhs", "diagU", "dc")}, EPS64)
    B64 = xc.solve_bound(n, EPS64)
    assert R["dc_bwd"] <= B64 and R["dc_bwd_host"] <= 0.01 * B64, (R["dc_bwd"] / EPS64, B64 / EPS64)
    dU = q["diagU"].ravel()
    damp = xc.LAMBDA0 * np.where(dU > 0, dU, 1.0)
    A32 = (q["S"] + np.diag(damp)).astype(np.float32)
    L = cholesky(A32, lower=True)
    x = solve_triangular(L, solve_triangular(L, q["rhs"].astype(np.float32), lower=True), lower=True, trans="T")
    assert L.dtype == np.float32 and x.dtype == np.float32
    e32 = xc.EPS["f32"]
    bwd, own = xc.backward_error(q["S"], q["rhs"], damp, x.astype(np.float64))
    B32 = xc.solve_bound(n, e32, e32)
    assert bwd <= B32 and own <= 0.01 * B32, (bwd / e32, B32 / e32)
    # what the bars see: an error of e in the component with the largest d_k |dc_k| leaves e times that component's share of
    # sum_j d_j |dc_j| (0.011 .. 0.071 on these cases) in row k.  1e-10 of it misses the f64 bar, 5 % the f32 bar.
    k = int(np.argmax(np.abs(q["dc"].ravel()) * np.sqrt(np.diag(q["S"]) + damp)))
    for rel, bar in ((1e-10, B64), (5e-2, B32)):
        bad = q["dc"].ravel().copy()
        bad[k] *= 1.0 + rel
        assert xc.backward_error(q["S"], q["rhs"], damp, bad)[0] > bar


# ============================================================================ the other four modes (tests/test_gpu_exact_variants.py)
def test_tie_matrix_is_the_reference_unpack():
    """T x is the reference's own unpacking of its shared-intrinsics parameter vector (oracle/sba_oracle.unpack_sharedcam, pySBA.py:313);
    with 13 parameters the per-camera tail is [p1, p2, cx, cy]."""
    from oracle import sba_oracle as orc11
    for C in (1, 5, 16):
        nt = 3 + 8 * C
        x = np.arange(nt) + 1.0
        T = ex.tie_matrix(C, 11)
        cams, off = orc11.unpack_sharedcam(np.concatenate([x, np.zeros(3)]), C)
        assert off == nt and T.shape == (11 * C, nt) and np.array_equal((T @ x).reshape(C, 11), cams)
        assert np.all(T.sum(axis=1) == 1) and np.array_equal(T.sum(axis=0), np.r_[np.full(3, C), np.ones(nt - 3)])
        nt = 3 + 10 * C
        x = np.arange(nt) + 1.0
        cams = (ex.tie_matrix(C, 13) @ x).reshape(C, 13)
        assert np.array_equal(cams[:, 6:9], np.tile(x[:3], (C, 1))) and np.array_equal(cams[:, :6], x[3:3 + 6 * C].reshape(C, 6))
        assert np.array_equal(cams[:, 9:], x[3 + 6 * C:].reshape(C, 4))


def test_tied_system_against_full_mpmath():
    """exact_model.tied_system sums T^T S T in np.longdouble; on t5x30 (65 -> 53 unknowns, the shared 3 x 3 block sums 25 entries) it
    agrees with the same sums in mpmath to 0.1 eps64 of T^T (d d^T) T (observed: 2e-4), the vectors likewise."""
    E, X = xc.exact("t5x30"), xc.reduced("t5x30")
    T = ex.tie_matrix(5, 13)
    A = ex.tied_system(T, X.S_ld, X.rhs, E.diagU, E.gc)
    F = ex.tied_system(T, X.S_ld, X.rhs, E.diagU, E.gc, full_mp=True)
    dd = T.T @ np.outer(X.d, X.d) @ T
    assert A["S"].shape == (53, 53) and np.array_equal(A["S"], A["S"].T)
    assert np.max(np.abs((A["S_ld"] - F["S_ld"]).astype(np.float64)) / dd) <= 0.1 * EPS64
    with mp.workdps(ex.SUM_DPS):
        for key, v, scale in (("rhs", X.rhs, T.T @ xc.rhs_scale("t5x30", EPS64)), ("g", E.gc, T.T @ E.gc_mag.ravel()), ("diagU", E.diagU, T.T @ E.diagU.ravel())):
            want = np.array([float(mp.fsum([mp.mpf(float(x)) for x in np.ravel(v)[T[:, a] > 0]])) for a in range(53)])
            assert np.max(np.abs(A[key] - want) / scale) <= EPS64, key          # rounded once: half an ulp of the sum itself
    t = xc.tied("t5x30")
    assert np.array_equal(t.S, A["S"]) and np.array_equal(t.g, A["g"])


@pytest.mark.parametrize("name,kind", [("edge11", "cams"), ("t5x30", "affine")])
def test_squared_variant_sums_against_full_mpmath(name, kind):
    """exact_model.sq_system sums the products of its mpmath rows in np.longdouble; against every sum in mpmath: H to 0.1 eps64 h_i h_j,
    g and the cost to 0.1 eps64 of their scales (observed: at most 4e-3)."""
    c = xc.case(name)
    X = xc.sq_exact(name, kind)
    F = ex.sq_system(X.delta, X.Jc, X.Jp, c.w, c.ci, c.pi, c.pts, c.C, kind, full_mp=True)
    g_s, cost_s = xc.sq_scales(name, kind, EPS64)
    hh = X.h[:, :, None] * X.h[:, None, :]
    assert X.H.shape == ((6, 11, 11) if kind == "cams" else (1, 12, 12))
    assert np.max(np.abs((X.H_ld - F["H_ld"]).astype(np.float64)) / hh) <= 0.1 * EPS64
    assert np.max(np.abs((X.g_ld - F["g_ld"]).astype(np.float64)) / g_s) <= 0.1 * EPS64
    assert abs(float(X.cost_ld - F["cost_ld"])) / cost_s <= 0.1 * EPS64
    assert np.max(np.abs(X.H) / hh) <= 1.0 + 4 * EPS64 and np.all(np.abs(X.g) <= g_s * (1 + 4 * EPS64))      # Cauchy-Schwarz; the scale bounds g
    # rho = w Delta^2 of the UNWEIGHTED pixel error: with the weights of the case, w Delta is the residual of the weighted blocks
    r = xc._blocks(name)[0]
    assert np.max(np.abs(c.w[:, None] * X.delta - r) / np.abs(r).max()) <= 4 * EPS64
    assert np.max(np.abs(X.rho - c.w[:, None] * X.delta ** 2) / X.rho.max()) <= 4 * EPS64


_VARIANT_Q = ("dp", "s_cost", "s_pred", "s_dx2", "s_x2", "s_gmax")


@pytest.mark.parametrize("name", xc.POINTS_ONLY_CASES)
def test_numpy_model_of_a_points_only_trial(name):
    """The model's ratios of a points-only trial (dc = 0) against the recorded MODEL_MAX_VARIANT, and those under the bars K in use."""
    q = xc.model_quantities(name, mode="points")
    assert q["rho"] > 0.25 and not np.any(q["dc"]) and np.array_equal(q["cams_new"], xc.case(name).cams)
    R = xc.ratios(name, {k: q[k] for k in ("dc", "dp", "cams_new", "pts_new", "scal")}, EPS64)
    assert R["cond"] <= 1e3 and R["fixed_zero"]
    for k in _VARIANT_Q:
        assert R[k] <= xc.MODEL_MAX_VARIANT["points"][k] <= xc.K[k], (k, R[k])


@pytest.mark.parametrize("name", xc.SHARED_CASES)
def test_numpy_model_of_a_shared_intrinsics_trial(name):
    """The model's tied trial: ratios against MODEL_MAX_VARIANT and under K; its ds under the a-priori bound of every route the device
    takes; and what bar (ii) sees: one term S[f of camera 1, f of camera 2] left out of the sum for S_s[f, f] (one `ib` term of
    k_tie_system) before the solve misses the f64 bar by 4e7 and more, and the f32 bar by a factor 3.9 .. 5 on d16x24, t18x12 and m9x40;
    on g24x10 and v34x6 that one term (two cameras with few common points) stays at 0.08 of the f32 bar: the f32 engine's bar sees a
    wrong tied sum only from about 1e-5 of d_i d_j on."""
    c = xc.case(name)
    q = xc.model_quantities(name, mode="shared")
    assert q["rho"] > 0.25 and np.all(q["dc"][:, 6:9] == q["dc"][0, 6:9])
    R = xc.ratios(name, {k: q[k] for k in ("S", "rhs", "dc", "dp", "cams_new", "pts_new", "scal")}, EPS64)
    for k in ("S", "rhs") + _VARIANT_Q:
        assert R[k] <= xc.MODEL_MAX_VARIANT["shared"][k] <= xc.K[k], (k, R[k])
    assert R["S"] <= xc.K["S_lin"] / 16.0
    ds, bwd, own = xc.tied_backward_error(name, q["S"], q["rhs"], q["diagU"], q["dc"])
    B64, what64, r64 = xc.tied_solve_bound("f64", name)
    B32, what32, r32 = xc.tied_solve_bound("f32", name)
    assert np.array_equal(ds, q["ds"]) and bwd <= B64 and own <= 0.01 * B64, (bwd / EPS64, B64 / EPS64)
    n, nt = c.C * c.ncp, ds.size
    assert (r64, r32) == {131: ("BLOCKED", "BLOCKED"), 195: ("LL", "LL_F32"), 275: ("BIG_DAG", "BIG_DAG_F32"), 183: ("LL", "LL_F32"),
                          75: ("BLOCKED", "BLOCKED")}[nt]
    assert xc.chol_route("f64", n) == {176: "BLOCKED", 264: "BIG_DAG", 374: "BIG_DAG", 234: "LL", 99: "BLOCKED"}[n]
    T = ex.tie_matrix(c.C, c.ncp)
    dU = T.T @ q["diagU"].ravel()
    A = T.T @ q["S"] @ T + np.diag(xc.LAMBDA0 * np.where(dU > 0, dU, 1.0))
    A[0, 0] -= q["S"][1 * c.ncp + 6, 2 * c.ncp + 6]
    bad = np.linalg.solve(A, T.T @ q["rhs"])
    seen = xc.tied_backward_error(name, q["S"], q["rhs"], q["diagU"], (T @ bad).reshape(c.C, c.ncp))[1]
    print(f"\n[exact] tied model {name}: ds_bwd={bwd / EPS64:.3g} eps64, B64={B64 / EPS64:.4g} eps64, B32={B32 / xc.EPS['f32']:.4g} eps32, one term dropped: {seen / B32:.3g} x B32")
    assert seen > 1e6 * B64 and (seen > 2 * B32 or name.startswith(("g24x10", "v34x6")))


@pytest.mark.parametrize("name", xc.SHARED_GTOL_CASES)
def test_tied_gradient_maximum_and_what_its_bar_sees(name):
    """max |g| in the tied unknowns: the model under K / 16; the untied maximum misses the f32 bar by more than a factor 1e3."""
    q = xc.model_quantities(name, mode="shared")
    E, t = xc.exact(name), xc.tied(name)
    assert xc.ratios(name, dict(gmax_tied=q["gmax_tied"]), EPS64)["gmax_tied"] <= xc.K["gmax_tied"] / 16.0
    assert int(np.argmax(np.abs(t.g))) == 1 and np.max(np.abs(t.g)) > 1.3 * np.max(np.abs(E.gc)) > np.max(np.abs(E.gp))
    assert xc.ratios(name, dict(gmax_tied=q["gmax"]), xc.EPS["f32"])["gmax_tied"] > 1e3 * xc.K["gmax_tied"]


_SQ_Q = {"cams": ("H", "g", "cost", "lam", "res", "tcost"), "affine": ("cost", "lam", "res", "tcost")}


@pytest.mark.parametrize("name,kind", [(n, "cams") for n in xc.SQ_CAMS_CASES] + [(n, "affine") for n in xc.SQ_AFFINE_CASES])
def test_numpy_model_of_a_squared_variant_trial(name, kind):
    """Where the K of the squared variants come from, and what each bar sees (all at eps32, the wider bar): the factor 2 of the rows
    turned into 1 (H, g, the step's residual); the last observation left out of the sums (H and g, or the affine's residual); the
    trial cost evaluated at the old parameters (a theta read from the wrong buffer); lambda from tau x the smallest diagonal entry."""
    c = xc.case(name)
    q = xc.sq_model(name, kind)
    assert q["gain"] > 0.25                                   # the LM control accepts the trial
    R = xc.sq_ratios(name, kind, q, EPS64)
    assert abs(R["gain_exact"] - q["gain"]) <= 1e-6
    for k in _SQ_Q[kind]:
        assert R[k] <= xc.K[f"sq_{kind}_{k}"] / 16.0, (k, R[k])
    if kind == "affine":                                      # the step read back from the stored theta: the allowance covers the rounding
        th = xc.IDENT12 + q["x"].ravel()
        assert xc.sq_ratios(name, kind, dict(theta=th, tcost=q["tcost"]), EPS64)["res"] <= xc.K["sq_affine_res"] / 16.0
    e32 = xc.EPS["f32"]
    X = xc.sq_exact(name, kind)
    lam_x = xc.SQ_TAU * float(np.max(np.einsum("gii->gi", X.H)))
    half = xc.sq_model(name, kind, row_factor=1.0)
    solve = lambda H, g: np.stack([np.linalg.solve(H[k] + lam_x * np.eye(H.shape[1]), -g[k]) for k in range(H.shape[0])])      # noqa: E731
    bad = xc.sq_ratios(name, kind, dict(H=half["H"], g=half["g"], x=solve(half["H"], half["g"]), tcost=q["cost"],
                                        lam=xc.SQ_TAU * float(np.min(np.einsum("gii->gi", X.H)))), e32)
    for k in ("H", "g", "res", "tcost", "lam"):
        assert bad[k] > xc.K.get(f"sq_{kind}_{k}", xc.K["sq_cams_" + k]), (k, bad[k])
    m = c.M - 1                                               # the last observation dropped from the sums
    rows = xc.sq_model(name, kind)
    d1 = ex.sq_system(X.delta[m:], X.Jc[m:], X.Jp[m:], c.w[m:], c.ci[m:], np.zeros(1, np.int64), c.pts[c.pi[m:]], c.C, kind)
    Hl, gl = rows["H"] - d1["H"], rows["g"] - d1["g"]
    lost = xc.sq_ratios(name, kind, dict(H=Hl, g=gl, x=solve(Hl, gl), tcost=q["tcost"]), e32)
    for k in (("H", "g") if kind == "cams" else ("res",)):
        assert lost[k] > xc.K[f"sq_{kind}_{k}"], (k, lost[k])
