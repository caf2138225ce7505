"""oracle/exact_model.py pinned before it pins anything else, and the numpy float64 models pinned by it (CPU only).

The exact reference evaluates the camera model from its definition in mpmath and differentiates it by central differences
far below float64 resolution; it shares no series and no derivative formula with sba_model.hpp or oracle/lm_schur_model.py.
Here it is checked against itself at twice the precision, against the exact-rational OpenCV vectors (F8), against the
reference's finite-difference Jacobian (F3) and against the closed form at zero rotation.  Then it checks the numpy models
per column kind, the model's damped point step, and scipy's own robust-loss functions.  Last, the numpy model's error
ratios on the cases of tests/test_gpu_exact_model.py are recomputed: they are where that file's K constants come from
(oracle/exact_cases.py: K = 16 x the largest ratio, not below 16), so the constants' origin is executable.

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


_QUANTITIES = ("blocks", "diagU", "gc", "gp", "cost", "gmax", "dp", "s_cost", "s_pred", "s_dx2", "s_x2", "s_gmax")


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
    if "huber" in name:                                      # both branches of the loss are taken, on the exact residuals
        z = xc.exact(name).r ** 2
        assert np.sum(z > 1.0) >= 12 and np.sum(z <= 1.0) >= 12
