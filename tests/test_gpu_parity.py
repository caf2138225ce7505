"""GPU parity tests: every call goes through the C ABI (libsba_hip.so) and is checked against the
oracle (oracle/sba_oracle.py = the reference's algorithm restated), the committed golden fixtures
(produced by the reference itself) and, at full size, size-independent properties.

Tolerances (stated once, used below):
  fp64 device path   residual / projection  <= 1e-9 px absolute (values ~1e3 px => ~1e-12 relative)
                     analytic Jacobian vs the reference's scipy 3-point FD Jacobian <= 1e-6 relative to max|J|
                     converged cost vs reference at its own ftol: relative <= 1e-5, RMS reprojection <= 1e-4 px
  fp32 device path   residual <= 2e-3 px, converged cost relative <= 1e-4, RMS <= 1e-3 px
"""
import os
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from lasercalib_amd import _native  # noqa: E402
from lasercalib_amd.pySBA import PySBA, assemble_jacobian  # noqa: E402
from lasercalib_amd.synth import make_rig  # noqa: E402
from oracle import lm_schur_model as model  # noqa: E402
from oracle import sba_oracle as orc  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert _native.device_count() > 0, "no HIP device visible: GPU tests must run on the MI355X box"


def _problem(rig, dtype="f64", weights=None, cams=None, pts=None):
    return _native.Problem(rig["cams0"] if cams is None else cams, rig["pts0"] if pts is None else pts,
                           rig["points_2d"], rig["camera_ind"], rig["point_ind"], weights=weights, dtype=dtype)


# ----------------------------------------------------------------------------- F1: rotate / project
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_project_rotate_golden(golden, dtype):
    g = golden("f1_project.npz")
    rot = _native.rotate_rows(g["points"], g["cam_rows"][:, :3], dtype=dtype)
    uv = _native.project_rows(g["points"], g["cam_rows"], dtype=dtype)
    near = slice(128, 160)       # rows that put points a few cm from the camera: pixel values up to 1e10, compared relatively
    far = np.r_[0:128, 160:g["points"].shape[0]]
    if dtype == "f64":
        assert np.max(np.abs(rot - g["rotated"])) <= 1e-9
        scale = np.maximum(1.0, np.abs(g["projected"]) / 1e3)
        assert np.max(np.abs(uv - g["projected"]) / scale) <= 1e-7
        return
    # fp32: a-priori rounding bound, 4 eps32 (|uv| + f cond^2) per row with cond = |p| / p_z of the camera-frame point
    # (observed: at most 1.0 of the un-multiplied bound, 5e-4 px), coordinates up to 1.7e3 mm for the rotation
    eps = float(np.finfo(np.float32).eps)
    assert np.max(np.abs(rot - g["rotated"])) <= 4 * eps * 1.7e3
    pc = g["rotated"] + g["cam_rows"][:, 3:6]
    cond = np.linalg.norm(pc, axis=1) / np.abs(pc[:, 2])
    bound = 4 * eps * (np.max(np.abs(g["projected"]), axis=1) + g["cam_rows"][:, 6] * cond * cond)
    err = np.max(np.abs(uv - g["projected"]), axis=1)
    assert np.all(err[far] <= bound[far]) and np.max(err[far]) <= 3e-3
    assert np.max(np.abs(uv[near] - g["projected"][near]) / np.maximum(1.0, np.abs(g["projected"][near]))) <= 0.5


def test_project_theta_zero_is_identity():
    pts = np.array([[1.0, 2.0, 3.0], [-4.0, 5.0, 6.0]])
    rot = _native.rotate_rows(pts, np.zeros((2, 3)))
    assert np.array_equal(rot, pts)          # pySBA.py:66-68: theta = 0 leaves the point unchanged


def test_project_empty():
    assert _native.project_rows(np.zeros((0, 3)), np.zeros((0, 11))).shape == (0, 2)


def test_pysba_project_matches_oracle_like_sba_print_does():
    # the call sba_print.py:17 makes: numpy fancy-indexed arguments
    rig = make_rig(5, 300, seed=4, visibility=0.7)
    sba = PySBA(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"])
    got = sba.project(sba.points3D[sba.point2DIndices], sba.cameraArray[sba.cameraIndices]) - sba.points2D
    ref = orc.project(rig["pts0"][rig["point_ind"]], rig["cams0"][rig["camera_ind"]]) - rig["points_2d"]
    assert got.shape == ref.shape and np.max(np.abs(got - ref)) <= 1e-9


# ----------------------------------------------------------------------------- F2: fun
@pytest.mark.parametrize("tag", ["a", "b"])
@pytest.mark.parametrize("wtag", ["unit", "w"])
def test_residual_golden_f64(golden, tag, wtag):
    g = golden("f2_fun.npz")
    C, N = g[f"{tag}_shape"]
    x0 = g[f"{tag}_x0"]
    w = g[f"{tag}_w"] if wtag == "w" else None
    with _native.Problem(x0[:11 * C].reshape(C, 11), x0[11 * C:].reshape(N, 3), g[f"{tag}_uv"], g[f"{tag}_ci"],
                         g[f"{tag}_pi"], weights=w) as prob:
        r, cost = prob.residual()
        r2, _ = prob.residual(x0)                  # explicit-x path
    ref = g[f"{tag}_{wtag}_res"]
    assert np.max(np.abs(r - ref)) <= 1e-9
    assert np.array_equal(r, r2)
    assert abs(cost - 0.5 * ref @ ref) <= 1e-9 * (0.5 * ref @ ref)


def test_residual_f32(golden):
    g = golden("f2_fun.npz")
    C, N = g["a_shape"]
    x0 = g["a_x0"]
    with _native.Problem(x0[:11 * C].reshape(C, 11), x0[11 * C:].reshape(N, 3), g["a_uv"], g["a_ci"], g["a_pi"],
                         dtype="f32") as prob:
        r, cost = prob.residual()
    ref = g["a_unit_res"]
    assert np.max(np.abs(r - ref)) <= 5e-3
    assert abs(cost - 0.5 * ref @ ref) <= 1e-4 * (0.5 * ref @ ref)


def test_pysba_fun_and_getResiduals_quirk(golden):
    g = golden("f2_fun.npz")
    C, N = g["b_shape"]
    x0 = g["b_x0"]
    sba = PySBA(x0[:11 * C].reshape(C, 11).copy(), x0[11 * C:].reshape(N, 3).copy(), g["b_uv"], g["b_ci"], g["b_pi"],
                pointWeights=g["b_w"])
    r = sba.fun(x0, C, N, sba.cameraIndices, sba.point2DIndices, sba.points2D, sba.pointWeights)
    assert np.max(np.abs(r - g["b_w_res"])) <= 1e-9
    with pytest.raises(ValueError):                 # reference bug kept: pySBA.py:207-213 broadcasts (M,) against (M,2)
        sba.getResiduals()


def test_unsorted_observations_keep_caller_order():
    rig = make_rig(4, 150, seed=9, visibility=0.8)
    rng = np.random.default_rng(1)
    shuf = rng.permutation(rig["point_ind"].size)
    ref = orc.fun(np.hstack((rig["cams0"].ravel(), rig["pts0"].ravel())), 4, 150, rig["camera_ind"][shuf],
                  rig["point_ind"][shuf], rig["points_2d"][shuf], 1.0)
    with _native.Problem(rig["cams0"], rig["pts0"], rig["points_2d"][shuf], rig["camera_ind"][shuf],
                         rig["point_ind"][shuf]) as prob:
        r, _ = prob.residual()
        _, Jc, Jp = prob.residual_jacobian()
    assert np.max(np.abs(r - ref)) <= 1e-9
    _, Jc_m, Jp_m = model.residual_jacobian(rig["cams0"], rig["pts0"], rig["points_2d"][shuf], rig["camera_ind"][shuf],
                                            rig["point_ind"][shuf], 1.0)
    assert np.max(np.abs(Jc - Jc_m)) <= 1e-7 and np.max(np.abs(Jp - Jp_m)) <= 1e-7


# ----------------------------------------------------------------------------- F3: Jacobian
# fp32 bound: the blocks are ~60 dependent f32 operations on values conditioned like the projection itself; every entry
# is held to 2e-5 of the largest entry of its own COLUMN KIND (rotation / translation / f / k1 / k2 / centre / point), the
# same a-priori form as the fp32 `project` bound above.  Observed on F3: 1.5e-6 (a), 1.2e-6 (b) of max|J|.
_J_TOL = {"f64": 1e-6, "f32": 2e-5}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_jacobian_vs_reference_fd(golden, tag, dtype):
    """Both instantiations of the materialising kernel (k_resjac<double>, k_resjac<float> -- the one bench.py's
    `roofline_resjac` times) against the reference's own 3-point finite-difference Jacobian (F3)."""
    from scipy.sparse import csr_matrix
    g = golden("f3_jacobian.npz")
    C, N = g[f"{tag}_shape"]
    x0 = g[f"{tag}_x0"]
    with _native.Problem(x0[:11 * C].reshape(C, 11), x0[11 * C:].reshape(N, 3), g[f"{tag}_uv"], g[f"{tag}_ci"],
                         g[f"{tag}_pi"], dtype=dtype) as prob:
        r, Jc, Jp = prob.residual_jacobian()
    J = assemble_jacobian(Jc, Jp, g[f"{tag}_ci"], g[f"{tag}_pi"], C, N)
    J.sort_indices()
    Jref = csr_matrix((g[f"{tag}_J_data"], g[f"{tag}_J_indices"], g[f"{tag}_J_indptr"]), shape=J.shape)
    assert np.array_equal(J.indices, g[f"{tag}_A_indices"]) and np.array_equal(J.indptr, g[f"{tag}_A_indptr"])
    err = abs(J - Jref).max()
    assert err <= _J_TOL[dtype] * abs(Jref).max(), err        # f64: FD truncation of the 3-point rule dominates
    # per column kind, so that small-valued columns are pinned too (f64: at the finite differences' own accuracy per kind; the
    # rounding-level pin of every kind is tests/test_gpu_exact_model.py)
    D = abs(J - Jref).tocsc()
    R = abs(Jref).tocsc()
    kind = np.concatenate([np.tile(np.arange(11), C), 11 + np.tile(np.arange(3), N)])
    for k in range(14):
        cols = np.nonzero(kind == k)[0]
        assert D[:, cols].max() <= _J_TOL[dtype] * R[:, cols].max(), (k, D[:, cols].max(), R[:, cols].max())


def test_jacobian_f32_at_bench_size_vs_model():
    """k_resjac<float> on the workload bench.py times it on (16 cameras x 50,000 points, dense), against the f64 numpy model of
    the analytic blocks (itself pinned by F3) on a sample of 20,000 observations spread over the whole list."""
    rig = make_rig(16, 50000, seed=0)
    with _native.Problem(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"], dtype="f32") as prob:
        r, Jc, Jp = prob.residual_jacobian()
    sel = np.random.default_rng(0).choice(rig["camera_ind"].size, 20000, replace=False)
    sel.sort()
    # the model evaluates gathered rows: hand it the sampled observations with their own point rows
    ci, pi = rig["camera_ind"][sel], rig["point_ind"][sel]
    upts, inv = np.unique(pi, return_inverse=True)
    r_m, Jc_m, Jp_m = model.residual_jacobian(rig["cams0"], rig["pts0"][upts], rig["points_2d"][sel], ci, inv, 1.0)
    assert np.max(np.abs(r.reshape(-1, 2)[sel] - r_m.reshape(-1, 2))) <= 5e-3                      # px, the fp32 residual bar used above
    for k in range(11):
        assert np.max(np.abs(Jc[sel][:, :, k] - Jc_m[:, :, k])) <= _J_TOL["f32"] * np.max(np.abs(Jc_m[:, :, k])), k
    assert np.max(np.abs(Jp[sel] - Jp_m)) <= _J_TOL["f32"] * np.max(np.abs(Jp_m))


def test_jacobian_theta_zero_camera():
    rig = make_rig(3, 60, seed=2)
    cams = rig["cams0"].copy()
    cams[1, 0:3] = 0.0                                  # series branch of the Rodrigues derivative
    cams[2, 0:3] = 1e-7
    with _problem(rig, cams=cams) as prob:
        r, Jc, Jp = prob.residual_jacobian()
    res_m, Jc_m, Jp_m = model.residual_jacobian(cams, rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"], 1.0)
    assert np.all(np.isfinite(Jc)) and np.max(np.abs(Jc - Jc_m)) <= 1e-6 * np.max(np.abs(Jc_m))
    # and against central differences of the oracle's residual in the rotation parameters
    x = np.hstack((cams.ravel(), rig["pts0"].ravel()))
    f = lambda xx: orc.fun(xx, 3, 60, rig["camera_ind"], rig["point_ind"], rig["points_2d"], 1.0)
    for k in range(3):
        h = 1e-6
        e = np.zeros_like(x); e[11 + k] = h
        fd = (f(x + e) - f(x - e)) / (2 * h)
        sel = rig["camera_ind"] == 1
        assert np.max(np.abs(Jc[sel, :, k].ravel() - fd.reshape(-1, 2)[sel].ravel())) <= 1e-4 * max(1.0, np.max(np.abs(fd)))


# ----------------------------------------------------------------------------- F4: converged solves
def _solve(rig_like, ftol, dtype="f64", mode=_native.MODE_FULL, weights=None, **kw):
    with _native.Problem(rig_like["cams0"], rig_like["pts0"], rig_like["uv"], rig_like["ci"], rig_like["pi"],
                         weights=weights, dtype=dtype) as prob:
        opts = prob.make_opts(ftol=ftol, mode=mode, **kw)
        return prob.solve_lm(opts)


def _f4(g, tag):
    return dict(cams0=g[f"{tag}_cams0"], pts0=g[f"{tag}_pts0"], uv=g[f"{tag}_uv"], ci=g[f"{tag}_ci"], pi=g[f"{tag}_pi"])


@pytest.mark.parametrize("tag", ["cfg1", "mid", "sparse"])
def test_converged_solve_matches_reference_f64(golden, tag):
    """ftol = 1e-4, the value the reference's caller uses (scripts/calibrate_camera.py:71)."""
    g = golden("f4_solves.npz")
    p = _f4(g, tag)
    cams, pts, rep, log = _solve(p, 1e-4)
    ref_cost = float(g[f"{tag}_loose_cost"])
    assert rep.status in (2, 3, 4)
    # the exact damped solve converges at least as far as the reference's TRF step does at the same ftol
    assert rep.cost <= ref_cost * (1 + 1e-9)
    assert abs(rep.cost - ref_cost) <= 1e-5 * ref_cost
    rms = orc.rms_reprojection(cams, pts, p["uv"], p["ci"], p["pi"])
    assert abs(rms - float(g[f"{tag}_loose_rms"])) <= 1e-4
    assert abs(0.5 * np.sum(orc.fun(np.hstack((cams.ravel(), pts.ravel())), cams.shape[0], pts.shape[0], p["ci"], p["pi"],
                                    p["uv"], 1.0) ** 2) - rep.cost) <= 1e-9 * rep.cost
    # gauge-free summaries, at the scale the reference's own loose-vs-tight solves differ by
    intr, ratios = orc.gauge_invariants(cams)
    d_ref = np.abs(g[f"{tag}_loose_intr"] - g[f"{tag}_tight_intr"]).max(axis=0)
    assert np.all(np.abs(intr - g[f"{tag}_tight_intr"]).max(axis=0) <= 20 * d_ref + np.array([0.5, 1e-4, 1e-4, 0.5, 0.5]))
    assert np.max(np.abs(ratios - g[f"{tag}_tight_centre_ratios"])) <= 1e-3


@pytest.mark.parametrize("tag", ["cfg1", "sparse"])
def test_tight_solve_is_an_optimum_the_reference_accepts(golden, tag):
    """ftol = 1e-8.  The reference's TRF/LSMR step crawls near the optimum (cost reductions ~4e-7 per
    iteration on the 2x500 rig) and stops on ftol well above the true minimum, so parity at tight
    tolerance is one-sided: the device result must be no worse than the reference's, must be a
    stationary point, and the reference's own solver restarted FROM it must not improve it."""
    g = golden("f4_solves.npz")
    p = _f4(g, tag)
    cams, pts, rep, log = _solve(p, 1e-8)
    ref_cost = float(g[f"{tag}_tight_cost"])
    assert rep.status in (2, 3, 4)
    assert rep.cost <= ref_cost * (1 + 1e-9)
    # ... and from below by the minimum itself (F9: independent exact optimisers on the reference's own fun): at ftol 1e-8 the device
    # stops within 1e-6 of it (observed 1.5e-8), the reference's TRF/LSMR 5e-4 to 1.3e-2 above it
    f9 = golden("f9_tight.npz")
    assert np.array_equal(f9[f"{tag}_uv"], p["uv"]) and np.array_equal(f9[f"{tag}_cams0"], p["cams0"])      # the same rig
    best = float(f9[f"{tag}_cost"])
    if float(f9[f"{tag}_optimality"]) < 1e-4:           # the independent optimisers converged (sparse): two-sided
        assert best * (1 - 1e-9) <= rep.cost <= best * (1 + 1e-6), (rep.cost, best)
    else:
        # the two-camera rig: none of the independent optimisers converges within its cap (1 500 exact trust-region steps reach 23.5494,
        # MINPACK 23.5232, a dense LM 23.65; stored gradient norm 95) -- their result is an upper bound only, and the pin from below is the
        # solver-independent certificate: the gradient of the ORACLE's fun (sparse 3-point finite differences) vanishes at the device's point
        assert rep.cost <= best, (rep.cost, best)
        from scipy.optimize._numdiff import approx_derivative
        x = np.hstack((cams.ravel(), pts.ravel()))
        a = (cams.shape[0], pts.shape[0], p["ci"], p["pi"], p["uv"], 1.0)
        J = approx_derivative(orc.fun, x, method="3-point", sparsity=orc.sparsity(*a[:4]), args=a)
        g0 = approx_derivative(orc.fun, np.hstack((p["cams0"].ravel(), p["pts0"].ravel())), method="3-point", sparsity=orc.sparsity(*a[:4]), args=a)
        x0 = np.hstack((p["cams0"].ravel(), p["pts0"].ravel()))
        grad, grad0 = J.T @ orc.fun(x, *a), g0.T @ orc.fun(x0, *a)
        # (1.2e6 at the initial guess, 11 at the device's point.  This rig's valley is long and nearly flat -- the reference's own tight solve
        #  sits 1.3 % higher in cost with a gradient of 0.12 -- so the gradient is a weak certificate and the cost bound above does the work)
        assert np.max(np.abs(grad)) <= 1e-4 * np.max(np.abs(grad0)), (np.max(np.abs(grad)), np.max(np.abs(grad0)))
    res, _, _ = orc.bundle_adjust(cams, pts, p["uv"], p["ci"], p["pi"], ftol=1e-8, max_nfev=20)
    assert res.cost >= rep.cost * (1 - 1e-6)            # scipy cannot lower it further
    eng = model.ModelEngine(p["cams0"], p["pts0"], p["uv"], p["ci"], p["pi"])
    out = model.run_lm_single(eng, ftol=1e-8)
    assert abs(rep.cost - out["cost"]) <= 1e-8 * out["cost"]


@pytest.mark.parametrize("tag", ["sparse", "var"])
def test_tight_optimum_two_sided_against_independent_exact_optimisers(golden, tag):
    """SURVEY 8(d)'s tight bar, two-sided: relative cost difference <= 1e-8 in fp64.  The pin is F9 (tests/golden/f9_tight.npz,
    oracle/make_golden.py f9): the minimum of the REFERENCE'S OWN `fun` found by scipy's TRF with the exact (SVD) trust-region
    subproblem on a dense finite-difference Jacobian and polished by MINPACK's lmder -- nothing of the device algorithm or of
    oracle/lm_schur_model.py is in it.  (The reference's own TRF/LSMR call stalls on ftol above this minimum: f4_solves.npz holds
    23.7608 / 113.5547 for cfg1 / sparse at ftol 1e-8, the minimum is 23.4586 / 113.4915.)  Gauge-free summaries at 1e-6.
    The third F9 rig, the two-camera cfg1, is not here: the independent optimisers do not converge on it within their caps (see
    test_tight_solve_is_an_optimum_the_reference_accepts for what pins it instead)."""
    g = golden("f9_tight.npz")
    p = _f4(g, tag)
    assert float(g[f"{tag}_optimality"]) < 1e-4        # the pin itself is a stationary point of the reference's fun (||J^T r||_inf; 1e5 at the start)
    cams, pts, rep, log = _solve(p, 1e-12, xtol=1e-12, gtol=1e-12)
    best = float(g[f"{tag}_cost"])
    assert rep.status in (1, 2, 3, 4)
    assert abs(rep.cost - best) <= 1e-8 * best, (rep.cost, best, (rep.cost - best) / best)
    x = np.hstack((cams.ravel(), pts.ravel()))
    cost_ref_fun = 0.5 * np.sum(orc.fun(x, cams.shape[0], pts.shape[0], p["ci"], p["pi"], p["uv"], 1.0) ** 2)
    assert abs(cost_ref_fun - rep.cost) <= 1e-10 * rep.cost           # the reported cost IS the reference's fun at the returned x
    assert abs(orc.rms_reprojection(cams, pts, p["uv"], p["ci"], p["pi"]) - float(g[f"{tag}_rms"])) <= 1e-8
    intr, ratios = orc.gauge_invariants(cams)
    assert np.max(np.abs(ratios - g[f"{tag}_centre_ratios"])) <= 1e-6
    d = np.abs(intr - g[f"{tag}_intr"]).max(axis=0)                  # columns f, k1, k2, cx, cy
    assert d[0] <= 1e-6 * 2400 and d[3] <= 2e-3 and d[4] <= 2e-3 and d[1] <= 1e-6 and d[2] <= 1e-6, d
    # fp32 engine on the same rigs, run until its own rounding noise stops it (xtol): it stalls 7e-5 (sparse) / 2.5e-4 (var) above the
    # minimum, with the f32-lane Cholesky as with the f64 one (5e-5 / 5e-4: profiles/r4_fp32_engine_vs_minimum.txt) -- the fp32 bar of
    # SURVEY 8(d), 1e-4, is a bar against the reference AT ftol 1e-4 (test_converged_solve_f32), where both sit ~1e-3 above the minimum
    cams32, pts32, rep32, _ = _solve(p, 1e-9, dtype="f32")
    c32 = 0.5 * np.sum(orc.fun(np.hstack((cams32.ravel(), pts32.ravel())), cams.shape[0], pts.shape[0], p["ci"], p["pi"], p["uv"], 1.0) ** 2)
    assert best * (1 - 1e-9) <= c32 <= best * (1 + 1e-3), (c32, best)


@pytest.mark.parametrize("tag", ["cfg1", "mid"])
def test_converged_solve_f32(golden, tag):
    g = golden("f4_solves.npz")
    p = _f4(g, tag)
    cams, pts, rep, log = _solve(p, 1e-4, dtype="f32")
    ref_cost = float(g[f"{tag}_loose_cost"])
    cost64 = 0.5 * np.sum(orc.fun(np.hstack((cams.ravel(), pts.ravel())), cams.shape[0], pts.shape[0], p["ci"], p["pi"],
                                  p["uv"], 1.0) ** 2)
    assert abs(cost64 - ref_cost) <= 1e-4 * ref_cost
    rms = orc.rms_reprojection(cams, pts, p["uv"], p["ci"], p["pi"])
    assert abs(rms - float(g[f"{tag}_loose_rms"])) <= 1e-3


def test_device_lm_follows_cpu_model_iteration_by_iteration(golden):
    g = golden("f4_solves.npz")
    p = _f4(g, "sparse")
    cams, pts, rep, log = _solve(p, 1e-4)
    eng = model.ModelEngine(p["cams0"], p["pts0"], p["uv"], p["ci"], p["pi"])
    out = model.run_lm_single(eng, ftol=1e-4)
    assert rep.iterations == out["iterations"] and rep.nfev == out["nfev"] and rep.status == out["status"]
    assert abs(rep.cost - out["cost"]) <= 1e-9 * out["cost"]
    assert np.max(np.abs(cams - out["cams"])) <= 1e-6 and np.max(np.abs(pts - out["pts"])) <= 1e-6


def test_weighted_solve_matches_oracle():
    rig = make_rig(4, 400, seed=12, visibility=0.8)
    rng = np.random.default_rng(3)
    w = rng.uniform(0.5, 2.0, rig["point_ind"].size)
    res, c_ref, p_ref = orc.bundle_adjust(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"],
                                          weights=w.reshape(-1, 1), ftol=1e-8)
    cams, pts, rep, _ = _solve(dict(cams0=rig["cams0"], pts0=rig["pts0"], uv=rig["points_2d"], ci=rig["camera_ind"],
                                    pi=rig["point_ind"]), 1e-8, weights=w)
    # above: the reference's call at the same tolerance; below: the minimum itself, by the independent exact optimisers of
    # oracle.tight_optimum started from the device's solution (see test_tight_optimum_two_sided_...)
    best, _ = orc.tight_optimum(cams, pts, rig["points_2d"], rig["camera_ind"], rig["point_ind"], weights=w.reshape(-1, 1), max_nfev=(25, 10))
    assert rep.cost <= res.cost * (1 + 1e-9) and best * (1 - 1e-9) <= rep.cost <= best * (1 + 1e-5), (rep.cost, best, res.cost)
    again, _, _ = orc.bundle_adjust(cams, pts, rig["points_2d"], rig["camera_ind"], rig["point_ind"],
                                    weights=w.reshape(-1, 1), ftol=1e-8, max_nfev=20)
    assert again.cost >= rep.cost * (1 - 1e-6)
    eng = model.ModelEngine(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"], w=w)
    out = model.run_lm_single(eng, ftol=1e-8)
    assert abs(rep.cost - out["cost"]) <= 1e-8 * out["cost"]


def test_config2_scipy_drives_device_residual_and_jacobian():
    """BASELINE config 2: 8 cams x 5k points, fp64, only the residual / Jacobian kernels on the GPU while scipy's TRF
    still drives the iterations (same keyword set as pySBA.py:141 except that jac= is the analytic device Jacobian)."""
    from scipy.optimize import least_squares
    rig = make_rig(8, 5000, seed=0)
    C, N = 8, 5000
    ci, pi, uv = rig["camera_ind"], rig["point_ind"], rig["points_2d"]
    x0 = np.hstack((rig["cams0"].ravel(), rig["pts0"].ravel()))
    with _native.Problem(rig["cams0"], rig["pts0"], uv, ci, pi) as prob:
        fun = lambda x: prob.residual(x)[0]

        def jac(x):
            _, Jc, Jp = prob.residual_jacobian(x)
            return assemble_jacobian(Jc, Jp, ci, pi, C, N)
        res = least_squares(fun, x0, jac=jac, x_scale="jac", ftol=1e-4, method="trf")
    ref, _, _ = orc.bundle_adjust(rig["cams0"], rig["pts0"], uv, ci, pi, ftol=1e-4)
    # same optimiser, same stopping rule; the Jacobians differ by the FD truncation error only
    assert res.status == ref.status and abs(res.nfev - ref.nfev) <= 1
    assert abs(res.cost - ref.cost) <= 1e-6 * ref.cost
    # parameter bounds of SURVEY 8(d) at ftol = 1e-4, per block (LSMR amplifies the FD-vs-analytic Jacobian difference along
    # weak directions; observed: rotvec 6e-6, t 1.2e-2 mm, f 9e-3 px, k 4e-6, centre 1.5e-2 px, points 6e-4 mm)
    dc = np.abs(res.x[:C * 11] - ref.x[:C * 11]).reshape(C, 11).max(axis=0)
    assert np.all(dc[0:3] <= 5e-5) and np.all(dc[3:6] <= 0.05) and dc[6] <= 0.05 and np.all(dc[7:9] <= 1e-4) and np.all(dc[9:11] <= 0.05)
    assert np.max(np.abs(res.x[C * 11:] - ref.x[C * 11:])) <= 0.02


# ----------------------------------------------------------------------------- class surface end to end
def test_pysba_bundleAdjust_surface(golden, capsys):
    g = golden("f4_solves.npz")
    p = _f4(g, "cfg1")
    cams_in, pts_in = p["cams0"].copy(), p["pts0"].copy()
    sba = PySBA(cams_in, pts_in, p["uv"], p["ci"], p["pi"])
    res = sba.bundleAdjust(1e-4)
    out = capsys.readouterr().out
    assert "Iteration" in out and "`ftol` termination condition is satisfied." in out
    assert np.array_equal(cams_in, p["cams0"]) and np.array_equal(pts_in, p["pts0"])   # inputs never written (pySBA.py:145-146 rebinds)
    assert sba.cameraArray is not cams_in and sba.cameraArray.shape == (2, 11) and sba.points3D.shape == (500, 3)
    assert res.status == 2 and res.success and res.x.shape == (2 * 11 + 500 * 3,)
    assert abs(res.cost - float(g["cfg1_loose_cost"])) <= 1e-5 * float(g["cfg1_loose_cost"])
    assert res.fun.shape == (1000 * 2,) and abs(0.5 * res.fun @ res.fun - res.cost) <= 1e-9 * res.cost
    assert res.jac.shape == (2000, 1522) and res.grad.shape == (1522,)
    assert abs(np.max(np.abs(res.grad)) - res.optimality) <= 1e-6 * max(1.0, res.optimality)
    blob = pickle.dumps(sba)                             # calibrate_camera.py:86-88
    back = pickle.loads(blob)
    assert type(back).__module__ == "lasercalib.pySBA" and np.array_equal(back.cameraArray, sba.cameraArray)
    pickle.loads(pickle.dumps(res))


def test_nocam_matches_reference(golden):
    g = golden("f5_variants.npz")
    sba = PySBA(g["cams0"].copy(), g["pts0"].copy(), g["uv"], g["ci"], g["pi"])
    res = sba.bundleAdjust_nocam()
    assert res.x.shape == (g["pts0"].size,)
    assert res.cost <= float(g["nocam_cost"]) * (1 + 1e-9)
    assert abs(res.cost - float(g["nocam_cost"])) <= 1e-6 * float(g["nocam_cost"])
    assert np.max(np.abs(sba.points3D - g["nocam_pts"])) <= 1e-3       # mm; points-only BA has no gauge freedom
    assert np.array_equal(sba.cameraArray, g["cams0"])


def test_sharedcam_matches_reference(golden):
    """PySBA.bundleAdjust_sharedcam (pySBA.py:297-325): f, k1, k2 tied across cameras."""
    g = golden("f5_variants.npz")
    sba = PySBA(g["cams0"].copy(), g["pts0"].copy(), g["uv"], g["ci"], g["pi"])
    res = sba.bundleAdjust_sharedcam()
    C, N = g["cams0"].shape[0], g["pts0"].shape[0]
    assert res.x.shape == (3 + 8 * C + 3 * N,) and res.status in (2, 3, 4)
    assert np.all(sba.cameraArray[:, 6:9] == sba.cameraArray[0, 6:9])          # one shared (f, k1, k2)
    assert np.array_equal(res.x[:3], sba.cameraArray[0, 6:9])
    ref = float(g["sharedcam_cost"])
    # one-sided like every tight-tolerance comparison with the reference's TRF step: never worse, same basin
    assert res.cost <= ref * (1 + 1e-9) and res.cost >= 0.95 * ref
    # the oracle's residual function in the reference's parameterisation agrees with the device result vector
    f = orc.fun_sharedcam(res.x, C, N, g["ci"], g["pi"], g["uv"], 1.0)
    assert np.max(np.abs(f - res.fun)) <= 1e-8 and abs(0.5 * f @ f - res.cost) <= 1e-9 * res.cost
    # scipy restarted from the device solution (same variant, same arguments) cannot improve it
    again, _, _ = orc.bundle_adjust_sharedcam(sba.cameraArray, sba.points3D, g["uv"], g["ci"], g["pi"], ftol=1e-6)
    assert again.cost >= res.cost * (1 - 1e-5)
    # trajectory = numpy model of the device algorithm with the same tying
    cams0 = g["cams0"].copy()
    cams0[:, 6:9] = cams0[:, 6:9].mean(axis=0)
    eng = model.ModelEngine(cams0, g["pts0"], g["uv"], g["ci"], g["pi"], shared_intrinsics=True)
    out = model.run_lm_single(eng, ftol=1e-6)
    assert abs(out["cost"] - res.cost) <= 1e-7 * res.cost and abs(out["nfev"] - res.nfev) <= 2
    # Jacobian in the shared layout: J^T r = gradient, optimality consistent
    assert res.jac.shape == (2 * g["ci"].size, 3 + 8 * C + 3 * N)
    assert abs(np.max(np.abs(res.grad)) - res.optimality) <= 1e-6 * max(1.0, res.optimality)


def test_camonly_squared_error_variant(golden):
    """PySBA.bundle_adjustment_camonly (pySBA.py:151-173): cameras free, points fixed, residual = w*(pixel error)^2."""
    g = golden("f5_variants.npz")
    sba = PySBA(g["cams0"].copy(), g["pts0"].copy(), g["uv"], g["ci"], g["pi"])
    res = sba.bundle_adjustment_camonly()                      # ftol = 1e-4 like the reference's default
    C, N = g["cams0"].shape[0], g["pts0"].shape[0]
    ref = float(g["camonly_cost"])
    assert res.status in (2, 3, 4) and res.x.shape == (11 * C,)
    assert np.array_equal(sba.points3D, g["pts0"]) and np.array_equal(res.x.reshape(C, 11), sba.cameraArray)
    # both solvers stop on ftol = 1e-4: the costs agree to within that stopping tolerance
    assert abs(res.cost - ref) <= 1e-4 * ref
    f = orc.fun_camonly(res.x, C, N, g["ci"], g["pi"], g["uv"], 1.0, g["pts0"])      # the reference's own residual function
    assert np.max(np.abs(f - res.fun)) <= 1e-6 and abs(0.5 * f @ f - res.cost) <= 1e-9 * res.cost
    again, _ = orc.bundle_adjust_camonly(sba.cameraArray, g["pts0"], g["uv"], g["ci"], g["pi"], ftol=1e-4)
    assert again.cost >= res.cost * (1 - 1e-4)
    # res.jac / res.grad exist like on scipy's OptimizeResult: dense Jacobian of the squared residual, checked against
    # scipy's own finite differences of the reference function at the solution
    from scipy.optimize._numdiff import approx_derivative
    Jfd = approx_derivative(orc.fun_camonly, res.x, method="3-point", args=(C, N, g["ci"], g["pi"], g["uv"], 1.0, g["pts0"]))
    assert res.jac.shape == Jfd.shape == (2 * g["ci"].size, 11 * C)
    assert np.max(np.abs(res.jac - Jfd)) <= 1e-6 * np.max(np.abs(Jfd))
    assert np.max(np.abs(res.grad - res.jac.T @ res.fun)) <= 1e-12 * np.max(np.abs(res.grad))
    assert np.max(np.abs(res.grad - Jfd.T @ f)) <= 1e-4 * np.max(np.abs(Jfd.T @ f))      # the FD entries carry ~1e-6 each


def test_transform_points_3d_squared_error_variant(golden):
    """PySBA.bundleAdjust_transform_points_3d (pySBA.py:176-205): one 3x4 affine on the points, squared pixel error."""
    g = golden("f5_variants.npz")
    sba = PySBA(g["cams0"].copy(), g["pts0"].copy(), g["uv"], g["ci"], g["pi"])
    res = sba.bundleAdjust_transform_points_3d()               # ftol = 1e-3
    C, N = g["cams0"].shape[0], g["pts0"].shape[0]
    ref = float(g["transform_cost"])
    assert res.status in (2, 3, 4) and res.x.shape == (12,)
    assert np.array_equal(sba.cameraArray, g["cams0"])
    assert abs(res.cost - ref) <= 1e-3 * ref                  # within the stopping tolerance both solvers used
    f = orc.fun_transform_points_3d(res.x, C, N, g["cams0"], g["ci"], g["pi"], g["uv"], 1.0, g["pts0"])
    assert np.max(np.abs(f - res.fun)) <= 1e-6 and abs(0.5 * f @ f - res.cost) <= 1e-9 * res.cost
    T = np.vstack((res.x.reshape(3, 4), [0, 0, 0, 1]))
    moved = (T @ np.vstack((g["pts0"].T, np.ones((1, N))))).T[:, :3]
    assert np.max(np.abs(moved - sba.points3D)) <= 1e-9       # points3D replaced by the transformed points (pySBA.py:197-204)
    assert np.max(np.abs(sba.points3D - g["transform_pts"])) <= 0.5      # mm, against the reference's result
    assert np.max(np.abs(res.x - g["transform_x"])[[0, 1, 2, 4, 5, 6, 8, 9, 10]]) <= 2e-3
    from scipy.optimize._numdiff import approx_derivative
    Jfd = approx_derivative(orc.fun_transform_points_3d, res.x, method="3-point",
                            args=(C, N, g["cams0"], g["ci"], g["pi"], g["uv"], 1.0, g["pts0"]))
    assert res.jac.shape == Jfd.shape == (2 * g["ci"].size, 12)
    assert np.max(np.abs(res.jac - Jfd)) <= 1e-6 * np.max(np.abs(Jfd))


def test_nonfinite_start_raises_value_error():
    rig = make_rig(2, 50, seed=1)
    cams = rig["cams0"].copy()
    cams[0, 6] = np.nan
    sba = PySBA(cams, rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"])
    with pytest.raises(ValueError):                   # scipy: least_squares.py:844-845
        sba.bundleAdjust(1e-4)


def test_bad_indices_rejected():
    rig = make_rig(2, 50, seed=1)
    ci = rig["camera_ind"].copy()
    ci[3] = 7
    with pytest.raises(_native.SbaError):
        _native.Problem(rig["cams0"], rig["pts0"], rig["points_2d"], ci, rig["point_ind"])


def test_point_with_single_observation_and_unseen_point():
    # ragged input: a point seen once (rank-deficient 3x3 block, kept stable by the damping) and a point never seen
    rig = make_rig(4, 120, seed=6, visibility=0.9)
    keep = ~((rig["point_ind"] == 5) & (rig["camera_ind"] != 0)) & (rig["point_ind"] != 17)
    p = dict(cams0=rig["cams0"], pts0=rig["pts0"], uv=rig["points_2d"][keep], ci=rig["camera_ind"][keep], pi=rig["point_ind"][keep])
    cams, pts, rep, _ = _solve(p, 1e-6)
    assert rep.status in (2, 3, 4) and np.all(np.isfinite(cams)) and np.all(np.isfinite(pts))
    assert np.array_equal(pts[17], rig["pts0"][17])     # unseen point: zero gradient, never moves
    eng = model.ModelEngine(p["cams0"], p["pts0"], p["uv"], p["ci"], p["pi"])
    out = model.run_lm_single(eng, ftol=1e-6)
    assert abs(rep.cost - out["cost"]) <= 1e-8 * out["cost"]


@pytest.mark.parametrize("C,N,vis", [(17, 150, 0.6), (17, 64, 1.0), (20, 200, 0.7), (32, 120, 0.5), (46, 90, 0.4)])
def test_more_than_16_cameras_uses_camera_groups(C, N, vis):
    """Camera groups of 16 + group pairs, PARTIAL last group (17, 20, 46), streamed Cholesky (176 < 11C <= 512):
    the device trajectory must be the numpy model's, iteration for iteration (17 = the reference's own example rig)."""
    rig = make_rig(C, N, seed=8, visibility=vis)
    p = dict(cams0=rig["cams0"], pts0=rig["pts0"], uv=rig["points_2d"], ci=rig["camera_ind"], pi=rig["point_ind"])
    cams, pts, rep, _ = _solve(p, 1e-6)
    eng = model.ModelEngine(p["cams0"], p["pts0"], p["uv"], p["ci"], p["pi"])
    out = model.run_lm_single(eng, ftol=1e-6)
    assert rep.iterations == out["iterations"]
    assert abs(rep.cost - out["cost"]) <= 1e-8 * out["cost"]
    # gauge-free, few points per camera: the parameters agree to the conditioning of the solve, not to rounding
    assert np.allclose(cams, out["cams"], rtol=1e-4, atol=1e-3) and np.allclose(pts, out["pts"], rtol=1e-4, atol=1e-3)


def test_more_than_16_cameras_f32():
    rig = make_rig(17, 300, seed=9, visibility=0.7)
    prob = _problem(rig, "f32")
    cams, pts, rep, _ = prob.solve_lm(prob.make_opts(ftol=1e-4))
    prob.close()
    ref, _, _ = orc.bundle_adjust(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"], ftol=1e-4)
    assert rep.status in (2, 3, 4) and abs(rep.cost - ref.cost) <= 1e-4 * ref.cost       # fp32 bar of SURVEY 8(d); observed 4e-6


# ----------------------------------------------------------------------------- full size (BASELINE config 3) properties
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_full_size_16x50k_properties(dtype):
    rig = make_rig(16, 50000, seed=0)
    p = dict(cams0=rig["cams0"], pts0=rig["pts0"], uv=rig["points_2d"], ci=rig["camera_ind"], pi=rig["point_ind"])
    with _native.Problem(p["cams0"], p["pts0"], p["uv"], p["ci"], p["pi"], dtype=dtype) as prob:
        r0, c0 = prob.residual()
        opts = prob.make_opts(ftol=1e-4)
        cams, pts, rep, log = prob.solve_lm(opts)
        r1, c1 = prob.residual(np.hstack((cams.ravel(), pts.ravel())))
    M = p["ci"].size
    # sampled check of the residual against the oracle at full size
    idx = np.random.default_rng(0).choice(M, 5000, replace=False)
    ref = orc.project(p["pts0"][p["pi"][idx]], p["cams0"][p["ci"][idx]]) - p["uv"][idx]
    assert np.max(np.abs(r0.reshape(-1, 2)[idx] - ref)) <= (1e-8 if dtype == "f64" else 5e-3)
    assert rep.status == 2 and rep.cost < 1e-3 * c0
    costs = [row.cost for row in log if row.accepted]
    assert all(b <= a for a, b in zip(costs, costs[1:]))        # accepted costs never increase
    assert abs(c1 - rep.cost) <= (1e-9 if dtype == "f64" else 1e-4) * c1
    # noise floor: 0.3 px Gaussian noise => RMS reprojection ~ 0.3*sqrt(2)*sqrt(dof ratio)
    rms = np.sqrt(np.mean(np.sum(r1.reshape(-1, 2) ** 2, axis=1)))
    assert 0.35 < rms < 0.45
    # gauge-free recovery of the truth
    intr, ratios = orc.gauge_invariants(cams)
    intr_t, ratios_t = orc.gauge_invariants(rig["cams_true"])
    assert np.max(np.abs(ratios - ratios_t)) <= 1e-3
    assert np.max(np.abs(intr[:, 0] - intr_t[:, 0])) <= 3.0       # focal length, px


# ----------------------------------------------------------------------------- dense fast path == general path
@pytest.mark.parametrize("dtype,C,N,vis,rtol", [("f32", 16, 333, 1.0, 2e-5), ("f32", 5, 77, 1.0, 2e-5), ("f64", 16, 333, 1.0, 1e-9),
                                                 ("f64", 3, 40, 1.0, 1e-9), ("f32", 16, 333, 0.5, 2e-5), ("f32", 9, 120, 0.7, 2e-5)])
def test_dense_kernels_match_general_kernels(monkeypatch, dtype, C, N, vis, rtol):
    """One camera group runs k_schur_fused_bf3 in f32 (dense rigs directly, sparse ones through the per-point visibility
    mask) and k_backsub_dense on dense rigs; SBA_NO_DENSE forces the general kernels.  Same problem, observation order
    shuffled (the upload must restore (point, camera) order), with weights: reduced system, trial scalars and the whole
    solve must agree to rounding."""
    rig = make_rig(C, N, seed=21, visibility=vis)
    rng = np.random.default_rng(5)
    perm = rng.permutation(rig["camera_ind"].size)
    uv, ci, pi = rig["points_2d"][perm], rig["camera_ind"][perm], rig["point_ind"][perm]
    wts = rng.uniform(0.5, 1.5, ci.size)

    def run(disable):
        if disable:
            monkeypatch.setenv("SBA_NO_DENSE", "1")
        else:
            monkeypatch.delenv("SBA_NO_DENSE", raising=False)
        import torch
        torch.cuda.set_device(0)
        prob = _native.Problem(rig["cams0"], rig["pts0"], uv, ci, pi, weights=wts, dtype=dtype,
                               stream=torch.cuda.current_stream().cuda_stream)
        prob.lm_begin(prob.make_opts(ftol=1e-6))
        prob.lm_linearize()
        E = torch.zeros(prob.exchange_size(), dtype=torch.float64, device="cuda")
        prob.lm_form_reduced(E.data_ptr())
        sc = torch.zeros(8, dtype=torch.float64, device="cuda")
        prob.lm_solve_trial(E.data_ptr(), sc.data_ptr())
        torch.cuda.synchronize()
        Eh, sch = E.cpu().numpy().copy(), sc.cpu().numpy().copy()
        prob.close()
        prob = _native.Problem(rig["cams0"], rig["pts0"], uv, ci, pi, weights=wts, dtype=dtype)
        cams, pts, rep, _ = prob.solve_lm(prob.make_opts(ftol=1e-8 if dtype == "f64" else 1e-4))
        prob.close()
        return Eh, sch, cams, pts, rep

    Ed, sd, cd, pd_, rd = run(False)
    Eg, sg, cg, pg, rg_ = run(True)
    n = 11 * C
    scale = np.abs(Eg[:n * n]).max()
    assert np.max(np.abs(Ed[:n * n] - Eg[:n * n])) <= rtol * scale
    for a, b in ((n * n, n * n + n), (n * n + n, n * n + 2 * n), (n * n + 2 * n, n * n + 3 * n), (n * n + 3 * n, n * n + 3 * n + 1)):
        assert np.max(np.abs(Ed[a:b] - Eg[a:b])) <= rtol * max(np.abs(Eg[a:b]).max(), 1.0)
    assert np.allclose(sd[:4], sg[:4], rtol=50 * rtol, atol=1e-6)      # trial cost, predicted reduction, |dx|^2, |x|^2
    assert rd.status == rg_.status or {rd.status, rg_.status} <= {2, 3, 4}
    # f64 solves stop at ftol=1e-8 and must agree tightly.  f32 ones stop at ftol=1e-4, where the two rounding histories
    # may end one crawling LM step apart on these small, gauge-free rigs (observed 0.7 % between them), so each fp32 solve is
    # held to the fp32 bar against the REFERENCE instead: at least as converged as scipy at the same ftol (1e-4 relative)
    if dtype == "f64":
        assert abs(rd.cost - rg_.cost) <= 1e-7 * rg_.cost
    else:
        ref, _, _ = orc.bundle_adjust(rig["cams0"], rig["pts0"], uv, ci, pi, weights=wts.reshape(-1, 1), ftol=1e-4)
        assert rd.cost <= ref.cost * (1 + 1e-4) and rg_.cost <= ref.cost * (1 + 1e-4)
        if C * N <= 1000:
            # (from below: the minimum itself -- oracle.tight_optimum, independent exact optimisers from the dense path's solution;
            #  dense SVD steps, so only on the smallest rig)
            best, _ = orc.tight_optimum(cd, pd_, uv, ci, pi, weights=wts.reshape(-1, 1), max_nfev=(60, 30))
            assert min(rd.cost, rg_.cost) >= best * (1 - 1e-4), (rd.cost, rg_.cost, best)
        else:
            assert min(rd.cost, rg_.cost) >= 0.9 * ref.cost, "basin guard only (two-sided pins: the 5-camera case here, F9 in test_tight_optimum_two_sided_...)"
