"""GPU tests of sba_align / sba_apply_similarity (include/sba_hip.h) through the C ABI.

References: a planted similarity (the truth is exact), ``align_oracle`` / ``apply_oracle``, the numpy restatement in
tests/test_align_host.py (SVD for R, scipy for the composition; the library uses Horn's quaternion matrix and quaternion
products), and the handle itself: moving every camera and point together leaves every residual where it was.

Bars.  Planted and device-against-numpy: scale and R 1e-12, t 1e-9 mm, distances 1e-9 mm, singular values 1e-12 relative --
the numpy restatement meets the planted values to 6e-16 / 8e-16 / 6e-14 mm (tests/test_align_host.py), three orders of margin
are left for the other summation order at up to 2 000 points.  Targets 1e6 mm away: t relative to 1e6, at the bar of the scale
(1e-12 relative, 1e-6 mm).  Residual invariance: 1e-9 px on a float64 handle; on a float32 handle 4 x the largest difference
between the float32 and the float64 engine's residuals at the same untransformed parameters (that engine's own rounding)."""
import os
import sys

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lasercalib_amd import _native  # noqa: E402
from lasercalib_amd.pySBA import PySBA  # noqa: E402
from lasercalib_amd.synth import _project_np, make_rig  # noqa: E402
from test_align_host import PLANTED, align_oracle, apply_oracle, centres_of, planted_map, rotation_angle  # noqa: E402

DTYPES = ["f64", "f32"]
R_TRUE = Rotation.from_rotvec(PLANTED["rho"]).as_matrix()
TOL_S, TOL_R, TOL_T, TOL_MM, TOL_SV = 1e-12, 1e-12, 1e-9, 1e-9, 1e-12


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert _native.device_count() > 0, "no HIP device visible: GPU tests must run on the MI355X box"


def _prob(rig, dtype="f64", cams=None, pts=None):
    return _native.Problem(rig["cams0"] if cams is None else cams, rig["pts0"] if pts is None else pts,
                           rig["points_2d"], rig["camera_ind"], rig["point_ind"], dtype=dtype)


def _planted_errors(aln, label, t_true=PLANTED["t"], s_true=PLANTED["s"]):
    ds, dR, dt = abs(aln.scale / s_true - 1), np.abs(aln.R - R_TRUE).max(), np.abs(aln.t - t_true).max()
    print(f"{label}: scale {ds:.1e} relative, R {dR:.1e}, t {dt:.1e} mm, rms_after {aln.rms_after:.1e} mm, max_after {aln.max_after:.1e} mm")
    return ds, dR, dt


def _rms_px(cams, pts, rig):
    r = _project_np(pts[rig["point_ind"]], cams[rig["camera_ind"]]) - rig["points_2d"]
    return float(np.sqrt(np.mean(np.sum(r * r, axis=1))))


# ----------------------------------------------------------------------------- 1. planted similarity
PLANTED_RIGS = [("4x300", dict(n_cams=4, n_points=300)),
                ("17x2000 visibility 0.45", dict(n_cams=17, n_points=2000, visibility=0.45, min_cams_per_point=4)),
                ("128x1500 13 columns", dict(n_cams=128, n_points=1500, tangential=True))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,args", PLANTED_RIGS, ids=[r[0] for r in PLANTED_RIGS])
def test_planted_similarity_is_recovered(name, args, dtype):
    rig = make_rig(**args)
    tgt = planted_map(rig["pts0"])
    with _prob(rig, dtype) as prob:
        aln = prob.align(target_points=tgt)
        cams, pts = prob.get_params()
    ds, dR, dt = _planted_errors(aln, f"{name} {dtype}")
    assert aln.n_points_used == rig["n_points"] and aln.n_cams_used == 0
    assert ds <= TOL_S and dR <= TOL_R and dt <= TOL_T and aln.rms_after <= TOL_MM
    assert aln.max_after >= aln.rms_after and aln.rms_before > 100.0
    assert np.abs(pts - aln.transform(rig["pts0"])).max() <= 1e-9             # the handle's points are where the estimate puts them
    assert np.array_equal(cams[:, 6:], rig["cams0"][:, 6:])                    # intrinsics and distortion: unchanged, 11 or 13 columns


# ----------------------------------------------------------------------------- 2. device against the numpy restatement
def _against_oracle(aln, o, label):
    ds, dR, dt = abs(aln.scale / o["scale"] - 1), np.abs(aln.R - o["R"]).max(), np.abs(aln.t - o["t"]).max()
    d_mm = max(abs(aln.rms_before - o["rms_before"]), abs(aln.rms_after - o["rms_after"]), abs(aln.max_after - o["max_after"]))
    d_sv = np.abs(aln.sv / o["sv"] - 1).max()
    print(f"{label}: device - numpy: scale {ds:.1e}, R {dR:.1e}, t {dt:.1e} mm, rms / max {d_mm:.1e} mm, sv {d_sv:.1e} relative")
    assert (aln.n_points_used, aln.n_cams_used) == (o["n_points_used"], o["n_cams_used"])
    assert ds <= TOL_S and dR <= TOL_R and dt <= TOL_T and d_mm <= TOL_MM and d_sv <= TOL_SV


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_scale", [True, False])
def test_device_matches_numpy_on_noisy_weighted_targets(dtype, with_scale):
    rig = make_rig(17, 2000, visibility=0.45, min_cams_per_point=4)
    rng = np.random.default_rng(11)
    tgt = planted_map(rig["pts0"]) + rng.normal(0.0, 5.0, (2000, 3))
    pw = rng.uniform(0.2, 3.0, 2000)
    pw[::3] = 0.0
    tc = planted_map(centres_of(rig["cams0"])) + rng.normal(0.0, 5.0, (17, 3))
    cw = rng.uniform(0.5, 50.0, 17)
    cw[4] = 0.0
    with _prob(rig, dtype) as prob:
        aln = prob.align(tgt, pw, tc, cw, with_scale=with_scale, apply=False)
    o = align_oracle(rig["pts0"], tgt, pw, rig["cams0"], tc, cw, with_scale=with_scale)
    _against_oracle(aln, o, f"17x2000 noisy {dtype} with_scale={with_scale}")
    assert aln.n_points_used == 1333 and aln.n_cams_used == 16
    if not with_scale:
        assert aln.scale == 1.0


# ----------------------------------------------------------------------------- 3. edge shapes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [3, 257, 513])
def test_point_counts_at_the_workgroup_boundary(n, dtype):
    rig = make_rig(4, n, seed=2)
    tgt = planted_map(rig["pts0"])
    with _prob(rig, dtype) as prob:
        aln = prob.align(target_points=tgt, apply=False)
    ds, dR, dt = _planted_errors(aln, f"N = {n} {dtype}")
    assert aln.n_points_used == n
    assert ds <= TOL_S and dR <= TOL_R and dt <= TOL_T and aln.rms_after <= TOL_MM


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_cams", [3, 17])
def test_centres_only(n_cams, dtype):
    rig = make_rig(n_cams, 50, seed=3)
    tc = planted_map(centres_of(rig["cams0"]))
    with _prob(rig, dtype) as prob:
        aln = prob.align(target_centres=tc, apply=False)
    ds, dR, dt = _planted_errors(aln, f"centres only, C = {n_cams} {dtype}")
    assert (aln.n_points_used, aln.n_cams_used) == (0, n_cams)
    assert ds <= TOL_S and dR <= TOL_R and dt <= TOL_T and aln.rms_after <= TOL_MM


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_point_and_two_centres(dtype):
    rig = make_rig(4, 20, seed=4)
    pw, cw = np.zeros(20), np.array([0.0, 2.0, 0.0, 0.5])
    pw[7] = 1.5
    tgt, tc = planted_map(rig["pts0"]), planted_map(centres_of(rig["cams0"]))
    with _prob(rig, dtype) as prob:
        aln = prob.align(tgt, pw, tc, cw, apply=False)
    ds, dR, dt = _planted_errors(aln, f"one point and two centres {dtype}")
    assert (aln.n_points_used, aln.n_cams_used) == (1, 2)
    assert ds <= TOL_S and dR <= TOL_R and dt <= TOL_T and aln.rms_after <= TOL_MM


@pytest.mark.parametrize("dtype", DTYPES)
def test_targets_far_from_the_origin(dtype):
    rig = make_rig(4, 300)
    t_far = 1e6 * np.array([0.48, -0.6, 0.64])                       # |t| = 1e6 mm exactly
    tgt = planted_map(rig["pts0"], t=t_far)
    with _prob(rig, dtype) as prob:
        aln = prob.align(target_points=tgt, apply=False)
    ds, dR, dt = _planted_errors(aln, f"targets at 1e6 mm {dtype}", t_true=t_far)
    assert ds <= TOL_S and dR <= TOL_R and dt / 1e6 <= 1e-12 and aln.rms_after <= TOL_MM


# ----------------------------------------------------------------------------- 4. refusals
@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_leave_the_handle_untouched(dtype):
    rig = make_rig(4, 300)
    N = 300
    tgt = planted_map(rig["pts0"])
    line = np.linspace(-500.0, 500.0, N)[:, None] * np.array([[0.6, -0.3, 0.74]]) + 10.0
    two = np.zeros(N)
    two[[5, 200]] = 1.0
    neg, nan_w, nan_t = np.ones(N), np.ones(N), tgt.copy()
    neg[17], nan_w[290], nan_t[100, 1] = -1.0, np.nan, np.nan
    skew = R_TRUE.copy()
    skew[0, 1] += 1e-6
    with _prob(rig, dtype) as prob:
        def untouched():
            cams, pts = prob.get_params()
            return np.array_equal(cams, rig["cams0"]) and np.array_equal(pts, rig["pts0"])

        cases = [("fewer than 3 correspondences", lambda: prob.align(tgt, two)),
                 ("fewer than 3 correspondences", lambda: prob.align()),
                 ("rotation is not unique", lambda: prob.align(target_points=line)),
                 ("weight is negative or not finite", lambda: prob.align(tgt, neg)),
                 ("weight is negative or not finite", lambda: prob.align(tgt, nan_w)),
                 ("weight is negative or not finite", lambda: prob.align(target_centres=np.zeros((4, 3)), centre_weights=[1, 1, np.inf, 1])),
                 ("target is not finite", lambda: prob.align(nan_t)),
                 ("target is not finite", lambda: prob.align(nan_t, np.ones(N))),
                 ("not orthogonal", lambda: prob.apply_similarity(1.0, skew, np.zeros(3))),
                 ("reflection", lambda: prob.apply_similarity(1.0, np.diag([1.0, 1.0, -1.0]), np.zeros(3))),
                 ("scale must be positive", lambda: prob.apply_similarity(0.0, R_TRUE, np.zeros(3))),
                 ("scale must be positive", lambda: prob.apply_similarity(np.nan, R_TRUE, np.zeros(3)))]
        for text, call in cases:
            with pytest.raises(_native.SbaError, match=f"status -1: .*{text}"):
                call()
            assert untouched(), text
        w0 = np.ones(N)
        w0[100] = 0.0
        aln = prob.align(nan_t, w0, apply=False)                   # a NaN target under a zero weight is accepted
        assert aln.n_points_used == N - 1 and aln.rms_after <= TOL_MM and untouched()
        # between sba_lm_begin and sba_lm_finish: SBA_ERR_STATE
        prob.lm_begin(prob.make_opts(ftol=1e-4))
        with pytest.raises(_native.SbaError, match="status -5: .*sba_lm_begin"):
            prob.align(tgt)
        with pytest.raises(_native.SbaError, match="status -5: .*sba_lm_begin"):
            prob.apply_similarity(1.0, R_TRUE, np.zeros(3))
        prob.lm_run()
        prob.lm_finish()
        assert prob.align(tgt, apply=False).n_points_used == N     # and accepted again afterwards


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_handle_of_a_multi_rank_job_is_refused(dtype):
    rig = make_rig(4, 300)
    with _prob(rig, dtype) as prob:
        h = prob.ipc_export(1)
        prob.ipc_attach(0, [h])
        with pytest.raises(_native.SbaError, match="status -6"):
            prob.align(target_points=planted_map(rig["pts0"]))
        with pytest.raises(_native.SbaError, match="status -6"):
            prob.apply_similarity(1.0, R_TRUE, np.zeros(3))


# ----------------------------------------------------------------------------- 5. invariance of the residuals
@pytest.mark.parametrize("dtype", DTYPES)
def test_residuals_stay_where_they_were(dtype):
    rig = make_rig(17, 2000, visibility=0.45, min_cams_per_point=4)
    tgt = planted_map(rig["pts0"]) + np.random.default_rng(3).normal(0.0, 5.0, (2000, 3))
    with _prob(rig, dtype) as prob:
        r0, c0 = prob.residual()
        aln = prob.align(target_points=tgt)
        r1, c1 = prob.residual()
        cams1, pts1 = prob.get_params()
    if dtype == "f64":
        bar = 1e-9
    else:
        with _prob(rig, "f64") as p64:
            r64, _ = p64.residual()
        own = float(np.abs(r0 - r64).max())
        bar = 4.0 * own
        print(f"f32 engine against f64 engine at the same parameters: {own:.2e} px")
    d = float(np.abs(r1 - r0).max())
    print(f"{dtype}: largest residual change under the similarity {d:.2e} px (bar {bar:.2e}), cost {c0:.6f} -> {c1:.6f}, scale {aln.scale:.6f}")
    assert abs(aln.scale - PLANTED["s"]) < 1e-2 and d <= bar
    # the returned rows are the numpy apply step of the reported similarity
    cams_o, pts_o = apply_oracle(rig["cams0"], rig["pts0"], aln.scale, aln.R, aln.t)
    Rd, Ro = Rotation.from_rotvec(cams1[:, 0:3]).as_matrix(), Rotation.from_rotvec(cams_o[:, 0:3]).as_matrix()
    assert np.abs(Rd - Ro).max() <= 1e-12 and np.abs(cams1[:, 3:] - cams_o[:, 3:]).max() <= 1e-9 and np.abs(pts1 - pts_o).max() <= 1e-9


@pytest.mark.parametrize("dtype", DTYPES)
def test_fixed_scale_reports_exactly_one(dtype):
    rig = make_rig(4, 300)
    with _prob(rig, dtype) as prob:
        aln = prob.align(target_points=planted_map(rig["pts0"], s=1.0), with_scale=False)
    ds, dR, dt = _planted_errors(aln, f"with_scale = 0 {dtype}", s_true=1.0)
    assert aln.scale == 1.0 and dR <= TOL_R and dt <= TOL_T and aln.rms_after <= TOL_MM


# ----------------------------------------------------------------------------- 6. state after the call
@pytest.mark.parametrize("dtype", DTYPES)
def test_handle_state_is_what_set_params_leaves(dtype):
    rig = make_rig(6, 600, visibility=0.5)
    tgt = planted_map(rig["pts0"]) + np.random.default_rng(9).normal(0.0, 5.0, (600, 3))
    mask = np.zeros(600, bool)
    mask[[3, 77]] = True                                              # anchored points move with everything else
    with _prob(rig, dtype) as a:
        a.set_fixed_points(mask)
        aln = a.align(target_points=tgt)
        cams1, pts1 = a.get_params()
        assert np.abs(pts1[mask] - aln.transform(rig["pts0"][mask])).max() <= 1e-9
        ra, ca = a.residual()
        sa = a.solve_lm(a.make_opts(ftol=1e-8))
    with _prob(rig, dtype, cams=cams1, pts=pts1) as b:
        b.set_fixed_points(mask)
        rb, cb = b.residual()
        sb = b.solve_lm(b.make_opts(ftol=1e-8))
    assert np.array_equal(ra, rb) and ca == cb
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
    assert sa[2].cost == sb[2].cost and sa[2].nfev == sb[2].nfev and sa[2].status == sb[2].status
    # apply = 0 leaves parameters and a subsequent solve as on an untouched handle
    with _prob(rig, dtype) as c:
        c.align(target_points=tgt, apply=False)
        cams_c, pts_c = c.get_params()
        sc = c.solve_lm(c.make_opts(ftol=1e-8))
    with _prob(rig, dtype) as d:
        sd = d.solve_lm(d.make_opts(ftol=1e-8))
    assert np.array_equal(cams_c, rig["cams0"]) and np.array_equal(pts_c, rig["pts0"])
    assert np.array_equal(sc[0], sd[0]) and np.array_equal(sc[1], sd[1]) and sc[2].cost == sd[2].cost and sc[2].nfev == sd[2].nfev


# ----------------------------------------------------------------------------- 7. rotation vectors at the edges
@pytest.mark.parametrize("dtype", DTYPES)
def test_rotation_vectors_at_zero_and_pi(dtype):
    rig = make_rig(6, 100, seed=5)
    cams = rig["cams0"].copy()
    axis = np.array([0.48, -0.6, 0.64])
    cams[0, 0:3] = 0.0
    cams[1, 0:3] = 1e-9 * axis
    cams[2, 0:3] = (np.pi - 1e-9) * axis
    cams[3, 0:3] = PLANTED["rho"]                                     # composed with R^T: the identity, rho' = 0
    cams[4, 0:3] = -(np.pi - 1e-9) * axis
    near_pi = Rotation.from_rotvec((np.pi - 1e-9) * axis).as_matrix()
    cams[5, 0:3] = Rotation.from_matrix(near_pi @ R_TRUE).as_rotvec()  # composed with R^T: a rotation by pi - 1e-9
    s, t = 0.75, np.array([5.0, -7.0, 11.0])
    with _prob(rig, dtype, cams=cams) as prob:
        prob.apply_similarity(s, R_TRUE, t)
        cams1, pts1 = prob.get_params()
    want = Rotation.from_rotvec(cams[:, 0:3]).as_matrix() @ R_TRUE.T
    got = Rotation.from_rotvec(cams1[:, 0:3]).as_matrix()
    d = np.abs(got - want).max(axis=(1, 2))
    print(f"{dtype}: |R(rho') - R(rho) R^T| per camera {d}, |rho'| of the identity case {np.linalg.norm(cams1[3, 0:3]):.1e}")
    assert d.max() <= 1e-12 and np.all(np.isfinite(cams1))
    assert np.linalg.norm(cams1[3, 0:3]) <= 1e-12 and abs(np.linalg.norm(cams1[5, 0:3]) - np.pi) <= 1e-8
    assert np.linalg.norm(cams1[:, 0:3], axis=1).max() <= np.pi + 1e-12
    assert np.abs(cams1[:, 3:6] - (s * cams[:, 3:6] - want @ t)).max() <= 1e-9
    assert np.array_equal(cams1[:, 6:], cams[:, 6:]) and np.abs(pts1 - (s * rig["pts0"] @ R_TRUE.T + t)).max() <= 1e-9


# ----------------------------------------------------------------------------- 8. determinism
def _report_bits(aln):
    return (aln.scale, aln.R.tobytes(), aln.t.tobytes(), aln.rms_before, aln.rms_after, aln.max_after, aln.n_points_used,
            aln.n_cams_used, aln.sv.tobytes())


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_calls_and_two_handles_give_the_same_bits(dtype):
    rig = make_rig(17, 2000, visibility=0.45, min_cams_per_point=4)
    rng = np.random.default_rng(21)
    tgt = planted_map(rig["pts0"]) + rng.normal(0.0, 5.0, (2000, 3))
    tc = planted_map(centres_of(rig["cams0"])) + rng.normal(0.0, 5.0, (17, 3))
    pw = rng.uniform(0.2, 3.0, 2000)
    with _prob(rig, dtype) as a:
        r1 = _report_bits(a.align(tgt, pw, tc, apply=False))
        r2 = _report_bits(a.align(tgt, pw, tc, apply=False))
        a.align(tgt, pw, tc)
        out_a = a.get_params()
    with _prob(rig, dtype) as b:
        r3 = _report_bits(b.align(tgt, pw, tc))
        out_b = b.get_params()
    assert r1 == r2 == r3
    assert np.array_equal(out_a[0], out_b[0]) and np.array_equal(out_a[1], out_b[1])


# ----------------------------------------------------------------------------- 9. the class mirror
def test_pysba_align_brings_the_solution_back_to_the_initial_frame():
    rig = make_rig(8, 2000)
    cams0, pts0 = rig["cams0"].copy(), rig["pts0"].copy()
    sba = PySBA(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"])
    sba.bundleAdjust(1e-4)
    cams_s, pts_s = sba.cameraArray, sba.points3D
    keep_c, keep_p = cams_s.copy(), pts_s.copy()
    rms_s = _rms_px(cams_s, pts_s, rig)
    aln = sba.align(points=pts0)
    rms_a = _rms_px(sba.cameraArray, sba.points3D, rig)
    print(f"PySBA.align(points=pts0): scale {aln.scale:.6f}, angle {np.degrees(rotation_angle(np.eye(3), aln.R)):.4f} deg, |t| "
          f"{np.linalg.norm(aln.t):.3f} mm, rms {aln.rms_before:.4f} -> {aln.rms_after:.4f} mm; reprojection rms {rms_s:.9f} -> {rms_a:.9f} px")
    assert abs(rms_a - rms_s) <= 1e-9
    assert aln.rms_after <= aln.rms_before and aln.n_points_used == 2000 and aln.n_cams_used == 0
    assert sba.cameraArray is not cams_s and sba.points3D is not pts_s                    # rebound ...
    assert np.array_equal(cams_s, keep_c) and np.array_equal(pts_s, keep_p)               # ... the solve's arrays untouched
    assert np.array_equal(rig["cams0"], cams0) and np.array_equal(rig["pts0"], pts0)      # and the caller's
    assert np.abs(sba.points3D - aln.transform(pts_s)).max() <= 1e-9
    cams_a, pts_a = sba.cameraArray, sba.points3D
    aln_c = sba.align(cameras=cams0, update=False)
    assert aln_c.n_cams_used == 8 and aln_c.n_points_used == 0
    assert sba.cameraArray is cams_a and sba.points3D is pts_a                            # update=False: nothing rebound
    o = align_oracle(cams=cams_a, tgt_centres=centres_of(cams0))
    assert abs(aln_c.scale / o["scale"] - 1) <= TOL_S and np.abs(aln_c.R - o["R"]).max() <= TOL_R


# ----------------------------------------------------------------------------- 10. two optimisers, one frame
def test_two_optimisers_are_brought_into_one_frame(golden):
    g = golden("f9_tight.npz")
    x = g["sparse_x"]
    cams_ref, pts_ref = x[:66].reshape(6, 11), x[66:].reshape(600, 3)
    rig = dict(points_2d=g["sparse_uv"], camera_ind=g["sparse_ci"], point_ind=g["sparse_pi"])
    with _native.Problem(g["sparse_cams0"], g["sparse_pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"]) as prob:
        cams_d, pts_d, rep, _log = prob.solve_lm(prob.make_opts(ftol=1e-10))
        r0, c0 = prob.residual()
        aln = prob.align(target_points=pts_ref)
        r1, c1 = prob.residual()
        cams_a, pts_a = prob.get_params()
    d = float(np.abs(r1 - r0).max())
    assert d <= 1e-9 and aln.rms_after < aln.rms_before
    Ra, Rr = Rotation.from_rotvec(cams_a[:, 0:3]).as_matrix(), Rotation.from_rotvec(cams_ref[:, 0:3]).as_matrix()
    ang = max(rotation_angle(Ra[c], Rr[c]) for c in range(6))
    dc = np.linalg.norm(centres_of(cams_a) - centres_of(cams_ref), axis=1).max()
    dt = np.linalg.norm(cams_a[:, 3:6] - cams_ref[:, 3:6], axis=1).max()
    dX = np.linalg.norm(pts_a - pts_ref, axis=1)
    print(f"F9 sparse, device at ftol 1e-10 (cost {rep.cost:.6f}) aligned to the stored optimum (cost {float(g['sparse_cost']):.6f}): "
          f"scale {aln.scale:.9f}, rotation {np.degrees(rotation_angle(np.eye(3), aln.R)):.6f} deg, |t| {np.linalg.norm(aln.t):.4f} mm, "
          f"point rms {aln.rms_before:.4e} -> {aln.rms_after:.4e} mm (max {aln.max_after:.4e}); remaining: camera rotation "
          f"{np.degrees(ang):.3e} deg, |dt| {dt:.3e} mm, centres {dc:.3e} mm, |dX| max {dX.max():.3e} mm; residual change {d:.1e} px")
