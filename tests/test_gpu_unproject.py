"""GPU tests of sba_unproject and sba_unproject_rows (include/sba_hip.h) through the C ABI: 3-D points on known planes from the
handle's cameras and pixels, and the inverse camera model on gathered rows.

Two references: exact geometry (the noise-free rays of a point meet its plane in the true point) and ``unproject_oracle`` /
``rows_oracle``, the numpy restatements in tests/test_unproject_host.py, which are checked there against the same geometry and
against the reference's algebra.  Device and oracle are both float64 on the same inputs and differ in summation order and fused
multiply-adds only: eps64 x scale x cond(G) x views = 1.1e-16 x 2.3e3 mm x 1 / 0.1^2 x 64 = 1.6e-9 mm (the planes of these
tests meet every ray at |nh . d| >= 0.1, asserted in the host file), hence the project's bars for this arithmetic
(tests/test_gpu_triangulate.py): 1e-8 mm on coordinates, 1e-8 px on rms_px / max_px; integers and flags have to be equal."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lasercalib_amd import _native, dataset  # noqa: E402
from lasercalib_amd.synth import _project_np, make_rig  # noqa: E402
from test_gpu_triangulate import LAYOUT_CASES, NOISY, _check_route, _close  # noqa: E402
from test_unproject_host import (ROW_BEHIND, ROW_OK, ROW_PARALLEL, ROW_UNUSABLE, UNP_ANCHORED, UNP_NO_VIEW, UNP_OK,  # noqa: E402
                                 check_status_result, rays_oracle, rows_oracle, status_problem, tilted_planes, unproject_oracle,
                                 z_planes_of)

TOL_MM, TOL_PX = 1e-8, 1e-8


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert _native.device_count() > 0, "no HIP device visible: GPU tests must run on the MI355X box"


def _against_oracle(unp, o, label=""):
    d_x, d_rms, d_max = _close(unp.points, o["points"], TOL_MM), _close(unp.rms_px, o["rms_px"], TOL_PX), _close(unp.max_px, o["max_px"], TOL_PX)
    print(f"{label}: device - oracle: X {d_x:.2e} mm, rms {d_rms:.2e} px, max {d_max:.2e} px")
    assert np.array_equal(unp.status, o["status"]) and np.array_equal(unp.n_views, o["n_views"])
    assert np.array_equal(unp.used, o["used"])
    assert (unp.n_obs_unusable, unp.n_obs_used) == (o["n_obs_unusable"], o["n_obs_used"])
    hist = np.bincount(unp.status, minlength=5)
    assert [unp.n_ok, unp.n_anchored, unp.n_no_view, unp.n_degenerate, unp.n_behind] == list(hist)
    assert d_x <= TOL_MM and d_rms <= TOL_PX and d_max <= TOL_PX


# ----------------------------------------------------------------------------- 1. exact geometry, every layout
@pytest.mark.parametrize("name,args,layout", LAYOUT_CASES, ids=[c[0] for c in LAYOUT_CASES])
def test_noise_free_rays_meet_the_plane_in_the_true_point(name, args, layout):
    rig = make_rig(noise_px=0.0, **args)
    N, ci, pi, truth = rig["n_points"], rig["camera_ind"], rig["point_ind"], rig["pts_true"]
    zp, tp = z_planes_of(truth), tilted_planes(truth)
    with _native.Problem(rig["cams_true"], rig["pts0"], rig["points_2d"], ci, pi, layout=layout) as prob:
        _check_route(prob, rig, layout)
        allv = prob.unproject(zp)
        one = prob.unproject(zp, ref_cam=1)
        tilt = prob.unproject(tp)
        tilt1 = prob.unproject(tp, ref_cam=1)
    sees = np.bincount(pi[ci == 1], minlength=N) > 0
    err = [np.abs(allv.points - truth).max(), np.abs(one.points[sees] - truth[sees]).max(), np.abs(tilt.points - truth).max(),
           np.abs(tilt1.points[sees] - truth[sees]).max()]
    print(f"{name}: max |X - truth| mm: z-planes {err[0]:.3e} (all views) {err[1]:.3e} (camera 1), tilted {err[2]:.3e} / {err[3]:.3e}; "
          f"max_px {allv.max_px.max():.3e}")
    for u in (allv, tilt):
        assert np.all(u.status == UNP_OK) and u.used.all() and u.ok.all()
        assert np.array_equal(u.n_views, np.bincount(pi, minlength=N))
        assert (u.n_ok, u.n_obs_unusable, u.n_obs_used) == (N, 0, ci.size)
    for u in (one, tilt1):
        assert np.array_equal(u.ok, sees) and np.all(u.status[~sees] == UNP_NO_VIEW) and np.isnan(u.points[~sees]).all()
        assert np.array_equal(u.used, ci == 1) and np.array_equal(u.n_views, sees.astype(np.int32))
    assert max(err) <= 1e-8 and allv.max_px.max() <= 1e-8
    off = np.abs(np.sum(tp[:, :3] * tilt.points, axis=1) - tp[:, 3]) / np.linalg.norm(tp[:, :3], axis=1)
    assert off.max() <= 1e-9
    _against_oracle(allv, unproject_oracle(rig["cams_true"], rig["points_2d"], ci, pi, N, zp), name)


# ----------------------------------------------------------------------------- 2. noisy lists against the oracle
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("k", range(len(NOISY)))
def test_noisy_shuffled_weighted_anchored_against_the_oracle(k, dtype):
    rig = make_rig(noise_px=0.3, **NOISY[k])
    N, M = rig["n_points"], rig["camera_ind"].size
    rng = np.random.default_rng(17)
    w = rng.uniform(0.25, 3.0, M)
    w[rng.random(M) < 0.05] = 0.0
    fixed = np.zeros(N, bool)
    fixed[rng.choice(N, 20, replace=False)] = True
    s = rng.permutation(M)
    uv, ci, pi, w = rig["points_2d"][s], rig["camera_ind"][s], rig["point_ind"][s], w[s]
    if dtype == "f32":                 # the oracle is given what the handle holds
        uv, w = uv.astype(np.float32).astype(np.float64), w.astype(np.float32).astype(np.float64)
    cams, held = rig["cams0"], rig["pts0"]
    zp, tp = z_planes_of(rig["pts_true"]), tilted_planes(rig["pts_true"])
    with _native.Problem(cams, held, uv, ci, pi, weights=w, dtype=dtype) as prob:
        prob.set_fixed_points(fixed)
        runs = [(prob.unproject(zp), dict(planes=zp)), (prob.unproject(zp, ref_cam=1), dict(planes=zp, ref_cam=1)),
                (prob.unproject(tp, min_views=2), dict(planes=tp, min_views=2)),
                (prob.unproject(zp[0]), dict(planes=zp[0]))]
    for unp, kw in runs:
        o = unproject_oracle(cams, uv, ci, pi, N, w=w, fixed=fixed, pts=held, **kw)
        _against_oracle(unp, o, f"{NOISY[k]} {dtype} {[(a, b) for a, b in kw.items() if a != 'planes']}")
    allv = runs[0][0]
    assert allv.n_anchored == 20 and np.array_equal(allv.points[fixed], held[fixed])
    assert allv.n_obs_unusable == int(((w == 0) & ~fixed[pi]).sum())
    assert allv.n_ok >= 0.9 * N
    dist = np.linalg.norm(allv.points[allv.ok] - rig["pts_true"][allv.ok], axis=1)
    print(f"median distance to the truth from the perturbed cameras: {np.median(dist):.2f} mm")


# ----------------------------------------------------------------------------- 3. every status
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_statuses_on_a_hand_built_problem(dtype):
    sp = status_problem()
    uv = sp["uv"].astype(np.float32).astype(np.float64) if dtype == "f32" else sp["uv"]
    with _native.Problem(sp["cams"], sp["held"], uv, sp["ci"], sp["pi"], weights=sp["w"], dtype=dtype) as prob:
        prob.set_fixed_points(sp["fixed"])
        u1, u2, u0 = prob.unproject(sp["planes"]), prob.unproject(sp["planes"], min_views=2), prob.unproject(sp["planes"], min_views=0)
    if dtype == "f64":
        check_status_result(sp, u1, 1)
        check_status_result(sp, u2, 2)
    assert list(u1.status) == sp["expect1"] and list(u2.status) == sp["expect2"] and list(u0.status) == sp["expect1"]
    kw = dict(w=sp["w"], fixed=sp["fixed"], pts=sp["held"])
    _against_oracle(u1, unproject_oracle(sp["cams"], uv, sp["ci"], sp["pi"], 8, sp["planes"], **kw), "statuses")
    _against_oracle(u2, unproject_oracle(sp["cams"], uv, sp["ci"], sp["pi"], 8, sp["planes"], min_views=2, **kw), "statuses, min_views 2")


# ----------------------------------------------------------------------------- 4. sba_unproject_rows
@pytest.mark.parametrize("tangential", [False, True])
def test_rows_invert_the_projection(tangential):
    rig = make_rig(17, 3000, seed=3, visibility=0.45, noise_px=0.0, tangential=tangential)
    ci, pi = rig["camera_ind"], rig["point_ind"]
    rows, X = rig["cams_true"][ci], rig["pts_true"][pi]
    uv = _native.project_rows(X, rows)
    planes = tilted_planes(rig["pts_true"])[pi]
    out = _native.unproject_rows(uv, rows, planes)
    o = rows_oracle(uv, rows, planes)
    x, y, conv, _R, origin, d = rays_oracle(rows, uv)
    diffs = [np.abs(out["points"] - X).max(), np.abs(out["xn"] - np.stack([x, y], 1)).max(), np.abs(out["origin"] - origin).max(),
             np.abs(out["dir"] - d).max(), np.abs(out["points"] - o["points"]).max(), np.abs(out["depth"] - o["depth"]).max()]
    print(f"tangential {tangential}: |X - truth| {diffs[0]:.2e} mm, xn {diffs[1]:.2e}, origin {diffs[2]:.2e}, dir {diffs[3]:.2e}, "
          f"X - oracle {diffs[4]:.2e} mm, depth - oracle {diffs[5]:.2e} mm")
    assert conv.all() and np.all(out["status"] == ROW_OK) and np.array_equal(out["status"], o["status"])
    assert diffs[0] <= 1e-8 and diffs[1] <= 1e-13 and diffs[2] <= 1e-12 and diffs[3] <= 1e-12 and diffs[4] <= 1e-8 and diffs[5] <= 1e-8
    assert np.all(out["depth"] > 0)
    # rays only
    rays = _native.unproject_rows(uv, rows)
    assert set(rays) == {"xn", "origin", "dir", "status"}
    for name in rays:
        assert np.array_equal(rays[name], out[name]), name


def test_rows_single_plane_equals_per_row_planes_and_small_n():
    rig = make_rig(6, 700, seed=7, noise_px=0.3)
    rows, uv = rig["cams0"][rig["camera_ind"]], rig["points_2d"]
    n = uv.shape[0]
    assert n % 256 != 0 and n > 256
    pl = np.array([0.1, -0.05, 1.0, 53.0])
    one, per_row = _native.unproject_rows(uv, rows, pl), _native.unproject_rows(uv, rows, np.tile(pl, (n, 1)))
    for name in one:
        assert np.array_equal(one[name], per_row[name]), name
    assert np.all(one["status"] == ROW_OK)
    first = _native.unproject_rows(uv[:1], rows[:1], pl)
    for name in one:
        assert np.array_equal(first[name], one[name][:1]), name
    none = _native.unproject_rows(np.empty((0, 2)), np.empty((0, 11)), pl)
    assert none["points"].shape == (0, 3) and none["status"].shape == (0,)


def test_rows_statuses():
    sp = status_problem()
    cams, pts = sp["cams"], sp["pts"]
    rows = cams[[0, 4, 0, 0]]
    uv = _project_np(pts[[0, 0, 4, 5]], rows)
    uv[1] = sp["uv"][sp["k_fold"]]
    planes = np.stack([sp["planes"][0], sp["planes"][0], sp["planes"][4], sp["planes"][5]])
    out = _native.unproject_rows(uv, rows, planes)
    assert list(out["status"]) == [ROW_OK, ROW_UNUSABLE, ROW_PARALLEL, ROW_BEHIND]
    assert np.array_equal(out["status"], rows_oracle(uv, rows, planes)["status"])
    for name in ("xn", "origin", "dir", "points", "depth"):
        assert np.isnan(out[name][1]).all(), name
    assert np.isnan(out["points"][2]).all() and np.isnan(out["depth"][2]) and np.isfinite(out["dir"][2]).all()
    assert np.isfinite(out["points"][3]).all() and out["depth"][3] < 0 and abs(out["points"][3, 2] - 2000.0) <= 1e-8
    assert np.abs(out["points"][0] - pts[0]).max() <= 1e-8
    rays = _native.unproject_rows(uv, rows)
    assert list(rays["status"]) == [ROW_OK, ROW_UNUSABLE, ROW_OK, ROW_OK]


def test_rows_errors():
    rig = make_rig(2, 20)
    rows, uv = rig["cams0"][rig["camera_ind"]], rig["points_2d"]
    n = uv.shape[0]
    for bad in ((0.0, 0.0, 0.0, 1.0), (np.nan, 0.0, 1.0, 1.0), (0.0, 0.0, 1.0, np.inf), np.ones((3, 4))):
        with pytest.raises(_native.SbaError, match="status -1"):
            _native.unproject_rows(uv, rows, bad)
    lib = _native.load()
    out = np.full((n, 3), 7.0)
    args = (_native._dptr(uv), _native._dptr(rows), None, 0, None, None, None)
    assert lib.sba_unproject_rows(0, 0, n, *args, _native._dptr(out), None, None) == -1      # points_out without a plane
    assert lib.sba_unproject_rows(0, 5, n, *args, None, None, None) == -1                    # unknown camera model
    assert lib.sba_unproject_rows(0, 0, -1, *args, None, None, None) == -1
    assert np.all(out == 7.0)


def test_pysba_undistort_then_the_ideal_camera_reproduces_project():
    from lasercalib_amd.pySBA import PySBA
    rig = make_rig(17, 2000, seed=3, visibility=0.45, noise_px=0.0, tangential=True)
    ci, pi = rig["camera_ind"], rig["point_ind"]
    rows, X = rig["cams_true"][ci], rig["pts_true"][pi]
    sba = PySBA(rig["cams_true"], rig["pts0"], rig["points_2d"], ci, pi)
    uv = sba.project(X, rows)
    ideal = sba.undistort(uv, rows)
    pinhole = rows.copy()
    pinhole[:, 7:11] = 0.0                      # k1, k2, p1, p2
    diff = np.abs(sba.project(X, pinhole) - ideal).max()
    print(f"undistort, then the distortion-free model: {diff:.2e} px")
    assert diff <= 1e-9 and np.abs(ideal - uv).max() > 1e-3
    rows[0, 7:11], uv[0] = (-0.5, 0.0, 0.0, 0.0), (rows[0, -2] + rows[0, 6] * 0.6, rows[0, -1])
    assert np.isnan(sba.undistort(uv, rows)[0]).all()


# ----------------------------------------------------------------------------- 5. one view: the handle against the rows
def test_one_view_equals_the_rows():
    rig = make_rig(17, 3000, seed=3, visibility=0.45, noise_px=0.3)
    N, ci, pi, uv, cams = rig["n_points"], rig["camera_ind"], rig["point_ind"], rig["points_2d"], rig["cams0"]
    zp = z_planes_of(rig["pts_true"])
    with _native.Problem(cams, rig["pts0"], uv, ci, pi) as prob:
        unp = prob.unproject(zp, ref_cam=1)
    sel = np.nonzero(ci == 1)[0]
    out = _native.unproject_rows(uv[sel], cams[ci[sel]], zp[pi[sel]])
    assert np.all(out["status"] == ROW_OK) and np.array_equal(np.nonzero(unp.ok)[0], pi[sel])
    diff = np.abs(unp.points[pi[sel]] - out["points"]).max()
    print(f"sba_unproject(ref_cam=1) - sba_unproject_rows: {diff:.2e} mm; rms_px of one view {np.nanmax(unp.rms_px):.2e}")
    assert diff <= 1e-8 and np.nanmax(unp.max_px) <= 1e-8


# ----------------------------------------------------------------------------- 6. the handle: untouched, or written back
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("C,N", [(16, 400), (64, 600)])
def test_unproject_leaves_the_handle_as_it_was(C, N, dtype):
    rig = make_rig(C, N, seed=29, visibility=0.6 if C > 16 else 1.0)
    args = (rig["points_2d"], rig["camera_ind"], rig["point_ind"])
    zp = z_planes_of(rig["pts_true"])
    opts = dict(ftol=1e-6, max_iter=6)
    with _native.Problem(rig["cams0"], rig["pts0"], *args, dtype=dtype) as a:
        before, (_r, cost_before) = a.get_params(), a.residual(want_r=False)
        u1 = a.unproject(zp)
        a.unproject(zp, ref_cam=1, min_views=1)
        u2 = a.unproject(zp)
        after, (_r, cost_after) = a.get_params(), a.residual(want_r=False)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and cost_before == cost_after
        for name in ("points", "status", "n_views", "rms_px", "max_px", "used"):           # a repeated call: the same bits
            assert np.array_equal(getattr(u1, name), getattr(u2, name), equal_nan=name in ("points", "rms_px", "max_px")), name
        ca, pa, ra, _ = a.solve_lm(a.make_opts(**opts))
    with _native.Problem(rig["cams0"], rig["pts0"], *args, dtype=dtype) as b:
        _r, cost_fresh = b.residual(want_r=False)
        cb, pb, rb, _ = b.solve_lm(b.make_opts(**opts))
    assert cost_before == cost_fresh
    assert np.array_equal(ca, cb) and np.array_equal(pa, pb) and ra.cost == rb.cost


def test_write_back_moves_exactly_the_ok_points():
    sp = status_problem()
    with _native.Problem(sp["cams"], sp["held"], sp["uv"], sp["ci"], sp["pi"], weights=sp["w"]) as prob:
        prob.set_fixed_points(sp["fixed"])
        unp = prob.unproject(sp["planes"], write_back=True)
        cams, now = prob.get_params()
    ok = unp.status == UNP_OK
    assert ok.sum() == 4 and np.array_equal(now[ok], unp.points[ok]) and np.array_equal(now[~ok], sp["held"][~ok])
    assert np.array_equal(cams, sp["cams"]) and unp.status[1] == UNP_ANCHORED


def test_bundle_adjust_from_the_written_back_points():
    from lasercalib_amd.pySBA import PySBA
    rig = make_rig(17, 3000, seed=3, visibility=0.45, noise_px=0.3)
    args = (rig["points_2d"], rig["camera_ind"], rig["point_ind"])
    with _native.Problem(rig["cams0"], np.zeros((3000, 3)), *args) as prob:
        unp = prob.unproject(z_planes_of(rig["pts_true"]), write_back=True)
        _c, start = prob.get_params()
    assert unp.ok.all() and np.array_equal(start, unp.points)
    res = PySBA(rig["cams0"].copy(), start, *args).bundleAdjust(1e-4)
    ref = PySBA(rig["cams0"].copy(), rig["pts_true"].copy(), *args).bundleAdjust(1e-4)
    rel = abs(res.cost - ref.cost) / ref.cost
    print(f"bundleAdjust(1e-4): cost {res.cost:.9e} from the un-projected points (nfev {res.nfev}), {ref.cost:.9e} from pts_true "
          f"(nfev {ref.nfev}), rel {rel:.2e}")
    assert res.status > 0 and ref.status > 0
    assert rel <= 1e-6


# ----------------------------------------------------------------------------- 7. errors
def test_errors_leave_the_outputs_untouched():
    import ctypes as C
    rig = make_rig(4, 60, seed=41)
    N, M = 60, rig["camera_ind"].size
    zp = z_planes_of(rig["pts_true"])
    with _native.Problem(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"]) as prob:
        for planes in ((0.0, 0.0, 0.0, 1.0), (0.0, np.nan, 1.0, 1.0), (0.0, 0.0, 1.0, np.inf), zp[:7], np.vstack([zp[:-1], [[0, 0, 0, 1]]])):
            with pytest.raises(_native.SbaError, match="status -1"):
                prob.unproject(planes)
        for ref_cam in (-1, 4):
            with pytest.raises(_native.SbaError, match="status -1"):
                prob.unproject(zp, ref_cam=ref_cam)
        # the raw call: nothing is written on failure
        pts, status, used = np.full((N, 3), 7.0), np.full(N, 9, np.int32), np.full(M, 5, np.uint8)
        rep = _native.UnpReport()
        rep.n_ok = 123
        bad = np.ascontiguousarray([0.0, 0.0, 0.0, 1.0])
        rc = prob._lib.sba_unproject(prob._h, None, _native._dptr(bad), 1, _native._dptr(pts), status.ctypes.data_as(C.POINTER(C.c_int32)),
                                     None, None, None, used.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(rep))
        assert rc == -1 and np.all(pts == 7.0) and np.all(status == 9) and np.all(used == 5) and rep.n_ok == 123
        assert prob._lib.sba_unproject(prob._h, None, None, 1, None, None, None, None, None, None, None) == -1
        # NULL opts and NULL outputs are fine
        assert prob._lib.sba_unproject(prob._h, None, _native._dptr(zp), N, None, None, None, None, None, None, C.byref(rep)) == 0
        assert rep.n_ok == N
        prob.lm_begin(prob.make_opts(ftol=1e-4))
        with pytest.raises(_native.SbaError, match="status -5"):
            prob.unproject(zp)
        prob.lm_finish()
        assert prob.unproject(zp).ok.all()
        h = prob.ipc_export(1)
        prob.ipc_attach(0, [h])
        with pytest.raises(_native.SbaError, match="status -6"):
            prob.unproject(zp)


# ----------------------------------------------------------------------------- 8. the Python surface
def test_pysba_unproject(monkeypatch):
    from lasercalib_amd.pySBA import PySBA
    rig = make_rig(6, 300, seed=9, noise_px=0.0)
    start = np.zeros((300, 3))
    z = rig["pts_true"][:, 2]
    sba = PySBA(rig["cams_true"], start, rig["points_2d"], rig["camera_ind"], rig["point_ind"])
    unp = sba.unproject(z=z)
    assert sba.points3D is not start and not start.any()
    assert unp.ok.all() and np.array_equal(sba.points3D, unp.points) and np.abs(unp.points - rig["pts_true"]).max() <= 1e-8
    ground = z == 0.0
    unp0 = sba.unproject(z=0.0, ref_cam=2, update=False)
    assert np.abs(unp0.points[ground] - rig["pts_true"][ground]).max() <= 1e-8 and np.all(unp0.n_views == 1)
    same = sba.unproject(planes=z_planes_of(rig["pts_true"]), update=False)
    assert np.array_equal(same.points, unp.points)
    with pytest.raises(ValueError):
        sba.unproject()
    with pytest.raises(ValueError):
        sba.unproject(z=0.0, planes=(0, 0, 1, 0))
    monkeypatch.setenv("LASERCALIB_SBA_USE_FIXED", "1")
    sba2 = PySBA(rig["cams_true"], start, rig["points_2d"], rig["camera_ind"], rig["point_ind"], points3Dfixed=np.array([3, 5]))
    unp2 = sba2.unproject(z=z)
    assert list(np.nonzero(unp2.status == UNP_ANCHORED)[0]) == [3, 5]
    assert np.array_equal(sba2.points3D[[3, 5]], start[[3, 5]]) and np.abs(sba2.points3D[0] - rig["pts_true"][0]).max() <= 1e-8


def test_dataset_from_unprojection():
    rig = make_rig(4, 40, seed=2, noise_px=0.0, visibility=0.6)
    cent = np.full((40, 2, 4), np.nan)
    cent[rig["point_ind"], :, rig["camera_ind"]] = rig["points_2d"]
    z = rig["pts_true"][:, 2]
    ds = dataset.make_dataset_unprojected(cent, rig["cams_true"], z)
    ref = dataset.make_dataset(cent, rig["pts_true"])
    assert set(ds) == set(ref) and ds["n_pts"] == 40 and ds["n_cams"] == 4
    assert np.array_equal(ds["point_ind"], ref["point_ind"]) and np.array_equal(ds["camera_ind"], ref["camera_ind"])
    assert np.array_equal(ds["points_2d"], ref["points_2d"]) and np.abs(ds["points_3d"] - ref["points_3d"]).max() <= 1e-8
    assert all(ds[k].dtype == ref[k].dtype for k in ("points_2d", "points_3d", "camera_ind", "point_ind"))
    # the reference's route: only the frames the 3-D init camera saw survive
    sees = ~np.isnan(cent[:, 0, 0])
    assert 0 < sees.sum() < 40
    ds0 = dataset.make_dataset_unprojected(cent, rig["cams_true"], z, cam_idx_3dpts=0)
    ref0 = dataset.make_dataset(cent[sees], rig["pts_true"][sees])
    assert ds0["n_pts"] == sees.sum() and np.array_equal(ds0["point_ind"], ref0["point_ind"])
    assert np.array_equal(ds0["camera_ind"], ref0["camera_ind"]) and np.abs(ds0["points_3d"] - ref0["points_3d"]).max() <= 1e-8
    ds2 = dataset.make_dataset_unprojected(cent, rig["cams_true"], 0.0, min_views=2)
    two = (~np.isnan(cent[:, 0, :])).sum(axis=1) >= 2
    assert ds2["n_pts"] == two.sum()
