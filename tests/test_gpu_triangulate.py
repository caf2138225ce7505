"""GPU tests of sba_triangulate (include/sba_hip.h) through the C ABI: 3-D points from the handle's cameras and pixels.

Two references, neither of them a run of somebody else's triangulator: exact geometry (noise-free rays meet in the true point)
and ``tri_oracle``, the numpy restatement of the estimator in tests/test_triangulate_host.py, which is checked there against
the same geometry.  Device and oracle are both float64 on the same inputs and differ in summation order and fused multiply-adds
only: eps64 x scale x cond(A) x views = 1.1e-16 x 2.3e3 mm x 1e3 x 8 = 2e-9 mm (the largest condition number on these rigs is
949, on the 64-camera one), hence the bars 1e-8 mm on coordinates, 1e-8 px on rms_px / max_px, 1e-12 on spread; integers and
flags have to be equal."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lasercalib_amd import _native, dataset  # noqa: E402
from lasercalib_amd.synth import _project_np, make_rig  # noqa: E402
from test_triangulate_host import (OUTLIER_RIGS, TRI_ANCHORED, TRI_BEHIND, TRI_DEGENERATE, TRI_OK, TRI_TOO_FEW,  # noqa: E402
                                   outlier_rig, plant_outliers, tri_oracle)

TOL_MM, TOL_PX, TOL_SPREAD = 1e-8, 1e-8, 1e-12


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert _native.device_count() > 0, "no HIP device visible: GPU tests must run on the MI355X box"


def _close(a, b, tol):
    """max |a - b| with NaN allowed only where both are NaN."""
    assert np.array_equal(np.isnan(a), np.isnan(b))
    m = ~np.isnan(a)
    return float(np.abs(a[m] - b[m]).max()) if m.any() else 0.0


def _against_oracle(tri, o, label=""):
    d_x, d_rms = _close(tri.points, o["points"], TOL_MM), _close(tri.rms_px, o["rms_px"], TOL_PX)
    d_max, d_spread = _close(tri.max_px, o["max_px"], TOL_PX), _close(tri.spread, o["spread"], TOL_SPREAD)
    print(f"{label}: device - oracle: X {d_x:.2e} mm, rms {d_rms:.2e} px, max {d_max:.2e} px, spread {d_spread:.2e}")
    assert np.array_equal(tri.status, o["status"]) and np.array_equal(tri.n_views, o["n_views"])
    assert np.array_equal(tri.inliers, o["inliers"])
    assert (tri.n_obs_unusable, tri.n_obs_trimmed, tri.n_points_trimmed) == (o["n_obs_unusable"], o["n_obs_trimmed"], o["n_points_trimmed"])
    hist = np.bincount(tri.status, minlength=5)
    assert [tri.n_ok, tri.n_anchored, tri.n_too_few, tri.n_degenerate, tri.n_behind] == list(hist)
    assert d_x <= TOL_MM and d_rms <= TOL_PX and d_max <= TOL_PX and d_spread <= TOL_SPREAD


# the layouts the upload can produce: (name, rig arguments, layout route)
LAYOUT_CASES = [
    ("16x2000 dense, dense kernel", dict(n_cams=16, n_points=2000, seed=0), "auto"),
    ("16x2000 dense, host pass", dict(n_cams=16, n_points=2000, seed=0), "host"),
    ("16x2000 visibility 0.6, masked, host", dict(n_cams=16, n_points=2000, seed=4, visibility=0.6), "host"),
    ("16x2000 visibility 0.6, masked, device", dict(n_cams=16, n_points=2000, seed=4, visibility=0.6), "device"),
    ("17x3000 visibility 0.45, host", dict(n_cams=17, n_points=3000, seed=3, visibility=0.45), "host"),
    ("17x3000 visibility 0.45, device", dict(n_cams=17, n_points=3000, seed=3, visibility=0.45), "device"),
    ("64x3000 visibility 0.1, host", dict(n_cams=64, n_points=3000, seed=2, visibility=0.1), "auto"),
    ("64x3000 visibility 0.1, device", dict(n_cams=64, n_points=3000, seed=2, visibility=0.1), "device"),
    ("2x500", dict(n_cams=2, n_points=500, seed=1), "auto"),
    ("6x3000", dict(n_cams=6, n_points=3000, seed=7), "auto"),
    ("17x2000 visibility 0.45, 13 columns", dict(n_cams=17, n_points=2000, seed=3, visibility=0.45, tangential=True), "auto"),
]


def _check_route(prob, rig, layout):
    """The upload took the route and left the layout flags this case is in the list for."""
    C, N, M = rig["n_cams"], rig["n_points"], rig["camera_ind"].size
    rep = prob.upload_report()
    dense = M == N * C
    route = "host" if layout == "host" else "device dense" if dense else \
        "device general" if (layout == "device" or M >= 100000) else "host"
    assert rep["route"] == route, rep
    assert rep["dense"] == dense and rep["masked"] == (C <= 16 and not dense) and rep["group_indexed"] == (C > 16), rep
    return rep


@pytest.mark.parametrize("name,args,layout", LAYOUT_CASES, ids=[c[0] for c in LAYOUT_CASES])
def test_noise_free_rays_meet_in_the_true_point(name, args, layout):
    rig = make_rig(noise_px=0.0, **args)
    N = rig["n_points"]
    with _native.Problem(rig["cams_true"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"], layout=layout) as prob:
        _check_route(prob, rig, layout)
        tri = prob.triangulate()
    err = np.abs(tri.points - rig["pts_true"]).max()
    print(f"{name}: max |X - truth| = {err:.3e} mm, max_px {tri.max_px.max():.3e}")
    assert np.all(tri.status == TRI_OK) and tri.inliers.all() and tri.ok.all()
    assert np.array_equal(tri.n_views, np.bincount(rig["point_ind"], minlength=N))
    assert err <= 1e-8 and tri.max_px.max() <= 1e-8
    assert (tri.n_ok, tri.n_obs_unusable, tri.n_obs_trimmed) == (N, 0, 0)
    _against_oracle(tri, tri_oracle(rig["cams_true"], rig["points_2d"], rig["camera_ind"], rig["point_ind"], N), name)


@pytest.mark.parametrize("layout", ["device", "host"])
def test_shuffled_list_comes_back_in_the_callers_order(layout):
    rig = make_rig(17, 3000, seed=3, visibility=0.45, noise_px=0.0)
    uv, ci, pi = rig["points_2d"], rig["camera_ind"], rig["point_ind"]
    with _native.Problem(rig["cams_true"], rig["pts0"], uv, ci, pi, layout=layout) as prob:
        ref = prob.triangulate()
    # a planted outlier so that the flags are not all ones
    uvb = uv.copy()
    uvb[5] += 60.0
    with _native.Problem(rig["cams_true"], rig["pts0"], uvb, ci, pi, layout=layout) as prob:
        refb = prob.triangulate(trim_px=3.0)
    assert not refb.inliers[5] and refb.inliers.sum() == uv.shape[0] - 1
    s = np.random.default_rng(5).permutation(uv.shape[0])
    with _native.Problem(rig["cams_true"], rig["pts0"], uv[s], ci[s], pi[s], layout=layout) as prob:
        assert prob.upload_report()["route"] == ("host" if layout == "host" else "device general")
        assert not prob.upload_report()["identity_perm"]
        tri = prob.triangulate()
    for name in ("points", "status", "n_views", "rms_px", "max_px", "spread"):
        assert np.array_equal(getattr(tri, name), getattr(ref, name)), name
    assert np.array_equal(tri.inliers, ref.inliers[s])
    assert np.abs(tri.points - rig["pts_true"]).max() <= 1e-8
    with _native.Problem(rig["cams_true"], rig["pts0"], uvb[s], ci[s], pi[s], layout=layout) as prob:
        trib = prob.triangulate(trim_px=3.0)
    assert np.array_equal(trib.inliers, refb.inliers[s]) and np.array_equal(trib.status, refb.status)
    assert _close(trib.points, refb.points, TOL_MM) <= TOL_MM


# ----------------------------------------------------------------------------- 2. f32 handles
@pytest.mark.parametrize("name,args,layout", LAYOUT_CASES, ids=[c[0] for c in LAYOUT_CASES])
def test_f32_handle_holds_what_the_oracle_is_given(name, args, layout):
    rig = make_rig(noise_px=0.0, **args)
    N = rig["n_points"]
    uv32 = rig["points_2d"].astype(np.float32).astype(np.float64)
    w32 = np.random.default_rng(3).uniform(0.5, 2.0, uv32.shape[0]).astype(np.float32).astype(np.float64)
    with _native.Problem(rig["cams_true"], rig["pts0"], uv32, rig["camera_ind"], rig["point_ind"], weights=w32, dtype="f32",
                         layout=layout) as prob:
        _check_route(prob, rig, layout)
        tri = prob.triangulate()
    err = np.abs(tri.points - rig["pts_true"]).max()
    print(f"{name}: f32 handle, max |X - truth| = {err:.3e} mm")
    _against_oracle(tri, tri_oracle(rig["cams_true"], uv32, rig["camera_ind"], rig["point_ind"], N, w=w32), name)
    assert np.all(tri.status == TRI_OK) and err <= 5e-3


# ----------------------------------------------------------------------------- 3. noisy pixels, weights, zero weights
NOISY = [dict(n_cams=16, n_points=2000, seed=0), dict(n_cams=17, n_points=3000, seed=3, visibility=0.45),
         dict(n_cams=64, n_points=3000, seed=2, visibility=0.1), dict(n_cams=17, n_points=2000, seed=3, visibility=0.45, tangential=True)]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("cams", ["cams_true", "cams0"])
@pytest.mark.parametrize("k", range(len(NOISY)))
def test_noisy_against_the_oracle(k, cams, weighted):
    rig = make_rig(noise_px=0.3, **NOISY[k])
    N, M = rig["n_points"], rig["camera_ind"].size
    w = None
    if weighted:
        rng = np.random.default_rng(17)
        w = rng.uniform(0.25, 3.0, M)
        w[rng.random(M) < 0.05] = 0.0
    with _native.Problem(rig[cams], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"], weights=w) as prob:
        tri = prob.triangulate()
    o = tri_oracle(rig[cams], rig["points_2d"], rig["camera_ind"], rig["point_ind"], N, w=w)
    _against_oracle(tri, o, f"{NOISY[k]} {cams} weighted={weighted}")
    assert tri.n_ok >= 0.8 * N
    if weighted:
        assert tri.n_obs_unusable == int((w == 0).sum())
    if cams == "cams_true" and NOISY[k]["n_cams"] <= 17:      # (two neighbouring views of the 64-camera ring have little parallax)
        assert np.nanmax(np.linalg.norm(tri.points - rig["pts_true"], axis=1)) < 5.0


# ----------------------------------------------------------------------------- 4. statuses
def _status_problem():
    rig = make_rig(4, 9, seed=1, noise_px=0.0)
    cams = rig["cams_true"].copy()
    cams[:, 7:9] = 0.0                                   # pinhole cameras: the images of a point behind a camera are exact
    cams[3] = cams[2]                                    # two cameras with identical rows
    fold = cams[0].copy()
    fold[7], fold[8] = -0.5, 0.0                         # r (1 + k1 r^2) peaks at 0.544 for r = 0.816: radius 0.6 has no pre-image
    cams = np.vstack([cams, fold])
    pts = rig["pts_true"].copy()
    pts[3] = (3000.0, 3000.0, 3000.0)                    # behind cameras 0 and 1 (they look from the ring at the origin)
    obs = [(0, 0), (1, 0), (1, 0), (2, 2), (2, 3), (3, 0), (3, 1), (4, 0), (4, 1), (5, 0), (5, 1),
           (6, 0), (6, 1), (6, 4), (7, 0), (7, 1), (7, 2)]            # (point, camera); point 8 has no observation
    pi = np.array([p for p, _c in obs])
    ci = np.array([c for _p, c in obs])
    uv = _project_np(pts[pi], cams[ci])
    uv[2] += 5.0                                         # the second pixel of point 1 in camera 0 differs from the first
    k = obs.index((6, 4))
    uv[k] = (fold[9] + fold[6] * 0.6, fold[10])
    held = pts + 7.0
    fixed = np.arange(9) == 4
    return cams, pts, held, uv, ci, pi, fixed, k


def test_statuses_on_a_hand_built_problem():
    cams, pts, held, uv, ci, pi, fixed, k_fold = _status_problem()
    with _native.Problem(cams, held, uv, ci, pi) as prob:
        prob.set_fixed_points(fixed)
        tri = prob.triangulate()
        tri3 = prob.triangulate(min_views=3)
        for bad in (dict(min_views=1), dict(trim_px=-1.0), dict(trim_px=float("inf")), dict(trim_px=float("nan")),
                    dict(max_drop=-1)):
            with pytest.raises(_native.SbaError, match="status -1"):
                prob.triangulate(**bad)
    assert list(tri.status) == [TRI_TOO_FEW, TRI_TOO_FEW, TRI_DEGENERATE, TRI_BEHIND, TRI_ANCHORED, TRI_OK, TRI_OK, TRI_OK, TRI_TOO_FEW]
    assert np.isnan(tri.points[[0, 1, 2, 8]]).all() and np.isfinite(tri.points[[3, 4, 5, 6, 7]]).all()
    assert np.array_equal(tri.points[4], held[4])
    assert np.abs(tri.points[[3, 5, 6, 7]] - pts[[3, 5, 6, 7]]).max() <= 1e-8
    from test_triangulate_host import _rotation
    depth = (_rotation(cams[:2]) @ tri.points[3] + cams[:2, 3:6])[:, 2]
    assert np.all(depth < 0)
    assert list(tri.n_views) == [0, 0, 0, 2, 0, 2, 2, 3, 0]
    expect_in = np.isin(pi, [3, 4, 5, 6, 7])
    expect_in[k_fold] = False
    assert np.array_equal(tri.inliers, expect_in)
    assert (tri.n_obs_unusable, tri.n_obs_trimmed, tri.n_points_trimmed) == (1, 0, 0)
    assert [tri.n_ok, tri.n_anchored, tri.n_too_few, tri.n_degenerate, tri.n_behind] == [3, 1, 3, 1, 1]
    assert list(tri3.status) == [TRI_TOO_FEW, TRI_TOO_FEW, TRI_TOO_FEW, TRI_TOO_FEW, TRI_ANCHORED, TRI_TOO_FEW, TRI_TOO_FEW, TRI_OK, TRI_TOO_FEW]
    _against_oracle(tri, tri_oracle(cams, uv, ci, pi, 9, fixed=fixed, pts=held), "statuses")
    _against_oracle(tri3, tri_oracle(cams, uv, ci, pi, 9, fixed=fixed, pts=held, min_views=3), "statuses, min_views 3")


# ----------------------------------------------------------------------------- 5. trimming
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("k", range(len(OUTLIER_RIGS)))
def test_trimming_finds_exactly_the_planted_outliers(k, dtype):
    rig = outlier_rig(k)
    uv, bad_obs = plant_outliers(rig)
    if dtype == "f32":
        uv = uv.astype(np.float32).astype(np.float64)
    with _native.Problem(rig["cams_true"], rig["pts0"], uv, rig["camera_ind"], rig["point_ind"], dtype=dtype) as prob:
        tri = prob.triangulate(trim_px=3.0, max_drop=1)
        plain = prob.triangulate()
    o = tri_oracle(rig["cams_true"], uv, rig["camera_ind"], rig["point_ind"], 4000, trim_px=3.0, max_drop=1)
    _against_oracle(tri, o, f"trim {OUTLIER_RIGS[k]} {dtype}")
    assert np.array_equal(np.nonzero(~tri.inliers)[0], np.sort(bad_obs))
    assert tri.n_obs_trimmed == 400 and tri.n_points_trimmed == 400
    assert np.linalg.norm(tri.points - rig["pts_true"], axis=1).max() < 5.0
    assert plain.inliers.all() and plain.n_obs_trimmed == 0
    _against_oracle(plain, tri_oracle(rig["cams_true"], uv, rig["camera_ind"], rig["point_ind"], 4000), "untrimmed")


def test_two_rounds_of_trimming():
    rig = outlier_rig(2)
    uv, bad_obs = plant_outliers(rig)
    uv[bad_obs[:50] + np.where(bad_obs[:50] % 6 == 5, -1, 1)] += 50.0          # a second outlier in 50 of the points (6 views each)
    with _native.Problem(rig["cams_true"], rig["pts0"], uv, rig["camera_ind"], rig["point_ind"]) as prob:
        tri = prob.triangulate(trim_px=3.0, max_drop=2)
    o = tri_oracle(rig["cams_true"], uv, rig["camera_ind"], rig["point_ind"], 4000, trim_px=3.0, max_drop=2)
    _against_oracle(tri, o, "two rounds")
    assert tri.n_obs_trimmed == 450 and tri.n_points_trimmed == 400


# ----------------------------------------------------------------------------- 6. the handle: untouched, or written back
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("C,N", [(16, 400), (64, 600)])
def test_triangulate_leaves_the_handle_as_it_was(C, N, dtype):
    rig = make_rig(C, N, seed=29, visibility=0.6 if C > 16 else 1.0)
    args = (rig["points_2d"], rig["camera_ind"], rig["point_ind"])
    opts = dict(ftol=1e-6, max_iter=6)
    with _native.Problem(rig["cams0"], rig["pts0"], *args, dtype=dtype) as a:
        before = a.get_params()
        a.triangulate()
        a.triangulate(trim_px=0.5, max_drop=2)
        after = a.get_params()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        ca, pa, ra, _ = a.solve_lm(a.make_opts(**opts))
    with _native.Problem(rig["cams0"], rig["pts0"], *args, dtype=dtype) as b:
        cb, pb, rb, _ = b.solve_lm(b.make_opts(**opts))
    assert np.array_equal(ca, cb) and np.array_equal(pa, pb) and ra.cost == rb.cost


def test_multi_rank_handle_is_unsupported():
    rig = make_rig(4, 60, seed=41)
    with _native.Problem(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"]) as prob:
        h = prob.ipc_export(1)
        prob.ipc_attach(0, [h])
        with pytest.raises(_native.SbaError, match="status -6"):
            prob.triangulate()


def test_write_back_starts_the_solve_from_the_triangulated_points(dtype="f64"):
    rig = make_rig(8, 2000, seed=0)
    args = (rig["points_2d"], rig["camera_ind"], rig["point_ind"])
    tight = dict(ftol=1e-12, xtol=1e-12, gtol=1e-12, mode=_native.MODE_POINTS_ONLY, max_nfev=400)
    with _native.Problem(rig["cams_true"], np.zeros((2000, 3)), *args, dtype=dtype) as prob:
        tri = prob.triangulate(write_back=True)
        cams, pts = prob.get_params()
        assert tri.ok.all() and np.array_equal(pts, tri.points) and np.array_equal(cams, rig["cams_true"])
        _c, p_tri, rep_tri, _ = prob.solve_lm(prob.make_opts(**tight))
    with _native.Problem(rig["cams_true"], rig["pts0"], *args, dtype=dtype) as prob:
        _c, p_ref, rep_ref, _ = prob.solve_lm(prob.make_opts(**tight))
    rel = abs(rep_tri.cost - rep_ref.cost) / rep_ref.cost
    print(f"{dtype}: cost from the triangulated start {rep_tri.cost:.12e}, from pts0 {rep_ref.cost:.12e}, rel {rel:.2e}, "
          f"initial cost {rep_tri.initial_cost:.6e}")
    assert rep_tri.status > 0 and rep_ref.status > 0
    assert rel <= 1e-8              # the project's two-sided bar for tight solves (F9)


def test_write_back_keeps_the_points_without_an_ok_estimate():
    cams, pts, held, uv, ci, pi, fixed, _k = _status_problem()
    with _native.Problem(cams, held, uv, ci, pi) as prob:
        prob.set_fixed_points(fixed)
        tri = prob.triangulate(write_back=True)
        _c, now = prob.get_params()
    ok = tri.status == TRI_OK
    assert ok.sum() == 3 and np.array_equal(now[ok], tri.points[ok]) and np.array_equal(now[~ok], held[~ok])


# ----------------------------------------------------------------------------- 7. the Python surface
def test_pysba_triangulate(monkeypatch):
    from lasercalib_amd.pySBA import PySBA
    rig = make_rig(6, 300, seed=9)
    start = np.zeros((300, 3))
    keep = start.copy()
    M = rig["camera_ind"].size
    w = np.ones(M)
    w[::7] = 0.0
    sba = PySBA(rig["cams_true"], start, rig["points_2d"], rig["camera_ind"], rig["point_ind"], pointWeights=w,
                points3Dfixed=np.array([3, 5]))
    tri = sba.triangulate()
    assert sba.points3D is not start and np.array_equal(start, keep)
    assert tri.ok.all() and np.array_equal(sba.points3D, tri.points) and tri.n_obs_unusable == int((w == 0).sum())
    assert np.linalg.norm(tri.points - rig["pts_true"], axis=1).max() < 5.0
    o = tri_oracle(rig["cams_true"], rig["points_2d"], rig["camera_ind"], rig["point_ind"], 300, w=w)
    _against_oracle(tri, o, "PySBA.triangulate")
    monkeypatch.setenv("LASERCALIB_SBA_USE_FIXED", "1")
    sba2 = PySBA(rig["cams_true"], start, rig["points_2d"], rig["camera_ind"], rig["point_ind"], points3Dfixed=np.array([3, 5]))
    tri2 = sba2.triangulate(update=False)
    assert sba2.points3D is start
    assert list(np.nonzero(tri2.status == TRI_ANCHORED)[0]) == [3, 5] and np.array_equal(tri2.points[[3, 5]], start[[3, 5]])
    sba2.triangulate()
    assert np.array_equal(sba2.points3D[[3, 5]], start[[3, 5]]) and np.abs(sba2.points3D[0]).max() > 0


def test_dataset_from_triangulation_feeds_bundle_adjust():
    from lasercalib_amd.pySBA import PySBA
    noise_px = 0.3
    rig = make_rig(17, 2000, visibility=0.45, min_cams_per_point=4, noise_px=noise_px)
    cent = np.full((2000, 2, 17), np.nan)
    cent[rig["point_ind"], :, rig["camera_ind"]] = rig["points_2d"]
    missed = np.isnan(cent[:, 0, 0])
    assert missed.sum() > 500 and not dataset.filter_points(cent, 4, 0)[missed].any()
    assert dataset.filter_points_by_views(cent, 4).all()
    ds = dataset.make_dataset_triangulated(cent, rig["cams0"])
    ref = dataset.make_dataset(cent, rig["pts0"])
    assert set(ds) == set(ref) and ds["n_pts"] == 2000 and ds["n_cams"] == 17             # the frames camera 0 missed are kept
    assert np.array_equal(ds["point_ind"], ref["point_ind"]) and np.array_equal(ds["camera_ind"], ref["camera_ind"])
    assert all(ds[k].dtype == ref[k].dtype for k in ("points_2d", "points_3d", "camera_ind", "point_ind"))
    n_cams, p3, p2, ci, pi = dataset.concatenate_datasets([ds])
    sba = PySBA(rig["cams0"].copy(), p3, p2, ci, pi)
    res = sba.bundleAdjust(1e-4)
    rms = np.sqrt(2.0 * res.cost / (2 * ci.size))
    print(f"bundleAdjust from the triangulated dataset: status {res.status}, rms {rms:.4f} px per component")
    assert res.status > 0 and rms <= noise_px
    # trimming removes the observations it flags from the list
    cent2 = cent.copy()
    first = np.argmax(~np.isnan(cent2[7, 0, :]))
    cent2[7, :, first] += 60.0
    ds2 = dataset.make_dataset_triangulated(cent2, rig["cams_true"], trim_px=3.0)
    assert ds2["n_pts"] == 2000 and ds2["camera_ind"].size == ci.size - 1
    assert not np.any((ds2["point_ind"] == 7) & (ds2["camera_ind"] == first))
