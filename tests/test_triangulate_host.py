"""CPU: the triangulation entry point is declared, exported and bound, and fails loudly without a device; the numpy restatement
of the estimator of include/sba_hip.h (``tri_oracle``, which tests/test_gpu_triangulate.py compares the kernels against) is
checked where geometry makes the truth exact -- noise-free rays meet in the true point -- and on planted outliers, which the
leave-one-out trimming has to find exactly; the pure-numpy half of ``dataset.make_dataset_triangulated`` is covered too.

Nothing here runs a reference triangulation (OpenCV is not a dependency): the oracle is the specification, written a second
time in another language and another summation order."""
import ctypes
import os
import re

import numpy as np
import pytest

from lasercalib_amd import _native, dataset
from lasercalib_amd.synth import make_rig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TRI_OK, TRI_ANCHORED, TRI_TOO_FEW, TRI_DEGENERATE, TRI_BEHIND = 0, 1, 2, 3, 4


# ----------------------------------------------------------------------------- numpy oracle (also used by the GPU tests)
def _rotation(cams):
    """(C, 3, 3) Rodrigues matrices of the camera rows; the series branch of sba_model.hpp below theta^2 = 1e-4."""
    r = cams[:, 0:3]
    th2 = np.sum(r * r, axis=1)
    small = th2 < 1e-4
    th = np.sqrt(np.where(small, 1.0, th2))
    c = np.where(small, 1.0 - th2 * (0.5 - th2 * (1.0 / 24 - th2 / 720)), np.cos(th))
    a = np.where(small, 1.0 - th2 * (1.0 / 6 - th2 * (1.0 / 120 - th2 / 5040)), np.sin(th) / th)
    b = np.where(small, 0.5 - th2 * (1.0 / 24 - th2 * (1.0 / 720 - th2 / 40320)), (1.0 - np.cos(th)) / np.where(small, 1.0, th2))
    K = np.zeros((cams.shape[0], 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -r[:, 2], r[:, 1], r[:, 2], -r[:, 0], -r[:, 1], r[:, 0]
    return c[:, None, None] * np.eye(3) + a[:, None, None] * K + b[:, None, None] * r[:, :, None] * r[:, None, :]


def _distort(rows, x, y):
    """Forward distortion of sba_model.hpp and its 2 x 2 Jacobian (gxx, gxy, gyy; symmetric)."""
    k1, k2 = rows[:, 7], rows[:, 8]
    n = x * x + y * y
    d = 1.0 + n * (k1 + k2 * n)
    dn = k1 + 2.0 * k2 * n
    fx, fy = x * d, y * d
    gxx, gxy, gyy = d + 2 * x * x * dn, 2 * x * y * dn, d + 2 * y * y * dn
    if rows.shape[1] == 13:
        p1, p2 = rows[:, 9], rows[:, 10]
        fx = fx + 2 * p1 * x * y + p2 * (n + 2 * x * x)
        fy = fy + p1 * (n + 2 * y * y) + 2 * p2 * x * y
        gxx = gxx + 2 * p1 * y + 6 * p2 * x
        gxy = gxy + 2 * (p1 * x + p2 * y)
        gyy = gyy + 6 * p1 * y + 2 * p2 * x
    return fx, fy, gxx, gxy, gyy


def _undistort(rows, xd, yd):
    """Newton inversion of the distortion from (xd, yd); returns x, y, converged."""
    x, y = xd.copy(), yd.copy()
    M = x.shape[0]
    active, ok = np.ones(M, bool), np.zeros(M, bool)
    with np.errstate(all="ignore"):
        for _ in range(20):
            idx = np.nonzero(active)[0]
            if idx.size == 0:
                break
            fx, fy, gxx, gxy, gyy = _distort(rows[idx], x[idx], y[idx])
            ex, ey = fx - xd[idx], fy - yd[idx]
            det = gxx * gyy - gxy * gxy
            sx, sy = (gyy * ex - gxy * ey) / det, (gxx * ey - gxy * ex) / det
            nx, ny = x[idx] - sx, y[idx] - sy
            bad = ~(det > 0) | ~np.isfinite(nx) | ~np.isfinite(ny)
            done = ~bad & (np.maximum(np.abs(sx), np.abs(sy)) <= 1e-15 * np.maximum(1.0, np.maximum(np.abs(nx), np.abs(ny))))
            x[idx], y[idx] = nx, ny
            ok[idx[done]] = True
            active[idx[bad | done]] = False
    return x, y, ok


def _project(rows, R, X):
    """Pixels (M, 2) and depths (M,) of X (M, 3) through camera rows (M, P) with rotations R (M, 3, 3)."""
    with np.errstate(all="ignore"):
        p = np.einsum("mij,mj->mi", R, X) + rows[:, 3:6]
        x, y = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
        fx, fy, _a, _b, _c = _distort(rows, x, y)
        P = rows.shape[1]
        return np.stack([rows[:, 6] * fx + rows[:, P - 2], rows[:, 6] * fy + rows[:, P - 1]], 1), p[:, 2]


def _chol_solve(A, b):
    """X = A^-1 b for stacks of symmetric 3 x 3 systems with the pivot test of k_cov_lin; returns X, ok."""
    with np.errstate(all="ignore"):
        a00, a10, a11, a20, a21, a22 = A[:, 0, 0], A[:, 1, 0], A[:, 1, 1], A[:, 2, 0], A[:, 2, 1], A[:, 2, 2]
        l00 = np.sqrt(a00)
        l10, l20 = a10 / l00, a20 / l00
        d1 = a11 - l10 * l10
        l11 = np.sqrt(d1)
        l21 = (a21 - l20 * l10) / l11
        d2 = a22 - l20 * l20 - l21 * l21
        l22 = np.sqrt(d2)
        ok = (a00 > 0) & (d1 > 1e-12 * a11) & (d2 > 1e-12 * a22) & np.isfinite(l22)
        y0 = b[:, 0] / l00
        y1 = (b[:, 1] - l10 * y0) / l11
        y2 = (b[:, 2] - l20 * y0 - l21 * y1) / l22
        x2 = y2 / l22
        x1 = (y1 - l21 * x2) / l11
        x0 = (y0 - l10 * x1 - l20 * x2) / l00
        X = np.stack([x0, x1, x2], 1)
        ok &= np.all(np.isfinite(X), axis=1)
    return np.where(ok[:, None], X, np.nan), ok


def tri_oracle(cams, uv, ci, pi, N, w=None, fixed=None, min_views=2, trim_px=None, max_drop=1, pts=None):
    """The estimator of sba_triangulate (include/sba_hip.h) in numpy float64.  ``pts``: the held coordinates, needed only with
    ``fixed``.  Returns a dict: points (N, 3), status, n_views, rms_px, max_px, spread, inliers (M,) bool in the caller's order,
    n_obs_unusable, n_obs_trimmed, n_points_trimmed."""
    cams, uv = np.asarray(cams, np.float64), np.asarray(uv, np.float64)
    ci, pi = np.asarray(ci, np.int64), np.asarray(pi, np.int64)
    M, P = ci.shape[0], cams.shape[1]
    w = np.ones(M) if w is None else np.asarray(w, np.float64)
    fixed = np.zeros(N, bool) if fixed is None else np.asarray(fixed).astype(bool)
    trim = float(trim_px) if trim_px else 0.0
    Rc = _rotation(cams)
    centre = -np.einsum("cji,cj->ci", Rc, cams[:, 3:6])
    rows = cams[ci]
    xd, yd = (uv[:, 0] - rows[:, P - 2]) / rows[:, 6], (uv[:, 1] - rows[:, P - 1]) / rows[:, 6]
    x, y, conv = _undistort(rows, xd, yd)
    usable = conv & (w != 0) & np.isfinite(w)
    v = np.einsum("mji,mj->mi", Rc[ci], np.stack([x, y, np.ones(M)], 1))
    with np.errstate(all="ignore"):
        d = v / np.linalg.norm(v, axis=1)[:, None]
    usable &= np.all(np.isfinite(d), axis=1)
    d = np.where(usable[:, None], d, 0.0)
    om = np.where(usable, w * w, 0.0)
    Pm = om[:, None, None] * (np.eye(3) - d[:, :, None] * d[:, None, :])
    Pc = np.einsum("mij,mj->mi", Pm, centre[ci])
    A, b, dsum = np.zeros((N, 3, 3)), np.zeros((N, 3)), np.zeros((N, 3))
    np.add.at(A, pi, Pm)
    np.add.at(b, pi, Pc)
    np.add.at(dsum, pi[usable], d[usable])
    nuse = np.bincount(pi[usable], minlength=N)
    pairs = np.unique(np.stack([pi[usable], ci[usable]], 1), axis=0)
    ncam = np.bincount(pairs[:, 0], minlength=N)
    X, ok = _chol_solve(A, b)
    status = np.where(fixed, TRI_ANCHORED, np.where(ncam < min_views, TRI_TOO_FEW, np.where(ok, TRI_OK, TRI_DEGENERATE)))
    have = status == TRI_OK
    X = np.where(have[:, None], X, np.nan)
    used = usable & have[pi]
    # per-observation error and depth at the estimate
    e, z = np.full(M, np.nan), np.full(M, np.nan)
    px, zz = _project(rows[used], Rc[ci[used]], X[pi[used]])
    e[used], z[used] = np.linalg.norm(px - uv[used], axis=1), zz
    n_trimmed_pts = 0
    trimmed = np.zeros(M, bool)
    if trim > 0:
        order = np.lexsort((np.arange(M), ci, pi))               # point-major, camera-minor: the layout's order
        start = np.searchsorted(pi[order], np.arange(N + 1))
        emax = np.full(N, -np.inf)
        np.maximum.at(emax, pi[used], np.where(np.isnan(e[used]), np.inf, e[used]))
        for p in np.nonzero(have & (emax > trim))[0]:
            obs = order[start[p]:start[p + 1]]
            obs = obs[used[obs]]
            Ap, bp, dropped = A[p].copy(), b[p].copy(), False
            for _round in range(max_drop):
                ecur = np.where(np.isnan(e[obs]), np.inf, e[obs])
                if not (ecur.max() > trim and obs.size > max(min_views, 3)):
                    break
                Aj, bj = Ap[None] - Pm[obs], bp[None] - Pc[obs]
                Xj, okj = _chol_solve(Aj, bj)
                m = np.full(obs.size, np.inf)
                for k in np.nonzero(okj)[0]:
                    others = np.delete(obs, k)
                    pxk, _z = _project(rows[others], Rc[ci[others]], np.repeat(Xj[k][None], others.size, 0))
                    mk = np.linalg.norm(pxk - uv[others], axis=1).max()
                    m[k] = mk if np.isfinite(mk) else np.inf
                if not np.isfinite(m.min()):
                    break
                k = int(np.argmin(m))                             # first minimum = the earlier position
                trimmed[obs[k]], used[obs[k]] = True, False
                Ap, bp, X[p] = Aj[k], bj[k], Xj[k]
                dsum[p] -= d[obs[k]]
                nuse[p] -= 1
                obs, dropped = np.delete(obs, k), True
                pxk, zk = _project(rows[obs], Rc[ci[obs]], np.repeat(X[p][None], obs.size, 0))
                e[obs], z[obs] = np.linalg.norm(pxk - uv[obs], axis=1), zk
            n_trimmed_pts += dropped
    n_views = np.where(have, nuse, 0).astype(np.int32)
    sq, mx, zmin = np.zeros(N), np.zeros(N), np.full(N, np.inf)
    np.add.at(sq, pi[used], e[used] ** 2)
    np.maximum.at(mx, pi[used], e[used])
    np.minimum.at(zmin, pi[used], z[used])
    nan_e = np.zeros(N, bool)
    np.logical_or.at(nan_e, pi[used], np.isnan(e[used]))
    mx[nan_e] = np.nan
    with np.errstate(all="ignore"):
        rms = np.sqrt(sq / n_views)
        mean_d = dsum / nuse[:, None]
        spread = 1.0 - np.sum(mean_d * mean_d, axis=1)
    status = np.where(have & (zmin <= 0), TRI_BEHIND, status).astype(np.int32)
    out_pts = X.copy()
    if fixed.any():
        out_pts[fixed] = np.asarray(pts, np.float64)[fixed]
    nan = ~have
    rms[nan], mx[nan], spread[nan] = np.nan, np.nan, np.nan
    return dict(points=out_pts, status=status, n_views=n_views, rms_px=rms, max_px=mx, spread=spread,
                inliers=used | fixed[pi], n_obs_unusable=int(np.sum(~usable & ~fixed[pi])), n_obs_trimmed=int(trimmed.sum()),
                n_points_trimmed=int(n_trimmed_pts))


def plant_outliers(rig):
    """One 40-80 px outlier in every tenth point (the draws of the issue, in its order); returns uv and the planted indices."""
    N = rig["n_points"]
    pi = rig["point_ind"]
    start = np.searchsorted(pi, np.arange(N))
    deg = np.bincount(pi, minlength=N)
    uv = rig["points_2d"].copy()
    rng = np.random.default_rng(11)
    bad_pts = np.arange(0, N, 10)
    bad_obs = start[bad_pts] + rng.integers(0, deg[bad_pts])
    ang = rng.uniform(0, 2 * np.pi, bad_obs.size)
    mag = rng.uniform(40, 80, bad_obs.size)
    uv[bad_obs] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1)
    return uv, bad_obs


OUTLIER_RIGS = [dict(n_cams=17, seed=3, visibility=0.45), dict(n_cams=17, seed=5, visibility=0.3), dict(n_cams=6, seed=7, visibility=1.0)]


def outlier_rig(k):
    return make_rig(n_points=4000, noise_px=0.3, min_cams_per_point=4, **OUTLIER_RIGS[k])


# ----------------------------------------------------------------------------- 1. declared, exported, bound, loud without a device
def _header():
    return open(os.path.join(ROOT, "include", "sba_hip.h")).read()


def test_triangulate_is_declared_exported_and_bound():
    assert re.search(r"\bint sba_triangulate\(sba_handle\* h, const sba_tri_opts\* opts", _header())
    assert "sba_triangulate" in _native.EXPORTED_SYMBOLS
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _native.load()
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "sba_triangulate")
    assert lib.sba_triangulate.argtypes is not None and len(lib.sba_triangulate.argtypes) == 10
    assert lib.sba_abi_version() == 2
    assert callable(_native.Problem.triangulate)


def test_struct_sizes_match_the_header():
    # sba_tri_opts: int32 x 2, double, int32 x 6 -> 4 + 4 + 8 + 24 = 40;  sba_tri_report: int64 x 8 + double x 4 = 96
    assert ctypes.sizeof(_native.TriOpts) == 40
    assert ctypes.sizeof(_native.TriReport) == 96
    text = _header()
    opts = re.search(r"typedef struct \{([^}]*)\} sba_tri_opts;", text).group(1)
    assert [t for t in re.findall(r"\b(int32_t|double|int64_t)\b", re.sub(r"/\*.*?\*/", "", opts, flags=re.S))] == \
        ["int32_t", "int32_t", "double", "int32_t", "int32_t"]
    assert [n for n, _t in _native.TriOpts._fields_] == ["min_views", "max_drop", "trim_px", "write_back", "reserved"]
    rep = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} sba_tri_report;", text).group(1), flags=re.S)
    names = re.findall(r"\b(n_[a-z_]+|seconds_[a-z]+)\b", rep)
    assert names == [n for n, _t in _native.TriReport._fields_]
    for code, name in enumerate(("OK", "ANCHORED", "TOO_FEW", "DEGENERATE", "BEHIND")):
        assert re.search(rf"\bSBA_TRI_{name} = {code}\b", text)
        assert getattr(_native, f"TRI_{name}") == code


def test_no_gpu_means_loud_failure():
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    if _native.load().sba_device_count() > 0:
        pytest.skip("a GPU is visible; the no-device path is exercised on the CPU-only container")
    from lasercalib_amd.pySBA import PySBA
    rig = make_rig(2, 20)
    with pytest.raises(_native.SbaError, match="no HIP device"):
        _native.Problem(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"]).triangulate()
    sba = PySBA(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"])
    with pytest.raises(_native.SbaError, match="no HIP device"):
        sba.triangulate()


# ----------------------------------------------------------------------------- 2. the oracle against exact geometry
@pytest.mark.parametrize("tangential", [False, True])
@pytest.mark.parametrize("visibility", [1.0, 0.45])
def test_oracle_meets_the_truth_on_noise_free_rays(visibility, tangential):
    rig = make_rig(17, 4000, seed=3, noise_px=0.0, visibility=visibility, tangential=tangential)
    o = tri_oracle(rig["cams_true"], rig["points_2d"], rig["camera_ind"], rig["point_ind"], 4000)
    err = np.abs(o["points"] - rig["pts_true"]).max()
    print(f"visibility {visibility} tangential {tangential}: max |X - truth| = {err:.3e} mm, max_px {np.nanmax(o['max_px']):.3e}")
    assert np.all(o["status"] == TRI_OK) and o["inliers"].all() and o["n_obs_unusable"] == 0
    assert np.array_equal(o["n_views"], np.bincount(rig["point_ind"], minlength=4000))
    assert err <= 1e-9
    assert np.all(o["spread"] > 0) and np.all(o["spread"] < 1)


def test_oracle_statuses_on_a_hand_built_problem():
    rig = make_rig(4, 6, seed=1, noise_px=0.0)
    cams = rig["cams_true"]
    uv_all = rig["points_2d"].reshape(6, 4, 2)
    ci = np.array([0, 0, 0, 0, 1, 2, 0, 1, 2, 3])                # point 0: one view; 1: one camera twice; 2, 3: three / four views
    pi = np.array([0, 1, 1, 2, 2, 2, 3, 3, 3, 3])
    uv = np.stack([uv_all[p, c] for p, c in zip(pi, ci)])
    w = np.ones(10)
    w[9] = 0.0
    o = tri_oracle(cams, uv, ci, pi, 6, w=w, fixed=np.arange(6) == 5, pts=rig["pts_true"])
    assert list(o["status"]) == [TRI_TOO_FEW, TRI_TOO_FEW, TRI_OK, TRI_OK, TRI_TOO_FEW, TRI_ANCHORED]
    assert np.isnan(o["points"][[0, 1, 4]]).all() and np.array_equal(o["points"][5], rig["pts_true"][5])
    assert np.abs(o["points"][[2, 3]] - rig["pts_true"][[2, 3]]).max() < 1e-9
    assert list(o["n_views"]) == [0, 0, 3, 3, 0, 0] and o["n_obs_unusable"] == 1
    assert list(o["inliers"]) == [False, False, False, True, True, True, True, True, True, False]
    assert list(tri_oracle(cams, uv, ci, pi, 6, w=w, min_views=4)["status"][[2, 3]]) == [TRI_TOO_FEW, TRI_TOO_FEW]


# ----------------------------------------------------------------------------- 3. trimming finds the planted outliers exactly
@pytest.mark.parametrize("k", range(len(OUTLIER_RIGS)))
def test_trimming_finds_exactly_the_planted_outliers(k):
    rig = outlier_rig(k)
    uv, bad_obs = plant_outliers(rig)
    assert bad_obs.size == 400
    o = tri_oracle(rig["cams_true"], uv, rig["camera_ind"], rig["point_ind"], 4000, trim_px=3.0, max_drop=1)
    flagged = np.nonzero(~o["inliers"])[0]
    err = np.linalg.norm(o["points"] - rig["pts_true"], axis=1).max()
    print(f"rig {OUTLIER_RIGS[k]}: {flagged.size} flagged, {np.intersect1d(flagged, bad_obs).size} of 400 planted, "
          f"largest point error {err:.3f} mm")
    assert np.array_equal(flagged, np.sort(bad_obs))
    assert o["n_obs_trimmed"] == 400 and o["n_points_trimmed"] == 400 and o["n_obs_unusable"] == 0
    assert err < 5.0


# ----------------------------------------------------------------------------- 4. the numpy half of the dataset builder
def _centroids():
    c = np.full((5, 2, 3), np.nan)
    seen = {0: (0, 1, 2), 1: (1, 2), 2: (0,), 3: (0, 2), 4: (1, 2)}      # frames 1 and 4: not seen by camera 0
    for i, cs in seen.items():
        for j in cs:
            c[i, :, j] = (100.0 * i + j, 50.0 * i + j)
    return c


def test_filter_points_by_views_keeps_frames_the_init_camera_missed():
    c = _centroids()
    assert list(dataset.filter_points(c, 2, 0)) == [True, False, False, True, False]
    assert list(dataset.filter_points_by_views(c, 2)) == [True, True, False, True, True]
    assert list(dataset.filter_points_by_views(c, 3)) == [True, False, False, False, False]


def test_reindex_drops_points_and_observations():
    c = _centroids()
    ci, pi, uv = dataset.observation_list(c)
    assert ci.size == 10
    keep_pts = np.array([True, True, False, False, True])
    keep_obs = np.ones(10, bool)
    keep_obs[1] = False                                            # (frame 0, camera 1): a trimmed observation
    X = np.arange(15.0).reshape(5, 3)
    out = dataset.reindex_dataset(3, X, uv, ci, pi, keep_pts, keep_obs)
    assert out["n_cams"] == 3 and out["n_pts"] == 3
    assert np.array_equal(out["points_3d"], X[[0, 1, 4]])
    assert list(out["point_ind"]) == [0, 0, 1, 1, 2, 2] and list(out["camera_ind"]) == [0, 2, 1, 2, 1, 2]
    assert np.array_equal(out["points_2d"], uv[[0, 2, 3, 4, 8, 9]])
    assert out["point_ind"].dtype == np.int64 and out["camera_ind"].dtype == np.int64
    assert out["points_2d"].dtype == np.float64 and out["points_3d"].dtype == np.float64
    ref = dataset.make_dataset(c, X)
    assert set(out) == set(ref) and all(type(out[k]) is type(ref[k]) for k in ref)
    assert dataset.is_point_major(out["point_ind"])
