"""CPU: the two un-projection entry points are declared, exported and bound, and fail loudly without a device; the numpy
restatement of the estimator of include/sba_hip.h (``unproject_oracle``, which tests/test_gpu_unproject.py compares the kernels
against) is checked where geometry makes the truth exact -- the noise-free rays of a point meet its plane in the true point --
against the reference's own algebra for one view and a z-plane (rigid_body.py:229-242, restated), and on a hand-built problem
that reaches every status; the pure-numpy half of ``dataset.make_dataset_unprojected`` is covered too.

The camera model pieces (``_rotation``, ``_distort``, ``_undistort``, ``_project``) are the ones of tests/test_triangulate_host.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lasercalib_amd import _native, dataset  # noqa: E402
from lasercalib_amd.synth import _project_np, make_rig  # noqa: E402
from test_triangulate_host import _project, _rotation, _undistort  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

UNP_OK, UNP_ANCHORED, UNP_NO_VIEW, UNP_DEGENERATE, UNP_BEHIND = 0, 1, 2, 3, 4
ROW_OK, ROW_UNUSABLE, ROW_PARALLEL, ROW_BEHIND = 0, 1, 2, 3

# the rigs of tests/test_gpu_triangulate.py: every layout the kernel reads
RIGS = [
    dict(n_cams=16, n_points=2000, seed=0),
    dict(n_cams=16, n_points=2000, seed=4, visibility=0.6),
    dict(n_cams=17, n_points=3000, seed=3, visibility=0.45),
    dict(n_cams=64, n_points=3000, seed=2, visibility=0.1),
    dict(n_cams=2, n_points=500, seed=1),
    dict(n_cams=6, n_points=3000, seed=7),
    dict(n_cams=17, n_points=2000, seed=3, visibility=0.45, tangential=True),
]
RIG_IDS = ["16x2000", "16x2000 vis 0.6", "17x3000 vis 0.45", "64x3000 vis 0.1", "2x500", "6x3000", "17x2000 vis 0.45 13 columns"]


# ----------------------------------------------------------------------------- numpy oracle (also used by the GPU tests)
def rays_oracle(rows, uv):
    """Per gathered row: undistorted (x, y), converged, R (M, 3, 3), origin -R^T t and unit direction (not yet masked)."""
    rows, uv = np.asarray(rows, np.float64), np.asarray(uv, np.float64)
    M, P = rows.shape
    R = _rotation(rows)
    origin = -np.einsum("mji,mj->mi", R, rows[:, 3:6])
    xd, yd = (uv[:, 0] - rows[:, P - 2]) / rows[:, 6], (uv[:, 1] - rows[:, P - 1]) / rows[:, 6]
    x, y, conv = _undistort(rows, xd, yd)
    v = np.einsum("mji,mj->mi", R, np.stack([x, y, np.ones(M)], 1))
    with np.errstate(all="ignore"):
        d = v / np.linalg.norm(v, axis=1)[:, None]
    return x, y, conv, R, origin, d


def _unit_planes(planes, n):
    pl = np.asarray(planes, np.float64).reshape(-1, 4)
    pl = np.broadcast_to(pl, (n, 4)) if pl.shape[0] == 1 else pl
    nn = np.sqrt(pl[:, 0] * pl[:, 0] + pl[:, 1] * pl[:, 1] + pl[:, 2] * pl[:, 2])
    return pl[:, :3] / nn[:, None], pl[:, 3] / nn


def rows_oracle(uv, rows, planes=None):
    """sba_unproject_rows (include/sba_hip.h) in numpy float64: dict xn, origin, dir, status and with planes points, depth."""
    x, y, conv, R, origin, d = rays_oracle(rows, uv)
    M = x.shape[0]
    ok = conv & np.all(np.isfinite(d), axis=1) & np.all(np.isfinite(origin), axis=1)
    status = np.where(ok, ROW_OK, ROW_UNUSABLE).astype(np.int32)
    out = dict(xn=np.stack([x, y], 1), origin=origin.copy(), dir=d.copy())
    if planes is not None:
        nh, dh = _unit_planes(planes, M)
        with np.errstate(all="ignore"):
            s = np.sum(nh * d, axis=1)
            tau = (dh - np.sum(nh * origin, axis=1)) / s
            X = origin + tau[:, None] * d
            z = np.einsum("mj,mj->m", R[:, 2, :], X) + np.asarray(rows)[:, 5]
        par = ok & (np.abs(s) <= 1e-6)
        bad = ok & ~par & ~(np.all(np.isfinite(X), axis=1) & np.isfinite(z))
        status[par] = ROW_PARALLEL
        status[bad] = ROW_UNUSABLE
        status[(status == ROW_OK) & (z <= 0)] = ROW_BEHIND
        X[(status == ROW_UNUSABLE) | par], z[(status == ROW_UNUSABLE) | par] = np.nan, np.nan
        out.update(points=X, depth=z)
    un = status == ROW_UNUSABLE
    out["xn"][un], out["origin"][un], out["dir"][un] = np.nan, np.nan, np.nan
    out["status"] = status
    return out


def unproject_oracle(cams, uv, ci, pi, N, planes, w=None, fixed=None, ref_cam=None, min_views=1, pts=None):
    """The estimator of sba_unproject (include/sba_hip.h) in numpy float64.  ``pts``: the held coordinates, needed only with
    ``fixed``.  Returns a dict: points (N, 3), status, n_views, rms_px, max_px, used (M,) bool in the caller's order,
    n_obs_unusable, n_obs_used."""
    cams, uv = np.asarray(cams, np.float64), np.asarray(uv, np.float64)
    ci, pi = np.asarray(ci, np.int64), np.asarray(pi, np.int64)
    M = ci.shape[0]
    w = np.ones(M) if w is None else np.asarray(w, np.float64)
    fixed = np.zeros(N, bool) if fixed is None else np.asarray(fixed).astype(bool)
    min_views = max(int(min_views), 1)
    rows = cams[ci]
    _x, _y, conv, R, centre, d = rays_oracle(rows, uv)
    examined = np.ones(M, bool) if ref_cam is None else ci == ref_cam
    usable = examined & conv & (w != 0) & np.isfinite(w) & np.all(np.isfinite(d), axis=1)
    d = np.where(usable[:, None], d, 0.0)
    om = np.where(usable, w * w, 0.0)
    Pm = om[:, None, None] * (np.eye(3) - d[:, :, None] * d[:, None, :])
    Pc = np.einsum("mij,mj->mi", Pm, centre)
    A, b = np.zeros((N, 3, 3)), np.zeros((N, 3))
    np.add.at(A, pi, Pm)
    np.add.at(b, pi, Pc)
    nuse = np.bincount(pi[usable], minlength=N)
    pairs = np.unique(np.stack([pi[usable], ci[usable]], 1), axis=0)
    ncam = np.bincount(pairs[:, 0], minlength=N)
    # the plane's basis and the 2 x 2 system
    nh, dh = _unit_planes(planes, N)
    X0 = dh[:, None] * nh
    k = np.argmin(np.abs(nh), axis=1)                                  # first minimum = the smaller index
    e1 = np.eye(3)[k] - nh[np.arange(N), k][:, None] * nh
    e1 = e1 / np.sqrt(np.sum(e1 * e1, axis=1))[:, None]
    e2 = np.cross(nh, e1)
    Ae1, Ae2 = np.einsum("nij,nj->ni", A, e1), np.einsum("nij,nj->ni", A, e2)
    r = b - np.einsum("nij,nj->ni", A, X0)
    G00, G10, G11 = np.sum(e1 * Ae1, 1), np.sum(e2 * Ae1, 1), np.sum(e2 * Ae2, 1)
    g0, g1 = np.sum(e1 * r, 1), np.sum(e2 * r, 1)
    with np.errstate(all="ignore"):
        l00 = np.sqrt(G00)
        l10 = G10 / l00
        pv = G11 - l10 * l10
        l11 = np.sqrt(pv)
        ok = (G00 > 0) & (pv > 1e-12 * G11) & np.isfinite(l11)
        w0 = g0 / l00
        w1 = (g1 - l10 * w0) / l11
        y1 = w1 / l11
        y0 = (w0 - l10 * y1) / l00
        X = X0 + e1 * y0[:, None] + e2 * y1[:, None]
        ok &= np.all(np.isfinite(X), axis=1)
    status = np.where(fixed, UNP_ANCHORED, np.where(ncam < min_views, UNP_NO_VIEW, np.where(ok, UNP_OK, UNP_DEGENERATE)))
    have = status == UNP_OK
    X = np.where(have[:, None], X, np.nan)
    used = usable & have[pi]
    e, z = np.full(M, np.nan), np.full(M, np.nan)
    px, zz = _project(rows[used], R[used], X[pi[used]])
    e[used], z[used] = np.linalg.norm(px - uv[used], axis=1), zz
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
    status = np.where(have & (zmin <= 0), UNP_BEHIND, status).astype(np.int32)
    out_pts = X.copy()
    if fixed.any():
        out_pts[fixed] = np.asarray(pts, np.float64)[fixed]
    rms[~have], mx[~have] = np.nan, np.nan
    used_out = used | fixed[pi]
    return dict(points=out_pts, status=status, n_views=n_views, rms_px=rms, max_px=mx, used=used_out,
                n_obs_unusable=int(np.sum(examined & ~usable & ~fixed[pi])), n_obs_used=int(used_out.sum()))


def z_planes_of(pts):
    """The plane z = pts[:, 2] of every point, as (N, 4) rows."""
    return _native.z_planes(pts[:, 2], pts.shape[0])


def tilted_planes(pts):
    """A tilted plane through every point: normal (a, b, 1) s with a, b ~ U(-0.15, 0.15), s ~ U(0.5, 4) from default_rng(5)."""
    rng = np.random.default_rng(5)
    N = pts.shape[0]
    a, b, s = rng.uniform(-0.15, 0.15, N), rng.uniform(-0.15, 0.15, N), rng.uniform(0.5, 4.0, N)
    n = np.stack([a, b, np.ones(N)], 1) * s[:, None]
    return np.hstack([n, np.sum(n * pts, axis=1)[:, None]])


def min_plane_incidence(rig, planes):
    """min |nh . d| over the observations of a noise-free rig (d from the true geometry)."""
    cams, ci, pi = rig["cams_true"], rig["camera_ind"], rig["point_ind"]
    centre = -np.einsum("cji,cj->ci", _rotation(cams), cams[:, 3:6])
    d = rig["pts_true"][pi] - centre[ci]
    d /= np.linalg.norm(d, axis=1)[:, None]
    nh, _dh = _unit_planes(planes, rig["n_points"])
    return float(np.abs(np.sum(nh[pi] * d, axis=1)).min())


def status_problem():
    """Eight points that reach every status: cams (5 rows: four pinhole cameras and camera 0 again with k1 = -0.5), the true and
    the held points, uv, ci, pi, weights, the anchor mask, the planes and the expected statuses for min_views 1 and 2."""
    rig = make_rig(4, 8, seed=1, noise_px=0.0)
    cams = rig["cams_true"].copy()
    cams[:, 7:9] = 0.0                                   # pinhole cameras: the image of a point on any plane is exact
    fold = cams[0].copy()
    fold[7], fold[8] = -0.5, 0.0                         # r (1 + k1 r^2) peaks at 0.544 for r = 0.816: radius 0.6 has no pre-image
    cams = np.vstack([cams, fold])
    pts = rig["pts_true"].copy()
    obs = [(0, 0), (0, 1), (0, 2),                       # 0: three views                                  OK
           (1, 0), (1, 1),                               # 1: anchored                                     ANCHORED
           (2, 3),                                       # 2: its only observation has weight 0            NO_VIEW
           (3, 0), (3, 0),                               # 3: two pixels of one camera                     OK / NO_VIEW for min_views 2
           (4, 0),                                       # 4: the plane contains the ray                   DEGENERATE
           (5, 0),                                       # 5: the plane lies behind the camera             BEHIND
           (6, 1), (6, 4),                               # 6: one good view, one pixel in the folded-back region   OK, 1 unusable
           (7, 0), (7, 1), (7, 2), (7, 3)]               # 7: four views, a tilted plane                   OK
    pi = np.array([p for p, _c in obs])
    ci = np.array([c for _p, c in obs])
    uv = _project_np(pts[pi], cams[ci])
    k_fold = obs.index((6, 4))
    uv[k_fold] = (fold[9] + fold[6] * 0.6, fold[10])
    w = np.ones(len(obs))
    w[obs.index((2, 3))] = 0.0
    planes = z_planes_of(pts)
    centre0 = -_rotation(cams[:1])[0].T @ cams[0, 3:6]
    ray = pts[4] - centre0
    n4 = np.cross(ray, [0.0, 0.0, 1.0])
    planes[4] = (*n4, n4 @ centre0)                      # through the centre of camera 0, containing the ray to point 4
    planes[5] = (0.0, 0.0, 1.0, 2000.0)                  # above the cameras (they look down from z = 1200)
    planes[7] = tilted_planes(pts)[7]
    held = pts + 7.0
    fixed = np.arange(8) == 1
    expect1 = [UNP_OK, UNP_ANCHORED, UNP_NO_VIEW, UNP_OK, UNP_DEGENERATE, UNP_BEHIND, UNP_OK, UNP_OK]
    expect2 = [UNP_OK, UNP_ANCHORED, UNP_NO_VIEW, UNP_NO_VIEW, UNP_NO_VIEW, UNP_NO_VIEW, UNP_NO_VIEW, UNP_OK]
    return dict(cams=cams, pts=pts, held=held, uv=uv, ci=ci, pi=pi, w=w, fixed=fixed, planes=planes, k_fold=k_fold,
                expect1=expect1, expect2=expect2)


def check_status_result(sp, res, min_views):
    """What both the oracle and the device have to return on ``status_problem`` (``res``: anything with the result's fields)."""
    get = (lambda k: res[k]) if isinstance(res, dict) else (lambda k: getattr(res, k))
    status, X, used, pi = get("status"), get("points"), get("used"), sp["pi"]
    assert list(status) == (sp["expect1"] if min_views == 1 else sp["expect2"])
    est = np.isin(status, [UNP_OK, UNP_BEHIND])
    assert np.isnan(X[~est & (status != UNP_ANCHORED)]).all() and np.isfinite(X[est]).all()
    assert np.array_equal(X[1], sp["held"][1])
    on_truth = status == UNP_OK
    assert np.abs(X[on_truth] - sp["pts"][on_truth]).max() <= 1e-8
    assert np.isnan(get("rms_px")[~est]).all() and np.all(get("n_views")[~est] == 0)
    expect_used = (est | (status == UNP_ANCHORED))[pi] & (sp["w"] != 0)
    expect_used[sp["k_fold"]] = False
    assert np.array_equal(used, expect_used)
    assert get("n_obs_unusable") == 2 and get("n_obs_used") == int(expect_used.sum())
    if min_views == 1:
        assert list(get("n_views")) == [3, 0, 0, 2, 0, 1, 1, 4]
        assert np.isfinite(X[5]).all() and abs(X[5, 2] - 2000.0) <= 1e-8
        depth = (_rotation(sp["cams"][:1])[0] @ X[5] + sp["cams"][0, 3:6])[2]
        assert depth < 0


# ----------------------------------------------------------------------------- 1. declared, exported, bound, loud without a device
def _header():
    return open(os.path.join(ROOT, "include", "sba_hip.h")).read()


def _built():
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _native.load()


def test_unproject_is_declared_exported_and_bound():
    text = _header()
    assert re.search(r"\bint sba_unproject_rows\(int device, int cam_model, int64_t n, const double\* uv", text)
    assert re.search(r"\bint sba_unproject\(sba_handle\* h, const sba_unp_opts\* opts", text)
    assert "sba_unproject_rows" in _native.EXPORTED_SYMBOLS and "sba_unproject" in _native.EXPORTED_SYMBOLS
    lib = _built()
    raw = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(raw, "sba_unproject_rows") and hasattr(raw, "sba_unproject")
    assert len(lib.sba_unproject_rows.argtypes) == 13 and len(lib.sba_unproject.argtypes) == 11
    assert lib.sba_abi_version() == 2
    assert callable(_native.Problem.unproject) and callable(_native.unproject_rows)


def test_struct_sizes_match_the_header():
    assert ctypes.sizeof(_native.UnpOpts) == 32
    assert ctypes.sizeof(_native.UnpReport) == 72
    text = _header()
    opts = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} sba_unp_opts;", text).group(1), flags=re.S)
    assert re.findall(r"\b(use_ref_cam|ref_cam|min_views|write_back|reserved)\b", opts) == [n for n, _t in _native.UnpOpts._fields_]
    rep = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} sba_unp_report;", text).group(1), flags=re.S)
    assert re.findall(r"\b(n_[a-z_]+|seconds_[a-z]+)\b", rep) == [n for n, _t in _native.UnpReport._fields_]
    for code, name in enumerate(("OK", "ANCHORED", "NO_VIEW", "DEGENERATE", "BEHIND")):
        assert re.search(rf"\bSBA_UNP_{name} = {code}\b", text) and getattr(_native, f"UNP_{name}") == code
    for code, name in enumerate(("OK", "UNUSABLE", "PARALLEL", "BEHIND")):
        assert re.search(rf"\bSBA_UNP_ROW_{name} = {code}\b", text) and getattr(_native, f"UNP_ROW_{name}") == code


def test_no_gpu_means_loud_failure():
    if _built().sba_device_count() > 0:
        pytest.skip("a GPU is visible; the no-device path is exercised on the CPU-only container")
    from lasercalib_amd.pySBA import PySBA
    rig = make_rig(2, 20)
    with pytest.raises(_native.SbaError, match="no HIP device"):
        _native.unproject_rows(rig["points_2d"], rig["cams0"][rig["camera_ind"]], planes=(0.0, 0.0, 1.0, 0.0))
    with pytest.raises(_native.SbaError, match="no HIP device"):
        _native.Problem(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"]).unproject((0.0, 0.0, 1.0, 0.0))
    sba = PySBA(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"])
    with pytest.raises(_native.SbaError, match="no HIP device"):
        sba.unproject(z=0.0)
    with pytest.raises(_native.SbaError, match="no HIP device"):
        sba.undistort(rig["points_2d"], rig["cams0"][rig["camera_ind"]])


def test_plane_arguments():
    assert np.array_equal(_native.z_planes(3.0, 5), [[0.0, 0.0, 1.0, 3.0]])
    assert np.array_equal(_native.z_planes([1.0, 2.0], 2), [[0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 1.0, 2.0]])
    with pytest.raises(ValueError):
        _native.z_planes([1.0, 2.0], 3)
    assert _native._planes((0, 0, 1, 2), 7, "t").shape == (1, 4)
    with pytest.raises(ValueError):
        _native._planes(np.zeros((3, 3)), 3, "t")


# ----------------------------------------------------------------------------- 2. the oracle against exact geometry
@pytest.mark.parametrize("args", RIGS, ids=RIG_IDS)
def test_oracle_meets_the_truth_on_noise_free_rays(args):
    rig = make_rig(noise_px=0.0, **args)
    N, ci, pi = rig["n_points"], rig["camera_ind"], rig["point_ind"]
    planes = z_planes_of(rig["pts_true"])
    o = unproject_oracle(rig["cams_true"], rig["points_2d"], ci, pi, N, planes)
    err = np.abs(o["points"] - rig["pts_true"]).max()
    assert np.all(o["status"] == UNP_OK) and o["used"].all() and o["n_obs_unusable"] == 0
    assert np.array_equal(o["n_views"], np.bincount(pi, minlength=N))
    o1 = unproject_oracle(rig["cams_true"], rig["points_2d"], ci, pi, N, planes, ref_cam=1)
    sees = np.bincount(pi[ci == 1], minlength=N) > 0
    err1 = np.abs(o1["points"][sees] - rig["pts_true"][sees]).max()
    print(f"{args}: max |X - truth| = {err:.3e} mm (all views), {err1:.3e} mm (camera 1), max_px {np.nanmax(o['max_px']):.3e}")
    assert np.array_equal(o1["status"] == UNP_OK, sees) and np.all(o1["status"][~sees] == UNP_NO_VIEW)
    assert np.array_equal(o1["used"], (ci == 1)) and np.isnan(o1["points"][~sees]).all()
    assert err <= 1e-8 and err1 <= 1e-8


@pytest.mark.parametrize("args", RIGS, ids=RIG_IDS)
def test_oracle_on_tilted_planes(args):
    rig = make_rig(noise_px=0.0, **args)
    N = rig["n_points"]
    planes = tilted_planes(rig["pts_true"])
    inc = min_plane_incidence(rig, planes)
    assert inc >= 0.1, inc                       # cond(G) <= 1 / 0.1^2: every case stays inside the tolerance
    o = unproject_oracle(rig["cams_true"], rig["points_2d"], rig["camera_ind"], rig["point_ind"], N, planes)
    err = np.abs(o["points"] - rig["pts_true"]).max()
    off = np.abs(np.sum(planes[:, :3] * o["points"], axis=1) - planes[:, 3]) / np.linalg.norm(planes[:, :3], axis=1)
    print(f"{args}: tilted planes, min |nh . d| {inc:.3f}, max |X - truth| = {err:.3e} mm, off the plane {off.max():.3e} mm")
    assert np.all(o["status"] == UNP_OK)
    assert err <= 1e-8 and off.max() <= 1e-9


@pytest.mark.parametrize("args", RIGS, ids=RIG_IDS)
def test_one_view_equals_the_reference_formula(args):
    rig = make_rig(noise_px=0.0, **args)
    N, ci, pi, cams = rig["n_points"], rig["camera_ind"], rig["point_ind"], rig["cams_true"]
    o = unproject_oracle(cams, rig["points_2d"], ci, pi, N, z_planes_of(rig["pts_true"]), ref_cam=1)
    sel = np.nonzero(ci == 1)[0]
    x, y, conv, R, _c, _d = rays_oracle(cams[ci[sel]], rig["points_2d"][sel])
    assert conv.all()
    xy1, t, z = np.stack([x, y, np.ones(sel.size)], 1), cams[1, 3:6], rig["pts_true"][pi[sel], 2]
    # rigid_body.py:229-242, restated
    z_cam = (z + (R[0].T @ t)[2]) / (xy1 @ R[0])[:, 2]
    X = (xy1 * z_cam[:, None] - t) @ R[0]
    diff = np.abs(o["points"][pi[sel]] - X).max()
    print(f"{args}: oracle - reference formula, one view: {diff:.3e} mm")
    assert diff <= 1e-8


def test_rows_oracle_inverts_the_projection():
    rig = make_rig(17, 500, seed=3, noise_px=0.0, visibility=0.45, tangential=True)
    ci, pi = rig["camera_ind"], rig["point_ind"]
    rows = rig["cams_true"][ci]
    o = rows_oracle(rig["points_2d"], rows, z_planes_of(rig["pts_true"])[pi])
    assert np.all(o["status"] == ROW_OK) and np.abs(o["points"] - rig["pts_true"][pi]).max() <= 1e-8
    assert np.all(o["depth"] > 0) and np.abs(np.linalg.norm(o["dir"], axis=1) - 1).max() <= 1e-15


# ----------------------------------------------------------------------------- 3. every status
@pytest.mark.parametrize("min_views", [1, 2])
def test_oracle_statuses_on_a_hand_built_problem(min_views):
    sp = status_problem()
    o = unproject_oracle(sp["cams"], sp["uv"], sp["ci"], sp["pi"], 8, sp["planes"], w=sp["w"], fixed=sp["fixed"], pts=sp["held"],
                         min_views=min_views)
    check_status_result(sp, o, min_views)
    # min_views <= 0 is read as 1
    o0 = unproject_oracle(sp["cams"], sp["uv"], sp["ci"], sp["pi"], 8, sp["planes"], w=sp["w"], fixed=sp["fixed"], pts=sp["held"],
                          min_views=0)
    assert list(o0["status"]) == sp["expect1"]


# ----------------------------------------------------------------------------- 4. the numpy half of the dataset builder
def test_dataset_keeps_the_frames_with_an_ok_estimate():
    rig = make_rig(4, 12, seed=2, noise_px=0.0, visibility=0.6)
    cent = np.full((12, 2, 4), np.nan)
    cent[rig["point_ind"], :, rig["camera_ind"]] = rig["points_2d"]
    ci, pi, uv = dataset.observation_list(cent)
    assert np.array_equal(ci, rig["camera_ind"]) and np.array_equal(pi, rig["point_ind"])
    o = unproject_oracle(rig["cams_true"], uv, ci, pi, 12, z_planes_of(rig["pts_true"]), ref_cam=0)
    ok = o["status"] == UNP_OK
    sees = ~np.isnan(cent[:, 0, 0])
    assert np.array_equal(ok, sees) and 0 < ok.sum() < 12
    out = dataset.reindex_dataset(4, o["points"], uv, ci, pi, ok)
    ref = dataset.make_dataset(cent[ok], rig["pts_true"][ok])
    assert set(out) == set(ref) and out["n_pts"] == ok.sum() and out["n_cams"] == 4
    assert np.array_equal(out["camera_ind"], ref["camera_ind"]) and np.array_equal(out["point_ind"], ref["point_ind"])
    assert np.array_equal(out["points_2d"], ref["points_2d"]) and np.abs(out["points_3d"] - ref["points_3d"]).max() <= 1e-8
    assert all(out[k].dtype == ref[k].dtype for k in ("points_2d", "points_3d", "camera_ind", "point_ind"))
    assert "make_dataset_unprojected" in dataset.__all__
