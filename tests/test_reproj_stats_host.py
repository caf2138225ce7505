"""CPU: sba_reproj_stats is declared, exported and bound; ``reproj_stats_oracle``, the numpy restatement of the definitions in
include/sba_hip.h (which tests/test_gpu_reproj_stats.py compares the kernels against), is checked where the truth is exact:
its pooled numbers are ``report``'s formulas, its quantiles bracket the order statistics, a planted radial misfit comes back
as the analytic radial profile with no tangential part, and a planted tangential misfit shows in the tangential profile.

Edge condition.  The GPU tests compare counts, histograms and the worst list EXACTLY.  That is a fair comparison only when no
error lies so close to a histogram edge (and no radius so close to a radial-bin edge) that the rounding of another evaluation
order could move it across, and when the largest errors are distinct.  ``test_no_observation_sits_on_a_bin_edge`` asserts this
for every rig, parameter set and pixel precision the GPU tests use: no e within 1e-8 px of a histogram edge, no
r nr / r_max within 1e-9 of an integer, the 32 largest errors distinct."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from lasercalib_amd import _native, report
from lasercalib_amd.synth import _project_np, make_rig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RIGS = [("3x40", dict(n_cams=3, n_points=40)),
        ("4x300", dict(n_cams=4, n_points=300)),
        ("3x2500 dense", dict(n_cams=3, n_points=2500)),
        ("17x2000 visibility 0.45", dict(n_cams=17, n_points=2000, visibility=0.45, min_cams_per_point=4)),
        ("128x1500 13 columns", dict(n_cams=128, n_points=1500, tangential=True))]
FULL = dict(hist_bin_px=1.0 / 16, grid=(16, 12), image_size=(3208.0, 2200.0), radial_bins=16, n_worst=32)
QS = (0.5, 0.95, 0.99)


@functools.lru_cache(maxsize=None)
def rig_of(name):
    return make_rig(**dict(RIGS)[name])


def f32_round(a):
    """what an SBA_F32 handle keeps of a float64 array"""
    return None if a is None else np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


# ----------------------------------------------------------------------------- numpy restatement (also used by the GPU tests)
def quantile_bin(h, q):
    """first bin whose running total reaches t = q n, and t"""
    t = q * int(h.sum())
    return int(np.argmax(np.cumsum(h) >= t)), t


def hist_quantile(h, q, m, bin_px):
    n = int(h.sum())
    if n == 0:
        return np.nan
    k, t = quantile_bin(h, q)
    if k == len(h) - 1:
        return m
    before = int(h[:k].sum())
    return (k + (t - before) / int(h[k])) * bin_px


def _binned(key, nbins, a, b, e2):
    """[n, mean a, mean b, rms] per bin from the bins ``key`` of the used observations"""
    n = np.bincount(key, minlength=nbins).astype(np.float64)
    out = np.full((nbins, 4), np.nan)
    out[:, 0] = n
    has = n > 0
    for col, val in ((1, a), (2, b), (3, e2)):
        s = np.bincount(key, weights=val, minlength=nbins)
        out[has, col] = s[has] / n[has]
    out[has, 3] = np.sqrt(out[has, 3])
    return out


def reproj_stats_oracle(cams, pts, uv, ci, pi, w, opts):
    """sba_reproj_stats on float64 numpy arrays, from the text of include/sba_hip.h.  opts: the keywords of
    ``Problem.reproj_stats`` (select, hist_bins, hist_bin_px, grid, image_size, radial_bins, r_max_px, n_worst).
    For an SBA_F32 handle pass ``f32_round(uv)`` and ``f32_round(w)``."""
    o = dict(select="all", hist_bins=None, hist_bin_px=None, grid=None, image_size=None, radial_bins=0, r_max_px=None, n_worst=0)
    o.update(opts)
    cams, pts, uv = np.asarray(cams, float), np.asarray(pts, float), np.asarray(uv, float)
    C, N, M, P = cams.shape[0], pts.shape[0], uv.shape[0], cams.shape[1]
    B = o["hist_bins"] or 1024
    bin_px = o["hist_bin_px"] or 1.0 / 16
    inv = 1.0 / bin_px
    with np.errstate(all="ignore"):
        d = _project_np(pts[pi], cams[ci]) - uv
        e = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2)
    finite = np.isfinite(d[:, 0]) & np.isfinite(d[:, 1])
    if o["select"] == "all":
        sel = np.ones(M, bool)
    elif o["select"] == "used":
        sel = np.ones(M, bool) if w is None else np.asarray(w) > 0
    else:
        sel = np.zeros(M, bool) if w is None else np.asarray(w) == 0
    use = sel & finite
    out = dict(n_selected=int(sel.sum()), n_unselected=int(M - sel.sum()), n_nonfinite=int((sel & ~finite).sum()),
               err_out=np.where(finite, e, np.nan))
    cu, pu, du, dv, eu, uvu = ci[use], pi[use], d[use, 0], d[use, 1], e[use], uv[use]
    # histogram
    k = np.minimum(np.floor(eu * inv), B - 1).astype(np.int64)
    hist = np.bincount(cu * B + k, minlength=C * B).reshape(C, B)
    out["cam_hist"] = hist
    out["n_overflow"] = int(hist[:, B - 1].sum())
    # per camera
    cs = np.full((C, 9), np.nan)
    for c in range(C):
        m = cu == c
        n = int(m.sum())
        cs[c, 0] = n
        if n:
            ec = eu[m]
            cs[c, 1:6] = du[m].mean(), dv[m].mean(), ec.mean(), np.sqrt(np.mean(ec * ec)), ec.max()
            cs[c, 6:9] = [hist_quantile(hist[c], q, ec.max(), bin_px) for q in QS]
    out["cam_stats"] = cs
    # residual field
    out["cam_grid"] = None
    if o["grid"] is not None and o["grid"][0] * o["grid"][1] > 0:
        gx, gy = o["grid"]
        width, height = o["image_size"]
        ix = np.clip(np.floor(uvu[:, 0] * (gx / width)), 0, gx - 1).astype(np.int64)
        iy = np.clip(np.floor(uvu[:, 1] * (gy / height)), 0, gy - 1).astype(np.int64)
        out["cam_grid"] = _binned((cu * gy + iy) * gx + ix, C * gy * gx, du, dv, eu * eu).reshape(C, gy, gx, 4)
    # radial profile
    out["cam_radial"] = None
    if o["radial_bins"]:
        nr = o["radial_bins"]
        r_max = o["r_max_px"] or 0.5 * np.sqrt(o["image_size"][0] ** 2 + o["image_size"][1] ** 2)
        dx, dy = uvu[:, 0] - cams[cu, P - 2], uvu[:, 1] - cams[cu, P - 1]
        r = np.sqrt(dx * dx + dy * dy)
        b = np.minimum(np.floor(r * (nr / r_max)), nr - 1).astype(np.int64)
        with np.errstate(all="ignore"):
            rx, ry = np.where(r > 0, dx / r, 0.0), np.where(r > 0, dy / r, 0.0)
        out["cam_radial"] = _binned(cu * nr + b, C * nr, du * rx + dv * ry, rx * dv - ry * du, eu * eu).reshape(C, nr, 4)
        out["radial_t"] = r * (nr / r_max)
    # per point
    n = np.bincount(pu, minlength=N).astype(np.float64)
    ps = np.full((N, 3), np.nan)
    ps[:, 0] = n
    has = n > 0
    ps[has, 1] = np.sqrt(np.bincount(pu, weights=eu * eu, minlength=N)[has] / n[has])
    mx = np.zeros(N)
    np.maximum.at(mx, pu, eu)
    ps[has, 2] = mx[has]
    out["pt_stats"] = ps
    # the K worst: e descending, ties to the smaller index
    K = o["n_worst"]
    cand = np.nonzero(use)[0]
    order = cand[np.lexsort((cand, -e[cand]))][:K]
    out["n_worst"] = len(order)
    out["worst_idx"] = np.concatenate([order, np.full(K - len(order), -1, np.int64)])
    out["worst_err"] = np.concatenate([e[order], np.full(K - len(order), np.nan)])
    # global
    nn = int(use.sum())
    total = hist.sum(axis=0)
    if nn:
        out.update(mean_du=du.mean(), mean_dv=dv.mean(), mean=eu.mean(), rms=np.sqrt(np.mean(eu * eu)), max=eu.max())
    else:
        out.update(mean_du=np.nan, mean_dv=np.nan, mean=np.nan, rms=np.nan, max=np.nan)
    for q, name in zip(QS, ("q50", "q95", "q99")):
        out[name] = hist_quantile(total, q, out["max"], bin_px)
    out["e_used"] = eu
    return out


def near_hist_edges(e, bin_px, B, tol_px=1e-8):
    """how many errors lie within tol_px of a histogram edge (edges 1 .. B - 1; beyond the last everything is the overflow bin)"""
    t = e / bin_px
    t = t[t < B - 0.5]
    return int((np.abs(t - np.round(t)) * bin_px <= tol_px).sum())


# ----------------------------------------------------------------------------- 1. declared, exported, bound
def _header():
    return open(os.path.join(ROOT, "include", "sba_hip.h")).read()


def test_reproj_stats_is_declared_exported_and_bound():
    text = _header()
    assert re.search(r"\bint sba_reproj_stats\(sba_handle\* h, const sba_reproj_opts\* opts", text)
    assert "sba_reproj_stats" in _native.EXPORTED_SYMBOLS
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _native.load()
    raw = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(raw, "sba_reproj_stats")
    assert lib.sba_reproj_stats.argtypes is not None and len(lib.sba_reproj_stats.argtypes) == 11
    assert lib.sba_abi_version() == 2
    assert callable(_native.Problem.reproj_stats)
    from lasercalib_amd.pySBA import PySBA
    assert callable(PySBA.reprojection_stats)
    assert callable(report.device_reprojection_summary) and callable(report.per_camera_table) and callable(report.radial_profile_table)


def test_struct_layouts_match_the_header():
    # sba_reproj_opts: int32 x 2 + double + int32 x 4 + double x 3 + int32 x 6 = 8 + 8 + 16 + 24 + 24 = 80
    # sba_reproj_report: int64 x 4 + int32 x 2 + double x 10 = 32 + 8 + 80 = 120
    assert ctypes.sizeof(_native.ReprojOpts) == 80
    assert ctypes.sizeof(_native.ReprojReport) == 120
    text = _header()
    opts = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} sba_reproj_opts;", text).group(1), flags=re.S)
    names = re.findall(r"\b(select|hist_bins|hist_bin_px|grid_x|grid_y|radial_bins|n_worst|width|height|r_max_px|reserved)\b", opts)
    assert names == [n for n, _t in _native.ReprojOpts._fields_]
    rep = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} sba_reproj_report;", text).group(1), flags=re.S)
    names = re.findall(r"\b(n_selected|n_unselected|n_nonfinite|n_overflow|n_worst|reserved|mean_du|mean_dv|mean|rms|max|q50|q95|q99|"
                       r"seconds_device|seconds_total)\b", rep)
    assert names == [n for n, _t in _native.ReprojReport._fields_]


# ----------------------------------------------------------------------------- 2. the restatement against report's formulas
class _HostSBA:
    """the attributes ``report.reprojection_errors`` reads, projecting on the host"""

    def __init__(self, rig, cams, pts):
        self.cameraArray, self.points3D, self.points2D = cams, pts, rig["points_2d"]
        self.cameraIndices, self.point2DIndices = rig["camera_ind"], rig["point_ind"]

    project = staticmethod(_project_np)


@pytest.mark.parametrize("name", ["4x300", "17x2000 visibility 0.45"])
def test_oracle_pools_like_report(name):
    rig = rig_of(name)
    o = reproj_stats_oracle(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"], None, {})
    s = report.reprojection_summary(_HostSBA(rig, rig["cams0"], rig["pts0"]))
    assert o["n_selected"] == s["n_obs"] and o["n_nonfinite"] == 0 and o["n_unselected"] == 0
    for key in ("mean", "rms", "max"):
        print(f"{name} {key}: oracle {o[key]:.15g} report {s[key]:.15g}")
        assert abs(o[key] / s[key] - 1) <= 1e-12
    # the camera rows add up to the pooled ones
    n = o["cam_stats"][:, 0]
    assert n.sum() == s["n_obs"]
    assert abs(np.sum(n * o["cam_stats"][:, 3]) / n.sum() / s["mean"] - 1) <= 1e-12
    assert o["cam_stats"][:, 5].max() == o["max"]
    assert o["pt_stats"][:, 0].sum() == s["n_obs"] and np.nanmax(o["pt_stats"][:, 2]) == o["max"]


@pytest.mark.parametrize("which", ["cams0", "true"])
@pytest.mark.parametrize("name", ["4x300", "17x2000 visibility 0.45"])
def test_quantile_bins_bracket_the_order_statistics(name, which):
    rig = rig_of(name)
    cams, pts = (rig["cams0"], rig["pts0"]) if which == "cams0" else (rig["cams_true"], rig["pts_true"])
    bin_px = 1.0 / 16
    o = reproj_stats_oracle(cams, pts, rig["points_2d"], rig["camera_ind"], rig["point_ind"], None, dict(hist_bin_px=bin_px))
    hists = [(o["cam_hist"].sum(axis=0), o["e_used"])]
    hists += [(o["cam_hist"][c], o["e_used"][rig["camera_ind"] == c]) for c in range(rig["n_cams"])]
    for h, e in hists:
        srt = np.sort(e)
        for q in QS:
            k, t = quantile_bin(h, q)
            x = srt[int(np.ceil(t)) - 1]                              # order statistic of rank ceil(q n)
            assert min(len(h) - 1, int(np.floor(x / bin_px))) == k
            v = hist_quantile(h, q, srt[-1], bin_px)
            if k < len(h) - 1:
                assert k * bin_px <= v <= (k + 1) * bin_px
            else:
                assert v == srt[-1]
    assert abs(o["q50"] - np.median(o["e_used"])) <= bin_px


# ----------------------------------------------------------------------------- 3. planted misfit: the truth is exact
def planted_rig(tangential, pixels="f64"):
    """4 x 300 without noise at the true parameters, with k2 (11 columns) or p1 (13 columns) of every camera raised by 1e-3:
    returns the rig, the evaluated cameras and the analytic residual d (M, 2).  pixels="f32": as an SBA_F32 handle sees it --
    the pixels it keeps are the float32-rounded ones, and their (known) rounding is part of the analytic residual."""
    rig = make_rig(4, 300, noise_px=0, perturb=False, tangential=tangential)
    cams = rig["cams_true"].copy()
    ci, pi = rig["camera_ind"], rig["point_ind"]
    P = cams.shape[1]
    # normalised coordinates of the truth: the observed pixels are exact, so invert nothing -- project the truth's geometry
    rv = rig["cams_true"][ci, :3]
    theta = np.linalg.norm(rv, axis=1)[:, None]
    ax = rv / theta
    X = rig["pts_true"][pi]
    p = np.cos(theta) * X + np.sin(theta) * np.cross(ax, X) + np.sum(X * ax, axis=1)[:, None] * (1 - np.cos(theta)) * ax + cams[ci, 3:6]
    x, y = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    n = x * x + y * y
    f = cams[ci, 6]
    if tangential:
        cams[:, 9] += 1e-3
        d = (f * 1e-3)[:, None] * np.stack([2 * x * y, n + 2 * y * y], axis=1)
    else:
        cams[:, 8] += 1e-3
        d = (f * 1e-3 * n * n)[:, None] * np.stack([x, y], axis=1)
    uv = rig["points_2d"] if pixels == "f64" else f32_round(rig["points_2d"])
    d = d + (rig["points_2d"] - uv)
    dx, dy = uv[:, 0] - cams[ci, P - 2], uv[:, 1] - cams[ci, P - 1]
    r = np.sqrt(dx * dx + dy * dy)
    return rig, cams, dict(d=d, rx=dx / r, ry=dy / r, r=r, radial_11=f * 1e-3 * n * n * np.sqrt(n))


PLANTED_OPTS = dict(radial_bins=8, image_size=(3208.0, 2200.0))


def planted_profile(rig, truth, nr=8, r_max=0.5 * np.sqrt(3208.0 ** 2 + 2200.0 ** 2)):
    """(C, nr, 2) analytic mean radial / tangential residual per camera and bin (NaN where a bin is empty)"""
    ci, C = rig["camera_ind"], rig["n_cams"]
    b = np.minimum(np.floor(truth["r"] * (nr / r_max)), nr - 1).astype(np.int64)
    rad = truth["d"][:, 0] * truth["rx"] + truth["d"][:, 1] * truth["ry"]
    tan = truth["rx"] * truth["d"][:, 1] - truth["ry"] * truth["d"][:, 0]
    n = np.bincount(ci * nr + b, minlength=C * nr).astype(np.float64)
    with np.errstate(all="ignore"):
        out = np.stack([np.bincount(ci * nr + b, weights=v, minlength=C * nr) / n for v in (rad, tan)], axis=1)
    return out.reshape(C, nr, 2), n.reshape(C, nr)


def check_planted(cam_radial, rig, truth, tangential, label, exact_pixels=True):
    """The profile against the analytic one, to 1e-9 px.  With exact pixels a k2 misfit is purely radial: every mean tangential
    is at most 1e-9 px.  An SBA_F32 handle keeps float32 pixels, rounded by up to 1.2e-4 px at 2 000 px; that rounding is part of
    its residuals and of the analytic profile it is compared with (``planted_rig(pixels="f32")``), in both components, so the
    tangential means are then held to the analytic values only (exact_pixels=False)."""
    exp, n = planted_profile(rig, truth)
    assert np.array_equal(cam_radial[:, :, 0], n)
    has = n > 0
    d_rad = np.abs(cam_radial[:, :, 1] - exp[:, :, 0])[has].max()
    d_tan = np.abs(cam_radial[:, :, 2] - exp[:, :, 1])[has].max()
    print(f"{label}: radial mean off by {d_rad:.1e} px, tangential mean off by {d_tan:.1e} px, "
          f"largest |radial| {np.abs(exp[:, :, 0][has]).max():.3g} px, largest |tangential| {np.abs(exp[:, :, 1][has]).max():.3g} px")
    assert d_rad <= 1e-9 and d_tan <= 1e-9
    if tangential:
        assert np.abs(exp[:, :, 1][has]).max() > 1e-2              # the formula says the tangential part is there ...
        big = has & (np.abs(exp[:, :, 1]) > 1e-2)
        assert np.all(np.abs(cam_radial[:, :, 2][big]) > 1e-2)     # ... and the profile shows it in those bins
    else:
        if exact_pixels:
            assert np.abs(cam_radial[:, :, 2][has]).max() <= 1e-9  # a k2 misfit is purely radial
        assert np.abs(exp[:, :, 0][has]).max() > 1e-2


def test_planted_k2_misfit_is_purely_radial():
    rig, cams, truth = planted_rig(False)
    # the residual is along (x, y), and so is the pixel's offset from the principal point: radial = f 1e-3 n^2 |xy|
    rad = truth["d"][:, 0] * truth["rx"] + truth["d"][:, 1] * truth["ry"]
    assert np.abs(rad - truth["radial_11"]).max() <= 1e-12 * np.abs(rad).max() + 1e-12
    o = reproj_stats_oracle(cams, rig["pts_true"], rig["points_2d"], rig["camera_ind"], rig["point_ind"], None, PLANTED_OPTS)
    check_planted(o["cam_radial"], rig, truth, False, "k2 + 1e-3, 11 columns")


def test_planted_p1_misfit_shows_in_the_tangential_profile():
    rig, cams, truth = planted_rig(True)
    o = reproj_stats_oracle(cams, rig["pts_true"], rig["points_2d"], rig["camera_ind"], rig["point_ind"], None, PLANTED_OPTS)
    check_planted(o["cam_radial"], rig, truth, True, "p1 + 1e-3, 13 columns")


# ----------------------------------------------------------------------------- 4. the edge condition of the exact comparisons
@pytest.mark.parametrize("pixels", ["f64", "f32"])
@pytest.mark.parametrize("which", ["cams0", "true"])
@pytest.mark.parametrize("name", [r[0] for r in RIGS])
def test_no_observation_sits_on_a_bin_edge(name, which, pixels):
    rig = rig_of(name)
    cams, pts = (rig["cams0"], rig["pts0"]) if which == "cams0" else (rig["cams_true"], rig["pts_true"])
    uv = rig["points_2d"] if pixels == "f64" else f32_round(rig["points_2d"])
    o = reproj_stats_oracle(cams, pts, uv, rig["camera_ind"], rig["point_ind"], None, FULL)
    near_e = near_hist_edges(o["e_used"], 1.0 / 16, 1024)
    tr = o["radial_t"][o["radial_t"] < 15.0]
    near_r = int((np.abs(tr - np.round(tr)) <= 1e-9).sum())
    worst = o["worst_err"]
    print(f"{name} {which} {pixels}: {near_e} errors within 1e-8 px of an edge, {near_r} radii within 1e-9 of a bin edge, "
          f"smallest gap among the 32 largest errors {np.min(-np.diff(worst)):.2e} px")
    assert near_e == 0 and near_r == 0
    assert len(np.unique(worst)) == 32 and o["n_worst"] == 32
