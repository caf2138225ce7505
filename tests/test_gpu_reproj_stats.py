"""GPU tests of sba_reproj_stats (include/sba_hip.h) through the C ABI.

Reference: ``reproj_stats_oracle``, the numpy restatement of the header's definitions in tests/test_reproj_stats_host.py, and
for the planted misfits the analytic residual itself.  An SBA_F32 handle computes in float64 on float32-rounded pixels and
weights; the restatement is given exactly those.

Exact comparisons: every count (n per camera, cell, radial bin and point, the report's counts), ``cam_hist`` and ``worst_idx``.
They hold under the edge condition that tests/test_reproj_stats_host.py asserts for these rigs: no error within 1e-8 px of a
histogram edge, no radius within 1e-9 of a radial-bin edge, the 32 largest errors distinct.  (Grid cells and radial bins are
formed from the observed pixels by the same float64 expressions on both sides.)
To 1e-9 px absolute: every mean, rms, max, ``err_out``, ``worst_err`` and quantile -- the project's bar for float64
residuals (tests/test_gpu_parity.py).  Measured on the MI355X: 4.1e-13 ... 2.1e-12 px, three orders under the bar."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lasercalib_amd import _native, report  # noqa: E402
from lasercalib_amd.pySBA import PySBA  # noqa: E402
from test_reproj_stats_host import (FULL, PLANTED_OPTS, RIGS, check_planted, f32_round, near_hist_edges, planted_rig,  # noqa: E402
                                    reproj_stats_oracle, rig_of)

DTYPES = ["f64", "f32"]
TOL_PX = 1e-9
RIG_IDS = [r[0] for r in RIGS]
REP_COUNTS = ("n_selected", "n_unselected", "n_nonfinite", "n_overflow", "n_worst")
REP_VALUES = ("mean_du", "mean_dv", "mean", "rms", "max", "q50", "q95", "q99")
ALL = dict(FULL, points=True, errors=True)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert _native.device_count() > 0, "no HIP device visible: GPU tests must run on the MI355X box"


def _prob(rig, dtype="f64", cams=None, pts=None, weights=None, order=None):
    uv, ci, pi = rig["points_2d"], rig["camera_ind"], rig["point_ind"]
    if order is not None:
        uv, ci, pi = uv[order], ci[order], pi[order]
        weights = None if weights is None else weights[order]
    return _native.Problem(rig["cams0"] if cams is None else cams, rig["pts0"] if pts is None else pts, uv, ci, pi,
                           weights=weights, dtype=dtype)


def _oracle(rig, dtype, opts, cams=None, pts=None, weights=None):
    narrow = f32_round if dtype == "f32" else (lambda a: a)
    okw = {k: v for k, v in opts.items() if k not in ("points", "errors")}
    return reproj_stats_oracle(rig["cams0"] if cams is None else cams, rig["pts0"] if pts is None else pts,
                               narrow(rig["points_2d"]), rig["camera_ind"], rig["point_ind"], narrow(weights), okw)


def _maxdiff(a, b):
    """largest |a - b|; NaN must sit at the same places"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b))
    m = ~np.isnan(a)
    return float(np.abs(a[m] - b[m]).max()) if m.any() else 0.0


def _against_oracle(st, o, label):
    for name in REP_COUNTS:
        assert getattr(st, name) == o[name], name
    assert np.array_equal(st.cam_hist, o["cam_hist"])
    assert np.array_equal(st.total_hist, o["cam_hist"].sum(axis=0))
    assert np.array_equal(st.worst_idx, o["worst_idx"][: o["n_worst"]])
    diffs = {"cam_stats": _maxdiff(st.cam_stats, o["cam_stats"]),
             "worst_err": _maxdiff(st.worst_err, o["worst_err"][: o["n_worst"]]),
             "rep": max(_maxdiff(getattr(st, n), o[n]) for n in REP_VALUES)}
    assert np.array_equal(st.cam_stats[:, 0], o["cam_stats"][:, 0])
    for name, mine in (("cam_grid", st.cam_grid), ("cam_radial", st.cam_radial), ("pt_stats", st.pt_stats)):
        if o[name] is None or mine is None:
            assert o[name] is None and mine is None or name == "pt_stats", name
            continue
        assert np.array_equal(mine[..., 0], o[name][..., 0]), name
        diffs[name] = _maxdiff(mine, o[name])
    if st.errors is not None:
        diffs["err_out"] = _maxdiff(st.errors, o["err_out"])
    print(f"{label}: device - numpy (px): " + ", ".join(f"{k} {v:.1e}" for k, v in diffs.items()))
    for k, v in diffs.items():
        assert v <= TOL_PX, k
    return diffs


# ----------------------------------------------------------------------------- 1. device against the restatement
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", RIG_IDS)
def test_device_matches_the_restatement(name, dtype):
    rig = rig_of(name)
    with _prob(rig, dtype) as prob:
        st = prob.reproj_stats(**ALL)
        up = prob.upload_report()
    assert st.cam_grid.shape == (rig["n_cams"], 12, 16, 4) and st.cam_radial.shape == (rig["n_cams"], 16, 4)
    assert st.n_worst == 32 and st.n_selected == len(rig["camera_ind"])
    if name.startswith("3x2500"):
        assert up["n_chunks"] == 9                                  # three chunks per camera, the last one partial
    if name.startswith("17x"):
        assert not up["dense"] and not up["masked"]                 # sparse, and one camera more than a visibility mask holds
    if name.startswith("128x"):
        assert up["dense"] and not up["masked"]
    _against_oracle(st, _oracle(rig, dtype, ALL), f"{name} {dtype}")
    assert st.seconds_device > 0 and st.seconds_total >= st.seconds_device


@pytest.mark.parametrize("dtype", DTYPES)
def test_defaults_and_other_bin_counts(dtype):
    rig = rig_of("4x300")
    with _prob(rig, dtype) as prob:
        st = prob.reproj_stats()                                     # all defaults: 1024 bins of 1/16 px, nothing optional but the points
        assert st.cam_hist.shape == (4, 1024) and st.cam_grid is None and st.cam_radial is None and len(st.worst_idx) == 0
        _against_oracle(st, _oracle(rig, dtype, {}), f"defaults {dtype}")
        for opts in (dict(hist_bins=2, hist_bin_px=20.0, n_worst=5), dict(hist_bins=4096, hist_bin_px=0.01, n_worst=4096),
                     dict(hist_bins=7, hist_bin_px=3.0, grid=(1, 1), image_size=(10.0, 10.0), radial_bins=1, r_max_px=5.0, n_worst=1),
                     dict(hist_bins=64, hist_bin_px=0.25, grid=(256, 1), image_size=(3208.0, 2200.0), radial_bins=64, n_worst=1300)):
            st = prob.reproj_stats(errors=True, **opts)
            o = _oracle(rig, dtype, opts)
            # the edge condition of the exact comparisons, for these bins and this list length
            assert near_hist_edges(o["e_used"], opts["hist_bin_px"], opts["hist_bins"]) == 0
            assert len(np.unique(o["worst_err"][: o["n_worst"]])) == o["n_worst"]
            _against_oracle(st, o, f"{opts} {dtype}")


# ----------------------------------------------------------------------------- 2. planted misfit
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tangential", [False, True], ids=["k2 11 columns", "p1 13 columns"])
def test_planted_misfit_comes_back_as_the_analytic_profile(tangential, dtype):
    rig, cams, truth = planted_rig(tangential, pixels=dtype)
    with _prob(rig, dtype, cams=cams, pts=rig["pts_true"]) as prob:
        st = prob.reproj_stats(**PLANTED_OPTS)
    check_planted(st.cam_radial, rig, truth, tangential, f"device {dtype}", exact_pixels=dtype == "f64")
    text = report.radial_profile_table(st)
    assert len(text.splitlines()) == 1 + 8 + 2 + 4
    assert len(report.per_camera_table(st).splitlines()) == 1 + 4


# ----------------------------------------------------------------------------- 3. selection
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["4x300", "17x2000 visibility 0.45"])
def test_used_and_held_out_partition_all(name, dtype):
    rig = rig_of(name)
    M = len(rig["camera_ind"])
    rng = np.random.default_rng(3)
    w = rng.uniform(0.5, 2.0, M)
    w[rng.permutation(M)[: M // 4]] = 0.0
    with _prob(rig, dtype, weights=w) as prob:
        st = {sel: prob.reproj_stats(select=sel, **ALL) for sel in ("all", "used", "held_out")}
    for sel, s in st.items():
        _against_oracle(s, _oracle(rig, dtype, dict(ALL, select=sel), weights=w), f"{name} {dtype} select={sel}")
    assert st["used"].n_selected == M - M // 4 and st["held_out"].n_selected == M // 4 and st["all"].n_selected == M
    assert st["used"].n_unselected == M // 4 and st["all"].n_unselected == 0
    assert np.array_equal(st["used"].cam_hist + st["held_out"].cam_hist, st["all"].cam_hist)
    for key in ("cam_stats", "cam_grid", "cam_radial", "pt_stats"):
        assert np.array_equal(getattr(st["used"], key)[..., 0] + getattr(st["held_out"], key)[..., 0], getattr(st["all"], key)[..., 0])
    assert np.array_equal(st["used"].errors, st["all"].errors)      # err_out covers every observation, whatever select is


@pytest.mark.parametrize("dtype", DTYPES)
def test_nothing_selected(dtype):
    rig = rig_of("4x300")
    M = len(rig["camera_ind"])
    with _prob(rig, dtype) as prob:                                  # a handle without weights: held_out selects nothing
        st = prob.reproj_stats(select="held_out", **ALL)
        used = prob.reproj_stats(select="used", **ALL)
        every = prob.reproj_stats(**ALL)
    assert st.n_selected == 0 and st.n_unselected == M and st.n_worst == 0 and st.n_overflow == 0
    assert not st.cam_hist.any()
    for a in (st.cam_stats, st.cam_grid, st.cam_radial, st.pt_stats):
        assert not a[..., 0].any() and np.isnan(a[..., 1:]).all()
    assert all(np.isnan(getattr(st, n)) for n in REP_VALUES)
    assert np.array_equal(st.errors, every.errors) and not np.isnan(st.errors).any()
    for key in ("cam_stats", "cam_hist", "cam_grid", "cam_radial", "pt_stats", "worst_idx", "worst_err"):
        assert np.array_equal(getattr(used, key), getattr(every, key), equal_nan=True)
    # a camera none of whose observations is selected
    w = np.ones(M)
    w[rig["camera_ind"] == 2] = 0.0
    with _prob(rig, dtype, weights=w) as prob:
        st = prob.reproj_stats(select="used", **ALL)
    assert st.cam_stats[2, 0] == 0 and np.isnan(st.cam_stats[2, 1:]).all() and not st.cam_hist[2].any()
    assert np.isnan(st.cam_grid[2, :, :, 1:]).all() and np.isnan(st.cam_radial[2, :, 1:]).all()
    _against_oracle(st, _oracle(rig, dtype, dict(ALL, select="used"), weights=w), f"camera 2 held out {dtype}")


# ----------------------------------------------------------------------------- 4. non-finite
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["4x300", "17x2000 visibility 0.45"])
def test_a_nan_point_is_counted_and_left_out(name, dtype):
    rig = rig_of(name)
    p = 7
    pts = rig["pts0"].copy()
    pts[p, 1] = np.nan
    with _prob(rig, dtype) as prob:
        prob.set_params(np.hstack([rig["cams0"].ravel(), pts.ravel()]))
        st = prob.reproj_stats(**ALL)
    mine = rig["point_ind"] == p
    assert st.n_nonfinite == int(mine.sum()) > 0
    assert st.pt_stats[p, 0] == 0 and np.isnan(st.pt_stats[p, 1:]).all()
    assert np.isnan(st.errors[mine]).all() and not np.isnan(st.errors[~mine]).any()
    _against_oracle(st, _oracle(rig, dtype, ALL, pts=pts), f"{name} {dtype} NaN point")
    for a in (st.cam_stats, st.cam_grid, st.cam_radial, st.pt_stats):                 # no NaN where n > 0
        assert not np.isnan(a[a[..., 0] > 0]).any()
    assert not any(np.isnan(getattr(st, n)) for n in REP_VALUES) and not np.isnan(st.worst_err).any()


# ----------------------------------------------------------------------------- 5. order and repeatability
def _same_bits(a, b, keys=("cam_stats", "cam_hist", "cam_grid", "cam_radial", "pt_stats")):
    for key in keys:
        assert np.array_equal(getattr(a, key), getattr(b, key), equal_nan=True), key
    for n in REP_COUNTS + REP_VALUES:
        assert getattr(a, n) == getattr(b, n), n


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["4x300", "3x2500 dense", "17x2000 visibility 0.45", "128x1500 13 columns"])
def test_a_shuffled_list_returns_the_same_bits(name, dtype):
    rig = rig_of(name)
    M = len(rig["camera_ind"])
    with _prob(rig, dtype) as prob:
        ref = prob.reproj_stats(**ALL)
        again = prob.reproj_stats(**ALL)
    _same_bits(ref, again)
    assert np.array_equal(ref.errors, again.errors) and np.array_equal(ref.worst_idx, again.worst_idx)
    assert np.array_equal(ref.worst_err, again.worst_err)
    orders = {"shuffled": np.random.default_rng(9).permutation(M),
              "camera descending": np.lexsort((rig["point_ind"], -rig["camera_ind"]))}
    for label, order in orders.items():
        with _prob(rig, dtype, order=order) as prob:
            st = prob.reproj_stats(**ALL)
        _same_bits(st, ref)
        assert np.array_equal(st.errors, ref.errors[order]), label          # err_out and worst_idx follow the permutation
        assert np.array_equal(order[st.worst_idx], ref.worst_idx) and np.array_equal(st.worst_err, ref.worst_err), label


# ----------------------------------------------------------------------------- 6. state and errors
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_handle_is_left_as_found(dtype):
    rig = rig_of("4x300")
    with _prob(rig, dtype) as a:
        ra, ca = a.residual()
        sa = a.solve_lm(a.make_opts(ftol=1e-8))
    with _prob(rig, dtype) as b:
        b.reproj_stats(**ALL)
        cams_b, pts_b = b.get_params()
        rb, cb = b.residual()
        b.reproj_stats(select="used", n_worst=4096)
        sb = b.solve_lm(b.make_opts(ftol=1e-8))
    assert np.array_equal(cams_b, rig["cams0"]) and np.array_equal(pts_b, rig["pts0"])
    assert np.array_equal(ra, rb) and ca == cb
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
    assert sa[2].cost == sb[2].cost and sa[2].nfev == sb[2].nfev and sa[2].status == sb[2].status


def test_error_codes():
    rig = rig_of("3x40")
    size = dict(image_size=(3208.0, 2200.0))
    bad = [dict(hist_bins=1), dict(hist_bins=4097), dict(hist_bins=-3), dict(hist_bin_px=-1.0), dict(hist_bin_px=np.inf),
           dict(hist_bin_px=np.nan), dict(grid=(0, 3), **size), dict(grid=(3, 0), **size), dict(grid=(-1, -1), **size),
           dict(grid=(17, 16), **size), dict(grid=(4, 4)), dict(grid=(4, 4), image_size=(0.0, 2200.0)),
           dict(grid=(4, 4), image_size=(3208.0, np.nan)), dict(grid=(4, 4), image_size=(np.inf, 2200.0)),
           dict(radial_bins=65, **size), dict(radial_bins=-1, **size), dict(radial_bins=4), dict(radial_bins=4, r_max_px=-2.0),
           dict(radial_bins=4, r_max_px=np.inf), dict(n_worst=4097), dict(n_worst=-1)]
    with _prob(rig) as prob:
        ref = prob.reproj_stats(**ALL)
        for opts in bad:
            with pytest.raises(_native.SbaError, match="status -1: sba_reproj_stats"):
                prob.reproj_stats(**opts)
        # the raw entry point: select out of range, and the outputs of a failed call stay as they were
        lib = _native.load()
        for sel in (-1, 3):
            opts = _native.ReprojOpts(select=sel)
            keep = np.full((3, 9), 7.0)
            rep = _native.ReprojReport(n_selected=-5)
            rc = lib.sba_reproj_stats(prob._h, ctypes.byref(opts), _native._dptr(keep), None, None, None, None, None, None, None, ctypes.byref(rep))
            assert rc == -1 and (keep == 7.0).all() and rep.n_selected == -5
        assert prob.reproj_stats(radial_bins=4, r_max_px=100.0).cam_radial.shape == (3, 4, 4)      # r_max_px given: no image size needed
        # opts NULL: all defaults
        rep = _native.ReprojReport()
        cs = np.empty((3, 9))
        assert lib.sba_reproj_stats(prob._h, None, _native._dptr(cs), None, None, None, None, None, None, None, ctypes.byref(rep)) == 0
        assert rep.n_selected == 120 and rep.n_worst == 0 and np.array_equal(cs, prob.reproj_stats().cam_stats)
        # between sba_lm_begin and sba_lm_finish: SBA_ERR_STATE
        prob.lm_begin(prob.make_opts(ftol=1e-4))
        with pytest.raises(_native.SbaError, match="status -5: .*sba_lm_begin"):
            prob.reproj_stats()
        prob.lm_run()
        prob.lm_finish()
        assert prob.reproj_stats().n_selected == 120
        again = prob.reproj_stats(**ALL)
        assert again.rms < ref.rms                                   # (the solve moved the handle's parameters)
    # before sba_upload: SBA_ERR_STATE
    desc = _native.ProblemDesc(3, 40, 120, _native.SBA_F64, 0, None, 0, _native.CAM_RADIAL, (ctypes.c_int32 * 2)())
    h = ctypes.c_void_p()
    _native._check(lib.sba_create(ctypes.byref(desc), ctypes.byref(h)))
    try:
        rep = _native.ReprojReport()
        assert lib.sba_reproj_stats(h, None, None, None, None, None, None, None, None, None, ctypes.byref(rep)) == -5
    finally:
        lib.sba_destroy(h)
    # a handle of a multi-rank job: SBA_ERR_UNSUPPORTED
    with _prob(rig) as prob:
        prob.ipc_attach(0, [prob.ipc_export(1)])
        with pytest.raises(_native.SbaError, match="status -6"):
            prob.reproj_stats()


# ----------------------------------------------------------------------------- 7. after a solve, through PySBA and report
def test_summary_after_a_solve():
    rig = rig_of("4x300")
    sba = PySBA(rig["cams0"].copy(), rig["pts0"].copy(), rig["points_2d"], rig["camera_ind"], rig["point_ind"])
    sba.bundleAdjust(1e-4)
    host, dev = report.reprojection_summary(sba), report.device_reprojection_summary(sba)
    print("host  ", host)
    print("device", dev)
    assert list(dev) == list(host) and dev["n_obs"] == host["n_obs"] == 1200
    for key in ("mean", "rms", "max"):
        assert abs(dev[key] - host[key]) <= TOL_PX, key
    for key in ("median", "p99"):
        assert abs(dev[key] - host[key]) <= 1.0 / 16, key
    st = sba.reprojection_stats(**ALL)
    from lasercalib_amd.pySBA import _env_dtype
    with _native.Problem(sba.cameraArray, sba.points3D, rig["points_2d"], rig["camera_ind"], rig["point_ind"], dtype=_env_dtype()) as prob:
        direct = prob.reproj_stats(**ALL)
    _same_bits(st, direct)
    assert np.array_equal(st.errors, direct.errors) and np.array_equal(st.worst_idx, direct.worst_idx)
    assert abs(st.rms - host["rms"]) <= TOL_PX and _maxdiff(st.errors, report.reprojection_errors(sba)) <= TOL_PX
