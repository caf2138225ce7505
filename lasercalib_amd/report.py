"""Reporting pass after a solve: the numeric part of the reference's ``lasercalib/sba_print.py``.

``sba_print`` (sba_print.py:8-46) prints the camera table, histograms the per-observation reprojection error and draws
the rig.  The plotting stays with the caller; what it computes is here, with the 800k-observation reprojection pass
going through the device ``project`` kernel (``sba_project``) instead of numpy temporaries:

* :func:`reprojection_errors`  -- sba_print.py:17-19  (``||project(points3D[pi], cameraArray[ci]) - points2D||`` per observation)
* :func:`camera_table`         -- sba_print.py:12-15  (one row per camera; plain text, no ``prettytable``)
* :func:`camera_extrinsics`    -- sba_print.py:33-42  (4x4 pose handed to the pyramid drawer)
"""
from __future__ import annotations

import numpy as np
from scipy.spatial.transform import Rotation as R

__all__ = ["reprojection_errors", "reprojection_summary", "camera_table", "camera_extrinsics",
           "device_reprojection_summary", "per_camera_table", "radial_profile_table"]


def reprojection_errors(sba) -> np.ndarray:
    """(M,) Euclidean pixel error of every observation at the instance's current parameters (sba_print.py:17-19)."""
    r = sba.project(sba.points3D[sba.point2DIndices], sba.cameraArray[sba.cameraIndices]) - sba.points2D
    return np.sqrt(np.sum(r ** 2, axis=1))


def reprojection_summary(sba) -> dict:
    """Mean / RMS / median / 99th percentile of :func:`reprojection_errors` (the histogram's range, sba_print.py:21)."""
    e = reprojection_errors(sba)
    return {"n_obs": int(e.size), "mean": float(e.mean()), "rms": float(np.sqrt(np.mean(e ** 2))),
            "median": float(np.median(e)), "p99": float(np.percentile(e, 99)), "max": float(e.max())}


def device_reprojection_summary(sba) -> dict:
    """The keys of :func:`reprojection_summary` from ``PySBA.reprojection_stats`` (sba_reproj_stats): nothing but the result
    crosses the bus.  n_obs, mean, rms and max are exact sums over the observations; median and p99 are read off the integer
    histogram of the errors, by linear interpolation inside a bin of 1/16 px (1024 bins: errors of 64 px and more share the last
    bin, and a quantile that falls there is reported as the largest error)."""
    st = sba.reprojection_stats(points=False)
    return {"n_obs": int(st.n_selected - st.n_nonfinite), "mean": float(st.mean), "rms": float(st.rms),
            "median": float(st.q50), "p99": float(st.q99), "max": float(st.max)}


def per_camera_table(stats) -> str:
    """One row per camera of a ``ReprojStats``: n, mean du, mean dv, mean, rms, max, q50, q95, q99 (pixels), as fixed-width text."""
    cols = ("n", "mean du", "mean dv", "mean", "rms", "max", "q50", "q95", "q99")
    head = " cam " + " ".join(f"{c:>10s}" for c in cols)
    rows = [f"{i:4d} {int(row[0]):10d} " + " ".join(f"{v:10.4g}" for v in row[1:]) for i, row in enumerate(stats.cam_stats)]
    return "\n".join([head] + rows)


def radial_profile_table(stats) -> str:
    """The radial / tangential profile of a ``ReprojStats`` (``radial_bins`` > 0), pooled over the cameras: per radial bin the
    count, the mean radial and tangential residual and the rms (pixels), then one line per camera with its mean radial
    residual per bin.  Pooled means weight every camera's bin by its count."""
    if stats.cam_radial is None:
        raise ValueError("the radial profile was not computed (radial_bins=0)")
    prof, edges = stats.cam_radial, stats.radial_edges
    n = prof[:, :, 0]
    tot = n.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        pooled = [np.where(tot > 0, np.nansum(n * prof[:, :, k], axis=0) / tot, np.nan) for k in (1, 2)]
        rms = np.where(tot > 0, np.sqrt(np.nansum(n * prof[:, :, 3] ** 2, axis=0) / tot), np.nan)
    head = f"{'r from':>9s} {'r to':>9s} {'n':>10s} {'radial':>10s} {'tangential':>10s} {'rms':>10s}"
    rows = [f"{edges[b]:9.1f} {edges[b + 1]:9.1f} {int(tot[b]):10d} {pooled[0][b]:10.4g} {pooled[1][b]:10.4g} {rms[b]:10.4g}"
            for b in range(prof.shape[1])]
    cam_head = " cam " + " ".join(f"{edges[b]:9.0f}+" for b in range(prof.shape[1]))
    cam_rows = [f"{c:4d} " + " ".join(f"{v:10.4g}" for v in prof[c, :, 1]) for c in range(prof.shape[0])]
    return "\n".join([head] + rows + ["mean radial residual per camera and bin", cam_head] + cam_rows)


_COLS = ("rx", "ry", "rz", "tx", "ty", "tz", "f", "k1", "k2", "cx", "cy")


def camera_table(sba) -> str:
    """The camera rows ``sba_print`` feeds to PrettyTable (sba_print.py:12-15), as fixed-width text."""
    cams = np.asarray(sba.cameraArray, dtype=np.float64)
    head = " cam " + " ".join(f"{c:>12s}" for c in _COLS[: cams.shape[1]])
    rows = [f"{i:4d} " + " ".join(f"{v:12.6g}" for v in row) for i, row in enumerate(cams)]
    return "\n".join([head] + rows)


def camera_uncertainty_table(sba, cov) -> str:
    """``camera_table`` with the standard deviation of every parameter (``cov``: the result of ``PySBA.covariance``)."""
    cams = np.asarray(sba.cameraArray, dtype=np.float64)
    std = cov.camera_std()
    cols = _COLS if cams.shape[1] == 11 else _COLS[:9] + ("p1", "p2") + _COLS[9:]
    head = " cam " + " ".join(f"{c:>22s}" for c in cols[: cams.shape[1]])
    rows = [f"{i:4d} " + " ".join(f"{v:11.5g} +-{s:8.2g}" for v, s in zip(row, srow)) for i, (row, srow) in enumerate(zip(cams, std))]
    return "\n".join([head] + rows)


def camera_extrinsics(sba) -> np.ndarray:
    """(C,4,4) matrices ``ex`` of sba_print.py:33-42: rotation block = R(-rotvec), translation = -R(-rotvec) t."""
    cams = np.asarray(sba.cameraArray, dtype=np.float64)
    out = np.tile(np.eye(4), (cams.shape[0], 1, 1))
    for i, row in enumerate(cams):
        r_f = R.from_rotvec(-row[0:3]).as_matrix()
        out[i, :3, :3] = r_f              # (r_inv).T with r_inv = r_f.T
        out[i, :3, 3] = -r_f @ row[3:6]
    return out
