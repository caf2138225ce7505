"""Time sba_reproj_stats next to the residual kernel of the same handle and to the host route; one JSON line per rig (does not
touch bench.py).

    python tools/time_reproj_stats.py [--rigs 16x50000:f32,16x50000:f64,17x10000:f32:0.45,64x200000:f32] [--out profiles/reproj_stats_timing.jsonl]

A rig is CxN:dtype[:visibility].  Every rig is evaluated at its initial guess with everything requested that a calibration
report would ask for: the camera table and histograms (1024 bins of 1/16 px), a 16 x 12 residual field over 3208 x 2200, 16
radial bins, the per-point table and the 32 worst observations.  device_ms: HIP-event time of the call's kernels
(``seconds_device``), taken after a warm-up call; total_ms: ``seconds_total``, the whole call inside the library (private
buffers, kernels, read-back, the host's quantiles and sort); core_device_ms / core_total_ms: the same with nothing optional
(camera table and histograms only: the camera-major pass and its fold); residual_us: sba_time_kernel("residual") on the same
handle; host_summary_ms: wall time of ``report.reprojection_summary`` on a PySBA instance of the same arrays (gathered operands
up, pixels down, numpy statistics); pysba_stats_ms: wall time of ``PySBA.reprojection_stats`` with the same options, which
includes building and uploading a problem of its own.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lasercalib_amd import _native, report  # noqa: E402
from lasercalib_amd.pySBA import PySBA  # noqa: E402
from lasercalib_amd.synth import make_rig  # noqa: E402

FULL = dict(grid=(16, 12), image_size=(3208.0, 2200.0), radial_bins=16, n_worst=32, points=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rigs", default="16x50000:f32,16x50000:f64,17x10000:f32:0.45,64x200000:f32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reproj_stats_timing.jsonl"))
    a = ap.parse_args()
    rows = []
    for spec in a.rigs.split(","):
        parts = spec.split(":")
        C, N = (int(v) for v in parts[0].split("x"))
        dtype = parts[1]
        vis = float(parts[2]) if len(parts) > 2 else 1.0
        rig = make_rig(C, N, seed=0, visibility=vis, min_cams_per_point=4 if vis < 1.0 else 2)
        with _native.Problem(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"], dtype=dtype) as p:
            p.reproj_stats(**FULL)                               # warm-up
            st = p.reproj_stats(**FULL)
            p.reproj_stats(points=False)
            core = p.reproj_stats(points=False)
            res_us = p.time_kernel("residual", 20)
            chunks = p.upload_report()["n_chunks"]
        os.environ["LASERCALIB_SBA_DTYPE"] = dtype
        sba = PySBA(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"])
        report.reprojection_summary(sba)                         # warm-up
        t0 = time.perf_counter()
        host = report.reprojection_summary(sba)
        host_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        sba.reprojection_stats(**FULL)
        pysba_s = time.perf_counter() - t0
        rows.append({"rig": f"{C}x{N}", "dtype": dtype, "visibility": vis, "n_obs": int(rig["point_ind"].size), "n_chunks": chunks,
                     "device_ms": round(st.seconds_device * 1e3, 4), "total_ms": round(st.seconds_total * 1e3, 3),
                     "core_device_ms": round(core.seconds_device * 1e3, 4), "core_total_ms": round(core.seconds_total * 1e3, 3),
                     "residual_us": round(res_us, 2), "device_over_residual": round(st.seconds_device * 1e6 / res_us, 1),
                     "core_over_residual": round(core.seconds_device * 1e6 / res_us, 1),
                     "host_summary_ms": round(host_s * 1e3, 2), "pysba_stats_ms": round(pysba_s * 1e3, 2),
                     "rms_px": st.rms, "host_rms_px": host["rms"], "q50_px": st.q50, "host_median_px": host["median"],
                     "n_overflow": st.n_overflow})
        print(json.dumps(rows[-1]), flush=True)
        del rig, sba
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
