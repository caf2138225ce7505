"""Time sba_triangulate next to the residual kernel of the same handle; one JSON line per run (does not touch bench.py).

    python tools/time_triangulate.py [--rigs 16x50000:f32,16x50000:f64,17x10000:f32:0.45:4,64x200000:f32] [--out profiles/triangulate_timing.jsonl]

A rig is CxN:dtype[:visibility[:min_cams_per_point]]; every rig runs twice, as it is and with one 40-80 px outlier planted in
1 % of its points and trim_px = 3.  linear_ms / trim_ms / device_ms: HIP-event times of the call's kernels (camera table + every
point; the trimming of the listed points; both plus the flag scatter), taken after a warm-up call; wall_ms: the whole call
(private buffers, read-back); residual_us: sba_time_kernel("residual") on the same handle, the existing streaming kernel with
the same reads.  bytes: the algorithmic traffic of k_ray_fit from the shapes alone -- per observation 2 s + 4 read (+ s with
weights; s = 4 or 8, the handle's dtype) and 1 written (the flag), per point 24 written for X and 28 for the diagnostics -- and
hbm_share: bytes / linear time as a share of the 8.0 TB/s HBM3E peak of the MI355X.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lasercalib_amd import _native  # noqa: E402
from lasercalib_amd.synth import make_rig  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, HBM3E peak of the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rigs", default="16x50000:f32,16x50000:f64,17x10000:f32:0.45:4,64x200000:f32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triangulate_timing.jsonl"))
    a = ap.parse_args()
    rows = []
    for spec in a.rigs.split(","):
        parts = spec.split(":")
        C, N = (int(v) for v in parts[0].split("x"))
        dtype = parts[1]
        vis = float(parts[2]) if len(parts) > 2 else 1.0
        minc = int(parts[3]) if len(parts) > 3 else 2
        rig = make_rig(C, N, seed=0, visibility=vis, min_cams_per_point=minc)
        pi = rig["point_ind"]
        M = int(pi.size)
        s = 4 if dtype == "f32" else 8
        for planted in (False, True):
            uv = rig["points_2d"]
            if planted:
                rng = np.random.default_rng(11)
                start, deg = np.searchsorted(pi, np.arange(N)), np.bincount(pi, minlength=N)
                bad_pts = np.arange(0, N, 100)
                bad = start[bad_pts] + rng.integers(0, deg[bad_pts])
                ang, mag = rng.uniform(0, 2 * np.pi, bad.size), rng.uniform(40, 80, bad.size)
                uv = uv.copy()
                uv[bad] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1)
            trim = 3.0 if planted else None
            with _native.Problem(rig["cams_true"], rig["pts0"], uv, rig["camera_ind"], pi, dtype=dtype) as p:
                p.triangulate(trim_px=trim)                      # warm-up
                t0 = time.perf_counter()
                tri = p.triangulate(trim_px=trim)
                wall = time.perf_counter() - t0
                res_us = p.time_kernel("residual", 20)
            nbytes = M * (2 * s + 4 + 1) + N * (24 + 28)
            rows.append({"rig": f"{C}x{N}", "dtype": dtype, "visibility": vis, "n_obs": M, "planted": int(planted and bad.size),
                         "trim_px": trim, "linear_ms": round(tri.seconds_linear * 1e3, 4), "trim_ms": round(tri.seconds_trim * 1e3, 4),
                         "device_ms": round(tri.seconds_device * 1e3, 4), "wall_ms": round(wall * 1e3, 3),
                         "residual_us": round(res_us, 2), "linear_over_residual": round(tri.seconds_linear * 1e6 / res_us, 2),
                         "bytes": nbytes, "hbm_share": round(nbytes / tri.seconds_linear / HBM_PEAK, 4),
                         "n_ok": tri.n_ok, "n_obs_trimmed": tri.n_obs_trimmed, "n_points_trimmed": tri.n_points_trimmed})
            print(json.dumps(rows[-1]), flush=True)
        del rig
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
