"""Time sba_align next to the residual kernel of the same handle; one JSON line per rig (does not touch bench.py).

    python tools/time_align.py [--rigs 16x50000:f32,16x50000:f64,64x200000:f32] [--out profiles/align_timing.jsonl]

A rig is CxN:dtype.  Every rig is aligned to a planted similarity of its own points plus 5 mm of noise, with weights, points and
camera centres together.  device_ms: HIP-event time of the call's kernels (three passes with their folds, the application and
the camera table), taken after a warm-up call; estimate_ms: the same with apply = 0 (the three passes alone); wall_ms: the
whole call -- private buffers, the upload of the targets (24 N + 8 N bytes of pageable host memory), the synchronisation for
the host's Jacobi rotations, the read-back of 25 doubles; residual_us: sba_time_kernel("residual") on the same handle.
bytes: the algorithmic traffic of the three passes and the application from the shapes alone -- per point 3 x (24 + 24 + 8)
read and 24 + 24 + 3 s read / written by the application (s = 4 or 8, the handle's dtype) -- and hbm_share: bytes / device
time as a share of the 8.0 TB/s HBM3E peak of the MI355X.  device_ms is the whole device phase: besides the streaming kernels
it holds the three one-workgroup fold launches, the camera kernels and k_cam_prep, nine launches in all, so hbm_share is the
share of the call's device time, not of the streaming kernels alone, and reads low where launch boundaries dominate.
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


def _rotation(rho):
    th = np.linalg.norm(rho)
    k = rho / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rigs", default="16x50000:f32,16x50000:f64,64x200000:f32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_timing.jsonl"))
    a = ap.parse_args()
    R, t, s_true = _rotation(np.array([0.3, -2.0, 1.1])), np.array([51.0, -20.0, 300.0]), 1.0348
    rows = []
    for spec in a.rigs.split(","):
        parts = spec.split(":")
        C, N = (int(v) for v in parts[0].split("x"))
        dtype = parts[1]
        rig = make_rig(C, N, seed=0)
        rng = np.random.default_rng(11)
        tgt = s_true * rig["pts0"] @ R.T + t + rng.normal(0.0, 5.0, (N, 3))
        pw = rng.uniform(0.2, 3.0, N)
        s = 4 if dtype == "f32" else 8
        with _native.Problem(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"], dtype=dtype) as p:
            est = p.align(tgt, pw, apply=False)                 # warm-up, and the centres the second call is given
            cams, _ = p.get_params()
            rot = _native.rotate_rows(np.tile(np.eye(3), (C, 1)), np.repeat(cams[:, 0:3], 3, axis=0)).reshape(C, 3, 3)
            tc = est.transform(-np.einsum("cij,cj->ci", rot, cams[:, 3:6]))
            est = p.align(tgt, pw, tc, apply=False)
            t0 = time.perf_counter()
            aln = p.align(tgt, pw, tc)
            wall = time.perf_counter() - t0
            res_us = p.time_kernel("residual", 20)
        nbytes = N * (3 * 56 + 48 + 3 * s)
        rows.append({"rig": f"{C}x{N}", "dtype": dtype, "n_obs": int(rig["point_ind"].size), "device_ms": round(aln.seconds_device * 1e3, 4),
                     "estimate_ms": round(est.seconds_device * 1e3, 4), "wall_ms": round(wall * 1e3, 3),
                     "residual_us": round(res_us, 2), "device_over_residual": round(aln.seconds_device * 1e6 / res_us, 2),
                     "bytes": nbytes, "hbm_share": round(nbytes / aln.seconds_device / HBM_PEAK, 4),
                     "scale": aln.scale, "rms_before_mm": aln.rms_before, "rms_after_mm": aln.rms_after,
                     "n_points_used": aln.n_points_used, "n_cams_used": aln.n_cams_used})
        print(json.dumps(rows[-1]), flush=True)
        del rig
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
