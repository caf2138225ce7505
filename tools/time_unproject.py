"""Time sba_unproject next to the linear pass of sba_triangulate on the same handle; one JSON line per run, appended (does not
touch bench.py).

    python tools/time_unproject.py [--rigs 16x50000:f32,16x50000:f64,64x200000:f32] [--out profiles/unproject_timing.jsonl]

A rig is CxN:dtype[:visibility[:min_cams_per_point]]; the planes are z = the true height of every point, the cameras the
perturbed ones.  device_ms: HIP-event time of the call's kernels (camera table, every point, flag scatter), taken after a warm-up
call; ref_cam_ms: the same with the observations of camera 0 only; wall_ms: the whole call (private buffers, the planes' upload,
read-back); tri_linear_ms: seconds_linear of sba_triangulate in the same process on the same handle -- the kernel that does the
same per-observation work with a 3 x 3 instead of a 2 x 2 solve (and three more sums per point).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lasercalib_amd import _native  # noqa: E402
from lasercalib_amd.synth import make_rig  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rigs", default="16x50000:f32,16x50000:f64,64x200000:f32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unproject_timing.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for spec in a.rigs.split(","):
        parts = spec.split(":")
        C, N = (int(v) for v in parts[0].split("x"))
        dtype = parts[1]
        vis = float(parts[2]) if len(parts) > 2 else 1.0
        minc = int(parts[3]) if len(parts) > 3 else 2
        rig = make_rig(C, N, seed=0, visibility=vis, min_cams_per_point=minc)
        planes = _native.z_planes(rig["pts_true"][:, 2], N)
        with _native.Problem(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"], dtype=dtype) as p:
            p.unproject(planes)                              # warm-up
            p.triangulate()
            t0 = time.perf_counter()
            unp = p.unproject(planes)
            wall = time.perf_counter() - t0
            one = p.unproject(planes, ref_cam=0)
            tri = p.triangulate()
        row = {"rig": f"{C}x{N}", "dtype": dtype, "visibility": vis, "n_obs": int(rig["point_ind"].size),
               "device_ms": round(unp.seconds_device * 1e3, 4), "ref_cam_ms": round(one.seconds_device * 1e3, 4),
               "wall_ms": round(wall * 1e3, 3), "tri_linear_ms": round(tri.seconds_linear * 1e3, 4),
               "device_over_tri_linear": round(unp.seconds_device / tri.seconds_linear, 3), "n_ok": unp.n_ok, "tri_n_ok": tri.n_ok}
        print(json.dumps(row), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")
        del rig


if __name__ == "__main__":
    main()
