"""Time sba_covariance next to the LM step of the same handle; one JSON line per rig (does not touch bench.py).

    python tools/time_covariance.py [--rigs 16x50000:f64,64x200000:f32,128x1000000:f32:13] [--iters 5]

cams_ms / all_ms: device time (HIP events, kernels only) of a cameras-only call (points=False) and of a call with every point;
form_ms / inverse_ms / points_ms: the split of the second call (S formation, factorisation + inverse + gauge projection, camera
blocks + point pass); cams_wall_ms / all_wall_ms: wall time of the whole calls (host layout pass, uploads and read-back included);
lm_step_ms: device time per LM iteration of the same handle (always re-linearising, as bench.py does).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lasercalib_amd import _native  # noqa: E402
from lasercalib_amd.synth import make_rig  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rigs", default="16x50000:f64,16x50000:f32,64x200000:f64,64x200000:f32")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--vis", type=float, default=1.0)
    a = ap.parse_args()
    for spec in a.rigs.split(","):
        parts = spec.split(":")
        shape, dtype = parts[0], parts[1]
        ncp = int(parts[2]) if len(parts) > 2 else 11
        C, N = (int(v) for v in shape.split("x"))
        rig = make_rig(C, N, seed=0, visibility=a.vis, tangential=(ncp == 13))
        with _native.Problem(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"], dtype=dtype) as p:
            _, _, rep, _ = p.solve_lm(p.make_opts(max_iter=a.iters, always_relinearize=True))
            step_ms = rep.seconds_device * 1e3 / max(rep.iterations, 1)
            p.covariance(points=False)                       # warm-up
            cams = p.covariance(points=False)
            full = p.covariance(points=True)
        print(json.dumps({"rig": f"{C}x{N}", "params": ncp, "dtype": dtype, "n_obs": int(rig["camera_ind"].size),
                          "cams_ms": round(cams.seconds_device * 1e3, 3), "all_ms": round(full.seconds_device * 1e3, 3),
                          "form_ms": round(full.seconds_form * 1e3, 3), "inverse_ms": round(full.seconds_inverse * 1e3, 3),
                          "points_ms": round(full.seconds_points * 1e3, 3),
                          "cams_wall_ms": round(cams.seconds_total * 1e3, 3), "all_wall_ms": round(full.seconds_total * 1e3, 3),
                          "lm_step_ms": round(step_ms, 3),
                          "cams_in_steps": round(cams.seconds_device * 1e3 / step_ms, 2),
                          "all_in_steps": round(full.seconds_device * 1e3 / step_ms, 2),
                          "all_wall_in_steps": round(full.seconds_total * 1e3 / step_ms, 2)}), flush=True)
        del rig


if __name__ == "__main__":
    main()
