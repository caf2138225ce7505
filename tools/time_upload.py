"""Time the creation of a Problem (sba_create + sba_upload: the observation layout and the parameter upload); one JSON line
per shape and route (does not touch bench.py).

    python tools/time_upload.py [--routes auto,device,host] [--ladder] [--reps 15] [--warmup 5] [--tree PATH] [--tag NAME]

wall_ms: median / quartiles of the host-clock time of ``Problem(...)`` (the constructor returns after the upload's last
stream synchronise), over --reps calls after --warmup; the phase columns are the medians of the upload report's seconds
(h2d, device layout, host layout, tables).  --tree PATH imports lasercalib_amd from another checkout; one that has neither
the ``layout`` argument nor the report is timed through its plain constructor only ("plain": true, route "plain").
Shapes (make_rig(..., seed=0)): 17 x 4 000 vis 0.45 min 4 (the reference's example size); 17 x 50 000 vis 0.45 min 4 as
emitted and shuffled; 16 x 50 000 vis 0.5; 64 x 200 000 vis 0.1 min 4; --ladder adds 17 cameras at 1.3k .. 390k points
(about 10k .. 3M observations), as emitted and shuffled (suffix s).  Fails without a GPU; there is no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

SHAPES = [("17x4000", 17, 4000, 0.45, 4, False), ("17x50000", 17, 50000, 0.45, 4, False), ("17x50000s", 17, 50000, 0.45, 4, True),
          ("16x50000", 16, 50000, 0.5, 2, False), ("64x200000", 64, 200000, 0.1, 4, False)]
LADDER = [1300, 3900, 6500, 13000, 26000, 65000, 130000, 390000]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--routes", default="auto,device,host")
    ap.add_argument("--ladder", action="store_true")
    ap.add_argument("--shapes", default="")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from lasercalib_amd import _native
    from lasercalib_amd.synth import make_rig
    if _native.device_count() <= 0:
        raise SystemExit("time_upload.py needs a GPU")
    import inspect
    plain = "layout" not in inspect.signature(_native.Problem.__init__).parameters
    routes = ["plain"] if plain else a.routes.split(",")
    shapes = [s for s in SHAPES if not a.shapes or s[0] in a.shapes.split(",")]
    if a.ladder:
        shapes = shapes + [(f"ladder17x{n}" + ("s" if sh else ""), 17, n, 0.45, 4, sh) for n in LADDER for sh in (False, True)]
    for name, C, N, vis, mincam, shuffle in shapes:
        rig = make_rig(C, N, seed=0, visibility=vis, min_cams_per_point=mincam)
        uv, ci, pi = rig["points_2d"], rig["camera_ind"], rig["point_ind"]
        if shuffle:
            o = np.random.default_rng(0).permutation(ci.size)
            uv, ci, pi = np.ascontiguousarray(uv[o]), np.ascontiguousarray(ci[o]), np.ascontiguousarray(pi[o])
        for route in routes:
            kw = {} if plain else {"layout": route}
            wall, reps = [], []
            for it in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                prob = _native.Problem(rig["cams0"], rig["pts0"], uv, ci, pi, dtype=a.dtype, **kw)
                t1 = time.perf_counter()
                if it >= a.warmup:
                    wall.append((t1 - t0) * 1e3)
                    if not plain:
                        reps.append(prob.upload_report())
                prob.close()
            q = np.percentile(wall, [25, 50, 75])
            line = {"tag": a.tag, "shape": name, "n_obs": int(ci.size), "dtype": a.dtype, "route_asked": route, "plain": plain,
                    "wall_ms": round(float(q[1]), 4), "wall_q1_ms": round(float(q[0]), 4), "wall_q3_ms": round(float(q[2]), 4),
                    "reps": a.reps, "warmup": a.warmup}
            if reps:
                line["route_taken"] = reps[-1]["route"]
                line["stream_syncs"] = reps[-1]["stream_syncs"]
                for k in ("seconds_total", "seconds_h2d", "seconds_device_layout", "seconds_host_layout", "seconds_tables"):
                    line[k.replace("seconds_", "") + "_ms"] = round(float(np.median([r[k] for r in reps])) * 1e3, 4)
            print(json.dumps(line), flush=True)
        del rig


if __name__ == "__main__":
    main()
