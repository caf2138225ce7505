"""Time sba_warp_frames next to sba_undistort_frames on full-size frames; one JSON line per run, appended (does not touch bench.py).

    python tools/time_warp.py [--size 3208x2200x3] [--frames 32,128] [--grid 2000] [--host-frames 16] [--reps 7] [--out profiles/warp_timing.jsonl]

Frames are uniform random bytes (the kernels' work does not depend on the values).  One camera of the example rig's kind: f 1780,
k1 = 3.6e-4, k2 = -1.4e-2, looking down on the floor from 2.5 m, tilted by 0.24 rad.  In the same run, on device-resident frames
into device-resident outputs, bilinear:

* ``plane_view``: the floor (z = 0) on a ``--grid`` x ``--grid`` grid of 1.5 mm pixels, nearly all of which the camera sees
  (``plane_view_outside_fraction``);
* ``warp_inverse_k``: ``warp_frames`` with m = K^-1, the camera's own matrix -- sba_undistort_frames restated, at the source's size;
* ``undistort``: ``undistort_frames`` with the same lens and matrix -- the same taps through the other front end;
* d2d: ``dst.copy_(src)`` of the larger batch under HIP events -- the yardstick.

Each call is timed at two batch sizes (both far larger than the 256 MiB Infinity Cache); the slope (t2 - t1) / (b2 - b1) is the
kernel's time per frame without the call's fixed cost (streams, launch, drain, and the model of every destination pixel, which is
evaluated once per workgroup and call), reported as ``*_call_fixed_ms``.  ``*_us_per_out_MB`` is the slope per 10^6 bytes written,
which is what compares outputs of different sizes; ``warp_over_undistort`` is the ratio of the two slopes at equal output size.
host: the whole ``plane_view`` call on pageable numpy frames into a numpy output (staging copies both ways included).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lasercalib_amd import _native, imaging  # noqa: E402


def timed(fn, reps):
    fn()                                                     # warm-up
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3208x2200x3")
    ap.add_argument("--frames", default="32,128")
    ap.add_argument("--grid", type=int, default=2000)
    ap.add_argument("--host-frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_timing.jsonl"))
    a = ap.parse_args()
    import torch
    W, H, C = (int(v) for v in a.size.split("x"))
    b1, b2 = (int(v) for v in a.frames.split(","))
    assert _native.device_count() > 0, "time_warp.py needs the GPU"
    frame_bytes = W * H * C
    assert b1 * frame_bytes > (256 << 20) and b2 > b1, "batches must exceed the 256 MiB Infinity Cache"

    f = 1780.0 * W / 3208
    row11 = np.array([2.9, 0.0, 0.0, 30.0, -20.0, 2500.0, f, 3.6e-4, -1.4e-2, (W - 1) / 2 + 3.3, (H - 1) / 2 - 2.6])
    lens = imaging.Lens.from_camera_row(row11)
    G = a.grid
    grid = imaging.PlaneGrid.z_plane(0.0, (-0.75 * G, 0.75 * G), (-0.75 * G, 0.75 * G), 1.5)
    inv_k = imaging.virtual_camera_matrix(lens.camera_matrix)
    g = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.randint(0, 256, (b2, H, W, C), dtype=torch.uint8, device="cuda", generator=g)
    dst = torch.empty_like(frames)
    view = torch.empty((b2, G, G, C), dtype=torch.uint8, device="cuda")

    out = {"size": a.size, "frames": [b1, b2], "frame_bytes": frame_bytes, "grid": [G, G], "reps": a.reps}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    dst.copy_(frames)
    tc = []
    for _ in range(a.reps):
        ev[0].record()
        dst.copy_(frames)
        ev[1].record()
        ev[1].synchronize()
        tc.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    copy_frame_s = statistics.median(tc) / b2
    out.update({"d2d_copy_ms": round(copy_frame_s * b2 * 1e3, 4), "d2d_us_per_frame": round(copy_frame_s * 1e6, 2),
                "d2d_GBps": round(2 * frame_bytes / copy_frame_s * 1e-9, 1)})

    calls = {
        "plane_view": (lambda n: imaging.plane_view(frames[:n], row11, grid, out=view[:n]), G * G * C),
        "warp_inverse_k": (lambda n: imaging.warp_frames(frames[:n], lens, inv_k, (W, H), out=dst[:n]), frame_bytes),
        "undistort": (lambda n: imaging.undistort_frames(frames[:n], lens, out=dst[:n]), frame_bytes),
    }
    slope = {}
    for key, (call, out_bytes) in calls.items():
        t1 = timed(lambda: call(b1), a.reps)
        t2 = timed(lambda: call(b2), a.reps)
        per_frame = slope[key] = (t2 - t1) / (b2 - b1)
        out.update({f"{key}_call_ms": [round(t1 * 1e3, 4), round(t2 * 1e3, 4)], f"{key}_us_per_frame": round(per_frame * 1e6, 2),
                    f"{key}_frames_per_s": round(1.0 / per_frame, 1), f"{key}_us_per_out_MB": round(per_frame * 1e6 / (out_bytes * 1e-6), 3),
                    f"{key}_call_fixed_ms": round((t1 - per_frame * b1) * 1e3, 4)})
    out["warp_over_undistort"] = round(slope["warp_inverse_k"] / slope["undistort"], 4)
    out["plane_view_over_undistort_per_out_byte"] = round(slope["plane_view"] / (G * G * C) / (slope["undistort"] / frame_bytes), 4)
    flags = imaging.plane_view(frames[:0], row11, grid, want_flags=True)[1]
    out["plane_view_outside_fraction"] = round(float(np.mean((flags & imaging.SBA_UNDIST_OUTSIDE) != 0)), 4)
    del dst, frames, view

    hb = a.host_frames
    host = np.random.default_rng(0).integers(0, 256, size=(hb, H, W, C), dtype=np.uint8)
    hout = np.empty((hb, G, G, C), np.uint8)
    th = timed(lambda: imaging.plane_view(host, row11, grid, out=hout), max(3, a.reps // 2))
    out.update({"host_frames": hb, "host_call_ms": round(th * 1e3, 3), "host_frames_per_s": round(hb / th, 1),
                "host_GBps_in": round(hb * frame_bytes / th * 1e-9, 2), "host_GBps_out": round(hb * G * G * C / th * 1e-9, 2)})
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
