"""Time sba_undistort_frames on full-size frames; one JSON line per run, appended (does not touch bench.py).

    python tools/time_undistort.py [--size 3208x2200x3] [--frames 32,128] [--host-frames 16] [--reps 7] [--out profiles/undistort_timing.jsonl]

Frames are uniform random bytes (the kernel's work does not depend on the values).  Two lenses: the example rig's
(k1 = 3.6e-4, k2 = -1.4e-2: the picture hardly moves) and a strong barrel (k1 = -0.25, k2 = 0.05: a destination row bends over
~100 source rows), each with its own camera matrix as the new one, bilinear and nearest.

* kernel: the call on device-resident frames into a device-resident output is timed at two batch sizes (both far larger than the
  256 MiB Infinity Cache); the slope (t2 - t1) / (b2 - b1) is the kernel's time per frame without the call's fixed cost (streams,
  launch, drain), which is reported as ``*_call_fixed_ms``.  ``*_GBps`` counts the bytes read plus the bytes written.
* ``identity_*``: no distortion and the same matrix: one tap per pixel, read and written in order -- the kernel's own copy rate.
* d2d: ``dst.copy_(src)`` of the larger batch under HIP events in the same run -- the yardstick; ``*_over_copy`` is copy time /
  kernel time for the same bytes (1 = as fast as a copy).
* one_frame_ms: the call on a single frame, where the float64 model of every pixel is paid for one frame alone.
* host: the whole call on pageable numpy frames into a numpy output (staging copies both ways included).
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
    ap.add_argument("--host-frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort_timing.jsonl"))
    a = ap.parse_args()
    import torch
    W, H, C = (int(v) for v in a.size.split("x"))
    b1, b2 = (int(v) for v in a.frames.split(","))
    assert _native.device_count() > 0, "time_undistort.py needs the GPU"
    frame_bytes = W * H * C
    assert b1 * frame_bytes > (256 << 20) and b2 > b1, "batches must exceed the 256 MiB Infinity Cache"

    f, cx, cy = 2388.5 * W / 3208, (W - 1) / 2 + 3.3, (H - 1) / 2 - 2.6
    lenses = {"rig": imaging.Lens(f, f, cx, cy, 3.6e-4, -1.4e-2), "barrel": imaging.Lens(f, f, cx, cy, -0.25, 0.05),
              "identity": imaging.Lens(f, f, cx, cy)}
    g = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.randint(0, 256, (b2, H, W, C), dtype=torch.uint8, device="cuda", generator=g)
    dst = torch.empty_like(frames)

    row = {"size": a.size, "frames": [b1, b2], "frame_bytes": frame_bytes, "reps": a.reps}
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
    row.update({"d2d_copy_ms": round(copy_frame_s * b2 * 1e3, 4), "d2d_frames_per_s": round(1.0 / copy_frame_s, 1),
                "d2d_GBps": round(2 * frame_bytes / copy_frame_s * 1e-9, 1)})

    for name, lens in lenses.items():
        for interpolation in (("linear",) if name == "identity" else ("linear", "nearest")):
            key = f"{name}_{interpolation}"
            t1 = timed(lambda: imaging.undistort_frames(frames[:b1], lens, interpolation=interpolation, out=dst[:b1]), a.reps)
            t2 = timed(lambda: imaging.undistort_frames(frames, lens, interpolation=interpolation, out=dst), a.reps)
            per_frame = (t2 - t1) / (b2 - b1)
            row.update({f"{key}_call_ms": [round(t1 * 1e3, 4), round(t2 * 1e3, 4)], f"{key}_frames_per_s": round(1.0 / per_frame, 1),
                        f"{key}_us_per_frame": round(per_frame * 1e6, 2), f"{key}_GBps": round(2 * frame_bytes / per_frame * 1e-9, 1),
                        f"{key}_call_fixed_ms": round((t1 - per_frame * b1) * 1e3, 4), f"{key}_over_copy": round(copy_frame_s / per_frame, 3)})
    row["one_frame_ms"] = round(timed(lambda: imaging.undistort_frames(frames[:1], lenses["barrel"], out=dst[:1]), a.reps) * 1e3, 4)
    flags = imaging.undistort_frames(frames[:0], lenses["barrel"], want_flags=True)[1]
    row["barrel_outside_fraction"] = round(float(np.mean((flags & imaging.SBA_UNDIST_OUTSIDE) != 0)), 4)
    del dst, frames

    hb = a.host_frames
    host = np.random.default_rng(0).integers(0, 256, size=(hb, H, W, C), dtype=np.uint8)
    hout = np.empty_like(host)
    th = timed(lambda: imaging.undistort_frames(host, lenses["barrel"], out=hout), max(3, a.reps // 2))
    row.update({"host_frames": hb, "host_call_ms": round(th * 1e3, 3), "host_frames_per_s": round(hb / th, 1),
                "host_GBps_each_way": round(hb * frame_bytes / th * 1e-9, 2)})
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
