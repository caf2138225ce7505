"""Time sba_refine_corners on full-size frames; one JSON line per run, appended (does not touch bench.py).

    python tools/time_corners.py [--size 3208x2200x3] [--frames 32,128] [--corners 600] [--host-frames 8] [--reps 7] [--label TEXT]
                                 [--out profiles/corners_timing.jsonl]

The frames hold a checkerboard of 60-pixel squares turned by 0.5 rad, shifted from frame to frame, with soft edges; every frame
gets ``--corners`` of its lattice corners, each started up to 1.5 px off, at the reference's settings (window 3 x 3, 200
iterations, eps 1e-5, the grey value of BGR frames).

* device-resident frames: the call is timed at two batch sizes; the slope (t2 - t1) / (frames2 - frames1) is the time per
  frame without the call's fixed cost.  Every timing is the median of ``--reps`` calls; ``*_spread`` is (min, max) of them.
  A call reads only the patches under its corners, so unlike the streaming frame calls it does not depend on the size of a frame.
* ``host``: the same call on pageable numpy frames, staging copies included: here every byte of every frame crosses the bus for
  the sake of 600 patches.
* ``oracle``: the numpy restatement of the rule (tests/test_corners_host.py) on the host, on the first 100 corners of frame 0
  (forming the grey plane of the whole frame is in its time), whose results the device call must equal bit for bit before
  anything is timed.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from lasercalib_amd import _native, imaging  # noqa: E402

Q, THETA = 60.0, 0.5


def timed(fn, reps):
    fn()                                                     # warm-up
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t), min(t), max(t)


def lattice_corners(W, H, shift, n, rng):
    """n lattice corners of the board shifted by `shift` pixels in x that lie 12 px inside the frame, each moved by up to 1.5 px."""
    c, s = math.cos(THETA), math.sin(THETA)
    k = int(math.hypot(W, H) / Q) + 2
    i, j = np.meshgrid(np.arange(-k, k + 1), np.arange(-k, k + 1))
    x, y = shift + Q * (i * c - j * s).ravel(), Q * (i * s + j * c).ravel()
    keep = (x > 12) & (x < W - 13) & (y > 12) & (y < H - 13)
    pts = np.stack([x[keep], y[keep]], axis=1)
    assert len(pts) >= n, "the frame holds fewer corners than asked for"
    pts = pts[rng.choice(len(pts), size=n, replace=False)]
    return pts + rng.uniform(-1.5, 1.5, size=pts.shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3208x2200x3")
    ap.add_argument("--frames", default="32,128")
    ap.add_argument("--corners", type=int, default=600)
    ap.add_argument("--host-frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corners_timing.jsonl"))
    a = ap.parse_args()
    import torch
    from test_corners_host import refine_corners_oracle
    W, H, C = (int(v) for v in a.size.split("x"))
    b1, b2 = (int(v) for v in a.frames.split(","))
    assert _native.device_count() > 0, "time_corners.py needs the GPU"
    assert b2 > b1

    frames = torch.empty((b2, H, W, C), dtype=torch.uint8, device="cuda")
    xs, ys = torch.arange(W, device="cuda", dtype=torch.float32)[None, :], torch.arange(H, device="cuda", dtype=torch.float32)[:, None]
    c, s = math.cos(THETA), math.sin(THETA)
    rng = np.random.default_rng(0)
    corners = []
    for f in range(b2):
        shift = 3.37 * f
        d1, d2 = (xs - shift) * c + ys * s, -(xs - shift) * s + ys * c
        board = torch.tanh(12.0 * torch.sin(math.pi / Q * d1)) * torch.tanh(12.0 * torch.sin(math.pi / Q * d2))
        frames[f] = (125.0 + 85.0 * board).round().to(torch.uint8)[:, :, None]
        corners.append(lattice_corners(W, H, shift, a.corners, rng))
    torch.cuda.synchronize()

    row = {"size": a.size, "frames": [b1, b2], "corners_per_frame": a.corners, "reps": a.reps, "label": a.label}
    first = frames[:1].cpu().numpy()                          # the results are right before they are timed
    t0 = time.perf_counter()
    want = refine_corners_oracle(first[0], corners[0][:100])
    row["oracle_us_per_corner"] = round((time.perf_counter() - t0) / 100 * 1e6, 1)
    got = imaging.refine_corners(frames[:1], [corners[0][:100]])
    for g, w in zip((got.xy, got.status, got.iterations, got.tensor), want):
        assert np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g, w.view(np.uint64) if w.dtype == np.float64 else w)

    res = imaging.refine_corners(frames, corners)
    row.update({"ok_share": round(float(res.ok.mean()), 4), "mean_iterations": round(float(res.iterations.mean()), 2),
                "max_iterations": int(res.iterations.max())})
    (t1, lo1, hi1), (t2, lo2, hi2) = (timed(lambda: imaging.refine_corners(frames[:b], corners[:b]), a.reps) for b in (b1, b2))
    per_frame = (t2 - t1) / (b2 - b1)
    row.update({"device_call_ms": [round(t1 * 1e3, 4), round(t2 * 1e3, 4)],
                "device_call_ms_spread": [[round(lo1 * 1e3, 4), round(hi1 * 1e3, 4)], [round(lo2 * 1e3, 4), round(hi2 * 1e3, 4)]],
                "device_us_per_frame": round(per_frame * 1e6, 3),
                "device_us_per_frame_spread": [round((lo2 - hi1) / (b2 - b1) * 1e6, 3), round((hi2 - lo1) / (b2 - b1) * 1e6, 3)],
                "device_ns_per_corner": round(per_frame / a.corners * 1e9, 2),
                "device_call_fixed_ms": round((t1 - per_frame * b1) * 1e3, 4)})
    hb = a.host_frames
    host = frames[:hb].cpu().numpy()
    th, lo, hi = timed(lambda: imaging.refine_corners(host, corners[:hb]), max(3, a.reps // 2))
    row.update({"host_frames": hb, "host_call_ms": round(th * 1e3, 3), "host_call_ms_spread": [round(lo * 1e3, 3), round(hi * 1e3, 3)],
                "host_us_per_frame": round(th / hb * 1e6, 1)})
    row["oracle_us_per_frame"] = round(row["oracle_us_per_corner"] * a.corners, 1)
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
