"""Time sba_detect_dots on full-size frames; one JSON line per run, appended (does not touch bench.py).

    python tools/time_detect.py [--size 3208x2200x3] [--frames 32,128] [--host-frames 16] [--reps 10] [--out profiles/detect_timing.jsonl]

Frames are dark noise (0..30 counts, all channels) with one Gaussian spot each, threshold 50: what a recording looks like.

* kernel: the call on device-resident frames is timed at two batch sizes (both far larger than the 256 MiB Infinity Cache, so
  the frames come from HBM); the slope (t2 - t1) / (bytes2 - bytes1) is the kernels' rate without the call's fixed cost (result
  buffers, two streams, read-back), which is reported as ``call_fixed_ms``.  ``bright_*``: the same on all-255 frames, where
  no vector takes the dark fast path.
* d2d: ``dst.copy_(src)`` of the larger batch under HIP events in the same run -- the yardstick.  Its read rate is bytes / time
  (it also writes as many bytes); ``kernel_over_copy_read`` is the kernel's rate as a fraction of it.
* host: the whole call on pageable numpy frames (staging copies included), frames/s and bytes/s: bound by the host-to-device
  copy, not by the kernel.
* numpy_ms_per_frame: the reference's detector restated in numpy (threshold, then the three moments) on one frame on the host.
  It stands in for OpenCV, which is not installed here; cv.threshold + cv.moments are a single fused pass each and faster.
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

from lasercalib_amd import _native  # noqa: E402


def numpy_detector(frame, thr):
    green = frame[:, :, 1]
    img = np.where(green > thr, 255, 0).astype(np.uint8).astype(np.float64)
    m00 = img.sum()
    if m00 == 0:
        return None
    m10 = (img.sum(axis=0) * np.arange(img.shape[1])).sum()
    m01 = (img.sum(axis=1) * np.arange(img.shape[0])).sum()
    return int(m01 / m00), int(m10 / m00)


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_timing.jsonl"))
    a = ap.parse_args()
    import torch
    W, H, C = (int(v) for v in a.size.split("x"))
    b1, b2 = (int(v) for v in a.frames.split(","))
    assert _native.device_count() > 0, "time_detect.py needs the GPU"
    frame_bytes = W * H * C
    assert b1 * frame_bytes > (256 << 20) and b2 >= 16 and b2 > b1, "batches must exceed the 256 MiB Infinity Cache"

    g = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.randint(0, 31, (b2, H, W, C), dtype=torch.uint8, device="cuda", generator=g)
    y, x = torch.meshgrid(torch.arange(33, device="cuda"), torch.arange(33, device="cuda"), indexing="ij")
    spot = (230.0 * torch.exp(-0.5 * ((x - 16.3) ** 2 + (y - 15.6) ** 2) / 2.0 ** 2)).round().clamp(0, 255).to(torch.uint8)
    for f in range(b2):
        x0, y0 = (37 * f) % (W - 40), (53 * f) % (H - 40)
        frames[f, y0:y0 + 33, x0:x0 + 33, 1] = torch.maximum(frames[f, y0:y0 + 33, x0:x0 + 33, 1], spot)
    ch = 1 if C > 1 else 0
    dots = _native.detect_dots(frames, threshold=50, channel=ch, max_extent=40)
    assert np.all(dots.status == _native.DOT_OK), dots.status

    row = {"size": a.size, "frames": [b1, b2], "frame_bytes": frame_bytes, "reps": a.reps}
    for name, src in (("kernel", frames), ("bright", None)):
        if src is None:
            frames.fill_(255)
            src = frames
        t1 = timed(lambda: _native.detect_dots(src[:b1], threshold=50, channel=ch), a.reps)
        t2 = timed(lambda: _native.detect_dots(src, threshold=50, channel=ch), a.reps)
        per_byte = (t2 - t1) / ((b2 - b1) * frame_bytes)
        row.update({f"{name}_call_ms": [round(t1 * 1e3, 4), round(t2 * 1e3, 4)], f"{name}_GBps": round(1e-9 / per_byte, 1),
                    f"{name}_frames_per_s": round(1.0 / (per_byte * frame_bytes), 1),
                    f"{name}_call_fixed_ms": round((t1 - per_byte * b1 * frame_bytes) * 1e3, 4),
                    f"{name}_call_GBps": round(b2 * frame_bytes / t2 * 1e-9, 1)})
        if name == "kernel":
            dst = torch.empty_like(frames)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            dst.copy_(frames)
            tc = []
            for _ in range(a.reps):
                ev[0].record()
                dst.copy_(frames)
                ev[1].record()
                ev[1].synchronize()
                tc.append(ev[0].elapsed_time(ev[1]) * 1e-3)
            copy_s = statistics.median(tc)
            row.update({"d2d_copy_ms": round(copy_s * 1e3, 4), "d2d_read_GBps": round(b2 * frame_bytes / copy_s * 1e-9, 1)})
            del dst
    row["kernel_over_copy_read"] = round(row["kernel_GBps"] / row["d2d_read_GBps"], 3)
    row["bright_over_copy_read"] = round(row["bright_GBps"] / row["d2d_read_GBps"], 3)

    hb = a.host_frames
    rng = np.random.default_rng(0)
    host = rng.integers(0, 31, size=(hb, H, W, C), dtype=np.uint8)
    host[:, 100:133, 200:233, ch] = spot.cpu().numpy()
    th = timed(lambda: _native.detect_dots(host, threshold=50, channel=ch), max(3, a.reps // 3))
    row.update({"host_frames": hb, "host_call_ms": round(th * 1e3, 3), "host_frames_per_s": round(hb / th, 1),
                "host_GBps": round(hb * frame_bytes / th * 1e-9, 2)})
    if C >= 3:
        tn = timed(lambda: numpy_detector(host[0], 50), 3)
        row["numpy_ms_per_frame"] = round(tn * 1e3, 2)
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
