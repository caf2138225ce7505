"""Time sba_frames_to_yuv on full-size frames; one JSON line per run, appended (does not touch bench.py).

    python tools/time_yuv.py [--size 3208x2200] [--frames 32,128] [--host-frames 16] [--reps 5] [--out profiles/yuv_timing.jsonl]

The frames are uniform random bytes; the conversion's own work does not depend on the values.  Every rate of (a) is the slope
(t2 - t1) / (b2 - b1) between two batch sizes, both far larger than the 256 MiB Infinity Cache: the time per frame without a
call's fixed cost, which is reported as ``*_call_fixed_ms``.

(a) on device-resident BGR frames into device-resident planes: BGR -> NV12 and BGR -> I420, each with nearest and with averaged
    chroma.  ``*_GBps`` counts the bytes read (3 a pixel) plus the bytes written (1.5).  Next to them, in the same run:
    * ``copy_*``: ``dst.copy_(src)`` of as many bytes read plus written, under HIP events; ``*_over_copy`` is copy time / kernel
      time (1 = as fast as a copy);
    * ``convert_nv12_bgr_*``: sba_convert_frames NV12 -> BGR, the way in, which moves the same 4.5 bytes per pixel.
(b) ``imaging.undistort_frames`` on ``--host-frames`` pageable host frames, returning BGR against returning NV12
    (``out_pixel_format="nv12"``): the whole call, upload and download included.
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
    ap.add_argument("--size", default="3208x2200")
    ap.add_argument("--frames", default="32,128")
    ap.add_argument("--host-frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_timing.jsonl"))
    a = ap.parse_args()
    import torch
    W, H = (int(v) for v in a.size.split("x"))
    b1, b2 = (int(v) for v in a.frames.split(","))
    assert _native.device_count() > 0, "time_yuv.py needs the GPU"
    assert W % 2 == 0 and H % 2 == 0, "the stacked layouts timed here need even sizes"
    px = W * H
    assert b1 * px * 3 // 2 > (256 << 20) and b2 > b1, "batches must exceed the 256 MiB Infinity Cache"
    moved = px * 3 + px * 3 // 2                             # bytes read + written per frame, either way

    g = torch.Generator(device="cuda").manual_seed(0)
    bgr = torch.randint(0, 256, (b2, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    yuv = torch.empty((b2, H * 3 // 2, W), dtype=torch.uint8, device="cuda")
    row = {"size": a.size, "frames": [b1, b2], "pixels": px, "reps": a.reps, "bytes_per_frame": moved}

    def slope(key, fn):
        t1, t2 = timed(lambda: fn(b1), a.reps), timed(lambda: fn(b2), a.reps)
        per = (t2 - t1) / (b2 - b1)
        row.update({f"{key}_call_ms": [round(t1 * 1e3, 4), round(t2 * 1e3, 4)], f"{key}_frames_per_s": round(1.0 / per, 1),
                    f"{key}_us_per_frame": round(per * 1e6, 2), f"{key}_GBps": round(moved / per * 1e-9, 1),
                    f"{key}_call_fixed_ms": round((t1 - per * b1) * 1e3, 4)})
        return per

    per = {}
    for fmt in ("nv12", "i420"):
        for chroma in ("nearest", "average"):
            key = f"bgr_{fmt}_{chroma}"
            per[key] = slope(key, lambda n: imaging.frames_to_yuv(bgr[:n], fmt, chroma=chroma, out=yuv[:n]))
    # the way in on the same buffers: the planes just written back into the frames' memory
    nv12 = imaging.frames_to_yuv(bgr, "nv12", out=yuv)
    per["convert_nv12_bgr"] = slope("convert_nv12_bgr", lambda n: imaging.convert_frames(nv12[:n], "nv12", out_format="bgr", out=bgr[:n]))
    # the yardstick: a copy that reads and writes as many bytes, i.e. of moved / 2 bytes per frame
    n = b2 * moved // 2
    flat = bgr.reshape(-1)
    ca, cb = flat[:n], yuv.reshape(-1)[:n] if yuv.numel() >= n else torch.empty(n, dtype=torch.uint8, device="cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    cb.copy_(ca)
    tc = []
    for _ in range(a.reps):
        ev[0].record()
        cb.copy_(ca)
        ev[1].record()
        ev[1].synchronize()
        tc.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    copy_per = statistics.median(tc) / b2
    row.update({"copy_us_per_frame": round(copy_per * 1e6, 2), "copy_GBps": round(moved / copy_per * 1e-9, 1)})
    for key, p in per.items():
        row[f"{key}_over_copy"] = round(copy_per / p, 3)
        row[f"{key}_over_convert"] = round(per["convert_nv12_bgr"] / p, 3)
    del ca, cb, flat, nv12, yuv

    # (b) from the host and back: undistorted frames returned as BGR and as NV12
    nh = a.host_frames
    host = bgr[:nh].cpu().numpy()
    del bgr
    torch.cuda.empty_cache()
    lens = imaging.Lens(2400.0, 2400.0, W / 2 - 0.5, H / 2 - 0.5, -0.12, 0.03, 0.0005, -0.0004, 0.0)
    out_bgr, out_nv12 = np.empty((nh, H, W, 3), np.uint8), np.empty((nh, H * 3 // 2, W), np.uint8)
    want = imaging.frames_to_yuv(imaging.undistort_frames(host, lens), "nv12")
    assert np.array_equal(imaging.undistort_frames(host, lens, out_pixel_format="nv12", out=out_nv12), want)
    reps = max(3, a.reps // 2 + 1)
    t_bgr = timed(lambda: imaging.undistort_frames(host, lens, out=out_bgr), reps)
    t_nv12 = timed(lambda: imaging.undistort_frames(host, lens, out_pixel_format="nv12", out=out_nv12), reps)
    row.update({"undistort_host_frames": nh, "undistort_host_bgr_ms": round(t_bgr * 1e3, 3), "undistort_host_nv12_ms": round(t_nv12 * 1e3, 3),
                "undistort_host_bgr_frames_per_s": round(nh / t_bgr, 1), "undistort_host_nv12_frames_per_s": round(nh / t_nv12, 1),
                "undistort_host_nv12_over_bgr": round(t_bgr / t_nv12, 3)})
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
