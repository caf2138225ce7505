"""Time sba_undistort_yuv on full-size frames; one JSON line per run, appended (does not touch bench.py).

    python tools/time_undistort_yuv.py [--size 3208x2200] [--frames 32,128] [--host-frames 16] [--reps 5]
                                       [--out profiles/undistort_yuv_timing.jsonl]

The frames are uniform random bytes; the work does not depend on the values.  Every rate on device frames is the slope
(t2 - t1) / (b2 - b1) between two batch sizes, both far larger than the 256 MiB Infinity Cache: the time per frame without a
call's fixed cost, which is reported as ``*_call_fixed_ms``.  In ONE run, on device-resident NV12 frames into device-resident
NV12 frames under a barrel lens:

(a) ``yuv``: the new call, ``imaging.undistort_yuv``; next to it ``yuv_i420`` (planar chroma on both sides) and ``yuv_nearest``;
(b) ``three_calls``: what it replaces, ``convert_frames -> undistort_frames -> frames_to_yuv`` device to device, and its three
    stages by themselves (``stage_convert``, ``stage_undistort_bgr``: k_undistort<3> alone, ``stage_to_yuv``);
(c) ``copy``: ``dst.copy_(src)`` of as many bytes as (a) reads plus writes (3 a pixel), under HIP events.
(a) and (b) are measured twice, alternately (``yuv_0``, ``three_calls_0``, ``yuv_1``, ``three_calls_1``), and the faster round of
each is what the ratios use.
``yuv_over_three_calls`` is time (b) / time (a) (above 1: the new call is faster), ``yuv_over_copy`` is time (c) / time (a).
The bytes of (a) are compared with nothing here: tests/test_gpu_undistort_yuv.py pins them to the rule; its luma plane is
checked against the luma of ``undistort_frames`` on the Y plane before anything is timed.

From the host: ``--host-frames`` pageable NV12 frames in and NV12 out through the new call, against what a user did before from
BGR frames, ``undistort_frames(host BGR, out_pixel_format="nv12")``: the whole call, upload and download included.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort_yuv_timing.jsonl"))
    a = ap.parse_args()
    import torch
    W, H = (int(v) for v in a.size.split("x"))
    b1, b2 = (int(v) for v in a.frames.split(","))
    assert _native.device_count() > 0, "time_undistort_yuv.py needs the GPU"
    assert W % 2 == 0 and H % 2 == 0, "the stacked layouts timed here need even sizes"
    px = W * H
    assert b1 * px * 3 // 2 > (256 << 20) and b2 > b1, "batches must exceed the 256 MiB Infinity Cache"
    moved = px * 3                                           # bytes (a) reads plus writes per frame: 1.5 + 1.5 a pixel
    lens = imaging.Lens(2400.0, 2400.0, W / 2 - 0.5, H / 2 - 0.5, -0.12, 0.03, 0.0005, -0.0004, 0.0)

    g = torch.Generator(device="cuda").manual_seed(0)
    src = torch.randint(0, 256, (b2, H * 3 // 2, W), dtype=torch.uint8, device="cuda", generator=g)
    dst = torch.empty_like(src)
    bgr, und = (torch.empty((b2, H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
    row = {"size": a.size, "frames": [b1, b2], "pixels": px, "reps": a.reps, "bytes_per_frame": moved}

    # before anything is timed: the luma of the new call is the one-channel rule of the existing one
    one = imaging.undistort_frames(src[:2, :H], lens, border_value=16)
    assert torch.equal(imaging.undistort_yuv(src[:2], "nv12", lens)[:, :H], one), "luma differs from undistort_frames on the Y plane"

    def slope(key, fn):
        t1, t2 = timed(lambda: fn(b1), a.reps), timed(lambda: fn(b2), a.reps)
        per = (t2 - t1) / (b2 - b1)
        row.update({f"{key}_call_ms": [round(t1 * 1e3, 4), round(t2 * 1e3, 4)], f"{key}_frames_per_s": round(1.0 / per, 1),
                    f"{key}_us_per_frame": round(per * 1e6, 2), f"{key}_call_fixed_ms": round((t1 - per * b1) * 1e3, 4)})
        return per

    def three_calls(n):
        imaging.convert_frames(src[:n], "nv12", out=bgr[:n])
        imaging.undistort_frames(bgr[:n], lens, out=und[:n])
        imaging.frames_to_yuv(und[:n], "nv12", out=dst[:n])

    per = {}
    # (a) and (b) alternate, so that neither has the quieter half of the run
    for rnd in range(2):
        per[f"yuv_{rnd}"] = slope(f"yuv_{rnd}", lambda n: imaging.undistort_yuv(src[:n], "nv12", lens, out=dst[:n]))
        per[f"three_calls_{rnd}"] = slope(f"three_calls_{rnd}", three_calls)
    per["yuv"], per["three_calls"] = (min(per[f"{k}_0"], per[f"{k}_1"]) for k in ("yuv", "three_calls"))
    per["yuv_i420"] = slope("yuv_i420", lambda n: imaging.undistort_yuv(src[:n], "i420", lens, out=dst[:n]))
    per["yuv_nearest"] = slope("yuv_nearest", lambda n: imaging.undistort_yuv(src[:n], "nv12", lens, interpolation="nearest", out=dst[:n]))
    per["stage_convert"] = slope("stage_convert", lambda n: imaging.convert_frames(src[:n], "nv12", out=bgr[:n]))
    per["stage_undistort_bgr"] = slope("stage_undistort_bgr", lambda n: imaging.undistort_frames(bgr[:n], lens, out=und[:n]))
    per["stage_to_yuv"] = slope("stage_to_yuv", lambda n: imaging.frames_to_yuv(und[:n], "nv12", out=dst[:n]))
    row.update({"yuv_us_per_frame": round(per["yuv"] * 1e6, 2), "three_calls_us_per_frame": round(per["three_calls"] * 1e6, 2),
                "yuv_GBps": round(moved / per["yuv"] * 1e-9, 1)})

    # (c) the yardstick: a copy that reads and writes as many bytes, i.e. of moved / 2 bytes per frame
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    dst.copy_(src)
    tc = []
    for _ in range(a.reps):
        ev[0].record()
        dst.copy_(src)
        ev[1].record()
        ev[1].synchronize()
        tc.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    copy_per = statistics.median(tc) / b2
    row.update({"copy_us_per_frame": round(copy_per * 1e6, 2), "copy_GBps": round(moved / copy_per * 1e-9, 1),
                "yuv_over_three_calls": round(per["three_calls"] / per["yuv"], 3), "yuv_over_copy": round(copy_per / per["yuv"], 3),
                "yuv_over_undistort_bgr_stage": round(per["stage_undistort_bgr"] / per["yuv"], 3)})

    # from the host and back: NV12 in, NV12 out, against BGR in, NV12 out through the three-stage route
    nh = a.host_frames
    host_yuv, host_bgr = src[:nh].cpu().numpy(), bgr[:nh].cpu().numpy()
    del src, dst, bgr, und
    torch.cuda.empty_cache()
    out_a, out_b = np.empty((nh, H * 3 // 2, W), np.uint8), np.empty((nh, H * 3 // 2, W), np.uint8)
    reps = max(3, a.reps // 2 + 1)
    t_yuv = timed(lambda: imaging.undistort_yuv(host_yuv, "nv12", lens, out=out_a), reps)
    t_bgr = timed(lambda: imaging.undistort_frames(host_bgr, lens, out_pixel_format="nv12", out=out_b), reps)
    row.update({"host_frames": nh, "host_yuv_ms": round(t_yuv * 1e3, 3), "host_bgr_to_nv12_ms": round(t_bgr * 1e3, 3),
                "host_yuv_frames_per_s": round(nh / t_yuv, 1), "host_bgr_to_nv12_frames_per_s": round(nh / t_bgr, 1),
                "host_yuv_over_bgr_to_nv12": round(t_bgr / t_yuv, 3)})
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
