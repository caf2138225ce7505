"""Time sba_convert_frames on full-size frames; one JSON line per run, appended (does not touch bench.py).

    python tools/time_convert.py [--size 3208x2200] [--frames 32,128] [--torch-frames 4] [--reps 5] [--out profiles/convert_timing.jsonl]

The video is dark with a moving bright green dot, the detectors' usual case; the conversion's own work does not depend on the
values.  Every rate is the slope (t2 - t1) / (b2 - b1) between two batch sizes, both far larger than the 256 MiB Infinity Cache:
the time per frame without a call's fixed cost, which is reported as ``*_call_fixed_ms``.

(a) on device-resident frames into a device-resident output: NV12 -> G plane, NV12 -> BGR, I420 -> BGR.  ``*_GBps`` counts the
    bytes read (1.5 a pixel) plus the bytes written (1 or 3).  Next to each, in the same run:
    * ``*_copy_*``: ``dst.copy_(src)`` of as many bytes read plus written, under HIP events -- the yardstick; ``*_over_copy`` is
      copy time / kernel time (1 = as fast as a copy);
    * ``*_torch_*``: the same conversion written in torch element-wise ops (int32 tensors, the same integers, checked equal to
      the kernel's bytes here), on ``--torch-frames`` frames.
(b) ``find_laser_dots`` on host NV12 frames (``pixel_format="nv12"``: upload, conversion to the G plane on the device, detector)
    against ``find_laser_dots`` on the same video as host BGR frames (upload, detector), both pageable numpy arrays.
(c) what the one-chunk intermediate plane costs: ``find_laser_dots`` on device NV12 frames against the detector alone on the
    device G plane.
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
from lasercalib_amd import feature_detection as fd  # noqa: E402


def timed(fn, reps):
    fn()                                                     # warm-up
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t)


def torch_convert(torch, y, u, v, out_format, m=_native.YUV_BT601):
    """The header's rule in torch element-wise ops; y (B, H, W), u and v (B, ceil(H / 2), ceil(W / 2)) uint8 tensors."""
    H, W = y.shape[1:]
    y_offset, cy, cvr, cug, cvg, cub = m
    up = lambda c: c.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)[:, :H, :W].to(torch.int32) - 128      # noqa: E731
    U, V = up(u), up(v)
    l = (y.to(torch.int32) - y_offset).clamp_(min=0) * cy
    fin = lambda s: ((s + (1 << 19)) >> 20).clamp_(0, 255).to(torch.uint8)      # noqa: E731
    if out_format == "g":
        return fin(l + cug * U + cvg * V)
    return torch.stack((fin(l + cub * U), fin(l + cug * U + cvg * V), fin(l + cvr * V)), dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3208x2200")
    ap.add_argument("--frames", default="32,128")
    ap.add_argument("--torch-frames", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convert_timing.jsonl"))
    a = ap.parse_args()
    import torch
    W, H = (int(v) for v in a.size.split("x"))
    b1, b2 = (int(v) for v in a.frames.split(","))
    assert _native.device_count() > 0, "time_convert.py needs the GPU"
    assert W % 2 == 0 and H % 2 == 0, "the stacked layouts timed here need even sizes"
    px = W * H
    assert b1 * px * 3 // 2 > (256 << 20) and b2 > b1, "batches must exceed the 256 MiB Infinity Cache"

    # the video: dark, a little noise, a green dot of radius 6 that moves; built as NV12 / I420 on the device
    g = torch.Generator(device="cuda").manual_seed(0)
    y = torch.randint(16, 40, (b2, H, W), dtype=torch.uint8, device="cuda", generator=g)
    u = torch.randint(120, 136, (b2, H // 2, W // 2), dtype=torch.uint8, device="cuda", generator=g)
    v = torch.randint(120, 136, (b2, H // 2, W // 2), dtype=torch.uint8, device="cuda", generator=g)
    for f in range(b2):
        r, c = 200 + (37 * f) % (H - 400), 200 + (91 * f) % (W - 400)
        y[f, r - 6:r + 6, c - 6:c + 6] = 200
        u[f, r // 2 - 3:r // 2 + 3, c // 2 - 3:c // 2 + 3] = 60
        v[f, r // 2 - 3:r // 2 + 3, c // 2 - 3:c // 2 + 3] = 50
    nv12 = torch.cat((y.reshape(b2, -1), torch.stack((u, v), dim=-1).reshape(b2, -1)), dim=1).reshape(b2, H * 3 // 2, W)
    i420 = torch.cat((y.reshape(b2, -1), u.reshape(b2, -1), v.reshape(b2, -1)), dim=1).reshape(b2, H * 3 // 2, W)
    del y, u, v

    row = {"size": a.size, "frames": [b1, b2], "pixels": px, "reps": a.reps}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    tf = a.torch_frames
    cases = (("nv12_g", nv12, "nv12", "g", 1), ("nv12_bgr", nv12, "nv12", "bgr", 3), ("i420_bgr", i420, "i420", "bgr", 3))
    for key, src, fmt, out_format, C in cases:
        dst = torch.empty((b2, H, W) if C == 1 else (b2, H, W, C), dtype=torch.uint8, device="cuda")
        t1 = timed(lambda: imaging.convert_frames(src[:b1], fmt, out_format=out_format, out=dst[:b1]), a.reps)
        t2 = timed(lambda: imaging.convert_frames(src, fmt, out_format=out_format, out=dst), a.reps)
        per = (t2 - t1) / (b2 - b1)
        moved = px * 3 // 2 + px * C                          # bytes read + written per frame
        # the yardstick: a copy that reads and writes as many bytes, i.e. of moved / 2 bytes per frame
        n = b2 * moved // 2
        pool = dst.reshape(-1) if dst.numel() >= 2 * n else torch.empty(2 * n, dtype=torch.uint8, device="cuda")
        ca, cb = pool[:n], pool[n:2 * n]
        cb.copy_(ca)
        tc = []
        for _ in range(a.reps):
            ev[0].record()
            cb.copy_(ca)
            ev[1].record()
            ev[1].synchronize()
            tc.append(ev[0].elapsed_time(ev[1]) * 1e-3)
        copy_per = statistics.median(tc) / b2
        del pool, ca, cb
        # the same conversion in torch element-wise ops, and that it gives the kernel's bytes
        got = imaging.convert_frames(src[:tf], fmt, out_format=out_format, out=dst[:tf])
        flat = src[:tf].reshape(tf, -1)
        yy = flat[:, :px].reshape(tf, H, W)
        if fmt == "nv12":
            pair = flat[:, px:].reshape(tf, H // 2, W // 2, 2)
            uu, vv = pair[..., 0], pair[..., 1]
        else:
            uu, vv = flat[:, px:px + px // 4].reshape(tf, H // 2, W // 2), flat[:, px + px // 4:].reshape(tf, H // 2, W // 2)
        assert torch.equal(torch_convert(torch, yy, uu, vv, out_format), got), f"{key}: torch ops and kernel differ"

        def torch_run():
            torch_convert(torch, yy, uu, vv, out_format)
            torch.cuda.synchronize()
        tt = timed(torch_run, a.reps) / tf
        row.update({f"{key}_call_ms": [round(t1 * 1e3, 4), round(t2 * 1e3, 4)], f"{key}_frames_per_s": round(1.0 / per, 1),
                    f"{key}_us_per_frame": round(per * 1e6, 2), f"{key}_GBps": round(moved / per * 1e-9, 1),
                    f"{key}_call_fixed_ms": round((t1 - per * b1) * 1e3, 4),
                    f"{key}_copy_us_per_frame": round(copy_per * 1e6, 2), f"{key}_copy_GBps": round(moved / copy_per * 1e-9, 1),
                    f"{key}_over_copy": round(copy_per / per, 3),
                    f"{key}_torch_us_per_frame": round(tt * 1e6, 1), f"{key}_torch_over_kernel": round(tt / per, 1)})
        del dst, got
    del i420

    # (c) the intermediate plane: detector on device NV12 frames against the detector alone on the device G plane
    plane = imaging.convert_frames(nv12, "nv12", out_format="g")
    for key, fn in (("dots_device_nv12", lambda n: fd.find_laser_dots(nv12[:n], threshold=50, channel=1, pixel_format="nv12")),
                    ("dots_device_plane", lambda n: fd.find_laser_dots(plane[:n], threshold=50, channel=0))):
        t1, t2 = timed(lambda: fn(b1), a.reps), timed(lambda: fn(b2), a.reps)
        per = (t2 - t1) / (b2 - b1)
        row.update({f"{key}_call_ms": [round(t1 * 1e3, 4), round(t2 * 1e3, 4)], f"{key}_us_per_frame": round(per * 1e6, 2),
                    f"{key}_frames_per_s": round(1.0 / per, 1)})
    want = fd.find_laser_dots(plane, threshold=50, channel=0)
    assert np.all(want.status == fd.SBA_DOT_OK), "the video's dot is not found"
    del plane

    # (b) from the host: NV12 frames as decoded against the same video as BGR frames
    host_nv12 = nv12.cpu().numpy()
    host_bgr = imaging.convert_frames(nv12, "nv12", out_format="bgr").cpu().numpy()
    del nv12
    torch.cuda.empty_cache()
    got = fd.find_laser_dots(host_nv12, threshold=50, channel=1, pixel_format="nv12")
    ref = fd.find_laser_dots(host_bgr, threshold=50, channel=1)
    assert all(np.array_equal(getattr(got, k), getattr(ref, k), equal_nan=True) for k in ("sums", "box", "centroid", "status"))
    assert all(np.array_equal(getattr(got, k), getattr(want, k), equal_nan=True) for k in ("sums", "box", "centroid", "status"))
    reps = max(3, a.reps // 2 + 1)
    for key, arr, kw, nbytes in (("dots_host_nv12", host_nv12, dict(pixel_format="nv12"), px * 3 // 2), ("dots_host_bgr", host_bgr, {}, px * 3)):
        t1 = timed(lambda: fd.find_laser_dots(arr[:b1], threshold=50, channel=1, **kw), reps)
        t2 = timed(lambda: fd.find_laser_dots(arr, threshold=50, channel=1, **kw), reps)
        per = (t2 - t1) / (b2 - b1)
        row.update({f"{key}_call_ms": [round(t1 * 1e3, 3), round(t2 * 1e3, 3)], f"{key}_frames_per_s": round(1.0 / per, 1),
                    f"{key}_upload_GBps": round(nbytes / per * 1e-9, 2)})
    row["dots_host_nv12_over_bgr"] = round(row["dots_host_nv12_frames_per_s"] / row["dots_host_bgr_frames_per_s"], 3)
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
