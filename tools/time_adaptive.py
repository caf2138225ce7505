"""Time sba_adaptive_threshold on full-size frames; one JSON line per run, appended (does not touch bench.py).

    python tools/time_adaptive.py [--size 3208x2200] [--frames 32,128] [--host-frames 16] [--reps 7] [--label "run 1"]
                                  [--out profiles/adaptive_timing.jsonl]

Frames are uniform random bytes (the kernel's work does not depend on the values).

* kernel: the call on device-resident frames into device-resident masks is timed at two batch sizes (both far larger than the
  256 MiB Infinity Cache); the slope (t2 - t1) / (b2 - b1) is the time per frame without the call's fixed cost, which is reported
  as ``*_call_fixed_ms``.  Inputs: one-channel frames (``plane_*``) and BGR frames read as grey (``bgr_*``).  Window lists: ArUco's
  (3, 13, 23) in ONE call (``*_3win``), the same three windows as three calls (``*_3calls``), (23,) and (127,) alone.
  ``*_GBps`` counts the bytes the call reads and writes once: the frame and one byte per pixel and window.
* d2d: ``dst.copy_(src)`` under HIP events; ``*_over_copy`` is the time the copy needs for as many bytes as the call reads and
  writes (half of them read, half written, as a copy does) / the call's time: 1 = the copy's rate.
* torch: the same masks written with torch ops (``F.pad(mode="replicate")``, ``avg_pool2d`` of a float32 plane, rounding), what a
  caller would otherwise do; compared with the library's masks on one frame (float32 sums of window 23 are exact: < 2^24), timed
  on a few frames.
* host: the whole call on pageable numpy BGR frames into numpy masks.
* check: frame 0 and the last frame of the large batch equal an integer restatement of the rule in torch (int64 running sums,
  rule 4 in int64), so the timed kernel is also a right one.
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

ARUCO = (3, 13, 23)
DELTA = 7


def timed(fn, reps):
    fn()                                                     # warm-up
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t)


def gray_of(frames):
    import torch
    v, w = frames.to(torch.int32), _native.GRAY_BGR
    return ((v[..., 0] * w[0] + v[..., 1] * w[1] + v[..., 2] * w[2] + (1 << 14)) >> 15).to(torch.uint8)


def torch_rule(plane, b, delta):
    """The header's rule for (B, H, W) uint8 planes in torch, exactly: int64 running sums, the nearest integer in int64."""
    import torch
    r = b // 2
    x = torch.nn.functional.pad(plane[:, None].to(torch.float32), (r, r, r, r), mode="replicate")[:, 0].to(torch.int64)
    c = torch.nn.functional.pad(torch.cumsum(x, dim=2), (1, 0))
    rows = c[:, :, b:] - c[:, :, :-b]
    c = torch.nn.functional.pad(torch.cumsum(rows, dim=1), (0, 0, 1, 0))
    S = c[:, b:] - c[:, :-b]
    mean = (2 * S + b * b) // (2 * b * b)
    return torch.where(plane.to(torch.int64) - mean <= -delta, 255, 0).to(torch.uint8), mean.to(torch.uint8)


def torch_masks(plane, blocks, delta):
    """As a caller without the library would write it: float32 throughout."""
    import torch
    F = torch.nn.functional
    x = plane[:, None].to(torch.float32)
    out = []
    for b in blocks:
        r = b // 2
        mean = torch.round(F.avg_pool2d(F.pad(x, (r, r, r, r), mode="replicate"), b, stride=1))
        out.append(torch.where(x - mean <= -delta, 255, 0).to(torch.uint8)[:, 0])
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3208x2200")
    ap.add_argument("--frames", default="32,128")
    ap.add_argument("--host-frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_timing.jsonl"))
    a = ap.parse_args()
    import torch
    W, H = (int(v) for v in a.size.split("x"))
    b1, b2 = (int(v) for v in a.frames.split(","))
    assert _native.device_count() > 0, "time_adaptive.py needs the GPU"
    px = W * H
    assert b1 * px * 2 > (256 << 20) and b2 > b1, "batches must exceed the 256 MiB Infinity Cache"
    row = {"size": a.size, "frames": [b1, b2], "pixels": px, "reps": a.reps, "label": a.label}

    g = torch.Generator(device="cuda").manual_seed(0)
    bgr = torch.randint(0, 256, (b2, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    plane = gray_of(bgr[:8])
    plane = torch.cat([plane, torch.randint(0, 256, (b2 - 8, H, W), dtype=torch.uint8, device="cuda", generator=g)])

    dst = torch.empty_like(bgr)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    dst.copy_(bgr)
    tc = []
    for _ in range(a.reps):
        ev[0].record()
        dst.copy_(bgr)
        ev[1].record()
        ev[1].synchronize()
        tc.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    copy_s_per_byte = statistics.median(tc) / (2 * bgr.numel())             # per byte moved: read or written
    row.update({"d2d_GBps": round(1e-9 / copy_s_per_byte, 1)})
    del dst

    out = torch.empty((3, b2, H, W), dtype=torch.uint8, device="cuda")

    def call(f, blocks):
        _native.adaptive_threshold(f, blocks, (DELTA,) * len(blocks), channel=-1 if f.dim() == 4 else 0, out=out[:len(blocks), :f.shape[0]])

    def three_calls(f):
        for k, b in enumerate(ARUCO):
            _native.adaptive_threshold(f, (b,), (DELTA,), channel=-1 if f.dim() == 4 else 0, out=out[k:k + 1, :f.shape[0]])

    def slope(key, frames, fn, moved):
        t1, t2 = timed(lambda: fn(frames[:b1]), a.reps), timed(lambda: fn(frames), a.reps)
        per_frame = (t2 - t1) / (b2 - b1)
        row.update({f"{key}_call_ms": [round(t1 * 1e3, 4), round(t2 * 1e3, 4)], f"{key}_us_per_frame": round(per_frame * 1e6, 2),
                    f"{key}_GBps": round(moved / per_frame * 1e-9, 1), f"{key}_call_fixed_ms": round((t1 - per_frame * b1) * 1e3, 4),
                    f"{key}_over_copy": round(copy_s_per_byte * moved / per_frame, 3)})
        return per_frame

    for name, frames, C in (("plane", plane, 1), ("bgr", bgr, 3)):
        t3 = slope(f"{name}_3win", frames, lambda f: call(f, ARUCO), px * (C + 3))
        for k in (0, b2 - 1):                                # the timed call's masks of the first and the last frame
            src = frames[k:k + 1] if C == 1 else gray_of(frames[k:k + 1])
            for j, b in enumerate(ARUCO):
                assert torch.equal(out[j, k:k + 1], torch_rule(src, b, DELTA)[0]), f"{name}: window {b} of frame {k} differs from the rule"
        tc3 = slope(f"{name}_3calls", frames, three_calls, 3 * px * (C + 1))
        row[f"{name}_3calls_over_3win"] = round(tc3 / t3, 3)
        slope(f"{name}_23", frames, lambda f: call(f, (23,)), px * (C + 1))
        slope(f"{name}_127", frames, lambda f: call(f, (127,)), px * (C + 1))
        assert torch.equal(out[0, :1], torch_rule(frames[:1] if C == 1 else gray_of(frames[:1]), 127, DELTA)[0]), f"{name}: window 127 differs"
    row["checked_frames"] = [0, b2 - 1]

    tb = 4
    lib = _native.adaptive_threshold(plane[:1], ARUCO, (DELTA,) * 3, channel=0)[0]
    assert torch.equal(torch_masks(plane[:1], ARUCO, DELTA), lib), "the torch formulation differs"
    t_torch = timed(lambda: (torch_masks(plane[:tb], ARUCO, DELTA), torch.cuda.synchronize()), a.reps)
    row.update({"torch_frames": tb, "torch_us_per_frame": round(t_torch / tb * 1e6, 2),
                "torch_over_plane_3win": round(t_torch / tb / (row["plane_3win_us_per_frame"] * 1e-6), 2)})
    row["one_frame_ms"] = round(timed(lambda: call(bgr[:1], ARUCO), a.reps) * 1e3, 4)
    del bgr, plane, out
    torch.cuda.empty_cache()

    hb = a.host_frames
    host = np.random.default_rng(0).integers(0, 256, size=(hb, H, W, 3), dtype=np.uint8)
    masks = np.empty((3, hb, H, W), np.uint8)
    th = timed(lambda: _native.adaptive_threshold(host, ARUCO, (DELTA,) * 3, out=masks), max(3, a.reps // 2))
    row.update({"host_frames": hb, "host_call_ms": round(th * 1e3, 3), "host_us_per_frame": round(th / hb * 1e6, 1),
                "host_GBps_both_ways": round(hb * px * 6 / th * 1e-9, 2)})
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
