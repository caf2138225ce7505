"""Time sba_background_accumulate and sba_background_suppress on full-size frames; one JSON line per run, appended (does not
touch bench.py).

    python tools/time_background.py [--size 3208x2200x3] [--frames 32,128] [--host-frames 16] [--reps 7] [--out profiles/background_timing.jsonl]

Frames are those of tools/time_detect.py: dark noise of 0..30 counts with one Gaussian spot per frame (the kernels' work does
not depend on the values; sba_detect_dots' does, and this is its usual case).

* kernels: each call on device-resident frames is timed at two batch sizes (both far larger than the 256 MiB Infinity Cache);
  the slope (t2 - t1) / (b2 - b1) is the kernel's time per frame without the call's fixed cost, reported as ``*_call_fixed_ms``.
  ``accumulate_all`` keeps all four accumulators (on the device), ``accumulate_sum`` only the sum; ``suppress_gate`` /
  ``suppress_subtract`` write a device-resident one-channel output with a level and a mask.
* yardsticks of the SAME run: ``dots`` -- sba_detect_dots on the same frames, which reads the same bytes (``accumulate_*_over_dots``
  is dots time / accumulate time per frame: 1 = as fast); ``d2d`` -- ``dst.copy_(src)`` of the larger batch under HIP events
  (``suppress_*_over_copy`` compares the bytes moved per second: a suppress call reads C and writes 1 byte per pixel, the copy
  reads C and writes C); ``torch`` -- the statistics restated in torch element-wise ops on the smaller batch
  (``frames[..., c].to(int64).sum(0)``, the square sum, ``(... > t).sum(0)``, ``amax(0)``).
* host: the whole calls on pageable numpy frames (staging copies included).
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "background_timing.jsonl"))
    a = ap.parse_args()
    import torch
    W, H, C = (int(v) for v in a.size.split("x"))
    b1, b2 = (int(v) for v in a.frames.split(","))
    assert _native.device_count() > 0, "time_background.py needs the GPU"
    frame_bytes = W * H * C
    assert b1 * frame_bytes > (256 << 20) and b2 > b1, "batches must exceed the 256 MiB Infinity Cache"
    ch, thr = (1 if C > 1 else 0), 50

    g = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.randint(0, 31, (b2, H, W, C), dtype=torch.uint8, device="cuda", generator=g)
    y, x = torch.meshgrid(torch.arange(33, device="cuda"), torch.arange(33, device="cuda"), indexing="ij")
    spot = (230.0 * torch.exp(-0.5 * ((x - 16.3) ** 2 + (y - 15.6) ** 2) / 2.0 ** 2)).round().clamp(0, 255).to(torch.uint8)
    for f in range(b2):
        x0, y0 = (37 * f) % (W - 40), (53 * f) % (H - 40)
        frames[f, y0:y0 + 33, x0:x0 + 33, ch] = torch.maximum(frames[f, y0:y0 + 33, x0:x0 + 33, ch], spot)

    row = {"size": a.size, "frames": [b1, b2], "frame_bytes": frame_bytes, "reps": a.reps}

    def slope(key, fn, bytes_per_frame):
        t1, t2 = timed(lambda: fn(b1), a.reps), timed(lambda: fn(b2), a.reps)
        per_frame = (t2 - t1) / (b2 - b1)
        row.update({f"{key}_call_ms": [round(t1 * 1e3, 4), round(t2 * 1e3, 4)], f"{key}_frames_per_s": round(1.0 / per_frame, 1),
                    f"{key}_us_per_frame": round(per_frame * 1e6, 2), f"{key}_GBps": round(bytes_per_frame / per_frame * 1e-9, 1),
                    f"{key}_call_fixed_ms": round((t1 - per_frame * b1) * 1e3, 4)})
        return per_frame

    # the yardsticks first: sba_detect_dots on the same frames, and a device-to-device copy of them
    dots = slope("dots", lambda b: _native.detect_dots(frames[:b], threshold=thr, channel=ch), frame_bytes)
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
    copy_frame_s = statistics.median(tc) / b2
    del dst
    row.update({"d2d_copy_ms": round(copy_frame_s * b2 * 1e3, 4), "d2d_frames_per_s": round(1.0 / copy_frame_s, 1),
                "d2d_GBps": round(2 * frame_bytes / copy_frame_s * 1e-9, 1)})

    acc = {"sum": torch.zeros((H, W), dtype=torch.int32, device="cuda"), "sumsq": torch.zeros((H, W), dtype=torch.int64, device="cuda"),
           "hot": torch.zeros((H, W), dtype=torch.int32, device="cuda"), "vmax": torch.zeros((H, W), dtype=torch.uint8, device="cuda")}
    for key, planes in (("accumulate_all", acc), ("accumulate_sum", {"sum": acc["sum"]})):
        per = slope(key, lambda b: _native.background_accumulate(frames[:b], threshold=thr, channel=ch, accumulate=False, **planes), frame_bytes)
        row[f"{key}_over_dots"] = round(dots / per, 3)

    # what the kernel computed, restated in torch on the smaller batch (and checked against it)
    _native.background_accumulate(frames[:b1], threshold=thr, channel=ch, accumulate=False, **acc)

    def restated():
        v = frames[:b1, ..., ch].to(torch.int64)
        out = v.sum(0), (v * v).sum(0), (v > thr).sum(0), v.amax(0)
        torch.cuda.synchronize()
        return out

    ref = restated()
    assert all(torch.equal(acc[k].to(torch.int64), r) for k, r in zip(("sum", "sumsq", "hot", "vmax"), ref)), "kernel and torch differ"
    del ref
    tt = timed(restated, max(2, a.reps // 3))
    row.update({"torch_ms": round(tt * 1e3, 3), "torch_frames_per_s": round(b1 / tt, 1),
                "accumulate_all_over_torch": round(tt / b1 * row["accumulate_all_frames_per_s"], 2)})

    level = torch.randint(0, 64, (H, W), dtype=torch.uint8, device="cuda", generator=g)
    mask = (torch.rand((H, W), device="cuda", generator=g) < 0.01).to(torch.uint8)
    out = torch.empty((b2, H, W), dtype=torch.uint8, device="cuda")
    for mode in ("gate", "subtract"):
        per = slope(f"suppress_{mode}", lambda b: _native.background_suppress(frames[:b], level=level, mask=mask, mode=mode, channel=ch,
                                                                              out=out[:b]), frame_bytes + W * H)
        row[f"suppress_{mode}_over_copy"] = round((frame_bytes + W * H) / per / (2 * frame_bytes / copy_frame_s), 3)
    del out, frames

    hb = a.host_frames
    host = np.random.default_rng(0).integers(0, 31, size=(hb, H, W, C), dtype=np.uint8)
    hacc = {"sum": np.zeros((H, W), np.uint32), "sumsq": np.zeros((H, W), np.uint64), "hot": np.zeros((H, W), np.uint32),
            "vmax": np.zeros((H, W), np.uint8)}
    hout = np.empty((hb, H, W), np.uint8)
    hlevel, hmask = level.cpu().numpy(), mask.cpu().numpy()
    reps = max(3, a.reps // 2)
    th = {"host_dots": timed(lambda: _native.detect_dots(host, threshold=thr, channel=ch), reps),
          "host_accumulate_all": timed(lambda: _native.background_accumulate(host, threshold=thr, channel=ch, accumulate=False, **hacc), reps),
          "host_suppress_gate": timed(lambda: _native.background_suppress(host, level=hlevel, mask=hmask, channel=ch, out=hout), reps)}
    row["host_frames"] = hb
    for key, t in th.items():
        row.update({f"{key}_call_ms": round(t * 1e3, 3), f"{key}_frames_per_s": round(hb / t, 1), f"{key}_GBps_in": round(hb * frame_bytes / t * 1e-9, 2)})
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
