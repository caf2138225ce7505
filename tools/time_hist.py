"""Time sba_frame_histograms on full-size frames against sba_detect_dots on the same frames; one JSON line per run, appended
(does not touch bench.py).

    python tools/time_hist.py [--size 3208x2200x3] [--frames 32,128] [--host-frames 16] [--reps 10] [--label TEXT]
                              [--out profiles/hist_timing.jsonl]

Three contents, because the cost of a histogram depends on the values -- equal values meet in one bin:

* ``dark``: dark noise (0..30 counts, all channels) with one Gaussian spot per frame: what a recording looks like
  (tools/time_detect.py renders the same frames)
* ``random``: uniform random bytes
* ``zero``: the constant 0 -- every pixel of every wave in one bin

Per content, device-resident frames: the call is timed at two batch sizes (both far larger than the 256 MiB Infinity Cache), the
slope (t2 - t1) / (frames2 - frames1) is the kernels' time per frame without the call's fixed cost.  ``hist`` and ``dots``
(sba_detect_dots, threshold 50: the project's yardstick for a kernel that reads every byte once and writes almost nothing)
alternate in the same run; ``*_hist_over_dots`` is the ratio of their rates, 1.0 = as fast as the detector.
``total_only`` is the histogram call without per-frame rows (``want_hist=False``).  Also in the run: ``d2d``, ``dst.copy_(src)``
of the larger batch under HIP events; ``bincount``, the same per-frame histograms from ``torch.bincount`` on the channel (8
frames, HIP events); ``host``: both calls on pageable numpy frames, staging copies included, in frames/s.
``--label`` is stored in the row (which build was timed).
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


def event_timed(torch, fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fn()
    t = []
    for _ in range(reps):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        t.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3208x2200x3")
    ap.add_argument("--frames", default="32,128")
    ap.add_argument("--host-frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hist_timing.jsonl"))
    a = ap.parse_args()
    import torch
    W, H, C = (int(v) for v in a.size.split("x"))
    b1, b2 = (int(v) for v in a.frames.split(","))
    assert _native.device_count() > 0, "time_hist.py needs the GPU"
    frame_bytes = W * H * C
    assert b1 * frame_bytes > (256 << 20) and b2 > b1, "batches must exceed the 256 MiB Infinity Cache"
    ch = 1 if C > 1 else 0

    g = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.empty((b2, H, W, C), dtype=torch.uint8, device="cuda")
    y, x = torch.meshgrid(torch.arange(33, device="cuda"), torch.arange(33, device="cuda"), indexing="ij")
    spot = (230.0 * torch.exp(-0.5 * ((x - 16.3) ** 2 + (y - 15.6) ** 2) / 2.0 ** 2)).round().clamp(0, 255).to(torch.uint8)

    def fill(content):
        if content == "zero":
            frames.zero_()
        else:
            frames.random_(0, 31 if content == "dark" else 256, generator=g)
        if content == "dark":
            for f in range(b2):
                x0, y0 = (37 * f) % (W - 40), (53 * f) % (H - 40)
                frames[f, y0:y0 + 33, x0:x0 + 33, ch] = torch.maximum(frames[f, y0:y0 + 33, x0:x0 + 33, ch], spot)

    row = {"size": a.size, "frames": [b1, b2], "frame_bytes": frame_bytes, "reps": a.reps, "label": a.label}
    calls = {"hist": lambda src: _native.frame_histograms(src, channel=ch),
             "total_only": lambda src: _native.frame_histograms(src, channel=ch, want_hist=False),
             "dots": lambda src: _native.detect_dots(src, threshold=50, channel=ch)}
    for content in ("dark", "random", "zero"):
        fill(content)
        hist, total = calls["hist"](frames[:8])              # the counts are right before they are timed
        want = torch.stack([torch.bincount(frames[f, :, :, ch].flatten().int(), minlength=256) for f in range(8)]).cpu().numpy()
        assert np.array_equal(hist, want) and np.array_equal(total, want.sum(axis=0).astype(np.uint64)), content
        t = {}
        for name, fn in calls.items():                       # the three calls side by side: small batch, then large
            t[name] = [timed(lambda: fn(frames[:b1]), a.reps), timed(lambda: fn(frames), a.reps)]
        for name, (t1, t2) in t.items():
            per_frame = (t2 - t1) / (b2 - b1)
            row.update({f"{content}_{name}_call_ms": [round(t1 * 1e3, 4), round(t2 * 1e3, 4)],
                        f"{content}_{name}_us_per_frame": round(per_frame * 1e6, 3),
                        f"{content}_{name}_frames_per_s": round(1.0 / per_frame, 1),
                        f"{content}_{name}_GBps": round(frame_bytes / per_frame * 1e-9, 1),
                        f"{content}_{name}_call_fixed_ms": round((t1 - per_frame * b1) * 1e3, 4)})
        row[f"{content}_hist_over_dots"] = round(row[f"{content}_dots_us_per_frame"] / row[f"{content}_hist_us_per_frame"], 3)
        row[f"{content}_total_only_over_dots"] = round(row[f"{content}_dots_us_per_frame"] / row[f"{content}_total_only_us_per_frame"], 3)
        offsets = (torch.arange(8, device="cuda", dtype=torch.int32) * 256)[:, None]
        tb = event_timed(torch, lambda: torch.bincount((frames[:8, :, :, ch].reshape(8, -1).int() + offsets).flatten(), minlength=8 * 256), 5)
        row[f"{content}_bincount_us_per_frame"] = round(tb / 8 * 1e6, 1)
        if content == "dark":
            dst = torch.empty_like(frames)
            copy_s = event_timed(torch, lambda: dst.copy_(frames), a.reps)
            row.update({"d2d_copy_us_per_frame": round(copy_s / b2 * 1e6, 3), "d2d_read_GBps": round(b2 * frame_bytes / copy_s * 1e-9, 1)})
            del dst

    hb = a.host_frames
    rng = np.random.default_rng(0)
    host = rng.integers(0, 31, size=(hb, H, W, C), dtype=np.uint8)
    host[:, 100:133, 200:233, ch] = spot.cpu().numpy()
    for name in ("hist", "dots"):
        th = timed(lambda: calls[name](host), max(3, a.reps // 3))
        row.update({f"host_{name}_call_ms": round(th * 1e3, 3), f"host_{name}_frames_per_s": round(hb / th, 1),
                    f"host_{name}_GBps": round(hb * frame_bytes / th * 1e-9, 2)})
    row["host_frames"] = hb
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
