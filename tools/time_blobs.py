"""Time sba_detect_blobs on full-size frames against sba_detect_dots on the same frames; one JSON line per run, appended
(does not touch bench.py).

    python tools/time_blobs.py [--size 3208x2200x3] [--frames 32,128] [--host-frames 16] [--reps 5] [--cases dark,dense]
                               [--out profiles/blobs_timing.jsonl]

Two kinds of device-resident frames, threshold 50, the reference's radii (1, 4):

* dark:  dark noise (0..30 counts, all channels) with one Gaussian spot each -- what a recording looks like;
* dense: the same noise with 1 % of the pixels set, the bad case: after the dilation about half the frame is mask.

Each call is timed at two batch sizes (both far larger than the 256 MiB Infinity Cache); the slope (t2 - t1) / (b2 - b1) is the
time per frame without the call's fixed cost (buffers, streams, read-back), as in tools/time_detect.py.  ``*_dots_frames_per_s``
is sba_detect_dots -- one pass over the bytes at the HBM rate -- on the same frames in the same run, the yardstick;
``*_dots_over_blobs`` is how many times longer the connected-component call takes per frame.  ``host_*``: the whole call on
pageable numpy frames (staging copies included) for both detectors: bound by the host-to-device copy.
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="dark,dense", help="which kinds of frames to time (a profiler run may want one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blobs_timing.jsonl"))
    a = ap.parse_args()
    import torch
    W, H, C = (int(v) for v in a.size.split("x"))
    b1, b2 = (int(v) for v in a.frames.split(","))
    assert _native.device_count() > 0, "time_blobs.py needs the GPU"
    frame_bytes = W * H * C
    assert b2 > b1 >= 1
    ch = 1 if C > 1 else 0

    g = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.randint(0, 31, (b2, H, W, C), dtype=torch.uint8, device="cuda", generator=g)
    y, x = torch.meshgrid(torch.arange(33, device="cuda"), torch.arange(33, device="cuda"), indexing="ij")
    spot = (230.0 * torch.exp(-0.5 * ((x - 16.3) ** 2 + (y - 15.6) ** 2) / 2.0 ** 2)).round().clamp(0, 255).to(torch.uint8)
    for f in range(b2):
        x0, y0 = (37 * f) % (W - 40), (53 * f) % (H - 40)
        frames[f, y0:y0 + 33, x0:x0 + 33, ch] = torch.maximum(frames[f, y0:y0 + 33, x0:x0 + 33, ch], spot)
    blobs = _native.detect_blobs(frames[:b1], threshold=50, channel=ch)
    assert np.all(blobs.status == _native.BLOB_OK), blobs.status

    row = {"size": a.size, "frames": [b1, b2], "frame_bytes": frame_bytes, "reps": a.reps}
    for name in a.cases.split(","):
        if name == "dense":
            for f in range(b2):
                hit = torch.rand((H, W), device="cuda", generator=g) < 0.01
                frames[f, :, :, ch][hit] = 200
            blobs = _native.detect_blobs(frames[:2], threshold=50, channel=ch, max_blobs=64)
            row["dense_components_per_frame"] = int(blobs.n_components[0])
        for call, fn in (("blobs", lambda src: _native.detect_blobs(src, threshold=50, channel=ch)),
                         ("dots", lambda src: _native.detect_dots(src, threshold=50, channel=ch))):
            t1 = timed(lambda: fn(frames[:b1]), a.reps)
            t2 = timed(lambda: fn(frames), a.reps)
            per_frame = (t2 - t1) / (b2 - b1)
            row.update({f"{name}_{call}_call_ms": [round(t1 * 1e3, 3), round(t2 * 1e3, 3)],
                        f"{name}_{call}_frames_per_s": round(1.0 / per_frame, 1),
                        f"{name}_{call}_GBps": round(frame_bytes / per_frame * 1e-9, 1),
                        f"{name}_{call}_call_fixed_ms": round((t1 - per_frame * b1) * 1e3, 3)})
        row[f"{name}_dots_over_blobs"] = round(row[f"{name}_dots_frames_per_s"] / row[f"{name}_blobs_frames_per_s"], 2)

    hb = a.host_frames
    if hb <= 0:
        print(json.dumps(row), flush=True)
        return
    rng = np.random.default_rng(0)
    host = rng.integers(0, 31, size=(hb, H, W, C), dtype=np.uint8)
    host[:, 100:133, 200:233, ch] = spot.cpu().numpy()
    for call, fn in (("blobs", lambda: _native.detect_blobs(host, threshold=50, channel=ch)),
                     ("dots", lambda: _native.detect_dots(host, threshold=50, channel=ch))):
        th = timed(fn, max(3, a.reps // 2))
        row.update({f"host_{call}_call_ms": round(th * 1e3, 3), f"host_{call}_frames_per_s": round(hb / th, 1),
                    f"host_{call}_GBps": round(hb * frame_bytes / th * 1e-9, 2)})
    row["host_frames"] = hb
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
