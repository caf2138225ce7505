"""Time sba_resize_frames on full-size frames; one JSON line per run, appended (does not touch bench.py).

    python tools/time_resize.py [--size 3208x2200x3] [--frames 32,128] [--host-frames 16] [--reps 7] [--out profiles/resize_timing.jsonl]

Frames are dark (uniform random bytes below 40: the detector's usual diet, and the resize's work does not depend on the values).

* kernel: the call on device-resident frames into a device-resident output is timed at two batch sizes (both far larger than the
  256 MiB Infinity Cache); the slope (t2 - t1) / (b2 - b1) is the kernel's time per frame without the call's fixed cost, which is
  reported as ``*_call_fixed_ms``.  ``*_read_GBps`` counts the source bytes alone: the output is a sixteenth to a quarter of them.
  Cases: 4 x 4 colour, 4 x 4 grey, 2 x 2 colour and factor 1 with grey (only the conversion).
* detect: ``sba_detect_dots`` on the same frames, the same way -- the project's fastest reader of these bytes; ``*_over_detect``
  is detector time / resize time per frame (1 = as fast as the detector reads).
* d2d: ``dst.copy_(src)`` of the larger batch under HIP events -- ``*_over_copy`` is copy time / resize time for the same source bytes.
* torch: the same 4 x 4 reduction written with torch ops (``avg_pool2d`` of a float32 copy, rounded half to even: exact at 4 x 4), what a
  caller would otherwise do; checked against the library's result on one frame, timed on the smaller batch.
* host: the whole call on pageable numpy frames into a numpy preview, against ``imaging.undistort_frames`` on the same frames into
  a full-size numpy output: what the shrinking output saves on the bus.
* check: frame 0 and the last frame of the large batch equal an integer restatement of the rule in torch (int32 sums; for the
  power-of-two areas measured here the rule is the quotient with ties to even), so the timed kernel is also a right one.
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


def torch_rule(frames, fx, fy, gray):
    """The header's rule for a power-of-two area (or 2 x 2) in torch integer ops, on the device."""
    import torch
    v = frames.to(torch.int32)
    if gray:
        w = _native.GRAY_BGR
        v = ((v[..., 0] * w[0] + v[..., 1] * w[1] + v[..., 2] * w[2] + (1 << 14)) >> 15)[..., None]
    B, H, W, C = v.shape
    s = v[:, :H // fy * fy, :W // fx * fx].reshape(B, H // fy, fy, W // fx, fx, C).sum(dim=(2, 4))
    area = fx * fy
    assert area & (area - 1) == 0
    if (fx, fy) == (2, 2):
        out = (s + 2) >> 2
    else:
        q, r = s // area, s % area
        out = q + ((2 * r > area) | ((2 * r == area) & (q % 2 == 1))).to(torch.int32)
    out = out.to(torch.uint8)
    return out[..., 0] if gray else out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3208x2200x3")
    ap.add_argument("--frames", default="32,128")
    ap.add_argument("--host-frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_timing.jsonl"))
    a = ap.parse_args()
    import torch
    W, H, C = (int(v) for v in a.size.split("x"))
    b1, b2 = (int(v) for v in a.frames.split(","))
    assert _native.device_count() > 0, "time_resize.py needs the GPU"
    frame_bytes = W * H * C
    assert b1 * frame_bytes > (256 << 20) and b2 > b1, "batches must exceed the 256 MiB Infinity Cache"

    g = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.randint(0, 40, (b2, H, W, C), dtype=torch.uint8, device="cuda", generator=g)
    row = {"size": a.size, "frames": [b1, b2], "frame_bytes": frame_bytes, "reps": a.reps}

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
    row.update({"d2d_us_per_frame": round(copy_frame_s * 1e6, 2), "d2d_GBps": round(2 * frame_bytes / copy_frame_s * 1e-9, 1)})
    del dst

    def slope(key, fn):
        t1, t2 = timed(lambda: fn(frames[:b1]), a.reps), timed(lambda: fn(frames), a.reps)
        per_frame = (t2 - t1) / (b2 - b1)
        row.update({f"{key}_call_ms": [round(t1 * 1e3, 4), round(t2 * 1e3, 4)], f"{key}_us_per_frame": round(per_frame * 1e6, 2),
                    f"{key}_frames_per_s": round(1.0 / per_frame, 1), f"{key}_read_GBps": round(frame_bytes / per_frame * 1e-9, 1),
                    f"{key}_call_fixed_ms": round((t1 - per_frame * b1) * 1e3, 4)})
        return per_frame

    detect = slope("detect", lambda f: _native.detect_dots(f, threshold=50, channel=1))
    cases = {"4x4_colour": (4, 4, False), "4x4_gray": (4, 4, True), "2x2_colour": (2, 2, False), "1x1_gray": (1, 1, True)}
    for key, (fx, fy, gray) in cases.items():
        shape = (b2, H // fy, W // fx) + (() if gray else (C,))
        out = torch.empty(shape, dtype=torch.uint8, device="cuda")
        per_frame = slope(key, lambda f: imaging.resize_frames(f, (fx, fy), gray=gray, out=out[:f.shape[0]]))
        row.update({f"{key}_over_detect": round(detect / per_frame, 3), f"{key}_over_copy": round(copy_frame_s / per_frame, 3)})
        for k in (0, b2 - 1):
            assert torch.equal(out[k:k + 1], torch_rule(frames[k:k + 1], fx, fy, gray)), f"{key}: frame {k} differs from the rule"
        del out
    row["checked_frames"] = [0, b2 - 1]

    def pooled(f):                                           # 4 x 4, as a caller without the library would write it
        x = f.permute(0, 3, 1, 2).to(torch.float32)
        return torch.round(torch.nn.functional.avg_pool2d(x, 4)).to(torch.uint8).permute(0, 2, 3, 1)

    tb = min(b1, 8)
    assert torch.equal(pooled(frames[:1]).contiguous(), imaging.resize_frames(frames[:1], 4)), "the torch formulation differs"
    t_pool = timed(lambda: (pooled(frames[:tb]), torch.cuda.synchronize()), a.reps)
    row.update({"torch_pool_frames": tb, "torch_pool_us_per_frame": round(t_pool / tb * 1e6, 2),
                "torch_pool_over_4x4_colour": round(t_pool / tb / (row["4x4_colour_us_per_frame"] * 1e-6), 2)})
    row["one_frame_ms"] = round(timed(lambda: imaging.resize_frames(frames[:1], 4), a.reps) * 1e3, 4)
    del frames
    torch.cuda.empty_cache()

    hb = a.host_frames
    host = np.random.default_rng(0).integers(0, 40, size=(hb, H, W, C), dtype=np.uint8)
    small = np.empty((hb, H // 4, W // 4, C), np.uint8)
    reps = max(3, a.reps // 2)
    th = timed(lambda: imaging.resize_frames(host, 4, out=small), reps)
    f = 2388.5 * W / 3208
    lens = imaging.Lens(f, f, (W - 1) / 2 + 3.3, (H - 1) / 2 - 2.6, -0.25, 0.05)
    full = np.empty_like(host)
    tu = timed(lambda: imaging.undistort_frames(host, lens, out=full), reps)
    row.update({"host_frames": hb, "host_preview_call_ms": round(th * 1e3, 3), "host_preview_frames_per_s": round(hb / th, 1),
                "host_preview_GBps_in": round(hb * frame_bytes / th * 1e-9, 2), "host_undistort_call_ms": round(tu * 1e3, 3),
                "host_undistort_frames_per_s": round(hb / tu, 1), "host_preview_over_undistort": round(tu / th, 2)})
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
