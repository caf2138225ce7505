"""GPU tests of sba_refine_corners (include/sba_hip.h) through ``lasercalib_amd.imaging.refine_corners``: sub-pixel refinement of
corners in a batch of frames.

The reference is ``refine_corners_oracle`` of tests/test_corners_host.py (the header's rule in numpy, pinned there to answers
known without it).  EVERY comparison is bit equality of ``refined``, ``status``, ``iterations`` and ``tensor``, except the one
of the library's own window (weights == NULL), whose tolerance is derived below.  Frames are 40 x 44 unless named.
"""
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lasercalib_amd import _native, imaging  # noqa: E402
from lasercalib_amd.imaging import Lens  # noqa: E402
from test_corners_host import (CONVERGED, INVALID, LEFT_IMAGE, MAX_ITER, RESTORED, SINGULAR, TRUTH_BOUND, batch_oracle,  # noqa: E402
                               refine_corners_oracle, render_corner, rendered_corners, symmetric_corner, window_oracle)
from test_gpu_detect import device_view, pitched  # noqa: E402
from test_warp_host import inverse_k  # noqa: E402

H, W = 40, 44

# The library's own window (weights == NULL) is built with the C runtime's exp, the oracle's with Python's; the two may differ in
# the last bit of a weight.  Measured on the oracle when this file was written (12 rendered corners, four starts each; every
# weight moved one ulp up, one ulp down, and in four random patterns): statuses and iteration counts do not change, positions by
# 3.6e-15 px at the most.  The tolerance is 8 times that.
NULL_WINDOW_TOL = 8 * 3.6e-15


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert _native.device_count() > 0, "no HIP device visible: GPU tests must run on the MI355X box"


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def scene(C, B, first=0):
    """(B, H, W, C) frames, every channel of every frame another rendered corner, and the true centres (B, C, 2)."""
    pool = rendered_corners()
    frames, centres = np.zeros((B, H, W, C), np.uint8), np.zeros((B, C, 2))
    for f in range(B):
        for c in range(C):
            img, q = pool[(first + f * C + c) % len(pool)]
            frames[f, :, :, c], centres[f, c] = img, q
    return frames, centres


def starts_around(centre, n, seed, reach=2.0):
    """n starts: the centre rounded to whole pixels, then random ones within +-reach."""
    rng = np.random.default_rng(seed)
    pts = np.array(centre)[None, :] + rng.uniform(-reach, reach, size=(n, 2))
    if n:
        pts[0] = np.rint(centre)
    return pts


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def check(res, want, what=None):
    refined, status, iterations, tensor = want
    assert res.xy.dtype == np.float64 and res.status.dtype == np.int32 and res.iterations.dtype == np.int32 and res.tensor.dtype == np.float64
    assert res.xy.shape == refined.shape and res.tensor.shape == tensor.shape, what
    assert np.array_equal(res.status, status), (what, res.status, status)
    assert np.array_equal(res.iterations, iterations), (what, res.iterations, iterations)
    assert np.array_equal(bits(res.xy), bits(refined)), (what, np.max(np.abs(res.xy - refined)))
    assert np.array_equal(bits(res.tensor), bits(tensor)), what


def channel_of(C, channel):
    return dict(channel=channel) if C > 1 else {}


# ----------------------------------------------------------------------------- 1. windows, channels, host and device frames
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("win", [(1, 1), (3, 3), (5, 2), (15, 15)])
def test_windows_and_channels_host_and_device(torch, win, C):
    n = 3 if win == (15, 15) else 6
    frames, centres = scene(C, 2, first=3 * C)
    dev = torch.from_numpy(frames).cuda()
    met = set()
    for channel in list(range(C)) + ([-1] if C > 1 else []):
        c = 1 if channel == -1 else channel                     # the grey value is mostly channel 1
        per_frame = [starts_around(centres[f, c], n, seed=10 * f + c) for f in range(2)]
        want = batch_oracle(frames, per_frame, win=win, channel=channel)
        met |= set(want[1].tolist())
        check(imaging.refine_corners(frames, per_frame, win=win, **channel_of(C, channel)), want, (win, C, channel, "host"))
        check(imaging.refine_corners(dev, per_frame, win=win, **channel_of(C, channel)), want, (win, C, channel, "device"))
    assert CONVERGED in met, met
    if C == 1:                                                  # (B, H, W) is the one-channel layout
        per_frame = [starts_around(centres[f, 0], n, seed=f) for f in range(2)]
        check(imaging.refine_corners(frames[..., 0], per_frame, win=win), batch_oracle(frames, per_frame, win=win), (win, "3-D"))


def test_default_channel_is_grey_for_colour_and_the_plane_for_one_channel():
    frames, centres = scene(3, 1)
    per_frame = [starts_around(centres[0, 1], 4, seed=1)]
    check(imaging.refine_corners(frames, per_frame), batch_oracle(frames, per_frame, channel=-1))
    check(imaging.refine_corners(frames, per_frame, channel_order="rgb"), batch_oracle(frames, per_frame, channel=-1, gray_w=(9798, 19235, 3735)))
    plane = np.ascontiguousarray(frames[..., :1])
    check(imaging.refine_corners(plane, per_frame), batch_oracle(plane, per_frame, channel=0))


# ----------------------------------------------------------------------------- 2. pitches and bases
@pytest.mark.parametrize("C", [1, 3, 4])
def test_padded_rows_and_frames_and_misaligned_bases(torch, C):
    frames, centres = scene(C, 3, first=7)
    channel = -1 if C > 1 else 0
    per_frame = [starts_around(centres[f, min(1, C - 1)], 5, seed=f) for f in range(3)]
    want = batch_oracle(frames, per_frame, channel=channel)
    for row_pitch in (W * C, W * C + 5):
        buf, view, frame_pitch = pitched(frames, row_pitch, 13, fill=253)
        check(imaging.refine_corners(view, per_frame), want, (C, row_pitch, "host"))
        for offset in (0, 1, 7, 15):
            shifted = np.full(buf.size + 16, 253, np.uint8)
            shifted[offset:offset + buf.size] = buf
            _keep, dev = device_view(torch, shifted, (3, H, W, C), (frame_pitch, row_pitch, C, 1), offset=offset)
            assert dev.data_ptr() % 16 == offset
            check(imaging.refine_corners(dev, per_frame), want, (C, row_pitch, offset, "device"))
            host = np.lib.stride_tricks.as_strided(shifted[offset:], shape=(3, H, W, C), strides=(frame_pitch, row_pitch, C, 1))
            check(imaging.refine_corners(host, per_frame), want, (C, row_pitch, offset, "host"))


# ----------------------------------------------------------------------------- 3. corner counts and chunks
COUNTED = {}


def counted():
    """Six frames and their corners, 0, 1, 63, 64, 65 and 257 of them, with the oracle's answer per frame; shared."""
    if not COUNTED:
        frames, centres = scene(1, 6, first=20)
        per_frame = {k: starts_around(centres[f, 0], k, seed=k, reach=2.5).reshape(-1, 2) for f, k in enumerate((0, 1, 63, 64, 65, 257))}
        COUNTED["frames"], COUNTED["corners"] = frames, per_frame
        COUNTED["want"] = {k: refine_corners_oracle(frames[f], per_frame[k], max_iter=12) for f, k in enumerate((0, 1, 63, 64, 65, 257))}
    return COUNTED


@pytest.mark.parametrize("order", [(1, 0, 63, 64, 65, 257), (257, 65, 0, 64, 63, 1), (65, 257, 64, 1, 63, 0)])
def test_corner_counts_across_the_wave_boundary_and_empty_frames(torch, order):
    S = counted()
    index = {k: f for f, k in enumerate((0, 1, 63, 64, 65, 257))}
    frames = np.stack([S["frames"][index[k]] for k in order])
    per_frame = [S["corners"][k] for k in order]
    want = tuple(np.concatenate([S["want"][k][i] for k in order]) for i in range(4))
    assert len(want[1]) == 450 and len(set(want[2].tolist())) > 3          # corners that stop early sit beside ones that run on
    res = imaging.refine_corners(frames, per_frame, max_iter=12)
    check(res, want, order)
    assert [len(c) for c in res.corners] == list(order)
    check(imaging.refine_corners(torch.from_numpy(frames).cuda(), per_frame, max_iter=12), want, (order, "device"))
    check(imaging.refine_corners(frames, per_frame, max_iter=12, chunk_frames=2), want, (order, "chunks of 2"))


def test_seven_host_frames_in_chunks():
    frames, centres = scene(3, 7, first=40)
    per_frame = [starts_around(centres[f, 1], (5, 0, 9, 1, 0, 0, 7)[f], seed=f).reshape(-1, 2) for f in range(7)]
    want = batch_oracle(frames, per_frame, channel=-1)
    for chunk in (1, 2, 3, 7, 0):
        check(imaging.refine_corners(frames, per_frame, chunk_frames=chunk), want, chunk)


def test_no_frames_and_no_corners():
    res = imaging.refine_corners(np.zeros((0, H, W, 3), np.uint8), [])
    assert res.corners == [] and res.xy.shape == (0, 2) and res.status.shape == (0,) and res.tensor.shape == (0, 3)
    frames, _ = scene(3, 2)
    res = imaging.refine_corners(frames, [np.zeros((0, 2)), np.zeros((0, 2))])
    assert [c.shape for c in res.corners] == [(0, 2), (0, 2)] and res.status.shape == (0,)
    lib = _native.load()                                        # n_frames = 0 reads nothing: not even corner_start
    assert lib.sba_refine_corners(0, None, 0, H, W, 3, W * 3, H * W * 3, None, None, None, None, None, None, None, None) == 0


# ----------------------------------------------------------------------------- 4. every status, side by side in a wave
def status_scene():
    """Two frames -- the symmetric corner, and a corner 0.4 px from the left border -- and a list that ends in every way."""
    frames = np.stack([symmetric_corner()[0], render_corner(H, W, 0.4, 20.0, 0.7)])
    a = [(22.0, 19.0), (22.9, 18.2), (np.nan, 3.0), (30.0, 30.0), (3.0, np.inf), (21.0, 19.6), (32768.0, 5.0), (22.0, 5.0), (25.5, 22.5),
         (-np.inf, 2.0), (5.0, -32768.0), (20.2, 20.9), (26.0, 15.5), (1e300, 1.0), (-100.0, -100.0), (23.5, 19.0)]
    b = [(0.25, 15.0), (2.0, 20.0), (5.75, 16.5), (0.5, 15.0), (3.0, 21.0), (6.75, 17.5), (30.0, 8.0), (6.25, 16.5), (1.0, 19.0), (1.25, 15.0)]
    return frames, [np.array(a), np.array(b)]


def test_every_status_mixed_in_one_list(torch):
    frames, per_frame = status_scene()
    want = batch_oracle(frames, per_frame)
    met = set(want[1].tolist())
    assert {CONVERGED, SINGULAR, INVALID, CONVERGED | RESTORED, LEFT_IMAGE | RESTORED, MAX_ITER | RESTORED} <= met, met
    assert want[2][0] == 1 and want[0][0].tolist() == [22.0, 19.0]          # the exact fixed point of the host file
    res = imaging.refine_corners(frames, per_frame)
    check(res, want)
    assert np.array_equal(res.ok, want[1] == CONVERGED)
    cov = res.covariance_shape()
    assert np.all(np.isnan(cov[(want[1] & (SINGULAR | INVALID)) != 0])) and np.all(np.isfinite(cov[res.ok]))
    check(imaging.refine_corners(torch.from_numpy(frames).cuda(), per_frame), want, "device")
    one = refine_corners_oracle(frames[0], [(24.0, 21.0)], win=(1, 1))      # 2 px outside a (1, 1) window's reach
    assert one[1][0] & RESTORED
    check(imaging.refine_corners(frames[:1], [np.array([(24.0, 21.0)])], win=(1, 1)), one)


@pytest.mark.parametrize("max_iter", [1, 2, 200])
def test_max_iter(max_iter):
    frames, per_frame = status_scene()
    want = batch_oracle(frames, per_frame, max_iter=max_iter)
    assert want[2].max() == max_iter and np.any(want[1] & MAX_ITER)
    check(imaging.refine_corners(frames, per_frame, max_iter=max_iter), want)


def test_eps_zero_runs_to_max_iter_or_a_repeated_position():
    frames, centres = scene(1, 2, first=11)
    per_frame = [starts_around(centres[f, 0], 4, seed=f) for f in range(2)]
    want = batch_oracle(frames, per_frame, eps=0.0, max_iter=60)
    assert np.all((want[1] == MAX_ITER) | (want[1] == CONVERGED)) and np.any(want[1] == MAX_ITER)
    check(imaging.refine_corners(frames, per_frame, eps=0.0, max_iter=60), want)


def test_explicit_weights_and_zero_zone():
    frames, centres = scene(3, 2, first=30)
    per_frame = [starts_around(centres[f, 1], 6, seed=f) for f in range(2)]
    rng = np.random.default_rng(8)
    weights = rng.uniform(0.0, 3.0, size=(5, 11))               # win (5, 2): 2 wy + 1 = 5 rows of 2 wx + 1 = 11
    weights[rng.random(weights.shape) < 0.2] = 0.0
    weights[0, 0] = 1e-300
    want = batch_oracle(frames, per_frame, win=(5, 2), channel=1, weights=weights)
    check(imaging.refine_corners(frames, per_frame, win=(5, 2), channel=1, weights=weights), want)
    check(imaging.refine_corners(frames, per_frame, win=(5, 2), channel=1, weights=weights, zero_zone=(1, 1)), want, "not applied to explicit weights")
    for zero_zone in ((1, 1), (2, 0), (3, 3), (-1, 1)):
        want = batch_oracle(frames, per_frame, zero_zone=zero_zone, channel=2)
        check(imaging.refine_corners(frames, per_frame, zero_zone=zero_zone, channel=2), want, zero_zone)


# ----------------------------------------------------------------------------- 5. the smallest and the largest frames
def test_frames_of_one_pixel_and_of_one_row(torch):
    rng = np.random.default_rng(4)
    for shape in ((2, 1, 1, 3), (2, 1, 5, 1), (2, 5, 1, 4), (1, 2, 2, 3)):
        frames = rng.integers(0, 256, size=shape, dtype=np.uint8)
        per_frame = [np.array([(0.0, 0.0), (0.4, 0.3), (shape[2] - 0.5, shape[1] - 0.5), (2.3, 0.0), (-3.0, 7.5)]) for _ in range(shape[0])]
        for win in ((1, 1), (3, 3)):
            want = batch_oracle(frames, per_frame, win=win, channel=0)
            check(imaging.refine_corners(frames, per_frame, win=win, channel=0), want, (shape, win))
            check(imaging.refine_corners(torch.from_numpy(frames).cuda(), per_frame, win=win, channel=0), want, (shape, win, "device"))


def test_a_full_size_frame_with_corners_at_its_four_borders(torch):
    Hf, Wf = 2200, 3208
    frame = np.full((1, Hf, Wf), 90, np.uint8)
    pool = rendered_corners()
    places = [(0, 1080), (Wf - W, 1000), (1600, 0), (1500, Hf - H), (0, 0), (Wf - W, Hf - H), (1604, 1100)]    # left, right, top, bottom, ...
    corners = []
    for k, (x0, y0) in enumerate(places):
        img, q = pool[50 + k]
        frame[0, y0:y0 + H, x0:x0 + W] = img
        corners += [(x0 + q[0] + 0.6, y0 + q[1] - 0.7), (float(round(x0 + q[0])), float(round(y0 + q[1])))]
    corners += [(0.3, 1100.2), (Wf - 0.4, 1020.0), (1620.0, 0.2), (1520.0, Hf - 0.3), (0.0, 0.0), (Wf - 0.01, Hf - 0.01), (Wf + 2.0, Hf + 2.0)]
    # the windows of these hang over the border: a patch cut off by it
    for k, (x0, y0) in enumerate([(-20, 500), (Wf - 24, 1500), (800, -18), (2400, Hf - 21)]):
        img, q = pool[60 + k]
        xs, ys = max(x0, 0), max(y0, 0)
        xe, ye = min(x0 + W, Wf), min(y0 + H, Hf)
        frame[0, ys:ye, xs:xe] = img[ys - y0:ye - y0, xs - x0:xe - x0]
        corners.append((float(np.clip(round(x0 + q[0]), 0, Wf - 1)), float(np.clip(round(y0 + q[1]), 0, Hf - 1))))
    per_frame = [np.array(corners)]
    want = batch_oracle(frame, per_frame)
    assert np.count_nonzero(want[1] == CONVERGED) >= 14
    check(imaging.refine_corners(frame, per_frame), want, "host")
    check(imaging.refine_corners(torch.from_numpy(frame).cuda(), per_frame), want, "device")


# ----------------------------------------------------------------------------- 6. the library's own window
def test_null_weights_build_opencvs_window_in_the_library():
    frames, centres = scene(1, 3, first=0)
    per_frame = [starts_around(centres[f, 0], 4, seed=f) for f in range(3)]
    start = np.array([0, 4, 8, 12], np.int64)
    xy = np.concatenate(per_frame)
    for win, zero_zone in (((3, 3), (-1, -1)), ((3, 3), (1, 1)), ((5, 2), (0, 0)), ((2, 2), (2, 2))):
        want = batch_oracle(frames, per_frame, win=win, zero_zone=zero_zone)
        explicit = _native.refine_corners(frames, start, xy, win=win, zero_zone=zero_zone, weights=window_oracle(win, zero_zone))
        assert all(np.array_equal(bits(e), bits(w)) for e, w in zip(explicit, want))
        refined, status, iterations, tensor = _native.refine_corners(frames, start, xy, win=win, zero_zone=zero_zone, weights=None)
        assert np.array_equal(status, want[1]) and np.array_equal(iterations, want[2]), (win, zero_zone)
        print("weights == NULL against the explicit window:", win, zero_zone, np.max(np.abs(refined - want[0])), "px")
        assert np.max(np.abs(refined - want[0])) <= NULL_WINDOW_TOL, (win, zero_zone)
        assert np.allclose(tensor, want[3], rtol=1e-12, atol=0)
    lib = _native.load()                                        # opts == NULL is the reference's call
    refined, status = np.zeros_like(xy), np.zeros(12, np.int32)
    rc = lib.sba_refine_corners(0, frames.ctypes.data, 3, H, W, 1, W, H * W, _native._iptr(start), _native._dptr(xy), None, None,
                                _native._dptr(refined), status.ctypes.data, None, None)
    want = batch_oracle(frames, per_frame)
    assert rc == 0 and np.array_equal(status, want[1]) and np.max(np.abs(refined - want[0])) <= NULL_WINDOW_TOL


# ----------------------------------------------------------------------------- 7. the workflow
def render_board(Hb, Wb, cx, cy, q, theta, lo=40, hi=210, ss=8):
    """An endless checkerboard of squares of q pixels, turned by theta about (cx, cy), box-filtered ss x ss per pixel."""
    off = (np.arange(ss) + 0.5) / ss - 0.5
    X = (np.arange(Wb)[:, None] + off[None, :]).reshape(-1)[None, :] - cx
    Y = (np.arange(Hb)[:, None] + off[None, :]).reshape(-1)[:, None] - cy
    d1, d2 = X * math.cos(theta) + Y * math.sin(theta), -X * math.sin(theta) + Y * math.cos(theta)
    fine = np.where((np.floor(d1 / q) + np.floor(d2 / q)) % 2 == 0, float(hi), float(lo))
    return np.rint(fine.reshape(Hb, ss, Wb, ss).mean(axis=(1, 3))).astype(np.uint8)


def test_workflow_a_board_seen_through_a_barrel_lens(torch):
    """6 x 4 corners of a board of 14-pixel squares, turned by 0.5 rad, seen through a lens that moves them by up to 2.7 px
    (``imaging.warp_frames``), refined from starts rounded to whole pixels: they land within the host file's bound of where
    the lens model says they are.  Measured with the oracles of both calls on the host when this was written: 0.105 px worst."""
    Hb, Wb, q, theta, centre = 104, 128, 14.0, 0.5, (63.2, 51.7)
    board = render_board(Hb, Wb, centre[0], centre[1], q, theta)
    ij = np.array([(i - 2, j - 1) for j in range(4) for i in range(6)], dtype=np.float64)
    src = np.stack([centre[0] + q * (ij[:, 0] * math.cos(theta) - ij[:, 1] * math.sin(theta)),
                    centre[1] + q * (ij[:, 0] * math.sin(theta) + ij[:, 1] * math.cos(theta))], axis=1)
    lens = Lens(100.0, 100.0, 63.5, 51.5, 0.25)
    seen = imaging.warp_frames(torch.from_numpy(board[None, :, :, None]).cuda(), lens, inverse_k(100.0, 63.5, 51.5), (Wb, Hb))
    seen = seen[0] if isinstance(seen, tuple) else seen
    predicted = lens.undistort_points(src) * 100.0 + (63.5, 51.5)
    assert 2.0 < np.max(np.hypot(*(predicted - src).T)) < 3.5
    res = imaging.refine_corners(seen, [np.rint(predicted)])
    worst = np.max(np.hypot(*(res.corners[0] - predicted).T))
    print("board through a lens: worst distance to the predicted positions", worst, "px")
    assert np.all(res.ok) and worst <= TRUTH_BOUND
    check(res, batch_oracle(seen.cpu().numpy(), [np.rint(predicted)], channel=0))
    weights = imaging.corner_weights(res)
    assert weights.shape == (24,) and np.all(weights > 0.3) and np.median(weights) == pytest.approx(1.0)
    again = imaging.corner_sub_pix(seen[0, :, :, 0], np.rint(predicted).astype(np.float32).reshape(-1, 1, 2), (3, 3), (-1, -1), (3, 200, 1e-5))
    assert again.shape == (24, 1, 2) and again.dtype == np.float32
    assert np.array_equal(again.reshape(-1, 2), res.xy.astype(np.float32))
