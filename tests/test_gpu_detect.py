"""GPU tests of sba_detect_dots (include/sba_hip.h) through ``lasercalib_amd.feature_detection``: laser-dot moments, boxes,
centroids and statuses of batches of frames.

The reference is ``dots_oracle`` of tests/test_detect_host.py (exact integers; checked there against closed forms, a brute-force
sum, the reference's OpenCV calls written out, and hand-built frames).  The device's sums are exact integers too and each
centroid is one IEEE division of two of them, so EVERY comparison here is bit equality (``same_dots``: np.array_equal, NaNs
matched by position) -- nothing needs a tolerance.  The only bound is the accuracy cap of the host file, on the distance of the
weighted centroid to a rendered spot's true centre.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lasercalib_amd import _native, feature_detection as fd  # noqa: E402
from test_blobs_host import blob_diff, blobs_oracle  # noqa: E402
from test_detect_host import (NONE, OK, RMS_CAP, SPREAD, TOO_LARGE, TOO_SMALL, all_bright_sums, centroid_errors,  # noqa: E402
                              dots_oracle, opencv_restatement, render_spots, same_dots)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert _native.device_count() > 0, "no HIP device visible: GPU tests must run on the MI355X box"


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def pitched(frames, row_pitch, frame_slack, fill=255):
    """A view with the values of `frames` (B, H, W, C) inside a buffer with the given row pitch and frame slack; the padding
    holds `fill` (bright), so reading a byte of it would show."""
    B, H, W, C = frames.shape
    frame_pitch = H * row_pitch + frame_slack
    buf = np.full(B * frame_pitch + 64, fill, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf, shape=(B, H, W, C), strides=(frame_pitch, row_pitch, C, 1))
    view[...] = frames
    return buf, view, frame_pitch


def device_view(torch, buf, shape, strides, offset=0):
    """The same bytes on the device, as a strided uint8 tensor starting `offset` bytes into its allocation."""
    t = torch.from_numpy(buf).cuda()
    return t, torch.as_strided(t, shape, strides, storage_offset=offset)


RANDOM = {}


def random_frames(C):
    """(5, 47, 61, C) random frames: three fifths of the pixels dark, the rest uniform, some exactly 255; shared, never written."""
    if C not in RANDOM:
        rng = np.random.default_rng(40 + C)
        f = rng.integers(0, 256, size=(5, 47, 61, C), dtype=np.uint8)
        f[rng.random(f.shape) < 0.6] = 0
        f[rng.random(f.shape) < 0.02] = 255
        f.setflags(write=False)
        RANDOM[C] = f
    return RANDOM[C]


ORACLE = {}


def oracle_of(C, channel, thr):
    if (C, channel, thr) not in ORACLE:
        ORACLE[C, channel, thr] = dots_oracle(random_frames(C), threshold=thr, channel=channel)
    return ORACLE[C, channel, thr]


# ----------------------------------------------------------------------------- 1. random frames, every layout
@pytest.mark.parametrize("C", [3, 1, 4])
def test_random_frames_host_and_device_every_channel_and_threshold(torch, C):
    frames = random_frames(C)
    B, H, W, _ = frames.shape
    for row_pitch in (W * C, W * C + 5):                                            # C = 3: 183 (packed) and 188
        buf, view, frame_pitch = pitched(frames, row_pitch, 13)
        assert view.strides == (frame_pitch, row_pitch, C, 1)
        keep, dev = device_view(torch, buf, (B, H, W, C), (frame_pitch, row_pitch, C, 1))
        for channel in range(C):
            for thr in (0, 50, 254, 255):
                want = oracle_of(C, channel, thr)
                assert same_dots(fd.find_laser_dots(view, threshold=thr, channel=channel), want), (row_pitch, channel, thr, "host")
                assert same_dots(fd.find_laser_dots(dev, threshold=thr, channel=channel), want), (row_pitch, channel, thr, "device")
                if thr == 255:
                    assert np.all(want.status == NONE) and not want.sums.any()
                else:
                    assert np.all(want.sums[:, 0] > 0)
    if C == 1:                                                                       # (B, H, W) is the one-channel layout
        assert same_dots(fd.find_laser_dots(frames[..., 0], channel=0), oracle_of(1, 0, 50))


def test_misaligned_device_base(torch):
    frames = random_frames(3)
    B, H, W, C = frames.shape
    want = oracle_of(3, 1, 50)
    for offset in (1, 7, 15):
        big = torch.full((B * H * W * C + 32,), 255, dtype=torch.uint8, device="cuda")
        view = big[offset:offset + B * H * W * C].view(B, H, W, C)
        view.copy_(torch.from_numpy(frames.copy()))
        assert view.data_ptr() % 16 == (big.data_ptr() + offset) % 16 and view.data_ptr() % 16 != 0
        assert same_dots(fd.find_laser_dots(view), want), offset


def test_empty_frame_among_frames_with_dots():
    frames = random_frames(3).copy()
    frames[2, :, :, 1] = 50                                  # nothing ABOVE the threshold; the other channels stay bright
    got = fd.find_laser_dots(frames)
    assert same_dots(got, dots_oracle(frames))
    assert got.status[2] == NONE and np.isnan(got.centroid[2]).all() and list(got.box[2]) == [61, 47, -1, -1]
    assert not got.sums[2].any() and np.all(got.status[[0, 1, 3, 4]] == OK) and np.isnan(got.spread_px[2])


# ----------------------------------------------------------------------------- 1b. the seams of the row scanner, both detectors
def seam_frames(W, C):
    """(2, 5, W, C) frames: the other channels random bytes, channel C // 2 zero but for about min(a third of the pixels, 40) of
    random value, some exactly 255, and a few set by hand at both ends of the rows and either side of byte 4096 of a row (one
    step of 64 lanes x 16 bytes x 4 loads in flight): some 40 non-zero pixels a frame at the most, for at most 64 components."""
    rng = np.random.default_rng(1000 * C + W)
    f = rng.integers(0, 256, size=(2, 5, W, C), dtype=np.uint8)
    g = rng.integers(1, 256, size=(2, 5, W), dtype=np.uint8)
    g[rng.random(g.shape) < 0.2] = 255
    g[rng.random(g.shape) >= min(0.3, 35.0 / (5 * W))] = 0
    for y, x in ((0, 0), (2, 1), (2, W - 1), (3, 4096 // C - 1), (3, 4096 // C + 1), (1, W - 2), (4, W - 1)):
        if 0 <= x < W:
            g[:, y, x] = (255, 51)
    f[..., C // 2] = g
    return f


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("W", [1, 5, 16, 17, 1400])
def test_both_detectors_see_the_same_pixels_at_the_seams_of_a_row(torch, W, C):
    """W = 1 and 5 (C = 1): a row that lies wholly in the head or, at a misaligned base, has an empty body; 16: exactly one
    vector; 17: a body with a tail; 1400 x 3 = 4200 bytes: more than one full step of the unrolled loop."""
    frames = seam_frames(W, C)
    n = frames.size
    sources = [("host, a frame per chunk", frames, dict(chunk_frames=1))]
    for offset in (0, 1, 15):
        big = torch.full((n + 32,), 255, dtype=torch.uint8, device="cuda")               # bright around the frames
        view = big[offset:offset + n].view(frames.shape)
        view.copy_(torch.from_numpy(frames))
        assert big.data_ptr() % 16 == 0 and view.data_ptr() % 16 == offset
        sources.append((f"device, base + {offset}", view, {}))
    for roi in [{}] + ([dict(roi_rect=(1, 1, W, 4))] if W > 1 else []):
        kw = dict(threshold=50, channel=C // 2, **roi)
        want_dots = dots_oracle(frames, **kw)
        want_blobs = blobs_oracle(frames, dilate_radius=0, close_radius=0, max_blobs=64, **kw)
        assert 0 < want_blobs.n_components.min() and want_blobs.n_components.max() <= 64, want_blobs.n_components
        for name, src, how in sources:
            dots = fd.find_laser_dots(src, **kw, **how)
            blobs = fd.find_laser_blobs(src, dilate_radius=0, close_radius=0, max_blobs=64, **kw, **how)
            assert same_dots(dots, want_dots), (name, roi)
            assert blob_diff(blobs, want_blobs) is None, (blob_diff(blobs, want_blobs), name, roi)
            for dot_sum, blob_col in ((0, 3), (6, 4), (9, 7)):                           # n = n_raw, sum w, n_sat
                assert np.array_equal(dots.sums[:, dot_sum], blobs.blobs[:, :, blob_col].sum(axis=1)), (name, roi, dot_sum)


# ----------------------------------------------------------------------------- 2. where a 32-bit partial sum overflows
@pytest.mark.parametrize("H,W,C,thr", [(2200, 3208, 3, 50), (8, 16384, 1, 0), (16384, 8, 1, 254)])
def test_all_255_frames_match_the_closed_forms(torch, H, W, C, thr):
    frames = torch.full((2, H, W, C), 255, dtype=torch.uint8, device="cuda")
    got = fd.find_laser_dots(frames, threshold=thr, channel=C // 2)
    want = all_bright_sums(H, W, thr)
    assert want[3] > 2 ** 32 or want[4] > 2 ** 32
    for f in range(2):
        assert [int(v) for v in got.sums[f]] == want
        assert list(got.box[f]) == [0, 0, W - 1, H - 1] and got.status[f] == OK
        assert tuple(got.centroid[f]) == (float(want[1]) / want[0], float(want[2]) / want[0], float(want[7]) / want[6], float(want[8]) / want[6])
    if C == 1:                                               # the same frames from the host, staged one frame at a time
        host = fd.find_laser_dots(np.full((2, H, W), 255, np.uint8), threshold=thr, channel=0, chunk_frames=1)
        assert same_dots(host, got)


# ----------------------------------------------------------------------------- 3. regions and status rules
REGIONS = [("rect", dict(roi_rect=(5, 3, 40, 30)), False), ("circle", dict(roi_circle=(30, 20, 17)), False),
           ("both", dict(roi_rect=(20, 0, 61, 25), roi_circle=(30, 20, 17)), False),
           ("rect-partly-outside", dict(roi_rect=(-9, 40, 33, 500)), False), ("circle-partly-outside", dict(roi_circle=(66, -3, 12)), False),
           ("circle-covers-all", dict(roi_circle=(30, 20, 100000)), False), ("one-column", dict(roi_rect=(1, 0, 2, 47)), False),
           ("rect-empty", dict(roi_rect=(17, 5, 17, 40)), True), ("disjoint", dict(roi_rect=(50, 0, 61, 47), roi_circle=(10, 20, 9)), True)]


@pytest.mark.parametrize("name,roi,keeps_nothing", REGIONS, ids=[r[0] for r in REGIONS])
def test_regions(torch, name, roi, keeps_nothing):
    frames = random_frames(3)
    want = dots_oracle(frames, **roi)
    assert np.all(want.status == NONE) if keeps_nothing else np.all(want.sums[:, 0] > 0)
    assert same_dots(fd.find_laser_dots(frames, **roi), want)
    assert same_dots(fd.find_laser_dots(torch.from_numpy(frames.copy()).cuda(), **roi), want)


def test_status_rules():
    f = np.zeros((3, 40, 50, 3), np.uint8)
    f[0, 10:13, 20:23, 1] = 220                              # one blob, n = 9, extent 3
    f[1, 10:13, 20:23, 1] = 220
    f[1, 30:33, 40:43, 1] = 220                              # two distant blobs, n = 18, extent 23
    for kw, want in ((dict(max_extent=5), [OK, SPREAD, NONE]), (dict(max_extent=3), [OK, SPREAD, NONE]),
                     (dict(max_extent=2), [SPREAD, SPREAD, NONE]), (dict(max_extent=23), [OK, OK, NONE]),
                     (dict(min_area=9), [OK, OK, NONE]), (dict(min_area=10), [TOO_SMALL, OK, NONE]),
                     (dict(max_area=9), [OK, TOO_LARGE, NONE]), (dict(max_area=8), [TOO_LARGE, TOO_LARGE, NONE]),
                     (dict(min_area=19, max_area=1, max_extent=1), [TOO_SMALL, TOO_SMALL, NONE])):
        got = fd.find_laser_dots(f, **kw)
        assert list(got.status) == want, kw
        assert same_dots(got, dots_oracle(f, **kw))
    got = fd.find_laser_dots(f, max_extent=5)
    table = fd.centroid_table(got)
    assert tuple(table[0]) == (11.0, 21.0) and np.isnan(table[1:]).all()
    assert tuple(fd.centroid_table(got, accept=(OK, SPREAD))[1]) == (21.0, 31.0)


# ----------------------------------------------------------------------------- 4. chunking, repeatability, arguments
def test_chunking_and_repeatability(torch):
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, size=(9, 31, 45, 3), dtype=np.uint8)
    frames[rng.random(frames.shape) < 0.5] = 0
    frames[4] = 0
    want = dots_oracle(frames, max_extent=40)
    one = fd.find_laser_dots(frames, max_extent=40, chunk_frames=9)
    assert same_dots(one, want)
    for chunk in (2, 1, 4, 0):
        assert same_dots(fd.find_laser_dots(frames, max_extent=40, chunk_frames=chunk), want), chunk
    # host frames in each class of layout a pitched copy tells apart -- packed, padded rows, a gap between packed frames, both --
    # in five chunks, the last one short: both staging buffers are used again; the padding is bright
    for row_slack, frame_slack in ((0, 0), (5, 0), (0, 13), (5, 13)):
        _buf, view, _fp = pitched(frames, 45 * 3 + row_slack, frame_slack)
        assert same_dots(fd.find_laser_dots(view, max_extent=40, chunk_frames=2), want), (row_slack, frame_slack)
    dev = torch.from_numpy(frames).cuda()
    assert same_dots(fd.find_laser_dots(dev, max_extent=40), want)
    again = fd.find_laser_dots(dev, max_extent=40)
    assert same_dots(again, one) and again.sums.tobytes() == one.sums.tobytes() and again.centroid.tobytes() == one.centroid.tobytes()
    # n_frames = 0 writes nothing
    lib = _native.load()
    sums, box = np.full(12, 7, np.uint64), np.full(4, 7, np.int32)
    cen, st = np.full(4, 7.0), np.full(1, 7, np.int32)
    rc = lib.sba_detect_dots(0, frames.ctypes.data, 0, 31, 45, 3, 135, 31 * 135, None, sums.ctypes.data, box.ctypes.data,
                             cen.ctypes.data, st.ctypes.data)
    assert rc == 0 and np.all(sums == 7) and np.all(box == 7) and np.all(cen == 7.0) and st[0] == 7
    assert len(fd.find_laser_dots(np.zeros((0, 31, 45, 3), np.uint8)).status) == 0


def test_null_options_are_the_reference_defaults_and_outputs_are_optional():
    frames = random_frames(3)
    lib = _native.load()
    want = oracle_of(3, 1, 50)
    sums, st = np.zeros((5, 12), np.uint64), np.zeros(5, np.int32)
    rc = lib.sba_detect_dots(0, frames.ctypes.data, 5, 47, 61, 3, 183, 47 * 183, None, sums.ctypes.data, None, None, st.ctypes.data)
    assert rc == 0 and np.array_equal(sums, want.sums) and np.array_equal(st, want.status)


def test_rejected_arguments():
    lib = _native.load()
    frames = np.zeros((2, 8, 10, 3), np.uint8)
    p = frames.ctypes.data
    INVALID, UNSUPPORTED = -1, -6

    def call(ptr=p, n=2, h=8, w=10, c=3, rp=30, fp=240, **o):
        opts = _native.DotOpts(channel=1, threshold=50)
        for k, v in o.items():
            setattr(opts, k, v)
        out = np.zeros(24, np.uint64)
        rc = lib.sba_detect_dots(0, ptr, n, h, w, c, rp, fp, ctypes.byref(opts), out.ctypes.data, None, None, None)
        return rc, (lib.sba_last_error(None) or b"").decode()

    assert call()[0] == 0
    for kw, code in ((dict(ptr=None), INVALID), (dict(c=2), INVALID), (dict(c=0), INVALID), (dict(channel=3), INVALID),
                     (dict(channel=-1), INVALID), (dict(c=1, rp=10, fp=80, channel=1), INVALID), (dict(threshold=256), INVALID),
                     (dict(threshold=-1), INVALID), (dict(rp=29), INVALID), (dict(fp=239), INVALID), (dict(n=-1), INVALID),
                     (dict(h=-1), INVALID), (dict(w=-1), INVALID), (dict(w=16385, rp=3 * 16385, fp=8 * 3 * 16385), UNSUPPORTED),
                     (dict(h=16385, fp=16385 * 30), UNSUPPORTED)):
        rc, msg = call(**kw)
        assert rc == code and msg, (kw, rc, msg)
    assert call(ptr=None, n=0)[0] == 0


# ----------------------------------------------------------------------------- 5. full-size frames
def test_full_size_frames_against_the_reference_and_the_true_centre(torch):
    rng = np.random.default_rng(21)
    H, W, S = 2200, 3208, 33
    spots, centres = render_spots(4, S, rng)
    frames = np.repeat(rng.integers(0, 31, size=(1, H, W, 3), dtype=np.uint8), 4, axis=0)        # dark noise, all channels
    corner = [(17, 5), (W - S - 3, H - S - 1), (1601, 1093), (2999, 40)]
    for f, (x0, y0) in enumerate(corner):
        frames[f, y0:y0 + S, x0:x0 + S, 1] = spots[f]
    truth = centres + np.asarray(corner, dtype=np.float64)
    got = fd.find_laser_dots(frames, threshold=50, max_extent=40)
    dev = fd.find_laser_dots(torch.from_numpy(frames).cuda(), threshold=50, max_extent=40)
    assert same_dots(got, dev) and np.all(got.status == OK)
    assert same_dots(got, dots_oracle(frames, threshold=50, max_extent=40))
    ref = [opencv_restatement(frames[f], 50) for f in range(4)]
    for f in (0, 3):
        assert fd.green_laser_finder_faster(frames[f], 50) == ref[f]
    assert [tuple(r) for r in fd.centroid_table(got, subpixel=False)] == ref
    err = centroid_errors(got, truth)[2]
    print(f"weighted centroid to true centre, px: {err}")
    assert np.sqrt(np.mean(err ** 2)) <= RMS_CAP["weighted"]
