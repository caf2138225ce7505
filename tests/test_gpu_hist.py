"""GPU tests of sba_frame_histograms (include/sba_hip.h) through ``lasercalib_amd.imaging.frame_histograms``: the 256-bin
histogram of one channel of every frame of a batch, and the running total of a video.

The reference is ``hist_oracle`` of tests/test_hist_host.py (np.bincount over the region mask of the laser-dot oracle, pinned there
to a brute-force loop and to that oracle's counts).  Every count is an integer, so EVERY comparison here is bit equality.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lasercalib_amd import _native, feature_detection as fd, imaging  # noqa: E402
from test_detect_host import render_spots  # noqa: E402
from test_gpu_convert import rendered_video  # noqa: E402
from test_gpu_detect import device_view, pitched, random_frames  # noqa: E402
from test_hist_host import hist_oracle  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert _native.device_count() > 0, "no HIP device visible: GPU tests must run on the MI355X box"


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def check(got, want, preload=None, what=None):
    """`got` holds exactly the rows `want` and their sum on top of `preload`."""
    assert got.hist.dtype == np.uint32 and got.hist.shape == want.shape and got.total.dtype == np.uint64 and got.total.shape == (256,)
    assert np.array_equal(got.hist, want), what
    base = np.zeros(256, np.uint64) if preload is None else preload
    assert np.array_equal(got.total, base + want.sum(axis=0, dtype=np.uint64)), what


def on_device(torch, frames, offset=0, fill=253):
    """The frames packed on the device, `offset` bytes into an allocation filled with `fill`."""
    big = torch.full((frames.size + 32,), fill, dtype=torch.uint8, device="cuda")
    view = big[offset:offset + frames.size].view(frames.shape)
    view.copy_(torch.from_numpy(np.array(frames)))            # a writable copy
    assert big.data_ptr() % 16 == 0
    return view


ORACLE = {}


def oracle_of(C, channel, limited):
    if (C, channel, limited) not in ORACLE:
        f = random_frames(C)
        ORACLE[C, channel, limited] = hist_oracle(np.minimum(f, 250) if limited else f, channel)
    return ORACLE[C, channel, limited]


# ----------------------------------------------------------------------------- 1. random frames, every layout
@pytest.mark.parametrize("C", [3, 1, 4])
def test_random_frames_host_and_device_every_channel_and_pitch(torch, C):
    for limited in (False, True):                            # limited: values 0..250 and the padding 253 -- a byte of it would show
        frames = np.minimum(random_frames(C), 250) if limited else random_frames(C)
        B, H, W, _ = frames.shape
        for row_pitch in (W * C, W * C + 5):
            buf, view, frame_pitch = pitched(frames, row_pitch, 13, fill=253)
            _keep, dev = device_view(torch, buf, (B, H, W, C), (frame_pitch, row_pitch, C, 1))
            for channel in range(C):
                want = oracle_of(C, channel, limited)
                assert want[:, 0].min() > 0.5 * H * W and (limited or want[:, 255].min() > 0) and not (limited and want[:, 251:].any())
                check(imaging.frame_histograms(view, channel=channel), want, what=(limited, row_pitch, channel, "host"))
                check(imaging.frame_histograms(dev, channel=channel), want, what=(limited, row_pitch, channel, "device"))
    if C == 1:                                               # (B, H, W) is the one-channel layout
        check(imaging.frame_histograms(random_frames(1)[..., 0], channel=0), oracle_of(1, 0, False))


def test_misaligned_device_base(torch):
    frames = np.minimum(random_frames(3), 250)
    for offset in (1, 7, 15):
        view = on_device(torch, frames, offset)
        assert view.data_ptr() % 16 == offset
        check(imaging.frame_histograms(view), oracle_of(3, 1, True), what=offset)


# ----------------------------------------------------------------------------- 2. the seams of a row and of a band
def seam_frames(H, W, C):
    """(3, H, W, C) frames of values 0..250: random bytes; the constant 9 but for one pixel in ten; the constant 9."""
    rng = np.random.default_rng(7000 * C + 10 * W + H)
    f = rng.integers(0, 251, size=(3, H, W, C), dtype=np.uint8)
    f[1][rng.random((H, W, C)) >= 0.1] = 9
    f[2] = 9
    return f


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("W", [1, 15, 16, 17, 63, 64, 65, 341, 342, 1023, 1024, 1025, 1365, 1366, 4097])
def test_widths_either_side_of_a_group_a_wave_and_an_unrolled_step(torch, W, C):
    """16 bytes are a lane's group, 1024 a wave's load, 4096 one step of four loads in flight: W C falls on either side of each."""
    frames = seam_frames(5, W, C)
    for channel in sorted({0, C // 2, C - 1}):
        want = hist_oracle(frames, channel)
        check(imaging.frame_histograms(frames, channel=channel, chunk_frames=2), want, what=("host", channel))
        for offset in (0, 1, 15):
            check(imaging.frame_histograms(on_device(torch, frames, offset), channel=channel), want, what=(offset, channel))
    if W > 2:                                                # a region that starts and ends inside the row
        roi = dict(roi_rect=(1, 1, W - 1, 4))
        check(imaging.frame_histograms(on_device(torch, frames, 3), channel=C // 2, **roi), hist_oracle(frames, C // 2, **roi))


@pytest.mark.parametrize("H", [1, 3, 4, 5, 31, 32, 33, 65])
def test_heights_either_side_of_the_rows_of_a_wave_and_of_a_band(torch, H):
    """Four waves take a row each; a band is 4 to 32 rows."""
    frames = seam_frames(H, 61, 3)
    want = hist_oracle(frames, 1)
    check(imaging.frame_histograms(frames), want)
    check(imaging.frame_histograms(on_device(torch, frames, 5)), want)
    many = np.ascontiguousarray(np.tile(frames, (100, 1, 1, 1)))         # 300 frames: H = 65 makes bands of 8 rows, two a wave
    check(imaging.frame_histograms(on_device(torch, many)), np.tile(want, (100, 1)))


# ----------------------------------------------------------------------------- 3. equal values: the register count
def test_constant_frames_and_frames_that_break_the_constant(torch):
    H, W = 47, 61
    frames = np.zeros((8, H, W, 3), np.uint8)
    frames[1], frames[2] = 7, 255
    frames[3, 0::2], frames[3, 1::2] = 11, 200               # rows alternate between two constants
    frames[4, 0::4], frames[4, 1::4], frames[4, 2::4], frames[4, 3::4] = 1, 2, 1, 3     # so do the rows of ONE wave
    frames[5] = 40
    for k, x in enumerate((0, 15, 16, W - 1)):               # uniform but for one pixel at either end of a row and of a group
        frames[5, 3 + 5 * k, x, 1] = 41 + k
    frames[6] = 40
    frames[6, :, 0, 1] = 250                                 # the first pixel of every row, which the register count is taken from, is the odd one
    frames[7, :, :, 1] = np.arange(W, dtype=np.uint8)[None, :]           # no two neighbours alike
    want = hist_oracle(frames, 1)
    assert list(want[[0, 1, 2], [0, 7, 255]]) == [H * W] * 3 and want[5, 40] == H * W - 4 and want[6, 250] == H
    for channel in (0, 1, 2):
        check(imaging.frame_histograms(frames, channel=channel), hist_oracle(frames, channel), what=channel)
        for offset in (0, 9):
            check(imaging.frame_histograms(on_device(torch, frames, offset), channel=channel), hist_oracle(frames, channel), what=(channel, offset))
    for C in (1, 4):
        f = np.ascontiguousarray(np.repeat(frames[..., 1:2], C, axis=3))
        check(imaging.frame_histograms(on_device(torch, f, 4), channel=C - 1), want, what=C)


def test_full_size_constant_frames_with_a_spot(torch):
    """32 frames of 3208 x 2200 x 3 make bands of 32 rows: 102 656 pixels of a band fall into one bin, more than 16 bits hold; the
    9 x 9 spot breaks the constant in the middle of nine rows."""
    H, W, B = 2200, 3208, 32
    frames = torch.full((B, H, W, 3), 7, dtype=torch.uint8, device="cuda")
    spot = np.random.default_rng(4).integers(100, 256, size=(9, 9), dtype=np.uint8)
    spot[4, 4], spot[0, 0] = 255, 7
    frames[5, 1001:1010, 1601:1610, 1] = torch.from_numpy(spot).cuda()
    want = np.zeros((B, 256), np.uint32)
    want[:, 7] = H * W
    want[5] = hist_oracle(np.pad(spot, 3, constant_values=7)[None], 0)[0]
    want[5, 7] += H * W - 15 * 15
    assert want[5].sum() == H * W and want[5, 7] == H * W - 80
    check(imaging.frame_histograms(frames), want)
    check(imaging.frame_histograms(frames, channel=0), np.tile(want[:1], (B, 1)))
    again = imaging.frame_histograms(frames)
    assert again.hist.tobytes() == want.tobytes()                         # two calls return the same bits


@pytest.mark.parametrize("H,W", [(16384, 8), (8, 16384)])
def test_the_largest_dimension_all_255(torch, H, W):
    frames = torch.full((2, H, W, 1), 255, dtype=torch.uint8, device="cuda")
    want = np.zeros((2, 256), np.uint32)
    want[:, 255] = 131072
    got = imaging.frame_histograms(frames, channel=0)
    check(got, want)
    assert list(got.n_saturated()) == [131072] * 2 and list(got.vmin()) == [255] * 2
    check(imaging.frame_histograms(np.full((2, H, W), 255, np.uint8), channel=0, chunk_frames=1), want)


# ----------------------------------------------------------------------------- 4. regions
REGIONS = [("rect-odd-edges", dict(roi_rect=(5, 3, 40, 30)), False), ("circle-partly-outside", dict(roi_circle=(66, -3, 22)), False),
           ("both", dict(roi_rect=(21, 1, 61, 25), roi_circle=(30, 20, 17)), False), ("rect-partly-outside", dict(roi_rect=(-9, 40, 33, 500)), False),
           ("rect-empty", dict(roi_rect=(17, 5, 17, 40)), True), ("disjoint", dict(roi_rect=(50, 0, 61, 47), roi_circle=(10, 20, 9)), True)]


@pytest.mark.parametrize("name,roi,keeps_nothing", REGIONS, ids=[r[0] for r in REGIONS])
def test_regions_and_the_count_of_the_dot_detector(torch, name, roi, keeps_nothing):
    frames = random_frames(3)
    dev = on_device(torch, frames, 0)
    want = hist_oracle(frames, 1, **roi)
    assert not want.any() if keeps_nothing else want.sum(axis=1).min() > 0
    preload = np.arange(256, dtype=np.uint64) + (1 << 40)
    check(imaging.frame_histograms(frames, total=preload, **roi), want, preload)          # an empty region: zeros, and the total unchanged
    got = imaging.frame_histograms(dev, total=preload, **roi)
    check(got, want, preload)
    above = got.count_above()
    for t in (0, 50, 200):
        assert np.array_equal(above[:, t], fd.find_laser_dots(dev, threshold=t, **roi).sums[:, 0].astype(np.int64)), t
    assert np.array_equal(got.n_saturated(), fd.find_laser_dots(dev, threshold=0, **roi).sums[:, 9].astype(np.int64))


# ----------------------------------------------------------------------------- 5. chunking and the running total
def test_chunking_streaming_and_the_preloaded_total(torch):
    rng = np.random.default_rng(12)
    frames = rng.integers(0, 256, size=(7, 31, 45, 3), dtype=np.uint8)
    frames[rng.random(frames.shape) < 0.5] = 0
    frames[4] = 0
    want = hist_oracle(frames, 1)
    preload = np.arange(256, dtype=np.uint64) + (1 << 40)
    end = preload + want.sum(axis=0, dtype=np.uint64)
    for chunk in (1, 2, 3, 7, 0):
        check(imaging.frame_histograms(frames, total=preload, chunk_frames=chunk), want, preload, what=chunk)
        _buf, view, _fp = pitched(frames, 45 * 3 + 5, 13, fill=253)
        check(imaging.frame_histograms(view, total=preload, chunk_frames=chunk), want, preload, what=(chunk, "pitched"))
    assert np.array_equal(preload, np.arange(256, dtype=np.uint64) + (1 << 40))            # the total handed in is not written
    dev = torch.from_numpy(frames).cuda()
    for a, b in ((slice(0, 3), slice(3, 7)), (slice(3, 7), slice(0, 3)), (slice(5, 7), slice(0, 5))):   # two calls, in either order
        first = imaging.frame_histograms(frames[a], total=preload, chunk_frames=2)
        second = imaging.frame_histograms(dev[b], total=first)                              # a previous result is continued
        assert np.array_equal(second.total, end) and np.array_equal(first.hist, want[a]) and np.array_equal(second.hist, want[b])
    for src in (frames, dev):
        only = imaging.frame_histograms(src, total=preload, per_frame=False, chunk_frames=3)
        assert only.hist is None and np.array_equal(only.total, end)
    lib = _native.load()                                     # no frame, or no output asked for: nothing is written
    hist, total = np.full((7, 256), 9, np.uint32), np.full(256, 9, np.uint64)
    assert lib.sba_frame_histograms(0, frames.ctypes.data, 0, 31, 45, 3, 135, 31 * 135, None, hist.ctypes.data, total.ctypes.data) == 0
    assert lib.sba_frame_histograms(0, frames.ctypes.data, 7, 31, 45, 3, 135, 31 * 135, None, None, None) == 0
    assert np.all(hist == 9) and np.all(total == 9)
    assert lib.sba_frame_histograms(0, frames.ctypes.data, 7, 31, 45, 3, 135, 31 * 135, None, hist.ctypes.data, None) == 0     # NULL options: channel 1
    assert np.array_equal(hist, want) and np.all(total == 9)
    empty = imaging.frame_histograms(np.zeros((0, 31, 45, 3), np.uint8), total=preload)
    assert empty.hist.shape == (0, 256) and np.array_equal(empty.total, preload)


# ----------------------------------------------------------------------------- 6. the planes the detectors read
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_decoder_frames_and_the_background_go_the_detectors_way(torch, device):
    y, uv = rendered_video()                                 # 12 frames of 96 x 128, NV12
    nv12 = (torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()) if device else (y, uv)
    green = imaging.convert_frames(nv12, "nv12", out_format="g")
    want = hist_oracle(green.cpu().numpy() if device else green, 0)
    roi = dict(roi_circle=(60, 50, 45))
    for chunk in (0, 5):
        check(imaging.frame_histograms(nv12, pixel_format="nv12", chunk_frames=chunk), want, what=chunk)
    check(imaging.frame_histograms(nv12, pixel_format="nv12", **roi), hist_oracle(green.cpu().numpy() if device else green, 0, **roi))
    only = imaging.frame_histograms(nv12, pixel_format="nv12", per_frame=False, chunk_frames=5)
    assert only.hist is None and np.array_equal(only.total, want.sum(axis=0, dtype=np.uint64))
    bgr = imaging.convert_frames(nv12, "nv12", out_format="bgr")
    model = imaging.BackgroundModel(96, 128, channel=1, threshold=40).add(bgr)
    level, mask = model.level(k_sigma=1.0), model.hot_mask(0.5)
    clean = model.suppress(bgr, level=level, mask=mask)
    want = hist_oracle(clean.cpu().numpy() if device else clean, 0)
    assert want[:, 0].min() > 0 and want[:, 100:].any()      # the background is gone, the dots are not
    preload = np.full(256, 1 << 40, np.uint64)
    for chunk in (0, 5):
        check(imaging.frame_histograms(bgr, background=(level, mask), total=preload, chunk_frames=chunk), want, preload, what=chunk)
    check(imaging.frame_histograms(nv12, pixel_format="nv12", background=(level, mask), chunk_frames=5), want)
    clean = model.suppress(bgr)                              # the model itself: its default level and mask
    check(imaging.frame_histograms(bgr, background=model), hist_oracle(clean.cpu().numpy() if device else clean, 0))


# ----------------------------------------------------------------------------- 7. the workflow: a threshold for a new video
def test_the_suggested_threshold_makes_the_detector_accept_every_frame(torch):
    rng = np.random.default_rng(31)
    spots, _centres = render_spots(24, 65, rng, sigma=(1.5, 3.0), amp=(180.0, 255.0), noise=20)
    frames = np.zeros((24, 65, 65, 3), np.uint8)
    frames[..., 1] = spots
    frames[..., 0] = 255                                     # a bright OTHER channel changes nothing
    oracle = imaging.FrameHistograms(hist_oracle(frames, 1), None)
    at50 = oracle.count_above()[:, 50]
    min_area, max_area = int(at50.min()), int(at50.max())
    assert min_area >= 4 and oracle.vmax().min() > 150       # a dot in every frame; the noise floor is 20
    t_cpu = oracle.suggest_threshold(min_area, max_area)     # the oracle alone satisfies the condition ...
    assert t_cpu is not None and oracle.threshold_table(min_area, max_area)[t_cpu] == 24
    above = oracle.count_above()[:, t_cpu]
    assert np.all((above >= min_area) & (above <= max_area))
    got = imaging.frame_histograms(torch.from_numpy(frames).cuda())      # ... and so does the device
    t = got.suggest_threshold(min_area, max_area)
    assert t == t_cpu and t > 20
    dots = fd.find_laser_dots(frames, threshold=t, min_area=min_area, max_area=max_area)
    assert np.all(dots.status == fd.SBA_DOT_OK), dots.status
    assert np.all(fd.find_laser_dots(frames, threshold=10, min_area=min_area, max_area=max_area).status == fd.SBA_DOT_TOO_LARGE)
