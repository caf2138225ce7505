"""GPU tests of sba_adaptive_threshold (include/sba_hip.h) through ``lasercalib_amd._native``, ``lasercalib_amd.imaging`` and the
raw C ABI.

The reference is ``adaptive_oracle`` of tests/test_adaptive_host.py, the header's rule in numpy with int64 sums (pinned there
to answers known without it).  The rule is exact -- integer sums, the integer nearest to S / b^2 --, so EVERY comparison here
is bit equality of masks AND means; nothing needs a tolerance.  Buffers with padding are pre-filled with a sentinel and
compared whole, so a byte written into the padding shows.

The boundaries of the kernel (csrc/sba_adaptive.hpp) that the shapes below straddle.  A wave reads a row of a workgroup's tile
with its halo -- L = R + 1 rounded up to four columns on the left, R = b / 2 on the right -- four columns per lane, 256 per
step; a lane reads words where its four pixels lie inside the frame and the address is aligned, single bytes clamped to the
frame elsewhere.  Up to window 97 the tile is as wide as one step allows (232 columns at window 23, 248 at 3, 200 at 51, 172
at 81), 64 rows up to window 65 and 32 beyond, in one segment of rows; window 101 takes 128 x 32 in two segments of 16 rows
and two steps, window 127 takes 64 x 32 in four segments of 8.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lasercalib_amd import _native, imaging  # noqa: E402
from test_adaptive_host import adaptive_oracle, workflow_scene  # noqa: E402

SENTINEL = 0xA5
CUSTOM = (11000, 768, 21000)                                  # weights that no standard has; they sum to 2^15
H0, W0 = 97, 131


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert _native.device_count() > 0, "no HIP device visible: GPU tests must run on the MI355X box"


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


FRAMES = {}


def random_frames(B, H, W, C, lo=0, hi=256):
    """Uniform random frames (B, H, W, C), or (B, H, W) for C = 0; shared, never written."""
    key = (B, H, W, C, lo, hi)
    if key not in FRAMES:
        a = np.random.default_rng(1000 * H + 10 * W + C).integers(lo, hi, size=(B, H, W) + ((C,) if C else ()), dtype=np.uint8)
        a.setflags(write=False)
        FRAMES[key] = a
    return FRAMES[key]


def host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def check(frames, blocks, deltas=None, invert=True, max_value=255, channel=None, gray_w=None, **kw):
    """One call for masks and means against the oracle, bit for bit -> (masks, means) as numpy arrays."""
    deltas = (7,) * len(blocks) if deltas is None else deltas
    f = host(frames)
    channel = (0 if f.ndim == 3 or f.shape[3] == 1 else -1) if channel is None else channel
    masks, means = _native.adaptive_threshold(frames, blocks, deltas, invert=invert, max_value=max_value, channel=channel,
                                              gray_w=gray_w, mean_out=True, **kw)
    masks, means = host(masks), host(means)
    want_masks, want_means = adaptive_oracle(f if f.ndim == 3 or f.shape[3] > 1 else f[..., 0], blocks, deltas, invert, max_value,
                                             channel, gray_w)
    assert masks.shape == means.shape == (len(blocks),) + f.shape[:3]
    assert np.array_equal(means, want_means), f"means differ at {np.argwhere(means != want_means)[:4].tolist()}"
    assert np.array_equal(masks, want_masks), f"masks differ at {np.argwhere(masks != want_masks)[:4].tolist()}"
    return masks, means


def test_constants_are_those_of_the_kernel():
    src = open(os.path.join(os.path.dirname(_native.__file__), "csrc", "sba_adaptive.hpp")).read()
    assert "constexpr int AT_RUN = 4;" in src and "constexpr int AT_STEP = 64 * AT_RUN;" in src and "constexpr int AT_THREADS = 256" in src
    assert "constexpr int AT_LDS_VALUES = 32768;" in src and "constexpr int AT_ONE_STEP_R = 48, AT_TALL_R = 32;" in src
    assert _native.ADAPTIVE_STEP == 64 * 4
    tiles = {b: _native.adaptive_tile(b) for b in (3, 13, 23, 51, 65, 67, 81, 97, 99, 101, 105, 107, 127)}
    assert tiles == {3: (248, 64, 1), 13: (240, 64, 1), 23: (232, 64, 1), 51: (200, 64, 1), 65: (188, 64, 1), 67: (184, 32, 1),
                     81: (172, 32, 1), 97: (156, 32, 1), 99: (128, 32, 2), 101: (128, 32, 2), 105: (128, 32, 2), 107: (64, 32, 4),
                     127: (64, 32, 4)}, tiles


@pytest.mark.parametrize("C,channel", [(0, 0), (1, 0), (3, 0), (3, 1), (3, 2), (3, -1), (4, 0), (4, 1), (4, 2), (4, 3), (4, -1)])
def test_channels_and_gray(C, channel):
    check(random_frames(2, H0, W0, C), (3, 13, 23), channel=channel)


def test_custom_gray_weights():
    for C in (3, 4):
        masks, _ = check(random_frames(2, H0, W0, C), (5, 23), channel=-1, gray_w=CUSTOM)
        other, _ = adaptive_oracle(random_frames(2, H0, W0, C), (5, 23), (7, 7), True, 255, -1)
        assert not np.array_equal(masks, other)                             # the weights matter on these frames
    check(random_frames(2, H0, W0, 3), (5,), channel=-1, gray_w=(0, 0, 0))  # all zero: OpenCV's


@pytest.mark.parametrize("blocks", [(3,), (3, 13, 23), (127,), (5, 127, 3, 63), (23, 23), (51,), (81, 7), (101,)])
def test_window_lists(blocks):
    check(random_frames(2, H0, W0, 0), blocks)
    check(random_frames(2, H0, W0, 3), blocks)


@pytest.mark.parametrize("invert", (True, False))
def test_threshold_types_deltas_and_max_values(invert):
    frames = random_frames(2, H0, W0, 0, 100, 116)                          # a narrow band: |v - mean| is of the order of the deltas
    for delta in (-256, -3, 0, 7, 256):
        masks, _ = check(frames, (3, 13), (delta, delta), invert=invert)
        if abs(delta) == 256:
            assert np.all(masks == (255 if (delta < 0) == invert else 0))
        else:
            assert 0 < np.count_nonzero(masks) < masks.size
    for max_value in (1, 200, 255):
        masks, _ = check(frames, (13,), (3,), invert=invert, max_value=max_value)
        assert set(np.unique(masks)) == {0, max_value}
    check(frames, (3, 5, 7, 9), (-3, 0, 7, 2), invert=invert)               # a delta per window


# either side of: the tile's 232 columns and 64 rows, the four columns of a lane (widths 244 to 246 and 11, 12: the right edge
# cuts a lane's pixels at every position), and frames narrower or lower than the halo
SHAPES_23 = [(63, 231), (64, 232), (65, 233), (66, 234), (129, 465), (2, 244), (3, 245), (5, 246), (11, 12), (12, 11), (23, 24), (1, 300),
             (130, 1)]


@pytest.mark.parametrize("H,W", SHAPES_23)
def test_shapes_around_the_tile_of_the_small_windows(H, W):
    check(random_frames(1, H, W, 0), (3, 13, 23))
    check(random_frames(1, H, W, 3), (23,))
    if H < 10:
        check(random_frames(1, H, W + 16, 0), (3,))                         # window 3 alone: 248 columns


@pytest.mark.parametrize("b,shapes", [(51, [(63, 199), (64, 200), (65, 201), (66, 401)]),
                                      (81, [(31, 171), (32, 172), (33, 173), (65, 345)]),
                                      (101, [(15, 127), (16, 128), (17, 129), (33, 257), (31, 130)]),
                                      (127, [(7, 63), (8, 64), (9, 65), (33, 129), (16, 128), (31, 130)])])
def test_shapes_around_the_tiles_and_row_segments_of_the_large_windows(b, shapes):
    for H, W in shapes:
        check(random_frames(1, H, W, 0), (b,))
    check(random_frames(1, shapes[2][0], shapes[2][1], 4), (b, 3))


@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (5, 1), (2, 3)])
def test_frames_smaller_than_the_window(H, W):
    for C in (0, 3):
        check(random_frames(3, H, W, C), (3, 23, 127))
    if (H, W) == (1, 5):
        row = np.array([[[0, 40, 80, 120, 160]]], np.uint8)
        masks, means = check(row, (23,), (0,))
        assert means[0, 0].tolist() == [[66, 73, 80, 87, 94]] and masks[0, 0].tolist() == [[255, 255, 255, 0, 0]]


def patterns(H, W):
    y, x = np.mgrid[:H, :W]
    rng = np.random.default_rng(3)
    return {"all 255": np.full((H, W), 255, np.uint8), "all 0": np.zeros((H, W), np.uint8),
            "254 or 255": rng.integers(254, 256, size=(H, W), dtype=np.uint8), "checkerboard": (((x + y) & 1) * 255).astype(np.uint8),
            "rows": ((y & 1) * 255 + 0 * x).astype(np.uint8), "columns": ((x & 1) * 255 + 0 * y).astype(np.uint8)}


@pytest.mark.parametrize("blocks", [(3, 13, 23), (127, 5), (63,)])
def test_value_patterns_that_stress_the_sums(blocks):
    frames = np.stack(list(patterns(H0, W0 + 200).values()))               # 331 columns: the running sums of a row wrap 16 bits
    for delta in (0, 1):
        check(frames, blocks, (delta,) * len(blocks))
    check(np.repeat(frames[..., None], 3, axis=3), blocks)                   # grey of equal channels is the value itself


def test_full_size_frame_with_the_windows_of_the_marker_search():
    check(random_frames(1, 2200, 3208, 3), imaging.marker_threshold_windows())


@pytest.mark.parametrize("src_dev,out_dev", [(False, False), (False, True), (True, False), (True, True)])
def test_host_and_device_on_either_side(torch, src_dev, out_dev):
    frames = random_frames(3, H0, W0, 3)
    src = torch.from_numpy(frames.copy()).cuda() if src_dev else frames
    masks, means = _native.adaptive_threshold(src, (3, 13, 23), (7, 7, 7), mean_out=True, out_on_device=out_dev)
    assert _native._is_tensor(masks) == _native._is_tensor(means) == out_dev
    want = adaptive_oracle(frames, (3, 13, 23), (7, 7, 7))
    assert np.array_equal(host(masks), want[0]) and np.array_equal(host(means), want[1])


@pytest.mark.parametrize("src_off,out_off", [(1, 15), (7, 1), (15, 7), (0, 0)])
@pytest.mark.parametrize("on_device", (False, True))
def test_padded_unaligned_source_and_outputs_through_the_c_abi(torch, on_device, src_off, out_off):
    """Bases off by 1, 7 and 15 bytes independently, padded rows, frames and windows; the padding keeps its sentinel."""
    B, H, W, C, K = 2, 37, 71, 3, 3
    frames = random_frames(B, H, W, C)
    sr, sf = W * C + 5, H * (W * C + 5) + 11
    src = np.full(src_off + B * sf, SENTINEL, np.uint8)
    osr, osf = W + 3, H * (W + 3) + 9
    osw = B * osf + 13
    for b in range(B):
        for r in range(H):
            src[src_off + b * sf + r * sr:][:W * C] = frames[b, r].ravel()
    outs = [np.full(out_off + K * osw, SENTINEL, np.uint8) for _ in range(2)]
    want = adaptive_oracle(frames, (3, 13, 23), (7, 0, -3), True, 200, -1)
    lib = _native.load()
    opts = _native.AdaptiveOpts(n_windows=K, invert=1, max_value=200, channel=-1, frames_on_device=int(on_device), out_on_device=int(on_device))
    opts.block[:K], opts.delta[:K] = (3, 13, 23), (7, 0, -3)
    if on_device:
        keep = [torch.from_numpy(a).cuda() for a in [src] + outs]
        torch.cuda.synchronize()
        ptrs = [t.data_ptr() for t in keep]
    else:
        ptrs = [a.ctypes.data for a in [src] + outs]
    for which in ((1, 1), (1, 0), (0, 1)):                                 # both, the masks only, the means only
        rc = lib.sba_adaptive_threshold(0, ctypes.c_void_p(ptrs[0] + src_off), B, H, W, C, sr, sf, ctypes.byref(opts), osr, osf, osw,
                                        ctypes.c_void_p(ptrs[1] + out_off if which[0] else None),
                                        ctypes.c_void_p(ptrs[2] + out_off if which[1] else None))
        assert rc == 0, lib.sba_last_error(None)
        got = [host(t) for t in keep[1:]] if on_device else outs
        for side in range(2):
            expect = np.full(out_off + K * osw, SENTINEL, np.uint8)
            if which[side]:
                for k in range(K):
                    for b in range(B):
                        for r in range(H):
                            expect[out_off + k * osw + b * osf + r * osr:][:W] = want[side][k, b, r]
            assert np.array_equal(got[side], expect), (which, side)
        if on_device:
            for t in keep[1:]:
                t.fill_(SENTINEL)
            torch.cuda.synchronize()
        else:
            for a in outs:
                a.fill(SENTINEL)


@pytest.mark.parametrize("on_device", (False, True))
def test_out_is_a_strided_view_into_a_canvas(torch, on_device):
    frames = random_frames(2, 37, 71, 0)
    canvas = np.full((3, 2, 50, 90), SENTINEL, np.uint8)
    means = np.full((3, 2, 50, 90), SENTINEL, np.uint8)
    if on_device:
        canvas, means, src = torch.from_numpy(canvas).cuda(), torch.from_numpy(means).cuda(), torch.from_numpy(frames.copy()).cuda()
    else:
        src = frames
    got = _native.adaptive_threshold(src, (3, 13, 23), (7, 7, 7), channel=0, out=canvas[:, :, 5:42, 11:82], mean_out=means[:, :, 5:42, 11:82])
    assert got[0].shape == (3, 2, 37, 71)
    want = adaptive_oracle(frames, (3, 13, 23), (7, 7, 7), True, 255, 0)
    for a, w in zip((canvas, means), want):
        expect = np.full((3, 2, 50, 90), SENTINEL, np.uint8)
        expect[:, :, 5:42, 11:82] = w
        assert np.array_equal(host(a), expect)
    res = imaging.adaptive_threshold(src, 13, out=canvas[0][:, 5:42, 11:82])    # the public face: one window, (B, H, W)
    assert res.shape == (2, 37, 71) and np.array_equal(host(canvas)[0, :, 5:42, 11:82], want[0][1])


def test_chunks_and_no_frames(torch):
    frames = random_frames(7, 41, 67, 3)
    want = adaptive_oracle(frames, (3, 13, 23), (7, 7, 7))
    for chunk in (1, 2, 3, 7, 0):
        masks, means = _native.adaptive_threshold(frames, (3, 13, 23), (7, 7, 7), mean_out=True, chunk_frames=chunk)
        assert np.array_equal(masks, want[0]) and np.array_equal(means, want[1]), chunk
    dev = torch.from_numpy(frames.copy()).cuda()
    masks, _ = _native.adaptive_threshold(dev, (3, 13, 23), (7, 7, 7), chunk_frames=2)
    assert np.array_equal(host(masks), want[0])
    for empty in (frames[:0], dev[:0]):
        masks, means = _native.adaptive_threshold(empty, (3, 13), (7, 7), mean_out=True)
        assert tuple(masks.shape) == tuple(means.shape) == (2, 0, 41, 67)
    assert imaging.adaptive_threshold(frames[:0], 3).shape == (0, 41, 67)
    assert imaging.adaptive_threshold(np.zeros((2, 0, 5), np.uint8), (3, 5)).shape == (2, 2, 0, 5)


def test_two_calls_return_the_same_bytes_and_one_call_equals_single_window_calls(torch):
    frames = torch.from_numpy(random_frames(2, 150, 300, 3).copy()).cuda()
    a = _native.adaptive_threshold(frames, (3, 13, 23), (7, 7, 7), mean_out=True)
    b = _native.adaptive_threshold(frames, (3, 13, 23), (7, 7, 7), mean_out=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k, w in enumerate((3, 13, 23)):
        one = _native.adaptive_threshold(frames, (w,), (7,), mean_out=True)
        assert torch.equal(one[0][0], a[0][k]) and torch.equal(one[1][0], a[1][k])


def test_public_face(torch):
    frames = random_frames(2, H0, W0, 3)
    want = adaptive_oracle(frames, (3, 13, 23), (6, 6, 6), True, 255, -1)
    got = imaging.adaptive_threshold(frames, (3, 13, 23), C=6.5)            # binary_inv: floor
    assert isinstance(got, np.ndarray) and np.array_equal(got, want[0])
    want_b = adaptive_oracle(frames, (13,), (7,), False, 200, 1)
    got, mean = imaging.adaptive_threshold(torch.from_numpy(frames.copy()).cuda(), 13, C=6.5, threshold_type="binary", max_value=200,
                                           channel=1, return_mean=True)   # binary: ceil
    assert got.is_cuda and np.array_equal(host(got), want_b[0][0]) and np.array_equal(host(mean), want_b[1][0])
    rgb = imaging.adaptive_threshold(frames[..., ::-1].copy(), 13, C=6, channel_order="rgb")
    assert np.array_equal(rgb, want[0][1])
    gray = random_frames(1, H0, W0, 0)[0]
    for kind in (imaging.THRESH_BINARY, imaging.THRESH_BINARY_INV):
        got = imaging.adaptive_threshold_cv(gray, 255, imaging.ADAPTIVE_THRESH_MEAN_C, kind, 23, 7)
        assert got.shape == gray.shape and np.array_equal(got, adaptive_oracle(gray[None], (23,), (7,), bool(kind), 255, 0)[0][0, 0])
    assert not imaging.adaptive_threshold_cv(gray, 0, 0, 1, 23, 7).any()


def test_workflow_scene_masks_stay_on_the_device_and_are_labelled_there(torch):
    img, corners = workflow_scene()
    frames = torch.from_numpy(np.stack([img, img])).cuda()
    masks = imaging.adaptive_threshold(frames, (13, 23, 51), C=7)
    assert masks.is_cuda and tuple(masks.shape) == (3, 2, 160, 240)
    for k in range(3):
        blobs = _native.detect_blobs(masks[k], threshold=127, channel=0, dilate_radius=0, close_radius=0, max_blobs=16)
        assert blobs.n_components.tolist() == [6, 6], (k, blobs.n_components)
        rec = blobs.blobs[:, :6].astype(np.int64)
        assert np.all(rec[:, :, 0] == 144), rec[:, :, 0]                    # n of a component, the first value of its record
        boxes = sorted(tuple(int(v) for v in r[8:12]) for r in rec[0])
        assert boxes == sorted((cx, cy, cx + 11, cy + 11) for cy, cx in corners), boxes
