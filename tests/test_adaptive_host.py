"""CPU: the rule of sba_adaptive_threshold (include/sba_hip.h) restated in numpy -- ``adaptive_oracle``, the reference of
tests/test_gpu_adaptive.py -- and pinned to answers known without it: the three forms of the rounding (rule 4) agree for every
sum of every window, constant frames, a single bright pixel, frames smaller than the window, and the workflow scene in which
the local mean separates six dark squares under uneven light where none of the 256 global thresholds does.  Where ``cv2``
imports, ``imaging.adaptive_threshold_cv`` is compared with ``cv2.adaptiveThreshold`` and ``cv2.blur`` on a GPU; without cv2
(or without a GPU) that test skips.
"""
import numpy as np
import pytest

GRAY_BGR = (3735, 19235, 9798)


def plane_of(frames, channel, gray_w=None):
    """Rule 1: (B, H, W[, C]) uint8 -> (B, H, W) int64 values."""
    f = np.asarray(frames)
    if f.ndim == 3:
        assert channel == 0
        return f.astype(np.int64)
    if channel == -1:
        w = GRAY_BGR if gray_w is None or not any(gray_w) else gray_w
        f = f.astype(np.int64)
        return (f[..., 0] * w[0] + f[..., 1] * w[1] + f[..., 2] * w[2] + (1 << 14)) >> 15
    return f[..., channel].astype(np.int64)


def window_sums(v, b):
    """Rules 2 and 3: the sums over b x b windows of the edge-padded planes v (B, H, W) int64."""
    r = b // 2
    p = np.pad(v, ((0, 0), (r, r), (r, r)), mode="edge")
    c = np.cumsum(p, axis=2)
    c = np.concatenate((np.zeros_like(c[:, :, :1]), c), axis=2)
    rows = c[:, :, b:] - c[:, :, :-b]                                     # sums along the rows: (B, H + 2 r, W)
    c = np.cumsum(rows, axis=1)
    c = np.concatenate((np.zeros_like(c[:, :1]), c), axis=1)
    return c[:, b:] - c[:, :-b]


def adaptive_oracle(frames, blocks, deltas, invert=True, max_value=255, channel=-1, gray_w=None):
    """-> (masks, means), each (K, B, H, W) uint8: the header's rule, int64 sums, rule 4 in integers."""
    v = plane_of(frames, channel, gray_w)
    masks, means = [], []
    for b, delta in zip(blocks, deltas):
        S = window_sums(v, int(b))
        mean = (2 * S + b * b) // (2 * b * b)
        d = v - mean
        on = d <= -int(delta) if invert else d > -int(delta)
        masks.append(np.where(on, max_value or 255, 0).astype(np.uint8))
        means.append(mean.astype(np.uint8))
    return np.stack(masks), np.stack(means)


def one(frame, b, delta=0, invert=True, max_value=255):
    m, a = adaptive_oracle(np.asarray(frame, np.uint8)[None], (b,), (delta,), invert, max_value, 0)
    return m[0, 0], a[0, 0]


def workflow_scene():
    """Six dark 12 x 12 squares on a floor lit from the right, with one level of pixel noise -> (image, top-left corners (y, x))."""
    H, W = 160, 240
    y, x = np.mgrid[:H, :W]
    bg = 60 + (x * 150) // 240
    img = bg.copy()
    corners = ((20, 30), (20, 120), (20, 200), (100, 40), (100, 130), (100, 205))
    for cy, cx in corners:
        img[cy:cy + 12, cx:cx + 12] = (bg[cy:cy + 12, cx:cx + 12] * 35) // 100
    return (img + ((x + y) & 1)).astype(np.uint8), corners


@pytest.mark.parametrize("lo", (3, 45, 87))
def test_three_forms_of_the_rounding_agree_for_every_sum(lo):
    """Rule 4 for every odd b in 3..127 and every S in 0..255 b^2: floor((2 S + b^2) / (2 b^2)) equals OpenCV's float32 form
    rint(fl32(S) * fl32(1.0f / b^2)) and its float64 form rint(S * (1.0 / b^2))."""
    for b in range(lo, min(lo + 42, 128), 2):
        n = b * b
        S = np.arange(255 * n + 1, dtype=np.int64)
        exact = (2 * S + n) // (2 * n)
        f32 = np.rint(S.astype(np.float32) * (np.float32(1.0) / np.float32(n)))
        assert f32.dtype == np.float32 and np.array_equal(f32.astype(np.int64), exact), b
        f64 = np.rint(S.astype(np.float64) * (1.0 / n))
        assert np.array_equal(f64.astype(np.int64), exact), b
        assert exact[-1] == 255


def test_the_float32_form_is_not_exact_beyond_the_limit():
    """Why 127 is the limit: at b = 165 the float32 form differs from the integer nearest to S / b^2."""
    n = 165 * 165
    S = np.arange(255 * n + 1, dtype=np.int64)
    f32 = np.rint(S.astype(np.float32) * (np.float32(1.0) / np.float32(n))).astype(np.int64)
    assert not np.array_equal(f32, (2 * S + n) // (2 * n))


@pytest.mark.parametrize("c", (0, 1, 128, 255))
@pytest.mark.parametrize("b", (3, 23, 127))
def test_constant_frame(c, b):
    frame = np.full((9, 14), c, np.uint8)
    for delta in (-256, -3, 0, 7, 256):
        for max_value in (1, 200, 255):
            inv, mean = one(frame, b, delta, True, max_value)
            binary, _ = one(frame, b, delta, False, max_value)
            assert np.all(mean == c)
            assert np.all(inv == (max_value if delta <= 0 else 0)) and np.all(binary == (0 if delta <= 0 else max_value))


def test_single_bright_pixel():
    frame = np.zeros((9, 11), np.uint8)
    frame[4, 5] = 255
    mask, mean = one(frame, 3)
    want = np.zeros((9, 11), np.uint8)
    want[3:6, 4:7] = 28                                                   # round(255 / 9)
    assert np.array_equal(mean, want)
    assert mask[4, 5] == 0 and mask.sum() == 255 * (9 * 11 - 1)            # 255 - 28 > 0; everywhere else v <= mean
    frame = np.zeros((9, 11), np.uint8)
    frame[0, 0] = 255                                                     # the corner is replicated: 4 of the 9 taps
    _, mean = one(frame, 3)
    assert mean[0, 0] == 113 and mean[0, 1] == 57 and mean[1, 0] == 57 and mean[1, 1] == 28 and mean[0, 2] == 0    # round(1020 / 9), round(510 / 9)


def test_frames_smaller_than_the_window():
    mask, mean = one([[0]], 23)
    assert mean.tolist() == [[0]] and mask.tolist() == [[255]]
    for b in (3, 23, 127):
        mask, mean = one([[77]], b, 0)
        assert mean.tolist() == [[77]] and mask.tolist() == [[255]]
    row = np.array([[0, 40, 80, 120, 160]], np.uint8)
    mask, mean = one(row, 23)
    # all 23 rows of a window are the one row, so mean = (taps of the row) / 23: at x = 0 twelve copies of 0, then 40, 80, 120 and
    # eight copies of 160: 1520 / 23 = 66.09; at x = 2 ten of each end: 1840 / 23 = 80; a step to the right adds 160: 6.96
    assert mean.tolist() == [[66, 73, 80, 87, 94]] and mask.tolist() == [[255, 255, 255, 0, 0]]
    mask_t, mean_t = one(row.T, 23)
    assert np.array_equal(mask_t, mask.T) and np.array_equal(mean_t, mean.T)


def test_gray_and_channels():
    rng = np.random.default_rng(5)
    f = rng.integers(0, 256, size=(2, 7, 9, 4), dtype=np.uint8)
    g = plane_of(f, -1)
    assert g[1, 2, 3] == (int(f[1, 2, 3, 0]) * 3735 + int(f[1, 2, 3, 1]) * 19235 + int(f[1, 2, 3, 2]) * 9798 + 16384) >> 15
    assert np.array_equal(plane_of(f, 3), f[..., 3]) and g.max() <= 255
    m, a = adaptive_oracle(f, (3, 5), (7, -2), True, 200, -1)
    m1, a1 = adaptive_oracle(g.astype(np.uint8), (5,), (-2,), True, 200, 0)
    assert m.shape == (2, 2, 7, 9) and np.array_equal(m[1], m1[0]) and np.array_equal(a[1], a1[0]) and set(np.unique(m)) <= {0, 200}


def test_workflow_scene_local_mean_separates_what_no_global_threshold_does():
    ndimage = pytest.importorskip("scipy.ndimage")
    img, corners = workflow_scene()
    eight = np.ones((3, 3), int)
    masks, _ = adaptive_oracle(img[None], (13, 23, 51, 3), (7, 7, 7, 7), True, 255, 0)
    for k in range(3):
        lab, n = ndimage.label(masks[k, 0], structure=eight)
        assert n == 6 and np.bincount(lab.ravel())[1:].tolist() == [144] * 6, (k, n)
        for (cy, cx), sl in zip(sorted(corners), ndimage.find_objects(lab)):
            assert (sl[0].start, sl[0].stop, sl[1].start, sl[1].stop) == (cy, cy + 12, cx, cx + 12)
    lab, n = ndimage.label(masks[3, 0], structure=eight)                  # window 3 sees only the edges: rings
    assert n == 6 and np.bincount(lab.ravel())[1:].tolist() == [44] * 6
    for t in range(256):
        lab, n = ndimage.label((255 - img.astype(np.int64)) > t, structure=eight)
        assert not (n == 6 and np.bincount(lab.ravel())[1:].tolist() == [144] * 6), t


def test_marker_windows_and_argument_checks_of_the_python_face():
    from lasercalib_amd import imaging
    assert imaging.marker_threshold_windows() == (3, 13, 23)
    assert imaging.marker_threshold_windows(4, 30, 9) == (5, 13, 23)
    assert imaging.marker_threshold_windows(3, 3, 10) == (3,)
    with pytest.raises(ValueError):
        imaging.marker_threshold_windows(2, 23, 10)
    assert (imaging.ADAPTIVE_THRESH_MEAN_C, imaging.THRESH_BINARY, imaging.THRESH_BINARY_INV) == (0, 0, 1)
    f = np.zeros((1, 4, 6), np.uint8)
    with pytest.raises(ValueError, match="odd integer in 3..127"):
        imaging.adaptive_threshold(f, 4)
    with pytest.raises(ValueError, match="odd integer in 3..127"):
        imaging.adaptive_threshold(f, (3, 129))
    with pytest.raises(ValueError, match="up to 4"):
        imaging.adaptive_threshold(f, (3, 5, 7, 9, 11))
    with pytest.raises(ValueError, match="one per window"):
        imaging.adaptive_threshold(f, (3, 5), C=(1, 2, 3))
    with pytest.raises(ValueError, match="threshold_type"):
        imaging.adaptive_threshold(f, 3, threshold_type="trunc")
    with pytest.raises(ValueError, match="channel must be"):
        imaging.adaptive_threshold(f, 3, channel=-1)
    with pytest.raises(ValueError, match="ADAPTIVE_THRESH_MEAN_C"):
        imaging.adaptive_threshold_cv(f[0], 255, 1, 1, 3, 7)
    with pytest.raises(ValueError, match="thresholdType"):
        imaging.adaptive_threshold_cv(f[0], 255, 0, 2, 3, 7)
    with pytest.raises(ValueError, match="one grey image"):
        imaging.adaptive_threshold_cv(f, 255, 0, 1, 3, 7)


def test_adaptive_threshold_cv_against_opencv():
    cv2 = pytest.importorskip("cv2")
    from lasercalib_amd import _native, imaging
    if _native.device_count() == 0:
        pytest.skip("needs a GPU")
    img = np.random.default_rng(9).integers(0, 256, size=(97, 131), dtype=np.uint8)
    for b in (3, 13, 23, 51, 127):
        for kind, C in ((cv2.THRESH_BINARY_INV, 7), (cv2.THRESH_BINARY, 7), (cv2.THRESH_BINARY_INV, 6.5), (cv2.THRESH_BINARY, -2.5)):
            want = cv2.adaptiveThreshold(img, 255, cv2.ADAPTIVE_THRESH_MEAN_C, kind, b, C)
            assert np.array_equal(imaging.adaptive_threshold_cv(img, 255, 0, kind, b, C), want), (b, kind, C)
        _, mean = imaging.adaptive_threshold(img[None], b, return_mean=True)
        assert np.array_equal(mean[0], cv2.blur(img, (b, b), borderType=cv2.BORDER_REPLICATE)), b
