"""CPU tests of the laser-dot detector (sba_detect_dots, include/sba_hip.h; lasercalib_amd/feature_detection.py): the binding,
the numpy oracle the GPU tests compare against bit for bit, the parity argument with the reference's OpenCV calls, the accuracy
of the three centroids, and the path of ``centroid_table`` into the dataset builder.

``dots_oracle`` restates the header's definitions in integer arithmetic (numpy int64 marginal sums, then Python ints), with
the ROI as a plain per-pixel mask.  ``opencv_restatement`` restates ``green_laser_finder_faster`` of the reference
(lasercalib/feature_detection.py:44-54) with the two OpenCV definitions it uses written out, factors of 255 included:
``cv.threshold(src, t, 255, THRESH_BINARY)`` is ``255 where src > t else 0`` and ``cv.moments`` of an 8-bit image is
``m_pq = sum I(y, x) x^p y^q`` in float64.  cv2 and skimage are not installed here, so no fixture could be recorded from the
reference itself; the identity ``int(m10 / m00) == sum m x // n`` is checked on random frames instead.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from lasercalib_amd import _native, dataset, feature_detection as fd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NONE, TOO_SMALL, TOO_LARGE, SPREAD = 0, 1, 2, 3, 4


# ----------------------------------------------------------------------------- the oracle
def roi_mask(H, W, roi_rect=None, roi_circle=None):
    """(H, W) bool: inside the rectangle (half-open, clipped; all zero = whole frame) and inside the circle (r <= 0 = off)."""
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    keep = np.ones((H, W), bool)
    if roi_rect is not None and any(int(v) != 0 for v in roi_rect):
        x0, y0, x1, y1 = (int(v) for v in roi_rect)
        keep &= (x >= x0) & (x < x1) & (y >= y0) & (y < y1)
    if roi_circle is not None and int(roi_circle[2]) > 0:
        cx, cy, r = (int(v) for v in roi_circle)
        keep &= (x - cx) ** 2 + (y - cy) ** 2 <= r * r
    return keep


def dots_oracle(frames, threshold=50, channel=1, min_area=0, max_area=0, max_extent=0, roi_rect=None, roi_circle=None):
    """LaserDots of (B, H, W, C) or (B, H, W) uint8 frames by the definitions of include/sba_hip.h, in exact integers."""
    frames = np.asarray(frames)
    if frames.ndim == 3:
        frames = frames[..., None]
    B, H, W, _ = frames.shape
    keep = roi_mask(H, W, roi_rect, roi_circle)
    xs, ys = np.arange(W, dtype=np.int64), np.arange(H, dtype=np.int64)
    sums, box = np.zeros((B, 12), np.uint64), np.zeros((B, 4), np.int32)
    centroid, status = np.full((B, 4), np.nan), np.zeros(B, np.int32)
    for f in range(B):
        g = frames[f, :, :, channel].astype(np.int64)
        m = (g > threshold) & keep
        mi = m.astype(np.int64)
        w = (g - threshold) * mi
        col, row, wcol, wrow = mi.sum(axis=0), mi.sum(axis=1), w.sum(axis=0), w.sum(axis=1)
        n = int(col.sum())
        s = [n, int(col @ xs), int(row @ ys), int(col @ (xs * xs)), int(row @ (ys * ys)), int((mi @ xs) @ ys),
             int(wcol.sum()), int(wcol @ xs), int(wrow @ ys), int(((g == 255) & m).sum()), 0, 0]
        sums[f] = s
        if n == 0:
            box[f], status[f] = (W, H, -1, -1), NONE
            continue
        cx, cy = np.nonzero(col)[0], np.nonzero(row)[0]
        box[f] = (cx[0], cy[0], cx[-1], cy[-1])
        centroid[f] = (float(s[1]) / float(n), float(s[2]) / float(n), float(s[7]) / float(s[6]), float(s[8]) / float(s[6]))
        ext = max(int(box[f, 2] - box[f, 0]), int(box[f, 3] - box[f, 1])) + 1
        status[f] = (TOO_SMALL if n < min_area else TOO_LARGE if max_area > 0 and n > max_area
                     else SPREAD if max_extent > 0 and ext > max_extent else OK)
    return _native.LaserDots(sums, box, centroid, status)


def all_bright_sums(H, W, threshold, value=255):
    """Closed forms of the twelve sums of an H x W frame whose every pixel has `value` > threshold."""
    n, sx, sy = H * W, H * W * (W - 1) // 2, W * H * (H - 1) // 2
    sxx, syy = H * (W - 1) * W * (2 * W - 1) // 6, W * (H - 1) * H * (2 * H - 1) // 6
    sxy = (W * (W - 1) // 2) * (H * (H - 1) // 2)
    w = value - threshold
    return [n, sx, sy, sxx, syy, sxy, w * n, w * sx, w * sy, n if value == 255 else 0, 0, 0]


def opencv_restatement(frame, laser_intensity_thresh):
    """green_laser_finder_faster of the reference (feature_detection.py:44-54), cv.threshold and cv.moments written out."""
    green = frame[:, :, 1]
    thresh = np.where(green > laser_intensity_thresh, 255, 0).astype(np.uint8)        # cv.threshold(green, t, 255, 0)
    img = thresh.astype(np.float64)                                                   # cv.moments: m_pq = sum I x^p y^q, float64
    yy, xx = np.mgrid[0:img.shape[0], 0:img.shape[1]].astype(np.float64)
    M = {"m00": float(img.sum()), "m10": float((img * xx).sum()), "m01": float((img * yy).sum())}
    if M["m00"] != 0:
        cy = int(M["m10"] / M["m00"])
        cx = int(M["m01"] / M["m00"])
        return (cx, cy)
    return None


def same_dots(a, b):
    """Bit equality of two LaserDots, NaNs matched by position."""
    return (np.array_equal(a.sums, b.sums) and np.array_equal(a.box, b.box) and np.array_equal(a.status, b.status)
            and np.array_equal(a.centroid, b.centroid, equal_nan=True)
            and np.array_equal(np.signbit(a.centroid), np.signbit(b.centroid)))


def render_spots(n_spots, size, rng, sigma=(1.0, 3.0), amp=(150.0, 255.0), noise=30, margin=8.0):
    """(n_spots, size, size) uint8 frames, one Gaussian spot each on dark noise of 0..noise counts, and the (n_spots, 2) true
    centres (x, y) in pixel coordinates (a pixel's centre is at its integer index)."""
    c = rng.uniform(margin, size - 1 - margin, size=(n_spots, 2))
    sg, a = rng.uniform(*sigma, size=n_spots), rng.uniform(*amp, size=n_spots)
    y, x = np.mgrid[0:size, 0:size].astype(np.float64)
    r2 = (x[None] - c[:, 0, None, None]) ** 2 + (y[None] - c[:, 1, None, None]) ** 2
    img = a[:, None, None] * np.exp(-0.5 * r2 / sg[:, None, None] ** 2) + rng.integers(0, noise + 1, size=r2.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8), c


# measured here with render_spots(2000, 33, default_rng(0)) (sigma 1-3 px, peak 150-255, 8 bit, threshold 50, dark noise 0..30):
# 2-D RMS distance to the true centre, pixels.  The caps are 1.5 x these.
RMS_MEASURED = {"truncated": 0.8136, "binary": 0.1698, "weighted": 0.0576}         # largest weighted error: 0.186 px
RMS_CAP = {k: 1.5 * v for k, v in RMS_MEASURED.items()}


def centroid_errors(dots, centres):
    """2-D distances of the truncated, binary and weighted centroids to the true centres: three (B,) arrays."""
    n = dots.sums[:, 0].astype(np.int64)
    trunc = np.stack([dots.sums[:, 1].astype(np.int64) // n, dots.sums[:, 2].astype(np.int64) // n], axis=1).astype(np.float64)
    return [np.linalg.norm(c - centres, axis=1) for c in (trunc, dots.centroid[:, :2], dots.centroid[:, 2:])]


# ----------------------------------------------------------------------------- 1. the binding
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _native.load()


def test_symbol_is_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "sba_hip.h")).read()
    assert re.search(r"\bint\s+sba_detect_dots\s*\(", text) and "SBA_ABI_VERSION 2" in text
    assert "sba_detect_dots" in _native.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "sba_detect_dots")
    assert lib.sba_detect_dots.argtypes is not None and len(lib.sba_detect_dots.argtypes) == 13
    assert ctypes.sizeof(_native.DotOpts) == 64
    assert (fd.SBA_DOT_OK, fd.SBA_DOT_NONE, fd.SBA_DOT_TOO_SMALL, fd.SBA_DOT_TOO_LARGE, fd.SBA_DOT_SPREAD) == (0, 1, 2, 3, 4)
    import lasercalib.feature_detection as shim
    assert shim.green_laser_finder_faster is fd.green_laser_finder_faster and shim.centroid_table is fd.centroid_table


def test_without_a_gpu_the_call_fails_loudly_and_arguments_are_checked_first(lib):
    frames = np.zeros((2, 5, 7, 3), np.uint8)
    frames[1, 2, 3, 1] = 200
    with pytest.raises(_native.SbaError, match="channel out of range"):      # checked before any device work, GPU or not
        fd.find_laser_dots(frames, channel=3)
    with pytest.raises(_native.SbaError, match="status -6"):
        fd.find_laser_dots(np.zeros((1, 2, 16385), np.uint8), channel=0)
    with pytest.raises(ValueError, match="contiguous"):
        fd.find_laser_dots(frames[:, :, ::2])
    with pytest.raises(ValueError, match="uint8"):
        fd.find_laser_dots(frames.astype(np.int16))
    if lib.sba_device_count() > 0:
        assert same_dots(fd.find_laser_dots(frames), dots_oracle(frames))
        assert fd.green_laser_finder_faster(frames[1], 50) == (2, 3)
        return
    with pytest.raises(_native.SbaError, match="no HIP device"):
        fd.find_laser_dots(frames)
    with pytest.raises(_native.SbaError, match="no HIP device"):
        fd.green_laser_finder_faster(frames[1], 50)


# ----------------------------------------------------------------------------- 2. the oracle
@pytest.mark.parametrize("H,W,thr", [(7, 5, 0), (13, 31, 50), (1, 1, 254), (40, 3, 100)])
def test_oracle_all_bright_frame_matches_closed_forms(H, W, thr):
    for value in (255, thr + 1):
        d = dots_oracle(np.full((1, H, W, 3), value, np.uint8), threshold=thr)
        assert [int(v) for v in d.sums[0]] == all_bright_sums(H, W, thr, value)
        assert list(d.box[0]) == [0, 0, W - 1, H - 1] and d.status[0] == OK
        assert np.allclose(d.centroid[0], [(W - 1) / 2, (H - 1) / 2] * 2, rtol=0, atol=1e-12)
    # a brute-force sum over the pixels, in Python ints
    rng = np.random.default_rng(3)
    f = rng.integers(0, 256, size=(1, H, W, 3), dtype=np.uint8)
    d = dots_oracle(f, threshold=thr, channel=2)
    px = [(x, y, int(f[0, y, x, 2])) for y in range(H) for x in range(W) if f[0, y, x, 2] > thr]
    brute = [len(px), sum(x for x, _, _ in px), sum(y for _, y, _ in px), sum(x * x for x, _, _ in px), sum(y * y for _, y, _ in px),
             sum(x * y for x, y, _ in px), sum(v - thr for _, _, v in px), sum((v - thr) * x for x, _, v in px),
             sum((v - thr) * y for _, y, v in px), sum(v == 255 for _, _, v in px), 0, 0]
    assert [int(v) for v in d.sums[0]] == brute


def test_truncation_identity_with_the_opencv_restatement():
    """int(m10 / m00) == sum m x // n: m00 = 255 n and m10 = 255 sum m x are exact in float64, a quotient that is not an integer
    lies at least 1 / n from one, and one that is divides exactly."""
    rng = np.random.default_rng(11)
    checked = 0
    for trial in range(60):
        H, W = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        thr = int(rng.choice([0, 50, 128, 200, 254, 255]))
        frame = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        if trial % 3 == 0:                                   # sparse frames: few pixels, quotients near integers
            frame[rng.random((H, W)) < 0.9] = 0
        d = dots_oracle(frame[None], threshold=thr)
        n, sx, sy = (int(v) for v in d.sums[0, :3])
        want = None if n == 0 else (sy // n, sx // n)
        assert opencv_restatement(frame, thr) == want
        table = fd.centroid_table(d, subpixel=False)
        assert (np.isnan(table[0]).all() if want is None else tuple(table[0]) == want)
        checked += want is not None
    assert checked >= 40


def _blob(frame, x, y, r=1, value=220, channel=1):
    frame[y - r:y + r + 1, x - r:x + r + 1, channel] = value


def test_oracle_reaches_each_status():
    f = np.zeros((6, 30, 40, 3), np.uint8)
    f[:, :, :, 0] = 255                                      # a bright OTHER channel changes nothing
    _blob(f[1], 10, 12)                                      # 9 pixels
    _blob(f[2], 10, 12)
    _blob(f[3], 10, 12)
    _blob(f[4], 10, 12); _blob(f[4], 30, 20)                 # two distant blobs
    _blob(f[5], 10, 12)
    f[5, 12, 10, 1] = 50                                     # value == threshold does not count
    d = dots_oracle(f, min_area=9, max_area=9, max_extent=5)
    assert list(d.status) == [NONE, OK, OK, OK, TOO_LARGE, TOO_SMALL]
    assert list(dots_oracle(f, max_extent=5).status) == [NONE, OK, OK, OK, SPREAD, OK]
    assert list(dots_oracle(f, max_extent=3).status)[1] == OK and list(dots_oracle(f, max_extent=2).status)[1] == SPREAD
    assert list(dots_oracle(f, min_area=10).status) == [NONE, TOO_SMALL, TOO_SMALL, TOO_SMALL, OK, TOO_SMALL]
    assert list(dots_oracle(f, min_area=10, max_area=17, max_extent=5).status)[4] == TOO_LARGE       # the first that applies
    assert list(d.box[0]) == [40, 30, -1, -1] and np.isnan(d.centroid[0]).all()
    assert list(d.box[1]) == [9, 11, 11, 13] and tuple(d.centroid[1]) == (10.0, 12.0, 10.0, 12.0)
    assert list(d.box[4]) == [9, 11, 31, 21] and d.sums[4, 0] == 18 and d.sums[5, 0] == 8
    assert np.allclose(d.spread_px[1], np.sqrt(2 * 2 / 3)) and np.isnan(d.spread_px[0])
    assert np.array_equal(d.n, d.sums[:, 0]) and list(d.ok) == [False, True, True, True, False, False]


def test_oracle_both_roi_kinds():
    f = np.full((1, 20, 30, 3), 255, np.uint8)
    d = dots_oracle(f, roi_rect=(4, 2, 10, 7))
    assert d.sums[0, 0] == 6 * 5 and list(d.box[0]) == [4, 2, 9, 6]
    d = dots_oracle(f, roi_rect=(-5, 15, 8, 99))             # partly outside: clipped
    assert d.sums[0, 0] == 8 * 5 and list(d.box[0]) == [0, 15, 7, 19]
    d = dots_oracle(f, roi_circle=(10, 9, 3))
    assert d.sums[0, 0] == 29 and list(d.box[0]) == [7, 6, 13, 12] and tuple(d.centroid[0, :2]) == (10.0, 9.0)
    d = dots_oracle(f, roi_circle=(0, 0, 2))                 # a quarter of the 13-pixel disc
    assert d.sums[0, 0] == 6 and list(d.box[0]) == [0, 0, 2, 2]
    d = dots_oracle(f, roi_rect=(9, 0, 30, 20), roi_circle=(10, 9, 3))
    assert d.sums[0, 0] == 29 - 6 and list(d.box[0]) == [9, 6, 13, 12]            # loses x = 7 (1 pixel) and x = 8 (5)
    d = dots_oracle(f, roi_rect=(25, 0, 30, 20), roi_circle=(10, 9, 3))
    assert d.sums[0, 0] == 0 and d.status[0] == NONE
    assert dots_oracle(f, roi_rect=(7, 3, 7, 9)).status[0] == NONE               # an empty rectangle keeps nothing
    assert dots_oracle(f, roi_rect=(0, 0, 0, 0), roi_circle=(0, 0, 0)).sums[0, 0] == 600     # both off


# ----------------------------------------------------------------------------- 3. accuracy of the three centroids
def test_weighted_beats_binary_beats_truncated_on_rendered_spots():
    rng = np.random.default_rng(0)
    frames, centres = render_spots(2000, 33, rng)
    d = dots_oracle(frames, threshold=50, channel=0)
    assert np.all(d.status == OK) and d.sums[:, 0].min() >= 1
    rms = {k: float(np.sqrt(np.mean(e ** 2))) for k, e in zip(("truncated", "binary", "weighted"), centroid_errors(d, centres))}
    worst = float(centroid_errors(d, centres)[2].max())
    print(f"2-D RMS error, px: {rms}; weighted max {worst:.4f}")
    assert rms["weighted"] < rms["binary"] < rms["truncated"]
    for k in rms:
        assert rms[k] <= RMS_CAP[k], (k, rms[k], RMS_CAP[k])
    assert rms["truncated"] > 2 * 0.3            # the reference's detector alone: more than twice the 0.3 px the synthetic rigs assume


# ----------------------------------------------------------------------------- 4. centroid_table and the dataset builder
def test_centroid_table_order_nan_rows_and_path_into_the_dataset():
    rng = np.random.default_rng(5)
    n_frames, n_cams = 12, 3
    tables, dots_all = [], []
    for c in range(n_cams):
        frames, _ = render_spots(n_frames, 33, rng)
        frames[rng.random(n_frames) < 0.25] = 0                          # this camera did not see the dot in these frames
        frames[3, 2:5, 2:5] = 255                                        # frame 3: a second blob -> SPREAD, whatever else it holds
        frames[3, 28:31, 28:31] = 255
        d = dots_oracle(frames, threshold=50, channel=0, max_extent=20)
        dots_all.append(d)
        tables.append(fd.centroid_table(d))
    d = dots_all[0]
    t = tables[0]
    assert t.shape == (n_frames, 2) and t.dtype == np.float64
    assert d.status[3] == SPREAD and (d.status == NONE).any()
    assert np.array_equal(np.isnan(t[:, 0]), d.status != OK) and np.array_equal(np.isnan(t[:, 0]), np.isnan(t[:, 1]))
    ok = d.status == OK
    assert np.array_equal(t[ok], d.centroid[ok][:, [3, 2]])              # (row, col) = (weighted y, weighted x)
    assert np.array_equal(fd.centroid_table(d, weighted=False)[ok], d.centroid[ok][:, [1, 0]])
    ti = fd.centroid_table(d, subpixel=False)
    n = d.sums[ok, 0].astype(np.int64)
    assert np.array_equal(ti[ok], np.stack([d.sums[ok, 2].astype(np.int64) // n, d.sums[ok, 1].astype(np.int64) // n], axis=1))
    assert np.array_equal(ti[ok], np.floor(d.centroid[ok][:, [1, 0]])) and np.isnan(ti[~ok]).all()
    both = fd.centroid_table(d, accept=(OK, SPREAD))
    assert not np.isnan(both[3]).any() and np.array_equal(np.isnan(both[:, 0]), d.status == NONE)
    # scripts/get_points3d.py:39-58: stack per camera, flip to (x, y), filter, build the observation list
    centroids = np.stack(tables, axis=2)
    centroids = np.flip(centroids, axis=1)
    keep = dataset.filter_points(centroids, 2, 0)
    seen = np.stack([dd.status == OK for dd in dots_all], axis=1)
    assert np.array_equal(keep, (seen.sum(axis=1) >= 2) & seen[:, 0]) and keep.any() and not keep.all()
    cam_ind, pt_ind, pts2d = dataset.observation_list(centroids[keep])
    frames_kept = np.nonzero(keep)[0]
    assert cam_ind.size == seen[keep].sum()
    for c, p, uv in zip(cam_ind, pt_ind, pts2d):
        assert tuple(uv) == tuple(dots_all[c].centroid[frames_kept[p], 2:])          # (x, y), the device's bits unchanged
