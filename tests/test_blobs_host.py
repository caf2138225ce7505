"""CPU tests of the connected-component laser-dot detector (sba_detect_blobs, include/sba_hip.h;
lasercalib_amd/feature_detection.py): the binding, the scipy oracle the GPU tests compare against bit for bit, and the host-side
helpers.

``blobs_oracle`` restates the header: the raw mask, ``scipy.ndimage.binary_dilation(border_value=0)`` with disk(r1) and disk(r2),
``binary_erosion(border_value=1)`` with disk(r2) (skimage >= 0.23's ``binary_closing``, mode='ignore'), ``ndimage.label`` with the
3 x 3 structure (``measure.label``'s 8-connectivity and raster numbering), then the 12 integers of every component in int64 /
Python ints and the acceptance rules in Python big integers.  skimage and cv2 are not installed, so neither is imported.
"""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from lasercalib_amd import _native, feature_detection as fd
from test_detect_host import roi_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NONE, OVERFLOW, REJECTED, MULTIPLE = 0, 1, 2, 3, 4
EIGHT = np.ones((3, 3), bool)


# ----------------------------------------------------------------------------- the oracle
def disk(r):
    """skimage.morphology.disk written out: L = arange(-r, r + 1); X, Y = meshgrid(L, L); (X ** 2 + Y ** 2 <= r ** 2)."""
    L = np.arange(-r, r + 1)
    X, Y = np.meshgrid(L, L)
    return np.array((X ** 2 + Y ** 2) <= r ** 2, dtype=np.uint8)


def morph(raw, dilate_radius=1, close_radius=4):
    """binary_dilation(disk(r1)), then binary_closing(disk(r2)) = dilation with a 0 border, erosion with a 1 border."""
    m = np.asarray(raw, bool)
    if dilate_radius > 0:
        m = ndimage.binary_dilation(m, structure=disk(dilate_radius), border_value=0)
    if close_radius > 0:
        m = ndimage.binary_dilation(m, structure=disk(close_radius), border_value=0)
        m = ndimage.binary_erosion(m, structure=disk(close_radius), border_value=1)
    return m


def records(lab, ncomp, raw, value, threshold):
    """(ncomp, 12) Python-int records of the components of ``lab``: exact int64 scatter-adds over the set pixels only."""
    ys, xs = np.nonzero(lab)
    k = lab[ys, xs].astype(np.int64) - 1
    rec = np.zeros((ncomp, 12), np.int64)
    israw = raw[ys, xs]
    v = value[ys, xs].astype(np.int64)
    w = np.where(israw, v - threshold, 0)
    for col, q in ((0, np.ones_like(k)), (1, xs), (2, ys), (3, israw.astype(np.int64)), (4, w), (5, w * xs), (6, w * ys),
                   (7, (israw & (v == 255)).astype(np.int64))):
        np.add.at(rec[:, col], k, q)
    rec[:, 8], rec[:, 9] = np.iinfo(np.int64).max, np.iinfo(np.int64).max
    np.minimum.at(rec[:, 8], k, xs); np.minimum.at(rec[:, 9], k, ys)
    np.maximum.at(rec[:, 10], k, xs); np.maximum.at(rec[:, 11], k, ys)
    return [[int(c) for c in row] for row in rec]


def judge(ncomp, recs, K, min_area=0, max_area=0, centre=None, max_centre_dist=0):
    """(status, accepted index or -1) of one frame from its listed records, in Python big integers."""
    if ncomp == 0:
        return NONE, -1
    if ncomp > K:
        return OVERFLOW, -1
    cx, cy = (0, 0) if centre is None else (int(centre[0]), int(centre[1]))
    acc = []
    for i, r in enumerate(recs[:K]):
        n = r[0]
        good = n >= min_area and (max_area == 0 or n <= max_area)
        if good and max_centre_dist > 0:
            good = (r[1] - cx * n) ** 2 + (r[2] - cy * n) ** 2 <= (max_centre_dist * n) ** 2
        if good:
            acc.append(i)
    return (REJECTED, -1) if not acc else (MULTIPLE, -1) if len(acc) > 1 else (OK, acc[0])


def blobs_oracle(frames, threshold=70, channel=1, dilate_radius=1, close_radius=4, max_blobs=8, min_area=0, max_area=0,
                 centre=None, max_centre_dist=0, roi_rect=None, roi_circle=None):
    """LaserBlobs (mask and labels included) of (B, H, W, C) or (B, H, W) uint8 frames by the definitions of include/sba_hip.h."""
    frames = np.asarray(frames)
    if frames.ndim == 3:
        frames = frames[..., None]
    B, H, W, _ = frames.shape
    K = max_blobs if max_blobs > 0 else 8
    keep = roi_mask(H, W, roi_rect, roi_circle)
    ncomp, blobs = np.zeros(B, np.int32), np.zeros((B, K, 12), np.uint64)
    accepted, centroid, status = np.full(B, -1, np.int32), np.full((B, 4), np.nan), np.zeros(B, np.int32)
    mask, labels = np.zeros((B, H, W), np.uint8), np.zeros((B, H, W), np.int32)
    for f in range(B):
        g = frames[f, :, :, channel]
        raw = (g > threshold) & keep
        m = morph(raw, dilate_radius, close_radius)
        lab, n = ndimage.label(m, structure=EIGHT)
        mask[f], labels[f], ncomp[f] = m, lab, n
        recs = records(lab, n, raw, g, threshold)
        for k, r in enumerate(recs[:K]):
            blobs[f, k] = r
        status[f], accepted[f] = judge(n, recs, K, min_area, max_area, centre, max_centre_dist)
        if status[f] == OK:
            r = recs[accepted[f]]
            centroid[f, 0], centroid[f, 1] = float(r[1]) / float(r[0]), float(r[2]) / float(r[0])
            if r[4]:
                centroid[f, 2], centroid[f, 3] = float(r[5]) / float(r[4]), float(r[6]) / float(r[4])
    return _native.LaserBlobs(ncomp, blobs, accepted, centroid, status, mask, labels)


def blob_diff(a, b):
    """The first stage at which two LaserBlobs differ -- 'mask', 'labels', 'n_components', 'blobs', 'accepted', 'status',
    'centroid' -- or None when they are bit-equal (NaNs matched by position); mask and labels are compared when both have them."""
    if a.mask is not None and b.mask is not None and not np.array_equal(a.mask, b.mask):
        return "mask"
    if a.labels is not None and b.labels is not None and not np.array_equal(a.labels, b.labels):
        return "labels"
    for name in ("n_components", "blobs", "accepted", "status"):
        x, y = getattr(a, name), getattr(b, name)
        if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(x, y):
            return name
    if not (np.array_equal(a.centroid, b.centroid, equal_nan=True) and np.array_equal(np.signbit(a.centroid), np.signbit(b.centroid))):
        return "centroid"
    return None


def mask_frames(masks, value=200, C=3, channel=1):
    """(B, H, W, C) uint8 frames whose thresholded channel holds ``value`` where the (B, H, W) masks are set; the other channels
    are bright everywhere, so reading the wrong one shows."""
    masks = np.asarray(masks, bool)
    f = np.full(masks.shape + (C,), 255, np.uint8)
    f[..., channel] = np.where(masks, value, 0)
    return f


def two_dots(gap, diagonal=False, size=40):
    """Two 3 x 3 dots with `gap` unset columns between them on one row, or `gap` unset columns AND rows on the diagonal."""
    m = np.zeros((size, size), bool)
    m[10:13, 5:8] = True
    y = 10 + (3 + gap if diagonal else 0)
    m[y:y + 3, 8 + gap:11 + gap] = True
    return m


# ----------------------------------------------------------------------------- 1. the binding
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _native.load()


def test_symbol_is_declared_exported_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "sba_hip.h")).read()
    assert re.search(r"\bint\s+sba_detect_blobs\s*\(", text) and "SBA_ABI_VERSION 2" in text
    assert "sba_detect_blobs" in _native.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "sba_detect_blobs")
    assert lib.sba_detect_blobs.argtypes is not None and len(lib.sba_detect_blobs.argtypes) == 16
    assert (fd.SBA_BLOB_OK, fd.SBA_BLOB_NONE, fd.SBA_BLOB_OVERFLOW, fd.SBA_BLOB_REJECTED, fd.SBA_BLOB_MULTIPLE) == (0, 1, 2, 3, 4)
    enum = re.search(r"typedef enum \{([^}]*)\} sba_blob_status;", text).group(1)
    assert [s.strip() for s in enum.split(",")] == ["SBA_BLOB_OK = 0", "SBA_BLOB_NONE = 1", "SBA_BLOB_OVERFLOW = 2",
                                                    "SBA_BLOB_REJECTED = 3", "SBA_BLOB_MULTIPLE = 4"]
    import lasercalib.feature_detection as shim
    assert shim.green_laser_finder is fd.green_laser_finder and shim.find_laser_blobs is fd.find_laser_blobs
    assert shim.blob_centroid_table is fd.blob_centroid_table
    for name in ("green_laser_finder", "find_laser_blobs", "blob_centroid_table", "LaserBlobs", "SBA_BLOB_MULTIPLE"):
        assert name in fd.__all__


def test_struct_sizes_match_the_header():
    text = open(os.path.join(ROOT, "include", "sba_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} sba_blob_opts;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    n_ints = 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        assert decl.startswith("int32_t "), decl
        for name in decl[len("int32_t "):].split(","):
            dim = re.search(r"\[(\d+)\]", name)
            n_ints += int(dim.group(1)) if dim else 1
    assert n_ints == 24 and ctypes.sizeof(_native.BlobOpts) == 4 * n_ints == 96
    assert [n for n, _ in _native.BlobOpts._fields_] == re.findall(r"\b([a-z_0-9]+)(?:\[\d+\])?\s*[,;]", body)
    assert ctypes.sizeof(_native.DotOpts) == 64                           # the older detector's options keep their layout


def test_without_a_gpu_the_call_fails_loudly_and_arguments_are_checked_first(lib):
    frames = np.zeros((2, 5, 7, 3), np.uint8)
    frames[1, 2, 3, 1] = 200
    for kw, text in ((dict(channel=3), "channel out of range"), (dict(threshold=256), "threshold"), (dict(dilate_radius=9), "radius"),
                     (dict(close_radius=-1), "radius"), (dict(max_blobs=65), "max_blobs"), (dict(max_blobs=-1), "max_blobs"),
                     (dict(min_area=-1), "negative"), (dict(max_area=-1), "negative"), (dict(max_centre_dist=-1), "negative")):
        with pytest.raises(_native.SbaError, match=text):                    # checked before any device work, GPU or not
            fd.find_laser_blobs(frames, **kw)
    with pytest.raises(_native.SbaError, match="status -6"):
        fd.find_laser_blobs(np.zeros((1, 2, 16385), np.uint8), channel=0)
    with pytest.raises(ValueError, match="contiguous"):
        fd.find_laser_blobs(frames[:, :, ::2])
    with pytest.raises(ValueError, match="uint8"):
        fd.find_laser_blobs(frames.astype(np.int16))
    if lib.sba_device_count() > 0:
        assert blob_diff(fd.find_laser_blobs(frames, want_mask=True, want_labels=True), blobs_oracle(frames)) is None
        return
    with pytest.raises(_native.SbaError, match="no HIP device"):
        fd.find_laser_blobs(frames)
    with pytest.raises(_native.SbaError, match="no HIP device"):
        fd.green_laser_finder(frames[1])


# ----------------------------------------------------------------------------- 2. the oracle checks itself
def test_disks_equal_the_patterns_of_skimages_formula():
    assert disk(1).tolist() == [[0, 1, 0], [1, 1, 1], [0, 1, 0]]
    rows = ["000010000", "001111100", "011111110", "011111110", "111111111", "011111110", "011111110", "001111100", "000010000"]
    assert ["".join(str(v) for v in r) for r in disk(4)] == rows
    for r in range(9):
        assert np.array_equal(fd.disk(r), disk(r)) and fd.disk(r).dtype == np.uint8 and disk(r).shape == (2 * r + 1,) * 2
    assert disk(0).tolist() == [[1]]


def test_morphed_mask_contains_the_raw_mask_and_labels_come_in_raster_order():
    rng = np.random.default_rng(2)
    for density in (0.002, 0.03, 0.3):
        for radii in ((1, 4), (0, 0), (2, 3), (8, 8)):
            raw = rng.random((45, 70)) < density
            o = blobs_oracle(mask_frames(raw[None]), dilate_radius=radii[0], close_radius=radii[1], max_blobs=64)
            assert np.all(o.mask[0][raw] == 1)
            lab, n = o.labels[0], int(o.n_components[0])
            assert n == lab.max() and set(np.unique(lab)) == set(range(n + 1)) - ({0} if o.mask[0].all() else set())
            first = [int(np.flatnonzero(lab.ravel() == k)[0]) for k in range(1, n + 1)]
            assert first == sorted(first)                               # numbered by their first pixel in raster order
            for k in range(min(n, 64)):
                sel = lab == k + 1
                ys, xs = np.nonzero(sel)
                r = [int(v) for v in o.blobs[0, k]]
                assert r[:4] == [sel.sum(), xs.sum(), ys.sum(), (sel & raw).sum()] and r[8:] == [xs.min(), ys.min(), xs.max(), ys.max()]
                assert r[4] == 130 * r[3] and r[7] == 0                   # value 200, threshold 70


def test_two_dots_join_at_a_gap_of_6_and_stay_two_at_7_on_the_diagonal_at_4_and_5():
    for gap, diagonal, want in ((6, False, 1), (7, False, 2), (4, True, 1), (5, True, 2)):
        o = blobs_oracle(mask_frames(two_dots(gap, diagonal)[None]))
        assert o.n_components[0] == want and o.status[0] == (OK if want == 1 else MULTIPLE), (gap, diagonal)
    o = blobs_oracle(mask_frames(two_dots(2)[None]), dilate_radius=0, close_radius=0)     # without the morphology they stay apart
    assert o.n_components[0] == 2 and [int(v) for v in o.blobs[0, 0, :3]] == [9, 54, 99]


def test_the_border_rule_keeps_a_blob_in_the_corner():
    raw = np.zeros((20, 20), bool)
    raw[0:2, 0:2] = True
    ours = morph(raw, 0, 4)
    assert ours[0:2, 0:2].all() and ours.sum() >= 4
    theirs = ndimage.binary_closing(raw, structure=disk(4))              # scipy's closing erodes with a 0 border
    assert theirs.sum() == 0
    o = blobs_oracle(mask_frames(raw[None]))
    assert o.status[0] == OK and o.n_components[0] == 1 and tuple(o.blobs[0, 0, 8:10]) == (0, 0)
    inner = np.zeros((40, 40), bool)
    inner[18:21, 17:22] = True
    assert np.array_equal(morph(inner, 1, 4), ndimage.binary_closing(ndimage.binary_dilation(inner, disk(1)), structure=disk(4)))


def island_mask():
    """Two raw pixels a knight's-move-and-a-bit apart, (14, 13) and (16, 17) as (row, col): closed by disk(4), the dilated discs
    overlap in a lens whose middle pixel (15, 15) survives the erosion while nothing joins it to either pixel -- a component of
    the morphed mask that holds no raw pixel."""
    raw = np.zeros((40, 40), bool)
    raw[14, 13] = raw[16, 17] = True
    return raw


def test_a_closing_island_without_a_raw_pixel_has_a_nan_weighted_centroid():
    raw = island_mask()
    o = blobs_oracle(mask_frames(raw[None]), dilate_radius=0, close_radius=4)
    assert o.n_components[0] == 3 and o.status[0] == MULTIPLE
    assert [[int(v) for v in o.blobs[0, k]] for k in range(3)] == [[1, 13, 14, 1, 130, 1690, 1820, 0, 13, 14, 13, 14],
                                                                   [1, 15, 15, 0, 0, 0, 0, 0, 15, 15, 15, 15],
                                                                   [1, 17, 16, 1, 130, 2210, 2080, 0, 17, 16, 17, 16]]
    lone = blobs_oracle(mask_frames(raw[None]), dilate_radius=0, close_radius=4, centre=(15, 15), max_centre_dist=1)
    assert lone.status[0] == OK and lone.accepted[0] == 1               # the distance filter singles the island out
    assert tuple(lone.centroid[0, :2]) == (15.0, 15.0) and np.isnan(lone.centroid[0, 2:]).all()
    assert tuple(fd.blob_centroid_table(lone)[0]) == (15.0, 15.0) and np.isnan(fd.blob_centroid_table(lone, weighted=True)).all()


def test_every_status_is_reached():
    m = np.zeros((5, 60, 80), bool)
    m[1, 10:13, 10:13] = True                                            # one dot
    m[2, 10:13, 10:13] = True
    m[2, 40:43, 60:63] = True                                            # two dots, far apart
    for i in range(10):
        m[3, 5, 5 + 7 * i] = True                                        # ten components
    m[4, 30:34, 30:36] = True
    o = blobs_oracle(mask_frames(m), dilate_radius=0, close_radius=0)
    assert list(o.status) == [NONE, OK, MULTIPLE, OVERFLOW, OK] and list(o.n_components) == [0, 1, 2, 10, 1]
    assert list(o.accepted) == [-1, 0, -1, -1, 0] and np.isnan(o.centroid[[0, 2, 3]]).all()
    assert tuple(o.centroid[1]) == (11.0, 11.0, 11.0, 11.0) and [int(v) for v in o.blobs[3, 7, :3]] == [1, 54, 5] and not o.blobs[1, 1:].any()
    assert list(blobs_oracle(mask_frames(m), dilate_radius=0, close_radius=0, min_area=10).status) == [NONE, REJECTED, REJECTED, OVERFLOW, OK]
    assert list(blobs_oracle(mask_frames(m), dilate_radius=0, close_radius=0, max_area=9, max_blobs=16).status) == [NONE, OK, MULTIPLE, MULTIPLE, REJECTED]
    near = blobs_oracle(mask_frames(m), dilate_radius=0, close_radius=0, centre=(11, 11), max_centre_dist=5)
    assert list(near.status) == [NONE, OK, OK, OVERFLOW, REJECTED] and near.accepted[2] == 0
    assert list(blobs_oracle(mask_frames(m), dilate_radius=0, close_radius=0, centre=(61, 41), max_centre_dist=1).accepted) == [-1, -1, 1, -1, -1]


def test_the_integer_distance_filter_at_the_16384_wide_extreme():
    """A component that fills a 16384 x 16384 frame but for its first row: n (2^14 - 1) 2^14, centroid x = 8191.5 exactly.  The test
    (sum x - cx n)^2 + (sum y - cy n)^2 <= (d n)^2 has terms above 2^82: beyond 64-bit integers, and float64 does not resolve them."""
    W = H = 16384
    n = W * (H - 1)
    sx, sy = (H - 1) * (W * (W - 1) // 2), W * (H * (H - 1) // 2)
    rec = [n, sx, sy, 0, 0, 0, 0, 0, 0, 1, W - 1, H - 1]
    assert 2 * sx == 16383 * n and 2 * sy == 16384 * n                   # centroid (8191.5, 8192)
    # from (0, 0) the centroid is sqrt(8191.5^2 + 8192^2) = 11584.88.. away, from (2047, 0) sqrt(6144.5^2 + 8192^2) = 10240.30..
    assert judge(1, [rec], 8, centre=(0, 0), max_centre_dist=11585) == (OK, 0)
    assert judge(1, [rec], 8, centre=(0, 0), max_centre_dist=11584) == (REJECTED, -1)
    assert judge(1, [rec], 8, centre=(2047, 0), max_centre_dist=10241) == (OK, 0)
    assert judge(1, [rec], 8, centre=(2047, 0), max_centre_dist=10240) == (REJECTED, -1)
    # exactly on the boundary (<= accepts): one pixel at (16383, 0), the centre a 3-4-5 triangle away: 12288, 16384, 20480
    rec1 = [1, 16383, 0, 1, 1, 16383, 0, 0, 16383, 0, 16383, 0]
    assert judge(1, [rec1], 8, centre=(16383 - 12288, -16384), max_centre_dist=20480) == (OK, 0)
    assert judge(1, [rec1], 8, centre=(16383 - 12288, -16384), max_centre_dist=20479) == (REJECTED, -1)
    big = (sx - 0 * n) ** 2 + (sy - 0 * n) ** 2
    assert big > 2 ** 82 and float(big) == float(big + 2 ** 20)          # what a float64 comparison would not see


def test_blob_centroid_table_order_and_nan_rows():
    m = np.zeros((4, 30, 50), bool)
    m[0, 4:7, 20:25] = True
    m[2, 4:7, 20:25] = True
    m[2, 20:23, 40:43] = True
    m[3, 10, 10:13] = True
    f = mask_frames(m)
    f[3, 10, 12, 1] = 255                                                # weights 130, 130, 185: the weighted centroid moves right
    o = blobs_oracle(f, dilate_radius=0, close_radius=0)
    t = fd.blob_centroid_table(o)
    assert t.shape == (4, 2) and t.dtype == np.float64 and list(o.status) == [OK, NONE, MULTIPLE, OK]
    assert tuple(t[0]) == (5.0, 22.0) and np.isnan(t[1:3]).all() and tuple(t[3]) == (10.0, 11.0)           # (row, col)
    tw = fd.blob_centroid_table(o, weighted=True)
    assert tuple(tw[0]) == (5.0, 22.0) and tw[3, 0] == 10.0 and tw[3, 1] == (130 * 10 + 130 * 11 + 185 * 12) / 445
    assert o.blobs[3, 0, 7] == 1 and np.array_equal(np.isnan(tw), np.isnan(t))


def test_green_laser_finder_validates_its_footprints():
    img = np.zeros((8, 8, 3), np.uint8)
    for bad in (np.ones((3, 3)), np.ones((2, 2)), disk(9), np.ones(3), disk(2)[:, :3]):
        with pytest.raises(ValueError, match="disk"):
            fd.green_laser_finder(img, small_footprint=bad)
        with pytest.raises(ValueError, match="disk"):
            fd.green_laser_finder(img, big_footprint=bad)
    with pytest.raises(ValueError, match="frame"):
        fd.green_laser_finder(img[:, :, 0])
    assert fd._disk_radius(None, 4, "x") == 4 and fd._disk_radius(disk(0), 1, "x") == 0 and fd._disk_radius(disk(8).astype(bool), 1, "x") == 8
    assert fd._disk_radius(disk(3) * 255, 1, "x") == 3
