"""GPU tests of sba_detect_blobs (include/sba_hip.h) through ``lasercalib_amd.feature_detection``: the morphed mask, the labels,
the component records, the verdicts and the centroids of batches of frames.

The reference is ``blobs_oracle`` of tests/test_blobs_host.py (scipy.ndimage morphology and labelling, exact integers; checked
there against hand-built cases).  The device's values are exact integers too and each centroid is one IEEE division of two of
them, so EVERY comparison here is bit equality: ``blob_diff`` names the first stage that differs -- mask, labels, n_components,
blobs, accepted, status, centroid -- or is None.  Nothing needs a tolerance.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lasercalib_amd import _native, feature_detection as fd  # noqa: E402
from test_blobs_host import MULTIPLE, NONE, OK, OVERFLOW, REJECTED, blob_diff, blobs_oracle, island_mask, mask_frames, two_dots  # noqa: E402
from test_detect_host import render_spots  # noqa: E402
from test_gpu_detect import device_view, pitched  # noqa: E402

MORPH_ROWS, TILE_ROWS, MORPH_WORDS = _native.BLOB_MORPH_ROWS, _native.BLOB_TILE_ROWS, _native.BLOB_MORPH_WORDS


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert _native.device_count() > 0, "no HIP device visible: GPU tests must run on the MI355X box"


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def test_the_geometry_constants_are_those_of_the_kernels():
    text = open(os.path.join(os.path.dirname(_native.__file__), "csrc", "sba_blobs.hpp")).read()
    import re
    for name, value in (("MORPH_ROWS", MORPH_ROWS), ("TILE_ROWS", TILE_ROWS), ("MORPH_WORDS", MORPH_WORDS)):
        assert int(re.search(rf"\b{name} = (\d+)", text).group(1)) == value


def check(frames, on=None, **kw):
    """The device's answer for `frames` (and for `on`, the same frames elsewhere, when given) against the oracle, every stage."""
    want = blobs_oracle(frames, **kw)
    for src in (frames,) if on is None else (frames, on):
        got = fd.find_laser_blobs(src, want_mask=True, want_labels=True, **kw)
        assert blob_diff(got, want) is None, (blob_diff(got, want), kw)
    return want


def random_masks(shape, densities, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.random(shape) < d for d in densities])


# ----------------------------------------------------------------------------- 1. sizes that straddle words, bands and tiles
@pytest.mark.parametrize("W", [1, 63, 64, 65, 127, 130, 200])
def test_widths_and_heights_that_straddle_words_bands_and_tiles(torch, W):
    heights = sorted({r + d for r in (MORPH_ROWS, TILE_ROWS, 2 * TILE_ROWS) for d in (-1, 0, 1)})
    for i, H in enumerate(heights):
        frames = mask_frames(random_masks((H, W), (0.03, 0.3), 100 * W + H))
        dev = torch.from_numpy(frames).cuda() if i % 2 else None
        check(frames, dev, max_blobs=64)
        check(frames, dilate_radius=0, close_radius=0, max_blobs=64)


def test_a_frame_wider_than_one_morphology_band(torch):
    W = 64 * MORPH_WORDS * 2 + 70                                        # three bands of words, the last one partial
    frames = mask_frames(random_masks((TILE_ROWS + 3, W), (0.01, 0.1), 5))
    check(frames, torch.from_numpy(frames).cuda(), max_blobs=64)
    check(frames, dilate_radius=8, close_radius=8, max_blobs=64)


# ----------------------------------------------------------------------------- 2. random masks, every radius pair
DENSITIES = (0.002, 0.01, 0.03, 0.1, 0.3)


@pytest.mark.parametrize("radii", [(1, 4), (0, 0), (0, 4), (2, 3), (0, 8), (8, 8)])
@pytest.mark.parametrize("shape", [(45, 70), (150, 200)])
def test_random_masks(torch, shape, radii):
    frames = mask_frames(random_masks(shape, DENSITIES, shape[0]))
    want = check(frames, torch.from_numpy(frames).cuda(), dilate_radius=radii[0], close_radius=radii[1], max_blobs=64)
    assert want.n_components.max() > 1 or radii[1] == 8


@pytest.mark.parametrize("C", [1, 3, 4])
def test_layouts_channels_pitches_and_a_misaligned_base(torch, C):
    rng = np.random.default_rng(30 + C)
    frames = rng.integers(0, 256, size=(3, 47, 61, C), dtype=np.uint8)
    frames[rng.random(frames.shape) < 0.9] = 0
    frames[rng.random(frames.shape) < 0.01] = 255
    B, H, W, _ = frames.shape
    for channel in range(C):
        want = blobs_oracle(frames, channel=channel, threshold=50, max_blobs=32)
        assert want.blobs[:, :, 7].any()                                  # saturated pixels are counted
        for row_pitch in (W * C, W * C + 5):
            buf, view, frame_pitch = pitched(frames, row_pitch, 13)
            keep, dev = device_view(torch, buf, (B, H, W, C), (frame_pitch, row_pitch, C, 1))
            for src in (view, dev):
                got = fd.find_laser_blobs(src, channel=channel, threshold=50, max_blobs=32, want_mask=True, want_labels=True)
                assert blob_diff(got, want) is None, (blob_diff(got, want), channel, row_pitch)
    want = blobs_oracle(frames, channel=C // 2, threshold=50, max_blobs=32)
    for offset in (1, 7, 15):
        big = torch.full((B * H * W * C + 32,), 255, dtype=torch.uint8, device="cuda")
        view = big[offset:offset + B * H * W * C].view(B, H, W, C)
        view.copy_(torch.from_numpy(frames))
        assert view.data_ptr() % 16 != 0
        got = fd.find_laser_blobs(view, channel=C // 2, threshold=50, max_blobs=32, want_mask=True, want_labels=True)
        assert blob_diff(got, want) is None, (blob_diff(got, want), offset)
    if C == 1:
        assert blob_diff(fd.find_laser_blobs(frames[..., 0], channel=0, threshold=50, max_blobs=32), want) is None


# ----------------------------------------------------------------------------- 3. structured masks (radii 0, 0: the shapes survive)
def structured_masks(H, W):
    """name -> (H, W) mask; H and W span several tiles and words."""
    y, x = np.mgrid[0:H, 0:W]
    out = {}
    u = np.zeros((H, W), bool)
    u[2:H - 4, 3] = u[2:H - 4, W - 9] = True
    u[H - 5, 3:W - 8] = True
    out["U"] = u
    comb = (x % 4 == 1) & (y < H - 1)
    comb[H - 1, 1:W] = True                                              # the arms meet only in the last row
    out["comb"] = comb
    sp = np.zeros((H, W), bool)
    top, left, bottom, right = 0, 0, H - 1, W - 1
    while top <= bottom and left <= right:                               # a rectangular spiral, one pixel wide, one line of gap
        sp[top, left:right + 1] = True
        sp[top:bottom + 1, right] = True
        if bottom - top >= 2 and right - left >= 2:
            sp[bottom, left + 2:right + 1] = True
            sp[top + 2:bottom + 1, left + 2] = True
        top, left, bottom, right = top + 2, left + 2, bottom - 2, right - 2
        if top <= bottom and left <= right:
            sp[top, left] = True                                         # the arm turns inwards: joins the next ring
    out["spiral"] = sp
    out["checkerboard"] = (x + y) % 2 == 0
    out["diagonals"] = (x == y) | (x == H - 1 - y)
    corner = np.zeros((H, W), bool)
    corner[10, 63] = corner[11, 64] = True                               # corner to corner across a word boundary
    corner[TILE_ROWS - 2:TILE_ROWS, 126:128] = corner[TILE_ROWS:TILE_ROWS + 2, 128:130] = True        # across a tile corner
    corner[2 * TILE_ROWS - 1, 64] = corner[2 * TILE_ROWS, 63] = True     # the other diagonal of a tile corner
    out["corners"] = corner
    out["full"] = np.ones((H, W), bool)
    snake = (y % 2 == 0)
    snake |= (y % 4 == 1) & (x == W - 1)
    snake |= (y % 4 == 3) & (x == 0)
    out["snake"] = snake
    return out


def test_structured_masks(torch):
    H, W = 2 * TILE_ROWS + 7, 64 * 2 + 13
    masks = structured_masks(H, W)
    names = list(masks)
    frames = mask_frames(np.stack([masks[n] for n in names]))
    want = check(frames, torch.from_numpy(frames).cuda(), dilate_radius=0, close_radius=0, max_blobs=64)
    n = dict(zip(names, want.n_components))
    assert n["U"] == 1 and n["comb"] == 1 and n["checkerboard"] == 1 and n["full"] == 1 and n["snake"] == 1 and n["diagonals"] == 1
    assert n["corners"] == 3 and n["spiral"] == 1, n
    from scipy import ndimage
    assert ndimage.label(masks["diagonals"])[1] > 1 and ndimage.label(masks["checkerboard"])[1] > 1      # 4-connectivity would differ
    assert int(want.blobs[names.index("full"), 0, 0]) == H * W


# ----------------------------------------------------------------------------- 4. the reference's rule through the default morphology
def test_gap_pairs_join_and_part_as_the_oracle_says():
    masks = np.stack([two_dots(6), two_dots(7), two_dots(4, True), two_dots(5, True)])
    want = check(mask_frames(masks))
    assert list(want.n_components) == [1, 2, 1, 2] and list(want.status) == [OK, MULTIPLE, OK, MULTIPLE]


def test_dots_at_all_four_borders_and_corners(torch):
    H, W = 50, 90
    spots = [(0, 0), (0, W - 2), (H - 2, 0), (H - 2, W - 2), (0, 44), (H - 2, 44), (24, 0), (24, W - 2)]
    masks = np.zeros((1 + len(spots), H, W), bool)
    for i, (y0, x0) in enumerate(spots):
        masks[0, y0:y0 + 2, x0:x0 + 2] = True
        masks[1 + i, y0:y0 + 2, x0:x0 + 2] = True
    frames = mask_frames(masks)
    want = check(frames, torch.from_numpy(frames).cuda(), max_blobs=16)
    assert want.n_components[0] == 8 and np.all(want.n_components[1:] == 1) and np.all(want.status[1:] == OK)
    check(frames, dilate_radius=0, close_radius=8, max_blobs=16)


def test_an_empty_frame_between_frames_with_dots():
    masks = np.zeros((3, 40, 70), bool)
    masks[0, 5:8, 5:8] = masks[2, 30:33, 60:63] = True
    want = check(mask_frames(masks))
    assert list(want.status) == [OK, NONE, OK] and not want.blobs[1].any() and np.isnan(want.centroid[1]).all()


def test_more_components_than_max_blobs():
    masks = np.zeros((2, 40, 140), bool)
    for i in range(10):
        masks[0, 3 + (i % 3) * 12, 5 + 13 * i] = True
    masks[1, 20, 20] = True
    want = check(mask_frames(masks), max_blobs=4)
    assert list(want.status) == [OVERFLOW, OK] and list(want.n_components) == [10, 1] and want.blobs.shape == (2, 4, 12)
    assert np.all(want.blobs[0, :, 0] > 0) and want.labels[0].max() == 10
    assert list(check(mask_frames(masks), max_blobs=10).status) == [MULTIPLE, OK]
    assert check(mask_frames(masks), max_blobs=0).blobs.shape == (2, 8, 12)


def test_every_filter():
    masks = np.zeros((3, 60, 80), bool)
    masks[0, 10:13, 10:13] = True
    masks[1, 10:13, 10:13] = masks[1, 40:44, 60:66] = True
    masks[2, :40, :40] = island_mask()                                   # closed by disk(4): an island without a raw pixel
    frames = mask_frames(masks)
    seen = set()
    for kw in (dict(), dict(min_area=60), dict(max_area=60), dict(min_area=1000), dict(centre=(11, 11), max_centre_dist=3),
               dict(centre=(60, 40), max_centre_dist=12), dict(centre=(-500, 9000), max_centre_dist=20),
               dict(min_area=60, max_area=70, centre=(11, 11), max_centre_dist=3), dict(max_area=1)):
        want = check(frames, **kw)
        seen |= set(int(s) for s in want.status)
    assert seen == {OK, REJECTED, MULTIPLE}
    lone = check(frames[2:], dilate_radius=0, close_radius=4, centre=(15, 15), max_centre_dist=1)
    assert lone.status[0] == OK and lone.accepted[0] == 1 and np.isnan(lone.centroid[0, 2:]).all() and lone.blobs[0, 1, 3] == 0


def test_regions_that_cut_a_dot(torch):
    masks = np.zeros((2, 50, 90), bool)
    masks[0, 20:27, 30:37] = True
    masks[1, 20:27, 30:37] = masks[1, 5:8, 70:73] = True
    frames = mask_frames(masks)
    dev = torch.from_numpy(frames).cuda()
    for roi in (dict(roi_rect=(33, 0, 90, 50)), dict(roi_rect=(0, 23, 34, 24)), dict(roi_circle=(30, 20, 4)), dict(roi_circle=(36, 26, 3)),
                dict(roi_rect=(-5, 22, 35, 400), roi_circle=(33, 23, 2)), dict(roi_rect=(60, 0, 90, 50)), dict(roi_rect=(7, 3, 7, 9)),
                dict(roi_circle=(200, 200, 10))):
        for radii in ((1, 4), (0, 0)):
            check(frames, dev, dilate_radius=radii[0], close_radius=radii[1], **roi)
    cut = blobs_oracle(frames, roi_rect=(33, 0, 90, 50), dilate_radius=0, close_radius=0)
    assert cut.blobs[0, 0, 0] == 4 * 7 and cut.blobs[0, 0, 8] == 33


def test_a_one_by_one_frame(torch):
    frames = np.zeros((2, 1, 1, 3), np.uint8)
    frames[1, 0, 0, 1] = 255
    want = check(frames, torch.from_numpy(frames).cuda())
    assert list(want.status) == [NONE, OK] and [int(v) for v in want.blobs[1, 0]] == [1, 0, 0, 1, 185, 0, 0, 1, 0, 0, 0, 0]
    assert tuple(want.centroid[1]) == (0.0, 0.0, 0.0, 0.0)


# ----------------------------------------------------------------------------- 5. chunking, repeatability, arguments
def test_chunking_and_repeatability(torch):
    frames = mask_frames(random_masks((45, 70), (0.0, 0.01, 0.03, 0.0, 0.1, 0.002, 0.3), 77))
    want = blobs_oracle(frames, max_blobs=16)
    dev = torch.from_numpy(frames).cuda()
    runs = []
    for src in (frames, dev):
        for chunk in (1, 2, 0):
            got = fd.find_laser_blobs(src, max_blobs=16, chunk_frames=chunk, want_mask=True, want_labels=True)
            assert blob_diff(got, want) is None, (blob_diff(got, want), chunk)
            runs.append(got)
    # host frames in each class of layout a pitched copy tells apart -- packed, padded rows, a gap between packed frames, both --
    # in four chunks, the last one short: both staging buffers are used again; the padding is bright
    for row_slack, frame_slack in ((0, 0), (5, 0), (0, 13), (5, 13)):
        _buf, view, _fp = pitched(frames, 70 * 3 + row_slack, frame_slack)
        got = fd.find_laser_blobs(view, max_blobs=16, chunk_frames=2, want_mask=True, want_labels=True)
        assert blob_diff(got, want) is None, (blob_diff(got, want), row_slack, frame_slack)
    again =fd.find_laser_blobs(dev, max_blobs=16, want_mask=True, want_labels=True)
    for got in runs:
        assert again.blobs.tobytes() == got.blobs.tobytes() and again.centroid.tobytes() == got.centroid.tobytes()
        assert again.labels.tobytes() == got.labels.tobytes() and again.status.tobytes() == got.status.tobytes()
    # n_frames = 0 writes nothing
    lib = _native.load()
    nc, st = np.full(1, 7, np.int32), np.full(1, 7, np.int32)
    tab, cen = np.full(96, 7, np.uint64), np.full(4, 7.0)
    rc = lib.sba_detect_blobs(0, frames.ctypes.data, 0, 45, 70, 3, 210, 45 * 210, None, nc.ctypes.data, tab.ctypes.data, None,
                              cen.ctypes.data, st.ctypes.data, None, None)
    assert rc == 0 and nc[0] == 7 and st[0] == 7 and np.all(tab == 7) and np.all(cen == 7.0)
    assert len(fd.find_laser_blobs(np.zeros((0, 45, 70, 3), np.uint8)).status) == 0


def test_null_options_are_the_defaults_and_every_output_is_optional():
    frames = mask_frames(np.stack([two_dots(6), two_dots(7)]), value=71)
    frames[1, 11, 6, 1] = 70                                             # value == threshold 70 does not count
    lib = _native.load()
    want = blobs_oracle(frames, threshold=70, channel=1, dilate_radius=1, close_radius=4, max_blobs=8)
    B, H, W, C = frames.shape
    nc, st, acc = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    tab, cen = np.zeros((B, 8, 12), np.uint64), np.zeros((B, 4))
    args = (0, frames.ctypes.data, B, H, W, C, W * C, H * W * C, None)
    rc = lib.sba_detect_blobs(*args, nc.ctypes.data, tab.ctypes.data, acc.ctypes.data, cen.ctypes.data, st.ctypes.data, None, None)
    assert rc == 0 and blob_diff(_native.LaserBlobs(nc, tab, acc, cen, st), want) is None
    assert want.blobs[1, 0, 3] == 8 and list(want.status) == [OK, MULTIPLE]
    assert lib.sba_detect_blobs(*args, None, None, None, None, None, None, None) == 0
    # judged without the table, two frames in one chunk: each frame from its own rows of the chunk's table (reversed, so that
    # the second frame, judged from the first one's rows, would come out OK with the centroid of the wrong component)
    rev = np.ascontiguousarray(frames[::-1])
    rargs = (0, rev.ctypes.data) + args[2:]
    out = [(np.full(B, 7, np.int32), np.full((B, 4), 7.0), np.full(B, 7, np.int32)) for _ in range(2)]
    for (a, c, s), table in zip(out, (tab, None)):
        assert lib.sba_detect_blobs(*rargs, None, None if table is None else table.ctypes.data, a.ctypes.data, c.ctypes.data, s.ctypes.data, None, None) == 0
        assert list(s) == [MULTIPLE, OK] and list(a) == [-1, 0] and np.array_equal(c, want.centroid[::-1], equal_nan=True)
    labels = np.zeros((B, H, W), np.int32)
    assert lib.sba_detect_blobs(*args, None, None, None, None, None, None, labels.ctypes.data) == 0 and np.array_equal(labels, want.labels)
    mask = np.zeros((B, H, W), np.uint8)
    assert lib.sba_detect_blobs(*args, None, None, None, None, None, mask.ctypes.data, None) == 0 and np.array_equal(mask, want.mask)


def test_rejected_arguments():
    lib = _native.load()
    frames = np.zeros((2, 8, 10, 3), np.uint8)
    p = frames.ctypes.data
    INVALID, UNSUPPORTED = -1, -6

    def call(ptr=p, n=2, h=8, w=10, c=3, rp=30, fp=240, **o):
        opts = _native.BlobOpts(channel=1, threshold=70, dilate_radius=1, close_radius=4)
        for k, v in o.items():
            setattr(opts, k, v)
        out = np.zeros(2, np.int32)
        rc = lib.sba_detect_blobs(0, ptr, n, h, w, c, rp, fp, ctypes.byref(opts), out.ctypes.data, None, None, None, None, None, None)
        return rc, (lib.sba_last_error(None) or b"").decode()

    assert call()[0] == 0
    for kw, code in ((dict(ptr=None), INVALID), (dict(c=2), INVALID), (dict(channel=3), INVALID), (dict(channel=-1), INVALID),
                     (dict(threshold=256), INVALID), (dict(threshold=-1), INVALID), (dict(rp=29), INVALID), (dict(fp=239), INVALID),
                     (dict(n=-1), INVALID), (dict(h=-1), INVALID), (dict(w=-1), INVALID), (dict(dilate_radius=9), INVALID),
                     (dict(dilate_radius=-1), INVALID), (dict(close_radius=9), INVALID), (dict(close_radius=-1), INVALID),
                     (dict(max_blobs=65), INVALID), (dict(max_blobs=-1), INVALID), (dict(min_area=-1), INVALID), (dict(max_area=-1), INVALID),
                     (dict(max_centre_dist=-1), INVALID), (dict(w=16385, rp=3 * 16385, fp=8 * 3 * 16385), UNSUPPORTED),
                     (dict(h=16385, fp=16385 * 30), UNSUPPORTED)):
        rc, msg = call(**kw)
        assert rc == code and msg.startswith("sba_detect_blobs"), (kw, rc, msg)
    assert call(ptr=None, n=0)[0] == 0


def test_the_distance_filter_on_a_16384_wide_frame(torch):
    H, W = 9, 16384
    frames = torch.full((1, H, W), 255, dtype=torch.uint8, device="cuda")
    frames[0, 0] = 0                                                     # the component: rows 1..8, centroid (8191.5, 4.5)
    got = [fd.find_laser_blobs(frames, channel=0, dilate_radius=0, close_radius=0, centre=(0, 4), max_centre_dist=d) for d in (8192, 8191)]
    n = 8 * W
    assert [int(v) for v in got[0].blobs[0, 0]] == [n, 8 * (W * (W - 1) // 2), W * 36, n, 185 * n, 185 * 8 * (W * (W - 1) // 2),
                                                    185 * W * 36, n, 0, 1, W - 1, 8]
    assert (got[0].status[0], got[1].status[0]) == (OK, REJECTED)        # 8191.5^2 + 0.5^2 lies between 8191^2 and 8192^2
    assert tuple(got[0].centroid[0]) == (8191.5, 4.5, 8191.5, 4.5)


# ----------------------------------------------------------------------------- 6. the reference's function and full-size frames
def test_green_laser_finder_on_rendered_spots():
    rng = np.random.default_rng(4)
    spots, _ = render_spots(6, 33, rng, noise=30)
    frames = np.zeros((6, 33, 80, 3), np.uint8)
    frames[:, :, :33, 1] = spots
    frames[3:, :, 45:78, 1] = spots[:3]                                  # frames 3..5 hold two spots
    want = blobs_oracle(frames, threshold=70)
    assert list(want.n_components[:3]) == [1, 1, 1] and np.all(want.n_components[3:] == 2)
    for f in range(6):
        got = fd.green_laser_finder(frames[f])
        if want.n_components[f] == 1:
            assert got == (want.centroid[f, 1], want.centroid[f, 0]) and all(isinstance(v, float) for v in got)
        else:
            assert got is None
    from test_blobs_host import disk
    assert fd.green_laser_finder(frames[0], 70, 1100, disk(1), disk(4)) == fd.green_laser_finder(frames[0])
    w2 = blobs_oracle(frames[:1], threshold=50, dilate_radius=2, close_radius=0)
    assert fd.green_laser_finder(frames[0], 50, small_footprint=disk(2), big_footprint=disk(0)) == (w2.centroid[0, 1], w2.centroid[0, 0])


def test_full_size_frames_tell_a_reflection_from_a_single_spot(torch):
    rng = np.random.default_rng(21)
    H, W, S = 2200, 3208, 33
    spots, _ = render_spots(2, S, rng)
    frames = np.repeat(rng.integers(0, 31, size=(1, H, W, 3), dtype=np.uint8), 2, axis=0)            # dark noise, all channels
    frames[0, 1000:1000 + S, 1500:1500 + S, 1] = spots[0]
    frames[1, 1000:1000 + S, 1500:1500 + S, 1] = spots[0]
    frames[1, 1000:1000 + S, 1800:1800 + S, 1] = spots[1] // 2 + 60      # a dimmer reflection 300 px away
    dev = torch.from_numpy(frames).cuda()
    want = check(frames, dev, threshold=50)
    assert list(want.status) == [OK, MULTIPLE] and list(want.n_components) == [1, 2]
    assert np.all(fd.find_laser_dots(dev, threshold=50).status == fd.SBA_DOT_OK)          # the moments alone call both frames good
    table = fd.blob_centroid_table(want)
    assert abs(table[0, 0] - 1016) < 10 and abs(table[0, 1] - 1516) < 10 and np.isnan(table[1]).all()


def test_smoke_passes_with_its_blob_case(capsys):
    import __graft_entry__ as g
    g.smoke()
    assert "smoke ok (connected components)" in capsys.readouterr().out
