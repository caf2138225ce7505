"""Host tests of the conversion to encoder frames (sba_frames_to_yuv, include/sba_hip.h): the numpy oracle of its rule, the
integer matrices of ``imaging.RgbMatrix``, the layouts a result is allocated in and the Python argument checks.  No GPU.

``to_yuv_oracle`` follows the header's rule literally, in int64; tests/test_gpu_yuv.py compares the kernel with it bit for bit.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lasercalib_amd import _native, imaging  # noqa: E402
from lasercalib_amd.imaging import RgbMatrix  # noqa: E402
from test_convert_host import BT601 as YUV_BT601, convert_oracle  # noqa: E402

BT601 = (16, 269484, 528482, 102760, -155188, -305135, 460324, 460324, -385875, -74448)      # OpenCV's table, as the header states it
IN_FORMATS = ("bgr", "rgb", "bgra", "rgba", "gray")
PRESETS = ("bt601", "bt709", "bt601-full", "bt709-full")


def rgb_planes(frames, in_format):
    """(R, G, B) int64 planes (B, H, W) of frames (B, H, W, C) or (B, H, W) in ``in_format``."""
    f = np.asarray(frames).astype(np.int64)
    if f.ndim == 3 or f.shape[3] == 1:
        g = f if f.ndim == 3 else f[..., 0]
        return g, g, g
    return (f[..., 0], f[..., 1], f[..., 2]) if in_format in ("rgb", "rgba") else (f[..., 2], f[..., 1], f[..., 0])


def to_yuv_oracle(frames, matrix=BT601, in_format="bgr", chroma="nearest"):
    """The rule of include/sba_hip.h in int64 -> plain uint8 planes y (B, H, W), u and v (B, ceil(H / 2), ceil(W / 2))."""
    y_offset, cry, cgy, cby, cru, cgu, cbu, crv, cgv, cbv = (int(c) for c in matrix)
    R, G, B = rgb_planes(frames, in_format)
    H, W = R.shape[1:]
    y = np.clip((cry * R + cgy * G + cby * B + (1 << 19) + (y_offset << 20)) >> 20, 0, 255)     # >> on int64: the arithmetic shift
    jj, ii = 2 * np.arange((H + 1) // 2), 2 * np.arange((W + 1) // 2)
    if chroma == "nearest":
        r, g, b = (p[:, jj][:, :, ii] for p in (R, G, B))
        sh = 20
    else:
        r, g, b = (sum(p[:, np.minimum(jj + db, H - 1)][:, :, np.minimum(ii + da, W - 1)] for da in (0, 1) for db in (0, 1)) for p in (R, G, B))
        sh = 22
    cc = (1 << (sh - 1)) + (128 << sh)
    u = np.clip((cru * r + cgu * g + cbu * b + cc) >> sh, 0, 255)
    v = np.clip((crv * r + cgv * g + cbv * b + cc) >> sh, 0, 255)
    return y.astype(np.uint8), u.astype(np.uint8), v.astype(np.uint8)


def one(R, G, B, matrix=BT601):
    y, u, v = to_yuv_oracle(np.array([[[[R, G, B]]]], np.uint8), matrix, "rgb")
    return int(y[0, 0, 0]), int(u[0, 0, 0]), int(v[0, 0, 0])


# ----------------------------------------------------------------------------- the default table, over all 2^24 triples
def test_default_table_over_every_triple():
    """The four properties that identify OpenCV's BT.601 table: the ranges with no clip ever active, grey -> 128, the primaries,
    and the round trip through the forward table of sba_convert_frames."""
    y_offset, cry, cgy, cby, cru, cgu, cbu, crv, cgv, cbv = BT601
    G, B = (a.astype(np.int64) for a in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))
    lo, hi = np.full(3, 1 << 40), np.full(3, -(1 << 40))
    worst = np.zeros(3, np.int64)
    for R in range(256):
        sums = (cry * R + cgy * G + cby * B + (1 << 19) + (y_offset << 20), cru * R + cgu * G + cbu * B + (1 << 19) + (128 << 20),
                crv * R + cgv * G + cbv * B + (1 << 19) + (128 << 20))
        yuv = [s >> 20 for s in sums]                                          # BEFORE the clip
        lo, hi = np.minimum(lo, [a.min() for a in yuv]), np.maximum(hi, [a.max() for a in yuv])
        back = convert_oracle(*(a.reshape(-1, 1, 1).astype(np.uint8) for a in yuv), YUV_BT601, "rgb").reshape(256, 256, 3).astype(np.int64)
        worst = np.maximum(worst, [np.abs(back[..., 0] - R).max(), np.abs(back[..., 1] - G).max(), np.abs(back[..., 2] - B).max()])
    assert lo.tolist() == [16, 16, 16] and hi.tolist() == [235, 240, 240]      # no clip is ever active
    assert worst.tolist() == [2, 1, 2]                                         # an integer fact of the two tables
    for g in range(256):
        assert one(g, g, g)[1:] == (128, 128)
    assert one(255, 0, 0) == (82, 90, 240) and one(0, 255, 0) == (145, 54, 34) and one(0, 0, 255) == (41, 240, 110)
    assert one(0, 0, 0) == (16, 128, 128) and one(255, 255, 255) == (235, 128, 128)
    assert _native.RGB_BT601 == BT601 == RgbMatrix.preset("bt601").as_tuple()


# ----------------------------------------------------------------------------- the rule on values worked by hand
def test_pinned_values_under_a_custom_matrix():
    one20 = 1 << 20
    # Y = R + G, U = 128 - R, V = 128 + B / 2: both clips
    m = (0, one20, one20, 0, -one20, 0, 0, 0, 0, one20 // 2)
    assert one(200, 200, 0, m) == (255, 0, 128)             # 400 -> 255; 128 - 200 = -72 -> 0
    assert one(10, 20, 255, m) == (30, 118, 255)            # 128 + 127.5 = 255.5 -> (255.5 + 0.5) floor = 256 -> 255
    assert one(10, 20, 253, m) == (30, 118, 255)            # 128 + 126.5 + 0.5 = 255
    assert one(10, 20, 252, m) == (30, 118, 254)
    # the floor of a negative sum: s = -(2^19 + 1) + 2^19 = -1, and -1 >> 20 = -1 (not 0, as a division that truncates gives):
    # with an offset of 1 the byte tells the two apart: (-1 + 2^20) >> 20 = 0, truncation of -1 / 2^20 plus 1 would be 1
    assert one(1, 0, 0, (1, -(1 << 19) - 1, 0, 0, 0, 0, 0, 0, 0, 0)) == (0, 128, 128)
    assert one(1, 0, 0, (1, -(1 << 19), 0, 0, 0, 0, 0, 0, 0, 0)) == (1, 128, 128)
    # the rounding is half up: 0.5 -> 1, just below -> 0
    assert one(1, 0, 0, (0, 1 << 19, 0, 0, 0, 0, 0, 0, 0, 0))[0] == 1 and one(1, 0, 0, (0, (1 << 19) - 1, 0, 0, 0, 0, 0, 0, 0, 0))[0] == 0


def test_average_at_an_odd_edge_and_on_constant_blocks():
    # U = 128 + B: nearest takes the top-left pixel, average (sum + 2) >> 2 over the block with the existing pixel repeated
    m = (0, 0, 0, 0, 0, 0, 1 << 20, 0, 0, 0)
    frame = np.zeros((1, 3, 3, 3), np.uint8)
    frame[0, :, :, 0] = [[1, 2, 3], [4, 5, 6], [7, 8, 10]]                     # B of BGR
    _y, u, v = to_yuv_oracle(frame, m, "bgr", "nearest")
    assert u[0].tolist() == [[129, 131], [135, 138]] and np.all(v == 128)
    _y, u, _v = to_yuv_oracle(frame, m, "bgr", "average")
    # (1+2+4+5 + 2) >> 2 = 3;  (3+3+6+6 + 2) >> 2 = 5;  (7+8+7+8 + 2) >> 2 = 8;  (4 * 10 + 2) >> 2 = 10
    assert u[0].tolist() == [[131, 133], [136, 138]]
    # on blocks of four equal pixels the two modes agree, under any matrix: 4 s + 2^21 + 128 2^22 = 4 (s + 2^19 + 128 2^20)
    rng = np.random.default_rng(7)
    small = rng.integers(0, 256, size=(3, 5, 7, 3), dtype=np.uint8)
    blocks = np.repeat(np.repeat(small, 2, axis=1), 2, axis=2)[:, :9, :13]     # odd sizes: the edge repeats the same pixel
    for matrix in (BT601, RgbMatrix.preset("bt709-full").as_tuple(), at_bound()):
        a, b = to_yuv_oracle(blocks, matrix, "bgr", "nearest"), to_yuv_oracle(blocks, matrix, "bgr", "average")
        assert all(np.array_equal(p, q) for p, q in zip(a, b))


def test_oracle_input_formats():
    rng = np.random.default_rng(2)
    bgra = rng.integers(0, 256, size=(2, 5, 7, 4), dtype=np.uint8)
    want = to_yuv_oracle(bgra[..., :3], BT601, "bgr", "average")
    rgba = bgra[..., [2, 1, 0, 3]]
    for frames, fmt in ((bgra, "bgra"), (rgba, "rgba"), (rgba[..., :3], "rgb")):
        assert all(np.array_equal(p, q) for p, q in zip(to_yuv_oracle(frames, BT601, fmt, "average"), want))
    grey = bgra[..., 0]
    want = to_yuv_oracle(np.stack([grey] * 3, axis=-1), BT601, "bgr")
    assert all(np.array_equal(p, q) for p, q in zip(to_yuv_oracle(grey, BT601, "gray"), want))
    assert all(np.array_equal(p, q) for p, q in zip(to_yuv_oracle(grey[..., None], BT601, "bgr"), want))
    assert np.all(want[1] == 128) and np.all(want[2] == 128)


# ----------------------------------------------------------------------------- matrices
def test_presets_and_from_standard():
    # OpenCV's table is the three-decimal constants 0.257, 0.504, 0.098, -0.148, -0.291, 0.439, -0.368, -0.071 times 2^20, each
    # within one unit of the rounded product
    dec = (0.257, 0.504, 0.098, -0.148, -0.291, 0.439, 0.439, -0.368, -0.071)
    diff = np.array(BT601[1:]) - np.array([int(round(c * 2 ** 20)) for c in dec])
    assert np.all(np.abs(diff) <= 1), diff
    for name, kr, kb, full in (("bt709", 0.2126, 0.0722, False), ("bt601-full", 0.299, 0.114, True), ("bt709-full", 0.2126, 0.0722, True)):
        m = RgbMatrix.preset(name)
        assert m == RgbMatrix.from_standard(kr, kb, full) and m.y_offset == (0 if full else 16)
        kg = 1 - kr - kb
        sy, sc = (1.0, 1.0) if full else (219 / 255, 224 / 255)
        exact = (kr * sy, kg * sy, kb * sy, -kr / (2 * (1 - kb)) * sc, -kg / (2 * (1 - kb)) * sc, 0.5 * sc,
                 0.5 * sc, -kg / (2 * (1 - kr)) * sc, -kb / (2 * (1 - kr)) * sc)
        assert m.as_tuple()[1:] == tuple(int(round(c * 2 ** 20)) for c in exact)
    # the exact BT.601 ratios lie within a unit of the third decimal of OpenCV's constants
    diff = np.abs(np.array(RgbMatrix.from_standard(0.299, 0.114).as_tuple()[1:]) - np.array(BT601[1:]))
    assert np.all(diff <= 1049) and np.any(diff > 1), diff
    full = RgbMatrix.preset("bt601-full")
    assert (full.cbu, full.crv) == (1 << 19, 1 << 19) and full.cry + full.cgy + full.cby == 1 << 20
    # grey stays grey under every preset, in both chroma modes, with plain rounding: the chroma rows sum to -1, 0 or 1
    grey = np.repeat(np.repeat(np.arange(256, dtype=np.uint8).reshape(1, 16, 16), 2, axis=1), 2, axis=2)
    for name in PRESETS:
        t = RgbMatrix.preset(name).as_tuple()
        assert abs(sum(t[4:7])) <= 1 and abs(sum(t[7:10])) <= 1
        for chroma in ("nearest", "average"):
            y, u, v = to_yuv_oracle(grey, t, "gray", chroma)
            assert np.all(u == 128) and np.all(v == 128), (name, chroma)
        y, _u, _v = to_yuv_oracle(grey, t, "gray")
        assert (int(y.min()), int(y.max())) == ((0, 255) if name.endswith("-full") else (16, 235))
    with pytest.raises(ValueError):
        RgbMatrix.preset("bt2020")
    with pytest.raises(ValueError):
        RgbMatrix.from_standard(0.7, 0.4)
    with pytest.raises(ValueError):
        RgbMatrix(16.5, *BT601[1:])


def at_bound():
    """A matrix with mixed signs whose three rows all sit AT the coefficient bound: 255 (|a| + |b| + |c|) < 2^28 allows a
    magnitude sum of (2^28 - 1) // 255 = 1052688 (255 * 1052688 = 2^28 - 16).  Around the offsets of 128 every row reaches both
    clips."""
    top = ((1 << 28) - 1) // 255
    half = top // 2                                                        # 526344: a row (half, -half, 0) spans -128.0006..128.0006
    return (128, half, -half, 0, -half, 0, half, half - 1, 1, -half)


def test_coefficient_bound():
    top = ((1 << 28) - 1) // 255
    assert top == 1052688 and 255 * top < 1 << 28 <= 255 * (top + 1)
    for name in PRESETS:
        assert _native.rgb_matrix_in_bound(RgbMatrix.preset(name).as_tuple())
    m = at_bound()
    assert all(sum(abs(c) for c in m[i:i + 3]) == top for i in (1, 4, 7))
    assert _native.rgb_matrix_in_bound(m) and RgbMatrix(*m).as_tuple() == m
    # one past it: any coefficient one further from zero
    for i in range(1, 10):
        bad = list(m)
        bad[i] += 1 if bad[i] >= 0 else -1
        assert not _native.rgb_matrix_in_bound(bad), (i, bad)
        with pytest.raises(ValueError):
            RgbMatrix(*bad)
    # the full-range luma row lies just inside
    assert _native.rgb_matrix_in_bound((0, 1 << 20, 0, 0, 0, 0, 0, 0, 0, 0)) and not _native.rgb_matrix_in_bound((0, top + 1, 0, 0, 0, 0, 0, 0, 0, 0))
    assert not _native.rgb_matrix_in_bound((-1,) + BT601[1:]) and not _native.rgb_matrix_in_bound((256,) + BT601[1:])
    assert not _native.rgb_matrix_in_bound(BT601[:9])
    # under the bound every sum of both modes fits an int32: the extreme inputs of rows at the bound, every sign pattern
    for a in (top, -top):
        for row in ((a, 0, 0), (a // 2, -(a - a // 2), 0), (a // 3, a // 3, a - 2 * (a // 3))):
            for rgb in ((255, 255, 255), (0, 0, 0), (255, 0, 255), (0, 255, 0)):
                s = sum(c * x for c, x in zip(row, rgb))
                for total in (s + (1 << 19) + (255 << 20), 4 * s + (1 << 21) + (128 << 22)):
                    assert -(1 << 31) <= total < (1 << 31)


# ----------------------------------------------------------------------------- layouts of a result
def test_allocated_layouts_against_hand_built_pitches():
    B = 3
    for fmt in _native.YUV_FORMATS:
        st = _native.yuv_planes_alloc(fmt, B, 6, 8, False)                     # even sizes: ffmpeg's stacked frames
        assert isinstance(st, np.ndarray) and st.shape == (B, 9, 8)
        L = _native._yuv_layout(st, fmt)
        base = st.ctypes.data
        assert (L.n_frames, L.height, L.width, L.y, L.y_row_pitch, L.y_frame_pitch) == (B, 6, 8, base, 8, 72)
        if fmt in ("nv12", "nv21"):
            first, second = base + 48, base + 49
            assert (L.c_step, L.c_row_pitch, L.c_frame_pitch) == (2, 8, 72)
        else:
            first, second = base + 48, base + 60
            assert (L.c_step, L.c_row_pitch, L.c_frame_pitch) == (1, 4, 72)
        assert (L.u, L.v) == ((first, second) if fmt in ("nv12", "i420") else (second, first))
        planes = _native.yuv_planes_alloc(fmt, B, 5, 7, False)                 # an odd size: the tuple of planes
        assert isinstance(planes, tuple) and planes[0].shape == (B, 5, 7)
        assert [p.shape for p in planes[1:]] == ([(B, 3, 4, 2)] if fmt in ("nv12", "nv21") else [(B, 3, 4)] * 2)
        L = _native._yuv_layout(planes, fmt)
        assert (L.height, L.width, L.y, L.y_row_pitch, L.y_frame_pitch) == (5, 7, planes[0].ctypes.data, 7, 35)
        if fmt in ("nv12", "nv21"):
            first, second = planes[1].ctypes.data, planes[1].ctypes.data + 1
            assert (L.c_step, L.c_row_pitch, L.c_frame_pitch) == (2, 8, 24)
        else:
            first, second = planes[1].ctypes.data, planes[2].ctypes.data
            assert (L.c_step, L.c_row_pitch, L.c_frame_pitch) == (1, 4, 12)
        assert (L.u, L.v) == ((first, second) if fmt in ("nv12", "i420") else (second, first))
    assert _native.yuv_planes_alloc("i420", 2, 6, 7, False)[1].shape == (2, 3, 4)      # one odd size is enough for the tuple


def test_python_arguments_are_checked_before_the_library_is_needed(monkeypatch):
    def no_library():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_native, "load", no_library)
    bgr, grey = np.zeros((2, 4, 6, 3), np.uint8), np.zeros((2, 4, 6), np.uint8)
    for kw, match in ((dict(in_format="yuv"), "in_format"), (dict(in_format="bgra"), "byte"), (dict(in_format="gray"), "byte"),
                      (dict(pixel_format="yuyv"), "pixel_format"), (dict(chroma="bilinear"), "chroma"), (dict(matrix="bt2020"), "unknown matrix"),
                      (dict(matrix=BT601[:9]), "argument"), (dict(out=np.zeros((2, 6, 8), np.uint8)), "out holds"),
                      (dict(out=np.zeros((3, 6, 6), np.uint8)), "out holds"), (dict(out=(grey, np.zeros((2, 2, 3), np.uint8))), "uv must be")):
        with pytest.raises((ValueError, TypeError), match=match):
            imaging.frames_to_yuv(bgr, **kw)
    ro = np.zeros((2, 6, 6), np.uint8)
    ro.setflags(write=False)
    with pytest.raises(ValueError, match="writeable"):
        imaging.frames_to_yuv(bgr, out=ro)
    with pytest.raises(ValueError, match="uint8"):
        imaging.frames_to_yuv(bgr.astype(np.float32))
    with pytest.raises(ValueError, match="ten 32-bit"):
        _native.frames_to_yuv(bgr, matrix=(1 << 31,) + BT601[1:])
    with pytest.raises(AssertionError, match="the library was asked for"):     # valid arguments reach the library
        imaging.frames_to_yuv(grey, in_format="bgr")
    lens = imaging.Lens(100.0, 100.0, 3.0, 2.0)
    with pytest.raises(ValueError, match="out_pixel_format"):
        imaging.undistort_frames(bgr, lens, out_pixel_format="yuyv")
    with pytest.raises(ValueError, match="out holds"):
        imaging.undistort_frames(bgr, lens, out_pixel_format="nv12", out=np.zeros((2, 9, 6), np.uint8))
    assert imaging._matrix("BT601", imaging.RgbMatrix) == BT601 and imaging._matrix(list(BT601), imaging.RgbMatrix) == BT601


# ----------------------------------------------------------------------------- OpenCV, where it is installed
def test_oracle_equals_opencv():
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(4)
    H, W = 48, 62
    bgr = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    y, u, v = to_yuv_oracle(bgr[None], BT601, "bgr", "nearest")
    want = np.concatenate([y[0].ravel(), u[0].ravel(), v[0].ravel()]).reshape(H + H // 2, W)
    assert np.array_equal(cv2.cvtColor(bgr, cv2.COLOR_BGR2YUV_I420), want)
    y, u, v = to_yuv_oracle(bgr[None, ..., ::-1], BT601, "rgb", "nearest")
    assert np.array_equal(cv2.cvtColor(np.ascontiguousarray(bgr[..., ::-1]), cv2.COLOR_RGB2YUV_I420),
                          np.concatenate([y[0].ravel(), u[0].ravel(), v[0].ravel()]).reshape(H + H // 2, W))
