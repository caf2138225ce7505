"""Host tests of the conversion of decoder frames (sba_convert_frames, include/sba_hip.h): the numpy oracle of its rule, the
integer matrices of ``imaging.YuvMatrix`` and how ``_native._yuv_layout`` reads plane tuples and stacked arrays.  No GPU.

``convert_oracle`` follows the header's rule literally, in int64; tests/test_gpu_convert.py compares the kernel with it bit for
bit.
"""
import numpy as np
import pytest

from lasercalib_amd import _native, imaging
from lasercalib_amd.imaging import YuvMatrix

BT601 = (16, 1220542, 1673527, -409993, -852492, 2116026)      # OpenCV's table, as the header states it
FORMATS = ("bgr", "rgb", "bgra", "rgba", "b", "g", "r")


def convert_oracle(y, u, v, matrix=BT601, out_format="bgr"):
    """The rule of include/sba_hip.h in int64.  y (B, H, W), u and v (B, ceil(H / 2), ceil(W / 2)): plain uint8 planes, whatever
    the layout they came from.  -> (B, H, W, 3 | 4) uint8, or (B, H, W) for a single plane."""
    y_offset, cy, cvr, cug, cvg, cub = (int(c) for c in matrix)
    y, u, v = (np.asarray(a).astype(np.int64) for a in (y, u, v))
    B, H, W = y.shape
    assert u.shape == v.shape == (B, (H + 1) // 2, (W + 1) // 2)
    yy, xx = np.arange(H) >> 1, np.arange(W) >> 1
    U, V = u[:, yy][:, :, xx] - 128, v[:, yy][:, :, xx] - 128            # nearest chroma
    l = np.maximum(y - y_offset, 0) * cy
    half = 1 << 19
    r = np.clip((l + cvr * V + half) >> 20, 0, 255)                      # >> on int64 is the arithmetic shift: floor
    g = np.clip((l + cug * U + cvg * V + half) >> 20, 0, 255)
    b = np.clip((l + cub * U + half) >> 20, 0, 255)
    a = np.full_like(r, 255)
    planes = {"bgr": (b, g, r), "rgb": (r, g, b), "bgra": (b, g, r, a), "rgba": (r, g, b, a), "b": (b,), "g": (g,), "r": (r,)}[out_format]
    out = np.stack(planes, axis=-1).astype(np.uint8)
    return out[..., 0] if len(planes) == 1 else out


def one(Y, U, V, matrix=BT601):
    px = convert_oracle(np.full((1, 1, 1), Y, np.uint8), np.full((1, 1, 1), U, np.uint8), np.full((1, 1, 1), V, np.uint8), matrix, "rgb")
    return tuple(int(c) for c in px[0, 0, 0])


# ----------------------------------------------------------------------------- the rule on values worked by hand
def test_pinned_values_under_the_default_table():
    """(Y, U, V) -> (R, G, B), each worked from the rule with cy = 1220542, cvr = 1673527, cug = -409993, cvg = -852492,
    cub = 2116026, 2^19 = 524288, 2^20 = 1048576."""
    # black and white of the limited range: l = 0 and l = 219 cy = 267298698; u = v = 0
    #   (0 + 524288) >> 20 = 0;   (267298698 + 524288) >> 20 = floor(255.417) = 255
    assert one(16, 128, 128) == (0, 0, 0)
    assert one(235, 128, 128) == (255, 255, 255)
    # BT.601 red (81, 90, 240): l = 65 cy = 79335230, u = -38, v = 112
    #   R: 79335230 + 187435024 + 524288 = 267294542 -> floor(254.91) = 254
    #   G: 79335230 + 15579734 - 95479104 + 524288 = -39852 -> floor(-0.04) = -1 -> 0   (the floor of a negative sum)
    #   B: 79335230 - 80408988 + 524288 = -549470 -> floor(-0.52) = -1 -> 0
    assert one(81, 90, 240) == (254, 0, 0)
    # BT.601 green (145, 54, 34): l = 129 cy = 157449918, u = -74, v = -94
    #   R: 157449918 - 157311538 + 524288 = 662668 -> 0
    #   G: 157449918 + 30339482 + 80134248 + 524288 = 268447936 -> floor(256.01) = 256 -> 255   (the clip)
    #   B: 157449918 - 156585924 + 524288 = 1388282 -> floor(1.32) = 1
    assert one(145, 54, 34) == (0, 255, 1)
    # BT.601 blue (41, 240, 110): l = 25 cy = 30513550, u = 112, v = -18
    #   R: 30513550 - 30123486 + 524288 = 914352 -> 0
    #   G: 30513550 - 45919216 + 15344856 + 524288 = 463478 -> 0
    #   B: 30513550 + 236994912 + 524288 = 268032750 -> floor(255.62) = 255
    assert one(41, 240, 110) == (0, 0, 255)
    # below the offset the luma is clamped, not negative: Y = 0 is Y = 16
    assert one(0, 128, 128) == (0, 0, 0) and one(0, 90, 240) == one(16, 90, 240)


def test_oracle_formats_and_nearest_chroma():
    rng = np.random.default_rng(1)
    y = rng.integers(0, 256, size=(2, 5, 7), dtype=np.uint8)
    u, v = (rng.integers(0, 256, size=(2, 3, 4), dtype=np.uint8) for _ in range(2))
    rgb = convert_oracle(y, u, v, BT601, "rgb")
    assert rgb.shape == (2, 5, 7, 3)
    for f, yy, xx in ((0, 0, 0), (1, 4, 6), (0, 3, 5), (1, 2, 1)):       # odd x odd: the last row and column have their own sample
        assert tuple(rgb[f, yy, xx]) == one(y[f, yy, xx], u[f, yy >> 1, xx >> 1], v[f, yy >> 1, xx >> 1])
    bgra = convert_oracle(y, u, v, BT601, "bgra")
    assert np.array_equal(bgra[..., :3], rgb[..., ::-1]) and np.all(bgra[..., 3] == 255)
    assert np.array_equal(convert_oracle(y, u, v, BT601, "rgba")[..., :3], rgb)
    assert np.array_equal(convert_oracle(y, u, v, BT601, "bgr"), rgb[..., ::-1])
    for k, name in enumerate("rgb"):
        assert np.array_equal(convert_oracle(y, u, v, BT601, name), rgb[..., k])


# ----------------------------------------------------------------------------- matrices
def test_presets_and_from_standard():
    assert YuvMatrix.preset("bt601").as_tuple() == BT601 == _native.YUV_BT601
    # the table is the three-decimal constants times 2^20, rounded
    assert BT601[1:] == tuple(int(round(c * 2 ** 20)) for c in (1.164, 1.596, -0.391, -0.813, 2.018))
    # from_standard uses the exact ratios: 1.164383, 1.596027, -0.391762, -0.812968, 2.017232.  OpenCV's constants are these
    # given to three decimals -- rounded (1.164, 1.596, -0.813) or off by the last digit (-0.391 for -0.3918, 2.018 for
    # 2.0172) -- so each lies within one unit of the third decimal of its exact value: the integers differ by less than
    # 0.001 * 2^20 = 1048.6, plus half a unit for each of the two roundings to an integer
    m = YuvMatrix.from_standard(0.299, 0.114, False)
    assert m.y_offset == 16
    diff = np.abs(np.array(m.as_tuple()[1:]) - np.array(BT601[1:]))
    assert np.all(diff <= 1049) and np.any(diff > 1), diff
    # where OpenCV's constant IS the rounded one, half of that
    assert np.all(diff[[0, 1, 3]] <= 525), diff
    exact = (255 / 219, 2 * 0.701 * 255 / 224, -2 * 0.114 * 0.886 / 0.587 * 255 / 224, -2 * 0.299 * 0.701 / 0.587 * 255 / 224, 2 * 0.886 * 255 / 224)
    assert m.as_tuple()[1:] == tuple(int(round(c * 2 ** 20)) for c in exact)
    full = YuvMatrix.preset("bt601-full")
    assert full.y_offset == 0 and full.cy == 1 << 20 and full.cvr == int(round(1.402 * 2 ** 20)) and full.cub == int(round(1.772 * 2 ** 20))
    hd = YuvMatrix.preset("bt709")
    assert hd == YuvMatrix.from_standard(0.2126, 0.0722) and hd.cvr == int(round(2 * (1 - 0.2126) * 255 / 224 * 2 ** 20))
    assert YuvMatrix.preset("bt709-full").cub == int(round(2 * (1 - 0.0722) * 2 ** 20))
    # grey stays grey under every preset: the chroma terms vanish at U = V = 128
    for name in ("bt601", "bt709", "bt601-full", "bt709-full"):
        t = YuvMatrix.preset(name).as_tuple()
        px = one(180, 128, 128, t)
        assert px[0] == px[1] == px[2]
    assert one(255, 128, 128, full.as_tuple()) == (255, 255, 255) and one(0, 128, 128, full.as_tuple()) == (0, 0, 0)
    with pytest.raises(ValueError):
        YuvMatrix.preset("bt2020")
    with pytest.raises(ValueError):
        YuvMatrix.from_standard(0.7, 0.4)


def at_bound():
    """A matrix with mixed signs whose three rows all sit AT the coefficient bound: with room = 2^31 - 1 - 2^19 for
    255 |cy| + 128 (|a| + |b|), each row's chroma magnitudes add up to floor((room - 255 |cy|) / 128)."""
    room = (1 << 31) - 1 - (1 << 19)
    cy = -4000037
    rest = (room - 255 * abs(cy)) // 128
    cvg = -2500003
    return (200, cy, -rest, rest - abs(cvg), cvg, rest)


def test_coefficient_bound():
    for name in ("bt601", "bt709", "bt601-full", "bt709-full"):
        assert _native.yuv_matrix_in_bound(YuvMatrix.preset(name).as_tuple())
    m = at_bound()
    assert m[3] > 0 and _native.yuv_matrix_in_bound(m) and YuvMatrix(*m).as_tuple() == m
    # one past it: any coefficient one further from zero
    for i in range(1, 6):
        bad = list(m)
        bad[i] += 1 if bad[i] > 0 else -1
        assert not _native.yuv_matrix_in_bound(bad), (i, bad)
        with pytest.raises(ValueError):
            YuvMatrix(*bad)
    # 255 * 8421504 = 2^31 - 128: with the 2^19 of the rounding that is past the bound, 2^23 is not
    assert not _native.yuv_matrix_in_bound((16, 8421504, 0, 0, 0, 0)) and _native.yuv_matrix_in_bound((16, 1 << 23, 0, 0, 0, 0))
    assert not _native.yuv_matrix_in_bound((-1,) + BT601[1:]) and not _native.yuv_matrix_in_bound((256,) + BT601[1:])
    # under the bound every intermediate of the rule fits an int32: the extreme inputs of the matrix at the bound
    y_offset, cy, cvr, cug, cvg, cub = m
    for Y in (0, 255):
        for U in (0, 255):
            for V in (0, 255):
                l = max(Y - y_offset, 0) * cy
                for s in (l + cvr * (V - 128), l + cug * (U - 128) + cvg * (V - 128), l + cub * (U - 128)):
                    assert -(1 << 31) <= s + (1 << 19) < (1 << 31)


# ----------------------------------------------------------------------------- layouts
def strided(shape, strides, base, rng, slack=64):
    """A uint8 buffer and a view of `shape` with the byte `strides` starting `base` bytes in, filled with random bytes."""
    need = base + sum((n - 1) * s for n, s in zip(shape, strides) if n > 0) + 1
    buf = rng.integers(0, 256, size=need + slack, dtype=np.uint8)
    return buf, np.lib.stride_tricks.as_strided(buf[base:], shape=shape, strides=strides)


def test_layout_of_plane_tuples_against_hand_built_pitches():
    rng = np.random.default_rng(2)
    B, H, W = 3, 5, 7                                                     # odd x odd: 3 x 4 chroma samples
    ybuf, y = strided((B, H, W), (5 * 11 + 3, 11, 1), 5, rng)
    cbuf, uv = strided((B, 3, 4, 2), (3 * 13 + 7, 13, 2, 1), 1, rng)
    for fmt in ("nv12", "nv21"):
        L = _native._yuv_layout((y, uv), fmt)
        assert (L.tensor, L.n_frames, L.height, L.width) == (False, B, H, W)
        assert (L.y, L.y_row_pitch, L.y_frame_pitch) == (ybuf.ctypes.data + 5, 11, 58)
        assert (L.c_row_pitch, L.c_frame_pitch, L.c_step) == (13, 46, 2)
        first, second = cbuf.ctypes.data + 1, cbuf.ctypes.data + 2
        assert (L.u, L.v) == ((first, second) if fmt == "nv12" else (second, first))
    ubuf, u = strided((B, 3, 4), (40, 9, 1), 15, rng)
    vbuf, v = strided((B, 3, 4), (40, 9, 1), 0, rng)
    L = _native._yuv_layout((y, u, v), "i420")
    assert (L.u, L.v, L.c_row_pitch, L.c_frame_pitch, L.c_step) == (ubuf.ctypes.data + 15, vbuf.ctypes.data, 9, 40, 1)
    L = _native._yuv_layout((y, u, v), "yv12")                            # the format's order: the second plane is V
    assert (L.u, L.v) == (vbuf.ctypes.data, ubuf.ctypes.data + 15)
    # the two halves of an interleaved plane are planar planes with a step of 2
    L = _native._yuv_layout((y, uv[..., 0], uv[..., 1]), "i420")
    assert (L.u, L.v, L.c_row_pitch, L.c_frame_pitch, L.c_step) == (cbuf.ctypes.data + 1, cbuf.ctypes.data + 2, 13, 46, 2)
    # a single frame, a single row, a single column: strides of axes of length 1 say nothing
    L = _native._yuv_layout((np.zeros((1, 1, 1), np.uint8), np.zeros((1, 1, 1, 2), np.uint8)), "nv12")
    assert (L.y_row_pitch, L.y_frame_pitch, L.c_row_pitch, L.c_frame_pitch, L.c_step) == (1, 1, 2, 2, 2)
    L = _native._yuv_layout((np.zeros((0, 4, 6), np.uint8), np.zeros((0, 2, 3), np.uint8), np.zeros((0, 2, 3), np.uint8)), "i420")
    assert (L.n_frames, L.height, L.width, L.c_step) == (0, 4, 6, 1)
    # what is refused
    with pytest.raises(ValueError, match="uv must be"):
        _native._yuv_layout((y, uv[:, :2]), "nv12")
    with pytest.raises(ValueError, match="same strides"):
        _native._yuv_layout((y, u, strided((B, 3, 4), (44, 9, 1), 0, rng)[1]), "i420")
    with pytest.raises(ValueError, match="apart"):
        _native._yuv_layout((y, strided((B, 3, 4), (60, 15, 3), 0, rng)[1], strided((B, 3, 4), (60, 15, 3), 0, rng)[1]), "i420")
    with pytest.raises(ValueError, match="apart"):
        _native._yuv_layout((y[:, :, ::2], uv), "nv12")
    with pytest.raises(ValueError, match="ascending"):
        _native._yuv_layout((y[:, ::-1], uv), "nv12")
    with pytest.raises(ValueError, match="uint8"):
        _native._yuv_layout((y.astype(np.int16), uv), "nv12")
    with pytest.raises(ValueError, match="tuple of"):
        _native._yuv_layout((y, uv), "i420")
    with pytest.raises(ValueError, match="pixel_format"):
        _native._yuv_layout((y, uv), "p010")


def test_layout_of_stacked_frames_against_hand_built_pitches():
    rng = np.random.default_rng(3)
    # nv12 as ffmpeg's pipe delivers it, with padded rows and frames and an odd height: H = 5 -> 5 + 3 rows
    buf, st = strided((2, 8, 6), (8 * 10 + 4, 10, 1), 3, rng)
    L = _native._yuv_layout(st, "nv12")
    base = buf.ctypes.data + 3
    assert (L.n_frames, L.height, L.width) == (2, 5, 6)
    assert (L.y, L.u, L.v) == (base, base + 5 * 10, base + 5 * 10 + 1)
    assert (L.y_row_pitch, L.y_frame_pitch, L.c_row_pitch, L.c_frame_pitch, L.c_step) == (10, 84, 10, 84, 2)
    L = _native._yuv_layout(st, "nv21")
    assert (L.u, L.v) == (base + 51, base + 50)
    # yuv420p: packed rows, even sizes; the frame pitch may be padded
    buf, st = strided((2, 6, 8), (6 * 8 + 16, 8, 1), 0, rng)
    L = _native._yuv_layout(st, "i420")
    base = buf.ctypes.data
    assert (L.height, L.width) == (4, 8)
    assert (L.y, L.u, L.v) == (base, base + 32, base + 32 + 8)
    assert (L.y_row_pitch, L.y_frame_pitch, L.c_row_pitch, L.c_frame_pitch, L.c_step) == (8, 64, 4, 64, 1)
    L = _native._yuv_layout(st, "yv12")
    assert (L.u, L.v) == (base + 40, base + 32)
    # stacked and tuple forms describe the same bytes
    y, u, v = st[:, :4], st[:, 4:5].reshape(2, 2, 4), st[:, 5:6].reshape(2, 2, 4)
    assert np.shares_memory(u, st)
    T = _native._yuv_layout((y, u, v), "i420")
    for k in ("y", "u", "v", "y_row_pitch", "y_frame_pitch", "c_row_pitch", "c_frame_pitch", "c_step", "height", "width"):
        assert getattr(T, k) == getattr(_native._yuv_layout(st, "i420"), k), k
    # errors: a stacked I420 frame needs an even width and height, and says so
    with pytest.raises(ValueError, match="even width and height"):
        _native._yuv_layout(np.zeros((1, 8, 6), np.uint8), "i420")       # 8 rows = 5 + 3: H = 5
    with pytest.raises(ValueError, match="even width and height"):
        _native._yuv_layout(np.zeros((1, 6, 7), np.uint8), "yv12")
    with pytest.raises(ValueError, match="even width"):
        _native._yuv_layout(np.zeros((1, 6, 7), np.uint8), "nv12")
    with pytest.raises(ValueError, match="fit no H"):
        _native._yuv_layout(np.zeros((1, 7, 6), np.uint8), "nv12")
    with pytest.raises(ValueError, match="packed rows"):
        _native._yuv_layout(strided((2, 6, 8), (60, 10, 1), 0, rng)[1], "i420")
    with pytest.raises(ValueError, match="stacked"):
        _native._yuv_layout(np.zeros((6, 8), np.uint8), "nv12")


def test_python_arguments_are_checked_before_the_library_is_needed():
    with pytest.raises(ValueError, match="channel"):
        list(imaging.planes_in_chunks(np.zeros((1, 3, 2), np.uint8), "nv12", "bt601", 3, 0, 0))
    with pytest.raises(ValueError):
        imaging._matrix((16, 8421504, 0, 0, 0, 0), imaging.YuvMatrix)
    assert imaging._matrix("BT601", imaging.YuvMatrix) == BT601 and imaging._matrix(list(BT601), imaging.YuvMatrix) == BT601


# ----------------------------------------------------------------------------- OpenCV, where it is installed
def test_oracle_equals_opencv():
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(4)
    H, W = 48, 62
    st = rng.integers(0, 256, size=(H + H // 2, W), dtype=np.uint8)
    y = st[None, :H]
    uv = st[H:].reshape(1, H // 2, W // 2, 2)
    assert np.array_equal(cv2.cvtColor(st, cv2.COLOR_YUV2BGR_NV12), convert_oracle(y, uv[..., 0], uv[..., 1])[0])
    assert np.array_equal(cv2.cvtColor(st, cv2.COLOR_YUV2RGB_NV21), convert_oracle(y, uv[..., 1], uv[..., 0], out_format="rgb")[0])
    u, v = st[H:H + H // 4].reshape(1, H // 2, W // 2), st[H + H // 4:].reshape(1, H // 2, W // 2)
    assert np.array_equal(cv2.cvtColor(st, cv2.COLOR_YUV2BGR_I420), convert_oracle(y, u, v)[0])
