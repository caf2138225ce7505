"""Host tests of the previews (sba_resize_frames, include/sba_hip.h): the numpy oracle of its rule, the geometry of
``imaging.mosaic`` and how ``_native.resize_frames`` reads its arguments.  No GPU.

``resize_oracle`` follows the header's rule literally: int64 sums, an ``np.float32`` scale and product, ``np.rint``, and the
``(s + 2) >> 2`` case; tests/test_gpu_resize.py compares the kernel with it bit for bit.
"""
import ctypes

import numpy as np
import pytest

from lasercalib_amd import _native, imaging

GRAY_BGR = (3735, 19235, 9798)                                # OpenCV's weights of B, G, R, as the header states them


def resize_oracle(frames, fx, fy, gray=None):
    """The rule of include/sba_hip.h.  frames (B, H, W, C) or (B, H, W) uint8; ``gray``: None, or the three integer weights of
    the channels 0, 1, 2.  -> (B, H // fy, W // fx, C), (B, H // fy, W // fx) for 3-D frames and with gray."""
    f = np.asarray(frames)
    flat = f.ndim == 3
    v = (f[..., None] if flat else f).astype(np.int64)
    if gray is not None:
        w0, w1, w2 = (int(w) for w in gray)
        assert min(w0, w1, w2) >= 0 and w0 + w1 + w2 == 1 << 15 and v.shape[3] >= 3
        v = ((v[..., 0] * w0 + v[..., 1] * w1 + v[..., 2] * w2 + (1 << 14)) >> 15)[..., None]      # step 1, per SOURCE pixel
    B, H, W, C = v.shape
    oh, ow = H // fy, W // fx
    s = v[:, :oh * fy, :ow * fx].reshape(B, oh, fy, ow, fx, C).sum(axis=(2, 4))                   # the remainder is not read
    if fx == 2 and fy == 2:
        out = (s + 2) >> 2
    else:
        scale = np.float32(1.0) / np.float32(fx * fy)                                              # ONE float32 division
        prod = s.astype(np.float32) * scale                                                        # ONE float32 multiply
        assert prod.dtype == np.float32
        out = np.rint(prod).astype(np.int64)                                                       # to nearest, ties to even
    assert out.min(initial=0) >= 0 and out.max(initial=0) <= 255
    out = out.astype(np.uint8)
    return out[..., 0] if flat or gray is not None else out


def block(values, fx, fy):
    """The one output value of a single fx x fy block of one channel holding ``values`` (row-major, padded with zeros)."""
    a = np.zeros(fx * fy, np.uint8)
    a[:len(values)] = values
    return int(resize_oracle(a.reshape(1, fy, fx), fx, fy)[0, 0, 0])


def gray_of(*px):
    return int(resize_oracle(np.array(px, np.uint8).reshape(1, 1, 1, len(px)), 1, 1, GRAY_BGR)[0, 0, 0])


# ----------------------------------------------------------------------------- the rule on values worked by hand
def test_pinned_block_values():
    # 2 x 2, its own rule: {0, 0, 1, 1}: s = 2, (2 + 2) >> 2 = 1   (half up; ties-to-even of 0.5 would give 0)
    assert block([0, 0, 1, 1], 2, 2) == 1
    assert block([1, 0, 0, 0], 2, 2) == 0 and block([1, 1, 1, 0], 2, 2) == 1 and block([255] * 4, 2, 2) == 255
    # 4 x 4, scale = 1/16 exactly: s = 8 -> 0.5 -> 0 (tie to even), s = 24 -> 1.5 -> 2, s = 40 -> 2.5 -> 2 (tie to even)
    assert block([8], 4, 4) == 0 and block([24], 4, 4) == 2 and block([40], 4, 4) == 2
    assert block([9], 4, 4) == 1 and block([255] * 16, 4, 4) == 255
    # 2 x 4 (fx = 2, fy = 4), scale = 1/8 exactly: s = 4 -> 0.5 -> 0, s = 12 -> 1.5 -> 2
    assert block([4], 2, 4) == 0 and block([12], 2, 4) == 2
    # 3 x 2, area 6: fl32(1/6) = 0x3e2aaaab = 11184811 * 2^-26 (above 1/6 by 2^-26 / 3).
    #   s = 3: 3 * 11184811 = 33554433 = 2^25 + 1, which needs 26 bits; to 24 bits it is 2^25, so the product is
    #   2^25 * 2^-26 = 0.5 exactly (0x3f000000), and rint(0.5) = 0: the float32 multiply rounds the excess of the scale away.
    #   s = 9: 100663299 -> 1.5 (0x3fc00000) -> 2;   s = 15: -> 2.5 (0x40200000) -> 2
    scale = np.float32(1.0) / np.float32(6)
    assert scale.view(np.uint32) == 0x3E2AAAAB
    assert (np.float32(3) * scale).view(np.uint32) == 0x3F000000
    assert block([3], 3, 2) == 0 and block([9], 3, 2) == 2 and block([15], 3, 2) == 2 and block([4], 3, 2) == 1
    # 1 x 1 copies
    assert block([0], 1, 1) == 0 and block([137], 1, 1) == 137 and block([255], 1, 1) == 255


def test_pinned_gray_values():
    # white: 255 * 32768 + 16384 = 8372224, >> 15 = 255 (255.5 floored): no clip is needed
    assert gray_of(255, 255, 255) == 255 and gray_of(0, 0, 0) == 0
    # pure B: 255 * 3735 + 16384 = 968809 -> 29.57 -> 29;  pure G: 255 * 19235 + 16384 = 4921309 -> 150.19 -> 150
    # pure R: 255 * 9798 + 16384 = 2514874 -> 76.75 -> 76
    assert gray_of(255, 0, 0) == 29 and gray_of(0, 255, 0) == 150 and gray_of(0, 0, 255) == 76
    # rounding is to nearest: (1, 1, 1) -> 32768 + 16384 >> 15 = 1;  B = 4: 14940 + 16384 = 31324 -> 0;  B = 5: 35059 -> 1
    assert gray_of(1, 1, 1) == 1 and gray_of(4, 0, 0) == 0 and gray_of(5, 0, 0) == 1
    # a fourth channel is ignored
    assert gray_of(10, 200, 30, 0) == gray_of(10, 200, 30, 255) == gray_of(10, 200, 30)
    assert GRAY_BGR == _native.GRAY_BGR and sum(GRAY_BGR) == 1 << _native.GRAY_SHIFT


def test_gray_comes_before_the_average():
    """Grey is rounded per source pixel and the rounded values are averaged: not the grey of the averaged colour."""
    px = np.zeros((1, 2, 2, 3), np.uint8)
    px[0, :, :, 0] = 4                                        # each pixel: grey 0 (31324 >> 15); the mean colour (4, 0, 0) as well
    px[0, 0, 0] = (5, 0, 0)                                   # grey 1
    assert int(resize_oracle(px, 2, 2, GRAY_BGR)[0, 0, 0]) == 0          # s = 1: (1 + 2) >> 2 = 0
    px[0, :, :, 0] = 5                                        # four times grey 1: s = 4 -> 1
    assert int(resize_oracle(px, 2, 2, GRAY_BGR)[0, 0, 0]) == 1


@pytest.mark.parametrize("fx,fy", [(4, 1), (1, 4), (4, 2), (2, 4), (4, 4), (8, 8), (16, 4), (16, 16)])
def test_power_of_two_areas_are_exact_division_with_ties_to_even(fx, fy):
    """Areas 4, 8, 16, 64 and 256, every sum there is.  (2 x 2 has its own rule, half up: test_pinned_block_values.)"""
    area = fx * fy
    s = np.arange(255 * area + 1, dtype=np.int64)
    got = np.rint(s.astype(np.float32) * (np.float32(1.0) / np.float32(area))).astype(np.int64)
    q, r = np.divmod(s, area)
    want = q + ((2 * r > area) | ((2 * r == area) & (q % 2 == 1)))
    assert np.array_equal(got, want)


def test_every_sum_is_exact_in_float32_and_stays_a_byte():
    for area in (6, 35, 255, 256, 15, 3):
        s = np.arange(255 * area + 1, dtype=np.int64)
        assert np.array_equal(s.astype(np.float32).astype(np.int64), s)
        out = np.rint(s.astype(np.float32) * (np.float32(1.0) / np.float32(area)))
        assert out.max() == 255 and out.min() == 0
        assert np.all(np.abs(out - s / area) <= 0.5 + 1e-4)


def test_oracle_shapes_and_unread_remainder():
    rng = np.random.default_rng(3)
    f = rng.integers(0, 256, size=(2, 11, 14, 3), dtype=np.uint8)
    out = resize_oracle(f, 4, 3)
    assert out.shape == (2, 3, 3, 3)
    g = f.copy()
    g[:, 9:] = 255
    g[:, :, 12:] = 255
    assert np.array_equal(resize_oracle(g, 4, 3), out)
    assert resize_oracle(f[..., 0], 4, 3).shape == (2, 3, 3) and np.array_equal(resize_oracle(f[..., 0], 4, 3), out[..., 0])
    assert resize_oracle(f, 1, 1, GRAY_BGR).shape == (2, 11, 14)
    assert np.array_equal(resize_oracle(f, 1, 1), f)
    # a block by hand: channel 1 of output pixel (1, 2) of frame 1
    blk = f[1, 3:6, 8:12, 1].astype(np.int64)
    assert out[1, 1, 2, 1] == int(np.rint(np.float32(blk.sum()) * (np.float32(1) / np.float32(12))))


# ----------------------------------------------------------------------------- imaging: factors and weights
def test_factor_and_weights_of_the_public_call():
    assert imaging._factor(4) == (4, 4) and imaging._factor((3, 2)) == (3, 2) and imaging._factor(np.int64(16)) == (16, 16)
    for bad in (0, 17, (4, 0), (1, 2, 3), 2.5, "4", None):
        with pytest.raises(ValueError):
            imaging._factor(bad)
    assert imaging._gray_weights(False, "bgr") is None and imaging._gray_weights(None, "rgb") is None
    assert imaging._gray_weights(np.bool_(True), "bgr") == GRAY_BGR and imaging._gray_weights(np.bool_(False), "bgr") is None
    assert imaging._gray_weights(True, "bgr") == GRAY_BGR and imaging._gray_weights(True, "rgb") == GRAY_BGR[::-1]
    assert imaging._gray_weights((32768, 0, 0), "bgr") == (32768, 0, 0)
    for bad in ((1, 2, 3), (-1, 32769, 0), (16384, 16384), (0.5, 0.25, 0.25), "bgr"):
        with pytest.raises(ValueError):
            imaging._gray_weights(bad, "bgr")
    with pytest.raises(ValueError):
        imaging._gray_weights(True, "gbr")


# ----------------------------------------------------------------------------- mosaic, with the oracle in the kernel's place
@pytest.fixture
def oracle_native(monkeypatch):
    calls = []

    def fake(frames, fx, fy, gray_w=None, out=None, out_on_device=None, chunk_frames=0, device=0):
        calls.append((np.asarray(frames).shape, fx, fy, gray_w))
        res = resize_oracle(frames, fx, fy, gray_w)
        if out is None:
            return res
        assert tuple(out.shape) == res.shape
        out[...] = res
        return out

    monkeypatch.setattr(_native, "resize_frames", fake)
    return calls


def cameras(sizes, n_frames=2, channels=3, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(1, 256, size=(n_frames, h, w) + ((channels,) if channels else ()), dtype=np.uint8) for h, w in sizes]


def test_mosaic_geometry_gap_fill_and_unequal_sizes(oracle_native):
    sizes = [(16, 24), (12, 20), (16, 24)]
    cams = cameras(sizes)
    canvas, origins = imaging.mosaic(cams, 4, gap=2, fill=77)
    # previews 4 x 6, 3 x 5, 4 x 6; tiles 4 x 6; ceil(sqrt(3)) = 2 columns, 2 rows
    assert canvas.shape == (2, 4 + 2 + 4, 6 + 2 + 6, 3) and canvas.dtype == np.uint8
    assert origins.tolist() == [[0, 0], [8, 0], [0, 6]]
    want = np.full_like(canvas, 77)
    for cam, (x, y) in zip(cams, origins):
        p = resize_oracle(cam, 4, 4)
        want[:, y:y + p.shape[1], x:x + p.shape[2]] = p
    assert np.array_equal(canvas, want)
    assert np.all(canvas[:, 4:6] == 77) and np.all(canvas[:, :, 6:8] == 77)           # the gaps
    assert np.all(canvas[:, 3, 8:14] == 77) and np.all(canvas[:, 0:4, 13] == 77)      # the part of tile 1 its preview leaves
    assert np.all(canvas[:, 6:, 8:] == 77)                                            # the tile no camera has
    assert len(oracle_native) == 3                            # one call per camera
    # a click maps back: canvas pixel (9, 2) lies in camera 1 at preview (1, 2), source block starting at (4, 8)
    x, y = origins[1]
    assert np.array_equal(canvas[0, 2, 9], resize_oracle(cams[1][:1, 8:12, 4:8], 4, 4)[0, 0, 0])


def test_mosaic_columns_factor_pair_and_gray(oracle_native):
    cams = cameras([(9, 12), (9, 12), (6, 8), (9, 10), (9, 12)], n_frames=1)
    canvas, origins = imaging.mosaic(cams, (2, 3), columns=3, gray=True)
    assert canvas.shape == (1, 3 + 3, 6 * 3) and origins.tolist() == [[0, 0], [6, 0], [12, 0], [0, 3], [6, 3]]
    assert all(c[1:] == (2, 3, GRAY_BGR) for c in oracle_native)
    for cam, (x, y) in zip(cams, origins):
        p = resize_oracle(cam, 2, 3, GRAY_BGR)
        assert np.array_equal(canvas[:, y:y + p.shape[1], x:x + p.shape[2]], p)
    assert np.all(canvas[:, 3:, 12:] == 0) and np.all(canvas[:, 2, 12:16] == 0)      # fill = 0
    one_row, o = imaging.mosaic(cams, 2, columns=5)
    assert one_row.shape == (1, 4, 30, 3) and o[:, 1].tolist() == [0] * 5
    one_col, o = imaging.mosaic(cameras([(8, 8), (8, 8)], channels=0), 2, columns=1, gap=1, fill=9)
    assert one_col.shape == (2, 9, 4) and o.tolist() == [[0, 0], [0, 5]] and np.all(one_col[:, 4] == 9)


def test_mosaic_rejects_what_it_cannot_place(oracle_native):
    a, b = cameras([(8, 8), (8, 8)])
    with pytest.raises(ValueError, match="same number of frames"):
        imaging.mosaic([a, b[:1]], 2)
    with pytest.raises(ValueError, match="channels"):
        imaging.mosaic([a, np.ascontiguousarray(b[..., 0])], 2)
    with pytest.raises(ValueError, match="larger than"):
        imaging.mosaic([a, b[:, :3]], 4)
    with pytest.raises(ValueError):
        imaging.mosaic([], 2)
    with pytest.raises(ValueError):
        imaging.mosaic([a], 2, fill=256)


# ----------------------------------------------------------------------------- _native.resize_frames: what reaches the C call
class FakeLib:
    def __init__(self):
        self.args = None

    def sba_resize_frames(self, *args):
        self.args = args
        return 0


@pytest.fixture
def fake_lib(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(_native, "load", lambda: lib)
    return lib


def c_args(lib):
    device, ptr, B, H, W, Cn, sr, sf, fx, fy, osr, osf, opts, optr = lib.args
    return dict(ptr=ptr.value, B=B, H=H, W=W, C=Cn, sr=sr, sf=sf, fx=fx, fy=fy, osr=osr, osf=osf, opts=opts._obj, optr=optr.value)


def test_native_takes_pitches_from_strided_views(fake_lib):
    big = np.zeros((3, 40, 50, 3), np.uint8)
    frames = big[:, 2:34, 5:45]                               # 32 x 40 inside 40 x 50
    canvas = np.zeros((3, 20, 30, 3), np.uint8)
    tile = canvas[:, 4:12, 7:17]                              # 8 x 10
    out = _native.resize_frames(frames, 4, 4, out=tile)
    a = c_args(fake_lib)
    assert out is tile
    assert (a["B"], a["H"], a["W"], a["C"], a["fx"], a["fy"]) == (3, 32, 40, 3, 4, 4)
    assert (a["sr"], a["sf"]) == (50 * 3, 40 * 50 * 3) and a["ptr"] == frames.ctypes.data == big.ctypes.data + 2 * 150 + 15
    assert (a["osr"], a["osf"]) == (30 * 3, 20 * 30 * 3) and a["optr"] == tile.ctypes.data == canvas.ctypes.data + 4 * 90 + 21
    o = a["opts"]
    assert (o.frames_on_device, o.out_on_device, o.gray, o.chunk_frames) == (0, 0, 0, 0) and list(o.gray_w) == [0, 0, 0]
    assert ctypes.sizeof(_native.ResizeOpts) == 48

    plane = np.zeros((3, 20, 30), np.uint8)
    _native.resize_frames(frames, 4, 2, gray_w=(0, 0, 32768), out=plane[:, 1:17, 3:13], chunk_frames=2)
    a = c_args(fake_lib)
    assert (a["osr"], a["osf"], a["fx"], a["fy"]) == (30, 600, 4, 2)
    assert (a["opts"].gray, list(a["opts"].gray_w), a["opts"].chunk_frames) == (1, [0, 0, 32768], 2)


def test_native_allocates_the_floor_sizes(fake_lib):
    f = np.zeros((2, 11, 14, 4), np.uint8)
    assert _native.resize_frames(f, 4, 3).shape == (2, 3, 3, 4)
    assert (c_args(fake_lib)["osr"], c_args(fake_lib)["osf"]) == (12, 36)
    assert _native.resize_frames(f, 4, 3, gray_w=(0, 0, 0)).shape == (2, 3, 3)
    assert _native.resize_frames(np.zeros((2, 11, 14), np.uint8), 5, 7).shape == (2, 1, 2)
    assert _native.resize_frames(f[:0], 2, 2).shape == (0, 5, 7, 4)


def test_native_rejects_layouts_the_kernel_cannot_write(fake_lib):
    f = np.zeros((2, 16, 16, 3), np.uint8)
    wide = np.zeros((2, 4, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="contiguous"):
        _native.resize_frames(f, 4, 4, out=wide[:, :, ::2])                  # every second pixel
    with pytest.raises(ValueError, match="contiguous"):
        _native.resize_frames(f, 4, 4, out=np.zeros((2, 4, 4, 4), np.uint8)[..., :3])     # pixels 4 bytes apart
    with pytest.raises(ValueError, match="contiguous"):
        _native.resize_frames(np.zeros((2, 16, 16, 4), np.uint8)[..., :3], 4, 4)
    with pytest.raises(ValueError, match="shape"):
        _native.resize_frames(f, 4, 4, out=np.zeros((2, 4, 5, 3), np.uint8))
    with pytest.raises(ValueError, match="shape"):
        _native.resize_frames(f, 4, 4, gray_w=GRAY_BGR, out=np.zeros((2, 4, 4, 3), np.uint8))
    ro = np.zeros((2, 4, 4, 3), np.uint8)
    ro.setflags(write=False)
    with pytest.raises(ValueError, match="writeable"):
        _native.resize_frames(f, 4, 4, out=ro)
    for fx, fy in ((0, 4), (4, 17)):
        with pytest.raises(ValueError, match="factors"):
            _native.resize_frames(f, fx, fy)
    with pytest.raises(ValueError, match="gray_w"):
        _native.resize_frames(f, 4, 4, gray_w=(1, 2))
    assert fake_lib.args is None                              # none of them reached the library


# ----------------------------------------------------------------------------- OpenCV itself, where it is installed
def test_oracle_equals_opencv():
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(11)
    for C in (1, 3, 4):
        img = rng.integers(0, 256, size=(48, 96, C), dtype=np.uint8)
        src = img[..., 0] if C == 1 else img
        for fx, fy in ((2, 2), (4, 4), (3, 2), (8, 8)):
            got = cv2.resize(src, (96 // fx, 48 // fy), interpolation=cv2.INTER_AREA)
            assert np.array_equal(got, resize_oracle(src[None], fx, fy)[0]), (C, fx, fy)
    for lo, hi in ((0, 2), (254, 256), (0, 256)):
        bgr = rng.integers(lo, hi, size=(37, 53, 3), dtype=np.uint8)
        assert np.array_equal(cv2.cvtColor(bgr, cv2.COLOR_BGR2GRAY), resize_oracle(bgr[None], 1, 1, GRAY_BGR)[0])
        rgb = np.ascontiguousarray(bgr[..., ::-1])
        assert np.array_equal(cv2.cvtColor(rgb, cv2.COLOR_RGB2GRAY), resize_oracle(rgb[None], 1, 1, GRAY_BGR[::-1])[0])
