"""GPU tests of sba_resize_frames (include/sba_hip.h) through ``lasercalib_amd.imaging`` and the raw C ABI.

The reference is ``resize_oracle`` of tests/test_resize_host.py, the header's rule in numpy (checked there on values worked by
hand).  The rule is exact -- integer sums, one float32 multiply of exactly representable values --, so EVERY comparison here is
bit equality; nothing needs a tolerance.  Buffers with padding are pre-filled with a sentinel and compared whole, so a byte
written into the padding shows.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lasercalib_amd import _native, imaging  # noqa: E402
from test_resize_host import GRAY_BGR, resize_oracle  # noqa: E402

SENTINEL = 0xA5
FACTORS = ((1, 1), (2, 2), (4, 4), (3, 2), (2, 3), (8, 8), (16, 16), (5, 7))
CUSTOM = (11000, 768, 21000)                                  # weights that no standard has; they sum to 2^15


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert _native.device_count() > 0, "no HIP device visible: GPU tests must run on the MI355X box"


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def segment_px(fx, channels, gray):
    """rs_segment_px of csrc/sba_resize.hpp: the output pixels a wave takes in one step."""
    per_px, step = fx * (1 if gray else channels), 16 // np.gcd(16, fx * channels)
    return _native.RESIZE_ITEMS // per_px // step * step


def test_constants_are_those_of_the_kernel():
    src = open(os.path.join(os.path.dirname(_native.__file__), "csrc", "sba_resize.hpp")).read()
    assert "constexpr int RS_RUN = 16;" in src and "constexpr int RS_ITEMS = 64 * RS_RUN;" in src
    assert _native.RESIZE_ITEMS == 64 * 16 and _native.RESIZE_MAX_FACTOR == 16
    assert segment_px(4, 3, False) == 84 and segment_px(4, 3, True) == 256 and segment_px(16, 4, False) == 16
    assert segment_px(1, 1, False) == 1024 and segment_px(5, 3, False) == 64 and segment_px(7, 1, False) == 144


FRAMES = {}


def random_frames(B, H, W, C, lo=0, hi=256):
    """Uniform random frames (B, H, W, C), or (B, H, W) for C = 0; shared, never written."""
    key = (B, H, W, C, lo, hi)
    if key not in FRAMES:
        a = np.random.default_rng(1000 * H + 10 * W + C).integers(lo, hi, size=(B, H, W) + ((C,) if C else ()), dtype=np.uint8)
        a.setflags(write=False)
        FRAMES[key] = a
    return FRAMES[key]


def aligned_bytes(n, fill=None):
    """A uint8 array of n bytes whose address is a multiple of 64, so that a base offset is the misalignment it says."""
    raw = np.empty(n + 64, np.uint8)
    off = (-raw.ctypes.data) % 64
    a = raw[off:off + n]
    if fill is not None:
        a[...] = fill
    return a


def view_in(buf, shape, row_slack, frame_slack, base):
    """A (B, H, W, C) view into the flat uint8 ``buf`` (numpy or torch): rows row_slack bytes apart beyond their own, frames
    frame_slack bytes beyond their rows, the first pixel ``base`` bytes in.  -> (view, bytes needed)."""
    B, H, W, C = shape
    sr = W * C + row_slack
    sf = H * sr + frame_slack
    need = base + B * sf
    if buf is None:
        return None, need
    if isinstance(buf, np.ndarray):
        v = np.lib.stride_tricks.as_strided(buf[base:], shape=shape, strides=(sf, sr, C, 1))
    else:
        v = buf.as_strided(shape, (sf, sr, C, 1), base)
    return v, need


def to_device(torch, a):
    return torch.from_numpy(np.array(a)).cuda()              # a copy: the shared frames are read-only


def gray_arg(gray):
    return {None: False, "bgr": True, "custom": CUSTOM}[gray]


def gray_weights(gray):
    return {None: None, "bgr": GRAY_BGR, "custom": CUSTOM}[gray]


# ----------------------------------------------------------------------------- channels x factors x grey
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("fx,fy", FACTORS)
def test_channels_and_factors(C, fx, fy):
    """Two frames whose width spans more than one segment for the larger factors and leaves a remainder in both directions."""
    out_w, out_h = 70, 6
    f = random_frames(2, out_h * fy + fy - 1, out_w * fx + fx - 1, C)
    for gray in (None, "bgr", "custom") if C > 1 else (None,):
        got = imaging.resize_frames(f, (fx, fy), gray=gray_arg(gray))
        want = resize_oracle(f, fx, fy, gray_weights(gray))
        assert got.shape == want.shape and got.dtype == np.uint8
        assert np.array_equal(got, want), (C, fx, fy, gray)
    if C > 1:
        rgb = imaging.resize_frames(f, (fx, fy), gray=True, channel_order="rgb")
        assert np.array_equal(rgb, resize_oracle(f, fx, fy, GRAY_BGR[::-1]))
    else:
        flat = np.ascontiguousarray(f[..., 0])
        assert np.array_equal(imaging.resize_frames(flat, (fx, fy)), resize_oracle(flat, fx, fy))


# ----------------------------------------------------------------------------- sizes around every boundary
SHAPES = [(3, 4, 4, None), (3, 4, 4, "bgr"), (1, 2, 2, None), (4, 3, 2, None), (4, 2, 3, "custom"), (1, 16, 16, None), (3, 1, 1, "bgr")]


@pytest.mark.parametrize("C,fx,fy,gray", SHAPES)
def test_output_widths_and_heights(C, fx, fy, gray, torch):
    """out_w either side of a vector of 16 output bytes, of the 64 lanes and of their multiples; out_h either side of a wave's
    and a workgroup's rows.  The body is dark and the columns and rows beyond the last whole block hold 255: were they read,
    the result would jump."""
    w = gray_weights(gray)
    cases = [(ow, 3, rem) for ow in (1, 15, 16, 17, 63, 64, 65, 127, 128, 129) for rem in (0, 1)]
    cases += [(17, oh, rem) for oh in (1, 2, 3, 31, 33) for rem in (0, 1)]
    for ow, oh, rem in cases:
        rx, ry = rem * (fx - 1), rem * (fy - 1)
        body = random_frames(2, oh * fy, ow * fx, C, 0, 9)
        f = np.full((2, oh * fy + ry, ow * fx + rx, C), 255, np.uint8)
        f[:, :oh * fy, :ow * fx] = body
        want = resize_oracle(body, fx, fy, w)
        assert np.array_equal(imaging.resize_frames(f, (fx, fy), gray=gray_arg(gray)), want), (ow, oh, rem, "host")
        got = imaging.resize_frames(to_device(torch, f), (fx, fy), gray=gray_arg(gray))
        assert np.array_equal(got.cpu().numpy(), want), (ow, oh, rem, "device")


@pytest.mark.parametrize("C,fx,fy,gray", [(3, 4, 4, None), (3, 4, 4, "bgr"), (4, 16, 1, None), (1, 1, 2, None), (4, 1, 1, "bgr"), (3, 5, 7, None)])
def test_segments_of_a_row(C, fx, fy, gray, torch):
    """out_w either side of one and of two segments: the last segment holds one pixel, all but one, or is full."""
    P = segment_px(fx, C, gray is not None)
    for ow in (P - 1, P, P + 1, 2 * P - 1, 2 * P + 1):
        f = random_frames(1, 2 * fy, ow * fx + fx - 1, C)
        got = imaging.resize_frames(to_device(torch, f), (fx, fy), gray=gray_arg(gray))
        assert np.array_equal(got.cpu().numpy(), resize_oracle(f, fx, fy, gray_weights(gray))), ow


def test_bands_of_many_rows(torch):
    """Enough rows, segments and frames that a workgroup takes its largest band, 32 output rows (8 per wave), and the last band
    is cut.  A factor of 1 without grey copies, so the frames themselves are the oracle's result."""
    f = torch.randint(0, 256, (8, 4100, 1025), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    small = f[:1, :40].cpu().numpy()
    assert np.array_equal(resize_oracle(small, 1, 1), small)
    out = torch.full((8, 4100, 1025 + 3), SENTINEL, dtype=torch.uint8, device="cuda")
    imaging.resize_frames(f, 1, out=out[:, :, :1025])
    assert torch.equal(out[:, :, :1025], f) and bool((out[:, :, 1025:] == SENTINEL).all())


# ----------------------------------------------------------------------------- pitches, bases, padding
@pytest.mark.parametrize("C,fx,fy,gray", [(3, 4, 4, None), (3, 4, 4, "bgr"), (1, 2, 2, None), (4, 3, 2, "custom"), (4, 1, 1, None)])
@pytest.mark.parametrize("side", ["host", "device"])
def test_odd_pitches_and_misaligned_bases(C, fx, fy, gray, side, torch):
    """Source and output in padded buffers with odd pitches, their bases misaligned independently by 1..15 bytes; the output
    buffer is compared whole, so its padding must still hold the sentinel."""
    B, oh, ow = 2, 5, 150
    f = random_frames(B, oh * fy + fy - 1, ow * fx + fx - 1, C)
    Co = 1 if gray else C
    want = resize_oracle(f, fx, fy, gray_weights(gray))
    want = want[..., None] if gray else want
    for sbase, obase in ((1, 15), (15, 1), (8, 4), (3, 0), (0, 7), (5, 5), (12, 13)):
        _v, sneed = view_in(None, f.shape, 7, 29, sbase)
        _v, oneed = view_in(None, (B, oh, ow, Co), 5, 31, obase)
        sbuf, obuf = aligned_bytes(sneed, 0xFF), aligned_bytes(oneed, SENTINEL)
        view_in(sbuf, f.shape, 7, 29, sbase)[0][...] = f
        expect = obuf.copy()
        view_in(expect, (B, oh, ow, Co), 5, 31, obase)[0][...] = want
        if side == "device":
            sbuf, obuf = torch.from_numpy(sbuf).cuda(), torch.from_numpy(obuf).cuda()
            assert sbuf.data_ptr() % 64 == 0 and obuf.data_ptr() % 64 == 0
        src, dst = view_in(sbuf, f.shape, 7, 29, sbase)[0], view_in(obuf, (B, oh, ow, Co), 5, 31, obase)[0]
        imaging.resize_frames(src, (fx, fy), gray=gray_arg(gray), out=dst)
        got = obuf.cpu().numpy() if side == "device" else obuf
        assert np.array_equal(got, expect), (sbase, obase)


# ----------------------------------------------------------------------------- host and device on either side, chunks
@pytest.mark.parametrize("C,fx,fy,gray", [(3, 4, 4, None), (3, 2, 2, "bgr"), (1, 3, 2, None)])
def test_memory_sides_and_chunks(C, fx, fy, gray, torch):
    f = random_frames(5, 6 * fy + 1, 100 * fx, C)
    want = resize_oracle(f, fx, fy, gray_weights(gray))
    fd = to_device(torch, f)
    for src, src_dev in ((f, False), (fd, True)):
        for out_dev in (False, True):
            for chunk in (1, 2, 0):
                got = _native.resize_frames(src, fx, fy, gray_w=gray_weights(gray), out_on_device=out_dev, chunk_frames=chunk)
                assert _native._is_tensor(got) == out_dev
                assert np.array_equal(got.cpu().numpy() if out_dev else got, want), (src_dev, out_dev, chunk)
    # host frames into a host output in each class of layout a pitched copy tells apart -- packed, padded rows, a gap between
    # packed frames, both -- in three chunks, the last one short: both staging buffers are used twice, the padding stays
    oshape = want.shape if want.ndim == 4 else want.shape + (1,)
    for row_slack, frame_slack in ((0, 0), (7, 0), (0, 29), (7, 29)):
        sbuf = aligned_bytes(view_in(None, f.shape, row_slack, frame_slack, 3)[1], 0xFF)
        obuf = aligned_bytes(view_in(None, oshape, row_slack and row_slack - 2, frame_slack and frame_slack + 2, 5)[1], SENTINEL)
        view_in(sbuf, f.shape, row_slack, frame_slack, 3)[0][...] = f
        expect = obuf.copy()
        view_in(expect, oshape, row_slack and row_slack - 2, frame_slack and frame_slack + 2, 5)[0][...] = want.reshape(oshape)
        dst = view_in(obuf, oshape, row_slack and row_slack - 2, frame_slack and frame_slack + 2, 5)[0]
        imaging.resize_frames(view_in(sbuf, f.shape, row_slack, frame_slack, 3)[0], (fx, fy), gray=gray_arg(gray), out=dst, chunk_frames=2)
        assert np.array_equal(obuf, expect), (row_slack, frame_slack)
    assert isinstance(imaging.resize_frames(f, (fx, fy)), np.ndarray) and _native._is_tensor(imaging.resize_frames(fd, (fx, fy)))
    host_out = np.empty(want.shape, np.uint8)
    assert imaging.resize_frames(fd, (fx, fy), gray=gray_arg(gray), out=host_out) is host_out and np.array_equal(host_out, want)
    dev_out = torch.empty(want.shape, dtype=torch.uint8, device="cuda")
    imaging.resize_frames(f, (fx, fy), gray=gray_arg(gray), out=dev_out)
    assert np.array_equal(dev_out.cpu().numpy(), want)


# ----------------------------------------------------------------------------- rounding
@pytest.mark.parametrize("lo,hi", [(0, 2), (254, 256), (255, 256), (0, 256)])
def test_rounding_stress(lo, hi):
    """Frames of {0, 1} and of {254, 255} put many sums on a tie; all-255 frames reach the largest sum of every factor."""
    for C, gray in ((1, None), (3, None), (3, "bgr"), (4, "custom")):
        for fx, fy in ((2, 2), (4, 4), (2, 4), (3, 2), (8, 8), (16, 16), (5, 7), (6, 1)):
            f = random_frames(1, 8 * fy, 40 * fx, C, lo, hi)
            got = imaging.resize_frames(f, (fx, fy), gray=gray_arg(gray))
            assert np.array_equal(got, resize_oracle(f, fx, fy, gray_weights(gray))), (C, gray, fx, fy)


# ----------------------------------------------------------------------------- mosaic
@pytest.mark.parametrize("gray", [None, "bgr"])
def test_mosaic_of_three_cameras(gray, torch):
    """Two sizes of camera in one canvas, on the device and on the host: previews, gaps and fill equal the oracle's canvas."""
    cams = [random_frames(3, 64, 96, 3), random_frames(3, 40, 72, 3), random_frames(3, 64, 96, 3)[:, ::-1].copy()]
    want = np.full((3, 16 + 3 + 16, 24 + 3 + 24) + (() if gray else (3,)), 200, np.uint8)
    where = [(0, 0), (27, 0), (0, 19)]
    for cam, (x, y) in zip(cams, where):
        p = resize_oracle(cam, 4, 4, gray_weights(gray))
        want[:, y:y + p.shape[1], x:x + p.shape[2]] = p
    canvas, origins = imaging.mosaic(cams, 4, gap=3, fill=200, gray=gray_arg(gray))
    assert isinstance(canvas, np.ndarray) and origins.tolist() == [list(o) for o in where]
    assert np.array_equal(canvas, want)
    dcanvas, dorigins = imaging.mosaic([to_device(torch, c) for c in cams], 4, gap=3, fill=200, gray=gray_arg(gray), on_device=True)
    assert _native._is_tensor(dcanvas) and np.array_equal(dorigins, origins)
    assert np.array_equal(dcanvas.cpu().numpy(), want)
    mixed, _o = imaging.mosaic([cams[0], to_device(torch, cams[1]), cams[2]], 4, gap=3, fill=200, gray=gray_arg(gray), on_device=True)
    assert np.array_equal(mixed.cpu().numpy(), want)


# ----------------------------------------------------------------------------- decoder frames
def test_decoder_frames_are_converted_in_chunks(torch):
    rng = np.random.default_rng(9)
    nv12 = rng.integers(0, 256, size=(5, 48 + 24, 64), dtype=np.uint8)                 # stacked: 48 luma rows, 24 rows of UV
    bgr = imaging.convert_frames(nv12, "nv12")
    want = imaging.resize_frames(bgr, 4)
    assert np.array_equal(want, resize_oracle(bgr, 4, 4))
    got = imaging.resize_frames(nv12, 4, pixel_format="nv12")
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    assert np.array_equal(imaging.resize_frames(nv12, 4, pixel_format="nv12", chunk_frames=2), want)
    dev = imaging.resize_frames(to_device(torch, nv12), 4, pixel_format="nv12", chunk_frames=3)
    assert _native._is_tensor(dev) and np.array_equal(dev.cpu().numpy(), want)
    gray = imaging.resize_frames(nv12, (2, 4), gray=True, pixel_format="nv12", channel_order="rgb")      # the chunks are BGR
    assert np.array_equal(gray, resize_oracle(bgr, 2, 4, GRAY_BGR))
    bt709 = imaging.resize_frames(nv12, 4, pixel_format="nv12", matrix="bt709")
    assert np.array_equal(bt709, resize_oracle(imaging.convert_frames(nv12, "nv12", matrix="bt709"), 4, 4))


# ----------------------------------------------------------------------------- the reference's shapes
def oracle_in_strips(f, fx, fy, strips=8):
    rows = f.shape[1] // fy // strips * fy
    parts = [resize_oracle(f[:, lo:lo + rows], fx, fy) for lo in range(0, rows * strips, rows)]
    if rows * strips < f.shape[1] // fy * fy:
        parts.append(resize_oracle(f[:, rows * strips:], fx, fy))
    return np.concatenate(parts, axis=1)


def test_reference_frame_shapes(torch):
    """scripts/run_viewers.py:121: 3208 x 2200 x 3 -> 802 x 550; scripts/charuco_intrinsics.py:55: -> 1604 x 1100."""
    g = torch.Generator(device="cuda").manual_seed(2)
    fd = torch.randint(0, 256, (1, 2200, 3208, 3), dtype=torch.uint8, device="cuda", generator=g)
    f = fd.cpu().numpy()
    p4 = imaging.resize_frames(fd, 4)
    assert tuple(p4.shape) == (1, 550, 802, 3) and np.array_equal(p4.cpu().numpy(), oracle_in_strips(f, 4, 4))
    p2 = imaging.resize_frames(fd, 2)
    assert tuple(p2.shape) == (1, 1100, 1604, 3) and np.array_equal(p2.cpu().numpy(), oracle_in_strips(f, 2, 2))


def test_largest_sensor_at_sixteen(torch):
    g = torch.Generator(device="cuda").manual_seed(3)
    fd = torch.randint(0, 256, (1, 7000, 9344), dtype=torch.uint8, device="cuda", generator=g)
    got = imaging.resize_frames(fd, 16)
    assert tuple(got.shape) == (1, 437, 584)
    assert np.array_equal(got.cpu().numpy(), oracle_in_strips(fd.cpu().numpy(), 16, 16))


# ----------------------------------------------------------------------------- no frames; the C ABI's errors
def test_no_frames(torch):
    assert imaging.resize_frames(np.zeros((0, 16, 16, 3), np.uint8), 4).shape == (0, 4, 4, 3)
    assert imaging.resize_frames(np.zeros((0, 16, 16, 3), np.uint8), 4, gray=True).shape == (0, 4, 4)
    assert tuple(imaging.resize_frames(torch.zeros((0, 16, 16), dtype=torch.uint8, device="cuda"), (2, 8)).shape) == (0, 2, 8)
    assert imaging.resize_frames(np.zeros((0, 2, 2, 3), np.uint8), 4).shape == (0, 0, 0, 3)     # no frames: no pixel is missed
    lib = _native.load()
    out = np.full(64, SENTINEL, np.uint8)
    assert lib.sba_resize_frames(0, None, 0, 16, 16, 3, 48, 768, 4, 4, 12, 48, None, ctypes.c_void_p(out.ctypes.data)) == 0
    assert lib.sba_resize_frames(0, None, 0, 16, 16, 3, 48, 768, 4, 4, 12, 48, None, None) == 0
    assert np.all(out == SENTINEL)


def test_every_cabi_error_is_reported_and_leaves_out_untouched():
    lib = _native.load()
    B, H, W, Cn = 2, 9, 14, 3
    f = np.ascontiguousarray(random_frames(B, H, W, Cn))

    def call(n_frames=B, height=H, width=W, channels=Cn, row_pitch=None, frame_pitch=None, fx=4, fy=3, out_row_pitch=None,
             out_frame_pitch=None, gray=0, gray_w=(0, 0, 0), null=(), device=0, use_opts=True):
        out = np.full(B * H * W * 4, SENTINEL, np.uint8)
        rp = max(width, 0) * channels if row_pitch is None else row_pitch
        fp = max(height, 0) * rp if frame_pitch is None else frame_pitch
        ow, oh = (max(width, 0) // fx, max(height, 0) // fy) if fx > 0 and fy > 0 else (0, 0)
        orp = ow * (1 if gray else channels) if out_row_pitch is None else out_row_pitch
        ofp = oh * orp if out_frame_pitch is None else out_frame_pitch
        opts = _native.ResizeOpts()
        opts.gray, opts.gray_w = gray, (ctypes.c_int32 * 3)(*gray_w)
        rc = lib.sba_resize_frames(device, None if "frames" in null else ctypes.c_void_p(f.ctypes.data), n_frames, height, width, channels,
                                   rp, fp, fx, fy, orp, ofp, ctypes.byref(opts) if use_opts else None,
                                   None if "out" in null else ctypes.c_void_p(out.ctypes.data))
        msg = (lib.sba_last_error(None) or b"").decode()
        assert np.all(out == SENTINEL) or rc == 0, "a failed call wrote into out"
        return rc, msg, out

    # the defaults of this helper are a valid call, with and without an options struct, colour and grey
    for kw in (dict(), dict(use_opts=False), dict(gray=1), dict(gray=1, gray_w=CUSTOM), dict(fx=14, fy=9), dict(fx=1, fy=1)):
        rc, msg, out = call(**kw)
        assert rc == 0, msg
        fx, fy, w = kw.get("fx", 4), kw.get("fy", 3), (None if not kw.get("gray") else kw.get("gray_w", GRAY_BGR))
        want = resize_oracle(f, fx, fy, w)
        assert np.array_equal(out[:want.size].reshape(want.shape), want) and np.all(out[want.size:] == SENTINEL)

    invalid = [
        dict(n_frames=-1), dict(height=-1), dict(width=-1), dict(null=("frames",)), dict(null=("out",)),
        dict(channels=2), dict(channels=0), dict(channels=5),
        dict(fx=0), dict(fy=0), dict(fx=17), dict(fy=17), dict(fx=-4),
        dict(fx=15), dict(fy=10), dict(width=3, row_pitch=W * Cn), dict(height=2, frame_pitch=H * W * Cn),
        dict(out_row_pitch=3 * 3 - 1), dict(gray=1, out_row_pitch=2), dict(out_frame_pitch=3 * 9 - 1),
        dict(row_pitch=W * Cn - 1), dict(frame_pitch=H * W * Cn - 1),
        dict(channels=1, gray=1, row_pitch=W * Cn),
        dict(gray=1, gray_w=(-1, 32768, 1)), dict(gray=1, gray_w=(1, 2, 3)), dict(gray=1, gray_w=(16384, 16384, 1)),
        dict(gray=1, gray_w=(32768, 32768, -32768)),
    ]
    seen = set()
    for kw in invalid:
        rc, msg, _out = call(**kw)
        assert rc == -1, (kw, rc, msg)                        # SBA_ERR_INVALID
        assert msg.startswith("sba_resize_frames: ") and len(msg) > 25, (kw, msg)
        seen.add(msg)
    assert len(seen) >= 12                                    # the texts tell the causes apart
    rc, msg, _out = call(width=16385, row_pitch=16385 * Cn, frame_pitch=H * 16385 * Cn)
    assert rc == -6 and "16384" in msg                        # SBA_ERR_UNSUPPORTED, as for the detectors
    rc, msg, _out = call(device=99)
    assert rc in (-1, -2) and msg                             # the device is checked as everywhere
    # gray_w is read only with gray; weights that would be wrong are then no error
    assert call(gray=0, gray_w=(1, 2, 3))[0] == 0
    with pytest.raises(_native.SbaError, match="larger than the frame"):
        imaging.resize_frames(np.zeros((1, 3, 16, 3), np.uint8), 4)
