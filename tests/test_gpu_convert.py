"""GPU tests of sba_convert_frames (include/sba_hip.h) through ``lasercalib_amd.imaging``, the detectors, the background model
and the raw C ABI.

The reference is ``convert_oracle`` of tests/test_convert_host.py, the header's rule in int64 numpy (checked there on values
worked by hand).  The rule is integer arithmetic, so EVERY comparison here is bit equality; nothing needs a tolerance.  Buffers
with padding are pre-filled with a sentinel and compared whole, so a byte written into the padding shows.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lasercalib_amd import _native, imaging  # noqa: E402
from lasercalib_amd import feature_detection as fd  # noqa: E402
from lasercalib_amd.imaging import YuvMatrix  # noqa: E402
from test_convert_host import BT601, FORMATS, at_bound, convert_oracle  # noqa: E402

SENTINEL = 0xA5
RUN, WAVE_COLS, TILE_ROWS = _native.CONVERT_RUN, _native.CONVERT_WAVE_COLS, _native.CONVERT_TILE_ROWS
SOURCES = ("nv12", "nv21", "i420", "yv12")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert _native.device_count() > 0, "no HIP device visible: GPU tests must run on the MI355X box"


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def test_constants_are_those_of_the_kernel():
    src = open(os.path.join(os.path.dirname(_native.__file__), "csrc", "sba_convert.hpp")).read()
    assert "constexpr int CV_RUN = 16;" in src and "constexpr int CV_HALF = 32;" in src
    assert "CV_WAVE_COLS = CV_RUN * CV_HALF;" in src and "CV_TILE_ROWS = DOT_WAVES * 2 * 2;" in src
    assert (RUN, WAVE_COLS, TILE_ROWS) == (16, 16 * 32, 4 * 2 * 2)


# ----------------------------------------------------------------------------- sources: plain planes -> a format's memory
PLANES, ORACLE = {}, {}


def random_planes(B, H, W):
    """(y, u, v) uniform random plain planes; shared, never written."""
    key = (B, H, W)
    if key not in PLANES:
        rng = np.random.default_rng(1000 * H + W)
        p = tuple(rng.integers(0, 256, size=s, dtype=np.uint8) for s in ((B, H, W), (B, (H + 1) // 2, (W + 1) // 2), (B, (H + 1) // 2, (W + 1) // 2)))
        for a in p:
            a.setflags(write=False)
        PLANES[key] = p
    return PLANES[key]


def oracle_of(B, H, W, out_format, matrix=BT601):
    key = (B, H, W, out_format, tuple(matrix))
    if key not in ORACLE:
        ORACLE[key] = convert_oracle(*random_planes(B, H, W), matrix, out_format)
        ORACLE[key].setflags(write=False)
    return ORACLE[key]


def aligned_bytes(n, fill=None):
    """A uint8 array of n bytes whose address is a multiple of 64, so that a base offset is the misalignment it says."""
    raw = np.empty(n + 64, np.uint8)
    off = (-raw.ctypes.data) % 64
    a = raw[off:off + n]
    if fill is not None:
        a[...] = fill
    return a


def view_in(shape, inner, row_slack, frame_slack, base, values=None):
    """A sentinel-filled aligned buffer and a view of `shape` = (B, rows, ...) into it: `inner` bytes per row packed, `row_slack`
    bytes behind every row, `frame_slack` behind every frame, starting `base` bytes in."""
    B, R = shape[0], shape[1]
    row_pitch = inner + row_slack
    frame_pitch = R * row_pitch + frame_slack
    buf = aligned_bytes(base + B * frame_pitch + 32, SENTINEL)
    tail = shape[2:]
    tail_strides = tuple(int(np.prod(tail[i + 1:])) for i in range(len(tail)))
    strides = (frame_pitch, row_pitch) + tail_strides
    view = np.lib.stride_tricks.as_strided(buf[base:], shape=shape, strides=strides)
    if values is not None:
        view[...] = values
    return buf, view, strides


def source(fmt, planes, slack=(0, 0, 0), bases=(0, 0, 0)):
    """The planes in the memory layout of `fmt` as a tuple in the format's order: [(buffer, view, strides, base), ...].  slack =
    (row slack of y, row slack of chroma, frame slack of all); bases = (y, first chroma plane, second chroma plane)."""
    y, u, v = planes
    B, H, W = y.shape
    ch, cw = u.shape[1:]
    out = [view_in((B, H, W), W, slack[0], slack[2], bases[0], y) + (bases[0],)]
    if fmt in ("nv12", "nv21"):
        pair = np.stack((u, v) if fmt == "nv12" else (v, u), axis=-1)
        out.append(view_in((B, ch, cw, 2), 2 * cw, slack[1], slack[2], bases[1], pair) + (bases[1],))
    else:
        first, second = (u, v) if fmt == "i420" else (v, u)
        out.append(view_in((B, ch, cw), cw, slack[1], slack[2], bases[1], first) + (bases[1],))
        out.append(view_in((B, ch, cw), cw, slack[1], slack[2], bases[2], second) + (bases[2],))
    return out


def to_device(torch, parts):
    """[(buffer, view, strides, base)] -> (the device copies of the buffers, the same views on the device)."""
    keep = [torch.from_numpy(np.ascontiguousarray(buf)).cuda() for buf, _v, _s, _b in parts]
    views = tuple(torch.as_strided(t, v.shape, s, storage_offset=b) for t, (_buf, v, s, b) in zip(keep, parts))
    return keep, views


def check(torch, fmt, planes, out_format, want, slack=(0, 0, 0), bases=(0, 0, 0), out_slack=(0, 0), out_base=0, device=False, **kw):
    """One call from the given layout into a sentinel-filled output of the given layout; result and padding bit-equal."""
    parts = source(fmt, planes, slack, bases)
    shape = want.shape if want.ndim == 4 else want.shape + (1,)
    C = shape[3]
    obuf, oview, ostr = view_in(shape, shape[2] * C, out_slack[0], out_slack[1], out_base)
    expect, _ev, _ = view_in(shape, shape[2] * C, out_slack[0], out_slack[1], out_base, want.reshape(shape))
    if want.ndim == 3:
        oview, ostr = oview[..., 0], ostr[:3]
    before = [buf.copy() for buf, *_ in parts]
    if device:
        keep, views = to_device(torch, parts)
        dbuf = torch.from_numpy(np.ascontiguousarray(obuf)).cuda()
        dout = torch.as_strided(dbuf, oview.shape, ostr, storage_offset=out_base)
        assert dout.data_ptr() % 16 == out_base % 16 and views[0].data_ptr() % 16 == bases[0] % 16
        ret = imaging.convert_frames(views, fmt, out_format=out_format, out=dout, **kw)
        assert ret is dout
        got = dbuf.cpu().numpy()
        for t, b in zip(keep, before):
            assert np.array_equal(t.cpu().numpy(), b), "the source was written"
    else:
        ret = imaging.convert_frames(tuple(v for _b, v, _s, _o in parts), fmt, out_format=out_format, out=oview, **kw)
        assert ret is oview
        got = obuf
        for (buf, *_), b in zip(parts, before):
            assert np.array_equal(buf, b), "the source was written"
    if not np.array_equal(got, expect):
        bad = np.flatnonzero(got != expect)
        raise AssertionError(f"{fmt} -> {out_format}, device={device}, slack={slack}, bases={bases}, out {out_slack} + {out_base}: "
                             f"{bad.size} bytes differ, the first at {bad[0]} (got {got[bad[0]]}, expected {expect[bad[0]]})")


# ----------------------------------------------------------------------------- 1. every input triple
def all_triples():
    """64 NV12 frames of 512 x 512 that hold each of the 2^24 (Y, U, V) triples exactly once: the chroma plane of every frame is
    the 256 x 256 table of all (U, V), its luma Y = 4 f + 2 (y & 1) + (x & 1)."""
    f, yy, xx = np.arange(64)[:, None, None], np.arange(512)[None, :, None], np.arange(512)[None, None, :]
    y = (4 * f + 2 * (yy & 1) + (xx & 1)).astype(np.uint8)
    u = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, None, :], (64, 256, 256))
    v = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (64, 256, 256))
    return y, np.ascontiguousarray(u), np.ascontiguousarray(v)


@pytest.fixture(scope="module")
def triples(torch):
    y, u, v = all_triples()
    half = np.arange(512) >> 1
    code = (y.astype(np.int32) << 16) | (u.astype(np.int32)[:, half][:, :, half] << 8) | v.astype(np.int32)[:, half][:, :, half]
    assert np.all(np.bincount(code.ravel(), minlength=1 << 24) == 1), "each triple exactly once"
    return (y, u, v), (torch.from_numpy(y).cuda(), torch.from_numpy(np.stack((u, v), axis=-1)).cuda())


@pytest.mark.parametrize("name", ["bt601", "bt709-full", "at the bound"])
def test_every_input_triple(triples, name):
    (y, u, v), dev = triples
    matrix = YuvMatrix(*at_bound()) if name == "at the bound" else YuvMatrix.preset(name)
    got = imaging.convert_frames(dev, "nv12", out_format="bgr", matrix=matrix).cpu().numpy()
    lo_hi = [255, 0]
    for f in range(0, 64, 8):                                              # the oracle in slices: its int64 planes are large
        want = convert_oracle(y[f:f + 8], u[f:f + 8], v[f:f + 8], matrix.as_tuple(), "bgr")
        part = got[f:f + 8]
        if not np.array_equal(part, want):
            i, r, c, k = (int(j[0]) for j in np.nonzero(part != want))
            raise AssertionError(f"{name}: {np.count_nonzero(part != want)} bytes differ in frames {f}..{f + 7}; (Y, U, V) = "
                                 f"{(y[f + i, r, c], u[f + i, r >> 1, c >> 1], v[f + i, r >> 1, c >> 1])} channel {k}: "
                                 f"got {part[i, r, c, k]}, expected {want[i, r, c, k]}")
        lo_hi = [min(lo_hi[0], int(want.min())), max(lo_hi[1], int(want.max()))]
    assert lo_hi == [0, 255]                                               # both clips are met


# ----------------------------------------------------------------------------- 2. formats x layouts
# base offsets 0, 1, 5, 15 handed round y, the chroma planes and the output; the last two rows add 4 and 8, where the kernel
# reads and writes in pieces of 4 and 8 bytes
BASES = [((0, 1, 5), 15), ((1, 5, 15), 0), ((5, 15, 0), 1), ((15, 0, 1), 5), ((4, 8, 12), 8), ((8, 12, 4), 4)]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("fmt", SOURCES)
def test_formats_and_layouts(torch, fmt, device):
    B, H, W = 3, 37, 53                                                    # three full blocks and a cut one, an odd last row
    planes = random_planes(B, H, W)
    for out_format in FORMATS:
        want = oracle_of(B, H, W, out_format)
        check(torch, fmt, planes, out_format, want, device=device)                                       # packed
        for k, (bases, out_base) in enumerate(BASES):
            if out_format not in ("bgr", "g", "rgba") and k % 3:
                continue                                                   # the other formats: two of the six rotations
            check(torch, fmt, planes, out_format, want, slack=(5, 3, 13), bases=bases, out_slack=(7, 9), out_base=out_base, device=device)
    # a result allocated by the call lies on the side of the source
    parts = source(fmt, planes)
    views = to_device(torch, parts)[1] if device else tuple(p[1] for p in parts)
    got = imaging.convert_frames(views, fmt, out_format="rgb")
    assert (got.is_cuda and got.dtype == torch.uint8) if device else isinstance(got, np.ndarray)
    assert np.array_equal(got.cpu().numpy() if device else got, oracle_of(B, H, W, "rgb"))
    # pitches that are multiples of 16 on every plane and on the output: every row of every stream on the 16-byte path
    check(torch, fmt, planes, "bgr", oracle_of(B, H, W, "bgr"), slack=(11, 16 - (2 * 27 if fmt[0] == "n" else 27) % 16, 16), out_slack=(1, 0), device=device)


def test_chroma_planes_with_a_step_of_two(torch):
    """u and v two bytes apart in planes of their own (not the halves of one interleaved plane), from host and device."""
    B, H, W = 2, 21, 35
    y, u, v = random_planes(B, H, W)
    ch, cw = u.shape[1:]
    wide_u, wide_v = (np.full((B, ch, cw, 2), SENTINEL, np.uint8) for _ in range(2))
    wide_u[..., 0], wide_v[..., 0] = u, v
    for out_format in ("bgr", "g"):
        want = oracle_of(B, H, W, out_format)
        got = imaging.convert_frames((y, wide_u[..., 0], wide_v[..., 0]), "i420", out_format=out_format)
        assert np.array_equal(got, want)
        du, dv = torch.from_numpy(wide_u).cuda(), torch.from_numpy(wide_v).cuda()
        got = imaging.convert_frames((torch.from_numpy(y.copy()).cuda(), du[..., 0], dv[..., 0]), "i420", out_format=out_format)
        assert np.array_equal(got.cpu().numpy(), want)
        # the halves of one plane handed over as planar planes are read as that plane
        pair = np.stack((v, u), axis=-1)
        assert np.array_equal(imaging.convert_frames((y, pair[..., 1], pair[..., 0]), "i420", out_format=out_format), want)


# ----------------------------------------------------------------------------- 3. widths and heights at the kernel's boundaries
WIDTHS = [1, 2, 3, RUN - 1, RUN, RUN + 1, 2 * RUN - 1, 2 * RUN + 1, WAVE_COLS - 1, WAVE_COLS, WAVE_COLS + 1, WAVE_COLS + RUN + 1]
HEIGHTS = [1, 2, 3, 4, 5, TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, 2 * TILE_ROWS + 1]


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_widths_and_heights_either_side_of_every_boundary(torch, fmt):
    B = 2
    for W in WIDTHS:
        for H in HEIGHTS:
            planes = random_planes(B, H, W)
            for out_format in ("bgr", "g"):
                want = oracle_of(B, H, W, out_format)
                check(torch, fmt, planes, out_format, want, device=True)
                if W % 2 and H % 2:                                        # odd x odd: the last pixel alone on its chroma sample
                    check(torch, fmt, planes, out_format, want, slack=(3, 1, 5), bases=(1, 5, 15), out_slack=(3, 5), out_base=15, device=True)
                    check(torch, fmt, planes, out_format, want, slack=(3, 1, 5), bases=(5, 15, 1), out_slack=(3, 5), out_base=0, device=False)
    for out_format in ("bgra", "r"):
        check(torch, fmt, random_planes(B, TILE_ROWS + 1, WAVE_COLS + 1), out_format, oracle_of(B, TILE_ROWS + 1, WAVE_COLS + 1, out_format), device=True)


# ----------------------------------------------------------------------------- 4. chunking
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_any_chunking_gives_the_same_bytes(torch, device):
    n, H, W = 5, 19, 37
    planes = random_planes(n, H, W)
    for fmt, out_format in (("nv12", "bgr"), ("yv12", "g")):
        want = oracle_of(n, H, W, out_format)
        for chunk in (1, 2, 3, n - 1, n, n + 1):
            check(torch, fmt, planes, out_format, want, slack=(5, 3, 13), bases=(1, 5, 15), out_slack=(7, 9), out_base=5, device=device,
                  chunk_frames=chunk)
        # the other classes of layout a pitched copy tells apart -- packed, padded rows without a gap, a gap between packed
        # frames -- on every plane and on the output, in three chunks, the last one short
        for slack, out_slack in (((0, 0, 0), (0, 0)), ((5, 3, 0), (7, 0)), ((0, 0, 13), (0, 9))):
            check(torch, fmt, planes, out_format, want, slack=slack, bases=(1, 5, 15), out_slack=out_slack, out_base=5, device=device,
                  chunk_frames=2)
    # host planes into a device output and device planes into a host output, in chunks
    parts = source("nv12", planes)
    host, dev = tuple(p[1] for p in parts), to_device(torch, parts)[1]
    want = oracle_of(n, H, W, "bgr")
    out = torch.full(want.shape, SENTINEL, dtype=torch.uint8, device="cuda")
    assert imaging.convert_frames(host, "nv12", out=out, chunk_frames=2) is out and np.array_equal(out.cpu().numpy(), want)
    out = np.full(want.shape, SENTINEL, np.uint8)
    assert imaging.convert_frames(dev, "nv12", out=out, chunk_frames=2) is out and np.array_equal(out, want)


def test_no_frames_write_nothing(torch):
    lib = _native.load()
    out = np.full(4096, SENTINEL, np.uint8)
    y = np.zeros(4096, np.uint8)
    opts = _native.ConvertOpts()
    p = ctypes.c_void_p(y.ctypes.data)
    assert lib.sba_convert_frames(0, p, p, p, 0, 8, 8, 8, 64, 4, 16, 1, None, 24, 192, ctypes.byref(opts), ctypes.c_void_p(out.ctypes.data)) == 0
    assert lib.sba_convert_frames(0, None, None, None, 0, 8, 8, 8, 64, 4, 16, 1, None, 24, 192, None, None) == 0
    assert np.all(out == SENTINEL)
    got = imaging.convert_frames((np.zeros((0, 6, 8), np.uint8), np.zeros((0, 3, 4, 2), np.uint8)), "nv12")
    assert got.shape == (0, 6, 8, 3) and got.dtype == np.uint8
    got = imaging.convert_frames(torch.zeros((0, 9, 8), dtype=torch.uint8, device="cuda"), "nv21", out_format="g")
    assert tuple(got.shape) == (0, 6, 8) and got.is_cuda
    # frames without pixels
    got = imaging.convert_frames((np.zeros((3, 0, 8), np.uint8), np.zeros((3, 0, 4, 2), np.uint8)), "nv12")
    assert got.shape == (3, 0, 8, 3)


# ----------------------------------------------------------------------------- 5. stacked and tuple input agree
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_stacked_and_tuple_layouts_agree(torch, device):
    B = 3
    for fmt, H, W in (("nv12", 21, 38), ("nv21", 20, 38), ("i420", 20, 36), ("yv12", 24, 40)):
        y, u, v = random_planes(B, H, W)
        ch, cw = u.shape[1:]
        st = np.empty((B, H + ch, W), np.uint8)
        st[:, :H] = y
        if fmt in ("nv12", "nv21"):
            st[:, H:] = np.stack((u, v) if fmt == "nv12" else (v, u), axis=-1).reshape(B, ch, W)
            tup = (st[:, :H], st[:, H:].reshape(B, ch, cw, 2))
        else:
            first, second = (u, v) if fmt == "i420" else (v, u)
            st.reshape(B, -1)[:, H * W:H * W + ch * cw] = first.reshape(B, -1)
            st.reshape(B, -1)[:, H * W + ch * cw:] = second.reshape(B, -1)
            tup = (y, first, second)
        for out_format in ("bgr", "g"):
            want = oracle_of(B, H, W, out_format)
            a = torch.from_numpy(st).cuda() if device else st
            b = tuple(torch.from_numpy(np.array(p)).cuda() for p in tup) if device else tup
            ga, gb = imaging.convert_frames(a, fmt, out_format=out_format), imaging.convert_frames(b, fmt, out_format=out_format)
            if device:
                ga, gb = ga.cpu().numpy(), gb.cpu().numpy()
            assert np.array_equal(ga, gb) and np.array_equal(ga, want), (fmt, out_format)


# ----------------------------------------------------------------------------- 6. the C ABI's errors
def test_every_cabi_error_is_reported_and_leaves_out_untouched():
    lib = _native.load()
    B, H, W = 2, 9, 13                                                     # 5 x 7 chroma samples
    y, u, v = (np.ascontiguousarray(p) for p in random_planes(B, H, W))
    ch, cw = 5, 7

    def call(n_frames=B, height=H, width=W, y_row_pitch=W, y_frame_pitch=H * W, c_row_pitch=cw, c_frame_pitch=ch * cw, c_step=1,
             matrix=None, out_format=0, out_row_pitch=None, out_frame_pitch=None, null=(), device=0):
        out = np.full((B, H, W, 4), SENTINEL, np.uint8)
        C = {0: 3, 1: 3, 2: 4, 3: 4}.get(out_format, 1)
        orp = max(width, 0) * C if out_row_pitch is None else out_row_pitch
        ofp = max(height, 0) * orp if out_frame_pitch is None else out_frame_pitch
        opts = _native.ConvertOpts()
        opts.out_format = out_format
        m = None if matrix is None else ctypes.byref(_native.YuvMatrix(*matrix))
        ptr = {"y": y, "u": u, "v": v, "out": out}
        args = [None if k in null else ctypes.c_void_p(a.ctypes.data) for k, a in ptr.items()]
        rc = lib.sba_convert_frames(device, args[0], args[1], args[2], n_frames, height, width, y_row_pitch, y_frame_pitch, c_row_pitch,
                                    c_frame_pitch, c_step, m, orp, ofp, ctypes.byref(opts), args[3])
        msg = (lib.sba_last_error(None) or b"").decode()
        assert np.all(out == SENTINEL) or rc == 0, "a failed call wrote into out"
        return rc, msg, out

    for fmt in range(7):                                                   # the defaults of this helper are a valid call
        rc, msg, out = call(out_format=fmt)
        C = _native.PIXEL_BYTES[FORMATS[fmt]]
        assert rc == 0, msg
        got = out.reshape(-1)[:B * H * W * C].reshape((B, H, W, C) if C > 1 else (B, H, W))
        assert np.array_equal(got, oracle_of(B, H, W, FORMATS[fmt]))
    bound = at_bound()
    invalid = [
        dict(n_frames=-1), dict(height=-1), dict(width=-1),
        dict(null=("y",)), dict(null=("u",)), dict(null=("v",)), dict(null=("out",)),
        dict(c_step=0), dict(c_step=3), dict(c_step=-1),
        dict(y_row_pitch=W - 1), dict(y_frame_pitch=H * W - 1),
        dict(c_row_pitch=cw - 1), dict(c_step=2, c_row_pitch=2 * (cw - 1), c_frame_pitch=1000), dict(c_frame_pitch=ch * cw - 1),
        dict(out_row_pitch=3 * W - 1), dict(out_format=2, out_row_pitch=4 * W - 1), dict(out_format=5, out_row_pitch=W - 1),
        dict(out_frame_pitch=H * 3 * W - 1),
        dict(out_format=7), dict(out_format=-1),
        dict(matrix=bound[:5] + (bound[5] + 1,)), dict(matrix=bound[:2] + (bound[2] - 1,) + bound[3:]), dict(matrix=bound[:3] + (bound[3] + 1,) + bound[4:]),
        dict(matrix=(bound[0], bound[1] - 1) + bound[2:]), dict(matrix=(256,) + BT601[1:]), dict(matrix=(-1,) + BT601[1:]),
        dict(matrix=(16, -(1 << 31), 0, 0, 0, 0)),
    ]
    seen = set()
    for kw in invalid:
        rc, msg, _out = call(**kw)
        assert rc == -1 and msg.startswith("sba_convert_frames: ") and len(msg) > 25, (kw, rc, msg)
        seen.add(msg)
    assert len(seen) >= 13                                                 # the texts tell the errors apart
    assert call(c_step=2, c_row_pitch=2 * (cw - 1) + 1, c_frame_pitch=1000, n_frames=0)[0] == 0      # the smallest pitch that holds a row
    assert call(matrix=bound, n_frames=0)[0] == 0
    for kw in (dict(height=16385, y_frame_pitch=16385 * W, c_frame_pitch=8193 * cw), dict(width=16385, y_row_pitch=16385, y_frame_pitch=16385 * H, c_row_pitch=8193, c_frame_pitch=8193 * ch)):
        rc, msg, _out = call(n_frames=0, **kw)
        assert rc == -6 and "16384" in msg, (kw, rc, msg)                  # the detectors' size limit keeps its own status
    rc, msg, _out = call(device=4096)
    assert rc == -2 and msg                                                # no such device
    with pytest.raises(_native.SbaError, match="sba_convert_frames"):
        _native.convert_frames((y, u, v), "i420", matrix=(16, 8421504, 0, 0, 0, 0))
    with pytest.raises(ValueError, match="out has the shape"):
        imaging.convert_frames((y, u, v), "i420", out=np.zeros((B, H, W), np.uint8))
    with pytest.raises(ValueError, match="out_format"):
        imaging.convert_frames((y, u, v), "i420", out_format="yuv")


# ----------------------------------------------------------------------------- 7. through the detectors and the background model
def rendered_video():
    """12 frames of 96 x 128: a bright green spot moves over a dim coloured background, frame 7 has a second spot.  Built as
    YUV with a forward BT.601 transform in numpy -> (y, uv) NV12 planes."""
    n, H, W = 12, 96, 128
    yy, xx = np.mgrid[0:H, 0:W]
    rgb = np.empty((n, H, W, 3), np.float64)
    rgb[..., 0] = 30 + 20 * np.sin(xx / 17.0)                             # dim, coloured, smooth
    rgb[..., 1] = 25 + 15 * np.cos(yy / 11.0)
    rgb[..., 2] = 35 + 10 * np.sin((xx + yy) / 23.0)
    for f in range(n):
        spots = [(20 + 5 * f, 15 + 8 * f)] + ([(70, 30)] if f == 7 else [])
        for cy_, cx_ in spots:
            d2 = (yy - cy_) ** 2 + (xx - cx_) ** 2
            rgb[f, ..., 1] += 220 * np.exp(-d2 / 18.0)
            rgb[f, ..., 0] += 40 * np.exp(-d2 / 18.0)
    rgb = np.clip(rgb, 0, 255)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    yl = 16 + (65.481 * r + 128.553 * g + 24.966 * b) / 255
    cb = 128 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255
    cr = 128 + (112.0 * r - 93.786 * g - 18.214 * b) / 255
    sub = lambda a: a.reshape(n, H // 2, 2, W // 2, 2).mean(axis=(2, 4))      # noqa: E731
    y = np.clip(np.rint(yl), 0, 255).astype(np.uint8)
    uv = np.stack([np.clip(np.rint(sub(c)), 0, 255).astype(np.uint8) for c in (cb, cr)], axis=-1)
    return y, np.ascontiguousarray(uv)


def same_fields(a, b, fields):
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y, equal_nan=x.dtype.kind == "f")), f


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_through_the_detectors_and_the_background_model(torch, device):
    y, uv = rendered_video()
    nv12 = (torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()) if device else (y, uv)
    bgr = imaging.convert_frames(nv12, "nv12", out_format="bgr")
    host_bgr = bgr.cpu().numpy() if device else bgr
    assert np.array_equal(host_bgr, convert_oracle(y, uv[..., 0], uv[..., 1], BT601, "bgr"))
    dot_fields = ("sums", "box", "centroid", "status")
    blob_fields = ("n_components", "blobs", "accepted", "centroid", "status", "mask", "labels")
    for chunk in (0, 5):
        want = fd.find_laser_dots(bgr, threshold=90, channel=1, max_extent=40)
        got = fd.find_laser_dots(nv12, threshold=90, channel=1, max_extent=40, pixel_format="nv12", chunk_frames=chunk)
        same_fields(got, want, dot_fields)
        assert np.all(want.status[np.arange(12) != 7] == fd.SBA_DOT_OK) and want.status[7] == fd.SBA_DOT_SPREAD
        want = fd.find_laser_blobs(bgr, threshold=90, channel=1, want_mask=True, want_labels=True)
        got = fd.find_laser_blobs(nv12, threshold=90, channel=1, want_mask=True, want_labels=True, pixel_format="nv12", chunk_frames=chunk)
        same_fields(got, want, blob_fields)
        assert list(want.n_components) == [1] * 7 + [2] + [1] * 4 and want.status[7] == fd.SBA_BLOB_MULTIPLE
    # the other channels name the other planes, and the stacked form is the same video
    for channel in (0, 2):
        same_fields(fd.find_laser_dots(nv12, threshold=40, channel=channel, pixel_format="nv12"),
                    fd.find_laser_dots(bgr, threshold=40, channel=channel), dot_fields)
    st = np.concatenate([y, uv.reshape(12, 48, 128)], axis=1)
    same_fields(fd.find_laser_dots(torch.from_numpy(st).cuda() if device else st, threshold=90, pixel_format="nv12"),
                fd.find_laser_dots(bgr, threshold=90), dot_fields)
    # the background model: the same statistics, the same suppressed frames, and both in front of a detector
    a = imaging.BackgroundModel(96, 128, channel=1, threshold=40).add(nv12, pixel_format="nv12", chunk_frames=5)
    b = imaging.BackgroundModel(96, 128, channel=1, threshold=40).add(bgr)
    sa, sb = a.state(), b.state()
    assert sa.keys() == sb.keys() and sa["n"] == 12
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    use = np.arange(12) % 3 != 1
    sa = imaging.BackgroundModel(96, 128, channel=1, threshold=40, on_device=False).add(nv12, use=use, pixel_format="nv12", chunk_frames=5).state()
    sb = imaging.BackgroundModel(96, 128, channel=1, threshold=40, on_device=False).add(bgr, use=use).state()
    assert sa["n"] == 8 and all(np.array_equal(sa[k], sb[k]) for k in sa)
    level, mask = b.level(k_sigma=1.0), b.hot_mask(0.5)
    for mode in ("gate", "subtract"):
        want = b.suppress(bgr, mode=mode, level=level, mask=mask)
        got = a.suppress(nv12, mode=mode, level=level, mask=mask, pixel_format="nv12", chunk_frames=5)
        assert type(got) is type(want) and np.array_equal(got.cpu().numpy() if device else got, want.cpu().numpy() if device else want)
    same_fields(fd.find_laser_dots(nv12, threshold=90, pixel_format="nv12", background=(level, mask), chunk_frames=5),
                fd.find_laser_dots(bgr, threshold=90, background=(level, mask)), dot_fields)
    same_fields(fd.find_laser_blobs(nv12, threshold=90, pixel_format="nv12", background=a),
                fd.find_laser_blobs(bgr, threshold=90, background=b), blob_fields[:5])
