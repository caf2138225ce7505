"""GPU tests of sba_frames_to_yuv (include/sba_hip.h) through ``lasercalib_amd.imaging`` and the raw C ABI.

The reference is ``to_yuv_oracle`` of tests/test_yuv_host.py, the header's rule in int64 numpy (checked there on values worked
by hand).  The rule is integer arithmetic, so EVERY comparison here is bit equality; nothing needs a tolerance.  Buffers with
padding are pre-filled with a sentinel and compared whole, so a byte written into the padding shows.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lasercalib_amd import _native, imaging  # noqa: E402
from lasercalib_amd.imaging import RgbMatrix  # noqa: E402
from test_convert_host import convert_oracle  # noqa: E402
from test_gpu_convert import SENTINEL, view_in  # noqa: E402
from test_yuv_host import BT601, IN_FORMATS, at_bound, to_yuv_oracle  # noqa: E402

RUN, WAVE_COLS, TILE_ROWS = _native.CONVERT_RUN, _native.CONVERT_WAVE_COLS, _native.CONVERT_TILE_ROWS   # the kernel has k_convert's geometry
TARGETS = ("nv12", "nv21", "i420", "yv12")
CHANNELS = {"bgr": 3, "rgb": 3, "bgra": 4, "rgba": 4, "gray": 1}
MATRICES = ["bt601", "bt709-full", "at the bound"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert _native.device_count() > 0, "no HIP device visible: GPU tests must run on the MI355X box"


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def matrix_of(name):
    return RgbMatrix(*at_bound()) if name == "at the bound" else RgbMatrix.preset(name)


def test_the_kernel_has_the_geometry_of_k_convert():
    src = open(os.path.join(os.path.dirname(_native.__file__), "csrc", "sba_yuv.hpp")).read()
    assert "* CV_HALF + (lane & (CV_HALF - 1))) * CV_RUN;" in src and "(P.height + CV_TILE_ROWS - 1) / CV_TILE_ROWS" in src
    assert (RUN, WAVE_COLS, TILE_ROWS) == (16, 512, 16)


# ----------------------------------------------------------------------------- frames, oracles, layouts
FRAMES, ORACLE = {}, {}


def random_frames(B, H, W, C, lo=0, hi=256):
    """Uniform random frames (B, H, W, C), or (B, H, W) for C = 1; shared, never written."""
    key = (B, H, W, C, lo, hi)
    if key not in FRAMES:
        rng = np.random.default_rng(1000 * H + W + 7 * C + lo)
        FRAMES[key] = rng.integers(lo, hi, size=(B, H, W, C) if C > 1 else (B, H, W), dtype=np.uint8)
        FRAMES[key].setflags(write=False)
    return FRAMES[key]


def oracle_of(frames, key, in_format, chroma, matrix=BT601):
    key = key + (in_format, chroma, tuple(matrix))
    if key not in ORACLE:
        ORACLE[key] = to_yuv_oracle(frames, matrix, in_format, chroma)
        for p in ORACLE[key]:
            p.setflags(write=False)
    return ORACLE[key]


def target(fmt, B, H, W, slack=(0, 0, 0), bases=(0, 0, 0), values=None):
    """Sentinel-filled memory in the layout of `fmt` as a tuple in the format's order: [(buffer, view, strides, base), ...], holding
    `values` = (y, u, v) when given.  slack = (row slack of y, row slack of chroma, frame slack of all); bases = (y, first chroma
    plane, second chroma plane)."""
    ch, cw = (H + 1) // 2, (W + 1) // 2
    y, u, v = values if values is not None else (None, None, None)
    out = [view_in((B, H, W), W, slack[0], slack[2], bases[0], y) + (bases[0],)]
    if fmt in ("nv12", "nv21"):
        pair = None if values is None else np.stack((u, v) if fmt == "nv12" else (v, u), axis=-1)
        out.append(view_in((B, ch, cw, 2), 2 * cw, slack[1], slack[2], bases[1], pair) + (bases[1],))
    else:
        first, second = (u, v) if fmt == "i420" else (v, u)
        out.append(view_in((B, ch, cw), cw, slack[1], slack[2], bases[1], first) + (bases[1],))
        out.append(view_in((B, ch, cw), cw, slack[1], slack[2], bases[2], second) + (bases[2],))
    return out


def on_device(torch, parts):
    """[(buffer, view, strides, base)] -> (the device copies of the buffers, the same views on the device)."""
    keep = [torch.from_numpy(np.ascontiguousarray(buf)).cuda() for buf, _v, _s, _b in parts]
    views = tuple(torch.as_strided(t, v.shape, s, storage_offset=b) for t, (_buf, v, s, b) in zip(keep, parts))
    return keep, views


def check(torch, frames, in_format, fmt, chroma, want, matrix="bt601", src_slack=(0, 0), src_base=0, slack=(0, 0, 0), bases=(0, 0, 0),
          device_in=False, device_out=False, **kw):
    """One call from frames in the given layout into sentinel-filled planes of the given layout; planes and padding bit-equal."""
    shape = frames.shape if frames.ndim == 4 else frames.shape + (1,)
    B, H, W, C = shape
    sbuf, sview, sstr = view_in(shape, W * C, src_slack[0], src_slack[1], src_base, frames.reshape(shape))
    src = [(sbuf, sview if frames.ndim == 4 else sview[..., 0], sstr if frames.ndim == 4 else sstr[:3], src_base)]
    before = sbuf.copy()
    parts = target(fmt, B, H, W, slack, bases)
    expect = [p[0] for p in target(fmt, B, H, W, slack, bases, want)]
    if device_in:
        skeep, (sv,) = on_device(torch, src)
        assert sv.data_ptr() % 16 == src_base % 16
    else:
        sv = src[0][1]
    if device_out:
        keep, views = on_device(torch, parts)
    else:
        views = tuple(p[1] for p in parts)
    ret = imaging.frames_to_yuv(sv, fmt, in_format=in_format, matrix=matrix, chroma=chroma, out=views, **kw)
    assert ret is views
    got = [t.cpu().numpy() for t in keep] if device_out else [p[0] for p in parts]
    assert np.array_equal(skeep[0].cpu().numpy() if device_in else sbuf, before), "the source was written"
    for k, (g, e) in enumerate(zip(got, expect)):
        if not np.array_equal(g, e):
            bad = np.flatnonzero(g != e)
            raise AssertionError(f"{in_format} -> {fmt} ({chroma}), in {'device' if device_in else 'host'} {src_slack} + {src_base}, out "
                                 f"{'device' if device_out else 'host'} {slack} + {bases}: plane {k}: {bad.size} bytes differ, the first at "
                                 f"{bad[0]} (got {g[bad[0]]}, expected {e[bad[0]]})")


# ----------------------------------------------------------------------------- 1. every input triple
@pytest.fixture(scope="module")
def triples(torch):
    """(64, 512, 512, 3) BGR frames that hold each of the 2^24 (B, G, R) triples exactly once, on the host and on the device."""
    code = np.arange(1 << 24, dtype=np.uint32).reshape(64, 512, 512)
    bgr = np.stack((code & 255, code >> 8 & 255, code >> 16), axis=-1).astype(np.uint8)
    return bgr, torch.from_numpy(bgr).cuda()


@pytest.fixture(scope="module")
def spread_triples(torch, triples):
    """The same triples at the even / even positions of (64, 1024, 1024, 3) frames, the other pixels 255 - their block's: the
    positions the nearest mode must not read."""
    dev = torch.empty((64, 1024, 1024, 3), dtype=torch.uint8, device="cuda")
    dev[:] = (255 - triples[1]).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    dev[:, ::2, ::2] = triples[1]
    return dev


def first_difference(got, want):
    idx = tuple(int(j[0]) for j in np.nonzero(got != want))
    return f"{np.count_nonzero(got != want)} bytes differ, the first at {idx}: got {got[idx]}, expected {want[idx]}"


@pytest.mark.parametrize("name", MATRICES)
def test_every_triple_for_luma(triples, name):
    bgr, dev = triples
    m = matrix_of(name)
    y, _uv = imaging.frames_to_yuv(dev, "nv12", matrix=m, out=(dev.new_empty((64, 512, 512)), dev.new_empty((64, 256, 256, 2))))
    got = y.cpu().numpy()
    lo_hi = [255, 0]
    for f in range(0, 64, 8):                                              # the oracle in slices: its int64 planes are large
        want = to_yuv_oracle(bgr[f:f + 8], m.as_tuple())[0]
        assert np.array_equal(got[f:f + 8], want), f"{name}, frames {f}..{f + 7}: " + first_difference(got[f:f + 8], want)
        lo_hi = [min(lo_hi[0], int(want.min())), max(lo_hi[1], int(want.max()))]
    assert lo_hi == {"bt601": [16, 235], "bt709-full": [0, 255], "at the bound": [0, 255]}[name]


@pytest.mark.parametrize("name", MATRICES)
def test_every_triple_for_nearest_chroma(triples, spread_triples, name):
    bgr, _dev = triples
    m = matrix_of(name)
    _y, u, v = imaging.frames_to_yuv(spread_triples, "i420", matrix=m, out=tuple(spread_triples.new_empty(s) for s in
                                                                                  ((64, 1024, 1024), (64, 512, 512), (64, 512, 512))))
    u, v = u.cpu().numpy(), v.cpu().numpy()
    seen = set()
    for f in range(0, 64, 8):                                              # the oracle only at the positions read: 1 x 1 frames
        _wy, wu, wv = to_yuv_oracle(bgr[f:f + 8].reshape(-1, 1, 1, 3), m.as_tuple())
        for got, want, what in ((u[f:f + 8], wu.reshape(8, 512, 512), "U"), (v[f:f + 8], wv.reshape(8, 512, 512), "V")):
            assert np.array_equal(got, want), f"{name}, {what}, frames {f}..{f + 7}: " + first_difference(got, want)
            seen |= {int(want.min()), int(want.max())}
    # both ends of the range are met (a full-range row of -1/2, +1/2 reaches 128 - 127.5 + 0.5 = 1)
    assert (min(seen), max(seen)) == {"bt601": (16, 240), "bt709-full": (1, 255), "at the bound": (0, 255)}[name]


# ----------------------------------------------------------------------------- 2. the average mode
@pytest.mark.parametrize("name", MATRICES)
def test_average_mode(torch, name):
    B, H, W = 3, 37, 53                                                    # three full blocks and a cut one, an odd last row
    m = matrix_of(name)
    for lo, hi in ((0, 256), (0, 2), (254, 256)):                          # sums 0..4 and 1016..1020: every rounding of a block
        frames = random_frames(B, H, W, 3, lo, hi)
        want = oracle_of(frames, (B, H, W, 3, lo, hi), "bgr", "average", m.as_tuple())
        for fmt in ("nv12", "i420"):
            check(torch, frames, "bgr", fmt, "average", want, matrix=m, device_in=True, device_out=True)
    frames = random_frames(2, 2 * TILE_ROWS + 1, WAVE_COLS + RUN + 1, 3)
    want = oracle_of(frames, frames.shape, "bgr", "average", m.as_tuple())
    check(torch, frames, "bgr", "nv12", "average", want, matrix=m, device_in=True, device_out=True)


# ----------------------------------------------------------------------------- 3. formats x layouts
# base offsets 0, 1, 5, 15 handed round the source, y and the chroma planes; the last two rows add 4 and 8, where the kernel reads
# and writes in pieces of 4 and 8 bytes
BASES = [(0, (1, 5, 15)), (1, (5, 15, 0)), (5, (15, 0, 1)), (15, (0, 1, 5)), (4, (8, 12, 4)), (8, (4, 8, 12))]


@pytest.mark.parametrize("device_out", [False, True], ids=["to host", "to device"])
@pytest.mark.parametrize("device_in", [False, True], ids=["from host", "from device"])
@pytest.mark.parametrize("fmt", TARGETS)
def test_formats_and_layouts(torch, fmt, device_in, device_out):
    B, H, W = 3, 37, 53
    for in_format in IN_FORMATS:
        frames = random_frames(B, H, W, CHANNELS[in_format])
        for chroma in ("nearest", "average"):
            want = oracle_of(frames, (B, H, W), in_format, chroma)
            check(torch, frames, in_format, fmt, chroma, want, device_in=device_in, device_out=device_out)                 # packed
            for k, (src_base, bases) in enumerate(BASES):
                if (in_format not in ("bgr", "gray") or chroma == "average") and k % 3:
                    continue                                               # the other combinations: two of the six rotations
                check(torch, frames, in_format, fmt, chroma, want, src_slack=(7, 9), src_base=src_base, slack=(5, 3, 13), bases=bases,
                      device_in=device_in, device_out=device_out)
    # pitches that are multiples of 16 on the source and on every plane: every row of every stream on the 16-byte path
    frames = random_frames(B, H, W, 3)
    check(torch, frames, "bgr", fmt, "nearest", oracle_of(frames, (B, H, W), "bgr", "nearest"), src_slack=(1, 0),
          slack=(11, 16 - (2 * 27 if fmt[0] == "n" else 27) % 16, 16), device_in=device_in, device_out=device_out)
    # a result allocated by the call lies on the side of the frames: a tuple for an odd size, stacked frames for an even one
    src = torch.from_numpy(np.array(frames)).cuda() if device_in else frames
    got = imaging.frames_to_yuv(src, fmt)
    assert isinstance(got, tuple) and len(got) == (2 if fmt[0] == "n" else 3)
    assert all((p.is_cuda and p.dtype == torch.uint8) if device_in else isinstance(p, np.ndarray) for p in got)
    y, u, v = oracle_of(frames, (B, H, W), "bgr", "nearest")
    order = (y, np.stack((u, v) if fmt == "nv12" else (v, u), axis=-1)) if fmt[0] == "n" else (y, u, v) if fmt == "i420" else (y, v, u)
    assert all(np.array_equal(p.cpu().numpy() if device_in else p, w) for p, w in zip(got, order))
    even = random_frames(B, 20, 36, 3)
    got = imaging.frames_to_yuv(torch.from_numpy(np.array(even)).cuda() if device_in else even, fmt, chroma="average")
    got = got.cpu().numpy() if device_in else got
    y, u, v = oracle_of(even, (B, 20, 36), "bgr", "average")
    order = (y, np.stack((u, v) if fmt == "nv12" else (v, u), axis=-1)) if fmt[0] == "n" else (y, u, v) if fmt == "i420" else (y, v, u)
    assert got.shape == (B, 30, 36) and np.array_equal(got.reshape(B, -1), np.concatenate([p.reshape(B, -1) for p in order], axis=1))


def test_chroma_planes_with_a_step_of_two(torch):
    """u and v two bytes apart in planes of their own (not the halves of one interleaved plane): the bytes in between stay."""
    B, H, W = 2, 21, 35
    frames = random_frames(B, H, W, 3)
    ch, cw = 11, 18
    for chroma in ("nearest", "average"):
        y, u, v = oracle_of(frames, (B, H, W), "bgr", chroma)
        for device in (False, True):
            wide_u, wide_v, got_y = (np.full(s, SENTINEL, np.uint8) for s in ((B, ch, cw, 2), (B, ch, cw, 2), (B, H, W)))
            if device:
                wide_u, wide_v, got_y = (torch.from_numpy(a).cuda() for a in (wide_u, wide_v, got_y))
            for chunk in (0, 1):
                imaging.frames_to_yuv(frames, "i420", chroma=chroma, out=(got_y, wide_u[..., 0], wide_v[..., 0]), chunk_frames=chunk)
                a, b, c = (t.cpu().numpy() if device else t for t in (got_y, wide_u, wide_v))
                assert np.array_equal(a, y) and np.array_equal(b[..., 0], u) and np.array_equal(c[..., 0], v)
                assert np.all(b[..., 1] == SENTINEL) and np.all(c[..., 1] == SENTINEL), "a byte between two samples was written"
        # the halves of one plane handed over as planar planes are written as that plane
        pair = np.full((B, ch, cw, 2), SENTINEL, np.uint8)
        imaging.frames_to_yuv(frames, "i420", chroma=chroma, out=(np.empty((B, H, W), np.uint8), pair[..., 1], pair[..., 0]))
        assert np.array_equal(pair[..., 1], u) and np.array_equal(pair[..., 0], v)


# ----------------------------------------------------------------------------- 4. widths and heights at the kernel's boundaries
WIDTHS = [1, 2, 3, RUN - 1, RUN, RUN + 1, 2 * RUN - 1, 2 * RUN + 1, WAVE_COLS - 1, WAVE_COLS, WAVE_COLS + 1, WAVE_COLS + RUN - 1, WAVE_COLS + RUN + 1]
HEIGHTS = [1, 2, 3, 4, 5, TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1, 2 * TILE_ROWS - 1, 2 * TILE_ROWS + 1]


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_widths_and_heights_either_side_of_every_boundary(torch, fmt):
    B = 2
    for W in WIDTHS:
        for H in HEIGHTS:
            frames = random_frames(B, H, W, 3)
            for chroma in ("nearest", "average"):
                want = oracle_of(frames, (B, H, W), "bgr", chroma)
                check(torch, frames, "bgr", fmt, chroma, want, device_in=True, device_out=True)
                if W % 2 and H % 2:                                        # odd x odd: the last pixel alone in its block
                    check(torch, frames, "bgr", fmt, chroma, want, src_slack=(3, 5), src_base=15, slack=(3, 1, 5), bases=(1, 5, 15),
                          device_in=True, device_out=True)
                    check(torch, frames, "bgr", fmt, chroma, want, src_slack=(3, 5), src_base=1, slack=(3, 1, 5), bases=(5, 15, 0))
    for in_format in ("rgba", "gray"):
        frames = random_frames(B, TILE_ROWS + 1, WAVE_COLS + 1, CHANNELS[in_format])
        check(torch, frames, in_format, fmt, "average", oracle_of(frames, frames.shape[:3], in_format, "average"), device_in=True, device_out=True)


# ----------------------------------------------------------------------------- 5. chunking
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_any_chunking_gives_the_same_bytes(torch, device):
    n, H, W = 5, 19, 37
    for fmt, in_format, chroma in (("nv12", "bgr", "nearest"), ("yv12", "gray", "average")):
        frames = random_frames(n, H, W, CHANNELS[in_format])
        want = oracle_of(frames, (n, H, W), in_format, chroma)
        for chunk in (1, 2, n - 1, n, n + 1):
            check(torch, frames, in_format, fmt, chroma, want, src_slack=(7, 9), src_base=5, slack=(5, 3, 13), bases=(1, 5, 15),
                  device_in=device, device_out=device, chunk_frames=chunk)
        # the other classes of layout a pitched copy tells apart -- packed, padded rows without a gap, a gap between packed
        # frames -- on the source and on every plane, in three chunks, the last one short
        for src_slack, slack in (((0, 0), (0, 0, 0)), ((7, 0), (5, 3, 0)), ((0, 9), (0, 0, 13))):
            check(torch, frames, in_format, fmt, chroma, want, src_slack=src_slack, src_base=5, slack=slack, bases=(1, 5, 15),
                  device_in=device, device_out=device, chunk_frames=2)
        # host frames into device planes and device frames into host planes, in chunks
        check(torch, frames, in_format, fmt, chroma, want, device_in=device, device_out=not device, chunk_frames=2)


def test_no_frames_write_nothing(torch):
    lib = _native.load()
    out = np.full(4096, SENTINEL, np.uint8)
    src = np.zeros(4096, np.uint8)
    opts = _native.ToYuvOpts()
    p, q = ctypes.c_void_p(src.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    assert lib.sba_frames_to_yuv(0, p, 0, 8, 8, 3, 24, 192, q, q, q, 8, 64, 4, 16, 1, None, ctypes.byref(opts)) == 0
    assert lib.sba_frames_to_yuv(0, None, 0, 8, 8, 3, 24, 192, None, None, None, 8, 64, 4, 16, 1, None, None) == 0
    assert np.all(out == SENTINEL)
    got = imaging.frames_to_yuv(np.zeros((0, 6, 8, 3), np.uint8))
    assert got.shape == (0, 9, 8) and got.dtype == np.uint8
    got = imaging.frames_to_yuv(torch.zeros((0, 5, 8), dtype=torch.uint8, device="cuda"), "yv12")
    assert [tuple(p.shape) for p in got] == [(0, 5, 8), (0, 3, 4), (0, 3, 4)] and all(p.is_cuda for p in got)
    got = imaging.frames_to_yuv(np.zeros((3, 0, 8, 3), np.uint8))              # frames without pixels
    assert got.shape == (3, 0, 8)


# ----------------------------------------------------------------------------- 6. the C ABI's errors
def test_every_cabi_error_is_reported_and_leaves_the_planes_untouched():
    lib = _native.load()
    B, H, W = 2, 9, 13                                                     # 5 x 7 chroma samples
    ch, cw = 5, 7
    frames = np.ascontiguousarray(random_frames(B, H, W, 4))

    def call(n_frames=B, height=H, width=W, channels=3, row_pitch=None, frame_pitch=None, y_row_pitch=W, y_frame_pitch=H * W, c_row_pitch=cw,
             c_frame_pitch=ch * cw, c_step=1, matrix=None, in_format=0, chroma=0, null=(), device=0):
        planes = {k: np.full((B, H, W), SENTINEL, np.uint8) for k in "yuv"}
        rp = max(width, 0) * channels if row_pitch is None else row_pitch
        fp = max(height, 0) * rp if frame_pitch is None else frame_pitch
        opts = _native.ToYuvOpts()
        opts.in_format, opts.chroma = in_format, chroma
        m = None if matrix is None else ctypes.byref(_native.RgbMatrix(*matrix))
        ptr = dict(frames=frames, **planes)
        a = [None if k in null else ctypes.c_void_p(v.ctypes.data) for k, v in ptr.items()]
        rc = lib.sba_frames_to_yuv(device, a[0], n_frames, height, width, channels, rp, fp, a[1], a[2], a[3], y_row_pitch, y_frame_pitch,
                                   c_row_pitch, c_frame_pitch, c_step, m, ctypes.byref(opts))
        msg = (lib.sba_last_error(None) or b"").decode()
        assert rc == 0 or all(np.all(p == SENTINEL) for p in planes.values()), "a failed call wrote into a plane"
        return rc, msg, planes

    for in_format, chroma, channels in ((0, 0, 3), (1, 1, 3), (2, 0, 4), (3, 1, 4), (0, 1, 1), (3, 0, 1)):   # the defaults are a valid call
        rc, msg, planes = call(in_format=in_format, chroma=chroma, channels=channels)
        assert rc == 0, msg
        src = frames.reshape(-1)[:B * H * W * channels].reshape((B, H, W, channels) if channels > 1 else (B, H, W))
        want = to_yuv_oracle(src, BT601, "gray" if channels == 1 else ("bgr", "rgb", "bgra", "rgba")[in_format], ("nearest", "average")[chroma])
        assert np.array_equal(planes["y"].reshape(-1)[:B * H * W], want[0].reshape(-1))
        assert np.array_equal(planes["u"].reshape(-1)[:B * ch * cw], want[1].reshape(-1))
        assert np.array_equal(planes["v"].reshape(-1)[:B * ch * cw], want[2].reshape(-1))
    bound = at_bound()

    def past(i):
        m = list(bound)
        m[i] += 1 if m[i] >= 0 else -1
        return tuple(m)

    invalid = [
        dict(n_frames=-1), dict(height=-1), dict(width=-1),
        dict(null=("frames",)), dict(null=("y",)), dict(null=("u",)), dict(null=("v",)),
        dict(channels=2), dict(channels=0), dict(channels=5),
        dict(c_step=0), dict(c_step=3), dict(c_step=-1),
        dict(row_pitch=3 * W - 1), dict(frame_pitch=H * 3 * W - 1), dict(channels=4, in_format=2, row_pitch=4 * W - 1),
        dict(y_row_pitch=W - 1), dict(y_frame_pitch=H * W - 1),
        dict(c_row_pitch=cw - 1), dict(c_step=2, c_row_pitch=2 * (cw - 1), c_frame_pitch=1000), dict(c_frame_pitch=ch * cw - 1),
        dict(in_format=4), dict(in_format=-1), dict(in_format=2), dict(channels=4, in_format=1), dict(channels=1, in_format=6),
        dict(chroma=2), dict(chroma=-1),
        dict(matrix=past(1)), dict(matrix=past(2)), dict(matrix=past(5)), dict(matrix=past(6)), dict(matrix=past(8)), dict(matrix=past(9)),
        dict(matrix=(256,) + BT601[1:]), dict(matrix=(-1,) + BT601[1:]), dict(matrix=(16, -(1 << 31), 0, 0, 0, 0, 0, 0, 0, 0)),
    ]
    seen = set()
    for kw in invalid:
        rc, msg, _planes = call(**kw)
        assert rc == -1 and msg.startswith("sba_frames_to_yuv: ") and len(msg) > 25, (kw, rc, msg)
        seen.add(msg)
    assert len(seen) >= 15                                                 # the texts tell the errors apart
    assert call(c_step=2, c_row_pitch=2 * (cw - 1) + 1, c_frame_pitch=1000, n_frames=0)[0] == 0      # the smallest pitch that holds a row
    assert call(matrix=bound, n_frames=0)[0] == 0
    for kw in (dict(height=16385, y_frame_pitch=16385 * W, c_frame_pitch=8193 * cw), dict(width=16385, y_row_pitch=16385, y_frame_pitch=16385 * H, c_row_pitch=8193, c_frame_pitch=8193 * ch)):
        rc, msg, _planes = call(n_frames=0, **kw)
        assert rc == -6 and "16384" in msg, (kw, rc, msg)                  # the detectors' size limit keeps its own status
    rc, msg, _planes = call(device=4096)
    assert rc == -2 and msg                                                # no such device
    with pytest.raises(_native.SbaError, match="sba_frames_to_yuv"):
        _native.frames_to_yuv(np.ascontiguousarray(frames[..., :3]), matrix=past(1))


# ----------------------------------------------------------------------------- 7. with the other frame functions
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_undistorted_frames_leave_as_yuv(torch, device):
    n, H, W = 5, 40, 52
    frames = random_frames(n, H, W, 3)
    src = torch.from_numpy(np.array(frames)).cuda() if device else frames
    lens = imaging.Lens(60.0, 58.0, 25.5, 19.0, -0.2, 0.05, 0.001, -0.002, 0.01)
    for kw in (dict(), dict(out_size=(36, 30), interpolation="nearest", border_value=7)):
        plain = imaging.undistort_frames(src, lens, **kw)
        for fmt, chroma, chunk in (("nv12", "nearest", 0), ("i420", "average", 2), ("nv21", "average", n + 1)):
            want = imaging.frames_to_yuv(plain, fmt, chroma=chroma, matrix="bt709")
            got = imaging.undistort_frames(src, lens, out_pixel_format=fmt, out_matrix="bt709", out_chroma=chroma, chunk_frames=chunk, **kw)
            assert type(got) is type(want) and tuple(got.shape) == tuple(want.shape)
            assert np.array_equal(got.cpu().numpy() if device else got, want.cpu().numpy() if device else want), (fmt, chroma, chunk, kw)
    # the diagnostics come with it, once per call, and a caller's planes are written in place
    plain, flags, qmap = imaging.undistort_frames(src, lens, want_flags=True, want_map=True)
    out = np.full((n, H + H // 2, W), SENTINEL, np.uint8)
    got, f2, m2 = imaging.undistort_frames(src, lens, out_pixel_format="nv12", out=out, want_flags=True, want_map=True, chunk_frames=2)
    assert got is out and np.array_equal(f2, flags) and np.array_equal(m2, qmap)
    assert np.array_equal(out, imaging.frames_to_yuv(plain.cpu().numpy() if device else plain, "nv12"))
    # without the new arguments a call is what it was
    again = imaging.undistort_frames(src, lens)
    assert type(again) is type(plain) and np.array_equal(again.cpu().numpy() if device else again, plain.cpu().numpy() if device else plain)


def test_round_trip_through_convert_frames(torch):
    B, H, W = 2, 38, 54
    frames = random_frames(B, H, W, 3)
    dev = torch.from_numpy(np.array(frames)).cuda()
    for fmt in TARGETS:
        for chroma in ("nearest", "average"):
            back = imaging.convert_frames(imaging.frames_to_yuv(dev, fmt, chroma=chroma), fmt).cpu().numpy()
            assert np.array_equal(back, convert_oracle(*oracle_of(frames, (B, H, W), "bgr", chroma))), (fmt, chroma)
    # on frames of constant 2 x 2 blocks the trip is that of single pixels: off by at most 2, 1, 2 in R, G, B (tests/test_yuv_host.py)
    blocks = np.repeat(np.repeat(random_frames(B, H // 2, W // 2, 3), 2, axis=1), 2, axis=2)
    back = imaging.convert_frames(imaging.frames_to_yuv(blocks, "nv12"), "nv12")
    err = np.abs(back.astype(np.int64) - blocks).reshape(-1, 3).max(axis=0)
    assert np.all(err <= (2, 1, 2)), err                                   # B, G, R
