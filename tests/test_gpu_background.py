"""GPU: sba_background_accumulate and sba_background_suppress against the numpy oracle of tests/test_background_host.py.
Every accumulator and every output byte is compared for EQUALITY: the statistics are integers, and no layout, chunking,
split of the frames over calls or over workgroups may change a bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from lasercalib_amd import _native

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_background_host import accumulate_oracle, suppress_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

PLANES = ("sum", "sumsq", "hot", "vmax")
DTYPES = {"sum": np.uint32, "sumsq": np.uint64, "hot": np.uint32, "vmax": np.uint8}
SIGNED = {"sum": np.int32, "sumsq": np.int64, "hot": np.int32, "vmax": np.uint8}         # torch dtypes holding the same bits
JUNK = 0xA5                                                                               # what a plane holds before a fresh call
INVALID, UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def torch():
    import torch
    assert _native.device_count() > 0
    return torch


def rand_frames(shape, seed, plain=False):
    """Uniform bytes, unless `plain` with a tenth of them exactly 0 and a tenth exactly 255."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, size=shape, dtype=np.uint8)
    if not plain:
        r = rng.random(shape)
        f[r < 0.1], f[r > 0.9] = 0, 255
    return f


FRAMES, ORACLE = {}, {}


def frames_of(C_):
    """(7, 37, 53, C) random frames; shared, never written."""
    if C_ not in FRAMES:
        FRAMES[C_] = rand_frames((7, 37, 53, C_), 70 + C_)
        FRAMES[C_].setflags(write=False)
    return FRAMES[C_]


def oracle_of(C_, channel, thr=100):
    if (C_, channel, thr) not in ORACLE:
        ORACLE[C_, channel, thr] = accumulate_oracle(frames_of(C_), channel=channel, threshold=thr)
    return ORACLE[C_, channel, thr]


def padded(frames, offset, row_slack, frame_slack, fill=255):
    """The frames inside a buffer filled with `fill`: first byte at `offset`, `row_slack` bytes behind every row, `frame_slack`
    behind every frame.  Returns (buffer, numpy view, strides)."""
    B, H, W, C_ = frames.shape
    rp = W * C_ + row_slack
    fp = H * rp + frame_slack
    buf = np.full(offset + B * fp + 32, fill, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[offset:], shape=frames.shape, strides=(fp, rp, C_, 1))
    view[...] = frames
    return buf, view, (fp, rp, C_, 1)


def on_device(torch, buf, shape, strides, offset):
    t = torch.from_numpy(buf).cuda()
    return t, torch.as_strided(t, shape, strides, storage_offset=offset)


def accumulate(torch, frames, planes=PLANES, stats_dev=False, start=None, **kw):
    """Calls the library with fresh planes full of JUNK (accumulate=False) or with copies of `start` -> the planes and n as a dict."""
    H, W = frames.shape[1:3]
    host = {k: (np.full((H, W), JUNK, DTYPES[k]) if start is None else start[k].copy()) for k in planes}
    given = {k: torch.from_numpy(v.view(SIGNED[k])).cuda() for k, v in host.items()} if stats_dev else host
    n = _native.background_accumulate(frames, n_used=0 if start is None else start["n"], accumulate=start is not None, **given, **kw)
    got = {k: (v.cpu().numpy().view(DTYPES[k]) if stats_dev else v) for k, v in given.items()}
    got["n"] = n
    return got


def assert_same(got, want, planes=PLANES, what=""):
    assert got["n"] == want["n"], f"{what}: n {got['n']} != {want['n']}"
    for k in planes:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), \
            f"{what}: {k} differs at {np.argwhere(got[k] != want[k])[:4].tolist()}"


# ----------------------------------------------------------------------------- 1. layouts
@pytest.mark.parametrize("C_", [1, 3, 4])
def test_accumulate_layouts(torch, C_):
    f = frames_of(C_)
    for channel in range(C_):
        want = oracle_of(C_, channel)
        for offset, row_slack, frame_slack in ((0, 0, 0), (1, 3, 7), (3, 1, 13), (5, 11, 1)):
            buf, view, strides = padded(f, offset, row_slack, frame_slack)
            _t, dview = on_device(torch, buf, f.shape, strides, offset)
            for src, side in ((view, "host"), (dview, "device")):
                for stats_dev in (False, True):
                    got = accumulate(torch, src, stats_dev=stats_dev, threshold=100, channel=channel)
                    assert_same(got, want, what=f"C={C_} channel={channel} offset={offset} {side} frames, stats_dev={stats_dev}")
    assert np.array_equal(view, f) and np.all(buf[:offset] == 255), "the frames were written"


@pytest.mark.parametrize("C_", [1, 3, 4])
def test_suppress_layouts_and_untouched_padding(torch, C_):
    f = frames_of(C_)
    B, H, W = f.shape[:3]
    rng = np.random.default_rng(5)
    level = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    mask = (rng.random((H, W)) < 0.2).astype(np.uint8) * rng.integers(1, 256, size=(H, W), dtype=np.uint8)
    for channel in range(C_):
        for mode in ("gate", "subtract"):
            want = suppress_oracle(f, channel, level, mask, mode)
            for offset, row_slack, frame_slack in ((0, 0, 0), (1, 3, 7), (3, 1, 13), (5, 11, 1)):
                buf, view, strides = padded(f, offset, row_slack, frame_slack)
                # the output: sentinel 0x5A everywhere, other odd pitches than the input's
                obuf, oview, ostrides = padded(np.full((B, H, W, 1), 0x5A, np.uint8), offset + 2, row_slack + 2, frame_slack + 4, fill=0x5A)
                expect = obuf.copy()
                np.lib.stride_tricks.as_strided(expect[offset + 2:], shape=(B, H, W), strides=ostrides[:3])[...] = want
                what = f"C={C_} channel={channel} {mode} offset={offset}"
                # host frames, host model, host output
                out = np.lib.stride_tricks.as_strided(obuf[offset + 2:], shape=(B, H, W), strides=ostrides[:3])
                got = _native.background_suppress(view, level=level, mask=mask, mode=mode, channel=channel, out=out)
                assert got is out and np.array_equal(obuf, expect), f"{what}, host: bytes or padding differ"
                # device frames, device model, device output
                _t, dview = on_device(torch, buf, f.shape, strides, offset)
                dobuf = torch.full((obuf.size,), 0x5A, dtype=torch.uint8, device="cuda")
                dout = torch.as_strided(dobuf, (B, H, W), ostrides[:3], storage_offset=offset + 2)
                _native.background_suppress(dview, level=torch.from_numpy(level).cuda(), mask=torch.from_numpy(mask).cuda(), mode=mode,
                                            channel=channel, out=dout)
                assert np.array_equal(dobuf.cpu().numpy(), expect), f"{what}, device: bytes or padding differ"
    # mixed sides and an output the wrapper allocates: device frames with a host model, host frames with a device model
    want = suppress_oracle(f, 0, level, mask, "gate")
    assert np.array_equal(_native.background_suppress(torch.tensor(f).cuda(), level=level, mask=mask, channel=0).cpu().numpy(), want)
    assert np.array_equal(_native.background_suppress(f, level=torch.from_numpy(level).cuda(), mask=torch.from_numpy(mask).cuda(), channel=0), want)


# ----------------------------------------------------------------------------- 2. boundaries of the 16-byte groups
# row lengths in bytes either side of one 16-byte group, of a wave's 64 groups and of four waves' (those that the channel count
# divides are used), and a few more that 3 divides
ROW_BYTES = (15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 18, 48, 1026, 4098)


@pytest.mark.parametrize("C_", [1, 3])
@pytest.mark.parametrize("B", [1, 5])
def test_row_lengths_either_side_of_the_group_boundaries(torch, C_, B):
    for nbytes in ROW_BYTES:
        if nbytes % C_:
            continue
        W = nbytes // C_
        f = rand_frames((B, 3, W, C_), nbytes + B)
        channel = C_ - 1
        want = accumulate_oracle(f, channel=channel, threshold=128)
        for src in (f, torch.tensor(f).cuda()):
            assert_same(accumulate(torch, src, threshold=128, channel=channel), want, what=f"C={C_} W={W} B={B}")
        assert_same(accumulate(torch, f, planes=("sum",), threshold=128, channel=channel), want, planes=("sum",), what=f"sum only, W={W}")
    for W in (1, 5, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025):         # and of the output's groups of 16 pixels
        f = rand_frames((B, 3, W, C_), W + B)
        level = rand_frames((3, W), W)
        for mode in ("gate", "subtract"):
            want = suppress_oracle(f, 0, level, None, mode)
            assert np.array_equal(_native.background_suppress(f, level=level, mode=mode, channel=0), want), f"suppress C={C_} W={W} {mode}"
            got = _native.background_suppress(torch.tensor(f).cuda(), level=level, mode=mode, channel=0)
            assert np.array_equal(got.cpu().numpy(), want), f"suppress C={C_} W={W} {mode}, device"


# ----------------------------------------------------------------------------- 3. chunking and splitting
@pytest.mark.parametrize("side", ["host", "device"])
def test_any_chunking_and_any_split_give_the_same_bits(torch, side):
    f = frames_of(3)
    src = f if side == "host" else torch.tensor(f).cuda()
    want = oracle_of(3, 1)
    level = rand_frames(f.shape[1:3], 9)
    clean = suppress_oracle(f, 1, level, None, "gate")
    for chunk in (1, 2, 3, 7, 0):
        assert_same(accumulate(torch, src, threshold=100, chunk_frames=chunk), want, what=f"chunk_frames={chunk}")
        got = _native.background_suppress(src, level=level, chunk_frames=chunk)
        assert np.array_equal(got if side == "host" else got.cpu().numpy(), clean), f"suppress chunk_frames={chunk}"
    # each class of layout a pitched copy tells apart -- packed, padded rows, a gap between packed frames, both -- on the frames
    # and on the output, in four chunks, the last one short: both staging buffers are used twice, the padding stays
    for row_slack, frame_slack in ((0, 0), (3, 0), (0, 7), (3, 7)):
        buf, view, strides = padded(f, 1, row_slack, frame_slack)
        obuf, oview, ostrides = padded(np.full(clean.shape + (1,), 0x5A, np.uint8), 3, row_slack and row_slack + 2, frame_slack and frame_slack + 4, fill=0x5A)
        expect = obuf.copy()
        np.lib.stride_tricks.as_strided(expect[3:], shape=clean.shape, strides=ostrides[:3])[...] = clean
        src, out = view, oview[..., 0]
        if side == "device":
            (_t, src), (dobuf, out) = on_device(torch, buf, f.shape, strides, 1), on_device(torch, obuf, clean.shape, ostrides[:3], 3)
        assert_same(accumulate(torch, src, threshold=100, chunk_frames=2), want, what=f"slack {row_slack}, {frame_slack}")
        assert _native.background_suppress(src, level=level, out=out, chunk_frames=2) is out
        assert np.array_equal(obuf if side == "host" else dobuf.cpu().numpy(), expect), f"suppress, slack {row_slack}, {frame_slack}: bytes or padding"
    # 0-2 then 3-6, and the other way round
    for first, second in ((slice(0, 3), slice(3, 7)), (slice(3, 7), slice(0, 3))):
        part = accumulate(torch, src[first], threshold=100)
        assert_same(part, accumulate_oracle(f[first], threshold=100), what="first part")
        assert_same(accumulate(torch, src[second], start=part, threshold=100), want, what=f"{first} then {second}")
    # a use mask against a call on the kept frames
    use = np.array([0, 1, 1, 0, 1, 1, 0], np.uint8)
    kept = accumulate_oracle(f[use != 0], threshold=100)
    assert_same(accumulate_oracle(f, threshold=100, use=use), kept)
    for chunk in (0, 2):
        assert_same(accumulate(torch, src, use=use, threshold=100, chunk_frames=chunk), kept, what=f"use mask, chunk_frames={chunk}")
    assert_same(accumulate(torch, src, use=use, start=kept, threshold=100), accumulate_oracle(f, threshold=100, use=use, into=kept), what="use mask, adding")
    # no frame takes part: adding changes nothing, n included; a fresh call gives zeros
    for stats_dev in (False, True):
        assert_same(accumulate(torch, src, use=np.zeros(7, np.uint8), start=kept, stats_dev=stats_dev, threshold=100), kept, what="use all zero")
        zeros = accumulate(torch, src, use=np.zeros(7, np.uint8), stats_dev=stats_dev, threshold=100)
        assert zeros["n"] == 0 and not any(zeros[k].any() for k in PLANES)


# ----------------------------------------------------------------------------- 4. the frames of a chunk split over grid.y
def test_frames_split_over_workgroups_merge_to_the_same_bits(torch):
    assert (_native.BG_SPLIT_GROUPS, _native.BG_SPLIT_FRAMES) == (65536, 16)
    f = rand_frames((300, 4, 5, 1), 1)
    want = accumulate_oracle(f, channel=0, threshold=100)
    use = (np.arange(300) % 3 != 1).astype(np.uint8)
    for src in (f, torch.tensor(f).cuda()):
        for stats_dev in (False, True):
            assert_same(accumulate(torch, src, stats_dev=stats_dev, threshold=100, channel=0), want, what=f"300 frames of 4 x 5, stats_dev={stats_dev}")
            half = accumulate(torch, src[:140], stats_dev=stats_dev, threshold=100, channel=0)
            assert_same(accumulate(torch, src[140:], start=half, stats_dev=stats_dev, threshold=100, channel=0), want, what="split, adding")
        assert_same(accumulate(torch, src, use=use, threshold=100, channel=0), accumulate_oracle(f, 0, 100, use=use), what="split, use mask")
        for planes in (("sum",), ("vmax",), ("sumsq", "hot")):
            assert_same(accumulate(torch, src, planes=planes, threshold=100, channel=0), want, planes=planes, what=f"split, {planes}")
    # either side of the frame count: 16 frames are one share, 17 are split; chunk_frames = 16 keeps 300 frames unsplit
    f3 = rand_frames((17, 5, 7, 3), 2)
    for n in (16, 17):
        assert_same(accumulate(torch, f3[:n], threshold=100), accumulate_oracle(f3[:n], threshold=100), what=f"{n} frames")
    assert_same(accumulate(torch, f, threshold=100, channel=0, chunk_frames=16), want, what="chunks of 16")
    # either side of the frame size: 4096 rows of 16 groups are BG_SPLIT_GROUPS, 4095 rows are below
    big = rand_frames((18, 4096, 256, 1), 3, plain=True)
    dbig = torch.from_numpy(big).cuda()
    for rows in (4095, 4096):
        assert_same(accumulate(torch, dbig[:, :rows], stats_dev=True, threshold=100, channel=0),
                    accumulate_oracle(big[:, :rows], channel=0, threshold=100), what=f"{rows} rows")


# ----------------------------------------------------------------------------- 5. the width of the accumulators
def test_accumulators_use_their_whole_width(torch):
    H, W = 5, 21
    f = np.full((3, H, W, 1), 255, np.uint8)
    start = {"sum": np.full((H, W), 2 ** 32 - 1 - 3 * 255, np.uint32), "sumsq": np.full((H, W), 2 ** 32 - 1, np.uint64),
             "hot": np.full((H, W), 2 ** 32 - 1 - 3, np.uint32), "vmax": np.full((H, W), 7, np.uint8), "n": 2 ** 24 - 3}
    for stats_dev in (False, True):
        got = accumulate(torch, f, start=start, stats_dev=stats_dev, threshold=254, channel=0)
        assert got["n"] == 2 ** 24
        assert np.all(got["sum"] == 2 ** 32 - 1) and np.all(got["hot"] == 2 ** 32 - 1) and np.all(got["vmax"] == 255)
        assert np.all(got["sumsq"] == 2 ** 32 - 1 + 3 * 255 * 255), "the square sum carries into its high word"
    # one frame too many: refused before anything is touched
    start["n"] = 2 ** 24 - 2
    planes = {k: start[k].copy() for k in PLANES}
    with pytest.raises(_native.SbaError, match="status -6.*2\\^24"):
        _native.background_accumulate(f, n_used=start["n"], threshold=254, channel=0, **planes)
    assert all(np.array_equal(planes[k], start[k]) for k in PLANES)
    # a fresh call does not look at the count it is handed
    assert _native.background_accumulate(f, n_used=2 ** 24, accumulate=False, channel=0, sum=planes["sum"]) == 3 and np.all(planes["sum"] == 765)


# ----------------------------------------------------------------------------- 6. NULL outputs, no frames
def test_null_planes_null_model_and_no_frames(torch):
    f = frames_of(3)
    want = oracle_of(3, 1)
    for stats_dev in (False, True):
        for k in PLANES:
            assert_same(accumulate(torch, f, planes=(k,), stats_dev=stats_dev, threshold=100), want, planes=(k,), what=f"{k} alone")
        assert accumulate(torch, f, planes=(), stats_dev=stats_dev)["n"] == 7
    level, mask = rand_frames(f.shape[1:3], 3), (rand_frames(f.shape[1:3], 4) > 200).astype(np.uint8)
    for mode in ("gate", "subtract"):
        assert np.array_equal(_native.background_suppress(f, level=None, mask=mask, mode=mode), suppress_oracle(f, 1, None, mask, mode))
        assert np.array_equal(_native.background_suppress(f, level=level, mask=None, mode=mode), suppress_oracle(f, 1, level, None, mode))
        assert np.array_equal(_native.background_suppress(f, mode=mode), f[..., 1])
    # n_frames = 0: adding leaves the planes as they are, a fresh call zeroes them; suppress writes nothing
    for stats_dev in (False, True):
        assert_same(accumulate(torch, f[:0], start=want, stats_dev=stats_dev), want, what="no frames, adding")
        zeros = accumulate(torch, f[:0], stats_dev=stats_dev)
        assert zeros["n"] == 0 and not any(zeros[k].any() for k in PLANES)
    assert _native.background_suppress(f[:0], level=level).shape == (0,) + f.shape[1:3]


# ----------------------------------------------------------------------------- 7. errors
def test_errors_leave_planes_and_output_untouched(torch):
    lib = _native.load()
    H, W, Cn, B = 6, 10, 3, 2
    f = rand_frames((B, H, W, Cn), 8)
    planes = {k: np.full((H, W), JUNK, DTYPES[k]) for k in PLANES}
    out = np.full((B, H, W), JUNK, np.uint8)
    ok = dict(frames=f.ctypes.data, n=B, h=H, w=W, c=Cn, rp=W * Cn, fp=H * W * Cn, channel=1, threshold=50, mode=0, orp=W, ofp=H * W,
              out=out.ctypes.data, n_used=0)

    def call(which, **change):
        a = dict(ok, **change)
        if which == "accumulate":
            o = _native.BgAccumulateOpts(channel=a["channel"], threshold=a["threshold"], accumulate=1)
            n = C.c_uint64(a["n_used"])
            rc = lib.sba_background_accumulate(0, C.c_void_p(a["frames"]), a["n"], a["h"], a["w"], a["c"], a["rp"], a["fp"], C.byref(o), None,
                                               *(C.c_void_p(planes[k].ctypes.data) for k in PLANES), C.byref(n))
            assert rc == 0 or n.value == a["n_used"], "n_used was written"
        else:
            o = _native.BgSuppressOpts(channel=a["channel"], mode=a["mode"])
            rc = lib.sba_background_suppress(0, C.c_void_p(a["frames"]), a["n"], a["h"], a["w"], a["c"], a["rp"], a["fp"], None, None,
                                             a["orp"], a["ofp"], C.byref(o), C.c_void_p(a["out"]))
        return rc, (lib.sba_last_error(None) or b"").decode()

    frame_errors = [(dict(frames=None), INVALID, "null frames"), (dict(c=2), INVALID, "channels"), (dict(channel=3), INVALID, "channel"),
                    (dict(channel=-1), INVALID, "channel"), (dict(n=-1), INVALID, "negative"), (dict(h=-1), INVALID, "negative"),
                    (dict(rp=W * Cn - 1), INVALID, "row_pitch"), (dict(fp=H * W * Cn - 1), INVALID, "frame_pitch"),
                    (dict(w=16385, rp=16385 * Cn, fp=H * 16385 * Cn, orp=16385, ofp=H * 16385), UNSUPPORTED, "16384"),
                    (dict(h=16385, fp=16385 * W * Cn, ofp=16385 * W), UNSUPPORTED, "16384")]
    own = {"accumulate": [(dict(threshold=256), INVALID, "threshold"), (dict(threshold=-1), INVALID, "threshold"),
                          (dict(n_used=2 ** 24 - 1), UNSUPPORTED, "2^24"), (dict(n_used=2 ** 24), UNSUPPORTED, "2^24")],
           "suppress": [(dict(mode=2), INVALID, "mode"), (dict(mode=-1), INVALID, "mode"), (dict(out=None), INVALID, "null out"),
                        (dict(orp=W - 1), INVALID, "out_row_pitch"), (dict(ofp=H * W - 1), INVALID, "out_frame_pitch")]}
    for which in ("accumulate", "suppress"):
        for change, code, text in frame_errors + own[which]:
            before = {k: planes[k].copy() for k in PLANES}
            rc, msg = call(which, **change)
            assert rc == code and msg.startswith(f"sba_background_{which}: ") and text in msg, (which, change, rc, msg)
            assert all(np.array_equal(planes[k], before[k]) for k in PLANES) and np.all(out == JUNK), (which, change)
        rc, msg = call(which)
        assert rc == 0, (which, msg)
    assert np.array_equal(out, f[..., 1]) and np.array_equal(planes["vmax"], np.maximum(f[..., 1].max(0), JUNK))

    # the wrappers refuse what the library could not describe
    with pytest.raises(ValueError, match="all be numpy arrays or all be device tensors"):
        _native.background_accumulate(f, sum=np.zeros((H, W), np.uint32), hot=torch.zeros((H, W), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="sumsq"):
        _native.background_accumulate(f, sumsq=np.zeros((H, W), np.uint32))
    with pytest.raises(ValueError, match="use must hold"):
        _native.background_accumulate(f, sum=np.zeros((H, W), np.uint32), use=[1, 0, 1])
    with pytest.raises(ValueError, match="mode"):
        _native.background_suppress(f, mode="clip")
    with pytest.raises(ValueError, match="level"):
        _native.background_suppress(f, level=np.zeros((H, W + 1), np.uint8))


# ----------------------------------------------------------------------------- 8. determinism
def test_two_calls_give_the_same_bits(torch):
    f = torch.from_numpy(rand_frames((40, 24, 100, 3), 11)).cuda()           # 24 x 19 groups, 40 frames: the split path with its atomics
    a, b = (accumulate(torch, f, stats_dev=True, threshold=100) for _ in range(2))
    assert_same(a, b)
    assert_same(a, accumulate_oracle(f.cpu().numpy(), threshold=100))
    level = rand_frames((24, 100), 12)
    x, y = (_native.background_suppress(f, level=level, mode="subtract").cpu().numpy() for _ in range(2))
    assert np.array_equal(x, y)
