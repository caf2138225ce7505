"""GPU tests of sba_undistort_frames (include/sba_hip.h) through ``lasercalib_amd.imaging`` and the raw C ABI.

The reference is ``undistort_oracle`` of tests/test_undistort_host.py, the header's rule in numpy (checked there on cases with
known answers).  The rule is IEEE float64 operation by operation followed by integer arithmetic, so EVERY comparison here is
bit equality -- pixels, flags and map; nothing needs a tolerance.  Buffers with padding are pre-filled with a sentinel and
compared whole, so a byte written into (or a result depending on) the padding shows.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lasercalib_amd import _native, imaging  # noqa: E402
from lasercalib_amd.imaging import Lens  # noqa: E402
from test_undistort_host import CX, CY, F, FOLDED, LENSES, OUTSIDE, RANGE, undistort_oracle  # noqa: E402

SENTINEL = 0xA5
TR, TC = _native.UNDIST_TILE_ROWS, _native.UNDIST_TILE_COLS


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert _native.device_count() > 0, "no HIP device visible: GPU tests must run on the MI355X box"


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


RANDOM, ORACLE = {}, {}


def random_frames(C):
    """(5, 47, 61, C) uniform random frames; shared, never written."""
    if C not in RANDOM:
        f = np.random.default_rng(70 + C).integers(0, 256, size=(5, 47, 61, C), dtype=np.uint8)
        f.setflags(write=False)
        RANDOM[C] = f
    return RANDOM[C]


def oracle_of(C, lens, new_k, out_hw=(47, 61), border=0, nearest=False):
    key = (C, tuple(lens), tuple(new_k), tuple(out_hw), border, nearest)
    if key not in ORACLE:
        ORACLE[key] = undistort_oracle(random_frames(C), lens, new_k, out_hw, border=border, nearest=nearest)
    return ORACLE[key]


def padded(shape, row_slack, frame_slack, base, values=None):
    """A uint8 buffer full of SENTINEL and a (B, H, W, C) view into it that starts `base` bytes in, with `row_slack` bytes behind
    every row and `frame_slack` behind every frame; the view holds `values` when given."""
    B, H, W, C = shape
    row_pitch = W * C + row_slack
    frame_pitch = H * row_pitch + frame_slack
    buf = np.full(base + B * frame_pitch + 32, SENTINEL, np.uint8)
    strides = (frame_pitch, row_pitch, C, 1)
    view = np.lib.stride_tricks.as_strided(buf[base:], shape=shape, strides=strides)
    if values is not None:
        view[...] = values
    return buf, view, strides


def on_device(torch, buf, shape, strides, base):
    t = torch.from_numpy(buf).cuda()
    return t, torch.as_strided(t, shape, strides, storage_offset=base)


def lens_of(name):
    lens, nk = LENSES[name]
    return Lens(*lens), nk


def run_layouts(torch, C, lens9, nk, out_hw, want, **kw):
    """The call from host and device memory, packed and padded with misaligned bases on both sides; everything bit-equal to `want`."""
    frames = random_frames(C)
    lens = Lens(*lens9)
    wo, wf, wm = want
    size = (out_hw[1], out_hw[0])
    got, flags, qmap = imaging.undistort_frames(frames, lens, nk, size, want_flags=True, want_map=True, **kw)
    assert isinstance(got, np.ndarray) and np.array_equal(got, wo), "host packed"
    assert np.array_equal(flags, wf) and np.array_equal(qmap, wm) and flags.dtype == np.uint8 and qmap.dtype == np.int32
    dev = torch.from_numpy(frames.copy()).cuda()
    got = imaging.undistort_frames(dev, lens, nk, size, **kw)
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), wo), "device packed"
    # odd pitches, misaligned bases: source (row + 5, frame + 13, base 3) and output (row + 7, frame + 9, base 5)
    sbuf, sview, sstr = padded(frames.shape, 5, 13, 3, frames)
    obuf, oview, ostr = padded(wo.shape, 7, 9, 5)
    expect, eview, _ = padded(wo.shape, 7, 9, 5, wo)
    src_before = sbuf.copy()
    ret = imaging.undistort_frames(sview, lens, nk, size, out=oview, **kw)
    assert ret is oview and np.array_equal(obuf, expect), "host padded: result or padding"
    assert np.array_equal(sbuf, src_before)
    keep_s, dsrc = on_device(torch, sbuf, frames.shape, sstr, 3)
    keep_o, dout = on_device(torch, np.full_like(obuf, SENTINEL), wo.shape, ostr, 5)
    assert dsrc.data_ptr() % 16 != dout.data_ptr() % 16 and dout.data_ptr() % 16 != 0
    ret = imaging.undistort_frames(dsrc, lens, nk, size, out=dout, **kw)
    assert ret is dout and np.array_equal(keep_o.cpu().numpy(), expect), "device padded: result or padding"
    assert np.array_equal(keep_s.cpu().numpy(), src_before)


# ----------------------------------------------------------------------------- 1. random frames, every lens, layout and option
@pytest.mark.parametrize("C", [3, 1, 4])
@pytest.mark.parametrize("name", list(LENSES))
def test_random_frames_every_lens_layout_and_option(torch, C, name):
    lens9, nk = LENSES[name]
    for interpolation in ("linear", "nearest"):
        for border in (0, 200):
            want = oracle_of(C, lens9, nk, border=border, nearest=interpolation == "nearest")
            run_layouts(torch, C, lens9, nk, (47, 61), want, interpolation=interpolation, border_value=border)
    flags = oracle_of(C, lens9, nk)[1]
    if name == "identity":
        assert not flags.any() and np.array_equal(oracle_of(C, lens9, nk)[0], random_frames(C))
    if name == "folded":
        assert np.any(flags & FOLDED) and np.any(flags & OUTSIDE)
    if name == "wild":
        assert np.any(flags & RANGE)


def test_three_dimensional_frames_are_one_channel(torch):
    lens, nk = lens_of("barrel")
    frames = random_frames(1)
    want = oracle_of(1, *LENSES["barrel"])[0][..., 0]
    got = imaging.undistort_frames(frames[..., 0], lens, nk)
    assert got.shape == (5, 47, 61) and np.array_equal(got, want)
    got = imaging.undistort_frames(torch.from_numpy(frames[..., 0].copy()).cuda(), lens, nk)
    assert tuple(got.shape) == (5, 47, 61) and np.array_equal(got.cpu().numpy(), want)


def test_default_matrix_is_the_lens_own(torch):
    lens9, _ = LENSES["rig"]
    want = oracle_of(3, lens9, lens9[:4])
    got = imaging.undistort_frames(random_frames(3), Lens(*lens9))
    assert np.array_equal(got, want[0])
    K = np.array([[F, 0, CX], [0, F, CY], [0, 0, 1.0]])
    assert np.array_equal(imaging.undistort_frames(random_frames(3), Lens(*lens9), K), want[0])


# ----------------------------------------------------------------------------- 2. output sizes
@pytest.mark.parametrize("out_hw", [(23, 130), (1, 1), (130, 23)])
def test_output_size_differs_from_the_source(torch, out_hw):
    lens9, _ = LENSES["barrel"]
    nk = (F * out_hw[1] / 61, F * out_hw[0] / 47, CX * out_hw[1] / 61, CY * out_hw[0] / 47)      # the whole view, rescaled
    run_layouts(torch, 3, lens9, nk, out_hw, oracle_of(3, lens9, nk, out_hw))


@pytest.mark.parametrize("C", [3, 1, 4])
def test_output_widths_around_vectors_waves_and_tiles(torch, C):
    """Widths 1, 15, 16, 17 (around one 16-byte store), 63, 64, 65 (around a wave), 255, 257 (around the 256-pixel tile)."""
    assert TC == 256
    lens9, _ = LENSES["pincushion"]
    for w in (1, 15, 16, 17, 63, 64, 65, 255, 257):
        nk = (F * w / 61, F, 31.0 * w / 61, 22.5)
        for nearest in (False, True):
            run_layouts(torch, C, lens9, nk, (5, w), oracle_of(C, lens9, nk, (5, w), border=77, nearest=nearest),
                        interpolation="nearest" if nearest else "linear", border_value=77)


def test_output_heights_around_the_tile(torch):
    lens9, _ = LENSES["barrel"]
    for h in (TR - 1, TR, TR + 1, 2 * TR - 1, 2 * TR, 2 * TR + 1):
        nk = (F, F * h / 47, CX, CY * h / 47)
        run_layouts(torch, 3, lens9, nk, (h, 61), oracle_of(3, lens9, nk, (h, 61)))


# ----------------------------------------------------------------------------- 3. chunking
@pytest.mark.parametrize("C", [3, 1])
def test_any_chunk_size_gives_the_same_bits(torch, C):
    lens9, nk = LENSES["barrel"]
    want = oracle_of(C, lens9, nk)[0]
    frames = random_frames(C)
    dev = torch.from_numpy(frames.copy()).cuda()
    for chunk in (1, 2, 0, 5, 7):
        assert np.array_equal(imaging.undistort_frames(frames, Lens(*lens9), nk, chunk_frames=chunk), want), ("host", chunk)
        assert np.array_equal(imaging.undistort_frames(dev, Lens(*lens9), nk, chunk_frames=chunk).cpu().numpy(), want), ("device", chunk)
    # a single frame, and chunks of two padded frames
    sbuf, sview, _ = padded(frames.shape, 5, 13, 3, frames)
    assert np.array_equal(imaging.undistort_frames(sview, Lens(*lens9), nk, chunk_frames=2), want)
    assert np.array_equal(imaging.undistort_frames(frames[3:4], Lens(*lens9), nk), want[3:4])
    # host frames into a host output in each class of layout a pitched copy tells apart -- packed, padded rows, a gap between
    # packed frames, both -- in three chunks, the last one short: both staging buffers are used twice, the padding stays
    for row_slack, frame_slack in ((0, 0), (5, 0), (0, 13), (5, 13)):
        sbuf, sview, _ = padded(frames.shape, row_slack, frame_slack, 3, frames)
        obuf, oview, _ = padded(want.shape, row_slack and row_slack + 2, frame_slack and frame_slack - 4, 5)
        expect = padded(want.shape, row_slack and row_slack + 2, frame_slack and frame_slack - 4, 5, want)[0]
        assert imaging.undistort_frames(sview, Lens(*lens9), nk, out=oview, chunk_frames=2) is oview
        assert np.array_equal(obuf, expect), (row_slack, frame_slack)


# ----------------------------------------------------------------------------- 4. edge cases
def test_no_frames_still_gives_flags_and_map(torch):
    lens9, nk = LENSES["folded"]
    _, wf, wm = oracle_of(3, lens9, nk)
    out, flags, qmap = imaging.undistort_frames(np.zeros((0, 47, 61, 3), np.uint8), Lens(*lens9), nk, want_flags=True, want_map=True)
    assert out.shape == (0, 47, 61, 3) and np.array_equal(flags, wf) and np.array_equal(qmap, wm)
    out, flags, qmap = imaging.undistort_frames(torch.zeros((0, 47, 61, 3), dtype=torch.uint8, device="cuda"), Lens(*lens9), nk, want_map=True)
    assert tuple(out.shape) == (0, 47, 61, 3) and flags is None and np.array_equal(qmap, wm)
    region = imaging.invertible_region(Lens(*lens9), nk, (61, 47))
    assert region.dtype == bool and region.shape == (47, 61) and np.array_equal(region, (wf & FOLDED) == 0) and not region.all()
    assert imaging.invertible_region(Lens(*LENSES["rig"][0]), None, (61, 47)).all()


def test_diagnostics_only_reads_no_frame():
    lens9, nk = LENSES["wild"]
    _, wf, wm = oracle_of(3, lens9, nk)
    out, flags, qmap = _native.undistort_frames(random_frames(3), lens9, nk, (47, 61), want_flags=True, want_map=True, want_frames=False)
    assert out is None and np.array_equal(flags, wf) and np.array_equal(qmap, wm)
    out, flags, qmap = _native.undistort_frames(random_frames(3), lens9, nk, (47, 61), want_flags=True, want_frames=False)
    assert out is None and qmap is None and np.array_equal(flags, wf)


def test_wide_frame_whose_tiles_span_many_source_rows(torch):
    """One 300 x 2100 x 3 frame under a strong barrel: a 256-pixel tile row of the destination bends over many source rows."""
    H, W = 300, 2100
    frame = np.random.default_rng(5).integers(0, 256, size=(1, H, W, 3), dtype=np.uint8)
    lens9 = (700.0, 700.0, 1049.3, 149.6, -0.22, 0.03, 1e-3, -5e-4, 0.0)
    nk = (560.0, 560.0, 1050.0, 150.0)
    want, wf, wm = undistort_oracle(frame, lens9, nk, (H, W))
    rows = wm[..., 1] >> 5
    span = max(int(rows[y, x0:x0 + TC].max() - rows[y, x0:x0 + TC].min()) for y in (0, H - 1) for x0 in range(0, W, TC))
    assert span >= 16 and np.any(wf & OUTSIDE) and not np.all(wf & OUTSIDE)
    got, flags, qmap = imaging.undistort_frames(frame, Lens(*lens9), nk, want_flags=True, want_map=True)
    assert np.array_equal(got, want) and np.array_equal(flags, wf) and np.array_equal(qmap, wm)
    got = imaging.undistort_frames(torch.from_numpy(frame).cuda(), Lens(*lens9), nk)
    assert np.array_equal(got.cpu().numpy(), want)


def test_sources_too_narrow_for_a_pair_of_pixels(torch):
    """A source one column wide is read tap by tap (two neighbouring pixels cannot be read together); one row high, or two columns
    wide, it is the narrowest that takes the usual path."""
    rng = np.random.default_rng(11)
    for shape in ((2, 9, 1, 3), (2, 1, 9, 3), (2, 1, 1, 1), (2, 7, 2, 4)):
        frames = rng.integers(0, 256, size=shape, dtype=np.uint8)
        H, W = shape[1:3]
        lens9 = (6.0, 6.0, (W - 1) / 2 + 0.3, (H - 1) / 2 - 0.2, -0.05, 0.01, 0, 0, 0)
        nk = (5.0, 5.0, 5.5, 4.5)
        for nearest in (False, True):
            want, wf, _ = undistort_oracle(frames, lens9, nk, (10, 12), border=33, nearest=nearest)
            assert np.any(wf & OUTSIDE) and (not nearest or not np.all(wf & OUTSIDE))      # bilinear in one column always needs a second
            kw = dict(interpolation="nearest" if nearest else "linear", border_value=33)
            assert np.array_equal(imaging.undistort_frames(frames, Lens(*lens9), nk, (12, 10), **kw), want), (shape, nearest, "host")
            got = imaging.undistort_frames(torch.from_numpy(frames).cuda(), Lens(*lens9), nk, (12, 10), **kw)
            assert np.array_equal(got.cpu().numpy(), want), (shape, nearest, "device")


# ----------------------------------------------------------------------------- 5. the C ABI's errors
def test_every_cabi_error_is_reported_and_leaves_out_untouched():
    lib = _native.load()
    frames = np.ascontiguousarray(random_frames(3))
    B, H, W, C = frames.shape
    good_lens = LENSES["barrel"][0]
    nan, inf = float("nan"), float("inf")

    def call(n_frames=B, height=H, width=W, channels=C, row_pitch=W * C, frame_pitch=H * W * C, lens=good_lens, new_k=(F, F, CX, CY),
             out_h=H, out_w=W, out_row_pitch=None, out_frame_pitch=None, interpolation=0, border=0, null_frames=False, null_out=False,
             want_flags=False):
        out = np.full((B, 47, 61, C), SENTINEL, np.uint8)
        ls = None if lens is None else ctypes.byref(_native.LensStruct(*lens))
        nk = None if new_k is None else np.array(new_k, dtype=np.float64)
        opts = _native.UndistortOpts()
        opts.interpolation, opts.border_value = interpolation, border
        orp = max(out_w, 0) * channels if out_row_pitch is None else out_row_pitch
        ofp = max(out_h, 0) * orp if out_frame_pitch is None else out_frame_pitch
        flags = np.full((47, 61), SENTINEL, np.uint8)
        rc = lib.sba_undistort_frames(0, None if null_frames else ctypes.c_void_p(frames.ctypes.data), n_frames, height, width, channels,
                                      row_pitch, frame_pitch, ls, _native._dptr(nk), out_h, out_w, orp, ofp, ctypes.byref(opts),
                                      None if null_out else ctypes.c_void_p(out.ctypes.data), flags.ctypes.data if want_flags else None, None)
        msg = (lib.sba_last_error(None) or b"").decode()
        assert np.all(out == SENTINEL) or rc == 0, "a failed call wrote into out"
        assert np.all(flags == SENTINEL) or rc == 0, "a failed call wrote into flags_out"
        return rc, msg

    assert call()[0] == 0                                       # the defaults of this helper are a valid call
    assert call(null_out=True, want_flags=True)[0] == 0
    invalid = [
        dict(null_frames=True), dict(n_frames=-1), dict(height=-1), dict(width=-1), dict(channels=2), dict(channels=0),
        dict(row_pitch=W * C - 1), dict(frame_pitch=H * W * C - 1),
        dict(lens=None), dict(new_k=None),
        dict(lens=good_lens[:4] + (nan,) + good_lens[5:]), dict(lens=(inf,) + good_lens[1:]), dict(lens=good_lens[:8] + (nan,)),
        dict(new_k=(F, F, nan, CY)), dict(new_k=(F, inf, CX, CY)),
        dict(lens=(0.0,) + good_lens[1:]), dict(lens=(F, -F) + good_lens[2:]), dict(new_k=(0.0, F, CX, CY)), dict(new_k=(F, -1.0, CX, CY)),
        dict(out_h=-1), dict(out_w=-1), dict(out_h=16385), dict(out_w=16385),
        dict(out_row_pitch=W * C - 1), dict(out_frame_pitch=H * W * C - 1),
        dict(interpolation=2), dict(interpolation=-1), dict(border=256), dict(border=-1),
        dict(null_out=True),
    ]
    seen = set()
    for kw in invalid:
        for want_flags in ((False,) if kw == dict(null_out=True) else (False, True)):
            rc, msg = call(want_flags=want_flags, **kw)
            assert rc == -1 and msg.startswith("sba_undistort_frames: ") and len(msg) > 25, (kw, rc, msg)
        seen.add(msg)
    assert len(seen) >= 15                                       # the texts tell the errors apart
    rc, msg = call(height=16385, frame_pitch=16385 * W * C, null_frames=False, n_frames=0)
    assert rc == -6 and "16384" in msg                            # the detectors' size limit keeps its own status
    with pytest.raises(_native.SbaError, match="sba_undistort_frames"):
        _native.undistort_frames(frames, (F, F, CX, CY, 0, 0, 0, 0, inf), (F, F, CX, CY), (47, 61))
