"""GPU tests of sba_undistort_yuv (include/sba_hip.h) through ``lasercalib_amd.imaging`` and the raw C ABI.

The reference is ``undistort_yuv_oracle`` of tests/test_undistort_yuv_host.py, the header's rule in numpy (pinned there to
answers known without it).  The rule is IEEE float64 operation by operation followed by integer arithmetic, so EVERY comparison
here is bit equality -- the three planes, flags and map; nothing needs a tolerance.  Buffers with padding are pre-filled with a
sentinel and compared whole, so a byte written into the padding (or between two samples of a plane with a step of two) shows.
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
from test_gpu_convert import SENTINEL  # noqa: E402
from test_gpu_yuv import on_device, target  # noqa: E402
from test_undistort_host import CX, CY, F, LENSES, undistort_oracle  # noqa: E402
from test_undistort_yuv_host import undistort_yuv_oracle  # noqa: E402

FORMATS = ("nv12", "nv21", "i420", "yv12")
TR, TC, GROUPS = _native.UNDIST_YUV_TILE_ROWS, _native.UNDIST_YUV_TILE_COLS, _native.UNDIST_YUV_GROUPS
BORDER = (7, 99, 201)
# misalignments of (y, first chroma plane, second chroma plane), handed round both sides
BASES = [((1, 5, 15), (3, 9, 6)), ((15, 0, 1), (5, 2, 11)), ((4, 8, 12), (8, 4, 0)), ((0, 0, 0), (13, 7, 1))]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert _native.device_count() > 0, "no HIP device visible: GPU tests must run on the MI355X box"


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def test_the_constants_are_the_kernels():
    src = open(os.path.join(os.path.dirname(_native.__file__), "csrc", "sba_undistort_yuv.hpp")).read()
    assert "constexpr int UY_TILE_COLS = 128, UY_TILE_ROWS = 2 * DOT_WAVES;" in src and "constexpr int64_t UY_GROUPS = 2048;" in src
    assert (TR, TC, GROUPS) == (8, 128, 2048)


# ----------------------------------------------------------------------------- planes, oracles, layouts
PLANES, ORACLE = {}, {}


def random_planes(B, H, W):
    """Uniform random (y, u, v) of B frames of W x H; shared, never written."""
    key = (B, H, W)
    if key not in PLANES:
        rng = np.random.default_rng(1000 * H + W + B)
        ch, cw = (H + 1) // 2, (W + 1) // 2
        PLANES[key] = tuple(rng.integers(0, 256, size=s, dtype=np.uint8) for s in ((B, H, W), (B, ch, cw), (B, ch, cw)))
        for p in PLANES[key]:
            p.setflags(write=False)
    return PLANES[key]


def oracle_of(B, H, W, lens, new_k, out_hw, border=BORDER, nearest=False):
    key = (B, H, W, tuple(lens), tuple(new_k), tuple(out_hw), tuple(border), nearest)
    if key not in ORACLE:
        ORACLE[key] = undistort_yuv_oracle(*random_planes(B, H, W), lens, new_k, out_hw, border=border, nearest=nearest)
        for p in ORACLE[key]:
            p.setflags(write=False)
    return ORACLE[key]


def in_order(fmt, planes):
    """(y, u, v) as the tuple of arrays `fmt` is handed over in."""
    y, u, v = planes
    if fmt in ("nv12", "nv21"):
        return y, np.stack((u, v) if fmt == "nv12" else (v, u), axis=-1)
    return (y, u, v) if fmt == "i420" else (y, v, u)


def check(torch, planes, fmt_in, fmt_out, lens9, nk, out_hw, want, border=BORDER, nearest=False, src_slack=(0, 0, 0), src_bases=(0, 0, 0),
          slack=(0, 0, 0), bases=(0, 0, 0), device_in=False, device_out=False, **kw):
    """One call from planes in the given layout into sentinel-filled planes of the given layout; planes and padding bit-equal."""
    B, H, W = planes[0].shape
    Ho, Wo = out_hw
    src = target(fmt_in, B, H, W, src_slack, src_bases, planes)
    before = [p[0].copy() for p in src]
    parts = target(fmt_out, B, Ho, Wo, slack, bases)
    expect = [p[0] for p in target(fmt_out, B, Ho, Wo, slack, bases, want)]
    if device_in:
        skeep, sviews = on_device(torch, src)
        assert all(v.data_ptr() % 16 == b % 16 for v, b in zip(sviews, src_bases))
    else:
        sviews = tuple(p[1] for p in src)
    if device_out:
        keep, views = on_device(torch, parts)
    else:
        views = tuple(p[1] for p in parts)
    ret = imaging.undistort_yuv(sviews, fmt_in, Lens(*lens9), nk, (Wo, Ho), interpolation="nearest" if nearest else "linear", border=border,
                                out_pixel_format=fmt_out, out=views, **kw)
    assert ret is views
    got = [t.cpu().numpy() for t in keep] if device_out else [p[0] for p in parts]
    after = [t.cpu().numpy() for t in skeep] if device_in else [p[0] for p in src]
    assert all(np.array_equal(a, b) for a, b in zip(after, before)), "the source was written"
    for k, (g, e) in enumerate(zip(got, expect)):
        if not np.array_equal(g, e):
            bad = np.flatnonzero(g != e)
            raise AssertionError(f"{fmt_in} -> {fmt_out} {W} x {H} -> {Wo} x {Ho} (nearest {nearest}), in {'device' if device_in else 'host'} "
                                 f"{src_slack} + {src_bases}, out {'device' if device_out else 'host'} {slack} + {bases}: plane {k}: "
                                 f"{bad.size} bytes differ, the first at {bad[0]} (got {g[bad[0]]}, expected {e[bad[0]]})")


# ----------------------------------------------------------------------------- 1. lenses, formats, layouts
@pytest.mark.parametrize("name", list(LENSES))
def test_every_lens_and_interpolation(torch, name):
    lens9, nk = LENSES[name]
    for (H, W), out_hw in (((47, 61), (40, 70)), ((48, 64), (37, 53))):
        planes = random_planes(3, H, W)
        for nearest in (False, True):
            want = oracle_of(3, H, W, lens9, nk, out_hw, nearest=nearest)
            check(torch, planes, "nv12", "nv12", lens9, nk, out_hw, want, nearest=nearest)
            check(torch, planes, "i420", "i420", lens9, nk, out_hw, want, nearest=nearest, src_slack=(5, 3, 13), src_bases=(3, 9, 6),
                  slack=(7, 5, 9), bases=(1, 5, 15), device_in=True, device_out=True)
    if name == "identity":
        planes = random_planes(3, 47, 61)
        assert all(np.array_equal(a, b) for a, b in zip(oracle_of(3, 47, 61, lens9, nk, (47, 61)), planes))


@pytest.mark.parametrize("fmt_out", FORMATS)
@pytest.mark.parametrize("fmt_in", FORMATS)
def test_every_pair_of_formats(torch, fmt_in, fmt_out):
    lens9, nk = LENSES["barrel"]
    planes = random_planes(3, 47, 61)
    want = oracle_of(3, 47, 61, lens9, nk, (37, 53))
    check(torch, planes, fmt_in, fmt_out, lens9, nk, (37, 53), want)
    check(torch, planes, fmt_in, fmt_out, lens9, nk, (37, 53), want, src_slack=(5, 3, 13), src_bases=(1, 5, 15), slack=(7, 5, 9), bases=(3, 9, 6),
          device_in=True, device_out=True)


@pytest.mark.parametrize("device_out", [False, True], ids=["to host", "to device"])
@pytest.mark.parametrize("device_in", [False, True], ids=["from host", "from device"])
def test_host_and_device_memory_with_misaligned_padded_planes(torch, device_in, device_out):
    lens9, nk = LENSES["pincushion"]
    planes = random_planes(3, 47, 61)
    for k, (fmt_in, fmt_out) in enumerate((("nv12", "i420"), ("yv12", "nv21"), ("i420", "i420"), ("nv21", "nv12"))):
        want = oracle_of(3, 47, 61, lens9, nk, (37, 53), nearest=bool(k % 2))
        src_bases, bases = BASES[k]
        check(torch, planes, fmt_in, fmt_out, lens9, nk, (37, 53), want, nearest=bool(k % 2), src_slack=(7, 9, 5), src_bases=src_bases,
              slack=(5, 3, 13), bases=bases, device_in=device_in, device_out=device_out)
    # pitches that are multiples of 16 on every plane: every row of every plane on the 16-byte path
    want = oracle_of(3, 47, 61, lens9, nk, (37, 53))
    for fmt in ("nv12", "i420"):
        check(torch, planes, fmt, fmt, lens9, nk, (37, 53), want, slack=(11, 16 - (2 * 27 if fmt == "nv12" else 27) % 16, 16),
              device_in=device_in, device_out=device_out)
    # a result allocated by the call lies on the side of the frames: a tuple for an odd size, stacked frames for an even one
    src = in_order("nv12", planes)
    src = tuple(torch.from_numpy(np.array(p)).cuda() for p in src) if device_in else src
    got = imaging.undistort_yuv(src, "nv12", Lens(*lens9), nk, (53, 37), border=BORDER, out_pixel_format="yv12")
    assert isinstance(got, tuple) and len(got) == 3
    assert all((p.is_cuda and p.dtype == torch.uint8) if device_in else isinstance(p, np.ndarray) for p in got)
    assert all(np.array_equal(p.cpu().numpy() if device_in else p, w) for p, w in zip(got, in_order("yv12", want)))
    got = imaging.undistort_yuv(src, "nv12", Lens(*lens9), nk, (52, 36), border=BORDER)
    got = got.cpu().numpy() if device_in else got
    w = in_order("nv12", oracle_of(3, 47, 61, lens9, nk, (36, 52)))
    assert got.shape == (3, 54, 52) and np.array_equal(got[:, :36], w[0]) and np.array_equal(got[:, 36:].reshape(3, 18, 26, 2), w[1])


def test_chroma_planes_of_their_own_with_a_step_of_two(torch):
    """u and v two bytes apart in planes of their own (not the halves of one interleaved plane), on both sides: the source is
    read sample by sample, the bytes between two samples of the result stay."""
    lens9, nk = LENSES["barrel"]
    B, H, W, out_hw = 3, 47, 61, (37, 53)
    y, u, v = random_planes(B, H, W)
    for nearest in (False, True):
        wy, wu, wv = oracle_of(B, H, W, lens9, nk, out_hw, nearest=nearest)
        for device in (False, True):
            rng = np.random.default_rng(3)
            su, sv = (rng.integers(0, 256, size=(B, 24, 31, 2), dtype=np.uint8) for _ in range(2))      # noise between the samples
            su[..., 0], sv[..., 0] = u, v
            wide_u, wide_v, got_y = (np.full(s, SENTINEL, np.uint8) for s in ((B, 19, 27, 2), (B, 19, 27, 2), (B, 37, 53)))
            sy = np.array(y)
            if device:
                su, sv, sy, wide_u, wide_v, got_y = (torch.from_numpy(a).cuda() for a in (su, sv, sy, wide_u, wide_v, got_y))
            for chunk in (0, 1, 2):
                imaging.undistort_yuv((sy, su[..., 0], sv[..., 0]), "i420", Lens(*lens9), nk, (53, 37), border=BORDER,
                                      interpolation="nearest" if nearest else "linear", out=(got_y, wide_u[..., 0], wide_v[..., 0]),
                                      chunk_frames=chunk)
                a, b, c = (t.cpu().numpy() if device else t for t in (got_y, wide_u, wide_v))
                assert np.array_equal(a, wy) and np.array_equal(b[..., 0], wu) and np.array_equal(c[..., 0], wv), (nearest, device, chunk)
                assert np.all(b[..., 1] == SENTINEL) and np.all(c[..., 1] == SENTINEL), "a byte between two samples was written"
    # the halves of one plane handed over as planar planes are read and written as that plane
    wy, wu, wv = oracle_of(B, H, W, lens9, nk, out_hw)
    pair_in, pair = np.stack((v, u), axis=-1), np.full((B, 19, 27, 2), SENTINEL, np.uint8)
    imaging.undistort_yuv((y, pair_in[..., 1], pair_in[..., 0]), "i420", Lens(*lens9), nk, (53, 37), border=BORDER,
                          out=(np.empty((B, 37, 53), np.uint8), pair[..., 1], pair[..., 0]))
    assert np.array_equal(pair[..., 1], wu) and np.array_equal(pair[..., 0], wv)


# ----------------------------------------------------------------------------- 2. boundaries of the tile and of the stores
@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_output_widths_around_vectors_waves_and_tiles(torch, fmt):
    """Luma widths 1, 2, 15 / 16 / 17 (one 16-byte store), 31 / 33 (a planar chroma row around one), 63 / 65 (a wave), 127 / 128 /
    129 (the tile of TC = 128 columns) and 255 / 257 (two tiles), odd ones included: the last chroma sample stands alone."""
    assert TC == 128
    lens9, _ = LENSES["pincushion"]
    planes = random_planes(2, 47, 61)
    for k, w in enumerate((1, 2, 15, 16, 17, 31, 33, 63, 65, TC - 1, TC, TC + 1, 2 * TC - 1, 2 * TC + 1)):
        nk = (F * w / 61, F, 31.0 * w / 61, 22.5)
        nearest = bool(k % 2)
        src_bases, bases = BASES[k % 4]
        check(torch, planes, fmt, fmt, lens9, nk, (5, w), oracle_of(2, 47, 61, lens9, nk, (5, w), nearest=nearest), nearest=nearest,
              src_slack=(5, 3, 13), src_bases=src_bases, slack=(7, 5, 9), bases=bases, device_in=True, device_out=True)


def test_output_heights_around_the_tile(torch):
    assert TR == 8
    lens9, _ = LENSES["barrel"]
    planes = random_planes(2, 47, 61)
    for k, h in enumerate((1, 2, 3, TR - 1, TR, TR + 1, 2 * TR - 1, 2 * TR, 2 * TR + 1)):
        nk = (F, F * h / 47, CX, CY * h / 47)
        fmt = FORMATS[k % 4]
        check(torch, planes, fmt, fmt, lens9, nk, (h, 61), oracle_of(2, 47, 61, lens9, nk, (h, 61)), slack=(7, 5, 9), bases=BASES[k % 4][1],
              device_in=True, device_out=True)


def test_small_sources_take_the_tap_by_tap_fallbacks(torch):
    """A luma plane one column wide, and a chroma plane one column wide (luma up to two), cannot be read as pairs of neighbouring
    samples: 1 x 1, 2 x 2, 1 x 9 take the fallback of both, 3 x 1, 4 x 2, 9 x 1 the usual path of both or of luma alone."""
    for W, H in ((1, 1), (2, 2), (3, 1), (4, 2), (1, 9), (9, 1)):
        planes = random_planes(2, H, W)
        lens9 = (6.0, 6.0, (W - 1) / 2 + 0.3, (H - 1) / 2 - 0.2, -0.05, 0.01, 0, 0, 0)
        nk = (5.0, 5.0, 5.5, 4.5)
        for nearest in (False, True):
            want = oracle_of(2, H, W, lens9, nk, (10, 12), border=(33, 66, 99), nearest=nearest)
            _o, flags, _m = undistort_oracle(planes[0][..., None], lens9, nk, (10, 12))
            assert np.any(flags & 1) and not np.all(want[0] == 33)
            for k, fmt in enumerate(FORMATS):
                check(torch, planes, fmt, FORMATS[(k + 1) % 4], lens9, nk, (10, 12), want, border=(33, 66, 99), nearest=nearest,
                      device_in=bool(k % 2), device_out=bool(k % 2))
        # planes of their own with a step of two: the fallback reads sample by sample too
        y, u, v = planes
        ch, cw = u.shape[1:]
        su, sv = (np.full((2, ch, cw, 2), SENTINEL, np.uint8) for _ in range(2))
        su[..., 0], sv[..., 0] = u, v
        got = imaging.undistort_yuv((y, su[..., 0], sv[..., 0]), "i420", Lens(*lens9), nk, (12, 10), border=(33, 66, 99))      # stacked: even
        want = oracle_of(2, H, W, lens9, nk, (10, 12), border=(33, 66, 99))
        assert np.array_equal(got.reshape(2, -1), np.concatenate([p.reshape(2, -1) for p in want], axis=1)), (W, H)


def test_wide_frame_under_a_strong_barrel(torch):
    """One 2100 x 300 frame under a strong barrel: a tile row of the destination bends over many source rows."""
    H, W = 300, 2100
    planes = random_planes(1, H, W)
    lens9 = (700.0, 700.0, 1049.3, 149.6, -0.22, 0.03, 1e-3, -5e-4, 0.0)
    nk = (560.0, 560.0, 1050.0, 150.0)
    want = oracle_of(1, H, W, lens9, nk, (H, W))
    _o, wf, wm = undistort_oracle(planes[0][..., None], lens9, nk, (H, W), border=BORDER[0])
    rows = wm[..., 1] >> 5
    span = max(int(rows[y, x0:x0 + TC].max() - rows[y, x0:x0 + TC].min()) for y in (0, H - 1) for x0 in range(0, W, TC))
    assert span >= 8 and np.any(wf & 1) and not np.all(wf & 1)
    got, flags, qmap = imaging.undistort_yuv(in_order("nv12", planes), "nv12", Lens(*lens9), nk, border=BORDER, want_flags=True, want_map=True)
    assert got.shape == (1, 450, 2100) and np.array_equal(flags, wf) and np.array_equal(qmap, wm)
    assert np.array_equal(got[:, :H], want[0]) and np.array_equal(got[:, H:].reshape(1, 150, 1050, 2), np.stack(want[1:], axis=-1))
    dev = tuple(torch.from_numpy(np.array(p)).cuda() for p in in_order("i420", planes))
    got = imaging.undistort_yuv(dev, "i420", Lens(*lens9), nk, border=BORDER).cpu().numpy()
    assert np.array_equal(got.reshape(1, -1), np.concatenate([p.reshape(1, -1) for p in want], axis=1))


# ----------------------------------------------------------------------------- 3. chunking and the frame loop
@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_any_chunk_size_gives_the_same_bits(torch, fmt):
    lens9, nk = LENSES["barrel"]
    planes = random_planes(5, 47, 61)
    want = oracle_of(5, 47, 61, lens9, nk, (37, 53))
    for chunk in (1, 2, 0, 5, 7):
        for device in (False, True):
            check(torch, planes, fmt, fmt, lens9, nk, (37, 53), want, device_in=device, device_out=device, chunk_frames=chunk)
    # host planes in each class of layout a pitched copy tells apart, in three chunks, the last one short: both staging buffers
    # are used twice, the padding stays
    for row_slack, frame_slack in ((5, 0), (0, 13), (5, 13)):
        check(torch, planes, fmt, fmt, lens9, nk, (37, 53), want, src_slack=(row_slack, row_slack, frame_slack), src_bases=(3, 9, 6),
              slack=(row_slack and row_slack + 2, row_slack, frame_slack and frame_slack - 4), bases=(5, 1, 2), chunk_frames=2)
    # a host source into a device result and back
    check(torch, planes, fmt, fmt, lens9, nk, (37, 53), want, device_out=True, chunk_frames=2)
    check(torch, planes, fmt, fmt, lens9, nk, (37, 53), want, device_in=True, chunk_frames=3)


def test_a_workgroup_walks_several_frames_of_its_chunk(torch):
    """A launch aims at GROUPS = 2048 workgroups: 3 * GROUPS + 1 frames of one tile each give every workgroup
    ceil(6145 / 2048) = 4 frames of the chunk to walk (the last one a single frame)."""
    assert GROUPS == 2048
    B = 3 * GROUPS + 1
    H, W, out_hw = 6, 8, (5, 9)
    assert out_hw[0] <= TR and out_hw[1] <= TC and -(-B // GROUPS) >= 3
    lens9 = (10.0, 10.0, 3.6, 2.4, -0.1, 0.01, 0, 0, 0)
    nk = (9.0, 9.0, 4.1, 2.2)
    planes = random_planes(B, H, W)
    want = oracle_of(B, H, W, lens9, nk, out_hw)
    check(torch, planes, "nv12", "nv12", lens9, nk, out_hw, want, device_in=True, device_out=True)
    check(torch, planes, "i420", "nv21", lens9, nk, out_hw, want)
    assert not np.array_equal(want[0][0], want[0][1]) and not np.array_equal(want[1][B - 2], want[1][B - 1])


# ----------------------------------------------------------------------------- 4. diagnostics, identity, the existing call
def test_no_frames_and_no_out_still_give_flags_and_map(torch):
    lens9, nk = LENSES["folded"]
    planes = random_planes(3, 47, 61)
    _o, wf, wm = undistort_oracle(planes[0][..., None], lens9, nk, (40, 70))
    empty = tuple(p[:0] for p in in_order("nv12", planes))
    out, flags, qmap = imaging.undistort_yuv(empty, "nv12", Lens(*lens9), nk, (70, 40), want_flags=True, want_map=True)
    assert out.shape == (0, 60, 70) and np.array_equal(flags, wf) and np.array_equal(qmap, wm)
    assert flags.dtype == np.uint8 and qmap.dtype == np.int32
    out, flags, qmap = _native.undistort_yuv(in_order("i420", planes), "i420", lens9, nk, (40, 70), want_map=True, want_frames=False)
    assert out is None and flags is None and np.array_equal(qmap, wm)
    # the same as the existing call's for the same geometry
    _o, ff, fm = _native.undistort_frames(np.array(planes[0]), lens9, nk, (40, 70), want_flags=True, want_map=True, want_frames=False)
    out, flags, qmap = _native.undistort_yuv(in_order("i420", planes), "i420", lens9, nk, (40, 70), want_flags=True, want_map=True,
                                             want_frames=False)
    assert out is None and np.array_equal(flags, ff) and np.array_equal(qmap, fm)
    # an output without pixels
    assert imaging.undistort_yuv(in_order("i420", planes), "i420", Lens(*lens9), nk, (0, 0)).shape == (3, 0, 0)


def test_identity_lens_returns_the_input(torch):
    for H, W in ((48, 64), (47, 61), (2 * TR + 3, 2 * TC + 5)):
        planes = random_planes(2, H, W)
        lens = Lens(F, 1.1 * F, CX * W / 61, CY * H / 47)
        for fmt in FORMATS:
            src = in_order(fmt, planes)
            for interpolation in ("linear", "nearest"):
                got = imaging.undistort_yuv(src, fmt, lens, interpolation=interpolation)
                got = got if isinstance(got, tuple) else (got,)
                flat = np.concatenate([p.reshape(2, -1) for p in got], axis=1)
                assert np.array_equal(flat, np.concatenate([p.reshape(2, -1) for p in src], axis=1)), (H, W, fmt, interpolation)
        dev = tuple(torch.from_numpy(np.array(p)).cuda() for p in in_order("nv12", planes))
        got = imaging.undistort_yuv(dev, "nv12", lens)
        got = got if isinstance(got, tuple) else (got,)
        flat = np.concatenate([p.cpu().numpy().reshape(2, -1) for p in got], axis=1)
        assert np.array_equal(flat, np.concatenate([p.reshape(2, -1) for p in in_order("nv12", planes)], axis=1))


def test_luma_equals_undistort_frames_on_the_y_plane(torch):
    planes = random_planes(3, 47, 61)
    ydev = torch.from_numpy(np.array(planes[0])).cuda()
    dev = tuple(torch.from_numpy(np.array(p)).cuda() for p in in_order("nv12", planes))
    for name in ("rig", "pincushion", "wild"):
        lens9, nk = LENSES[name]
        for interpolation in ("linear", "nearest"):
            one = imaging.undistort_frames(ydev, Lens(*lens9), nk, (70, 40), interpolation=interpolation, border_value=BORDER[0])
            got = imaging.undistort_yuv(dev, "nv12", Lens(*lens9), nk, (70, 40), interpolation=interpolation, border=BORDER)
            assert tuple(one.shape) == (3, 40, 70) and np.array_equal(got[:, :40].cpu().numpy(), one.cpu().numpy()), (name, interpolation)


# ----------------------------------------------------------------------------- 5. the C ABI's errors
def test_every_cabi_error_is_reported_and_leaves_the_planes_untouched():
    lib = _native.load()
    B, H, W = 3, 47, 61
    ch, cw = 24, 31
    y, u, v = (np.ascontiguousarray(p) for p in random_planes(B, H, W))
    good_lens = LENSES["barrel"][0]
    nan, inf = float("nan"), float("inf")
    i420 = dict(y_row_pitch=W, y_frame_pitch=H * W, c_row_pitch=cw, c_frame_pitch=ch * cw, c_step=1)

    def call(n_frames=B, height=H, width=W, lens=good_lens, new_k=(F, F, CX, CY), out_h=H, out_w=W, src=None, out=None, interpolation=0,
             border=(0, 0, 0), null_src=False, null_out=False, null_plane=None, want_flags=False):
        oy, ou, ov = (np.full(s, SENTINEL, np.uint8) for s in ((B, H, W), (B, ch, cw), (B, ch, cw)))
        flags = np.full((H, W), SENTINEL, np.uint8)
        s, o = dict(i420), dict(i420)
        s.update(src or {})
        o.update(out or {})
        sp = [y.ctypes.data, u.ctypes.data, v.ctypes.data]
        op = [oy.ctypes.data, ou.ctypes.data, ov.ctypes.data]
        if null_plane is not None:
            (sp if null_plane[0] == "src" else op)[null_plane[1]] = None
        S = _native.YuvPlanes(*sp, s["y_row_pitch"], s["y_frame_pitch"], s["c_row_pitch"], s["c_frame_pitch"], s["c_step"], 0)
        D = _native.YuvPlanes(*op, o["y_row_pitch"], o["y_frame_pitch"], o["c_row_pitch"], o["c_frame_pitch"], o["c_step"], 0)
        ls = None if lens is None else ctypes.byref(_native.LensStruct(*lens))
        nk = None if new_k is None else np.array(new_k, dtype=np.float64)
        opts = _native.UndistortYuvOpts()
        opts.interpolation, (opts.border_y, opts.border_u, opts.border_v) = interpolation, border
        rc = lib.sba_undistort_yuv(0, None if null_src else ctypes.byref(S), n_frames, height, width, ls, _native._dptr(nk), out_h, out_w,
                                   None if null_out else ctypes.byref(D), ctypes.byref(opts), flags.ctypes.data if want_flags else None, None)
        msg = (lib.sba_last_error(None) or b"").decode()
        assert rc == 0 or all(np.all(p == SENTINEL) for p in (oy, ou, ov)), "a failed call wrote into a plane"
        assert rc == 0 or np.all(flags == SENTINEL), "a failed call wrote into flags_out"
        return rc, msg

    assert call()[0] == 0                                       # the defaults of this helper are a valid call
    assert call(null_out=True, want_flags=True)[0] == 0
    invalid = [
        dict(null_src=True), dict(n_frames=-1), dict(height=-1), dict(width=-1),
        dict(null_plane=("src", 0)), dict(null_plane=("src", 1)), dict(null_plane=("src", 2)),
        dict(src=dict(c_step=0)), dict(src=dict(c_step=3)),
        dict(src=dict(y_row_pitch=W - 1)), dict(src=dict(y_frame_pitch=H * W - 1)), dict(src=dict(c_row_pitch=cw - 1)),
        dict(src=dict(c_step=2)),                                # a step of two needs 2 * (cw - 1) + 1 bytes a row
        dict(src=dict(c_frame_pitch=ch * cw - 1)), dict(src=dict(c_row_pitch=-1)),
        dict(src=dict(y_frame_pitch=1 << 62)), dict(src=dict(c_frame_pitch=1 << 62)),
        dict(lens=None), dict(new_k=None),
        dict(lens=good_lens[:4] + (nan,) + good_lens[5:]), dict(lens=(inf,) + good_lens[1:]), dict(lens=good_lens[:8] + (nan,)),
        dict(new_k=(F, F, nan, CY)), dict(new_k=(F, inf, CX, CY)),
        dict(lens=(0.0,) + good_lens[1:]), dict(lens=(F, -F) + good_lens[2:]), dict(new_k=(0.0, F, CX, CY)), dict(new_k=(F, -1.0, CX, CY)),
        dict(out_h=-1), dict(out_w=-1), dict(out_h=16385), dict(out_w=16385),
        dict(interpolation=2), dict(interpolation=-1),
        dict(border=(256, 0, 0)), dict(border=(0, 256, 0)), dict(border=(0, 0, 256)), dict(border=(-1, 0, 0)), dict(border=(0, -1, 0)),
        dict(border=(0, 0, -1)),
        dict(null_plane=("out", 0)), dict(null_plane=("out", 1)), dict(null_plane=("out", 2)),
        dict(out=dict(c_step=0)), dict(out=dict(c_step=3)), dict(out=dict(c_step=2)),
        dict(out=dict(y_row_pitch=W - 1)), dict(out=dict(y_frame_pitch=H * W - 1)), dict(out=dict(c_row_pitch=cw - 1)),
        dict(out=dict(c_frame_pitch=ch * cw - 1)), dict(out=dict(y_frame_pitch=1 << 62)),
        dict(out_w=W + 1), dict(out_h=H + 1),                   # the planes of the result are too small for that size
        dict(null_out=True),
    ]
    seen = set()
    for kw in invalid:
        for want_flags in ((False,) if kw == dict(null_out=True) else (False, True)):
            rc, msg = call(want_flags=want_flags, **kw)
            assert rc == -1 and msg.startswith("sba_undistort_yuv: ") and len(msg) > 25, (kw, rc, msg)
        seen.add(msg)
    assert len(seen) >= 22                                       # the texts tell the errors apart, and the two sides
    rc, msg = call(height=16385, src=dict(y_frame_pitch=16385 * W, c_frame_pitch=8193 * cw), n_frames=0)
    assert rc == -6 and "16384" in msg                            # the size limit keeps its own status
    rc, msg = call(width=16386, src=dict(y_row_pitch=16386, y_frame_pitch=16386 * H, c_row_pitch=8193, c_frame_pitch=8193 * ch), n_frames=0)
    assert rc == -6 and "16384" in msg
    with pytest.raises(_native.SbaError, match="sba_undistort_yuv"):
        _native.undistort_yuv((y, u, v), "i420", (F, F, CX, CY, 0, 0, 0, 0, inf), (F, F, CX, CY), (47, 61))
