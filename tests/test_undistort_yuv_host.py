"""CPU tests of the plane-by-plane undistortion of YUV 4:2:0 frames (include/sba_hip.h: sba_undistort_yuv;
lasercalib_amd/imaging.py: undistort_yuv).

``undistort_yuv_oracle`` is the rule of the header restated in numpy: every line of its float64 part is one IEEE operation per
operation of the rule, in the rule's order, and everything behind it is integer arithmetic, so it defines the bytes of the
three planes exactly.  It is the reference of tests/test_gpu_undistort_yuv.py and is pinned here to answers that are known
without it -- an identity lens returns the input, a shift by one luma pixel averages neighbouring chroma samples, a shift by
(2, 2) moves chroma by one sample -- and, for luma, to ``undistort_oracle`` of tests/test_undistort_host.py under every lens
of that file.  The rest covers what runs on the host: the struct layouts against the header's text and every ValueError of
the Python layer.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lasercalib_amd import _native, imaging  # noqa: E402
from lasercalib_amd.imaging import Lens  # noqa: E402
from test_undistort_host import CX, CY, F, LENSES, undistort_oracle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source_position(x, y, lens, new_k):
    """(sx, sy, in_range) of the header's model at the destination positions (x, y), float64 arrays."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = (np.float64(v) for v in lens)
    fxn, fyn, cxn, cyn = (np.float64(v) for v in new_k)
    with np.errstate(over="ignore", invalid="ignore"):
        ifx, ify = 1.0 / fxn, 1.0 / fyn
        xn, yn = (x - cxn) * ifx, (y - cyn) * ify
        x2, y2 = xn * xn, yn * yn
        r2, xy = x2 + y2, xn * yn
        t = r2 * k3; t = k2 + t; t = r2 * t; t = k1 + t; t = r2 * t      # noqa: E702
        rad = 1.0 + t
        xd = xn * rad + ((2.0 * p1) * xy + p2 * (r2 + 2.0 * x2))
        yd = yn * rad + (p1 * (r2 + 2.0 * y2) + (2.0 * p2) * xy)
        sx, sy = fx * xd + cx, fy * yd + cy
        in_range = (sx > -32768) & (sx < 32768) & (sy > -32768) & (sy < 32768)
    return sx, sy, in_range


def _resample(plane, qx, qy, in_range, border, nearest):
    """One (B, H, W) plane at the positions (qx, qy) on its 1/32 grid: the taps, weights and rounding of the header."""
    B, H, W = plane.shape
    if nearest:
        ix, iy = (qx + 16) >> 5, (qy + 16) >> 5
        taps = [(0, 0, np.full(qx.shape, 1024, np.int64))]
    else:
        ix, iy, ax, ay = qx >> 5, qy >> 5, qx & 31, qy & 31
        taps = [(0, 0, (32 - ax) * (32 - ay)), (1, 0, ax * (32 - ay)), (0, 1, (32 - ax) * ay), (1, 1, ax * ay)]
    acc = np.zeros((B,) + qx.shape, np.int64)
    for dx, dy, w in taps:
        tx, ty = ix + dx, iy + dy
        inside = in_range & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        if H and W:
            v = np.where(inside[None], plane[:, np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)].astype(np.int64), border)
        else:
            v = np.full(acc.shape, border, np.int64)
        acc += v * w[None]
    return ((acc + 512) >> 10).astype(np.uint8)


def undistort_yuv_oracle(y, u, v, lens, new_k, out_hw, border=(16, 128, 128), nearest=False):
    """(Y, U, V) of the rule in include/sba_hip.h.  ``y`` (B, H, W), ``u`` and ``v`` (B, (H + 1) // 2, (W + 1) // 2) uint8;
    ``lens`` = (fx, fy, cx, cy, k1, k2, p1, p2, k3), ``new_k`` = (fxn, fyn, cxn, cyn), ``out_hw`` = (height, width),
    ``border`` = (Y, U, V)."""
    Ho, Wo = out_hw
    Hc, Wc = (Ho + 1) // 2, (Wo + 1) // 2
    # luma: whole pixels, the position on the 1/32 grid of the luma plane
    x = np.broadcast_to(np.arange(Wo, dtype=np.float64)[None, :], (Ho, Wo))
    yy = np.broadcast_to(np.arange(Ho, dtype=np.float64)[:, None], (Ho, Wo))
    sx, sy, ok = _source_position(x, yy, lens, new_k)
    qx = np.floor(np.where(ok, sx, 0.0) * 32.0 + 0.5).astype(np.int64)
    qy = np.floor(np.where(ok, sy, 0.0) * 32.0 + 0.5).astype(np.int64)
    Y = _resample(y, qx, qy, ok, border[0], nearest)
    # chroma: the centres of the 2 x 2 blocks, the position on the 1/32 grid of the chroma plane
    x = np.broadcast_to((2.0 * np.arange(Wc, dtype=np.float64) + 0.5)[None, :], (Hc, Wc))
    yy = np.broadcast_to((2.0 * np.arange(Hc, dtype=np.float64) + 0.5)[:, None], (Hc, Wc))
    sx, sy, ok = _source_position(x, yy, lens, new_k)
    with np.errstate(invalid="ignore"):
        mx = sx * 16.0; mx = mx - 8.0; mx = mx + 0.5      # noqa: E702
        my = sy * 16.0; my = my - 8.0; my = my + 0.5      # noqa: E702
        qcx = np.where(ok, np.floor(mx), 0.0).astype(np.int64)
        qcy = np.where(ok, np.floor(my), 0.0).astype(np.int64)
    return Y, _resample(u, qcx, qcy, ok, border[1], nearest), _resample(v, qcx, qcy, ok, border[2], nearest)


def random_planes(B, H, W, seed=0):
    rng = np.random.default_rng(100 * H + W + seed)
    ch, cw = (H + 1) // 2, (W + 1) // 2
    return tuple(rng.integers(0, 256, size=s, dtype=np.uint8) for s in ((B, H, W), (B, ch, cw), (B, ch, cw)))


# ----------------------------------------------------------------------------- the oracle against known answers
@pytest.mark.parametrize("size", [(61, 47), (64, 48), (1, 1), (3, 2)])
def test_oracle_identity_returns_the_input(size):
    W, H = size
    y, u, v = random_planes(2, H, W)
    lens = (F, F, CX * W / 61, CY * H / 47, 0, 0, 0, 0, 0)
    for nearest in (False, True):
        Y, U, V = undistort_yuv_oracle(y, u, v, lens, lens[:4], (H, W), border=(1, 2, 3), nearest=nearest)
        assert np.array_equal(Y, y) and np.array_equal(U, u) and np.array_equal(V, v)


def test_oracle_identity_at_the_size_of_the_rig():
    W, H = 3208, 2200
    y, u, v = random_planes(1, H, W)
    lens = (2388.5, 2391.25, 1552.3, 1080.6, 0, 0, 0, 0, 0)
    Y, U, V = undistort_yuv_oracle(y, u, v, lens, lens[:4], (H, W))
    assert np.array_equal(Y, y) and np.array_equal(U, u) and np.array_equal(V, v)


@pytest.mark.parametrize("name", list(LENSES))
def test_oracle_luma_is_the_one_channel_rule_of_undistort_frames(name):
    lens, nk = LENSES[name]
    y, u, v = random_planes(2, 47, 61)
    for nearest in (False, True):
        Y, _U, _V = undistort_yuv_oracle(y, u, v, lens, nk, (40, 70), border=(7, 99, 201), nearest=nearest)
        want, _f, _m = undistort_oracle(y[..., None], lens, nk, (40, 70), border=7, nearest=nearest)
        assert np.array_equal(Y, want[..., 0])


def test_oracle_shift_by_one_luma_pixel_averages_neighbouring_chroma():
    y, u, v = random_planes(2, 47, 61)
    lens = LENSES["identity"][0]
    Y, U, V = undistort_yuv_oracle(y, u, v, lens, (F, F, CX - 1, CY), (47, 61), border=(9, 50, 200))
    assert np.array_equal(Y[:, :, :-1], y[:, :, 1:]) and np.all(Y[:, :, -1] == 9)
    for got, c, b in ((U, u.astype(int), 50), (V, v.astype(int), 200)):
        assert np.array_equal(got[:, :, :-1], (c[:, :, :-1] + c[:, :, 1:] + 1) >> 1)      # half a chroma sample: weights 512, 512
        assert np.array_equal(got[:, :, -1], (c[:, :, -1] + b + 1) >> 1)


def test_oracle_shift_by_two_moves_chroma_by_one_sample():
    y, u, v = random_planes(2, 47, 61)
    lens = LENSES["identity"][0]
    for nearest in (False, True):
        Y, U, V = undistort_yuv_oracle(y, u, v, lens, (F, F, CX - 2, CY - 2), (47, 61), border=(9, 50, 200), nearest=nearest)
        assert np.array_equal(Y[:, :-2, :-2], y[:, 2:, 2:]) and np.all(Y[:, -2:] == 9) and np.all(Y[:, :, -2:] == 9)
        for got, c, b in ((U, u, 50), (V, v, 200)):
            assert np.array_equal(got[:, :-1, :-1], c[:, 1:, 1:]) and np.all(got[:, -1] == b) and np.all(got[:, :, -1] == b)


def test_oracle_out_of_range_positions_take_the_borders():
    lens, nk = LENSES["wild"]
    y, u, v = random_planes(1, 47, 61)
    Y, U, V = undistort_yuv_oracle(y, u, v, lens, nk, (47, 61), border=(1, 2, 3))
    _o, flags, _m = undistort_oracle(y[..., None], lens, nk, (47, 61))
    bad = (flags & 4) != 0
    assert bad.any() and np.all(Y[0][bad] == 1)
    assert np.any(U == 2) and np.any(V == 3) and U[0, 0, 0] == 2 and V[0, 0, 0] == 3      # the corner block lies out of range too


# ----------------------------------------------------------------------------- struct layouts against the header's text
def header_fields(text, name):
    """The member names of the struct typedef'd as `name`, in order, from the header's text."""
    body = text[:text.index("} " + name + ";")]
    body = re.sub(r"/\*.*?\*/", "", body[body.rindex("typedef struct {") + len("typedef struct {"):], flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[\d+\]", "", n).strip(" *") for n in decl.split(None, 1)[1].split(",")]
    return names


def test_struct_layouts_match_the_header():
    text = open(os.path.join(ROOT, "include", "sba_hip.h")).read()
    assert ctypes.sizeof(_native.YuvPlanes) == 64 and ctypes.sizeof(_native.UndistortYuvOpts) == 48
    assert header_fields(text, "sba_yuv_planes") == [n for n, _t in _native.YuvPlanes._fields_]
    assert header_fields(text, "sba_undistort_yuv_opts") == [n for n, _t in _native.UndistortYuvOpts._fields_]
    assert [n for n, _t in _native.YuvPlanes._fields_] == ["y", "u", "v", "y_row_pitch", "y_frame_pitch", "c_row_pitch", "c_frame_pitch",
                                                          "c_step", "reserved"]
    assert [n for n, _t in _native.UndistortYuvOpts._fields_][:7] == ["frames_on_device", "out_on_device", "interpolation", "border_y",
                                                                     "border_u", "border_v", "chunk_frames"]
    assert _native.YuvPlanes.y_row_pitch.offset == 24 and _native.YuvPlanes.c_step.offset == 56
    assert "sba_undistort_yuv" in _native.EXPORTED_SYMBOLS and re.search(r"#define SBA_ABI_VERSION 2\b", text)
    assert "undistort_yuv" in imaging.__all__


# ----------------------------------------------------------------------------- every ValueError of the Python layer
def test_python_side_value_errors(monkeypatch):
    """Every ValueError is raised before the library is needed: loading it here is an error."""
    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_native, "load", no_library)
    lens = Lens(F, F, CX, CY, -0.1)
    y, u, v = (np.zeros(s, np.uint8) for s in ((2, 47, 61), (2, 24, 31), (2, 24, 31)))
    uv = np.zeros((2, 24, 31, 2), np.uint8)
    stacked = np.zeros((2, 72, 64), np.uint8)
    out_i420 = tuple(np.zeros(s, np.uint8) for s in ((2, 47, 61), (2, 24, 31), (2, 24, 31)))
    read_only = tuple(a.copy() for a in out_i420)
    read_only[1].setflags(write=False)
    bad_calls = [
        dict(pixel_format="yuv444"),
        dict(frames=(y, uv)),                                                     # two planes for a three-plane format
        dict(frames=(y.astype(np.int8), u, v)),                                   # dtype
        dict(frames=(y, u[:, :, :30], v[:, :, :30])),                             # chroma of another size
        dict(frames=(y, u, np.zeros((2, 24, 62), np.uint8)[:, :, ::2])),          # the two chroma planes with different strides
        dict(frames=np.zeros((2, 70, 64), np.uint8)),                             # 70 rows fit no H
        dict(frames=np.zeros((2, 72, 63), np.uint8), pixel_format="nv12"),        # stacked nv12 of an odd width
        dict(lens=(F, F, CX, CY)),                                                # not a Lens
        dict(new_camera_matrix=np.eye(2)),
        dict(new_camera_matrix=np.array([[F, 0.1, CX], [0, F, CY], [0, 0, 1]])),  # skew
        dict(new_camera_matrix=(0.0, F, CX, CY)),
        dict(new_camera_matrix=(F, F, np.nan, CY)),
        dict(out_size=(61,)),
        dict(out_size=(-1, 47)),
        dict(out_size=(16385, 47)),
        dict(interpolation="cubic"),
        dict(border=16), dict(border=(16, 128)), dict(border=(16, 128, 256)), dict(border=(-1, 128, 128)), dict(border=(16, 0.5, 128)),
        dict(out_pixel_format="rgb"),
        dict(out=out_i420[:2]),                                                   # two planes for i420
        dict(out=tuple(a[:1] for a in out_i420)),                                 # another number of frames
        dict(out=out_i420, out_size=(60, 47)),                                    # another size
        dict(out=(out_i420[0], uv), out_pixel_format="i420"),
        dict(out=read_only),
        dict(out=tuple(a.astype(np.int8) for a in out_i420)),
        dict(out=[[0]]),
    ]
    for kw in bad_calls:
        args = dict(frames=(y, u, v), pixel_format="i420", lens=lens)
        args.update(kw)
        with pytest.raises(ValueError):
            imaging.undistort_yuv(**args)
    with pytest.raises(ValueError):
        imaging.undistort_yuv(stacked, "nv12", lens, out=np.zeros((2, 72, 62), np.uint8))      # stacked frames of another width
    nk = (F, F, CX, CY)
    with pytest.raises(ValueError):
        _native.undistort_yuv((y, u, v), "i420", lens.as_tuple(), nk, (47, 61), want_frames=False)          # nothing asked for
    with pytest.raises(ValueError):
        _native.undistort_yuv((y, u, v), "i420", lens.as_tuple(), nk, (47, 61), want_frames=False, want_flags=True, out=out_i420)
