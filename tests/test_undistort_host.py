"""CPU tests of the undistortion (include/sba_hip.h: sba_undistort_frames; lasercalib_amd/imaging.py).

``undistort_oracle`` is the rule of the header restated in numpy: every line of it is one IEEE float64 operation per operation
of the rule, in the rule's order, and everything behind the float64 part is integer arithmetic, so it defines the bytes, the
flags and the map exactly.  It is the reference of tests/test_gpu_undistort.py and is checked here on cases whose answer is
known without it: the identity, a whole-pixel shift, a half-pixel shift, a folding lens and a lens that leaves the range.
The rest of the file covers what runs on the host: the struct layouts, the Lens constructors, every ValueError of the Python
layer and optimal_new_camera_matrix.
"""
import ctypes

import numpy as np
import pytest

from lasercalib_amd import _native, imaging
from lasercalib_amd.imaging import Lens

OUTSIDE, FOLDED, RANGE = 1, 2, 4


def undistort_oracle(frames, lens, new_k, out_hw, border=0, nearest=False):
    """(out, flags, map) of the rule in include/sba_hip.h.  ``frames`` (B, H, W, C) uint8, ``lens`` = (fx, fy, cx, cy, k1, k2,
    p1, p2, k3), ``new_k`` = (fxn, fyn, cxn, cyn), ``out_hw`` = (height, width)."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = (np.float64(v) for v in lens)
    fxn, fyn, cxn, cyn = (np.float64(v) for v in new_k)
    B, H, W, C = frames.shape
    Ho, Wo = out_hw
    x = np.broadcast_to(np.arange(Wo, dtype=np.float64)[None, :], (Ho, Wo))
    y = np.broadcast_to(np.arange(Ho, dtype=np.float64)[:, None], (Ho, Wo))
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
        dp = r2 * (3.0 * k3); dp = (2.0 * k2) + dp; dp = r2 * dp; dp = k1 + dp      # noqa: E702
        j00 = rad + (2.0 * x2) * dp + ((2.0 * p1) * yn + (6.0 * p2) * xn)
        j11 = rad + (2.0 * y2) * dp + ((6.0 * p1) * yn + (2.0 * p2) * xn)
        j01 = (2.0 * xy) * dp + ((2.0 * p1) * xn + (2.0 * p2) * yn)
        det = j00 * j11 - j01 * j01
    qx = np.floor(np.where(in_range, sx, 0.0) * 32.0 + 0.5).astype(np.int64)
    qy = np.floor(np.where(in_range, sy, 0.0) * 32.0 + 0.5).astype(np.int64)
    flags = np.zeros((Ho, Wo), np.uint8)
    flags[~(det > 0)] |= FOLDED
    flags[~in_range] |= RANGE
    if nearest:
        ix, iy = (qx + 16) >> 5, (qy + 16) >> 5
        taps = [(0, 0, np.full((Ho, Wo), 1024, np.int64))]
    else:
        ix, iy, ax, ay = qx >> 5, qy >> 5, qx & 31, qy & 31
        taps = [(0, 0, (32 - ax) * (32 - ay)), (1, 0, ax * (32 - ay)), (0, 1, (32 - ax) * ay), (1, 1, ax * ay)]
    acc = np.zeros((B, Ho, Wo, C), np.int64)
    outside = ~in_range
    for dx, dy, w in taps:
        tx, ty = ix + dx, iy + dy
        inside = in_range & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        outside = outside | ((w > 0) & ~inside)
        v = np.where(inside[None, :, :, None], frames[:, np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1), :].astype(np.int64), border)
        acc += v * w[None, :, :, None]
    flags[outside] |= OUTSIDE
    return ((acc + 512) >> 10).astype(np.uint8), flags, np.stack([qx, qy], axis=-1).astype(np.int32)


# the lenses of the GPU tests, for a 61 x 47 image: (lens, new_k)
F, CX, CY = 80.0, 30.2, 23.1
LENSES = {
    "identity": ((F, F, CX, CY, 0, 0, 0, 0, 0), (F, F, CX, CY)),
    "rig": ((F, F, CX, CY, 3.6e-4, -1.4e-2, 0, 0, 0), (F, F, CX, CY)),                         # the example rig's coefficients
    "barrel": ((F, F, CX, CY, -0.25, 0.02, 0, 0, 0), (0.8 * F, 0.8 * F, 29.0, 24.0)),
    "pincushion": ((F, 1.1 * F, CX, CY, 0.2, 0.05, 1e-3, -5e-4, 0.01), (F, F, 31.0, 22.5)),  # tangential terms, fx != fy
    "folded": ((F, F, CX, CY, -0.6, 0.02, 0, 0, 0), (F / 2, F / 2, CX, CY)),
    "wild": ((F, F, CX, CY, 5e3, 1e6, 0, 0, 1e9), (F / 8, F / 8, CX, CY)),
}


@pytest.fixture(scope="module")
def batch():
    f = np.random.default_rng(7).integers(0, 256, size=(2, 47, 61, 3), dtype=np.uint8)
    f.setflags(write=False)
    return f


# ----------------------------------------------------------------------------- the oracle by itself
def test_oracle_identity_returns_the_input(batch):
    lens, nk = LENSES["identity"]
    for nearest in (False, True):
        out, flags, qmap = undistort_oracle(batch, lens, nk, (47, 61), nearest=nearest)
        assert np.array_equal(out, batch) and not flags.any()
        assert np.array_equal(qmap[..., 0], np.broadcast_to(32 * np.arange(61), (47, 61)))
        assert np.array_equal(qmap[..., 1], np.broadcast_to(32 * np.arange(47)[:, None], (47, 61)))


def test_oracle_whole_pixel_shift(batch):
    lens, _ = LENSES["identity"]
    out, flags, _ = undistort_oracle(batch, lens, (F, F, CX + 3, CY), (47, 61), border=200)
    assert np.array_equal(out[:, :, 3:], batch[:, :, :-3]) and np.all(out[:, :, :3] == 200)
    assert np.all(flags[:, :3] == OUTSIDE) and not flags[:, 3:].any()


def test_oracle_half_pixel_shift_averages_neighbours(batch):
    lens, _ = LENSES["identity"]
    out, flags, _ = undistort_oracle(batch, lens, (F, F, CX + 0.5, CY), (47, 61))
    a, b = batch[:, :, :-1].astype(int), batch[:, :, 1:].astype(int)
    assert np.array_equal(out[:, :, 1:], ((a + b + 1) >> 1).astype(np.uint8))
    assert np.array_equal(out[:, :, 0], ((batch[:, :, 0].astype(int) + 1) >> 1).astype(np.uint8))      # half border 0, half pixel 0
    assert np.all(flags[:, 0] == OUTSIDE) and not flags[:, 1:].any()
    near, _, _ = undistort_oracle(batch, lens, (F, F, CX + 0.5, CY), (47, 61), nearest=True)          # x - 0.5 rounds up: to x itself
    assert np.array_equal(near, batch)


def test_oracle_folded_lens_shows_folded_and_outside(batch):
    lens, nk = LENSES["folded"]
    _, flags, _ = undistort_oracle(batch, lens, nk, (47, 61))
    assert np.any(flags & FOLDED) and np.any(flags & OUTSIDE) and not np.any(flags & RANGE)
    assert flags[23, 30] == 0                                 # the centre is neither
    # k1 = -0.6, k2 = 0.02: along an axis det = (1 + k1 r2 + k2 r2^2)(1 + 3 k1 r2 + 5 k2 r2^2) turns negative at r2 = 0.574
    r2 = ((np.arange(61) - CX) / (F / 2)) ** 2
    row = np.abs(np.arange(47) - CY).argmin()
    yn2 = ((row - CY) / (F / 2)) ** 2
    want = ~((1 - 0.6 * (r2 + yn2) + 0.02 * (r2 + yn2) ** 2 > 0) & (1 - 1.8 * (r2 + yn2) + 0.1 * (r2 + yn2) ** 2 > 0))
    near = np.abs(1 - 1.8 * (r2 + yn2) + 0.1 * (r2 + yn2) ** 2) < 0.05          # leave out pixels at the turning point
    assert np.array_equal(((flags[row] & FOLDED) != 0)[~near], want[~near])


def test_oracle_wild_lens_shows_range(batch):
    lens, nk = LENSES["wild"]
    out, flags, qmap = undistort_oracle(batch, lens, nk, (47, 61), border=9)
    bad = (flags & RANGE) != 0
    assert bad.any() and not bad.all()
    assert np.all(flags[bad] & OUTSIDE) and np.all(out[:, bad] == 9) and not qmap[bad].any()


# ----------------------------------------------------------------------------- struct layouts, constructors, ValueErrors
def test_struct_sizes_match_the_header():
    assert ctypes.sizeof(_native.LensStruct) == 9 * 8 == 72
    assert ctypes.sizeof(_native.UndistortOpts) == 12 * 4 == 48
    assert [n for n, _ in _native.LensStruct._fields_] == ["fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3"]
    assert [n for n, _ in _native.UndistortOpts._fields_][:5] == ["frames_on_device", "out_on_device", "interpolation", "border_value", "chunk_frames"]
    assert "sba_undistort_frames" in _native.EXPORTED_SYMBOLS


def test_lens_constructors():
    row11 = np.array([0.1, 0.2, 0.3, 1, 2, 3, 2388.5, 3.6e-4, -1.4e-2, 1552.0, 1080.5])
    assert Lens.from_camera_row(row11).as_tuple() == (2388.5, 2388.5, 1552.0, 1080.5, 3.6e-4, -1.4e-2, 0, 0, 0)
    row13 = np.array([0.1, 0.2, 0.3, 1, 2, 3, 2388.5, 3.6e-4, -1.4e-2, 1e-3, -5e-4, 1552.0, 1080.5])
    assert Lens.from_camera_row(row13).as_tuple() == (2388.5, 2388.5, 1552.0, 1080.5, 3.6e-4, -1.4e-2, 1e-3, -5e-4, 0)
    K = np.array([[900.0, 0, 320.5], [0, 910.0, 240.25], [0, 0, 1]])
    assert Lens.from_opencv(K, [0.1, 0.2, 0.3, 0.4]).as_tuple() == (900.0, 910.0, 320.5, 240.25, 0.1, 0.2, 0.3, 0.4, 0.0)
    assert Lens.from_opencv(K, [[0.1, 0.2, 0.3, 0.4, 0.5]]).as_tuple()[4:] == (0.1, 0.2, 0.3, 0.4, 0.5)
    lens8 = Lens.from_opencv(K, [0.1, 0.2, 0.3, 0.4, 0.5, 0, 0, 0])
    assert lens8.k3 == 0.5 and np.array_equal(lens8.camera_matrix, K)
    assert np.array_equal(lens8.distortion_coefficients, [0.1, 0.2, 0.3, 0.4, 0.5])
    for bad in ([0.1, 0.2, 0.3, 0.4, 0.5, 1e-3, 0, 0], [0.1, 0.2, 0.3], np.zeros(12) + 1e-9):
        with pytest.raises(ValueError):
            Lens.from_opencv(K, bad)
    with pytest.raises(ValueError):
        Lens.from_opencv(K[:2], [0, 0, 0, 0])
    with pytest.raises(ValueError):
        Lens.from_opencv(K + np.array([[0, 1e-3, 0], [0, 0, 0], [0, 0, 0]]), [0, 0, 0, 0])
    for n in (10, 12, 14):
        with pytest.raises(ValueError):
            Lens.from_camera_row(np.zeros(n))
    for bad in ((0.0, 1, 0, 0), (1, -1.0, 0, 0), (1, 1, np.nan, 0), (1, 1, 0, 0, np.inf)):
        with pytest.raises(ValueError):
            Lens(*bad)


def test_python_side_value_errors():
    """Every ValueError is raised before the library is called: none of these needs a GPU."""
    lens = Lens(F, F, CX, CY, -0.1)
    frames = np.zeros((2, 47, 61, 3), np.uint8)
    bad_calls = [
        dict(frames=frames.astype(np.float32)),                                  # dtype
        dict(frames=np.zeros((2, 47, 61, 2), np.uint8)),                          # channels
        dict(frames=frames[:, :, ::2]),                                           # pixels not contiguous
        dict(lens=(F, F, CX, CY)),                                                # not a Lens
        dict(new_camera_matrix=np.eye(2)),
        dict(new_camera_matrix=np.array([[F, 0.1, CX], [0, F, CY], [0, 0, 1]])),  # skew
        dict(new_camera_matrix=(0.0, F, CX, CY)),
        dict(new_camera_matrix=(F, F, np.nan, CY)),
        dict(out_size=(61,)),
        dict(out_size=(-1, 47)),
        dict(out_size=(16385, 47)),
        dict(interpolation="cubic"),
        dict(border_value=256),
        dict(border_value=-1),
        dict(border_value=0.5),
        dict(out=np.zeros((2, 47, 60, 3), np.uint8)),                             # shape
        dict(out=np.zeros((2, 47, 61, 3), np.int8)),                              # dtype
        dict(out=np.zeros((2, 47, 122, 3), np.uint8)[:, :, ::2]),                 # pixels not contiguous
        dict(out=[[0]]),                                                          # not an array
    ]
    for kw in bad_calls:
        args = dict(frames=frames, lens=lens)
        args.update(kw)
        with pytest.raises(ValueError):
            imaging.undistort_frames(**args)
    ro = np.zeros((2, 47, 61, 3), np.uint8)
    ro.setflags(write=False)
    with pytest.raises(ValueError):
        imaging.undistort_frames(frames, lens, out=ro)
    with pytest.raises(ValueError):
        _native.undistort_frames(frames, lens.as_tuple(), (F, F, CX, CY), (47, 61), want_frames=False)     # nothing asked for
    with pytest.raises(ValueError):
        _native.undistort_frames(frames, lens.as_tuple(), (F, F, CX, CY), (47, 61), want_frames=False, want_flags=True, out=frames.copy())
    for kw in (dict(lens=None), dict(size=(61,)), dict(size=(61, 20000)), dict(new_camera_matrix=np.zeros(5))):
        args = dict(lens=lens, new_camera_matrix=None, size=(61, 47))
        args.update(kw)
        with pytest.raises(ValueError):
            imaging.invertible_region(**args)
    for kw in (dict(lens="x"), dict(alpha=-0.1), dict(alpha=1.5), dict(image_size=(1, 47)), dict(new_size=(61, 1)), dict(image_size=61),
               dict(lens=Lens(F, F, CX, CY, -50.0))):                              # folds inside the image
        args = dict(lens=lens, image_size=(61, 47), alpha=0.0)
        args.update(kw)
        with pytest.raises(ValueError):
            imaging.optimal_new_camera_matrix(**args)


# ----------------------------------------------------------------------------- optimal_new_camera_matrix
# A barrel lens on a 161 x 121 image with the principal point in the image centre: the edges of the undistorted image bow inwards
# and touch the inner rectangle at their midpoints, which the 9 x 9 grid samples (column / row 4), so alpha = 0 is exact there.
BW, BH = 161, 121
BARREL = Lens(120.0, 120.0, (BW - 1) / 2, (BH - 1) / 2, -0.28, 0.05)


def test_newton_inversion_round_trips():
    uv = np.random.default_rng(3).uniform([0, 0], [BW - 1, BH - 1], size=(200, 2))
    xy = BARREL.undistort_points(uv)
    xd, yd, *_ = BARREL.distort(xy[:, 0], xy[:, 1])
    back = np.stack([BARREL.fx * xd + BARREL.cx, BARREL.fy * yd + BARREL.cy], axis=1)
    assert np.max(np.abs(back - uv)) < 1e-10                   # pixels; float64 Newton steps converge to rounding error


@pytest.mark.parametrize("new_size", [None, (97, 75)])
def test_alpha_zero_keeps_only_valid_pixels(new_size):
    K, roi = imaging.optimal_new_camera_matrix(BARREL, (BW, BH), 0.0, new_size)
    w, h = new_size or (BW, BH)
    frames = np.zeros((1, BH, BW, 1), np.uint8)
    _, flags, _ = undistort_oracle(frames, BARREL.as_tuple(), (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), (h, w))
    assert not np.any(flags & OUTSIDE) and not flags.any()
    assert roi == (0, 0, w, h)                                 # the whole new image is valid
    # and it is tight: the midpoints of the four edges come from the source's edges
    _, _, qmap = undistort_oracle(frames, BARREL.as_tuple(), (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), (h, w))
    if new_size is None:
        assert qmap[(h - 1) // 2, 0, 0] == 0 and qmap[(h - 1) // 2, w - 1, 0] == 32 * (BW - 1)
        assert qmap[0, (w - 1) // 2, 1] == 0 and qmap[h - 1, (w - 1) // 2, 1] == 32 * (BH - 1)


@pytest.mark.parametrize("new_size", [None, (200, 90)])
def test_alpha_one_keeps_every_source_pixel(new_size):
    K, roi = imaging.optimal_new_camera_matrix(BARREL, (BW, BH), 1.0, new_size)
    w, h = new_size or (BW, BH)
    g = np.stack(np.meshgrid(np.arange(9) * (BW - 1) / 8, np.arange(9) * (BH - 1) / 8), axis=-1).reshape(-1, 2)
    xy = BARREL.undistort_points(g)
    u, v = K[0, 0] * xy[:, 0] + K[0, 2], K[1, 1] * xy[:, 1] + K[1, 2]
    eps = 1e-9
    assert u.min() >= -eps and u.max() <= w - 1 + eps and v.min() >= -eps and v.max() <= h - 1 + eps
    assert abs(u.min()) < eps and abs(u.max() - (w - 1)) < eps and abs(v.min()) < eps and abs(v.max() - (h - 1)) < eps   # and tight
    x, y, rw, rh = roi
    assert 0 <= x and 0 <= y and rw > 0 and rh > 0 and x + rw <= w and y + rh <= h
    assert rw < w and rh < h                                    # border surrounds the valid region
    _, flags, _ = undistort_oracle(np.zeros((1, BH, BW, 1), np.uint8), BARREL.as_tuple(), (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), (h, w))
    assert not np.any(flags[y:y + rh, x:x + rw] & OUTSIDE) and np.any(flags & OUTSIDE)


def test_alpha_blends_and_roi_stays_inside():
    K0, _ = imaging.optimal_new_camera_matrix(BARREL, (BW, BH), 0.0)
    K1, _ = imaging.optimal_new_camera_matrix(BARREL, (BW, BH), 1.0)
    Kh, roi = imaging.optimal_new_camera_matrix(BARREL, (BW, BH), 0.25)
    assert np.allclose(Kh, 0.75 * K0 + 0.25 * K1, rtol=0, atol=1e-12)
    assert K1[0, 0] < Kh[0, 0] < K0[0, 0]
    x, y, rw, rh = roi
    assert 0 <= x and 0 <= y and x + rw <= BW and y + rh <= BH and rw > 0 and rh > 0
    pin = Lens(120.0, 125.0, 83.0, 57.5, 0.15, 0.02, 1e-3, -2e-3)            # a pincushion with tangential terms
    for alpha in (0.0, 0.5, 1.0):
        K, roi = imaging.optimal_new_camera_matrix(pin, (BW, BH), alpha)
        x, y, rw, rh = roi
        assert 0 <= x and 0 <= y and x + rw <= BW and y + rh <= BH and rw > 0 and rh > 0
        assert K[0, 1] == 0 and K[2, 2] == 1 and K[0, 0] > 0 and K[1, 1] > 0
