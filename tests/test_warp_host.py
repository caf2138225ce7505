"""CPU tests of the plane views and virtual cameras (include/sba_hip.h: sba_warp_frames; lasercalib_amd/imaging.py).

``warp_oracle`` is the rule of the header restated in numpy, on the pattern of ``undistort_oracle`` of
tests/test_undistort_host.py: every line of the float64 part is one IEEE operation per operation of the rule, in the rule's
order, and everything behind it is integer arithmetic, so it defines the bytes, the flags and the map exactly.  It is the
reference of tests/test_gpu_warp.py and is pinned here to answers known without it: with the inverse of a power-of-two camera
matrix it is ``undistort_oracle`` bit for bit, a quarter turn is a transposition, a horizon puts whole rows behind the camera,
and the positions it finds on a plane are those the bundle adjustment's camera model projects the plane's points to.
The rest of the file covers what runs on the host: PlaneGrid, virtual_camera_matrix, plane_mosaic's owner rule and every
ValueError of the new Python entry points.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lasercalib_amd import _native, imaging  # noqa: E402
from lasercalib_amd.imaging import Lens, PlaneGrid  # noqa: E402
from oracle import sba_oracle, sba_oracle_tangential  # noqa: E402
from test_undistort_host import LENSES, undistort_oracle  # noqa: E402

OUTSIDE, FOLDED, RANGE, BEHIND = 1, 2, 4, 8


def warp_oracle(frames, lens, m, out_hw, border=0, nearest=False):
    """(out, flags, map) of the rule of sba_warp_frames in include/sba_hip.h.  ``frames`` (B, H, W, C) uint8, ``lens`` = (fx, fy,
    cx, cy, k1, k2, p1, p2, k3), ``m`` 3 x 3 or nine values, row-major, ``out_hw`` = (height, width)."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = (np.float64(v) for v in lens)
    m = np.asarray(m, dtype=np.float64).reshape(9)
    B, H, W, C = frames.shape
    Ho, Wo = out_hw
    x = np.broadcast_to(np.arange(Wo, dtype=np.float64)[None, :], (Ho, Wo))
    y = np.broadcast_to(np.arange(Ho, dtype=np.float64)[:, None], (Ho, Wo))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        X = (m[0] * x + m[1] * y) + m[2]
        Y = (m[3] * x + m[4] * y) + m[5]
        Z = (m[6] * x + m[7] * y) + m[8]
        front = Z > 0
        Zs = np.where(front, Z, 1.0)
        xn, yn = np.where(front, X / Zs, 0.0), np.where(front, Y / Zs, 0.0)
        x2, y2 = xn * xn, yn * yn
        r2, xy = x2 + y2, xn * yn
        t = r2 * k3; t = k2 + t; t = r2 * t; t = k1 + t; t = r2 * t      # noqa: E702
        rad = 1.0 + t
        xd = xn * rad + ((2.0 * p1) * xy + p2 * (r2 + 2.0 * x2))
        yd = yn * rad + (p1 * (r2 + 2.0 * y2) + (2.0 * p2) * xy)
        sx, sy = fx * xd + cx, fy * yd + cy
        in_range = front & (sx > -32768) & (sx < 32768) & (sy > -32768) & (sy < 32768)
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
    flags[~front] |= BEHIND
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


# ----------------------------------------------------------------------------- shared cases (also used by tests/test_gpu_warp.py)
POW2_MATRICES = [(64.0, 30.25, 23.5), (32.0, 29.0, 24.0), (128.0, 31.5, 22.125)]      # (fn, cxn, cyn): both front ends are exact
IDENTITY_LENS = (1.0, 1.0, 0.0, 0.0, 0, 0, 0, 0, 0)
HORIZON = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 1.0, -20.5]])


def inverse_k(fn, cxn, cyn):
    return np.array([[1 / fn, 0, -cxn / fn], [0, 1 / fn, -cyn / fn], [0, 0, 1.0]])


def quarter_turn(H):
    return np.array([[0, 1.0, 0], [-1.0, 0, H - 1.0], [0, 0, 1.0]])


# A camera of the example rig's kind above the floor: 3208 x 2200 pixels, f 1780, the rig's k1 and k2, a rotation of 2.9 rad about
# the x axis (it looks down, a little tilted), 2.5 m above the origin; and the same with tangential terms
ROW11 = np.array([2.9, 0.0, 0.0, 30.0, -20.0, 2500.0, 1780.0, 3.6e-4, -1.4e-2, 1604.0, 1100.0])
ROW13 = np.concatenate([ROW11[:9], [1e-3, -5e-4], ROW11[9:]])
FLOOR = dict(z=10.0, x_range=(-600.0, 600.0), y_range=(-450.0, 450.0), mm_per_pixel=4.0)      # 300 x 225 pixels
MAP_BOUND = 0.5 / 32 + 1e-6            # pixels: rounding to the 1/32 grid plus float64 noise


def small_camera(row, W=61, H=47, W0=3208.0):
    """``row`` scaled to a W x H source: the same view in fewer pixels."""
    s = W / W0
    r = np.array(row, dtype=np.float64)
    r[6] *= s
    r[-2:] = (W - 1) / 2 + 0.2, (H - 1) / 2 - 0.4
    return r


@pytest.fixture(scope="module")
def batch():
    f = np.random.default_rng(7).integers(0, 256, size=(2, 47, 61, 3), dtype=np.uint8)      # that of tests/test_undistort_host.py
    f.setflags(write=False)
    return f


# ----------------------------------------------------------------------------- the oracle, pinned to answers known without it
@pytest.mark.parametrize("name", list(LENSES))
def test_oracle_equals_undistortion_for_power_of_two_matrices(batch, name):
    lens = LENSES[name][0]
    for fn, cxn, cyn in POW2_MATRICES:
        for nearest in (False, True):
            want = undistort_oracle(batch, lens, (fn, fn, cxn, cyn), (47, 61), border=50, nearest=nearest)
            for scale in (1.0, 4.0):
                got = warp_oracle(batch, lens, scale * inverse_k(fn, cxn, cyn), (47, 61), border=50, nearest=nearest)
                for g, w in zip(got, want):
                    assert np.array_equal(g, w), (name, fn, nearest, scale)
                assert not np.any(got[1] & BEHIND)


def test_oracle_quarter_turn_is_a_transposition(batch):
    H, W = batch.shape[1:3]
    for nearest in (False, True):
        out, flags, qmap = warp_oracle(batch, IDENTITY_LENS, quarter_turn(H), (W, H), nearest=nearest)
        assert np.array_equal(out, np.transpose(batch, (0, 2, 1, 3))[:, :, ::-1]) and not flags.any()
    assert np.array_equal(qmap[..., 0], np.broadcast_to(32 * np.arange(W)[:, None], (W, H)))


def test_oracle_horizon_puts_whole_rows_behind(batch):
    lens = LENSES["rig"][0]
    out, flags, qmap = warp_oracle(batch, lens, HORIZON, (47, 61), border=9)
    assert np.all(flags[:21] == (BEHIND | RANGE | OUTSIDE)) and not np.any(flags[21:] & BEHIND)
    assert np.all(out[:, :21] == 9) and not qmap[:21].any()
    assert np.any(flags[21:] == 0)                                 # and in front of it the source is seen


@pytest.mark.parametrize("row, project", [(ROW11, sba_oracle.project), (ROW13, sba_oracle_tangential.project)], ids=["11", "13"])
def test_oracle_map_is_the_projection_of_the_plane(row, project):
    grid = PlaneGrid.z_plane(**FLOOR)
    assert grid.size == (300, 225)
    _, flags, qmap = warp_oracle(np.zeros((1, 2200, 3208, 1), np.uint8), Lens.from_camera_row(row).as_tuple(), grid.matrix(row), (225, 300))
    assert not flags.any()                                          # the whole grid is seen
    world = grid.world_points().reshape(-1, 3)
    uv = project(world, np.broadcast_to(row, (world.shape[0], row.shape[0])).copy()).reshape(225, 300, 2)
    err = np.abs(qmap / 32.0 - uv).max()
    print(f"max |q / 32 - project| = {err:.7f} px (bound {MAP_BOUND:.6f})")
    assert err <= MAP_BOUND
    assert np.ptp(qmap[..., 0]) > 32 * 700 and np.ptp(qmap[..., 1]) > 32 * 500      # the grid covers a good part of the image


# ----------------------------------------------------------------------------- PlaneGrid, virtual_camera_matrix
def test_plane_grid_round_trips_and_matrix_against_a_hand_built_rotation():
    grid = PlaneGrid((10.0, -20.0, 5.0), (2.0, 1.0, 0.0), (-1.0, 2.0, 0.5), (7, 5))
    P = grid.world_points()
    assert P.shape == (5, 7, 3) and np.array_equal(P[3, 4], [10 + 8 - 3, -20 + 4 + 6, 5 + 1.5])
    px = grid.pixel_of(P)
    want = np.stack(np.meshgrid(np.arange(7.0), np.arange(5.0)), axis=-1)
    assert np.max(np.abs(px - want)) < 1e-12
    assert np.max(np.abs(grid.pixel_of(P + 3.0 * np.cross(grid.u_step, grid.v_step)) - want)) < 1e-10      # off the plane: its foot
    # a quarter turn about z: R = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    row = np.array([0, 0, np.pi / 2, 1.0, 2.0, 3.0, 100.0, 0, 0, 50.0, 40.0])
    R = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    M = grid.matrix(row)
    assert np.allclose(M, np.stack([R @ grid.u_step, R @ grid.v_step, R @ grid.origin + [1, 2, 3]], axis=1), rtol=0, atol=1e-14)
    assert np.allclose(M[:, 0], [-1, 2, 0], atol=1e-14) and np.allclose(M[:, 2], [20 + 1, 10 + 2, 5 + 3], atol=1e-13)
    lens = Lens.from_camera_row(row)
    assert np.array_equal(grid.matrix((lens, R, [1, 2, 3])), np.stack([R @ grid.u_step, R @ grid.v_step, R @ grid.origin + [1, 2, 3]], axis=1))
    assert np.array_equal(imaging.rodrigues([0, 0, 0]), np.eye(3))
    # Rodrigues agrees with the bundle adjustment's rotate
    rv = np.array([0.3, -2.1, 1.7])
    pts = np.random.default_rng(2).normal(size=(5, 3))
    assert np.allclose(pts @ imaging.rodrigues(rv).T, sba_oracle.rotate(pts, np.broadcast_to(rv, (5, 3))), rtol=0, atol=1e-14)
    z = PlaneGrid.z_plane(10.0, (0, 10), (0, 6), 2.0)
    assert z.size == (5, 3) and np.array_equal(z.world_points()[2, 4], [8.0, 4.0, 10.0])


def test_virtual_camera_matrix():
    for fn, cxn, cyn in POW2_MATRICES:
        K = np.array([[fn, 0, cxn], [0, fn, cyn], [0, 0, 1]])
        assert np.array_equal(imaging.virtual_camera_matrix(K), inverse_k(fn, cxn, cyn))
    K = np.array([[90.0, 0.7, 31.0], [0, 95.0, 22.0], [0, 0, 1]])           # skew
    assert np.allclose(imaging.virtual_camera_matrix(K) @ K, np.eye(3), rtol=0, atol=1e-13)
    R = imaging.rodrigues([0.1, -0.2, 0.05])
    assert np.allclose(imaging.virtual_camera_matrix(K, R), R.T @ np.linalg.inv(K), rtol=0, atol=1e-15)
    for bad in (dict(new_camera_matrix=np.eye(2)), dict(new_camera_matrix=np.array([[90.0, 0, 31], [0.1, 95, 22], [0, 0, 1]])),
                dict(new_camera_matrix=np.diag([0.0, 1, 1])), dict(rotation=2 * np.eye(3)), dict(rotation=np.diag([1.0, 1, -1])),
                dict(rotation=np.eye(4)), dict(new_camera_matrix=K * np.nan)):
        args = dict(new_camera_matrix=K)
        args.update(bad)
        with pytest.raises(ValueError):
            imaging.virtual_camera_matrix(**args)


# ----------------------------------------------------------------------------- plane_mosaic
def brute_force_owner(flags, maps, sizes):
    n, (Ho, Wo) = len(flags), flags[0].shape
    owner = np.full((Ho, Wo), -1, np.int32)
    for y in range(Ho):
        for x in range(Wo):
            best = None
            for k in range(n):
                if flags[k][y, x] != 0:
                    continue
                qx, qy = int(maps[k][y, x, 0]), int(maps[k][y, x, 1])
                W, H = sizes[k]
                d = min(qx, 32 * (W - 1) - qx, qy, 32 * (H - 1) - qy)
                if best is None or d > best:
                    best, owner[y, x] = d, k
    return owner


def two_floor_cameras():
    """Two 61 x 47 cameras (each sees some 4.5 m x 3.5 m of the floor) above a 40 x 25 floor grid of 200 mm pixels: their views
    overlap in the middle and leave the rim of the grid to nobody."""
    grid = PlaneGrid.z_plane(0.0, (-4000.0, 4000.0), (-2500.0, 2500.0), 200.0)
    rows = [small_camera(ROW11), small_camera(ROW11)]
    rows[0][3], rows[1][3] = 1200.0, -1200.0                                 # t_x: one looks at the left half, one at the right half
    rows[1][:3] = (2.9, 0.05, 0.0)
    return grid, rows


def test_plane_mosaic_owner_rule_against_a_brute_force_loop():
    grid, rows = two_floor_cameras()
    w, h = grid.size
    rng = np.random.default_rng(5)
    views, flags, maps = [], [], []
    for k, row in enumerate(rows):
        src = rng.integers(0, 256, size=(2, 47, 61, 3), dtype=np.uint8)
        out, fl, qm = warp_oracle(src, Lens.from_camera_row(row).as_tuple(), grid.matrix(row), (h, w), nearest=True)
        views.append(out), flags.append(fl), maps.append(qm)
    want = brute_force_owner(flags, maps, [(61, 47)] * 2)
    assert set(np.unique(want)) == {-1, 0, 1}                               # both cameras own pixels, some pixels nobody does
    both = (flags[0] == 0) & (flags[1] == 0)
    assert np.any(want[both] == 0) and np.any(want[both] == 1)              # and the overlap is split between them
    mosaic, owner = imaging.plane_mosaic(views, flags, maps, [(61, 47)] * 2, fill=77)
    assert owner.dtype == np.int32 and np.array_equal(owner, want)
    by_hand = np.full_like(views[0], 77)
    for k in range(2):
        by_hand[:, want == k] = views[k][:, want == k]
    assert np.array_equal(mosaic, by_hand)
    # ties go to the lowest index: the same camera twice
    _, owner = imaging.plane_mosaic([views[1], views[1]], [flags[1]] * 2, [maps[1]] * 2, [(61, 47)] * 2)
    assert np.array_equal(owner, np.where(flags[1] == 0, 0, -1))
    # one-channel views without a channel axis
    mosaic, owner = imaging.plane_mosaic([v[..., 0] for v in views], flags, maps, [(61, 47)] * 2, fill=77)
    assert np.array_equal(mosaic, by_hand[..., 0]) and np.array_equal(owner, want)
    for bad in (dict(views=[]), dict(flags=flags[:1]), dict(fill=256), dict(views=[views[0], views[1][:, :-1]]),
                dict(flags=[flags[0], flags[1][:-1]]), dict(maps=[maps[0], maps[1][..., :1]]), dict(views=[views[0][0, 0], views[1][0, 0]])):                  # no batch axis
        args = dict(views=views, flags=flags, maps=maps, source_sizes=[(61, 47)] * 2)
        args.update(bad)
        with pytest.raises(ValueError):
            imaging.plane_mosaic(**args)


# ----------------------------------------------------------------------------- struct and ValueError checks
def test_python_side_value_errors():
    """Every ValueError is raised before the library is called: none of these needs a GPU."""
    assert "sba_warp_frames" in _native.EXPORTED_SYMBOLS
    assert imaging.SBA_WARP_BEHIND == _native.WARP_BEHIND == 8
    lens = Lens(80.0, 80.0, 30.2, 23.1, -0.1)
    frames = np.zeros((2, 47, 61, 3), np.uint8)
    m = inverse_k(64.0, 30.25, 23.5)
    bad_calls = [
        dict(frames=frames.astype(np.float32)), dict(frames=np.zeros((2, 47, 61, 2), np.uint8)), dict(frames=frames[:, :, ::2]),
        dict(lens=lens.as_tuple()),
        dict(matrix=np.eye(2)), dict(matrix=np.zeros(9)), dict(matrix=np.full((3, 3), np.nan)), dict(matrix=np.where(m == 0, m, np.inf)),
        dict(out_size=(61,)), dict(out_size=(-1, 47)), dict(out_size=(16385, 47)),
        dict(interpolation="cubic"), dict(border_value=256), dict(border_value=-1), dict(border_value=0.5),
        dict(out=np.zeros((2, 47, 60, 3), np.uint8)), dict(out=np.zeros((2, 47, 61, 3), np.int8)),
        dict(out=np.zeros((2, 47, 122, 3), np.uint8)[:, :, ::2]), dict(out=[[0]]),
    ]
    for kw in bad_calls:
        args = dict(frames=frames, lens=lens, matrix=m, out_size=(61, 47))
        args.update(kw)
        with pytest.raises(ValueError):
            imaging.warp_frames(**args)
    with pytest.raises(ValueError):
        _native.warp_frames(frames, lens.as_tuple(), np.zeros(8), (47, 61))
    with pytest.raises(ValueError):
        _native.warp_frames(frames, lens.as_tuple(), m, (47, 61), want_frames=False)                  # nothing asked for
    with pytest.raises(ValueError):
        _native.warp_frames(frames, lens.as_tuple(), m, (47, 61), want_frames=False, want_flags=True, out=frames.copy())
    grid = PlaneGrid.z_plane(**FLOOR)
    for bad in (dict(camera=np.zeros(12)), dict(camera=(lens, np.eye(2), [0, 0, 1])), dict(camera=(lens, np.eye(3), [0, 1])),
                dict(grid=(300, 225)), dict(frames=frames[..., :2])):
        args = dict(frames=frames, camera=ROW11, grid=grid)
        args.update(bad)
        with pytest.raises(ValueError):
            imaging.plane_view(**args)
    for bad in (dict(origin=(0, 0)), dict(u_step=(np.nan, 0, 0)), dict(v_step=(2, 0, 0)), dict(size=(-1, 5)), dict(size=(5,))):
        args = dict(origin=(0, 0, 0), u_step=(1, 0, 0), v_step=(0, 1, 0), size=(4, 4))
        args.update(bad)
        with pytest.raises(ValueError):
            PlaneGrid(**args)
    for bad in (dict(mm_per_pixel=0.0), dict(x_range=(5, 5)), dict(y_range=(1, 0)), dict(z=np.inf)):
        args = dict(FLOOR)
        args.update(bad)
        with pytest.raises(ValueError):
            PlaneGrid.z_plane(**args)
    with pytest.raises(ValueError):
        imaging.rodrigues([0, 1])
