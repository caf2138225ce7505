"""GPU tests of sba_warp_frames (include/sba_hip.h) through ``lasercalib_amd.imaging`` and ``lasercalib_amd._native``.

The reference is ``warp_oracle`` of tests/test_warp_host.py, the header's rule in numpy (pinned there to answers known without
it).  The rule is IEEE float64 operation by operation followed by integer arithmetic, so every comparison of pixels, flags and
map is bit equality; the one tolerance, of the map against the bundle adjustment's projection, is rounding to the 1/32-pixel grid
plus float64 noise.  Buffers with padding are pre-filled with a sentinel and compared whole.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lasercalib_amd import _native, imaging  # noqa: E402
from lasercalib_amd.imaging import Lens, PlaneGrid  # noqa: E402
from test_gpu_undistort import SENTINEL, on_device, padded  # noqa: E402
from test_undistort_host import LENSES  # noqa: E402
from test_warp_host import (BEHIND, FLOOR, HORIZON, IDENTITY_LENS, MAP_BOUND, OUTSIDE, POW2_MATRICES, RANGE, ROW11, ROW13,  # noqa: E402
                            brute_force_owner, inverse_k, quarter_turn, small_camera, two_floor_cameras, warp_oracle)

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
        f = np.random.default_rng(90 + C).integers(0, 256, size=(5, 47, 61, C), dtype=np.uint8)
        f.setflags(write=False)
        RANDOM[C] = f
    return RANDOM[C]


def oracle_of(C, lens9, m, out_hw, border=0, nearest=False):
    key = (C, tuple(lens9), tuple(np.asarray(m, dtype=np.float64).ravel()), tuple(out_hw), border, nearest)
    if key not in ORACLE:
        ORACLE[key] = warp_oracle(random_frames(C), lens9, m, out_hw, border=border, nearest=nearest)
    return ORACLE[key]


# the view of a tilted camera onto a floor grid that reaches beyond what the 61 x 47 source sees: a true perspective (Z varies
# with y), with pixels inside and outside the source
SMALL = small_camera(ROW11)
PERSPECTIVE_GRID = PlaneGrid.z_plane(10.0, (-1500.0, 1500.0), (-1100.0, 1100.0), 50.0)      # 60 x 44
PERSPECTIVE = PERSPECTIVE_GRID.matrix(SMALL)


def run_layouts(torch, C, lens9, m, out_hw, want, **kw):
    """The call from host and device memory, packed and padded with misaligned bases on both sides; everything bit-equal to `want`."""
    frames = random_frames(C)
    lens = Lens(*lens9)
    wo, wf, wm = want
    size = (out_hw[1], out_hw[0])
    got, flags, qmap = imaging.warp_frames(frames, lens, m, size, want_flags=True, want_map=True, **kw)
    assert isinstance(got, np.ndarray) and np.array_equal(got, wo), "host packed"
    assert np.array_equal(flags, wf) and np.array_equal(qmap, wm) and flags.dtype == np.uint8 and qmap.dtype == np.int32
    dev = torch.from_numpy(frames.copy()).cuda()
    got = imaging.warp_frames(dev, lens, m, size, **kw)
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), wo), "device packed"
    sbuf, sview, sstr = padded(frames.shape, 5, 13, 3, frames)
    obuf, oview, ostr = padded(wo.shape, 7, 9, 5)
    expect, _, _ = padded(wo.shape, 7, 9, 5, wo)
    src_before = sbuf.copy()
    ret = imaging.warp_frames(sview, lens, m, size, out=oview, **kw)
    assert ret is oview and np.array_equal(obuf, expect), "host padded: result or padding"
    assert np.array_equal(sbuf, src_before)
    keep_s, dsrc = on_device(torch, sbuf, frames.shape, sstr, 3)
    keep_o, dout = on_device(torch, np.full_like(obuf, SENTINEL), wo.shape, ostr, 5)
    ret = imaging.warp_frames(dsrc, lens, m, size, out=dout, **kw)
    assert ret is dout and np.array_equal(keep_o.cpu().numpy(), expect), "device padded: result or padding"
    assert np.array_equal(keep_s.cpu().numpy(), src_before)


# ----------------------------------------------------------------------------- 1. a perspective view, every lens, layout and option
@pytest.mark.parametrize("C", [3, 1, 4])
@pytest.mark.parametrize("name", list(LENSES))
def test_perspective_view_every_lens_layout_and_option(torch, C, name):
    lens9 = LENSES[name][0]
    for interpolation in ("linear", "nearest"):
        want = oracle_of(C, lens9, PERSPECTIVE, (44, 60), border=200, nearest=interpolation == "nearest")
        run_layouts(torch, C, lens9, PERSPECTIVE, (44, 60), want, interpolation=interpolation, border_value=200)
    flags = oracle_of(C, lens9, PERSPECTIVE, (44, 60), border=200)[1]
    assert not np.any(flags & BEHIND)
    if name in ("identity", "rig"):
        assert np.any(flags == 0) and np.any(flags == OUTSIDE)


# ----------------------------------------------------------------------------- 2. the answers known without the oracle
def test_power_of_two_matrix_equals_undistort_frames_on_the_device(torch):
    frames = random_frames(3)
    dev = torch.from_numpy(frames.copy()).cuda()
    for name in ("barrel", "pincushion", "wild"):
        lens = Lens(*LENSES[name][0])
        for fn, cxn, cyn in POW2_MATRICES:
            K = np.array([[fn, 0, cxn], [0, fn, cyn], [0, 0, 1]])
            for interpolation in ("linear", "nearest"):
                want, wf, wm = imaging.undistort_frames(dev, lens, K, interpolation=interpolation, border_value=50, want_flags=True, want_map=True)
                for scale in (1.0, 4.0):
                    got, gf, gm = imaging.warp_frames(dev, lens, scale * imaging.virtual_camera_matrix(K), (61, 47), interpolation=interpolation,
                                                      border_value=50, want_flags=True, want_map=True)
                    assert torch.equal(got, want) and np.array_equal(gf, wf) and np.array_equal(gm, wm), (name, fn, interpolation, scale)
                assert np.array_equal(imaging.warp_frames(frames, lens, inverse_k(fn, cxn, cyn), (61, 47), interpolation=interpolation,
                                                          border_value=50), want.cpu().numpy())


def test_quarter_turn_is_a_transposition(torch):
    for C in (1, 3, 4):
        frames = random_frames(C)
        want = np.ascontiguousarray(np.transpose(frames, (0, 2, 1, 3))[:, :, ::-1])
        for src in (frames, torch.from_numpy(frames.copy()).cuda()):
            for interpolation in ("linear", "nearest"):
                got, flags, _ = imaging.warp_frames(src, Lens(*IDENTITY_LENS), quarter_turn(47), (47, 61), interpolation=interpolation,
                                                    want_flags=True)
                got = got if isinstance(got, np.ndarray) else got.cpu().numpy()
                assert np.array_equal(got, want) and not flags.any(), (C, interpolation)


def test_horizon_puts_whole_rows_behind(torch):
    lens9 = LENSES["rig"][0]
    want = oracle_of(3, lens9, HORIZON, (47, 61), border=9)
    run_layouts(torch, 3, lens9, HORIZON, (47, 61), want, border_value=9)
    got, flags, qmap = imaging.warp_frames(torch.from_numpy(random_frames(3).copy()).cuda(), Lens(*lens9), HORIZON, (61, 47), border_value=9,
                                           want_flags=True, want_map=True)
    assert np.all(flags[:21] == (BEHIND | RANGE | OUTSIDE)) and not np.any(flags[21:] & BEHIND)
    assert bool((got[:, :21] == 9).all()) and not qmap[:21].any() and np.any(flags[21:] == 0)
    assert imaging.SBA_WARP_BEHIND == BEHIND


# ----------------------------------------------------------------------------- 3. output sizes and alignments
@pytest.mark.parametrize("C", [3, 1, 4])
def test_output_widths_around_the_tile_and_one(torch, C):
    assert TC == 256
    lens9 = LENSES["pincushion"][0]
    for w in (1, 255, 256, 257):
        grid = PlaneGrid.z_plane(10.0, (-1500.0, 1500.0), (-100.0, 100.0), 3000.0 / w)
        grid = PlaneGrid(grid.origin, grid.u_step, (0.0, 40.0, 0.0), (w, 5))
        m = grid.matrix(SMALL)
        for nearest in (False, True):
            run_layouts(torch, C, lens9, m, (5, w), oracle_of(C, lens9, m, (5, w), border=77, nearest=nearest),
                        interpolation="nearest" if nearest else "linear", border_value=77)


def test_output_heights_around_the_tile(torch):
    lens9 = LENSES["barrel"][0]
    for h in (1, TR - 1, TR, TR + 1, 2 * TR - 1, 2 * TR, 2 * TR + 1):
        grid = PlaneGrid((-1500.0, -1100.0, 10.0), (50.0, 0.0, 0.0), (0.0, 2200.0 / h, 0.0), (60, h))
        m = grid.matrix(SMALL)
        run_layouts(torch, 3, lens9, m, (h, 60), oracle_of(3, lens9, m, (h, 60)))


@pytest.mark.parametrize("base", [1, 7, 15])
def test_padded_output_at_misaligned_bases_leaves_the_padding(torch, base):
    lens9 = LENSES["rig"][0]
    for C in (1, 3, 4):
        frames = random_frames(C)
        wo = oracle_of(C, lens9, PERSPECTIVE, (44, 60), border=31)[0]
        dev = torch.from_numpy(frames.copy()).cuda()
        for row_slack, frame_slack in ((3, 0), (0, 5), (11, 17)):
            expect, _, ostr = padded(wo.shape, row_slack, frame_slack, base, wo)
            obuf, oview, _ = padded(wo.shape, row_slack, frame_slack, base)
            assert imaging.warp_frames(frames, Lens(*lens9), PERSPECTIVE, (60, 44), border_value=31, out=oview) is oview
            assert np.array_equal(obuf, expect), ("host", C, row_slack, frame_slack)
            # torch's allocations are 256-byte aligned: the view starts `base` bytes off a 16-byte boundary
            keep, dout = on_device(torch, np.full_like(obuf, SENTINEL), wo.shape, ostr, base)
            assert dout.data_ptr() % 16 == base
            imaging.warp_frames(dev, Lens(*lens9), PERSPECTIVE, (60, 44), border_value=31, out=dout)
            assert np.array_equal(keep.cpu().numpy(), expect), ("device", C, row_slack, frame_slack)


def test_sources_too_narrow_for_a_pair_of_pixels(torch):
    """A source one column wide (1 x 1, 1 x 5 either way) is read tap by tap: two neighbouring pixels cannot be read together."""
    rng = np.random.default_rng(11)
    for shape in ((2, 1, 1, 1), (2, 1, 5, 3), (2, 5, 1, 3), (2, 1, 1, 4)):
        frames = rng.integers(0, 256, size=shape, dtype=np.uint8)
        H, W = shape[1:3]
        lens9 = (6.0, 6.0, (W - 1) / 2 + 0.3, (H - 1) / 2 - 0.2, -0.05, 0.01, 0, 0, 0)
        m = np.array([[0.2, 0.01, -1.1], [-0.02, 0.2, -0.9], [0.0, 0.01, 1.0]])
        for nearest in (False, True):
            want, wf, _ = warp_oracle(frames, lens9, m, (10, 12), border=33, nearest=nearest)
            assert np.any(wf & OUTSIDE) and (not nearest or not np.all(wf & OUTSIDE))
            kw = dict(interpolation="nearest" if nearest else "linear", border_value=33)
            assert np.array_equal(imaging.warp_frames(frames, Lens(*lens9), m, (12, 10), **kw), want), (shape, nearest, "host")
            got = imaging.warp_frames(torch.from_numpy(frames).cuda(), Lens(*lens9), m, (12, 10), **kw)
            assert np.array_equal(got.cpu().numpy(), want), (shape, nearest, "device")


# ----------------------------------------------------------------------------- 4. memory sides, chunks, many frames, no frames
def test_host_and_device_memory_on_either_side(torch):
    lens9 = LENSES["barrel"][0]
    frames = random_frames(3)
    want = oracle_of(3, lens9, PERSPECTIVE, (44, 60))[0]
    dev = torch.from_numpy(frames.copy()).cuda()
    got, _, _ = _native.warp_frames(frames, lens9, PERSPECTIVE, (44, 60), out_on_device=True)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want), "host in, device out"
    got, _, _ = _native.warp_frames(dev, lens9, PERSPECTIVE, (44, 60), out_on_device=False)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want), "device in, host out"
    out = torch.full((5, 44, 60, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    assert _native.warp_frames(frames, lens9, PERSPECTIVE, (44, 60), out=out, out_on_device=True)[0] is out
    assert np.array_equal(out.cpu().numpy(), want)
    out = np.full((5, 44, 60, 3), SENTINEL, np.uint8)
    assert _native.warp_frames(dev, lens9, PERSPECTIVE, (44, 60), out=out, out_on_device=False)[0] is out and np.array_equal(out, want)


@pytest.mark.parametrize("C", [3, 1])
def test_any_chunk_size_gives_the_same_bits(torch, C):
    lens9 = LENSES["pincushion"][0]
    want = oracle_of(C, lens9, PERSPECTIVE, (44, 60))[0]
    frames = random_frames(C)
    dev = torch.from_numpy(frames.copy()).cuda()
    for chunk in (1, 2, 0, 5):
        assert np.array_equal(imaging.warp_frames(frames, Lens(*lens9), PERSPECTIVE, (60, 44), chunk_frames=chunk), want), ("host", chunk)
        assert np.array_equal(imaging.warp_frames(dev, Lens(*lens9), PERSPECTIVE, (60, 44), chunk_frames=chunk).cpu().numpy(), want), ("device", chunk)
    sbuf, sview, _ = padded(frames.shape, 5, 13, 3, frames)
    obuf, oview, _ = padded(want.shape, 7, 9, 5)
    assert imaging.warp_frames(sview, Lens(*lens9), PERSPECTIVE, (60, 44), out=oview, chunk_frames=2) is oview
    assert np.array_equal(obuf, padded(want.shape, 7, 9, 5, want)[0])


def test_every_workgroup_walks_more_than_one_frame(torch):
    """2050 frames of 8 x 8 into 8 x 8: one tile in x, two in y, so 684 frame groups of three frames, the last one short."""
    frames = np.random.default_rng(13).integers(0, 256, size=(2050, 8, 8, 3), dtype=np.uint8)
    lens9 = (10.0, 10.0, 3.4, 3.6, -0.1, 0.01, 1e-3, -1e-3, 0.0)
    m = np.array([[0.1, 0.01, -0.4], [-0.01, 0.1, -0.3], [0.002, 0.004, 1.0]])
    want = warp_oracle(frames, lens9, m, (8, 8), border=5)[0]
    assert np.array_equal(imaging.warp_frames(torch.from_numpy(frames).cuda(), Lens(*lens9), m, (8, 8), border_value=5).cpu().numpy(), want)
    assert np.array_equal(imaging.warp_frames(frames, Lens(*lens9), m, (8, 8), border_value=5), want)


def test_no_frames_and_diagnostics_only(torch):
    lens9 = LENSES["folded"][0]
    _, wf, wm = oracle_of(3, lens9, HORIZON, (47, 61))
    out, flags, qmap = imaging.warp_frames(np.zeros((0, 47, 61, 3), np.uint8), Lens(*lens9), HORIZON, (61, 47), want_flags=True, want_map=True)
    assert out.shape == (0, 47, 61, 3) and np.array_equal(flags, wf) and np.array_equal(qmap, wm)
    out, flags, qmap = imaging.warp_frames(torch.zeros((0, 47, 61, 3), dtype=torch.uint8, device="cuda"), Lens(*lens9), HORIZON, (61, 47),
                                           want_map=True)
    assert tuple(out.shape) == (0, 47, 61, 3) and flags is None and np.array_equal(qmap, wm)
    out, flags, qmap = _native.warp_frames(random_frames(3), lens9, HORIZON, (47, 61), want_flags=True, want_frames=False)
    assert out is None and qmap is None and np.array_equal(flags, wf)
    assert np.any(wf & BEHIND) and np.any(wf & 2)                           # the folding lens folds in front of the horizon only
    assert not np.any(wf[wf & BEHIND != 0] & 2)


# ----------------------------------------------------------------------------- 5. tied to the camera model, and the mosaic
@pytest.mark.parametrize("row", [ROW11, ROW13], ids=["11", "13"])
def test_plane_view_map_is_the_device_projection_of_the_plane(row):
    grid = PlaneGrid.z_plane(**FLOOR)
    _, flags, qmap = imaging.plane_view(np.zeros((0, 2200, 3208, 1), np.uint8), row, grid, want_flags=True, want_map=True)
    assert flags.shape == (225, 300) and not flags.any()
    world = grid.world_points().reshape(-1, 3)
    uv = _native.project_rows(world, np.broadcast_to(row, (world.shape[0], row.shape[0])).copy()).reshape(225, 300, 2)
    err = np.abs(qmap / 32.0 - uv).max()
    print(f"max |q / 32 - sba_project| = {err:.7f} px (bound {MAP_BOUND:.6f})")
    assert err <= MAP_BOUND
    # the (Lens, R, t) form of the same camera gives the same map
    triple = (Lens.from_camera_row(row), imaging.rodrigues(row[:3]), row[3:6])
    assert np.array_equal(imaging.plane_view(np.zeros((0, 2200, 3208, 1), np.uint8), triple, grid, want_map=True)[2], qmap)


def test_plane_mosaic_of_two_cameras_over_one_floor_texture(torch):
    grid, rows = two_floor_cameras()
    for row in rows:
        row[7:9] = 0.0                                        # pinhole cameras: the way from a camera's pixel to the floor is a matrix
    w, h = grid.size
    texture = np.random.default_rng(17).integers(0, 256, size=(2, h, w, 3), dtype=np.uint8)
    sources, want = [], []
    for row in rows:                                          # what each camera sees: the texture warped into it, nearest rule
        lens = Lens.from_camera_row(row)
        to_texture = np.linalg.inv(grid.matrix(row)) @ np.linalg.inv(lens.camera_matrix)
        src = imaging.warp_frames(texture, Lens(*IDENTITY_LENS), to_texture, (61, 47), interpolation="nearest")
        assert np.array_equal(src, warp_oracle(texture, IDENTITY_LENS, to_texture, (47, 61), nearest=True)[0])
        sources.append(src)
        want.append(warp_oracle(src, lens.as_tuple(), grid.matrix(row), (h, w), nearest=True))
    owner_want = brute_force_owner([x[1] for x in want], [x[2] for x in want], [(61, 47)] * 2)
    assert set(np.unique(owner_want)) == {-1, 0, 1}
    by_hand = np.full_like(texture, 77)
    for k in range(2):
        by_hand[:, owner_want == k] = want[k][0][:, owner_want == k]
    for dev in (False, True):
        views, flags, maps = [], [], []
        for k, row in enumerate(rows):
            src = torch.from_numpy(sources[k]).cuda() if dev else sources[k]
            v, f, q = imaging.plane_view(src, row, grid, interpolation="nearest", want_flags=True, want_map=True)
            assert np.array_equal(f, want[k][1]) and np.array_equal(q, want[k][2])
            views.append(v), flags.append(f), maps.append(q)
        mosaic, owner = imaging.plane_mosaic(views, flags, maps, [(61, 47)] * 2, fill=77)
        if dev:
            assert mosaic.is_cuda and owner.is_cuda
            mosaic, owner = mosaic.cpu().numpy(), owner.cpu().numpy()
        assert np.array_equal(owner, owner_want) and np.array_equal(mosaic, by_hand)
    # What the mosaic shows is the floor itself.  A camera pixel is some 75 mm of floor, a pixel of the grid 200 mm: the source
    # pixel nearest to a grid point lies within 0.5 + 1/64 pixels of it, about 45 mm on the tilted floor, and so inside the grid
    # point's own 200 mm cell, whose texture value that source pixel took.
    seen = owner_want >= 0
    assert np.array_equal(by_hand[:, seen], texture[:, seen])
