"""CPU tests of the sub-pixel corner refinement (sba_refine_corners, include/sba_hip.h; ``imaging.refine_corners``): the numpy
oracle the GPU tests compare against bit for bit, pinned to answers known without it, and the host side of the Python interface.

``refine_corners_oracle`` restates the header's rule.  The patch and the per-position products are numpy element-wise float64
operations (one IEEE operation each, never fused); the five sums are scalar loops over Python floats in the rule's order: per
window row from left to right starting from 0.0, the row totals from top to bottom starting from 0.0.  The window's weights are
``math.exp`` per entry.

MEASURED when this file was written (``rendered_corners``: 80 checker corners of 40 x 44 pixels at random sub-pixel centres,
edges 0.3 .. pi/2 - 0.3 rad from the image axes, box-filtered 8 x 8 per pixel, four starts within +-2 px each): every start
converges, in at most 17 iterations; the four results of a corner agree within 2.2e-5 px; the worst distance to the true
centre is 0.0929 px (what rounding to bytes and the box filter of a pixel leave of a corner's position in a 7 x 7 window).
``TRUTH_BOUND`` is 1.25 x that.
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lasercalib_amd import _native, imaging  # noqa: E402
from test_resize_host import GRAY_BGR, resize_oracle  # noqa: E402

CONVERGED, MAX_ITER, SINGULAR, LEFT_IMAGE, RESTORED, INVALID = 1, 2, 4, 8, 16, 32
WORST_TRUTH_PX = 0.0929                                        # measured: see the module's docstring
TRUTH_BOUND = 1.25 * WORST_TRUTH_PX


# ----------------------------------------------------------------------------- the oracle
def window_oracle(win, zero_zone=(-1, -1)):
    (wx, wy), (zx, zy) = win, zero_zone
    m = np.empty((2 * wy + 1, 2 * wx + 1))
    for i in range(2 * wy + 1):
        yy = float(i - wy) / float(wy)
        vy = math.exp(-(yy * yy))
        for j in range(2 * wx + 1):
            xx = float(j - wx) / float(wx)
            m[i, j] = vy * math.exp(-(xx * xx))
    if zx >= 0 and zy >= 0 and zx < wx and zy < wy:
        m[wy - zy:wy + zy + 1, wx - zx:wx + zx + 1] = 0.0
    return m


def tap_plane(image, channel=None, gray_w=GRAY_BGR):
    """T of the rule as a float64 (H, W) array: byte ``channel`` of (H, W, C) or (H, W) pixels, or with -1 the grey value."""
    image = np.asarray(image)
    if image.ndim == 2:
        image = image[..., None]
    if channel is None:
        channel = 0 if image.shape[2] == 1 else -1
    if channel == -1:
        return resize_oracle(image[None], 1, 1, gray_w)[0].astype(np.float64)
    return image[:, :, channel].astype(np.float64)


def two_level_sum(values):
    total = 0.0
    for row in values.tolist():
        r = 0.0
        for v in row:
            r = r + v
        total = total + r
    return total


def refine_one(T, x, y, wx, wy, m, max_iter, eps2, patch32=False):
    """The rule for one corner on the tap plane T -> (rx, ry, status, iterations, (a, b, c)).  ``patch32`` is NOT the rule: the
    patch rounded to float32, as OpenCV holds it, to measure what that is worth (test_oracle_against_opencv)."""
    H, W = T.shape
    if not (math.isfinite(x) and math.isfinite(y)) or abs(x) >= 32768.0 or abs(y) >= 32768.0:
        return x, y, INVALID, 0, (0.0, 0.0, 0.0)
    jj, ii = np.arange(-(wx + 1), wx + 2), np.arange(-(wy + 1), wy + 2)
    dj, di = np.arange(-wx, wx + 1, dtype=np.float64)[None, :], np.arange(-wy, wy + 1, dtype=np.float64)[:, None]
    cx, cy, it, tensor, status = x, y, 0, (0.0, 0.0, 0.0), 0
    while True:
        ix, iy = math.floor(cx), math.floor(cy)
        ax, ay = cx - ix, cy - iy
        w, h = 1.0 - ax, 1.0 - ay
        u0, u1 = np.clip(ix + jj, 0, W - 1)[None, :], np.clip(ix + jj + 1, 0, W - 1)[None, :]
        v0, v1 = np.clip(iy + ii, 0, H - 1)[:, None], np.clip(iy + ii + 1, 0, H - 1)[:, None]
        top = w * T[v0, u0] + ax * T[v0, u1]
        bot = w * T[v1, u0] + ax * T[v1, u1]
        S = h * top + ay * bot
        if patch32:
            S = S.astype(np.float32).astype(np.float64)
        gx, gy = S[1:-1, 2:] - S[1:-1, :-2], S[2:, 1:-1] - S[:-2, 1:-1]
        gxx, gxy, gyy = (gx * gx) * m, (gx * gy) * m, (gy * gy) * m
        e1, e2 = gxx * dj + gxy * di, gxy * dj + gyy * di
        a, b, c, b1, b2 = (two_level_sum(v) for v in (gxx, gxy, gyy, e1, e2))
        tensor = (a, b, c)
        det = a * c - b * b
        if not abs(det) > 2.0 ** -104:
            status = SINGULAR
            break
        s = 1.0 / det
        nx = (cx + (c * s) * b1) - (b * s) * b2
        ny = (cy - (b * s) * b1) + (a * s) * b2
        err = (nx - cx) * (nx - cx) + (ny - cy) * (ny - cy)
        cx, cy, it = nx, ny, it + 1
        if not (0.0 <= cx < W and 0.0 <= cy < H):
            status = LEFT_IMAGE
            break
        if err <= eps2:
            status = CONVERGED
            break
        if it == max_iter:
            status = MAX_ITER
            break
    if abs(cx - x) > wx or abs(cy - y) > wy:
        cx, cy, status = x, y, status | RESTORED
    return cx, cy, status, it, tensor


def refine_corners_oracle(image, corners, win=(3, 3), zero_zone=(-1, -1), max_iter=200, eps=1e-5, channel=None, gray_w=GRAY_BGR,
                          weights=None, patch32=False):
    """The rule of include/sba_hip.h for one image (H, W) or (H, W, C) uint8 and (n, 2) corners ->
    (refined (n, 2) float64, status (n,) int32, iterations (n,) int32, tensor (n, 3) float64)."""
    T = tap_plane(image, channel, gray_w)
    wx, wy = win
    m = window_oracle(win, zero_zone) if weights is None else np.asarray(weights, dtype=np.float64)
    corners = np.asarray(corners, dtype=np.float64).reshape(-1, 2)
    n = len(corners)
    refined, status, iterations, tensor = np.zeros((n, 2)), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 3))
    for k, (x, y) in enumerate(corners.tolist()):
        rx, ry, status[k], iterations[k], tensor[k] = refine_one(T, x, y, wx, wy, m, max_iter, float(eps) * float(eps), patch32)
        refined[k] = rx, ry
    return refined, status, iterations, tensor


def batch_oracle(frames, corners_per_frame, **kw):
    """The oracle over a batch: the four arrays over all corners in order."""
    parts = [refine_corners_oracle(f, c, **kw) for f, c in zip(frames, corners_per_frame)]
    return tuple(np.concatenate([p[i] for p in parts]) if parts else None for i in range(4))


# ----------------------------------------------------------------------------- rendered images
def render_corner(H, W, qx, qy, theta=0.0, lo=40, hi=200, ss=8):
    """An (H, W) uint8 checker corner at (qx, qy) (pixel (u, v) covers [u - 0.5, u + 0.5] x [v - 0.5, v + 0.5]), its edges
    turned by theta from the image axes, every pixel the mean of ss x ss point samples, rounded to a byte."""
    off = (np.arange(ss) + 0.5) / ss - 0.5
    X = (np.arange(W)[:, None] + off[None, :]).reshape(-1)[None, :] - qx
    Y = (np.arange(H)[:, None] + off[None, :]).reshape(-1)[:, None] - qy
    d1, d2 = X * math.cos(theta) + Y * math.sin(theta), -X * math.sin(theta) + Y * math.cos(theta)
    fine = np.where(d1 * d2 > 0, float(hi), float(lo))
    return np.rint(fine.reshape(H, ss, W, ss).mean(axis=(1, 3))).astype(np.uint8)


RENDERED = {}


def rendered_corners(n=80, H=40, W=44, seed=5):
    """n (image, true centre) pairs; shared, never written."""
    if (n, H, W, seed) not in RENDERED:
        rng = np.random.default_rng(seed)
        out = []
        for _ in range(n):
            qx, qy = W / 2 + rng.uniform(-3, 3), H / 2 + rng.uniform(-3, 3)
            img = render_corner(H, W, qx, qy, rng.uniform(0.3, math.pi / 2 - 0.3), lo=int(rng.integers(10, 80)), hi=int(rng.integers(150, 250)))
            img.setflags(write=False)
            out.append((img, (qx, qy)))
        RENDERED[n, H, W, seed] = out
    return RENDERED[n, H, W, seed]


def four_starts(q, rng):
    return np.array(q)[None, :] + rng.uniform(-2, 2, size=(4, 2))


def symmetric_corner():
    return render_corner(40, 44, 22, 19), (22.0, 19.0)


# ----------------------------------------------------------------------------- the oracle, pinned
def test_exact_fixed_point_and_return_to_truth():
    img, q = symmetric_corner()
    sub = img[0:39, 1:44]                                      # rows and columns at equal distances from (22, 19)
    assert np.array_equal(sub, sub[::-1, ::-1])                # point-symmetric
    assert img[19, 5] == 120 and img[5, 22] == 120 and img[30, 30] == 200 and img[30, 5] == 40     # the mid row and column are exact
    refined, status, iterations, tensor = refine_corners_oracle(img, [q])
    assert refined[0].tolist() == [22.0, 19.0] and status[0] == CONVERGED and iterations[0] == 1
    assert tensor[0, 0] > 0 and tensor[0, 2] > 0
    start = (22.0 + 1.3 * math.cos(0.7), 19.0 + 1.3 * math.sin(0.7))
    refined, status, iterations, _ = refine_corners_oracle(img, [start])
    print("return to truth:", np.hypot(*(refined[0] - q)), "px after", iterations[0], "iterations")
    assert status[0] == CONVERGED and np.hypot(*(refined[0] - q)) < 1e-5


def test_rendered_corners_from_four_starts():
    rng = np.random.default_rng(17)
    worst_truth = worst_spread = worst_it = 0
    for img, q in rendered_corners():
        refined, status, iterations, _ = refine_corners_oracle(img, four_starts(q, rng))
        assert np.all(status == CONVERGED), (q, status)
        worst_spread = max(worst_spread, np.max(np.hypot(*(refined - refined[0]).T)))
        worst_truth = max(worst_truth, np.max(np.hypot(*(refined - np.array(q)).T)))
        worst_it = max(worst_it, int(iterations.max()))
    print(f"rendered corners: worst distance to truth {worst_truth:.4f} px, spread between starts {worst_spread:.2e} px, "
          f"at most {worst_it} iterations")
    assert worst_spread < 1e-4
    assert worst_truth <= TRUTH_BOUND


def test_constant_image_and_straight_edge_are_singular():
    flat = np.full((40, 44), 90, np.uint8)
    edge = flat.copy()
    edge[:, 20:] = 200
    for img in (flat, edge, edge.T.copy()):
        refined, status, iterations, tensor = refine_corners_oracle(img, [(20.4, 18.6)])
        assert status[0] == SINGULAR and iterations[0] == 0 and refined[0].tolist() == [20.4, 18.6]
    assert tensor[0, 0] == 0 and tensor[0, 2] > 0              # the transposed edge: only gy


def test_window_over_the_edge_converges_under_border_replication():
    # the replica of the border rows and columns continues slanted edges straight up and to the left: the picture the window
    # sees is no longer a true corner, so what is asked is convergence, within a pixel of the truth
    img = render_corner(40, 44, 2.3, 1.7, 0.6)
    refined, status, _, _ = refine_corners_oracle(img, [(2.0, 2.0)])
    assert status[0] == CONVERGED and np.hypot(*(refined[0] - (2.3, 1.7))) < 1.0
    img = render_corner(40, 44, 41.6, 38.2, 0.6)               # and at the far corner of the frame
    refined, status, _, _ = refine_corners_oracle(img, [(42.0, 38.0)])
    assert status[0] == CONVERGED and np.hypot(*(refined[0] - (41.6, 38.2))) < 1.0


def test_a_start_outside_the_windows_reach_is_restored():
    img, q = symmetric_corner()
    start = (q[0] + 2.0, q[1] + 2.0)                          # 2 px from the corner, the window reaches 1
    refined, status, iterations, _ = refine_corners_oracle(img, [start], win=(1, 1))
    assert status[0] & RESTORED and iterations[0] >= 1 and refined[0].tolist() == list(start)
    res = imaging.CornerRefinement(refined, refined, status, iterations, np.ones((1, 3)))
    assert not res.ok[0]


def test_non_finite_and_huge_inputs_are_invalid():
    img, _ = symmetric_corner()
    bad = [(np.nan, 3.0), (3.0, np.inf), (-np.inf, 2.0), (32768.0, 5.0), (5.0, -32768.0), (1e300, 1.0)]
    refined, status, iterations, tensor = refine_corners_oracle(img, bad + [(22.0, 19.0)])
    assert np.all(status[:6] == INVALID) and status[6] == CONVERGED and not iterations[:6].any() and not tensor[:6].any()
    assert np.array_equal(refined[:6], np.array(bad), equal_nan=True)
    refined, status, _, _ = refine_corners_oracle(img, [(32767.5, 5.0), (-100.0, -100.0)])      # in range: read with the border replicated
    assert np.all(status == SINGULAR)


def test_leaving_the_image_and_max_iter():
    img = render_corner(40, 44, 1.2, 20.0, 0.7)
    found = set()
    for x in np.linspace(0.1, 6.0, 60):
        _, status, iterations, _ = refine_corners_oracle(img, [(x, 23.0)], max_iter=3)
        found.add(int(status[0]))
        assert 1 <= iterations[0] <= 3 or status[0] & SINGULAR
    assert any(s & MAX_ITER for s in found)
    print("statuses met near the border with max_iter = 3:", sorted(found))


def test_zero_zone():
    img, q = rendered_corners()[0]
    start = [(q[0] + 0.8, q[1] - 0.6)]
    plain = refine_corners_oracle(img, start)
    zeroed = refine_corners_oracle(img, start, zero_zone=(1, 1))
    assert zeroed[1][0] == CONVERGED and not np.array_equal(plain[0], zeroed[0])
    for ignored in ((3, 3), (3, 1), (1, 3), (-1, 1), (5, 5)):              # as large as the window, or half of it negative
        again = refine_corners_oracle(img, start, zero_zone=ignored)
        assert all(np.array_equal(p, a) for p, a in zip(plain, again)), ignored
    m = window_oracle((3, 2), (1, 0))
    assert m.shape == (5, 7) and not m[2, 2:5].any() and np.count_nonzero(m) == 35 - 3 and m[2, 1] == math.exp(-(2 / 3) ** 2)
    assert np.array_equal(m, imaging.corner_window((3, 2), (1, 0)))


def test_grey_equals_the_plane_of_the_resize_oracle():
    rng = np.random.default_rng(3)
    img, q = rendered_corners()[1]
    colour = np.stack([img, 255 - img, (img // 2 + 30).astype(np.uint8)], axis=-1)
    colour = np.clip(colour.astype(int) + rng.integers(-3, 4, size=colour.shape), 0, 255).astype(np.uint8)
    for weights in (GRAY_BGR, (1 << 15, 0, 0), (10000, 10000, 12768)):
        plane = resize_oracle(colour[None], 1, 1, weights)[0]
        want = refine_corners_oracle(plane, [q, (q[0] + 1, q[1] - 1)])
        got = refine_corners_oracle(colour, [q, (q[0] + 1, q[1] - 1)], channel=-1, gray_w=weights)
        assert all(np.array_equal(w, g) for w, g in zip(want, got))
    four = np.concatenate([colour, np.full(colour.shape[:2] + (1,), 7, np.uint8)], axis=-1)     # a fourth channel is ignored
    assert all(np.array_equal(w, g) for w, g in zip(refine_corners_oracle(colour, [q]), refine_corners_oracle(four, [q])))
    assert np.array_equal(refine_corners_oracle(colour, [q], channel=1)[0], refine_corners_oracle(colour[..., 1], [q])[0])


# ----------------------------------------------------------------------------- the Python side
def test_struct_size_and_status_bits():
    assert ctypes.sizeof(_native.CornerOpts) == 72 and _native.CornerOpts.eps.offset == 0 and _native.CornerOpts.reserved.offset == 52
    assert (_native.CORNER_CONVERGED, _native.CORNER_MAX_ITER, _native.CORNER_SINGULAR, _native.CORNER_LEFT_IMAGE, _native.CORNER_RESTORED,
            _native.CORNER_INVALID) == (CONVERGED, MAX_ITER, SINGULAR, LEFT_IMAGE, RESTORED, INVALID)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sba_hip.h")).read()
    for name, bit in (("CONVERGED", 1), ("MAX_ITER", 2), ("SINGULAR", 4), ("LEFT_IMAGE", 8), ("RESTORED", 16), ("INVALID", 32)):
        assert f"SBA_CORNER_{name} = {bit}" in header


@pytest.fixture
def oracle_native(monkeypatch):
    """``_native.refine_corners`` answered by the oracle: the host side of the public calls without a GPU."""
    calls = []

    def fake(frames, corner_start, corners, win=(3, 3), zero_zone=(-1, -1), max_iter=200, eps=1e-5, channel=0, gray_w=None,
             weights=None, chunk_frames=0, device=0):
        calls.append(dict(win=win, zero_zone=zero_zone, max_iter=max_iter, eps=eps, channel=channel, gray_w=gray_w, weights=weights))
        per_frame = [corners[corner_start[f]:corner_start[f + 1]] for f in range(len(frames))]
        return batch_oracle(frames, per_frame, win=win, max_iter=max_iter, eps=eps, channel=channel,
                            gray_w=GRAY_BGR if gray_w is None else gray_w, weights=weights)

    monkeypatch.setattr(_native, "refine_corners", fake)
    return calls


def test_value_errors_of_the_public_call(oracle_native):
    img, q = symmetric_corner()
    frames = img[None]
    for kw in (dict(win=(0, 3)), dict(win=(3, 16)), dict(win=3), dict(win=(2.5, 3)), dict(max_iter=0), dict(max_iter=10001),
               dict(eps=-1e-3), dict(eps=float("nan")), dict(channel=1), dict(channel=-1), dict(weights=np.ones((7, 5))),
               dict(weights=-np.ones((7, 7))), dict(weights=np.full((7, 7), np.inf)), dict(zero_zone=(1,))):
        with pytest.raises(ValueError):
            imaging.refine_corners(frames, [np.array([q])], **kw)
    with pytest.raises(ValueError, match="per frame"):
        imaging.refine_corners(np.stack([img, img]), np.array([q]))
    with pytest.raises(ValueError, match="per frame"):
        imaging.refine_corners(frames, [np.array([q]), np.array([q])])
    with pytest.raises(ValueError, match=r"\(k, 2\)"):
        imaging.refine_corners(frames, [np.zeros((2, 3))])
    with pytest.raises(ValueError, match="channel"):
        imaging.refine_corners(np.zeros((1, 8, 8, 3), np.uint8), [np.zeros((0, 2))], channel=3)
    assert not oracle_native


def test_shapes_defaults_and_explicit_weights_of_the_public_call(oracle_native):
    img, q = symmetric_corner()
    res = imaging.refine_corners(img[None], np.array([q, (23.0, 20.0)]))
    assert isinstance(res.corners, np.ndarray) and res.corners.shape == (2, 2) and res.ok.tolist() == [True, True]
    call = oracle_native[-1]
    assert call["channel"] == 0 and call["gray_w"] is None and np.array_equal(call["weights"], window_oracle((3, 3)))
    colour = np.repeat(img[None, :, :, None], 3, axis=3)
    res = imaging.refine_corners(np.concatenate([colour, colour, colour]), [np.array([q]), np.zeros((0, 2)), [q, q]], zero_zone=(1, 1),
                                 channel_order="rgb")
    assert [c.shape for c in res.corners] == [(1, 2), (0, 2), (2, 2)] and res.status.shape == (3,) and res.tensor.shape == (3, 3)
    call = oracle_native[-1]
    assert call["channel"] == -1 and tuple(call["gray_w"]) == GRAY_BGR[::-1] and np.array_equal(call["weights"], window_oracle((3, 3), (1, 1)))
    cov = res.covariance_shape()
    a, b, c = res.tensor[0]
    assert cov.shape == (3, 2, 2) and np.allclose(cov[0] @ np.array([[a, b], [b, c]]), np.eye(2), atol=1e-12)
    flat = imaging.refine_corners(np.full((1, 9, 9), 5, np.uint8), np.array([(4.0, 4.0)]))
    assert flat.status[0] == SINGULAR and not flat.ok[0] and np.all(np.isnan(flat.covariance_shape()))


def test_corner_sub_pix_keeps_shape_and_dtype(oracle_native):
    img, q = symmetric_corner()
    pts = np.array([[[q[0] + 0.4, q[1] - 0.3]], [[q[0] - 1.0, q[1] + 0.5]]], np.float32)         # (n, 1, 2) float32, as cv.aruco returns
    out = imaging.corner_sub_pix(img, pts, (3, 3), (-1, -1), (3, 200, 1e-5))
    assert out.shape == (2, 1, 2) and out.dtype == np.float32 and np.all(np.abs(out.reshape(-1, 2) - q) < 1e-3)
    assert oracle_native[-1]["max_iter"] == 200 and oracle_native[-1]["eps"] == 1e-5
    want = refine_corners_oracle(img, pts.reshape(-1, 2).astype(np.float64))[0]
    assert np.array_equal(out.reshape(-1, 2), want.astype(np.float32))
    out = imaging.corner_sub_pix(img, pts.reshape(2, 2).astype(np.float64), (2, 4), (-1, -1), (1, 7, 0.5))     # COUNT only: eps 0
    assert out.shape == (2, 2) and out.dtype == np.float64
    assert oracle_native[-1]["win"] == (2, 4) and oracle_native[-1]["max_iter"] == 7 and oracle_native[-1]["eps"] == 0.0
    imaging.corner_sub_pix(img, pts, (3, 3), (-1, -1), (2, 7, 0.5))                                          # EPS only: OpenCV's 100
    assert oracle_native[-1]["max_iter"] == 100 and oracle_native[-1]["eps"] == 0.5
    with pytest.raises(ValueError):
        imaging.corner_sub_pix(img[None, None], pts)
    with pytest.raises(ValueError):
        imaging.corner_sub_pix(img, np.zeros((4, 3)))


def test_corner_weights_on_a_hand_made_tensor():
    # eigenvalues of [[a, b], [b, c]]: (5, 0, 5) -> 5, 5; (10, 0, 2) -> 10, 2; (5, 3, 5) -> 8, 2; (4, 0, 0) -> 4, 0 (an edge)
    tensor = np.array([[5.0, 0, 5], [10, 0, 2], [5, 3, 5], [4, 0, 0], [9, 0, 9], [7, 0, 7]])
    status = np.array([CONVERGED, CONVERGED, CONVERGED, CONVERGED, CONVERGED | RESTORED, MAX_ITER], np.int32)
    res = imaging.CornerRefinement(None, np.zeros((6, 2)), status, np.ones(6, np.int32), tensor)
    assert res.ok.tolist() == [True, True, True, True, False, False]
    w = imaging.corner_weights(res)                            # smaller eigenvalues of the ok ones: 5, 2, 2, 0 -> median 2
    assert np.allclose(w, [2.5, 1.0, 1.0, 0.0, 0.0, 0.0]) and np.median(w[:4]) == 1.0
    assert np.allclose(imaging.corner_weights(res, floor=0.25), [2.5, 1.0, 1.0, 0.25, 0.0, 0.0])
    none_ok = imaging.CornerRefinement(None, np.zeros((1, 2)), np.array([SINGULAR], np.int32), np.zeros(1, np.int32), np.zeros((1, 3)))
    assert imaging.corner_weights(none_ok).tolist() == [0.0]


def test_oracle_against_opencv():
    """Within the reach of a float32 patch, measured here: the largest distance between the oracle and the oracle with its patch
    rounded to float32 on the same corners.  OpenCV also holds its window and its bilinear coefficients in float32 and stops,
    as the oracle does, within eps = 1e-5 px of its fixed point: 8 x the reach plus 2 eps is asked.  (cv2 was not installed where this was written:
    the reach came out at 7.6e-8 px, the comparison itself has not run.)"""
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(23)
    worst = reach = 0.0
    for img, q in rendered_corners()[:20]:
        starts = four_starts(q, rng).astype(np.float32).astype(np.float64)
        ours = refine_corners_oracle(img, starts)[0]
        reach = max(reach, float(np.max(np.abs(ours - refine_corners_oracle(img, starts, patch32=True)[0]))))
        theirs = cv2.cornerSubPix(np.array(img), starts.astype(np.float32).reshape(-1, 1, 2), (3, 3), (-1, -1),
                                  (cv2.TERM_CRITERIA_EPS + cv2.TERM_CRITERIA_MAX_ITER, 200, 1e-5)).reshape(-1, 2)
        worst = max(worst, float(np.max(np.abs(ours - theirs))))
    print("oracle against cv2.cornerSubPix: worst difference", worst, "px; reach of a float32 patch", reach, "px")
    assert worst <= 8 * reach + 2e-5
