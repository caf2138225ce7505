"""GPU: the reason sba_background_* exists.  A lamp and a reflection that are lit in every frame make find_laser_blobs answer
MULTIPLE for a whole video; with the background learned from the same frames and gated out, both detectors return, bit for bit,
what they return on the same video rendered without lamp and reflection.

Bit equality rests on two conditions on the scene, which the tests assert on their own inputs with the numpy oracle:
  1. outside the mask the level is nowhere above the detectors' threshold: the gate then removes no pixel that counts;
  2. the spot's pixels above the threshold stay farther from the mask than the morphology reaches
     (dilate_radius + 2 close_radius pixels).
A third frame set lets the spot cross the lamp: there the dot is lost or shrunk -- the limitation, not a rescue."""
import os
import sys

import numpy as np
import pytest

from lasercalib_amd import feature_detection as fd, imaging

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_background_host import accumulate_oracle, level_oracle, suppress_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

B, H, W = 40, 96, 128
THRESHOLD, DILATE, CLOSE = 70, 1, 4
REACH = DILATE + 2 * CLOSE
LAMP = (slice(4, 12), slice(100, 108))               # 8 x 8, flickering 180..230
REFLECTION = (slice(86, 91), slice(15, 20))          # 5 x 5, a constant 90
AMP, SIGMA = 88.0, 2.5                                # the spot: the peak stays low enough for condition 1 with 40 frames


def clear_path():
    """Two legs, 5.5 pixels a frame: along row 30 to the right, along row 66 back; 15 rows and more from lamp and reflection."""
    f = np.arange(B)
    leg = f % 20
    x = np.where(f < 20, 10.0 + 5.5 * leg, 114.5 - 5.5 * leg)
    return np.stack([x + 0.25 * (f % 4), np.where(f < 20, 30.0, 66.0) + 0.2 * (f % 5)], axis=1)


def crossing_path():
    """The first leg along row 8, through the lamp (frames 17 and 18 lie on it), the second along row 50."""
    f = np.arange(B)
    return np.stack([8.0 + 5.5 * (f % 20) + 0.25 * (f % 4), np.where(f < 20, 8.0, 50.0) + 0.2 * (f % 5)], axis=1)


def render(path, static_light):
    """(B, H, W, 3) uint8: a Gaussian spot on the path over a dark integer pattern, green strongest; with ``static_light`` the
    lamp (its green flickers by a fixed integer sequence) and the reflection on top."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    f = np.arange(B)[:, None, None]
    dark = ((x[None] * 7 + y[None] * 13 + f * 3) % 4).astype(np.float64)
    r2 = (x[None] - path[:, 0, None, None]) ** 2 + (y[None] - path[:, 1, None, None]) ** 2
    green = np.clip(np.rint(dark + AMP * np.exp(-0.5 * r2 / SIGMA ** 2)), 0, 255).astype(np.uint8)
    frames = np.stack([green // 3, green, green // 4], axis=-1)
    if static_light:
        ly, lx = np.mgrid[LAMP[0], LAMP[1]]
        frames[(slice(None),) + LAMP + (1,)] = (180 + (f * 7 + lx[None] * 3 + ly[None] * 5) % 51).astype(np.uint8)
        frames[(slice(None),) + REFLECTION + (1,)] = 90
    return frames


SCENE = {}


def scene(name):
    """raw and clean frames of the path ``name``, and the model's level and mask by the oracle; rendered once, never written."""
    if name not in SCENE:
        path = clear_path() if name == "clear" else crossing_path()
        raw, clean = render(path, True), render(path, False)
        acc = accumulate_oracle(raw, channel=1, threshold=THRESHOLD)
        level = level_oracle(acc, 4.0, 4)
        mask = imaging.BackgroundModel.from_state(dict(acc, height=H, width=W, channel=1, threshold=THRESHOLD), on_device=False).hot_mask(0.5, grow=2)
        for a in (raw, clean, level, mask):
            a.setflags(write=False)
        SCENE[name] = raw, clean, level, mask
    return SCENE[name]


def assert_conditions(raw, clean, level, mask):
    assert mask[LAMP].all() and mask[REFLECTION].all() and mask.sum() < 400, "the mask is lamp and reflection, grown by 2"
    assert int(level[mask == 0].max()) <= THRESHOLD, "condition 1: outside the mask the level stays at or below the threshold"
    my, mx = np.nonzero(mask)
    for f in range(B):
        sy, sx = np.nonzero(clean[f, ..., 1] > THRESHOLD)
        assert sy.size >= 5, "the spot shows in every frame"
        d2 = (sy[:, None] - my[None]) ** 2 + (sx[:, None] - mx[None]) ** 2
        assert d2.min() > REACH ** 2, f"condition 2: frame {f} has a spot pixel within {REACH} pixels of the mask"
    # what follows from them: gated raw frames and clean frames show the detectors the same pixels above the threshold
    gated = suppress_oracle(raw, channel=1, level=level, mask=mask, mode="gate")
    g = clean[..., 1]
    assert np.array_equal(gated > THRESHOLD, g > THRESHOLD) and np.array_equal(gated[g > THRESHOLD], g[g > THRESHOLD])


def test_scene_meets_the_conditions_of_bit_equality():
    assert_conditions(*scene("clear"))


@pytest.fixture(scope="module")
def model():
    raw = scene("clear")[0]
    m = imaging.BackgroundModel(H, W, channel=1, threshold=THRESHOLD)
    m.add(raw[:13]).add(raw[13:])
    return m


def test_model_from_raw_frames_is_the_oracles(model):
    raw, _clean, level, mask = scene("clear")
    acc = accumulate_oracle(raw, channel=1, threshold=THRESHOLD)
    st = model.state()
    assert model.n == B and all(np.array_equal(st[k], acc[k]) and st[k].dtype == acc[k].dtype for k in ("sum", "sumsq", "hot", "vmax"))
    assert np.array_equal(model.level(4, 4), level) and np.array_equal(model.hot_mask(0.5, grow=2), mask)
    import torch
    for src in (raw, torch.tensor(raw).cuda()):
        got = model.suppress(src, level=level, mask=mask)
        got = got if isinstance(got, np.ndarray) else got.cpu().numpy()
        assert np.array_equal(got, suppress_oracle(raw, 1, level, mask, "gate"))


@pytest.mark.parametrize("on_device", [False, True])
def test_blobs_lamp_makes_every_frame_multiple_and_the_model_cures_it(model, on_device):
    raw, clean, level, mask = scene("clear")
    if on_device:
        import torch
        raw_in, clean_in = torch.tensor(raw).cuda(), torch.tensor(clean).cuda()
    else:
        raw_in, clean_in = raw, clean
    kw = dict(threshold=THRESHOLD, dilate_radius=DILATE, close_radius=CLOSE)
    sick = fd.find_laser_blobs(raw_in, **kw)
    assert np.all(sick.status == fd.SBA_BLOB_MULTIPLE) and np.all(sick.n_components == 3), "the problem: no frame of this camera is usable"
    want = fd.find_laser_blobs(clean_in, want_mask=True, **kw)
    assert np.all(want.status == fd.SBA_BLOB_OK)
    # the pair with the parameters the scene was checked for, and the model by itself (its default mask is not grown)
    for background, chunk in (((model.level(4, 4), model.hot_mask(0.5, grow=2)), 0), ((level, mask), 7), (model, 0)):
        got = fd.find_laser_blobs(raw_in, background=background, chunk_frames=chunk, want_mask=True, **kw)
        assert np.all(got.status == fd.SBA_BLOB_OK)
        assert np.array_equal(got.n_components, want.n_components) and np.array_equal(got.accepted, want.accepted)
        assert np.array_equal(got.blobs, want.blobs), "component records differ"
        assert got.centroid.tobytes() == want.centroid.tobytes() and np.array_equal(got.mask, want.mask)
    path = clear_path()
    assert np.max(np.abs(want.centroid[:, 2:] - path)) < 0.3          # and the centroids are where the spot was put


def test_dots_with_the_model_equal_dots_on_clean_frames(model):
    raw, clean, level, mask = scene("clear")
    kw = dict(threshold=THRESHOLD, max_extent=24)
    sick = fd.find_laser_dots(raw, **kw)
    assert np.all(sick.status == fd.SBA_DOT_SPREAD)
    want = fd.find_laser_dots(clean, **kw)
    assert np.all(want.status == fd.SBA_DOT_OK)
    import torch
    for src in (raw, torch.tensor(raw).cuda()):
        for chunk in (0, 16):
            got = fd.find_laser_dots(src, background=(level, mask), chunk_frames=chunk, **kw)
            assert np.array_equal(got.status, want.status) and np.array_equal(got.sums, want.sums) and np.array_equal(got.box, want.box)
            assert got.centroid.tobytes() == want.centroid.tobytes()
    with pytest.raises(ValueError, match="channel"):
        fd.find_laser_dots(raw, channel=0, background=model)


def test_spot_crossing_the_lamp_is_lost_not_rescued():
    raw, clean, level, mask = scene("crossing")
    kw = dict(threshold=THRESHOLD, dilate_radius=DILATE, close_radius=CLOSE)
    want = fd.find_laser_blobs(clean, **kw)
    got = fd.find_laser_blobs(raw, background=(level, mask), **kw)
    overlap = [f for f in range(B) if np.any((clean[f, ..., 1] > THRESHOLD) & (mask != 0))]
    assert len(overlap) >= 2, "the path crosses the lamp"
    for f in range(B):
        if f in overlap:
            lost = got.status[f] == fd.SBA_BLOB_NONE
            n_raw = int(got.blobs[f, 0, 3]) if not lost else 0
            assert lost or n_raw < int(want.blobs[f, 0, 3]), f"frame {f}: the masked part of the spot cannot come back"
            if got.status[f] == fd.SBA_BLOB_OK:
                cx, cy = got.centroid[f, 2:]
                assert mask[int(round(cy)), int(round(cx))] == 0, f"frame {f}: a weighted centroid inside the mask"
        elif np.min(_dist_to_mask(clean[f, ..., 1] > THRESHOLD, mask)) > REACH:
            assert got.status[f] == fd.SBA_BLOB_OK and np.array_equal(got.blobs[f], want.blobs[f])


def _dist_to_mask(spot, mask):
    sy, sx = np.nonzero(spot)
    my, mx = np.nonzero(mask)
    return np.sqrt(((sy[:, None] - my[None]) ** 2 + (sx[:, None] - mx[None]) ** 2).astype(np.float64)).ravel()
