"""CPU tests of the per-frame value histograms (sba_frame_histograms, include/sba_hip.h; ``imaging.FrameHistograms``): the numpy
oracle the GPU tests compare against bit for bit, its identity with the laser-dot oracle, and the host-side methods of
``FrameHistograms`` on hand-built histograms with known answers.

``hist_oracle`` restates the header's rule: ``np.bincount`` of the channel over the pixels inside both regions, the regions as
the per-pixel mask ``roi_mask`` of tests/test_detect_host.py that ``dots_oracle`` uses.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lasercalib_amd.imaging import FrameHistograms  # noqa: E402
from test_detect_host import dots_oracle, roi_mask  # noqa: E402


def hist_oracle(frames, channel=1, roi_rect=None, roi_circle=None):
    """(B, 256) uint32 histograms of (B, H, W, C) or (B, H, W) uint8 frames by the definition of include/sba_hip.h."""
    frames = np.asarray(frames)
    if frames.ndim == 3:
        frames = frames[..., None]
    B, H, W, _ = frames.shape
    keep = roi_mask(H, W, roi_rect, roi_circle)
    return np.stack([np.bincount(frames[f, :, :, channel][keep], minlength=256) for f in range(B)]).astype(np.uint32).reshape(B, 256)


def of(*rows):
    """FrameHistograms of rows given as {value: count} dicts."""
    hist = np.zeros((len(rows), 256), np.uint32)
    for f, row in enumerate(rows):
        for v, n in row.items():
            hist[f, v] = n
    return FrameHistograms(hist, hist.sum(axis=0).astype(np.uint64))


# ----------------------------------------------------------------------------- the oracle
def test_oracle_equals_a_brute_force_loop_with_both_regions():
    rng = np.random.default_rng(2)
    frames = rng.integers(0, 256, size=(2, 7, 9, 3), dtype=np.uint8)
    rect, circle = (1, 0, 8, 6), (4, 3, 3)
    for channel in range(3):
        want = np.zeros((2, 256), np.uint32)
        inside = 0
        for f in range(2):
            for y in range(7):
                for x in range(9):
                    if 1 <= x < 8 and 0 <= y < 6 and (x - 4) ** 2 + (y - 3) ** 2 <= 9:
                        want[f, int(frames[f, y, x, channel])] += 1
                        inside += 1
        assert inside == 2 * (29 - 1)                       # the 29-pixel disc loses (4, 6) to the rectangle; x = 1..7 keeps the rest
        assert np.array_equal(hist_oracle(frames, channel, rect, circle), want)
    assert hist_oracle(frames, 0).sum() == 2 * 63 and hist_oracle(frames, 0).dtype == np.uint32
    assert not hist_oracle(frames, 1, roi_rect=(3, 2, 3, 5)).any()                     # an empty rectangle: 256 zeros
    assert hist_oracle(frames[..., 0], 0).sum() == 2 * 63                              # (B, H, W) is the one-channel layout


def test_count_above_is_the_n_of_the_dot_oracle_at_every_threshold():
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, size=(4, 23, 31, 3), dtype=np.uint8)
    frames[rng.random(frames.shape) < 0.5] = 0
    frames[rng.random(frames.shape) < 0.03] = 255
    for roi in ({}, dict(roi_rect=(2, 3, 29, 20), roi_circle=(15, 11, 10))):
        hist = hist_oracle(frames, 1, **roi)
        h = FrameHistograms(hist, hist.sum(axis=0).astype(np.uint64))
        above = h.count_above()
        assert above.shape == (4, 256) and above.dtype == np.int64
        for t in (0, 50, 254, 255):
            assert np.array_equal(above[:, t], dots_oracle(frames, threshold=t, channel=1, **roi).sums[:, 0].astype(np.int64)), (roi, t)
        assert np.array_equal(h.n_saturated(), dots_oracle(frames, threshold=0, channel=1, **roi).sums[:, 9].astype(np.int64))
        assert not above[:, 255].any() and h.n_saturated().min() > 0


# ----------------------------------------------------------------------------- FrameHistograms on hand-built histograms
def test_extremes_saturation_and_the_empty_region():
    h = of({3: 5, 200: 1}, {}, {255: 7}, {0: 2, 255: 1})
    assert list(h.vmin()) == [3, -1, 255, 0] and list(h.vmax()) == [200, -1, 255, 255]
    assert list(h.n_saturated()) == [0, 0, 7, 1]
    above = h.count_above()
    assert list(above[0, [0, 2, 3, 199, 200]]) == [6, 6, 1, 1, 0] and not above[1].any() and list(above[3, [0, 254, 255]]) == [1, 1, 0]
    total_only = FrameHistograms(None, h.total)              # without rows the total is the one row
    assert list(total_only.vmin()) == [0] and list(total_only.n_saturated()) == [8] and total_only.count_above()[0, 0] == 14


def test_percentile_at_the_edges_and_at_ties():
    h = of({10: 1, 20: 2, 30: 1}, {}, {7: 100})
    # frame 0: cumulative counts 1 (v = 10), 3 (20), 4 (30); n = 4
    assert list(h.percentile(0)) == [0, -1, 0]               # a count of 0 is reached at v = 0
    assert list(h.percentile(100)) == [30, -1, 7]
    assert list(h.percentile(25)) == [10, -1, 7]             # ceil(1.0) = 1: exactly reached by v = 10 -- the tie goes to the smallest v
    assert list(h.percentile(26)) == [20, -1, 7]             # ceil(1.04) = 2
    assert list(h.percentile(75)) == [20, -1, 7]             # ceil(3.0) = 3
    assert list(h.percentile(75.0000001)) == [30, -1, 7]
    assert list(h.percentile(50)) == [20, -1, 7] and list(h.percentile(1)) == [10, -1, 7]
    big = of({0: 2 ** 28 - 1, 255: 1})                      # n = 2^28: q n / 100 is 2^28 - 0.27 and 2^28 - 2.7
    assert list(big.percentile(100)) == [255] and list(big.percentile(99.9999999)) == [255] and list(big.percentile(99.999999)) == [0]


def otsu_float(row):
    """Brute force in float64: the first t of the largest w0 w1 (mu0 - mu1)^2."""
    p = row.astype(np.float64) / row.sum()
    v = np.arange(256.0)
    best, best_t = -1.0, 0
    for t in range(256):
        w0, w1 = p[:t + 1].sum(), p[t + 1:].sum()
        var = 0.0 if w0 == 0.0 or w1 == 0.0 else w0 * w1 * ((p[:t + 1] * v[:t + 1]).sum() / w0 - (p[t + 1:] * v[t + 1:]).sum() / w1) ** 2
        if var > best:
            best, best_t = var, t
    return best_t


def test_otsu_two_spikes_ties_and_a_float_brute_force():
    h = of({40: 10, 200: 3}, {}, {9: 4}, {0: 1, 255: 1}, {40: 10, 41: 10, 200: 3, 201: 3})
    # two spikes: every t in [40, 200) separates them equally well, the lowest wins; one value: all ties at 0
    assert list(h.otsu()) == [40, -1, 0, 0, 41]
    rng = np.random.default_rng(5)
    rows = rng.integers(1, 1000, size=(50, 256)).astype(np.uint32)
    rows[::2] = (rows[::2] * np.exp(-0.5 * ((np.arange(256) - 60) / 25.0) ** 2) + rows[::2] * 0.3 * np.exp(-0.5 * ((np.arange(256) - 190) / 12.0) ** 2)).astype(np.uint32) + 1
    assert rows.min() > 0                                    # an empty bin is an exact tie of t - 1 and t, which float64 may break either way
    got = FrameHistograms(rows, rows.sum(axis=0).astype(np.uint64)).otsu()
    assert list(got) == [otsu_float(r) for r in rows]
    assert 60 < got[0] < 190
    huge = of({0: 2 ** 28 - 9, 255: 9})                      # (s0 N - S n0)^2 is about 2^128 here: no fixed-width integer holds it
    assert list(huge.otsu()) == [0]


def test_threshold_table_and_suggestion_on_a_table_built_by_hand():
    # count_above of frame 0: 12 for t < 5, 5 for 5 <= t < 15, 0 from 15; frame 1: 30 for t < 3, 5 for 3 <= t < 25, 1 for 25 <= t < 35;
    # frame 2: an empty region
    h = of({5: 7, 15: 5}, {3: 25, 25: 4, 35: 1}, {})
    above = h.count_above()
    assert list(above[0, [0, 4, 5, 14, 15, 255]]) == [12, 12, 5, 5, 0, 0] and list(above[1, [2, 3, 24, 25, 34, 35]]) == [30, 5, 5, 1, 1, 0]
    table = h.threshold_table(4, 6)
    want = np.zeros(256, np.int64)
    want[5:15] += 1                                          # frame 0 holds 5 pixels above t = 5..14
    want[3:25] += 1                                          # frame 1 holds 5 above t = 3..24
    assert np.array_equal(table, want) and table.dtype == np.int64 and table.max() == 2
    assert h.suggest_threshold(4, 6) == (5 + 14) // 2        # the one run of the maximum: 5..14
    # two runs of equal length: the lowest wins.  1 pixel above: frame 0 never, frame 1 for t = 25..34; 12 above: frame 0 for t = 0..4
    assert np.array_equal(np.flatnonzero(h.threshold_table(1, 1)), np.arange(25, 35))
    two = of({9: 3, 19: 2}, {29: 2, 39: 3})                  # 2 above: t = 9..18 in frame 0, never in frame 1 (5, then 3, then 0) ...
    assert np.array_equal(np.flatnonzero(two.threshold_table(2, 2)), np.arange(9, 19))
    two = of({9: 3, 19: 2}, {49: 1, 59: 2})                  # ... and t = 49..58 in this frame 1: runs 9..18 and 49..58, ten each
    assert np.array_equal(np.flatnonzero(two.threshold_table(2, 2)), np.concatenate([np.arange(9, 19), np.arange(49, 59)]))
    assert two.suggest_threshold(2, 2) == (9 + 18) // 2
    longer = of({9: 3, 19: 2}, {49: 1, 60: 2})               # the second run is one longer: it wins
    assert longer.suggest_threshold(2, 2) == (49 + 59) // 2
    assert h.suggest_threshold(1000, 2000) is None           # the maximum is 0
    assert of({}).suggest_threshold(0, 5) == 127             # an empty region holds 0 pixels above every t: one run 0..255
    assert of({}).suggest_threshold(1, 5) is None and list(of({}).threshold_table(1, 5)) == [0] * 256
