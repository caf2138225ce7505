"""CPU: the numpy oracle of sba_background_accumulate / sba_background_suppress (include/sba_hip.h) on hand-computed cases,
the host arithmetic of imaging.BackgroundModel on injected accumulators, and the binding.  The oracle is integer arithmetic;
tests/test_gpu_background.py holds the library to it bit for bit."""
import os
import pickle
import re

import numpy as np
import pytest

from lasercalib_amd import _native, imaging

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the oracle
def accumulate_oracle(frames, channel=1, threshold=50, use=None, into=None):
    """The rule of include/sba_hip.h: a dict sum (uint32), sumsq (uint64), hot (uint32), vmax (uint8), all (H, W), and n, of the
    frames (B, H, W, C) whose ``use`` flag is set, added to the dict ``into`` when given (which is left unchanged)."""
    frames = np.asarray(frames)
    v = frames[..., channel].astype(np.uint64)
    if use is not None:
        v = v[np.asarray(use) != 0]
    H, W = frames.shape[1:3]
    acc = {"sum": v.sum(0, dtype=np.uint64).astype(np.uint32), "sumsq": (v * v).sum(0, dtype=np.uint64),
           "hot": (v > threshold).sum(0, dtype=np.uint64).astype(np.uint32),
           "vmax": v.max(0).astype(np.uint8) if v.shape[0] else np.zeros((H, W), np.uint8), "n": int(v.shape[0])}
    if into is not None:
        with np.errstate(over="ignore"):
            acc = {"sum": into["sum"] + acc["sum"], "sumsq": into["sumsq"] + acc["sumsq"], "hot": into["hot"] + acc["hot"],
                   "vmax": np.maximum(into["vmax"], acc["vmax"]), "n": into["n"] + acc["n"]}
    return acc


def suppress_oracle(frames, channel=1, level=None, mask=None, mode="gate"):
    """(B, H, W) uint8: gate = 0 where the mask is set or v <= level, else v; subtract = 0 where the mask is set, else max(v - level, 0)."""
    v = np.asarray(frames)[..., channel].astype(np.int64)
    level = np.zeros(v.shape[1:], np.int64) if level is None else np.asarray(level).astype(np.int64)
    out = np.where(v > level[None], v, 0) if mode == "gate" else np.maximum(v - level[None], 0)
    if mask is not None:
        out = np.where(np.asarray(mask)[None] != 0, 0, out)
    return out.astype(np.uint8)


def level_oracle(acc, k_sigma=4.0, margin=4):
    n = acc["n"]
    mean = acc["sum"].astype(np.float64) / n
    std = np.sqrt(np.maximum(acc["sumsq"].astype(np.float64) / n - mean * mean, 0.0))
    return np.clip(np.ceil(mean + k_sigma * std) + margin, 0, 255).astype(np.uint8)


def model_from(acc, H, W, channel=1, threshold=50):
    return imaging.BackgroundModel.from_state(dict(acc, height=H, width=W, channel=channel, threshold=threshold), on_device=False)


# two 2 x 3 frames of 3 channels; the green values are the ones that count
G0 = np.array([[0, 10, 200], [51, 50, 255]], np.uint8)
G1 = np.array([[3, 10, 100], [49, 52, 255]], np.uint8)


def two_frames():
    f = np.zeros((2, 2, 3, 3), np.uint8)
    f[..., 0], f[..., 2] = 7, 250                   # blue and red must not leak in
    f[0, ..., 1], f[1, ..., 1] = G0, G1
    return f


# ----------------------------------------------------------------------------- 1. the oracle on hand-computed cases
def test_accumulate_oracle_by_hand():
    acc = accumulate_oracle(two_frames(), channel=1, threshold=50)
    assert acc["n"] == 2
    assert acc["sum"].tolist() == [[3, 20, 300], [100, 102, 510]] and acc["sum"].dtype == np.uint32
    assert acc["sumsq"].tolist() == [[9, 200, 50000], [51 * 51 + 49 * 49, 50 * 50 + 52 * 52, 2 * 255 * 255]] and acc["sumsq"].dtype == np.uint64
    assert acc["hot"].tolist() == [[0, 0, 2], [1, 1, 2]]              # 50 is not above the threshold 50, 51 and 52 are
    assert acc["vmax"].tolist() == [[3, 10, 200], [51, 52, 255]] and acc["vmax"].dtype == np.uint8
    assert accumulate_oracle(two_frames(), channel=0)["sum"].tolist() == [[14] * 3] * 2


def test_accumulate_oracle_use_mask_and_adding():
    f = two_frames()
    only1 = accumulate_oracle(f, use=[0, 1])
    assert only1["n"] == 1 and only1["sum"].tolist() == G1.astype(int).tolist() and only1["vmax"].tolist() == G1.tolist()
    none = accumulate_oracle(f, use=[0, 0])
    assert none["n"] == 0 and not none["sum"].any() and not none["vmax"].any()
    both = accumulate_oracle(f[1:], into=accumulate_oracle(f[:1]))
    whole = accumulate_oracle(f)
    assert all(np.array_equal(both[k], whole[k]) for k in whole)
    # the sum wraps at 2^32 like the library's uint32 would, the square sum carries into its high word
    big = {"sum": np.full((2, 3), 2 ** 32 - 1 - 255, np.uint32), "sumsq": np.full((2, 3), 2 ** 32 - 1, np.uint64),
           "hot": np.zeros((2, 3), np.uint32), "vmax": np.zeros((2, 3), np.uint8), "n": 5}
    got = accumulate_oracle(f[:1], into=big)
    assert got["sum"][1, 2] == 2 ** 32 - 1 and got["sumsq"][1, 2] == 2 ** 32 - 1 + 255 * 255 and got["n"] == 6


def test_suppress_oracle_both_modes_and_mask_precedence():
    f = two_frames()
    level = np.array([[0, 10, 150], [60, 40, 254]], np.uint8)
    mask = np.array([[0, 0, 0], [0, 1, 1]], np.uint8)
    gate = suppress_oracle(f, level=level, mode="gate")
    assert gate[0].tolist() == [[0, 0, 200], [0, 50, 255]]            # 0 <= 0 and 10 <= 10 go, values above their level stay as they are
    assert gate[1].tolist() == [[3, 0, 0], [0, 52, 255]]
    sub = suppress_oracle(f, level=level, mode="subtract")
    assert sub[0].tolist() == [[0, 0, 50], [0, 10, 1]] and sub[1].tolist() == [[3, 0, 0], [0, 12, 1]]
    for mode, plain in (("gate", gate), ("subtract", sub)):           # the mask wins over the level, in both modes
        got = suppress_oracle(f, level=level, mask=mask, mode=mode)
        assert got[:, 1, 1:].tolist() == [[0, 0], [0, 0]] and np.array_equal(got[:, 0], plain[:, 0]) and np.array_equal(got[:, 1, 0], plain[:, 1, 0])
    assert np.array_equal(suppress_oracle(f), f[..., 1])               # no level, no mask: the channel itself
    assert np.array_equal(suppress_oracle(f, mask=255 * mask)[:, 0], f[:, 0, :, 1])      # any non-zero mask value removes


# ----------------------------------------------------------------------------- 2. BackgroundModel on injected accumulators
def injected():
    """Four frames seen by three pixels: constant 10; 0, 0, 0, 200 (the dot passed once); 180, 200, 220, 200 (a lamp)."""
    vals = np.array([[10, 10, 10, 10], [0, 0, 0, 200], [180, 200, 220, 200]], np.uint64).T.reshape(4, 1, 3)
    return {"sum": vals.sum(0).astype(np.uint32), "sumsq": (vals * vals).sum(0), "hot": (vals > 50).sum(0).astype(np.uint32),
            "vmax": vals.max(0).astype(np.uint8), "n": 4}


def test_model_statistics_and_level_known_answers():
    m = model_from(injected(), 1, 3)
    assert m.n == 4 and m.mean().tolist() == [[10.0, 50.0, 200.0]] and m.max().tolist() == [[10, 200, 220]]
    assert m.hot_fraction().tolist() == [[0.0, 0.25, 1.0]]
    # variances: 0; (200^2 / 4) - 50^2 = 7500; (180^2 + 2 * 200^2 + 220^2) / 4 - 200^2 = 200
    assert np.allclose(m.std(), np.sqrt([[0.0, 7500.0, 200.0]]), rtol=0, atol=1e-12)
    # ceil(10 + 0) + 4 = 14; ceil(50 + 4 * 86.60) + 4 = 401 -> 255; ceil(200 + 2 * 14.14) + 1 = 230
    assert m.level().tolist() == [[14, 255, 255]]
    assert m.level(k_sigma=2.0, margin=1).tolist() == [[11, ceil_int(50 + 2 * 7500 ** 0.5) + 1, 230]]
    assert m.level(k_sigma=0.0, margin=0).tolist() == [[10, 50, 200]] and m.level(0.0, -20).tolist() == [[0, 30, 180]]
    assert m.level().dtype == np.uint8 and np.array_equal(m.level(), level_oracle(injected()))


def ceil_int(x):
    return int(np.ceil(x))


def test_model_variance_is_clamped_at_zero():
    # a constant 255 over 3 frames: sumsq / n - mean^2 must not go below zero through rounding
    acc = {"sum": np.full((1, 1), 765, np.uint32), "sumsq": np.full((1, 1), 3 * 65025, np.uint64), "hot": np.full((1, 1), 3, np.uint32),
           "vmax": np.full((1, 1), 255, np.uint8), "n": 3}
    m = model_from(acc, 1, 1)
    assert m.std()[0, 0] == 0.0 and m.level(4.0, 0)[0, 0] == 255


def test_hot_mask_fraction_and_grow():
    hot = np.zeros((7, 9), np.uint32)
    hot[3, 4], hot[0, 0], hot[6, 8] = 10, 2, 3
    acc = {"sum": np.zeros((7, 9), np.uint32), "sumsq": np.zeros((7, 9), np.uint64), "hot": hot, "vmax": np.zeros((7, 9), np.uint8), "n": 10}
    m = model_from(acc, 7, 9)
    assert m.hot_mask(0.25).sum() == 2 and m.hot_mask(0.25)[3, 4] == 1 and m.hot_mask(0.25)[6, 8] == 1 and m.hot_mask(0.25).dtype == np.uint8
    assert m.hot_mask(0.2)[0, 0] == 0 and m.hot_mask(0.19)[0, 0] == 1          # strictly more than fraction * n
    grown = m.hot_mask(0.5, grow=2)                                            # disk(2) around (3, 4): 13 pixels
    yy, xx = np.mgrid[0:7, 0:9]
    assert np.array_equal(grown, ((yy - 3) ** 2 + (xx - 4) ** 2 <= 4).astype(np.uint8)) and grown.sum() == 13
    corner = m.hot_mask(0.25, grow=1)                                          # at the border the disk is cut, not wrapped
    assert corner[6, 8] == 1 and corner[5, 8] == 1 and corner[6, 7] == 1 and corner[0, 0] == 0 and corner.sum() == 5 + 3


def test_state_round_trip_and_pickle():
    m = model_from(injected(), 1, 3, channel=2, threshold=77)
    st = pickle.loads(pickle.dumps(m.state()))
    m2 = imaging.BackgroundModel.from_state(st, on_device=False)
    assert (m2.height, m2.width, m2.channel, m2.threshold, m2.n) == (1, 3, 2, 77, 4)
    for k in ("sum", "sumsq", "hot", "vmax"):
        assert np.array_equal(st[k], injected()[k]) and st[k].dtype == injected()[k].dtype and np.array_equal(m2.state()[k], st[k])
    assert np.array_equal(m2.level(), m.level())
    with pytest.raises(ValueError):
        imaging.BackgroundModel.from_state(dict(st, sum=np.zeros((2, 3), np.uint32)))
    with pytest.raises(ValueError, match="no frame"):
        imaging.BackgroundModel(4, 5, on_device=False).level()


# ----------------------------------------------------------------------------- 3. the binding
def test_new_symbols_are_listed_and_declared():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sba_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sba_[a-z_0-9]+)\s*\(", text))
    for name in ("sba_background_accumulate", "sba_background_suppress"):
        assert name in _native.EXPORTED_SYMBOLS and name in declared
    import ctypes
    assert ctypes.sizeof(_native.BgAccumulateOpts) == 48 and ctypes.sizeof(_native.BgSuppressOpts) == 48
    assert _native.BG_MODES == {"gate": 0, "subtract": 1} and _native.BG_MAX_FRAMES == 2 ** 24
