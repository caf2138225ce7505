"""CPU: libsba_hip.so exports sba_adaptive_threshold as include/sba_hip.h declares it, every argument error is returned without a
GPU and leaves both outputs untouched, and without a GPU the call fails loudly (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

from lasercalib_amd import _native, imaging

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _native.load()


def test_symbol_is_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sba_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint sba_adaptive_threshold\s*\(", text)
    struct = re.search(r"typedef struct \{([^}]*)\}\s*sba_adaptive_opts\s*;", text)
    assert struct
    words = 0                                                             # the header's struct holds int32_t fields only
    for decl in struct.group(1).split(";"):
        decl = decl.strip()
        if decl:
            assert decl.startswith("int32_t "), decl
            words += sum(int(n.group(1)) if (n := re.search(r"\[(\d+)\]", name)) else 1 for name in decl[len("int32_t "):].split(","))
    assert ctypes.sizeof(_native.AdaptiveOpts) == 4 * words == 88
    assert [n for n, _ in _native.AdaptiveOpts._fields_] == ["n_windows", "block", "delta", "invert", "max_value", "channel", "gray_w",
                                                            "frames_on_device", "out_on_device", "chunk_frames", "reserved"]
    assert "sba_adaptive_threshold" in _native.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "sba_adaptive_threshold")
    assert len(lib.sba_adaptive_threshold.argtypes) == 14
    assert lib.sba_abi_version() == 2


def test_argument_errors_need_no_gpu_and_no_gpu_means_loud_failure(lib):
    frames = np.zeros((2, 4, 6, 3), np.uint8)
    out, mean = np.full((2, 2, 4, 6), 0xA5, np.uint8), np.full((2, 2, 4, 6), 0xA5, np.uint8)

    def call(n_frames=2, height=4, width=6, channels=3, row_pitch=18, frame_pitch=72, out_row=6, out_frame=24, out_window=48,
             frames_ptr=frames.ctypes.data, out_ptr=out.ctypes.data, mean_ptr=mean.ctypes.data, block=(3, 5), delta=(7, 7), **o):
        opts = _native.AdaptiveOpts(n_windows=len(block), invert=1, channel=-1)
        opts.block[:len(block)], opts.delta[:len(delta)] = block, delta
        for k, v in o.items():
            setattr(opts, k, (ctypes.c_int32 * 3)(*v) if k == "gray_w" else v)
        rc = lib.sba_adaptive_threshold(0, frames_ptr, n_frames, height, width, channels, row_pitch, frame_pitch, ctypes.byref(opts),
                                        out_row, out_frame, out_window, out_ptr, mean_ptr)
        return rc, (lib.sba_last_error(None) or b"").decode()

    cases = [
        (dict(n_frames=-1), "negative size"),
        (dict(frames_ptr=None), "null frames"),
        (dict(channels=2), "channels must be 1, 3 or 4"),
        (dict(channel=3), "channel out of range"),
        (dict(channel=-2), "channel out of range"),
        (dict(n_windows=0), "n_windows must be in 1..4"),
        (dict(n_windows=5), "n_windows must be in 1..4"),
        (dict(block=(3, 4)), "a block must be odd and in 3..127"),
        (dict(block=(1,)), "a block must be odd and in 3..127"),
        (dict(block=(3, 129)), "a block must be odd and in 3..127"),
        (dict(delta=(7, 257)), "a delta must be in -256..256"),
        (dict(delta=(-257, 0)), "a delta must be in -256..256"),
        (dict(invert=2), "invert must be 0"),
        (dict(max_value=256), "max_value must be in 0..255"),
        (dict(max_value=-1), "max_value must be in 0..255"),
        (dict(channels=1, row_pitch=6, frame_pitch=24), "channel -1 (gray) needs 3 or 4 channels"),
        (dict(gray_w=(-1, 32768, 1)), "a gray weight is negative"),
        (dict(gray_w=(1, 2, 3)), "the gray weights must sum to 2^15"),
        (dict(out_row=5), "out_row_pitch is smaller than width"),
        (dict(out_frame=23), "out_frame_pitch is smaller than height * out_row_pitch"),
        (dict(out_window=47), "out_window_pitch is smaller than n_frames * out_frame_pitch"),
        (dict(out_ptr=None, mean_ptr=None), "null out and null mean_out"),
        (dict(row_pitch=17), "row_pitch is smaller"),
        (dict(frame_pitch=71), "frame_pitch is smaller"),
    ]
    for kw, text in cases:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("sba_adaptive_threshold: " + text), (kw, rc, msg)
    assert lib.sba_adaptive_threshold(0, frames.ctypes.data, 2, 20000, 6, 3, 18, 360000, None, 6, 120000, 240000, out.ctypes.data, None) == -6
    assert np.all(out == 0xA5) and np.all(mean == 0xA5)
    rc, msg = call(block=(3,), delta=(7,), out_window=0, out_ptr=None, mean_ptr=None)     # one window needs no window pitch: the next check answers
    assert rc == -1 and msg.startswith("sba_adaptive_threshold: null out and null mean_out"), (rc, msg)

    with pytest.raises(_native.SbaError, match="sba_adaptive_threshold: channel out of range"):
        _native.adaptive_threshold(frames, (3,), (7,), channel=3)
    with pytest.raises(ValueError, match="same strides"):
        _native.adaptive_threshold(frames, (3, 5), (7, 7), out=out, mean_out=np.zeros((2, 2, 4, 8), np.uint8)[..., :6])
    with pytest.raises(ValueError, match="expected"):
        _native.adaptive_threshold(frames, (3, 5), (7, 7), out=out[:1])
    with pytest.raises(ValueError, match="neither"):
        _native.adaptive_threshold(frames, (3,), (7,), out=False)
    if lib.sba_device_count() == 0:                                        # with a GPU tests/test_gpu_adaptive.py takes over
        with pytest.raises(_native.SbaError, match="no HIP device"):
            _native.adaptive_threshold(frames, (3, 13, 23), (7, 7, 7))
        with pytest.raises(_native.SbaError, match="no HIP device"):
            imaging.adaptive_threshold(frames, 23)
        with pytest.raises(_native.SbaError, match="no HIP device"):
            imaging.adaptive_threshold_cv(frames[0, :, :, 0], 255, 0, 1, 13, 7)
        assert np.all(out == 0xA5)
