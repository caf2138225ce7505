"""CPU: libsba_hip.so exports sba_refine_corners as include/sba_hip.h declares it, an argument error is returned without a GPU
and leaves the outputs untouched, and without a GPU the call fails loudly (no CPU fallback)."""
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
    assert re.search(r"\bint sba_refine_corners\s*\(", text) and re.search(r"\}\s*sba_corner_opts\s*;", text)
    assert "sba_refine_corners" in _native.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "sba_refine_corners")
    assert len(lib.sba_refine_corners.argtypes) == 16
    assert lib.sba_abi_version() == 2


def test_argument_errors_need_no_gpu_and_no_gpu_means_loud_failure(lib):
    frames = np.zeros((2, 8, 9, 3), np.uint8)
    start = np.array([0, 1, 3], np.int64)
    xy = np.array([[4.0, 4.0], [3.0, 3.0], [5.0, 4.0]])
    refined, status = np.full((3, 2), -7.0), np.full(3, -7, np.int32)
    ok = np.ones((7, 7))

    def call(opts=None, row_pitch=27, channels=3, start=start, xy=xy, weights=None, refined=refined, status=status, n_frames=2):
        o = None
        if opts is not None:
            o = _native.CornerOpts()
            o.eps, o.channel, o.win_x, o.win_y, o.zero_x, o.zero_y, o.max_iter = 1e-5, -1, 3, 3, -1, -1, 200
            for k, v in opts.items():
                setattr(o, k, (ctypes.c_int32 * 3)(*v) if k == "gray_w" else v)
        rc = lib.sba_refine_corners(0, frames.ctypes.data, n_frames, 8, 9, channels, row_pitch, 216, None if start is None else _native._iptr(start),
                                    _native._dptr(xy), None if o is None else ctypes.byref(o), _native._dptr(weights),
                                    _native._dptr(refined), None if status is None else status.ctypes.data, None, None)
        return rc, (lib.sba_last_error(None) or b"").decode()

    cases = [
        (dict(row_pitch=26), "row_pitch is smaller"),
        (dict(channels=2), "channels must be 1, 3 or 4"),
        (dict(start=None), "null corner_start"),
        (dict(start=np.array([1, 1, 3], np.int64)), "corner_start[0] must be 0"),
        (dict(start=np.array([0, 2, 1], np.int64)), "corner_start must not decrease"),
        (dict(opts=dict(win_x=0)), "win_x and win_y must be in 1..15"),
        (dict(opts=dict(win_y=16)), "win_x and win_y must be in 1..15"),
        (dict(opts=dict(max_iter=0)), "max_iter must be in 1..10000"),
        (dict(opts=dict(max_iter=10001)), "max_iter must be in 1..10000"),
        (dict(opts=dict(eps=-1.0)), "eps must be >= 0"),
        (dict(opts=dict(eps=float("nan"))), "eps must be >= 0"),
        (dict(opts=dict(channel=3)), "channel out of range"),
        (dict(opts=dict(channel=-2)), "channel out of range"),
        (dict(opts=dict(channel=-1), channels=1, row_pitch=9), "channel -1 (gray) needs 3 or 4 channels"),
        (dict(opts=dict(gray_w=(1, 2, 3))), "the gray weights must sum to 2^15"),
        (dict(opts=dict(gray_w=(-1, 32768, 1))), "a gray weight is negative"),
        (dict(weights=-ok), "a weight is negative or not finite"),
        (dict(weights=np.where(np.eye(7) > 0, np.nan, 1.0)), "a weight is negative or not finite"),
        (dict(xy=None), "null corners, refined or status"),
        (dict(refined=None), "null corners, refined or status"),
        (dict(status=None), "null corners, refined or status"),
    ]
    for kw, text in cases:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("sba_refine_corners: " + text), (kw, rc, msg)
    assert np.all(refined == -7.0) and np.all(status == -7)
    if lib.sba_device_count() == 0:                                        # with a GPU tests/test_gpu_corners.py takes over
        rc, msg = call()
        assert rc != 0 and "no HIP device" in msg
        with pytest.raises(_native.SbaError, match="no HIP device"):
            _native.refine_corners(frames, start, xy, channel=-1)
        with pytest.raises(_native.SbaError, match="no HIP device"):
            imaging.refine_corners(frames, [xy[:1], xy[1:]])
        with pytest.raises(_native.SbaError, match="no HIP device"):
            imaging.corner_sub_pix(frames[0, :, :, 0], xy.astype(np.float32).reshape(-1, 1, 2), (3, 3), (-1, -1), (3, 200, 1e-5))
