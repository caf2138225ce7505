"""CPU: libsba_hip.so exports sba_warp_frames as include/sba_hip.h declares it, an argument error is returned without a GPU and
leaves the output untouched, and without a GPU the call fails loudly (no CPU fallback)."""
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
    assert re.search(r"\bint sba_warp_frames\s*\(", text) and re.search(r"\bSBA_WARP_BEHIND\s*=\s*8\b", text)
    assert "sba_warp_frames" in _native.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "sba_warp_frames")
    assert len(lib.sba_warp_frames.argtypes) == 18
    assert lib.sba_warp_frames.argtypes == lib.sba_undistort_frames.argtypes      # the same call but for what the doubles mean
    assert lib.sba_abi_version() == 2


def test_argument_errors_need_no_gpu_and_no_gpu_means_loud_failure(lib):
    frames = np.zeros((2, 4, 6, 3), np.uint8)
    out = np.full((2, 4, 6, 3), 0xA5, np.uint8)
    lens = _native.LensStruct(50.0, 50.0, 2.5, 1.5, 0, 0, 0, 0, 0)
    eye = np.eye(3)

    def call(m=eye, row_pitch=18, out_row_pitch=18):
        m = None if m is None else np.ascontiguousarray(m, dtype=np.float64)
        rc = lib.sba_warp_frames(0, frames.ctypes.data, 2, 4, 6, 3, row_pitch, 72, ctypes.byref(lens), _native._dptr(m), 4, 6,
                                 out_row_pitch, 72, None, out.ctypes.data, None, None)
        return rc, (lib.sba_last_error(None) or b"").decode()

    rc, msg = call(m=None)
    assert rc == -1 and msg.startswith("sba_warp_frames: null m"), (rc, msg)
    nan = eye.copy()
    nan[2, 1] = np.nan
    rc, msg = call(m=nan)
    assert rc == -1 and msg.startswith("sba_warp_frames: a value of m is not finite"), (rc, msg)
    rc, msg = call(m=np.full((3, 3), -np.inf))
    assert rc == -1 and msg.startswith("sba_warp_frames: a value of m is not finite"), (rc, msg)
    rc, msg = call(row_pitch=17)
    assert rc == -1 and msg.startswith("sba_warp_frames: row_pitch is smaller"), (rc, msg)
    rc, msg = call(out_row_pitch=17)
    assert rc == -1 and msg.startswith("sba_warp_frames: out_row_pitch is smaller"), (rc, msg)
    assert np.all(out == 0xA5)
    if lib.sba_device_count() == 0:                                        # with a GPU tests/test_gpu_warp.py takes over
        with pytest.raises(_native.SbaError, match="no HIP device"):
            _native.warp_frames(frames, (50.0, 50.0, 2.5, 1.5, 0, 0, 0, 0, 0), eye, (4, 6))
        with pytest.raises(_native.SbaError, match="no HIP device"):
            imaging.warp_frames(frames, imaging.Lens(50.0, 50.0, 2.5, 1.5), eye, (6, 4))
        row = np.array([np.pi, 0, 0, 0, 0, 100.0, 50.0, 0, 0, 2.5, 1.5])
        with pytest.raises(_native.SbaError, match="no HIP device"):
            imaging.plane_view(frames, row, imaging.PlaneGrid.z_plane(0.0, (-3, 3), (-2, 2), 1.0))
