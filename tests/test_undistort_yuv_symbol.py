"""CPU: libsba_hip.so exports sba_undistort_yuv as include/sba_hip.h declares it, an argument error is returned without a GPU and
leaves every output untouched, and without a GPU the call fails loudly (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

from lasercalib_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _native.load()


def test_symbol_is_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sba_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint sba_undistort_yuv\s*\(", text)
    assert "sba_undistort_yuv" in _native.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "sba_undistort_yuv")
    assert len(lib.sba_undistort_yuv.argtypes) == 13
    assert lib.sba_abi_version() == 2


def test_argument_errors_need_no_gpu_and_no_gpu_means_loud_failure(lib):
    y, uv = np.zeros((1, 4, 6), np.uint8), np.zeros((1, 2, 3, 2), np.uint8)
    oy, ouv = np.full((1, 4, 6), 0xA5, np.uint8), np.full((1, 2, 3, 2), 0xA5, np.uint8)
    flags, qmap = np.full((4, 6), 0xA5, np.uint8), np.full((4, 6, 2), -1, np.int32)
    src = _native.YuvPlanes(y.ctypes.data, uv.ctypes.data, uv.ctypes.data + 1, 6, 24, 6, 12, 2, 0)
    out = _native.YuvPlanes(oy.ctypes.data, ouv.ctypes.data, ouv.ctypes.data + 1, 6, 24, 6, 12, 2, 0)
    lens = _native.LensStruct(5.0, 5.0, 2.5, 1.5, 0, 0, 0, 0, 0)
    nk = np.array([5.0, 5.0, 2.5, 1.5])
    opts = _native.UndistortYuvOpts()
    opts.border_u = 256

    def call(s, o):
        return lib.sba_undistort_yuv(0, ctypes.byref(s), 1, 4, 6, ctypes.byref(lens), _native._dptr(nk), 4, 6, ctypes.byref(out),
                                     ctypes.byref(o), flags.ctypes.data, qmap.ctypes.data)

    assert call(src, opts) == -1
    assert (lib.sba_last_error(None) or b"").decode().startswith("sba_undistort_yuv: border")
    bad = _native.YuvPlanes(y.ctypes.data, uv.ctypes.data, uv.ctypes.data + 1, 6, 24, 6, 12, 3, 0)          # c_step = 3
    assert call(bad, _native.UndistortYuvOpts()) == -1
    assert (lib.sba_last_error(None) or b"").decode().startswith("sba_undistort_yuv: src: c_step")
    assert np.all(oy == 0xA5) and np.all(ouv == 0xA5) and np.all(flags == 0xA5) and np.all(qmap == -1)
    if lib.sba_device_count() == 0:                                        # with a GPU tests/test_gpu_undistort_yuv.py takes over
        with pytest.raises(_native.SbaError, match="no HIP device"):
            _native.undistort_yuv((y, uv), "nv12", (5.0, 5.0, 2.5, 1.5, 0, 0, 0, 0, 0), (5.0, 5.0, 2.5, 1.5), (4, 6))
