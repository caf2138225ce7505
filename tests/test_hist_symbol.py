"""CPU: libsba_hip.so exports sba_frame_histograms as include/sba_hip.h declares it, an argument error is returned without a GPU
and leaves both outputs untouched, and without a GPU the call fails loudly (no CPU fallback)."""
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
    assert re.search(r"\bint sba_frame_histograms\s*\(", text) and re.search(r"\}\s*sba_hist_opts\s*;", text)
    assert "sba_frame_histograms" in _native.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "sba_frame_histograms")
    assert len(lib.sba_frame_histograms.argtypes) == 11
    assert ctypes.sizeof(_native.HistOpts) == 4 * (1 + 1 + 4 + 3 + 1 + 4)
    assert lib.sba_abi_version() == 2


def test_argument_errors_need_no_gpu_and_no_gpu_means_loud_failure(lib):
    frames = np.zeros((2, 4, 6, 3), np.uint8)
    hist, total = np.full((2, 256), 0xA5A5A5A5, np.uint32), np.full(256, 0xA5A5A5A5A5A5A5A5, np.uint64)

    def call(row_pitch=18, frame_pitch=72, **o):
        opts = _native.HistOpts(channel=1)
        for k, v in o.items():
            setattr(opts, k, v)
        rc = lib.sba_frame_histograms(0, frames.ctypes.data, 2, 4, 6, 3, row_pitch, frame_pitch, ctypes.byref(opts), hist.ctypes.data,
                                      total.ctypes.data)
        return rc, (lib.sba_last_error(None) or b"").decode()

    rc, msg = call(channel=3)
    assert rc == -1 and msg.startswith("sba_frame_histograms: channel out of range"), (rc, msg)
    rc, msg = call(row_pitch=17)
    assert rc == -1 and msg.startswith("sba_frame_histograms: row_pitch is smaller"), (rc, msg)
    assert np.all(hist.view(np.uint8) == 0xA5) and np.all(total.view(np.uint8) == 0xA5)
    with pytest.raises(_native.SbaError, match="sba_frame_histograms: channel out of range"):
        imaging.frame_histograms(frames, channel=3)
    with pytest.raises(ValueError, match="256 counts"):
        _native.frame_histograms(frames, total=np.zeros(255, np.uint64))
    if lib.sba_device_count() == 0:                                        # with a GPU tests/test_gpu_hist.py takes over
        with pytest.raises(_native.SbaError, match="no HIP device"):
            _native.frame_histograms(frames)
        with pytest.raises(_native.SbaError, match="no HIP device"):
            imaging.frame_histograms(frames, per_frame=False)
