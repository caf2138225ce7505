"""CPU: libsba_hip.so exports sba_frames_to_yuv as include/sba_hip.h declares it, the ctypes structs have the header's layout,
and without a GPU the call fails loudly (no CPU fallback)."""
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
    assert re.search(r"\bint sba_frames_to_yuv\s*\(", text)
    assert "sba_frames_to_yuv" in _native.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "sba_frames_to_yuv")
    assert len(lib.sba_frames_to_yuv.argtypes) == 18


def test_struct_layouts_match_header():
    text = open(os.path.join(ROOT, "include", "sba_hip.h")).read()
    assert ctypes.sizeof(_native.RgbMatrix) == 40 and ctypes.sizeof(_native.ToYuvOpts) == 48
    m = re.search(r"typedef struct \{ int32_t ([a-z_, ]+); \} sba_rgb_matrix;", text)
    assert m and [n.strip() for n in m.group(1).split(",")] == [n for n, _t in _native.RgbMatrix._fields_]
    body = text[text.index("typedef enum { SBA_CHROMA_NEAREST"):text.index("} sba_to_yuv_opts;")]
    assert re.findall(r"int32_t (\w+)", body) == [n for n, _t in _native.ToYuvOpts._fields_]
    assert "{16, 269484, 528482, 102760, -155188, -305135, 460324, 460324, -385875, -74448}" in text
    assert _native.CHROMA_MODES == {"nearest": 0, "average": 1}


def test_argument_errors_need_no_gpu_and_no_gpu_means_loud_failure(lib):
    src, out = np.zeros((1, 4, 6, 3), np.uint8), np.full((1, 6, 6), 0xA5, np.uint8)
    p, q = ctypes.c_void_p(src.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    assert lib.sba_frames_to_yuv(0, p, 1, 4, 6, 3, 18, 72, q, q, q, 6, 36, 6, 36, 3, None, None) == -1      # c_step = 3
    assert (lib.sba_last_error(None) or b"").decode().startswith("sba_frames_to_yuv: c_step")
    assert np.all(out == 0xA5)
    if lib.sba_device_count() == 0:                                        # with a GPU tests/test_gpu_yuv.py takes over
        with pytest.raises(_native.SbaError, match="no HIP device"):
            _native.frames_to_yuv(src)
