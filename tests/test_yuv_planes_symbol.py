"""CPU: the three entry points that take a set of YUV 4:2:0 planes -- sba_convert_frames reads one, sba_frames_to_yuv writes one,
sba_undistort_yuv does both -- report a defect of the planes in the same words, with status -1, before the device is touched and
with every output left as it was.  The sentences are literals: what sba_convert_frames said before the three shared one check."""
import ctypes
import os

import numpy as np
import pytest

from lasercalib_amd import _native

H, W, CH, CW = 3, 5, 2, 3                                                   # one frame of 5 x 3, chroma 3 x 2
PLANAR = dict(y_row_pitch=W, y_frame_pitch=H * W, c_row_pitch=CW, c_frame_pitch=CH * CW, c_step=1)

NULL_PLANE = "null plane"
C_STEP = "c_step must be 1 (planar) or 2 (interleaved)"
Y_ROW = "y_row_pitch is smaller than width"
Y_FRAME = "y_frame_pitch is smaller than height * y_row_pitch"
C_ROW = "c_row_pitch is smaller than c_step * ((width + 1) / 2 - 1) + 1"
C_FRAME = "c_frame_pitch is smaller than ((height + 1) / 2) * c_row_pitch"
OVERFLOW = "n_frames * a frame pitch overflows"

# (name, what is changed of the planar defaults, n_frames, the sentence)
DEFECTS = [
    ("null y", dict(y=None), 1, NULL_PLANE),
    ("null u", dict(u=None), 1, NULL_PLANE),
    ("null v", dict(v=None), 1, NULL_PLANE),
    ("c_step 0", dict(c_step=0), 1, C_STEP),
    ("c_step 3", dict(c_step=3), 1, C_STEP),
    ("y_row_pitch = width - 1", dict(y_row_pitch=W - 1), 1, Y_ROW),
    ("y_frame_pitch = height * y_row_pitch - 1", dict(y_frame_pitch=H * W - 1), 1, Y_FRAME),
    ("c_row_pitch = cw - 1", dict(c_row_pitch=CW - 1), 1, C_ROW),
    # the frame pitch follows the row pitch, so that the row pitch is the only defect
    ("c_step 2, c_row_pitch = 2 (cw - 1)", dict(c_step=2, c_row_pitch=2 * (CW - 1), c_frame_pitch=CH * 2 * (CW - 1)), 1, C_ROW),
    ("c_frame_pitch = ch * c_row_pitch - 1", dict(c_frame_pitch=CH * CW - 1), 1, C_FRAME),
    ("c_row_pitch = -1", dict(c_row_pitch=-1), 1, C_ROW),
    ("y_frame_pitch = 2^62, three frames", dict(y_frame_pitch=1 << 62), 3, OVERFLOW),
]
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _native.load()


class Planes:
    """Three host planes filled with the sentinel, and their description with ``changes`` applied."""

    def __init__(self, changes=None):
        self.mem = [np.full((1, H, W), SENTINEL, np.uint8), np.full((1, CH, CW), SENTINEL, np.uint8), np.full((1, CH, CW), SENTINEL, np.uint8)]
        d = dict(PLANAR, y=self.mem[0].ctypes.data, u=self.mem[1].ctypes.data, v=self.mem[2].ctypes.data)
        d.update(changes or {})
        self.d = d

    def struct(self):
        d = self.d
        return _native.YuvPlanes(d["y"], d["u"], d["v"], d["y_row_pitch"], d["y_frame_pitch"], d["c_row_pitch"], d["c_frame_pitch"], d["c_step"], 0)

    def loose(self):
        d = self.d
        return (ctypes.c_void_p(d["y"]), ctypes.c_void_p(d["u"]), ctypes.c_void_p(d["v"]), d["y_row_pitch"], d["y_frame_pitch"],
                d["c_row_pitch"], d["c_frame_pitch"], d["c_step"])

    def untouched(self):
        return all(np.all(m == SENTINEL) for m in self.mem)


def last_error(lib):
    return (lib.sba_last_error(None) or b"").decode()


def convert(lib, changes, n):
    src, out = Planes(changes), np.full((1, H, W, 3), SENTINEL, np.uint8)
    y, u, v, *pitches = src.loose()
    rc = lib.sba_convert_frames(0, y, u, v, n, H, W, *pitches, None, 3 * W, 3 * W * H, None, ctypes.c_void_p(out.ctypes.data))
    return rc, last_error(lib), bool(np.all(out == SENTINEL))


def to_yuv(lib, changes, n):
    frames, out = np.zeros((1, H, W, 3), np.uint8), Planes(changes)
    rc = lib.sba_frames_to_yuv(0, ctypes.c_void_p(frames.ctypes.data), n, H, W, 3, 3 * W, 3 * W * H, *out.loose(), None, None)
    return rc, last_error(lib), out.untouched()


def undistort(lib, side, changes, n):
    src, out = Planes(changes if side == "src" else None), Planes(changes if side == "out" else None)
    flags, qmap = np.full((H, W), SENTINEL, np.uint8), np.full((H, W, 2), -1, np.int32)
    lens, nk = _native.LensStruct(5.0, 5.0, 2.0, 1.0, 0, 0, 0, 0, 0), np.array([5.0, 5.0, 2.0, 1.0])
    s, o = src.struct(), out.struct()
    rc = lib.sba_undistort_yuv(0, ctypes.byref(s), n, H, W, ctypes.byref(lens), _native._dptr(nk), H, W, ctypes.byref(o), None,
                               flags.ctypes.data, qmap.ctypes.data)
    return rc, last_error(lib), out.untouched() and bool(np.all(flags == SENTINEL)) and bool(np.all(qmap == -1))


@pytest.mark.parametrize("name,changes,n,sentence", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_a_defect_of_the_planes_reads_the_same_from_all_three_entry_points(lib, name, changes, n, sentence):
    got = {"sba_convert_frames: ": convert(lib, changes, n),
           "sba_frames_to_yuv: ": to_yuv(lib, changes, n),
           "sba_undistort_yuv: src: ": undistort(lib, "src", changes, n),
           "sba_undistort_yuv: out: ": undistort(lib, "out", changes, n)}
    for prefix, (rc, text, untouched) in got.items():
        assert rc == -1, (prefix, rc, text)
        assert text == prefix + sentence, (prefix, text)
        assert untouched, prefix
    assert len({text[len(prefix):] for prefix, (_rc, text, _u) in got.items()}) == 1
