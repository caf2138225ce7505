"""GPU: the one clause of the chroma-mode rule (chroma_mode, sba_frames.hpp) that the tests of the three YUV calls leave open.
Two chroma planes one byte apart are the halves of ONE interleaved plane only when its rows hold all their 2 cw bytes; with a
row pitch of 2 cw - 1 they are planes of their own with a step of two, read sample by sample.  Bit equality with the oracles of
tests/test_convert_host.py and tests/test_undistort_yuv_host.py, from host and from device memory."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lasercalib_amd import _native, imaging  # noqa: E402
from lasercalib_amd.imaging import Lens  # noqa: E402
from test_convert_host import convert_oracle  # noqa: E402
from test_undistort_yuv_host import undistort_yuv_oracle  # noqa: E402

B, H, W = 2, 5, 7
CH, CW = (H + 1) // 2, (W + 1) // 2                                        # 3 x 4
PITCH = 2 * CW - 1                                                         # a row of pairs would need 2 cw = 8 bytes
LENS9, NEW_K = (6.0, 6.0, 3.0, 2.0, -0.1, 0.01, 0, 0, 0), (6.0, 6.0, 3.0, 2.0)     # a mild barrel
BORDER = (7, 99, 201)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert _native.device_count() > 0, "no HIP device visible: GPU tests must run on the MI355X box"


@pytest.mark.parametrize("device", [False, True], ids=["from host", "from device"])
def test_planes_one_byte_apart_whose_rows_are_too_short_for_pairs(device):
    import torch
    rng = np.random.default_rng(11)
    y = rng.integers(0, 256, size=(B, H, W), dtype=np.uint8)
    buf = rng.integers(0, 256, size=B * CH * PITCH + 1, dtype=np.uint8)
    before, strides = buf.copy(), (CH * PITCH, PITCH, 2)
    if device:
        y_in, dbuf = torch.from_numpy(y).cuda(), torch.from_numpy(buf).cuda()
        u, v = (torch.as_strided(dbuf, (B, CH, CW), strides, off) for off in (0, 1))
    else:
        y_in = y
        u, v = (np.lib.stride_tricks.as_strided(buf[off:], (B, CH, CW), strides) for off in (0, 1))
    L = _native._yuv_layout((y_in, u, v), "i420")
    assert (L.v - L.u, L.c_step, L.c_row_pitch, L.c_frame_pitch) == (1, 2, PITCH, CH * PITCH)
    # the same samples as contiguous planes (the last sample of a row of v is the first of the next row of u)
    uc, vc = (np.ascontiguousarray(np.lib.stride_tricks.as_strided(buf[off:], (B, CH, CW), strides)) for off in (0, 1))

    def host(a):
        return a.cpu().numpy() if device else a

    bgr = imaging.convert_frames((y_in, u, v), "i420", out_format="bgr")
    assert np.array_equal(host(bgr), convert_oracle(y, uc, vc))

    empty = (lambda s: torch.empty(s, dtype=torch.uint8, device="cuda")) if device else (lambda s: np.empty(s, np.uint8))
    out = (empty((B, H, W)), empty((B, CH, CW)), empty((B, CH, CW)))
    ret = imaging.undistort_yuv((y_in, u, v), "i420", Lens(*LENS9), NEW_K, (W, H), border=BORDER, out=out)
    assert ret is out
    want = undistort_yuv_oracle(y, uc, vc, LENS9, NEW_K, (H, W), border=BORDER)
    for k, (g, w) in enumerate(zip(out, want)):
        assert np.array_equal(host(g), w), f"plane {k}"
    assert np.array_equal(host(dbuf) if device else buf, before), "the source was written"
