"""CPU: the upload-layout entry points (sba_upload_ex, sba_get_upload_report, sba_get_layout) are declared, exported and
listed, their structs have the header's sizes, and the numpy statement of the layout rule that tests/test_gpu_upload_layout.py
holds the device against (expected_layout) is itself checked against a plain-Python transcription of the host loops of
Engine::upload (csrc/sba_engine.hpp: validation, counting sort by point, canonical camera order, camera-major copy)."""
import ctypes
import os
import re

import numpy as np
import pytest

from lasercalib_amd import _native
from lasercalib_amd.synth import make_rig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_CAMS = 16


# ----------------------------------------------------------------------------- the rule (also used by the GPU tests)
def expected_layout(uv, ci, pi, w, C, N, dtype):
    """The layout every upload route must produce, stated with numpy sorts.  dtype: the engine's ("f32" / "f64")."""
    T = np.float32 if dtype == "f32" else np.float64
    M = ci.size
    idx = np.arange(M)
    perm = np.lexsort((idx, ci, pi)) if C <= GROUP_CAMS else np.lexsort((idx, pi))
    pt_start = np.concatenate(([0], np.cumsum(np.bincount(pi, minlength=N)))).astype(np.int32)
    cam_pm, pt_pm = ci[perm].astype(np.int32), pi[perm].astype(np.int32)
    uv_pm = uv[perm].astype(T).astype(np.float64)
    w_pm = np.ones(M) if w is None else w[perm].astype(T).astype(np.float64)
    cm = np.argsort(cam_pm, kind="stable")
    out = dict(perm=perm.astype(np.int64), pt_start=pt_start, cam_pm=cam_pm, pt_pm=pt_pm, uv_pm=uv_pm, w_pm=w_pm,
               pt_cm=pt_pm[cm], uv_cm=uv_pm[cm], w_cm=w_pm[cm],
               cam_start=np.concatenate(([0], np.cumsum(np.bincount(ci, minlength=C)))).astype(np.int32))
    vis = np.zeros(N, np.uint16)
    if C <= GROUP_CAMS:
        np.bitwise_or.at(vis, pi, (1 << ci).astype(np.uint16))
    out["vis_mask"] = vis
    return out


def strip_points(rig, points):
    """The rig's observation list without the observations of the given points (they stay in the problem, unobserved)."""
    keep = ~np.isin(rig["point_ind"], points)
    return rig["points_2d"][keep], rig["camera_ind"][keep], rig["point_ind"][keep]


def reorder(uv, ci, pi, order, seed=0):
    """'emitted' (as it is), 'shuffled', or 'camdesc' (cameras descending inside every point)."""
    if order == "emitted":
        return uv, ci, pi
    o = np.random.default_rng(seed).permutation(ci.size) if order == "shuffled" else np.lexsort((-ci, pi))
    return uv[o], ci[o], pi[o]


# ----------------------------------------------------------------------------- the host loops, line by line
def host_loops(ci, pi, C, N):
    """perm, pt_start, vis_mask (or None), cam_start, camera-major order, identity_perm as Engine::upload's host pass builds them."""
    M = len(ci)
    sorted_, cam_sorted = True, True
    for i in range(1, M):
        if pi[i] < pi[i - 1]:
            sorted_ = False
        elif pi[i] == pi[i - 1] and ci[i] <= ci[i - 1]:
            cam_sorted = False
    ptstart = [0] * (N + 1)
    for i in range(M):
        ptstart[pi[i] + 1] += 1
    for p in range(N):
        ptstart[p + 1] += ptstart[p]
    identity = sorted_
    if sorted_:
        perm = list(range(M))
    else:
        perm = [0] * M
        fill = ptstart[:-1].copy()
        for i in range(M):
            perm[fill[pi[i]]] = i
            fill[pi[i]] += 1
    nodup = C <= GROUP_CAMS
    vmask = None
    if nodup and sorted_ and cam_sorted:
        vmask = [0] * N
        for i in range(M):
            vmask[pi[i]] |= 1 << ci[i]
    elif nodup:
        vmask = [0] * N
        for p in range(N):
            slot = [-1] * C
            a, b = ptstart[p], ptstart[p + 1]
            for k in range(a, b):
                i = perm[k]
                if slot[ci[i]] >= 0:
                    nodup = False
                    break
                slot[ci[i]] = i
                vmask[p] |= 1 << ci[i]
            if not nodup:
                break
            k = a
            for c in range(C):
                if slot[c] >= 0:
                    if perm[k] != slot[c]:
                        perm[k] = slot[c]
                        identity = False
                    k += 1
    cip = [ci[i] for i in perm]
    camcount = [0] * (C + 1)
    for k in range(M):
        camcount[cip[k] + 1] += 1
    for c in range(C):
        camcount[c + 1] += camcount[c]
    fill = camcount[:-1].copy()
    cm = [0] * M
    for k in range(M):
        cm[fill[cip[k]]] = k
        fill[cip[k]] += 1
    return perm, ptstart, (vmask if nodup else None), camcount, cm, identity


@pytest.mark.parametrize("C,N,vis,mincam", [(17, 60, 0.45, 4), (16, 50, 0.5, 2), (8, 70, 0.4, 2), (40, 40, 0.1, 4), (5, 61, 0.6, 2)])
@pytest.mark.parametrize("order", ["emitted", "shuffled", "camdesc"])
def test_numpy_rule_is_the_host_pass(C, N, vis, mincam, order):
    rig = make_rig(C, N, seed=0, visibility=vis, min_cams_per_point=mincam)
    uv, ci, pi = reorder(*strip_points(rig, [3, N - 1]), order)
    exp = expected_layout(uv, ci, pi, None, C, N, "f64")
    perm, ptstart, vmask, camcount, cm, identity = host_loops(ci.tolist(), pi.tolist(), C, N)
    assert np.array_equal(exp["perm"], perm)
    assert np.array_equal(exp["pt_start"], ptstart)
    assert np.array_equal(exp["cam_start"], camcount)
    assert np.array_equal(exp["pt_cm"], exp["pt_pm"][cm])
    if C <= GROUP_CAMS:
        assert vmask is not None and np.array_equal(exp["vis_mask"], vmask)
    assert identity == np.array_equal(exp["perm"], np.arange(ci.size))
    assert exp["pt_start"][4] == exp["pt_start"][3]              # the stripped point is empty


def test_duplicates_above_one_group_keep_the_callers_order():
    ci = np.array([20, 3, 20, 1, 1, 7], dtype=np.int64)
    pi = np.array([1, 0, 1, 1, 0, 0], dtype=np.int64)
    exp = expected_layout(np.zeros((6, 2)), ci, pi, None, 24, 2, "f64")
    perm, ptstart, vmask, *_ = host_loops(ci.tolist(), pi.tolist(), 24, 2)
    assert np.array_equal(exp["perm"], perm) and perm == [1, 4, 5, 0, 2, 3] and vmask is None


# ----------------------------------------------------------------------------- the ABI
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _native.load()


def test_layout_symbols_declared_exported_and_listed(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sba_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name in ("sba_upload_ex", "sba_get_upload_report", "sba_get_layout"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text)
        assert name in _native.EXPORTED_SYMBOLS
        assert hasattr(raw, name)
    assert lib.sba_abi_version() == 2
    assert "#define SBA_ABI_VERSION 2" in text


def test_layout_struct_layouts():
    assert ctypes.sizeof(_native.UploadOpts) == 32          # 2 + 6 reserved int32
    assert ctypes.sizeof(_native.UploadReport) == 88        # 10 + 2 reserved int32, 5 doubles


def test_layout_argument_is_checked_before_any_device_work(lib):
    rig = make_rig(2, 20)
    with pytest.raises(ValueError, match="layout"):
        _native.Problem(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"], layout="gpu")
