"""CPU: the similarity registration entry points are declared, exported and bound; ``align_oracle`` / ``apply_oracle``, the numpy
restatement of the estimator and of the apply step of include/sba_hip.h (which tests/test_gpu_align.py compares the kernels
against), are checked where the truth is exact -- a planted similarity is recovered, a degenerate set is recognised, a moved
solution projects to the same pixels; ``convert_params.apply_similarity_to_camlist`` is held to the same algebra.

The restatement takes R from the SVD (U diag(1, 1, d) V^T) and composes rotations with scipy; the library takes R from Horn's
quaternion matrix by Jacobi rotations and composes quaternions: the same mathematics by two routes."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from lasercalib_amd import _native, convert_params
from lasercalib_amd.synth import _project_np, make_rig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

PLANTED = dict(s=1.0348, rho=np.array([0.3, -2.0, 1.1]), t=np.array([51.0, -20.0, 300.0]))


# ----------------------------------------------------------------------------- numpy restatement (also used by the GPU tests)
def centres_of(cams):
    """(C, 3) camera centres -R(rho)^T t of camera rows."""
    Rc = Rotation.from_rotvec(cams[:, 0:3]).as_matrix()
    return -np.einsum("cji,cj->ci", Rc, cams[:, 3:6])


def planted_map(X, s=PLANTED["s"], rho=PLANTED["rho"], t=PLANTED["t"]):
    return s * X @ Rotation.from_rotvec(rho).as_matrix().T + t


def align_oracle(src_pts=None, tgt_pts=None, pw=None, cams=None, tgt_centres=None, cw=None, with_scale=True):
    """Steps 1-5 of sba_align on float64 numpy arrays.  Returns a dict: scale, R, t, rms_before, rms_after, max_after,
    n_points_used, n_cams_used, sv, unique (the rotation-uniqueness condition s2 + d s3 > 1e-10 s1)."""
    src, dst, w = [], [], []
    n_p = n_c = 0
    if tgt_pts is not None:
        wp = np.ones(len(src_pts)) if pw is None else np.asarray(pw, float)
        use = wp > 0
        src.append(src_pts[use]); dst.append(np.asarray(tgt_pts, float)[use]); w.append(wp[use])
        n_p = int(use.sum())
    if tgt_centres is not None:
        wc = np.ones(len(cams)) if cw is None else np.asarray(cw, float)
        use = wc > 0
        src.append(centres_of(cams)[use]); dst.append(np.asarray(tgt_centres, float)[use]); w.append(wc[use])
        n_c = int(use.sum())
    src, dst, w = np.vstack(src), np.vstack(dst), np.concatenate(w)
    W = w.sum()
    m_s, m_d = (w[:, None] * src).sum(0) / W, (w[:, None] * dst).sum(0) / W
    a, b = src - m_s, dst - m_d
    H = np.einsum("k,ki,kj->ij", w, b, a)
    v_a = np.sum(w * np.sum(a * a, axis=1))
    U, S, Vt = np.linalg.svd(H)
    d = 1.0 if np.linalg.det(U @ Vt) >= 0 else -1.0
    R = U @ np.diag([1.0, 1.0, d]) @ Vt
    s = np.trace(R.T @ H) / v_a if with_scale else 1.0
    t = m_d - s * R @ m_s
    moved = s * src @ R.T + t
    dist = np.linalg.norm(dst - moved, axis=1)
    return dict(scale=s, R=R, t=t, sv=S, unique=bool(S[1] + d * S[2] > 1e-10 * S[0]),
                rms_before=np.sqrt(np.sum(w * np.sum((dst - src) ** 2, axis=1)) / W),
                rms_after=np.sqrt(np.sum(w * dist ** 2) / W), max_after=dist.max(), n_points_used=n_p, n_cams_used=n_c)


def apply_oracle(cams, pts, s, R, t):
    """The apply step: X <- s R X + t, R(rho') = R(rho) R^T, t' = s t_c - R(rho') t; other columns unchanged."""
    new = np.array(cams, dtype=np.float64)
    Rc = Rotation.from_rotvec(cams[:, 0:3]).as_matrix() @ R.T
    new[:, 0:3] = Rotation.from_matrix(Rc).as_rotvec()
    new[:, 3:6] = s * cams[:, 3:6] - Rc @ t
    return new, s * pts @ R.T + t


def rotation_angle(Ra, Rb):
    """angle of Ra^T Rb in radians, from the antisymmetric part and the trace (fine at small angles)."""
    D = Ra.T @ Rb
    v = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.arctan2(np.linalg.norm(v), 0.5 * (np.trace(D) - 1.0)))


def _check_planted(o, label, s_true=PLANTED["s"]):
    R_true = Rotation.from_rotvec(PLANTED["rho"]).as_matrix()
    ds, dR, dt = abs(o["scale"] / s_true - 1), np.abs(o["R"] - R_true).max(), np.abs(o["t"] - PLANTED["t"]).max()
    print(f"{label}: scale {ds:.1e} relative, R {dR:.1e}, t {dt:.1e} mm, rms_after {o['rms_after']:.1e} mm")
    assert ds <= 1e-14 and dR <= 1e-14 and dt <= 1e-12
    assert abs(np.linalg.det(o["R"]) - 1) <= 1e-14 and o["unique"]


# ----------------------------------------------------------------------------- 1. declared, exported, bound
def _header():
    return open(os.path.join(ROOT, "include", "sba_hip.h")).read()


def test_align_is_declared_exported_and_bound():
    text = _header()
    assert re.search(r"\bint sba_align\(sba_handle\* h, const sba_align_opts\* opts", text)
    assert re.search(r"\bint sba_apply_similarity\(sba_handle\* h, double scale, const double\* R", text)
    assert "sba_align" in _native.EXPORTED_SYMBOLS and "sba_apply_similarity" in _native.EXPORTED_SYMBOLS
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _native.load()
    raw = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(raw, "sba_align") and hasattr(raw, "sba_apply_similarity")
    assert lib.sba_align.argtypes is not None and len(lib.sba_align.argtypes) == 7
    assert lib.sba_apply_similarity.argtypes is not None and len(lib.sba_apply_similarity.argtypes) == 4
    assert lib.sba_abi_version() == 2
    assert callable(_native.Problem.align) and callable(_native.Problem.apply_similarity)
    from lasercalib_amd.pySBA import PySBA
    assert callable(PySBA.align)


def test_struct_layouts_match_the_header():
    # sba_align_opts: int32 x 8 = 32;  sba_align_report: double x 16 + int64 + int32 x 2 + double x 5 = 128 + 16 + 40 = 184
    assert ctypes.sizeof(_native.AlignOpts) == 32
    assert ctypes.sizeof(_native.AlignReport) == 184
    text = _header()
    opts = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} sba_align_opts;", text).group(1), flags=re.S)
    assert re.findall(r"\b(with_scale|apply|reserved)\b", opts) == [n for n, _t in _native.AlignOpts._fields_]
    rep = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} sba_align_report;", text).group(1), flags=re.S)
    names = re.findall(r"\b(scale|R|t|rms_before|rms_after|max_after|n_points_used|n_cams_used|reserved|sv|seconds_device|seconds_total)\b", rep)
    assert names == [n for n, _t in _native.AlignReport._fields_]


def test_alignment_object_transforms_points():
    rep = _native.AlignReport()
    R = Rotation.from_rotvec(PLANTED["rho"]).as_matrix()
    rep.scale, rep.R, rep.t = 2.0, (ctypes.c_double * 9)(*R.ravel()), (ctypes.c_double * 3)(1.0, 2.0, 3.0)
    aln = _native.Alignment(rep)
    X = np.arange(12.0).reshape(4, 3)
    assert np.array_equal(aln.R, R) and aln.scale == 2.0
    assert np.allclose(aln.transform(X), 2.0 * X @ R.T + [1.0, 2.0, 3.0], rtol=0, atol=1e-13)


# ----------------------------------------------------------------------------- 2. the restatement against planted truth
def test_oracle_recovers_a_planted_similarity():
    X = make_rig(4, 300)["pts_true"]
    _check_planted(align_oracle(X, planted_map(X)), "300 points")


def test_oracle_recovers_it_from_a_planar_set_and_with_weights():
    X = make_rig(4, 300)["pts_true"]
    flat = X[X[:, 2] == 0.0]
    assert 100 < len(flat) < 200
    o = align_oracle(flat, planted_map(flat))
    assert o["sv"][2] <= 1e-9 * o["sv"][0]                       # planar: H has rank 2, the rotation is still unique
    _check_planted(o, "planar")
    w = np.random.default_rng(5).uniform(0.2, 3.0, 300)
    w[::3] = 0.0
    tgt = planted_map(X)
    tgt[::3] = 1e9                                               # unused targets do not matter
    o = align_oracle(X, tgt, pw=w)
    assert o["n_points_used"] == 200
    _check_planted(o, "weighted, every third weight zero")


def test_oracle_uses_points_and_centres_together_and_fixed_scale():
    rig = make_rig(4, 300)
    X, cams = rig["pts_true"], rig["cams_true"]
    o = align_oracle(X, planted_map(X), cams=cams, tgt_centres=planted_map(centres_of(cams)))
    assert (o["n_points_used"], o["n_cams_used"]) == (300, 4)
    _check_planted(o, "points and centres")
    assert np.abs(centres_of(cams) - np.array([[1500 * np.cos(a), 1500 * np.sin(a), 1200] for a in np.pi / 2 * np.arange(4)])).max() < 1e-9
    o = align_oracle(X, planted_map(X, s=1.0), with_scale=False)
    assert o["scale"] == 1.0
    _check_planted(o, "rigid", s_true=1.0)


def test_oracle_flags_collinear_points_and_keeps_det_plus_one_on_a_reflection():
    u = np.linspace(-500.0, 500.0, 40)[:, None] * np.array([[0.6, -0.3, 0.74]]) + np.array([10.0, 20.0, 30.0])
    o = align_oracle(u, planted_map(u))
    print(f"collinear: (s2 + d s3) / s1 = {(o['sv'][1] + o['sv'][2]) / o['sv'][0]:.1e}")
    assert not o["unique"]
    X = make_rig(4, 300)["pts_true"]
    assert align_oracle(X, planted_map(X))["unique"]
    o = align_oracle(X, planted_map(X * np.array([-1.0, 1.0, 1.0])))
    assert abs(np.linalg.det(o["R"]) - 1) <= 1e-14 and o["rms_after"] > 1.0


def _f9_sparse():
    g = np.load(os.path.join(GOLDEN, "f9_tight.npz"), allow_pickle=False)
    x = g["sparse_x"]
    return x[:66].reshape(6, 11), x[66:].reshape(600, 3), g["sparse_ci"], g["sparse_pi"], g["sparse_uv"]


def test_apply_step_leaves_every_projection_where_it_was():
    cams, pts, ci, pi, _uv = _f9_sparse()
    R = Rotation.from_rotvec(PLANTED["rho"]).as_matrix()
    cams2, pts2 = apply_oracle(cams, pts, PLANTED["s"], R, PLANTED["t"])
    d = np.abs(_project_np(pts2[pi], cams2[ci]) - _project_np(pts[pi], cams[ci])).max()
    print(f"largest pixel change {d:.1e}")
    assert d <= 1e-9
    assert np.array_equal(cams2[:, 6:], cams[:, 6:])
    assert np.abs(centres_of(cams2) - planted_map(centres_of(cams))).max() <= 1e-9


# ----------------------------------------------------------------------------- 3. the exported-file rewrite
def test_camlist_rewrite_follows_the_same_algebra():
    cams, pts, ci, pi, _uv = _f9_sparse()
    R = Rotation.from_rotvec(PLANTED["rho"]).as_matrix()
    s, t = PLANTED["s"], PLANTED["t"]
    readable = convert_params.camera_array_to_readable(cams)
    aruco = [{"camera_matrix": p["K"].T, "distortion_coefficients": np.array([p["d"][0], p["d"][1], 0, 0, 0]),
              "rc_ext": p["R"].T, "tc_ext": p["t"].copy()} for p in readable]
    keep = [(a["rc_ext"].copy(), a["tc_ext"].copy()) for a in aruco]
    moved = convert_params.apply_similarity_to_camlist(aruco, s, R, t)
    cams2, pts2 = apply_oracle(cams, pts, s, R, t)
    for c, (new, old) in enumerate(zip(moved, aruco)):
        assert np.abs(new["rc_ext"] - Rotation.from_rotvec(cams2[c, 0:3]).as_matrix()).max() <= 1e-14
        assert np.abs(new["tc_ext"] - cams2[c, 3:6]).max() <= 1e-12 * 3000
        assert new["camera_matrix"] is old["camera_matrix"] and new["distortion_coefficients"] is old["distortion_coefficients"]
        assert np.array_equal(old["rc_ext"], keep[c][0]) and np.array_equal(old["tc_ext"], keep[c][1])      # input untouched
    # projection invariance of the rewritten extrinsics: camera coordinates grow by s, pixels stay
    worst = 0.0
    for c in range(6):
        X = pts[pi[ci == c]]
        before = X @ aruco[c]["rc_ext"].T + aruco[c]["tc_ext"]
        after = (s * X @ R.T + t) @ moved[c]["rc_ext"].T + moved[c]["tc_ext"]
        assert np.abs(after - s * before).max() <= 1e-9
        worst = max(worst, np.abs(after[:, :2] / after[:, 2:] - before[:, :2] / before[:, 2:]).max() * cams[c, 6])
    print(f"largest pixel change through the rewritten rc_ext / tc_ext: {worst:.1e}")
    assert worst <= 1e-9
    # readable-format dicts ('R' = rc_ext^T, 't') take the same path
    moved_r = convert_params.apply_similarity_to_camlist(readable, s, R, t)
    for new, old, ref in zip(moved_r, readable, moved):
        assert np.abs(new["R"].T - ref["rc_ext"]).max() <= 1e-15 and np.abs(new["t"] - ref["tc_ext"]).max() <= 1e-12
        assert new["K"] is old["K"] and new["d"] is old["d"]                                                   # carried over
    import lasercalib.convert_params as shim
    assert shim.apply_similarity_to_camlist is convert_params.apply_similarity_to_camlist
    with pytest.raises(ValueError):
        convert_params.apply_similarity_to_camlist(aruco, s, np.diag([1.0, 1.0, -1.0]), t)
    with pytest.raises(ValueError):
        convert_params.apply_similarity_to_camlist(aruco, 0.0, R, t)
