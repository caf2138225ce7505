"""GPU: the observation layout built by the device pass (csrc/sba_layout.hpp, Problem(..., layout="device")).

* against the numpy statement of the rule (tests/test_upload_layout_host.py::expected_layout, itself checked there against a
  transcription of the host loops): exact equality of every array of Problem.layout();
* against the host route (layout="host"): the same layout, the same report flags and, layout being identical, bit-equal
  solves (no tolerance: identical kernels on identical data);
* the lists the device pass declines end exactly as the host route ends them; device tensors give what numpy arrays give.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lasercalib_amd import _native  # noqa: E402
from lasercalib_amd.synth import make_rig  # noqa: E402
from test_upload_layout_host import expected_layout, reorder, strip_points  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RIGS = [(17, 300, 0.45, 4), (16, 300, 0.5, 2), (8, 400, 0.4, 2), (40, 150, 0.1, 4), (128, 120, 0.1, 4)]
ORDERS = ["emitted", "shuffled", "camdesc"]
FLAGS = ("dense", "masked", "group_indexed", "identity_perm", "n_blocks", "n_chunks", "max_degree")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert _native.device_count() > 0, "no HIP device visible: GPU tests must run on the MI355X box"


def _f7(tag):
    g = np.load(os.path.join(GOLDEN, "f7_dataset.npz"), allow_pickle=False)
    C = int(g[f"cat_{tag}_n_cams"])
    pts = np.ascontiguousarray(g[f"cat_{tag}_points_3d"], dtype=np.float64)
    cams = make_rig(C, 4, seed=0)["cams0"]
    return cams, pts, g[f"cat_{tag}_points_2d"].astype(np.float64), g[f"cat_{tag}_camera_ind"].astype(np.int64), \
        g[f"cat_{tag}_point_ind"].astype(np.int64)


def _weights(M, on):
    return np.random.default_rng(9).uniform(0.5, 1.5, M) if on else None


def _assert_layout(got, exp, weights, C):
    for key in ("perm", "pt_start", "cam_pm", "pt_pm", "uv_pm", "pt_cm", "uv_cm", "cam_start"):
        assert np.array_equal(got[key], exp[key]), key
    if weights:
        assert np.array_equal(got["w_pm"], exp["w_pm"]) and np.array_equal(got["w_cm"], exp["w_cm"])
    if C <= 16:
        assert np.array_equal(got["vis_mask"], exp["vis_mask"])


def _check_device_layout(cams, pts, uv, ci, pi, w, dtype):
    C, N = cams.shape[0], pts.shape[0]
    with _native.Problem(cams, pts, uv, ci, pi, weights=w, dtype=dtype, layout="device") as dev:
        rep, lay = dev.upload_report(), dev.layout()
    exp = expected_layout(uv, ci, pi, w, C, N, dtype)
    assert rep["route"] == "device general" and rep["decline_reason"] is None, rep
    _assert_layout(lay, exp, w is not None, C)
    assert rep["identity_perm"] == np.array_equal(exp["perm"], np.arange(ci.size))
    with _native.Problem(cams, pts, uv, ci, pi, weights=w, dtype=dtype, layout="host") as host:
        hrep, hlay = host.upload_report(), host.layout()
    assert hrep["route"] == "host"
    for key in lay:
        assert np.array_equal(lay[key], hlay[key]), key
    for key in FLAGS:
        assert rep[key] == hrep[key], (key, rep[key], hrep[key])
    return rep


def _solve(prob):
    cams, pts, rep, log = prob.solve_lm(prob.make_opts(ftol=1e-8))
    rows = [(r.iteration, r.accepted, r.nfev, r.cost, r.cost_reduction, r.step_norm, r.optimality, r.lambda_, r.rho) for r in log]
    return cams, pts, rep.cost, rep.nfev, rows, prob.residual()[0]


def _assert_same_solve(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[2] == b[2] and a[3] == b[3]
    assert np.array_equal(np.array(a[4]), np.array(b[4]), equal_nan=True)
    assert np.array_equal(a[5], b[5])


# ----------------------------------------------------------------------------- 1 + 2: the rule, and the host route
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("C,N,vis,mincam", RIGS)
def test_device_layout_is_the_rule_and_the_host_layout(C, N, vis, mincam, order, weights, dtype):
    rig = make_rig(C, N, seed=0, visibility=vis, min_cams_per_point=mincam)
    uv, ci, pi = reorder(*strip_points(rig, [5, N - 1]), order)
    rep = _check_device_layout(rig["cams0"], rig["pts0"], uv, ci, pi, _weights(ci.size, weights), dtype)
    # as emitted nothing moves; above one camera group nothing reorders inside a point either
    assert rep["identity_perm"] == (order == "emitted" or (order == "camdesc" and C > 16))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("weights", [False, True])
def test_reference_dataset_layout(dtype, weights):
    cams, pts, uv, ci, pi = _f7("two")
    assert cams.shape[0] == 5 and pts.shape[0] == 61 and ci.size == 230
    _check_device_layout(cams, pts, uv, ci, pi, _weights(ci.size, weights), dtype)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("C,N,vis,mincam", RIGS)
def test_solves_are_bit_equal_between_the_routes(C, N, vis, mincam, order, dtype):
    rig = make_rig(C, N, seed=0, visibility=vis, min_cams_per_point=mincam)
    uv, ci, pi = reorder(rig["points_2d"], rig["camera_ind"], rig["point_ind"], order)
    w = _weights(ci.size, True)
    out = []
    for route in ("host", "device"):
        with _native.Problem(rig["cams0"], rig["pts0"], uv, ci, pi, weights=w, dtype=dtype, layout=route) as prob:
            assert prob.upload_report()["route"] == ("host" if route == "host" else "device general")
            out.append(_solve(prob))
    _assert_same_solve(*out)


# ----------------------------------------------------------------------------- 3: determinism
def test_shuffled_upload_repeats_its_permutation():
    rig = make_rig(17, 2000, seed=0, visibility=0.45, min_cams_per_point=4)
    uv, ci, pi = reorder(rig["points_2d"], rig["camera_ind"], rig["point_ind"], "shuffled")
    perms = []
    for _ in range(5):
        with _native.Problem(rig["cams0"], rig["pts0"], uv, ci, pi, dtype="f32", layout="device") as prob:
            assert prob.upload_report()["route"] == "device general"
            perms.append(prob.layout()["perm"])
    for p in perms[1:]:
        assert np.array_equal(p, perms[0])
    assert np.array_equal(perms[0], np.lexsort((np.arange(ci.size), pi)))


# ----------------------------------------------------------------------------- 4: declines
def _outcome(cams, pts, uv, ci, pi, route, solve=False):
    try:
        with _native.Problem(cams, pts, uv, ci, pi, dtype="f64", layout=route) as prob:
            return ("ok", prob.upload_report(), prob.layout(), _solve(prob) if solve else None)
    except Exception as e:  # noqa: BLE001  (type and text are compared)
        return ("raised", type(e), str(e))


def _assert_declined_like_host(cams, pts, uv, ci, pi, reason, solve=False):
    h = _outcome(cams, pts, uv, ci, pi, "host", solve)
    d = _outcome(cams, pts, uv, ci, pi, "device", solve)
    assert h[0] == d[0]
    if h[0] == "raised":
        assert h[1:] == d[1:]
        return h
    assert d[1]["route"] == "host" and d[1]["decline_reason"] == reason, d[1]
    for key in h[2]:
        assert np.array_equal(h[2][key], d[2][key]), key
    for key in FLAGS:
        assert h[1][key] == d[1][key]
    if solve:
        _assert_same_solve(h[3], d[3])
    return h


def test_reference_three_dataset_list_declines_to_the_host():
    cams, pts, uv, ci, pi = _f7("three")
    pairs = pi * cams.shape[0] + ci
    assert pairs.size - np.unique(pairs).size == 67 and np.any(pi[1:] < pi[:-1])
    assert pts.shape[0] - np.unique(pi).size == 21
    _assert_declined_like_host(cams, pts, uv, ci, pi, "duplicate pair")


@pytest.mark.parametrize("what", ["camera", "point", "negative"])
def test_out_of_range_indices_raise_the_host_message(what):
    rig = make_rig(8, 200, seed=1, visibility=0.5)
    uv, ci, pi = rig["points_2d"], rig["camera_ind"].copy(), rig["point_ind"].copy()
    if what == "camera":
        ci[[700, 311]] = 8
    elif what == "point":
        pi[123] = 200
    else:
        ci[55] = -1
    h = _assert_declined_like_host(rig["cams0"], rig["pts0"], uv, ci, pi, None)
    assert h[0] == "raised" and "out of range at observation %d" % {"camera": 311, "point": 123, "negative": 55}[what] in h[2]


def test_single_duplicate_pair_in_one_group_declines_with_the_same_solve():
    rig = make_rig(8, 200, seed=2, visibility=0.6)
    uv, ci, pi = (np.concatenate([a, a[40:41]]) for a in (rig["points_2d"], rig["camera_ind"], rig["point_ind"]))
    _assert_declined_like_host(rig["cams0"], rig["pts0"], uv, ci, pi, "duplicate pair", solve=True)


def test_point_with_257_observations_raises_the_host_message():
    rig = make_rig(40, 60, seed=3, visibility=0.2, min_cams_per_point=4)
    extra = np.full(257, int(np.nonzero(rig["point_ind"] == 7)[0][0]))
    uv, ci, pi = (np.concatenate([a[rig["point_ind"] != 7], a[extra]]) for a in (rig["points_2d"], rig["camera_ind"], rig["point_ind"]))
    h = _assert_declined_like_host(rig["cams0"], rig["pts0"], uv, ci, pi, None)
    assert h[0] == "raised" and "more than 256 observations" in h[2]


def test_duplicates_above_one_group_are_not_a_decline():
    rig = make_rig(40, 60, seed=3, visibility=0.2, min_cams_per_point=4)
    extra = np.full(200, int(np.nonzero(rig["point_ind"] == 7)[0][0]))
    uv, ci, pi = (np.concatenate([a, a[extra]]) for a in (rig["points_2d"], rig["camera_ind"], rig["point_ind"]))
    rep = _check_device_layout(rig["cams0"], rig["pts0"], uv, ci, pi, None, "f64")
    assert rep["max_degree"] <= 256 and rep["max_degree"] > 200


# ----------------------------------------------------------------------------- 5: device arrays
def test_device_tensors_equal_numpy_arrays():
    torch = pytest.importorskip("torch")
    rig = make_rig(17, 400, seed=4, visibility=0.45, min_cams_per_point=4)
    uv, ci, pi = reorder(rig["points_2d"], rig["camera_ind"], rig["point_ind"], "shuffled")
    w = _weights(ci.size, True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")      # noqa: E731
    for dtype in ("f32", "f64"):
        for route in ("device", "host", "auto"):
            with _native.Problem(rig["cams0"], rig["pts0"], uv, ci, pi, weights=w, dtype=dtype, layout="host") as ref:
                lay_ref, sol_ref = ref.layout(), _solve(ref)
            with _native.Problem(rig["cams0"], rig["pts0"], t(uv), t(ci), t(pi), weights=t(w), dtype=dtype, layout=route) as prob:
                rep, lay, sol = prob.upload_report(), prob.layout(), _solve(prob)
            assert rep["route"] == ("device general" if route == "device" else "host")
            for key in lay:
                assert np.array_equal(lay[key], lay_ref[key]), key
            _assert_same_solve(sol, sol_ref)
    with pytest.raises(ValueError, match="points_2d"):
        _native.Problem(rig["cams0"], rig["pts0"], t(uv).float(), t(ci), t(pi))
    with pytest.raises(ValueError, match="camera_ind"):
        _native.Problem(rig["cams0"], rig["pts0"], t(uv), t(np.stack([ci, ci], 1))[:, 0], t(pi))
    bad = ci.copy()
    bad[17] = 17
    with pytest.raises(_native.SbaError, match="camera/point index out of range at observation 17"):
        _native.Problem(rig["cams0"], rig["pts0"], t(uv), t(bad), t(pi), layout="device")


def test_pysba_passes_device_tensors_through(capsys):
    torch = pytest.importorskip("torch")
    from lasercalib_amd.pySBA import PySBA
    rig = make_rig(6, 300, seed=6, visibility=0.7)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")      # noqa: E731
    a = PySBA(rig["cams0"].copy(), rig["pts0"].copy(), rig["points_2d"], rig["camera_ind"], rig["point_ind"])
    b = PySBA(rig["cams0"].copy(), rig["pts0"].copy(), t(rig["points_2d"]), t(rig["camera_ind"]), t(rig["point_ind"]))
    ra, rb = a.bundleAdjust(1e-6), b.bundleAdjust(1e-6)
    capsys.readouterr()
    assert ra.cost == rb.cost and ra.nfev == rb.nfev
    assert np.array_equal(a.cameraArray, b.cameraArray) and np.array_equal(a.points3D, b.points3D)
    assert np.array_equal(ra.fun, rb.fun)


# ----------------------------------------------------------------------------- 6: dense lists
def test_dense_canonical_list_keeps_the_dense_kernel():
    rig = make_rig(12, 500, seed=5)
    for route in ("auto", "device"):
        with _native.Problem(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"], dtype="f32",
                             layout=route) as prob:
            rep = prob.upload_report()
            assert rep["route"] == "device dense" and rep["dense"] and rep["identity_perm"], rep
            lay = prob.layout()
    exp = expected_layout(rig["points_2d"], rig["camera_ind"], rig["point_ind"], None, 12, 500, "f32")
    _assert_layout(lay, exp, False, 99)


# ----------------------------------------------------------------------------- 7: size
def test_large_shuffled_list():
    rig = make_rig(17, 50000, seed=0, visibility=0.45, min_cams_per_point=4)
    uv, ci, pi = reorder(rig["points_2d"], rig["camera_ind"], rig["point_ind"], "shuffled")
    assert ci.size > 300000
    _check_device_layout(rig["cams0"], rig["pts0"], uv, ci, pi, _weights(ci.size, True), "f32")
    with _native.Problem(rig["cams0"], rig["pts0"], uv, ci, pi, dtype="f32") as prob:          # above the crossover: automatic
        assert prob.upload_report()["route"] == "device general"
