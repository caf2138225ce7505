"""GPU: the f32 image of the reduced camera system that the fp32 engine's own loop hands its one-workgroup Cholesky.

In the library's single-rank loop (``lm_begin`` / ``lm_run`` / ``lm_finish``, ``solve_lm``) ``k_build_exchange<float>`` writes the lower
block triangle of S a second time, as floats in the LDS layout of ``k_cholesky_blocked<float, ...>``, and that kernel copies the image
instead of narrowing the doubles of ``E``.  The phase API with a buffer of the caller's keeps the f64 load.  Every float that
reaches the LDS is the same on both ways, so the two loops must agree bit for bit -- which is what pins the image here: rows, block
offsets, the padded tail, the 17- and 20-float row strides, the damped diagonal and the sign of an empty entry all show up as a
different bit somewhere in six iterations.

(On the commit before the image both loops were run on every rig below and compared the same way: they were bit-equal there too,
so the phase API is the reference and no arrays are pinned from a dump.)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from lasercalib_amd import _native  # noqa: E402
from lasercalib_amd.synth import make_rig  # noqa: E402

FULL, SHARED = _native.MODE_FULL, _native.MODE_SHARED_INTR
ITERS = 6


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for name in ("SBA_CHOL", "SBA_CHOL_F32", "SBA_CHOL_F32_TAU", "SBA_NO_WIDE", "SBA_NO_DENSE", "SBA_FUSED_MFMA"):
        monkeypatch.delenv(name, raising=False)


# (cameras, points, make_rig keywords): what each covers is in the id
RIGS = [
    pytest.param(16, 300, {}, id="16x300-n176-fewer-chunks-than-workgroups"),
    pytest.param(16, 5000, {}, id="16x5000-n176-more-chunks-than-workgroups"),
    pytest.param(5, 400, {}, id="5x400-n55-padded-tail-in-last-block"),
    pytest.param(17, 300, {}, id="17x300-n187-16-block-rows-20-float-rows"),
    pytest.param(20, 300, {}, id="20x300-n220-14-block-rows-last-size-on-20-float-rows"),
    pytest.param(21, 300, {}, id="21x300-n231-15-block-rows-first-size-on-17-float-rows"),
    pytest.param(23, 300, {}, id="23x300-n253-16-block-rows-17-float-rows"),
    pytest.param(16, 300, {"tangential": True}, id="16x300-tangential-n208"),
    pytest.param(16, 2000, {"visibility": 0.5, "min_cams_per_point": 4}, id="16x2000-masked-one-launch-route"),
]


def _problem(rig):
    return _native.Problem(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"], dtype="f32")


def _opts(prob, **kw):
    return prob.make_opts(ftol=0.0, xtol=0.0, gtol=0.0, max_iter=ITERS, **kw)


def _own_loop(rig, x0):
    with _problem(rig) as prob:
        prob.set_params(x0)
        prob.lm_begin(_opts(prob))
        _, done = prob.lm_run()
        costs = np.array([r.cost for r in prob.iteration_log()])
        cams, pts, rep = prob.lm_finish()
    return cams.copy(), pts.copy(), costs, done, int(rep.reserved)


def _phase_loop(rig, x0):
    """The iterations as bench.py's phase_api branch enqueues them, with a buffer of the caller's for the reduced system."""
    with _problem(rig) as prob:
        E = torch.empty(prob.exchange_size(), dtype=torch.float64, device="cuda")
        sc = torch.empty(8, dtype=torch.float64, device="cuda")
        prob.set_params(x0)
        prob.lm_begin(_opts(prob))
        done, status = 0, -1
        while done < ITERS and status < 0:
            for _ in range(ITERS - done):
                prob.lm_linearize()
                prob.lm_form_reduced(E.data_ptr())
                prob.lm_solve_trial(E.data_ptr(), sc.data_ptr())
                prob.lm_decide_async(sc.data_ptr(), 1)
            status, done = prob.lm_poll()
        costs = np.array([r.cost for r in prob.iteration_log()])
        cams, pts, rep = prob.lm_finish()
    return cams.copy(), pts.copy(), costs, done, int(rep.reserved)


@pytest.mark.parametrize("C,N,kw", RIGS)
def test_own_loop_equals_phase_api_bit_for_bit(C, N, kw):
    rig = make_rig(C, N, seed=40 + C, **kw)
    x0 = np.hstack((rig["cams0"].ravel(), rig["pts0"].ravel()))
    cams_a, pts_a, costs_a, done_a, retries_a = _own_loop(rig, x0)
    cams_b, pts_b, costs_b, done_b, retries_b = _phase_loop(rig, x0)
    print(f"{C} x {N} {kw}: iterations {done_a} / {done_b}, f64 repeats {retries_a} / {retries_b}, "
          f"max |d cams| {np.max(np.abs(cams_a - cams_b)):.3e}, max |d pts| {np.max(np.abs(pts_a - pts_b)):.3e}, "
          f"costs {costs_a.tolist()} / {costs_b.tolist()}")
    assert done_a == ITERS and done_b == ITERS
    assert np.all(np.isfinite(cams_a)) and np.all(np.isfinite(pts_a)) and costs_a[-1] < costs_a[0]
    assert retries_a == retries_b
    assert np.array_equal(costs_a, costs_b)
    assert np.array_equal(cams_a, cams_b)
    assert np.array_equal(pts_a, pts_b)


def _spd(n, rng, cond):
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.geomspace(1.0, cond, n)) @ Q.T
    return 0.5 * (A + A.T)


def _solve_on_device(C, S, rhs, dU, lam):
    """The entry point of tests/test_gpu_cholesky.py: an arbitrary system handed to sba_lm_solve_trial in the caller's buffer."""
    rig = make_rig(C, 40, seed=C)
    n = 11 * C
    with _native.Problem(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"], dtype="f32") as prob:
        prob.lm_begin(prob.make_opts(ftol=0, xtol=0, gtol=0, lambda0=lam))
        E = torch.zeros(prob.exchange_size(), dtype=torch.float64, device="cuda")
        E[: n * n] = torch.from_numpy(S.ravel())
        E[n * n: n * n + n] = torch.from_numpy(rhs)
        E[n * n + n: n * n + 2 * n] = torch.from_numpy(dU)
        sc = torch.zeros(8, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        prob.lm_solve_trial(E.data_ptr(), sc.data_ptr())
        step = prob.lm_get_step().ravel()
        _, _, rep = prob.lm_finish()
    return step, int(rep.reserved)


@pytest.mark.parametrize("C", [5, 16])
def test_refused_f32_factorisation_is_repeated_in_f64_from_E(C):
    """The systems of test_gpu_cholesky.py::test_f32_lane_factorisation_of_the_fp32_engine that the f32 lanes refuse: condition 1e9
    (pivots below 2^-23 of their diagonal entries) and an indefinite one.  The f64 repeat reads E, is counted, and gives the f64
    kernel's answer (that test's bar: 1e-5 of the largest component); the indefinite system ends as a zero step."""
    rng = np.random.default_rng(300 + C)
    n = 11 * C
    rhs = rng.standard_normal(n)
    dU = np.ones(n)
    S = _spd(n, rng, 1e9)
    ref = np.linalg.solve(S + 1e-6 * np.eye(n), rhs)
    step, retries = _solve_on_device(C, S, rhs, dU, 1e-6)
    err = np.max(np.abs(step - ref)) / np.max(np.abs(ref))
    print(f"C = {C}: condition 1e9, f64 repeats {retries}, error {err:.3e}")
    assert retries == 1 and err <= 1e-5
    S[n - 5, n - 5] = -1.0
    step, retries = _solve_on_device(C, S, rhs, dU, 1e-6)
    assert retries == 1 and np.all(step == 0.0)


def _solve(prob, x0, mode, **kw):
    prob.set_params(x0)
    cams, pts, rep, _ = prob.solve_lm(prob.make_opts(mode=mode, **kw))
    return cams.copy(), pts.copy(), rep.cost, rep.iterations, rep.status


FULL_STOPPED = (FULL, dict(ftol=0.0, xtol=0.0, gtol=0.0, max_iter=3))      # ends with an image of a system nobody solves
SHARED_RUN = (SHARED, dict(ftol=1e-6, max_nfev=40))                        # tied: k_tie_system, no image
FULL_RUN = (FULL, dict(ftol=1e-6, max_nfev=40))


@pytest.mark.parametrize("order", [(FULL_STOPPED, SHARED_RUN, FULL_RUN), (SHARED_RUN, FULL_STOPPED, FULL_RUN)],
                         ids=["full-shared-full", "shared-full-full"])
def test_image_is_never_stale_on_a_reused_handle(order):
    rig = make_rig(16, 120, seed=77, visibility=0.7, min_cams_per_point=4)
    x0 = np.hstack((rig["cams0"].ravel(), rig["pts0"].ravel()))
    with _problem(rig) as used:
        for k, (mode, kw) in enumerate(order):
            got = _solve(used, x0, mode, **kw)
            with _problem(rig) as fresh:
                want = _solve(fresh, x0, mode, **kw)
            assert got[2:] == want[2:], (k, got[2:], want[2:])
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), k
