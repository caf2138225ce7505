"""GPU: one handle, many calls.  Whatever a handle did before, a solve on it gives the bits of the same solve on a fresh handle.

PySBA and the C ABI keep one ``Problem`` and call it again and again with other modes, losses, fixed-point masks and parameter
sets, with ``covariance``, ``triangulate``, ``align``, ``reproj_stats`` and ``unproject`` in between.  A handle carries grow-only
buffers (the large Cholesky's workspace, its two copies of x, the tie tables), epoch counters (``chol_epoch``, ``chol_dag_epoch``
and the flags of the one-launch factorisation), the parity ``cur`` of the double-buffered cameras, points and prepared cameras,
``has_fixed``, the loss, the squared variants' 16 x 16 systems and ``theta``, and the LM state from one call to the next.  None of
it may reach the next solve.

The reference of every assertion is the identical call on a FRESH handle brought to the same starting point the same way: both
handles receive ``set_params(x)`` right before the solve under test (except where the test is about the parameters a call left
on the handle), so the upload and ``set_params`` rounding paths cannot differ.  The engine is bit-reproducible across handles
(tests/test_gpu_large_cams.py::test_two_handles_solving_at_once_on_one_card, tests/test_gpu_fused_f64.py), so there are three
kinds of bar in this file and no other:

  * bit equality: ``np.array_equal`` on cameras and points, ``==`` on cost, nfev, iterations and status.  Every case first runs a
    CONTROL, fresh against fresh, under the same bar: a used-handle failure is then the handle's, not the route's;
  * one independent f64 anchor per case: the cost the last solve on the used handle reports equals
    ``0.5 * sum(fun(x) ** 2)`` of the oracle at the returned parameters, to 1e-9 relative (f64) or 1e-4 (f32) -- the bars of
    tests/test_gpu_large_cams.py::test_large_rigs_vs_reference_oracle (linear loss, MODE_FULL / SHARED_INTR / POINTS_ONLY);
  * (none so far) a control-derived bar for a route whose control is not bit-equal.

Rigs have 80 .. 150 points: what can go wrong lives in the system size, its padding and the parities, not in the point count.
"""
import collections

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from lasercalib_amd import _native  # noqa: E402
from lasercalib_amd.synth import make_rig  # noqa: E402
from oracle import sba_oracle as orc  # noqa: E402
from oracle import sba_oracle_tangential as orc13  # noqa: E402

FULL, POINTS_ONLY, SHARED = _native.MODE_FULL, _native.MODE_POINTS_ONLY, _native.MODE_SHARED_INTR
CAMS_SQ, TRANSFORM_SQ = _native.MODE_CAMS_ONLY_SQ, _native.MODE_TRANSFORM_SQ
MODE_NAMES = {FULL: "FULL", POINTS_ONLY: "POINTS_ONLY", SHARED: "SHARED_INTR", CAMS_SQ: "CAMS_ONLY_SQ", TRANSFORM_SQ: "TRANSFORM_SQ"}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert _native.device_count() > 0, "no HIP device visible: GPU tests must run on the MI355X box"


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for name in ("SBA_CHOL", "SBA_CHOL_F32", "SBA_CHOL_BIG", "SBA_CHOL_BIG_MIN_N", "SBA_NO_WIDE", "SBA_NO_DENSE"):
        monkeypatch.delenv(name, raising=False)


# cameras -> (points, visibility, 13-parameter model): some 30 observations per camera, every point seen by at least 4 cameras
RIGS = {5: (80, 0.9, False), 16: (100, 0.6, False), 17: (100, 0.6, False), 20: (100, 0.5, False), 23: (100, 0.5, False),
        24: (100, 0.5, False), 47: (110, 0.3, False), 64: (120, 0.3, False), 96: (140, 0.25, False), 128: (150, 0.2, True)}
_rigs = {}


def _rig(C):
    if C not in _rigs:
        N, vis, tangential = RIGS[C]
        rig = make_rig(C, N, seed=300 + C, visibility=vis, min_cams_per_point=4, tangential=tangential)
        rig["x0"] = np.hstack((rig["cams0"].ravel(), rig["pts0"].ravel()))
        rig["tangential"] = tangential
        _rigs[C] = rig
    return _rigs[C]


def _problem(C, dtype):
    rig = _rig(C)
    return _native.Problem(rig["cams0"], rig["pts0"], rig["points_2d"], rig["camera_ind"], rig["point_ind"], dtype=dtype)


Out = collections.namedtuple("Out", "cams pts cost nfev iterations status theta")
CONVERGE = dict(ftol=1e-6, max_nfev=60)        # to convergence in batches of iterations, as the product runs (no max_iter)
SQ = dict(ftol=1e-4, max_nfev=60)              # the squared variants' tolerance (bundle_adjustment_camonly)


def _solve(prob, x, mode=FULL, **opts):
    """set_params(x) (None: from the handle's current parameters), then one solve."""
    if x is not None:
        prob.set_params(x)
    kw = dict(SQ if mode in (CAMS_SQ, TRANSFORM_SQ) else CONVERGE)
    kw.update(opts)
    cams, pts, rep, _ = prob.solve_lm(prob.make_opts(mode=mode, **kw))
    theta = prob.get_transform().copy() if mode == TRANSFORM_SQ else None
    return Out(cams.copy(), pts.copy(), rep.cost, rep.nfev, rep.iterations, rep.status, theta)


def _diff(a, b):
    """The fields in which two solves differ (empty: the same bits), with the size of the difference."""
    out = []
    for name in ("cost", "nfev", "iterations", "status"):
        va, vb = getattr(a, name), getattr(b, name)
        if va != vb:
            out.append(f"{name} {va!r} vs {vb!r}" + (f" (relative {abs(va - vb) / abs(vb):.2e})" if name == "cost" and vb else ""))
    for name in ("cams", "pts", "theta"):
        va, vb = getattr(a, name), getattr(b, name)
        if (va is None) != (vb is None) or (va is not None and not np.array_equal(va, vb)):
            out.append(f"{name} differ" + (f" (largest |difference| {np.nanmax(np.abs(va - vb)):.3e})" if va is not None and vb is not None else ""))
    return out


_PREPS = {
    None: lambda prob, rig: None,
    "huber": lambda prob, rig: prob.set_robust_loss("huber", 1.0),
    "mask": lambda prob, rig: prob.set_fixed_points(_mask(rig)),
}
_refs = {}


def _mask(rig):
    m = np.zeros(rig["pts0"].shape[0], dtype=bool)
    m[::7] = True
    return m


def _fresh(C, dtype, x=None, mode=FULL, prep=None, env=None, cached=True, **opts):
    """The solve on a handle that has done nothing else; cached=True: computed once per process and shared (never modified)."""
    rig = _rig(C)
    x = rig["x0"] if x is None else x
    key = (C, dtype, x.tobytes(), mode, prep, env, tuple(sorted(opts.items())))
    if cached and key in _refs:
        return _refs[key]
    with _problem(C, dtype) as prob:
        _PREPS[prep](prob, rig)
        out = _solve(prob, x, mode, **opts)
    if cached:
        _refs[key] = out
    return out


def _control(C, dtype, what, **kw):
    """Fresh against fresh under the bar of the used handle; returns the (shared) reference."""
    ref = _fresh(C, dtype, **kw)
    again = _fresh(C, dtype, cached=False, **kw)
    d = _diff(again, ref)
    assert not d, f"CONTROL, two fresh handles, {C} cameras {dtype}, {what}: the engine is not bit-reproducible on this route: {d}"
    return ref


def _anchor(C, dtype, out):
    """The reported cost against the oracle's residual function at the returned parameters (f64, independent of the engine)."""
    rig = _rig(C)
    o = orc13 if rig["tangential"] else orc
    x = np.hstack((out.cams.ravel(), out.pts.ravel()))
    cost64 = 0.5 * np.sum(o.fun(x, C, rig["pts0"].shape[0], rig["camera_ind"], rig["point_ind"], rig["points_2d"], 1.0) ** 2)
    rel = abs(cost64 - out.cost) / cost64
    print(f"anchor {C} cameras {dtype}: reported {out.cost!r}, oracle {cost64!r}, relative {rel:.2e}")
    assert rel <= (1e-9 if dtype == "f64" else 1e-4), (out.cost, cost64, rel)


# ----------------------------------------------------------------------------- (a) mode sequences across the Cholesky routes
SEQUENCE = (FULL, SHARED, FULL, POINTS_ONLY, SHARED)
SEQ_CASES = [(16, "f32"), (16, "f64"), (20, "f32"), (24, "f64"), (47, "f32"), (47, "f64"), (64, "f32"), (64, "f64"), (96, "f32"),
             (128, "f32"), (128, "f64")]


def _run_sequence(C, dtype, env=None):
    refs = {mode: _control(C, dtype, MODE_NAMES[mode], mode=mode, env=env) for mode in dict.fromkeys(SEQUENCE)}
    assert refs[FULL].nfev >= 3 and refs[SHARED].nfev >= 3, "the solves must take trial steps for the sequence to mean anything"
    bad = []
    with _problem(C, dtype) as prob:
        for step, mode in enumerate(SEQUENCE):
            out = _solve(prob, _rig(C)["x0"], mode)
            d = _diff(out, refs[mode])
            if d:
                bad.append(f"step {step} ({MODE_NAMES[mode]} after {' -> '.join(MODE_NAMES[m] for m in SEQUENCE[:step]) or 'nothing'}): {d}")
    assert not bad, f"{C} cameras {dtype}: used handle vs fresh handle: " + "; ".join(bad)
    _anchor(C, dtype, out)


@pytest.mark.parametrize("C,dtype", SEQ_CASES)
def test_mode_sequence_on_one_handle_equals_fresh_handles(C, dtype):
    """FULL -> SHARED_INTR -> FULL -> POINTS_ONLY -> SHARED_INTR on one handle, from x0 each time, every step against a fresh
    handle.  The reduced system has n = P C unknowns in MODE_FULL and 3 + (P - 3) C tied ones in MODE_SHARED_INTR; the camera
    counts put the two on different factorisations (chol_route, sba_chol_solve.hpp) or different paddings (cholbig_npad = the next multiple of 64
    above 16 ceil(n / 16)); MODE_POINTS_ONLY has no camera system and leaves the buffers of the other two as they are.

        cameras  n FULL / tied   MODE_FULL                                         MODE_SHARED_INTR
        16       176 / 131       BLOCKED (all in LDS; f32: on f32 lanes)           BLOCKED
        20       220 / 163       LL_F32 (f32 lanes, left-looking kernel behind)    BLOCKED                          [f32]
        24       264 / 195       BIG_DAG, npad 320 (5 block rows)                  LL (left-looking, 264 <= 512)    [f64]
        47       517 / 379       BIG_DAG(_F32), npad 576, x in 9 blocks            BIG_DAG(_F32), npad 448, 6 blocks
        64       704 / 515       BIG_DAG(_F32), npad 768, x in 11 blocks           BIG_DAG(_F32), npad 576, 9 blocks
        96       1056 / 771      BIG_DAG_F32, npad 1088, x in 17 blocks            BIG_DAG_F32, npad 832, 13 blocks [f32]
        128      1664 / 1283     BIG_DAG(_F32), npad 1728, 26 blocks (13 param.)   BIG_DAG(_F32), npad 1344, 21 blocks

    (f32: k_chol_big_dag<float> with the f64 instance behind it; f64: the f64 walker.)  All BIG routes end in
    k_chol_big_back_all, whose two copies of x lived npad apart before this test existed: 64 cameras, FULL then SHARED_INTR, put
    the second solve's copy 1 at [576, 1152) over the x the first one left in [0, 704)."""
    _run_sequence(C, dtype)


def test_mode_sequence_with_the_per_column_launches(monkeypatch):
    """SBA_CHOL_BIG=launches: k_chol_big_prepare / k_chol_big_step per block column (BIG_LAUNCHES) share k_chol_big_back_all, and
    with it the two copies of x, with the one-launch factorisation: the 64-camera sequence once more."""
    monkeypatch.setenv("SBA_CHOL_BIG", "launches")
    _run_sequence(64, "f64", env="launches")


# ----------------------------------------------------------------------------- (b) a solve that ends on the last enqueued iteration
EXACT = dict(ftol=1e-15, xtol=1e-15, gtol=1e-15)          # nothing but max_iter stops the first solve
END_CASES = [(47, "f32"), (47, "f64"), (64, "f32"), (64, "f64")]


def _first_then_second(C, dtype, first_mode, second_mode, warm=False):
    """first_mode with max_iter = K (exactly K iterations are enqueued: no launch follows the last real one), then second_mode to
    convergence from x0, against a fresh handle; K = 2 .. 5, further until both parities of the launch count have occurred."""
    x0 = _rig(C)["x0"]
    x_true = np.hstack((_rig(C)["cams_true"].ravel(), _rig(C)["pts_true"].ravel()))
    ref = _control(C, dtype, MODE_NAMES[second_mode], mode=second_mode)
    assert ref.nfev >= 3
    bad, parities, K = [], set(), 2
    while K <= 5 or (len(parities) < 2 and K <= 12):
        with _problem(C, dtype) as prob:
            if warm:        # the buffers already have the size of the larger system: nothing is allocated (and filled) later on
                # (from the true parameters, not from x0: the x this launch leaves behind must not be the x that the first
                #  iteration of the solve under test computes anyway -- a stale copy of those bits would pass for the right answer)
                _solve(prob, x_true, FULL, max_iter=1, **EXACT)
            first = _solve(prob, x0, first_mode, max_iter=K, **EXACT)
            assert first.status == 0 and first.iterations == K == first.nfev - 1, (K, first.status, first.iterations, first.nfev)
            launches = first.nfev - 1 + (1 if warm else 0)          # trial solves = launches of the back substitution so far
            parities.add(launches & 1)
            out = _solve(prob, x0, second_mode)
        d = _diff(out, ref)
        if d:
            bad.append(f"K = {K} ({launches} launches before, parity {launches & 1}): {d}")
        K += 1
    assert parities == {0, 1}, f"only parity {parities} of the launch count occurred"
    assert not bad, (f"{C} cameras {dtype}, {'FULL(1) -> ' if warm else ''}{MODE_NAMES[first_mode]}(max_iter=K) -> {MODE_NAMES[second_mode]} "
                     "vs a fresh handle: " + "; ".join(bad))
    _anchor(C, dtype, out)


@pytest.mark.parametrize("C,dtype", END_CASES)
def test_full_stopped_by_max_iter_then_shared_intrinsics(C, dtype):
    """The smaller system after the larger one, no drained launch in between.  Before the copies of x were placed at a fixed
    stride, an EVEN number of launches left the x of the FULL solve where copy 1 of the SHARED_INTR solve begins (64 cameras:
    [576, 704) of the old copy 0 = block rows 0 and 1 of the new copy 1) and block row 0 took a stale x_1 without waiting: all
    four cases failed then at K = 2 and K = 4 and passed at K = 3 and 5 (another iteration count, cameras off by 0.1 .. 2 units)."""
    _first_then_second(C, dtype, FULL, SHARED)


@pytest.mark.parametrize("warm", [False, True], ids=["fresh-buffers", "sized-buffers"])
@pytest.mark.parametrize("C,dtype", END_CASES)
def test_shared_intrinsics_stopped_by_max_iter_then_full(C, dtype, warm):
    """The mirror order.  On a handle that starts with SHARED_INTR the workspace grows for the FULL solve and both copies are
    filled anew; sized-buffers solves one FULL iteration first, as a handle in use has: nothing is refilled then, and the x of
    the SHARED_INTR solve (64 cameras: old copy 1, [576, 1091)) lay inside copy 0 of the FULL solve that follows: all four
    sized-buffers cases failed then at K = 2 and K = 4 (3 and 5 launches before the FULL solve); fresh-buffers always passed."""
    _first_then_second(C, dtype, SHARED, FULL, warm=warm)


@pytest.mark.parametrize("C,dtype", END_CASES)
def test_full_stopped_by_max_iter_then_full(C, dtype):
    """Two systems of the same size, no drained launch in between: the hand-over protocol for equal npad."""
    _first_then_second(C, dtype, FULL, FULL)


# ----------------------------------------------------------------------------- (c) option state does not stick
@pytest.mark.parametrize("C,dtype", [(16, "f64"), (23, "f32"), (64, "f64")])
def test_loss_and_fixed_points_do_not_stick(C, dtype):
    rig = _rig(C)
    x0 = rig["x0"]
    plain = _control(C, dtype, "plain FULL")
    huber = _control(C, dtype, "FULL with the Huber loss", prep="huber")
    fixed = _control(C, dtype, "FULL with fixed points", prep="mask")
    assert _diff(huber, plain) and _diff(fixed, plain), "the options must change the solve for this test to mean anything"
    bad = []

    def check(what, out, ref):
        d = _diff(out, ref)
        if d:
            bad.append(f"{what}: {d}")

    with _problem(C, dtype) as prob:
        check("plain", _solve(prob, x0), plain)
        prob.set_robust_loss("huber", 1.0)
        check("huber", _solve(prob, x0), huber)
        prob.set_robust_loss("linear")
        check("linear loss after huber", _solve(prob, x0), plain)
        prob.set_fixed_points(_mask(rig))
        check("fixed points", _solve(prob, x0), fixed)
        prob.set_fixed_points(None)
        check("fixed points cleared", _solve(prob, x0), plain)
        prob.set_fixed_points(np.zeros(rig["pts0"].shape[0], dtype=bool))
        out = _solve(prob, x0)
        check("all-False mask", out, plain)
    assert not bad, f"{C} cameras {dtype}: used handle vs fresh handle: " + "; ".join(bad)
    _anchor(C, dtype, out)


# ----------------------------------------------------------------------------- (d) squared variants and points-only in between
@pytest.mark.parametrize("C,dtype", [(5, "f64"), (16, "f32")])
def test_squared_variants_between_full_solves(C, dtype):
    x0 = _rig(C)["x0"]
    seq = (CAMS_SQ, FULL, TRANSFORM_SQ, FULL, POINTS_ONLY, FULL, TRANSFORM_SQ)
    refs = {mode: _control(C, dtype, MODE_NAMES[mode], mode=mode) for mode in dict.fromkeys(seq)}
    assert refs[CAMS_SQ].nfev >= 2 and refs[TRANSFORM_SQ].nfev >= 2 and refs[FULL].nfev >= 3
    assert not np.array_equal(refs[TRANSFORM_SQ].theta, np.eye(3, 4).ravel()), "the transform must move for this test to mean anything"
    bad = []
    with _problem(C, dtype) as prob:
        for step, mode in enumerate(seq):
            out = _solve(prob, x0, mode)            # (TRANSFORM_SQ: theta = get_transform() right after the solve, part of the comparison)
            d = _diff(out, refs[mode])
            if d:
                bad.append(f"step {step} ({MODE_NAMES[mode]}): {d}")
            if mode == FULL:
                last_full = out
    assert not bad, f"{C} cameras {dtype}: used handle vs fresh handle: " + "; ".join(bad)
    _anchor(C, dtype, last_full)


# ----------------------------------------------------------------------------- (e) calls between solves
def _read_only_calls(prob, rig):
    N = rig["pts0"].shape[0]
    _, pts = prob.get_params()
    prob.covariance()
    prob.reproj_stats()
    prob.triangulate(write_back=False)
    prob.align(target_points=pts, apply=False)
    prob.unproject(_native.z_planes(rig["pts_true"][:, 2], N), write_back=False)


@pytest.mark.parametrize("C,dtype", [(17, "f32"), (64, "f64")])
def test_read_only_calls_between_solves_change_nothing(C, dtype):
    rig = _rig(C)
    x0 = rig["x0"]
    ref = _control(C, dtype, "FULL")
    with _problem(C, dtype) as prob:
        first = _solve(prob, x0)
        before = prob.get_params()
        _read_only_calls(prob, rig)
        after = prob.get_params()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), "a read-only call moved the parameters"
        assert np.array_equal(before[0], first.cams) and np.array_equal(before[1], first.pts)
        second = _solve(prob, x0)
    assert not _diff(first, ref), _diff(first, ref)
    assert not _diff(second, first), f"{C} cameras {dtype}: the solve after the read-only calls vs the one before: {_diff(second, first)}"
    _anchor(C, dtype, second)


@pytest.mark.parametrize("C,dtype", [(17, "f32"), (64, "f64")])
def test_solve_from_what_a_writing_call_left_on_the_handle(C, dtype):
    """triangulate(write_back=True) and align(apply=True) change the handle's parameters on the device: the f64 copies, and with
    them the points in the engine's type and the prepared cameras of the CURRENT side of the double buffers.  A solve started
    from there (no set_params) equals a fresh handle given the same parameters by set_params(get_params())."""
    rig = _rig(C)
    ang = 0.3
    R = np.array([[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]])
    bad = []
    with _problem(C, dtype) as prob:
        _solve(prob, rig["x0"], max_iter=3)               # (the current side of the double buffers is where the accepted steps left it)
        tri = prob.triangulate(write_back=True)
        assert tri.ok.sum() >= rig["pts0"].shape[0] // 2
        cams, pts = prob.get_params()
        assert np.array_equal(pts[tri.ok], tri.points[tri.ok])
        x_tri = np.hstack((cams.ravel(), pts.ravel()))
        out = _solve(prob, None, max_iter=3)              # (stopped early: the solve after the alignment still has steps to take)
        d = _diff(out, _control(C, dtype, "FULL from the triangulated points", x=x_tri, max_iter=3))
        if d:
            bad.append(f"after triangulate(write_back=True): {d}")
        _, pts = prob.get_params()
        al = prob.align(target_points=1.1 * pts @ R.T + np.array([10.0, -20.0, 30.0]), apply=True)
        assert abs(al.scale - 1.1) <= 1e-6
        cams, pts = prob.get_params()
        x_al = np.hstack((cams.ravel(), pts.ravel()))
        out = _solve(prob, None, max_iter=4)
        d = _diff(out, _control(C, dtype, "FULL from the aligned solution", x=x_al, max_iter=4))
        if d:
            bad.append(f"after align(apply=True): {d}")
    assert not bad, f"{C} cameras {dtype}: used handle vs fresh handle: " + "; ".join(bad)
    _anchor(C, dtype, out)
