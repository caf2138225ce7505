"""One LM iteration of the other four modes of sba_solve_lm against the exact reference (oracle/exact_model.py), as
tests/test_gpu_exact_model.py holds SBA_MODE_FULL: default routing (no SBA_* knob), inputs rounded to float32, both engines, the
iteration driven through the phase API (lm_begin, lm_linearize, lm_form_reduced, download, lm_solve_trial, lm_get_step, lm_decide,
get_params, lm_finish; get_transform for the affine).  Bars: error <= K eps_T scale with K from oracle/exact_cases.py (16 x the numpy
float64 model's own largest ratio, asserted in tests/test_exact_model_host.py); the solves are held by their backward error in the
device's OWN system against the a-priori bound of the factorisation that ran, as part (e) does.

SBA_MODE_POINTS_ONLY (k_nocam_step, the back substitution with dc = 0, the trial camera buffers copied at lm_begin), lambda0 = 1e-2:
  m9x40, g24x10, t5x30, d16x24+huber+fixed.  dc all zeros; the cameras after the accepted step bit-identical to the input (they are
  then read from the buffers lm_begin copied); dp per point against the exact -V'^-1 g_p (bar dp 256); the five trial scalars with
  their bars (176 / 153.6 / 16 / 16 / 592); the log row's step norm and optimality are sqrt(scalar 2) and scalar 4 exactly (the camera
  parts are exactly 0); fixed points bit-identical.
SBA_MODE_SHARED_INTR (build_tie_tables, k_tie_system, the tie / first arguments of every factorisation and of chol_epilogue_body,
chol_route(n_tied, n), the tied gradient of lm_finish), lambda0 = 1e-2, f, k1, k2 of every camera at their mean ("+shared"):
  case            n    n_tied  f64 route  f32 route     (oracle/exact_cases.chol_route, the mirror of chol_route in sba_chol_solve.hpp)
  d16x24+shared   176  131     BLOCKED    BLOCKED       k_cholesky_blocked, f32 lanes in the f32 engine
  g24x10+shared   264  195     LL         LL_F32        left-looking (its untied system takes BIG_DAG)
  v34x6+shared    374  275     BIG_DAG    BIG_DAG_F32   above 256 unknowns
  t18x12+shared   234  183     LL         LL_F32        13 parameters, a per-camera tail of four
  m9x40+shared    99   75      BLOCKED    BLOCKED       through the visibility mask
  report.reserved == 0 in every pass.  (i) the untied E against the exact S and rhs (bars S 15520, linear loss 352, rhs 2400);
  (ii) lm_get_step is T ds: f, k1, k2 bit-equal over the cameras, ds a backward-stable solution of A_s ds = rhs_s, A_s = T^T S_E T +
  lam diag(T^T diagU_E), rhs_s = T^T rhs_E formed in longdouble from the downloaded buffer, bar = solve_bound at n_tied + C eps64;
  (iii) the cameras after the accepted step are cams + T ds to one rounding, shared columns bit-equal; (iv) dp given the device's dc
  and the five scalars, existing bars; (v) m9x40+fscale, t18x12+fscale: the optimality of a solve stopped by gtol = 1e12 against
  max(|T^T g_c|, |g_p|) exact (bar gmax_tied 123.2); there the tied maximum (the shared k1) is 1.9 / 1.35 x the untied one.
SBA_MODE_CAMS_ONLY_SQ (k_sq_linearize<T,1>, k_reduce16, k_sq_pack_cams, k_sq_trial<T,1>), lambda0 = tau = 1e-3:
  edge11, edge13, m9x40 (9 .. 40 observations per camera), v34x6.  Diagonal blocks of E against the exact H_c over h_i h_j (6720),
  every other entry exactly 0, rhs = -g and the g_c slot = g (4960), the diagU slot exactly 1, the cost slot (624), lambda (read from
  the log row and the decision undone) against tau max diag H (416), dc a backward-stable solution of E + lam I on the route of n =
  C NCP, dc against the EXACT system by its residual (976), the accepted trial cost against the exact cost at cams + dc (2080), points
  bit-identical.  tau = 1e-3: lam / diag H runs from 1e-3 (the strongest parameter) to 3e2 .. 5e2 (the weakest): damping decides the
  step of the weak parameters and is negligible for the strong ones, and the first step is accepted on every case (gain 0.47 .. 0.93).
SBA_MODE_TRANSFORM_SQ (k_sq_linearize<T,2>, k_reduce16, k_sq_solve12, k_sq_trial<T,2>, the two theta buffers), tau = 1e-3:
  d16x24, m9x40, t5x30, b6x200 (1200 observations: two chunks of k_sq_linearize<T,2>, two partials for k_reduce16).  The 16 x 16 sums
  are not exposed: x = theta - identity of get_transform after the accepted step is held by its residual in the exact system,
  |(H + lam I) x + g|_i <= K eps_T (h_i sum_j h_j |x_j| + lam |x_i| + scale(g_i)) (272), the accepted trial cost and the report's cost
  against the exact cost at the device's theta (496), the report's initial cost (704), lambda (416); cameras and points bit-identical;
  a second lm_begin on the same handle (the buffer parity now flipped) gives the same theta and cost bit for bit.

Bars that rest on a number nobody had measured before this file: every sq_* bar (H, g, cost, lambda, the residual, the trial costs),
gmax_tied, and the C eps64 term of the tied solve; the points-only and shared trials reuse the bars of test_gpu_exact_model.py, which
hold the numpy model on the new cases with less than their usual factor 16 for dp (model: 38 points only, 16.04 shared; bar 256).

Observed on the MI355X, error / (eps_T * scale), to be read against the K above ([exact] lines of a run with -s):
  points only          T   dp     s0     s1     s2  s3        s4
  m9x40                f64 19     5.64   0      0   0.611     10.4
  m9x40                f32 14.7   1.88   1.79   0   1.14e-09  8.86
  g24x10               f64 7.12   8.18   0      0   0         11.2
  g24x10               f32 12.9   2.13   4.27   0   0         4.53
  t5x30                f64 19.2   6.58   0      0   0.872     0.663
  t5x30                f32 52.7   4.56   5.33   0   1.62e-09  2.14
  d16x24+huber+fixed   f64 32.5   2      0      0   0.552     1.26
  d16x24+huber+fixed   f32 34.2   3.05   2.08   0   1.03e-09  6.04
  shared intrinsics    T   S      rhs    ds_bwd / B  dp     s0      s1     s2  s3        s4
  d16x24+shared        f64 6.5    16.6   0.000164    3.07   0.267   0      0   0         15.6
  d16x24+shared        f32 8.09   11.7   0.000136    3.81   0.231   1.47   0   0         4.91
  g24x10+shared        f64 17.5   27.7   0.000612    3.81   0.189   0      0   0         16
  g24x10+shared        f32 8.67   17.9   8.31e-05    3.99   0.0212  1.34   0   0         1.62
  v34x6+shared         f64 15.7   52.7   0.000108    1.08   0.237   0      0   0.528     0.386
  v34x6+shared         f32 8.91   31.4   4.91e-05    3.33   0.145   1.16   0   9.84e-10  4.78
  t18x12+shared        f64 18.5   35.5   0.000145    0.762  0.384   0      0   0         7.99
  t18x12+shared        f32 5.1    35.9   0.00012     6.89   0.0568  0.612  0   0         4.38
  m9x40+shared         f64 4.14   18.6   0.000542    6.55   0.376   0      0   0.611     31.1
  m9x40+shared         f32 2.96   8.58   0.000416    8.08   0.138   0.28   0   1.14e-09  19.6
  gtol stop            T   gmax_tied  (the untied maximum instead: 1.4e15 / 2.6e6 / 9.5e14 / 1.8e6)
  m9x40+fscale         f64 3.02
  m9x40+fscale         f32 7.99
  t18x12+fscale        f64 4.87
  t18x12+fscale        f32 1.1
  cameras only, sq     T   H      g      cost   lam    res    tcost  dc_bwd / B  route
  edge11               f64 136    192    22.9   8.62   48.8   7.59   0.00272     BLOCKED
  edge11               f32 128    186    1.73   29.4   36     60.3   0.00206     BLOCKED, f32 lanes
  edge13               f64 240    283    37.6   10     36.3   0.966  0.00036     BLOCKED
  edge13               f32 215    253    16     74.2   30     94.9   0.00142     BLOCKED, f32 lanes
  m9x40                f64 354    219    20     15.1   45.3   3.78   0.0011      BLOCKED
  m9x40                f32 129    183    7.32   4.26   30.6   31.2   0.00042     BLOCKED, f32 lanes
  v34x6                f64 280    276    18.1   21.9   62.1   29.1   0.000121    BIG_DAG
  v34x6                f32 339    506    4.54   24.1   65.4   30.6   2.56e-05    BIG_DAG_F32
  affine, sq           T   cost   lam    res    tcost  report's cost
  d16x24               f64 29.9   22.7   0      11.5   10.4
  d16x24               f32 4.27   12.4   8.15   12     11.6
  m9x40                f64 20.8   16     0      7.43   6.29
  m9x40                f32 7.38   19.8   8.94   6.04   5.9
  t5x30                f64 4.78   24.3   0      6.07   5.2
  t5x30                f32 5.62   26.3   10.8   29.1   26.9
  b6x200               f64 45.9   20.7   0      37.5   38.4
  b6x200               f32 24.3   20.2   3.65   14.3   14.2
  report.reserved was 0 in every pass.  (affine, f64: theta is read back as identity + x with |x| ~ 2e-2 .. 5e-2, so half an ulp of theta
  is 20 .. 50 eps64 of x; the whole f64 residual lies inside that allowance, which is then the effective bar.)

A bug the first run of this file exposed: in the two squared variants sba_lm_solve_trial returned before k_trial_scalars, so the scalar
array the C ABI requires (a null one is SBA_ERR_INVALID) was never written and sba_lm_decide, which reads it, took a trial cost of 0
and accepted every step with gain cost / predicted.  solve_lm's own loop passes no array and was not affected.  Fixed in
Engine::lm_solve_trial (launch_sq_scalars); before: trial cost scalar 0 against 1.4e5 .. 3.7e7 exact; after: the tcost column above.
sba_lm_finish of the squared variants now also reports the f64 repeats (report.reserved), which it left unset.

Mutations, each built on a scratch copy (never committed) and run once against this file and against test_gpu_parity /
test_gpu_handle_reuse / test_gpu_wide / test_gpu_cholesky (187 older tests):
 (1) two entries of tie_first swapped (build_tie_tables): nothing fails, here or there.  tie_first is read in one place per kernel, the
     sum of x^2 over the system's unknowns for the xtol test (chol_epilogue_body, sba_chol_blocked.hpp:755, sba_chol_ll.hpp:164), and a
     sum does not see a permutation: an equivalent mutant.  A first entry pointing at the WRONG camera's column would move only
     |x| of the xtol stop, which one iteration does not read.
 (2) one `ib` term of k_tie_system dropped (S[f of camera 1, f of camera 2] from S_s[f, f]): (ii) fails on all five f64 cases (ds_bwd
     2.0e-4 / 5.8e-6 against B = 1e-13) and on the f32 cases d16x24, t18x12, m9x40 (2.0e-4 against 4.7e-5); g24x10 and v34x6 in f32 pass,
     as worked out on the host (0.08 of the f32 bar).  Of the older tests test_sharedcam_matches_reference fails (final cost 4 % high).
 (3) the factor 2 in f0 of k_sq_linearize turned into 1: all 16 squared-variant cases here fail (H at 6e6 eps32 / 3e15 eps64); of the
     older tests the two converged-cost tests of the variants in test_gpu_parity fail.
 (4) theta in k_sq_trial<T, 2> indexed without the `^ 1`: all 8 affine cases fail (trial cost at 2.9e6 x the bar: it is the cost at the
     identity); of the older tests test_transform_points_3d_squared_error_variant and two cases of
     test_squared_variants_between_full_solves fail.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from lasercalib_amd import _native  # noqa: E402
from oracle import exact_cases as xc  # noqa: E402
from test_gpu_exact_model import _configure, _need_gpu, _show  # noqa: E402,F401

DTYPES = ("f64", "f32")
_PASS = {}


def _used_lambda(row):
    """The damping of the trial the log row belongs to: the row holds it AFTER the decision (decide_core, sba_kernels.hpp:256-270:
    accepted: x max(1/3, 1 - (2 rho - 1)^3); rejected: x nu = 2 on a first trial)."""
    if row.accepted:
        t = 2.0 * row.rho - 1.0
        return row.lambda_ / max(1.0 / 3.0, 1.0 - t * t * t)
    return row.lambda_ / 2.0


def _iteration(name, dtype, mode, lambda0, twice=False):
    """One iteration of `mode` through the phase API on one handle (a second one after lm_finish when `twice`), cached."""
    key = (name, dtype, mode)
    if key in _PASS:
        return _PASS[key]
    import torch
    torch.cuda.set_device(0)
    c = xc.case(name)
    n = c.C * c.ncp
    runs = []
    with _native.Problem(c.cams, c.pts, c.uv, c.ci, c.pi, weights=c.w, dtype=dtype,
                         stream=torch.cuda.current_stream().cuda_stream) as prob:
        _configure(prob, c)
        for _ in range(2 if twice else 1):
            d = {}
            prob.lm_begin(prob.make_opts(ftol=1e-8, lambda0=lambda0, mode=mode))
            prob.lm_linearize()
            E = torch.zeros(prob.exchange_size(), dtype=torch.float64, device="cuda")
            prob.lm_form_reduced(E.data_ptr())
            torch.cuda.synchronize()
            Eh = E.cpu().numpy()
            d["E"] = Eh.copy()
            d["S"] = Eh[:n * n].reshape(n, n).copy()           # downloaded BEFORE lm_solve_trial, which may damp E in place
            d["rhs"] = Eh[n * n:n * n + n].copy()
            d["diagU"] = Eh[n * n + n:n * n + 2 * n].reshape(c.C, c.ncp).copy()
            d["gc"] = Eh[n * n + 2 * n:n * n + 3 * n].reshape(c.C, c.ncp).copy()
            d["cost"] = float(Eh[-1])
            sc = torch.zeros(8, dtype=torch.float64, device="cuda")
            scp = sc.data_ptr()
            prob.lm_solve_trial(E.data_ptr(), scp)
            torch.cuda.synchronize()
            d["scal"] = sc.cpu().numpy().copy()
            d["dc"] = prob.lm_get_step()
            d["status"], d["accepted"], d["row"] = prob.lm_decide(scp, 1)
            d["lam"] = _used_lambda(d["row"])
            d["cams_new"], d["pts_new"] = prob.get_params()
            d["dp"] = d["pts_new"] - c.pts
            d["upload"] = prob.upload_report()
            d["rep"] = prob.lm_finish()[2]
            d["reserved"] = int(d["rep"].reserved)
            if mode == _native.MODE_TRANSFORM_SQ:
                d["theta"] = prob.get_transform()
            runs.append(d)
    _PASS[key] = runs if twice else runs[0]
    return _PASS[key]


def _hold(R, keys, K=None, prefix=""):
    for k in keys:
        bar = (K or xc.K)[prefix + k]
        assert R[k] <= bar, (k, R[k], bar)


# ----------------------------------------------------------------------------- SBA_MODE_POINTS_ONLY
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", xc.POINTS_ONLY_CASES)
def test_points_only_iteration(name, dtype):
    c, eps = xc.case(name), xc.EPS[dtype]
    d = _iteration(name, dtype, _native.MODE_POINTS_ONLY, xc.LAMBDA0)
    assert d["accepted"] and d["reserved"] == 0
    assert d["dc"].shape == (c.C, c.ncp) and not np.any(d["dc"])
    assert np.array_equal(d["cams_new"], c.cams)             # read from the buffers lm_begin copied: the step flipped the parity
    if c.fixed is not None:
        assert np.array_equal(d["pts_new"][c.fixed], c.pts[c.fixed])
    assert np.any(d["dp"] != 0.0)
    R = xc.ratios(name, {k: d[k] for k in ("dc", "dp", "cams_new", "pts_new", "scal")}, eps, readback=True)
    _show("points_only", name, dtype, R)
    assert R["cond"] <= 1e3 and R["fixed_zero"]
    _hold(R, ("dp", "s_cost", "s_pred", "s_dx2", "s_x2", "s_gmax"))
    row, sc = d["row"], d["scal"]                             # the camera parts of the step norm and of max |g| are exactly 0
    assert row.step_norm == np.sqrt(sc[2]) and row.optimality == sc[4] and row.cost == sc[0]


# ----------------------------------------------------------------------------- SBA_MODE_SHARED_INTR
_SHARED_ROUTES = {"d16x24+shared": ("BLOCKED", "BLOCKED"), "g24x10+shared": ("LL", "LL_F32"), "v34x6+shared": ("BIG_DAG", "BIG_DAG_F32"),
                  "t18x12+shared": ("LL", "LL_F32"), "m9x40+shared": ("BLOCKED", "BLOCKED")}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", xc.SHARED_CASES)
def test_shared_intrinsics_iteration(name, dtype):
    c, eps = xc.case(name), xc.EPS[dtype]
    assert np.all(c.cams[:, 6:9] == c.cams[0, 6:9])
    d = _iteration(name, dtype, _native.MODE_SHARED_INTR, xc.LAMBDA0)
    B, what, route = xc.tied_solve_bound(dtype, name)
    assert route == _SHARED_ROUTES[name][DTYPES.index(dtype)], route
    if name == "g24x10+shared":
        assert xc.chol_route(dtype, c.C * c.ncp).startswith("BIG_DAG")      # the untied system of the same rig goes elsewhere
    assert what == ("f64 refined" if dtype == "f64" else "f32 lanes") and d["reserved"] == 0
    # (i) the untied system in the exchange buffer
    S, rhs = d["S"], d["rhs"]
    assert np.array_equal(S, S.T)
    R = xc.ratios(name, dict(S=S, rhs=rhs), eps)
    _hold(R, ("S", "rhs"))
    assert R["S"] <= xc.K["S_lin"]
    # (ii) the step is T ds, ds a backward-stable solution of the tied system formed from the downloaded buffer
    dc = d["dc"]
    T = xc.tied(name).T
    assert np.all(np.isfinite(dc)) and np.any(dc != 0.0)
    assert np.all(dc[:, 6:9] == dc[0, 6:9])
    ds, bwd, own = xc.tied_backward_error(name, S, rhs, d["diagU"], dc)
    assert ds.size == 3 + (c.ncp - 3) * c.C and np.array_equal((T @ ds).reshape(c.C, c.ncp), dc)
    print(f"\n[exact] tied_solve {name} {dtype} n_tied={ds.size} n={c.C * c.ncp} {route} {what}: ds_bwd={bwd:.3g} B={B:.3g} "
          f"fraction={bwd / B:.3g} host={own / B:.2g}")
    assert own <= 0.01 * B
    assert bwd <= B, (bwd, B)
    # (iii) the accepted cameras
    assert d["accepted"]
    assert np.all(np.abs(d["cams_new"] - (c.cams + dc)) <= np.spacing(np.abs(c.cams + dc)))
    assert np.all(d["cams_new"][:, 6:9] == d["cams_new"][0, 6:9])
    # (iv) the point step given the device's dc, and the trial scalars
    R2 = xc.ratios(name, {k: d[k] for k in ("dc", "dp", "cams_new", "pts_new", "scal")}, eps, readback=True)
    R.update(R2, ds_bwd_over_B=bwd / B)
    _show("shared", name, dtype, R)
    assert R2["cond"] <= 1e3
    _hold(R2, ("dp", "s_cost", "s_pred", "s_dx2", "s_x2", "s_gmax"))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", xc.SHARED_GTOL_CASES)
def test_shared_intrinsics_optimality_of_a_gtol_stop(name, dtype):
    """(v) sba_lm_finish's gradient in the tied unknowns: max(|T^T g_c|, |g_p|), not the untied maximum."""
    c, eps = xc.case(name), xc.EPS[dtype]
    with _native.Problem(c.cams, c.pts, c.uv, c.ci, c.pi, weights=c.w, dtype=dtype) as prob:
        cams, pts, rep, _ = prob.solve_lm(prob.make_opts(gtol=1e12, mode=_native.MODE_SHARED_INTR))
    assert rep.status == 1 and rep.nfev == 1 and np.array_equal(cams, c.cams) and np.array_equal(pts, c.pts)
    E, Td = xc.exact(name), xc.tied(name)
    tied_max, untied_max = max(np.max(np.abs(Td.g)), np.max(np.abs(E.gp))), max(np.max(np.abs(E.gc)), np.max(np.abs(E.gp)))
    R = xc.ratios(name, dict(gmax_tied=rep.optimality, gmax=rep.optimality), eps)
    _show("shared_gtol", name, dtype, dict(gmax_tied=R["gmax_tied"], against_untied=R["gmax"], tied_over_untied=tied_max / untied_max))
    assert tied_max > 1.3 * untied_max and R["gmax"] > 1e3 * xc.K["gmax"]       # the untied maximum would miss the bar by far
    _hold(R, ("gmax_tied",))


# ----------------------------------------------------------------------------- SBA_MODE_CAMS_ONLY_SQ
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", xc.SQ_CAMS_CASES)
def test_cams_only_squared_iteration(name, dtype):
    c, eps = xc.case(name), xc.EPS[dtype]
    n, P = c.C * c.ncp, c.ncp
    d = _iteration(name, dtype, _native.MODE_CAMS_ONLY_SQ, xc.SQ_TAU)
    S = d["S"]
    blocks = np.kron(np.eye(c.C), np.ones((P, P))) > 0
    assert not np.any(S[~blocks]) and np.array_equal(S, S.T)
    H = np.stack([S[k * P:(k + 1) * P, k * P:(k + 1) * P] for k in range(c.C)])
    assert np.array_equal(d["rhs"], -d["gc"].ravel()) and np.all(d["diagU"] == 1.0)
    q = dict(H=H, g=d["gc"], cost=d["cost"], lam=d["lam"], x=d["dc"], tcost=d["scal"][0])
    R = xc.sq_ratios(name, "cams", q, eps)
    assert d["accepted"] and d["row"].cost == d["scal"][0] < d["cost"] and not np.any(d["scal"][1:])
    B, what = xc.device_solve_bound(dtype, n)
    R["dc_bwd"], own = xc.backward_error(S, d["rhs"], np.full(n, d["lam"]), d["dc"])
    R["dc_bwd_over_B"] = R["dc_bwd"] / B
    _show("sq_cams", name, dtype, R)
    print(f"[exact] sq_cams_solve {name} {dtype} n={n} {xc.chol_route(dtype, n)} {what} B={B:.3g} host={own / B:.2g} reserved={d['reserved']} "
          f"lam={d['lam']:.6g} gain={d['row'].rho:.3g} exact_gain={R['gain_exact']:.3g}")
    assert d["reserved"] == 0
    assert np.all(np.isfinite(d["dc"])) and np.any(d["dc"] != 0.0)
    _hold(R, ("H", "g", "cost", "lam", "res", "tcost"), prefix="sq_cams_")
    assert own <= 0.01 * B and R["dc_bwd"] <= B + 4 * xc.EPS["f64"], (R["dc_bwd"], B)      # (4 eps64: lam with the decision undone)
    assert np.array_equal(d["pts_new"], c.pts)
    assert np.all(np.abs(d["cams_new"] - (c.cams + d["dc"])) <= np.spacing(np.abs(c.cams + d["dc"])))
    if name == "m9x40":                                       # k_reduce16's strided loop sees cameras of unequal observation counts
        assert len(set(np.bincount(c.ci, minlength=c.C).tolist())) > 3


# ----------------------------------------------------------------------------- SBA_MODE_TRANSFORM_SQ
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", xc.SQ_AFFINE_CASES)
def test_affine_squared_iteration(name, dtype):
    c, eps = xc.case(name), xc.EPS[dtype]
    if name == "b6x200":
        assert c.M > 1024                                     # more than one chunk of k_sq_linearize<T, 2>
    first, second = _iteration(name, dtype, _native.MODE_TRANSFORM_SQ, xc.SQ_TAU, twice=True)
    d = first
    assert d["accepted"] and d["status"] < 0
    assert np.array_equal(d["cams_new"], c.cams) and np.array_equal(d["pts_new"], c.pts)
    theta = d["theta"]
    assert np.all(np.isfinite(theta)) and np.any(theta != xc.IDENT12)
    R = xc.sq_ratios(name, "affine", dict(cost=d["rep"].initial_cost, lam=d["lam"], theta=theta, tcost=d["scal"][0]), eps)
    assert d["row"].cost == d["scal"][0] < d["rep"].initial_cost and not np.any(d["scal"][1:])
    R["fcost"] = xc.sq_ratios(name, "affine", dict(theta=theta, tcost=d["rep"].cost), eps)["tcost"]
    _show("sq_affine", name, dtype, R)
    print(f"[exact] sq_affine_step {name} {dtype} lam={d['lam']:.6g} gain={d['row'].rho:.3g} exact_gain={R['gain_exact']:.3g} |x|={np.linalg.norm(theta - xc.IDENT12):.3g}")
    _hold(R, ("cost", "lam", "res", "tcost"), prefix="sq_affine_")
    assert R["fcost"] <= xc.K["sq_affine_tcost"]
    # a second lm_begin on the same handle starts from the identity again, on the other parity of the theta and parameter buffers
    assert np.array_equal(second["theta"], theta)
    assert second["scal"][0] == d["scal"][0] and second["row"].cost == d["row"].cost and second["rep"].cost == d["rep"].cost and second["rep"].initial_cost == d["rep"].initial_cost
    assert second["accepted"] and np.array_equal(second["cams_new"], c.cams) and np.array_equal(second["pts_new"], c.pts)
