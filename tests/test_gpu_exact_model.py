"""The device's model derivatives, gradient, reduced camera system, camera step and point step against the exact reference
(oracle/exact_model.py).

The exact reference evaluates the camera model from its definition in mpmath and differentiates it far below float64
resolution; tests/test_exact_model_host.py pins it.  Here the f32 and the f64 engine are held to it on small rigs, default
routing (no SBA_* knob) except in the last test, all inputs rounded to float32 so that both engines and the reference see the
same numbers.
Compared: (a) the materialised blocks per column kind, (b) diagU / g_c / cost of the exchange buffer and get_gradient()'s
g_p after one linearisation, and both gradients, the cost and the report's optimality of a solve stopped by gtol, (c) the
point step of one accepted iteration given the device's own dc, per point, and the five trial scalars, (d) every entry of
the reduced system S and of its right-hand side in the exchange buffer against the exact S = blockdiag(U) - sum W V'^-1 W^T
and rhs = -g_c + sum W V'^-1 g_p over the free points (V' damped, S not), S bitwise symmetric and zero between cameras
without a common free point, (e) dc as a backward-stable solution of the device's OWN system: |A dc - rhs|_i <= B d_i sum_j
d_j |dc_j| with A = S_E + lam diag(D) from the downloaded buffer, and no f64 repeat of a refused f32 factorisation.  No
dense solve is compared with dc anywhere: neither the bar of (d) nor that of (e) depends on the conditioning of S (raw
condition numbers 4e8 .. 2e9 on these cases, diagonal over nine decades).

Cases (oracle/exact_cases.py), with the kernels their default route runs (plan_route and the back substitution's dispatch in
sba_engine.hpp; "bs LW" = k_backsub_dense<T, LW>, points per chunk 16 / 12 / 8 / 4 for LW 16 / 0 (packed) / 32 / 64):
  d16x24   16 x 24 dense, 384 obs     f32 k_schur_fused_bf3, f64 k_schur_fused_f64; bs LW 16, 2 chunks (16 + 8 points)
  m9x40    9 x 40 at 0.6, 217 obs     the same two fused kernels through the visibility mask; bs LW 16 masked, 3 chunks
  w18x15   18 x 15 at 0.9, 252 obs    f32 k_schur_fused_wide (3 points per producer wave), f64 k_schur_fused_wide_f64;
                                      bs LW 0 (three points per wave, packed), 2 chunks (12 + 3 points)
  g24x10   24 x 10 at 0.8, 200 obs    two camera groups, group pairs: f32 k_schur_diag_bf3 / k_schur_offdiag_bf3 (U and g_c folded
                                      into the diagonal pairs), f64 k_schur_sym pairs + k_linearize_cams; k_linearize_points_wave<T, 32>;
                                      bs LW 32, 2 chunks (8 + 2 points)
  v34x6    34 x 6 dense, 204 obs      three groups (16, 16, 2): the same pair kernels, PARTIAL last group; k_linearize_points_wave<T, 64>;
                                      bs LW 64 (a point per wave, two cameras per lane up to 34), 2 chunks (4 + 2 points)
  t5x30    13 parameters, 5 x 30 at 0.8, 123 obs    f32 k_schur_fused_wide with the mask, f64 k_schur_sym with the point
                                      linearisation inside (LIN) + k_linearize_cams; bs LW 16 masked, 2 chunks
  t16x12   13 parameters, 16 x 12 dense, 192 obs    f32 k_schur_fused_wide (208 rows = 13 tiles exactly), f64 k_schur_sym LIN; bs LW 16, 1 partial chunk
  t18x12   13 parameters, 18 x 12 dense, 216 obs    f32 k_schur_fused_wide (15 row tiles: 2 points per producer wave), f64 group pairs
                                      (k_linearize_points, k_linearize_cams, k_schur_sym); bs LW 0 packed, 1 chunk
  edge11 / edge13   6 x 20 dense, 120 obs, weights 0.5 .. 1.5: rho = 0; |rho|^2 = 0.98e-4 and 1.02e-4 (either side of the series
                                      switch); |rho| = 3.1; an ordinary camera; a camera with k1 = -0.3, k2 = 0.1 and points out to
                                      n ~ 0.5; point 0 on camera 0's optical axis (x = y = 0).  Routes as d16x24 (11) / t16x12 (13).
  d16x24+huber, w18x15+huber          Huber, f_scale = 1, a dozen pixels displaced by 40 px (both branches taken, asserted on the
  d16x24+fixed, w18x15+fixed          exact residuals); every fifth point fixed (comes back bit-identical); both at once on d16x24.
  d16x24+huber+fixed                  These five enter (c) only.
The gtol stop takes its gradient from the plain kernels on every route (k_linearize_points / k_linearize_points_wave and
k_linearize_cams at the returned point, sba_lm_finish), the exchange buffer from the route's own fused or pair kernels: (b)
pins both.  Every route leaves g_p in plain form after lm_form_reduced (the fused kernels write it for the back substitution), so (b)
compares it on every case.  One deliberate narrowing sits in (c): the per-point factor L^-1 of V' and L^-1 g_p is evaluated in
double and STORED in the engine's dtype (point_factor_one, sba_kernels.hpp: `o[k] = (T)li[k]`), and the f32 engine forms
W^T dc in f32; both are held with eps32 like the rest of the f32 engine.

Bars: error <= K * eps_T * scale, the scale from exact values (oracle/exact_cases.py header), K = 16 x the numpy float64
model's own largest ratio on these cases in eps64 (asserted in tests/test_exact_model_host.py), never below 16:
  blocks 176   diagU 352   g_c 8800   g_p 5120   cost 208   max|g| 368   dp 256
  trial scalars: 0 cost 176   1 predicted reduction 153.6   2 |dp|^2 16   3 |X|^2 16   4 max|g_p| 592
(g_c and g_p: the residual is a cancelled difference of ~1e3 px values and carries ~1e2 eps of itself; the model shows the
same.)  r keeps the project's bars: 1e-9 px in f64, the a-priori 4 eps32 w (|uv| + f cond^2) per row in f32 (observed: at
most 5.3e-13 px, and 0.12 of the bound).  The cx and cy columns equal w and 0 exactly.
  (d)  S 15520 over d_i d_j, d = sqrt(diag U) exact (Cauchy-Schwarz: no term sum of S exceeds it); on the twelve cases with
       the linear loss also S 352 (the model's 968 eps64 comes from the Huber cases alone: a row is scaled by z^-1/4 and a
       residual of 1 .. 3 px carries 1e2 .. 1e3 eps of itself; its largest ratio with the linear loss is 21.5);
       rhs 2400 over g_c's scale + sum |W| |V'^-1| (g_p's scale).  The ratio over the term-magnitude matrix sum |Jc_i||Jc_j|
       + sum |W||V'^-1||W^T| is printed (S_terms) and asserts nothing.
  (e)  B is a-priori (oracle/exact_cases.solve_bound, device_solve_bound): Higham, Accuracy and Stability of Numerical
       Algorithms, Thm 10.3 / 10.4 with |L||L^T|_ij <= d_i d_j / (1 - gamma_(n+1)): (3n + 2) eps / (1 - (3n + 2) eps), eps of
       the factorisation that ran (known from the route, and report.reserved == 0 is asserted), plus 2 delta of the pivots'
       reciprocal square root -- 4e-15 refined (rsqrt_nr, sba_chol_blocked.hpp:40-46), one ulp of v_rsq_f32 on f32 lanes
       (sba_chol_blocked.hpp:178), 5e-8 where the fp32 engine factors in f64 with the estimate alone (sba_chol_blocked.hpp:
       647-651, sba_chol_ll.hpp:85) -- plus eps32 where S and rhs are narrowed to f32.  n = 65 .. 374: B = 197 .. 1124 eps64,
       201 .. 1128 eps32, and 1e-7 for the unrefined f64 pivots.  The host's longdouble evaluation of the residual is asserted
       below 1 % of B (observed: at most 5e-5 of it).

Observed on the MI355X, error / (eps_T * scale), to be read against the K above (s0 .. s4 = the trial scalars):
  case                T    blocks  diagU  g_c   g_p   cost   gtol g_c  g_p   max|g|  dp    s0       s1     s2  s3        s4     S      rhs    dc_bwd / B
  edge11              f64  10.3    13.6   136   155   5.67   137       154   15.3    7.33  0.413    0      0   0.599     17.9   10.1   18.9   0.000967
  edge11              f32  2.66    2.12   46.9  127   6.86   46.8      127   9.47    11.4  0.45     8      0   1.12e-09  26.5   1.8    7.79   0.000851
  edge13              f64  9.35    11.3   148   232   31.4   148       232   23.7    10.5  0.0988   0      0   0         34.5   12.8   27.9   0.0008
  edge13              f32  1.86    2.02   90.4  196   1.18   90.3      197   14.9    9.67  0.58     6.78   0   0         6.96   2.07   15     0.000506
  m9x40               f64  3.39    9.81   216   377   10     217       377   10.3    8.9   0.128    0      0   0.611     10.4   4.86   14.6   0.000203
  m9x40               f32  2.27    4.92   56.8  214   2.55   55.5      214   3.63    8.39  0.133    2.05   0   1.14e-09  9.48   3.93   12.5   0.000386
  t5x30               f64  2.45    3.46   100   169   3.87   100       169   7.01    11.2  0.167    0      0   0.872     0.663  2.86   12.4   0.000408
  t5x30               f32  4.6     5.46   28.9  149   8.41   29        149   7.43    26.8  0.118    3.3    0   1.62e-09  2.89   2.95   6.24   0.000977
  d16x24              f64  -       6.96   75.7  39.7  8.62   77.5      39.2  3.99    4.01  0.0893   0      0   0         14.8   5.99   19.5   0.000322
  d16x24              f32  -       9.7    91.4  32.8  0.906  91.1      32.8  2.96    6.16  0.0455   0.445  0   0         1.69   8.89   16.1   0.00017
  w18x15              f64  -       9.45   136   42.3  2.87   136       41.9  5.03    1.42  0.114    0      0   0         10.1   8.51   34     0.000281
  w18x15              f32  -       10.1   188   21.5  3.82   187       21.2  10.9    5.01  0.213    2.39   0   0         6.17   8.42   32.3   0.000173
  g24x10              f64  -       19.6   158   48.3  15.3   158       48.3  13.7    2.27  0.0519   0      0   0         11.2   18.7   33.2   0.000109
  g24x10              f32  -       9.53   152   36.7  4.88   151       36.7  7.52    5.97  0.0449   4.56   0   0         4.53   8.54   34.7   6.27e-05
  v34x6               f64  -       20     185   19.7  9.47   185       19.7  44.3    1.15  0.0302   0      0   0.528     3.99   18.8   42.1   5.58e-05
  v34x6               f32  -       8.64   179   23.3  3.09   180       23.3  13.8    4.81  0.0267   0.781  0   9.84e-10  3.37   7.8    39.2   3.25e-05
  t16x12              f64  -       10.3   109   31.6  2.88   109       31.6  2.16    2.1   0.00352  0      0   0         13.7   9.39   31     0.000259
  t16x12              f32  -       6.72   121   16.4  6.74   121       16.2  15.4    4.02  0.00546  0.292  0   0         4.01   5.61   35.5   0.00012
  t18x12              f64  -       19.7   146   45    0      146       45    18.7    2.1   0.194    0      0   0         20.2   17.9   37.2   6.21e-05
  t18x12              f32  -       6.41   148   50.3  1.66   149       50.1  14      6.96  0.178    1.49   0   0         11.9   5.8    36.5   0.000106
  d16x24+huber        f64  -       -      -     -     -      -         -     -       4.26  0.624    0      0   0         0.628  83.8   40.4   0.000119
  d16x24+huber        f32  -       -      -     -     -      -         -     -       9.49  0.952    3.84   0   0         6.08   75.1   16.2   0.000103
  d16x24+fixed        f64  -       -      -     -     -      -         -     -       3.12  0.179    0      0   0.552     14.8   5.81   21.5   0.000102
  d16x24+fixed        f32  -       -      -     -     -      -         -     -       5.08  0.191    1.39   0   1.03e-09  1.69   8.83   25.7   0.0001
  d16x24+huber+fixed  f64  -       -      -     -     -      -         -     -       2.73  2.5      0      0   0.552     0.628  92.3   50.7   0.00013
  d16x24+huber+fixed  f32  -       -      -     -     -      -         -     -       5.83  9.2      2.82   0   1.03e-09  6.08   178    35.5   6.07e-05
  w18x15+huber        f64  -       -      -     -     -      -         -     -       6.18  2.82     0      0   0         1.72   202    29.5   7.53e-05
  w18x15+huber        f32  -       -      -     -     -      -         -     -       6.73  1.46     3.41   0   0         7.35   185    39.7   9.25e-05
  w18x15+fixed        f64  -       -      -     -     -      -         -     -       2.05  0.0224   0      0   0         10.1   8.55   38     0.000148
  w18x15+fixed        f32  -       -      -     -     -      -         -     -       4.79  0.0115   3.54   0   0         6.17   9.1    71.9   0.000113

  Largest per quantity, f64 / f32:  blocks 10.3 / 4.6   diagU 20 / 10.1   g_c 217 / 188   g_p 377 / 214   cost 31.4 / 8.4
  max|g| 44.3 / 15.4   dp 11.2 / 26.8   s0 2.82 / 9.2   s1 0 / 8   s2 0 / 0   s3 0.87 / 2e-9   s4 34.5 / 26.5.
  (s1 and s2 are formed from the read-back step: in f64 their whole difference lies inside the read-back allowance.)
  S 202 / 185 (linear loss: 18.8 / 9.1; over the term magnitudes 348 / 328)   rhs 50.7 / 71.9   dc_bwd / B 9.7e-4 / 9.8e-4:
  the solves sit three decades under the a-priori bound (at most 0.23 eps64 and 0.2 eps32): d_i sum_j d_j |dc_j| adds up without
  the cancellation that A dc has.  What the bar of (e) does see is worked out on the host (tests/test_exact_model_host.py).
  The factorisations the default route of these sizes does not take (last test; dc_bwd / B, f64 / f32 engine):
    SBA_CHOL=ll            d16x24 3.2e-4 / 5.7e-3   m9x40 3.9e-4 / 5.3e-3     k_cholesky_ll (f32 engine: f64, unrefined pivots, B = 1e-7)
    SBA_CHOL=blocked       w18x15 2.6e-4 / 3.5e-4   t16x12 1.4e-4 / 1.9e-4   k_cholesky_stream (f64 in both engines)
    SBA_CHOL_BIG=launches  g24x10 1.6e-4 / 2.0e-4   v34x6 1.3e-4 / 1.2e-4     k_chol_big_prepare / k_chol_big_step (f64 in both)
    SBA_CHOL_F32=0         d16x24 f32 5.7e-3                                  k_cholesky_blocked, f64 with unrefined pivots
  report.reserved was 0 in every pass.

Mutations on a scratch copy (numeric only, never committed): (i) the k2 column of obs_resjac x 1.001 fails (a) on every
case in both dtypes (k2 at 8.4e3 eps32 / 4.5e12 eps64), diagU in all 20 cases of (b) and g_c of the gtol stop; (ii)
`gxx += 6 tp2 x` -> `2 tp2 x` in obs_jp_jvp only fails (c) on the four 13-parameter cases in both dtypes (dp at 370 .. 2100
eps32) and nothing in (a), and no test from before this file; (iii) robust_apply_jvp leaving s[k] unscaled fails (c) on the
three Huber cases in both dtypes and nothing in (a).
Mutations for (d) and (e), each built on a scratch copy and run against this file and, of the older files, against
test_gpu_parity / test_gpu_wide / test_gpu_large_cams ((iv) .. (vi)) or test_gpu_cholesky / test_gpu_chol_image ((vii)) only:
(iv) the m m' product dropped from k_schur_fused_bf3's consumers is NOT caught: all 151 tests here and all 107 older ones pass.
S of the three f32 cases on that kernel moves from 8.9 / 3.9 / 1.8 to 14.1 / 27.2 / 21.1 eps32 d_i d_j (d16x24 / m9x40 /
edge11), under the 352 the numpy model's own error allows; no bar derived from that model can see a product of 2^-16 of a
term.  (v) R and Tc swapped in the parameter-major branch of k_build_exchange fails (d) on all eight f32 cases of that branch
(fused bf3 and the bf3 group pairs), (e) on the same eight and on five f32 knob passes (the matrix is no longer the one that
was factored: refusals and repeats), and (c) on the same eight; 23 older tests fail too, converged solves and
kernel-against-kernel comparisons in f32.  (vi) lam D_p left out of V' in k_schur_fused_bf3's producer fails (d) on its six
f32 cases (S at 1.8e4 .. 1e5 eps32, rhs at 1.4e4 .. 3e4) and (c) on the same six (the point factor is shared); of the
older tests only the four f32 cases of test_dense_kernels_match_general_kernels fail.  (vii) the trailing update of block
(3, 2) of the first block column skipped in cholb_core<float> fails (e) on all thirteen f32 cases up to 256 unknowns, through
report.reserved: the f32 factorisation is refused and the f64 repeat gives a step that meets B; of the older tests the six
f32-lane cases of test_gpu_cholesky fail (they count repeats too).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from lasercalib_amd import _native  # noqa: E402
from oracle import exact_cases as xc  # noqa: E402

DTYPES = ("f64", "f32")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert _native.device_count() > 0, "no HIP device visible: GPU tests must run on the MI355X box"


def _configure(prob, c):
    if c.fixed is not None:
        prob.set_fixed_points(c.fixed)
    if c.loss != "linear":
        prob.set_robust_loss(c.loss, c.f_scale)


_DEVICE = {}


def _device(name, dtype):
    """Everything the tests of one (case, dtype) compare, from ONE pass over the device: the materialised blocks, one LM
    iteration through the phase API at lambda0 = 1e-2, and a solve stopped by gtol = 1e12 on a fresh handle."""
    if (name, dtype) in _DEVICE:
        return _DEVICE[name, dtype]
    import torch
    torch.cuda.set_device(0)
    c = xc.case(name)
    n = c.C * c.ncp
    d = {}
    with _native.Problem(c.cams, c.pts, c.uv, c.ci, c.pi, weights=c.w, dtype=dtype,
                         stream=torch.cuda.current_stream().cuda_stream) as prob:
        _configure(prob, c)
        if name in xc.BLOCK_CASES:
            d["r"], d["Jc"], d["Jp"] = prob.residual_jacobian()
        prob.lm_begin(prob.make_opts(ftol=1e-8, lambda0=xc.LAMBDA0))
        prob.lm_linearize()
        E = torch.zeros(prob.exchange_size(), dtype=torch.float64, device="cuda")
        prob.lm_form_reduced(E.data_ptr())
        torch.cuda.synchronize()
        Eh = E.cpu().numpy()
        assert Eh.size == n * n + 3 * n + 1
        d["S"] = Eh[:n * n].reshape(n, n).copy()           # downloaded BEFORE lm_solve_trial, which may damp E in place
        d["rhs"] = Eh[n * n:n * n + n].copy()
        d["diagU"] = Eh[n * n + n:n * n + 2 * n].reshape(c.C, c.ncp).copy()
        d["gc"] = Eh[n * n + 2 * n:n * n + 3 * n].reshape(c.C, c.ncp).copy()
        d["cost"] = float(Eh[-1])
        _, d["gp"] = prob.get_gradient()
        sc = torch.zeros(8, dtype=torch.float64, device="cuda")
        prob.lm_solve_trial(E.data_ptr(), sc.data_ptr())
        torch.cuda.synchronize()
        d["scal"] = sc.cpu().numpy().copy()
        d["dc"] = prob.lm_get_step()
        d["status"], d["accepted"], row = prob.lm_decide(sc.data_ptr(), 1)
        d["cams_new"], d["pts_new"] = prob.get_params()
        d["dp"] = d["pts_new"] - c.pts
        d["upload"] = prob.upload_report()
        d["reserved"] = int(prob.lm_finish()[2].reserved)  # f64 repeats of a refused f32 factorisation
    with _native.Problem(c.cams, c.pts, c.uv, c.ci, c.pi, weights=c.w, dtype=dtype) as prob:
        _configure(prob, c)
        cams, pts, rep, _ = prob.solve_lm(prob.make_opts(gtol=1e12))
        g_gc, g_gp = prob.get_gradient()
        d["gtol"] = dict(status=rep.status, nfev=rep.nfev, moved=not (np.array_equal(cams, c.cams) and np.array_equal(pts, c.pts)),
                         gc=g_gc, gp=g_gp, optimality=rep.optimality, cost=rep.cost)
    _DEVICE[name, dtype] = d
    return d


def _show(tag, name, dtype, R):
    print(f"\n[exact] {tag} {name} {dtype} " + " ".join(f"{k}={float(v):.3g}" for k, v in R.items() if np.isscalar(v) and not isinstance(v, bool)))


# ----------------------------------------------------------------------------- (a) blocks
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", xc.BLOCK_CASES)
def test_blocks_per_column_kind(name, dtype):
    """k_resjac<T>: every column of Jc and of Jp against the exact one, relative to that column kind's largest exact entry."""
    c, d, eps = xc.case(name), _device(name, dtype), xc.EPS[dtype]
    R = xc.ratios(name, dict(r=d["r"], Jc=d["Jc"], Jp=d["Jp"]), eps)
    _show("blocks", name, dtype, R)
    print("[exact] kinds", name, dtype, {k: round(float(v), 2) for k, v in R["blocks_by_kind"].items()})
    if dtype == "f64":
        assert R["r_abs"] <= 1e-9                         # px, the project's fp64 bar
    else:
        assert R["r"] <= 1.0                              # the a-priori per-row bound 4 eps32 w (|uv| + f cond^2)
    for kind, v in R["blocks_by_kind"].items():
        assert v <= xc.K["blocks"], (kind, v)
    cx, cy = c.ncp - 2, c.ncp - 1
    zero = np.zeros(c.M)
    assert np.array_equal(d["Jc"][:, 0, cx], c.w) and np.array_equal(d["Jc"][:, 1, cy], c.w)
    assert np.array_equal(d["Jc"][:, 1, cx], zero) and np.array_equal(d["Jc"][:, 0, cy], zero)


# ----------------------------------------------------------------------------- (b) sums of the linearisation
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", xc.BASE_CASES)
def test_linearisation_sums(name, dtype):
    """diagU, g_c and the cost of the exchange buffer and get_gradient()'s g_p after lm_linearize + lm_form_reduced."""
    d, eps = _device(name, dtype), xc.EPS[dtype]
    R = xc.ratios(name, {k: d[k] for k in ("diagU", "gc", "gp", "cost")}, eps)
    _show("sums", name, dtype, R)
    for k in ("diagU", "gc", "gp", "cost"):
        assert R[k] <= xc.K[k], (k, R[k], xc.K[k])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", xc.BASE_CASES)
def test_gradient_and_optimality_of_a_gtol_stop(name, dtype):
    """A solve stopped by gtol = 1e12 (status 1, nothing moved): get_gradient() both parts, the report's optimality = max |g|
    and its cost."""
    d, eps = _device(name, dtype), xc.EPS[dtype]
    g = d["gtol"]
    assert g["status"] == 1 and g["nfev"] == 1 and not g["moved"]
    R = xc.ratios(name, dict(gc=g["gc"], gp=g["gp"], cost=g["cost"], gmax=g["optimality"]), eps)
    _show("gtol", name, dtype, R)
    for k in ("gc", "gp", "cost", "gmax"):
        assert R[k] <= xc.K[k], (k, R[k], xc.K[k])


# ----------------------------------------------------------------------------- (c) point step and trial scalars
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", xc.ALL_CASES)
def test_point_step_and_trial_scalars(name, dtype):
    """One accepted iteration: the cameras move by the device's own dc; the point step read back as points_new - points_old
    is the exact damped 3 x 3 solve GIVEN that dc, per point; the five trial scalars are the exact sums."""
    c, d, eps = xc.case(name), _device(name, dtype), xc.EPS[dtype]
    assert d["accepted"], "the case must be one whose first step the LM control accepts"
    assert np.all(np.abs(d["cams_new"] - (c.cams + d["dc"])) <= np.spacing(np.abs(c.cams + d["dc"])))
    if c.fixed is not None:
        assert np.array_equal(d["pts_new"][c.fixed], c.pts[c.fixed])             # fixed points come back bit-identical
    R = xc.ratios(name, {k: d[k] for k in ("dc", "dp", "cams_new", "pts_new", "scal")}, eps, readback=True)
    _show("step", name, dtype, R)
    print("[exact] upload", name, dtype, {k: d["upload"][k] for k in ("route", "dense", "masked", "group_indexed")})
    assert R["cond"] <= 1e3 and R["fixed_zero"]
    for k in ("dp", "s_cost", "s_pred", "s_dx2", "s_x2", "s_gmax"):
        assert R[k] <= xc.K[k], (k, R[k], xc.K[k])
    if "huber" in name:                                   # both branches of the loss are taken (on the exact residuals)
        z = (xc.exact(name).r / c.f_scale) ** 2
        assert np.sum(z > 1.0) >= 12 and np.sum(z <= 1.0) >= 12


# ----------------------------------------------------------------------------- (d) the reduced camera system, entry by entry
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", xc.ALL_CASES)
def test_reduced_system_entries(name, dtype):
    """S and rhs of the exchange buffer after lm_form_reduced against the exact ones (oracle/exact_model.reduced_system), every
    entry over d_i d_j resp. the term magnitudes of rhs; S bitwise symmetric; cameras without a common free point: a zero block."""
    c, d, eps = xc.case(name), _device(name, dtype), xc.EPS[dtype]
    S, rhs = d["S"], d["rhs"]
    assert np.array_equal(S, S.T)
    X = xc.reduced(name)
    for a in range(c.C):
        for b in range(c.C):
            if not X.share[a, b]:
                assert not np.any(S[a * c.ncp:(a + 1) * c.ncp, b * c.ncp:(b + 1) * c.ncp]), (a, b)       # +-0 passes
    R = xc.ratios(name, dict(S=S, rhs=rhs), eps)
    _show("reduced", name, dtype, R)                      # S_terms: the same error over the term-magnitude matrix, information only
    assert R["S"] <= xc.K["S"], (R["S"], xc.K["S"])
    if c.loss == "linear":
        assert R["S"] <= xc.K["S_lin"], (R["S"], xc.K["S_lin"])
    assert R["rhs"] <= xc.K["rhs"], (R["rhs"], xc.K["rhs"])


# ----------------------------------------------------------------------------- (e) dc: a backward-stable solve of the device's own system
def _check_solve(name, dtype, d, env=None):
    """A = S_E + lam diag(D) from the downloaded buffer, D as the engine takes it on a first linearisation: k_lm_reset zeroes D2c
    (sba_lm_kernels.hpp:739), the factorisation's prologue takes d = fmax(D2c, diagU) while LMState::fresh is set and damps with
    lam * fmax_pos(d) (sba_chol_blocked.hpp:775-777, sba_lm_kernels.hpp:273-275; fmax_pos: 0 -> 1, sba_kernels.hpp:92)."""
    c = xc.case(name)
    R = xc.ratios(name, {k: d[k] for k in ("S", "rhs", "diagU", "dc")}, xc.EPS[dtype])
    B, what = xc.device_solve_bound(dtype, c.C * c.ncp, env)
    print(f"\n[exact] solve {name} {dtype} {env or ''} n={c.C * c.ncp} {what}: dc_bwd={R['dc_bwd']:.3g} B={B:.3g} "
          f"fraction={R['dc_bwd'] / B:.3g} host={R['dc_bwd_host'] / B:.2g} reserved={d['reserved']}")
    assert d["reserved"] == 0          # at lam = 1e-2 every pivot is >= lam / (1 + lam) of its diagonal entry: no refusal
    assert np.all(np.isfinite(d["dc"])) and np.any(d["dc"] != 0.0)
    assert R["dc_bwd_host"] <= 0.01 * B
    assert R["dc_bwd"] <= B, (R["dc_bwd"], B)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", xc.ALL_CASES)
def test_camera_step_is_a_backward_stable_solve(name, dtype):
    """|A dc - rhs|_i <= B d_i sum_j d_j |dc_j| per row, d = sqrt(diag A), B from oracle/exact_cases.device_solve_bound."""
    _check_solve(name, dtype, _device(name, dtype))


_KNOB_PASSES = [("d16x24", dt, {"SBA_CHOL": "ll"}) for dt in DTYPES] + [("m9x40", dt, {"SBA_CHOL": "ll"}) for dt in DTYPES] \
    + [("w18x15", dt, {"SBA_CHOL": "blocked"}) for dt in DTYPES] + [("t16x12", dt, {"SBA_CHOL": "blocked"}) for dt in DTYPES] \
    + [("g24x10", dt, {"SBA_CHOL_BIG": "launches"}) for dt in DTYPES] + [("v34x6", dt, {"SBA_CHOL_BIG": "launches"}) for dt in DTYPES] \
    + [("d16x24", "f32", {"SBA_CHOL_F32": "0"})]


def _device_solve_only(name, dtype, env, monkeypatch):
    """One linearisation and one trial solve under the given factorisation switches (read at sba_create): S, rhs, diagU, dc and the
    repeat count, cached under its own key."""
    key = (name, dtype, tuple(sorted(env.items())))
    if key in _DEVICE:
        return _DEVICE[key]
    import torch
    torch.cuda.set_device(0)
    for k in ("SBA_CHOL", "SBA_CHOL_BIG", "SBA_CHOL_F32"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = xc.case(name)
    n = c.C * c.ncp
    d = {}
    with _native.Problem(c.cams, c.pts, c.uv, c.ci, c.pi, weights=c.w, dtype=dtype,
                         stream=torch.cuda.current_stream().cuda_stream) as prob:
        prob.lm_begin(prob.make_opts(ftol=1e-8, lambda0=xc.LAMBDA0))
        prob.lm_linearize()
        E = torch.zeros(prob.exchange_size(), dtype=torch.float64, device="cuda")
        prob.lm_form_reduced(E.data_ptr())
        torch.cuda.synchronize()
        Eh = E.cpu().numpy()
        d["S"], d["rhs"] = Eh[:n * n].reshape(n, n).copy(), Eh[n * n:n * n + n].copy()
        d["diagU"] = Eh[n * n + n:n * n + 2 * n].reshape(c.C, c.ncp).copy()
        sc = torch.zeros(8, dtype=torch.float64, device="cuda")
        prob.lm_solve_trial(E.data_ptr(), sc.data_ptr())
        torch.cuda.synchronize()
        d["dc"] = prob.lm_get_step()
        d["reserved"] = int(prob.lm_finish()[2].reserved)
    _DEVICE[key] = d
    return d


@pytest.mark.parametrize("name,dtype,env", _KNOB_PASSES, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else v)
def test_camera_step_through_the_other_factorisations(monkeypatch, name, dtype, env):
    """Real systems (diagonal over nine decades) through the kernels the default route of these sizes does not take: k_cholesky_ll
    below 177 unknowns, k_cholesky_stream, k_chol_big_prepare / k_chol_big_step, and the fp32 engine's f64 k_cholesky_blocked."""
    _check_solve(name, dtype, _device_solve_only(name, dtype, env, monkeypatch), env)
