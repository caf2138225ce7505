// sba_triangulate.hpp -- 3-D points from the handle's current cameras and its 2-D observations (sba_triangulate,
// include/sba_hip.h): per observation the distortion is inverted (Newton) and the pixel becomes a ray; per point the
// weighted least-squares point closest to its rays, its pixel errors, and -- optionally -- a leave-one-out trimming of
// the observation whose removal explains the others best.  Everything here is float64 whatever the handle's dtype, runs on
// private buffers freed on return and touches no LM kernel, no LM state and no route.
//
// Pipeline (one stream, one synchronisation at the end):
//   k_tri_cam_prep    one thread per camera: R, centre -R^T t, t and the intrinsics into a table of TRI_CAM doubles per camera
//   k_ray_fit<TriFit> workgroup b owns the whole points of blk_desc[b] and their observations (<= 256, one per thread: the reads
//                     of uv_pm / ci_pm / w_pm are coalesced): ray terms into LDS, segmented sums per point, one thread per point
//                     solves the 3 x 3 system, the observation threads project the estimate back, a second per-point pass
//                     takes max / sum of squares / minimum depth; points whose largest error exceeds trim_px go on a work list
//   k_tri_trim        one wave per listed point, lanes over the leave-one-out candidates
//   k_tri_scatter     per-observation flags from the layout's order to the caller's
//   k_tri_write_back  opts->write_back: the estimates of the OK points into the handle's current points
// k_ray_fit is the kernel of every per-point ray fit: the skeleton holds the summation order, the shuffled-equals-sorted rule and
// the duplicate-camera pass, a small policy struct what the fit does with the sums (TriFit here, UnpFit in sba_unproject.hpp).
// RayFitJob is the host side the entries share; an entry point is a policy plus its own *_run.
#pragma once
#include "sba_kernels.hpp"

namespace SBA_NS {
using namespace sba_host;

constexpr int TRI_CAM = 23;          // doubles per camera in the table (odd stride: rows of different cameras spread over the LDS banks)
constexpr int TC_R = 0, TC_C = 9, TC_T = 12, TC_F = 15, TC_K1 = 16, TC_K2 = 17, TC_P1 = 18, TC_P2 = 19, TC_CX = 20, TC_CY = 21;
constexpr int TRI_TERMS = 15;        // doubles per observation row in LDS (k_ray_fit lists the columns); odd stride
constexpr int TRI_NEWTON_MAX = 20;
constexpr unsigned char TRI_OBS_OUT = 0, TRI_OBS_IN = 1, TRI_OBS_UNUSABLE = 2, TRI_OBS_TRIMMED = 3;

// one camera row (NCP columns) into its TRI_CAM table entry
__device__ __forceinline__ void tri_cam_row(const double* __restrict__ cam, double* __restrict__ o) {
  double cp[CAMPRE];
  campre_build<double>(cam, cp);
#pragma unroll
  for (int i = 0; i < 9; ++i) o[TC_R + i] = cp[CP_R + i];
  const double t0 = cp[CP_T], t1 = cp[CP_T + 1], t2 = cp[CP_T + 2];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o[TC_C + k] = -(cp[CP_R + k] * t0 + cp[CP_R + 3 + k] * t1 + cp[CP_R + 6 + k] * t2);
    o[TC_T + k] = cp[CP_T + k];
  }
  o[TC_F] = cp[CP_F]; o[TC_K1] = cp[CP_K1]; o[TC_K2] = cp[CP_K2];
  if constexpr (TANGENTIAL) { o[TC_P1] = cp[CP_P1]; o[TC_P2] = cp[CP_P2]; }
  else { o[TC_P1] = 0.0; o[TC_P2] = 0.0; }
  o[TC_CX] = cp[CP_CX]; o[TC_CY] = cp[CP_CY];
  o[TRI_CAM - 1] = 0.0;
}

__global__ void __launch_bounds__(64) k_tri_cam_prep(const double* __restrict__ cams, double* __restrict__ tab, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  tri_cam_row(cams + (size_t)c * NCP, tab + (size_t)c * TRI_CAM);
}

// forward distortion of sba_model.hpp on normalised coordinates and its symmetric 2 x 2 Jacobian
__device__ __forceinline__ void tri_distort(const double* __restrict__ cp, double x, double y, double& fx, double& fy, double& gxx,
                                            double& gxy, double& gyy) {
  const double k1 = cp[TC_K1], k2 = cp[TC_K2];
  const double n = x * x + y * y;
  const double d = 1.0 + n * (k1 + k2 * n);
  const double dn = k1 + 2.0 * k2 * n;
  fx = x * d; fy = y * d;
  gxx = d + 2.0 * x * x * dn; gxy = 2.0 * x * y * dn; gyy = d + 2.0 * y * y * dn;
  if constexpr (TANGENTIAL) {
    const double p1 = cp[TC_P1], p2 = cp[TC_P2];
    fx += 2.0 * p1 * x * y + p2 * (n + 2.0 * x * x);
    fy += p1 * (n + 2.0 * y * y) + 2.0 * p2 * x * y;
    gxx += 2.0 * p1 * y + 6.0 * p2 * x;
    gxy += 2.0 * (p1 * x + p2 * y);
    gyy += 6.0 * p1 * y + 2.0 * p2 * x;
  }
}

// Newton inversion of the distortion from (xd, yd).  false: no convergence in TRI_NEWTON_MAX steps, a non-positive Jacobian
// determinant (the folded-back region of a non-monotone distortion) or a non-finite value.
__device__ __forceinline__ bool tri_undistort(const double* __restrict__ cp, double xd, double yd, double& x, double& y) {
  x = xd; y = yd;
  for (int it = 0; it < TRI_NEWTON_MAX; ++it) {
    double fx, fy, gxx, gxy, gyy;
    tri_distort(cp, x, y, fx, fy, gxx, gxy, gyy);
    const double ex = fx - xd, ey = fy - yd;
    const double det = gxx * gyy - gxy * gxy;
    if (!(det > 0.0)) return false;
    const double sx = (gyy * ex - gxy * ey) / det, sy = (gxx * ey - gxy * ex) / det;
    x -= sx; y -= sy;
    if (!isfinite(x) || !isfinite(y)) return false;
    if (fmax(fabs(sx), fabs(sy)) <= 1e-15 * fmax(1.0, fmax(fabs(x), fabs(y)))) return true;
  }
  return false;
}

// the ray of pixel (u, v): unit direction d = normalise(R^T (x, y, 1)); false when the observation is unusable
__device__ __forceinline__ bool tri_ray(const double* __restrict__ cp, double u, double v, double& d0, double& d1, double& d2) {
  const double f = cp[TC_F];
  double x, y;
  bool ok = tri_undistort(cp, (u - cp[TC_CX]) / f, (v - cp[TC_CY]) / f, x, y);
  const double v0 = cp[TC_R + 0] * x + cp[TC_R + 3] * y + cp[TC_R + 6];
  const double v1 = cp[TC_R + 1] * x + cp[TC_R + 4] * y + cp[TC_R + 7];
  const double v2 = cp[TC_R + 2] * x + cp[TC_R + 5] * y + cp[TC_R + 8];
  const double nv = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
  d0 = v0 / nv; d1 = v1 / nv; d2 = v2 / nv;
  ok = ok && isfinite(d0) && isfinite(d1) && isfinite(d2);
  if (!ok) { d0 = 0.0; d1 = 0.0; d2 = 0.0; }
  return ok;
}

// omega (I - d d^T) as a00 a10 a11 a20 a21 a22 and omega (I - d d^T) c
__device__ __forceinline__ void tri_terms(const double* __restrict__ cp, double om, double d0, double d1, double d2, double* __restrict__ t) {
  const double c0 = cp[TC_C], c1 = cp[TC_C + 1], c2 = cp[TC_C + 2];
  const double dc = d0 * c0 + d1 * c1 + d2 * c2;
  t[0] = om * (1.0 - d0 * d0); t[1] = -om * d1 * d0; t[2] = om * (1.0 - d1 * d1);
  t[3] = -om * d2 * d0; t[4] = -om * d2 * d1; t[5] = om * (1.0 - d2 * d2);
  t[6] = om * (c0 - d0 * dc); t[7] = om * (c1 - d1 * dc); t[8] = om * (c2 - d2 * dc);
}

// X = A^-1 b by a 3 x 3 Cholesky factorisation with the pivot test of k_cov_lin (a pivot at or below 1e-12 of its diagonal
// entry: the rays do not fix the point)
__device__ __forceinline__ bool tri_solve(const double* __restrict__ A, const double* __restrict__ b, double& X0, double& X1, double& X2) {
  const double l00 = sqrt(A[0]);
  const double l10 = A[1] / l00, l20 = A[3] / l00;
  const double p1 = A[2] - l10 * l10;
  const double l11 = sqrt(p1);
  const double l21 = (A[4] - l20 * l10) / l11;
  const double p2 = A[5] - l20 * l20 - l21 * l21;
  const double l22 = sqrt(p2);
  if (!(A[0] > 0.0) || !(p1 > 1e-12 * A[2]) || !(p2 > 1e-12 * A[5]) || !isfinite(l22)) return false;
  const double y0 = b[0] / l00;
  const double y1 = (b[1] - l10 * y0) / l11;
  const double y2 = (b[2] - l20 * y0 - l21 * y1) / l22;
  X2 = y2 / l22;
  X1 = (y1 - l21 * X2) / l11;
  X0 = (y0 - l10 * X1 - l20 * X2) / l00;
  return isfinite(X0) && isfinite(X1) && isfinite(X2);
}

// pixel error (unweighted, in pixels) of X against (u, v) through the forward model, and the depth (R X + t)_z
__device__ __forceinline__ double tri_err(const double* __restrict__ cp, double X0, double X1, double X2, double u, double v, double& z) {
  const double p0 = cp[TC_R + 0] * X0 + cp[TC_R + 1] * X1 + cp[TC_R + 2] * X2 + cp[TC_T + 0];
  const double p1 = cp[TC_R + 3] * X0 + cp[TC_R + 4] * X1 + cp[TC_R + 5] * X2 + cp[TC_T + 1];
  const double p2 = cp[TC_R + 6] * X0 + cp[TC_R + 7] * X1 + cp[TC_R + 8] * X2 + cp[TC_T + 2];
  z = p2;
  const double iz = 1.0 / p2;
  double fx, fy, gxx, gxy, gyy;
  tri_distort(cp, p0 * iz, p1 * iz, fx, fy, gxx, gxy, gyy);
  const double eu = cp[TC_F] * fx + cp[TC_CX] - u, ev = cp[TC_F] * fy + cp[TC_CY] - v;
  return sqrt(eu * eu + ev * ev);
}

// the status values every fit shares (the other two are the fit's: ST_TOO_FEW, ST_DEGENERATE)
constexpr int RAY_OK = SBA_TRI_OK, RAY_ANCHORED = SBA_TRI_ANCHORED, RAY_BEHIND = SBA_TRI_BEHIND;

struct RayOut {          // per-point outputs and the per-observation states (layout order), device pointers
  double* X;             // N x 3
  int32_t *status, *n_views;
  double *rms, *mx;
  double* spread;        // NULL for a fit without it
  unsigned char* state;  // M, TRI_OBS_*
  int32_t* list;         // points to trim, or NULL
  int32_t* cnt;          // [0] entries of list, [1] points that lost an observation; NULL without list
};

// ------------------------------------------------------------------ steps 1-5 and 7 for every point, one launch (k_ray_fit)
// Segmented reduction over the observations of every point of the workgroup: entry e (of ne) of point q is reduced over the
// point's observations in the order s_ord and lands in s_term[row of the point's first observation][col0 + e].  One thread per
// (point, entry) walks the point when the workgroup holds many points; with few points of many views H threads share a walk
// (fixed split by position, partials combined in order: the result does not depend on which thread ran what).
// Every thread of the workgroup has to call it (it synchronises).  val(k, e): the value of observation k; op(e, s, v).
template <typename Val, typename Op, typename Init>
__device__ __forceinline__ void tri_segmented(int tid, int npts, int ne, const short* __restrict__ s_ps, const short* __restrict__ s_ord,
                                              double* s_part, double* s_term /* val may read it */, int col0, Val val, Op op, Init init) {
  int H = 1;
  while (H < 16 && 2 * H * npts * ne <= PM_BLOCK) H *= 2;
  if (H == 1) {
    for (int item = tid; item < npts * ne; item += PM_BLOCK) {
      const int q = item / ne, e = item - q * ne;
      const int qa = s_ps[q], qb = s_ps[q + 1];
      if (qb > qa) {
        double s = init(e);
        for (int k = qa; k < qb; ++k) s = op(e, s, val((int)s_ord[k], e));
        s_term[qa * TRI_TERMS + col0 + e] = s;
      }
    }
    return;
  }
  const int item = tid / H, h = tid - item * H;
  const bool act = item < npts * ne;
  int e = 0, qa = 0, qb = 0;
  if (act) {
    const int q = item / ne;
    e = item - q * ne;
    qa = s_ps[q]; qb = s_ps[q + 1];
    const int len = qb - qa;
    double s = init(e);
    for (int k = qa + len * h / H; k < qa + len * (h + 1) / H; ++k) s = op(e, s, val((int)s_ord[k], e));
    s_part[tid] = s;
  }
  __syncthreads();
  if (act && h == 0 && qb > qa) {
    double s = s_part[tid];
    for (int j = 1; j < H; ++j) s = op(e, s, s_part[tid + j]);
    s_term[qa * TRI_TERMS + col0 + e] = s;
  }
}

// The fit of the triangulation: the point closest to the rays by tri_solve, the spread of the ray directions, and the work list
// of the trimming.  A policy of k_ray_fit carries exactly these members (UnpFit of sba_unproject.hpp is the other one):
//   NE, COL_USABLE, COL_FIRST   the summed columns of an observation's row and where the two flags sit among them
//   DIRS                        the ray directions are stored (columns 9-11) and summed
//   ST_TOO_FEW, ST_DEGENERATE   the status of a point seen by fewer than min_views cameras / whose solve fails
//   examined(c)                 the observations of camera c take part at all
//   solve(p, t, X0, X1, X2)     the estimate of point p from the sums t[0..5] = A, t[6..8] = b
//   finish(p, solved, nuse, mx, t, out)   outputs of its own; solved: the point has an estimate (OK or BEHIND)
struct TriFit {
  static constexpr int NE = 14, COL_USABLE = 12, COL_FIRST = 13;
  static constexpr bool DIRS = true;
  static constexpr int ST_TOO_FEW = SBA_TRI_TOO_FEW, ST_DEGENERATE = SBA_TRI_DEGENERATE;
  double trim_px;        // > 0: points whose largest error exceeds it go on out.list
  __device__ __forceinline__ bool examined(int) const { return true; }
  __device__ __forceinline__ bool solve(int, const double* __restrict__ t, double& X0, double& X1, double& X2) const {
    return tri_solve(t, t + 6, X0, X1, X2);
  }
  __device__ __forceinline__ void finish(int p, bool solved, int nuse, double mx, const double* __restrict__ t, const RayOut& out) const {
    double spread = __builtin_nan("");
    if (solved) {
      const double m0 = t[9] / nuse, m1 = t[10] / nuse, m2 = t[11] / nuse;
      spread = 1.0 - (m0 * m0 + m1 * m1 + m2 * m2);
      if (trim_px > 0.0 && !(mx <= trim_px)) out.list[atomicAdd(out.cnt, 1)] = p;
    }
    out.spread[p] = spread;
  }
};

// columns of an observation's row in LDS: 0-5 A, 6-8 b, with Fit::DIRS 9-11 direction, Fit::COL_USABLE usable (0 / 1),
// Fit::COL_FIRST first usable view of its camera (0 / 1); after the solve columns 0, 1 of every row take the observation's error
// and depth, columns 2-4 of a point's first row its estimate, columns 5-7 of that row the sum of squares, the maximum and the
// minimum depth (the sums of columns 9 and up stay: TriFit::finish reads the direction sum there)
template <typename T, typename Fit>
__global__ void __launch_bounds__(PM_BLOCK) k_ray_fit(const double* __restrict__ tab, int C, const typename Vec2<T>::type* __restrict__ uv,
                                                       const T* __restrict__ w, const int32_t* __restrict__ ci,
                                                       const int32_t* __restrict__ pt_start, const int4* __restrict__ blk_desc,
                                                       const unsigned char* __restrict__ fixed, const double* __restrict__ pts_held,
                                                       int min_views, Fit fit, RayOut out) {
  extern __shared__ __align__(16) unsigned char smem[];
  double* s_cam = reinterpret_cast<double*>(smem);                 // [C][TRI_CAM]
  __shared__ double s_term[PM_BLOCK * TRI_TERMS];
  __shared__ double s_part[PM_BLOCK];
  __shared__ short s_cid[PM_BLOCK], s_ord[PM_BLOCK], s_ps[PM_BLOCK + 1];
  __shared__ unsigned char s_use[PM_BLOCK], s_pst[PM_BLOCK];
  const int4 bd = blk_desc[blockIdx.x];
  const int p_lo = bd.x, npts = bd.y - bd.x, o_lo = bd.z, nobs = bd.w - bd.z;
  const int tid = threadIdx.x;
  for (int i = tid; i < C * TRI_CAM; i += PM_BLOCK) s_cam[i] = tab[i];
  for (int i = tid; i <= npts; i += PM_BLOCK) s_ps[i] = (short)(pt_start[p_lo + i] - o_lo);
  __syncthreads();
  // ---- one observation per thread: its point (binary search in the point starts), its ray and the ray's terms; observations
  // the fit does not examine (the other cameras of a reference-camera call) get no ray
  bool usable = false, examined = false;
  double u = 0.0, v = 0.0;
  const double* cp = s_cam;
  int q = 0, qa = 0, qb = 0;
  if (tid < nobs) {
    const int o = o_lo + tid;
    const int c = ci[o];
    const auto m = uv[o];
    const double ww = w ? (double)w[o] : 1.0;
    int hi = npts;
    while (hi - q > 1) {
      const int mid = (q + hi) >> 1;
      if (s_ps[mid] <= tid) q = mid; else hi = mid;
    }
    qa = s_ps[q]; qb = s_ps[q + 1];
    u = (double)m.x; v = (double)m.y;
    cp = s_cam + c * TRI_CAM;
    examined = fit.examined(c);
    double d0 = 0.0, d1 = 0.0, d2 = 0.0;
    if (examined) usable = tri_ray(cp, u, v, d0, d1, d2) && ww != 0.0 && isfinite(ww);
    if (!usable) { d0 = 0.0; d1 = 0.0; d2 = 0.0; }
    double* t = s_term + tid * TRI_TERMS;
    tri_terms(cp, usable ? ww * ww : 0.0, d0, d1, d2, t);
    if constexpr (Fit::DIRS) { t[9] = d0; t[10] = d1; t[11] = d2; }
    t[Fit::COL_USABLE] = usable ? 1.0 : 0.0;
    s_cid[tid] = (short)c;
    s_use[tid] = usable ? 1 : 0;
  }
  __syncthreads();
  // ---- the order of the sums: ascending camera inside a point, whatever order the layout left (rigs of more than 16 cameras keep
  // the caller's order inside a point), so that a shuffled list gives the bits of the sorted one.  Lists already in camera
  // order -- the usual case -- pay one compare per observation; otherwise every observation counts its rank.
  const int unsorted = __syncthreads_or(tid < nobs && tid > qa && s_cid[tid] < s_cid[tid - 1]);
  if (tid < nobs) {
    int r = tid;
    if (unsorted) {
      const int c = s_cid[tid];
      r = qa;
      for (int i = qa; i < qb; ++i) { const int c2 = s_cid[i]; r += (c2 < c || (c2 == c && i < tid)) ? 1 : 0; }
    }
    s_ord[r] = (short)tid;
  }
  __syncthreads();
  // ---- distinct cameras: the observation at order position tid is the first usable view of its camera or not
  if (tid < nobs) {
    const int k = s_ord[tid];
    const int c = s_cid[k];
    bool first = s_use[k] != 0;
    for (int j = tid - 1; first && j >= qa && s_cid[s_ord[j]] == c; --j) first = s_use[s_ord[j]] == 0;
    s_term[k * TRI_TERMS + Fit::COL_FIRST] = first ? 1.0 : 0.0;
  }
  __syncthreads();
  // ---- per point: the nine sums of A and b, the direction sum if there is one, the usable views and the distinct cameras
  tri_segmented(tid, npts, Fit::NE, s_ps, s_ord, s_part, s_term, 0,
                [&](int k, int e) { return s_term[k * TRI_TERMS + e]; }, [](int, double s, double x) { return s + x; },
                [](int) { return 0.0; });
  __syncthreads();
  // ---- one thread per point: the fit's solve
  int st = Fit::ST_TOO_FEW, nuse = 0;
  double X0 = 0.0, X1 = 0.0, X2 = 0.0;
  const int p = p_lo + tid;
  const int pa = tid < npts ? (int)s_ps[tid] : 0, pb = tid < npts ? (int)s_ps[tid + 1] : 0;
  if (tid < npts) {
    const double nan = __builtin_nan("");
    double* t = s_term + pa * TRI_TERMS;
    int ncam = 0;
    if (pb > pa) { nuse = (int)t[Fit::COL_USABLE]; ncam = (int)t[Fit::COL_FIRST]; }
    if (fixed != nullptr && fixed[p] != 0) {
      st = RAY_ANCHORED;
      X0 = pts_held[3 * (size_t)p]; X1 = pts_held[3 * (size_t)p + 1]; X2 = pts_held[3 * (size_t)p + 2];
    } else if (ncam < min_views) {
      st = Fit::ST_TOO_FEW; X0 = nan; X1 = nan; X2 = nan;
    } else {
      if (fit.solve(p, t, X0, X1, X2)) st = RAY_OK;
      else { st = Fit::ST_DEGENERATE; X0 = nan; X1 = nan; X2 = nan; }
    }
    if (pb > pa) { t[2] = X0; t[3] = X1; t[4] = X2; }
    s_pst[tid] = (unsigned char)st;
  }
  __syncthreads();
  // ---- observation threads: error and depth at the estimate, and the observation's state (one rule for every fit: an
  // observation that was not examined is OUT, not UNUSABLE)
  if (tid < nobs) {
    const int pst = s_pst[q];
    const double* x = s_term + qa * TRI_TERMS + 2;
    double e = 0.0, z = __builtin_inf();
    if (usable && pst == RAY_OK) e = tri_err(cp, x[0], x[1], x[2], u, v, z);
    s_term[tid * TRI_TERMS] = e;
    s_term[tid * TRI_TERMS + 1] = z;
    out.state[o_lo + tid] = pst == RAY_ANCHORED ? TRI_OBS_IN : (examined && !usable) ? TRI_OBS_UNUSABLE
                            : (usable && pst == RAY_OK) ? TRI_OBS_IN : TRI_OBS_OUT;
  }
  __syncthreads();
  // ---- per point: sum of squares, maximum (NaN sticks) and minimum depth over the used observations
  tri_segmented(tid, npts, 3, s_ps, s_ord, s_part, s_term, 5,
                [&](int k, int f) { const double e = s_term[k * TRI_TERMS]; return f == 0 ? e * e : f == 1 ? e : s_term[k * TRI_TERMS + 1]; },
                [](int f, double s, double x) { return f == 0 ? s + x : f == 1 ? ((s != s || x != x) ? __builtin_nan("") : fmax(s, x)) : fmin(s, x); },
                [](int f) { return f == 2 ? __builtin_inf() : 0.0; });
  __syncthreads();
  // ---- outputs
  if (tid < npts) {
    const double nan = __builtin_nan("");
    const double* t = s_term + pa * TRI_TERMS;
    const bool solved = st == RAY_OK;
    double rms = nan, mx = nan;
    int nv = 0;
    if (solved) {
      const double sq = t[5], zmin = t[7];
      mx = t[6];
      nv = nuse;
      rms = sqrt(sq / nuse);
      if (zmin <= 0.0) st = RAY_BEHIND;
    }
    fit.finish(p, solved, nuse, mx, t, out);
    out.X[3 * (size_t)p] = X0; out.X[3 * (size_t)p + 1] = X1; out.X[3 * (size_t)p + 2] = X2;
    out.status[p] = st; out.n_views[p] = nv;
    out.rms[p] = rms; out.mx[p] = mx;
  }
}

// ------------------------------------------------------------------ step 6: leave-one-out trimming of the listed points
__device__ __forceinline__ double tri_wave_sum(double v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}
__device__ __forceinline__ double tri_wave_max(double v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v = fmax(v, __shfl_xor(v, s, 64));
  return v;
}
__device__ __forceinline__ double tri_wave_min(double v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v = fmin(v, __shfl_xor(v, s, 64));
  return v;
}

// One wave (= one workgroup of 64) per listed point; lane j solves the system without observation j and walks the point's
// other observations: quadratic in the views of a point, which is why only the listed points come here.
template <typename T>
__global__ void __launch_bounds__(64) k_tri_trim(const double* __restrict__ tab, const typename Vec2<T>::type* __restrict__ uv,
                                                  const T* __restrict__ w, const int32_t* __restrict__ ci,
                                                  const int32_t* __restrict__ pt_start, int min_views, int max_drop, double trim_px,
                                                  RayOut out) {
  __shared__ double s_d[PM_BLOCK * 3], s_om[PM_BLOCK], s_u[PM_BLOCK], s_v[PM_BLOCK], s_e[PM_BLOCK], s_z[PM_BLOCK];
  __shared__ short s_c[PM_BLOCK];
  __shared__ unsigned char s_use[PM_BLOCK];
  const int lane = threadIdx.x;
  const int nlist = out.cnt[0];
  const double inf = __builtin_inf();
  for (int it = blockIdx.x; it < nlist; it += gridDim.x) {
    const int p = out.list[it];
    const int a = pt_start[p], deg = min(pt_start[p + 1] - a, PM_BLOCK);
    __syncthreads();                         // the previous point's LDS reads are over
    double acc[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) acc[e] = 0.0;
    int nmine = 0;
    for (int k = lane; k < deg; k += 64) {
      const int o = a + k;
      const int c = ci[o];
      const auto m = uv[o];
      const double ww = w ? (double)w[o] : 1.0;
      const double* cp = tab + (size_t)c * TRI_CAM;
      const bool use = out.state[o] == TRI_OBS_IN;
      double d0, d1, d2;
      (void)tri_ray(cp, (double)m.x, (double)m.y, d0, d1, d2);
      const double om = use ? ww * ww : 0.0;
      s_d[k * 3] = d0; s_d[k * 3 + 1] = d1; s_d[k * 3 + 2] = d2;
      s_om[k] = om; s_u[k] = (double)m.x; s_v[k] = (double)m.y; s_c[k] = (short)c; s_use[k] = use ? 1 : 0;
      if (use) {
        double t[9];
        tri_terms(cp, om, d0, d1, d2, t);
#pragma unroll
        for (int e = 0; e < 9; ++e) acc[e] += t[e];
        ++nmine;
      }
    }
    double A[6], bb[3];
#pragma unroll
    for (int e = 0; e < 6; ++e) A[e] = tri_wave_sum(acc[e]);
#pragma unroll
    for (int e = 0; e < 3; ++e) bb[e] = tri_wave_sum(acc[6 + e]);
    int nused = (int)tri_wave_sum((double)nmine);
    double X0 = out.X[3 * (size_t)p], X1 = out.X[3 * (size_t)p + 1], X2 = out.X[3 * (size_t)p + 2];
    __syncthreads();
    for (int k = lane; k < deg; k += 64)
      if (s_use[k]) s_e[k] = tri_err(tab + (size_t)s_c[k] * TRI_CAM, X0, X1, X2, s_u[k], s_v[k], s_z[k]);
    __syncthreads();
    bool dropped = false;
    for (int r = 0; r < max_drop; ++r) {
      double emax = 0.0;
      for (int k = lane; k < deg; k += 64)
        if (s_use[k]) { const double e = s_e[k]; emax = fmax(emax, e != e ? inf : e); }
      emax = tri_wave_max(emax);
      if (!(emax > trim_px) || !(nused > max(min_views, 3))) break;
      double best_m = inf;
      int best_j = 0x7fffffff;
      for (int j = lane; j < deg; j += 64) {
        if (!s_use[j]) continue;
        double t[9], Aj[6], bj[3], Y0, Y1, Y2;
        tri_terms(tab + (size_t)s_c[j] * TRI_CAM, s_om[j], s_d[j * 3], s_d[j * 3 + 1], s_d[j * 3 + 2], t);
#pragma unroll
        for (int e = 0; e < 6; ++e) Aj[e] = A[e] - t[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) bj[e] = bb[e] - t[6 + e];
        if (!tri_solve(Aj, bj, Y0, Y1, Y2)) continue;
        double mj = 0.0;
        for (int i = 0; i < deg; ++i) {
          if (i == j || !s_use[i]) continue;
          double z;
          const double e = tri_err(tab + (size_t)s_c[i] * TRI_CAM, Y0, Y1, Y2, s_u[i], s_v[i], z);
          mj = e != e ? inf : fmax(mj, e);
        }
        if (mj < best_m) { best_m = mj; best_j = j; }
      }
      // argmin over the wave, ties to the earlier position
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) {
        const double om = __shfl_xor(best_m, s, 64);
        const int oj = __shfl_xor(best_j, s, 64);
        if (om < best_m || (om == best_m && oj < best_j)) { best_m = om; best_j = oj; }
      }
      if (!(best_m < inf)) break;
      {
        const int j = best_j;
        double t[9];
        tri_terms(tab + (size_t)s_c[j] * TRI_CAM, s_om[j], s_d[j * 3], s_d[j * 3 + 1], s_d[j * 3 + 2], t);
#pragma unroll
        for (int e = 0; e < 6; ++e) A[e] -= t[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) bb[e] -= t[6 + e];
        (void)tri_solve(A, bb, X0, X1, X2);
        __syncthreads();
        if (lane == 0) { s_use[j] = 0; out.state[a + j] = TRI_OBS_TRIMMED; }
        __syncthreads();
        --nused;
        dropped = true;
      }
      for (int k = lane; k < deg; k += 64)
        if (s_use[k]) s_e[k] = tri_err(tab + (size_t)s_c[k] * TRI_CAM, X0, X1, X2, s_u[k], s_v[k], s_z[k]);
      __syncthreads();
    }
    if (!dropped) continue;
    double sq = 0.0, mx = 0.0, zmin = inf, ds0 = 0.0, ds1 = 0.0, ds2 = 0.0, bad = 0.0;
    for (int k = lane; k < deg; k += 64)
      if (s_use[k]) {
        const double e = s_e[k];
        if (e != e) bad = 1.0;
        sq += e * e; mx = fmax(mx, e); zmin = fmin(zmin, s_z[k]);
        ds0 += s_d[k * 3]; ds1 += s_d[k * 3 + 1]; ds2 += s_d[k * 3 + 2];
      }
    sq = tri_wave_sum(sq); mx = tri_wave_max(mx); zmin = tri_wave_min(zmin); bad = tri_wave_max(bad);
    ds0 = tri_wave_sum(ds0); ds1 = tri_wave_sum(ds1); ds2 = tri_wave_sum(ds2);
    if (lane == 0) {
      out.X[3 * (size_t)p] = X0; out.X[3 * (size_t)p + 1] = X1; out.X[3 * (size_t)p + 2] = X2;
      out.status[p] = zmin <= 0.0 ? SBA_TRI_BEHIND : SBA_TRI_OK;
      out.n_views[p] = nused;
      out.rms[p] = sqrt(sq / nused);
      out.mx[p] = bad != 0.0 ? __builtin_nan("") : mx;
      const double m0 = ds0 / nused, m1 = ds1 / nused, m2 = ds2 / nused;
      out.spread[p] = 1.0 - (m0 * m0 + m1 * m1 + m2 * m2);
      atomicAdd(out.cnt + 1, 1);
    }
  }
}

// flags from the layout's order to the caller's (perm: layout position -> caller's index)
__global__ void __launch_bounds__(256) k_tri_scatter(const unsigned char* __restrict__ state, const int32_t* __restrict__ perm, int64_t M,
                                                     unsigned char* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < M) out[perm[k]] = state[k];
}

// opts->write_back: the estimates of the OK points replace the handle's current points (both precisions), all others stay
template <typename T>
__global__ void __launch_bounds__(256) k_tri_write_back(const double* __restrict__ X, const int32_t* __restrict__ status, int N,
                                                        double* __restrict__ pts, T* __restrict__ ptsT) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * N || status[i / 3] != SBA_TRI_OK) return;
  pts[i] = X[i];
  ptsT[i] = (T)X[i];
}

// what the engine hands over: its current parameters and the point-major observation layout, all device pointers
template <typename T>
struct TriIn {
  hipStream_t stream;
  int C, N;
  int64_t M;
  const double *cams;
  double* pts;
  T* ptsT;
  const typename Vec2<T>::type* uv;
  const T* w;
  const int32_t *ci, *pt_start;
  const int4* blk_desc;
  int nblk;
  const unsigned char* fixed;
  const int64_t* perm;            // host: layout position -> caller's index, or NULL for the identity
};

// The part of a ray-fit call that does not depend on the fit (tri_run and unp_run each hold one): the private buffers, the
// permutation as int32, the launches either side of the entry's own work, and the status / state read-back with its counts.
// The order of a call: fit(), [the entry's own launches], flags_and_write_back(), read_back() and the entry's own fetch()es,
// hipStreamSynchronize, deliver().
template <typename T>
struct RayFitJob {
  ArenaScope own{nullptr};          // private buffers: hipMalloc'd here, freed on return (the handle's arena stays as it was)
  const TriIn<T>& in;
  DevBuf<double> tab, X, rms, mx;
  DevBuf<int32_t> status, nviews, perm32;
  DevBuf<unsigned char> state, state_out;
  std::vector<int32_t> p32, h_stat;                  // (p32: staging of the permutation, lives until the synchronisation at the end)
  std::vector<unsigned char> h_state;
  int64_t n_status[5] = {}, n_state[4] = {};         // deliver(): points per status (RAY_* / Fit::ST_*), observations per TRI_OBS_*
  explicit RayFitJob(const TriIn<T>& in_) : in(in_) {
    const int N = in.N;
    const int64_t M = in.M;
    tab.alloc((size_t)in.C * TRI_CAM);
    X.alloc((size_t)N * 3); rms.alloc(N); mx.alloc(N); status.alloc(N); nviews.alloc(N); state.alloc(M);
    if (in.perm && M) {
      p32.resize((size_t)M);
      for (int64_t k = 0; k < M; ++k) p32[k] = (int32_t)in.perm[k];
      perm32.upload(p32, in.stream);
      state_out.alloc(M);
    }
  }
  RayOut out(double* spread, int32_t* list, int32_t* cnt) const { return {X.p, status.p, nviews.p, rms.p, mx.p, spread, state.p, list, cnt}; }
  template <typename Fit>
  void fit(int min_views, const Fit& f, const RayOut& o) {           // the camera table and every point
    hipLaunchKernelGGL(k_tri_cam_prep, dim3((in.C + 63) / 64), dim3(64), 0, in.stream, in.cams, tab.p, in.C);
    if (in.nblk > 0)
      hipLaunchKernelGGL((k_ray_fit<T, Fit>), dim3(in.nblk), dim3(PM_BLOCK), (size_t)in.C * TRI_CAM * sizeof(double), in.stream, tab.p, in.C,
                         in.uv, in.w, in.ci, in.pt_start, in.blk_desc, in.fixed, (const double*)in.pts, min_views, f, o);
    HIPCHK(hipGetLastError());
  }
  void flags_and_write_back(bool write_back) {
    if (state_out.n)
      hipLaunchKernelGGL(k_tri_scatter, dim3((unsigned)((in.M + 255) / 256)), dim3(256), 0, in.stream, state.p, perm32.p, in.M, state_out.p);
    if (write_back && in.N > 0)
      hipLaunchKernelGGL(k_tri_write_back<T>, dim3((3 * in.N + 255) / 256), dim3(256), 0, in.stream, X.p, status.p, in.N, in.pts, in.ptsT);
    HIPCHK(hipGetLastError());
  }
  void fetch(void* dst, const void* src, size_t bytes) { if (dst && bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, in.stream)); }
  void read_back() {
    h_stat.resize(in.N); h_state.resize((size_t)in.M);
    fetch(h_stat.data(), status.p, sizeof(int32_t) * h_stat.size());
    fetch(h_state.data(), state_out.n ? state_out.p : state.p, h_state.size());
  }
  // after the synchronisation: the counts, and the caller's status and in-the-estimate flags (either may be NULL)
  void deliver(int32_t* status_out, uint8_t* in_out) {
    for (int32_t s : h_stat) n_status[(uint32_t)s < 4 ? s : 4]++;
    for (unsigned char s : h_state) if (s < 4) n_state[s]++;
    if (status_out) std::copy(h_stat.begin(), h_stat.end(), status_out);
    if (in_out) for (int64_t k = 0; k < in.M; ++k) in_out[k] = h_state[k] == TRI_OBS_IN ? 1 : 0;
  }
};

template <typename T>
int tri_run(const TriIn<T>& in, const sba_tri_opts& opt, double* points_out, int32_t* status_out, int32_t* n_views_out, double* rms_out,
            double* max_out, double* spread_out, uint8_t* inlier_out, sba_tri_report* rep, std::string& err) {
  const auto t_start = std::chrono::steady_clock::now();
  if (opt.min_views < 2) { err = "sba_triangulate: min_views must be at least 2"; return SBA_ERR_INVALID; }
  if (!(opt.trim_px >= 0.0) || !std::isfinite(opt.trim_px)) { err = "sba_triangulate: trim_px must be finite and not negative"; return SBA_ERR_INVALID; }
  if (opt.max_drop < 0) { err = "sba_triangulate: max_drop must not be negative"; return SBA_ERR_INVALID; }
  hipStream_t st = in.stream;
  const int N = in.N;
  const bool trim = opt.trim_px > 0.0 && opt.max_drop > 0;
  RayFitJob<T> job(in);
  DevEvents<4> ev;
  DevBuf<double> spread;
  DevBuf<int32_t> list, cnt;
  spread.alloc(N); list.alloc(std::max(N, 1)); cnt.alloc(2);
  cnt.zero(st);
  const RayOut out = job.out(spread.p, list.p, cnt.p);
  // ---- device phases: [ev0, ev1) camera table + every point, [ev1, ev2) trimming, [ev2, ev3) flags / write-back
  HIPCHK(hipEventRecord(ev[0], st));
  job.fit((int)opt.min_views, TriFit{trim ? opt.trim_px : 0.0}, out);
  HIPCHK(hipEventRecord(ev[1], st));
  if (trim && N > 0)      // the length of the list stays on the device: a fixed grid strides over it
    hipLaunchKernelGGL(k_tri_trim<T>, dim3(std::min(N, 2048)), dim3(64), 0, st, job.tab.p, in.uv, in.w, in.ci, in.pt_start,
                       (int)opt.min_views, (int)opt.max_drop, opt.trim_px, out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ev[2], st));
  job.flags_and_write_back(opt.write_back != 0);
  HIPCHK(hipEventRecord(ev[3], st));
  // ---- read-back: the per-point arrays go straight into the caller's
  int32_t h_cnt[2] = {0, 0};
  job.read_back();
  job.fetch(h_cnt, cnt.p, sizeof h_cnt);
  job.fetch(points_out, job.X.p, sizeof(double) * 3 * N);
  job.fetch(n_views_out, job.nviews.p, sizeof(int32_t) * N);
  job.fetch(rms_out, job.rms.p, sizeof(double) * N);
  job.fetch(max_out, job.mx.p, sizeof(double) * N);
  job.fetch(spread_out, spread.p, sizeof(double) * N);
  HIPCHK(hipStreamSynchronize(st));
  job.deliver(status_out, inlier_out);
  if (rep) {
    const float ms[3] = {ev.ms(0, 1), ev.ms(1, 2), ev.ms(2, 3)};
    *rep = sba_tri_report{};
    rep->n_ok = job.n_status[SBA_TRI_OK]; rep->n_anchored = job.n_status[SBA_TRI_ANCHORED]; rep->n_too_few = job.n_status[SBA_TRI_TOO_FEW];
    rep->n_degenerate = job.n_status[SBA_TRI_DEGENERATE]; rep->n_behind = job.n_status[SBA_TRI_BEHIND];
    rep->n_obs_unusable = job.n_state[TRI_OBS_UNUSABLE]; rep->n_obs_trimmed = job.n_state[TRI_OBS_TRIMMED];
    rep->n_points_trimmed = h_cnt[1];
    rep->seconds_linear = ms[0] * 1e-3;
    rep->seconds_trim = ms[1] * 1e-3;
    rep->seconds_device = (ms[0] + ms[1] + ms[2]) * 1e-3;
    rep->seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
  }
  return SBA_OK;
}

}  // namespace SBA_NS
