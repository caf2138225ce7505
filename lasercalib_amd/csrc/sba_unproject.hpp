// sba_unproject.hpp -- the inverse camera model (sba_unproject_rows, sba_unproject; include/sba_hip.h): a pixel becomes a ray
// (the Newton inversion and the ray of sba_triangulate.hpp), and a ray or the rays of a point meet a known plane n . X = d.
// Everything here is float64 whatever the handle's dtype, runs on private buffers freed on return and touches no LM kernel, no
// LM state and no route.
//
// sba_unproject_rows (stateless, gathered rows):
//   k_unp_rows        one row per lane: the row's table entry (tri_cam_row), undistorted coordinates, origin, direction and the
//                     intersection with the row's plane
// sba_unproject (one stream, one synchronisation at the end):
//   k_tri_cam_prep    the camera table of sba_triangulate.hpp
//   k_unp_plane_fit   workgroup b owns the whole points of blk_desc[b] and their observations (<= 256, one per thread): ray terms
//                     into LDS, segmented sums per point (tri_segmented), one thread per point reduces A, b to the plane's 2 x 2
//                     system and solves it, the observation threads project the estimate back, a second per-point pass takes
//                     max / sum of squares / minimum depth
//   k_tri_scatter     per-observation flags from the layout's order to the caller's
//   k_tri_write_back  opts->write_back: the estimates of the OK points into the handle's current points
#pragma once
#include "sba_triangulate.hpp"

namespace SBA_NS {

constexpr double UNP_PARALLEL = 1e-6;          // |nh . dir| at or below it: the ray runs along the plane (sba_unproject_rows)
constexpr int64_t UNP_ROWS_CHUNK = 1 << 20;    // rows per launch of k_unp_rows
static_assert((int)SBA_UNP_OK == (int)SBA_TRI_OK, "k_tri_write_back moves the points of status 0");

// unit normal and offset of the plane n . X = d
__device__ __forceinline__ void unp_plane(const double* __restrict__ pl, double& n0, double& n1, double& n2, double& dh) {
  const double nn = sqrt(pl[0] * pl[0] + pl[1] * pl[1] + pl[2] * pl[2]);
  n0 = pl[0] / nn; n1 = pl[1] / nn; n2 = pl[2] / nn; dh = pl[3] / nn;
}

// ------------------------------------------------------------------ sba_unproject_rows
__global__ void __launch_bounds__(256) k_unp_rows(const double* __restrict__ uv, const double* __restrict__ cam,
                                                  const double* __restrict__ planes /* NULL: rays only */, int plane_stride /* 0 / 4 */,
                                                  int64_t n, double* __restrict__ xn, double* __restrict__ origin,
                                                  double* __restrict__ dir, double* __restrict__ X, double* __restrict__ depth,
                                                  int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double nan = __builtin_nan("");
  double cp[TRI_CAM];
  tri_cam_row(cam + NCP * i, cp);
  const double u = uv[2 * i], v = uv[2 * i + 1];
  double x, y, d0, d1, d2;
  // (tri_ray runs the same inversion again: the direction has the bits k_unp_plane_fit works with)
  bool ok = tri_undistort(cp, (u - cp[TC_CX]) / cp[TC_F], (v - cp[TC_CY]) / cp[TC_F], x, y);
  ok = tri_ray(cp, u, v, d0, d1, d2) && ok;
  const double c0 = cp[TC_C], c1 = cp[TC_C + 1], c2 = cp[TC_C + 2];
  ok = ok && isfinite(c0) && isfinite(c1) && isfinite(c2);
  int st = ok ? SBA_UNP_ROW_OK : SBA_UNP_ROW_UNUSABLE;
  double X0 = nan, X1 = nan, X2 = nan, z = nan;
  if (ok && planes != nullptr) {
    double n0, n1, n2, dh;
    unp_plane(planes + (size_t)plane_stride * i, n0, n1, n2, dh);
    const double s = n0 * d0 + n1 * d1 + n2 * d2;
    if (fabs(s) <= UNP_PARALLEL) st = SBA_UNP_ROW_PARALLEL;
    else {
      const double tau = (dh - (n0 * c0 + n1 * c1 + n2 * c2)) / s;
      X0 = c0 + tau * d0; X1 = c1 + tau * d1; X2 = c2 + tau * d2;
      z = cp[TC_R + 6] * X0 + cp[TC_R + 7] * X1 + cp[TC_R + 8] * X2 + cp[TC_T + 2];
      if (!(isfinite(X0) && isfinite(X1) && isfinite(X2) && isfinite(z))) st = SBA_UNP_ROW_UNUSABLE;
      else if (z <= 0.0) st = SBA_UNP_ROW_BEHIND;
    }
  }
  if (st == SBA_UNP_ROW_UNUSABLE) { x = nan; y = nan; d0 = nan; d1 = nan; d2 = nan; X0 = nan; X1 = nan; X2 = nan; z = nan; }
  const bool ray = st != SBA_UNP_ROW_UNUSABLE;
  if (xn) { xn[2 * i] = x; xn[2 * i + 1] = y; }
  if (origin) { origin[3 * i] = ray ? c0 : nan; origin[3 * i + 1] = ray ? c1 : nan; origin[3 * i + 2] = ray ? c2 : nan; }
  if (dir) { dir[3 * i] = d0; dir[3 * i + 1] = d1; dir[3 * i + 2] = d2; }
  if (X) { X[3 * i] = X0; X[3 * i + 1] = X1; X[3 * i + 2] = X2; }
  if (depth) depth[i] = z;
  if (status) status[i] = st;
}

// a plane the caller handed over: finite, with a normal that is not zero
inline bool unp_planes_ok(const double* planes, int64_t n_planes) {
  for (int64_t k = 0; k < n_planes; ++k) {
    const double* p = planes + 4 * k;
    const double nn = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
    if (!std::isfinite(nn) || !(nn > 0.0) || !std::isfinite(p[3])) return false;
  }
  return true;
}

inline int unp_rows_call(int device, int64_t n, const double* uv, const double* cam_rows, const double* planes, int64_t n_planes,
                         double* xn_out, double* origin_out, double* dir_out, double* points_out, double* depth_out,
                         int32_t* status_out) {
  HIPCHK(hipSetDevice(device));
  const bool per_row = n_planes > 1;
  DevBuf<double> d_uv, d_cam, d_pl, d_xn, d_or, d_dir, d_X, d_z;
  DevBuf<int32_t> d_st;
  const int64_t cap = std::min(n, UNP_ROWS_CHUNK);
  if (cap == 0) return SBA_OK;
  d_uv.alloc(cap * 2); d_cam.alloc(cap * NCP);
  if (n_planes) d_pl.alloc(per_row ? cap * 4 : 4);
  if (xn_out) d_xn.alloc(cap * 2);
  if (origin_out) d_or.alloc(cap * 3);
  if (dir_out) d_dir.alloc(cap * 3);
  if (points_out) d_X.alloc(cap * 3);
  if (depth_out) d_z.alloc(cap);
  if (status_out) d_st.alloc(cap);
  if (n_planes && !per_row) HIPCHK(hipMemcpy(d_pl.p, planes, sizeof(double) * 4, hipMemcpyHostToDevice));
  for (int64_t lo = 0; lo < n; lo += cap) {
    const int64_t m = std::min(cap, n - lo);
    HIPCHK(hipMemcpy(d_uv.p, uv + 2 * lo, sizeof(double) * m * 2, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_cam.p, cam_rows + NCP * lo, sizeof(double) * m * NCP, hipMemcpyHostToDevice));
    if (per_row) HIPCHK(hipMemcpy(d_pl.p, planes + 4 * lo, sizeof(double) * m * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_unp_rows, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, 0, d_uv.p, d_cam.p, d_pl.p, per_row ? 4 : 0, m,
                       d_xn.p, d_or.p, d_dir.p, d_X.p, d_z.p, d_st.p);
    HIPCHK(hipGetLastError());
    if (xn_out) HIPCHK(hipMemcpy(xn_out + 2 * lo, d_xn.p, sizeof(double) * m * 2, hipMemcpyDeviceToHost));
    if (origin_out) HIPCHK(hipMemcpy(origin_out + 3 * lo, d_or.p, sizeof(double) * m * 3, hipMemcpyDeviceToHost));
    if (dir_out) HIPCHK(hipMemcpy(dir_out + 3 * lo, d_dir.p, sizeof(double) * m * 3, hipMemcpyDeviceToHost));
    if (points_out) HIPCHK(hipMemcpy(points_out + 3 * lo, d_X.p, sizeof(double) * m * 3, hipMemcpyDeviceToHost));
    if (depth_out) HIPCHK(hipMemcpy(depth_out + lo, d_z.p, sizeof(double) * m, hipMemcpyDeviceToHost));
    if (status_out) HIPCHK(hipMemcpy(status_out + lo, d_st.p, sizeof(int32_t) * m, hipMemcpyDeviceToHost));
  }
  return SBA_OK;
}

// ------------------------------------------------------------------ sba_unproject
// The point of the plane nh . X = dh closest to the rays behind A = sum omega (I - d d^T), b = sum omega (I - d d^T) c:
// X = X0 + B y with X0 = dh nh and B = [e1 e2] a basis of the plane, (B^T A B) y = B^T (b - A X0) by a 2 x 2 Cholesky
// factorisation with the pivot test of tri_solve.  A as a00 a10 a11 a20 a21 a22.
__device__ __forceinline__ bool unp_solve(const double* __restrict__ A, const double* __restrict__ b, double n0, double n1, double n2,
                                          double dh, double& X0, double& X1, double& X2) {
  const double a0 = fabs(n0), a1 = fabs(n1), a2 = fabs(n2);
  const int k = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);      // the axis the normal leans on least, ties to the smaller index
  const double nk = k == 0 ? n0 : k == 1 ? n1 : n2;
  double e0 = (k == 0 ? 1.0 : 0.0) - nk * n0, e1 = (k == 1 ? 1.0 : 0.0) - nk * n1, e2 = (k == 2 ? 1.0 : 0.0) - nk * n2;
  const double en = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
  e0 /= en; e1 /= en; e2 /= en;
  const double f0 = n1 * e2 - n2 * e1, f1 = n2 * e0 - n0 * e2, f2 = n0 * e1 - n1 * e0;
  const double p0 = dh * n0, p1 = dh * n1, p2 = dh * n2;
  const double Ae0 = A[0] * e0 + A[1] * e1 + A[3] * e2, Ae1 = A[1] * e0 + A[2] * e1 + A[4] * e2, Ae2 = A[3] * e0 + A[4] * e1 + A[5] * e2;
  const double Af0 = A[0] * f0 + A[1] * f1 + A[3] * f2, Af1 = A[1] * f0 + A[2] * f1 + A[4] * f2, Af2 = A[3] * f0 + A[4] * f1 + A[5] * f2;
  const double r0 = b[0] - (A[0] * p0 + A[1] * p1 + A[3] * p2), r1 = b[1] - (A[1] * p0 + A[2] * p1 + A[4] * p2),
               r2 = b[2] - (A[3] * p0 + A[4] * p1 + A[5] * p2);
  const double G00 = e0 * Ae0 + e1 * Ae1 + e2 * Ae2, G10 = f0 * Ae0 + f1 * Ae1 + f2 * Ae2, G11 = f0 * Af0 + f1 * Af1 + f2 * Af2;
  const double g0 = e0 * r0 + e1 * r1 + e2 * r2, g1 = f0 * r0 + f1 * r1 + f2 * r2;
  const double l00 = sqrt(G00);
  const double l10 = G10 / l00;
  const double pv = G11 - l10 * l10;
  const double l11 = sqrt(pv);
  if (!(G00 > 0.0) || !(pv > 1e-12 * G11) || !isfinite(l11)) return false;
  const double w0 = g0 / l00;
  const double w1 = (g1 - l10 * w0) / l11;
  const double y1 = w1 / l11;
  const double y0 = (w0 - l10 * y1) / l00;
  X0 = p0 + e0 * y0 + f0 * y1; X1 = p1 + e1 * y0 + f1 * y1; X2 = p2 + e2 * y0 + f2 * y1;
  return isfinite(X0) && isfinite(X1) && isfinite(X2);
}

struct UnpOut {          // per-point outputs and the per-observation states (layout order), device pointers
  double* X;             // N x 3
  int32_t *status, *n_views;
  double *rms, *mx;
  unsigned char* state;  // M, TRI_OBS_*
};

// columns of an observation's row in LDS (stride TRI_TERMS, the stride tri_segmented works with): 0-5 A, 6-8 b, 9 usable (0 / 1),
// 10 first usable view of its camera (0 / 1); after the solve columns 0, 1 of every row take the observation's error and depth,
// columns 2-4 of a point's first row its estimate, columns 5-7 of that row the sum of squares, the maximum and the minimum depth
template <typename T>
__global__ void __launch_bounds__(PM_BLOCK) k_unp_plane_fit(const double* __restrict__ tab, int C, const typename Vec2<T>::type* __restrict__ uv,
                                                             const T* __restrict__ w, const int32_t* __restrict__ ci,
                                                             const int32_t* __restrict__ pt_start, const int4* __restrict__ blk_desc,
                                                             const unsigned char* __restrict__ fixed, const double* __restrict__ pts_held,
                                                             const double* __restrict__ planes, int plane_stride /* 0 / 4 */,
                                                             int min_views, int ref_cam /* < 0: every camera */, UnpOut out) {
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
  // ---- one observation per thread: its point (binary search in the point starts), its ray and the ray's terms; with a
  // reference camera the observations of the other cameras are not examined
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
    examined = ref_cam < 0 || c == ref_cam;
    double d0 = 0.0, d1 = 0.0, d2 = 0.0;
    if (examined) usable = tri_ray(cp, u, v, d0, d1, d2) && ww != 0.0 && isfinite(ww);
    if (!usable) { d0 = 0.0; d1 = 0.0; d2 = 0.0; }
    double* t = s_term + tid * TRI_TERMS;
    tri_terms(cp, usable ? ww * ww : 0.0, d0, d1, d2, t);
    t[9] = usable ? 1.0 : 0.0;
    s_cid[tid] = (short)c;
    s_use[tid] = usable ? 1 : 0;
  }
  __syncthreads();
  // ---- the order of the sums: ascending camera inside a point, whatever order the layout left (as k_tri_linear)
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
    s_term[k * TRI_TERMS + 10] = first ? 1.0 : 0.0;
  }
  __syncthreads();
  // ---- per point: the nine sums of A and b, the usable views and the distinct cameras
  tri_segmented(tid, npts, 11, s_ps, s_ord, s_part, s_term, 0,
                [&](int k, int e) { return s_term[k * TRI_TERMS + e]; }, [](int, double s, double x) { return s + x; },
                [](int) { return 0.0; });
  __syncthreads();
  // ---- one thread per point: the plane's 2 x 2 system
  int st = SBA_UNP_NO_VIEW, nuse = 0;
  double X0 = 0.0, X1 = 0.0, X2 = 0.0;
  const int p = p_lo + tid;
  const int pa = tid < npts ? (int)s_ps[tid] : 0, pb = tid < npts ? (int)s_ps[tid + 1] : 0;
  if (tid < npts) {
    const double nan = __builtin_nan("");
    double* t = s_term + pa * TRI_TERMS;
    int ncam = 0;
    if (pb > pa) { nuse = (int)t[9]; ncam = (int)t[10]; }
    if (fixed != nullptr && fixed[p] != 0) {
      st = SBA_UNP_ANCHORED;
      X0 = pts_held[3 * (size_t)p]; X1 = pts_held[3 * (size_t)p + 1]; X2 = pts_held[3 * (size_t)p + 2];
    } else if (ncam < min_views) {
      st = SBA_UNP_NO_VIEW; X0 = nan; X1 = nan; X2 = nan;
    } else {
      double n0, n1, n2, dh;
      unp_plane(planes + (size_t)plane_stride * p, n0, n1, n2, dh);
      if (unp_solve(t, t + 6, n0, n1, n2, dh, X0, X1, X2)) st = SBA_UNP_OK;
      else { st = SBA_UNP_DEGENERATE; X0 = nan; X1 = nan; X2 = nan; }
    }
    if (pb > pa) { t[2] = X0; t[3] = X1; t[4] = X2; }
    s_pst[tid] = (unsigned char)st;
  }
  __syncthreads();
  // ---- observation threads: error and depth at the estimate, and the observation's state
  if (tid < nobs) {
    const int pst = s_pst[q];
    const double* x = s_term + qa * TRI_TERMS + 2;
    double e = 0.0, z = __builtin_inf();
    if (usable && pst == SBA_UNP_OK) e = tri_err(cp, x[0], x[1], x[2], u, v, z);
    s_term[tid * TRI_TERMS] = e;
    s_term[tid * TRI_TERMS + 1] = z;
    out.state[o_lo + tid] = pst == SBA_UNP_ANCHORED ? TRI_OBS_IN : (examined && !usable) ? TRI_OBS_UNUSABLE
                            : (usable && pst == SBA_UNP_OK) ? TRI_OBS_IN : TRI_OBS_OUT;
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
    double rms = nan, mx = nan;
    int nv = 0;
    if (st == SBA_UNP_OK) {
      const double* t = s_term + pa * TRI_TERMS;
      const double sq = t[5], zmin = t[7];
      mx = t[6];
      nv = nuse;
      rms = sqrt(sq / nuse);
      if (zmin <= 0.0) st = SBA_UNP_BEHIND;
    }
    out.X[3 * (size_t)p] = X0; out.X[3 * (size_t)p + 1] = X1; out.X[3 * (size_t)p + 2] = X2;
    out.status[p] = st; out.n_views[p] = nv;
    out.rms[p] = rms; out.mx[p] = mx;
  }
}

template <typename T>
int unp_run(const TriIn<T>& in, const sba_unp_opts& opt, const double* planes, int64_t n_planes, double* points_out, int32_t* status_out,
            int32_t* n_views_out, double* rms_out, double* max_out, uint8_t* used_out, sba_unp_report* rep, std::string& err) {
  const auto t_start = std::chrono::steady_clock::now();
  const int C = in.C, N = in.N;
  const int64_t M = in.M;
  if (!planes || (n_planes != 1 && n_planes != N)) { err = "sba_unproject: planes must hold 1 or n_points rows of (n, d)"; return SBA_ERR_INVALID; }
  if (!unp_planes_ok(planes, n_planes)) { err = "sba_unproject: a plane is not finite or its normal is zero"; return SBA_ERR_INVALID; }
  if (opt.use_ref_cam && (opt.ref_cam < 0 || opt.ref_cam >= C)) { err = "sba_unproject: ref_cam is out of range"; return SBA_ERR_INVALID; }
  const int min_views = opt.min_views <= 0 ? 1 : (int)opt.min_views;
  ArenaScope own(nullptr);          // private buffers: hipMalloc'd here, freed on return (the handle's arena stays as it was)
  hipStream_t st = in.stream;
  hipEvent_t ev[2];
  for (auto& e : ev) HIPCHK(hipEventCreate(&e));
  struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int k = 0; k < 2; ++k) (void)hipEventDestroy(e[k]); } } evg{ev};
  DevBuf<double> tab, pl, X, rms, mx;
  DevBuf<int32_t> status, nviews, perm32;
  DevBuf<unsigned char> state, state_out;
  tab.alloc((size_t)C * TRI_CAM);
  pl.alloc((size_t)n_planes * 4);
  X.alloc((size_t)N * 3); rms.alloc(N); mx.alloc(N); status.alloc(N); nviews.alloc(N); state.alloc(M);
  HIPCHK(hipMemcpyAsync(pl.p, planes, sizeof(double) * 4 * (size_t)n_planes, hipMemcpyHostToDevice, st));
  std::vector<int32_t> p32;                     // (staging of the permutation: lives until the synchronisation at the end)
  if (in.perm && M) {
    p32.resize((size_t)M);
    for (int64_t k = 0; k < M; ++k) p32[k] = (int32_t)in.perm[k];
    perm32.upload(p32, st);
    state_out.alloc(M);
  }
  UnpOut out{X.p, status.p, nviews.p, rms.p, mx.p, state.p};
  HIPCHK(hipEventRecord(ev[0], st));
  hipLaunchKernelGGL(k_tri_cam_prep, dim3((C + 63) / 64), dim3(64), 0, st, in.cams, tab.p, C);
  if (in.nblk > 0)
    hipLaunchKernelGGL(k_unp_plane_fit<T>, dim3(in.nblk), dim3(PM_BLOCK), (size_t)C * TRI_CAM * sizeof(double), st, tab.p, C, in.uv, in.w,
                       in.ci, in.pt_start, in.blk_desc, in.fixed, (const double*)in.pts, (const double*)pl.p, n_planes == N && N > 1 ? 4 : 0,
                       min_views, opt.use_ref_cam ? (int)opt.ref_cam : -1, out);
  HIPCHK(hipGetLastError());
  if (state_out.n)
    hipLaunchKernelGGL(k_tri_scatter, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, state.p, perm32.p, M, state_out.p);
  if (opt.write_back && N > 0)
    hipLaunchKernelGGL(k_tri_write_back<T>, dim3((3 * N + 255) / 256), dim3(256), 0, st, X.p, status.p, N, in.pts, in.ptsT);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ev[1], st));
  // ---- read-back into staging: the caller's arrays are written after the synchronisation only
  std::vector<int32_t> h_stat(N), h_nv(n_views_out ? N : 0);
  std::vector<unsigned char> h_state((size_t)M);
  std::vector<double> h_X(points_out ? (size_t)N * 3 : 0), h_rms(rms_out ? N : 0), h_mx(max_out ? N : 0);
  auto fetch = [&](void* dst, const void* src, size_t bytes) { if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st)); };
  fetch(h_stat.data(), status.p, sizeof(int32_t) * h_stat.size());
  fetch(h_state.data(), state_out.n ? state_out.p : state.p, h_state.size());
  fetch(h_X.data(), X.p, sizeof(double) * h_X.size());
  fetch(h_nv.data(), nviews.p, sizeof(int32_t) * h_nv.size());
  fetch(h_rms.data(), rms.p, sizeof(double) * h_rms.size());
  fetch(h_mx.data(), mx.p, sizeof(double) * h_mx.size());
  HIPCHK(hipStreamSynchronize(st));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
  if (points_out) std::copy(h_X.begin(), h_X.end(), points_out);
  if (status_out) std::copy(h_stat.begin(), h_stat.end(), status_out);
  if (n_views_out) std::copy(h_nv.begin(), h_nv.end(), n_views_out);
  if (rms_out) std::copy(h_rms.begin(), h_rms.end(), rms_out);
  if (max_out) std::copy(h_mx.begin(), h_mx.end(), max_out);
  if (used_out) for (int64_t k = 0; k < M; ++k) used_out[k] = h_state[k] == TRI_OBS_IN ? 1 : 0;
  if (rep) {
    *rep = sba_unp_report{};
    for (int p = 0; p < N; ++p) {
      const int s = h_stat[p];
      (s == SBA_UNP_OK ? rep->n_ok : s == SBA_UNP_ANCHORED ? rep->n_anchored : s == SBA_UNP_NO_VIEW ? rep->n_no_view
       : s == SBA_UNP_DEGENERATE ? rep->n_degenerate : rep->n_behind)++;
    }
    for (int64_t k = 0; k < M; ++k) { rep->n_obs_unusable += h_state[k] == TRI_OBS_UNUSABLE; rep->n_obs_used += h_state[k] == TRI_OBS_IN; }
    rep->seconds_device = ms * 1e-3;
    rep->seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
  }
  return SBA_OK;
}

}  // namespace SBA_NS
