// sba_unproject.hpp -- the inverse camera model (sba_unproject_rows, sba_unproject; include/sba_hip.h): a pixel becomes a ray
// (the Newton inversion and the ray of sba_triangulate.hpp), and a ray or the rays of a point meet a known plane n . X = d.
// Everything here is float64 whatever the handle's dtype, runs on private buffers freed on return and touches no LM kernel, no
// LM state and no route.
//
// sba_unproject_rows (stateless, gathered rows):
//   k_unp_rows        one row per lane: the row's table entry (tri_cam_row), undistorted coordinates, origin, direction and the
//                     intersection with the row's plane
// sba_unproject (one stream, one synchronisation at the end; unp_run on the RayFitJob of sba_triangulate.hpp):
//   k_tri_cam_prep    the camera table of sba_triangulate.hpp
//   k_ray_fit<UnpFit> the per-point kernel of sba_triangulate.hpp with the fit of this file: the rays of every camera or of the
//                     reference camera alone, and one thread per point reduces A, b to the plane's 2 x 2 system and solves it
//   k_tri_scatter     per-observation flags from the layout's order to the caller's
//   k_tri_write_back  opts->write_back: the estimates of the OK points into the handle's current points
#pragma once
#include "sba_triangulate.hpp"

namespace SBA_NS {

constexpr double UNP_PARALLEL = 1e-6;          // |nh . dir| at or below it: the ray runs along the plane (sba_unproject_rows)
constexpr int64_t UNP_ROWS_CHUNK = 1 << 20;    // rows per launch of k_unp_rows
static_assert((int)SBA_UNP_OK == RAY_OK && (int)SBA_UNP_ANCHORED == RAY_ANCHORED && (int)SBA_UNP_BEHIND == RAY_BEHIND,
              "k_ray_fit sets these three for every fit; k_tri_write_back moves the points of status 0");

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
  // (tri_ray runs the same inversion again: the direction has the bits k_ray_fit works with)
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

// The fit of the un-projection (a policy of k_ray_fit; TriFit of sba_triangulate.hpp lists the members): the point of the
// point's plane closest to the rays by unp_solve, from every camera or from the reference camera alone; no direction sum and
// no output beyond the shared ones.
struct UnpFit {
  static constexpr int NE = 11, COL_USABLE = 9, COL_FIRST = 10;
  static constexpr bool DIRS = false;
  static constexpr int ST_TOO_FEW = SBA_UNP_NO_VIEW, ST_DEGENERATE = SBA_UNP_DEGENERATE;
  const double* planes;
  int plane_stride;      // 0: one plane for every point, 4: one per point
  int ref_cam;           // < 0: every camera
  __device__ __forceinline__ bool examined(int c) const { return ref_cam < 0 || c == ref_cam; }
  __device__ __forceinline__ bool solve(int p, const double* __restrict__ t, double& X0, double& X1, double& X2) const {
    double n0, n1, n2, dh;
    unp_plane(planes + (size_t)plane_stride * p, n0, n1, n2, dh);
    return unp_solve(t, t + 6, n0, n1, n2, dh, X0, X1, X2);
  }
  __device__ __forceinline__ void finish(int, bool, int, double, const double*, const RayOut&) const {}
};

template <typename T>
int unp_run(const TriIn<T>& in, const sba_unp_opts& opt, const double* planes, int64_t n_planes, double* points_out, int32_t* status_out,
            int32_t* n_views_out, double* rms_out, double* max_out, uint8_t* used_out, sba_unp_report* rep, std::string& err) {
  const auto t_start = std::chrono::steady_clock::now();
  const int C = in.C, N = in.N;
  if (!planes || (n_planes != 1 && n_planes != N)) { err = "sba_unproject: planes must hold 1 or n_points rows of (n, d)"; return SBA_ERR_INVALID; }
  if (!unp_planes_ok(planes, n_planes)) { err = "sba_unproject: a plane is not finite or its normal is zero"; return SBA_ERR_INVALID; }
  if (opt.use_ref_cam && (opt.ref_cam < 0 || opt.ref_cam >= C)) { err = "sba_unproject: ref_cam is out of range"; return SBA_ERR_INVALID; }
  const int min_views = opt.min_views <= 0 ? 1 : (int)opt.min_views;
  hipStream_t st = in.stream;
  RayFitJob<T> job(in);
  DevEvents<2> ev;
  DevBuf<double> pl;
  pl.alloc((size_t)n_planes * 4);
  HIPCHK(hipMemcpyAsync(pl.p, planes, sizeof(double) * 4 * (size_t)n_planes, hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(ev[0], st));
  job.fit(min_views, UnpFit{pl.p, n_planes == N && N > 1 ? 4 : 0, opt.use_ref_cam ? (int)opt.ref_cam : -1}, job.out(nullptr, nullptr, nullptr));
  job.flags_and_write_back(opt.write_back != 0);
  HIPCHK(hipEventRecord(ev[1], st));
  // ---- read-back into staging: the caller's arrays are written after the synchronisation only
  std::vector<int32_t> h_nv(n_views_out ? N : 0);
  std::vector<double> h_X(points_out ? (size_t)N * 3 : 0), h_rms(rms_out ? N : 0), h_mx(max_out ? N : 0);
  job.read_back();
  job.fetch(h_X.data(), job.X.p, sizeof(double) * h_X.size());
  job.fetch(h_nv.data(), job.nviews.p, sizeof(int32_t) * h_nv.size());
  job.fetch(h_rms.data(), job.rms.p, sizeof(double) * h_rms.size());
  job.fetch(h_mx.data(), job.mx.p, sizeof(double) * h_mx.size());
  HIPCHK(hipStreamSynchronize(st));
  const float ms = ev.ms(0, 1);
  if (points_out) std::copy(h_X.begin(), h_X.end(), points_out);
  if (n_views_out) std::copy(h_nv.begin(), h_nv.end(), n_views_out);
  if (rms_out) std::copy(h_rms.begin(), h_rms.end(), rms_out);
  if (max_out) std::copy(h_mx.begin(), h_mx.end(), max_out);
  job.deliver(status_out, used_out);
  if (rep) {
    *rep = sba_unp_report{};
    rep->n_ok = job.n_status[SBA_UNP_OK]; rep->n_anchored = job.n_status[SBA_UNP_ANCHORED]; rep->n_no_view = job.n_status[SBA_UNP_NO_VIEW];
    rep->n_degenerate = job.n_status[SBA_UNP_DEGENERATE]; rep->n_behind = job.n_status[SBA_UNP_BEHIND];
    rep->n_obs_unusable = job.n_state[TRI_OBS_UNUSABLE]; rep->n_obs_used = job.n_state[TRI_OBS_IN];
    rep->seconds_device = ms * 1e-3;
    rep->seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
  }
  return SBA_OK;
}

}  // namespace SBA_NS
