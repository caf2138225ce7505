// sba_align / sba_apply_similarity (include/sba_hip.h): the similarity dst ~ s R src + t between the handle's current points and
// camera centres and caller-given targets (Umeyama / Horn), and its application to every camera and point of the handle.
// Always float64.  Kernels:
//   k_align_means         one thread per correspondence (points first, the camera centres as last short block): w, w src, w dst,
//                         the counts and the bad-weight / bad-target flags, one partial record per workgroup
//   k_align_sums          second pass over centred values: H = sum w b a^T, v_a, v_b
//   k_align_stats         third pass at the estimate: sum w |dst - src|^2, sum w |dst - (s R src + t)|^2, the largest distance
//   k_align_fold          one workgroup: the partial records added in index order (no floating-point atomics: same bits every call)
//   k_align_apply_points  one thread per point: X <- s R X + t into both precisions
//   k_align_apply_cams    one thread per camera: rho' from q(rho) q(R)^-1, t' = s t - R(rho') t
// The rotation itself is found on the host (cyclic Jacobi on Horn's 4 x 4 matrix) from the 22 doubles read back after the second
// pass: the record of the first pass (W, the two weighted sums for the means, the counts, the flags) and H, v_a, v_b.
#pragma once
#include "sba_kernels.hpp"

namespace SBA_NS {
using namespace sba_host;

constexpr int ALN_BLOCK = 256;
constexpr int ALN_WAVES = ALN_BLOCK / 64;
// record layouts (sums first, then maxima)
constexpr int ALN1_SUM = 9, ALN1_MAX = 2;     // W, w src[3], w dst[3], points used, cameras used | bad weight, bad target
constexpr int ALN2_SUM = 11, ALN2_MAX = 0;    // H[9] row-major, v_a, v_b
constexpr int ALN3_SUM = 2, ALN3_MAX = 1;     // w |dst - src|^2, w |dst - (s R src + t)|^2 | largest distance after
constexpr int ALN_REC = 11;                   // longest record
constexpr int ALN_TOT1 = 0, ALN_TOT2 = 11, ALN_TOT3 = 22, ALN_TOT = 25;

struct AlignSrc {
  const double *pts, *cams;      // the handle's current points (N x 3) and camera rows (C x NCP)
  const double *tp, *pw;         // target points / weights (pw may be NULL = ones); tp NULL: nbp == 0
  const double *tc, *cw;         // target centres / weights
  int N, C, nbp;                 // nbp: workgroups over the points; the workgroups after them take the cameras
};
struct AlignSim { double s, R[9], t[3], q[4]; };      // q = (w, x, y, z) of R, w >= 0

// centre -R(rho)^T t of one camera row
__device__ __forceinline__ void align_centre(const double* __restrict__ cam, double (&c)[3]) {
  double cp[CAMPRE];
  campre_build<double>(cam, cp);
  const double t0 = cp[CP_T], t1 = cp[CP_T + 1], t2 = cp[CP_T + 2];
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = -(cp[CP_R + k] * t0 + cp[CP_R + 3 + k] * t1 + cp[CP_R + 6 + k] * t2);
}

// The correspondence of this thread.  w == 0: not in use (past the end, zero weight, or flagged), a and b are zero then.
// bad: 1 a weight that is negative or not finite, 2 a target that is not finite under a positive weight.
__device__ __forceinline__ void align_load(const AlignSrc& in, double& w, double (&a)[3], double (&b)[3], bool& is_cam, int& bad) {
  w = 0.0; bad = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) { a[k] = 0.0; b[k] = 0.0; }
  is_cam = (int)blockIdx.x >= in.nbp;
  const int i = (is_cam ? (int)blockIdx.x - in.nbp : (int)blockIdx.x) * ALN_BLOCK + (int)threadIdx.x;
  if (i >= (is_cam ? in.C : in.N)) return;
  const double* wp = is_cam ? in.cw : in.pw;
  const double* dp = (is_cam ? in.tc : in.tp) + (size_t)i * 3;
  const double ww = wp ? wp[i] : 1.0;
  if (!(ww >= 0.0) || !isfinite(ww)) { bad = 1; return; }
  if (ww == 0.0) return;
  const double d0 = dp[0], d1 = dp[1], d2 = dp[2];
  if (!isfinite(d0) || !isfinite(d1) || !isfinite(d2)) { bad = 2; return; }
  if (is_cam) align_centre(in.cams + (size_t)i * NCP, a);
  else {
    const double* sp = in.pts + (size_t)i * 3;
    a[0] = sp[0]; a[1] = sp[1]; a[2] = sp[2];
  }
  b[0] = d0; b[1] = d1; b[2] = d2;
  w = ww;
}

// v[0 .. NS) summed and v[NS .. NS + NM) maximised over the workgroup (in the wave, then across the waves through LDS in wave
// order); entry k goes to part[k * nb + blockIdx.x].  Every thread of the workgroup must call it.
template <int NS, int NM>
__device__ __forceinline__ void align_block_reduce(double (&v)[NS + NM], double* __restrict__ part, int nb) {
  __shared__ double red[ALN_WAVES][NS + NM];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NS + NM; ++k) {
    const double r = k < NS ? wave_sum(v[k]) : wave_max(v[k]);
    if (lane == 0) red[wid][k] = r;
  }
  __syncthreads();
  if (threadIdx.x < NS + NM) {
    const int k = threadIdx.x;
    double r = red[0][k];
    for (int q = 1; q < ALN_WAVES; ++q) r = k < NS ? r + red[q][k] : fmax(r, red[q][k]);
    part[(size_t)k * nb + blockIdx.x] = r;
  }
}

__global__ void __launch_bounds__(ALN_BLOCK) k_align_means(AlignSrc in, double* __restrict__ part, int nb) {
  double w, a[3], b[3];
  bool is_cam; int bad;
  align_load(in, w, a, b, is_cam, bad);
  double v[ALN1_SUM + ALN1_MAX];
  v[0] = w;
#pragma unroll
  for (int k = 0; k < 3; ++k) { v[1 + k] = w * a[k]; v[4 + k] = w * b[k]; }
  v[7] = (w > 0.0 && !is_cam) ? 1.0 : 0.0;
  v[8] = (w > 0.0 && is_cam) ? 1.0 : 0.0;
  v[9] = bad == 1 ? 1.0 : 0.0;
  v[10] = bad == 2 ? 1.0 : 0.0;
  align_block_reduce<ALN1_SUM, ALN1_MAX>(v, part, nb);
}

__global__ void __launch_bounds__(ALN_BLOCK) k_align_sums(AlignSrc in, const double* __restrict__ tot1, double* __restrict__ part, int nb) {
  double w, a[3], b[3];
  bool is_cam; int bad;
  align_load(in, w, a, b, is_cam, bad);
  const double W = tot1[0];
  double v[ALN2_SUM];
  if (w > 0.0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { a[k] -= tot1[1 + k] / W; b[k] -= tot1[4 + k] / W; }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) v[3 * i + j] = w * b[i] * a[j];
  v[9] = w * (a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  v[10] = w * (b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
  align_block_reduce<ALN2_SUM, ALN2_MAX>(v, part, nb);
}

__device__ __forceinline__ void align_map(const AlignSim& sim, const double (&x)[3], double (&y)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) y[k] = sim.s * (sim.R[3 * k] * x[0] + sim.R[3 * k + 1] * x[1] + sim.R[3 * k + 2] * x[2]) + sim.t[k];
}

__global__ void __launch_bounds__(ALN_BLOCK) k_align_stats(AlignSrc in, AlignSim sim, double* __restrict__ part, int nb) {
  double w, a[3], b[3];
  bool is_cam; int bad;
  align_load(in, w, a, b, is_cam, bad);
  double v[ALN3_SUM + ALN3_MAX] = {0.0, 0.0, 0.0};
  if (w > 0.0) {
    double y[3];
    align_map(sim, a, y);
    double d0 = 0.0, d1 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) { d0 += (b[k] - a[k]) * (b[k] - a[k]); d1 += (b[k] - y[k]) * (b[k] - y[k]); }
    v[0] = w * d0; v[1] = w * d1; v[2] = sqrt(d1);
  }
  align_block_reduce<ALN3_SUM, ALN3_MAX>(v, part, nb);
}

// second stage: thread k adds (or maximises) entry k of the nb partial records in index order
__global__ void __launch_bounds__(64) k_align_fold(const double* __restrict__ part, int nb, int ns, int nm, double* __restrict__ out) {
  const int k = threadIdx.x;
  if (k >= ns + nm) return;
  const double* p = part + (size_t)k * nb;
  double r = p[0];
  if (k < ns) for (int i = 1; i < nb; ++i) r += p[i];
  else for (int i = 1; i < nb; ++i) r = fmax(r, p[i]);
  out[k] = r;
}

template <typename T>
__global__ void __launch_bounds__(256) k_align_apply_points(AlignSim sim, int N, double* __restrict__ pts, T* __restrict__ ptsT) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= N) return;
  double* X = pts + (size_t)p * 3;
  const double x[3] = {X[0], X[1], X[2]};
  double y[3];
  align_map(sim, x, y);
#pragma unroll
  for (int k = 0; k < 3; ++k) { X[k] = y[k]; ptsT[(size_t)p * 3 + k] = (T)y[k]; }
}

// R(rho') = R(rho) R^T through quaternions (well conditioned at theta -> 0 and theta -> pi), t' = s t_c - R(rho') t
__global__ void __launch_bounds__(64) k_align_apply_cams(AlignSim sim, int C, double* __restrict__ cams) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double* cam = cams + (size_t)c * NCP;
  const double r0 = cam[0], r1 = cam[1], r2 = cam[2];
  const double th2 = r0 * r0 + r1 * r1 + r2 * r2;
  double pw, ph;                           // q(rho) = (cos(theta/2), sin(theta/2)/theta rho)
  if (th2 < 1e-8) { pw = 1.0 - th2 * (1.0 / 8 - th2 * (1.0 / 384)); ph = 0.5 - th2 * (1.0 / 48 - th2 * (1.0 / 3840)); }
  else {
    const double th = sqrt(th2);
    double sn, cs;
    sincos(0.5 * th, &sn, &cs);
    pw = cs; ph = sn / th;
  }
  const double px = ph * r0, py = ph * r1, pz = ph * r2;
  const double qw = sim.q[0], qx = -sim.q[1], qy = -sim.q[2], qz = -sim.q[3];      // q(R)^-1
  double w = pw * qw - px * qx - py * qy - pz * qz;
  double x = pw * qx + px * qw + py * qz - pz * qy;
  double y = pw * qy - px * qz + py * qw + pz * qx;
  double z = pw * qz + px * qy - py * qx + pz * qw;
  const double inv = 1.0 / sqrt(w * w + x * x + y * y + z * z);
  w *= inv; x *= inv; y *= inv; z *= inv;
  if (w < 0.0) { w = -w; x = -x; y = -y; z = -z; }
  const double vn = sqrt(x * x + y * y + z * z);
  const double f = vn < 1e-12 ? 2.0 : 2.0 * atan2(vn, w) / vn;
  // rotation matrix of the unit quaternion
  const double R00 = 1.0 - 2.0 * (y * y + z * z), R01 = 2.0 * (x * y - w * z), R02 = 2.0 * (x * z + w * y);
  const double R10 = 2.0 * (x * y + w * z), R11 = 1.0 - 2.0 * (x * x + z * z), R12 = 2.0 * (y * z - w * x);
  const double R20 = 2.0 * (x * z - w * y), R21 = 2.0 * (y * z + w * x), R22 = 1.0 - 2.0 * (x * x + y * y);
  const double t0 = cam[3], t1 = cam[4], t2 = cam[5];
  cam[0] = f * x; cam[1] = f * y; cam[2] = f * z;
  cam[3] = sim.s * t0 - (R00 * sim.t[0] + R01 * sim.t[1] + R02 * sim.t[2]);
  cam[4] = sim.s * t1 - (R10 * sim.t[0] + R11 * sim.t[1] + R12 * sim.t[2]);
  cam[5] = sim.s * t2 - (R20 * sim.t[0] + R21 * sim.t[1] + R22 * sim.t[2]);
}

// ------------------------------------------------------------------ host: the rotation from the sums
// cyclic Jacobi on a symmetric 4 x 4 matrix: A becomes diagonal, the columns of V are the eigenvectors
inline void align_jacobi4(double (&A)[4][4], double (&V)[4][4]) {
  for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0, dia = 0.0;
    for (int i = 0; i < 4; ++i) { dia += A[i][i] * A[i][i]; for (int j = i + 1; j < 4; ++j) off += A[i][j] * A[i][j]; }
    if (off <= 1e-36 * dia || off == 0.0) break;
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        if (std::fabs(A[p][q]) < 1e-300) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 4; ++k) { const double x = A[k][p], y = A[k][q]; A[k][p] = c * x - s * y; A[k][q] = s * x + c * y; }
        for (int k = 0; k < 4; ++k) { const double x = A[p][k], y = A[q][k]; A[p][k] = c * x - s * y; A[q][k] = s * x + c * y; }
        for (int k = 0; k < 4; ++k) { const double x = V[k][p], y = V[k][q]; V[k][p] = c * x - s * y; V[k][q] = s * x + c * y; }
      }
  }
}

// singular values of a 3 x 3 matrix, descending: one-sided Jacobi on its columns (small ones keep their relative accuracy)
inline void align_sv3(const double* H, double (&sv)[3]) {
  double G[3][3];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) G[i][j] = H[3 * i + j];
  for (int sweep = 0; sweep < 64; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double al = 0.0, be = 0.0, ga = 0.0;
        for (int k = 0; k < 3; ++k) { al += G[k][p] * G[k][p]; be += G[k][q] * G[k][q]; ga += G[k][p] * G[k][q]; }
        if (ga == 0.0 || std::fabs(ga) <= 1e-17 * std::sqrt(al * be)) continue;
        rotated = true;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(zeta * zeta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; ++k) { const double x = G[k][p], y = G[k][q]; G[k][p] = c * x - s * y; G[k][q] = s * x + c * y; }
      }
    if (!rotated) break;
  }
  for (int j = 0; j < 3; ++j) sv[j] = std::sqrt(G[0][j] * G[0][j] + G[1][j] * G[1][j] + G[2][j] * G[2][j]);
  std::sort(sv, sv + 3, [](double x, double y) { return x > y; });
}

inline void align_quat_to_R(const double* q, double* R) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z); R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z); R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y); R[7] = 2.0 * (y * z + w * x); R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// unit quaternion (w >= 0) of a rotation matrix: the largest of the four candidates is the pivot (Shepperd)
inline void align_R_to_quat(const double* R, double* q) {
  const double tr = R[0] + R[4] + R[8];
  const double c[4] = {1.0 + tr, 1.0 + R[0] - R[4] - R[8], 1.0 - R[0] + R[4] - R[8], 1.0 - R[0] - R[4] + R[8]};
  int m = 0;
  for (int k = 1; k < 4; ++k) if (c[k] > c[m]) m = k;
  if (m == 0) { q[0] = c[0]; q[1] = R[7] - R[5]; q[2] = R[2] - R[6]; q[3] = R[3] - R[1]; }
  else if (m == 1) { q[0] = R[7] - R[5]; q[1] = c[1]; q[2] = R[1] + R[3]; q[3] = R[2] + R[6]; }
  else if (m == 2) { q[0] = R[2] - R[6]; q[1] = R[1] + R[3]; q[2] = c[2]; q[3] = R[5] + R[7]; }
  else { q[0] = R[3] - R[1]; q[1] = R[2] + R[6]; q[2] = R[5] + R[7]; q[3] = c[3]; }
  const double nrm = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double sg = q[0] < 0.0 ? -1.0 / nrm : 1.0 / nrm;
  for (int k = 0; k < 4; ++k) q[k] *= sg;
}

// The estimate from the folded records of the first two passes (h: ALN_TOT1 and ALN_TOT2 records): the refusals, the singular
// values of H, the rotation as eigenvector of Horn's matrix, scale and translation.  Host only; nothing is launched.
inline int align_estimate(const double* h, bool with_scale, AlignSim& sim, double (&sv)[3], std::string& err) {
  if (h[9] > 0.0) { err = "sba_align: a weight is negative or not finite"; return SBA_ERR_INVALID; }
  if (h[10] > 0.0) { err = "sba_align: a target is not finite where its weight is positive"; return SBA_ERR_INVALID; }
  const int64_t n_pts = (int64_t)h[7];
  const int n_cams = (int)h[8];
  if (n_pts + n_cams < 3) { err = "sba_align: fewer than 3 correspondences are in use"; return SBA_ERR_INVALID; }
  const double W = h[0];
  const double* H = h + ALN_TOT2;
  const double va = h[ALN_TOT2 + 9];
  for (int k = 0; k < ALN_TOT3; ++k)
    if (!std::isfinite(h[k])) { err = "sba_align: the sums are not finite (the handle's parameters or the weights overflow)"; return SBA_ERR_INVALID; }
  align_sv3(H, sv);
  const double detH = H[0] * (H[4] * H[8] - H[5] * H[7]) - H[1] * (H[3] * H[8] - H[5] * H[6]) + H[2] * (H[3] * H[7] - H[4] * H[6]);
  const double d = detH < 0.0 ? -1.0 : 1.0;
  if (!(sv[1] + d * sv[2] > 1e-10 * sv[0])) {
    err = "sba_align: the rotation is not unique (collinear or coincident correspondences: s2 + d s3 <= 1e-10 s1)";
    return SBA_ERR_INVALID;
  }
  // Horn's matrix from S = sum w a b^T = H^T
  const double Sxx = H[0], Sxy = H[3], Sxz = H[6], Syx = H[1], Syy = H[4], Syz = H[7], Szx = H[2], Szy = H[5], Szz = H[8];
  double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                    {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                    {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                    {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
  double V[4][4];
  align_jacobi4(A, V);
  int m = 0;
  for (int k = 1; k < 4; ++k) if (A[k][k] > A[m][m]) m = k;
  double qn = 0.0;
  for (int k = 0; k < 4; ++k) { sim.q[k] = V[k][m]; qn += sim.q[k] * sim.q[k]; }
  qn = (sim.q[0] < 0.0 ? -1.0 : 1.0) / std::sqrt(qn);
  for (int k = 0; k < 4; ++k) sim.q[k] *= qn;
  align_quat_to_R(sim.q, sim.R);
  double trRtH = 0.0;
  for (int k = 0; k < 9; ++k) trRtH += sim.R[k] * H[k];
  if (with_scale && !(va > 0.0)) { err = "sba_align: the source correspondences coincide (no scale)"; return SBA_ERR_INVALID; }
  sim.s = with_scale ? trRtH / va : 1.0;
  if (!(sim.s > 0.0) || !std::isfinite(sim.s)) { err = "sba_align: the estimated scale is not positive"; return SBA_ERR_INVALID; }
  double ms[3], md[3];
  for (int k = 0; k < 3; ++k) { ms[k] = h[1 + k] / W; md[k] = h[4 + k] / W; }
  for (int k = 0; k < 3; ++k) sim.t[k] = md[k] - sim.s * (sim.R[3 * k] * ms[0] + sim.R[3 * k + 1] * ms[1] + sim.R[3 * k + 2] * ms[2]);
  return SBA_OK;
}

// what the engine hands over: its current parameters, all device pointers
template <typename T>
struct AlignIn {
  hipStream_t stream;
  int C, N;
  double *cams, *pts;
  T *ptsT, *campre;
};

// X <- s R X + t for every point, the cameras to match, the CamPre table: the state sba_set_params leaves for those values
template <typename T>
void align_apply(const AlignIn<T>& in, const AlignSim& sim) {
  hipStream_t st = in.stream;
  if (in.N > 0) hipLaunchKernelGGL(k_align_apply_points<T>, dim3((in.N + 255) / 256), dim3(256), 0, st, sim, in.N, in.pts, in.ptsT);
  if (in.C > 0) {
    hipLaunchKernelGGL(k_align_apply_cams, dim3((in.C + 63) / 64), dim3(64), 0, st, sim, in.C, in.cams);
    hipLaunchKernelGGL(k_cam_prep<T>, dim3((in.C + 63) / 64), dim3(64), 0, st, (const double*)in.cams, in.campre, in.C);
  }
  HIPCHK(hipGetLastError());
}

template <typename T>
int align_apply_run(const AlignIn<T>& in, double scale, const double* R, const double* t, std::string& err) {
  if (!R || !t) { err = "sba_apply_similarity: null argument"; return SBA_ERR_INVALID; }
  if (!(scale > 0.0) || !std::isfinite(scale)) { err = "sba_apply_similarity: scale must be positive and finite"; return SBA_ERR_INVALID; }
  double dev = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double g = 0.0;
      for (int k = 0; k < 3; ++k) g += R[3 * k + i] * R[3 * k + j];
      dev = std::fmax(dev, std::fabs(g - (i == j ? 1.0 : 0.0)));
      if (!std::isfinite(g)) dev = INFINITY;
    }
  if (!(dev <= 1e-9)) { err = "sba_apply_similarity: R is not orthogonal (max |R^T R - I| exceeds 1e-9)"; return SBA_ERR_INVALID; }
  const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
  if (det < 0.0) { err = "sba_apply_similarity: R is a reflection (det R < 0)"; return SBA_ERR_INVALID; }
  for (int k = 0; k < 3; ++k) if (!std::isfinite(t[k])) { err = "sba_apply_similarity: t is not finite"; return SBA_ERR_INVALID; }
  AlignSim sim;
  sim.s = scale;
  for (int k = 0; k < 9; ++k) sim.R[k] = R[k];
  for (int k = 0; k < 3; ++k) sim.t[k] = t[k];
  align_R_to_quat(R, sim.q);
  align_apply<T>(in, sim);
  HIPCHK(hipStreamSynchronize(in.stream));
  return SBA_OK;
}

template <typename T>
int align_run(const AlignIn<T>& in, const sba_align_opts& opt, const double* target_points, const double* point_weights,
              const double* target_centres, const double* centre_weights, sba_align_report* rep, std::string& err) {
  const auto t_start = std::chrono::steady_clock::now();
  ArenaScope own(nullptr);          // private buffers: hipMalloc'd here, freed on return (the handle's arena stays as it was)
  hipStream_t st = in.stream;
  const int C = in.C, N = in.N;
  const int nbp = target_points ? (N + ALN_BLOCK - 1) / ALN_BLOCK : 0;
  const int nbc = target_centres ? (C + ALN_BLOCK - 1) / ALN_BLOCK : 0;
  const int nb = nbp + nbc;
  if (nb == 0) { err = "sba_align: fewer than 3 correspondences are in use (no targets given)"; return SBA_ERR_INVALID; }
  DevEvents<4> ev;
  DevBuf<double> d_tp, d_pw, d_tc, d_cw, part, tot;
  auto up = [&](DevBuf<double>& b, const double* src, size_t cnt) {
    if (!src || !cnt) return;
    b.alloc(cnt);
    HIPCHK(hipMemcpyAsync(b.p, src, sizeof(double) * cnt, hipMemcpyHostToDevice, st));
  };
  if (nbp) { up(d_tp, target_points, (size_t)N * 3); up(d_pw, point_weights, N); }
  if (nbc) { up(d_tc, target_centres, (size_t)C * 3); up(d_cw, centre_weights, C); }
  part.alloc((size_t)nb * ALN_REC);
  tot.alloc(ALN_TOT);
  const AlignSrc src{in.pts, in.cams, d_tp.p, d_pw.p, d_tc.p, d_cw.p, N, C, nbp};
  double h[ALN_TOT] = {};
  // ---- [ev0, ev1): the two passes of the estimator
  HIPCHK(hipEventRecord(ev[0], st));
  hipLaunchKernelGGL(k_align_means, dim3(nb), dim3(ALN_BLOCK), 0, st, src, part.p, nb);
  hipLaunchKernelGGL(k_align_fold, dim3(1), dim3(64), 0, st, (const double*)part.p, nb, ALN1_SUM, ALN1_MAX, tot.p + ALN_TOT1);
  hipLaunchKernelGGL(k_align_sums, dim3(nb), dim3(ALN_BLOCK), 0, st, src, (const double*)(tot.p + ALN_TOT1), part.p, nb);
  hipLaunchKernelGGL(k_align_fold, dim3(1), dim3(64), 0, st, (const double*)part.p, nb, ALN2_SUM, ALN2_MAX, tot.p + ALN_TOT2);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ev[1], st));
  HIPCHK(hipMemcpyAsync(h, tot.p, sizeof(double) * ALN_TOT3, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  // ---- refusals and the estimate (nothing of the handle has been written yet)
  AlignSim sim;
  double sv[3];
  if (int rc = align_estimate(h, opt.with_scale != 0, sim, sv, err)) return rc;
  const double W = h[0];
  const int64_t n_pts = (int64_t)h[7];
  const int n_cams = (int)h[8];
  // ---- [ev2, ev3): the third pass and the application
  HIPCHK(hipEventRecord(ev[2], st));
  hipLaunchKernelGGL(k_align_stats, dim3(nb), dim3(ALN_BLOCK), 0, st, src, sim, part.p, nb);
  hipLaunchKernelGGL(k_align_fold, dim3(1), dim3(64), 0, st, (const double*)part.p, nb, ALN3_SUM, ALN3_MAX, tot.p + ALN_TOT3);
  HIPCHK(hipGetLastError());
  if (opt.apply) align_apply<T>(in, sim);
  HIPCHK(hipEventRecord(ev[3], st));
  HIPCHK(hipMemcpyAsync(h + ALN_TOT3, tot.p + ALN_TOT3, sizeof(double) * (ALN_TOT - ALN_TOT3), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (rep) {
    const float m0 = ev.ms(0, 1), m1 = ev.ms(2, 3);
    *rep = sba_align_report{};
    rep->scale = sim.s;
    for (int k = 0; k < 9; ++k) rep->R[k] = sim.R[k];
    for (int k = 0; k < 3; ++k) { rep->t[k] = sim.t[k]; rep->sv[k] = sv[k]; }
    rep->rms_before = std::sqrt(h[ALN_TOT3] / W);
    rep->rms_after = std::sqrt(h[ALN_TOT3 + 1] / W);
    rep->max_after = h[ALN_TOT3 + 2];
    rep->n_points_used = n_pts;
    rep->n_cams_used = n_cams;
    rep->seconds_device = (m0 + m1) * 1e-3;
    rep->seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
  }
  return SBA_OK;
}

}  // namespace SBA_NS
