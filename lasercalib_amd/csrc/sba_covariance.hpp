// sba_covariance.hpp -- Gauss-Newton covariance of the cameras and points at the handle's current parameters (sba_covariance,
// include/sba_hip.h).  Everything here is float64 whatever the handle's dtype, runs on private buffers freed on return, and
// never touches the LM state, the LM work buffers or the LM factorisation kernels.
//
// Pipeline (one stream):
//   k_cam_prep<double>      CamPre rows in f64 from the current camera parameters
//   k_cov_lin               one thread per point: residual + Jacobian blocks of its observations (obs_resjac, weights, IRLS
//                           scaling), V_p, its Cholesky factor L_p, and per (point, camera) slot G = W L_p^-T (P x 3); the
//                           observations' camera blocks J_c for the camera diagonal
//   k_cov_schur             one workgroup per camera pair (a >= b): S_ab = [a == b] sum J_c^T J_c - sum_p G_pa G_pb^T, undamped
//   k_cov_matq / _stats / _reg    S Q, ||S||, ||S Q||, alpha = mean diag S; S + alpha Q Q^T and the identity padding
//   k_cov_potrf_diag / _trsm / _syrk   right-looking tiled Cholesky (32 x 32 tiles, one launch triple per tile column)
//   k_cov_mirror, k_cov_inv  L^T into the upper triangle; one workgroup per column of the inverse (forward + back substitution)
//   k_cov_matq / _gram / _project   P X P with P = I - Q Q^T (free gauge only)
//   k_cov_blocks, k_cov_points     the camera diagonal blocks; Sigma_pp = V^-1 + L^-T (sum G^T X G) L^-1 per point
#pragma once
#include "sba_kernels.hpp"

namespace SBA_NS {
using namespace sba_host;

constexpr int COV_NB = 32;          // tile of the dense factorisation
constexpr int COV_INV_Q = 7;        // rows per thread of k_cov_inv: n_pad <= 7 * 256 = 1792 (128 cameras x 13 = 1664)
constexpr int COV_G = 7;            // similarity gauge: 3 rotation + 3 translation + 1 scale

// point status written by k_cov_lin
constexpr int COV_PT_OK = 0, COV_PT_ANCHORED = 1, COV_PT_DEGENERATE = 2;

// ------------------------------------------------------------------ per-point linearisation at lambda = 0
template <typename T>
__global__ void __launch_bounds__(128) k_cov_lin(const double* __restrict__ campre, const double* __restrict__ pts,
                                                 const typename Vec2<T>::type* __restrict__ uv, const T* __restrict__ w,
                                                 const int32_t* __restrict__ pt_start, const int32_t* __restrict__ ci,
                                                 const int32_t* __restrict__ obs_slot, const int32_t* __restrict__ slot_start,
                                                 const unsigned char* __restrict__ fixed, RLoss<double> loss, int N,
                                                 double* __restrict__ Jc_o, double* __restrict__ G, double* __restrict__ Linv,
                                                 int* __restrict__ pstat, double* __restrict__ cost_pt) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= N) return;
  const int s0 = slot_start[p], s1 = slot_start[p + 1];
  const int o0 = pt_start[p], o1 = pt_start[p + 1];
  const bool anchored = fixed != nullptr && fixed[p] != 0;
  bool degenerate = !anchored && (s1 - s0 < 2);
  for (size_t e = (size_t)s0 * NCP * 3; e < (size_t)s1 * NCP * 3; ++e) G[e] = 0.0;
  double V00 = 0, V10 = 0, V11 = 0, V20 = 0, V21 = 0, V22 = 0, cost = 0;
  const double X0 = pts[3 * (size_t)p], X1 = pts[3 * (size_t)p + 1], X2 = pts[3 * (size_t)p + 2];
  for (int o = o0; o < o1; ++o) {
    const int c = ci[o];
    double r[2], Jc[2][NCP], Jp[2][3];
    const auto q = uv[o];
    obs_resjac<double>(campre + (size_t)c * CAMPRE, X0, X1, X2, (double)q.x, (double)q.y, w ? (double)w[o] : 1.0, r, Jc, Jp);
    cost += robust_apply<double>(loss, r, Jc, Jp);
    double* jo = Jc_o + (size_t)o * 2 * NCP;
#pragma unroll
    for (int e = 0; e < NCP; ++e) { jo[e] = Jc[0][e]; jo[NCP + e] = Jc[1][e]; }
    if (anchored || degenerate) continue;
    V00 += Jp[0][0] * Jp[0][0] + Jp[1][0] * Jp[1][0];
    V10 += Jp[0][1] * Jp[0][0] + Jp[1][1] * Jp[1][0];
    V11 += Jp[0][1] * Jp[0][1] + Jp[1][1] * Jp[1][1];
    V20 += Jp[0][2] * Jp[0][0] + Jp[1][2] * Jp[1][0];
    V21 += Jp[0][2] * Jp[0][1] + Jp[1][2] * Jp[1][1];
    V22 += Jp[0][2] * Jp[0][2] + Jp[1][2] * Jp[1][2];
    double* g = G + (size_t)obs_slot[o] * NCP * 3;
#pragma unroll
    for (int a = 0; a < NCP; ++a)
#pragma unroll
      for (int d = 0; d < 3; ++d) g[a * 3 + d] += Jc[0][a] * Jp[0][d] + Jc[1][a] * Jp[1][d];
  }
  cost_pt[p] = cost;
  double i00 = 0, i10 = 0, i11 = 0, i20 = 0, i21 = 0, i22 = 0;
  if (!anchored && !degenerate) {
    // V = L L^T; a pivot below 1e-12 of its diagonal entry means the rays do not fix the point (a singular V_p)
    const double l00 = sqrt(V00);
    const double l10 = V10 / l00, l20 = V20 / l00;
    const double d1 = V11 - l10 * l10;
    const double l11 = sqrt(d1);
    const double l21 = (V21 - l20 * l10) / l11;
    const double d2 = V22 - l20 * l20 - l21 * l21;
    const double l22 = sqrt(d2);
    if (!(V00 > 0.0) || !(d1 > 1e-12 * V11) || !(d2 > 1e-12 * V22) || !isfinite(l22)) {
      degenerate = true;
    } else {
      i00 = 1.0 / l00; i11 = 1.0 / l11; i22 = 1.0 / l22;
      i10 = -l10 * i00 * i11;
      i21 = -l21 * i11 * i22;
      i20 = -(l20 * i00 + l21 * i10) * i22;
      for (int s = s0; s < s1; ++s) {          // G = W L^-T: row a of G = L^-1 (row a of W)
        double* g = G + (size_t)s * NCP * 3;
#pragma unroll
        for (int a = 0; a < NCP; ++a) {
          const double w0 = g[a * 3], w1 = g[a * 3 + 1], w2 = g[a * 3 + 2];
          g[a * 3] = i00 * w0;
          g[a * 3 + 1] = i10 * w0 + i11 * w1;
          g[a * 3 + 2] = i20 * w0 + i21 * w1 + i22 * w2;
        }
      }
    }
  }
  if (degenerate) {        // out of S entirely: no camera diagonal, no Schur term
    for (size_t e = (size_t)o0 * 2 * NCP; e < (size_t)o1 * 2 * NCP; ++e) Jc_o[e] = 0.0;
    for (size_t e = (size_t)s0 * NCP * 3; e < (size_t)s1 * NCP * 3; ++e) G[e] = 0.0;
  }
  double* li = Linv + 6 * (size_t)p;
  li[0] = i00; li[1] = i10; li[2] = i11; li[3] = i20; li[4] = i21; li[5] = i22;
  pstat[p] = anchored ? COV_PT_ANCHORED : degenerate ? COV_PT_DEGENERATE : COV_PT_OK;
}

// ------------------------------------------------------------------ the undamped reduced camera system
// One workgroup per camera pair (a >= b) in lower-triangle order.  Thread = (row i of the P x P block, one of 16 lanes over the
// observations / slots of camera a); the 16 partial rows are summed in LDS in a fixed order (deterministic).
__global__ void __launch_bounds__(256) k_cov_schur(const double* __restrict__ Jc_o, const double* __restrict__ G,
                                                   const int32_t* __restrict__ cam_obs_start, const int32_t* __restrict__ cam_obs,
                                                   const int32_t* __restrict__ cam_slot_start, const int32_t* __restrict__ cam_slots,
                                                   const int32_t* __restrict__ slot_pt, const int32_t* __restrict__ slot_start,
                                                   const int32_t* __restrict__ slot_cam, double* __restrict__ A, int ld) {
  __shared__ double red[16][16][NCP];
  const int t = blockIdx.x;
  int a = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
  while (a * (a + 1) / 2 > t) --a;
  while ((a + 1) * (a + 2) / 2 <= t) ++a;
  const int b = t - a * (a + 1) / 2;
  const int i = threadIdx.x & 15, lane = threadIdx.x >> 4;
  double acc[NCP];
#pragma unroll
  for (int e = 0; e < NCP; ++e) acc[e] = 0.0;
  if (i < NCP) {
    if (a == b)
      for (int k = cam_obs_start[a] + lane; k < cam_obs_start[a + 1]; k += 16) {
        const double* j = Jc_o + (size_t)cam_obs[k] * 2 * NCP;
        const double j0 = j[i], j1 = j[NCP + i];
#pragma unroll
        for (int e = 0; e < NCP; ++e) acc[e] += j0 * j[e] + j1 * j[NCP + e];
      }
    for (int k = cam_slot_start[a] + lane; k < cam_slot_start[a + 1]; k += 16) {
      const int s = cam_slots[k];
      const int p = slot_pt[s];
      int lo = slot_start[p], hi = slot_start[p + 1] - 1, s2 = -1;
      while (lo <= hi) {                    // the slots of a point are in camera order
        const int mid = (lo + hi) >> 1;
        const int cm = slot_cam[mid];
        if (cm == b) { s2 = mid; break; }
        if (cm < b) lo = mid + 1; else hi = mid - 1;
      }
      if (s2 < 0) continue;
      const double* g1 = G + (size_t)s * NCP * 3 + i * 3;
      const double u0 = g1[0], u1 = g1[1], u2 = g1[2];
      const double* g2 = G + (size_t)s2 * NCP * 3;
#pragma unroll
      for (int e = 0; e < NCP; ++e) acc[e] -= u0 * g2[e * 3] + u1 * g2[e * 3 + 1] + u2 * g2[e * 3 + 2];
    }
#pragma unroll
    for (int e = 0; e < NCP; ++e) red[lane][i][e] = acc[e];
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < NCP * NCP; idx += blockDim.x) {
    const int ii = idx / NCP, e = idx % NCP;
    if (a == b && e > ii) continue;        // diagonal block: the lower half, mirrored (exactly symmetric)
    double v = 0.0;
    for (int l = 0; l < 16; ++l) v += red[l][ii][e];
    const size_t row = (size_t)a * NCP + ii, col = (size_t)b * NCP + e;
    A[row + col * ld] = v;
    A[col + row * ld] = v;
  }
}

// T (n x 7, row-major) = A Q for a symmetric A (column-major, leading dimension ld): thread i reads column i = row i
__global__ void __launch_bounds__(256) k_cov_matq(const double* __restrict__ A, int ld, int n, const double* __restrict__ Q,
                                                  double* __restrict__ T) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double t[COV_G];
#pragma unroll
  for (int k = 0; k < COV_G; ++k) t[k] = 0.0;
  for (int j = 0; j < n; ++j) {
    const double v = A[(size_t)i + (size_t)j * ld];
#pragma unroll
    for (int k = 0; k < COV_G; ++k) t[k] += v * Q[j * COV_G + k];
  }
#pragma unroll
  for (int k = 0; k < COV_G; ++k) T[i * COV_G + k] = t[k];
}

// stats[0] = trace A, stats[1] = ||A||_F^2, stats[2] = ||T||_F^2 (T: n x 7 or NULL).  One workgroup of 256.
__global__ void __launch_bounds__(256) k_cov_stats(const double* __restrict__ A, int ld, int n, const double* __restrict__ T,
                                                   double* __restrict__ stats) {
  __shared__ double red[3][256];
  double tr = 0, fr = 0, tq = 0;
  for (int i = threadIdx.x; i < n; i += 256) tr += A[(size_t)i * ld + i];
  for (int j = 0; j < n; ++j)
    for (int i = threadIdx.x; i < n; i += 256) {
      const double v = A[(size_t)i + (size_t)j * ld];
      fr += v * v;
    }
  if (T)
    for (int k = threadIdx.x; k < n * COV_G; k += 256) tq += T[k] * T[k];
  red[0][threadIdx.x] = tr; red[1][threadIdx.x] = fr; red[2][threadIdx.x] = tq;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
      for (int q = 0; q < 3; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x < 3) stats[threadIdx.x] = red[threadIdx.x][0];
}

// A += alpha Q Q^T (alpha = stats[0] / n; use_q = 0: nothing added) on the n x n system, identity on the padding up to npad;
// dg = the diagonal of the result (the reference of the pivot test)
__global__ void __launch_bounds__(256) k_cov_reg(double* __restrict__ A, int ld, int n, int npad, const double* __restrict__ Q,
                                                 int use_q, const double* __restrict__ stats, double* __restrict__ dg) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (i >= npad || j >= npad) return;
  double& v = A[(size_t)i + (size_t)j * ld];
  if (i < n && j < n) {
    if (use_q) {
      const double alpha = stats[0] / n;
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < COV_G; ++k) s += Q[i * COV_G + k] * Q[j * COV_G + k];
      v += alpha * s;
    }
  } else {
    v = (i == j) ? 1.0 : 0.0;
  }
  if (i == j) dg[i] = v;
}

// ------------------------------------------------------------------ tiled Cholesky, lower, column-major, npad = 32 k
// diagonal tile k: unblocked factorisation in LDS.  A pivot that is not above 1e-14 of the tile's original diagonal entry is
// recorded in *info (1-based row, first one wins) and replaced by that entry, so that the launches after it stay finite.
__global__ void __launch_bounds__(256) k_cov_potrf_diag(double* __restrict__ A, int ld, int k, const double* __restrict__ dg,
                                                        int* __restrict__ info) {
  __shared__ double s[COV_NB][COV_NB + 1];
  const int o = k * COV_NB, tid = threadIdx.x;
  for (int idx = tid; idx < COV_NB * COV_NB; idx += 256) {
    const int r = idx % COV_NB, c = idx / COV_NB;
    s[r][c] = A[(size_t)(o + r) + (size_t)(o + c) * ld];
  }
  __syncthreads();
  for (int j = 0; j < COV_NB; ++j) {
    if (tid == 0) {
      double d = s[j][j];
      const double ref = dg[o + j];
      if (!(d > 1e-14 * ref) || !(ref > 0.0)) {
        if (*info == 0) *info = o + j + 1;
        d = ref > 0.0 ? ref : 1.0;
      }
      s[j][j] = sqrt(d);
    }
    __syncthreads();
    if (tid > j && tid < COV_NB) s[tid][j] /= s[j][j];
    __syncthreads();
    for (int idx = tid; idx < COV_NB * COV_NB; idx += 256) {
      const int r = idx % COV_NB, c = idx / COV_NB;
      if (c > j && r >= c) s[r][c] -= s[r][j] * s[c][j];
    }
    __syncthreads();
  }
  for (int idx = tid; idx < COV_NB * COV_NB; idx += 256) {
    const int r = idx % COV_NB, c = idx / COV_NB;
    if (r >= c) A[(size_t)(o + r) + (size_t)(o + c) * ld] = s[r][c];
  }
}

// tiles below diagonal tile k: A_ik <- A_ik L_kk^-T (one workgroup per tile, one thread per row)
__global__ void __launch_bounds__(64) k_cov_trsm(double* __restrict__ A, int ld, int k) {
  __shared__ double L[COV_NB][COV_NB + 1], B[COV_NB][COV_NB + 1];
  const int o = k * COV_NB, ro = (k + 1 + blockIdx.x) * COV_NB, tid = threadIdx.x;
  for (int idx = tid; idx < COV_NB * COV_NB; idx += 64) {
    const int r = idx % COV_NB, c = idx / COV_NB;
    L[r][c] = A[(size_t)(o + r) + (size_t)(o + c) * ld];
    B[r][c] = A[(size_t)(ro + r) + (size_t)(o + c) * ld];
  }
  __syncthreads();
  if (tid < COV_NB) {
    for (int j = 0; j < COV_NB; ++j) {
      double x = B[tid][j];
      for (int l = 0; l < j; ++l) x -= B[tid][l] * L[j][l];
      B[tid][j] = x / L[j][j];
    }
  }
  __syncthreads();
  for (int idx = tid; idx < COV_NB * COV_NB; idx += 64) {
    const int r = idx % COV_NB, c = idx / COV_NB;
    A[(size_t)(ro + r) + (size_t)(o + c) * ld] = B[r][c];
  }
}

// trailing update after tile column k: A_ij -= L_ik L_jk^T for k < j <= i < nt (one workgroup per tile, lower-triangle order)
__global__ void __launch_bounds__(256) k_cov_syrk(double* __restrict__ A, int ld, int k) {
  __shared__ double Li[COV_NB][COV_NB + 1], Lj[COV_NB][COV_NB + 1];
  const int t = blockIdx.x;
  int ii = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
  while (ii * (ii + 1) / 2 > t) --ii;
  while ((ii + 1) * (ii + 2) / 2 <= t) ++ii;
  const int jj = t - ii * (ii + 1) / 2;
  const int ri = (k + 1 + ii) * COV_NB, rj = (k + 1 + jj) * COV_NB, o = k * COV_NB, tid = threadIdx.x;
  for (int idx = tid; idx < COV_NB * COV_NB; idx += 256) {
    const int r = idx % COV_NB, c = idx / COV_NB;
    Li[r][c] = A[(size_t)(ri + r) + (size_t)(o + c) * ld];
    Lj[r][c] = A[(size_t)(rj + r) + (size_t)(o + c) * ld];
  }
  __syncthreads();
  const int r = tid % COV_NB, c0 = tid / COV_NB;
#pragma unroll
  for (int q = 0; q < COV_NB / 8; ++q) {
    const int c = c0 + 8 * q;
    double s = 0.0;
#pragma unroll 8
    for (int l = 0; l < COV_NB; ++l) s += Li[r][l] * Lj[c][l];
    A[(size_t)(ri + r) + (size_t)(rj + c) * ld] -= s;
  }
}

// upper triangle <- L^T, so that column i above the diagonal holds row i of L (contiguous for the back substitution)
__global__ void __launch_bounds__(256) k_cov_mirror(double* __restrict__ A, int ld, int npad) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
  if (r < c && c < npad) A[(size_t)r + (size_t)c * ld] = A[(size_t)c + (size_t)r * ld];
}

// column j of X = (L L^T)^-1: forward substitution L y = e_j down the columns of L, then back substitution L^T x = y up the
// columns of the mirrored upper triangle.  Thread t owns rows t + 256 q; the pivot value of step i is broadcast through LDS
// (two alternating slots: one barrier per step); the column of step i + 1 is loaded while step i waits for its barrier.
__global__ void __launch_bounds__(256) k_cov_inv(const double* __restrict__ A, int ld, int n, double* __restrict__ X) {
  __shared__ double bc[2];
  const int j = blockIdx.x, tid = threadIdx.x;
  double y[COV_INV_Q], cur[COV_INV_Q], nxt[COV_INV_Q];
#pragma unroll
  for (int q = 0; q < COV_INV_Q; ++q) {
    const int r = tid + 256 * q;
    y[q] = (r == j) ? 1.0 : 0.0;
    cur[q] = (r >= j && r < n) ? A[(size_t)r + (size_t)j * ld] : 0.0;
  }
  for (int i = j; i < n; ++i) {
    const int qi = i >> 8;
#pragma unroll
    for (int q = 0; q < COV_INV_Q; ++q) {
      const int r = tid + 256 * q;
      nxt[q] = (i + 1 < n && r >= i + 1 && r < n) ? A[(size_t)r + (size_t)(i + 1) * ld] : 0.0;
    }
    if ((i & 255) == tid) {
      double v = 0.0;
#pragma unroll
      for (int q = 0; q < COV_INV_Q; ++q) if (q == qi) v = y[q] / cur[q];
#pragma unroll
      for (int q = 0; q < COV_INV_Q; ++q) if (q == qi) y[q] = v;
      bc[i & 1] = v;
    }
    __syncthreads();
    const double yi = bc[i & 1];
#pragma unroll
    for (int q = 0; q < COV_INV_Q; ++q) {
      const int r = tid + 256 * q;
      if (r > i && r < n) y[q] -= cur[q] * yi;
      cur[q] = nxt[q];
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < COV_INV_Q; ++q) {
    const int r = tid + 256 * q;
    cur[q] = (r < n) ? A[(size_t)r + (size_t)(n - 1) * ld] : 0.0;
  }
  for (int i = n - 1; i >= 0; --i) {
    const int qi = i >> 8;
#pragma unroll
    for (int q = 0; q < COV_INV_Q; ++q) {
      const int r = tid + 256 * q;
      nxt[q] = (i > 0 && r <= i - 1) ? A[(size_t)r + (size_t)(i - 1) * ld] : 0.0;
    }
    if ((i & 255) == tid) {
      double v = 0.0;
#pragma unroll
      for (int q = 0; q < COV_INV_Q; ++q) if (q == qi) v = y[q] / cur[q];
#pragma unroll
      for (int q = 0; q < COV_INV_Q; ++q) if (q == qi) y[q] = v;
      bc[i & 1] = v;
    }
    __syncthreads();
    const double xi = bc[i & 1];
#pragma unroll
    for (int q = 0; q < COV_INV_Q; ++q) {
      const int r = tid + 256 * q;
      if (r < i) y[q] -= cur[q] * xi;
      cur[q] = nxt[q];
    }
  }
#pragma unroll
  for (int q = 0; q < COV_INV_Q; ++q) {
    const int r = tid + 256 * q;
    if (r < n) X[(size_t)r + (size_t)j * ld] = y[q];
  }
}

// G7 = Q^T T (7 x 7): one workgroup, thread (k, l) < 49
__global__ void __launch_bounds__(64) k_cov_gram(const double* __restrict__ Q, const double* __restrict__ T, int n,
                                                 double* __restrict__ G7) {
  const int k = threadIdx.x / COV_G, l = threadIdx.x % COV_G;
  if (threadIdx.x >= COV_G * COV_G) return;
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += Q[i * COV_G + k] * T[i * COV_G + l];
  G7[k * COV_G + l] = s;
}

// X <- P X P = X - Q T^T - T Q^T + Q G7 Q^T  (T = X Q, G7 = Q^T X Q)
__global__ void __launch_bounds__(256) k_cov_project(double* __restrict__ X, int ld, int n, const double* __restrict__ Q,
                                                     const double* __restrict__ T, const double* __restrict__ G7) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (i >= n || j >= n) return;
  double qi[COV_G], qj[COV_G];
#pragma unroll
  for (int k = 0; k < COV_G; ++k) { qi[k] = Q[i * COV_G + k]; qj[k] = Q[j * COV_G + k]; }
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < COV_G; ++k) {
    double gq = 0.0;
#pragma unroll
    for (int l = 0; l < COV_G; ++l) gq += G7[k * COV_G + l] * qj[l];
    s += qi[k] * (gq - T[j * COV_G + k]) - T[i * COV_G + k] * qj[k];
  }
  X[(size_t)i + (size_t)j * ld] += s;
}

// diagonal camera blocks (C x P x P), times scale
__global__ void __launch_bounds__(256) k_cov_blocks(const double* __restrict__ X, int ld, int C, double scale, double* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= C * NCP * NCP) return;
  const int c = idx / (NCP * NCP), a = (idx / NCP) % NCP, b = idx % NCP;
  out[idx] = scale * X[(size_t)(c * NCP + a) + (size_t)(c * NCP + b) * ld];
}

// Sigma_pp = V^-1 + L^-T (sum_{s, s'} G_s^T X[c_s, c_s'] G_s') L^-1  (X == nullptr: cameras held, V^-1 alone), packed xx xy xz yy yz zz
__global__ void __launch_bounds__(128) k_cov_points(const double* __restrict__ X, int ld, const double* __restrict__ G,
                                                    const double* __restrict__ Linv, const int* __restrict__ pstat,
                                                    const int32_t* __restrict__ slot_start, const int32_t* __restrict__ slot_cam,
                                                    int N, double scale, double* __restrict__ out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= N) return;
  double* o = out + 6 * (size_t)p;
  const int st = pstat[p];
  if (st != COV_PT_OK) {
    const double v = st == COV_PT_ANCHORED ? 0.0 : __builtin_nan("");
    for (int k = 0; k < 6; ++k) o[k] = v;
    return;
  }
  const double* li = Linv + 6 * (size_t)p;
  double Li[3][3] = {{li[0], 0.0, 0.0}, {li[1], li[2], 0.0}, {li[3], li[4], li[5]}};
  double M3[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  if (X) {
    const int s0 = slot_start[p], s1 = slot_start[p + 1];
    for (int s = s0; s < s1; ++s) {
      const double* g1 = G + (size_t)s * NCP * 3;
      const size_t r0 = (size_t)slot_cam[s] * NCP;
      for (int s2 = s0; s2 < s1; ++s2) {
        const double* g2 = G + (size_t)s2 * NCP * 3;
        const size_t c0 = (size_t)slot_cam[s2] * NCP;
        for (int a = 0; a < NCP; ++a) {
          const double* xc = X + c0 + (r0 + a) * ld;   // X[r0 + a][c0 + b] = X[c0 + b][r0 + a] (symmetric): contiguous in b
          double t0 = 0, t1 = 0, t2 = 0;
#pragma unroll
          for (int b = 0; b < NCP; ++b) {
            const double x = xc[b];
            t0 += x * g2[b * 3]; t1 += x * g2[b * 3 + 1]; t2 += x * g2[b * 3 + 2];
          }
          const double u0 = g1[a * 3], u1 = g1[a * 3 + 1], u2 = g1[a * 3 + 2];
          M3[0][0] += u0 * t0; M3[0][1] += u0 * t1; M3[0][2] += u0 * t2;
          M3[1][0] += u1 * t0; M3[1][1] += u1 * t1; M3[1][2] += u1 * t2;
          M3[2][0] += u2 * t0; M3[2][1] += u2 * t1; M3[2][2] += u2 * t2;
        }
      }
    }
  }
  // Sigma = L^-T (I + M3) L^-1
#pragma unroll
  for (int k = 0; k < 3; ++k) M3[k][k] += 1.0;
  double Z[3][3];     // Z = (I + M3) L^-1
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) Z[r][c] = M3[r][0] * Li[0][c] + M3[r][1] * Li[1][c] + M3[r][2] * Li[2][c];
  double S[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) S[r][c] = Li[0][r] * Z[0][c] + Li[1][r] * Z[1][c] + Li[2][r] * Z[2][c];
  o[0] = scale * S[0][0];
  o[1] = scale * 0.5 * (S[0][1] + S[1][0]);
  o[2] = scale * 0.5 * (S[0][2] + S[2][0]);
  o[3] = scale * S[1][1];
  o[4] = scale * 0.5 * (S[1][2] + S[2][1]);
  o[5] = scale * S[2][2];
}

// ------------------------------------------------------------------ host side
// The 7 null vectors of the similarity gauge on the camera rows (n x 7, row-major), orthonormalised.  For a world change
// X' = (1 + s) (I + [omega]x) X + tau, camera c keeps every projection when R' = R exp(-[omega]x), t' = (1 + s) t - R tau:
//   d rvec / d omega = -J_r^-1(rvec)  (J_r: right Jacobian of SO(3)),  d t / d tau = -R(rvec),  d t / d s = t,  intrinsics 0.
inline void cov_gauge_basis(const double* cams, int C, std::vector<double>& Q) {
  const int n = C * NCP;
  Q.assign((size_t)n * COV_G, 0.0);
  for (int c = 0; c < C; ++c) {
    const double* cp = cams + (size_t)c * NCP;
    const double r[3] = {cp[0], cp[1], cp[2]};
    const double th2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2], th = std::sqrt(th2);
    // R = cos I + sinc [r]x + (1 - cos)/th2 r r^T
    double a, b, beta;
    if (th2 < 1e-8) { a = 1.0 - th2 / 6; b = 0.5 - th2 / 24; beta = 1.0 / 12 + th2 / 720; }
    else { a = std::sin(th) / th; b = (1.0 - std::cos(th)) / th2; beta = 1.0 / th2 - (1.0 + std::cos(th)) / (2.0 * th * std::sin(th)); }
    const double cs = std::cos(th);
    double K[3][3] = {{0, -r[2], r[1]}, {r[2], 0, -r[0]}, {-r[1], r[0], 0}};
    double K2[3][3], R[3][3], Jri[3][3];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        K2[i][j] = K[i][0] * K[0][j] + K[i][1] * K[1][j] + K[i][2] * K[2][j];
      }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        R[i][j] = (i == j ? (th2 < 1e-8 ? 1.0 - th2 / 2 : cs) : 0.0) + a * K[i][j] + b * r[i] * r[j];
        Jri[i][j] = (i == j ? 1.0 : 0.0) + 0.5 * K[i][j] + beta * K2[i][j];
      }
    for (int i = 0; i < 3; ++i) {
      double* qr = &Q[(size_t)(c * NCP + i) * COV_G];
      double* qt = &Q[(size_t)(c * NCP + 3 + i) * COV_G];
      for (int k = 0; k < 3; ++k) { qr[k] = -Jri[i][k]; qt[3 + k] = -R[i][k]; }
      qt[6] = cp[3 + i];
    }
  }
  for (int pass = 0; pass < 2; ++pass)      // modified Gram-Schmidt, twice
    for (int k = 0; k < COV_G; ++k) {
      for (int l = 0; l < k; ++l) {
        double d = 0.0;
        for (int i = 0; i < n; ++i) d += Q[(size_t)i * COV_G + k] * Q[(size_t)i * COV_G + l];
        for (int i = 0; i < n; ++i) Q[(size_t)i * COV_G + k] -= d * Q[(size_t)i * COV_G + l];
      }
      double nn = 0.0;
      for (int i = 0; i < n; ++i) nn += Q[(size_t)i * COV_G + k] * Q[(size_t)i * COV_G + k];
      nn = std::sqrt(nn);
      for (int i = 0; i < n; ++i) Q[(size_t)i * COV_G + k] /= nn;
    }
}

// what the engine hands over: its current parameters and the point-major observation layout, all device pointers
template <typename T>
struct CovIn {
  hipStream_t stream;
  int C, N;
  int64_t M;
  const double *cams, *pts;
  const typename Vec2<T>::type* uv;
  const T* w;
  const int32_t *ci, *pt_start;
  const unsigned char* fixed;
  RLoss<double> loss;
};

// The anchors fix the datum only when there are at least three of them and they are not collinear (a rotation about the
// line through collinear anchors, or any motion leaving one or two points in place, keeps the cost): "" when they do.
inline std::string cov_anchor_problem(const std::vector<unsigned char>& fx, const std::vector<double>& pts) {
  std::vector<int> a;
  for (size_t p = 0; p < fx.size(); ++p) if (fx[p]) a.push_back((int)p);
  if (a.size() < 3) return "sba_covariance: " + std::to_string(a.size()) + " anchored point(s) do not fix the datum (at least 3 non-collinear are needed)";
  const double* p0 = &pts[3 * (size_t)a[0]];
  double best = -1, u[3] = {0, 0, 0};
  for (int p : a) {
    const double* q = &pts[3 * (size_t)p];
    const double d[3] = {q[0] - p0[0], q[1] - p0[1], q[2] - p0[2]};
    const double l = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    if (l > best) { best = l; u[0] = d[0]; u[1] = d[1]; u[2] = d[2]; }
  }
  double off = 0;                       // largest distance of an anchor from the line p0 + t u, relative to |u|
  for (int p : a) {
    const double* q = &pts[3 * (size_t)p];
    const double d[3] = {q[0] - p0[0], q[1] - p0[1], q[2] - p0[2]};
    const double c[3] = {d[1] * u[2] - d[2] * u[1], d[2] * u[0] - d[0] * u[2], d[0] * u[1] - d[1] * u[0]};
    off = std::max(off, c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
  }
  if (!(best > 0) || !(off > 1e-12 * best * best)) return "sba_covariance: the anchored points are collinear and do not fix the datum";
  return "";
}

template <typename T>
int cov_run(const CovIn<T>& in, const sba_cov_opts& opt, double* cam_full, double* cam_blocks, double* pt_cov, sba_cov_report* rep,
            std::string& err) {
  const auto t_start = std::chrono::steady_clock::now();
  ArenaScope own(nullptr);          // private buffers: hipMalloc'd here, freed on return (the handle's arena stays as it was)
  hipStream_t st = in.stream;
  const int C = in.C, N = in.N, n = C * NCP;
  const int64_t M = in.M;
  const bool cams_fixed = opt.cams_fixed != 0;
  const int npad = (n + COV_NB - 1) / COV_NB * COV_NB, nt = npad / COV_NB, ld = npad;
  const bool need_cams = !cams_fixed && (cam_full || cam_blocks || pt_cov);
  if (need_cams && npad > 256 * COV_INV_Q) { err = "sba_covariance: too many camera parameters"; return SBA_ERR_UNSUPPORTED; }
  DevEvents<4> ev;
  // ---- host prelude (part of seconds_total, not of the device phases): the layout, the anchors and the gauge basis
  std::vector<int32_t> ci((size_t)M), ps((size_t)N + 1);
  std::vector<unsigned char> fx(in.fixed ? N : 0);
  std::vector<double> cams_h((size_t)n), pts_h;
  if (M) HIPCHK(hipMemcpyAsync(ci.data(), in.ci, sizeof(int32_t) * M, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(ps.data(), in.pt_start, sizeof(int32_t) * (N + 1), hipMemcpyDeviceToHost, st));
  if (in.fixed && N) HIPCHK(hipMemcpyAsync(fx.data(), in.fixed, N, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(cams_h.data(), in.cams, sizeof(double) * n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  int n_anch = 0;
  for (unsigned char v : fx) n_anch += v != 0;
  if (!cams_fixed && n_anch > 0) {
    pts_h.resize((size_t)N * 3);
    HIPCHK(hipMemcpyAsync(pts_h.data(), in.pts, sizeof(double) * N * 3, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    err = cov_anchor_problem(fx, pts_h);
    if (!err.empty()) return SBA_ERR_INVALID;
  }
  const int g = (cams_fixed || n_anch > 0) ? 0 : COV_G;
  // (point, camera) slots: the distinct cameras of every point, in camera order, and both of their camera-major lists
  std::vector<int32_t> slot_start((size_t)N + 1, 0), slot_cam, slot_pt, obs_slot((size_t)M);
  slot_cam.reserve((size_t)M); slot_pt.reserve((size_t)M);
  {
    std::vector<int32_t> pos(C, -1), cams_of;
    for (int p = 0; p < N; ++p) {
      cams_of.clear();
      for (int o = ps[p]; o < ps[p + 1]; ++o) if (pos[ci[o]] < 0) { pos[ci[o]] = 0; cams_of.push_back(ci[o]); }
      std::sort(cams_of.begin(), cams_of.end());
      const int base = (int)slot_cam.size();
      for (size_t k = 0; k < cams_of.size(); ++k) { pos[cams_of[k]] = base + (int)k; slot_cam.push_back(cams_of[k]); slot_pt.push_back(p); }
      for (int o = ps[p]; o < ps[p + 1]; ++o) obs_slot[o] = pos[ci[o]];
      for (int c : cams_of) pos[c] = -1;
      slot_start[p + 1] = (int)slot_cam.size();
    }
  }
  const int nslot = (int)slot_cam.size();
  std::vector<int32_t> cam_slot_start(C + 1, 0), cam_slots(nslot), cam_obs_start(C + 1, 0), cam_obs((size_t)M);
  for (int s = 0; s < nslot; ++s) cam_slot_start[slot_cam[s] + 1]++;
  for (int64_t o = 0; o < M; ++o) cam_obs_start[ci[o] + 1]++;
  for (int c = 0; c < C; ++c) { cam_slot_start[c + 1] += cam_slot_start[c]; cam_obs_start[c + 1] += cam_obs_start[c]; }
  {
    std::vector<int32_t> f1(cam_slot_start.begin(), cam_slot_start.end() - 1), f2(cam_obs_start.begin(), cam_obs_start.end() - 1);
    for (int s = 0; s < nslot; ++s) cam_slots[f1[slot_cam[s]]++] = s;
    for (int64_t o = 0; o < M; ++o) cam_obs[f2[ci[o]]++] = (int32_t)o;
  }
  DevBuf<int32_t> d_slot_start, d_slot_cam, d_slot_pt, d_obs_slot, d_cam_slot_start, d_cam_slots, d_cam_obs_start, d_cam_obs;
  d_slot_start.upload(slot_start, st); d_slot_cam.upload(slot_cam, st); d_slot_pt.upload(slot_pt, st); d_obs_slot.upload(obs_slot, st);
  d_cam_slot_start.upload(cam_slot_start, st); d_cam_slots.upload(cam_slots, st);
  d_cam_obs_start.upload(cam_obs_start, st); d_cam_obs.upload(cam_obs, st);
  DevBuf<double> campre, Jc_o, G, Linv, cost_pt, A, X, Q, TQ, stats, G7, dg, blk, pout;
  DevBuf<int> pstat, d_info;
  campre.alloc((size_t)C * CAMPRE); Jc_o.alloc((size_t)M * 2 * NCP); G.alloc((size_t)nslot * NCP * 3);
  Linv.alloc((size_t)N * 6); cost_pt.alloc(N); pstat.alloc(N);
  if (need_cams) {
    A.alloc((size_t)npad * npad); X.alloc((size_t)npad * npad); stats.alloc(3); dg.alloc(npad); d_info.alloc(1);
    A.zero(st); X.zero(st); stats.zero(st); d_info.zero(st);
    if (g) {
      std::vector<double> q;
      cov_gauge_basis(cams_h.data(), C, q);
      Q.upload(q, st);
      TQ.alloc((size_t)n * COV_G); G7.alloc(COV_G * COV_G);
    }
    if (cam_blocks) blk.alloc((size_t)C * NCP * NCP);
  }
  if (pt_cov && N > 0) pout.alloc((size_t)N * 6);

  // ---- device phases, back to back on the stream: [ev0, ev1) S formation, [ev1, ev2) factor + inverse (+ P X P), [ev2, ev3) outputs
  HIPCHK(hipEventRecord(ev[0], st));
  hipLaunchKernelGGL(k_cam_prep<double>, dim3((C + 63) / 64), dim3(64), 0, st, in.cams, campre.p, C);
  if (N > 0)
    hipLaunchKernelGGL(k_cov_lin<T>, dim3((N + 127) / 128), dim3(128), 0, st, campre.p, in.pts, in.uv, in.w, in.pt_start, in.ci,
                       d_obs_slot.p, d_slot_start.p, in.fixed, in.loss, N, Jc_o.p, G.p, Linv.p, pstat.p, cost_pt.p);
  if (need_cams)
    hipLaunchKernelGGL(k_cov_schur, dim3(C * (C + 1) / 2), dim3(256), 0, st, Jc_o.p, G.p, d_cam_obs_start.p, d_cam_obs.p,
                       d_cam_slot_start.p, d_cam_slots.p, d_slot_pt.p, d_slot_start.p, d_slot_cam.p, A.p, ld);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ev[1], st));
  if (need_cams) {
    if (g) hipLaunchKernelGGL(k_cov_matq, dim3((n + 255) / 256), dim3(256), 0, st, A.p, ld, n, Q.p, TQ.p);
    hipLaunchKernelGGL(k_cov_stats, dim3(1), dim3(256), 0, st, A.p, ld, n, g ? TQ.p : (const double*)nullptr, stats.p);
    hipLaunchKernelGGL(k_cov_reg, dim3((npad + 255) / 256, npad), dim3(256), 0, st, A.p, ld, n, npad,
                       g ? Q.p : (const double*)nullptr, g, stats.p, dg.p);
    for (int k = 0; k < nt; ++k) {
      hipLaunchKernelGGL(k_cov_potrf_diag, dim3(1), dim3(256), 0, st, A.p, ld, k, dg.p, d_info.p);
      const int m = nt - k - 1;
      if (m > 0) {
        hipLaunchKernelGGL(k_cov_trsm, dim3(m), dim3(64), 0, st, A.p, ld, k);
        hipLaunchKernelGGL(k_cov_syrk, dim3(m * (m + 1) / 2), dim3(256), 0, st, A.p, ld, k);
      }
    }
    hipLaunchKernelGGL(k_cov_mirror, dim3((npad + 255) / 256, npad), dim3(256), 0, st, A.p, ld, npad);
    hipLaunchKernelGGL(k_cov_inv, dim3(n), dim3(256), 0, st, A.p, ld, n, X.p);
    if (g) {
      hipLaunchKernelGGL(k_cov_matq, dim3((n + 255) / 256), dim3(256), 0, st, X.p, ld, n, Q.p, TQ.p);
      hipLaunchKernelGGL(k_cov_gram, dim3(1), dim3(64), 0, st, Q.p, TQ.p, n, G7.p);
      hipLaunchKernelGGL(k_cov_project, dim3((n + 255) / 256, n), dim3(256), 0, st, X.p, ld, n, Q.p, TQ.p, G7.p);
    }
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipEventRecord(ev[2], st));
  if (blk.n) hipLaunchKernelGGL(k_cov_blocks, dim3((C * NCP * NCP + 255) / 256), dim3(256), 0, st, X.p, ld, C, 1.0, blk.p);
  if (pout.n)
    hipLaunchKernelGGL(k_cov_points, dim3((N + 127) / 128), dim3(128), 0, st, need_cams ? X.p : (const double*)nullptr, ld, G.p,
                       Linv.p, pstat.p, d_slot_start.p, d_slot_cam.p, N, 1.0, pout.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ev[3], st));
  // ---- read-back
  int info = 0;
  double stats_h[3] = {0, 0, 0};
  std::vector<int> h_stat(N);
  std::vector<double> h_cost(N);
  if (N) {
    HIPCHK(hipMemcpyAsync(h_stat.data(), pstat.p, sizeof(int) * N, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_cost.data(), cost_pt.p, sizeof(double) * N, hipMemcpyDeviceToHost, st));
  }
  if (need_cams) {
    HIPCHK(hipMemcpyAsync(stats_h, stats.p, sizeof(double) * 3, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&info, d_info.p, sizeof(int), hipMemcpyDeviceToHost, st));
  }
  if (blk.n) HIPCHK(hipMemcpyAsync(cam_blocks, blk.p, sizeof(double) * blk.n, hipMemcpyDeviceToHost, st));
  if (pout.n) HIPCHK(hipMemcpyAsync(pt_cov, pout.p, sizeof(double) * pout.n, hipMemcpyDeviceToHost, st));
  if (need_cams && cam_full)        // X is symmetric: its column-major rows are the row-major rows
    HIPCHK(hipMemcpy2DAsync(cam_full, sizeof(double) * n, X.p, sizeof(double) * ld, sizeof(double) * n, n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const float ms[3] = {ev.ms(0, 1), ev.ms(1, 2), ev.ms(2, 3)};
  // the counts and sigma^2 decide the scale of every output
  int n_deg = 0;
  int64_t m_used = 0;
  double ssr = 0.0;
  for (int p = 0; p < N; ++p) {
    if (h_stat[p] == COV_PT_DEGENERATE) { n_deg++; continue; }
    m_used += ps[p + 1] - ps[p];
    ssr += h_cost[p];
  }
  const int n_free = N - n_anch - n_deg;
  const int64_t dof = 2 * m_used - ((cams_fixed ? 0 : (int64_t)n) + 3 * (int64_t)n_free - g);
  const double sigma2 = dof > 0 ? ssr / (double)dof : std::nan("");
  const double scale = opt.scale ? sigma2 : 1.0;
  if (scale != 1.0) {
    if (need_cams && cam_full) for (size_t k = 0; k < (size_t)n * n; ++k) cam_full[k] *= scale;
    if (blk.n) for (size_t k = 0; k < blk.n; ++k) cam_blocks[k] *= scale;
    if (pout.n) for (size_t k = 0; k < pout.n; ++k) pt_cov[k] *= scale;
  }
  if (info) {          // a non-positive pivot: no output rather than a wrong one
    const double nan = std::nan("");
    if (need_cams && cam_full) std::fill(cam_full, cam_full + (size_t)n * n, nan);
    if (need_cams && cam_blocks) std::fill(cam_blocks, cam_blocks + (size_t)C * NCP * NCP, nan);
    if (pt_cov) std::fill(pt_cov, pt_cov + (size_t)N * 6, nan);
  }
  if (cams_fixed && cam_full) std::fill(cam_full, cam_full + (size_t)n * n, 0.0);
  if (cams_fixed && cam_blocks) std::fill(cam_blocks, cam_blocks + (size_t)C * NCP * NCP, 0.0);
  if (rep) {
    *rep = sba_cov_report{};
    rep->sigma2 = sigma2;
    rep->dof = dof;
    rep->gauge_rank = g;
    rep->n_points_degenerate = n_deg;
    rep->n_points_anchored = n_anch;
    rep->info = info;
    rep->gauge_residual = (g && stats_h[1] > 0) ? std::sqrt(stats_h[2]) / (std::sqrt(stats_h[1]) * std::sqrt((double)COV_G)) : 0.0;
    rep->seconds_form = ms[0] * 1e-3;
    rep->seconds_inverse = ms[1] * 1e-3;
    rep->seconds_points = ms[2] * 1e-3;
    rep->seconds_device = (ms[0] + ms[1] + ms[2]) * 1e-3;
    rep->seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
  }
  return SBA_OK;
}

}  // namespace SBA_NS
