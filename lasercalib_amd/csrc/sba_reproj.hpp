// sba_reproj.hpp -- reprojection diagnostics of the handle's current solution (sba_reproj_stats, include/sba_hip.h): per camera
// the error statistics, an integer histogram of the pixel error, a residual field over the image and a radial / tangential
// profile; per point [n, rms, max]; per observation the error in the caller's order; the K worst observations.  One streaming
// pass over data the handle already holds, in float64 whatever the handle's dtype, on private buffers freed on return; it touches
// no LM kernel, no LM state and no route.  No floating-point atomics: every sum is formed in the order
// of the canonical layout (cameras: camera-major position; points: camera-ascending), so that two calls, and a shuffled and a
// sorted observation list, return the same bits.  Kernels:
//   k_cam_prep<double>   CamPre rows in f64 from the current camera parameters (both passes read this one table)
//   k_rp_cams            one workgroup per camera-major chunk (<= 1024 observations of one camera, four per thread): residual,
//                        error, bins; the histogram in u32 LDS counters added to the C x B table with integer atomics; the
//                        record [n, sum du, sum dv, sum e, sum e^2, selected, non-finite | max e] by a wave reduction and the
//                        waves through LDS in wave order; the binned sums (grid cells, radial bins) by staging every
//                        observation's {bin, three values} in LDS, thread b then walks the records in index order and adds
//                        those of bin b (all lanes read one LDS address: a broadcast).  One partial record / table per chunk
//   k_rp_fold            per camera the partial records / tables of its chunks, added in chunk order
//   k_rp_obs             one thread per observation in point-major order: e at its point-major position (NaN: not finite)
//   k_rp_points          one thread per point: [n, rms, max] over its selected finite observations, summed camera-ascending
//   k_rp_compact         appends (point-major position, e) of the selected observations at or above a histogram bin (the cut
//                        the host found for the K worst) through one integer counter; the host sorts, so the order of the
//                        appends does not matter
// rp_residual is compiled with floating-point contraction off: k_rp_cams and k_rp_obs evaluate the same observation and must
// produce the same bits of e (the histogram of the one decides which entries of the other the compaction keeps).
#pragma once
#include "sba_kernels.hpp"

namespace SBA_NS {
using namespace sba_host;

constexpr int RP_BLOCK = 256;
constexpr int RP_WAVES = RP_BLOCK / 64;
constexpr int RP_PER = CM_CHUNK / RP_BLOCK;      // observations per thread of k_rp_cams
constexpr int RP_NSUM = 7, RP_NMAX = 1, RP_REC = RP_NSUM + RP_NMAX;
constexpr int RP_N = 0, RP_DU = 1, RP_DV = 2, RP_E = 3, RP_E2 = 4, RP_SEL = 5, RP_BAD = 6, RP_MAX = 7;
constexpr int RP_MAX_BINS = 256;                  // grid cells / radial bins a workgroup can walk (one thread each)
static_assert(RP_MAX_BINS <= RP_BLOCK && CM_CHUNK % RP_BLOCK == 0, "k_rp_cams: one thread per bin, whole rounds per chunk");

struct RpBins {
  int select;            // 0 all, 1 weight > 0, 2 weight == 0
  int B;                 // histogram bins, the last one is the overflow bin
  double inv;            // 1 / hist_bin_px
  int gx, gy;            // residual field (0, 0: off)
  double qx, qy;         // gx / width, gy / height
  int nr;                // radial bins (0: off)
  double qr;             // nr / r_max
};

// d = project(X, camera) - (u, v) and e = |d|, the forward model of sba_model.hpp (obs_project) without contraction
__device__ __forceinline__ void rp_residual(const double* __restrict__ cp, double X0, double X1, double X2, double u, double v,
                                            double& du, double& dv, double& e) {
#pragma clang fp contract(off)
  const double p0 = cp[CP_R + 0] * X0 + cp[CP_R + 1] * X1 + cp[CP_R + 2] * X2 + cp[CP_T + 0];
  const double p1 = cp[CP_R + 3] * X0 + cp[CP_R + 4] * X1 + cp[CP_R + 5] * X2 + cp[CP_T + 1];
  const double p2 = cp[CP_R + 6] * X0 + cp[CP_R + 7] * X1 + cp[CP_R + 8] * X2 + cp[CP_T + 2];
  const double iz = 1.0 / p2;
  const double x = p0 * iz, y = p1 * iz;
  const double n = x * x + y * y;
  const double d = 1.0 + n * (cp[CP_K1] + cp[CP_K2] * n);
  double xd = d * x, yd = d * y;
  if constexpr (TANGENTIAL) {
    const double tp1 = cp[CP_P1], tp2 = cp[CP_P2], xy2 = 2.0 * x * y;
    xd = xd + tp1 * xy2 + tp2 * (n + 2.0 * x * x);
    yd = yd + tp1 * (n + 2.0 * y * y) + tp2 * xy2;
  }
  du = (cp[CP_F] * xd + cp[CP_CX]) - u;
  dv = (cp[CP_F] * yd + cp[CP_CY]) - v;
  e = sqrt(du * du + dv * dv);
}

__device__ __forceinline__ bool rp_selected(int select, bool has_w, double w) {
  return select == 0 || (select == 1 ? (!has_w || w > 0.0) : (has_w && w == 0.0));
}
// min(nb - 1, floor(x)) for x >= 0 (infinity included), without converting an out-of-range value
__device__ __forceinline__ int rp_bin(double x, int nb) {
  const double t = floor(x);
  return t >= (double)(nb - 1) ? nb - 1 : (int)t;
}
__device__ __forceinline__ int rp_cell(double x, int nb) {          // clamp(floor(x), 0, nb - 1)
  const double t = floor(x);
  return t >= (double)(nb - 1) ? nb - 1 : t > 0.0 ? (int)t : 0;
}

// thread b adds the staged records of bin b in index order: [n, three sums] into out[b * 4 ..]
__device__ __forceinline__ void rp_walk(const short* __restrict__ s_bin, const double* __restrict__ s_val, int cnt, int nb,
                                        double* __restrict__ out) {
  const int b = threadIdx.x;
  if (b >= nb) return;
  double n = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int i = 0; i < cnt; ++i)
    if (s_bin[i] == b) { n += 1.0; s0 += s_val[3 * i]; s1 += s_val[3 * i + 1]; s2 += s_val[3 * i + 2]; }
  out[4 * b] = n; out[4 * b + 1] = s0; out[4 * b + 2] = s1; out[4 * b + 3] = s2;
}

template <typename T>
__global__ void __launch_bounds__(RP_BLOCK) k_rp_cams(const double* __restrict__ campre, const double* __restrict__ pts,
                                                       const typename Vec2<T>::type* __restrict__ uv, const T* __restrict__ w,
                                                       const int32_t* __restrict__ pi, const int32_t* __restrict__ chunk_cam,
                                                       const int32_t* __restrict__ chunk_begin, const int32_t* __restrict__ chunk_end,
                                                       RpBins o, double* __restrict__ part /*[chunk][RP_REC]*/,
                                                       unsigned long long* __restrict__ hist /*[C][B]*/,
                                                       double* __restrict__ grid_part /*[chunk][gx gy][4] or NULL*/,
                                                       double* __restrict__ rad_part /*[chunk][nr][4] or NULL*/) {
  extern __shared__ unsigned int s_hist[];          // [B]
  __shared__ double s_cp[CAMPRE];
  __shared__ double s_val[CM_CHUNK * 3];
  __shared__ short s_bin[CM_CHUNK];
  __shared__ double s_red[RP_WAVES][RP_REC];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int chunk = blockIdx.x;
  const int c = chunk_cam[chunk], begin = chunk_begin[chunk], cnt = min(chunk_end[chunk] - begin, CM_CHUNK);
  if (tid < CAMPRE) s_cp[tid] = campre[(size_t)c * CAMPRE + tid];
  for (int k = tid; k < o.B; k += RP_BLOCK) s_hist[k] = 0u;
  __syncthreads();
  const double cx = s_cp[CP_CX], cy = s_cp[CP_CY];
  double v[RP_REC];
#pragma unroll
  for (int k = 0; k < RP_REC; ++k) v[k] = 0.0;
  double du[RP_PER], dv[RP_PER], e2[RP_PER], ra[RP_PER], ta[RP_PER];
  short cell[RP_PER], rbin[RP_PER];
#pragma unroll
  for (int j = 0; j < RP_PER; ++j) {
    const int s = j * RP_BLOCK + tid;
    du[j] = 0.0; dv[j] = 0.0; e2[j] = 0.0; ra[j] = 0.0; ta[j] = 0.0; cell[j] = -1; rbin[j] = -1;
    if (s >= cnt) continue;
    const size_t i = (size_t)begin + s;
    const auto m = uv[i];
    const double uu = (double)m.x, vv = (double)m.y;
    const double ww = w ? (double)w[i] : 1.0;
    if (!rp_selected(o.select, w != nullptr, ww)) continue;
    v[RP_SEL] += 1.0;
    const double* X = pts + (size_t)pi[i] * 3;
    double a, b, e;
    rp_residual(s_cp, X[0], X[1], X[2], uu, vv, a, b, e);
    if (!isfinite(a) || !isfinite(b)) { v[RP_BAD] += 1.0; continue; }
    du[j] = a; dv[j] = b; e2[j] = e * e;
    v[RP_N] += 1.0; v[RP_DU] += a; v[RP_DV] += b; v[RP_E] += e; v[RP_E2] += e * e;
    v[RP_MAX] = fmax(v[RP_MAX], e);
    atomicAdd(&s_hist[rp_bin(e * o.inv, o.B)], 1u);
    if (o.gx > 0) cell[j] = (short)(rp_cell(vv * o.qy, o.gy) * o.gx + rp_cell(uu * o.qx, o.gx));
    if (o.nr > 0) {
      const double dx = uu - cx, dy = vv - cy;
      const double r = sqrt(dx * dx + dy * dy);
      rbin[j] = (short)rp_bin(r * o.qr, o.nr);
      if (r > 0.0) {
        const double rx = dx / r, ry = dy / r;
        ra[j] = a * rx + b * ry;
        ta[j] = rx * b - ry * a;
      }
    }
  }
  // ---- the record of the chunk: in the wave, then the waves in wave order
#pragma unroll
  for (int k = 0; k < RP_REC; ++k) {
    const double r = k < RP_NSUM ? wave_sum(v[k]) : wave_max(v[k]);
    if (lane == 0) s_red[wid][k] = r;
  }
  __syncthreads();                                   // (the LDS histogram is complete here too)
  if (tid < RP_REC) {
    double r = s_red[0][tid];
    for (int q = 1; q < RP_WAVES; ++q) r = tid < RP_NSUM ? r + s_red[q][tid] : fmax(r, s_red[q][tid]);
    part[(size_t)chunk * RP_REC + tid] = r;
  }
  for (int k = tid; k < o.B; k += RP_BLOCK) {
    const unsigned int hcount = s_hist[k];
    if (hcount) atomicAdd(&hist[(size_t)c * o.B + k], (unsigned long long)hcount);
  }
  // ---- binned sums: the residual field, then the radial profile, through the same staging area
  if (grid_part) {
#pragma unroll
    for (int j = 0; j < RP_PER; ++j) {
      const int s = j * RP_BLOCK + tid;
      s_bin[s] = cell[j];
      s_val[3 * s] = du[j]; s_val[3 * s + 1] = dv[j]; s_val[3 * s + 2] = e2[j];
    }
    __syncthreads();
    rp_walk(s_bin, s_val, cnt, o.gx * o.gy, grid_part + (size_t)chunk * (o.gx * o.gy) * 4);
    __syncthreads();
  }
  if (rad_part) {
#pragma unroll
    for (int j = 0; j < RP_PER; ++j) {
      const int s = j * RP_BLOCK + tid;
      s_bin[s] = rbin[j];
      s_val[3 * s] = ra[j]; s_val[3 * s + 1] = ta[j]; s_val[3 * s + 2] = e2[j];
    }
    __syncthreads();
    rp_walk(s_bin, s_val, cnt, o.nr, rad_part + (size_t)chunk * o.nr * 4);
  }
}

// entry k (of rec) of camera c: the partial records of its chunks in chunk order; entries from nsum on are maxima
__global__ void __launch_bounds__(256) k_rp_fold(const double* __restrict__ part, int rec, int nsum,
                                                  const int32_t* __restrict__ cam_chunk_start, int C, double* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= C * rec) return;
  const int c = t / rec, k = t - c * rec;
  double r = 0.0;
  if (k < nsum) for (int ch = cam_chunk_start[c]; ch < cam_chunk_start[c + 1]; ++ch) r += part[(size_t)ch * rec + k];
  else for (int ch = cam_chunk_start[c]; ch < cam_chunk_start[c + 1]; ++ch) r = fmax(r, part[(size_t)ch * rec + k]);
  out[t] = r;
}

template <typename T>
__global__ void __launch_bounds__(256) k_rp_obs(const double* __restrict__ campre, const double* __restrict__ pts,
                                                 const typename Vec2<T>::type* __restrict__ uv, const int32_t* __restrict__ ci,
                                                 const int32_t* __restrict__ pi, int64_t M, double* __restrict__ e_pm) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= M) return;
  const auto m = uv[k];
  const double* X = pts + (size_t)pi[k] * 3;
  double a, b, e;
  rp_residual(campre + (size_t)ci[k] * CAMPRE, X[0], X[1], X[2], (double)m.x, (double)m.y, a, b, e);
  e_pm[k] = (isfinite(a) && isfinite(b)) ? e : __builtin_nan("");
}

// [n, rms, max] of every point.  The sum runs over the point's observations by ascending camera (position breaks a tie): the
// order the layout leaves on rigs of up to 16 cameras; larger rigs keep the caller's order inside a point, and a point whose
// cameras do not ascend is walked by repeated selection of the next key (quadratic in its views, at most 256).
template <typename T>
__global__ void __launch_bounds__(256) k_rp_points(const double* __restrict__ e_pm, const T* __restrict__ w, const int32_t* __restrict__ ci,
                                                    const int32_t* __restrict__ pt_start, int N, int select, double* __restrict__ pt_stats) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= N) return;
  const int a = pt_start[p], b = pt_start[p + 1];
  double n = 0.0, s = 0.0, mx = 0.0;
  bool sorted = true;
  int last = -1;
  for (int k = a; k < b; ++k) {
    const int c = ci[k];
    sorted = sorted && c >= last;
    last = c;
    const double e = e_pm[k];
    if (e != e || !rp_selected(select, w != nullptr, w ? (double)w[k] : 1.0)) continue;
    n += 1.0; s += e * e; mx = fmax(mx, e);
  }
  if (!sorted) {
    s = 0.0;
    int lc = -1, lk = -1;
    for (int it = a; it < b; ++it) {
      int bc = 0x7fffffff, bk = 0x7fffffff;
      for (int k = a; k < b; ++k) {
        const int c = ci[k];
        if ((c > lc || (c == lc && k > lk)) && (c < bc || (c == bc && k < bk))) { bc = c; bk = k; }
      }
      lc = bc; lk = bk;
      const double e = e_pm[bk];
      if (e != e || !rp_selected(select, w != nullptr, w ? (double)w[bk] : 1.0)) continue;
      s += e * e;
    }
  }
  const double nan = __builtin_nan("");
  pt_stats[3 * (size_t)p] = n;
  pt_stats[3 * (size_t)p + 1] = n > 0.0 ? sqrt(s / n) : nan;
  pt_stats[3 * (size_t)p + 2] = n > 0.0 ? mx : nan;
}

template <typename T>
__global__ void __launch_bounds__(256) k_rp_compact(const double* __restrict__ e_pm, const T* __restrict__ w, int64_t M, int select,
                                                     double inv, int B, int kcut, unsigned int cap, int32_t* __restrict__ pos,
                                                     double* __restrict__ val, unsigned int* __restrict__ counter) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= M) return;
  const double e = e_pm[k];
  if (e != e || !rp_selected(select, w != nullptr, w ? (double)w[k] : 1.0)) return;
  if (rp_bin(e * inv, B) < kcut) return;
  const unsigned int slot = atomicAdd(counter, 1u);
  if (slot < cap) { pos[slot] = (int32_t)k; val[slot] = e; }
}

// ------------------------------------------------------------------ host
// quantile q of an integer histogram (include/sba_hip.h): n its total, m the largest error
inline double rp_quantile(const int64_t* h, int B, int64_t n, double m, double q, double bin_px) {
  if (n <= 0) return std::nan("");
  const double t = q * (double)n;
  int64_t cum = 0;
  for (int k = 0; k < B; ++k) {
    const int64_t before = cum;
    cum += h[k];
    if ((double)cum >= t) {
      if (k == B - 1) return m;
      return ((double)k + (t - (double)before) / (double)h[k]) * bin_px;
    }
  }
  return m;
}

// what the engine hands over: its current parameters and both observation layouts, all device pointers
template <typename T>
struct RpIn {
  hipStream_t stream;
  int C, N;
  int64_t M;
  const double *cams, *pts;
  const typename Vec2<T>::type *uv_cm, *uv_pm;
  const T *w_cm, *w_pm;              // NULL: the handle has no weights
  const int32_t *pi_cm, *ci_pm, *pi_pm, *pt_start;
  const int32_t *chunk_cam, *chunk_begin, *chunk_end, *cam_chunk_start;
  int nchunk;
  const int64_t* perm;               // host: layout position -> caller's index, or NULL for the identity
};

template <typename T>
int rp_run(const RpIn<T>& in, const sba_reproj_opts& opt, double* cam_stats, int64_t* cam_hist, double* cam_grid, double* cam_radial,
           double* pt_stats, double* err_out, int64_t* worst_idx, double* worst_err, sba_reproj_report* rep, std::string& err) {
  const auto t_start = std::chrono::steady_clock::now();
  // ---- options
  auto bad = [&](const char* what) { err = std::string("sba_reproj_stats: ") + what; return (int)SBA_ERR_INVALID; };
  if (opt.select < 0 || opt.select > 2) return bad("select must be 0, 1 or 2");
  if (opt.hist_bins != 0 && (opt.hist_bins < 2 || opt.hist_bins > 4096)) return bad("hist_bins must be 0 or 2..4096");
  if (opt.hist_bin_px != 0.0 && (!(opt.hist_bin_px > 0.0) || !std::isfinite(opt.hist_bin_px))) return bad("hist_bin_px must be positive and finite");
  const bool grid_on = opt.grid_x != 0 || opt.grid_y != 0;
  if (grid_on && (opt.grid_x < 1 || opt.grid_y < 1 || (int64_t)opt.grid_x * opt.grid_y > RP_MAX_BINS))
    return bad("grid_x and grid_y must be 0, 0 or at least 1 each with grid_x * grid_y <= 256");
  if (opt.radial_bins < 0 || opt.radial_bins > 64) return bad("radial_bins must be 0..64");
  if (opt.n_worst < 0 || opt.n_worst > 4096) return bad("n_worst must be 0..4096");
  if (!(opt.r_max_px >= 0.0) || !std::isfinite(opt.r_max_px)) return bad("r_max_px must be finite and not negative");
  const bool need_size = grid_on || (opt.radial_bins > 0 && opt.r_max_px == 0.0);
  if (need_size && (!(opt.width > 0.0) || !(opt.height > 0.0) || !std::isfinite(opt.width) || !std::isfinite(opt.height)))
    return bad("width and height must be positive and finite when the grid is on, or radial bins without r_max_px");
  const int B = opt.hist_bins ? opt.hist_bins : 1024;
  const double bin_px = opt.hist_bin_px != 0.0 ? opt.hist_bin_px : 1.0 / 16;
  const int G = grid_on ? opt.grid_x * opt.grid_y : 0;
  const int nr = opt.radial_bins;
  const int K = opt.n_worst;
  const bool do_grid = G > 0 && cam_grid != nullptr, do_rad = nr > 0 && cam_radial != nullptr;
  const bool want_worst = K > 0 && (worst_idx || worst_err || rep);
  RpBins o{};
  o.select = opt.select; o.B = B; o.inv = 1.0 / bin_px;
  if (do_grid) { o.gx = opt.grid_x; o.gy = opt.grid_y; o.qx = opt.grid_x / opt.width; o.qy = opt.grid_y / opt.height; }
  if (do_rad) {
    const double r_max = opt.r_max_px != 0.0 ? opt.r_max_px : 0.5 * std::sqrt(opt.width * opt.width + opt.height * opt.height);
    o.nr = nr; o.qr = nr / r_max;
  }
  ArenaScope own(nullptr);          // private buffers: hipMalloc'd here, freed on return (the handle's arena stays as it was)
  hipStream_t st = in.stream;
  const int C = in.C, N = in.N, nchunk = in.nchunk;
  const int64_t M = in.M;
  const bool need_e = M > 0 && (err_out || pt_stats || want_worst);
  DevEvents<4> ev;
  DevBuf<double> campre, part, tot, grid_part, grid_tot, rad_part, rad_tot, e_pm, ptst, wval;
  DevBuf<unsigned long long> hist;
  DevBuf<int32_t> wpos;
  DevBuf<unsigned int> counter;
  campre.alloc((size_t)C * CAMPRE);
  tot.alloc((size_t)C * RP_REC);
  hist.alloc((size_t)C * B);
  hist.zero(st);
  if (nchunk > 0) part.alloc((size_t)nchunk * RP_REC);
  if (do_grid) { grid_tot.alloc((size_t)C * G * 4); if (nchunk > 0) grid_part.alloc((size_t)nchunk * G * 4); }
  if (do_rad) { rad_tot.alloc((size_t)C * nr * 4); if (nchunk > 0) rad_part.alloc((size_t)nchunk * nr * 4); }
  if (need_e) e_pm.alloc((size_t)M);
  if (pt_stats && N > 0) ptst.alloc((size_t)N * 3);
  // ---- [ev0, ev1): both passes
  HIPCHK(hipEventRecord(ev[0], st));
  hipLaunchKernelGGL(k_cam_prep<double>, dim3((C + 63) / 64), dim3(64), 0, st, in.cams, campre.p, C);
  if (nchunk > 0)
    hipLaunchKernelGGL(k_rp_cams<T>, dim3(nchunk), dim3(RP_BLOCK), (size_t)B * sizeof(unsigned int), st, (const double*)campre.p, in.pts,
                       in.uv_cm, in.w_cm, in.pi_cm, in.chunk_cam, in.chunk_begin, in.chunk_end, o, part.p, hist.p, grid_part.p, rad_part.p);
  auto fold = [&](const DevBuf<double>& src, int rec, int nsum, DevBuf<double>& dst) {
    hipLaunchKernelGGL(k_rp_fold, dim3((C * rec + 255) / 256), dim3(256), 0, st, (const double*)src.p, rec, nsum, in.cam_chunk_start, C, dst.p);
  };
  // (a handle without observations has no chunk table: its totals are the zeros below)
  if (nchunk > 0) {
    fold(part, RP_REC, RP_NSUM, tot);
    if (do_grid) fold(grid_part, G * 4, G * 4, grid_tot);
    if (do_rad) fold(rad_part, nr * 4, nr * 4, rad_tot);
  } else {
    tot.zero(st); grid_tot.zero(st); rad_tot.zero(st);
  }
  if (need_e)
    hipLaunchKernelGGL(k_rp_obs<T>, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, (const double*)campre.p, in.pts, in.uv_pm, in.ci_pm,
                       in.pi_pm, M, e_pm.p);
  if (ptst.n && need_e)
    hipLaunchKernelGGL(k_rp_points<T>, dim3((N + 255) / 256), dim3(256), 0, st, (const double*)e_pm.p, in.w_pm, in.ci_pm, in.pt_start, N,
                       (int)opt.select, ptst.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ev[1], st));
  // ---- read-back into private host arrays: a failed call leaves the caller's untouched
  std::vector<double> h_tot((size_t)C * RP_REC), h_grid(grid_tot.n), h_rad(rad_tot.n), h_pt(ptst.n), h_e(err_out ? (size_t)M : 0);
  std::vector<int64_t> h_hist((size_t)C * B);
  auto fetch = [&](void* dst, const void* src, size_t bytes) { if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st)); };
  fetch(h_tot.data(), tot.p, sizeof(double) * h_tot.size());
  fetch(h_hist.data(), hist.p, sizeof(int64_t) * h_hist.size());
  fetch(h_grid.data(), grid_tot.p, sizeof(double) * h_grid.size());
  fetch(h_rad.data(), rad_tot.p, sizeof(double) * h_rad.size());
  fetch(h_pt.data(), ptst.p, sizeof(double) * h_pt.size());
  if (need_e) fetch(h_e.data(), e_pm.p, sizeof(double) * h_e.size());
  HIPCHK(hipStreamSynchronize(st));
  // ---- global values from the per-camera sums, in camera order; the histogram of all cameras
  const double nan = std::nan("");
  double g[RP_REC] = {};
  std::vector<int64_t> total((size_t)B, 0);
  for (int c = 0; c < C; ++c) {
    for (int k = 0; k < RP_NSUM; ++k) g[k] += h_tot[(size_t)c * RP_REC + k];
    g[RP_MAX] = std::fmax(g[RP_MAX], h_tot[(size_t)c * RP_REC + RP_MAX]);
    for (int k = 0; k < B; ++k) total[k] += h_hist[(size_t)c * B + k];
  }
  const int64_t n_fin = (int64_t)g[RP_N];
  // ---- the K worst: the lowest bin at and above which at least K observations lie, then a compaction of exactly those
  std::vector<int64_t> w_idx;
  std::vector<double> w_err;
  float ms_worst = 0.f;
  if (want_worst && n_fin > 0) {
    int kcut = 0;
    int64_t cnt = n_fin;
    int64_t acc = 0;
    for (int k = B - 1; k >= 0; --k) {
      acc += total[k];
      if (acc >= K) { kcut = k; cnt = acc; break; }
    }
    if (cnt > (int64_t)0x7fffffff) { err = "sba_reproj_stats: too many candidates for the worst list"; return SBA_ERR_UNSUPPORTED; }
    wpos.alloc((size_t)cnt); wval.alloc((size_t)cnt); counter.alloc(1);
    counter.zero(st);
    HIPCHK(hipEventRecord(ev[2], st));
    hipLaunchKernelGGL(k_rp_compact<T>, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, (const double*)e_pm.p, in.w_pm, M, (int)opt.select,
                       o.inv, B, kcut, (unsigned int)cnt, wpos.p, wval.p, counter.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev[3], st));
    std::vector<int32_t> h_pos((size_t)cnt);
    std::vector<double> h_val((size_t)cnt);
    unsigned int h_cnt = 0;
    fetch(h_pos.data(), wpos.p, sizeof(int32_t) * h_pos.size());
    fetch(h_val.data(), wval.p, sizeof(double) * h_val.size());
    fetch(&h_cnt, counter.p, sizeof h_cnt);
    HIPCHK(hipStreamSynchronize(st));
    ms_worst = ev.ms(2, 3);
    if ((int64_t)h_cnt != cnt) { err = "sba_reproj_stats: the compaction disagrees with the histogram"; return SBA_ERR_HIP; }
    std::vector<int64_t> order((size_t)cnt);
    std::vector<int64_t> idx((size_t)cnt);
    for (int64_t j = 0; j < cnt; ++j) { order[j] = j; idx[j] = in.perm ? in.perm[h_pos[j]] : (int64_t)h_pos[j]; }
    std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return h_val[x] > h_val[y] || (h_val[x] == h_val[y] && idx[x] < idx[y]); });
    const int64_t keep = std::min<int64_t>(K, cnt);
    for (int64_t j = 0; j < keep; ++j) { w_idx.push_back(idx[order[j]]); w_err.push_back(h_val[order[j]]); }
  }
  const float ms_main = ev.ms(0, 1);
  // ---- outputs
  for (int c = 0; c < C; ++c) {
    const double* r = h_tot.data() + (size_t)c * RP_REC;
    const int64_t n = (int64_t)r[RP_N];
    if (cam_stats) {
      double* s = cam_stats + (size_t)c * 9;
      s[0] = (double)n;
      if (n > 0) {
        s[1] = r[RP_DU] / n; s[2] = r[RP_DV] / n; s[3] = r[RP_E] / n; s[4] = std::sqrt(r[RP_E2] / n); s[5] = r[RP_MAX];
        const double qs[3] = {0.5, 0.95, 0.99};
        for (int k = 0; k < 3; ++k) s[6 + k] = rp_quantile(h_hist.data() + (size_t)c * B, B, n, r[RP_MAX], qs[k], bin_px);
      } else for (int k = 1; k < 9; ++k) s[k] = nan;
    }
  }
  if (cam_hist) std::copy(h_hist.begin(), h_hist.end(), cam_hist);
  auto binned = [&](const std::vector<double>& src, double* dst) {       // [n, sum a, sum b, sum e^2] -> [n, mean a, mean b, rms]
    for (size_t k = 0; k < src.size() / 4; ++k) {
      const double n = src[4 * k];
      dst[4 * k] = n;
      dst[4 * k + 1] = n > 0.0 ? src[4 * k + 1] / n : nan;
      dst[4 * k + 2] = n > 0.0 ? src[4 * k + 2] / n : nan;
      dst[4 * k + 3] = n > 0.0 ? std::sqrt(src[4 * k + 3] / n) : nan;
    }
  };
  if (do_grid) binned(h_grid, cam_grid);
  if (do_rad) binned(h_rad, cam_radial);
  if (pt_stats) {
    if (need_e) std::copy(h_pt.begin(), h_pt.end(), pt_stats);
    else for (int p = 0; p < N; ++p) { pt_stats[3 * (size_t)p] = 0.0; pt_stats[3 * (size_t)p + 1] = nan; pt_stats[3 * (size_t)p + 2] = nan; }
  }
  if (err_out) for (int64_t k = 0; k < M; ++k) err_out[in.perm ? in.perm[k] : k] = h_e[k];
  for (int k = 0; k < K; ++k) {
    const bool have = k < (int)w_idx.size();
    if (worst_idx) worst_idx[k] = have ? w_idx[k] : -1;
    if (worst_err) worst_err[k] = have ? w_err[k] : nan;
  }
  if (rep) {
    *rep = sba_reproj_report{};
    rep->n_selected = (int64_t)g[RP_SEL];
    rep->n_unselected = M - rep->n_selected;
    rep->n_nonfinite = (int64_t)g[RP_BAD];
    rep->n_overflow = total[B - 1];
    rep->n_worst = (int32_t)w_idx.size();
    if (n_fin > 0) {
      rep->mean_du = g[RP_DU] / n_fin; rep->mean_dv = g[RP_DV] / n_fin; rep->mean = g[RP_E] / n_fin;
      rep->rms = std::sqrt(g[RP_E2] / n_fin); rep->max = g[RP_MAX];
    } else { rep->mean_du = nan; rep->mean_dv = nan; rep->mean = nan; rep->rms = nan; rep->max = nan; }
    rep->q50 = rp_quantile(total.data(), B, n_fin, g[RP_MAX], 0.5, bin_px);
    rep->q95 = rp_quantile(total.data(), B, n_fin, g[RP_MAX], 0.95, bin_px);
    rep->q99 = rp_quantile(total.data(), B, n_fin, g[RP_MAX], 0.99, bin_px);
    rep->seconds_device = (ms_main + ms_worst) * 1e-3;
    rep->seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
  }
  return SBA_OK;
}

}  // namespace SBA_NS
