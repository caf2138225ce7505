// sba_detect.hpp -- sba_detect_dots (include/sba_hip.h): thresholded image moments of video frames, one laser dot per frame.
// Stands in for green_laser_finder_faster (lasercalib/feature_detection.py:44-54: cv.threshold + cv.moments) and, through the
// SPREAD status, for the "exactly one connected component" rule of green_laser_finder (:24-40) -- a one-pass stand-in on the
// bounding box of the bright pixels; the rule itself, with morphology and labelling, is sba_detect_blobs (sba_blobs.hpp).
//
// Three kernels per chunk of frames: k_dot_init (sums = 0, box = [W, H, -1, -1]), k_dot_moments (the streaming reduction,
// one workgroup per band of rows of one frame) and k_dot_finalize (one thread per frame: centroid and status).
//
// Every sum is an exact unsigned 64-bit integer.  With width, height <= DOT_MAX_DIM = 16384 and 8-bit pixels the sums of a
// whole frame are bounded by
//   sum m x^2 <= H W^3 / 3        = 16384^4 / 3       = 2.4e16        sum m x y <= (W^2 / 2)(H^2 / 2) = 1.8e16
//   sum w x   <= 255 H W^2 / 2    = 255 16384^3 / 2   = 5.6e14        sum w     <= 255 H W            = 6.8e10
// and even a weighted second moment (the two reserved slots could hold one) by sum w x^2 <= 255 * 16384 * 16384^3 / 3 = 6.1e18,
// all below 2^64 = 1.8e19.  Integer addition commutes, so the integer atomics that merge the workgroups' partial sums give the
// same bits on every run; there is no floating-point atomic.
//
// How the frames are read -- the regions, the walk over a row's bytes, the decode of 16 of them, the staging of host frames
// chunk by chunk -- is sba_frames.hpp, shared with sba_blobs.hpp; here is what is done with a pixel (DotSink) and with the sums.
#pragma once
#include "sba_frames.hpp"

namespace sba_detect {

constexpr int DOT_NSUM = 12;                 // slots of one frame's row of `sums`; the kernel fills the first DOT_NACC
constexpr int DOT_NACC = 10;

struct DotParams : FrameView {
  int32_t rows_per_band;
  int32_t min_area, max_area, max_extent;
};

// sums of one lane over one row: 32 bits hold n <= 16384, sum x <= 16384 * 16383 / 2 = 1.3e8, sum w <= 255 * 16384 = 4.2e6 of a
// WHOLE row (a lane sees a part of it); sum x^2 <= 1.5e12 and sum w x <= 3.4e10 of a row need 64
struct DotRow {
  uint32_t n, sx, w, sat;
  unsigned long long sxx, wx;
  int xmin, xmax;
};
struct DotAcc {
  unsigned long long s[DOT_NACC];            // n, sx, sy, sxx, syy, sxy, sw, swx, swy, n_sat
  int xmin, ymin, xmax, ymax;
};

// scan_row's sink: folds one group of NPIX pixels at x = xq, xq + 1, ... with the values v into R; wv = max(value - threshold, 0).
// The small sums over k fit 32 bits (NPIX <= 16: sum k^2 <= 1240, sum w k <= 255 * 120), then x = xq + k gives
//   sum m x = xq n + sum m k,   sum m x^2 = xq (xq n + 2 sum m k) + sum m k^2,   sum w x = xq sum w + sum w k.
struct DotSink {
  DotRow R;
  uint32_t thr, wsat;                        // value 255 <=> wv == wsat
  template <int NPIX>
  __device__ __forceinline__ void operator()(uint32_t xq, const uint32_t (&v)[NPIX]) {
    uint32_t n = 0, sk = 0, skk = 0, w = 0, wk = 0, sat = 0, lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < NPIX; ++k) {
      const uint32_t wv = v[k] > thr ? v[k] - thr : 0u, m = min(wv, 1u);
      n += m; sk += m * (uint32_t)k; skk += m * (uint32_t)(k * k);
      w += wv; wk += wv * (uint32_t)k;
      sat += wv == wsat ? 1u : 0u;
      lo = max(lo, m * (uint32_t)(NPIX - k));      // NPIX - (smallest k with m)
      hi = max(hi, m * (uint32_t)(k + 1));         // 1 + (largest k with m)
    }
    if (n == 0) return;
    const uint32_t xn = xq * n;                     // <= 16383 * 16
    R.n += n; R.sx += xn + sk;
    R.sxx += (unsigned long long)xq * (xn + 2 * sk) + skk;
    R.w += w; R.wx += (unsigned long long)xq * w + wk;
    R.sat += sat;
    R.xmin = min(R.xmin, (int)(xq + NPIX - lo));
    R.xmax = max(R.xmax, (int)(xq + hi - 1));
  }
};

__device__ __forceinline__ unsigned long long dot_wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ int dot_wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_down(v, o, 64));
  return v;
}
__device__ __forceinline__ int dot_wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_down(v, o, 64));
  return v;
}

__global__ void k_dot_init(unsigned long long* __restrict__ sums, int* __restrict__ box, int n_frames, int width, int height) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_frames) return;
  for (int k = 0; k < DOT_NSUM; ++k) sums[(size_t)f * DOT_NSUM + k] = 0;
  box[4 * f] = width; box[4 * f + 1] = height; box[4 * f + 2] = -1; box[4 * f + 3] = -1;
}

// grid (bands, frames), DOT_THREADS threads.  Wave w of the workgroup takes rows y0 + band * rows_per_band + w, + w + 4, ...
// Of a row it reads the pixels inside both regions (frame_row_span, scan_row).
template <int C>
__global__ void __launch_bounds__(DOT_THREADS) k_dot_moments(const DotParams P, unsigned long long* __restrict__ sums, int* __restrict__ box) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.y;
  const uint32_t thr = (uint32_t)P.threshold, channel = (uint32_t)P.channel;
  const uint32_t wsat = thr < 255u ? 255u - thr : 0xffffffffu;           // value 255 <=> w == 255 - thr; nothing passes thr = 255
  const int band_lo = P.y0 + (int)blockIdx.x * P.rows_per_band;
  const int band_hi = min(P.y1, band_lo + P.rows_per_band);
  const uint8_t* __restrict__ fp = P.frames + (int64_t)f * P.frame_pitch;

  DotAcc A;
#pragma unroll
  for (int k = 0; k < DOT_NACC; ++k) A.s[k] = 0;
  A.xmin = P.width; A.ymin = P.height; A.xmax = -1; A.ymax = -1;

  for (int y = band_lo + wave; y < band_hi; y += DOT_WAVES) {
    int xa, xb;
    // True as long as band_lo is P.y0 plus something >= 0.  It is here for the registers: it lets the compiler drop the row test of
    // frame_row_span, which otherwise costs C = 4 five VGPRs and one wave of occupancy.
    __builtin_assume(y >= P.y0);
    if (!frame_row_span(P, y, xa, xb)) continue;
    DotSink S{{0, 0, 0, 0, 0, 0, P.width, -1}, thr, wsat};
    scan_row<C>(fp + (int64_t)y * P.row_pitch, xa, xb, channel, thr, S);
    const DotRow& R = S.R;
    if (R.n) {
      const uint32_t uy = (uint32_t)y, ny = R.n * uy;                    // <= 16384 * 16383
      A.s[0] += R.n; A.s[1] += R.sx; A.s[2] += ny;
      A.s[3] += R.sxx; A.s[4] += (unsigned long long)ny * uy; A.s[5] += (unsigned long long)R.sx * uy;
      A.s[6] += R.w; A.s[7] += R.wx; A.s[8] += (unsigned long long)R.w * uy; A.s[9] += R.sat;
      A.xmin = min(A.xmin, R.xmin); A.xmax = max(A.xmax, R.xmax);
      A.ymin = min(A.ymin, y); A.ymax = max(A.ymax, y);
    }
  }

  __shared__ unsigned long long s_sum[DOT_WAVES][DOT_NACC];
  __shared__ int s_box[DOT_WAVES][4];
#pragma unroll
  for (int k = 0; k < DOT_NACC; ++k) {
    const unsigned long long t = dot_wave_sum(A.s[k]);
    if (lane == 0) s_sum[wave][k] = t;
  }
  const int bx0 = dot_wave_min(A.xmin), by0 = dot_wave_min(A.ymin), bx1 = dot_wave_max(A.xmax), by1 = dot_wave_max(A.ymax);
  if (lane == 0) { s_box[wave][0] = bx0; s_box[wave][1] = by0; s_box[wave][2] = bx1; s_box[wave][3] = by1; }
  __syncthreads();
  unsigned long long n_block = 0;
#pragma unroll
  for (int w = 0; w < DOT_WAVES; ++w) n_block += s_sum[w][0];
  if (n_block == 0) return;                                              // a dark band adds nothing
  const int t = threadIdx.x;
  if (t < DOT_NACC) {
    unsigned long long tot = 0;
#pragma unroll
    for (int w = 0; w < DOT_WAVES; ++w) tot += s_sum[w][t];
    if (tot) atomicAdd(&sums[(size_t)f * DOT_NSUM + t], tot);
  } else if (t < DOT_NACC + 4) {
    const int k = t - DOT_NACC;
    int r = s_box[0][k];
#pragma unroll
    for (int w = 1; w < DOT_WAVES; ++w) r = k < 2 ? min(r, s_box[w][k]) : max(r, s_box[w][k]);
    if (k < 2) atomicMin(&box[4 * f + k], r); else atomicMax(&box[4 * f + k], r);
  }
}

__global__ void k_dot_finalize(const unsigned long long* __restrict__ sums, const int* __restrict__ box, int n_frames, int min_area,
                               int max_area, int max_extent, double* __restrict__ centroid, int* __restrict__ status) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_frames) return;
  const unsigned long long* s = sums + (size_t)f * DOT_NSUM;
  const unsigned long long n = s[0];
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  double c0 = nan, c1 = nan, c2 = nan, c3 = nan;
  int st = SBA_DOT_NONE;
  if (n > 0) {
    c0 = (double)s[1] / (double)n; c1 = (double)s[2] / (double)n;       // one IEEE division of the two integers as doubles
    c2 = (double)s[7] / (double)s[6]; c3 = (double)s[8] / (double)s[6]; // sum w >= n > 0
    const int ext = max(box[4 * f + 2] - box[4 * f], box[4 * f + 3] - box[4 * f + 1]) + 1;
    if (n < (unsigned long long)min_area) st = SBA_DOT_TOO_SMALL;
    else if (max_area > 0 && n > (unsigned long long)max_area) st = SBA_DOT_TOO_LARGE;
    else if (max_extent > 0 && ext > max_extent) st = SBA_DOT_SPREAD;
    else st = SBA_DOT_OK;
  }
  centroid[4 * f] = c0; centroid[4 * f + 1] = c1; centroid[4 * f + 2] = c2; centroid[4 * f + 3] = c3;
  status[f] = st;
}

// ------------------------------------------------------------------------------------------------ host side
// init, moments and finalize of `nf` frames on stream st; P.frames points at the first of them
inline void dot_launch(DotParams P, int channels, int64_t nf, int64_t total_frames, unsigned long long* d_sums, int* d_box,
                       double* d_cen, int* d_st, hipStream_t st) {
  const unsigned fb = (unsigned)((nf + 255) / 256);
  hipLaunchKernelGGL(k_dot_init, dim3(fb), dim3(256), 0, st, d_sums, d_box, (int)nf, P.width, P.height);
  HIPCHK(hipGetLastError());
  const int64_t rows = (int64_t)P.y1 - P.y0;
  if (rows > 0 && P.x1 > P.x0) {
    const int rpb = P.rows_per_band = frame_rows_per_band(rows, total_frames);
    const dim3 grid((unsigned)((rows + rpb - 1) / rpb), (unsigned)nf);
    if (channels == 1) hipLaunchKernelGGL(k_dot_moments<1>, grid, dim3(DOT_THREADS), 0, st, P, d_sums, d_box);
    else if (channels == 3) hipLaunchKernelGGL(k_dot_moments<3>, grid, dim3(DOT_THREADS), 0, st, P, d_sums, d_box);
    else hipLaunchKernelGGL(k_dot_moments<4>, grid, dim3(DOT_THREADS), 0, st, P, d_sums, d_box);
    HIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_dot_finalize, dim3(fb), dim3(256), 0, st, d_sums, d_box, (int)nf, P.min_area, P.max_area, P.max_extent, d_cen, d_st);
  HIPCHK(hipGetLastError());
}

// Arguments are checked by the caller (sba_api.hip).  Device frames go DOT_MAX_CHUNK frames per launch, host frames
// chunk_frames (by default what fits DOT_STAGE_BYTES) per staging copy: frames_in_chunks.  Device memory besides its staging
// buffers: one set of results of a chunk, whatever n_frames is.
int dot_call(const FrameBatch& B, const sba_dot_opts& o, uint64_t* sums, int32_t* box, double* centroid, int32_t* status) {
  const int64_t n_frames = B.n_frames;
  if (n_frames == 0) return SBA_OK;
  HIPCHK(hipSetDevice(B.device));
  DotParams P{};
  static_cast<FrameView&>(P) = frame_view(B, o.channel, o.threshold, o.roi_rect, o.roi_circle);
  P.min_area = o.min_area; P.max_area = o.max_area; P.max_extent = o.max_extent;

  const bool on_device = o.frames_on_device != 0;
  const int64_t chunk = chunk_of(CHUNK_RECORDS, o.chunk_frames, B, on_device);

  DevBuf<unsigned long long> d_sums;
  DevBuf<int> d_box, d_st;
  DevBuf<double> d_cen;
  d_sums.alloc((size_t)chunk * DOT_NSUM); d_box.alloc((size_t)chunk * 4); d_cen.alloc((size_t)chunk * 4); d_st.alloc((size_t)chunk);
  frames_in_chunks(
      P, B.channels, n_frames, on_device, chunk,
      [&](const FrameView& V, int64_t, int64_t m, hipStream_t st) {
        static_cast<FrameView&>(P) = V;
        dot_launch(P, B.channels, m, n_frames, d_sums.p, d_box.p, d_cen.p, d_st.p, st);
      },
      [&](int64_t lo, int64_t m, hipStream_t st) {
        if (sums) HIPCHK(hipMemcpyAsync(sums + lo * DOT_NSUM, d_sums.p, sizeof(uint64_t) * m * DOT_NSUM, hipMemcpyDeviceToHost, st));
        if (box) HIPCHK(hipMemcpyAsync(box + lo * 4, d_box.p, sizeof(int32_t) * m * 4, hipMemcpyDeviceToHost, st));
        if (centroid) HIPCHK(hipMemcpyAsync(centroid + lo * 4, d_cen.p, sizeof(double) * m * 4, hipMemcpyDeviceToHost, st));
        if (status) HIPCHK(hipMemcpyAsync(status + lo, d_st.p, sizeof(int32_t) * m, hipMemcpyDeviceToHost, st));
      });
  return SBA_OK;
}

}  // namespace sba_detect
