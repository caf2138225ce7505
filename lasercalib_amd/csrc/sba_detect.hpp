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
#pragma once
#include "sba_common.hpp"

namespace sba_detect {
using namespace sba_host;

constexpr int DOT_THREADS = 256, DOT_WAVES = DOT_THREADS / 64;
constexpr int DOT_NSUM = 12;                 // slots of one frame's row of `sums`; the kernel fills the first DOT_NACC
constexpr int DOT_NACC = 10;
constexpr int DOT_MAX_DIM = 16384;
constexpr int DOT_UNROLL = 4;                // 16-byte loads a lane has in flight
constexpr int64_t DOT_STAGE_BYTES = (int64_t)64 << 20;     // default size of one staging buffer for host frames
constexpr int64_t DOT_MAX_CHUNK = 16384;     // frames per launch (grid.y) and per set of result buffers

struct DotParams {
  const uint8_t* frames;
  int64_t row_pitch, frame_pitch;
  int32_t height, width, channel, threshold;
  int32_t x0, y0, x1, y1;                    // the rectangle, clipped to the frame, half-open
  int32_t ccx, ccy;
  int64_t r2;                                // the circle's r^2; < 0 = no circle
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

// One group of NPIX pixels at x = xq, xq + 1, ...; wv[k] = max(value - threshold, 0).  The small sums over k fit 32 bits
// (NPIX <= 16: sum k^2 <= 1240, sum w k <= 255 * 120), then x = xq + k gives
//   sum m x = xq n + sum m k,   sum m x^2 = xq (xq n + 2 sum m k) + sum m k^2,   sum w x = xq sum w + sum w k.
template <int NPIX>
__device__ __forceinline__ void dot_fold(DotRow& R, uint32_t xq, const uint32_t (&wv)[NPIX], uint32_t wsat) {
  uint32_t n = 0, sk = 0, skk = 0, w = 0, wk = 0, sat = 0, lo = 0, hi = 0;
#pragma unroll
  for (int k = 0; k < NPIX; ++k) {
    const uint32_t m = min(wv[k], 1u);
    n += m; sk += m * (uint32_t)k; skk += m * (uint32_t)(k * k);
    w += wv[k]; wk += wv[k] * (uint32_t)k;
    sat += wv[k] == wsat ? 1u : 0u;
    lo = max(lo, m * (uint32_t)(NPIX - k));        // NPIX - (smallest k with m)
    hi = max(hi, m * (uint32_t)(k + 1));           // 1 + (largest k with m)
  }
  if (n == 0) return;
  const uint32_t xn = xq * n;                       // <= 16383 * 16
  R.n += n; R.sx += xn + sk;
  R.sxx += (unsigned long long)xq * (xn + 2 * sk) + skk;
  R.w += w; R.wx += (unsigned long long)xq * w + wk;
  R.sat += sat;
  R.xmin = min(R.xmin, (int)(xq + NPIX - lo));
  R.xmax = max(R.xmax, (int)(xq + hi - 1));
}

// The 16 bytes `v` start at byte s of the row.  Of the pixels whose thresholded channel lies in them, takes max(value - thr, 0);
// returns false, having done nothing else, when no lane of the wave has a pixel above the threshold (the usual case: frames are
// dark but for the dot).  A byte shifted in from beyond the 16 is zero and never above a threshold >= 0.
template <int C>
__device__ __forceinline__ bool dot_vector(DotRow& R, const uint4& v, uint32_t s, uint32_t channel, uint32_t thr, uint32_t wsat) {
  constexpr int NPIX = (16 + C - 1) / C;
  const uint32_t q = s / C, r = s - q * C;
  const uint32_t j0 = channel >= r ? channel - r : channel + C - r;      // first byte of the channel at or after s
  const uint32_t xq = q + (channel < r ? 1u : 0u);
  uint32_t d[4];
  if (C == 1) { d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w; }
  else {
    d[0] = __builtin_amdgcn_alignbyte(v.y, v.x, j0);
    d[1] = __builtin_amdgcn_alignbyte(v.z, v.y, j0);
    d[2] = __builtin_amdgcn_alignbyte(v.w, v.z, j0);
    d[3] = __builtin_amdgcn_alignbyte(0u, v.w, j0);
  }
  uint32_t w[NPIX], any = 0;
#pragma unroll
  for (int k = 0; k < NPIX; ++k) {                                       // byte k C of the 16: a constant after unrolling
    const uint32_t b = (d[(k * C) >> 2] >> (8 * ((k * C) & 3))) & 0xffu;
    w[k] = b > thr ? b - thr : 0u;
    any |= w[k];
  }
  if (!__any(any != 0)) return false;
  dot_fold<NPIX>(R, xq, w, wsat);
  return true;
}

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

// floor(sqrt(v)) for 0 <= v <= 2^62
__device__ __forceinline__ long long dot_isqrt(long long v) {
  long long d = (long long)sqrt((double)v);
  while (d * d > v) --d;
  while ((d + 1) * (d + 1) <= v) ++d;
  return d;
}

__global__ void k_dot_init(unsigned long long* __restrict__ sums, int* __restrict__ box, int n_frames, int width, int height) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_frames) return;
  for (int k = 0; k < DOT_NSUM; ++k) sums[(size_t)f * DOT_NSUM + k] = 0;
  box[4 * f] = width; box[4 * f + 1] = height; box[4 * f + 2] = -1; box[4 * f + 3] = -1;
}

// grid (bands, frames), DOT_THREADS threads.  Wave w of the workgroup takes rows y0 + band * rows_per_band + w, + w + 4, ...
// Of a row it reads the bytes [xa C, xb C) of the pixels inside both regions: the bytes up to the first 16-byte boundary of
// the ADDRESS and those behind the last one a byte per lane, the rest as aligned 16-byte loads, 64 lanes x DOT_UNROLL per step.
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
    int xa = P.x0, xb = P.x1;
    if (P.r2 >= 0) {
      const long long dy = (long long)y - P.ccy, rem = P.r2 - dy * dy;
      if (rem < 0) continue;
      const long long dx = dot_isqrt(rem);
      xa = (int)max((long long)xa, (long long)P.ccx - dx);
      xb = (int)min((long long)xb, (long long)P.ccx + dx + 1);
    }
    if (xa >= xb) continue;
    const uint8_t* __restrict__ rp = fp + (int64_t)y * P.row_pitch;
    const int bs = xa * C, be = xb * C;                                  // <= 16384 * 4
    const int head_end = min(be, bs + (int)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(rp + bs) & 15u)) & 15u));
    const int body_end = head_end + ((be - head_end) & ~15);
    DotRow R;
    R.n = 0; R.sx = 0; R.w = 0; R.sat = 0; R.sxx = 0; R.wx = 0; R.xmin = P.width; R.xmax = -1;

    {   // lanes 0..14: the bytes in front of the aligned body; lanes 32..46: those behind it
      const int b = lane < 32 ? bs + lane : body_end + (lane - 32);
      if (b < (lane < 32 ? head_end : be)) {
        const uint32_t q = (uint32_t)b / C;
        if ((uint32_t)b - q * C == channel) {
          const uint32_t v = rp[b];
          const uint32_t w1[1] = {v > thr ? v - thr : 0u};
          dot_fold<1>(R, q, w1, wsat);
        }
      }
    }
    for (int s0 = head_end + lane * 16; s0 < body_end + lane * 16; s0 += 64 * 16 * DOT_UNROLL) {   // the bound is wave-uniform
      uint4 v[DOT_UNROLL];
#pragma unroll
      for (int u = 0; u < DOT_UNROLL; ++u) {
        const int s = s0 + u * 64 * 16;
        v[u] = s < body_end ? *reinterpret_cast<const uint4*>(rp + s) : make_uint4(0u, 0u, 0u, 0u);
      }
#pragma unroll
      for (int u = 0; u < DOT_UNROLL; ++u) dot_vector<C>(R, v[u], (uint32_t)(s0 + u * 64 * 16), channel, thr, wsat);
    }
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
struct DotStream {
  hipStream_t s = nullptr;
  DotStream() { HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
  ~DotStream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
};
struct DotEvent {
  hipEvent_t e = nullptr;
  DotEvent() { HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); }
  ~DotEvent() { if (e) (void)hipEventDestroy(e); }
};

// init, moments and finalize of `nf` frames on stream st; P.frames points at the first of them
inline void dot_launch(DotParams P, int channels, int64_t nf, int64_t total_frames, unsigned long long* d_sums, int* d_box,
                       double* d_cen, int* d_st, hipStream_t st) {
  const unsigned fb = (unsigned)((nf + 255) / 256);
  hipLaunchKernelGGL(k_dot_init, dim3(fb), dim3(256), 0, st, d_sums, d_box, (int)nf, P.width, P.height);
  HIPCHK(hipGetLastError());
  const int64_t rows = (int64_t)P.y1 - P.y0;
  if (rows > 0 && P.x1 > P.x0) {
    // about 2048 workgroups over the whole call where the frames allow it, 4 to 32 rows each (one to eight per wave)
    int64_t rpb = rows * total_frames / 2048;
    rpb = std::max<int64_t>(DOT_WAVES, std::min<int64_t>(32, rpb / DOT_WAVES * DOT_WAVES));
    P.rows_per_band = (int)rpb;
    const dim3 grid((unsigned)((rows + rpb - 1) / rpb), (unsigned)nf);
    if (channels == 1) hipLaunchKernelGGL(k_dot_moments<1>, grid, dim3(DOT_THREADS), 0, st, P, d_sums, d_box);
    else if (channels == 3) hipLaunchKernelGGL(k_dot_moments<3>, grid, dim3(DOT_THREADS), 0, st, P, d_sums, d_box);
    else hipLaunchKernelGGL(k_dot_moments<4>, grid, dim3(DOT_THREADS), 0, st, P, d_sums, d_box);
    HIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_dot_finalize, dim3(fb), dim3(256), 0, st, d_sums, d_box, (int)nf, P.min_area, P.max_area, P.max_extent, d_cen, d_st);
  HIPCHK(hipGetLastError());
}

// Arguments are checked by the caller (sba_api.hip).  Device frames are read where they are, DOT_MAX_CHUNK frames per launch.
// Host frames go through two staging buffers of chunk_frames frames each, rows packed: the kernels of chunk k are queued
// before the copy of chunk k + 1 is issued on a second stream, so the two overlap whether or not the runtime makes the copy
// from pageable memory wait on the host.  Device memory: the two staging buffers and two sets of results, whatever n_frames is.
inline int dot_call(int device, const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels,
                    int64_t row_pitch, int64_t frame_pitch, const sba_dot_opts& o, uint64_t* sums, int32_t* box, double* centroid,
                    int32_t* status) {
  if (n_frames == 0) return SBA_OK;
  HIPCHK(hipSetDevice(device));
  DotParams P{};
  P.height = height; P.width = width; P.channel = o.channel; P.threshold = o.threshold;
  P.min_area = o.min_area; P.max_area = o.max_area; P.max_extent = o.max_extent;
  const int32_t* rr = o.roi_rect;
  if (rr[0] == 0 && rr[1] == 0 && rr[2] == 0 && rr[3] == 0) { P.x0 = 0; P.y0 = 0; P.x1 = width; P.y1 = height; }
  else {
    P.x0 = std::max(rr[0], 0); P.y0 = std::max(rr[1], 0); P.x1 = std::min(rr[2], width); P.y1 = std::min(rr[3], height);
  }
  P.ccx = o.roi_circle[0]; P.ccy = o.roi_circle[1];
  P.r2 = o.roi_circle[2] > 0 ? (int64_t)o.roi_circle[2] * o.roi_circle[2] : -1;

  const bool on_device = o.frames_on_device != 0;
  const int64_t row_bytes = (int64_t)width * channels, tight_frame = row_bytes * height;
  int64_t chunk = DOT_MAX_CHUNK;
  if (!on_device) {
    chunk = o.chunk_frames > 0 ? o.chunk_frames : std::max<int64_t>(1, DOT_STAGE_BYTES / std::max<int64_t>(1, tight_frame));
    chunk = std::min(chunk, DOT_MAX_CHUNK);
  }
  chunk = std::min(chunk, n_frames);
  const int nbuf = n_frames > chunk ? 2 : 1;

  DotStream s_run, s_copy;
  DotEvent ev_copied[2];
  DevBuf<uint8_t> d_stage[2];
  DevBuf<unsigned long long> d_sums[2];
  DevBuf<int> d_box[2], d_st[2];
  DevBuf<double> d_cen[2];
  for (int b = 0; b < nbuf; ++b) {
    if (!on_device) d_stage[b].alloc((size_t)std::max<int64_t>(16, chunk * tight_frame));
    d_sums[b].alloc((size_t)chunk * DOT_NSUM); d_box[b].alloc((size_t)chunk * 4); d_cen[b].alloc((size_t)chunk * 4); d_st[b].alloc((size_t)chunk);
  }
  auto stage = [&](int64_t lo, int b) {            // host frames [lo, lo + m) -> d_stage[b], rows packed
    const int64_t m = std::min(chunk, n_frames - lo);
    const uint8_t* src = frames + lo * frame_pitch;
    if (tight_frame == 0) { /* nothing to copy */ }
    else if (row_pitch == row_bytes && frame_pitch == tight_frame)
      HIPCHK(hipMemcpyAsync(d_stage[b].p, src, (size_t)(m * tight_frame), hipMemcpyHostToDevice, s_copy.s));
    else if (frame_pitch == row_pitch * height)
      HIPCHK(hipMemcpy2DAsync(d_stage[b].p, (size_t)row_bytes, src, (size_t)row_pitch, (size_t)row_bytes, (size_t)(m * height),
                              hipMemcpyHostToDevice, s_copy.s));
    else
      for (int64_t i = 0; i < m; ++i)
        HIPCHK(hipMemcpy2DAsync(d_stage[b].p + i * tight_frame, (size_t)row_bytes, src + i * frame_pitch, (size_t)row_pitch,
                                (size_t)row_bytes, (size_t)height, hipMemcpyHostToDevice, s_copy.s));
    HIPCHK(hipEventRecord(ev_copied[b].e, s_copy.s));
  };

  if (!on_device) stage(0, 0);
  int b = 0;
  for (int64_t lo = 0; lo < n_frames; lo += chunk, b ^= 1) {
    const int64_t m = std::min(chunk, n_frames - lo);
    if (on_device) { P.frames = frames + lo * frame_pitch; P.row_pitch = row_pitch; P.frame_pitch = frame_pitch; }
    else {
      P.frames = d_stage[b].p; P.row_pitch = row_bytes; P.frame_pitch = tight_frame;
      HIPCHK(hipStreamWaitEvent(s_run.s, ev_copied[b].e, 0));
    }
    dot_launch(P, channels, m, n_frames, d_sums[b].p, d_box[b].p, d_cen[b].p, d_st[b].p, s_run.s);
    if (!on_device && lo + chunk < n_frames) {     // the other buffer is free: its kernels and read-backs ended with the last pass
      stage(lo + chunk, b ^ 1);
    }
    if (sums) HIPCHK(hipMemcpyAsync(sums + lo * DOT_NSUM, d_sums[b].p, sizeof(uint64_t) * m * DOT_NSUM, hipMemcpyDeviceToHost, s_run.s));
    if (box) HIPCHK(hipMemcpyAsync(box + lo * 4, d_box[b].p, sizeof(int32_t) * m * 4, hipMemcpyDeviceToHost, s_run.s));
    if (centroid) HIPCHK(hipMemcpyAsync(centroid + lo * 4, d_cen[b].p, sizeof(double) * m * 4, hipMemcpyDeviceToHost, s_run.s));
    if (status) HIPCHK(hipMemcpyAsync(status + lo, d_st[b].p, sizeof(int32_t) * m, hipMemcpyDeviceToHost, s_run.s));
    HIPCHK(hipStreamSynchronize(s_run.s));         // the results of this chunk are on the host; its buffers may be reused
  }
  HIPCHK(hipStreamSynchronize(s_copy.s));
  return SBA_OK;
}

}  // namespace sba_detect
