// sba_hist.hpp -- sba_frame_histograms (include/sba_hip.h): the 256-bin histogram of one channel of every frame of a batch,
// inside the rectangle and the circle of the detectors, and the running total of a video.
//
// Two kernels per chunk of frames: k_hist (the streaming pass, one workgroup per band of rows of one frame, grid and rows as
// k_dot_moments) and k_hist_total (one workgroup: the chunk's histograms added to the call's 256 64-bit counters).  The
// chunk's `hist` is zeroed on the run stream in front of them.
//
// The frames are described, split into bands and staged as everywhere (sba_frames.hpp: FrameView, frame_row_span,
// frame_rows_per_band, frames_in_chunks).  scan_row is not used: it hands a vector on only when some lane holds a pixel above a
// threshold, and a histogram needs every pixel.  hist_row walks a row on the same plan -- the bytes in front of and behind the
// aligned body one per lane, the body as aligned 16-byte loads, DOT_UNROLL in flight, channel_words / channel_byte for the
// decode -- and hands every pixel to HistBins.
//
// EQUAL VALUES.  A wave has 256 32-bit bins of its own in LDS (4 waves: 4 KB).  The videos are dark frames with one spot: nearly
// every pixel of a wave falls into the same bin, and 64 lanes adding to one LDS address are served one after the other.  So a
// wave keeps ONE value, `dom`, in a register of every lane (the same in all of them) together with the lane's own count of it,
// `acc`; a pixel equal to dom costs a compare and an add and no LDS traffic, any other pixel is one LDS atomic.  dom is taken
// anew from the first pixel of the body of every row; when it changes, acc is first flushed into the bins.  The counts are
// exact whatever dom is: it only decides which pixels are counted in a register.  docs/EXPERIMENTS.md has the ladder this is the
// last step of, with the rates of each step.
//
// Every count is an unsigned integer: a lane's acc and a workgroup's bin hold at most the 32 x 16384 = 2^19 pixels of a band, a
// frame's bin at most 16384^2 = 2^28, a total 2^64.  Integer addition commutes, so the atomics give the same bits on every run.
#pragma once
#include "sba_frames.hpp"

namespace sba_detect {

constexpr int HIST_BINS = 256;

struct HistParams : FrameView {
  int32_t rows_per_band;
};

// The bins of one wave (`h`: HIST_BINS words of LDS) and its register count: value `dom`, the same in every lane, has been
// seen `acc` times by this lane since the last flush.
struct HistBins {
  uint32_t* h;
  uint32_t dom, acc;

  __device__ __forceinline__ void flush() {
    if (acc) atomicAdd(&h[dom], acc);
    acc = 0;
  }
  // cand: a value of the row that begins, of any one lane
  __device__ __forceinline__ void retarget(uint32_t cand) {
    cand = (uint32_t)__builtin_amdgcn_readfirstlane((int)cand);
    if (cand != dom) { flush(); dom = cand; }                            // wave-uniform
  }
  __device__ __forceinline__ void one(uint32_t v) {
    if (v == dom) ++acc; else atomicAdd(&h[v], 1u);
  }
  // the first n of the values b
  template <int NPIX>
  __device__ __forceinline__ void group(const uint32_t (&b)[NPIX], int n) {
    uint32_t same = 0;
#pragma unroll
    for (int k = 0; k < NPIX; ++k) same += (k < n && b[k] == dom) ? 1u : 0u;
    acc += same;
    if (same != (uint32_t)n) {
#pragma unroll
      for (int k = 0; k < NPIX; ++k)
        if (k < n && b[k] != dom) atomicAdd(&h[b[k]], 1u);
    }
  }
};

// The values of `channel` among the 16 bytes v that start at byte s of the row: b[0 .. n).  The channel's first byte is j0
// bytes into v, the others follow C apart; with C = 3 the sixth lies inside the 16 only when j0 = 0.
template <int C>
__device__ __forceinline__ int hist_decode(const uint4& v, uint32_t s, uint32_t channel, uint32_t (&b)[(16 + C - 1) / C]) {
  constexpr int NPIX = (16 + C - 1) / C;
  const uint32_t q = s / C, r = s - q * C;
  const uint32_t j0 = channel >= r ? channel - r : channel + C - r;
  uint32_t d[4];
  channel_words<C>(v, j0, d);
#pragma unroll
  for (int k = 0; k < NPIX; ++k) b[k] = channel_byte<C>(d, k);
  return (C == 3 && j0 != 0) ? NPIX - 1 : NPIX;
}

// One wave counts the pixels [xa, xb), xa < xb, of the row at rp: the bytes [xa C, xb C) up to the first 16-byte boundary of the
// ADDRESS and those behind the last one a byte per lane, the rest as aligned 16-byte loads, 64 lanes x DOT_UNROLL per step
// (scan_row's plan).  No byte outside [xa C, xb C) is read.
template <int C>
__device__ __forceinline__ void hist_row(const uint8_t* __restrict__ rp, int xa, int xb, uint32_t channel, HistBins& S) {
  constexpr int NPIX = (16 + C - 1) / C;
  const int lane = threadIdx.x & 63;
  const int bs = xa * C, be = xb * C;                                    // <= 16384 * 4
  const int head_end = min(be, bs + (int)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(rp + bs) & 15u)) & 15u));
  const int body_end = head_end + ((be - head_end) & ~15);
  {   // lanes 0..14: the bytes in front of the aligned body; lanes 32..46: those behind it
    const int b = lane < 32 ? bs + lane : body_end + (lane - 32);
    if (b < (lane < 32 ? head_end : be)) {
      const uint32_t q = (uint32_t)b / C;
      if ((uint32_t)b - q * C == channel) S.one(rp[b]);
    }
  }
  for (int s0 = head_end + lane * 16; s0 < body_end + lane * 16; s0 += 64 * 16 * DOT_UNROLL) {   // the bound is wave-uniform
    uint4 v[DOT_UNROLL];
#pragma unroll
    for (int u = 0; u < DOT_UNROLL; ++u) {
      const int s = s0 + u * 64 * 16;
      v[u] = s < body_end ? *reinterpret_cast<const uint4*>(rp + s) : make_uint4(0u, 0u, 0u, 0u);
    }
    uint32_t b[NPIX];
    if (s0 - lane * 16 == head_end) {                                    // the row's first step: lane 0 holds its first pixels
      hist_decode<C>(v[0], (uint32_t)s0, channel, b);
      S.retarget(b[0]);
    }
#pragma unroll
    for (int u = 0; u < DOT_UNROLL; ++u) {
      const int s = s0 + u * 64 * 16;
      const int n = hist_decode<C>(v[u], (uint32_t)s, channel, b);
      if (s < body_end) S.group(b, n);
    }
  }
}

// grid (bands, frames), DOT_THREADS threads.  Wave w of the workgroup takes rows y0 + band * rows_per_band + w, + w + 4, ...
// into its own bins; after one barrier thread t adds the waves' bins t and, when the sum is not zero, issues ONE atomic to
// hist[f][t]: a dark band issues a handful of them.
template <int C>
__global__ void __launch_bounds__(DOT_THREADS) k_hist(const HistParams P, uint32_t* __restrict__ hist) {
  static_assert(DOT_THREADS == HIST_BINS, "a thread per bin");
  __shared__ uint32_t s_h[DOT_WAVES][HIST_BINS];
  const int wave = threadIdx.x >> 6, t = threadIdx.x;
  const int f = blockIdx.y;
  const uint32_t channel = (uint32_t)P.channel;
  const int band_lo = P.y0 + (int)blockIdx.x * P.rows_per_band;
  const int band_hi = min(P.y1, band_lo + P.rows_per_band);
  const uint8_t* __restrict__ fp = P.frames + (int64_t)f * P.frame_pitch;
#pragma unroll
  for (int w = 0; w < DOT_WAVES; ++w) s_h[w][t] = 0;
  __syncthreads();

  HistBins S{s_h[wave], 0u, 0u};
  for (int y = band_lo + wave; y < band_hi; y += DOT_WAVES) {
    int xa, xb;
    __builtin_assume(y >= P.y0);                                         // as in k_dot_moments
    if (!frame_row_span(P, y, xa, xb)) continue;
    hist_row<C>(fp + (int64_t)y * P.row_pitch, xa, xb, channel, S);
  }
  S.flush();
  __syncthreads();
  uint32_t tot = 0;
#pragma unroll
  for (int w = 0; w < DOT_WAVES; ++w) tot += s_h[w][t];
  if (tot) atomicAdd(&hist[(size_t)f * HIST_BINS + t], tot);
}

// one workgroup of HIST_BINS threads: total[t] += the sum over the chunk's frames of hist[f][t]
__global__ void __launch_bounds__(HIST_BINS) k_hist_total(const uint32_t* __restrict__ hist, int n_frames, unsigned long long* __restrict__ total) {
  const int t = threadIdx.x;
  unsigned long long s = 0;
  for (int f = 0; f < n_frames; ++f) s += hist[(size_t)f * HIST_BINS + t];
  total[t] += s;
}

// ------------------------------------------------------------------------------------------------ host side
// Arguments are checked by the caller (sba_api.hip).  Chunks as dot_call: device frames DOT_MAX_CHUNK per launch, host frames
// chunk_frames per staging copy.  Device memory besides the staging buffers: one chunk's histograms and the 256 counters.
int hist_call(const FrameBatch& B, const sba_hist_opts& o, uint32_t* hist, uint64_t* total) {
  const int64_t n_frames = B.n_frames;
  const int32_t channels = B.channels;
  if (n_frames == 0 || (!hist && !total)) return SBA_OK;
  HIPCHK(hipSetDevice(B.device));
  HistParams P{};
  static_cast<FrameView&>(P) = frame_view(B, o.channel, 0, o.roi_rect, o.roi_circle);

  const bool on_device = o.frames_on_device != 0;
  const int64_t chunk = chunk_of(CHUNK_RECORDS, o.chunk_frames, B, on_device);

  DevBuf<uint32_t> d_hist;
  DevBuf<unsigned long long> d_total;
  d_hist.alloc((size_t)chunk * HIST_BINS);
  if (total) d_total.alloc(HIST_BINS);
  frames_in_chunks(
      P, channels, n_frames, on_device, chunk,
      [&](const FrameView& V, int64_t lo, int64_t m, hipStream_t st) {
        static_cast<FrameView&>(P) = V;
        if (total && lo == 0) HIPCHK(hipMemsetAsync(d_total.p, 0, sizeof(unsigned long long) * HIST_BINS, st));
        HIPCHK(hipMemsetAsync(d_hist.p, 0, sizeof(uint32_t) * m * HIST_BINS, st));
        const int64_t rows = (int64_t)P.y1 - P.y0;
        if (rows > 0 && P.x1 > P.x0) {
          const int rpb = P.rows_per_band = frame_rows_per_band(rows, n_frames);
          const dim3 grid((unsigned)((rows + rpb - 1) / rpb), (unsigned)m);
          if (channels == 1) hipLaunchKernelGGL(k_hist<1>, grid, dim3(DOT_THREADS), 0, st, P, d_hist.p);
          else if (channels == 3) hipLaunchKernelGGL(k_hist<3>, grid, dim3(DOT_THREADS), 0, st, P, d_hist.p);
          else hipLaunchKernelGGL(k_hist<4>, grid, dim3(DOT_THREADS), 0, st, P, d_hist.p);
          HIPCHK(hipGetLastError());
          if (total) {
            hipLaunchKernelGGL(k_hist_total, dim3(1), dim3(HIST_BINS), 0, st, d_hist.p, (int)m, d_total.p);
            HIPCHK(hipGetLastError());
          }
        }
      },
      [&](int64_t lo, int64_t m, hipStream_t st) {
        if (hist) HIPCHK(hipMemcpyAsync(hist + lo * HIST_BINS, d_hist.p, sizeof(uint32_t) * m * HIST_BINS, hipMemcpyDeviceToHost, st));
      });
  if (total) {
    unsigned long long sum[HIST_BINS];
    HIPCHK(hipMemcpy(sum, d_total.p, sizeof sum, hipMemcpyDeviceToHost));
    for (int v = 0; v < HIST_BINS; ++v) total[v] += sum[v];
  }
  return SBA_OK;
}

}  // namespace sba_detect
