// sba_frames.hpp -- how the laser-dot detectors (sba_detect.hpp: moments; sba_blobs.hpp: connected components) read a batch
// of 8-bit frames with interleaved channels: any base address, any pitches, from the host or the device, with a rectangle and a
// circle of interest.  Everything between "such a batch" and "the bytes of row y that count" is here, once: the description a
// kernel gets (FrameView), the pixels of a row inside both regions (frame_row_span), one wave's walk over them (scan_row), the
// rows of a workgroup (frame_rows_per_band) and the host's loop over chunks of frames with its staging (frames_in_chunks).
// What is done with a pixel once it is found is the consumer's sink (DotSink, BlobSink).
#pragma once
#include "sba_common.hpp"

namespace sba_detect {
using namespace sba_host;

constexpr int DOT_THREADS = 256, DOT_WAVES = DOT_THREADS / 64;            // of the kernels that scan rows: a wave per row
constexpr int DOT_MAX_DIM = 16384;
constexpr int DOT_UNROLL = 4;                // 16-byte loads a lane has in flight
constexpr int64_t DOT_STAGE_BYTES = (int64_t)64 << 20;     // default size of one staging buffer for host frames
constexpr int64_t DOT_MAX_CHUNK = 16384;     // frames per launch (grid.y)

struct FrameView {
  const uint8_t* frames;
  int64_t row_pitch, frame_pitch;
  int32_t height, width, channel, threshold;
  int32_t x0, y0, x1, y1;                    // the rectangle, clipped to the frame, half-open
  int32_t ccx, ccy;
  int64_t r2;                                // the circle's r^2; < 0 = no circle
};

// roi_rect = (x0, y0, x1, y1), all zero = the whole frame; roi_circle = (cx, cy, r), r <= 0 = no circle
inline FrameView frame_view(const uint8_t* frames, int64_t row_pitch, int64_t frame_pitch, int32_t height, int32_t width, int32_t channel,
                            int32_t threshold, const int32_t* rr, const int32_t* rc) {
  FrameView V{};
  V.frames = frames; V.row_pitch = row_pitch; V.frame_pitch = frame_pitch;
  V.height = height; V.width = width; V.channel = channel; V.threshold = threshold;
  if (rr[0] == 0 && rr[1] == 0 && rr[2] == 0 && rr[3] == 0) { V.x0 = 0; V.y0 = 0; V.x1 = width; V.y1 = height; }
  else { V.x0 = std::max(rr[0], 0); V.y0 = std::max(rr[1], 0); V.x1 = std::min(rr[2], width); V.y1 = std::min(rr[3], height); }
  V.ccx = rc[0]; V.ccy = rc[1];
  V.r2 = rc[2] > 0 ? (int64_t)rc[2] * rc[2] : -1;
  return V;
}

// about 2048 workgroups over the whole call where the frames allow it, 4 to 32 rows each (one to eight per wave)
inline int frame_rows_per_band(int64_t rows, int64_t total_frames) {
  const int64_t rpb = rows * total_frames / 2048;
  return (int)std::max<int64_t>(DOT_WAVES, std::min<int64_t>(32, rpb / DOT_WAVES * DOT_WAVES));
}

// floor(sqrt(v)) for 0 <= v <= 2^62
__device__ __forceinline__ long long dot_isqrt(long long v) {
  long long d = (long long)sqrt((double)v);
  while (d * d > v) --d;
  while ((d + 1) * (d + 1) <= v) ++d;
  return d;
}

// The pixels [xa, xb) of row y inside the rectangle and the circle (cx +- floor(sqrt(r^2 - (y - cy)^2))); false = none
__device__ __forceinline__ bool frame_row_span(const FrameView& V, int y, int& xa, int& xb) {
  if (y < V.y0 || y >= V.y1) return false;
  xa = V.x0; xb = V.x1;
  if (V.r2 >= 0) {
    const long long dy = (long long)y - V.ccy, rem = V.r2 - dy * dy;
    if (rem < 0) return false;
    const long long dx = dot_isqrt(rem);
    xa = (int)max((long long)xa, (long long)V.ccx - dx);
    xb = (int)min((long long)xb, (long long)V.ccx + dx + 1);
  }
  return xa < xb;
}

// The 16 bytes `v` start at byte s of the row.  Hands the values of the pixels whose thresholded channel lies in them to the
// sink; returns false, having done nothing else, when no lane of the wave has one above the threshold (the usual case: frames
// are dark but for the dot).  A byte shifted in from beyond the 16 is zero and never above a threshold >= 0.
template <int C, class Sink>
__device__ __forceinline__ bool scan_vector(const uint4& v, uint32_t s, uint32_t channel, uint32_t thr, Sink& sink) {
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
  uint32_t b[NPIX], any = 0;
#pragma unroll
  for (int k = 0; k < NPIX; ++k) {                                       // byte k C of the 16: a constant after unrolling
    b[k] = (d[(k * C) >> 2] >> (8 * ((k * C) & 3))) & 0xffu;
    any |= b[k] > thr ? 1u : 0u;
  }
  if (!__any(any != 0)) return false;
  sink(xq, b);
  return true;
}

// One wave reads the pixels [xa, xb), xa < xb, of the row at rp: the bytes [xa C, xb C) up to the first 16-byte boundary of the
// ADDRESS and those behind the last one a byte per lane, the rest as aligned 16-byte loads, 64 lanes x DOT_UNROLL per step.
// sink(x, value[N]) gets the values of the thresholded channel of the pixels x, x + 1, ..., x + N - 1: a single one (N = 1)
// that is above the threshold, or the pixels of a 16-byte vector, of which at least one lane of the wave has one above it
// (this lane may have none).  Returns whether any lane saw a pixel above the threshold; the same in every lane.
template <int C, class Sink>
__device__ __forceinline__ bool scan_row(const uint8_t* __restrict__ rp, int xa, int xb, uint32_t channel, uint32_t thr, Sink& sink) {
  const int lane = threadIdx.x & 63;
  const int bs = xa * C, be = xb * C;                                    // <= 16384 * 4
  const int head_end = min(be, bs + (int)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(rp + bs) & 15u)) & 15u));
  const int body_end = head_end + ((be - head_end) & ~15);
  bool on = false;
  {   // lanes 0..14: the bytes in front of the aligned body; lanes 32..46: those behind it
    const int b = lane < 32 ? bs + lane : body_end + (lane - 32);
    if (b < (lane < 32 ? head_end : be)) {
      const uint32_t q = (uint32_t)b / C;
      if ((uint32_t)b - q * C == channel) {
        const uint32_t v1[1] = {rp[b]};
        on = v1[0] > thr;
        if (on) sink(q, v1);
      }
    }
  }
  bool hit = __any(on);
  for (int s0 = head_end + lane * 16; s0 < body_end + lane * 16; s0 += 64 * 16 * DOT_UNROLL) {   // the bound is wave-uniform
    uint4 v[DOT_UNROLL];
#pragma unroll
    for (int u = 0; u < DOT_UNROLL; ++u) {
      const int s = s0 + u * 64 * 16;
      v[u] = s < body_end ? *reinterpret_cast<const uint4*>(rp + s) : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int u = 0; u < DOT_UNROLL; ++u) hit |= scan_vector<C>(v[u], (uint32_t)(s0 + u * 64 * 16), channel, thr, sink);
  }
  return hit;
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

// Takes the n_frames > 0 frames of V in chunks of `chunk` frames (1 <= chunk <= DOT_MAX_CHUNK, the caller's choice).  V is
// a copy, so a caller may write a chunk's view over its own.  Of the chunk [lo, lo + m) it calls
//   launch(view, lo, m, stream)   queues the kernels; view.frames points at the chunk's first frame
//   fetch(lo, m, stream)          queues the copies of the results to the host
//   done(lo, m)                   after the stream has been drained: the results are on the host
// in that order, so one set of result buffers serves every chunk.  Device frames are read where they are.  Host frames go
// through two staging buffers of `chunk` frames each, rows packed, filled on a second stream.
// THE ORDER: the copy of chunk k + 1 is issued after the kernels of chunk k are queued and before anything that can make the
// host wait for them (a read-back into pageable memory may, the drain does), so the two overlap whether or not the runtime
// makes a copy from pageable memory wait on the host; the kernels of chunk k + 1 wait on that copy's event.  The buffer the
// copy writes is free: its kernels were drained with chunk k - 1.  Device memory: the two staging buffers, whatever n_frames is.
template <class Launch, class Fetch, class Done>
inline void frames_in_chunks(const FrameView V, int32_t channels, int64_t n_frames, bool on_device, int64_t chunk, Launch&& launch,
                             Fetch&& fetch, Done&& done) {
  const int64_t row_bytes = (int64_t)V.width * channels, tight_frame = row_bytes * V.height;
  DotStream s_run, s_copy;
  DotEvent ev_copied[2];
  DevBuf<uint8_t> d_stage[2];
  if (!on_device)
    for (int b = 0; b < (n_frames > chunk ? 2 : 1); ++b) d_stage[b].alloc((size_t)std::max<int64_t>(16, chunk * tight_frame));
  auto stage = [&](int64_t lo, int b) {            // host frames [lo, lo + m) -> d_stage[b], rows packed
    const int64_t m = std::min(chunk, n_frames - lo);
    const uint8_t* src = V.frames + lo * V.frame_pitch;
    if (tight_frame == 0) { /* nothing to copy */ }
    else if (V.row_pitch == row_bytes && V.frame_pitch == tight_frame)
      HIPCHK(hipMemcpyAsync(d_stage[b].p, src, (size_t)(m * tight_frame), hipMemcpyHostToDevice, s_copy.s));
    else if (V.frame_pitch == V.row_pitch * V.height)
      HIPCHK(hipMemcpy2DAsync(d_stage[b].p, (size_t)row_bytes, src, (size_t)V.row_pitch, (size_t)row_bytes, (size_t)(m * V.height),
                              hipMemcpyHostToDevice, s_copy.s));
    else
      for (int64_t i = 0; i < m; ++i)
        HIPCHK(hipMemcpy2DAsync(d_stage[b].p + i * tight_frame, (size_t)row_bytes, src + i * V.frame_pitch, (size_t)V.row_pitch,
                                (size_t)row_bytes, (size_t)V.height, hipMemcpyHostToDevice, s_copy.s));
    HIPCHK(hipEventRecord(ev_copied[b].e, s_copy.s));
  };

  if (!on_device) stage(0, 0);
  int b = 0;
  for (int64_t lo = 0; lo < n_frames; lo += chunk, b ^= 1) {
    const int64_t m = std::min(chunk, n_frames - lo);
    FrameView Vc = V;
    if (on_device) Vc.frames = V.frames + lo * V.frame_pitch;
    else {
      Vc.frames = d_stage[b].p; Vc.row_pitch = row_bytes; Vc.frame_pitch = tight_frame;
      HIPCHK(hipStreamWaitEvent(s_run.s, ev_copied[b].e, 0));
    }
    launch(Vc, lo, m, s_run.s);
    if (!on_device && lo + chunk < n_frames) stage(lo + chunk, b ^ 1);
    fetch(lo, m, s_run.s);
    HIPCHK(hipStreamSynchronize(s_run.s));
    done(lo, m);
  }
  HIPCHK(hipStreamSynchronize(s_copy.s));
}

}  // namespace sba_detect
