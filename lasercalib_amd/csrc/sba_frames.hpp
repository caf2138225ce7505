// sba_frames.hpp -- what the frame functions share.  How the laser-dot detectors (sba_detect.hpp: moments; sba_blobs.hpp:
// connected components) read a batch of 8-bit frames with interleaved channels -- any base address, any pitches, from the host
// or the device, with a rectangle and a circle of interest -- is here, once: the description a kernel gets (FrameView), the
// pixels of a row inside both regions (frame_row_span), one wave's walk over them (scan_row), the rows of a workgroup
// (frame_rows_per_band); what is done with a pixel once it is found is the consumer's sink (DotSink, BlobSink).  So are the
// device helpers that more than one kernel uses (wave_lds_sync, channel_words / channel_byte) and ALL host-side plumbing of
// every frame function (the "host side" below): chunk size, pitched copies, the loop over chunks with its staging, the output,
// and a set of YUV 4:2:0 planes as the source or the output of a call (chroma_mode, YuvSource, YuvOutput).
// A frame call arrives here as ABI scalars -> FrameBatch -> checks (sba_api.hip) -> *_call (a feature header).  FrameBatch and
// FrameOut (sba_frame_calls.hpp) are host-only; what a *_call derives from them is here: frame_view(B, ...), frame_plane(B),
// frame_bytes(B), chunk_of(policy, ...), FrameOutput(FrameOut, ...).  Nothing of them reaches a kernel.
// (The store of a finished LDS row at any alignment stays written out in k_undistort and k_resize: as a shared function it
// compiled to other instructions in both.)
#pragma once
#include <optional>
#include "sba_common.hpp"
#include "sba_frame_calls.hpp"

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

// roi_rect = (x0, y0, x1, y1), all zero or none = the whole frame; roi_circle = (cx, cy, r), r <= 0 or none = no circle
inline FrameView frame_view(const uint8_t* frames, int64_t row_pitch, int64_t frame_pitch, int32_t height, int32_t width, int32_t channel,
                            int32_t threshold, const int32_t* rr = nullptr, const int32_t* rc = nullptr) {
  static const int32_t whole[4] = {0, 0, 0, 0};
  if (!rr) rr = whole;
  if (!rc) rc = whole;
  FrameView V{};
  V.frames = frames; V.row_pitch = row_pitch; V.frame_pitch = frame_pitch;
  V.height = height; V.width = width; V.channel = channel; V.threshold = threshold;
  if (rr[0] == 0 && rr[1] == 0 && rr[2] == 0 && rr[3] == 0) { V.x0 = 0; V.y0 = 0; V.x1 = width; V.y1 = height; }
  else { V.x0 = std::max(rr[0], 0); V.y0 = std::max(rr[1], 0); V.x1 = std::min(rr[2], width); V.y1 = std::min(rr[3], height); }
  V.ccx = rc[0]; V.ccy = rc[1];
  V.r2 = rc[2] > 0 ? (int64_t)rc[2] * rc[2] : -1;
  return V;
}

// What every call derives from its batch: the view its kernels read, the one plane frames_in_chunks stages, the packed bytes of
// a frame
inline FrameView frame_view(const FrameBatch& B, int32_t channel, int32_t threshold, const int32_t* rr = nullptr, const int32_t* rc = nullptr) {
  return frame_view(B.frames, B.row_pitch, B.frame_pitch, B.height, B.width, channel, threshold, rr, rc);
}
inline int64_t frame_bytes(const FrameBatch& B) { return (int64_t)B.width * B.channels * B.height; }

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

// LDS traffic between the lanes of ONE wave: the wave's DS operations complete in issue order; the fences keep the compiler
// from moving accesses across
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The channel bytes of a 16-byte group v of pixels with C channels, in two steps.  channel_words: the group shifted so that the
// channel's first byte, j0 (0..3) bytes into v, is byte 0; a byte shifted in from beyond the 16 is 0.  channel_byte: value k of
// the channel, byte k C of those words -- a constant shift once k is one.
template <int C>
__device__ __forceinline__ void channel_words(const uint4& v, uint32_t j0, uint32_t (&d)[4]) {
  if (C == 1) { d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w; }
  else {
    d[0] = __builtin_amdgcn_alignbyte(v.y, v.x, j0);
    d[1] = __builtin_amdgcn_alignbyte(v.z, v.y, j0);
    d[2] = __builtin_amdgcn_alignbyte(v.w, v.z, j0);
    d[3] = __builtin_amdgcn_alignbyte(0u, v.w, j0);
  }
}
template <int C>
__device__ __forceinline__ uint32_t channel_byte(const uint32_t (&d)[4], int k) { return (d[(k * C) >> 2] >> (8 * ((k * C) & 3))) & 0xffu; }

// The 16 bytes `v` start at byte s of the row.  Hands the values of the pixels whose thresholded channel lies in them to the
// sink; returns false, having done nothing else, when no lane of the wave has one above the threshold (the usual case: frames
// are dark but for the dot).  A byte from beyond the 16 is zero and never above a threshold >= 0.
template <int C, class Sink>
__device__ __forceinline__ bool scan_vector(const uint4& v, uint32_t s, uint32_t channel, uint32_t thr, Sink& sink) {
  constexpr int NPIX = (16 + C - 1) / C;
  const uint32_t q = s / C, r = s - q * C;
  const uint32_t j0 = channel >= r ? channel - r : channel + C - r;      // first byte of the channel at or after s
  const uint32_t xq = q + (channel < r ? 1u : 0u);
  uint32_t d[4];
  channel_words<C>(v, j0, d);
  uint32_t b[NPIX], any = 0;
#pragma unroll
  for (int k = 0; k < NPIX; ++k) {
    b[k] = channel_byte<C>(d, k);
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
// Everything between a caller's pointers and pitches and the kernels of a chunk: the size of a chunk (frames_per_chunk, and
// chunk_of, which names the two policies the calls have for it), the one routine that moves pitched frames (copy_frames), the
// loop over chunks with its staging (frames_in_chunks), the output of a call that writes frames (FrameOutput), and what the YUV 4:2:0 calls build from these: how two chroma planes are treated
// (chroma_mode), their planes as a staged source (YuvSource) and as an output (YuvOutput).
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

// The frames of a chunk: `requested` (an entry point's chunk_frames) when > 0, else as many as fit DOT_STAGE_BYTES at
// `staged_bytes` a frame -- the larger of what a frame takes in a staging buffer and in the packed buffer of a host output;
// 0 = neither exists (or the frame has no bytes), and only the launch limits the chunk.  At most DOT_MAX_CHUNK and n_frames,
// at least 1.
inline int64_t frames_per_chunk(int64_t requested, int64_t n_frames, int64_t staged_bytes) {
  int64_t chunk = DOT_MAX_CHUNK;
  if (requested > 0) chunk = requested;
  else if (staged_bytes > 0) chunk = std::max<int64_t>(1, DOT_STAGE_BYTES / staged_bytes);
  return std::max<int64_t>(1, std::min(std::min(chunk, DOT_MAX_CHUNK), n_frames));
}

// The chunk of a call.  The frame functions have two policies, and both are here:
//   CHUNK_RECORDS  calls whose results are small records per frame (dots, histograms, corners): chunk_frames is the size of a
//                  staging copy, so frames on the device ignore it and go DOT_MAX_CHUNK a launch;
//   CHUNK_FRAMES   calls that write frames, and the background statistics: chunk_frames is honoured wherever the frames are; by
//                  default a chunk is sized by the larger of the two sides (in_bytes, out_bytes: packed bytes of a frame; 0 = the
//                  call has no such side) as soon as ONE of them is host memory, whichever it is.
// sba_detect_blobs (chunk_frames caps the library's own choice) and sba_adaptive_threshold (each side counts only when it is host
// memory) follow neither and say so where they compute theirs.
enum ChunkPolicy { CHUNK_RECORDS, CHUNK_FRAMES };
inline int64_t chunk_of(ChunkPolicy policy, int64_t requested, int64_t n_frames, int64_t in_bytes, bool in_dev, int64_t out_bytes = 0,
                        bool out_dev = true) {
  if (policy == CHUNK_RECORDS) return frames_per_chunk(in_dev ? 0 : requested, n_frames, in_dev ? 0 : in_bytes);
  return frames_per_chunk(requested, n_frames, in_dev && out_dev ? 0 : std::max(in_bytes, out_bytes));
}
inline int64_t chunk_of(ChunkPolicy policy, int64_t requested, const FrameBatch& B, bool in_dev, int64_t out_bytes = 0, bool out_dev = true) {
  return chunk_of(policy, requested, B.n_frames, frame_bytes(B), in_dev, out_bytes, out_dev);
}

// m frames of `rows` rows of `row_bytes` bytes from one pitched layout to another, in either direction, queued on st.  Four
// classes of layout: both sides packed (one copy); packed rows with frames apart, such as a plane of a stacked frame or frames
// with a gap (one plain copy per frame -- not a 2-D copy of `rows` rows: the bytes are the same); padded rows with frames of
// rows x row pitch (one 2-D copy of m x rows rows); anything else (one 2-D copy per frame).
inline void copy_frames(uint8_t* dst, int64_t d_row, int64_t d_frame, const uint8_t* src, int64_t s_row, int64_t s_frame, int64_t row_bytes,
                        int64_t rows, int64_t m, hipMemcpyKind kind, hipStream_t st) {
  if (row_bytes == 0 || rows == 0) return;
  const int64_t tight = row_bytes * rows;
  if (d_row == row_bytes && s_row == row_bytes && d_frame == tight && s_frame == tight)
    HIPCHK(hipMemcpyAsync(dst, src, (size_t)(m * tight), kind, st));
  else if (d_row == row_bytes && s_row == row_bytes)
    for (int64_t i = 0; i < m; ++i) HIPCHK(hipMemcpyAsync(dst + i * d_frame, src + i * s_frame, (size_t)tight, kind, st));
  else if (d_frame == d_row * rows && s_frame == s_row * rows)
    HIPCHK(hipMemcpy2DAsync(dst, (size_t)d_row, src, (size_t)s_row, (size_t)row_bytes, (size_t)(m * rows), kind, st));
  else
    for (int64_t i = 0; i < m; ++i)
      HIPCHK(hipMemcpy2DAsync(dst + i * d_frame, (size_t)d_row, src + i * s_frame, (size_t)s_row, (size_t)row_bytes, (size_t)rows, kind, st));
}

// One plane of a batch of frames: frame f, row r at base + f frame_pitch + r row_pitch, row_bytes bytes of it count
struct FramePlane {
  const uint8_t* base;
  int64_t row_pitch, frame_pitch, row_bytes, rows;
};
inline FramePlane frame_plane(const FrameBatch& B) { return {B.frames, B.row_pitch, B.frame_pitch, (int64_t)B.width * B.channels, B.height}; }
constexpr int FRAME_MAX_PLANES = 3;
struct FrameNoDone { void operator()(int64_t, int64_t) const {} };

// Takes the n_frames > 0 frames of 1 <= n_planes <= FRAME_MAX_PLANES planes in chunks of `chunk` frames (1 <= chunk <=
// DOT_MAX_CHUNK: frames_per_chunk).  Of the chunk [lo, lo + m) it calls
//   launch(planes, lo, m, stream) queues the kernels; planes[p].base points at the chunk's first frame, with its pitches
//   fetch(lo, m, stream)          queues the copies of the results to the host
//   done(lo, m)                   after the stream has been drained: the results are on the host (optional)
// in that order, so one set of result buffers serves every chunk.  Device frames are read where they are.  Host frames go
// through two staging buffers of `chunk` frames each, filled on a second stream (one buffer when one chunk is all there is):
// the frames of plane 0, rows packed, then those of plane 1, ...
// THE ORDER: the copy of chunk k + 1 is issued after the kernels of chunk k are queued and before anything that can make the
// host wait for them (a read-back into pageable memory may, the drain does), so the two overlap whether or not the runtime
// makes a copy from pageable memory wait on the host; the kernels of chunk k + 1 wait on that copy's event.  The buffer the
// copy writes is free: its kernels were drained with chunk k - 1.  Device memory: the two staging buffers, whatever n_frames is.
template <class Launch, class Fetch, class Done = FrameNoDone>
inline void frames_in_chunks(const FramePlane* planes, int n_planes, int64_t n_frames, bool on_device, int64_t chunk, Launch&& launch,
                             Fetch&& fetch, Done&& done = Done()) {
  int64_t tight[FRAME_MAX_PLANES], tight_frame = 0;
  for (int p = 0; p < n_planes; ++p) tight_frame += tight[p] = planes[p].row_bytes * planes[p].rows;
  DotStream s_run, s_copy;
  DotEvent ev_copied[2];
  DevBuf<uint8_t> d_stage[2];
  if (!on_device)
    for (int b = 0; b < (n_frames > chunk ? 2 : 1); ++b) d_stage[b].alloc((size_t)std::max<int64_t>(16, chunk * tight_frame));
  auto stage = [&](int64_t lo, int b) {            // host frames [lo, lo + m) -> d_stage[b]
    const int64_t m = std::min(chunk, n_frames - lo);
    uint8_t* d = d_stage[b].p;
    for (int p = 0; p < n_planes; d += chunk * tight[p], ++p)
      copy_frames(d, planes[p].row_bytes, tight[p], planes[p].base + lo * planes[p].frame_pitch, planes[p].row_pitch,
                  planes[p].frame_pitch, planes[p].row_bytes, planes[p].rows, m, hipMemcpyHostToDevice, s_copy.s);
    HIPCHK(hipEventRecord(ev_copied[b].e, s_copy.s));
  };

  if (!on_device) stage(0, 0);
  int b = 0;
  for (int64_t lo = 0; lo < n_frames; lo += chunk, b ^= 1) {
    const int64_t m = std::min(chunk, n_frames - lo);
    FramePlane c[FRAME_MAX_PLANES];
    uint8_t* d = d_stage[b].p;
    for (int p = 0; p < n_planes; d += chunk * tight[p], ++p) {
      c[p] = planes[p];
      if (on_device) c[p].base += lo * c[p].frame_pitch;
      else { c[p].base = d; c[p].row_pitch = c[p].row_bytes; c[p].frame_pitch = tight[p]; }
    }
    if (!on_device) HIPCHK(hipStreamWaitEvent(s_run.s, ev_copied[b].e, 0));
    launch(c, lo, m, s_run.s);
    if (!on_device && lo + chunk < n_frames) stage(lo + chunk, b ^ 1);
    fetch(lo, m, s_run.s);
    HIPCHK(hipStreamSynchronize(s_run.s));
    done(lo, m);
  }
  HIPCHK(hipStreamSynchronize(s_copy.s));
}

// The same for frames with interleaved channels, one plane: launch(view, lo, m, stream) gets V with the chunk's first frame
// and its pitches.  V is a copy, so a caller may write a chunk's view over its own.
template <class Launch, class Fetch, class Done = FrameNoDone>
inline void frames_in_chunks(const FrameView V, int32_t channels, int64_t n_frames, bool on_device, int64_t chunk, Launch&& launch,
                             Fetch&& fetch, Done&& done = Done()) {
  const FramePlane plane{V.frames, V.row_pitch, V.frame_pitch, (int64_t)V.width * channels, V.height};
  frames_in_chunks(
      &plane, 1, n_frames, on_device, chunk,
      [&](const FramePlane* c, int64_t lo, int64_t m, hipStream_t st) {
        FrameView Vc = V;
        Vc.frames = c->base; Vc.row_pitch = c->row_pitch; Vc.frame_pitch = c->frame_pitch;
        launch(Vc, lo, m, st);
      },
      fetch, done);
}

// Where a call that turns frames into frames writes them: n frames of `rows` rows of `row_bytes` bytes.  An output on the
// device is written where it is, at the caller's pitches.  One on the host goes through ONE packed device buffer of a chunk,
// owned here: the kernels of a chunk write it, and it is fetched into the caller's pitches on the run stream before the chunk
// is drained (frames_in_chunks has queued the copy of the next chunk's frames by then, so the two copies run side by side).
struct FrameOutput {
  uint8_t* out;
  int64_t row_pitch, frame_pitch, row_bytes, rows;
  bool on_device;
  DevBuf<uint8_t> d_packed;
  FrameOutput(const FrameOut& o, int64_t row_bytes_, int64_t rows_, bool on_device_, int64_t chunk)
      : out(o.out), row_pitch(o.row_pitch), frame_pitch(o.frame_pitch), row_bytes(row_bytes_), rows(rows_), on_device(on_device_) {
    if (!on_device) d_packed.alloc((size_t)(chunk * row_bytes * rows));
  }
  // what the kernels of the chunk that starts at frame lo write: its first frame and the two pitches
  void target(int64_t lo, uint8_t*& p, int64_t& row, int64_t& frame) const {
    if (on_device) { p = out + lo * frame_pitch; row = row_pitch; frame = frame_pitch; }
    else { p = d_packed.p; row = row_bytes; frame = row_bytes * rows; }
  }
  // frames_in_chunks' fetch
  void fetch(int64_t lo, int64_t m, hipStream_t st) const {
    if (!on_device)
      copy_frames(out + lo * frame_pitch, row_pitch, frame_pitch, d_packed.p, row_bytes, row_bytes * rows, row_bytes, rows, m, hipMemcpyDeviceToHost, st);
  }
};

// ---- a set of 8-bit YUV 4:2:0 planes (sba_yuv_planes), read (YuvSource) or written (YuvOutput)
enum { CV_PLANAR = 0, CV_UV = 1, CV_VU = 2, CV_STEP2 = 3 };  // how a kernel reads or writes the chroma of a block

// The mode of two chroma planes of cw samples a row: two planes one byte apart are taken as ONE plane of pairs only when its
// rows hold all their 2 cw bytes without overlapping the next row
inline int chroma_mode(const uint8_t* u, const uint8_t* v, int64_t c_row_pitch, int32_t c_step, int64_t cw) {
  return c_step == 1 ? CV_PLANAR : c_row_pitch < 2 * cw ? CV_STEP2 : v == u + 1 ? CV_UV : u == v + 1 ? CV_VU : CV_STEP2;
}

// Planes that frames_in_chunks reads: the luma plane, then the chroma -- ONE plane of 2 ceil(width / 2) bytes a row when u and
// v are the halves of an interleaved plane (NV12, NV21), else two planes of c_step (ceil(width / 2) - 1) + 1 bytes a row.  A
// source without pixels (height or width 0) has planes without bytes: nothing of it is staged or read.
struct YuvSource {
  int mode, n_planes;                        // n_planes: luma, the kernel's u, and v when it is a plane of its own
  FramePlane planes[3];
  int64_t tight;                             // packed bytes of a frame
  YuvSource(const sba_yuv_planes& S, int32_t height, int32_t width) {
    const bool empty = height == 0 || width == 0;
    const int64_t cw = (width + 1) / 2, rows = empty ? 0 : height, c_rows = empty ? 0 : (height + 1) / 2;
    mode = chroma_mode(S.u, S.v, S.c_row_pitch, S.c_step, cw);
    const bool paired = mode == CV_UV || mode == CV_VU;
    n_planes = paired ? 2 : 3;
    const int64_t c_row = empty ? 0 : paired ? 2 * cw : (int64_t)S.c_step * (cw - 1) + 1;
    planes[0] = {S.y, S.y_row_pitch, S.y_frame_pitch, empty ? 0 : width, rows};
    planes[1] = {mode == CV_VU ? S.v : S.u, S.c_row_pitch, S.c_frame_pitch, c_row, c_rows};
    planes[2] = {S.v, S.c_row_pitch, S.c_frame_pitch, c_row, c_rows};
    tight = planes[0].row_bytes * rows + (n_planes - 1) * c_row * c_rows;
  }
  // what a kernel is given of the chunk `c` that frames_in_chunks hands to launch; paired: u is the lower address, v is not read
  void chunk(const FramePlane* c, const uint8_t*& y, const uint8_t*& u, const uint8_t*& v, int64_t& y_row, int64_t& y_frame, int64_t& c_row,
             int64_t& c_frame) const {
    y = c[0].base; u = c[1].base; v = c[n_planes - 1].base;
    y_row = c[0].row_pitch; y_frame = c[0].frame_pitch; c_row = c[1].row_pitch; c_frame = c[1].frame_pitch;
  }
};

// Planes that a call writes, a FrameOutput each: the luma plane, then ONE plane of pairs or two planes, as above.  Host planes of
// their own with c_step = 2 are the one layout a pitched copy cannot write without touching the bytes in between: the kernel
// writes them packed (`mode` and `c_step` are what the KERNEL is given: CV_PLANAR and 1 then), they are fetched into a packed
// host buffer of a chunk and spread from there by the host once the chunk is drained (done).
struct YuvOutput {
  int mode;
  int32_t c_step;
  int64_t tight;                             // packed bytes of a frame
  YuvOutput(const sba_yuv_planes& D_, int32_t height, int32_t width, bool on_device_)
      : D(D_), w(width), h(height), cw((width + 1) / 2), ch((height + 1) / 2), on_device(on_device_) {
    const int m = chroma_mode(D.u, D.v, D.c_row_pitch, D.c_step, cw);
    paired = m == CV_UV || m == CV_VU; spread = m == CV_STEP2 && !on_device;
    mode = spread ? CV_PLANAR : m;
    c_step = spread ? 1 : D.c_step;
    c_row = paired ? 2 * cw : cw;            // bytes of a row as a pitched copy moves it
    tight = w * h + (paired ? 1 : 2) * c_row * ch;
  }
  // once the frames of a chunk are known (frames_per_chunk)
  void alloc(int64_t chunk) {
    if (spread) { h_u.resize((size_t)(chunk * cw * ch)); h_v.resize((size_t)(chunk * cw * ch)); }
    uint8_t* lower = mode == CV_VU ? D.v : D.u;
    const int64_t c_row_pitch = spread ? cw : D.c_row_pitch, c_frame_pitch = spread ? cw * ch : D.c_frame_pitch;
    Oy.emplace(FrameOut{D.y, D.y_row_pitch, D.y_frame_pitch}, w, h, on_device, chunk);
    Ou.emplace(FrameOut{spread ? h_u.data() : lower, c_row_pitch, c_frame_pitch}, c_row, ch, on_device, chunk);
    Ov.emplace(FrameOut{spread ? h_v.data() : D.v, c_row_pitch, c_frame_pitch}, c_row, paired ? 0 : ch, on_device, chunk);
  }
  // what the kernels of the chunk that starts at frame lo write; paired: u is the lower address and v = u, not used
  void target(int64_t lo, uint8_t*& y, uint8_t*& u, uint8_t*& v, int64_t& y_row, int64_t& y_frame, int64_t& c_row_pitch, int64_t& c_frame) const {
    int64_t row, frame;
    Oy->target(lo, y, y_row, y_frame);
    Ou->target(lo, u, c_row_pitch, c_frame);
    v = u;
    if (!paired) Ov->target(lo, v, row, frame);                           // the same pitches as u
  }
  // frames_in_chunks' fetch and done
  void fetch(int64_t lo, int64_t m, hipStream_t st) const {
    Oy->fetch(lo, m, st);
    Ou->fetch(spread ? 0 : lo, m, st);                                    // spread: every chunk lands at the start of h_u, h_v
    Ov->fetch(spread ? 0 : lo, m, st);
  }
  void done(int64_t lo, int64_t m) const {
    if (!spread) return;
    for (int64_t f = 0; f < m; ++f)
      for (int64_t j = 0; j < ch; ++j) {
        const uint8_t *su = h_u.data() + (f * ch + j) * cw, *sv = h_v.data() + (f * ch + j) * cw;
        uint8_t *du = D.u + (lo + f) * D.c_frame_pitch + j * D.c_row_pitch, *dv = D.v + (lo + f) * D.c_frame_pitch + j * D.c_row_pitch;
        for (int64_t i = 0; i < cw; ++i) { du[2 * i] = su[i]; dv[2 * i] = sv[i]; }
      }
  }

 private:
  sba_yuv_planes D;
  int64_t w, h, cw, ch, c_row;
  bool on_device, paired, spread;
  std::vector<uint8_t> h_u, h_v;             // spread: the packed planes of a chunk on the host
  std::optional<FrameOutput> Oy, Ou, Ov;
};

}  // namespace sba_detect
