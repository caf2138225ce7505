// sba_background.hpp -- sba_background_accumulate and sba_background_suppress (include/sba_hip.h): what a pixel shows over the
// frames of a video (sum, square sum, count above the threshold, maximum of one channel) and the removal of what is always
// there.  The laser dot visits a pixel in a handful of frames, a lamp or a reflection sits in all of them: time is what tells
// them apart.  Every stored value is an integer, so any chunking and any split of the frames gives the same bits.
//
// k_bg_accumulate<C, ALL> is a reduction over time with one owner per pixel.  The bytes of a row are cut into groups of 16 from
// the row's first byte; a thread owns the pixels whose channel byte lies in its group, a wave 1024 contiguous bytes (waves run
// on across the rows).  The thread keeps its accumulators in registers over the frames of its share of the chunk and touches
// the caller's arrays once, at the end.  A group is ONE 16-byte load per frame at whatever alignment base and pitches give it
// (aligned whenever they are multiples of 16); the last group of a row, which may hold fewer than 16 bytes, loads the row's
// LAST 16 bytes instead and accumulates a few pixels of its neighbour beside its own, which it never stores -- no byte path
// but for rows shorter than 16 bytes.  Zero is neutral for all four accumulators, so a value shifted in from beyond the 16
// bytes needs no mask.  The loads of BG_UNROLL frames are in flight per lane, those of the next BG_UNROLL are issued before the
// first are folded.  Where a frame has too few groups to fill the chip (below BG_SPLIT_GROUPS) and the chunk more than
// BG_SPLIT_FRAMES frames, the frames are split over grid.y and merged with integer atomics: the sums into the arrays
// themselves, the maximum through 32-bit words that one more kernel folds into the bytes.
//
// k_bg_suppress<C> is element-wise: a thread owns 16 pixels of an output row (the last thread of a row the row's last 16, so
// that two threads may write the same bytes with the same values), folds level and mask into one byte per pixel once and
// walks the frames of its share.  The output leaves as 16-byte stores; padding is never written.
// How frames are described and staged chunk by chunk is sba_frames.hpp.
#pragma once
#include "sba_frames.hpp"

namespace sba_detect {

constexpr int BG_THREADS = 256;
constexpr int BG_UNROLL = 4;                 // frames whose loads a lane has in flight
constexpr int64_t BG_SPLIT_GROUPS = 65536;   // 16-byte groups of a frame (1024 waves) below which the frames are split over grid.y
constexpr int64_t BG_SPLIT_FRAMES = 16;      // frames of a share at least
constexpr int64_t BG_BLOCKS = 2048;          // workgroups a split launch aims at

__device__ __forceinline__ uint4 bg_load16(const uint8_t* p) {
  uint4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}
// the first n < 16 bytes at p, the rest zero
__device__ __forceinline__ uint4 bg_load_short(const uint8_t* p, int n) {
  uint32_t d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < 15; ++k)
    if (k < n) d[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
  return make_uint4(d[0], d[1], d[2], d[3]);
}

template <int C>
struct BgGroup {
  static constexpr int NPIX = (16 + C - 1) / C;
};

// a launch walks at most DOT_MAX_CHUNK = 16384 frames: 255^2 * 16384 < 2^32, the square sum of a share fits 32 bits
template <int C, bool ALL>
struct BgAcc {
  static constexpr int N = BgGroup<C>::NPIX;
  uint32_t s[N], q[N], h[N], m[N];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = q[k] = h[k] = m[k] = 0u;
  }
  __device__ __forceinline__ void fold(const uint4& v, uint32_t j0, uint32_t thr) {
    uint32_t d[4], b[N];
    channel_words<C>(v, j0, d);
#pragma unroll
    for (int k = 0; k < N; ++k) b[k] = channel_byte<C>(d, k);
#pragma unroll
    for (int k = 0; k < N; ++k) {
      s[k] += b[k];
      if (ALL) {
        q[k] += __umul24(b[k], b[k]);
        h[k] += b[k] > thr ? 1u : 0u;
        m[k] = max(m[k], b[k]);
      }
    }
  }
};

struct BgAccParams {
  FrameView V;
  uint32_t* sum;
  unsigned long long* sumsq;
  uint32_t* hot;
  uint8_t* vmax;
  uint32_t* vmax32;                          // split launches: the maximum as 32-bit words (k_bg_fold_max)
  const int32_t* idx;                        // the frames of the chunk that take part, ascending; nullptr: all of them
  int32_t n;                                 // how many take part
  int32_t frames_per_group;                  // of them a thread walks: grid.y shares
  int32_t row_groups;                        // 16-byte groups of a row
  int32_t add;                               // 0: the arrays are taken as zero and overwritten (not with `atomic`)
  int32_t atomic;                            // the frames are split: merge with atomics
};

// grid (groups of the frame / BG_THREADS, shares of the frames), BG_THREADS threads; P.V.frames is the chunk's first frame.
// ALL = false: only `sum` is asked for.
template <int C, bool ALL>
__global__ void __launch_bounds__(BG_THREADS) k_bg_accumulate(const BgAccParams P) {
  constexpr int N = BgGroup<C>::NPIX;
  const int t = (int)blockIdx.x * BG_THREADS + (int)threadIdx.x;          // <= 16384 * 4096
  if (t >= P.V.height * P.row_groups) return;
  const int y = t / P.row_groups, g = t - y * P.row_groups;
  const int be = P.V.width * C;                                           // bytes of a row
  const bool tiny = be < 16;                                              // the same in every thread
  const int os = g * 16, oe = min(be, os + 16);                           // the bytes this thread owns
  const int ls = tiny ? 0 : min(os, be - 16);                             // where it loads
  const uint32_t channel = (uint32_t)P.V.channel, thr = (uint32_t)P.V.threshold;
  const uint32_t q0 = (uint32_t)ls / C, r0 = (uint32_t)ls - q0 * C;
  const uint32_t j0 = channel >= r0 ? channel - r0 : channel + C - r0;    // the channel's first byte at or after ls
  const int xq = (int)(q0 + (channel < r0 ? 1u : 0u));                    // its pixel
  const uint8_t* __restrict__ rp = P.V.frames + ((int64_t)y * P.V.row_pitch + ls);
  const int j_lo = (int)blockIdx.y * P.frames_per_group, j_hi = min(P.n, j_lo + P.frames_per_group);
  auto frame = [&](int j) { return rp + (int64_t)(P.idx ? P.idx[j] : j) * P.V.frame_pitch; };

  BgAcc<C, ALL> A;
  A.clear();
  if (!tiny) {
    int j = j_lo;
    uint4 cur[BG_UNROLL];
    if (j + BG_UNROLL <= j_hi) {
#pragma unroll
      for (int u = 0; u < BG_UNROLL; ++u) cur[u] = bg_load16(frame(j + u));
    }
    while (j + BG_UNROLL <= j_hi) {
      const int jn = j + BG_UNROLL;
      const bool more = jn + BG_UNROLL <= j_hi;
      uint4 nxt[BG_UNROLL];
      if (more) {
#pragma unroll
        for (int u = 0; u < BG_UNROLL; ++u) nxt[u] = bg_load16(frame(jn + u));
      }
#pragma unroll
      for (int u = 0; u < BG_UNROLL; ++u) A.fold(cur[u], j0, thr);
      if (more) {
#pragma unroll
        for (int u = 0; u < BG_UNROLL; ++u) cur[u] = nxt[u];
      }
      j = jn;
    }
    for (; j < j_hi; ++j) A.fold(bg_load16(frame(j)), j0, thr);
  } else {
    for (int j = j_lo; j < j_hi; ++j) A.fold(bg_load_short(frame(j), be), j0, thr);
  }

#pragma unroll
  for (int k = 0; k < N; ++k) {
    const int pos = (xq + k) * C + (int)channel;                          // the byte of the row that value k came from
    if (pos < os || pos >= oe) continue;                                  // a neighbour's pixel, or beyond the 16 bytes
    const int64_t i = (int64_t)y * P.V.width + xq + k;
    if (P.atomic) {
      if (P.sum) atomicAdd(&P.sum[i], A.s[k]);
      if (ALL) {
        if (P.sumsq) atomicAdd(&P.sumsq[i], (unsigned long long)A.q[k]);
        if (P.hot) atomicAdd(&P.hot[i], A.h[k]);
        if (P.vmax32) atomicMax(&P.vmax32[i], A.m[k]);
      }
    } else {
      if (P.sum) P.sum[i] = (P.add ? P.sum[i] : 0u) + A.s[k];
      if (ALL) {
        if (P.sumsq) P.sumsq[i] = (P.add ? P.sumsq[i] : 0ull) + A.q[k];
        if (P.hot) P.hot[i] = (P.add ? P.hot[i] : 0u) + A.h[k];
        if (P.vmax) P.vmax[i] = (uint8_t)max(P.add ? (uint32_t)P.vmax[i] : 0u, A.m[k]);
      }
    }
  }
}

// after the split launches of a call: vmax = max(vmax, the words)
__global__ void __launch_bounds__(BG_THREADS) k_bg_fold_max(uint8_t* __restrict__ vmax, const uint32_t* __restrict__ vmax32, int64_t n, int add) {
  const int64_t i = (int64_t)blockIdx.x * BG_THREADS + threadIdx.x;
  if (i < n) vmax[i] = (uint8_t)max(add ? (uint32_t)vmax[i] : 0u, vmax32[i]);
}

struct BgSupParams {
  FrameView V;
  const uint8_t* level;                      // height * width, or nullptr: all 0
  const uint8_t* mask;                       // height * width, or nullptr: none
  uint8_t* out;
  int64_t out_row_pitch, out_frame_pitch;
  int32_t row_groups;                        // groups of 16 pixels of a row
  int32_t frames_per_group;
  int32_t mode;                              // 0 gate, 1 subtract
};

// grid (groups of the frame / BG_THREADS, shares of the frames), BG_THREADS threads; P.V.frames and P.out are the chunk's first frame
template <int C>
__global__ void __launch_bounds__(BG_THREADS) k_bg_suppress(const BgSupParams P, int n_frames) {
  constexpr int U = C == 1 ? 4 : 2;                                       // frames in flight: U * C 16-byte loads
  const int t = (int)blockIdx.x * BG_THREADS + (int)threadIdx.x;
  if (t >= P.V.height * P.row_groups) return;
  const int W = P.V.width;
  const int y = t / P.row_groups, g = t - y * P.row_groups;
  const bool tiny = W < 16;                                               // the same in every thread
  const int x0 = tiny ? 0 : min(g * 16, W - 16), np = tiny ? W : 16;
  const uint32_t channel = (uint32_t)P.V.channel;
  const bool subtract = P.mode == 1;

  // what a value has to exceed: the level, 255 under the mask (nothing exceeds it, and v - 255 <= 0)
  uint32_t lv[16];
  {
    const int64_t i = (int64_t)y * W + x0;
    uint4 l = make_uint4(0u, 0u, 0u, 0u), m = l;
    if (P.level) l = tiny ? bg_load_short(P.level + i, np) : bg_load16(P.level + i);
    if (P.mask) m = tiny ? bg_load_short(P.mask + i, np) : bg_load16(P.mask + i);
    const uint32_t lw[4] = {l.x, l.y, l.z, l.w}, mw[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) lv[k] = (mw[k >> 2] >> (8 * (k & 3)) & 0xffu) ? 255u : lw[k >> 2] >> (8 * (k & 3)) & 0xffu;
  }
  const int f_lo = (int)blockIdx.y * P.frames_per_group, f_hi = min(n_frames, f_lo + P.frames_per_group);
  const uint8_t* __restrict__ src = P.V.frames + ((int64_t)y * P.V.row_pitch + (int64_t)x0 * C);
  uint8_t* __restrict__ dst = P.out + ((int64_t)y * P.out_row_pitch + x0);

  if (tiny) {
    for (int f = f_lo; f < f_hi; ++f)
#pragma unroll
      for (int k = 0; k < 15; ++k)
        if (k < np) {
          const uint32_t v = src[(int64_t)f * P.V.frame_pitch + k * C + channel];
          dst[(int64_t)f * P.out_frame_pitch + k] = (uint8_t)(v > lv[k] ? (subtract ? v - lv[k] : v) : 0u);
        }
    return;
  }
  auto one = [&](const uint4 (&in)[C], int f) {
    uint32_t d[4 * C + 1];
#pragma unroll
    for (int c = 0; c < C; ++c) { d[4 * c] = in[c].x; d[4 * c + 1] = in[c].y; d[4 * c + 2] = in[c].z; d[4 * c + 3] = in[c].w; }
    d[4 * C] = 0u;
    if (C > 1) {                                                          // the channel's byte of pixel k to byte k C
#pragma unroll
      for (int w = 0; w < 4 * C; ++w) d[w] = __builtin_amdgcn_alignbyte(d[w + 1], d[w], channel);
    }
    uint32_t r[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const uint32_t v = (d[(k * C) >> 2] >> (8 * ((k * C) & 3))) & 0xffu;
      r[k >> 2] |= (v > lv[k] ? (subtract ? v - lv[k] : v) : 0u) << (8 * (k & 3));
    }
    const uint4 o = make_uint4(r[0], r[1], r[2], r[3]);
    __builtin_memcpy(dst + (int64_t)f * P.out_frame_pitch, &o, 16);
  };
  int f = f_lo;
  for (; f + U <= f_hi; f += U) {
    uint4 in[U][C];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int c = 0; c < C; ++c) in[u][c] = bg_load16(src + (int64_t)(f + u) * P.V.frame_pitch + 16 * c);
#pragma unroll
    for (int u = 0; u < U; ++u) one(in[u], f + u);
  }
  for (; f < f_hi; ++f) {
    uint4 in[C];
#pragma unroll
    for (int c = 0; c < C; ++c) in[c] = bg_load16(src + (int64_t)f * P.V.frame_pitch + 16 * c);
    one(in, f);
  }
}

// ------------------------------------------------------------------------------------------------ host side
// shares of the nf frames of a launch whose frame gives `blocks` workgroups, at least `min_frames` frames each
inline void bg_shares(int64_t blocks, int64_t nf, int64_t min_frames, int32_t& frames_per_group, unsigned& groups) {
  const int64_t want = std::max<int64_t>(1, std::min<int64_t>((nf + min_frames - 1) / min_frames, BG_BLOCKS / blocks));
  frames_per_group = (int32_t)((nf + want - 1) / want);
  groups = (unsigned)((nf + frames_per_group - 1) / frames_per_group);
}

inline void bg_accumulate_launch(BgAccParams P, int channels, bool all, hipStream_t st) {
  const int64_t threads = (int64_t)P.V.height * P.row_groups, blocks = (threads + BG_THREADS - 1) / BG_THREADS;
  unsigned groups = 1;
  P.frames_per_group = P.n;
  if (P.atomic) bg_shares(blocks, P.n, BG_SPLIT_FRAMES, P.frames_per_group, groups);
  const dim3 grid((unsigned)blocks, groups);
#define SBA_BG_ACC(Cn)                                                                                         \
  do {                                                                                                          \
    if (all) hipLaunchKernelGGL((k_bg_accumulate<Cn, true>), grid, dim3(BG_THREADS), 0, st, P);               \
    else hipLaunchKernelGGL((k_bg_accumulate<Cn, false>), grid, dim3(BG_THREADS), 0, st, P);                  \
  } while (0)
  if (channels == 1) SBA_BG_ACC(1);
  else if (channels == 3) SBA_BG_ACC(3);
  else SBA_BG_ACC(4);
#undef SBA_BG_ACC
  HIPCHK(hipGetLastError());
}

// Arguments are checked by the caller (sba_api.hip); n_frames > 0.  Accumulators in host memory pass through device copies,
// up before the first chunk (when the call adds to them) and down after the last.
int bg_accumulate_call(const FrameBatch& B, const sba_background_accumulate_opts& o, const uint8_t* use, uint32_t* sum, uint64_t* sumsq,
                       uint32_t* hot, uint8_t* vmax, uint64_t* n_used) {
  const int64_t n_frames = B.n_frames;
  const int32_t height = B.height, width = B.width, channels = B.channels;
  const int64_t px = (int64_t)height * width;
  const bool fresh = o.accumulate == 0, frames_dev = o.frames_on_device != 0, stats_dev = o.stats_on_device != 0;
  const int64_t chunk = chunk_of(CHUNK_FRAMES, o.chunk_frames, B, frames_dev);      // no frames written, yet chunk_frames holds for device frames too

  // the frames that take part, chunk by chunk, numbered from the chunk's first frame
  const int64_t n_chunks = n_frames > 0 ? (n_frames + chunk - 1) / chunk : 0;
  std::vector<int32_t> idx;
  std::vector<int64_t> first((size_t)n_chunks + 1, 0);
  int64_t used = n_frames;
  if (use) {
    idx.reserve((size_t)n_frames);
    for (int64_t c = 0; c < n_chunks; ++c) {
      for (int64_t f = c * chunk; f < std::min(n_frames, (c + 1) * chunk); ++f)
        if (use[f]) idx.push_back((int32_t)(f - c * chunk));
      first[(size_t)c + 1] = (int64_t)idx.size();
    }
    used = (int64_t)idx.size();
  }
  const uint64_t n_after = (fresh || !n_used ? 0 : *n_used) + (uint64_t)used;
  if (px == 0 || (used == 0 && !fresh)) { if (n_used) *n_used = n_after; return SBA_OK; }

  HIPCHK(hipSetDevice(B.device));
  DotStream s0;
  DevBuf<uint32_t> d_sum, d_hot, d_max32;
  DevBuf<unsigned long long> d_sq;
  DevBuf<uint8_t> d_max;
  DevBuf<int32_t> d_idx;
  BgAccParams P{};
  P.sum = sum; P.sumsq = reinterpret_cast<unsigned long long*>(sumsq); P.hot = hot; P.vmax = vmax;
  if (!stats_dev) {
    if (sum) { d_sum.alloc((size_t)px); P.sum = d_sum.p; }
    if (sumsq) { d_sq.alloc((size_t)px); P.sumsq = d_sq.p; }
    if (hot) { d_hot.alloc((size_t)px); P.hot = d_hot.p; }
    if (vmax) { d_max.alloc((size_t)px); P.vmax = d_max.p; }
  }
  auto zero = [&] {
    if (P.sum) HIPCHK(hipMemsetAsync(P.sum, 0, sizeof(uint32_t) * (size_t)px, s0.s));
    if (P.sumsq) HIPCHK(hipMemsetAsync(P.sumsq, 0, sizeof(uint64_t) * (size_t)px, s0.s));
    if (P.hot) HIPCHK(hipMemsetAsync(P.hot, 0, sizeof(uint32_t) * (size_t)px, s0.s));
  };
  auto download = [&] {
    if (!stats_dev) {
      if (sum) HIPCHK(hipMemcpyAsync(sum, P.sum, sizeof(uint32_t) * (size_t)px, hipMemcpyDeviceToHost, s0.s));
      if (sumsq) HIPCHK(hipMemcpyAsync(sumsq, P.sumsq, sizeof(uint64_t) * (size_t)px, hipMemcpyDeviceToHost, s0.s));
      if (hot) HIPCHK(hipMemcpyAsync(hot, P.hot, sizeof(uint32_t) * (size_t)px, hipMemcpyDeviceToHost, s0.s));
      if (vmax) HIPCHK(hipMemcpyAsync(vmax, P.vmax, (size_t)px, hipMemcpyDeviceToHost, s0.s));
    }
    HIPCHK(hipStreamSynchronize(s0.s));
  };
  if (used == 0) {                                                        // a fresh call without a frame: zeros
    zero();
    if (P.vmax) HIPCHK(hipMemsetAsync(P.vmax, 0, (size_t)px, s0.s));
    download();
    if (n_used) *n_used = n_after;
    return SBA_OK;
  }

  P.V = frame_view(B, o.channel, o.threshold);
  P.row_groups = (int32_t)(((int64_t)width * channels + 15) / 16);
  P.atomic = (int64_t)height * P.row_groups < BG_SPLIT_GROUPS && chunk > BG_SPLIT_FRAMES;
  const bool all = sumsq || hot || vmax;
  if (!stats_dev && !fresh) {
    if (sum) HIPCHK(hipMemcpyAsync(P.sum, sum, sizeof(uint32_t) * (size_t)px, hipMemcpyHostToDevice, s0.s));
    if (sumsq) HIPCHK(hipMemcpyAsync(P.sumsq, sumsq, sizeof(uint64_t) * (size_t)px, hipMemcpyHostToDevice, s0.s));
    if (hot) HIPCHK(hipMemcpyAsync(P.hot, hot, sizeof(uint32_t) * (size_t)px, hipMemcpyHostToDevice, s0.s));
    if (vmax) HIPCHK(hipMemcpyAsync(P.vmax, vmax, (size_t)px, hipMemcpyHostToDevice, s0.s));
  }
  if (P.atomic) {
    if (fresh) zero();
    if (vmax) {
      d_max32.alloc((size_t)px);
      P.vmax32 = d_max32.p;
      HIPCHK(hipMemsetAsync(P.vmax32, 0, sizeof(uint32_t) * (size_t)px, s0.s));
    }
  }
  if (use) {
    d_idx.alloc(idx.size());
    HIPCHK(hipMemcpyAsync(d_idx.p, idx.data(), sizeof(int32_t) * idx.size(), hipMemcpyHostToDevice, s0.s));
  }
  HIPCHK(hipStreamSynchronize(s0.s));                                     // the chunks run on streams of their own

  P.add = fresh ? 0 : 1;
  frames_in_chunks(
      P.V, channels, n_frames, frames_dev, chunk,
      [&](const FrameView& V, int64_t lo, int64_t m, hipStream_t st) {
        const int64_t c = lo / chunk;
        P.V = V;
        P.idx = use ? d_idx.p + first[(size_t)c] : nullptr;
        P.n = (int32_t)(use ? first[(size_t)c + 1] - first[(size_t)c] : m);
        if (P.n == 0) return;
        bg_accumulate_launch(P, channels, all, st);
        P.add = 1;
      },
      [](int64_t, int64_t, hipStream_t) {});
  if (P.vmax32) {
    hipLaunchKernelGGL(k_bg_fold_max, dim3((unsigned)((px + BG_THREADS - 1) / BG_THREADS)), dim3(BG_THREADS), 0, s0.s, P.vmax, P.vmax32, px,
                       fresh ? 0 : 1);
    HIPCHK(hipGetLastError());
  }
  download();
  if (n_used) *n_used = n_after;
  return SBA_OK;
}

// Arguments are checked by the caller (sba_api.hip).  Level and mask in host memory are copied to the device once; frames and
// output pass through the device as sba_frames.hpp has it (frames_in_chunks, FrameOutput).
int bg_suppress_call(const FrameBatch& B, const uint8_t* level, const uint8_t* mask, const FrameOut& out,
                     const sba_background_suppress_opts& o) {
  const int64_t n_frames = B.n_frames;
  const int32_t height = B.height, width = B.width, channels = B.channels;
  const int64_t px = (int64_t)height * width;
  if (n_frames == 0 || px == 0) return SBA_OK;
  HIPCHK(hipSetDevice(B.device));
  const bool in_dev = o.frames_on_device != 0, out_dev = o.out_on_device != 0;
  BgSupParams P{};
  P.V = frame_view(B, o.channel, 0);
  P.level = level; P.mask = mask; P.mode = o.mode;
  P.row_groups = (width + 15) / 16;
  DevBuf<uint8_t> d_level, d_mask;
  if (!o.model_on_device) {
    if (level) { d_level.alloc((size_t)px); HIPCHK(hipMemcpy(d_level.p, level, (size_t)px, hipMemcpyHostToDevice)); P.level = d_level.p; }
    if (mask) { d_mask.alloc((size_t)px); HIPCHK(hipMemcpy(d_mask.p, mask, (size_t)px, hipMemcpyHostToDevice)); P.mask = d_mask.p; }
  }
  const int64_t chunk = chunk_of(CHUNK_FRAMES, o.chunk_frames, B, in_dev, px, out_dev);   // px: never more than a frame takes
  FrameOutput O(out, width, height, out_dev, chunk);

  const int64_t blocks = ((int64_t)height * P.row_groups + BG_THREADS - 1) / BG_THREADS;
  frames_in_chunks(
      P.V, channels, n_frames, in_dev, chunk,
      [&](const FrameView& V, int64_t lo, int64_t m, hipStream_t st) {
        P.V = V;
        O.target(lo, P.out, P.out_row_pitch, P.out_frame_pitch);
        unsigned groups;
        bg_shares(blocks, m, 1, P.frames_per_group, groups);              // which share takes a frame does not change its bytes
        const dim3 grid((unsigned)blocks, groups);
        if (channels == 1) hipLaunchKernelGGL(k_bg_suppress<1>, grid, dim3(BG_THREADS), 0, st, P, (int)m);
        else if (channels == 3) hipLaunchKernelGGL(k_bg_suppress<3>, grid, dim3(BG_THREADS), 0, st, P, (int)m);
        else hipLaunchKernelGGL(k_bg_suppress<4>, grid, dim3(BG_THREADS), 0, st, P, (int)m);
        HIPCHK(hipGetLastError());
      },
      [&](int64_t lo, int64_t m, hipStream_t st) { O.fetch(lo, m, st); });
  return SBA_OK;
}

}  // namespace sba_detect
