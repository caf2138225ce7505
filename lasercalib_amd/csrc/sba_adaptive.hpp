// sba_adaptive.hpp -- sba_adaptive_threshold (include/sba_hip.h): cv.adaptiveThreshold(ADAPTIVE_THRESH_MEAN_C) of one value
// per pixel (a channel's byte or the grey value), for up to four window sizes in one call -- the first stage of
// cv2.aruco's detectMarkers, which runs it with the windows 3, 13 and 23.  The rule -- replicated border, integer window
// sums, the mean as the integer nearest to S / b^2, the comparison of v - mean with -delta -- is written out in the header.
//
// One kernel, k_adaptive<C, GRAY>, one launch per chunk for all windows.  A workgroup owns a TILE of tw x th pixels of one
// frame.  R is the largest half window of the call, L = R + 1 rounded up to a multiple of four.
//   * In: the values of the tile with a halo of L columns on the left, R on the right and R rows above and below are read from
//     global memory ONCE, a wave per row with AT_ROWS rows in flight, a lane four neighbouring pixels: tw and L are multiples
//     of four, so a lane's 4 C bytes start on a 4-byte boundary of the row and are read as C words where the ADDRESS allows it, byte by byte with
//     coordinates clamped to the frame -- the replicated border -- where the frame's edge cuts them or the row is not aligned.
//     What goes to LDS is not the value but the row's running sum I(j, i) = v(j, 0) + ... + v(j, i) (at_wave_scan: DPP adds,
//     no LDS), as 16-bit values that wrap: a difference of two of them is exact modulo 2^16, and every difference that is taken -- a value, or
//     the sum of up to 127 of them, 255 * 127 = 32385 -- is below 2^16.  So one LDS array of 2 bytes per pixel serves every
//     window: the row sum of window b = 2 r + 1 at column x is I(x + r) - I(x - r - 1), two reads, whatever b is.
//   * The walk, after ONE barrier: a thread owns a column of the tile (and, in the narrow tiles, one of 2 or 4 segments of its
//     rows).  Per window -- all windows side by side in registers, so that their LDS reads do not wait for each other -- it
//     adds the 2 r + 1 row sums of its first pixel and then walks down: S += rowsum(y + r + 1) - rowsum(y - r).  The lanes of
//     a wave read neighbouring 16-bit values of one LDS row, two lanes to a bank: no conflicts.  S <= 255 * 127^2 < 2^24 is
//     exact in float32, and mean = rint(fl32(S) * fl32(1 / b^2)) is the header's rule 4 for every b <= 127
//     (tests/test_adaptive_host.py checks that for every S).
//   * Out: a lane writes the byte of its column, the 64 lanes of a wave 64 neighbouring bytes of one output row, at any base
//     and pitch; padding is never written.  (The rows are not staged in LDS for 16-byte stores as k_resize's are: a thread owns
//     a column here, and a staged tile per window would take the LDS that the halo needs.)
// The tile is chosen on the host from R (at_tile) so that the LDS array stays within 64 KiB.  Up to window 97 a row of the tile
// with its halo is the 256 columns a wave reads in ONE step: tw = 256 - L - R rounded down to a multiple of four (232 at window
// 23, where 64 rows take 43 KiB: three workgroups to a CU), th = 64 up to window 65 and 32 beyond.  Larger windows take 128 x 32
// or 64 x 32 pixels and two steps a row; there the halo is most of what is read.
// No atomics, no scratch; a pixel's bytes depend on nothing but the frame.  Chunks, staging and outputs are those of
// sba_frames.hpp.
#pragma once
#include "sba_frames.hpp"

namespace sba_detect {

constexpr int AT_THREADS = 256, AT_WAVES = AT_THREADS / 64;
constexpr int AT_MAX_WINDOWS = 4, AT_MAX_BLOCK = 127;
constexpr int AT_RUN = 4;                                    // pixels of a row a lane reads in one step
constexpr int AT_STEP = 64 * AT_RUN;                         // columns a wave reads in one step
constexpr int AT_ROWS = 4;                                   // rows of the tile a wave has in flight
constexpr int AT_LDS_VALUES = 32768;                         // 16-bit values of a tile with its halo: 64 KiB
constexpr int AT_ONE_STEP_R = 48, AT_TALL_R = 32;            // largest R of the one-step tiles, and of those with 64 rows

struct AtParams {
  const uint8_t* src;                        // of the chunk's first frame
  int64_t row_pitch, frame_pitch;
  uint8_t* out[AT_MAX_WINDOWS];              // of the chunk's first frame, per window; null: not asked for
  uint8_t* mean[AT_MAX_WINDOWS];
  int64_t out_row_pitch, out_frame_pitch;
  int32_t height, width, channel;
  int32_t n_windows, r[AT_MAX_WINDOWS], delta[AT_MAX_WINDOWS];
  float scale[AT_MAX_WINDOWS];               // fl32(1.0f / b^2), formed on the host
  int32_t R, L;                              // the largest r; the halo on the left
  int32_t tw, th, seg_rows;                  // the tile; rows of a segment = th / (AT_THREADS / tw)
  int32_t pitch;                             // 16-bit values of an LDS row: tw + L + R rounded up to a multiple of AT_RUN
  int32_t invert, max_value;
  int32_t w0, w1, w2;                        // grey weights
};

// The 4 C bytes of the pixels xs .. xs + 3 of the row at rp, in C words; a pixel outside the frame is the nearest one inside
template <int C>
__device__ __forceinline__ uint4 at_load(const uint8_t* __restrict__ rp, int xs, int width) {
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  if (xs >= 0 && xs + AT_RUN <= width && (reinterpret_cast<uintptr_t>(rp + xs * C) & 3u) == 0) {
    const uint32_t* __restrict__ p = reinterpret_cast<const uint32_t*>(rp + xs * C);
#pragma unroll
    for (int i = 0; i < C; ++i) w[i] = p[i];
  } else {
#pragma unroll
    for (int q = 0; q < AT_RUN; ++q) {
      const uint8_t* __restrict__ p = rp + min(max(xs + q, 0), width - 1) * C;
#pragma unroll
      for (int c = 0; c < C; ++c) w[(q * C + c) >> 2] |= (uint32_t)p[c] << 8 * ((q * C + c) & 3);
    }
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// The running sum of t over the lanes of a wave, the lane's own value included, without LDS: inside a row of 16 lanes by shifts
// of 1, 2, 4 and 8 lanes (a lane without a source adds 0), then the total of row 0 into row 1 and of row 2 into row 3, then
// the total of the first two rows into the last two
__device__ __forceinline__ uint32_t at_wave_scan(uint32_t t) {
  int x = (int)t;
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);         // row_shr:1
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);         // row_shr:2
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);         // row_shr:4
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);         // row_shr:8
  x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);         // row_bcast:15 into rows 1 and 3
  x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);         // row_bcast:31 into rows 2 and 3
  return (uint32_t)x;
}

// grid (tiles of a row, tiles of a column, frames of the chunk), AT_THREADS threads, 2 * (th + 2 R) * pitch bytes of LDS
template <int C, bool GRAY>
__global__ void __launch_bounds__(AT_THREADS) k_adaptive(const AtParams P) {
  extern __shared__ __attribute__((aligned(16))) uint16_t s_run[];        // [th + 2 R][pitch]: I(j, i), modulo 2^16
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = (int)blockIdx.x * P.tw, y0 = (int)blockIdx.y * P.th;
  const int ncols = min(P.tw, P.width - x0), nrows = min(P.th, P.height - y0);
  const int lcols = ncols + P.L + P.R, lrows = nrows + 2 * P.R;           // LDS column i is frame column x0 - L + i
  const uint8_t* __restrict__ fp = P.src + (int64_t)blockIdx.z * P.frame_pitch;

  for (int j0 = wave; j0 < lrows; j0 += AT_WAVES * AT_ROWS) {             // LDS row j is frame row y0 - R + j; AT_ROWS rows in flight
    uint32_t carry[AT_ROWS];
#pragma unroll
    for (int u = 0; u < AT_ROWS; ++u) carry[u] = 0;
    for (int i0 = 0; i0 < lcols; i0 += AT_STEP) {                         // the bounds are the same in every lane
      const int i = i0 + lane * AT_RUN;
      uint4 raw[AT_ROWS];
#pragma unroll
      for (int u = 0; u < AT_ROWS; ++u) {
        const int j = j0 + u * AT_WAVES;
        raw[u] = make_uint4(0u, 0u, 0u, 0u);
        if (j < lrows) raw[u] = at_load<C>(fp + (int64_t)min(max(y0 - P.R + j, 0), P.height - 1) * P.row_pitch, x0 - P.L + i, P.width);
      }
#pragma unroll
      for (int u = 0; u < AT_ROWS; ++u) {
        const int j = j0 + u * AT_WAVES;
        uint32_t d[4], s[AT_RUN];                                         // s: the running sum inside the lane
        channel_words<C>(raw[u], GRAY ? 0u : (uint32_t)P.channel, d);
#pragma unroll
        for (int q = 0; q < AT_RUN; ++q) {
          uint32_t v;                                                     // rule 1
          if (GRAY) {
            const uint32_t c0 = d[(q * C) >> 2] >> 8 * ((q * C) & 3) & 255u, c1 = d[(q * C + 1) >> 2] >> 8 * ((q * C + 1) & 3) & 255u,
                           c2 = d[(q * C + 2) >> 2] >> 8 * ((q * C + 2) & 3) & 255u;
            v = (c0 * (uint32_t)P.w0 + c1 * (uint32_t)P.w1 + c2 * (uint32_t)P.w2 + (1u << 14)) >> 15;
          } else v = channel_byte<C>(d, q);
          s[q] = q ? s[q - 1] + v : v;
        }
        const uint32_t t = at_wave_scan(s[AT_RUN - 1]);                   // across the wave
        const uint32_t before = carry[u] + t - s[AT_RUN - 1];
        if (j < lrows && i < P.pitch)                                     // pitch is a multiple of AT_RUN: the four fit
          *reinterpret_cast<uint2*>(s_run + j * P.pitch + i) = make_uint2(((before + s[0]) & 0xffffu) | (before + s[1]) << 16,
                                                                          ((before + s[2]) & 0xffffu) | (before + s[3]) << 16);
        carry[u] += (uint32_t)__builtin_amdgcn_readlane((int)t, 63);
      }
    }
  }
  __syncthreads();

  const int seg = (int)threadIdx.x / P.tw, c = (int)threadIdx.x - seg * P.tw;
  const int ya = seg * P.seg_rows, yb = min(ya + P.seg_rows, nrows);       // seg_rows = th beyond the last segment: ya >= nrows
  if (c >= ncols || ya >= yb) return;
  // col[j pitch + e] is I at the tile's column c + e of LDS row j; the row sum of a window there is rowsum(row, r): the r + 1 <= L
  // columns to the left and the r <= R to the right exist
  const uint16_t* col = s_run + (c + P.L);
  auto rowsum = [](const uint16_t* p, int r) { return (uint32_t)(uint16_t)(p[r] - p[-r - 1]); };
  uint32_t S[AT_MAX_WINDOWS];                                             // the windows side by side: their LDS reads do not wait for each other
#pragma unroll
  for (int k = 0; k < AT_MAX_WINDOWS; ++k) {
    S[k] = 0;
    if (k < P.n_windows) {
      const int r = P.r[k];
      const uint16_t* p = col + (ya + P.R - r) * P.pitch;
#pragma unroll 4
      for (int j = 0; j <= 2 * r; ++j, p += P.pitch) S[k] += rowsum(p, r);
    }
  }
  const uint16_t* p = col + (ya + P.R) * P.pitch;
  int64_t at = (int64_t)blockIdx.z * P.out_frame_pitch + (int64_t)(y0 + ya) * P.out_row_pitch + (x0 + c);
#pragma unroll 2
  for (int y = ya; y < yb; ++y, p += P.pitch, at += P.out_row_pitch) {
    const int v = (int)(uint16_t)(p[0] - p[-1]);
#pragma unroll
    for (int k = 0; k < AT_MAX_WINDOWS; ++k)
      if (k < P.n_windows) {
        const int r = P.r[k];
        const int mean = __float2int_rn(__fmul_rn((float)S[k], P.scale[k]));
        if (P.mean[k]) P.mean[k][at] = (uint8_t)mean;
        if (P.out[k]) P.out[k][at] = (uint8_t)(((v - mean > -P.delta[k]) != (P.invert != 0)) ? P.max_value : 0);
        if (y + 1 < yb) S[k] += rowsum(p + (r + 1) * P.pitch, r) - rowsum(p - r * P.pitch, r);
      }
  }
}

// ------------------------------------------------------------------------------------------------ host side
// The tile of a call with the largest half window R.  R <= AT_ONE_STEP_R: the widest tile whose row with the halo is one step
// of a wave, 64 rows while 64 + 2 R rows of AT_STEP values fit the LDS array, else 32.  Beyond: 128 x 32 or 64 x 32, whichever
// fits (the last does at R = 63: 158 rows of 192 values).
inline void at_tile(AtParams& P) {
  P.L = (P.R + 1 + AT_RUN - 1) / AT_RUN * AT_RUN;
  if (P.R <= AT_ONE_STEP_R) {
    P.tw = (AT_STEP - P.L - P.R) / AT_RUN * AT_RUN; P.th = P.R <= AT_TALL_R ? 64 : 32;
    P.pitch = AT_STEP;
  } else {
    P.tw = 128; P.th = 32;
    P.pitch = (P.tw + P.L + P.R + AT_RUN - 1) / AT_RUN * AT_RUN;
    if ((P.th + 2 * P.R) * P.pitch > AT_LDS_VALUES) { P.tw = 64; P.pitch = (P.tw + P.L + P.R + AT_RUN - 1) / AT_RUN * AT_RUN; }
  }
  P.seg_rows = P.th / (AT_THREADS / P.tw);                                // one segment for every tw > 128
}

inline void at_launch(const AtParams& P, int channels, int64_t nf, hipStream_t st) {
  const dim3 grid((unsigned)((P.width + P.tw - 1) / P.tw), (unsigned)((P.height + P.th - 1) / P.th), (unsigned)nf), block(AT_THREADS);
  const size_t lds = (size_t)(P.th + 2 * P.R) * P.pitch * sizeof(uint16_t);
  const bool gray = P.channel < 0;
  if (channels == 1) hipLaunchKernelGGL((k_adaptive<1, false>), grid, block, lds, st, P);
  else if (channels == 3 && gray) hipLaunchKernelGGL((k_adaptive<3, true>), grid, block, lds, st, P);
  else if (channels == 3) hipLaunchKernelGGL((k_adaptive<3, false>), grid, block, lds, st, P);
  else if (gray) hipLaunchKernelGGL((k_adaptive<4, true>), grid, block, lds, st, P);
  else hipLaunchKernelGGL((k_adaptive<4, false>), grid, block, lds, st, P);
  HIPCHK(hipGetLastError());
}

// Arguments are checked by the caller (sba_api.hip): n_frames > 0, the windows, the weights set, one output at least.  Chunks,
// staging and outputs are those of sba_frames.hpp: a FrameOutput per window and kind of output, which share the pitches.
int adaptive_call(const FrameBatch& B, const sba_adaptive_opts& o, const FrameOut& out, int64_t out_window_pitch, uint8_t* mean_out) {
  const int64_t n_frames = B.n_frames;
  const int32_t height = B.height, width = B.width, channels = B.channels;
  if (height == 0 || width == 0) return SBA_OK;
  HIPCHK(hipSetDevice(B.device));
  const bool in_dev = o.frames_on_device != 0, out_dev = o.out_on_device != 0;
  const int K = o.n_windows;
  AtParams P{};
  P.height = height; P.width = width; P.channel = o.channel; P.n_windows = K;
  P.invert = o.invert; P.max_value = o.max_value ? o.max_value : 255;
  P.w0 = o.gray_w[0]; P.w1 = o.gray_w[1]; P.w2 = o.gray_w[2];
  for (int k = 0; k < K; ++k) {
    P.r[k] = o.block[k] / 2; P.delta[k] = o.delta[k];
    P.scale[k] = 1.0f / (float)(o.block[k] * o.block[k]);
    P.R = std::max(P.R, P.r[k]);
  }
  at_tile(P);
  const int64_t out_bytes = (int64_t)width * height * K * ((out.out ? 1 : 0) + (mean_out ? 1 : 0));
  // neither policy of chunk_of: a side counts only when it is host memory itself, so masks that stay on the device, up to eight
  // planes a frame, do not shrink the staging copies of host frames
  const int64_t chunk = frames_per_chunk(o.chunk_frames, n_frames, std::max(in_dev ? 0 : frame_bytes(B), out_dev ? 0 : out_bytes));
  std::optional<FrameOutput> O[2][AT_MAX_WINDOWS];                        // masks, means
  for (int k = 0; k < K; ++k) {
    if (out.out) O[0][k].emplace(FrameOut{out.out + k * out_window_pitch, out.row_pitch, out.frame_pitch}, width, height, out_dev, chunk);
    if (mean_out) O[1][k].emplace(FrameOut{mean_out + k * out_window_pitch, out.row_pitch, out.frame_pitch}, width, height, out_dev, chunk);
  }
  const FramePlane src = frame_plane(B);
  frames_in_chunks(
      &src, 1, n_frames, in_dev, chunk,
      [&](const FramePlane* c, int64_t lo, int64_t m, hipStream_t st) {
        P.src = c->base; P.row_pitch = c->row_pitch; P.frame_pitch = c->frame_pitch;
        for (int k = 0; k < K; ++k) {
          if (O[0][k]) O[0][k]->target(lo, P.out[k], P.out_row_pitch, P.out_frame_pitch);
          if (O[1][k]) O[1][k]->target(lo, P.mean[k], P.out_row_pitch, P.out_frame_pitch);
        }
        at_launch(P, channels, m, st);
      },
      [&](int64_t lo, int64_t m, hipStream_t st) {
        for (int k = 0; k < K; ++k)
          for (auto& side : O)
            if (side[k]) side[k]->fetch(lo, m, st);
      });
  return SBA_OK;
}

}  // namespace sba_detect
