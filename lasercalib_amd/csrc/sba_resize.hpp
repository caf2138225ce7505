// sba_resize.hpp -- sba_resize_frames (include/sba_hip.h): every output pixel is the average of a block of fx x fy source
// pixels (cv2.resize(..., INTER_AREA) at an integer factor), of every channel or of the grey value formed per source pixel
// (cv2.cvtColor(COLOR_BGR2GRAY)).  The rule -- integer sums, the 2 x 2 half-up case, otherwise one float32 multiply by
// fl32(1 / (fx fy)) rounded to nearest even -- is written out in the header and evaluated here by rs_gray and rs_round.
//
// One kernel, k_resize<C, GRAY>, a streaming read: every source byte once, 1 / (fx fy) of them (a third or a quarter of that
// with grey) written.  An ITEM is what is summed: a source byte, or with grey a source pixel.  A wave owns one output row of
// a SEGMENT of seg_px output pixels, that is RS_ITEMS = 64 x 16 items of each of its fy source rows at the most; seg_px is
// chosen so that a segment starts on a 16-byte boundary of the row.
//   * Down the rows: a lane owns the SAME 16 items of every source row, so the fy values of a column meet in its registers,
//     two 16-bit sums to a word (fy * 255 < 2^16).  Without grey the 16 items are one 16-byte load, and neighbouring lanes
//     read neighbouring vectors whatever C is: a 12-byte block of 3-channel pixels lies across lanes, not across loads.  With
//     grey a lane needs the 16 C bytes of its 16 pixels: the wave loads C vectors per lane in order (lane, lane + 64, ...),
//     passes them through LDS and each lane reads its own 16 C bytes back.  Rows of one band sit at different alignments
//     when the pitch is no multiple of 16, so a load chooses its width from its ADDRESS (cv_load16 of sba_convert.hpp); the
//     vector that the end of the segment cuts is read byte by byte, and what lies behind it -- the rest of the row, the
//     padding -- is never read.
//   * Along the row: the 1024 column sums go to LDS as 16-bit values; the sums of neighbouring lanes meet there.  Output
//     value j (pixel j / IC, channel j % IC) adds its fx items, IC apart, and is rounded.
//   * Out: the bytes of the output row are placed in LDS at the alignment of their destination address and leave as 16-byte
//     stores, with single bytes only in front of the first and behind the last 16-byte boundary of the ADDRESS, as in
//     sba_undistort.hpp: bases and pitches may be anything, padding is never written.
// The LDS traffic is between the lanes of one wave (wave_lds_sync); the waves of a workgroup take neighbouring output rows and
// never wait for each other.  How frames are staged chunk by chunk is frames_in_chunks (sba_frames.hpp).
#pragma once
#include "sba_convert.hpp"

namespace sba_detect {

constexpr int RS_RUN = 16;                                   // items of a row a lane owns
constexpr int RS_ITEMS = 64 * RS_RUN;                        // items of a row a wave takes in one step
constexpr int RS_OUT_LDS = 16 + RS_ITEMS;                    // an output row of a segment behind up to 15 bytes of misalignment
constexpr int RS_MAX_FACTOR = 16;

struct RsParams {
  const uint8_t* src;                        // of the chunk's first frame
  int64_t row_pitch, frame_pitch;
  uint8_t* out;
  int64_t out_row_pitch, out_frame_pitch;
  int32_t out_h, out_w, fx, fy;
  int32_t seg_px, rows_per_band;             // output pixels of a segment; output rows of a workgroup
  int32_t w0, w1, w2;                        // grey weights
  int32_t half_up;                           // fx == 2 && fy == 2
  float scale;                               // fl32(1.0f / (fx fy)), formed on the host
};

// The bytes [off, off + 16) of a row of which [0, nb) may be read; a byte that may not is zero
__device__ __forceinline__ uint4 rs_load(const uint8_t* __restrict__ rp, int off, int nb) {
  if (off + 16 <= nb) return cv_load16(rp + off);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (off + i < nb) w[i >> 2] |= (uint32_t)rp[off + i] << 8 * (i & 3);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// step 1 of the header's rule
__device__ __forceinline__ uint32_t rs_gray(const RsParams& P, uint32_t c0, uint32_t c1, uint32_t c2) {
  return (c0 * (uint32_t)P.w0 + c1 * (uint32_t)P.w1 + c2 * (uint32_t)P.w2 + (1u << 14)) >> 15;
}
// step 2: the value of the sum s <= 255 * 256
__device__ __forceinline__ uint32_t rs_round(const RsParams& P, uint32_t s) {
  if (P.half_up) return (s + 2u) >> 2;
  return (uint32_t)__float2int_rn(__fmul_rn((float)s, P.scale));
}

// grid (segments of a row, bands of rows_per_band output rows, frames of the chunk), DOT_THREADS threads
template <int C, bool GRAY>
__global__ void __launch_bounds__(DOT_THREADS) k_resize(const RsParams P) {
  constexpr int IC = GRAY ? 1 : C;                           // values of an output pixel = items of a source pixel
  constexpr int IB = GRAY ? C : 1;                           // bytes of an item
  __shared__ __attribute__((aligned(16))) uint16_t s_sum[DOT_WAVES][RS_ITEMS];
  __shared__ __attribute__((aligned(16))) uint8_t s_out[DOT_WAVES][RS_OUT_LDS];
  __shared__ __attribute__((aligned(16))) uint8_t s_raw[GRAY ? DOT_WAVES : 1][GRAY ? RS_ITEMS * C : 16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int px0 = (int)blockIdx.x * P.seg_px, npx = min(P.seg_px, P.out_w - px0);
  const int nitems = npx * P.fx * IC, nb = nitems * IB, nout = npx * IC;          // nitems <= RS_ITEMS: the host's seg_px
  const int64_t f = blockIdx.z;
  const uint8_t* __restrict__ fp = P.src + (f * P.frame_pitch + (int64_t)px0 * P.fx * C);
  uint16_t* sum = s_sum[wave];
  uint8_t* srow = s_out[wave];

  for (int y = (int)blockIdx.y * P.rows_per_band + wave; y < min(P.out_h, ((int)blockIdx.y + 1) * P.rows_per_band); y += DOT_WAVES) {
    const uint8_t* __restrict__ rp = fp + (int64_t)y * P.fy * P.row_pitch;
    uint32_t acc[RS_RUN / 2];                                // item k of the lane: bits 16 (k & 1) of acc[k >> 1]
#pragma unroll
    for (int i = 0; i < RS_RUN / 2; ++i) acc[i] = 0;
    if (!GRAY) {
      uint32_t lo[4] = {0u, 0u, 0u, 0u}, hi[4] = {0u, 0u, 0u, 0u};               // bytes 0 and 2, bytes 1 and 3 of a word
      for (int r0 = 0; r0 < P.fy; r0 += 4) {                // four rows in flight; the bound is the same in every lane
        uint4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          v[k] = r0 + k < P.fy ? rs_load(rp + (int64_t)(r0 + k) * P.row_pitch, lane * RS_RUN, nb) : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t w[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
          for (int i = 0; i < 4; ++i) { lo[i] += w[i] & 0x00ff00ffu; hi[i] += w[i] >> 8 & 0x00ff00ffu; }
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc[2 * i] = (lo[i] & 0xffffu) | hi[i] << 16;
        acc[2 * i + 1] = lo[i] >> 16 | (hi[i] & 0xffff0000u);
      }
    } else {
      uint8_t* raw = s_raw[wave];
      for (int r = 0; r < P.fy; ++r) {
        const uint8_t* __restrict__ p = rp + (int64_t)r * P.row_pitch;
        uint4 v[C];
#pragma unroll
        for (int q = 0; q < C; ++q) v[q] = rs_load(p, (q * 64 + lane) * 16, nb);
#pragma unroll
        for (int q = 0; q < C; ++q) *reinterpret_cast<uint4*>(raw + (q * 64 + lane) * 16) = v[q];
        wave_lds_sync();
        uint32_t w[4 * C];                                   // the lane's 16 pixels
#pragma unroll
        for (int q = 0; q < C; ++q) {
          const uint4 t = *reinterpret_cast<const uint4*>(raw + lane * (16 * C) + 16 * q);
          w[4 * q] = t.x; w[4 * q + 1] = t.y; w[4 * q + 2] = t.z; w[4 * q + 3] = t.w;
        }
        wave_lds_sync();                                      // read before the next row overwrites it
#pragma unroll
        for (int k = 0; k < RS_RUN; ++k) {                   // byte k C + c of the 16 C: constants after unrolling
          const uint32_t c0 = cv_byte(w[(k * C) >> 2], (k * C) & 3), c1 = cv_byte(w[(k * C + 1) >> 2], (k * C + 1) & 3),
                         c2 = cv_byte(w[(k * C + 2) >> 2], (k * C + 2) & 3);
          acc[k >> 1] += rs_gray(P, c0, c1, c2) << 16 * (k & 1);
        }
      }
    }
    *reinterpret_cast<uint4*>(sum + lane * RS_RUN) = make_uint4(acc[0], acc[1], acc[2], acc[3]);
    *reinterpret_cast<uint4*>(sum + lane * RS_RUN + 8) = make_uint4(acc[4], acc[5], acc[6], acc[7]);
    wave_lds_sync();

    uint8_t* dst = P.out + (f * P.out_frame_pitch + (int64_t)y * P.out_row_pitch + (int64_t)px0 * IC);
    const int a = (int)(reinterpret_cast<uintptr_t>(dst) & 15u);          // the LDS row lies as the destination does, modulo 16
    for (int j = lane; j < nout; j += 64) {
      const int px = j / IC, first = px * P.fx * IC + (j - px * IC);
      uint32_t s = 0;
      for (int dx = 0; dx < P.fx; ++dx) s += sum[first + dx * IC];       // first + (fx - 1) IC < nitems
      srow[a + j] = (uint8_t)rs_round(P, s);
    }
    wave_lds_sync();
    const int head = min(nout, (16 - a) & 15), nv = (nout - head) >> 4, tail = head + nv * 16;   // nv <= 64: a vector per lane
    if (lane < nv) *reinterpret_cast<uint4*>(dst + head + 16 * lane) = *reinterpret_cast<const uint4*>(srow + a + head + 16 * lane);
    const int b = lane < 32 ? lane : tail + (lane - 32);                  // lanes 0..14: in front of the vectors; 32..46: behind
    if (b < (lane < 32 ? head : nout)) dst[b] = srow[a + b];
    wave_lds_sync();                                          // read before the next row's sums and bytes overwrite them
  }
}

// ------------------------------------------------------------------------------------------------ host side
// The output pixels of a segment: as many as RS_ITEMS items of a source row hold, in whole multiples of the count after which
// a segment's first byte is a multiple of 16 bytes into the row again (>= 16 for every fx <= 16, C <= 4)
inline int rs_segment_px(int fx, int channels, bool gray) {
  const int per_px = fx * (gray ? 1 : channels), bytes_px = fx * channels;
  int g = 16, b = bytes_px;
  while (b) { const int t = g % b; g = b; b = t; }           // gcd(16, bytes of a block's row)
  const int step = 16 / g;
  return RS_ITEMS / per_px / step * step;
}

inline void rs_launch(RsParams P, int channels, bool gray, int64_t nf, hipStream_t st) {
  P.seg_px = rs_segment_px(P.fx, channels, gray);
  const int64_t nseg = (P.out_w + P.seg_px - 1) / P.seg_px;
  P.rows_per_band = frame_rows_per_band((int64_t)P.out_h * nseg, nf);
  const dim3 grid((unsigned)nseg, (unsigned)((P.out_h + P.rows_per_band - 1) / P.rows_per_band), (unsigned)nf), block(DOT_THREADS);
  if (gray) {
    if (channels == 3) hipLaunchKernelGGL((k_resize<3, true>), grid, block, 0, st, P);
    else hipLaunchKernelGGL((k_resize<4, true>), grid, block, 0, st, P);
  } else if (channels == 1) hipLaunchKernelGGL((k_resize<1, false>), grid, block, 0, st, P);
  else if (channels == 3) hipLaunchKernelGGL((k_resize<3, false>), grid, block, 0, st, P);
  else hipLaunchKernelGGL((k_resize<4, false>), grid, block, 0, st, P);
  HIPCHK(hipGetLastError());
}

// Arguments are checked by the caller (sba_api.hip): n_frames > 0, both output sizes > 0, the weights set.  Chunks, staging
// and output are those of sba_frames.hpp (chunk_of by CHUNK_FRAMES: the source is never the smaller side; frames_in_chunks;
// FrameOutput).  Which chunk, workgroup or buffer a frame passes through does not enter its arithmetic.
int resize_call(const FrameBatch& B, int32_t fx, int32_t fy, const FrameOut& out, const sba_resize_opts& o) {
  const int32_t channels = B.channels;
  HIPCHK(hipSetDevice(B.device));
  const bool gray = o.gray != 0, in_dev = o.frames_on_device != 0, out_dev = o.out_on_device != 0;
  RsParams P{};
  P.out_h = B.height / fy; P.out_w = B.width / fx; P.fx = fx; P.fy = fy;
  P.w0 = o.gray_w[0]; P.w1 = o.gray_w[1]; P.w2 = o.gray_w[2];
  P.half_up = fx == 2 && fy == 2;
  P.scale = 1.0f / (float)(fx * fy);
  const int64_t out_row = (int64_t)P.out_w * (gray ? 1 : channels);
  const int64_t chunk = chunk_of(CHUNK_FRAMES, o.chunk_frames, B, in_dev, out_row * P.out_h, out_dev);
  FrameOutput O(out, out_row, P.out_h, out_dev, chunk);
  const FramePlane plane = frame_plane(B);
  frames_in_chunks(
      &plane, 1, B.n_frames, in_dev, chunk,
      [&](const FramePlane* c, int64_t lo, int64_t m, hipStream_t st) {
        P.src = c->base; P.row_pitch = c->row_pitch; P.frame_pitch = c->frame_pitch;
        O.target(lo, P.out, P.out_row_pitch, P.out_frame_pitch);
        rs_launch(P, channels, gray, m, st);
      },
      [&](int64_t lo, int64_t m, hipStream_t st) { O.fetch(lo, m, st); });
  return SBA_OK;
}

}  // namespace sba_detect
