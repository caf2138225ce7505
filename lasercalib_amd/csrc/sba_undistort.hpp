// sba_undistort.hpp -- sba_undistort_frames (include/sba_hip.h): takes the lens out of a batch of video frames.  Stands in for
// cv.undistort as scripts/charuco_intrinsics.py:163-184 of the reference calls it; the rule per destination pixel -- float64
// model, 1/32-pixel source grid, integer bilinear weights, the three flags -- is written out in the header and evaluated here by
// ud_pixel, one IEEE operation per operation of the rule (no contraction).
//
// Two kernels.  k_undistort_geometry writes flags and map of every destination pixel (diagnostics, once per call).
// k_undistort<C> resamples: a workgroup owns a tile of UD_TILE_ROWS x UD_TILE_COLS destination pixels, a wave a row of it, a
// lane the pixels x0 + lane + 64 j.  The model is evaluated ONCE per pixel, into three registers (byte offset of the first tap,
// weights and which taps are read), and the workgroup then walks the frames of its share of the chunk: the float64 arithmetic is
// amortised over the batch and no map is ever stored.  Neighbouring lanes are neighbouring destination pixels, so their taps
// fall into neighbouring source bytes; a tap row is one read of 2 C bytes at a clamped position, with no branch around it, so
// that the eight reads of a lane's pixels are in flight together (under branches each was waited for by itself, and a frame
// took 1.6 to 2 times as long).  A row of results goes through LDS, placed at the alignment of its destination address, and
// leaves as 16-byte stores, with single bytes only in
// front of the first and behind the last 16-byte boundary of the ADDRESS: bases and pitches may be anything, padding is never
// written.  Nearest-neighbour is the same kernel with the position snapped to whole pixels (weight 1024 on one tap).
// How frames are described and staged chunk by chunk is sba_frames.hpp, shared with the detectors.
#pragma once
#include "sba_frames.hpp"

namespace sba_detect {

constexpr int UD_TILE_ROWS = DOT_WAVES, UD_TILE_COLS = 256, UD_PX = UD_TILE_COLS / 64;   // a wave per row, UD_PX pixels per lane
constexpr int UD_ROW_LDS = 16 + UD_TILE_COLS * 4;            // a row of results behind up to 15 bytes of misalignment
constexpr int UD_OUTSIDE = 1, UD_FOLDED = 2, UD_RANGE = 4;

struct UdParams {
  FrameView src;
  double fx, fy, cx, cy, k1, k2, p1, p2, k3;
  double ifx, ify, cxn, cyn;                 // 1 / fxn and 1 / fyn are formed once on the host
  uint8_t* out;
  int64_t out_row_pitch, out_frame_pitch;
  int32_t out_height, out_width, nearest, border;
  int32_t frames_per_group;                  // frames one workgroup walks: grid.z groups share a chunk
};

// The rule of include/sba_hip.h from "x2 = xn*xn" on, at the normalised position (xn, yn): the source position on the 1/32-pixel
// grid ((0, 0) when it is not in range) and the FOLDED and RANGE flags.  `front` is false where a projective front end
// (sba_warp.hpp) found the pixel behind the camera: it is then not in range whatever the lens says.
__device__ __forceinline__ void ud_lens(const UdParams& P, double xn, double yn, bool front, int& qx, int& qy, int& flags) {
#pragma clang fp contract(off)
  const double x2 = xn * xn, y2 = yn * yn, r2 = x2 + y2, xy = xn * yn;
  double t = r2 * P.k3; t = P.k2 + t; t = r2 * t; t = P.k1 + t; t = r2 * t;
  const double rad = 1.0 + t;
  const double xd = xn * rad + ((2.0 * P.p1) * xy + P.p2 * (r2 + 2.0 * x2));
  const double yd = yn * rad + (P.p1 * (r2 + 2.0 * y2) + (2.0 * P.p2) * xy);
  const double sx = P.fx * xd + P.cx, sy = P.fy * yd + P.cy;
  const bool in_range = front && sx > -32768.0 && sx < 32768.0 && sy > -32768.0 && sy < 32768.0;
  qx = in_range ? (int)floor(sx * 32.0 + 0.5) : 0;
  qy = in_range ? (int)floor(sy * 32.0 + 0.5) : 0;
  double dp = r2 * (3.0 * P.k3); dp = (2.0 * P.k2) + dp; dp = r2 * dp; dp = P.k1 + dp;
  const double j00 = rad + (2.0 * x2) * dp + ((2.0 * P.p1) * yn + (6.0 * P.p2) * xn);
  const double j11 = rad + (2.0 * y2) * dp + ((6.0 * P.p1) * yn + (2.0 * P.p2) * xn);
  const double j01 = (2.0 * xy) * dp + ((2.0 * P.p1) * xn + (2.0 * P.p2) * yn);
  const double det = j00 * j11 - j01 * j01;
  flags = (det > 0.0 ? 0 : UD_FOLDED) | (in_range ? 0 : UD_RANGE);
}

// The rule of sba_undistort_frames for destination pixel (x, y): the pinhole front end, then the lens
__device__ __forceinline__ void ud_pixel(const UdParams& P, int x, int y, int& qx, int& qy, int& flags) {
#pragma clang fp contract(off)
  const double xn = ((double)x - P.cxn) * P.ifx, yn = ((double)y - P.cyn) * P.ify;
  ud_lens(P, xn, yn, true, qx, qy, flags);
}

// The two kernels below are templates over the parameter block of a call: what differs between the calls that resample through
// a lens is the front end alone, the function model_pixel(Params, x, y, qx, qy, flags) found by the type of the block, and
// ud_base(Params) is the UdParams inside it.  sba_undistort_frames: UdParams itself and ud_pixel.
__host__ __device__ __forceinline__ const UdParams& ud_base(const UdParams& P) { return P; }
__host__ __device__ __forceinline__ UdParams& ud_base(UdParams& P) { return P; }
__device__ __forceinline__ void model_pixel(const UdParams& P, int x, int y, int& qx, int& qy, int& flags) { ud_pixel(P, x, y, qx, qy, flags); }

// What the resampling keeps of a pixel: a byte offset `off` into a frame of C channels and
//   tap = ax | ay << 5 | read << 10 | outside << 14 | left_second << 15 | right_first << 16 | row_step << 17
// Bit k of `read` (taps in the order (ix, iy) (ix+1, iy) (ix, iy+1) (ix+1, iy+1)): the tap has a non-zero weight and lies inside
// the source; `outside`: a tap with a non-zero weight does not, or the position is not in range.  Nearest-neighbour snaps the
// position to whole pixels first: ax = ay = 0 leaves its single tap with weight 32 * 32.
// A source of at least 2 x 1 pixels is read WITHOUT a branch (ud_clamped): `off` is pixel (clamp(ix, 0, W - 2), clamp(iy, 0,
// H - 1)), where the two pixels of a tap row can always be read together; the second tap row lies row_step rows below.  A tap
// that is read is then one of the two pixels loaded: the left tap the second one when ix = W - 1 (left_second), the right tap
// the first one when ix = -1 (right_first).  A smaller source is read tap by tap under its read bits; `off` is pixel (ix, iy).
__device__ __forceinline__ bool ud_clamped(const UdParams& P) { return P.src.width >= 2 && P.src.height >= 1; }
__device__ __forceinline__ void ud_taps(const UdParams& P, int C, int qx, int qy, bool in_range, int64_t& off, uint32_t& tap) {
  if (P.nearest) { qx = ((qx + 16) >> 5) << 5; qy = ((qy + 16) >> 5) << 5; }
  const int ix = qx >> 5, iy = qy >> 5, ax = qx & 31, ay = qy & 31;
  const int W = P.src.width, H = P.src.height;
  const bool x0 = ix >= 0 && ix < W, x1 = ix + 1 >= 0 && ix + 1 < W;
  const bool y0 = iy >= 0 && iy < H, y1 = iy + 1 >= 0 && iy + 1 < H;
  const uint32_t inside = (uint32_t)(x0 && y0) | (uint32_t)(x1 && y0) << 1 | (uint32_t)(x0 && y1) << 2 | (uint32_t)(x1 && y1) << 3;
  const uint32_t weighted = 1u | (ax != 0 ? 2u : 0u) | (ay != 0 ? 4u : 0u) | (ax != 0 && ay != 0 ? 8u : 0u);
  const uint32_t read = in_range ? inside & weighted : 0u;
  tap = (uint32_t)ax | (uint32_t)ay << 5 | read << 10 | (read != weighted ? 1u << 14 : 0u);
  if (ud_clamped(P)) {
    const int cx = min(max(ix, 0), W - 2), cy = min(max(iy, 0), H - 1), cy1 = min(max(iy + 1, 0), H - 1);
    off = (int64_t)cy * P.src.row_pitch + (int64_t)cx * C;
    tap |= (ix - cx == 1 ? 1u << 15 : 0u) | (ix + 1 == cx ? 1u << 16 : 0u) | (cy1 != cy ? 1u << 17 : 0u);
  } else {
    off = (int64_t)iy * P.src.row_pitch + (int64_t)ix * C;
  }
}

// grid over the destination pixels, one thread each; flags and map are packed rows of out_width
template <class Params>
__global__ void __launch_bounds__(256) k_undistort_geometry(const Params M, int channels, uint8_t* __restrict__ flags, int2* __restrict__ map) {
  const UdParams& P = ud_base(M);
  const int n = P.out_height * P.out_width;                               // <= 16384^2
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int y = i / P.out_width, x = i - y * P.out_width;
  int qx, qy, fl;
  int64_t off;
  uint32_t tap;
  model_pixel(M, x, y, qx, qy, fl);
  ud_taps(P, channels, qx, qy, !(fl & UD_RANGE), off, tap);
  if (flags) flags[i] = (uint8_t)(fl | (tap >> 14 & 1u ? UD_OUTSIDE : 0));
  if (map) map[i] = make_int2(qx, qy);
}

// One pixel / two neighbouring pixels of C bytes at any address, channels packed from bit 0
template <int C>
__device__ __forceinline__ uint32_t ud_load(const uint8_t* p) {
  uint32_t v = 0;
  __builtin_memcpy(&v, p, C);
  return v;
}
template <int C>
__device__ __forceinline__ void ud_load2(const uint8_t* p, uint32_t& a, uint32_t& b) {
  unsigned long long v = 0;
  __builtin_memcpy(&v, p, 2 * C);
  a = (uint32_t)v & (uint32_t)((1ull << 8 * C) - 1);
  b = (uint32_t)(v >> 8 * C) & (uint32_t)((1ull << 8 * C) - 1);
}

// grid (tiles in x, tiles in y, frame groups), DOT_THREADS threads; P.src.frames and P.out point at the chunk's first frame
template <int C, class Params>
__global__ void __launch_bounds__(DOT_THREADS) k_undistort(const Params M, int n_frames) {
  const UdParams& P = ud_base(M);
  __shared__ __attribute__((aligned(16))) uint8_t s_row[2][UD_TILE_ROWS][UD_ROW_LDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int y = (int)blockIdx.y * UD_TILE_ROWS + wave, x0 = (int)blockIdx.x * UD_TILE_COLS;
  const bool row_on = y < P.out_height;

  int64_t off[UD_PX];
  uint32_t tap[UD_PX];
#pragma unroll
  for (int j = 0; j < UD_PX; ++j) {
    const int x = x0 + lane + 64 * j;
    off[j] = 0; tap[j] = 0;                                               // a pixel beyond the image reads nothing
    if (row_on && x < P.out_width) {
      int qx, qy, fl;
      model_pixel(M, x, y, qx, qy, fl);
      ud_taps(P, C, qx, qy, !(fl & UD_RANGE), off[j], tap[j]);
    }
  }
  const int nb = row_on ? min(UD_TILE_COLS, P.out_width - x0) * C : 0;   // bytes of this wave's row
  const uint32_t bv = (uint32_t)P.border * 0x01010101u;
  const bool clamped = ud_clamped(P);
  const int f_lo = (int)blockIdx.z * P.frames_per_group, f_hi = min(n_frames, f_lo + P.frames_per_group);

  for (int f = f_lo; f < f_hi; ++f) {                                     // the same trip count in every wave of the workgroup
    const uint8_t* __restrict__ fp = P.src.frames + (int64_t)f * P.src.frame_pitch;
    uint32_t t[UD_PX][4];
    if (clamped) {                                                        // every load is issued before the first is waited for
#pragma unroll
      for (int j = 0; j < UD_PX; ++j) {
        const uint8_t* p = fp + off[j];
        ud_load2<C>(p, t[j][0], t[j][1]);
        ud_load2<C>(p + (tap[j] >> 17 & 1u ? P.src.row_pitch : 0), t[j][2], t[j][3]);
      }
#pragma unroll
      for (int j = 0; j < UD_PX; ++j) {
        const uint32_t k = tap[j];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const uint32_t a = t[j][2 * r], b = t[j][2 * r + 1];
          t[j][2 * r] = k >> (10 + 2 * r) & 1u ? (k >> 15 & 1u ? b : a) : bv;
          t[j][2 * r + 1] = k >> (11 + 2 * r) & 1u ? (k >> 16 & 1u ? a : b) : bv;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < UD_PX; ++j) {
        const uint32_t rd = tap[j] >> 10 & 15u;
        const uint8_t* p = fp + off[j];
        t[j][0] = t[j][1] = t[j][2] = t[j][3] = bv;
#pragma unroll
        for (int r = 0; r < 2; ++r, p += P.src.row_pitch) {
          if (rd >> 2 * r & 1u) t[j][2 * r] = ud_load<C>(p);
          if (rd >> 2 * r & 2u) t[j][2 * r + 1] = ud_load<C>(p + C);
        }
      }
    }
    uint8_t* dst = P.out + ((int64_t)f * P.out_frame_pitch + (int64_t)y * P.out_row_pitch + (int64_t)x0 * C);
    const int a = (int)(reinterpret_cast<uintptr_t>(dst) & 15u);          // the LDS row lies as the destination does, modulo 16
    uint8_t* srow = s_row[(f - f_lo) & 1][wave];
#pragma unroll
    for (int j = 0; j < UD_PX; ++j) {
      const uint32_t ax = tap[j] & 31u, ay = tap[j] >> 5 & 31u;
      const uint32_t w00 = (32u - ax) * (32u - ay), w10 = ax * (32u - ay), w01 = (32u - ax) * ay, w11 = ax * ay;
      uint32_t v = 0;
#pragma unroll
      for (int c = 0; c < C; ++c)
        v |= ((w00 * (t[j][0] >> 8 * c & 255u) + w10 * (t[j][1] >> 8 * c & 255u) + w01 * (t[j][2] >> 8 * c & 255u) +
               w11 * (t[j][3] >> 8 * c & 255u) + 512u) >> 10) << 8 * c;
      __builtin_memcpy(srow + a + (lane + 64 * j) * C, &v, C);
    }
    // The buffer of this frame's parity was last read two frames ago, in front of the barrier of the frame between.
    __syncthreads();
    const int head = min(nb, (16 - a) & 15), nv = (nb - head) >> 4, tail = head + nv * 16;   // nv <= 64: a vector per lane
    if (lane < nv) *reinterpret_cast<uint4*>(dst + head + 16 * lane) = *reinterpret_cast<const uint4*>(srow + a + head + 16 * lane);
    const int b = lane < 32 ? lane : tail + (lane - 32);                  // lanes 0..14: in front of the vectors; 32..46: behind
    if (b < (lane < 32 ? head : nb)) dst[b] = srow[a + b];
  }
}

// ------------------------------------------------------------------------------------------------ host side
template <class Params>
inline void ud_launch(const Params& M, int channels, int64_t nf, hipStream_t st) {
  const UdParams& P = ud_base(M);
  const unsigned gx = (unsigned)((P.out_width + UD_TILE_COLS - 1) / UD_TILE_COLS), gy = (unsigned)((P.out_height + UD_TILE_ROWS - 1) / UD_TILE_ROWS);
  // about 2048 workgroups where the frames allow it; which workgroup takes a frame does not change its bytes
  const int64_t groups = std::max<int64_t>(1, std::min<int64_t>(nf, 2048 / ((int64_t)gx * gy)));
  Params Q = M;
  const int32_t fpg = ud_base(Q).frames_per_group = (int32_t)((nf + groups - 1) / groups);
  const dim3 grid(gx, gy, (unsigned)((nf + fpg - 1) / fpg));
  if (channels == 1) hipLaunchKernelGGL((k_undistort<1, Params>), grid, dim3(DOT_THREADS), 0, st, Q, (int)nf);
  else if (channels == 3) hipLaunchKernelGGL((k_undistort<3, Params>), grid, dim3(DOT_THREADS), 0, st, Q, (int)nf);
  else hipLaunchKernelGGL((k_undistort<4, Params>), grid, dim3(DOT_THREADS), 0, st, Q, (int)nf);
  HIPCHK(hipGetLastError());
}

// The lens and the new camera matrix of a call; 1 / fxn and 1 / fyn are formed here, once
inline void ud_set_lens(UdParams& P, const sba_lens& L, const double* new_k) {
  P.fx = L.fx; P.fy = L.fy; P.cx = L.cx; P.cy = L.cy; P.k1 = L.k1; P.k2 = L.k2; P.p1 = L.p1; P.p2 = L.p2; P.k3 = L.k3;
  P.ifx = 1.0 / new_k[0]; P.ify = 1.0 / new_k[1]; P.cxn = new_k[2]; P.cyn = new_k[3];
}

// The diagnostics of a call, once: flags and map of every destination pixel of P into host memory (either may be NULL)
template <class Params>
inline void ud_geometry_out(const Params& M, int channels, uint8_t* flags_out, int32_t* map_out) {
  if (!flags_out && !map_out) return;
  const UdParams& P = ud_base(M);
  const int64_t out_px = (int64_t)P.out_height * P.out_width;
  DotStream s;
  DevBuf<uint8_t> d_flags;
  DevBuf<int2> d_map;
  if (flags_out) d_flags.alloc((size_t)out_px);
  if (map_out) d_map.alloc((size_t)out_px);
  hipLaunchKernelGGL(k_undistort_geometry<Params>, dim3((unsigned)((out_px + 255) / 256)), dim3(256), 0, s.s, M, channels, d_flags.p, d_map.p);
  HIPCHK(hipGetLastError());
  if (flags_out) HIPCHK(hipMemcpyAsync(flags_out, d_flags.p, (size_t)out_px, hipMemcpyDeviceToHost, s.s));
  if (map_out) HIPCHK(hipMemcpyAsync(map_out, d_map.p, sizeof(int2) * (size_t)out_px, hipMemcpyDeviceToHost, s.s));
  HIPCHK(hipStreamSynchronize(s.s));
}

// Arguments are checked by the caller (sba_api.hip).  Chunks, staging and output are those of sba_frames.hpp (chunk_of by
// CHUNK_FRAMES, frames_in_chunks, FrameOutput).  Which chunk, workgroup or buffer a frame passes through does not enter its
// arithmetic: any chunk_frames gives the same bytes.
// `M` holds the model of the call (lens and front end); source (B), output (out) and options are filled in here.
template <class Params>
inline int ud_call(Params& M, const FrameBatch& B, int32_t out_height, int32_t out_width, const FrameOut& out, const sba_undistort_opts& o,
                   uint8_t* flags_out, int32_t* map_out) {
  const int32_t channels = B.channels;
  const int64_t out_px = (int64_t)out_height * out_width;
  if (out_px == 0) return SBA_OK;
  HIPCHK(hipSetDevice(B.device));
  UdParams& P = ud_base(M);
  P.src = frame_view(B, 0, 0);
  P.out_height = out_height; P.out_width = out_width; P.nearest = o.interpolation == 1; P.border = o.border_value;
  ud_geometry_out(M, channels, flags_out, map_out);
  if (B.n_frames == 0 || !out.out) return SBA_OK;

  const bool in_dev = o.frames_on_device != 0, out_dev = o.out_on_device != 0;
  const int64_t out_row = (int64_t)out_width * channels;
  const int64_t chunk = chunk_of(CHUNK_FRAMES, o.chunk_frames, B, in_dev, out_row * out_height, out_dev);
  FrameOutput O(out, out_row, out_height, out_dev, chunk);
  frames_in_chunks(
      P.src, channels, B.n_frames, in_dev, chunk,
      [&](const FrameView& V, int64_t lo, int64_t m, hipStream_t st) {
        P.src = V;
        O.target(lo, P.out, P.out_row_pitch, P.out_frame_pitch);
        ud_launch(M, channels, m, st);
      },
      [&](int64_t lo, int64_t m, hipStream_t st) { O.fetch(lo, m, st); });
  return SBA_OK;
}

int undistort_call(const FrameBatch& B, const sba_lens& L, const double* new_k, int32_t out_height, int32_t out_width, const FrameOut& out,
                   const sba_undistort_opts& o, uint8_t* flags_out, int32_t* map_out) {
  UdParams P{};
  ud_set_lens(P, L, new_k);
  return ud_call(P, B, out_height, out_width, out, o, flags_out, map_out);
}

}  // namespace sba_detect
