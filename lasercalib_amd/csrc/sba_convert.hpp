// sba_convert.hpp -- sba_convert_frames (include/sba_hip.h): 8-bit YUV 4:2:0 frames as a video decoder leaves them (NV12, NV21,
// I420, YV12: three plane pointers, a chroma step) into interleaved BGR / RGB / BGRA / RGBA or one of the planes B, G, R.  The
// rule per pixel -- nearest chroma, an integer matrix with 20 fraction bits, floor, clip -- is written out in the header and
// evaluated here by cv_chroma and cv_pixel in 32-bit integers (the header's bound on the matrix is what makes that exact).
//
// One kernel, k_convert<FMT>, a pure streaming kernel: 1.5 bytes read and 1, 3 or 4 written per pixel.  A lane owns a BLOCK of
// CV_RUN = 16 pixels in TWO rows, so that one load of 8 chroma samples serves all 32 pixels; block columns are counted from
// x = 0.  Half a wave (32 lanes) holds neighbouring blocks of one row pair, the other half the row pair below, a wave per two
// row pairs: a workgroup's tile is CV_WAVE_COLS x CV_TILE_ROWS pixels.  A full block reads its two luma rows as 16 bytes each,
// its chroma as 8 + 8 bytes (planar) or 16 bytes (interleaved UV / VU), and writes 16, 48 or 64 bytes per row, assembled in
// registers.  The planes and the output are aligned independently of each other, and packed rows of an odd or half-aligned
// width alternate between alignments, so every one of these accesses chooses its width by itself from its ADDRESS (cv_load16,
// cv_store16): one 16-byte access, two of 8, four of 4, or single bytes.  Blocks cut by the right edge (width % 16 pixels, the
// last of them alone on its chroma sample when the width is odd) and the last row of an odd height take the byte path, pixel
// by pixel (cv_edge).  Padding is never read or written.
// The host side stages host planes (YuvSource, sba_frames.hpp, which also holds the chroma modes CV_*) chunk by chunk through
// two device buffers and a host output through one more, in the order frames_in_chunks (sba_frames.hpp) documents.
#pragma once
#include "sba_frames.hpp"

namespace sba_detect {

constexpr int CV_RUN = 16;                                   // pixels of a row a lane owns (in each of its two rows)
constexpr int CV_HALF = 32;                                  // lanes side by side on one row pair
constexpr int CV_WAVE_COLS = CV_RUN * CV_HALF;               // pixels a wave spans
constexpr int CV_TILE_ROWS = DOT_WAVES * 2 * 2;              // rows of a workgroup: two row pairs per wave

struct CvParams {
  const uint8_t *y, *u, *v;                  // of the chunk's first frame; CV_UV / CV_VU: u is the lower of the two addresses
  int64_t y_row_pitch, y_frame_pitch, c_row_pitch, c_frame_pitch;
  uint8_t* out;
  int64_t out_row_pitch, out_frame_pitch;
  int32_t height, width, c_step, c_mode;
  int32_t y_offset, cy, cvr, cug, cvg, cub;
};

__device__ __forceinline__ uint32_t cv_byte(uint32_t w, int k) { return w >> 8 * k & 255u; }

// 16 bytes at any address, in the widest pieces the address allows
__device__ __forceinline__ uint4 cv_load16(const uint8_t* p) {
  const uint32_t a = (uint32_t)reinterpret_cast<uintptr_t>(p);
  uint4 r;
  if ((a & 15u) == 0) r = *reinterpret_cast<const uint4*>(p);
  else if ((a & 7u) == 0) {
    const uint2 lo = *reinterpret_cast<const uint2*>(p), hi = *reinterpret_cast<const uint2*>(p + 8);
    r = make_uint4(lo.x, lo.y, hi.x, hi.y);
  } else if ((a & 3u) == 0) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
    r = make_uint4(q[0], q[1], q[2], q[3]);
  } else {
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 | (uint32_t)p[4 * i + 3] << 24;
    r = make_uint4(w[0], w[1], w[2], w[3]);
  }
  return r;
}
__device__ __forceinline__ uint2 cv_load8(const uint8_t* p) {
  const uint32_t a = (uint32_t)reinterpret_cast<uintptr_t>(p);
  uint2 r;
  if ((a & 7u) == 0) r = *reinterpret_cast<const uint2*>(p);
  else if ((a & 3u) == 0) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
    r = make_uint2(q[0], q[1]);
  } else {
    uint32_t w[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) w[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 | (uint32_t)p[4 * i + 3] << 24;
    r = make_uint2(w[0], w[1]);
  }
  return r;
}
__device__ __forceinline__ void cv_store16(uint8_t* p, const uint4 v) {
  const uint32_t a = (uint32_t)reinterpret_cast<uintptr_t>(p);
  if ((a & 15u) == 0) *reinterpret_cast<uint4*>(p) = v;
  else if ((a & 7u) == 0) {
    *reinterpret_cast<uint2*>(p) = make_uint2(v.x, v.y);
    *reinterpret_cast<uint2*>(p + 8) = make_uint2(v.z, v.w);
  } else if ((a & 3u) == 0) {
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
    q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
  } else {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 16; ++i) p[i] = (uint8_t)cv_byte(w[i >> 2], i & 3);
  }
}

// The chroma part of the three sums of the header's rule, rounding term included; shared by the pixels of a chroma sample
__device__ __forceinline__ void cv_chroma(const CvParams& P, uint32_t U, uint32_t V, int& cr, int& cg, int& cb) {
  const int u = (int)U - 128, v = (int)V - 128;
  cr = P.cvr * v + (1 << 19);
  cg = P.cug * u + P.cvg * v + (1 << 19);
  cb = P.cub * u + (1 << 19);
}
// clip255(s >> 20), written as the clip of the SUM followed by the shift (s -> floor(s / 2^20) is monotone, so the two agree).
// In the order of the header -- shift, then clip -- the compiler fuses pairs of pixels into v_ashr_pk_u8_i32, and the bytes that
// came out of that on an MI355X were wrong; the kernel must not contain that instruction.
__device__ __forceinline__ uint32_t cv_clip(int s) { return (uint32_t)min(max(s, 0), (256 << 20) - 1) >> 20; }

// FMT is sba_pixel_format.  The C bytes of a pixel, the first in bit 0.
template <int FMT> struct CvFormat { static constexpr int C = FMT <= 1 ? 3 : FMT <= 3 ? 4 : 1; };
template <int FMT>
__device__ __forceinline__ uint32_t cv_pixel(const CvParams& P, uint32_t Y, int cr, int cg, int cb) {
  const int l = max((int)Y - P.y_offset, 0) * P.cy;
  if (FMT == 4) return cv_clip(l + cb);
  if (FMT == 5) return cv_clip(l + cg);
  if (FMT == 6) return cv_clip(l + cr);
  const uint32_t r = cv_clip(l + cr), g = cv_clip(l + cg), b = cv_clip(l + cb);
  const uint32_t bgr = (FMT == 0 || FMT == 2) ? (b | g << 8 | r << 16) : (r | g << 8 | b << 16);
  return CvFormat<FMT>::C == 4 ? bgr | 0xff000000u : bgr;
}

// The byte path: the nx x ny pixels (nx <= 16, ny <= 2) of a block that the frame's right or lower edge cuts
template <int FMT>
__device__ __forceinline__ void cv_edge(const CvParams& P, const uint8_t* yp, const uint8_t* up, const uint8_t* vp, uint8_t* op, int nx, int ny) {
  constexpr int C = CvFormat<FMT>::C;
  for (int k = 0; 2 * k < nx; ++k) {
    int cr, cg, cb;
    cv_chroma(P, up[(int64_t)k * P.c_step], vp[(int64_t)k * P.c_step], cr, cg, cb);
    for (int r = 0; r < ny; ++r)
      for (int x = 2 * k; x < min(2 * k + 2, nx); ++x) {
        const uint32_t px = cv_pixel<FMT>(P, yp[r * P.y_row_pitch + x], cr, cg, cb);
        uint8_t* o = op + r * P.out_row_pitch + x * C;
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = (uint8_t)cv_byte(px, c);
      }
  }
}

// grid (ceil(width / CV_WAVE_COLS), ceil(height / CV_TILE_ROWS), frames of the chunk), DOT_THREADS threads
template <int FMT>
__global__ void __launch_bounds__(DOT_THREADS) k_convert(const CvParams P) {
  constexpr int C = CvFormat<FMT>::C, NW = 4 * C;                         // 32-bit words of a block's row in the output
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = ((int)blockIdx.x * CV_HALF + (lane & (CV_HALF - 1))) * CV_RUN;
  const int y0 = (((int)blockIdx.y * DOT_WAVES + wave) * 2 + lane / CV_HALF) * 2;
  if (x0 >= P.width || y0 >= P.height) return;
  const int64_t f = blockIdx.z;
  const uint8_t* yp = P.y + (f * P.y_frame_pitch + (int64_t)y0 * P.y_row_pitch + x0);
  const int64_t coff = f * P.c_frame_pitch + (int64_t)(y0 >> 1) * P.c_row_pitch + (int64_t)(x0 >> 1) * P.c_step;
  uint8_t* op = P.out + (f * P.out_frame_pitch + (int64_t)y0 * P.out_row_pitch + (int64_t)x0 * C);
  const int nx = min(CV_RUN, P.width - x0), ny = min(2, P.height - y0);
  if (nx < CV_RUN || ny < 2) {
    // CV_UV / CV_VU keep the lower address in u: the caller's planes are one byte apart
    const uint8_t* up = P.u + coff + (P.c_mode == CV_VU ? 1 : 0);
    const uint8_t* vp = P.c_mode == CV_PLANAR || P.c_mode == CV_STEP2 ? P.v + coff : P.u + coff + (P.c_mode == CV_UV ? 1 : 0);
    cv_edge<FMT>(P, yp, up, vp, op, nx, ny);
    return;
  }

  // every load of the block is issued before the first is used
  const uint4 ya = cv_load16(yp), yb = cv_load16(yp + P.y_row_pitch);
  uint32_t U[2], V[2];
  if (P.c_mode == CV_PLANAR) {
    const uint2 a = cv_load8(P.u + coff), b = cv_load8(P.v + coff);
    U[0] = a.x; U[1] = a.y; V[0] = b.x; V[1] = b.y;
  } else if (P.c_mode == CV_STEP2) {
    U[0] = U[1] = V[0] = V[1] = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      U[k >> 2] |= (uint32_t)P.u[coff + 2 * k] << 8 * (k & 3);
      V[k >> 2] |= (uint32_t)P.v[coff + 2 * k] << 8 * (k & 3);
    }
  } else {
    const uint4 c = cv_load16(P.u + coff);                                // bytes 0, 2, 4, ... and 1, 3, 5, ...
    const uint32_t e0 = __builtin_amdgcn_perm(c.y, c.x, 0x06040200u), e1 = __builtin_amdgcn_perm(c.w, c.z, 0x06040200u);
    const uint32_t o0 = __builtin_amdgcn_perm(c.y, c.x, 0x07050301u), o1 = __builtin_amdgcn_perm(c.w, c.z, 0x07050301u);
    const bool uv = P.c_mode == CV_UV;
    U[0] = uv ? e0 : o0; U[1] = uv ? e1 : o1; V[0] = uv ? o0 : e0; V[1] = uv ? o1 : e1;
  }
  const uint32_t Y[2][4] = {{ya.x, ya.y, ya.z, ya.w}, {yb.x, yb.y, yb.z, yb.w}};

  uint32_t w[2][NW];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int i = 0; i < NW; ++i) w[r][i] = 0;
#pragma unroll
  for (int k = 0; k < CV_RUN / 2; ++k) {
    int cr, cg, cb;
    cv_chroma(P, cv_byte(U[k >> 2], k & 3), cv_byte(V[k >> 2], k & 3), cr, cg, cb);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int x = 2 * k; x < 2 * k + 2; ++x) {
        const uint32_t px = cv_pixel<FMT>(P, cv_byte(Y[r][x >> 2], x & 3), cr, cg, cb);
        const int bit = 8 * C * x, word = bit >> 5, sh = bit & 31;       // constants after unrolling
        w[r][word] |= px << sh;
        if (sh + 8 * C > 32) w[r][word + 1] |= px >> (32 - sh);
      }
  }
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int q = 0; q < C; ++q)
      cv_store16(op + r * P.out_row_pitch + 16 * q, make_uint4(w[r][4 * q], w[r][4 * q + 1], w[r][4 * q + 2], w[r][4 * q + 3]));
}

// ------------------------------------------------------------------------------------------------ host side
inline int cv_channels(int fmt) { return fmt <= SBA_PIX_RGB ? 3 : fmt <= SBA_PIX_RGBA ? 4 : 1; }

inline void cv_launch(const CvParams& P, int fmt, int64_t nf, hipStream_t st) {
  const dim3 grid((unsigned)((P.width + CV_WAVE_COLS - 1) / CV_WAVE_COLS), (unsigned)((P.height + CV_TILE_ROWS - 1) / CV_TILE_ROWS), (unsigned)nf);
  const dim3 block(DOT_THREADS);
  switch (fmt) {
    case SBA_PIX_BGR: hipLaunchKernelGGL(k_convert<SBA_PIX_BGR>, grid, block, 0, st, P); break;
    case SBA_PIX_RGB: hipLaunchKernelGGL(k_convert<SBA_PIX_RGB>, grid, block, 0, st, P); break;
    case SBA_PIX_BGRA: hipLaunchKernelGGL(k_convert<SBA_PIX_BGRA>, grid, block, 0, st, P); break;
    case SBA_PIX_RGBA: hipLaunchKernelGGL(k_convert<SBA_PIX_RGBA>, grid, block, 0, st, P); break;
    case SBA_PIX_B: hipLaunchKernelGGL(k_convert<SBA_PIX_B>, grid, block, 0, st, P); break;
    case SBA_PIX_G: hipLaunchKernelGGL(k_convert<SBA_PIX_G>, grid, block, 0, st, P); break;
    default: hipLaunchKernelGGL(k_convert<SBA_PIX_R>, grid, block, 0, st, P); break;
  }
  HIPCHK(hipGetLastError());
}

// Arguments are checked by the caller (sba_api.hip).  Chunks, staging and output are those of sba_frames.hpp (chunk_of by
// CHUNK_FRAMES, frames_in_chunks over the planes of a YuvSource, FrameOutput).  Which chunk or buffer a frame passes through
// does not enter its arithmetic.
int convert_call(int device, const sba_yuv_planes& src, int64_t n_frames, int32_t height, int32_t width, const sba_yuv_matrix& M,
                 const FrameOut& out, const sba_convert_opts& o) {
  if (n_frames == 0 || height == 0 || width == 0) return SBA_OK;
  HIPCHK(hipSetDevice(device));
  const bool in_dev = o.frames_on_device != 0, out_dev = o.out_on_device != 0;
  const YuvSource S(src, height, width);
  CvParams P{};
  P.height = height; P.width = width; P.c_step = src.c_step; P.c_mode = S.mode;
  P.y_offset = M.y_offset; P.cy = M.cy; P.cvr = M.cvr; P.cug = M.cug; P.cvg = M.cvg; P.cub = M.cub;

  const int64_t out_row = (int64_t)width * cv_channels(o.out_format);
  const int64_t chunk = chunk_of(CHUNK_FRAMES, o.chunk_frames, n_frames, S.tight, in_dev, out_row * height, out_dev);
  FrameOutput O(out, out_row, height, out_dev, chunk);
  frames_in_chunks(
      S.planes, S.n_planes, n_frames, in_dev, chunk,
      [&](const FramePlane* c, int64_t lo, int64_t m, hipStream_t st) {
        S.chunk(c, P.y, P.u, P.v, P.y_row_pitch, P.y_frame_pitch, P.c_row_pitch, P.c_frame_pitch);
        O.target(lo, P.out, P.out_row_pitch, P.out_frame_pitch);
        cv_launch(P, o.out_format, m, st);
      },
      [&](int64_t lo, int64_t m, hipStream_t st) { O.fetch(lo, m, st); });
  return SBA_OK;
}

}  // namespace sba_detect
