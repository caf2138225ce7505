// sba_yuv.hpp -- sba_frames_to_yuv (include/sba_hip.h): interleaved BGR / RGB / BGRA / RGBA frames or one plane into 8-bit
// YUV 4:2:0 as an encoder takes it (NV12, NV21, I420, YV12: three plane pointers, a chroma step) -- the way back of
// sba_convert.hpp, with the destination described as that file's source.  The rule per pixel and per chroma sample -- an
// integer matrix with 20 fraction bits, floor, clip; chroma from the block's top-left pixel or from the sum of its four -- is
// written out in the header and evaluated here in 32-bit integers (the header's bound on the matrix is what makes that exact).
//
// One kernel, k_to_yuv<IN, CHROMA>, a pure streaming kernel: 1, 3 or 4 bytes read and 1.5 written per pixel.  Its geometry is
// k_convert's: a lane owns a BLOCK of CV_RUN = 16 pixels in TWO rows, half a wave holds neighbouring blocks of one row pair,
// the other half the pair below.  A full block reads its two rows as 16, 48 or 64 bytes each, forms 32 Y, 8 U and 8 V in
// registers and writes 16 bytes of luma per row and 8 + 8 bytes of chroma (planar) or 16 bytes (interleaved UV / VU).  Source,
// luma and chroma are aligned independently, so every one of these accesses chooses its width from its ADDRESS (cv_load16,
// cv_store16 of sba_convert.hpp, ty_store8 here).  Blocks cut by the right edge and the last row of an odd height take the
// byte path (ty_edge).  Padding -- and with c_step = 2 the byte between two samples of a plane of its own -- is never written.
// The host side stages host frames chunk by chunk through two device buffers and host planes through one packed buffer each
// (YuvOutput, sba_frames.hpp), in the order frames_in_chunks (sba_frames.hpp) documents.
#pragma once
#include "sba_convert.hpp"

namespace sba_detect {

enum { TY_BGR = 0, TY_RGB = 1, TY_BGRA = 2, TY_RGBA = 3, TY_GRAY = 4 };    // IN: sba_pixel_format, or the single plane

struct TyParams {
  const uint8_t* src;                        // of the chunk's first frame
  int64_t row_pitch, frame_pitch;
  uint8_t *y, *u, *v;                        // CV_UV / CV_VU: u is the lower of the two addresses, v is not used
  int64_t y_row_pitch, y_frame_pitch, c_row_pitch, c_frame_pitch;
  int32_t height, width, c_step, c_mode;
  int32_t yc;                                // 2^19 + (y_offset << 20)
  int32_t cry, cgy, cby, cru, cgu, cbu, crv, cgv, cbv;
};

template <int IN> struct TyFormat {
  static constexpr int C = IN == TY_GRAY ? 1 : IN <= TY_RGB ? 3 : 4;
  static constexpr bool RED_FIRST = IN == TY_RGB || IN == TY_RGBA;
};

// clip255(s >> SH) as the clip of the SUM followed by the shift, for the reason given at cv_clip (sba_convert.hpp)
template <int SH>
__device__ __forceinline__ uint32_t ty_clip(int s) { return (uint32_t)min(max(s, 0), (256 << SH) - 1) >> SH; }

// R, G, B of pixel x of a block's row held in the words w (x a constant after unrolling)
template <int IN>
__device__ __forceinline__ void ty_rgb(const uint32_t* w, int x, int& r, int& g, int& b) {
  constexpr int C = TyFormat<IN>::C;
  const int c0 = (int)cv_byte(w[(x * C) >> 2], (x * C) & 3);
  if (C == 1) { r = g = b = c0; return; }
  const int c1 = (int)cv_byte(w[(x * C + 1) >> 2], (x * C + 1) & 3), c2 = (int)cv_byte(w[(x * C + 2) >> 2], (x * C + 2) & 3);
  g = c1;
  r = TyFormat<IN>::RED_FIRST ? c0 : c2;
  b = TyFormat<IN>::RED_FIRST ? c2 : c0;
}
// the same of the pixel at p, byte by byte
template <int IN>
__device__ __forceinline__ void ty_rgb_at(const uint8_t* p, int& r, int& g, int& b) {
  if (TyFormat<IN>::C == 1) { r = g = b = p[0]; return; }
  g = p[1];
  r = TyFormat<IN>::RED_FIRST ? p[0] : p[2];
  b = TyFormat<IN>::RED_FIRST ? p[2] : p[0];
}

__device__ __forceinline__ uint32_t ty_luma(const TyParams& P, int r, int g, int b) { return ty_clip<20>(P.cry * r + P.cgy * g + P.cby * b + P.yc); }
// U and V of a chroma sample from R', G', B' (CHROMA 0: a pixel's bytes, 20 fraction bits) or from the sums over the four
// positions (CHROMA 1: 22 bits, one rounding)
template <int CHROMA>
__device__ __forceinline__ void ty_chroma(const TyParams& P, int r, int g, int b, uint32_t& U, uint32_t& V) {
  constexpr int SH = CHROMA ? 22 : 20;
  constexpr int cc = (1 << (SH - 1)) + (128 << SH);
  U = ty_clip<SH>(P.cru * r + P.cgu * g + P.cbu * b + cc);
  V = ty_clip<SH>(P.crv * r + P.cgv * g + P.cbv * b + cc);
}

// 8 bytes at any address, in the widest pieces the address allows
__device__ __forceinline__ void ty_store8(uint8_t* p, const uint2 v) {
  const uint32_t a = (uint32_t)reinterpret_cast<uintptr_t>(p);
  if ((a & 7u) == 0) *reinterpret_cast<uint2*>(p) = v;
  else if ((a & 3u) == 0) {
    uint32_t* q = reinterpret_cast<uint32_t*>(p);
    q[0] = v.x; q[1] = v.y;
  } else {
    const uint32_t w[2] = {v.x, v.y};
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = (uint8_t)cv_byte(w[i >> 2], i & 3);
  }
}

// The byte path: the nx x ny pixels (nx <= 16, ny <= 2) of a block that the frame's right or lower edge cuts.  A block with
// nx < 16 ends at the frame's last column and one with ny < 2 at its last row, so the header's min(.., W - 1) and
// min(.., H - 1) are min(.., nx - 1) and min(.., ny - 1) here.
template <int IN, int CHROMA>
__device__ __forceinline__ void ty_edge(const TyParams& P, const uint8_t* sp, uint8_t* yp, uint8_t* up, uint8_t* vp, int nx, int ny) {
  constexpr int C = TyFormat<IN>::C;
  for (int r = 0; r < ny; ++r)
    for (int x = 0; x < nx; ++x) {
      int R, G, B;
      ty_rgb_at<IN>(sp + r * P.row_pitch + x * C, R, G, B);
      yp[r * P.y_row_pitch + x] = (uint8_t)ty_luma(P, R, G, B);
    }
  for (int k = 0; 2 * k < nx; ++k) {
    int R = 0, G = 0, B = 0;
    if (CHROMA == 0) ty_rgb_at<IN>(sp + 2 * k * C, R, G, B);
    else
      for (int b = 0; b < 2; ++b)
        for (int a = 0; a < 2; ++a) {
          int r1, g1, b1;
          ty_rgb_at<IN>(sp + min(b, ny - 1) * P.row_pitch + min(2 * k + a, nx - 1) * C, r1, g1, b1);
          R += r1; G += g1; B += b1;
        }
    uint32_t U, V;
    ty_chroma<CHROMA>(P, R, G, B, U, V);
    up[(int64_t)k * P.c_step] = (uint8_t)U;
    vp[(int64_t)k * P.c_step] = (uint8_t)V;
  }
}

// grid (ceil(width / CV_WAVE_COLS), ceil(height / CV_TILE_ROWS), frames of the chunk), DOT_THREADS threads
template <int IN, int CHROMA>
__global__ void __launch_bounds__(DOT_THREADS) k_to_yuv(const TyParams P) {
  constexpr int C = TyFormat<IN>::C, NW = 4 * C;                          // 32-bit words of a block's row in the source
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = ((int)blockIdx.x * CV_HALF + (lane & (CV_HALF - 1))) * CV_RUN;
  const int y0 = (((int)blockIdx.y * DOT_WAVES + wave) * 2 + lane / CV_HALF) * 2;
  if (x0 >= P.width || y0 >= P.height) return;
  const int64_t f = blockIdx.z;
  const uint8_t* sp = P.src + (f * P.frame_pitch + (int64_t)y0 * P.row_pitch + (int64_t)x0 * C);
  uint8_t* yp = P.y + (f * P.y_frame_pitch + (int64_t)y0 * P.y_row_pitch + x0);
  const int64_t coff = f * P.c_frame_pitch + (int64_t)(y0 >> 1) * P.c_row_pitch + (int64_t)(x0 >> 1) * P.c_step;
  const int nx = min(CV_RUN, P.width - x0), ny = min(2, P.height - y0);
  if (nx < CV_RUN || ny < 2) {
    // CV_UV / CV_VU keep the lower address in u: the caller's planes are one byte apart
    uint8_t* up = P.u + coff + (P.c_mode == CV_VU ? 1 : 0);
    uint8_t* vp = P.c_mode == CV_PLANAR || P.c_mode == CV_STEP2 ? P.v + coff : P.u + coff + (P.c_mode == CV_UV ? 1 : 0);
    ty_edge<IN, CHROMA>(P, sp, yp, up, vp, nx, ny);
    return;
  }

  // every load of the block is issued before the first is used
  uint32_t w[2][NW];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int q = 0; q < C; ++q) {
      const uint4 t = cv_load16(sp + r * P.row_pitch + 16 * q);
      w[r][4 * q] = t.x; w[r][4 * q + 1] = t.y; w[r][4 * q + 2] = t.z; w[r][4 * q + 3] = t.w;
    }

  uint32_t Y[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}}, U[2] = {0u, 0u}, V[2] = {0u, 0u};
#pragma unroll
  for (int k = 0; k < CV_RUN / 2; ++k) {
    int sr = 0, sg = 0, sb = 0;                                           // R', G', B' of the block's chroma sample
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int x = 2 * k; x < 2 * k + 2; ++x) {
        int R, G, B;
        ty_rgb<IN>(w[r], x, R, G, B);
        Y[r][x >> 2] |= ty_luma(P, R, G, B) << 8 * (x & 3);
        if (CHROMA == 1 || (r == 0 && x == 2 * k)) { sr += R; sg += G; sb += B; }
      }
    uint32_t u1, v1;
    ty_chroma<CHROMA>(P, sr, sg, sb, u1, v1);
    U[k >> 2] |= u1 << 8 * (k & 3);
    V[k >> 2] |= v1 << 8 * (k & 3);
  }

#pragma unroll
  for (int r = 0; r < 2; ++r) cv_store16(yp + r * P.y_row_pitch, make_uint4(Y[r][0], Y[r][1], Y[r][2], Y[r][3]));
  if (P.c_mode == CV_PLANAR) {
    ty_store8(P.u + coff, make_uint2(U[0], U[1]));
    ty_store8(P.v + coff, make_uint2(V[0], V[1]));
  } else if (P.c_mode == CV_STEP2) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      P.u[coff + 2 * k] = (uint8_t)cv_byte(U[k >> 2], k & 3);
      P.v[coff + 2 * k] = (uint8_t)cv_byte(V[k >> 2], k & 3);
    }
  } else {
    const bool uv = P.c_mode == CV_UV;                                    // e: the bytes at the even addresses, o: at the odd ones
    const uint32_t e0 = uv ? U[0] : V[0], e1 = uv ? U[1] : V[1], o0 = uv ? V[0] : U[0], o1 = uv ? V[1] : U[1];
    cv_store16(P.u + coff, make_uint4(__builtin_amdgcn_perm(o0, e0, 0x05010400u), __builtin_amdgcn_perm(o0, e0, 0x07030602u),
                                      __builtin_amdgcn_perm(o1, e1, 0x05010400u), __builtin_amdgcn_perm(o1, e1, 0x07030602u)));
  }
}

// ------------------------------------------------------------------------------------------------ host side
template <int IN>
inline void ty_launch_in(const TyParams& P, int chroma, const dim3 grid, const dim3 block, hipStream_t st) {
  if (chroma) hipLaunchKernelGGL((k_to_yuv<IN, 1>), grid, block, 0, st, P);
  else hipLaunchKernelGGL((k_to_yuv<IN, 0>), grid, block, 0, st, P);
}
inline void ty_launch(const TyParams& P, int in, int chroma, int64_t nf, hipStream_t st) {
  const dim3 grid((unsigned)((P.width + CV_WAVE_COLS - 1) / CV_WAVE_COLS), (unsigned)((P.height + CV_TILE_ROWS - 1) / CV_TILE_ROWS), (unsigned)nf);
  const dim3 block(DOT_THREADS);
  switch (in) {
    case TY_BGR: ty_launch_in<TY_BGR>(P, chroma, grid, block, st); break;
    case TY_RGB: ty_launch_in<TY_RGB>(P, chroma, grid, block, st); break;
    case TY_BGRA: ty_launch_in<TY_BGRA>(P, chroma, grid, block, st); break;
    case TY_RGBA: ty_launch_in<TY_RGBA>(P, chroma, grid, block, st); break;
    default: ty_launch_in<TY_GRAY>(P, chroma, grid, block, st); break;
  }
  HIPCHK(hipGetLastError());
}

// Arguments are checked by the caller (sba_api.hip).  Chunks and staging of the source are those of sba_frames.hpp
// (chunk_of by CHUNK_FRAMES, frames_in_chunks); the planes are written through a YuvOutput of that file.  Which chunk or buffer
// a frame passes through does not enter its arithmetic.
int to_yuv_call(const FrameBatch& B, const sba_yuv_planes& out, const sba_rgb_matrix& M, const sba_to_yuv_opts& o) {
  const int64_t n_frames = B.n_frames;
  const int32_t height = B.height, width = B.width, channels = B.channels;
  if (n_frames == 0 || height == 0 || width == 0) return SBA_OK;
  HIPCHK(hipSetDevice(B.device));
  const bool in_dev = o.frames_on_device != 0, out_dev = o.out_on_device != 0;
  YuvOutput O(out, height, width, out_dev);
  TyParams P{};
  P.height = height; P.width = width; P.c_mode = O.mode; P.c_step = O.c_step;
  P.yc = (1 << 19) + (M.y_offset << 20);
  P.cry = M.cry; P.cgy = M.cgy; P.cby = M.cby; P.cru = M.cru; P.cgu = M.cgu; P.cbu = M.cbu; P.crv = M.crv; P.cgv = M.cgv; P.cbv = M.cbv;

  const int64_t chunk = chunk_of(CHUNK_FRAMES, o.chunk_frames, B, in_dev, O.tight, out_dev);
  O.alloc(chunk);
  const FramePlane plane = frame_plane(B);
  const int in = channels == 1 ? TY_GRAY : o.in_format;
  frames_in_chunks(
      &plane, 1, n_frames, in_dev, chunk,
      [&](const FramePlane* c, int64_t lo, int64_t m, hipStream_t st) {
        P.src = c->base; P.row_pitch = c->row_pitch; P.frame_pitch = c->frame_pitch;
        O.target(lo, P.y, P.u, P.v, P.y_row_pitch, P.y_frame_pitch, P.c_row_pitch, P.c_frame_pitch);
        ty_launch(P, in, o.chroma, m, st);
      },
      [&](int64_t lo, int64_t m, hipStream_t st) { O.fetch(lo, m, st); }, [&](int64_t lo, int64_t m) { O.done(lo, m); });
  return SBA_OK;
}

}  // namespace sba_detect
