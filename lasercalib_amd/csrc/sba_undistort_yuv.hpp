// sba_undistort_yuv.hpp -- sba_undistort_yuv (include/sba_hip.h): takes the lens out of 8-bit YUV 4:2:0 frames plane by plane,
// from a decoder's planes (the source of sba_convert.hpp) into an encoder's (the destination of sba_yuv.hpp), without a colour
// matrix in between.  The luma plane is a one-channel image under the rule of sba_undistort.hpp, word for word (ud_pixel,
// ud_taps with C = 1); a chroma plane is a half-size image under the same lens, its samples sited at the centres of their
// 2 x 2 blocks: the model is evaluated at (2 i + 0.5, 2 j + 0.5) and the position goes to the 1/32 grid of the chroma plane
// (uy_chroma_pos), from where ud_taps takes taps and weights with the chroma plane as the source.
//
// One kernel, k_undistort_yuv, writes all three planes of a tile in one launch.  What was chosen, and why:
//   * A workgroup owns UY_TILE_COLS = 128 luma columns x UY_TILE_ROWS = 2 DOT_WAVES luma rows, a wave one luma row PAIR and the
//     chroma row under it, a lane the luma pixels x0 + lane + 64 j of both rows and the chroma sample i0 + lane: as in
//     k_undistort neighbouring lanes are neighbouring samples, so their taps fall into neighbouring source bytes.  A row pair
//     per wave keeps a chroma row and the two luma rows it belongs to in one wave: no wave has chroma work the others lack.
//     (With 256 columns, k_undistort's width, a lane held ten samples and the kernel 255 registers: two waves a SIMD.)
//   * The float64 model runs ONCE per sample -- 4 luma positions and 1 chroma position a lane -- into a byte offset and a tap
//     word each, and the workgroup then walks the frames of its share of the chunk (the launch rule of ud_launch): no map is
//     stored.  Only those two words a sample are carried from frame to frame (see the frame loop): 110 registers, four waves
//     a SIMD.
//   * All tap loads of a frame are issued before the first is used: clamped and unbranched (ud_clamped) for the luma plane
//     and for the chroma planes separately, each with its tap-by-tap fallback for a source too narrow for a pair.  A tap row
//     is 2 bytes of luma; of chroma it is ONE 4-byte load where u and v are the halves of an interleaved plane (NV12 / NV21),
//     2 bytes from each plane where they are planar, and single bytes for planes of their own with c_step = 2 (the byte
//     behind the last sample of such a row need not exist).  The branches between these are the same in every lane.
//   * Finished rows -- two of luma, and one interleaved or two planar of chroma -- go through LDS, placed at the alignment of
//     their destination address, and leave as 16-byte stores with single bytes only in front of the first and behind the
//     last 16-byte boundary of the ADDRESS.  Chroma planes of their own with c_step = 2 are written byte by byte from
//     registers: the bytes in between must survive.  The LDS traffic is between the lanes of one wave (wave_lds_sync), so the
//     waves of a workgroup never wait for each other and a wave below the last row leaves at once.
// The kernel is bound by its scattered 2- and 4-byte tap loads, as k_undistort is; per output pixel it issues 2 + 2 / 4 (NV12)
// of them where k_undistort<3> issues 2 of three times the width, and it forms 1.5 one-channel samples instead of 3.
// The host side is that of sba_frames.hpp: a YuvSource on the way in (frames_in_chunks over two or three planes, as in
// convert_call) and a YuvOutput on the way out (as in to_yuv_call).
#pragma once
#include "sba_undistort.hpp"
#include "sba_convert.hpp"

namespace sba_detect {

constexpr int UY_TILE_COLS = 128, UY_TILE_ROWS = 2 * DOT_WAVES;            // luma pixels of a workgroup's tile: a row pair per wave
constexpr int UY_PX = UY_TILE_COLS / 64, UY_CPX = UY_PX / 2;                // luma pixels per lane and row, chroma samples per lane
constexpr int UY_ROW_LDS = 16 + UY_TILE_COLS;                               // a row of results behind up to 15 bytes of misalignment
constexpr int64_t UY_GROUPS = 2048;                                          // workgroups of a launch where the frames allow it

struct UyParams {
  UdParams L;                                // lens, new_k, the luma plane as source and as output, nearest, border = border_y
  const uint8_t *su, *sv;                    // source chroma of the chunk's first frame; CV_UV / CV_VU: su is the lower address, sv = su
  int64_t sc_row_pitch, sc_frame_pitch;
  uint8_t *ou, *ov;                          // output chroma likewise
  int64_t oc_row_pitch, oc_frame_pitch;
  int32_t sc_step, sc_mode, oc_mode;         // CV_PLANAR, CV_UV, CV_VU or CV_STEP2 (sba_frames.hpp) on either side
  int32_t border_u, border_v;
};

// Chroma sample (i, j): the model at the centre of its block -- the lines of ud_pixel up to sx, sy and in_range, at a position
// that is not a whole pixel (ud_pixel itself stays as it is: luma calls it) -- and the position on the 1/32 grid of the chroma
// plane, (sx - 0.5) / 2 in units of 1/32 sample, by the operations of the header; (0, 0) when the position is not in range.
__device__ __forceinline__ void uy_chroma_pos(const UdParams& P, int i, int j, int& qcx, int& qcy, bool& in_range) {
#pragma clang fp contract(off)
  const double x = 2.0 * (double)i + 0.5, y = 2.0 * (double)j + 0.5;     // exact
  const double xn = (x - P.cxn) * P.ifx, yn = (y - P.cyn) * P.ify;
  const double x2 = xn * xn, y2 = yn * yn, r2 = x2 + y2, xy = xn * yn;
  double t = r2 * P.k3; t = P.k2 + t; t = r2 * t; t = P.k1 + t; t = r2 * t;
  const double rad = 1.0 + t;
  const double xd = xn * rad + ((2.0 * P.p1) * xy + P.p2 * (r2 + 2.0 * x2));
  const double yd = yn * rad + (P.p1 * (r2 + 2.0 * y2) + (2.0 * P.p2) * xy);
  const double sx = P.fx * xd + P.cx, sy = P.fy * yd + P.cy;
  in_range = sx > -32768.0 && sx < 32768.0 && sy > -32768.0 && sy < 32768.0;
  double mx = sx * 16.0; mx = mx - 8.0; mx = mx + 0.5;
  double my = sy * 16.0; my = my - 8.0; my = my + 0.5;
  qcx = in_range ? (int)floor(mx) : 0;
  qcy = in_range ? (int)floor(my) : 0;
}

// The four taps of a sample from the two pairs loaded at its clamped position (ud_taps): which of a pair a tap is, or the border
__device__ __forceinline__ void uy_select(uint32_t k, uint32_t bv, uint32_t (&t)[4]) {
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const uint32_t a = t[2 * r], b = t[2 * r + 1];
    t[2 * r] = k >> (10 + 2 * r) & 1u ? (k >> 15 & 1u ? b : a) : bv;
    t[2 * r + 1] = k >> (11 + 2 * r) & 1u ? (k >> 16 & 1u ? a : b) : bv;
  }
}
__device__ __forceinline__ uint32_t uy_blend(uint32_t k, const uint32_t (&t)[4]) {
  const uint32_t ax = k & 31u, ay = k >> 5 & 31u;
  return ((32u - ax) * (32u - ay) * t[0] + ax * (32u - ay) * t[1] + (32u - ax) * ay * t[2] + ax * ay * t[3] + 512u) >> 10;
}

// The nb <= UY_TILE_COLS bytes of a finished row, which lie in LDS as their destination does modulo 16 (a = dst & 15)
__device__ __forceinline__ void uy_store_row(uint8_t* dst, const uint8_t* srow, int a, int nb, int lane) {
  const int head = min(nb, (16 - a) & 15), nv = (nb - head) >> 4, tail = head + nv * 16;   // nv <= 8: a vector per lane
  if (lane < nv) *reinterpret_cast<uint4*>(dst + head + 16 * lane) = *reinterpret_cast<const uint4*>(srow + a + head + 16 * lane);
  const int b = lane < 32 ? lane : tail + (lane - 32);                    // lanes 0..14: in front of the vectors; 32..46: behind
  if (b < (lane < 32 ? head : nb)) dst[b] = srow[a + b];
}

// grid (tiles in x, tiles in y, frame groups), DOT_THREADS threads; the plane pointers point at the chunk's first frame
__global__ void __launch_bounds__(DOT_THREADS) k_undistort_yuv(const UyParams P, int n_frames) {
  __shared__ __attribute__((aligned(16))) uint8_t s_row[DOT_WAVES][4][UY_ROW_LDS];      // per wave: two luma rows, two of chroma
  const UdParams& L = P.L;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = (int)blockIdx.x * UY_TILE_COLS, y0 = ((int)blockIdx.y * DOT_WAVES + wave) * 2;
  if (y0 >= L.out_height) return;                                         // no wave waits for another
  const bool row1 = y0 + 1 < L.out_height;
  const int i0 = x0 >> 1, jc = y0 >> 1;
  const int nbl = min(UY_TILE_COLS, L.out_width - x0), ncs = (nbl + 1) >> 1;   // luma bytes of a row, chroma samples of the row
  UdParams Cp = L;                                                        // a chroma plane as a source of sc_step-byte pixels
  Cp.src.width = (L.src.width + 1) >> 1; Cp.src.height = (L.src.height + 1) >> 1; Cp.src.row_pitch = P.sc_row_pitch;

  int64_t off[2][UY_PX], coff[UY_CPX];
  uint32_t tap[2][UY_PX], ctap[UY_CPX];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int j = 0; j < UY_PX; ++j) {
      const int x = x0 + lane + 64 * j;
      off[r][j] = 0; tap[r][j] = 0;                                       // a pixel beyond the image reads nothing
      if (x < L.out_width && (r == 0 || row1)) {
        int qx, qy, fl;
        ud_pixel(L, x, y0 + r, qx, qy, fl);
        ud_taps(L, 1, qx, qy, !(fl & UD_RANGE), off[r][j], tap[r][j]);
      }
      __builtin_amdgcn_sched_barrier(0);                                  // one float64 chain at a time: interleaved they take the registers of all
    }
#pragma unroll
  for (int k = 0; k < UY_CPX; ++k) {
    coff[k] = 0; ctap[k] = 0;
    if (lane + 64 * k < ncs) {
      int qcx, qcy;
      bool in_range;
      uy_chroma_pos(L, i0 + lane + 64 * k, jc, qcx, qcy, in_range);
      ud_taps(Cp, P.sc_step, qcx, qcy, in_range, coff[k], ctap[k]);
    }
  }
  const bool l_clamped = ud_clamped(L), c_clamped = ud_clamped(Cp);
  const bool s_paired = P.sc_mode == CV_UV || P.sc_mode == CV_VU;
  const uint32_t by = (uint32_t)L.border, bu = (uint32_t)P.border_u, bv = (uint32_t)P.border_v;
  // sample (i, j) of U and of V as bytes: interleaved halves lie one byte apart behind su
  const uint8_t* const ub = P.su + (P.sc_mode == CV_VU ? 1 : 0);
  const uint8_t* const vb = s_paired ? P.su + (P.sc_mode == CV_UV ? 1 : 0) : P.sv;
  const int f_lo = (int)blockIdx.z * L.frames_per_group, f_hi = min(n_frames, f_lo + L.frames_per_group);

  for (int f = f_lo; f < f_hi; ++f) {
    const uint8_t* __restrict__ yp = L.src.frames + (int64_t)f * L.src.frame_pitch;
    const int64_t cf = (int64_t)f * P.sc_frame_pitch;
    uint32_t t[2][UY_PX][4], tu[UY_CPX][4], tv[UY_CPX][4];
    // What a frame derives from a tap word -- weights, selections, the row step -- is formed again for every frame: carried
    // across the loop it took 160 registers where this takes half, and the kernel waits for loads, not for the VALU.
#pragma unroll
    for (int j = 0; j < UY_PX; ++j) { asm volatile("" : "+v"(tap[0][j])); asm volatile("" : "+v"(tap[1][j])); }
#pragma unroll
    for (int k = 0; k < UY_CPX; ++k) asm volatile("" : "+v"(ctap[k]));
    // ---- every load of the frame is issued before the first is waited for
    if (l_clamped) {
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int j = 0; j < UY_PX; ++j) {
          const uint8_t* p = yp + off[r][j];
          ud_load2<1>(p, t[r][j][0], t[r][j][1]);
          ud_load2<1>(p + (tap[r][j] >> 17 & 1u ? L.src.row_pitch : 0), t[r][j][2], t[r][j][3]);
        }
    } else {
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int j = 0; j < UY_PX; ++j) {
          const uint32_t rd = tap[r][j] >> 10 & 15u;
          const uint8_t* p = yp + off[r][j];
          t[r][j][0] = t[r][j][1] = t[r][j][2] = t[r][j][3] = by;
#pragma unroll
          for (int q = 0; q < 2; ++q, p += L.src.row_pitch) {
            if (rd >> 2 * q & 1u) t[r][j][2 * q] = p[0];
            if (rd >> 2 * q & 2u) t[r][j][2 * q + 1] = p[1];
          }
        }
    }
    if (c_clamped) {
#pragma unroll
      for (int k = 0; k < UY_CPX; ++k) {
        const int64_t o = cf + coff[k], step = ctap[k] >> 17 & 1u ? P.sc_row_pitch : 0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          if (s_paired) {                                                 // e: the bytes at the even addresses, o: at the odd ones
            uint32_t w;
            __builtin_memcpy(&w, P.su + o + q * step, 4);
            const uint32_t e0 = w & 255u, o0 = w >> 8 & 255u, e1 = w >> 16 & 255u, o1 = w >> 24;
            const bool uv = P.sc_mode == CV_UV;
            tu[k][2 * q] = uv ? e0 : o0; tu[k][2 * q + 1] = uv ? e1 : o1;
            tv[k][2 * q] = uv ? o0 : e0; tv[k][2 * q + 1] = uv ? o1 : e1;
          } else if (P.sc_mode == CV_PLANAR) {
            ud_load2<1>(P.su + o + q * step, tu[k][2 * q], tu[k][2 * q + 1]);
            ud_load2<1>(P.sv + o + q * step, tv[k][2 * q], tv[k][2 * q + 1]);
          } else {
            const uint8_t *pu = P.su + o + q * step, *pv = P.sv + o + q * step;
            tu[k][2 * q] = pu[0]; tu[k][2 * q + 1] = pu[2];
            tv[k][2 * q] = pv[0]; tv[k][2 * q + 1] = pv[2];
          }
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < UY_CPX; ++k) {
        const uint32_t rd = ctap[k] >> 10 & 15u;
        const uint8_t *pu = ub + cf + coff[k], *pv = vb + cf + coff[k];
        tu[k][0] = tu[k][1] = tu[k][2] = tu[k][3] = bu;
        tv[k][0] = tv[k][1] = tv[k][2] = tv[k][3] = bv;
#pragma unroll
        for (int q = 0; q < 2; ++q, pu += P.sc_row_pitch, pv += P.sc_row_pitch) {
          if (rd >> 2 * q & 1u) { tu[k][2 * q] = pu[0]; tv[k][2 * q] = pv[0]; }
          if (rd >> 2 * q & 2u) { tu[k][2 * q + 1] = pu[P.sc_step]; tv[k][2 * q + 1] = pv[P.sc_step]; }
        }
      }
    }
    if (l_clamped) {
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int j = 0; j < UY_PX; ++j) uy_select(tap[r][j], by, t[r][j]);
    }
    if (c_clamped) {
#pragma unroll
      for (int k = 0; k < UY_CPX; ++k) { uy_select(ctap[k], bu, tu[k]); uy_select(ctap[k], bv, tv[k]); }
    }

    // ---- the rows into LDS, each placed as its destination lies modulo 16
    uint8_t* const dy = L.out + ((int64_t)f * L.out_frame_pitch + (int64_t)y0 * L.out_row_pitch + x0);
    const int ay0 = (int)(reinterpret_cast<uintptr_t>(dy) & 15u), ay1 = (int)(reinterpret_cast<uintptr_t>(dy + L.out_row_pitch) & 15u);
#pragma unroll
    for (int j = 0; j < UY_PX; ++j) {
      s_row[wave][0][ay0 + lane + 64 * j] = (uint8_t)uy_blend(tap[0][j], t[0][j]);
      s_row[wave][1][ay1 + lane + 64 * j] = (uint8_t)uy_blend(tap[1][j], t[1][j]);
    }
    const int64_t co = (int64_t)f * P.oc_frame_pitch + (int64_t)jc * P.oc_row_pitch;
    uint8_t *du = P.ou + co, *dv = P.ov + co;
    int au = 0, av = 0;
    if (P.oc_mode == CV_STEP2) {                                          // the bytes in between survive: no vector store
#pragma unroll
      for (int k = 0; k < UY_CPX; ++k)
        if (lane + 64 * k < ncs) {
          du[2 * (int64_t)(i0 + lane + 64 * k)] = (uint8_t)uy_blend(ctap[k], tu[k]);
          dv[2 * (int64_t)(i0 + lane + 64 * k)] = (uint8_t)uy_blend(ctap[k], tv[k]);
        }
    } else if (P.oc_mode == CV_PLANAR) {
      du += i0; dv += i0;
      au = (int)(reinterpret_cast<uintptr_t>(du) & 15u); av = (int)(reinterpret_cast<uintptr_t>(dv) & 15u);
#pragma unroll
      for (int k = 0; k < UY_CPX; ++k) {
        s_row[wave][2][au + lane + 64 * k] = (uint8_t)uy_blend(ctap[k], tu[k]);
        s_row[wave][3][av + lane + 64 * k] = (uint8_t)uy_blend(ctap[k], tv[k]);
      }
    } else {                                                              // one row of pairs behind ou, the lower address
      du += 2 * i0;
      au = (int)(reinterpret_cast<uintptr_t>(du) & 15u);
      const bool uv = P.oc_mode == CV_UV;
#pragma unroll
      for (int k = 0; k < UY_CPX; ++k) {
        const uint32_t U = uy_blend(ctap[k], tu[k]), V = uy_blend(ctap[k], tv[k]);
        s_row[wave][2][au + 2 * (lane + 64 * k)] = (uint8_t)(uv ? U : V);
        s_row[wave][2][au + 2 * (lane + 64 * k) + 1] = (uint8_t)(uv ? V : U);
      }
    }
    wave_lds_sync();
    uy_store_row(dy, s_row[wave][0], ay0, nbl, lane);
    if (row1) uy_store_row(dy + L.out_row_pitch, s_row[wave][1], ay1, nbl, lane);
    if (P.oc_mode == CV_PLANAR) {
      uy_store_row(du, s_row[wave][2], au, ncs, lane);
      uy_store_row(dv, s_row[wave][3], av, ncs, lane);
    } else if (P.oc_mode != CV_STEP2) {
      uy_store_row(du, s_row[wave][2], au, 2 * ncs, lane);
    }
    wave_lds_sync();                                                      // read before the next frame's rows overwrite them
  }
}

// ------------------------------------------------------------------------------------------------ host side
inline void uy_launch(const UyParams& P, int64_t nf, hipStream_t st) {
  const unsigned gx = (unsigned)((P.L.out_width + UY_TILE_COLS - 1) / UY_TILE_COLS), gy = (unsigned)((P.L.out_height + UY_TILE_ROWS - 1) / UY_TILE_ROWS);
  // about UY_GROUPS workgroups where the frames allow it (ud_launch's rule); which workgroup takes a frame does not change its bytes
  const int64_t groups = std::max<int64_t>(1, std::min<int64_t>(nf, UY_GROUPS / ((int64_t)gx * gy)));
  UyParams Q = P;
  Q.L.frames_per_group = (int32_t)((nf + groups - 1) / groups);
  const dim3 grid(gx, gy, (unsigned)((nf + Q.L.frames_per_group - 1) / Q.L.frames_per_group));
  hipLaunchKernelGGL(k_undistort_yuv, grid, dim3(DOT_THREADS), 0, st, Q, (int)nf);
  HIPCHK(hipGetLastError());
}

// Arguments are checked by the caller (sba_api.hip).  The source is staged as a YuvSource and the planes are written through a
// YuvOutput (sba_frames.hpp), in chunks of chunk_of by CHUNK_FRAMES.  Which chunk, workgroup or buffer a frame passes through
// does not enter its arithmetic: any chunk_frames gives the same bytes.
int undistort_yuv_call(int device, const sba_yuv_planes& S, int64_t n_frames, int32_t height, int32_t width, const sba_lens& lens,
                       const double* new_k, int32_t out_height, int32_t out_width, const sba_yuv_planes* out,
                       const sba_undistort_yuv_opts& o, uint8_t* flags_out, int32_t* map_out) {
  if ((int64_t)out_height * out_width == 0) return SBA_OK;
  HIPCHK(hipSetDevice(device));
  UyParams P{};
  P.L.src = frame_view(S.y, S.y_row_pitch, S.y_frame_pitch, height, width, 0, 0);
  ud_set_lens(P.L, lens, new_k);
  P.L.out_height = out_height; P.L.out_width = out_width; P.L.nearest = o.interpolation == 1; P.L.border = o.border_y;
  P.border_u = o.border_u; P.border_v = o.border_v;
  ud_geometry_out(P.L, 1, flags_out, map_out);
  if (n_frames == 0 || !out) return SBA_OK;

  const bool in_dev = o.frames_on_device != 0, out_dev = o.out_on_device != 0;
  const YuvSource Sp(S, height, width);                                   // a source without pixels: every sample is the border
  YuvOutput O(*out, out_height, out_width, out_dev);
  P.sc_step = S.c_step; P.sc_mode = Sp.mode; P.oc_mode = O.mode;
  const int64_t chunk = chunk_of(CHUNK_FRAMES, o.chunk_frames, n_frames, Sp.tight, in_dev, O.tight, out_dev);
  O.alloc(chunk);
  frames_in_chunks(
      Sp.planes, Sp.n_planes, n_frames, in_dev, chunk,
      [&](const FramePlane* c, int64_t lo, int64_t m, hipStream_t st) {
        Sp.chunk(c, P.L.src.frames, P.su, P.sv, P.L.src.row_pitch, P.L.src.frame_pitch, P.sc_row_pitch, P.sc_frame_pitch);
        O.target(lo, P.L.out, P.ou, P.ov, P.L.out_row_pitch, P.L.out_frame_pitch, P.oc_row_pitch, P.oc_frame_pitch);
        uy_launch(P, m, st);
      },
      [&](int64_t lo, int64_t m, hipStream_t st) { O.fetch(lo, m, st); }, [&](int64_t lo, int64_t m) { O.done(lo, m); });
  return SBA_OK;
}

}  // namespace sba_detect
