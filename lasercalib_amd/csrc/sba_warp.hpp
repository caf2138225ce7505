// sba_warp.hpp -- sba_warp_frames (include/sba_hip.h): the view of a plane, or of a rotated virtual camera, through a calibrated
// camera.  Destination pixel (x, y) goes through a 3 x 3 matrix into normalised camera coordinates -- one IEEE division each --
// and from there through the lens of sba_undistort.hpp, word for word (ud_lens).  A pixel whose third homogeneous coordinate is
// not positive lies behind the camera: it carries BEHIND | RANGE | OUTSIDE, map (0, 0) and the border value.
//
// No kernel is written here.  k_undistort_geometry and k_undistort<C> (sba_undistort.hpp) are templates over the parameter block
// of a call and find the front end by its type: WarpParams is UdParams plus the nine values of the matrix, model_pixel the
// front end below.  Taps, loads, the LDS row, the stores, the frame walk, the launch rule and the staging are the very code
// sba_undistort_frames runs.  The front end is evaluated once per destination pixel, in front of the frame loop: its two
// divisions and three homogeneous coordinates are dead before the first frame is read.
#pragma once
#include "sba_undistort.hpp"

namespace sba_detect {

constexpr int WARP_BEHIND = 8;

struct WarpParams {
  UdParams U;                                // lens, source, output; ifx, ify, cxn, cyn are not used
  double m[9];                               // row-major
};

__host__ __device__ __forceinline__ const UdParams& ud_base(const WarpParams& Q) { return Q.U; }
__host__ __device__ __forceinline__ UdParams& ud_base(WarpParams& Q) { return Q.U; }

// The rule of sba_warp_frames for destination pixel (x, y): the projective front end, then the lens
__device__ __forceinline__ void model_pixel(const WarpParams& Q, int x, int y, int& qx, int& qy, int& flags) {
#pragma clang fp contract(off)
  const double xf = (double)x, yf = (double)y;
  const double X = (Q.m[0] * xf + Q.m[1] * yf) + Q.m[2];
  const double Y = (Q.m[3] * xf + Q.m[4] * yf) + Q.m[5];
  const double Z = (Q.m[6] * xf + Q.m[7] * yf) + Q.m[8];
  const bool front = Z > 0.0;
  const double xn = front ? X / Z : 0.0, yn = front ? Y / Z : 0.0;
  ud_lens(Q.U, xn, yn, front, qx, qy, flags);
  flags |= front ? 0 : WARP_BEHIND;
}

// Arguments are checked by the caller (sba_api.hip); everything behind the model is ud_call
int warp_call(const FrameBatch& B, const sba_lens& L, const double* m, int32_t out_height, int32_t out_width, const FrameOut& out,
              const sba_undistort_opts& o, uint8_t* flags_out, int32_t* map_out) {
  WarpParams Q{};
  static const double unit_k[4] = {1.0, 1.0, 0.0, 0.0};
  ud_set_lens(Q.U, L, unit_k);
  for (int k = 0; k < 9; ++k) Q.m[k] = m[k];
  return ud_call(Q, B, out_height, out_width, out, o, flags_out, map_out);
}

}  // namespace sba_detect
