// sba_detect.hip -- the kernels that work on video frames: the laser-dot detectors (sba_detect.hpp: moments; sba_blobs.hpp:
// connected components), the undistortion (sba_undistort.hpp), the background statistics (sba_background.hpp), the
// conversion of decoder frames (sba_convert.hpp), its way back to encoder frames (sba_yuv.hpp), the area-averaged previews
// (sba_resize.hpp), the undistortion of YUV 4:2:0 frames plane by plane (sba_undistort_yuv.hpp), the per-frame value
// histograms (sba_hist.hpp), the plane views and virtual cameras (sba_warp.hpp) the sub-pixel corner refinement (sba_corners.hpp) and the local-mean masks
// (sba_adaptive.hpp).  They do not depend on the engine's camera model, so they are compiled once, in a translation
// unit of their own.
#include "sba_blobs.hpp"
#include "sba_undistort.hpp"
#include "sba_background.hpp"
#include "sba_convert.hpp"
#include "sba_yuv.hpp"
#include "sba_resize.hpp"
#include "sba_undistort_yuv.hpp"
#include "sba_hist.hpp"
#include "sba_warp.hpp"
#include "sba_corners.hpp"
#include "sba_adaptive.hpp"

int sba_detect_call(int device, const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels,
                    int64_t row_pitch, int64_t frame_pitch, const sba_dot_opts& opts, uint64_t* sums, int32_t* box, double* centroid,
                    int32_t* status) {
  return sba_detect::dot_call(device, frames, n_frames, height, width, channels, row_pitch, frame_pitch, opts, sums, box, centroid, status);
}

int sba_blobs_call(int device, const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels,
                   int64_t row_pitch, int64_t frame_pitch, const sba_blob_opts& opts, int32_t* n_components, uint64_t* blobs,
                   int32_t* accepted, double* centroid, int32_t* status, uint8_t* mask_out, int32_t* labels_out) {
  return sba_detect::blob_call(device, frames, n_frames, height, width, channels, row_pitch, frame_pitch, opts, n_components, blobs,
                               accepted, centroid, status, mask_out, labels_out);
}

int sba_undistort_call(int device, const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels,
                       int64_t row_pitch, int64_t frame_pitch, const sba_lens& lens, const double* new_k, int32_t out_height,
                       int32_t out_width, int64_t out_row_pitch, int64_t out_frame_pitch, const sba_undistort_opts& opts, uint8_t* out,
                       uint8_t* flags_out, int32_t* map_out) {
  return sba_detect::undistort_call(device, frames, n_frames, height, width, channels, row_pitch, frame_pitch, lens, new_k, out_height,
                                    out_width, out_row_pitch, out_frame_pitch, opts, out, flags_out, map_out);
}

int sba_bg_accumulate_call(int device, const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels,
                           int64_t row_pitch, int64_t frame_pitch, const sba_background_accumulate_opts& opts, const uint8_t* use,
                           uint32_t* sum, uint64_t* sumsq, uint32_t* hot, uint8_t* vmax, uint64_t* n_used) {
  return sba_detect::bg_accumulate_call(device, frames, n_frames, height, width, channels, row_pitch, frame_pitch, opts, use, sum, sumsq,
                                        hot, vmax, n_used);
}

int sba_bg_suppress_call(int device, const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels,
                         int64_t row_pitch, int64_t frame_pitch, const uint8_t* level, const uint8_t* mask, int64_t out_row_pitch,
                         int64_t out_frame_pitch, const sba_background_suppress_opts& opts, uint8_t* out) {
  return sba_detect::bg_suppress_call(device, frames, n_frames, height, width, channels, row_pitch, frame_pitch, level, mask,
                                      out_row_pitch, out_frame_pitch, opts, out);
}

int sba_convert_call(int device, const sba_yuv_planes& src, int64_t n_frames, int32_t height, int32_t width, const sba_yuv_matrix& matrix,
                     int64_t out_row_pitch, int64_t out_frame_pitch, const sba_convert_opts& opts, uint8_t* out) {
  return sba_detect::convert_call(device, src, n_frames, height, width, matrix, out_row_pitch, out_frame_pitch, opts, out);
}

int sba_resize_call(int device, const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels,
                    int64_t row_pitch, int64_t frame_pitch, int32_t fx, int32_t fy, int64_t out_row_pitch, int64_t out_frame_pitch,
                    const sba_resize_opts& opts, uint8_t* out) {
  return sba_detect::resize_call(device, frames, n_frames, height, width, channels, row_pitch, frame_pitch, fx, fy, out_row_pitch,
                                 out_frame_pitch, opts, out);
}

int sba_to_yuv_call(int device, const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels, int64_t row_pitch,
                    int64_t frame_pitch, const sba_yuv_planes& out, const sba_rgb_matrix& matrix, const sba_to_yuv_opts& opts) {
  return sba_detect::to_yuv_call(device, frames, n_frames, height, width, channels, row_pitch, frame_pitch, out, matrix, opts);
}

int sba_undistort_yuv_call(int device, const sba_yuv_planes& src, int64_t n_frames, int32_t height, int32_t width, const sba_lens& lens,
                           const double* new_k, int32_t out_height, int32_t out_width, const sba_yuv_planes* out,
                           const sba_undistort_yuv_opts& opts, uint8_t* flags_out, int32_t* map_out) {
  return sba_detect::undistort_yuv_call(device, src, n_frames, height, width, lens, new_k, out_height, out_width, out, opts, flags_out,
                                        map_out);
}

int sba_hist_call(int device, const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels, int64_t row_pitch,
                  int64_t frame_pitch, const sba_hist_opts& opts, uint32_t* hist, uint64_t* total) {
  return sba_detect::hist_call(device, frames, n_frames, height, width, channels, row_pitch, frame_pitch, opts, hist, total);
}

int sba_warp_call(int device, const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels, int64_t row_pitch,
                  int64_t frame_pitch, const sba_lens& lens, const double* m, int32_t out_height, int32_t out_width, int64_t out_row_pitch,
                  int64_t out_frame_pitch, const sba_undistort_opts& opts, uint8_t* out, uint8_t* flags_out, int32_t* map_out) {
  return sba_detect::warp_call(device, frames, n_frames, height, width, channels, row_pitch, frame_pitch, lens, m, out_height, out_width,
                               out_row_pitch, out_frame_pitch, opts, out, flags_out, map_out);
}

int sba_corners_call(int device, const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels,
                     int64_t row_pitch, int64_t frame_pitch, const int64_t* corner_start, const double* corners,
                     const sba_corner_opts& opts, const double* weights, double* refined, int32_t* status, int32_t* iterations,
                     double* tensor) {
  return sba_detect::corners_call(device, frames, n_frames, height, width, channels, row_pitch, frame_pitch, corner_start, corners, opts,
                                  weights, refined, status, iterations, tensor);
}

int sba_adaptive_call(int device, const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels,
                      int64_t row_pitch, int64_t frame_pitch, const sba_adaptive_opts& opts, int64_t out_row_pitch, int64_t out_frame_pitch,
                      int64_t out_window_pitch, uint8_t* out, uint8_t* mean_out) {
  return sba_detect::adaptive_call(device, frames, n_frames, height, width, channels, row_pitch, frame_pitch, opts, out_row_pitch,
                                   out_frame_pitch, out_window_pitch, out, mean_out);
}
