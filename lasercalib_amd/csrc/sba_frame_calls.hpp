// sba_frame_calls.hpp -- what the C ABI (sba_api.hip) and the frame kernels' translation unit (sba_detect.hip) agree on, and
// nothing else: no HIP in it.  A frame entry point turns its ABI scalars into ONE description of the batch (FrameBatch) and, where
// it writes frames, ONE of where they go (FrameOut), checks them, and ends in the *_call declared here; the definition is in the
// feature header named beside it, compiled in sba_detect.hip.  These are THE declarations: the definitions see them too (every
// feature header includes sba_frames.hpp, which includes this).  A definition whose signature differs is one more overload and
// leaves the declared one undefined: libsba_hip.so then does not load, and no caller ever passes arguments to a function that
// reads them as something else.
#pragma once
#include <cstdint>
#include "../../include/sba_hip.h"

namespace sba_detect {

// n_frames 8-bit frames of height x width pixels with `channels` interleaved channels, on the host or on `device`: frame f, row
// r at frames + f frame_pitch + r row_pitch.  The leading eight arguments of an entry point, in their order.
struct FrameBatch {
  int device;
  const uint8_t* frames;
  int64_t n_frames;
  int32_t height, width, channels;
  int64_t row_pitch, frame_pitch;
};

// Where a call writes frames, and at which pitches
struct FrameOut {
  uint8_t* out;
  int64_t row_pitch, frame_pitch;
};

int dot_call(const FrameBatch& B, const sba_dot_opts& opts, uint64_t* sums, int32_t* box, double* centroid, int32_t* status);   // sba_detect.hpp
int blob_call(const FrameBatch& B, const sba_blob_opts& opts, int32_t* n_components, uint64_t* blobs, int32_t* accepted, double* centroid,
              int32_t* status, uint8_t* mask_out, int32_t* labels_out);                                                        // sba_blobs.hpp
// out_height x out_width pixels a frame, here and in warp_call
int undistort_call(const FrameBatch& B, const sba_lens& lens, const double* new_k, int32_t out_height, int32_t out_width, const FrameOut& out,
                   const sba_undistort_opts& opts, uint8_t* flags_out, int32_t* map_out);                                      // sba_undistort.hpp
int warp_call(const FrameBatch& B, const sba_lens& lens, const double* m, int32_t out_height, int32_t out_width, const FrameOut& out,
              const sba_undistort_opts& opts, uint8_t* flags_out, int32_t* map_out);                                           // sba_warp.hpp
int bg_accumulate_call(const FrameBatch& B, const sba_background_accumulate_opts& opts, const uint8_t* use, uint32_t* sum, uint64_t* sumsq,
                       uint32_t* hot, uint8_t* vmax, uint64_t* n_used);                                                        // sba_background.hpp
int bg_suppress_call(const FrameBatch& B, const uint8_t* level, const uint8_t* mask, const FrameOut& out,
                     const sba_background_suppress_opts& opts);                                                                // sba_background.hpp
int resize_call(const FrameBatch& B, int32_t fx, int32_t fy, const FrameOut& out, const sba_resize_opts& opts);                // sba_resize.hpp
int hist_call(const FrameBatch& B, const sba_hist_opts& opts, uint32_t* hist, uint64_t* total);                                // sba_hist.hpp
int corners_call(const FrameBatch& B, const int64_t* corner_start, const double* corners, const sba_corner_opts& opts, const double* weights,
                 double* refined, int32_t* status, int32_t* iterations, double* tensor);                                       // sba_corners.hpp
// window w of `out` and of `mean_out` starts w out_window_pitch bytes in; both share the pitches
int adaptive_call(const FrameBatch& B, const sba_adaptive_opts& opts, const FrameOut& out, int64_t out_window_pitch, uint8_t* mean_out);   // sba_adaptive.hpp
// the calls with a set of YUV 4:2:0 planes (sba_yuv_planes) of width x height luma samples on one side or on both
int convert_call(int device, const sba_yuv_planes& src, int64_t n_frames, int32_t height, int32_t width, const sba_yuv_matrix& matrix,
                 const FrameOut& out, const sba_convert_opts& opts);                                                           // sba_convert.hpp
int to_yuv_call(const FrameBatch& B, const sba_yuv_planes& out, const sba_rgb_matrix& matrix, const sba_to_yuv_opts& opts);    // sba_yuv.hpp
int undistort_yuv_call(int device, const sba_yuv_planes& src, int64_t n_frames, int32_t height, int32_t width, const sba_lens& lens,
                       const double* new_k, int32_t out_height, int32_t out_width, const sba_yuv_planes* out,
                       const sba_undistort_yuv_opts& opts, uint8_t* flags_out, int32_t* map_out);                              // sba_undistort_yuv.hpp

}  // namespace sba_detect
