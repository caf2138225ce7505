// sba_detect.hip -- the kernels that work on video frames, and the host half of every frame call: the laser-dot detectors
// (sba_detect.hpp: moments; sba_blobs.hpp: connected components), the undistortion (sba_undistort.hpp), the background
// statistics (sba_background.hpp), the conversion of decoder frames (sba_convert.hpp), its way back to encoder frames
// (sba_yuv.hpp), the area-averaged previews (sba_resize.hpp), the undistortion of YUV 4:2:0 frames plane by plane
// (sba_undistort_yuv.hpp), the per-frame value histograms (sba_hist.hpp), the plane views and virtual cameras (sba_warp.hpp),
// the sub-pixel corner refinement (sba_corners.hpp) and the local-mean masks (sba_adaptive.hpp).  They do not depend on the
// engine's camera model, so they are compiled once, in a translation unit of their own.  Each header DEFINES the *_call that
// sba_frame_calls.hpp declares and sba_api.hip calls -- not inline: this is the one translation unit that includes them.
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
