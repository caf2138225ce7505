// sba_engine_ncp11.hip -- the engine and all kernels for the 11-parameter camera model ([rvec, t, f, k1, k2, cx, cy]: the reference's, pySBA.py:31-35).
#define SBA_NCP 11
#include "sba_engine.hpp"

sba_host::EngineBase* sba_make_engine_ncp11(int dtype) { return SBA_NS::make_engine(dtype); }
int sba_rows_call_ncp11(int dtype, bool project, int device, int64_t n, const double* pts, const double* other, double* out) {
  return SBA_NS::rows_call_dtype(dtype, project, device, n, pts, other, out);
}
int sba_unproject_rows_ncp11(int device, int64_t n, const double* uv, const double* cam_rows, const double* planes, int64_t n_planes,
                             double* xn_out, double* origin_out, double* dir_out, double* points_out, double* depth_out, int32_t* status_out) {
  return SBA_NS::unp_rows_call(device, n, uv, cam_rows, planes, n_planes, xn_out, origin_out, dir_out, points_out, depth_out, status_out);
}
