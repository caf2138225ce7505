// sba_api.hip -- C ABI (include/sba_hip.h) over the per-camera-model engines.  gfx950 only; no CPU fallback:
// every entry point fails with SBA_ERR_NO_DEVICE / SBA_ERR_HIP when the GPU is not usable.
//
// The frame entry points (sba_detect_dots ... sba_adaptive_threshold, the second half of this file) all take one path: the ABI
// scalars become a FrameBatch (and a FrameOut where frames are written), the shared checks and the entry point's own run in the
// order tests/test_frame_arg_errors.py pins, and the call ends in the sba_detect::*_call that sba_frame_calls.hpp declares.
#include "sba_common.hpp"
#include "sba_frame_calls.hpp"

using namespace sba_host;
using sba_detect::FrameBatch;
using sba_detect::FrameOut;

// factories of the two engine translation units (sba_engine_ncp11.hip: the reference's 11-parameter radial camera,
// sba_engine_ncp13.hip: 13 parameters, radial + tangential)
sba_host::EngineBase* sba_make_engine_ncp11(int dtype);
sba_host::EngineBase* sba_make_engine_ncp13(int dtype);
int sba_rows_call_ncp11(int dtype, bool project, int device, int64_t n, const double* pts, const double* other, double* out);
int sba_rows_call_ncp13(int dtype, bool project, int device, int64_t n, const double* pts, const double* other, double* out);
int sba_unproject_rows_ncp11(int device, int64_t n, const double* uv, const double* cam_rows, const double* planes, int64_t n_planes,
                             double* xn_out, double* origin_out, double* dir_out, double* points_out, double* depth_out, int32_t* status_out);
int sba_unproject_rows_ncp13(int device, int64_t n, const double* uv, const double* cam_rows, const double* planes, int64_t n_planes,
                             double* xn_out, double* origin_out, double* dir_out, double* points_out, double* depth_out, int32_t* status_out);

// ============================================================================================== C ABI
struct sba_handle {
  int dtype;
  std::unique_ptr<EngineBase> eng;
  std::string err;
};

namespace {

template <typename F>
int guarded(sba_handle* h, F&& f) {
  ArenaScope arena_scope(h && h->eng ? &h->eng->arena : nullptr);    // buffers allocated during the call belong to the handle
  try {
    int rc = f();
    if (rc && h) h->err = h->eng ? h->eng->err : h->err;
    return rc;
  } catch (const HipError& e) {
    char buf[512];
    const char* base = strrchr(e.file, '/');
    snprintf(buf, sizeof buf, "HIP error %d (%s) at %s:%d: %s", (int)e.e, hipGetErrorString(e.e), base ? base + 1 : e.file, e.line, e.what);
    if (h) h->err = buf; else g_last_error = buf;
    return SBA_ERR_HIP;
  } catch (const RcclError& e) {
    char buf[512];
    Rccl& r = Rccl::get();
    snprintf(buf, sizeof buf, "RCCL error %d (%s) at sba_engine.hpp:%d: %s", e.code, r.error_string ? r.error_string(e.code) : "?", e.line, e.what);
    if (h) h->err = buf; else g_last_error = buf;
    return SBA_ERR_HIP;
  } catch (const std::exception& e) {
    if (h) h->err = e.what(); else g_last_error = e.what();
    return SBA_ERR_INVALID;
  }
}

int check_device(int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) { g_last_error = "no HIP device is visible (libsba_hip needs an MI355X / gfx950 GPU)"; return SBA_ERR_NO_DEVICE; }
  if (device < 0 || device >= n) { g_last_error = "device ordinal out of range"; return SBA_ERR_NO_DEVICE; }
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, device) != hipSuccess) { g_last_error = "hipGetDeviceProperties failed"; return SBA_ERR_NO_DEVICE; }
  if (std::string(p.gcnArchName).rfind("gfx950", 0) != 0) {
    g_last_error = std::string("device is ") + p.gcnArchName + ", libsba_hip is built for gfx950 only";
    return SBA_ERR_NO_DEVICE;
  }
  return SBA_OK;
}

}  // namespace

extern "C" {

int sba_abi_version(void) { return SBA_ABI_VERSION; }

int sba_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* sba_last_error(const sba_handle* h) { return h ? h->err.c_str() : g_last_error.c_str(); }

static int n_cam_params_of(int model) { return model == SBA_CAM_RADIAL_TANGENTIAL ? 13 : 11; }
static int rows_dispatch(int ncp, int dtype, bool project, int device, int64_t n, const double* pts, const double* other, double* out) {
  return ncp == 13 ? sba_rows_call_ncp13(dtype, project, device, n, pts, other, out)
                   : sba_rows_call_ncp11(dtype, project, device, n, pts, other, out);
}

int sba_rotate(int device, int dtype, int64_t n, const double* points, const double* rot_vecs, double* out) {
  if (n < 0 || (n > 0 && (!points || !rot_vecs || !out))) { g_last_error = "null argument"; return SBA_ERR_INVALID; }
  int rc = check_device(device);
  if (rc) return rc;
  return guarded(nullptr, [&] { return rows_dispatch(11, dtype, false, device, n, points, rot_vecs, out); });
}

int sba_project(int device, int dtype, int64_t n, const double* points, const double* cam_rows, double* uv_out) {
  return sba_project_model(device, dtype, SBA_CAM_RADIAL, n, points, cam_rows, uv_out);
}

int sba_project_model(int device, int dtype, int cam_model, int64_t n, const double* points, const double* cam_rows, double* uv_out) {
  if (n < 0 || (n > 0 && (!points || !cam_rows || !uv_out))) { g_last_error = "null argument"; return SBA_ERR_INVALID; }
  if (cam_model != SBA_CAM_RADIAL && cam_model != SBA_CAM_RADIAL_TANGENTIAL) { g_last_error = "unknown camera model"; return SBA_ERR_INVALID; }
  int rc = check_device(device);
  if (rc) return rc;
  return guarded(nullptr, [&] { return rows_dispatch(n_cam_params_of(cam_model), dtype, true, device, n, points, cam_rows, uv_out); });
}

int sba_unproject_rows(int device, int cam_model, int64_t n, const double* uv, const double* cam_rows, const double* planes,
                       int64_t n_planes, double* xn_out, double* origin_out, double* dir_out, double* points_out, double* depth_out,
                       int32_t* status_out) {
  if (n < 0 || (n > 0 && (!uv || !cam_rows))) { g_last_error = "null argument"; return SBA_ERR_INVALID; }
  if (cam_model != SBA_CAM_RADIAL && cam_model != SBA_CAM_RADIAL_TANGENTIAL) { g_last_error = "unknown camera model"; return SBA_ERR_INVALID; }
  if (n_planes != 0 && n_planes != 1 && n_planes != n) { g_last_error = "sba_unproject_rows: n_planes must be 0, 1 or n"; return SBA_ERR_INVALID; }
  if (n_planes == 0 && (points_out || depth_out)) { g_last_error = "sba_unproject_rows: points_out and depth_out need a plane"; return SBA_ERR_INVALID; }
  if (n_planes > 0) {
    if (!planes) { g_last_error = "null argument"; return SBA_ERR_INVALID; }
    for (int64_t k = 0; k < n_planes; ++k) {
      const double* p = planes + 4 * k;
      const double nn = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
      if (!std::isfinite(nn) || !(nn > 0.0) || !std::isfinite(p[3])) {
        g_last_error = "sba_unproject_rows: a plane is not finite or its normal is zero";
        return SBA_ERR_INVALID;
      }
    }
  }
  int rc = check_device(device);
  if (rc) return rc;
  return guarded(nullptr, [&] {
    return cam_model == SBA_CAM_RADIAL_TANGENTIAL
               ? sba_unproject_rows_ncp13(device, n, uv, cam_rows, planes, n_planes, xn_out, origin_out, dir_out, points_out, depth_out, status_out)
               : sba_unproject_rows_ncp11(device, n, uv, cam_rows, planes, n_planes, xn_out, origin_out, dir_out, points_out, depth_out, status_out);
  });
}

int sba_create(const sba_problem_desc* desc, sba_handle** out) {
  if (!desc || !out) { g_last_error = "null argument"; return SBA_ERR_INVALID; }
  *out = nullptr;
  if (desc->dtype != SBA_F64 && desc->dtype != SBA_F32) { g_last_error = "dtype must be SBA_F64 or SBA_F32"; return SBA_ERR_INVALID; }
  if (desc->cam_model != SBA_CAM_RADIAL && desc->cam_model != SBA_CAM_RADIAL_TANGENTIAL) { g_last_error = "unknown camera model"; return SBA_ERR_INVALID; }
  int rc = check_device(desc->device);
  if (rc) return rc;
  auto h = std::make_unique<sba_handle>();
  h->dtype = desc->dtype;
  rc = guarded(nullptr, [&] {
    std::unique_ptr<EngineBase> e(desc->cam_model == SBA_CAM_RADIAL_TANGENTIAL ? sba_make_engine_ncp13(desc->dtype)
                                                                                : sba_make_engine_ncp11(desc->dtype));
    ArenaScope sc(&e->arena);
    e->init(*desc);
    h->eng = std::move(e);
    return (int)SBA_OK;
  });
  if (rc) return rc;
  *out = h.release();
  return SBA_OK;
}

int sba_destroy(sba_handle* h) {
  if (!h) return SBA_OK;
  delete h;
  return SBA_OK;
}

int sba_upload(sba_handle* h, const double* cams, const double* points, const double* uv, const int64_t* cam_idx,
               const int64_t* pt_idx, const double* weights) {
  return sba_upload_ex(h, cams, points, uv, cam_idx, pt_idx, weights, nullptr);
}

int sba_upload_ex(sba_handle* h, const double* cams, const double* points, const double* uv, const int64_t* cam_idx,
                  const int64_t* pt_idx, const double* weights, const sba_upload_opts* opts) {
  if (!h) return SBA_ERR_INVALID;
  if (!cams || !points || ((!uv || !cam_idx || !pt_idx))) { h->err = "null argument"; return SBA_ERR_INVALID; }
  sba_upload_opts o{};
  if (opts) o = *opts;
  if (o.layout != SBA_LAYOUT_AUTO && o.layout != SBA_LAYOUT_HOST && o.layout != SBA_LAYOUT_DEVICE) {
    h->err = "unknown layout route";
    return SBA_ERR_INVALID;
  }
  return guarded(h, [&] { return h->eng->upload(cams, points, uv, cam_idx, pt_idx, weights, o); });
}

int sba_get_upload_report(sba_handle* h, sba_upload_report* report) {
  if (!h || !report) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->upload_report(report); });
}

int sba_get_layout(sba_handle* h, int64_t* perm, int32_t* pt_start, int32_t* cam_pm, int32_t* pt_pm, double* uv_pm, double* w_pm,
                   int32_t* pt_cm, double* uv_cm, double* w_cm, int32_t* cam_start, uint16_t* vis_mask) {
  if (!h) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->get_layout(perm, pt_start, cam_pm, pt_pm, uv_pm, w_pm, pt_cm, uv_cm, w_cm, cam_start, vis_mask); });
}

int sba_set_params(sba_handle* h, const double* x) {
  if (!h || !x) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->set_params_x(x); });
}

int sba_get_params(sba_handle* h, double* cams_out, double* points_out) {
  if (!h) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->get_params(cams_out, points_out); });
}

int sba_get_transform(sba_handle* h, double* theta12_out) {
  if (!h || !theta12_out) return SBA_ERR_INVALID;
  return h->eng->get_transform(theta12_out);
}

int sba_lm_get_step(sba_handle* h, double* delta_c_out) {
  if (!h || !delta_c_out) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->get_step(delta_c_out); });
}

int sba_get_gradient(sba_handle* h, double* gc_out, double* gp_out) {
  if (!h) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->get_gradient(gc_out, gp_out); });
}

int sba_residual(sba_handle* h, const double* x, double* r_out, double* cost_out) {
  if (!h) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->residual(x, r_out, cost_out); });
}

int sba_residual_jacobian(sba_handle* h, const double* x, double* r_out, double* Jc_out, double* Jp_out) {
  if (!h) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->residual_jacobian(x, r_out, Jc_out, Jp_out); });
}

int sba_solve_lm(sba_handle* h, const sba_lm_opts* opts, double* cams_out, double* points_out, sba_lm_report* report,
                 sba_lm_iter_log* log, int32_t log_capacity, int32_t* log_rows) {
  if (!h || !opts) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->solve(opts, cams_out, points_out, report, log, log_capacity, log_rows); });
}

int64_t sba_lm_exchange_size(const sba_handle* h) { return h ? h->eng->exchange_size() : 0; }

int sba_lm_begin(sba_handle* h, const sba_lm_opts* opts) {
  if (!h || !opts) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->lm_begin(opts); });
}
int sba_lm_linearize(sba_handle* h) {
  if (!h) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->lm_linearize(); });
}
int sba_lm_form_reduced(sba_handle* h, double* exchange_dev) {
  if (!h || !exchange_dev) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->lm_form_reduced(exchange_dev); });
}
int sba_lm_solve_trial(sba_handle* h, const double* exchange_dev, double* scalars_dev) {
  if (!h || !exchange_dev || !scalars_dev) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->lm_solve_trial(const_cast<double*>(exchange_dev), scalars_dev); });
}
int sba_lm_decide(sba_handle* h, const double* scalars_all_dev, int32_t n_ranks, int32_t* status_out,
                  int32_t* accepted_out, sba_lm_iter_log* row_out) {
  if (!h || !scalars_all_dev || n_ranks < 1) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->lm_decide(scalars_all_dev, n_ranks, status_out, accepted_out, row_out); });
}
int sba_lm_decide_async(sba_handle* h, const double* scalars_all_dev, int32_t n_ranks) {
  if (!h || n_ranks < 1 || (n_ranks > 1 && !scalars_all_dev)) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->lm_decide_async(scalars_all_dev, n_ranks); });
}
int sba_lm_poll(sba_handle* h, int32_t* status_out, int32_t* iterations_out) {
  if (!h) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->lm_poll(status_out, iterations_out); });
}

int sba_lm_run(sba_handle* h, int32_t* status_out, int32_t* iterations_out) {
  if (!h) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->lm_run(status_out, iterations_out); });
}
int sba_lm_get_log(sba_handle* h, sba_lm_iter_log* log, int32_t log_capacity, int32_t* log_rows) {
  if (!h || !log_rows) return SBA_ERR_INVALID;
  return h->eng->get_log(log, log_capacity, log_rows);
}
int sba_lm_finish(sba_handle* h, double* cams_out, double* points_out, sba_lm_report* report) {
  if (!h) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->lm_finish(cams_out, points_out, report); });
}

int sba_get_kernel_profile(sba_handle* h, double* total_us_out, int64_t* count_out) {
  if (!h || !total_us_out || !count_out) return SBA_ERR_INVALID;
  return h->eng->get_kernel_profile(total_us_out, count_out);
}

int sba_comm_get_unique_id(uint8_t* id_out) {
  if (!id_out) { g_last_error = "null argument"; return SBA_ERR_INVALID; }
  Rccl& r = Rccl::get();
  if (!r.ok) { g_last_error = r.why; return SBA_ERR_UNSUPPORTED; }
  Rccl::UniqueId uid;
  const int rc = r.get_unique_id(&uid);
  if (rc != 0) { g_last_error = std::string("ncclGetUniqueId failed: ") + r.error_string(rc); return SBA_ERR_HIP; }
  memcpy(id_out, uid.internal, Rccl::ID_BYTES);
  return SBA_OK;
}

int sba_comm_init(sba_handle* h, const uint8_t* id, int32_t rank, int32_t n_ranks) {
  if (!h || !id) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->comm_init(id, rank, n_ranks); });
}

int sba_ipc_export(sba_handle* h, int32_t n_ranks, uint8_t* handle_out) {
  if (!h || !handle_out) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->ipc_export(n_ranks, handle_out); });
}

int sba_ipc_attach(sba_handle* h, int32_t rank, int32_t n_ranks, const uint8_t* handles_all) {
  if (!h || !handles_all) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->ipc_attach(rank, n_ranks, handles_all); });
}

int sba_set_fixed_points(sba_handle* h, const uint8_t* fixed_mask) {
  if (!h) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->set_fixed_points(fixed_mask); });
}

int sba_set_robust_loss(sba_handle* h, int32_t loss, double f_scale) {
  if (!h) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->set_robust_loss(loss, f_scale); });
}

int sba_covariance(sba_handle* h, const sba_cov_opts* opts, double* cam_full, double* cam_blocks, double* pt_cov, sba_cov_report* rep) {
  if (!h) return SBA_ERR_INVALID;
  sba_cov_opts o{};
  if (opts) o = *opts;
  return guarded(h, [&] { return h->eng->covariance(&o, cam_full, cam_blocks, pt_cov, rep); });
}

int sba_triangulate(sba_handle* h, const sba_tri_opts* opts, double* points_out, int32_t* status_out, int32_t* n_views_out,
                    double* rms_px_out, double* max_px_out, double* spread_out, uint8_t* inlier_out, sba_tri_report* rep) {
  if (!h) return SBA_ERR_INVALID;
  sba_tri_opts o{};
  o.min_views = 2; o.max_drop = 1;
  if (opts) o = *opts;
  return guarded(h, [&] {
    return h->eng->triangulate(&o, points_out, status_out, n_views_out, rms_px_out, max_px_out, spread_out, inlier_out, rep);
  });
}

int sba_unproject(sba_handle* h, const sba_unp_opts* opts, const double* planes, int64_t n_planes, double* points_out, int32_t* status_out,
                  int32_t* n_views_out, double* rms_px_out, double* max_px_out, uint8_t* used_out, sba_unp_report* rep) {
  if (!h) return SBA_ERR_INVALID;
  sba_unp_opts o{};
  if (opts) o = *opts;
  return guarded(h, [&] {
    return h->eng->unproject(&o, planes, n_planes, points_out, status_out, n_views_out, rms_px_out, max_px_out, used_out, rep);
  });
}

int sba_align(sba_handle* h, const sba_align_opts* opts, const double* target_points, const double* point_weights,
              const double* target_centres, const double* centre_weights, sba_align_report* rep) {
  if (!h) return SBA_ERR_INVALID;
  sba_align_opts o{};
  o.with_scale = 1; o.apply = 1;
  if (opts) o = *opts;
  return guarded(h, [&] { return h->eng->align(&o, target_points, point_weights, target_centres, centre_weights, rep); });
}

int sba_apply_similarity(sba_handle* h, double scale, const double* R, const double* t) {
  if (!h) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->apply_similarity(scale, R, t); });
}

int sba_reproj_stats(sba_handle* h, const sba_reproj_opts* opts, double* cam_stats, int64_t* cam_hist, double* cam_grid,
                     double* cam_radial, double* pt_stats, double* err_out, int64_t* worst_idx, double* worst_err,
                     sba_reproj_report* rep) {
  if (!h) return SBA_ERR_INVALID;
  sba_reproj_opts o{};
  if (opts) o = *opts;
  return guarded(h, [&] {
    return h->eng->reproj_stats(&o, cam_stats, cam_hist, cam_grid, cam_radial, pt_stats, err_out, worst_idx, worst_err, rep);
  });
}

// ---------------------------------------------------------------------------------------------- frame entry points
// What an entry point (`fn`, for the error text) checks of its batch, in the order every one reports it: frame_args_invalid,
// then its own options and outputs, then frame_layout_invalid (the pitches, the size limit, the device).
//
// ADDING A FRAME FUNCTION touches: include/sba_hip.h (the prototype and its options); a feature header with the kernels and
// the *_call, included by sba_detect.hip and listed in the Makefile beside it; that *_call's declaration in sba_frame_calls.hpp;
// the entry point here (FrameBatch, the checks below, guarded(*_call)); _native.py (signature, EXPORTED_SYMBOLS, wrapper); a
// table in tests/test_frame_arg_errors.py and a tests/test_gpu_*.py.
static int detect_invalid(const char* fn, const char* what) { g_last_error = std::string(fn) + ": " + what; return SBA_ERR_INVALID; }

static int frame_args_invalid(const char* fn, const FrameBatch& B, int32_t channel, int32_t threshold) {
  if (B.n_frames < 0 || B.height < 0 || B.width < 0) return detect_invalid(fn, "negative size");
  if (B.n_frames > 0 && !B.frames) return detect_invalid(fn, "null frames");
  if (B.channels != 1 && B.channels != 3 && B.channels != 4) return detect_invalid(fn, "channels must be 1, 3 or 4");
  if (channel < 0 || channel >= B.channels) return detect_invalid(fn, "channel out of range");
  if (threshold < 0 || threshold > 255) return detect_invalid(fn, "threshold must be in 0..255");
  return SBA_OK;
}

// the size limit (`why_limit` ends its text), the device
static int frame_limit_invalid(const char* fn, int device, int32_t height, int32_t width, const char* why_limit) {
  if (height > 16384 || width > 16384) {
    g_last_error = std::string(fn) + ": width and height are limited to 16384" + why_limit;
    return SBA_ERR_UNSUPPORTED;
  }
  return check_device(device);
}

// the pitches, then frame_limit_invalid
static int frame_layout_invalid(const char* fn, const FrameBatch& B, const char* why_limit) {
  if (B.row_pitch < (int64_t)B.width * B.channels) return detect_invalid(fn, "row_pitch is smaller than width * channels");
  if ((__int128)B.height * B.row_pitch > B.frame_pitch) return detect_invalid(fn, "frame_pitch is smaller than height * row_pitch");
  if ((__int128)B.n_frames * B.frame_pitch > INT64_MAX) return detect_invalid(fn, "n_frames * frame_pitch overflows");
  return frame_limit_invalid(fn, B.device, B.height, B.width, why_limit);
}

// The pitches of an output of n_frames frames of `rows` rows of `row_bytes` bytes.  Each entry point words the first two
// texts in its own terms: `row_text` in full, `rows_text` is what it calls the rows; `overflow_text` as well where it differs.
static int out_pitch_invalid(const char* fn, int64_t n_frames, int64_t rows, int64_t row_bytes, const FrameOut& out, const char* row_text,
                             const char* rows_text, const char* overflow_text = "n_frames * out_frame_pitch overflows") {
  if (out.row_pitch < row_bytes) return detect_invalid(fn, row_text);
  if ((__int128)rows * out.row_pitch > out.frame_pitch)
    return detect_invalid(fn, (std::string("out_frame_pitch is smaller than ") + rows_text + " * out_row_pitch").c_str());
  if ((__int128)n_frames * out.frame_pitch > INT64_MAX) return detect_invalid(fn, overflow_text);
  return SBA_OK;
}

// The weights of a grey value from `channels` channels: all zero means OpenCV's for B, G, R, and they are filled in.
// `one_channel_text` is what the entry point says to a batch that has one channel only.
static int gray_weights_invalid(const char* fn, int32_t channels, int32_t (&gray_w)[3], const char* one_channel_text) {
  if (channels == 1) return detect_invalid(fn, one_channel_text);
  if (gray_w[0] == 0 && gray_w[1] == 0 && gray_w[2] == 0) { gray_w[0] = 3735; gray_w[1] = 19235; gray_w[2] = 9798; }
  if (gray_w[0] < 0 || gray_w[1] < 0 || gray_w[2] < 0) return detect_invalid(fn, "a gray weight is negative");
  if ((int64_t)gray_w[0] + gray_w[1] + gray_w[2] != 1 << 15) return detect_invalid(fn, "the gray weights must sum to 2^15");
  return SBA_OK;
}

// What the three calls that resample through a lens share of their options, in the order they report it.  The border is one
// value for interleaved frames and three for YUV planes: the caller says whether it is in range and what to say if not.
// `nothing_asked`: there are frames, and neither an output nor a diagnostic to write.
static int resample_invalid(const char* fn, int32_t out_height, int32_t out_width, int32_t interpolation, bool border_ok,
                            const char* border_text, bool nothing_asked) {
  if (out_height < 0 || out_height > 16384 || out_width < 0 || out_width > 16384) return detect_invalid(fn, "the output size must be in 0..16384");
  if (interpolation != 0 && interpolation != 1) return detect_invalid(fn, "interpolation must be 0 (bilinear) or 1 (nearest)");
  if (!border_ok) return detect_invalid(fn, border_text);
  if (nothing_asked) return detect_invalid(fn, "null out and no diagnostic asked for");
  return SBA_OK;
}

// A set of YUV 4:2:0 planes of `width` x `height` luma samples, read or written; `side` ("src", "out") opens the text of a call
// that has two sets and is empty for one that has one
static int yuv_planes_invalid(const char* fn, const char* side, const sba_yuv_planes& p, int64_t n_frames, int32_t height, int32_t width) {
  auto invalid = [&](const char* what) { return detect_invalid(fn, (*side ? std::string(side) + ": " + what : std::string(what)).c_str()); };
  if (n_frames > 0 && (!p.y || !p.u || !p.v)) return invalid("null plane");
  if (p.c_step != 1 && p.c_step != 2) return invalid("c_step must be 1 (planar) or 2 (interleaved)");
  const int64_t cw = ((int64_t)width + 1) / 2, ch = ((int64_t)height + 1) / 2;
  if (p.y_row_pitch < width) return invalid("y_row_pitch is smaller than width");
  if ((__int128)height * p.y_row_pitch > p.y_frame_pitch) return invalid("y_frame_pitch is smaller than height * y_row_pitch");
  if (cw > 0 && p.c_row_pitch < p.c_step * (cw - 1) + 1) return invalid("c_row_pitch is smaller than c_step * ((width + 1) / 2 - 1) + 1");
  if (p.c_row_pitch < 0 || (__int128)ch * p.c_row_pitch > p.c_frame_pitch) return invalid("c_frame_pitch is smaller than ((height + 1) / 2) * c_row_pitch");
  if ((__int128)n_frames * p.y_frame_pitch > INT64_MAX || (__int128)n_frames * p.c_frame_pitch > INT64_MAX)
    return invalid("n_frames * a frame pitch overflows");
  return SBA_OK;
}

// The lens and the new camera matrix of the two undistortions
static int lens_invalid(const char* fn, const sba_lens* lens, const double* new_k) {
  if (!lens || !new_k) return detect_invalid(fn, "null lens or new_k");
  const double lv[9] = {lens->fx, lens->fy, lens->cx, lens->cy, lens->k1, lens->k2, lens->p1, lens->p2, lens->k3};
  for (double v : lv) if (!std::isfinite(v)) return detect_invalid(fn, "a lens value is not finite");
  for (int k = 0; k < 4; ++k) if (!std::isfinite(new_k[k])) return detect_invalid(fn, "a new_k value is not finite");
  if (!(lens->fx > 0.0) || !(lens->fy > 0.0) || !(new_k[0] > 0.0) || !(new_k[1] > 0.0)) return detect_invalid(fn, "a focal length is not > 0");
  return SBA_OK;
}

int sba_detect_dots(int device, const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels,
                    int64_t row_pitch, int64_t frame_pitch, const sba_dot_opts* opts, uint64_t* sums, int32_t* box, double* centroid,
                    int32_t* status) {
  const char* fn = "sba_detect_dots";
  sba_dot_opts o{};
  o.channel = 1; o.threshold = 50;
  if (opts) o = *opts;
  const FrameBatch B{device, frames, n_frames, height, width, channels, row_pitch, frame_pitch};
  int rc = frame_args_invalid(fn, B, o.channel, o.threshold);
  if (rc) return rc;
  if (o.min_area < 0 || o.max_area < 0 || o.max_extent < 0) return detect_invalid(fn, "negative area or extent limit");
  // up to 16384 x 16384 every sum fits 64 bits: the largest a frame could ask for, sum w x^2 <= 255 * 16384 * 16384^3 / 3 = 6.1e18
  // < 2^64 = 1.8e19 (the sums actually returned are far smaller: sba_detect.hpp)
  rc = frame_layout_invalid(fn, B, " (the bound under which every sum fits 64 bits)");
  if (rc || n_frames == 0) return rc;
  return guarded(nullptr, [&] { return sba_detect::dot_call(B, o, sums, box, centroid, status); });
}

int sba_detect_blobs(int device, const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels,
                     int64_t row_pitch, int64_t frame_pitch, const sba_blob_opts* opts, int32_t* n_components, uint64_t* blobs,
                     int32_t* accepted, double* centroid, int32_t* status, uint8_t* mask_out, int32_t* labels_out) {
  const char* fn = "sba_detect_blobs";
  sba_blob_opts o{};
  o.channel = 1; o.threshold = 70; o.dilate_radius = 1; o.close_radius = 4;
  if (opts) o = *opts;
  const FrameBatch B{device, frames, n_frames, height, width, channels, row_pitch, frame_pitch};
  int rc = frame_args_invalid(fn, B, o.channel, o.threshold);
  if (rc) return rc;
  if (o.dilate_radius < 0 || o.dilate_radius > 8 || o.close_radius < 0 || o.close_radius > 8) return detect_invalid(fn, "a radius must be in 0..8");
  if (o.max_blobs < 0 || o.max_blobs > 64) return detect_invalid(fn, "max_blobs must be in 0..64");
  if (o.min_area < 0 || o.max_area < 0 || o.max_centre_dist < 0) return detect_invalid(fn, "negative area or distance limit");
  // up to 16384 x 16384 a pixel's index y W + x fits the 32-bit labels, every sum 64 bits
  rc = frame_layout_invalid(fn, B, "");
  if (rc || n_frames == 0) return rc;
  return guarded(nullptr, [&] { return sba_detect::blob_call(B, o, n_components, blobs, accepted, centroid, status, mask_out, labels_out); });
}

// sba_undistort_frames and sba_warp_frames: the same call but for the model behind the lens -- `model` is new_k, or (warp) the
// nine values of the matrix, which takes new_k's place
static int lens_frames(const char* fn, bool warp, const FrameBatch& B, const sba_lens* lens, const double* model, int32_t out_height,
                       int32_t out_width, const FrameOut& out, const sba_undistort_opts* opts, uint8_t* flags_out, int32_t* map_out) {
  sba_undistort_opts o{};
  if (opts) o = *opts;
  static const double unit_k[4] = {1.0, 1.0, 0.0, 0.0};
  int rc = frame_args_invalid(fn, B, 0, 0);
  if (!rc) rc = lens_invalid(fn, lens, warp ? unit_k : model);
  if (rc) return rc;
  if (warp) {
    if (!model) return detect_invalid(fn, "null m");
    for (int k = 0; k < 9; ++k) if (!std::isfinite(model[k])) return detect_invalid(fn, "a value of m is not finite");
  }
  rc = resample_invalid(fn, out_height, out_width, o.interpolation, o.border_value >= 0 && o.border_value <= 255,
                        "border_value must be in 0..255", !out.out && B.n_frames > 0 && !flags_out && !map_out);
  if (rc) return rc;
  if (out.out) rc = out_pitch_invalid(fn, B.n_frames, out_height, (int64_t)out_width * B.channels, out,
                                      "out_row_pitch is smaller than out_width * channels", "out_height");
  if (!rc) rc = frame_layout_invalid(fn, B, "");
  if (rc) return rc;
  return guarded(nullptr, [&] {
    return warp ? sba_detect::warp_call(B, *lens, model, out_height, out_width, out, o, flags_out, map_out)
                : sba_detect::undistort_call(B, *lens, model, out_height, out_width, out, o, flags_out, map_out);
  });
}

int sba_undistort_frames(int device, const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels,
                         int64_t row_pitch, int64_t frame_pitch, const sba_lens* lens, const double* new_k, int32_t out_height,
                         int32_t out_width, int64_t out_row_pitch, int64_t out_frame_pitch, const sba_undistort_opts* opts, uint8_t* out,
                         uint8_t* flags_out, int32_t* map_out) {
  return lens_frames("sba_undistort_frames", false, {device, frames, n_frames, height, width, channels, row_pitch, frame_pitch}, lens, new_k,
                     out_height, out_width, {out, out_row_pitch, out_frame_pitch}, opts, flags_out, map_out);
}

int sba_warp_frames(int device, const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels,
                    int64_t row_pitch, int64_t frame_pitch, const sba_lens* lens, const double* m, int32_t out_height, int32_t out_width,
                    int64_t out_row_pitch, int64_t out_frame_pitch, const sba_undistort_opts* opts, uint8_t* out, uint8_t* flags_out,
                    int32_t* map_out) {
  return lens_frames("sba_warp_frames", true, {device, frames, n_frames, height, width, channels, row_pitch, frame_pitch}, lens, m, out_height,
                     out_width, {out, out_row_pitch, out_frame_pitch}, opts, flags_out, map_out);
}

int sba_background_accumulate(int device, const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels,
                              int64_t row_pitch, int64_t frame_pitch, const sba_background_accumulate_opts* opts, const uint8_t* use,
                              uint32_t* sum, uint64_t* sumsq, uint32_t* hot, uint8_t* vmax, uint64_t* n_used) {
  const char* fn = "sba_background_accumulate";
  sba_background_accumulate_opts o{};
  o.channel = 1; o.threshold = 50;
  if (opts) o = *opts;
  const FrameBatch B{device, frames, n_frames, height, width, channels, row_pitch, frame_pitch};
  int rc = frame_args_invalid(fn, B, o.channel, o.threshold);
  if (rc) return rc;
  // 255 * 2^24 < 2^32: below it `sum` cannot overflow
  if ((o.accumulate && n_used ? *n_used : 0) + (uint64_t)n_frames > ((uint64_t)1 << 24)) {
    g_last_error = std::string(fn) + ": more than 2^24 frames in all (the bound under which the 32-bit sum cannot overflow)";
    return SBA_ERR_UNSUPPORTED;
  }
  rc = frame_layout_invalid(fn, B, "");
  if (rc) return rc;
  return guarded(nullptr, [&] { return sba_detect::bg_accumulate_call(B, o, use, sum, sumsq, hot, vmax, n_used); });
}

int sba_background_suppress(int device, const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels,
                            int64_t row_pitch, int64_t frame_pitch, const uint8_t* level, const uint8_t* mask, int64_t out_row_pitch,
                            int64_t out_frame_pitch, const sba_background_suppress_opts* opts, uint8_t* out) {
  const char* fn = "sba_background_suppress";
  sba_background_suppress_opts o{};
  o.channel = 1;
  if (opts) o = *opts;
  const FrameBatch B{device, frames, n_frames, height, width, channels, row_pitch, frame_pitch};
  const FrameOut O{out, out_row_pitch, out_frame_pitch};
  int rc = frame_args_invalid(fn, B, o.channel, 0);
  if (rc) return rc;
  if (o.mode != SBA_BG_GATE && o.mode != SBA_BG_SUBTRACT) return detect_invalid(fn, "mode must be 0 (gate) or 1 (subtract)");
  if (!out && n_frames > 0) return detect_invalid(fn, "null out");
  rc = out_pitch_invalid(fn, n_frames, height, width, O, "out_row_pitch is smaller than width", "height");
  if (!rc) rc = frame_layout_invalid(fn, B, "");
  if (rc || n_frames == 0) return rc;
  return guarded(nullptr, [&] { return sba_detect::bg_suppress_call(B, level, mask, O, o); });
}

int sba_convert_frames(int device, const uint8_t* y, const uint8_t* u, const uint8_t* v, int64_t n_frames, int32_t height, int32_t width,
                       int64_t y_row_pitch, int64_t y_frame_pitch, int64_t c_row_pitch, int64_t c_frame_pitch, int32_t c_step,
                       const sba_yuv_matrix* matrix, int64_t out_row_pitch, int64_t out_frame_pitch, const sba_convert_opts* opts,
                       uint8_t* out) {
  const char* fn = "sba_convert_frames";
  sba_convert_opts o{};
  if (opts) o = *opts;
  sba_yuv_matrix m{16, 1220542, 1673527, -409993, -852492, 2116026};      // OpenCV's cvtColor(COLOR_YUV2BGR_NV12 / _I420)
  if (matrix) m = *matrix;
  if (n_frames < 0 || height < 0 || width < 0) return detect_invalid(fn, "negative size");
  if (n_frames > 0 && !out) return detect_invalid(fn, "null out");
  if (o.out_format < SBA_PIX_BGR || o.out_format > SBA_PIX_R) return detect_invalid(fn, "unknown out_format");
  {   // every sum of the rule fits 32 bits: 255 |cy| + 128 (|a| + |b|) + 2^19 < 2^31 for each output row
    auto mag = [](int32_t c) { return c < 0 ? -(int64_t)c : (int64_t)c; };
    const int64_t rows[3] = {mag(m.cvr), mag(m.cug) + mag(m.cvg), mag(m.cub)};
    if (m.y_offset < 0 || m.y_offset > 255) return detect_invalid(fn, "matrix: y_offset must be in 0..255");
    for (int64_t ab : rows)
      if (255 * mag(m.cy) + 128 * ab + ((int64_t)1 << 19) >= ((int64_t)1 << 31))
        return detect_invalid(fn, "matrix: 255 |cy| + 128 (|a| + |b|) + 2^19 must stay below 2^31 for every output row");
  }
  const int64_t px = o.out_format <= SBA_PIX_RGB ? 3 : o.out_format <= SBA_PIX_RGBA ? 4 : 1;
  const sba_yuv_planes src{const_cast<uint8_t*>(y), const_cast<uint8_t*>(u), const_cast<uint8_t*>(v), y_row_pitch, y_frame_pitch, c_row_pitch,
                           c_frame_pitch, c_step, 0};
  const FrameOut O{out, out_row_pitch, out_frame_pitch};
  int rc = yuv_planes_invalid(fn, "", src, n_frames, height, width);
  if (!rc) rc = out_pitch_invalid(fn, n_frames, height, width * px, O, "out_row_pitch is smaller than width * bytes of a pixel", "height",
                                  "n_frames * a frame pitch overflows");
  if (!rc) rc = frame_limit_invalid(fn, device, height, width, "");
  if (rc || n_frames == 0) return rc;
  return guarded(nullptr, [&] { return sba_detect::convert_call(device, src, n_frames, height, width, m, O, o); });
}

int sba_resize_frames(int device, const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels,
                      int64_t row_pitch, int64_t frame_pitch, int32_t fx, int32_t fy, int64_t out_row_pitch, int64_t out_frame_pitch,
                      const sba_resize_opts* opts, uint8_t* out) {
  const char* fn = "sba_resize_frames";
  sba_resize_opts o{};
  if (opts) o = *opts;
  const FrameBatch B{device, frames, n_frames, height, width, channels, row_pitch, frame_pitch};
  const FrameOut O{out, out_row_pitch, out_frame_pitch};
  int rc = frame_args_invalid(fn, B, 0, 0);
  if (rc) return rc;
  if (fx < 1 || fx > 16 || fy < 1 || fy > 16) return detect_invalid(fn, "fx and fy must be in 1..16");
  if (n_frames > 0 && (fx > width || fy > height)) return detect_invalid(fn, "a factor is larger than the frame: the output would have no pixels");
  if (o.gray && (rc = gray_weights_invalid(fn, channels, o.gray_w, "gray needs 3 or 4 channels"))) return rc;
  if (!out && n_frames > 0) return detect_invalid(fn, "null out");
  rc = out_pitch_invalid(fn, n_frames, height / fy, (int64_t)(width / fx) * (o.gray ? 1 : channels), O,
                         "out_row_pitch is smaller than (width / fx) times the bytes of an output pixel", "(height / fy)");
  if (!rc) rc = frame_layout_invalid(fn, B, "");
  if (rc || n_frames == 0) return rc;
  return guarded(nullptr, [&] { return sba_detect::resize_call(B, fx, fy, O, o); });
}

int sba_frames_to_yuv(int device, const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels,
                      int64_t row_pitch, int64_t frame_pitch, uint8_t* y, uint8_t* u, uint8_t* v, int64_t y_row_pitch, int64_t y_frame_pitch,
                      int64_t c_row_pitch, int64_t c_frame_pitch, int32_t c_step, const sba_rgb_matrix* matrix, const sba_to_yuv_opts* opts) {
  const char* fn = "sba_frames_to_yuv";
  sba_to_yuv_opts o{};
  if (opts) o = *opts;
  sba_rgb_matrix m{16, 269484, 528482, 102760, -155188, -305135, 460324, 460324, -385875, -74448};   // OpenCV's cvtColor(COLOR_BGR2YUV_I420)
  if (matrix) m = *matrix;
  const FrameBatch B{device, frames, n_frames, height, width, channels, row_pitch, frame_pitch};
  int rc = frame_args_invalid(fn, B, 0, 0);
  if (rc) return rc;
  if (o.in_format < SBA_PIX_BGR || o.in_format > SBA_PIX_RGBA) return detect_invalid(fn, "in_format must be BGR, RGB, BGRA or RGBA");
  if (channels != 1 && channels != (o.in_format <= SBA_PIX_RGB ? 3 : 4)) return detect_invalid(fn, "in_format does not have `channels` bytes per pixel");
  if (o.chroma != SBA_CHROMA_NEAREST && o.chroma != SBA_CHROMA_AVERAGE) return detect_invalid(fn, "chroma must be 0 (nearest) or 1 (average)");
  {   // every sum of the rule fits 32 bits: 255 (|a| + |b| + |c|) < 2^28 for each row (the derivation is in the header)
    auto mag = [](int32_t c) { return c < 0 ? -(int64_t)c : (int64_t)c; };
    const int64_t rows[3] = {mag(m.cry) + mag(m.cgy) + mag(m.cby), mag(m.cru) + mag(m.cgu) + mag(m.cbu), mag(m.crv) + mag(m.cgv) + mag(m.cbv)};
    if (m.y_offset < 0 || m.y_offset > 255) return detect_invalid(fn, "matrix: y_offset must be in 0..255");
    for (int64_t abc : rows)
      if (255 * abc >= ((int64_t)1 << 28)) return detect_invalid(fn, "matrix: 255 (|a| + |b| + |c|) must stay below 2^28 for every row");
  }
  const sba_yuv_planes dst{y, u, v, y_row_pitch, y_frame_pitch, c_row_pitch, c_frame_pitch, c_step, 0};
  rc = yuv_planes_invalid(fn, "", dst, n_frames, height, width);
  if (!rc) rc = frame_layout_invalid(fn, B, "");
  if (rc || n_frames == 0) return rc;
  return guarded(nullptr, [&] { return sba_detect::to_yuv_call(B, dst, m, o); });
}

int sba_undistort_yuv(int device, const sba_yuv_planes* src, int64_t n_frames, int32_t height, int32_t width, const sba_lens* lens,
                      const double* new_k, int32_t out_height, int32_t out_width, const sba_yuv_planes* out,
                      const sba_undistort_yuv_opts* opts, uint8_t* flags_out, int32_t* map_out) {
  const char* fn = "sba_undistort_yuv";
  sba_undistort_yuv_opts o{};
  if (opts) o = *opts;
  if (n_frames < 0 || height < 0 || width < 0) return detect_invalid(fn, "negative size");
  if (!src) return detect_invalid(fn, "null src");
  int rc = yuv_planes_invalid(fn, "src", *src, n_frames, height, width);
  if (!rc) rc = lens_invalid(fn, lens, new_k);
  if (rc) return rc;
  auto in_range = [](int32_t b) { return b >= 0 && b <= 255; };
  rc = resample_invalid(fn, out_height, out_width, o.interpolation, in_range(o.border_y) && in_range(o.border_u) && in_range(o.border_v),
                        "border_y, border_u and border_v must be in 0..255", !out && n_frames > 0 && !flags_out && !map_out);
  if (rc) return rc;
  if (out) rc = yuv_planes_invalid(fn, "out", *out, n_frames, out_height, out_width);
  if (!rc) rc = frame_limit_invalid(fn, device, height, width, "");
  if (rc) return rc;
  return guarded(nullptr, [&] {
    return sba_detect::undistort_yuv_call(device, *src, n_frames, height, width, *lens, new_k, out_height, out_width, out, o, flags_out, map_out);
  });
}

int sba_frame_histograms(int device, const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels,
                         int64_t row_pitch, int64_t frame_pitch, const sba_hist_opts* opts, uint32_t* hist, uint64_t* total) {
  const char* fn = "sba_frame_histograms";
  sba_hist_opts o{};
  o.channel = 1;
  if (opts) o = *opts;
  const FrameBatch B{device, frames, n_frames, height, width, channels, row_pitch, frame_pitch};
  int rc = frame_args_invalid(fn, B, o.channel, 0);
  // up to 16384 x 16384 a frame's count fits 32 bits: at most 2^28 pixels fall into one bin
  if (!rc) rc = frame_layout_invalid(fn, B, " (the bound under which a count fits 32 bits)");
  if (rc || n_frames == 0 || (!hist && !total)) return rc;
  return guarded(nullptr, [&] { return sba_detect::hist_call(B, o, hist, total); });
}

int sba_refine_corners(int device, const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels,
                       int64_t row_pitch, int64_t frame_pitch, const int64_t* corner_start, const double* corners,
                       const sba_corner_opts* opts, const double* weights, double* refined, int32_t* status, int32_t* iterations,
                       double* tensor) {
  const char* fn = "sba_refine_corners";
  sba_corner_opts o{};
  o.eps = 1e-5; o.channel = channels == 1 ? 0 : -1; o.win_x = o.win_y = 3; o.zero_x = o.zero_y = -1; o.max_iter = 200;   // the reference's call
  if (opts) o = *opts;
  const FrameBatch B{device, frames, n_frames, height, width, channels, row_pitch, frame_pitch};
  int rc = frame_args_invalid(fn, B, o.channel == -1 ? 0 : o.channel, 0);
  if (rc) return rc;
  if (o.channel == -1 && (rc = gray_weights_invalid(fn, channels, o.gray_w, "channel -1 (gray) needs 3 or 4 channels"))) return rc;
  if (o.win_x < 1 || o.win_x > 15 || o.win_y < 1 || o.win_y > 15) return detect_invalid(fn, "win_x and win_y must be in 1..15");
  if (o.max_iter < 1 || o.max_iter > 10000) return detect_invalid(fn, "max_iter must be in 1..10000");
  if (!(o.eps >= 0.0)) return detect_invalid(fn, "eps must be >= 0");
  if (n_frames > 0 && !corner_start) return detect_invalid(fn, "null corner_start");
  int64_t n = 0;
  if (n_frames > 0) {
    if (corner_start[0] != 0) return detect_invalid(fn, "corner_start[0] must be 0");
    for (int64_t f = 0; f < n_frames; ++f)
      if (corner_start[f + 1] < corner_start[f]) return detect_invalid(fn, "corner_start must not decrease");
    n = corner_start[n_frames];
  }
  if (weights)
    for (int64_t i = 0; i < (int64_t)(2 * o.win_y + 1) * (2 * o.win_x + 1); ++i)
      if (!std::isfinite(weights[i]) || weights[i] < 0.0) return detect_invalid(fn, "a weight is negative or not finite");
  if (n > 0 && (!corners || !refined || !status)) return detect_invalid(fn, "null corners, refined or status");
  if (n > 0 && (height == 0 || width == 0)) return detect_invalid(fn, "corners in frames without pixels");
  rc = frame_layout_invalid(fn, B, "");
  if (rc || n == 0) return rc;
  return guarded(nullptr, [&] { return sba_detect::corners_call(B, corner_start, corners, o, weights, refined, status, iterations, tensor); });
}

int sba_adaptive_threshold(int device, const uint8_t* frames, int64_t n_frames, int32_t height, int32_t width, int32_t channels,
                           int64_t row_pitch, int64_t frame_pitch, const sba_adaptive_opts* opts, int64_t out_row_pitch,
                           int64_t out_frame_pitch, int64_t out_window_pitch, uint8_t* out, uint8_t* mean_out) {
  const char* fn = "sba_adaptive_threshold";
  sba_adaptive_opts o{};
  o.n_windows = 3; o.block[0] = 3; o.block[1] = 13; o.block[2] = 23; o.delta[0] = o.delta[1] = o.delta[2] = 7;   // detectMarkers' call
  o.invert = 1; o.channel = channels == 1 ? 0 : -1;
  if (opts) o = *opts;
  const FrameBatch B{device, frames, n_frames, height, width, channels, row_pitch, frame_pitch};
  const FrameOut O{out, out_row_pitch, out_frame_pitch};
  int rc = frame_args_invalid(fn, B, o.channel == -1 ? 0 : o.channel, 0);
  if (rc) return rc;
  if (o.n_windows < 1 || o.n_windows > 4) return detect_invalid(fn, "n_windows must be in 1..4");
  for (int k = 0; k < o.n_windows; ++k) {
    if (o.block[k] < 3 || o.block[k] > 127 || o.block[k] % 2 == 0) return detect_invalid(fn, "a block must be odd and in 3..127");
    if (o.delta[k] < -256 || o.delta[k] > 256) return detect_invalid(fn, "a delta must be in -256..256");
  }
  if (o.invert != 0 && o.invert != 1) return detect_invalid(fn, "invert must be 0 (binary) or 1 (binary, inverted)");
  if (o.max_value < 0 || o.max_value > 255) return detect_invalid(fn, "max_value must be in 0..255");
  if (o.channel == -1 && (rc = gray_weights_invalid(fn, channels, o.gray_w, "channel -1 (gray) needs 3 or 4 channels"))) return rc;
  rc = out_pitch_invalid(fn, n_frames, height, width, O, "out_row_pitch is smaller than width", "height");
  if (rc) return rc;
  if (o.n_windows > 1 && (__int128)n_frames * out_frame_pitch > out_window_pitch)
    return detect_invalid(fn, "out_window_pitch is smaller than n_frames * out_frame_pitch");
  if ((__int128)o.n_windows * out_window_pitch > INT64_MAX) return detect_invalid(fn, "n_windows * out_window_pitch overflows");
  if (!out && !mean_out && n_frames > 0) return detect_invalid(fn, "null out and null mean_out");
  rc = frame_layout_invalid(fn, B, "");
  if (rc || n_frames == 0) return rc;
  return guarded(nullptr, [&] { return sba_detect::adaptive_call(B, o, O, out_window_pitch, mean_out); });
}

int sba_time_kernel(sba_handle* h, const char* name, int32_t reps, double* mean_us_out) {
  if (!h || !name || !mean_us_out) return SBA_ERR_INVALID;
  return guarded(h, [&] { return h->eng->time_kernel(name, reps, mean_us_out); });
}

}  // extern "C"
