// sba_corners.hpp -- sba_refine_corners (include/sba_hip.h): sub-pixel refinement of corners in a batch of frames.  Stands in
// for cv.cornerSubPix as scripts/charuco_intrinsics.py:39-44 of the reference calls it per marker corner; the rule per corner --
// a float64 bilinear patch, central differences, five weighted sums in a fixed two-level order, one correctly rounded
// division, the stopping rules and status bits -- is written out in the header and evaluated here one IEEE operation per
// operation of the rule (no contraction).
//
// One kernel, k_refine_corners; a workgroup is ONE wave, so nothing a corner does waits for another wave.  A corner belongs to
// a GROUP of G = 4, 8, 16 or 32 neighbouring lanes, the smallest power of two that holds the 2 wy + 1 rows of its window (8 for
// the reference's 3 x 3 half sizes: 8 corners a wave).  All lanes of a group carry the corner's state (position, status,
// iteration count) and compute the scalar part redundantly, so nothing is broadcast.  An iteration has four phases with the
// wave's LDS as the only hand-over (wave_lds_sync, no workgroup barrier):
//   A  the (2 wy + 4) x (2 wx + 4) taps under the patch, ONE read per tap and iteration, spread flat over the group's lanes;
//      a tap is a byte (the selected channel, or the grey value of sba_resize_frames), clamped to the frame, kept as a byte
//   B  the (2 wy + 3) x (2 wx + 3) samples S as float64, flat over the lanes, four taps each out of LDS
//   C  a lane per window row: the five sums of its row from left to right
//   D  every lane of the group adds the row totals from top to bottom, solves the 2 x 2 system and moves the corner
// The wave loops while any of its corners runs; a group whose corner has stopped idles for as long as the slowest corner of
// ITS wave needs, never longer.  Corners are dealt to waves in the order given, so the corners of one frame -- which tend to
// need similar counts -- share waves.
//
// What bounds it: every iteration reads (2 wy + 4)(2 wx + 4) bytes per corner (100 at the default) out of frames that lie in
// L2 after the first one, and does 9 float64 operations per sample and 19 per window position in a serial chain of iterations
// whose length is that of the slowest corner of the wave: the kernel is latency-bound, not memory-bound.
// The weights (2 wy + 1)(2 wx + 1) doubles are staged into LDS once per wave.
#pragma once
#include "sba_frames.hpp"

namespace sba_detect {

constexpr int CN_MAX_WIN = 15;
constexpr int CN_CONVERGED = 1, CN_MAX_ITER = 2, CN_SINGULAR = 4, CN_LEFT_IMAGE = 8, CN_RESTORED = 16, CN_INVALID = 32;

struct CornerParams {
  const uint8_t* frames;                     // of the chunk's first frame
  int64_t row_pitch, frame_pitch;
  int32_t height, width, channels, channel;  // channel < 0: the grey value
  int32_t w0, w1, w2;                        // grey weights
  int32_t wx, wy, max_iter;
  int32_t log2_g;                            // lanes of a group = 1 << log2_g >= 2 wy + 1
  uint32_t magic_s, magic_t;                 // n / (2 wx + 3) = n * magic_s >> 16 for n < (2 wy + 3)(2 wx + 3); _t: 2 wx + 4
  double eps2;                               // eps * eps, formed on the host
  const double* weights;                     // (2 wy + 1)(2 wx + 1)
  const double* xy;                          // the chunk's corners
  const int32_t* frame;                      // frame of a corner, counted from the chunk's first
  int64_t n;
  double* refined;
  int32_t* status;
  int32_t* iterations;                       // or null
  double* tensor;                            // or null
};

// ceil(2^16 / d): n * magic >> 16 == n / d for every n < 2^16 / d, which covers n < 34 * 34 for d <= 34
inline uint32_t cn_magic(int d) { return (65536u + (uint32_t)d - 1u) / (uint32_t)d; }

// doubles and bytes of LDS a group needs; the wave's layout is [weights][doubles of group 0][group 1]...[bytes of group 0]...
__host__ __device__ inline int cn_group_doubles(int wx, int wy) { return (2 * wy + 3) * (2 * wx + 3) + 5 * (2 * wy + 1); }
__host__ __device__ inline int cn_group_bytes(int wx, int wy) { return ((2 * wy + 4) * (2 * wx + 4) + 7) & ~7; }
inline int cn_log2_group(int wy) { int l = 2; while ((1 << l) < 2 * wy + 1) ++l; return l; }
inline size_t cn_lds_bytes(int wx, int wy) {
  const int per_wave = 64 >> cn_log2_group(wy);
  return sizeof(double) * ((2 * wy + 1) * (2 * wx + 1) + (size_t)per_wave * cn_group_doubles(wx, wy)) + (size_t)per_wave * cn_group_bytes(wx, wy);
}

// T(u, v) of the rule; 0 <= u < width, 0 <= v < height
__device__ __forceinline__ uint32_t cn_tap(const CornerParams& P, const uint8_t* __restrict__ fp, int u, int v) {
  const uint8_t* __restrict__ p = fp + ((int64_t)v * P.row_pitch + (int64_t)u * P.channels);
  if (P.channel >= 0) return p[P.channel];
  return ((uint32_t)p[0] * (uint32_t)P.w0 + (uint32_t)p[1] * (uint32_t)P.w1 + (uint32_t)p[2] * (uint32_t)P.w2 + (1u << 14)) >> 15;
}

// grid: ceil(n / corners of a wave) workgroups of 64 threads; dynamic LDS cn_lds_bytes
__global__ void __launch_bounds__(64) k_refine_corners(const CornerParams P) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) unsigned char cn_lds[];
  const int lane = threadIdx.x, G = 1 << P.log2_g, grp = lane >> P.log2_g, g = lane & (G - 1), per_wave = 64 >> P.log2_g;
  const int wx = P.wx, wy = P.wy, W = P.width, H = P.height;
  const int nwx = 2 * wx + 1, nwy = 2 * wy + 1, nsx = nwx + 2, nsy = nwy + 2, ntx = nsx + 1, nty = nsy + 1;
  double* wts = reinterpret_cast<double*>(cn_lds);
  double* S = wts + nwy * nwx + grp * cn_group_doubles(wx, wy);
  double* rows = S + nsy * nsx;
  uint8_t* taps = cn_lds + sizeof(double) * (nwy * nwx + per_wave * cn_group_doubles(wx, wy)) + grp * cn_group_bytes(wx, wy);

  const int64_t k = (int64_t)blockIdx.x * per_wave + grp;
  const bool mine = k < P.n;
  double x = 0.0, y = 0.0, ta = 0.0, tb = 0.0, tc = 0.0;
  int st = 0, it = 0;
  const uint8_t* __restrict__ fp = P.frames;
  bool active = mine;
  if (mine) {
    x = P.xy[2 * k]; y = P.xy[2 * k + 1];
    fp = P.frames + (int64_t)P.frame[k] * P.frame_pitch;
    if (!(fabs(x) < 32768.0 && fabs(y) < 32768.0)) { st = CN_INVALID; active = false; }      // false for NaN and infinities too
  }
  double cx = x, cy = y;
  for (int i = lane; i < nwy * nwx; i += 64) wts[i] = P.weights[i];
  wave_lds_sync();

  while (__any(active)) {
    const double fx = floor(cx), fy = floor(cy);
    const int ix = (int)fx, iy = (int)fy;
    const double ax = cx - fx, ay = cy - fy;
    if (active) {                                                          // A: the taps, read once
      for (int t = g; t < nty * ntx; t += G) {
        const int r = (int)((uint32_t)t * P.magic_t >> 16), c = t - r * ntx;
        const int u = min(max(ix - (wx + 1) + c, 0), W - 1), v = min(max(iy - (wy + 1) + r, 0), H - 1);
        taps[t] = (uint8_t)cn_tap(P, fp, u, v);
      }
    }
    wave_lds_sync();
    if (active) {                                                          // B: the samples
      const double w = 1.0 - ax, h = 1.0 - ay;
      for (int s = g; s < nsy * nsx; s += G) {
        const int r = (int)((uint32_t)s * P.magic_s >> 16), c = s - r * nsx;
        const uint8_t* t0 = taps + r * ntx + c;
        const double top = w * (double)t0[0] + ax * (double)t0[1];
        const double bot = w * (double)t0[ntx] + ax * (double)t0[ntx + 1];
        S[s] = h * top + ay * bot;
      }
    }
    wave_lds_sync();
    if (active && g < nwy) {                                               // C: window row i = g - wy, left to right
      const double* Sm = S + g * nsx;                                      // sample rows i - 1, i, i + 1
      const double* S0 = Sm + nsx;
      const double* Sp = S0 + nsx;
      const double* m = wts + g * nwx;
      const double di = (double)(g - wy);
      double a = 0.0, b = 0.0, c = 0.0, b1 = 0.0, b2 = 0.0;
      for (int jj = 0; jj < nwx; ++jj) {                                   // window column j = jj - wx is sample column jj + 1
        const double dj = (double)(jj - wx);
        const double gx = S0[jj + 2] - S0[jj], gy = Sp[jj + 1] - Sm[jj + 1];
        const double gxx = (gx * gx) * m[jj], gxy = (gx * gy) * m[jj], gyy = (gy * gy) * m[jj];
        const double e1 = gxx * dj + gxy * di, e2 = gxy * dj + gyy * di;
        a = a + gxx; b = b + gxy; c = c + gyy; b1 = b1 + e1; b2 = b2 + e2;
      }
      rows[5 * g] = a; rows[5 * g + 1] = b; rows[5 * g + 2] = c; rows[5 * g + 3] = b1; rows[5 * g + 4] = b2;
    }
    wave_lds_sync();
    if (active) {                                                          // D: the totals top to bottom, the step
      double a = 0.0, b = 0.0, c = 0.0, b1 = 0.0, b2 = 0.0;
      for (int r = 0; r < nwy; ++r) {
        a = a + rows[5 * r]; b = b + rows[5 * r + 1]; c = c + rows[5 * r + 2]; b1 = b1 + rows[5 * r + 3]; b2 = b2 + rows[5 * r + 4];
      }
      ta = a; tb = b; tc = c;
      const double det = a * c - b * b;
      if (!(fabs(det) > 0x1p-104)) { st = CN_SINGULAR; active = false; }
      else {
        const double s = 1.0 / det;
        const double nx = (cx + (c * s) * b1) - (b * s) * b2;
        const double ny = (cy - (b * s) * b1) + (a * s) * b2;
        const double dx = nx - cx, dy = ny - cy;
        const double err = dx * dx + dy * dy;
        cx = nx; cy = ny; ++it;
        if (!(cx >= 0.0 && cx < (double)W && cy >= 0.0 && cy < (double)H)) { st = CN_LEFT_IMAGE; active = false; }
        else if (err <= P.eps2) { st = CN_CONVERGED; active = false; }
        else if (it == P.max_iter) { st = CN_MAX_ITER; active = false; }
      }
    }
  }

  if (mine && g == 0) {
    if (!(st & CN_INVALID) && (fabs(cx - x) > (double)wx || fabs(cy - y) > (double)wy)) { cx = x; cy = y; st |= CN_RESTORED; }
    P.refined[2 * k] = cx; P.refined[2 * k + 1] = cy;
    P.status[k] = st;
    if (P.iterations) P.iterations[k] = it;
    if (P.tensor) { P.tensor[3 * k] = ta; P.tensor[3 * k + 1] = tb; P.tensor[3 * k + 2] = tc; }
  }
}

// ------------------------------------------------------------------------------------------------ host side
// OpenCV's window: entry (i, j) = exp(-((i - wy) / wy)^2) * exp(-((j - wx) / wx)^2) in float64, the zero zone set to 0 when both
// of its half sizes are >= 0 and it is smaller than the window
inline std::vector<double> cn_window(int wx, int wy, int zx, int zy) {
  std::vector<double> m((size_t)(2 * wy + 1) * (2 * wx + 1));
  for (int i = 0; i <= 2 * wy; ++i) {
    const double yy = (double)(i - wy) / (double)wy, vy = std::exp(-(yy * yy));
    for (int j = 0; j <= 2 * wx; ++j) {
      const double xx = (double)(j - wx) / (double)wx;
      m[(size_t)i * (2 * wx + 1) + j] = vy * std::exp(-(xx * xx));
    }
  }
  if (zx >= 0 && zy >= 0 && zx < wx && zy < wy)
    for (int i = wy - zy; i <= wy + zy; ++i)
      for (int j = wx - zx; j <= wx + zx; ++j) m[(size_t)i * (2 * wx + 1) + j] = 0.0;
  return m;
}

// Arguments are checked by the caller (sba_api.hip): there are corners, the frames have pixels, the options are in range and
// the grey weights set.  Chunks of frames as hist_call; the launch of a chunk gets the corners of its frames, and the device
// buffers hold the corners of the largest chunk: they do not grow with n_frames.  Which chunk a corner passes through does not
// enter its arithmetic.
int corners_call(const FrameBatch& B, const int64_t* corner_start, const double* corners, const sba_corner_opts& o, const double* weights,
                 double* refined, int32_t* status, int32_t* iterations, double* tensor) {
  const int64_t n_frames = B.n_frames;
  HIPCHK(hipSetDevice(B.device));
  const bool on_device = o.frames_on_device != 0;
  const int64_t chunk = chunk_of(CHUNK_RECORDS, o.chunk_frames, B, on_device);
  int64_t most = 0;
  for (int64_t lo = 0; lo < n_frames; lo += chunk) most = std::max(most, corner_start[std::min(lo + chunk, n_frames)] - corner_start[lo]);

  const int wx = o.win_x, wy = o.win_y;
  const std::vector<double> window = weights ? std::vector<double>() : cn_window(wx, wy, o.zero_x, o.zero_y);
  const size_t n_w = (size_t)(2 * wy + 1) * (2 * wx + 1);
  DevBuf<double> d_w, d_xy, d_refined, d_tensor;
  DevBuf<int32_t> d_frame, d_status, d_iter;
  d_w.alloc(n_w);
  HIPCHK(hipMemcpy(d_w.p, weights ? weights : window.data(), sizeof(double) * n_w, hipMemcpyHostToDevice));
  d_xy.alloc((size_t)most * 2); d_refined.alloc((size_t)most * 2); d_frame.alloc((size_t)most); d_status.alloc((size_t)most);
  if (iterations) d_iter.alloc((size_t)most);
  if (tensor) d_tensor.alloc((size_t)most * 3);
  std::vector<int32_t> h_frame((size_t)most);

  CornerParams P{};
  P.height = B.height; P.width = B.width; P.channels = B.channels; P.channel = o.channel;
  P.w0 = o.gray_w[0]; P.w1 = o.gray_w[1]; P.w2 = o.gray_w[2];
  P.wx = wx; P.wy = wy; P.max_iter = o.max_iter; P.log2_g = cn_log2_group(wy);
  P.magic_s = cn_magic(2 * wx + 3); P.magic_t = cn_magic(2 * wx + 4);
  P.eps2 = o.eps * o.eps;
  P.weights = d_w.p; P.xy = d_xy.p; P.frame = d_frame.p;
  P.refined = d_refined.p; P.status = d_status.p; P.iterations = d_iter.p; P.tensor = d_tensor.p;
  const int per_wave = 64 >> P.log2_g;
  const size_t lds = cn_lds_bytes(wx, wy);

  const FramePlane plane = frame_plane(B);
  frames_in_chunks(
      &plane, 1, n_frames, on_device, chunk,
      [&](const FramePlane* c, int64_t lo, int64_t m, hipStream_t st) {
        const int64_t k0 = corner_start[lo], n = corner_start[lo + m] - k0;
        if (n == 0) return;
        for (int64_t f = 0; f < m; ++f)
          for (int64_t k = corner_start[lo + f]; k < corner_start[lo + f + 1]; ++k) h_frame[(size_t)(k - k0)] = (int32_t)f;
        P.frames = c->base; P.row_pitch = c->row_pitch; P.frame_pitch = c->frame_pitch; P.n = n;
        HIPCHK(hipMemcpyAsync(d_xy.p, corners + 2 * k0, sizeof(double) * 2 * n, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_frame.p, h_frame.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_refine_corners, dim3((unsigned)((n + per_wave - 1) / per_wave)), dim3(64), lds, st, P);
        HIPCHK(hipGetLastError());
      },
      [&](int64_t lo, int64_t m, hipStream_t st) {
        const int64_t k0 = corner_start[lo], n = corner_start[lo + m] - k0;
        if (n == 0) return;
        HIPCHK(hipMemcpyAsync(refined + 2 * k0, d_refined.p, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(status + k0, d_status.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        if (iterations) HIPCHK(hipMemcpyAsync(iterations + k0, d_iter.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        if (tensor) HIPCHK(hipMemcpyAsync(tensor + 3 * k0, d_tensor.p, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, st));
      });
  return SBA_OK;
}

}  // namespace sba_detect
