// sba_layout.hpp -- the engine's observation layout built on the device from the caller's raw arrays (sba_upload_ex).
// Input: uv float64 M x 2, cam_idx / pt_idx int64 M, optional weights float64 M, as the caller holds them.  Output: the buffers
// the host pass of Engine::upload fills -- point-major copies (uv_pm, ci_pm, pi_pm, w_pm, pt_start), the camera-major copy
// (uv_cm, pi_cm, w_cm, the per-camera starts), the one-group visibility mask and the permutation pm position -> caller's index.
//
// The order is the host pass's:  C <= GROUP_CAMS: by (point, camera);  C > GROUP_CAMS: by point, stable in the caller's index;
// camera-major: the pm list, stable by camera.  Every position is a function of the input alone: atomics are integer counters
// whose RESULT is order independent (degrees, histogram bins, min / max / or), and the one place where arrival order shows -- the
// cursor scatter into a point's segment -- is followed by a ranking pass on the total order (camera, caller's index).
// No workgroup waits for another one: every dependency is a kernel boundary.
//
// The head record (LAY_HEAD ints behind pt_start[N]) carries the facts the host needs, so that ONE copy brings back the point
// starts, the camera starts and the flags.  A list the device cannot lay out (index out of range, a point with more than
// PM_BLOCK observations) turns every later kernel of the pass into a no-op; the host then runs its own pass, which owns the
// error texts.
#pragma once
#include "sba_kernels.hpp"

namespace SBA_NS {

enum { LAY_BAD = 0,        // smallest observation index with a camera / point index out of range, INT_MAX when there is none
       LAY_UNSORTED = 1,   // some observation has a smaller point index than its predecessor
       LAY_CAM_UNSORTED = 2,   // ... the same point and a camera index that does not grow
       LAY_DUP = 3,        // C <= GROUP_CAMS: a (point, camera) pair occurs twice (found by the ranking pass)
       LAY_MAXDEG = 4,     // largest number of observations of one point
       LAY_CAM_START = 16, // C + 1 camera starts of the camera-major copy
       LAY_HEAD = 16 + 129 + 15 };
constexpr int LAY_TILE = 1024;      // elements of a scan tile: 256 threads x one 16-byte access
constexpr int LAY_MAX_CAMS = 128;   // bins of the camera histogram (= MAX_CAMS of the engine)

__device__ __forceinline__ bool lay_declined(const int* head) { return head[LAY_BAD] != 0x7fffffff || head[LAY_MAXDEG] > PM_BLOCK; }
__device__ __forceinline__ bool lay_identity(const int* head, int C) {
  return !head[LAY_UNSORTED] && (!head[LAY_CAM_UNSORTED] || C > GROUP_CAMS);
}

__device__ __forceinline__ bool lay_flag_down(const int* flag) {
  return __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
}

// exclusive scan of one value per thread over a 256-thread workgroup; *total = the workgroup's sum (s_w: 4 ints of LDS)
__device__ __forceinline__ int lay_block_scan(int v, int* s_w, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  __syncthreads();                    // s_w may still be read from an earlier call
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) { const int x = s_w[w]; if (w < wave) base += x; tot += x; }
  *total = tot;
  return base + inc - v;
}

__device__ __forceinline__ int4 lay_load4(const int* __restrict__ in, int i, int n) {
  if (i + 3 < n) return *reinterpret_cast<const int4*>(in + i);
  int4 v = make_int4(0, 0, 0, 0);
  if (i < n) v.x = in[i];
  if (i + 1 < n) v.y = in[i + 1];
  if (i + 2 < n) v.z = in[i + 2];
  return v;
}

// ------------------------------------------------------------------ exclusive scan of n ints: tile sums, scan of the sums, apply
// (in and out are 16-byte aligned; out holds n + 1 entries when want_total, the last one the grand total)
__global__ __launch_bounds__(256) void k_lay_tile_sums(const int* __restrict__ in, int n, int* __restrict__ tile_sum,
                                                       int* __restrict__ max_out /* or NULL */) {
  __shared__ int s_sum[4], s_max[4];
  const int i = blockIdx.x * LAY_TILE + threadIdx.x * 4;
  const int4 v = lay_load4(in, i, n);
  int s = v.x + v.y + v.z + v.w, m = max(max(v.x, v.y), max(v.z, v.w));
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { s += __shfl_xor(s, d, 64); m = max(m, __shfl_xor(m, d, 64)); }
  if ((threadIdx.x & 63) == 0) { s_sum[threadIdx.x >> 6] = s; s_max[threadIdx.x >> 6] = m; }
  __syncthreads();
  if (threadIdx.x == 0) {
    tile_sum[blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    if (max_out) atomicMax(max_out, max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3])));
  }
}

// one workgroup: tile_sum[0 .. ntiles) -> exclusive offsets in place
__global__ __launch_bounds__(256) void k_lay_scan_tiles(int* __restrict__ tile_sum, int ntiles) {
  __shared__ int s_w[4];
  int carry = 0;
  for (int b = 0; b < ntiles; b += 256) {
    const int i = b + threadIdx.x;
    const int v = i < ntiles ? tile_sum[i] : 0;
    int tot;
    const int ex = lay_block_scan(v, s_w, &tot);
    if (i < ntiles) tile_sum[i] = carry + ex;
    carry += tot;
  }
}

__global__ __launch_bounds__(256) void k_lay_scan_apply(const int* __restrict__ in, int n, const int* __restrict__ tile_off,
                                                        int* __restrict__ out, int want_total) {
  __shared__ int s_w[4];
  const int i = blockIdx.x * LAY_TILE + threadIdx.x * 4;
  const int4 v = lay_load4(in, i, n);
  int tot;
  const int ex = tile_off[blockIdx.x] + lay_block_scan(v.x + v.y + v.z + v.w, s_w, &tot);
  const int4 o = make_int4(ex, ex + v.x, ex + v.x + v.y, ex + v.x + v.y + v.z);
  if (i + 3 < n) *reinterpret_cast<int4*>(out + i) = o;
  else {
    if (i < n) out[i] = o.x;
    if (i + 1 < n) out[i + 1] = o.y;
    if (i + 2 < n) out[i + 2] = o.z;
  }
  if (want_total && i < n && i + 4 >= n) out[n] = o.w + v.w;      // the thread that holds element n - 1 (its tail entries are 0)
}

// ------------------------------------------------------------------ pass 1: validation, order tests, degrees
__global__ void k_lay_init(int* __restrict__ deg, int* __restrict__ cursor, int N, int* __restrict__ head) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < N) { deg[p] = 0; cursor[p] = 0; }
  if (p < LAY_HEAD) head[p] = p == LAY_BAD ? 0x7fffffff : 0;
}

__global__ __launch_bounds__(256) void k_lay_scan_obs(const long long* __restrict__ ci, const long long* __restrict__ pi, int M, int C,
                                                      int N, int* __restrict__ deg, int* __restrict__ head) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  const long long c = ci[i], p = pi[i];
  if (c < 0 || c >= C || p < 0 || p >= N) { atomicMin(&head[LAY_BAD], i); return; }
  if (i) {
    const long long pp = pi[i - 1];
    // (a shuffled list fails these tests in half of its lanes: the flag is read first, so that only the lanes that arrive before it
    //  is up queue on its address)
    if (p < pp) { if (lay_flag_down(&head[LAY_UNSORTED])) atomicOr(&head[LAY_UNSORTED], 1); }
    else if (p == pp && c <= ci[i - 1]) { if (lay_flag_down(&head[LAY_CAM_UNSORTED])) atomicOr(&head[LAY_CAM_UNSORTED], 1); }
  }
  atomicAdd(&deg[(int)p], 1);
}

// ------------------------------------------------------------------ pass 3: placement (skipped on the device when the list is in order)
// key = (camera, caller's index) for one camera group, (0, caller's index) otherwise: a total order, so the rank is unique
__global__ __launch_bounds__(256) void k_lay_scatter(const int* __restrict__ head, const long long* __restrict__ ci,
                                                     const long long* __restrict__ pi, int M, int C, const int* __restrict__ pt_start,
                                                     int* __restrict__ cursor, unsigned long long* __restrict__ keys) {
  if (lay_declined(head) || lay_identity(head, C)) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  const int p = (int)pi[i];
  const int pos = pt_start[p] + atomicAdd(&cursor[p], 1);
  const unsigned long long cam = C <= GROUP_CAMS ? (unsigned long long)ci[i] : 0ull;
  if (pos >= 0 && pos < M) keys[pos] = (cam << 32) | (unsigned)i;
}

__global__ __launch_bounds__(256) void k_lay_rank(int* __restrict__ head, const unsigned long long* __restrict__ keys,
                                                  const long long* __restrict__ pi, int M, int C, const int* __restrict__ pt_start,
                                                  int* __restrict__ perm) {
  if (lay_declined(head) || lay_identity(head, C)) return;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= M) return;
  const unsigned long long key = keys[k];
  const int i = (int)(unsigned)(key & 0xffffffffull);
  const int p = (int)pi[i];
  const int a = pt_start[p], b = pt_start[p + 1];       // b - a <= PM_BLOCK: the pass has not declined
  int r = 0;
  bool dup = false;
  for (int j = a; j < b; ++j) {
    const unsigned long long kj = keys[j];
    r += kj < key ? 1 : 0;
    dup = dup || (j != k && (kj >> 32) == (key >> 32));
  }
  if (a + r < M) perm[a + r] = i;
  if (dup && C <= GROUP_CAMS && lay_flag_down(&head[LAY_DUP])) atomicOr(&head[LAY_DUP], 1);
}

// ------------------------------------------------------------------ pass 4: point-major arrays through the permutation, narrowed
template <typename T>
__global__ __launch_bounds__(256) void k_lay_gather(const int* __restrict__ head, const int* __restrict__ perm,
                                                    const double2* __restrict__ uv, const long long* __restrict__ ci,
                                                    const long long* __restrict__ pi, const double* __restrict__ w, int M, int C,
                                                    typename Vec2<T>::type* __restrict__ uv_pm, int32_t* __restrict__ ci_pm,
                                                    int32_t* __restrict__ pi_pm, T* __restrict__ w_pm) {
  if (lay_declined(head)) return;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= M) return;
  const int i = lay_identity(head, C) ? k : perm[k];
  if (i < 0 || i >= M) return;
  const double2 m = uv[i];
  typename Vec2<T>::type v; v.x = (T)m.x; v.y = (T)m.y;
  uv_pm[k] = v; ci_pm[k] = (int32_t)ci[i]; pi_pm[k] = (int32_t)pi[i];
  if (w) w_pm[k] = (T)w[i];
}

// one camera group: which cameras see point p
__global__ void k_lay_mask(const int* __restrict__ head, const int32_t* __restrict__ ci_pm, const int* __restrict__ pt_start, int N,
                           uint16_t* __restrict__ vis_mask) {
  if (lay_declined(head)) return;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= N) return;
  unsigned m = 0;
  for (int o = pt_start[p]; o < pt_start[p + 1]; ++o) m |= 1u << (ci_pm[o] & 15);
  vis_mask[p] = (uint16_t)m;
}

// ------------------------------------------------------------------ pass 5: camera-major copy, a stable one-digit counting sort
// counts[c * nwg + g] = observations of camera c in the 256 pm positions of workgroup g; its exclusive scan in that order is
// where workgroup g's first observation of camera c goes
__global__ __launch_bounds__(256) void k_lay_cm_count(const int* __restrict__ head, const int32_t* __restrict__ ci_pm, int M, int C,
                                                      int nwg, int* __restrict__ counts) {
  __shared__ int s_hist[LAY_MAX_CAMS];
  const bool off = lay_declined(head);
  for (int c = threadIdx.x; c < LAY_MAX_CAMS; c += 256) s_hist[c] = 0;
  __syncthreads();
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (!off && k < M) {
    const int c = ci_pm[k];
    if (c >= 0 && c < C) atomicAdd(&s_hist[c], 1);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) counts[(size_t)c * nwg + blockIdx.x] = s_hist[c];
}

__global__ void k_lay_cm_starts(const int* __restrict__ offs, int M, int C, int nwg, int* __restrict__ head) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c <= C) head[LAY_CAM_START + c] = c < C ? offs[(size_t)c * nwg] : M;
}

template <typename T>
__global__ __launch_bounds__(256) void k_lay_cm_scatter(const int* __restrict__ head, const int32_t* __restrict__ ci_pm,
                                                        const int32_t* __restrict__ pi_pm, const typename Vec2<T>::type* __restrict__ uv_pm,
                                                        const T* __restrict__ w_pm, int M, int C, int nwg, const int* __restrict__ offs,
                                                        typename Vec2<T>::type* __restrict__ uv_cm, int32_t* __restrict__ pi_cm,
                                                        T* __restrict__ w_cm) {
  __shared__ int s_cnt[4][LAY_MAX_CAMS];
  if (lay_declined(head)) return;                              // (uniform over the grid)
  for (int c = threadIdx.x; c < 4 * LAY_MAX_CAMS; c += 256) (&s_cnt[0][0])[c] = 0;
  __syncthreads();
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int cam = k < M ? ci_pm[k] : -1;
  if (cam >= C) cam = -1;
  const bool valid = cam >= 0;
  // rank among the wave's lanes of the same camera: one ballot per camera present in the wave
  unsigned long long pending = __ballot(valid);
  int rank = 0;
  while (pending) {
    const int leader = __ffsll((long long)pending) - 1;
    const int c0 = __shfl(cam, leader, 64);
    const bool mine = valid && cam == c0;
    const unsigned long long m = __ballot(mine);
    if (mine) rank = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == leader) s_cnt[wave][c0] = __popcll(m);
    pending &= ~m;
  }
  __syncthreads();
  if (!valid) return;
  int d = offs[(size_t)cam * nwg + blockIdx.x] + rank;
  for (int w = 0; w < wave; ++w) d += s_cnt[w][cam];
  if (d < 0 || d >= M) return;
  uv_cm[d] = uv_pm[k]; pi_cm[d] = pi_pm[k];
  if (w_pm) w_cm[d] = w_pm[k];
}

}  // namespace SBA_NS
