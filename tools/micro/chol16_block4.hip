// Micro-benchmark: the f32 diagonal-tile factorisation of k_cholesky_blocked, one wave, 16 x 16 tile -> Linv^T.
//   0  as shipped before round 6: chol16_wave_t<float> -- a row per lane, one v_readlane_b32 per (pivot, column) pair (120 + 16 per tile)
//   1  4-pivot groups (lasercalib_amd/csrc/sba_chol16_block4.hpp): tile and identity in the f32 MFMA accumulator layout, scalar chain
//      inside the 4 x 4 diagonal blocks only, rank-4 updates on v_mfma_f32_16x16x4_f32; strips to MFMA operands by an LDS round trip
//   2  the same with the strips moved by v_permlane16_swap / v_permlane32_swap (the very routine the kernel calls)
// Prints cycles per tile (LDS -> registers -> LDS, growth test included), |A Ainv - I| with Ainv = Linv^T Linv formed in f64 on the
// host, and how many of 16 tiles with one negative diagonal entry (one per pivot position) each variant refuses.
//   hipcc -O3 -fno-slp-vectorize --offload-arch=gfx950 -o chol16_block4 tools/micro/chol16_block4.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cmath>
#include <vector>
#include "../../lasercalib_amd/csrc/sba_chol16_block4.hpp"
constexpr int CB = 16, LD = 20;

__device__ __forceinline__ float bcast(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }
// variant 0: the shipped loop (chol16_wave_t<float, false>)
__device__ __forceinline__ bool chol16_rows(float* __restrict__ blk, const float* __restrict__ a0, float tau) {
  const int lane = threadIdx.x & 63;
  const int i = lane & 15;
  const bool ident = lane >= 16;
  float a[CB];
#pragma unroll
  for (int j = 0; j < CB; ++j) { const float v = blk[i * LD + j]; a[j] = ident ? ((j == i) ? 1.0f : 0.0f) : v; }
  float dg = blk[i * LD + i];
  __builtin_amdgcn_wave_barrier();
  float akk = bcast(dg, 0);
  float piv = __builtin_amdgcn_rsqf(akk);
  float chk = piv;
#pragma unroll
  for (int k = 0; k < CB; ++k) {
    const float lik = a[k] * piv;
    a[k] = lik;
    if (k + 1 < CB) {
      dg = __builtin_fmaf(-lik, lik, dg);
      akk = bcast(dg, k + 1);
      piv = __builtin_amdgcn_rsqf(akk);
      chk += piv;
    }
#pragma unroll
    for (int j = k + 1; j < CB; ++j) a[j] -= lik * bcast(lik, j);
  }
  if (lane >= 16 && lane < 32) {
#pragma unroll
    for (int j = 0; j < CB; ++j) blk[i * LD + j] = a[j];
  }
  bool ok = isfinite(chk) && chk > 0.0f;
  if (a0) {
    __builtin_amdgcn_wave_barrier();
    const float li = blk[i * LD + i];
    const bool sunk = lane < 16 && !((1.0f / (li * li)) >= tau * a0[i]);
    ok = ok && !__any(sunk);
  }
  return ok;
}

// variant 1's operand move: the group's 16 lanes store their strip entries ([c][k]: V[k][c], then Z[k][c] 64 floats further) in the
// tile's own slot, whose entries are in registers by then, and every lane reads its operand back
struct LdsMove {
  template <int S>
  static __device__ __forceinline__ void run(float* blk, float v0, float v1, float v2, float v3, float z0, float z1, float z2, float z3,
                                             float& vb, float& zb) {
    static_assert(CB * LD >= 128, "2 x 4 x 16 floats of staging");
    const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
    float4* sv4 = reinterpret_cast<float4*>(blk);
    if (g == S) {
      sv4[c] = make_float4(v0, v1, v2, v3);
      sv4[16 + c] = make_float4(z0, z1, z2, z3);
    }
    __builtin_amdgcn_wave_barrier();
    vb = blk[4 * c + g]; zb = blk[64 + 4 * c + g];
    __builtin_amdgcn_wave_barrier();
  }
};

// (launch bounds of k_cholesky_blocked, though one wave is launched: with at most 256 registers per lane the compiler keeps the MFMA
//  accumulators in VGPRs, as in the kernel, instead of moving them through AGPRs)
template <int VAR>
__global__ __launch_bounds__(512) void k(const float* A, float* out, long long* cyc, int* okflag, int reps) {
  __shared__ __align__(16) float blk[CB * LD];
  __shared__ float a0[CB];
  const int lane = threadIdx.x & 63;
  long long total = 0;
  bool ok = true;
  for (int rep = 0; rep < reps; ++rep) {
    for (int t = lane; t < CB * CB; t += 64) blk[(t >> 4) * LD + (t & 15)] = A[t];
    if (lane < CB) a0[lane] = A[lane * CB + lane];
    __syncthreads();
    const long long t0 = clock64();
    if (VAR == 0) ok = chol16_rows(blk, a0, 1.2e-7f);
    else if (VAR == 1) ok = sba_block4::chol16_block4_f32<LD, LdsMove>(blk, a0, 1.2e-7f);
    else ok = sba_block4::chol16_block4_f32<LD>(blk, a0, 1.2e-7f);
    __syncthreads();
    total += clock64() - t0;
  }
  for (int t = lane; t < CB * CB; t += 64) out[t] = blk[(t >> 4) * LD + (t & 15)];
  if (lane == 0) { cyc[0] = total / reps; okflag[0] = ok ? 1 : 0; }
}

int main() {
  std::vector<float> A(256), L(256);
  float *dA, *dO; long long* dC; int* dK;
  (void)hipMalloc(&dA, 1024); (void)hipMalloc(&dO, 1024); (void)hipMalloc(&dC, 8); (void)hipMalloc(&dK, 4);
  auto launch = [&](int var, int reps, long long& c, int& ok) {
    (void)hipMemcpy(dA, A.data(), 1024, hipMemcpyHostToDevice);
    if (var == 0) hipLaunchKernelGGL((k<0>), dim3(1), dim3(64), 0, 0, dA, dO, dC, dK, reps);
    else if (var == 1) hipLaunchKernelGGL((k<1>), dim3(1), dim3(64), 0, 0, dA, dO, dC, dK, reps);
    else hipLaunchKernelGGL((k<2>), dim3(1), dim3(64), 0, 0, dA, dO, dC, dK, reps);
    (void)hipMemcpy(&c, dC, 8, hipMemcpyDeviceToHost);
    (void)hipMemcpy(&ok, dK, 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(L.data(), dO, 1024, hipMemcpyDeviceToHost);
    return hipDeviceSynchronize() == hipSuccess;
  };
  auto fill = [&](double diag, double scale) {
    for (int i = 0; i < 16; ++i) for (int j = 0; j < 16; ++j) A[i * 16 + j] = (float)(((i == j) ? diag : 0.0) + scale / (1 + i + j));
  };
  for (int pass = 0; pass < 2; ++pass) {          // a well-conditioned tile and one with cond ~ 1e4
    if (pass == 0) fill(20.0, 1.0); else fill(3e-4, 1.0);
    long long cyc[3] = {0, 0, 0};
    for (int var = 0; var < 3; ++var) {
      int ok = 0;
      if (!launch(var, 20, cyc[var], ok)) { printf("variant %d: launch failed\n", var); return 1; }
      double err = 0;       // out = Linv^T; A (Linv^T Linv) = I
      for (int r = 0; r < 16; ++r) for (int c2 = 0; c2 < 16; ++c2) {
        double s = 0;
        for (int m = 0; m < 16; ++m) { double ainv = 0; for (int q = 0; q < 16; ++q) ainv += (double)L[m * 16 + q] * L[c2 * 16 + q]; s += (double)A[r * 16 + m] * ainv; }
        err = fmax(err, fabs(s - (r == c2 ? 1.0 : 0.0)));
      }
      double low = 0;       // Linv^T is upper triangular: whatever is left of the diagonal must be exactly zero
      for (int r = 0; r < 16; ++r) for (int c2 = 0; c2 < r; ++c2) low = fmax(low, fabs((double)L[r * 16 + c2]));
      printf("tile %d variant %d: %lld cycles per tile (%.0f per pivot), accepted %d, |A Ainv - I| = %.2e, max below the diagonal %.1e\n",
             pass, var, cyc[var], cyc[var] / 16.0, ok, err, low);
    }
    for (int var = 1; var < 3; ++var)
      printf("tile %d: variant %d / variant 0 = %.3f (%.1f %% fewer cycles)\n", pass, var, (double)cyc[var] / cyc[0], 100.0 * (1.0 - (double)cyc[var] / cyc[0]));
  }
  // refusal: a diagonal entry that is negative, at every pivot position (every variant must refuse all 16), and row p made a copy of
  // row p - 1 up to one rounding unit of the diagonal entry: the pivot then IS the rounding noise of its row, some of these come out
  // positive and above 2^-23 of the entry and pass in every variant alike (printed to compare the variants, not as a bar)
  for (int var = 0; var < 3; ++var) {
    int refused_neg = 0, refused_sunk = 0;
    for (int p = 0; p < 16; ++p) {
      long long c; int ok;
      fill(20.0, 1.0);
      A[p * 16 + p] = -1.0f;
      if (!launch(var, 1, c, ok)) return 1;
      refused_neg += ok ? 0 : 1;
      if (p == 0) continue;
      fill(20.0, 1.0);
      for (int j = 0; j < 16; ++j) { A[p * 16 + j] = A[(p - 1) * 16 + j]; }
      for (int j = 0; j < 16; ++j) { A[j * 16 + p] = A[p * 16 + j]; }
      A[p * 16 + p] = A[(p - 1) * 16 + (p - 1)] * (1.0f + 1e-7f);
      A[p * 16 + p - 1] = A[(p - 1) * 16 + p] = A[(p - 1) * 16 + (p - 1)];
      if (!launch(var, 1, c, ok)) return 1;
      refused_sunk += ok ? 0 : 1;
    }
    printf("variant %d: refused %d of 16 tiles with a negative diagonal entry, %d of 15 tiles whose row p repeats row p - 1 (pivot = rounding noise)\n",
           var, refused_neg, refused_sunk);
  }
  return 0;
}
