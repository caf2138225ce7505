// sba_chol16_block4.hpp -- Cholesky of one 16 x 16 f32 tile by one wave, in 4-pivot groups (round 6).
//
// chol16_wave_t<float> (sba_chol_blocked.hpp) holds a row per lane and so needs one scalar broadcast per (pivot k, column j > k) and one per pivot: 120 + 16 =
// 136 v_readlane_b32 on the serial chain of a tile.  Here the tile C and T (identity -> Linv) live in the accumulator layout of
// v_mfma_f32_16x16x4_f32 -- register rg of lane (g, c) = (lane >> 4, lane & 15) holds entry [4 g + rg][c] -- so the four rows of pivot
// group s are the four registers of lane group s, and per group:
//   chain   the 4 x 4 diagonal block (10 broadcasts) is factored by every lane alike on wave-uniform values: 4 v_rsq_f32
//   strips  V = L_ss^-1 C[4s .. 4s+3][:] and Z = L_ss^-1 T[4s .. 4s+3][:]: per lane a 4-term forward substitution with those uniform
//           coefficients (V[k][i] = L[i][4s + k]; Z = rows 4s .. 4s+3 of Linv, final)
//   update  C -= V^T V and T -= V^T Z on the rows behind the group: lane (k, i) needs V[k][i] and Z[k][i] as MFMA operands -- three
//           lane swaps each (SwapMove; an LDS round trip costs 70 - 230 cycles per tile more: variant 1 of tools/micro/chol16_block4.hip,
//           which passes its own Move) -- then two independent MFMAs.
// 40 v_readlane_b32 per tile (24 in-group (pivot, column) pairs instead of 120), three MFMA rounds (the last group has no rows behind it).  Only the lower triangle of the tile is read.
// The contract is chol16_wave_t's: Linv^T replaces the tile; false (wave-uniform) when a pivot is non-positive or non-finite, or
// (a0 given) when a pivot L_ii^2 has sunk below tau * a0[i].
// Needs nothing but HIP: tools/micro/chol16_block4.hip times this very routine.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace sba_block4 {

using acc4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ float rl(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }

// Strip entries to MFMA operands without LDS: lane group S holds v0 .. v3 (rows of V) and z0 .. z3 (rows of Z) of its column; on return
// lane (k, i) holds V[k][i] and Z[k][i].  With rows r0 .. r3 of 16 lanes, v_permlane16_swap_b32 a, b leaves a = [a.r0 b.r0 a.r2 b.r2] and
// b = [a.r1 b.r1 a.r3 b.r3]; v_permlane32_swap_b32 a, b leaves a = [a.r0 a.r1 b.r0 b.r1] and b = [a.r2 a.r3 b.r2 b.r3].  Swapping (v0, v1)
// and (v2, v3) puts row S of each pair into rows (0, 1) or (2, 3) of one of the two registers, the 32-lane swap joins the two pairs.
// The compiler inserts no wait states around these instructions (docs/EXPERIMENTS.md, round 2): two before (VALU write -> swap read),
// two between dependent swaps, two after (swap write -> VALU read), written out.  All 64 lanes must be active.
struct SwapMove {
template <int S>
static __device__ __forceinline__ void run(float*, float v0, float v1, float v2, float v3, float z0, float z1, float z2, float z3,
                                           float& vb, float& zb) {
  unsigned a = __float_as_uint(v0), b = __float_as_uint(v1), c = __float_as_uint(v2), d = __float_as_uint(v3);
  unsigned e = __float_as_uint(z0), f = __float_as_uint(z1), g = __float_as_uint(z2), h = __float_as_uint(z3);
  asm volatile("s_nop 1\n\t"
               "v_permlane16_swap_b32 %0, %1\n\t"
               "v_permlane16_swap_b32 %2, %3\n\t"
               "v_permlane16_swap_b32 %4, %5\n\t"
               "v_permlane16_swap_b32 %6, %7\n\t"
               "s_nop 1"
               : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h));
  unsigned x = (S & 1) ? b : a, y = (S & 1) ? d : c, zx = (S & 1) ? f : e, zy = (S & 1) ? h : g;
  asm volatile("s_nop 1\n\t"
               "v_permlane32_swap_b32 %0, %1\n\t"
               "v_permlane32_swap_b32 %2, %3\n\t"
               "s_nop 1"
               : "+v"(x), "+v"(y), "+v"(zx), "+v"(zy));
  vb = __uint_as_float(S < 2 ? x : y);
  zb = __uint_as_float(S < 2 ? zx : zy);
}
};

// Move: how lane group s's strip entries become the MFMA operands of all lanes -- Move::run<s>(blk, v0 .. v3, z0 .. z3, vb, zb), called by
// all 64 lanes once the tile's entries are in registers (blk is free until the result is stored)
template <int LD, typename Move = SwapMove>
__device__ __forceinline__ bool chol16_block4_f32(float* __restrict__ blk, const float* __restrict__ a0, float tau) {
  const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  acc4 C, T;
#pragma unroll
  for (int rg = 0; rg < 4; ++rg) {
    const int r = 4 * g + rg;
    C[rg] = blk[max(r, c) * LD + min(r, c)];                 // (lower triangle only)
    T[rg] = (r == c) ? 1.0f : 0.0f;
  }
  __builtin_amdgcn_wave_barrier();
  float chk = 0.0f;
  float pv = 1.0f;                                           // 1 / L_cc of the lane's column index, for the growth test
  auto group = [&](auto sc) {                                // (the group index is a compile-time constant: lanes of v_readlane, swap pattern)
    constexpr int s = decltype(sc)::value;
    const int src = 20 * s;                                  // lane (s, 4 s): column 4 s + b of rows 4 s + a is register a of lane src + b
    float d00 = rl(C[0], src), d10 = rl(C[1], src), d20 = rl(C[2], src), d30 = rl(C[3], src);
    float d11 = rl(C[1], src + 1), d21 = rl(C[2], src + 1), d31 = rl(C[3], src + 1);
    float d22 = rl(C[2], src + 2), d32 = rl(C[3], src + 2);
    float d33 = rl(C[3], src + 3);
    // the in-group chain: wave-uniform values, the same instructions in every lane
    const float p0 = __builtin_amdgcn_rsqf(d00);
    const float l10 = d10 * p0, l20 = d20 * p0, l30 = d30 * p0;
    d11 = __builtin_fmaf(-l10, l10, d11);
    const float p1 = __builtin_amdgcn_rsqf(d11);
    d21 = __builtin_fmaf(-l20, l10, d21);
    d31 = __builtin_fmaf(-l30, l10, d31);
    d22 = __builtin_fmaf(-l20, l20, d22);
    d32 = __builtin_fmaf(-l30, l20, d32);
    d33 = __builtin_fmaf(-l30, l30, d33);
    const float l21 = d21 * p1, l31 = d31 * p1;
    d22 = __builtin_fmaf(-l21, l21, d22);
    const float p2 = __builtin_amdgcn_rsqf(d22);
    d32 = __builtin_fmaf(-l31, l21, d32);
    d33 = __builtin_fmaf(-l31, l31, d33);
    const float l32 = d32 * p2;
    d33 = __builtin_fmaf(-l32, l32, d33);
    const float p3 = __builtin_amdgcn_rsqf(d33);
    chk += (p0 + p1) + (p2 + p3);                            // a non-positive or non-finite pivot makes one of them NaN or infinite
    pv = (c == 4 * s) ? p0 : pv; pv = (c == 4 * s + 1) ? p1 : pv; pv = (c == 4 * s + 2) ? p2 : pv; pv = (c == 4 * s + 3) ? p3 : pv;
    // the strips: every lane solves with its own four registers, lane group s holds the rows that count
    const float z0 = T[0] * p0;
    const float z1 = __builtin_fmaf(-l10, z0, T[1]) * p1;
    const float z2 = __builtin_fmaf(-l21, z1, __builtin_fmaf(-l20, z0, T[2])) * p2;
    const float z3 = __builtin_fmaf(-l32, z2, __builtin_fmaf(-l31, z1, __builtin_fmaf(-l30, z0, T[3]))) * p3;
    if (g == s) { T[0] = z0; T[1] = z1; T[2] = z2; T[3] = z3; }
    if constexpr (s < 3) {
      const float v0 = C[0] * p0;
      const float v1 = __builtin_fmaf(-l10, v0, C[1]) * p1;
      const float v2 = __builtin_fmaf(-l21, v1, __builtin_fmaf(-l20, v0, C[2])) * p2;
      const float v3 = __builtin_fmaf(-l32, v2, __builtin_fmaf(-l31, v1, __builtin_fmaf(-l30, v0, C[3]))) * p3;
      float vb, zb;                                                  // V[g][c], Z[g][c]
      Move::template run<s>(blk, v0, v1, v2, v3, z0, z1, z2, z3, vb, zb);
      // rows up to the group's last are finished (T) or dead (C): their column of V^T is masked out of the A operand.  (The entries of V
      // left of the group are the rounding noise of eliminated columns: they only reach columns of C nobody reads again.)
      const float na = (c >= 4 * s + 4) ? -vb : 0.0f;
      C = __builtin_amdgcn_mfma_f32_16x16x4f32(na, vb, C, 0, 0, 0);
      T = __builtin_amdgcn_mfma_f32_16x16x4f32(na, zb, T, 0, 0, 0);
    }
  };
  group(std::integral_constant<int, 0>{});
  group(std::integral_constant<int, 1>{});
  group(std::integral_constant<int, 2>{});
  group(std::integral_constant<int, 3>{});
  // Linv^T[c][r] = Linv[r][c] = T[r][c]: the lane's four registers are four neighbours of row c
  if constexpr (LD % 4 == 0) {
    *reinterpret_cast<float4*>(blk + c * LD + 4 * g) = make_float4(T[0], T[1], T[2], T[3]);
  } else {
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) blk[c * LD + 4 * g + rg] = T[rg];
  }
  bool ok = isfinite(chk) && chk > 0.0f;
  if (a0) {                                                  // pivot growth test (wave-uniform pointer), chol16_wave_t's rule
    const bool sunk = lane < 16 && !((1.0f / (pv * pv)) >= tau * a0[c]);
    ok = ok && !__any(sunk);
  }
  return ok;
}

}  // namespace sba_block4
