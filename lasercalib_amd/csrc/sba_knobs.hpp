// sba_knobs.hpp -- the environment switches of the engine, read once per handle.  A header of its own so that the pure planning
// code (plan_route in sba_engine.hpp, plan_chol in sba_chol_solve.hpp) can take them without including the engine.
#pragma once
#include "sba_common.hpp"
#include "sba_chol_blocked.hpp"
#include "sba_ipc.hpp"

namespace SBA_NS {

// ============================================================================================== switches
// The environment switches ("Environment switches"), read once per handle, at sba_create: a process may change
// them between two handles.  read_knobs is the only place in the engine that looks at the environment.
struct Knobs {
  bool no_dense = false;             // SBA_NO_DENSE: no lane = (point, camera) kernels (fused Schur, dense back substitution)
  bool no_fused64 = false;           // SBA_NO_FUSED64: fp64 keeps the pair kernels (no k_schur_fused_f64 / k_schur_fused_wide_f64)
  bool no_wide = false;              // SBA_NO_WIDE: no wide kernels for 17+ cameras (pair kernels, point-aligned back substitution)
  bool wide_pw2 = false;             // SBA_WIDE_PW2: two points per producer wave in the wide kernels, never three
  // one-workgroup factorisations of up to 256 unknowns: the right-looking all-in-LDS kernel up to 176 (k_cholesky_blocked),
  // the left-looking kernel with the factor on chip above that (k_cholesky_ll, sba_chol_ll.hpp: 17..23 cameras).
  // SBA_CHOL=ll: the left-looking kernel for every size up to 256; SBA_CHOL=blocked: never (the streamed kernel above 176) -- A/B runs, tests
  bool chol_ll = true, chol_ll_all = false;
  // fp32 engine, up to 176 unknowns: factor on f32 lanes (v_mfma_f32_16x16x4, f32 pivot chain) and repeat in f64 only when that is
  // refused -- a non-positive pivot, or one below chol_f32_tau times its diagonal entry (2^-23: the entry's own rounding noise).
  // SBA_CHOL_F32=0 keeps the f64 factorisation of rounds 1-3; SBA_CHOL_F32_TAU overrides the threshold.
  bool chol_f32 = true;
  float chol_f32_tau = 1.1920929e-7f;
  bool chol_big_dag = true;          // SBA_CHOL_BIG=launches keeps one launch per block column (rounds 1-3)
  // systems larger than this take the multi-workgroup factorisation (sba_chol_big.hpp); up to CS_MAX_NB * CB = 512 unknowns the
  // streamed one-workgroup kernel could run too, but it only wins below ~210 (measured at 50k points, fp32: 17 cameras 379 vs 388 us
  // per iteration, 20: 417 vs 409, 24: 487 vs 454, 32: 647 vs 515).  SBA_CHOL_BIG_MIN_N moves it (diagnostics).
  int chol_big_min_n = 209;
  bool decide_kernel = false;        // SBA_DECIDE_KERNEL=1 keeps the separate k_decide launch (A/B measurements)
  bool schur_scan = false;           // SBA_SCHUR_SCAN=1: several groups, producers scan the point's observations (no k_group_index)
  bool no_bf3_pairs = false;         // SBA_NO_BF3_PAIRS=1: f32-input MFMA kernels for every group pair (A/B, equivalence test)
  // The lane = (point, camera) kernels (fused linearise + Schur, wide, dense back substitution) cost the DENSE instruction count
  // whatever the visibility; below this fraction of the N x C slots filled the observation-driven three-pass path would take over.
  // Rounds 1-3 set it to 0.35 unmeasured.  Round 4 measured it (profiles/r4_visibility_sweep*.txt: 16 / 17 cameras, 10k and 50k points,
  // fill 0.14 .. 0.45, both dtypes): the one-launch kernels win at EVERY fill a rig can have (two views of 16 cameras = 0.13: fp32
  // 78 vs 102 us per iteration at 16 x 10k, 111 vs 163 at 17 x 10k, 118 vs 155 at 16 x 50k; fp64 212 vs 245) because the three-pass
  // path is bound by its launches and pair kernels, not by the observation count.  So the threshold is 0; SBA_DENSE_MIN_VIS restores one.
  double dense_min_vis = 0.0;
  // instruments (stderr)
  bool schur_debug = false;          // SBA_SCHUR_DEBUG=k: stamps of the k-th fused Schur launch (k >= 2: one with the decision in its prologue)
  int schur_debug_skip = 0;
  bool chol_debug = false;           // SBA_CHOL_DEBUG: stamps of the first factorisation
  bool upload_debug = false;         // SBA_UPLOAD_DEBUG: phase times of sba_upload
  bool solve_debug = false;          // SBA_SOLVE_DEBUG: host-side phase times of every sba_solve
  // one-shot exchange (sba_ipc.hpp)
  long long ipc_timeout_ticks = IPC_TIMEOUT_TICKS;   // SBA_IPC_TIMEOUT_S: how long a gate waits for a peer (100 MHz ticks)
  bool ipc_allow_cached = false;     // SBA_IPC_ALLOW_CACHED=1: an exchange area in cached memory when uncached is not available
};

inline Knobs read_knobs() {
  Knobs k;
  auto set = [](const char* name) { return getenv(name) != nullptr; };
  k.no_dense = set("SBA_NO_DENSE");
  k.no_fused64 = set("SBA_NO_FUSED64");
  k.no_wide = set("SBA_NO_WIDE");
  k.wide_pw2 = set("SBA_WIDE_PW2");
  k.decide_kernel = set("SBA_DECIDE_KERNEL");
  k.schur_scan = set("SBA_SCHUR_SCAN");
  k.no_bf3_pairs = set("SBA_NO_BF3_PAIRS");
  k.chol_debug = set("SBA_CHOL_DEBUG");
  k.upload_debug = set("SBA_UPLOAD_DEBUG");
  k.solve_debug = set("SBA_SOLVE_DEBUG");
  k.ipc_allow_cached = set("SBA_IPC_ALLOW_CACHED");
  if (const char* e = getenv("SBA_CHOL")) { k.chol_ll = std::string(e) != "blocked"; k.chol_ll_all = std::string(e) == "ll"; }
  if (const char* e = getenv("SBA_CHOL_F32")) k.chol_f32 = atoi(e) != 0;
  if (const char* e = getenv("SBA_CHOL_F32_TAU")) { char* end = nullptr; const double v = strtod(e, &end); if (end != e && v >= 0 && v < 1) k.chol_f32_tau = (float)v; }
  if (const char* e = getenv("SBA_CHOL_BIG")) k.chol_big_dag = std::string(e) != "launches";
  if (const char* e = getenv("SBA_CHOL_BIG_MIN_N")) {
    char* end = nullptr;
    const long v = strtol(e, &end, 10);
    if (end != e && *end == 0 && v >= 0) k.chol_big_min_n = (int)std::min<long>(v, CS_MAX_NB * CB);
  }
  if (const char* e = getenv("SBA_DENSE_MIN_VIS")) { char* end = nullptr; const double v = strtod(e, &end); if (end != e && v >= 0 && v <= 1) k.dense_min_vis = v; }
  if (const char* e = getenv("SBA_SCHUR_DEBUG")) { k.schur_debug = true; k.schur_debug_skip = std::max(0, atoi(e) - 1); }
  if (const char* e = getenv("SBA_IPC_TIMEOUT_S")) {
    char* end = nullptr;
    const double sec = strtod(e, &end);
    if (end != e && sec > 0 && sec < 3600) k.ipc_timeout_ticks = (long long)(sec * 1e8);
  }
  return k;
}

}  // namespace SBA_NS
