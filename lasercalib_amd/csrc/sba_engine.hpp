// sba_engine.hpp -- the engine behind one sba_handle: device buffers, host-side layout, kernel launchers and the LM phases.
// Compiled once per camera model: SBA_NCP (11 = the reference's radial model, 13 = radial + tangential) selects the
// namespace (sba11 / sba13) all kernels live in; sba_engine_ncp11.hip / sba_engine_ncp13.hip are the two translation units.
#pragma once
#include "sba_common.hpp"
#include "sba_lm_kernels.hpp"
#include "sba_chol_blocked.hpp"
#include "sba_chol_ll.hpp"
#include "sba_chol_big.hpp"
#include "sba_sq_kernels.hpp"
#include "sba_schur_wide.hpp"
#include "sba_schur_f64.hpp"
#include "sba_ipc.hpp"
#include "sba_covariance.hpp"
#include "sba_triangulate.hpp"
#include "sba_unproject.hpp"
#include "sba_align.hpp"
#include "sba_reproj.hpp"
#include "sba_layout.hpp"
// (host side only; behind the kernels, whose order in the translation unit they leave alone)
#include "sba_knobs.hpp"
#include "sba_chol_solve.hpp"

namespace SBA_NS {
using namespace sba_host;

constexpr int MAX_CAMS = 128;        // sba_upload refuses larger rigs
// (the largest system, MAX_CAMS cameras of 13 parameters, fits the one-launch forms: k_chol_big_dag's block rows and the x of
//  k_chol_big_back_all in LDS)
static_assert(cholbig_npad(MAX_CAMS * 13) / BB <= CHOLDAG_MAX_NBR && (MAX_CAMS * 13 + BB - 1) / BB <= CHOLBIG_MAX_NBX, "large Cholesky sizes");

// ============================================================================================== routes
// What sba_upload knows about a problem when it picks the kernels
struct Layout {
  int C, N;
  int64_t M;
  bool dense, masked_ok, grp_indexed;
  int ngroups, npairs;
  int ncu;                           // compute units of the device
};

// What runs on a handle: every kernel choice that follows from its layout and its switches (plan_route)
struct Route {
  int ksplit = 1;                    // Schur launches: workgroups over the points per group pair (per slice for the wide kernels)
  bool fused_ok = false;             // the linearisation runs inside the Schur kernel (k_schur_fused_bf3 / _f64 / _wide / _wide_f64)
  bool fused_wide = false;           // ... k_schur_fused_wide(_f64): compact rows, one launch (implies fused_ok)
  bool fused_f64 = false;            // ... k_schur_fused_f64: fp64, one group, 11 parameters (sba_schur_f64.hpp)
  bool fused_masked = false;         // ... with the visibility mask
  bool lin_pts_ok = false;           // f64, one group: the point linearisation runs inside k_schur_sym (LIN)
  int wide_pw = 2;                   // wide kernels: points per producer wave, 3 (packed lanes, 12-point rounds) or 2
  int wide_ts = 1;                   // fp64 wide kernel: workgroups per slice (tile split, grid.y)
  bool dense_one_group = false;      // dense and <= 16 cameras: lane = (point, camera) kernels apply
  bool backsub_masked = false;       // sparse one-group rig dense enough for the lane = (point, camera) back substitution (visibility mask)
  bool backsub_wide = false;         // 17 .. 32 cameras: k_backsub_dense<T, 32>
  bool backsub_pack = false;         // ... three points per wave (17 .. 21 cameras): k_backsub_dense<T, 0>
  bool backsub_wave = false;         // 33 .. 128 cameras: k_backsub_dense<T, 64>
  int linp_lw = 0;                   // 24 .. 128 cameras with (point, camera) tables: k_linearize_points_wave<T, 32 / 64>; 0 = k_linearize_points
  int nlinp = 0;                     // ... its (persistent) workgroups = entries of cost_part / gmax_part
  int nbs_dense = 1;                 // workgroups of k_backsub_dense
  bool pairs_bf3 = false;            // several groups, fp32, indexed producers: the group pairs run on the bf16 pipe (k_schur_diag_bf3 / _offdiag_bf3)
  bool pairs_fold_u = false;         // ... and k_schur_diag_bf3 accumulates the camera blocks itself (no k_linearize_cams in the loop)
  bool vis_mask = false;             // a kernel of the route reads the one-group visibility mask
};

// No HIP call, no allocation, no environment: the layout and the switches in, the kernel choices out
template <typename T>
Route plan_route(const Layout& L, const Knobs& k) {
  Route r;
  const int C = L.C, N = L.N;
  const bool dense = L.dense;
  const bool dense_enough = (double)L.M >= k.dense_min_vis * (double)N * C;
  {
    const int target = 256;
    // workgroups per k-split: every pair is dealt to TS workgroups (tile split, grid.z of k_schur)
    // the diagonal and the off-diagonal pairs are two launches, one after the other, with the same k-split: it is sized so
    // that the SMALLER of the two still fills the chip (sized for the larger one, the 4 diagonal pairs of a 64-camera rig ran
    // on 84 of 256 CUs); the larger launch then simply takes several rounds of shorter workgroups
    const int wg_diag = L.ngroups * SchurSel<T, true>::TS, wg_off = (L.npairs - L.ngroups) * SchurSel<T, false>::TS;
    const int wg_per_ks = wg_off > 0 ? std::min(wg_diag, wg_off) : wg_diag;
    int ks = std::max(1, (target + wg_per_ks - 1) / wg_per_ks);
    const int maxks = std::max(1, (N + SCHUR_PTS - 1) / SCHUR_PTS);
    r.ksplit = std::min(ks, maxks);
    // Round 4: several camera groups -- the launches run in ROUNDS of one workgroup per CU, and a last round that is half empty costs
    // as much as a full one (64 cameras, k-split 64: 384 off-diagonal workgroups = 1.5 rounds).  Measured (profiles/r4_ksplit_sweep.txt):
    // 64 x 200k 3 674 -> 3 330 us per iteration with twice the k-split (512 + 768 workgroups: whole rounds, and a finer tail), 128 x 125k
    // with 13 parameters 10.67 -> 9.98 ms, 32 x 50k 470 -> 435 us.  So: aim at two rounds for the smaller launch, then pick, in a window
    // around that, the k-split with the smallest modelled makespan  sum over the two launches of  rounds x points per workgroup
    // (an off-diagonal workgroup builds two panels and 121 tiles: weight 2).
    if (L.ngroups > 1) {
      const int ncu = L.ncu;
      const int ks0 = std::max(1, (2 * ncu + wg_per_ks - 1) / wg_per_ks);
      double best = 1e300;
      int best_ks = ks0;
      for (int q = std::max(1, ks0 * 3 / 4); q <= ks0 * 3 / 2; ++q) {
        const double per = std::ceil((double)N / q);
        const double cost = std::ceil((double)wg_diag * q / ncu) * per + (wg_off > 0 ? 2.0 * std::ceil((double)wg_off * q / ncu) * per : 0.0);
        if (cost < best * (1 - 1e-9)) { best = cost; best_ks = q; }
      }
      r.ksplit = std::min(best_ks, maxks);
    }
  }
  // Up to 256 reduced-system rows, f32: the one-launch fused kernel of sba_schur_wide.hpp -- 17 .. 23 cameras of the 11-parameter
  // model (one group has k_schur_fused_bf3), every rig of up to 19 cameras of the 13-parameter model.  Like the masked
  // one-group kernel its producer cost does not shrink with the visibility (dense_min_vis).
  if constexpr (sizeof(T) == 4) {
    const bool rig_ok = C > GROUP_CAMS ? (dense || (L.grp_indexed && dense_enough))
                                       : (NCP != 11 && !k.no_dense && (dense || (L.masked_ok && dense_enough)));
    r.fused_wide = rig_ok && C * NCP <= 16 * WIDE_MAX_NTW && N > 0 && !k.no_wide;
    if (r.fused_wide) {
      r.wide_pw = (wide_ntw(C) <= 13 && 3 * C <= 64 && !k.wide_pw2) ? 3 : 2;
      r.ksplit = std::max(1, std::min(256, (N + 4 * r.wide_pw - 1) / (4 * r.wide_pw)));
    }
  }
#if SBA_NCP == 11
  // fp64, 17 and 18 cameras (12 / 13 row tiles): k_schur_fused_wide_f64 (sba_schur_f64.hpp), same eligibility; SBA_NO_FUSED64=1 or
  // SBA_NO_WIDE=1 keep the pair kernels
  if constexpr (sizeof(T) == 8) {
    r.fused_wide = C > GROUP_CAMS && C * NCP <= 16 * WIDE_MAX_NTW && (dense || (L.grp_indexed && dense_enough)) && N > 0 &&
                   !k.no_fused64 && !k.no_wide;
    if (r.fused_wide) {
      // 17, 18 cameras (12, 13 row tiles): one workgroup per slice, three points per producer wave; 19 .. 23 (14 .. 16 tiles): two
      // workgroups per slice share its tiles (a consumer wave holds at most ~23 f64 accumulator tiles), two points per wave
      r.wide_ts = wide_ntw(C) > 13 ? 2 : 1;
      r.wide_pw = (r.wide_ts == 1 && !k.wide_pw2) ? 3 : 2;
      r.ksplit = std::max(1, std::min(256 / r.wide_ts, (N + 4 * r.wide_pw - 1) / (4 * r.wide_pw)));
    }
  }
#endif
  r.dense_one_group = dense && C <= GROUP_CAMS && N > 0 && !k.no_dense;
  // 17 .. 23 cameras, dense or group-indexed and dense enough (the rigs of the wide fused kernels): the same back substitution
  // with a point per 32-lane wave half
  r.backsub_wide = C > GROUP_CAMS && C <= 32 && N > 0 && (dense || (L.grp_indexed && dense_enough)) && !k.no_dense && !k.no_wide;
  r.backsub_pack = r.backsub_wide && 3 * C <= 64 && !k.wide_pw2;       // three points per wave (17 .. 21 cameras)
  // 33 .. 128 cameras (round 4): a point per wave, up to two cameras per lane (k_backsub_dense<T, 64>)
  r.backsub_wave = C > 32 && N > 0 && (dense || (L.grp_indexed && dense_enough)) && !k.no_dense && !k.no_wide;
  const int bs_ppc = r.backsub_wave ? 4 : r.backsub_pack ? 12 : r.backsub_wide ? 8 : 16;
  // (the wave linearisation also forms the point factors inside the LM loop: k_point_factor's work)
  r.linp_lw = r.backsub_wave ? 64 : (r.backsub_wide && C > 23) ? 32 : 0;
  r.nlinp = r.linp_lw ? std::max(1, std::min((N + (PM_BLOCK / r.linp_lw) - 1) / (PM_BLOCK / r.linp_lw), 1024)) : 0;
  r.nbs_dense = std::max(1, std::min((N + bs_ppc - 1) / bs_ppc, sizeof(T) == 4 ? 768 : 512));
  // the fused linearise+Schur kernel also serves sparse one-group rigs through the visibility mask
  const bool masked_fused = L.masked_ok && N > 0 && dense_enough && !k.no_dense;
  // (the fused kernel is built for the 11-parameter model only: 77 register accumulators per lane; 13 parameters need 104)
  // (fp64, round 3: k_schur_fused_f64, same structure on the f64 matrix pipe; SBA_NO_FUSED64=1 keeps the three-launch path)
  r.fused_f64 = NCP == 11 && sizeof(T) == 8 && (r.dense_one_group || masked_fused) && !k.no_fused64;
  r.fused_ok = (NCP == 11 && (r.dense_one_group || masked_fused) && sizeof(T) == 4) || r.fused_wide || r.fused_f64;
  r.fused_masked = r.fused_ok && !r.dense_one_group && !r.fused_wide;
  r.lin_pts_ok = (r.dense_one_group || masked_fused) && SCHUR_LIN_OK<T> && !r.fused_f64;
  // (the lane = (point, camera) back substitution serves sparse one-group rigs through the same mask, down to the visibility
  //  where the point-aligned kernel, whose cost follows the observation count, wins)
  r.backsub_masked = L.masked_ok && C <= GROUP_CAMS && N > 0 && dense_enough && !k.no_dense;
  r.vis_mask = r.fused_masked || (r.lin_pts_ok && !r.dense_one_group) || (r.fused_wide && C <= GROUP_CAMS && !dense) || r.backsub_masked;
  // several camera groups on the bf16 pair kernels (round 4); the diagonal pairs also accumulate U_c / g_c
  r.pairs_bf3 = sizeof(T) == 4 && L.ngroups > 1 && L.grp_indexed && !k.no_bf3_pairs;
  r.pairs_fold_u = r.pairs_bf3 && !r.fused_ok;
  return r;
}

// ============================================================================================== engine
template <typename T>
struct Engine : EngineBase {
  using T2 = typename Vec2<T>::type;
  int C = 0, N = 0;
  int64_t M = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  bool uploaded = false;
  bool has_w = false;
  bool identity_perm = true;
  bool dense = false;                // every point is observed by every camera exactly once
  bool masked_ok = false;            // one group, no duplicate (point, camera) pairs, not dense: visibility mask available
  DevBuf<uint16_t> vis_mask;
  DevBuf<uint16_t> grp_mask;         // several camera groups: k_group_index tables [ngroups][N] (Schur producers)
  DevBuf<int32_t> grp_start;
  bool grp_indexed = false;
  DevBuf<double> gdpart;
  std::vector<int64_t> perm;          // pm position -> caller's observation index
  int nblk = 0, nchunk = 0, ngroups = 0, npairs = 0;
  int n = 0;                          // 11*C
  Knobs kn;                           // the environment switches, read at sba_create
  Route rt;                           // the kernels this handle runs, chosen at sba_upload

  // static problem data
  DevBuf<T2> uv_pm, uv_cm;
  DevBuf<T> w_pm, w_cm;
  DevBuf<int32_t> ci_pm, pi_pm, pt_start, blk_pt, pi_cm, chunk_cam, chunk_begin, chunk_end, cam_chunk_start;
  DevBuf<int32_t> pair_ga, pair_gb;
  DevBuf<int4> blk_desc;
  // parameters (double-buffered: cur / trial)
  DevBuf<double> cams[2], pts[2];
  DevBuf<T> ptsT[2], campre[2];
  int cur = 0;
  // linearization + LM work space
  DevBuf<double> V, gp, D2p, D2c, U, gc, Upart, bpart, E_own, scal_own, delta_c, cost_part, gmax_part, trial_part;
  DevBuf<T> slabs, pfac;
  DevBuf<T2> r_pm;
  DevBuf<T> Jc_pm, Jp_pm;
  // The state record lives in a two-entry buffer: k_schur_fused_bf3 can carry the accept/reject decision of the previous trial
  // step in its prologue, reading one entry and publishing the updated record to the other (see FusedDecide).  d_state.p is the
  // entry every launch enqueued NOW has to use.
  DevBuf<LMState> d_state_buf;
  struct { LMState* p = nullptr; } d_state;
  int st_slot = 0;
  bool pending_decide = false;        // lm_decide_async was called and its decision has not been enqueued yet
  const double* pend_scal = nullptr;
  int pend_ranks = 1;
  DevBuf<double> gmax_alt;            // second array of gradient maxima (the fused kernel reads one and writes the other)
  double* gmax_cur = nullptr;         // the array the last linearisation wrote
  DevBuf<sba_lm_iter_log> d_log;
  int log_read = 0;
  int cur_at_begin = 0;
  LMState* h_state = nullptr;         // pinned
  sba_lm_opts opts{};
  bool lm_active = false;
  CholSolver<T> chol;                   // the reduced camera solve: its buffers, f32 image and launch state (sba_chol_solve.hpp)
  bool card_shared = false;             // sba_ipc_attach found a peer rank's exchange area on THIS device (a rehearsal of N ranks on one card):
                                        // kernels whose workgroups wait for each other are then not used where a launch-per-step form exists
  // SBA_SCHUR_DEBUG: armed from the switch at sba_create, cleared once its stamps are printed
  bool schur_debug = false;
  int schur_debug_skip = 0;           // fused Schur launches still to pass before the one whose stamps are printed
  // multi-rank (one handle per GPU, points sharded, cameras replicated): RCCL communicator + exchange buffers
  DevBuf<double> raw_uv, raw_w;         // the caller's raw arrays on the device (dense fast path of upload)
  DevBuf<long long> raw_ci, raw_pi;
  DevBuf<int> up_flag;
  DevBuf<unsigned char> pt_fixed_mask;   // sba_set_fixed_points: 1 = the point is a gauge anchor (never moves, not an unknown)
  bool has_fixed = false;
  double loss_delta = 0;                // sba_set_robust_loss: f_scale of the robust loss, 0 = linear loss
  int loss_kind = 0;                    // ... and which one (sba_loss)
  Rccl::comm_t comm = nullptr;
  int comm_rank = 0, comm_n = 1;
  DevBuf<double> xpack, sc_loc, sc_all, comm_tmp;
  double* h_comm = nullptr;             // pinned staging of the few scalars all-reduced at begin / finish
  // one-shot exchange through peer-mapped buffers instead of RCCL (sba_ipc.hpp; sba_ipc_export / sba_ipc_attach)
  bool ipc_on = false;
  bool ipc_dead = false;                // an exchange outside the LM loop timed out: the ranks' exchange counters no longer agree
  int ipc_planned = 0;                  // n_ranks the area was exported for
  double* ipc_mine = nullptr;           // this rank's area (uncached device memory)
  uint8_t ipc_my_handle[SBA_IPC_HANDLE_BYTES] = {};
  std::vector<double*> ipc_area;        // every rank's area as mapped into this process (own entry = ipc_mine)
  std::vector<char> ipc_opened;         // ... 1 where this handle called hipIpcOpenMemHandle (and has to close it)
  DevBuf<double*> ipc_ptrs;             // ... the same table on the device
  DevBuf<int> ipc_fail;                 // set by a gate that ran out of time outside the LM loop
  IpcLayout ipc_L{};
  unsigned long long ipc_seq[IPC_KINDS] = {0, 0, 0};     // exchanges enqueued so far, per kind (the value the flags carry)
  bool multi() const { return comm != nullptr || ipc_on; }
  long long N_global = 0;
  DevBuf<long long> schur_dbg;
  double initial_cost = 0;
  std::vector<sba_lm_iter_log> log;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_wait = nullptr;
  // in-loop kernel timing (opts.reserved[0] != 0): one HIP event pair per kernel class per LM iteration
  enum { KP_LINP = 0, KP_LINC, KP_SCHUR, KP_REDUCE, KP_CHOL, KP_BACKSUB, KP_N };
  hipEvent_t pev[KP_N][2] = {};
  bool pev_used[KP_N] = {};
  bool prof_on = false;
  double prof_us[KP_N] = {};
  long long prof_cnt[KP_N] = {};
  void prof_begin(int k) { if (prof_on) HIPCHK(hipEventRecord(pev[k][0], stream)); }
  void prof_end(int k) { if (prof_on) { HIPCHK(hipEventRecord(pev[k][1], stream)); pev_used[k] = true; } }
  void prof_collect() {   // call after a stream sync
    if (!prof_on) return;
    for (int k = 0; k < KP_N; ++k)
      if (pev_used[k]) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, pev[k][0], pev[k][1]) == hipSuccess) { prof_us[k] += (double)ms * 1e3; prof_cnt[k]++; }
        pev_used[k] = false;
      }
  }

  HostRes hres;
  bool have_hres = false;
  // small device-to-host results land in pinned memory (a copy into pageable memory is staged and blocks the caller per copy)
  double* h_land = nullptr;
  static constexpr size_t LAND_DOUBLES = (HostRes::PINNED_BYTES - HostRes::PINNED_STATE_BYTES) / sizeof(double);
  bool poll_clean = false;            // nothing has been enqueued since the last lm_poll: its state and log are current
  int n_decides = 0;                  // accept/reject kernels enqueued since lm_begin (upper bound of the log rows on the device)
  ~Engine() override {
    if (comm) (void)Rccl::get().comm_destroy(comm);
    if (stream) (void)hipStreamSynchronize(stream);
    ipc_close_peers();
    if (ipc_mine) { IpcLocalAreas::get().remove(ipc_my_handle); (void)hipFree(ipc_mine); }
    if (h_comm) (void)hipHostFree(h_comm);
    if (have_hres) {
      if (stream) (void)hipStreamSynchronize(stream);     // nothing of this handle may still be in flight when its buffers are recycled
      (void)hipStreamSynchronize(hres.stream);
      if (hres.copy_stream) (void)hipStreamSynchronize(hres.copy_stream);
      HostResPool::get().give(hres);
    }
  }

  void init(const sba_problem_desc& d) override {
    C = d.n_cams; N = d.n_points; M = d.n_obs; device = d.device; n = C * NCP;
    arena.device = device;
    HIPCHK(hipSetDevice(device));
    static_assert(sizeof(LMState) <= 1024 && KP_N * 2 + 2 <= (int)(sizeof(HostRes::ev) / sizeof(hipEvent_t)), "HostRes sizes");
    if (!HostResPool::get().take(device, &hres)) {
      hres.device = device;
      HIPCHK(hipStreamCreateWithFlags(&hres.stream, hipStreamNonBlocking));
      HIPCHK(hipStreamCreateWithFlags(&hres.copy_stream, hipStreamNonBlocking));
      HIPCHK(hipHostMalloc(&hres.pinned, HostRes::PINNED_BYTES, hipHostMallocDefault));
      for (auto& e : hres.ev) HIPCHK(hipEventCreate(&e));
      HIPCHK(hipEventCreateWithFlags(&hres.ev_wait, hipEventDisableTiming));
    }
    have_hres = true;
    if (d.use_stream) { stream = reinterpret_cast<hipStream_t>(d.stream); own_stream = false; }
    else { stream = hres.stream; own_stream = true; }
    h_state = static_cast<LMState*>(hres.pinned);
    h_land = reinterpret_cast<double*>(static_cast<char*>(hres.pinned) + HostRes::PINNED_STATE_BYTES);
    ev0 = hres.ev[0]; ev1 = hres.ev[1]; ev_wait = hres.ev_wait;
    for (int k = 0; k < KP_N; ++k) for (int j = 0; j < 2; ++j) pev[k][j] = hres.ev[2 + 2 * k + j];
    d_state_buf.alloc(2);
    d_state.p = d_state_buf.p;
    kn = read_knobs();
    chol.arm_debug(kn.chol_debug, stream);
    if (kn.schur_debug) { schur_debug = true; schur_debug_skip = kn.schur_debug_skip; schur_dbg.alloc(64); schur_dbg.zero(stream); }
    static bool attrs_set[16] = {};          // the function attributes are per process (and device), not per handle
    if (device < 16 && attrs_set[device]) return;
    // kernels whose dynamic LDS can exceed the 64 KB default
    // only the Schur flavours this dtype launches are instantiated (f32: producer/consumer + fused; f64: symmetric + PARTIAL)
    if constexpr (SCHUR_SYM<T>) {
      set_lds(&k_schur_sym<T, true, false>, 156 * 1024);
      set_lds(&k_schur_sym<T, false, false>, 156 * 1024);
      set_lds(&k_schur_sym<T, true, true>, 156 * 1024);
      set_lds(&k_schur_sym<T, false, true>, 156 * 1024);
      if constexpr (SCHUR_LIN_OK<T>) set_lds(&k_schur_sym<T, true, false, true>, 156 * 1024);
#if SBA_NCP == 11
      set_lds(&k_schur_fused_f64, SchurF64Cfg::LDS_BYTES);
      set_lds(&k_schur_fused_wide_f64<12, 2, 1>, SchurWide64Cfg<12, 2, 1>::LDS_BYTES);
      set_lds(&k_schur_fused_wide_f64<13, 2, 1>, SchurWide64Cfg<13, 2, 1>::LDS_BYTES);
      set_lds(&k_schur_fused_wide_f64<12, 3, 1>, SchurWide64Cfg<12, 3, 1>::LDS_BYTES);
      set_lds(&k_schur_fused_wide_f64<13, 3, 1>, SchurWide64Cfg<13, 3, 1>::LDS_BYTES);
      set_lds(&k_schur_fused_wide_f64<14, 2, 2>, SchurWide64Cfg<14, 2, 2>::LDS_BYTES);
      set_lds(&k_schur_fused_wide_f64<15, 2, 2>, SchurWide64Cfg<15, 2, 2>::LDS_BYTES);
      set_lds(&k_schur_fused_wide_f64<16, 2, 2>, SchurWide64Cfg<16, 2, 2>::LDS_BYTES);
#endif
    } else {
      set_lds(&k_schur<T, true, false>, 156 * 1024);
      set_lds(&k_schur<T, false, false>, 156 * 1024);
#if SBA_NCP == 11
      set_lds(&k_schur_fused_bf3, SchurBf3Cfg::LDS_BYTES);
#endif
      set_lds(&k_schur_fused_wide<12, 2>, SchurWideCfg<12, 2>::LDS_BYTES);
      set_lds(&k_schur_fused_wide<13, 2>, SchurWideCfg<13, 2>::LDS_BYTES);
      set_lds(&k_schur_fused_wide<14, 2>, SchurWideCfg<14, 2>::LDS_BYTES);
      set_lds(&k_schur_fused_wide<15, 2>, SchurWideCfg<15, 2>::LDS_BYTES);
      set_lds(&k_schur_fused_wide<16, 2>, SchurWideCfg<16, 2>::LDS_BYTES);
      set_lds(&k_schur_fused_wide<12, 3>, SchurWideCfg<12, 3>::LDS_BYTES);
      set_lds(&k_schur_fused_wide<13, 3>, SchurWideCfg<13, 3>::LDS_BYTES);
      set_lds(&k_schur_fused_wide<8, 2>, SchurWideCfg<8, 2>::LDS_BYTES);
      set_lds(&k_schur_fused_wide<8, 3>, SchurWideCfg<8, 3>::LDS_BYTES);
      set_lds(&k_schur_diag_bf3, SchurPairCfg::LDS_BYTES);
      set_lds(&k_schur_offdiag_bf3, SchurBf3OffCfg::LDS_BYTES);
    }
    set_lds(&k_resjac<T>, 100 * 1024);
    CholSolver<T>::set_attrs();
    set_lds(&k_backsub_trial<T>, 100 * 1024);
    set_lds(&k_linearize_points<T>, 100 * 1024);
    set_lds(&k_residual<T>, 100 * 1024);
    set_lds(&k_sq_linearize<T, 2>, 100 * 1024);
    set_lds(&k_sq_linearize<T, 1>, 100 * 1024);
    set_lds(&k_sq_trial<T, 1>, 100 * 1024);
    set_lds(&k_sq_trial<T, 2>, 100 * 1024);
    if (device < 16) attrs_set[device] = true;
  }

  void sync() { HIPCHK(hipStreamSynchronize(stream)); }
  // Wait for the stream with a short busy poll first: a blocking hipStreamSynchronize wakes the thread tens of microseconds after the
  // GPU is done, which is a visible share of a 20-iteration solve (2.6 ms); after SPIN_US the thread blocks like sync() does.
  void sync_spin() {
    constexpr double SPIN_US = 5000.0;
    HIPCHK(hipEventRecord(ev_wait, stream));
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      const hipError_t q = hipEventQuery(ev_wait);
      if (q == hipSuccess) return;
      if (q != hipErrorNotReady) { HIPCHK(q); }
      if (std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > SPIN_US) break;
    }
    HIPCHK(hipStreamSynchronize(stream));
  }

  // ------------------------------------------------------------------ upload + layout (dense kernel, general device pass, host pass)
  // An automatic upload of a list that is not the dense canonical one takes the general device pass (sba_layout.hpp) from this
  // many observations on; below it the host pass stays (a short list costs the host less than the pass's launches and its
  // read-back: DESIGN.md section 3 has the measurement).
  static constexpr int64_t LAYOUT_DEVICE_MIN_OBS = 100000;
  sba_upload_report up_rep{};             // what the last upload did (sba_get_upload_report)
  std::vector<int32_t> cam_start_h;       // camera starts of the camera-major copy (sba_get_layout)
  bool has_vis_mask = false;              // vis_mask holds the one-group visibility masks of this upload
  DevBuf<int32_t> lay_deg, lay_cursor, lay_perm, lay_counts, lay_offs, lay_tiles;     // work space of the general device pass
  DevBuf<unsigned long long> lay_keys;

  int upload(const double* cams_h, const double* pts_h, const double* uv_in, const int64_t* ci_in,
             const int64_t* pi_in, const double* w_in, const sba_upload_opts& uo) override {
    HIPCHK(hipSetDevice(device));
    const bool up_dbg = kn.upload_debug;
    up_rep = sba_upload_report{};
    const auto up_begin = std::chrono::steady_clock::now();
    auto up_t0 = up_begin;
    double* up_phase = &up_rep.seconds_tables;       // the phase of the report the next lap is booked to
    auto up_lap = [&](const char* what) {
      const auto t = std::chrono::steady_clock::now();
      const double s = std::chrono::duration<double>(t - up_t0).count();
      *up_phase += s;
      if (up_dbg) fprintf(stderr, "[upload] %-28s %7.3f ms\n", what, s * 1e3);
      up_t0 = t;
    };
    auto up_sync = [&] { sync(); ++up_rep.stream_syncs; };
    if (C <= 0 || N < 0 || M < 0) { err = "bad problem size"; return SBA_ERR_INVALID; }
    if (C > MAX_CAMS) { err = "more than 128 cameras is not supported yet"; return SBA_ERR_UNSUPPORTED; }
    if (M > (int64_t)0x7fffffff - 1024) { err = "too many observations for int32 device indices"; return SBA_ERR_UNSUPPORTED; }
    has_w = (w_in != nullptr);
    // The caller's raw arrays lie on the host (uv_h ...) or, with obs_on_device, on the device (uv_d ...); a route that needs
    // the other side fetches it once.
    const bool on_dev = uo.obs_on_device != 0;
    const double *uv_h = on_dev ? nullptr : uv_in, *w_h = on_dev ? nullptr : w_in;
    const int64_t *ci_h = on_dev ? nullptr : ci_in, *pi_h = on_dev ? nullptr : pi_in;
    const double *uv_d = on_dev ? uv_in : nullptr, *w_d = on_dev ? w_in : nullptr;
    const long long *ci_d = on_dev ? reinterpret_cast<const long long*>(ci_in) : nullptr;
    const long long *pi_d = on_dev ? reinterpret_cast<const long long*>(pi_in) : nullptr;
    std::vector<double> uv_hv, w_hv;
    std::vector<int64_t> ci_hv, pi_hv;
    auto raw_to_device = [&] {
      if (uv_d) return;
      double* const phase = up_phase;
      up_phase = &up_rep.seconds_h2d;
      raw_uv.alloc((size_t)M * 2); raw_ci.alloc(M); raw_pi.alloc(M);
      if (has_w) raw_w.alloc(M);
      HIPCHK(hipMemcpyAsync(raw_uv.p, uv_h, sizeof(double) * 2 * M, hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(raw_ci.p, ci_h, sizeof(int64_t) * M, hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(raw_pi.p, pi_h, sizeof(int64_t) * M, hipMemcpyHostToDevice, stream));
      if (has_w) HIPCHK(hipMemcpyAsync(raw_w.p, w_h, sizeof(double) * M, hipMemcpyHostToDevice, stream));
      uv_d = raw_uv.p; ci_d = raw_ci.p; pi_d = raw_pi.p; w_d = has_w ? raw_w.p : nullptr;
      up_lap("raw H2D");
      up_phase = phase;
    };
    auto raw_to_host = [&] {
      if (!on_dev || uv_h || M == 0) return;
      double* const phase = up_phase;
      up_phase = &up_rep.seconds_h2d;
      uv_hv.resize((size_t)M * 2); ci_hv.resize(M); pi_hv.resize(M);
      if (has_w) w_hv.resize(M);
      HIPCHK(hipMemcpyAsync(uv_hv.data(), uv_d, sizeof(double) * 2 * M, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipMemcpyAsync(ci_hv.data(), ci_d, sizeof(int64_t) * M, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipMemcpyAsync(pi_hv.data(), pi_d, sizeof(int64_t) * M, hipMemcpyDeviceToHost, stream));
      if (has_w) HIPCHK(hipMemcpyAsync(w_hv.data(), w_d, sizeof(double) * M, hipMemcpyDeviceToHost, stream));
      up_sync();
      uv_h = uv_hv.data(); ci_h = ci_hv.data(); pi_h = pi_hv.data(); w_h = has_w ? w_hv.data() : nullptr;
      up_lap("raw D2H");
      up_phase = phase;
    };
    // Device-side layout: when the list can only be the canonical dense one -- M = N*C -- the caller's raw
    // float64 / int64 arrays go to the GPU as they are and ONE kernel validates them (observation i must be point i / C, camera
    // i % C: that single test implies in-range, point-major, camera-minor, no duplicates, every camera sees every point),
    // narrows them to the device types and writes the point-major and the camera-major copies.  Anything else (sparse
    // visibility, unsorted or duplicated observations) takes the host path below.
    bool dev_dense = false;
    std::vector<int32_t> ptstart;
    bool sorted = true, cam_sorted = true;
    std::vector<uint16_t> vmask;
    bool nodup = (C <= GROUP_CAMS);
    if (M > 0 && M == (int64_t)N * C && uo.layout != SBA_LAYOUT_HOST) {
      raw_to_device();
      uv_pm.alloc(M); ci_pm.alloc(M); pi_pm.alloc(M); uv_cm.alloc(M); pi_cm.alloc(M); pt_start.alloc((size_t)N + 1);
      if (has_w) { w_pm.alloc(M); w_cm.alloc(M); }
      if (up_flag.n == 0) up_flag.alloc(1);
      up_flag.zero(stream);
      up_phase = &up_rep.seconds_device_layout;
      hipLaunchKernelGGL(k_upload_dense<T>, dim3((unsigned)((std::max<int64_t>(M, N + 1) + 255) / 256)), dim3(256), 0, stream,
                         reinterpret_cast<const double2*>(uv_d), ci_d, pi_d, has_w ? w_d : (const double*)nullptr, C, N, (long long)M,
                         uv_pm.p, ci_pm.p, pi_pm.p, has_w ? w_pm.p : (T*)nullptr, uv_cm.p, pi_cm.p, has_w ? w_cm.p : (T*)nullptr,
                         pt_start.p, up_flag.p);
      int flag = 1;
      HIPCHK(hipMemcpyAsync(&flag, up_flag.p, sizeof(int), hipMemcpyDeviceToHost, stream));
      up_sync();
      up_lap("device validate + layout");
      dev_dense = (flag == 0);
    }
    // Every other list -- sparse visibility, shuffled, camera-descending -- is laid out by the kernels of sba_layout.hpp from the same
    // raw arrays; they decline (index out of range, duplicate pair in one camera group, a point with more than 256 observations)
    // and the host pass below, which owns the error texts, takes over.
    bool dev_general = false;
    std::vector<int32_t> camcount_dev;
    if (!dev_dense && M > 0 && N > 0 &&
        (uo.layout == SBA_LAYOUT_DEVICE || (uo.layout == SBA_LAYOUT_AUTO && M >= LAYOUT_DEVICE_MIN_OBS))) {
      raw_to_device();
      up_phase = &up_rep.seconds_device_layout;
      dev_general = layout_device(uv_d, ci_d, pi_d, has_w ? w_d : (const double*)nullptr, ptstart, camcount_dev);
      up_lap("device layout (general)");
    }
    const bool dev_lay = dev_dense || dev_general;
    up_phase = &up_rep.seconds_tables;
    if (dev_general) {
      nodup = (C <= GROUP_CAMS);                  // (a duplicate pair in one camera group is a decline)
      dense = nodup && M == (int64_t)N * C;       // no duplicate and N * C observations: every camera sees every point
    } else if (dev_dense) {
      ptstart.resize((size_t)N + 1);
      for (int p = 0; p <= N; ++p) ptstart[p] = p * C;
      dense = true; identity_perm = true; perm.clear();
      if (C > PM_BLOCK) { err = "a point has more than 256 observations"; return SBA_ERR_UNSUPPORTED; }
      up_rep.max_degree = C;
    } else {
    raw_to_host();
    up_phase = &up_rep.seconds_host_layout;
    // one pass: range check, point-major order, and camera order inside a point (strictly increasing cameras inside every
    // point = no duplicate (point, camera) pair and already canonical: what get_points3d.py:78-86 emits)
    {
      int64_t bad[4] = {-1, -1, -1, -1};
      bool uns[4] = {false, false, false, false}, cuns[4] = {false, false, false, false};
      par_for(M, [&](int64_t lo, int64_t hi, int t) {
        for (int64_t i = lo; i < hi; ++i) {
          if (ci_h[i] < 0 || ci_h[i] >= C || pi_h[i] < 0 || pi_h[i] >= N) { if (bad[t] < 0) bad[t] = i; continue; }
          if (i) {
            if (pi_h[i] < pi_h[i - 1]) uns[t] = true;
            else if (pi_h[i] == pi_h[i - 1] && ci_h[i] <= ci_h[i - 1]) cuns[t] = true;
          }
        }
      });
      for (int t = 0; t < 4; ++t) {
        if (bad[t] >= 0) { err = "camera/point index out of range at observation " + std::to_string(bad[t]); return SBA_ERR_INVALID; }
        sorted = sorted && !uns[t];
        cam_sorted = cam_sorted && !cuns[t];
      }
    }
    // point-major order (stable counting sort by point)
    ptstart.assign((size_t)N + 1, 0);
    for (int64_t i = 0; i < M; ++i) ptstart[pi_h[i] + 1]++;
    int maxdeg = 0;
    for (int p = 0; p < N; ++p) { maxdeg = std::max(maxdeg, ptstart[p + 1]); ptstart[p + 1] += ptstart[p]; }
    dense = (M == (int64_t)N * C);
    for (int p = 0; p < N && dense; ++p) dense = (ptstart[p + 1] - ptstart[p] == C);
    if (maxdeg > PM_BLOCK) { err = "a point has more than 256 observations"; return SBA_ERR_UNSUPPORTED; }
    up_rep.max_degree = maxdeg;
    perm.resize(M);
    identity_perm = sorted;
    if (sorted) par_for(M, [&](int64_t lo, int64_t hi, int) { for (int64_t i = lo; i < hi; ++i) perm[i] = i; });   // (the canonical pass below may still reorder)
    else {
      std::vector<int32_t> fill(ptstart.begin(), ptstart.end() - 1);
      for (int64_t i = 0; i < M; ++i) perm[fill[pi_h[i]]++] = i;
    }
    // One camera group: put the observations of every point in camera order (what get_points3d.py:78-86 emits anyway) and
    // record which cameras see it.  Without duplicate (point, camera) pairs the lane = (point, camera) kernels apply:
    // dense = every camera sees every point (observation (p, c) at p*C + c), else through the visibility mask.
    if (nodup && sorted && cam_sorted) {           // already canonical: only the visibility masks are needed
      vmask.assign(N, 0);
      for (int64_t i = 0; i < M; ++i) vmask[pi_h[i]] |= (uint16_t)(1u << ci_h[i]);
    } else if (nodup) {
      vmask.assign(N, 0);
      std::vector<int64_t> slot(C);
      for (int p = 0; p < N && nodup; ++p) {
        std::fill(slot.begin(), slot.end(), (int64_t)-1);
        const int a = ptstart[p], b = ptstart[p + 1];
        for (int k = a; k < b; ++k) {
          const int64_t i = perm[k];
          if (slot[ci_h[i]] >= 0) { nodup = false; break; }
          slot[ci_h[i]] = i;
          vmask[p] |= (uint16_t)(1u << ci_h[i]);
        }
        if (!nodup) break;
        int k = a;
        for (int c = 0; c < C; ++c)
          if (slot[c] >= 0) { if (perm[k] != slot[c]) { perm[k] = slot[c]; identity_perm = false; } ++k; }
      }
    }
    dense = dense && nodup;
    up_lap("validate + sort + canonical");
    }   // host validation
    masked_ok = nodup && !dense;
    if (!dev_lay) up_phase = &up_rep.seconds_host_layout;
    std::vector<T2> uvp(dev_lay ? 0 : M);
    std::vector<T> wp(has_w && !dev_lay ? M : 0);
    std::vector<int32_t> cip(dev_lay ? 0 : M), pip(dev_lay ? 0 : M);
    if (!dev_lay) par_for(M, [&](int64_t lo, int64_t hi, int) {
      for (int64_t k = lo; k < hi; ++k) {
        const int64_t i = perm[k];
        uvp[k].x = (T)uv_h[2 * i]; uvp[k].y = (T)uv_h[2 * i + 1];
        if (has_w) wp[k] = (T)w_h[i];
        cip[k] = (int32_t)ci_h[i]; pip[k] = (int32_t)pi_h[i];
      }
    });
    up_lap("permute observations");
    // point-aligned blocks of <= 256 observations
    std::vector<int32_t> blk;
    blk.push_back(0);
    {
      int p = 0;
      while (p < N) {
        int q = p; int cnt = 0;
        while (q < N && cnt + (ptstart[q + 1] - ptstart[q]) <= PM_BLOCK && (q - p) < PM_BLOCK) { cnt += ptstart[q + 1] - ptstart[q]; ++q; }
        if (q == p) ++q;   // cannot happen (maxdeg <= 256) but never loop forever
        blk.push_back(q);
        p = q;
      }
    }
    nblk = (int)blk.size() - 1;
    std::vector<int4> bdesc(nblk);
    for (int b = 0; b < nblk; ++b) bdesc[b] = make_int4(blk[b], blk[b + 1], ptstart[blk[b]], ptstart[blk[b + 1]]);
    // camera-major order of the pm list (stable => points ascending inside a camera)
    std::vector<int32_t> camcount(C + 1, 0);
    if (dev_dense) { for (int c = 0; c <= C; ++c) camcount[c] = c * N; }
    else if (dev_general) camcount = camcount_dev;
    else {
      for (int64_t k = 0; k < M; ++k) camcount[cip[k] + 1]++;
      for (int c = 0; c < C; ++c) camcount[c + 1] += camcount[c];
    }
    std::vector<T2> uvc(dev_lay ? 0 : M);
    std::vector<T> wc(has_w && !dev_lay ? M : 0);
    std::vector<int32_t> pic(dev_lay ? 0 : M);
    if (!dev_lay) {
      std::vector<int32_t> fill(camcount.begin(), camcount.end() - 1);
      for (int64_t k = 0; k < M; ++k) {
        const int32_t d = fill[cip[k]]++;
        uvc[d] = uvp[k]; pic[d] = pip[k];
        if (has_w) wc[d] = wp[k];
      }
    }
    std::vector<int32_t> ch_cam, ch_beg, ch_end, cam_ch(C + 1, 0);
    for (int c = 0; c < C; ++c) {
      cam_ch[c] = (int32_t)ch_cam.size();
      for (int32_t b = camcount[c]; b < camcount[c + 1]; b += CM_CHUNK) {
        ch_cam.push_back(c); ch_beg.push_back(b); ch_end.push_back(std::min(camcount[c + 1], b + CM_CHUNK));
      }
    }
    cam_ch[C] = (int32_t)ch_cam.size();
    nchunk = (int)ch_cam.size();
    // camera groups / pairs for the Schur kernel
    ngroups = (C + GROUP_CAMS - 1) / GROUP_CAMS;
    std::vector<int32_t> pga, pgb;
    for (int a = 0; a < ngroups; ++a) { pga.push_back(a); pgb.push_back(a); }   // diagonal pairs first
    for (int a = 0; a < ngroups; ++a)
      for (int b = a + 1; b < ngroups; ++b) { pga.push_back(a); pgb.push_back(b); }
    npairs = (int)pga.size();

    up_lap("blocks + camera-major copies");
    up_phase = &up_rep.seconds_tables;
    cam_start_h = camcount;
    if (!dev_lay) {
      uv_pm.upload(uvp, stream); ci_pm.upload(cip, stream); pi_pm.upload(pip, stream);
      if (has_w) { w_pm.upload(wp, stream); w_cm.upload(wc, stream); }
      pt_start.upload(ptstart, stream);
      uv_cm.upload(uvc, stream); pi_cm.upload(pic, stream);
    }
    blk_pt.upload(blk, stream); blk_desc.upload(bdesc, stream);
    chunk_cam.upload(ch_cam, stream); chunk_begin.upload(ch_beg, stream); chunk_end.upload(ch_end, stream);
    cam_chunk_start.upload(cam_ch, stream);
    pair_ga.upload(pga, stream); pair_gb.upload(pgb, stream);
    grp_indexed = false;
    if (ngroups > 1 && N > 0 && !kn.schur_scan) {
      grp_mask.alloc((size_t)ngroups * N); grp_start.alloc((size_t)ngroups * N);
      if (up_flag.n == 0) up_flag.alloc(1);
      up_flag.zero(stream);
      hipLaunchKernelGGL(k_group_index, dim3((N + 255) / 256), dim3(256), 0, stream, ci_pm.p, pt_start.p, N, ngroups, grp_mask.p,
                         grp_start.p, up_flag.p);
      int flag = 1;
      HIPCHK(hipMemcpyAsync(&flag, up_flag.p, sizeof(int), hipMemcpyDeviceToHost, stream));
      up_sync();
      grp_indexed = (flag == 0);     // cameras strictly ascending inside every point; otherwise the producers scan
    }
    int ncu = 256;
    hipDeviceProp_t prop;
    if (ngroups > 1 && hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) ncu = prop.multiProcessorCount;
    rt = plan_route<T>(Layout{C, N, M, dense, masked_ok, grp_indexed, ngroups, npairs, ncu}, kn);
    const int ksplit = rt.ksplit;

    for (int b = 0; b < 2; ++b) {
      cams[b].alloc((size_t)C * NCP); pts[b].alloc((size_t)N * 3);
      ptsT[b].alloc((size_t)N * 3); campre[b].alloc((size_t)C * CAMPRE);
    }
    pfac.alloc((size_t)std::max(N, 1) * PF);
    V.alloc((size_t)N * 6); gp.alloc((size_t)N * 3); D2p.alloc((size_t)N * 3); D2c.alloc(n);
    U.alloc((size_t)C * NCP * NCP); gc.alloc(n); Upart.alloc((size_t)std::max(1, nchunk) * 256);
    bpart.alloc(std::max((size_t)ngroups * ksplit * GROUP_ROWS, rt.fused_wide ? (size_t)ksplit * WIDE_ROWS : (size_t)0));
    slabs.alloc(std::max((size_t)npairs * ksplit * GROUP_TILES * GROUP_TILES * 256, rt.fused_wide ? (size_t)ksplit * WIDE_SLOTS * 256 : (size_t)0));
    E_own.alloc((size_t)n * n + 3 * n + 1); scal_own.alloc(NSCAL); delta_c.alloc(n);
    chol.on_upload(stream);
    const int nres_blocks = (int)((M + PM_BLOCK - 1) / PM_BLOCK);
    const int nlinp = rt.nlinp;
    // (the one-group visibility masks are kept whenever they exist, also for routes that do not read them: sba_get_layout)
    if (dev_general) has_vis_mask = (C <= GROUP_CAMS);
    else {
      has_vis_mask = nodup && !vmask.empty();
      if (has_vis_mask) vis_mask.upload(vmask, stream);
    }
    if (rt.fused_ok) gdpart.alloc((size_t)ksplit * 2 * (rt.fused_wide ? WIDE_ROWS : GROUP_ROWS));
    if (rt.pairs_fold_u) gdpart.alloc((size_t)ngroups * ksplit * 2 * GROUP_ROWS);
    cost_part.alloc((size_t)std::max(std::max(std::max(std::max(nblk, nres_blocks), ksplit), nlinp), 1)); gmax_part.alloc(std::max(std::max(std::max(nblk, ksplit), nlinp), 1)); gmax_alt.alloc(std::max(std::max(std::max(nblk, ksplit), nlinp), 1));
    // (k_backsub_dense writes one partial row per WORKGROUP: nbs_dense of them, which exceeds the number of point-aligned blocks on
    //  dense rigs with few cameras -- 8 x 1000: 63 vs 32; sized for nblk alone the rows used to run over into the next buffer)
    trial_part.alloc((size_t)4 * std::max(std::max(nblk, rt.nbs_dense), 1));
    up_lap("allocations + H2D enqueue");
    up_sync();   // the staging vectors go out of scope now
    up_lap("H2D completion");
    uploaded = true;
    cur = 0;
    set_params(cams_h, pts_h);
    ++up_rep.stream_syncs;         // (set_params waits for its copies)
    up_lap("parameters");
    up_rep.route = dev_dense ? SBA_ROUTE_DEVICE_DENSE : dev_general ? SBA_ROUTE_DEVICE_GENERAL : SBA_ROUTE_HOST;
    up_rep.dense = dense; up_rep.masked = masked_ok; up_rep.group_indexed = grp_indexed; up_rep.identity_perm = identity_perm;
    up_rep.n_blocks = nblk; up_rep.n_chunks = nchunk;
    up_rep.seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - up_begin).count();
    return SBA_OK;
  }

  int upload_report(sba_upload_report* rep) override {
    if (!uploaded) { err = "sba_upload has not been called"; return SBA_ERR_STATE; }
    *rep = up_rep;
    return SBA_OK;
  }

  // The general device pass (sba_layout.hpp).  true: the layout buffers are built, ptstart / camcount / perm / identity_perm and
  // the report's max_degree are set; false: the pass declined (up_rep.decline_reason) and the host pass has to run.
  // Stream synchronisations: one for the point starts, the camera starts and the flags, one more for the permutation when it
  // is not the identity.
  bool layout_device(const double* uv_d, const long long* ci_d, const long long* pi_d, const double* w_d,
                     std::vector<int32_t>& ptstart, std::vector<int32_t>& camcount) {
    static_assert(LAY_MAX_CAMS == MAX_CAMS && LAY_CAM_START + MAX_CAMS + 1 <= LAY_HEAD, "layout head record");
    const int Mi = (int)M, gM = (Mi + 255) / 256, gN = (N + 255) / 256, nwg = gM;
    const int ncnt = C * nwg;                     // (M < 2^31 - 1024 and C <= 128: below 2^31)
    const int tN = (N + LAY_TILE - 1) / LAY_TILE, tC = (ncnt + LAY_TILE - 1) / LAY_TILE;
    uv_pm.alloc(M); ci_pm.alloc(M); pi_pm.alloc(M); uv_cm.alloc(M); pi_cm.alloc(M);
    if (has_w) { w_pm.alloc(M); w_cm.alloc(M); }
    pt_start.alloc((size_t)N + 1 + LAY_HEAD);
    lay_deg.alloc(N); lay_cursor.alloc(N); lay_perm.alloc(M); lay_keys.alloc(M);
    lay_counts.alloc(ncnt); lay_offs.alloc(ncnt); lay_tiles.alloc(std::max(tN, tC));
    if (C <= GROUP_CAMS) vis_mask.alloc(N);
    int* head = pt_start.p + N + 1;
    T* wpm = has_w ? w_pm.p : (T*)nullptr;
    auto scan = [&](const int* in, int cnt, int ntiles, int* out, int want_total, int* max_out) {
      hipLaunchKernelGGL(k_lay_tile_sums, dim3(ntiles), dim3(256), 0, stream, in, cnt, lay_tiles.p, max_out);
      hipLaunchKernelGGL(k_lay_scan_tiles, dim3(1), dim3(256), 0, stream, lay_tiles.p, ntiles);
      hipLaunchKernelGGL(k_lay_scan_apply, dim3(ntiles), dim3(256), 0, stream, in, cnt, (const int*)lay_tiles.p, out, want_total);
    };
    hipLaunchKernelGGL(k_lay_init, dim3(std::max(gN, 1)), dim3(256), 0, stream, lay_deg.p, lay_cursor.p, N, head);
    hipLaunchKernelGGL(k_lay_scan_obs, dim3(gM), dim3(256), 0, stream, ci_d, pi_d, Mi, C, N, lay_deg.p, head);
    scan(lay_deg.p, N, tN, pt_start.p, 1, head + LAY_MAXDEG);
    hipLaunchKernelGGL(k_lay_scatter, dim3(gM), dim3(256), 0, stream, (const int*)head, ci_d, pi_d, Mi, C, (const int*)pt_start.p,
                       lay_cursor.p, lay_keys.p);
    hipLaunchKernelGGL(k_lay_rank, dim3(gM), dim3(256), 0, stream, head, (const unsigned long long*)lay_keys.p, pi_d, Mi, C,
                       (const int*)pt_start.p, lay_perm.p);
    hipLaunchKernelGGL(k_lay_gather<T>, dim3(gM), dim3(256), 0, stream, (const int*)head, (const int*)lay_perm.p,
                       reinterpret_cast<const double2*>(uv_d), ci_d, pi_d, w_d, Mi, C, uv_pm.p, ci_pm.p, pi_pm.p, wpm);
    if (C <= GROUP_CAMS)
      hipLaunchKernelGGL(k_lay_mask, dim3(gN), dim3(256), 0, stream, (const int*)head, (const int32_t*)ci_pm.p, (const int*)pt_start.p, N,
                         vis_mask.p);
    hipLaunchKernelGGL(k_lay_cm_count, dim3(nwg), dim3(256), 0, stream, (const int*)head, (const int32_t*)ci_pm.p, Mi, C, nwg, lay_counts.p);
    scan(lay_counts.p, ncnt, tC, lay_offs.p, 0, (int*)nullptr);
    hipLaunchKernelGGL(k_lay_cm_starts, dim3(1), dim3(256), 0, stream, (const int*)lay_offs.p, Mi, C, nwg, head);
    hipLaunchKernelGGL(k_lay_cm_scatter<T>, dim3(nwg), dim3(256), 0, stream, (const int*)head, (const int32_t*)ci_pm.p,
                       (const int32_t*)pi_pm.p, (const T2*)uv_pm.p, (const T*)wpm, Mi, C, nwg, (const int*)lay_offs.p, uv_cm.p, pi_cm.p,
                       has_w ? w_cm.p : (T*)nullptr);
    std::vector<int32_t> hs((size_t)N + 1 + LAY_HEAD);
    HIPCHK(hipMemcpyAsync(hs.data(), pt_start.p, sizeof(int32_t) * hs.size(), hipMemcpyDeviceToHost, stream));
    sync(); ++up_rep.stream_syncs;
    HIPCHK(hipGetLastError());
    const int32_t* hh = hs.data() + N + 1;
    up_rep.max_degree = hh[LAY_MAXDEG];
    up_rep.decline_reason = hh[LAY_BAD] != 0x7fffffff ? SBA_DECLINE_INDEX_RANGE : hh[LAY_MAXDEG] > PM_BLOCK ? SBA_DECLINE_DEGREE
                            : hh[LAY_DUP] ? SBA_DECLINE_DUPLICATE : SBA_DECLINE_NONE;
    if (up_rep.decline_reason != SBA_DECLINE_NONE) return false;
    identity_perm = !hh[LAY_UNSORTED] && (!hh[LAY_CAM_UNSORTED] || C > GROUP_CAMS);
    camcount.assign(hh + LAY_CAM_START, hh + LAY_CAM_START + C + 1);
    hs.resize((size_t)N + 1);
    ptstart.swap(hs);
    perm.clear();
    if (!identity_perm) {
      std::vector<int32_t> p32(M);
      HIPCHK(hipMemcpyAsync(p32.data(), lay_perm.p, sizeof(int32_t) * M, hipMemcpyDeviceToHost, stream));
      sync(); ++up_rep.stream_syncs;
      perm.resize(M);
      par_for(M, [&](int64_t lo, int64_t hi, int) { for (int64_t k = lo; k < hi; ++k) perm[k] = p32[k]; });
    }
    return true;
  }

  int get_layout(int64_t* perm_o, int32_t* pt_start_o, int32_t* cam_pm_o, int32_t* pt_pm_o, double* uv_pm_o, double* w_pm_o,
                 int32_t* pt_cm_o, double* uv_cm_o, double* w_cm_o, int32_t* cam_start_o, uint16_t* vis_o) override {
    if (!uploaded) { err = "sba_upload has not been called"; return SBA_ERR_STATE; }
    HIPCHK(hipSetDevice(device));
    if (perm_o) for (int64_t k = 0; k < M; ++k) perm_o[k] = identity_perm ? k : perm[k];
    auto ints = [&](const DevBuf<int32_t>& b, size_t cnt, int32_t* out) {
      if (out && cnt) HIPCHK(hipMemcpyAsync(out, b.p, sizeof(int32_t) * cnt, hipMemcpyDeviceToHost, stream));
    };
    ints(pt_start, (size_t)N + 1, pt_start_o); ints(ci_pm, M, cam_pm_o); ints(pi_pm, M, pt_pm_o); ints(pi_cm, M, pt_cm_o);
    std::vector<T2> u_pm(uv_pm_o ? M : 0), u_cm(uv_cm_o ? M : 0);
    std::vector<T> ww_pm(w_pm_o && has_w ? M : 0), ww_cm(w_cm_o && has_w ? M : 0);
    if (!u_pm.empty()) HIPCHK(hipMemcpyAsync(u_pm.data(), uv_pm.p, sizeof(T2) * M, hipMemcpyDeviceToHost, stream));
    if (!u_cm.empty()) HIPCHK(hipMemcpyAsync(u_cm.data(), uv_cm.p, sizeof(T2) * M, hipMemcpyDeviceToHost, stream));
    if (!ww_pm.empty()) HIPCHK(hipMemcpyAsync(ww_pm.data(), w_pm.p, sizeof(T) * M, hipMemcpyDeviceToHost, stream));
    if (!ww_cm.empty()) HIPCHK(hipMemcpyAsync(ww_cm.data(), w_cm.p, sizeof(T) * M, hipMemcpyDeviceToHost, stream));
    if (vis_o && has_vis_mask && N) HIPCHK(hipMemcpyAsync(vis_o, vis_mask.p, sizeof(uint16_t) * N, hipMemcpyDeviceToHost, stream));
    sync();
    for (size_t k = 0; k < u_pm.size(); ++k) { uv_pm_o[2 * k] = (double)u_pm[k].x; uv_pm_o[2 * k + 1] = (double)u_pm[k].y; }
    for (size_t k = 0; k < u_cm.size(); ++k) { uv_cm_o[2 * k] = (double)u_cm[k].x; uv_cm_o[2 * k + 1] = (double)u_cm[k].y; }
    if (w_pm_o) for (int64_t k = 0; k < M; ++k) w_pm_o[k] = has_w ? (double)ww_pm[k] : 1.0;
    if (w_cm_o) for (int64_t k = 0; k < M; ++k) w_cm_o[k] = has_w ? (double)ww_cm[k] : 1.0;
    if (cam_start_o) for (int c = 0; c <= C; ++c) cam_start_o[c] = cam_start_h[c];
    if (vis_o && !has_vis_mask) for (int p = 0; p < N; ++p) vis_o[p] = 0;
    return SBA_OK;
  }

  void set_params(const double* cams_h, const double* pts_h) {
    HIPCHK(hipMemcpyAsync(cams[cur].p, cams_h, sizeof(double) * C * NCP, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(pts[cur].p, pts_h, sizeof(double) * (size_t)N * 3, hipMemcpyHostToDevice, stream));
    std::vector<T> pt((size_t)N * 3);
    for (size_t i = 0; i < pt.size(); ++i) pt[i] = (T)pts_h[i];
    HIPCHK(hipMemcpyAsync(ptsT[cur].p, pt.data(), sizeof(T) * pt.size(), hipMemcpyHostToDevice, stream));
    cam_prep(cur);
    sync();
  }

  void cam_prep(int b) {
    hipLaunchKernelGGL(k_cam_prep<T>, dim3((C + 63) / 64), dim3(64), 0, stream, cams[b].p, campre[b].p, C);
  }

  size_t lds_cams() const { return (size_t)C * CAMPRE * sizeof(T); }

  // ------------------------------------------------------------------ kernel launchers
  // The LM kernels read the current / trial buffers through a device-resident pointer table that k_decide swaps on
  // acceptance; the host mirror `cur` is refreshed from LMState::cur whenever the state is read back.
  ParamSets<T> psets{};              // both buffer sets + the side that was current at lm_begin
  void push_ptrs() {                 // (re)build the by-value kernel argument for the host's notion of `cur`
    for (int b = 0; b < 2; ++b) { psets.cams[b] = cams[b].p; psets.pts[b] = pts[b].p; psets.ptsT[b] = ptsT[b].p; psets.campre[b] = campre[b].p; }
    psets.base = cur;
    psets.loss_delta = (T)loss_delta;
    psets.loss_kind = loss_kind;
    psets.fixed = has_fixed ? pt_fixed_mask.p : nullptr;
  }
  // argument for launches inside the LM loop (side = base ^ LMState::cur) ...
  ParamSets<T> ps_lm() const { return psets; }
  // ... and for launches outside it (st == nullptr): the host's current side
  ParamSets<T> ps_now() const { ParamSets<T> q = psets; q.base = cur; return q; }
  void launch_residual(T2* r_out) {
    const int g = (int)((M + PM_BLOCK - 1) / PM_BLOCK);
    if (g == 0) return;
    hipLaunchKernelGGL(k_residual<T>, dim3(g), dim3(PM_BLOCK), lds_cams(), stream, campre[cur].p, C, ptsT[cur].p,
                       uv_pm.p, has_w ? w_pm.p : nullptr, ci_pm.p, pi_pm.p, M, r_out, cost_part.p, RLoss<T>{(T)loss_delta, loss_kind});
  }
  void launch_resjac(T2* r_out) {
    const int g = (int)((M + PM_BLOCK - 1) / PM_BLOCK);
    if (g == 0) return;
    const size_t lds = (((size_t)C * CAMPRE + 3) & ~(size_t)3) * sizeof(T) + (size_t)PM_BLOCK * (2 * NCP + 7) * sizeof(T);
    hipLaunchKernelGGL(k_resjac<T>, dim3(g), dim3(PM_BLOCK), lds, stream, campre[cur].p, C, ptsT[cur].p, uv_pm.p,
                       has_w ? w_pm.p : nullptr, ci_pm.p, pi_pm.p, M, r_out, Jc_pm.p, Jp_pm.p);
  }
  // the route's choices that also depend on the solve: points-only mode (free_cams == 0) has no camera system
  bool free_cams() const { return h_state && h_state->free_cams; }
  // the linearisation is folded into the Schur kernel (k_schur_fused_bf3 and its kin) whenever the cameras are free
  bool fused() const { return rt.fused_ok && free_cams(); }
  bool lin_pts() const { return rt.lin_pts_ok && free_cams(); }   // f64: points linearised inside k_schur_sym
  // inside the LM loop with free cameras the wave linearisation also forms the trial's point factors (launch_schur skips k_point_factor)
  bool linp_folds_pf(const LMState* st) const { return st != nullptr && rt.linp_lw != 0 && free_cams() && !lin_pts() && !fused(); }
  int n_linp_blocks() const { return rt.linp_lw ? rt.nlinp : nblk; }
  int n_lin_parts() const { return (fused() || lin_pts()) ? rt.ksplit : n_linp_blocks(); }       // entries of cost_part / gmax_part
  bool backsub_dense() const { return rt.dense_one_group || rt.backsub_masked || rt.backsub_wide || rt.backsub_wave; }
  int n_trial_parts() const { return backsub_dense() ? rt.nbs_dense : nblk; }
  // several camera groups, fp32, indexed producers: the group pairs run on the bf16 pipe (k_schur_diag_bf3 / k_schur_offdiag_bf3)
  bool pairs_bf3() const { return rt.pairs_bf3 && !fused(); }
  // (the name is historical: every Schur kernel that takes the previous step's decision in its prologue -- k_schur_fused_bf3,
  //  k_schur_fused_wide(_f64), k_schur_fused_f64)
  bool bf3_path() const { return fused() && !sq_mode(); }

  // st == nullptr: unconditional (used outside the LM loop); otherwise the launch is a no-op once the solve has
  // terminated or when the last step was rejected and nothing has to be re-linearized
  void launch_linearize_points(const LMState* st) {
    if (nblk == 0) return;
    if (rt.linp_lw) {
      const uint16_t* tm = dense ? (const uint16_t*)nullptr : grp_mask.p;
      const int32_t* ts = dense ? (const int32_t*)nullptr : grp_start.p;
      T* pfp = linp_folds_pf(st) ? pfac.p : nullptr;
      const unsigned char* fx = has_fixed ? pt_fixed_mask.p : (const unsigned char*)nullptr;
      if (rt.linp_lw == 64)
        hipLaunchKernelGGL((k_linearize_points_wave<T, 64>), dim3(rt.nlinp), dim3(PM_BLOCK), 0, stream, st ? ps_lm() : ps_now(), st, C, uv_pm.p,
                           has_w ? w_pm.p : nullptr, N, tm, ts, V.p, gp.p, D2p.p, cost_part.p, gmax_part.p, pfp, fx);
      else
        hipLaunchKernelGGL((k_linearize_points_wave<T, 32>), dim3(rt.nlinp), dim3(PM_BLOCK), 0, stream, st ? ps_lm() : ps_now(), st, C, uv_pm.p,
                           has_w ? w_pm.p : nullptr, N, tm, ts, V.p, gp.p, D2p.p, cost_part.p, gmax_part.p, pfp, fx);
      return;
    }
    const size_t lds = (size_t)PM_BLOCK * 9 * sizeof(double) + lds_cams();
    hipLaunchKernelGGL(k_linearize_points<T>, dim3(nblk), dim3(PM_BLOCK), lds, stream, st ? ps_lm() : ps_now(), st, C,
                       uv_pm.p, has_w ? w_pm.p : nullptr, ci_pm.p, pi_pm.p, pt_start.p, blk_desc.p, V.p, gp.p, D2p.p,
                       cost_part.p, gmax_part.p);
  }
  void launch_linearize_cams(const LMState* st) {
    if (nchunk == 0) return;
    hipLaunchKernelGGL(k_linearize_cams<T>, dim3(nchunk), dim3(256), 0, stream, st ? ps_lm() : ps_now(), st, uv_cm.p,
                       has_w ? w_cm.p : nullptr, pi_cm.p, chunk_cam.p, chunk_begin.p, chunk_end.p, Upart.p);
    hipLaunchKernelGGL(k_reduce_cams, dim3(C), dim3(1024), 0, stream, Upart.p, cam_chunk_start.p, U.p, gc.p, st);
  }
  void launch_schur() {
    if (fused() && rt.fused_wide) { launch_schur_wide(); return; }
#if SBA_NCP == 11
    if (fused()) { launch_schur_fused(); return; }
#endif
    if constexpr (SCHUR_LIN_OK<T>) {
      if (lin_pts()) {
        using CfgD = SchurSel<T, true>;
        hipLaunchKernelGGL((k_schur_sym<T, true, false, true>), dim3(rt.ksplit, 1, CfgD::TS), dim3(CfgD::THREADS), CfgD::LDS_BYTES,
                           stream, ps_lm(), d_state.p, C, uv_pm.p, has_w ? w_pm.p : nullptr, ci_pm.p, pi_pm.p, pt_start.p, N,
                           pfac.p, pair_ga.p, pair_gb.p, 0, rt.ksplit, 1, slabs.p, bpart.p, (long long*)nullptr,
                           rt.dense_one_group ? (const uint16_t*)nullptr : vis_mask.p, D2p.p, gp.p, cost_part.p, gmax_part.p);
        return;
      }
    }
    if (N > 0 && !linp_folds_pf(d_state.p))
      hipLaunchKernelGGL(k_point_factor<T>, dim3((N + 255) / 256), dim3(256), 0, stream, V.p, gp.p, D2p.p, d_state.p, N, pfac.p,
                         has_fixed ? pt_fixed_mask.p : (const unsigned char*)nullptr);
    // pairs are stored diagonal ones first: [0, ngroups) are (g,g); the rest are (ga<gb)
    // a camera count that is not a multiple of 16 leaves the last group's panel mostly empty: the PARTIAL
    // instantiations skip the MFMAs of empty tiles (kept apart so that the full-group kernels pay nothing for it)
    // (f64 only: the f32 consumers are paced by their producers and lose more to the per-tile branches than they save)
    if constexpr (SCHUR_SYM<T>) {
      if (C % GROUP_CAMS != 0) { launch_schur_kernels<true>(); return; }
    }
    launch_schur_kernels<false>();
  }
  FusedDecide make_fused_decide(double*& gm_out) {
    FusedDecide fd{};
    fd.st_in = fd.st_out = d_state.p;
    gm_out = (gmax_cur == gmax_part.p) ? gmax_alt.p : gmax_part.p;      // never the array a decision may still read
    if (pending_decide) {
      st_slot ^= 1;
      fd.st_out = d_state_buf.p + st_slot;
      fd.do_decide = 1;
      fd.scal_all = pend_scal; fd.n_ranks = pend_ranks;
      fd.trial_part = trial_part.p; fd.gmax_in = gmax_cur;
      fd.n_trial = n_trial_parts(); fd.n_gmax = n_lin_parts();
      fd.log = reinterpret_cast<LMLogRow*>(d_log.p); fd.log_cap = LOG_CAP;
    }
    return fd;
  }
  // after a fused launch: the record it published is the current one, its gradient maxima the ones a decision reads next
  void fused_launched(const FusedDecide& fd, double* gm_out) {
    d_state.p = fd.st_out;
    pending_decide = false;
    gmax_cur = gm_out;
  }
  long long* fused_stamps() const { return (schur_debug && schur_debug_skip == 0) ? schur_dbg.p : nullptr; }
  // SBA_SCHUR_DEBUG=k: the stamps of the k-th fused Schur launch on stderr
  void print_fused_stamps(const char* kernel, const char* per, bool prologue) {
    if (!schur_debug) return;
    if (schur_debug_skip > 0) { --schur_debug_skip; return; }
    const std::vector<long long> st = read_stamps(schur_dbg, 64, stream);
    fprintf(stderr, "[%s stamps, cycles since the first producer stamp; per %s: producer-done consumer-done]\n", kernel, per);
    for (int i = 0; i < 14; ++i) fprintf(stderr, "  it %2d: P %7lld  C %7lld\n", i, st[2 * i] - st[0], st[2 * i + 1] - st[0]);
    fprintf(stderr, "  phases (cycles): prologue %lld | main loop %lld | fold U %lld | slab stores %lld | tail %lld | whole kernel %lld\n",
            st[49] - st[48], st[50] - st[49], st[51] - st[50], st[52] - st[51], st[53] - st[52], st[53] - st[48]);
    if (prologue) {
      fprintf(stderr, "  prologue (cycles): loads requested + LDS zeroed %lld | first barrier passed (record arrived) %lld | decision taken %lld | camera table in LDS %lld | producers set up %lld\n",
              st[54] - st[48], st[55] - st[48], st[57] - st[48], st[56] - st[48], st[49] - st[48]);
      if (st[58])
        fprintf(stderr, "  decision (cycles since kernel start): partial sums folded %lld | record updated %lld\n", st[58] - st[48], st[59] - st[48]);
    }
    schur_debug = false;
  }
#if SBA_NCP == 11
  // one camera group: k_schur_fused_bf3 (f32) / k_schur_fused_f64
  void launch_schur_fused() {
    double* gm_out = nullptr;
    const FusedDecide fd = make_fused_decide(gm_out);
    const uint16_t* vis = rt.fused_masked ? vis_mask.p : (const uint16_t*)nullptr;
    if constexpr (sizeof(T) == 4) {
      hipLaunchKernelGGL(k_schur_fused_bf3, dim3(rt.ksplit), dim3(SCHUR_THREADS), SchurBf3Cfg::LDS_BYTES, stream,
                         ps_lm(), fd, C, uv_pm.p, has_w ? w_pm.p : nullptr, pt_start.p, vis, N, rt.ksplit, D2p.p, gp.p, pfac.p,
                         slabs.p, bpart.p, gdpart.p, cost_part.p, gm_out, fused_stamps());
      fused_launched(fd, gm_out);
      print_fused_stamps("schur_fused", "chunk", true);
    } else {
      hipLaunchKernelGGL(k_schur_fused_f64, dim3(rt.ksplit), dim3(SCHUR_THREADS), SchurF64Cfg::LDS_BYTES, stream,
                         ps_lm(), fd, C, uv_pm.p, has_w ? w_pm.p : nullptr, pt_start.p, vis, N, rt.ksplit, D2p.p, gp.p, pfac.p,
                         slabs.p, bpart.p, gdpart.p, cost_part.p, gm_out, fused_stamps());
      fused_launched(fd, gm_out);
      print_fused_stamps("schur_fused_f64", "chunk", false);
    }
  }
#endif
  // the instantiation of the wide kernels for this rig: go(NTW, PW) with wide_ntw(C) row tiles, the route's points per wave
  template <typename F> void wide_dispatch(F&& go) const {
    using std::integral_constant;
    using P2 = integral_constant<int, 2>;
    auto pw = [&](auto ntw) { if (rt.wide_pw == 3) go(ntw, integral_constant<int, 3>{}); else go(ntw, P2{}); };
    switch (wide_ntw(C)) {
      case 8: if constexpr (sizeof(T) == 4) pw(integral_constant<int, 8>{}); break;      // (fp64: 17 cameras and more, 12 tiles at least)
      case 12: pw(integral_constant<int, 12>{}); break;
      case 13: pw(integral_constant<int, 13>{}); break;
      case 14: go(integral_constant<int, 14>{}, P2{}); break;
      case 15: go(integral_constant<int, 15>{}, P2{}); break;
      default: go(integral_constant<int, 16>{}, P2{}); break;
    }
  }
  // k_schur_fused_wide (f32) / k_schur_fused_wide_f64: one launch, compact rows
  void launch_schur_wide() {
    double* gm_out = nullptr;
    const FusedDecide fd = make_fused_decide(gm_out);
    // sparse rigs: per (16-camera group, point) visibility mask + index of the point's first observation in the group -- the
    // k_group_index tables with several groups, the one-group mask and the point's start otherwise
    const bool tables = !dense;
    const uint16_t* tmask = !tables ? nullptr : C > GROUP_CAMS ? grp_mask.p : vis_mask.p;
    const int32_t* tstart = !tables ? nullptr : C > GROUP_CAMS ? grp_start.p : pt_start.p;
    wide_dispatch([&](auto ntw_c, auto pw_c) {
      constexpr int NTW = decltype(ntw_c)::value, PW = decltype(pw_c)::value;
      if constexpr (sizeof(T) == 4) {
        constexpr size_t lds = SchurWideCfg<NTW, PW>::LDS_BYTES;
        hipLaunchKernelGGL((k_schur_fused_wide<NTW, PW>), dim3(rt.ksplit), dim3(SCHUR_THREADS), lds, stream,
                           ps_lm(), fd, C, uv_pm.p, has_w ? w_pm.p : nullptr, tmask, tstart, N, rt.ksplit, D2p.p, gp.p, pfac.p, slabs.p,
                           bpart.p, gdpart.p, cost_part.p, gm_out, fused_stamps());
      } else {
#if SBA_NCP == 11
        constexpr int TS = NTW > 13 ? 2 : 1;      // = rt.wide_ts
        constexpr size_t lds64 = SchurWide64Cfg<NTW, PW, TS>::LDS_BYTES;
        hipLaunchKernelGGL((k_schur_fused_wide_f64<NTW, PW, TS>), dim3(rt.ksplit, TS), dim3(SCHUR_THREADS), lds64, stream,
                           ps_lm(), fd, C, uv_pm.p, has_w ? w_pm.p : nullptr, tmask, tstart, N, rt.ksplit, D2p.p, gp.p, pfac.p, slabs.p,
                           bpart.p, gdpart.p, cost_part.p, gm_out, fused_stamps());
#endif
      }
    });
    fused_launched(fd, gm_out);
    if constexpr (sizeof(T) == 4) print_fused_stamps("schur_fused_wide", "round", false);
    else print_fused_stamps("schur_fused_wide_f64", "chunk of 8 or 12 points", false);
  }
  template <bool PARTIAL> void launch_schur_kernels() {
    using CfgD = SchurSel<T, true>;
    using CfgO = SchurSel<T, false>;
    const int ksplit = rt.ksplit;
    if constexpr (SCHUR_SYM<T>) {
      hipLaunchKernelGGL((k_schur_sym<T, true, PARTIAL>), dim3(ksplit, ngroups, CfgD::TS), dim3(CfgD::THREADS), CfgD::LDS_BYTES,
                         stream, ps_lm(), d_state.p, C, uv_pm.p, has_w ? w_pm.p : nullptr, ci_pm.p, pi_pm.p, pt_start.p, N,
                         pfac.p, pair_ga.p, pair_gb.p, 0, ksplit, (int)dense, slabs.p, bpart.p, schur_debug ? schur_dbg.p : nullptr,
                         (const uint16_t*)nullptr, (double*)nullptr, (double*)nullptr, (double*)nullptr, (double*)nullptr,
                         grp_indexed ? grp_mask.p : (const uint16_t*)nullptr, grp_indexed ? grp_start.p : (const int32_t*)nullptr);
      if (schur_debug) {
        const std::vector<long long> st = read_stamps(schur_dbg, 64, stream);
        fprintf(stderr, "[schur_sym stamps, cycles; per chunk: produce-done after-barrier consume-done]\n");
        for (int i = 0; i < 8; ++i)
          fprintf(stderr, "  it %2d: P %7lld  B %7lld  C %7lld\n", i, st[3 * i] - st[0], st[3 * i + 1] - st[0], st[3 * i + 2] - st[0]);
        schur_debug = false;
      }
      if (npairs > ngroups)
        hipLaunchKernelGGL((k_schur_sym<T, false, PARTIAL>), dim3(ksplit, npairs - ngroups, CfgO::TS), dim3(CfgO::THREADS),
                           CfgO::LDS_BYTES, stream, ps_lm(), d_state.p, C, uv_pm.p,
                           has_w ? w_pm.p : nullptr, ci_pm.p, pi_pm.p, pt_start.p, N, pfac.p,
                           pair_ga.p, pair_gb.p, ngroups, ksplit, (int)dense, slabs.p, bpart.p, nullptr,
                           (const uint16_t*)nullptr, (double*)nullptr, (double*)nullptr, (double*)nullptr, (double*)nullptr,
                           grp_indexed ? grp_mask.p : (const uint16_t*)nullptr, grp_indexed ? grp_start.p : (const int32_t*)nullptr);
    } else {
      if (pairs_bf3())
        hipLaunchKernelGGL(k_schur_diag_bf3, dim3(ksplit, ngroups), dim3(SCHUR_THREADS), SchurPairCfg::LDS_BYTES, stream,
                           ps_lm(), d_state.p, C, uv_pm.p, has_w ? w_pm.p : nullptr, grp_mask.p, grp_start.p, N, pfac.p, pair_ga.p, 0, ksplit,
                           slabs.p, bpart.p, rt.pairs_fold_u ? gdpart.p : (double*)nullptr);
      else
        hipLaunchKernelGGL((k_schur<T, true, PARTIAL>), dim3(ksplit, ngroups, CfgD::TS), dim3(CfgD::THREADS), CfgD::LDS_BYTES,
                           stream, ps_lm(), d_state.p, C, uv_pm.p, has_w ? w_pm.p : nullptr, ci_pm.p, pi_pm.p, pt_start.p, N,
                           pfac.p, pair_ga.p, pair_gb.p, 0, ksplit, (int)dense, slabs.p, bpart.p,
                           schur_debug ? schur_dbg.p : nullptr, grp_indexed ? grp_mask.p : (const uint16_t*)nullptr,
                           grp_indexed ? grp_start.p : (const int32_t*)nullptr);
      if (schur_debug) {
        const std::vector<long long> st = read_stamps(schur_dbg, 64, stream);
        fprintf(stderr, "[schur stamps, cycles since first barrier; per chunk: producer-done consumer-done barrier-out]\n");
        for (int i = 0; i < 14; ++i)
          fprintf(stderr, "  it %2d: P %7lld  C %7lld  out %7lld\n", i, st[3 * i] - st[2], st[3 * i + 1] - st[2], st[3 * i + 2] - st[2]);
        schur_debug = false;
      }
      if (npairs > ngroups) {
        if (pairs_bf3())
          hipLaunchKernelGGL(k_schur_offdiag_bf3, dim3(ksplit, npairs - ngroups), dim3(SCHUR_THREADS), SchurBf3OffCfg::LDS_BYTES, stream,
                             ps_lm(), d_state.p, C, uv_pm.p, has_w ? w_pm.p : nullptr, grp_mask.p, grp_start.p, N, pfac.p, pair_ga.p, pair_gb.p,
                             ngroups, ksplit, slabs.p);
        else
          hipLaunchKernelGGL((k_schur<T, false, PARTIAL>), dim3(ksplit, npairs - ngroups, CfgO::TS), dim3(CfgO::THREADS),
                             CfgO::LDS_BYTES, stream, ps_lm(), d_state.p, C, uv_pm.p,
                             has_w ? w_pm.p : nullptr, ci_pm.p, pi_pm.p, pt_start.p, N, pfac.p,
                             pair_ga.p, pair_gb.p, ngroups, ksplit, (int)dense, slabs.p, bpart.p, nullptr,
                             grp_indexed ? grp_mask.p : (const uint16_t*)nullptr, grp_indexed ? grp_start.p : (const int32_t*)nullptr);
      }
    }
  }
  void launch_backsub_trial() {
    if (nblk == 0) return;
    const int nbs = rt.nbs_dense;
    const uint16_t* gm = dense ? (const uint16_t*)nullptr : grp_mask.p;
    const int32_t* gs = dense ? (const int32_t*)nullptr : grp_start.p;
    if (rt.backsub_pack) {
      hipLaunchKernelGGL((k_backsub_dense<T, 0>), dim3(nbs), dim3(PM_BLOCK), 0, stream, ps_lm(), C, uv_pm.p,
                         has_w ? w_pm.p : nullptr, N, pfac.p, gp.p, D2p.p, delta_c.p, d_state.p, trial_part.p, nbs, gm, gs);
      return;
    }
    if (rt.backsub_wave) {
      hipLaunchKernelGGL((k_backsub_dense<T, 64>), dim3(nbs), dim3(PM_BLOCK), 0, stream, ps_lm(), C, uv_pm.p,
                         has_w ? w_pm.p : nullptr, N, pfac.p, gp.p, D2p.p, delta_c.p, d_state.p, trial_part.p, nbs, gm, gs);
      return;
    }
    if (rt.backsub_wide) {
      hipLaunchKernelGGL((k_backsub_dense<T, 32>), dim3(nbs), dim3(PM_BLOCK), 0, stream, ps_lm(), C, uv_pm.p,
                         has_w ? w_pm.p : nullptr, N, pfac.p, gp.p, D2p.p, delta_c.p, d_state.p, trial_part.p, nbs, gm, gs);
      return;
    }
    if (backsub_dense()) {      // one group: dense, or through the visibility mask
      hipLaunchKernelGGL(k_backsub_dense<T>, dim3(nbs), dim3(PM_BLOCK), 0, stream, ps_lm(), C, uv_pm.p,
                         has_w ? w_pm.p : nullptr, N, pfac.p, gp.p, D2p.p, delta_c.p, d_state.p, trial_part.p, nbs,
                         rt.dense_one_group ? (const uint16_t*)nullptr : vis_mask.p, rt.dense_one_group ? (const int32_t*)nullptr : pt_start.p);
      return;
    }
    const size_t lds = (size_t)PM_BLOCK * 6 * sizeof(double) + (2 * (size_t)C * CAMPRE + (size_t)C * NCP) * sizeof(T);
    hipLaunchKernelGGL(k_backsub_trial<T>, dim3(nblk), dim3(PM_BLOCK), lds, stream, ps_lm(), C,
                       uv_pm.p, has_w ? w_pm.p : nullptr, ci_pm.p, pi_pm.p, pt_start.p, blk_desc.p,
                       pfac.p, gp.p, D2p.p, delta_c.p, d_state.p, trial_part.p, nblk);
  }

  // ------------------------------------------------------------------ model evaluation entry points
  int residual(const double* x, double* r_out, double* cost_out) override {
    if (!uploaded) { err = "sba_upload has not been called"; return SBA_ERR_STATE; }
    HIPCHK(hipSetDevice(device));
    if (x) set_params(x, x + (size_t)C * NCP);
    if (r_out && r_pm.n != (size_t)M) r_pm.alloc(M);
    launch_residual(r_out ? r_pm.p : nullptr);
    const int g = (int)((M + PM_BLOCK - 1) / PM_BLOCK);
    std::vector<double> part_v((size_t)g > LAND_DOUBLES ? g : 0);
    double* part = part_v.empty() ? h_land : part_v.data();
    if (g) HIPCHK(hipMemcpyAsync(part, cost_part.p, sizeof(double) * g, hipMemcpyDeviceToHost, stream));
    std::vector<T2> r(r_out ? M : 0);
    if (r_out && M) HIPCHK(hipMemcpyAsync(r.data(), r_pm.p, sizeof(T2) * M, hipMemcpyDeviceToHost, stream));
    sync();
    HIPCHK(hipGetLastError());
    double c = 0;
    for (int i = 0; i < g; ++i) c += part[i];
    if (cost_out) *cost_out = c;
    if (r_out)
      par_for(M, [&](int64_t lo, int64_t hi, int) {
        for (int64_t k = lo; k < hi; ++k) { const int64_t i = identity_perm ? k : perm[k]; r_out[2 * i] = (double)r[k].x; r_out[2 * i + 1] = (double)r[k].y; }
      });
    return SBA_OK;
  }

  int residual_jacobian(const double* x, double* r_out, double* Jc_out, double* Jp_out) override {
    if (!uploaded) { err = "sba_upload has not been called"; return SBA_ERR_STATE; }
    HIPCHK(hipSetDevice(device));
    if (x) set_params(x, x + (size_t)C * NCP);
    if (r_pm.n != (size_t)M) r_pm.alloc(M);
    if (Jc_pm.n != (size_t)M * 2 * NCP) { Jc_pm.alloc((size_t)M * 2 * NCP); Jp_pm.alloc((size_t)M * 6); }
    launch_resjac(r_pm.p);
    std::vector<T2> r(M);
    std::vector<T> jc((size_t)M * 2 * NCP), jp((size_t)M * 6);
    if (M) {
      HIPCHK(hipMemcpyAsync(r.data(), r_pm.p, sizeof(T2) * M, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipMemcpyAsync(jc.data(), Jc_pm.p, sizeof(T) * jc.size(), hipMemcpyDeviceToHost, stream));
      HIPCHK(hipMemcpyAsync(jp.data(), Jp_pm.p, sizeof(T) * jp.size(), hipMemcpyDeviceToHost, stream));
    }
    sync();
    HIPCHK(hipGetLastError());
    for (int64_t k = 0; k < M; ++k) {
      const int64_t i = identity_perm ? k : perm[k];
      if (r_out) { r_out[2 * i] = (double)r[k].x; r_out[2 * i + 1] = (double)r[k].y; }
      if (Jc_out) for (int e = 0; e < 2 * NCP; ++e) Jc_out[(size_t)i * 2 * NCP + e] = (double)jc[(size_t)k * 2 * NCP + e];
      if (Jp_out) for (int e = 0; e < 6; ++e) Jp_out[(size_t)i * 6 + e] = (double)jp[(size_t)k * 6 + e];
    }
    return SBA_OK;
  }

  // ------------------------------------------------------------------ squared-pixel-error variants (pySBA.py:151-205)
  bool sq_mode() const { return opts.mode == SBA_MODE_CAMS_ONLY_SQ || opts.mode == SBA_MODE_TRANSFORM_SQ; }
  int nblk_sq = 0, nchunk_sq = 0;
  DevBuf<double> sq_part, sq_16, theta[2];
  DevBuf<int32_t> sq_start;
  double h_theta[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  ThetaSets tsets() const { ThetaSets t; t.th[0] = theta[0].p; t.th[1] = theta[1].p; t.base = cur_at_begin; return t; }
  void sq_setup() {
    nblk_sq = (int)((M + PM_BLOCK - 1) / PM_BLOCK);
    std::vector<int32_t> st;
    if (opts.mode == SBA_MODE_CAMS_ONLY_SQ) {          // one 16x16 per camera, from the camera-major chunks
      nchunk_sq = nchunk;
      sq_16.alloc((size_t)C * 256);
    } else {                                           // one 16x16 for the whole problem
      nchunk_sq = (int)((M + SQ_CHUNK - 1) / SQ_CHUNK);
      st = {0, nchunk_sq};
      sq_start.upload(st, stream);
      sq_16.alloc(256);
      for (int b = 0; b < 2; ++b) if (theta[b].n != 12) theta[b].alloc(12);
    }
    sq_part.alloc((size_t)std::max(nchunk_sq, 1) * 256);
    if (trial_part.n < (size_t)4 * std::max(nblk_sq, 1)) trial_part.alloc((size_t)4 * std::max(nblk_sq, 1));
    if (gmax_part.n < (size_t)std::max(nblk_sq, 1)) gmax_part.alloc(std::max(nblk_sq, 1));
    gmax_part.zero(stream);
  }
  void launch_sq_linearize(const LMState* st) {
    if (nchunk_sq == 0) return;
    const ParamSets<T> ps = st ? ps_lm() : ps_now();
    ThetaSets ts = tsets();
    if (!st) ts.base = cur;
    if (opts.mode == SBA_MODE_CAMS_ONLY_SQ) {
      const size_t lds = ((size_t)4 * 16 * 130 + CAMPRE) * sizeof(T);
      hipLaunchKernelGGL((k_sq_linearize<T, 1>), dim3(nchunk_sq), dim3(256), lds, stream, ps, ts, st, C, uv_cm.p,
                         has_w ? w_cm.p : nullptr, (const int32_t*)nullptr, pi_cm.p, chunk_cam.p, chunk_begin.p, chunk_end.p, M, sq_part.p);
      hipLaunchKernelGGL(k_reduce16, dim3(C), dim3(1024), 0, stream, sq_part.p, cam_chunk_start.p, sq_16.p, st);
    } else {
      const size_t lds = ((size_t)4 * 16 * 130 + (size_t)C * CAMPRE) * sizeof(T);
      hipLaunchKernelGGL((k_sq_linearize<T, 2>), dim3(nchunk_sq), dim3(256), lds, stream, ps, ts, st, C, uv_pm.p,
                         has_w ? w_pm.p : nullptr, ci_pm.p, pi_pm.p, (const int32_t*)nullptr, (const int32_t*)nullptr,
                         (const int32_t*)nullptr, M, sq_part.p);
      hipLaunchKernelGGL(k_reduce16, dim3(1), dim3(1024), 0, stream, sq_part.p, sq_start.p, sq_16.p, st);
    }
  }
  void launch_sq_trial() {
    if (nblk_sq == 0) return;
    if (opts.mode == SBA_MODE_CAMS_ONLY_SQ)
      hipLaunchKernelGGL((k_sq_trial<T, 1>), dim3(nblk_sq), dim3(PM_BLOCK), lds_cams(), stream, ps_lm(), tsets(), d_state.p, C,
                         uv_pm.p, has_w ? w_pm.p : nullptr, ci_pm.p, pi_pm.p, M, trial_part.p, nblk_sq);
    else
      hipLaunchKernelGGL((k_sq_trial<T, 2>), dim3(nblk_sq), dim3(PM_BLOCK), lds_cams(), stream, ps_lm(), tsets(), d_state.p, C,
                         uv_pm.p, has_w ? w_pm.p : nullptr, ci_pm.p, pi_pm.p, M, trial_part.p, nblk_sq);
  }
  // the phase API's trial scalars (a caller that hands lm_decide a scalar array): the same fold of k_sq_trial's partials k_decide does
  void launch_sq_scalars(double* scal) {
    if (scal)
      hipLaunchKernelGGL(k_trial_scalars, dim3(1), dim3(DECIDE_THREADS), 0, stream, trial_part.p, gmax_rd(), nblk_sq, nblk_sq, d_state.p, scal);
  }
  // cost (0.5 sum rho^2) and max |gradient| from the 16x16 sums of the last squared-variant linearization
  void sq_read(double& cost, double& gmax) {
    const int ng = (opts.mode == SBA_MODE_CAMS_ONLY_SQ) ? C : 1;
    const int np = (opts.mode == SBA_MODE_CAMS_ONLY_SQ) ? NCP : 12;
    std::vector<double> h((size_t)ng * 256);
    HIPCHK(hipMemcpyAsync(h.data(), sq_16.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, stream));
    sync();
    cost = 0; gmax = 0;
    for (int g = 0; g < ng; ++g) {
      cost += 0.5 * h[(size_t)g * 256 + np * 16 + np];
      for (int i = 0; i < np; ++i) gmax = std::max(gmax, std::fabs(h[(size_t)g * 256 + i * 16 + np]));
    }
  }

  // shared intrinsics (pySBA.py:252-325): unknowns [f,k1,k2 | 6 extrinsics x C | 2 centre x C], pySBA.py:313 order
  // (tangential model: the per-camera tail is [p1, p2, cx, cy])
  void build_tie_tables() {
    constexpr int PC = NCP - 9;          // per-camera intrinsics that stay free: cx, cy (+ p1, p2 in the tangential model)
    n_tied = 3 + (6 + PC) * C;
    std::vector<int32_t> tie(n), start(n_tied + 1, 0), idx(n), firstv(n_tied);
    for (int c = 0; c < C; ++c)
      for (int e = 0; e < NCP; ++e)
        tie[c * NCP + e] = e < 6 ? 3 + 6 * c + e : e < 9 ? e - 6 : 3 + 6 * C + PC * c + (e - 9);
    for (int i = 0; i < n; ++i) start[tie[i] + 1]++;
    for (int a = 0; a < n_tied; ++a) start[a + 1] += start[a];
    std::vector<int32_t> fill(start.begin(), start.end() - 1);
    for (int i = 0; i < n; ++i) idx[fill[tie[i]]++] = i;
    for (int a = 0; a < n_tied; ++a) firstv[a] = idx[start[a]];
    h_tie = tie;
    tie_map.upload(tie, stream); tie_pre_start.upload(start, stream); tie_pre_idx.upload(idx, stream); tie_first.upload(firstv, stream);
    E_tied.alloc((size_t)n_tied * n_tied + 3 * (size_t)n_tied + 1);
    sync();
  }
  int n_tied = 0;
  std::vector<int32_t> h_tie;
  DevBuf<int32_t> tie_map, tie_pre_start, tie_pre_idx, tie_first;
  DevBuf<double> E_tied;

  // ------------------------------------------------------------------ LM phases
  int64_t exchange_size() const override { return (int64_t)n * n + 3 * (int64_t)n + 1; }
  static constexpr int LOG_CAP = 4096;
  static constexpr int BATCH = 4;      // LM iterations enqueued between two host polls of the state

  // ------------------------------------------------------------------ multi-rank plumbing (RCCL on the engine's stream)
  int comm_init(const uint8_t* id, int rank, int n_ranks) override {
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks || !id) { err = "bad communicator arguments"; return SBA_ERR_INVALID; }
    if (ipc_on || ipc_mine) { err = "the handle already has a peer-mapped exchange area (sba_ipc_export): the two exchanges are exclusive"; return SBA_ERR_STATE; }
    Rccl& r = Rccl::get();
    if (!r.ok) { err = r.why; return SBA_ERR_UNSUPPORTED; }
    HIPCHK(hipSetDevice(device));
    if (comm) { (void)r.comm_destroy(comm); comm = nullptr; }
    Rccl::UniqueId uid;
    memcpy(uid.internal, id, Rccl::ID_BYTES);
    RCCLCHK(r.comm_init_rank(&comm, n_ranks, uid, rank));
    comm_rank = rank; comm_n = n_ranks;
    // (a handle may be given a new communicator: the bump arena never returns memory, so only grow)
    if (sc_loc.n < (size_t)NSCAL) sc_loc.alloc(NSCAL);
    if (sc_all.n < (size_t)NSCAL * n_ranks) sc_all.alloc((size_t)NSCAL * n_ranks);
    if (comm_tmp.n < (size_t)std::max(n, 1) + 8) comm_tmp.alloc(std::max(n, 1) + 8);
    if (!h_comm) HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h_comm), sizeof(double) * (std::max(n, 1) + 8), hipHostMallocDefault));
    return SBA_OK;
  }
  // in-place all-reduce of a few host doubles (begin / finish only: the LM loop itself never leaves the device)
  // ------------------------------------------------------------------ one-shot exchange (sba_ipc.hpp)
  void ipc_close_peers() {
    for (size_t r = 0; r < ipc_area.size(); ++r)
      if (ipc_area[r] && r < ipc_opened.size() && ipc_opened[r]) (void)hipIpcCloseMemHandle(ipc_area[r]);
    ipc_area.clear(); ipc_opened.clear();
  }
  int ipc_export(int n_ranks, uint8_t* handle_out) override {
    if (n_ranks < 1 || !handle_out) { err = "bad arguments"; return SBA_ERR_INVALID; }
    if (ipc_on || ipc_mine) { err = "the handle already has an exchange area"; return SBA_ERR_STATE; }
    if (comm) { err = "the handle already has an RCCL communicator (the two exchanges are exclusive)"; return SBA_ERR_STATE; }
    HIPCHK(hipSetDevice(device));
    ipc_L = IpcLayout::make(n);
    void* pmem = nullptr;
    // uncached: the peers read what this rank's kernels wrote without a kernel boundary of THEIR stream in between.  A cached
    // allocation would still work between ranks that share one device (one L2) but not between GPUs, so it is never taken
    // silently: SBA_IPC_ALLOW_CACHED=1 asks for it (one-card rehearsals on a stack without the uncached flag) and says so.
    if (hipExtMallocWithFlags(&pmem, ipc_L.total * sizeof(double), hipDeviceMallocUncached) != hipSuccess) {
      (void)hipGetLastError();
      if (!kn.ipc_allow_cached) {
        err = "sba_ipc_export: uncached device memory (hipDeviceMallocUncached) is not available; the one-shot exchange needs it between GPUs "
              "(SBA_IPC_ALLOW_CACHED=1 accepts cached memory for ranks that share ONE device)";
        return SBA_ERR_HIP;
      }
      fprintf(stderr, "[sba_ipc] warning: exchange area in CACHED device memory (SBA_IPC_ALLOW_CACHED=1): valid between ranks on one device only\n");
      HIPCHK(hipMalloc(&pmem, ipc_L.total * sizeof(double)));
    }
    ipc_mine = static_cast<double*>(pmem);
    HIPCHK(hipMemsetAsync(ipc_mine, 0, ipc_L.total * sizeof(double), stream));
    sync();
    hipIpcMemHandle_t hm;
    HIPCHK(hipIpcGetMemHandle(&hm, ipc_mine));
    static_assert(sizeof(hm) == SBA_IPC_HANDLE_BYTES, "hipIpcMemHandle_t is 64 bytes");
    memcpy(handle_out, &hm, sizeof hm);
    memcpy(ipc_my_handle, &hm, sizeof hm);
    // ranks that live in the SAME process (several handles, one per thread or per device) cannot open each other's handles
    // (hipIpcOpenMemHandle refuses the exporting process): they find the pointer here instead
    IpcLocalAreas::get().add(ipc_my_handle, ipc_mine);
    ipc_planned = n_ranks;
    return SBA_OK;
  }
  int ipc_attach(int rank, int n_ranks, const uint8_t* handles) override {
    if (!ipc_mine || n_ranks != ipc_planned || rank < 0 || rank >= n_ranks || !handles) { err = "sba_ipc_export first, with the same n_ranks"; return SBA_ERR_STATE; }
    if (comm) { err = "the handle already has an RCCL communicator"; return SBA_ERR_STATE; }
    if (ipc_on) { err = "the handle is already attached to its peers' exchange areas"; return SBA_ERR_STATE; }
    HIPCHK(hipSetDevice(device));
    ipc_area.assign(n_ranks, nullptr);
    ipc_opened.assign(n_ranks, 0);
    for (int r = 0; r < n_ranks; ++r) {
      if (r == rank) { ipc_area[r] = ipc_mine; continue; }
      if (double* local = IpcLocalAreas::get().find(handles + (size_t)r * SBA_IPC_HANDLE_BYTES)) { ipc_area[r] = local; continue; }
      hipIpcMemHandle_t hp;
      memcpy(&hp, handles + (size_t)r * SBA_IPC_HANDLE_BYTES, sizeof hp);
      void* q = nullptr;
      const hipError_t oe = hipIpcOpenMemHandle(&q, hp, hipIpcMemLazyEnablePeerAccess);
      if (oe != hipSuccess) {
        (void)hipGetLastError();
        ipc_close_peers();
        err = std::string("hipIpcOpenMemHandle of rank ") + std::to_string(r) + "'s area failed: " + hipGetErrorString(oe);
        return SBA_ERR_HIP;
      }
      ipc_area[r] = static_cast<double*>(q);
      ipc_opened[r] = 1;
    }
    // ranks that share this card: their launches compete for its CUs, and k_chol_big_dag's progress argument (in-order dispatch of
    // ONE launch) does not cover several such launches holding each other's CUs on different XCDs -- they get the per-column launches
    card_shared = false;
    for (int r = 0; r < n_ranks; ++r) {
      if (r == rank) continue;
      hipPointerAttribute_t at;
      if (hipPointerGetAttributes(&at, ipc_area[r]) == hipSuccess) { if (at.device == device) card_shared = true; }
      else (void)hipGetLastError();
    }
    if (chol.debug) fprintf(stderr, "[sba_ipc_attach] rank %d of %d: %s\n", rank, n_ranks, card_shared ? "a peer's exchange area lives on this device: ranks share the card (per-column launches for the large Cholesky)" : "no peer on this device");
    ipc_ptrs.upload(ipc_area, stream);
    if (ipc_fail.n == 0) ipc_fail.alloc(1);
    ipc_fail.zero(stream);
    comm_rank = rank; comm_n = n_ranks;
    if (sc_all.n < (size_t)NSCAL * n_ranks) sc_all.alloc((size_t)NSCAL * n_ranks);
    if (comm_tmp.n < (size_t)std::max(n, 1) + 8) comm_tmp.alloc(std::max(n, 1) + 8);
    if (!h_comm) HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h_comm), sizeof(double) * (std::max(n, 1) + 8), hipHostMallocDefault));
    sync();
    ipc_on = true;
    return SBA_OK;
  }
  void ipc_publish(int kind, unsigned long long seq, const LMState* st) {
    hipLaunchKernelGGL(k_ipc_publish, dim3(1), dim3(1), 0, stream, ipc_mine, ipc_L.flag_of(kind, (int)(seq & 1)), seq, st);
  }
  void ipc_gate(int kind, unsigned long long seq, LMState* st, size_t copy_off, int ncopy, double* dst) {
    hipLaunchKernelGGL(k_ipc_gate, dim3(1), dim3(64), 0, stream, ipc_ptrs.p, comm_n, ipc_L.flag_of(kind, (int)(seq & 1)), seq, st,
                       st ? (int*)nullptr : ipc_fail.p, copy_off, ncopy, dst, kn.ipc_timeout_ticks);
  }
  void comm_reduce(double* v, int count, int op) {
    for (int i = 0; i < count; ++i) h_comm[i] = v[i];
    if (ipc_on) {
      // after a timeout the ranks' exchange counters no longer agree (some passed the gate, some did not): the handle cannot
      // take part in another exchange and has to be destroyed -- on every rank
      if (ipc_dead) throw HipError{hipErrorNotReady, "an earlier exchange of this handle timed out (sba_ipc): destroy it and start over", __FILE__, __LINE__};
      const unsigned long long s = ++ipc_seq[2];
      const size_t slot = ipc_L.vec_slot((int)(s & 1));
      HIPCHK(hipMemcpyAsync(ipc_mine + slot, h_comm, sizeof(double) * count, hipMemcpyHostToDevice, stream));
      ipc_publish(2, s, nullptr);
      ipc_gate(2, s, nullptr, 0, 0, nullptr);
      hipLaunchKernelGGL(k_ipc_reduce_vec, dim3(1), dim3(256), 0, stream, ipc_ptrs.p, comm_n, slot, count, op == Rccl::kMax ? 1 : 0, comm_tmp.p);
      int failed = 0;
      HIPCHK(hipMemcpyAsync(h_comm, comm_tmp.p, sizeof(double) * count, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipMemcpyAsync(&failed, ipc_fail.p, sizeof(int), hipMemcpyDeviceToHost, stream));
      sync();
      if (failed) { ipc_dead = true; throw HipError{hipErrorNotReady, "a peer rank did not reach the exchange in time (sba_ipc; SBA_IPC_TIMEOUT_S, default 5 s)", __FILE__, __LINE__}; }
      for (int i = 0; i < count; ++i) v[i] = h_comm[i];
      return;
    }
    HIPCHK(hipMemcpyAsync(comm_tmp.p, h_comm, sizeof(double) * count, hipMemcpyHostToDevice, stream));
    RCCLCHK(Rccl::get().all_reduce(comm_tmp.p, comm_tmp.p, count, Rccl::kFloat64, op, comm, stream));
    HIPCHK(hipMemcpyAsync(h_comm, comm_tmp.p, sizeof(double) * count, hipMemcpyDeviceToHost, stream));
    sync();
    for (int i = 0; i < count; ++i) v[i] = h_comm[i];
  }
  void comm_sum(double* v, int count) { comm_reduce(v, count, Rccl::kSum); }
  void comm_max(double* v, int count) { comm_reduce(v, count, Rccl::kMax); }

  int lm_begin(const sba_lm_opts* o) override {
    if (!uploaded) { err = "sba_upload has not been called"; return SBA_ERR_STATE; }
    HIPCHK(hipSetDevice(device));
    opts = *o;
    st_slot = 0;
    d_state.p = d_state_buf.p;
    pending_decide = false;
    prof_on = opts.reserved[0] != 0;
    for (int k = 0; k < KP_N; ++k) { prof_us[k] = 0; prof_cnt[k] = 0; }
    for (auto& u : pev_used) u = false;
    if (opts.mode < SBA_MODE_FULL || opts.mode > SBA_MODE_TRANSFORM_SQ) { err = "unsupported mode"; return SBA_ERR_UNSUPPORTED; }
    if (opts.mode == SBA_MODE_SHARED_INTR) build_tie_tables();
    // initial cost; scipy raises ValueError when it is not finite (least_squares.py:844-845)
    double c0 = 0;
    int rc = SBA_OK;
    if (multi() && sq_mode() && comm_n > 1) { err = "the squared-error variants (camonly, transform_points_3d) run on one GPU only"; return SBA_ERR_UNSUPPORTED; }  // (same on every rank)
    // With a communicator a failure on THIS rank must not keep it out of the collective its peers are about to enter: the
    // failure travels as a flag inside that all-reduce and every rank returns an error together.
    try { rc = residual(nullptr, nullptr, &c0); }
    catch (const HipError& e) {
      if (!multi()) throw;
      err = std::string("HIP error in lm_begin: ") + hipGetErrorString(e.e) + " (" + e.what + ")";
      rc = SBA_ERR_HIP;
    }
    if (rc && !multi()) return rc;
    N_global = N;
    if (multi()) {
      // every rank must see the same initial cost (a non-finite one on ANY rank fails the solve on ALL of them, before the
      // first collective of the loop) and the same default evaluation budget, 100 x the GLOBAL number of parameters
      double v[3] = {rc ? 0.0 : c0, (double)N, rc ? 1.0 : 0.0};
      comm_sum(v, 3);
      if (v[2] > 0) {
        if (!rc) { err = "lm_begin failed on " + std::to_string((int)(v[2] + 0.5)) + " peer rank(s)"; rc = SBA_ERR_STATE; }
        return rc;
      }
      c0 = v[0];
      N_global = (long long)(v[1] + 0.5);
    }
    initial_cost = c0;
    LMState s{};
    s.lam = opts.lambda0 > 0 ? opts.lambda0 : 1e-4;
    // x_scale = 1 (unscaled damping): lambda = tau * max diag(J^T J), set on the device.  tau is tiny because the
    // parameters of these variants differ by orders of magnitude in scale (rotation vs focal length; affine matrix vs
    // translation column), and only a near Gauss-Newton step moves the weakly scaled ones -- scipy gets the same
    // effect from its large initial trust radius
    if (sq_mode()) s.lam = -(opts.lambda0 > 0 ? opts.lambda0 : 1e-9);
    s.nu = 2.0;
    s.cost = c0;
    s.ftol = opts.ftol; s.xtol = opts.xtol; s.gtol = opts.gtol;
    s.lam_min = 1e-12; s.lam_max = 1e12;
    s.nfev = 1; s.njev = 1;
    const long long nparam = opts.mode == SBA_MODE_CAMS_ONLY_SQ ? (long long)n : opts.mode == SBA_MODE_TRANSFORM_SQ ? 12LL :
        (opts.mode == SBA_MODE_FULL ? (long long)n : opts.mode == SBA_MODE_SHARED_INTR ? (long long)n_tied : 0) + 3LL * N_global;
    s.max_nfev = opts.max_nfev > 0 ? opts.max_nfev : 100 * nparam;
    s.status = -1; s.fresh = 1; s.need_lin = 1;
    s.always_relin = opts.always_relinearize ? 1 : 0;
    s.max_iter = opts.max_iter > 0 ? opts.max_iter : 0;
    s.cur = 0;
    s.free_cams = (opts.mode == SBA_MODE_POINTS_ONLY) ? 0 : 1;
    *h_state = s;
    HIPCHK(hipMemcpyAsync(d_state.p, h_state, sizeof(LMState), hipMemcpyHostToDevice, stream));
    // column scalings and camera step cleared, trial camera buffers = copies of the current ones (points-only mode needs valid ones)
    hipLaunchKernelGGL(k_lm_reset<T>, dim3(256), dim3(256), 0, stream, D2p.p, D2p.n, D2c.p, delta_c.p, n, cams[cur].p, cams[1 - cur].p,
                       campre[cur].p, campre[1 - cur].p, C * CAMPRE);
    push_ptrs();
    cur_at_begin = cur;
    if (d_log.n == 0) d_log.alloc(LOG_CAP);
    if (sq_mode()) {
      // points never move in these variants, but the buffer parity flips with every accepted step: both sides equal
      HIPCHK(hipMemcpyAsync(pts[1 - cur].p, pts[cur].p, sizeof(double) * (size_t)N * 3, hipMemcpyDeviceToDevice, stream));
      HIPCHK(hipMemcpyAsync(ptsT[1 - cur].p, ptsT[cur].p, sizeof(T) * (size_t)N * 3, hipMemcpyDeviceToDevice, stream));
      sq_setup();
      if (opts.mode == SBA_MODE_TRANSFORM_SQ) {
        const double ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};     // x0 of pySBA.py:193
        for (int b = 0; b < 2; ++b) HIPCHK(hipMemcpyAsync(theta[b].p, ident, sizeof ident, hipMemcpyHostToDevice, stream));
      }
      launch_sq_linearize(nullptr);
      double g0 = 0;
      sq_read(c0, g0);
      initial_cost = c0;
      h_state->cost = c0;
      HIPCHK(hipMemcpyAsync(d_state.p, h_state, sizeof(LMState), hipMemcpyHostToDevice, stream));
      sync();                      // `ident` above is a stack array
    }
    // no host synchronisation here: everything above is ordered on the stream in front of the first iteration, and the pinned
    // state mirror it was copied from is next written by lm_poll's device-to-host copy on the same stream
    log.clear();
    log_read = 0;
    n_decides = 0;
    poll_clean = false;
    pending_decide = false;
    gmax_cur = gmax_part.p;
    lm_active = true;
    if (!std::isfinite(c0)) { err = "Residuals are not finite in the initial point."; return SBA_ERR_NONFINITE; }
    return SBA_OK;
  }

  int lm_linearize() override {
    if (!lm_active) { err = "sba_lm_begin has not been called"; return SBA_ERR_STATE; }
    poll_clean = false;
    if (!bf3_path()) flush_decide();
    if (sq_mode()) { launch_sq_linearize(d_state.p); return SBA_OK; }
    if (fused()) return SBA_OK;          // the fused Schur kernel linearises
    if (!lin_pts()) {                    // (f64 one-group rigs: k_schur_sym<LIN> linearises the points)
      prof_begin(KP_LINP);
      launch_linearize_points(d_state.p);
      prof_end(KP_LINP);
    }
    if (h_state->free_cams && !rt.pairs_fold_u) { prof_begin(KP_LINC); launch_linearize_cams(d_state.p); prof_end(KP_LINC); }
    return SBA_OK;
  }

  int lm_form_reduced(double* E) override { return form_reduced(E, nullptr); }
  int form_reduced(double* E, double* Pk, bool own_loop = false /* run_loop's single-rank iteration: E is E_own */) {
    if (!lm_active) { err = "sba_lm_begin has not been called"; return SBA_ERR_STATE; }
    poll_clean = false;
    chol.image_written(false);
    if (!bf3_path()) flush_decide();
    if (sq_mode()) {
      if (opts.mode == SBA_MODE_CAMS_ONLY_SQ)
        hipLaunchKernelGGL(k_sq_pack_cams, dim3(64), dim3(256), 0, stream, sq_16.p, C, d_state.p, E);
      return SBA_OK;
    }
    if (h_state->free_cams) {
      prof_begin(KP_SCHUR);
      launch_schur();
      prof_end(KP_SCHUR);
    }
    prof_begin(KP_REDUCE);
    {
      const int fc = (int)h_state->free_cams;
      const bool wide = fused() && rt.fused_wide;
      // (wide: one slab per workgroup with ntw (ntw + 1) / 2 tiles, passed as one "pair")
      // tile slots per pair the grid covers: one pair -> its own tile count (no workgroups that return at once)
      const int ntw = wide_ntw(C);
      const int nt_launch = wide ? ntw * (ntw + 1) / 2 : npairs == 1 ? GROUP_TILES * (GROUP_TILES + 1) / 2 : GROUP_TILES * GROUP_TILES;
      const int np_arg = wide ? 1 : npairs;
      const int nblocks = (fc ? 4 * nt_launch * np_arg + (n + 15) / 16 : 0) + 1;
      // slab tiles: 3 = the wide kernels' compact rows, 1 = parameter-major (the bf16 kernels), 0 = camera-major
      const int emajor_mode = wide ? 3 : ((fused() && sizeof(T) == 4) || pairs_bf3()) ? 1 : 0;
      // the f32 image for the factorisation: the library's own single-rank loop only, and not for a tied solve
      const CholPlan cp = plan_chol<T>(n, n, kn, card_shared);
      float* img = chol.image_for(cp, own_loop && !multi() && !Pk && E == E_own.p && fc && opts.mode != SBA_MODE_SHARED_INTR);
      hipLaunchKernelGGL(k_build_exchange<T>, dim3(nblocks), dim3(1024), 0, stream, slabs.p, bpart.p, rt.ksplit, pair_ga.p,
                         pair_gb.p, np_arg, U.p, gc.p, cost_part.p, n_lin_parts(), C, fc, E, d_state.p,
                         (fused() || rt.pairs_fold_u) ? gdpart.p : (const double*)nullptr, Pk, emajor_mode, nt_launch,
                         img, img ? cp.img_ld : 0);
      chol.image_written(img != nullptr);
    }
    prof_end(KP_REDUCE);
    return SBA_OK;
  }

  // scal == nullptr: single rank, the partials are folded inside k_decide and no scalar exchange is needed
  int lm_solve_trial(double* E, double* scal) override {
    if (!lm_active) { err = "sba_lm_begin has not been called"; return SBA_ERR_STATE; }
    poll_clean = false;
    if (opts.mode == SBA_MODE_TRANSFORM_SQ) {
      hipLaunchKernelGGL(k_sq_solve12, dim3(1), dim3(64), 0, stream, sq_16.p, d_state.p, tsets());
      launch_sq_trial();
      launch_sq_scalars(scal);
      return SBA_OK;
    }
    if (h_state->free_cams) {
      prof_begin(KP_CHOL);
      const bool tied = (opts.mode == SBA_MODE_SHARED_INTR);
      const int n_sys = tied ? n_tied : n;
      double* Esys = E;
      if (tied) {   // collapse the camera system onto the tied unknowns
        hipLaunchKernelGGL(k_tie_system, dim3(n_tied), dim3(256), 0, stream, E, n, n_tied, tie_pre_start.p, tie_pre_idx.p,
                           E_tied.p, d_state.p);
        Esys = E_tied.p;
      }
      chol.solve(plan_chol<T>(n_sys, n, kn, card_shared),
                 {stream, Esys, n_sys, C, d_state.p, D2c.p, ps_lm(), delta_c.p, tied ? tie_map.p : nullptr, tied ? tie_first.p : nullptr},
                 !tied && E == E_own.p);
      prof_end(KP_CHOL);
    } else {
      hipLaunchKernelGGL(k_nocam_step, dim3(1), dim3(64), 0, stream, d_state.p, E, n);
      if (N > 0)
        hipLaunchKernelGGL(k_point_factor<T>, dim3((N + 255) / 256), dim3(256), 0, stream, V.p, gp.p, D2p.p, d_state.p, N, pfac.p,
                         has_fixed ? pt_fixed_mask.p : (const unsigned char*)nullptr);
    }
    if (sq_mode()) { launch_sq_trial(); launch_sq_scalars(scal); return SBA_OK; }
    prof_begin(KP_BACKSUB);
    launch_backsub_trial();
    prof_end(KP_BACKSUB);
    if (scal)
      hipLaunchKernelGGL(k_trial_scalars, dim3(1), dim3(DECIDE_THREADS), 0, stream, trial_part.p, gmax_rd(), n_trial_parts(), n_lin_parts(), d_state.p, scal);
    return SBA_OK;
  }

  // enqueue the accept / reject / terminate kernel; nothing is read back
  int lm_decide_async(const double* scal_all, int n_ranks) override {
    if (!lm_active) { err = "sba_lm_begin has not been called"; return SBA_ERR_STATE; }
    poll_clean = false;
    ++n_decides;
    if (!kn.decide_kernel && bf3_path()) {
      // the next k_schur_fused_bf3 takes the decision in its prologue; whatever else needs the decided record first
      // (lm_poll, another linearisation path) enqueues the kernel below through flush_decide()
      pending_decide = true; pend_scal = scal_all; pend_ranks = n_ranks;
      return SBA_OK;
    }
    launch_decide(scal_all, n_ranks);
    return SBA_OK;
  }
  const double* gmax_rd() const { return (bf3_path() && gmax_cur) ? gmax_cur : gmax_part.p; }
  void launch_decide(const double* scal_all, int n_ranks) {
    hipLaunchKernelGGL(k_decide<T>, dim3(1), dim3(DECIDE_THREADS), 0, stream, d_state.p, scal_all, n_ranks, trial_part.p,
                       gmax_rd(), sq_mode() ? nblk_sq : n_trial_parts(), sq_mode() ? nblk_sq : n_lin_parts(), reinterpret_cast<LMLogRow*>(d_log.p), LOG_CAP);
  }
  void flush_decide() {
    if (!pending_decide) return;
    launch_decide(pend_scal, pend_ranks);
    pending_decide = false;
  }

  // read the state back (one sync); returns the scipy status or -1 while the solve is still running
  int lm_poll(int32_t* status_out, int32_t* iterations_out) override {
    if (!lm_active) { err = "sba_lm_begin has not been called"; return SBA_ERR_STATE; }
    flush_decide();
    HIPCHK(hipMemcpyAsync(h_state, d_state.p, sizeof(LMState), hipMemcpyDeviceToHost, stream));
    // the log rows written since the last poll travel with the state: at most one row per accept/reject kernel enqueued so far,
    // into the pinned landing area when they fit (the usual case: a batch of iterations), otherwise by a second copy below
    constexpr size_t ROW_DOUBLES = (sizeof(sba_lm_iter_log) + 7) / 8;
    const int maybe = std::min(n_decides, (int)LOG_CAP) - log_read;
    const bool rows_landed = maybe > 0 && (size_t)maybe * ROW_DOUBLES <= LAND_DOUBLES;
    if (rows_landed)
      HIPCHK(hipMemcpyAsync(h_land, d_log.p + log_read, sizeof(sba_lm_iter_log) * maybe, hipMemcpyDeviceToHost, stream));
    sync_spin();
    HIPCHK(hipGetLastError());
    prof_collect();
    const LMState& s = *h_state;
    if (s.comm_fail) { err = "a peer rank did not reach the exchange in time (sba_ipc; SBA_IPC_TIMEOUT_S, default 5 s): the sharded solve was stopped and the handle can take no further exchange"; lm_active = false; ipc_dead = true; return SBA_ERR_STATE; }
    cur = cur_at_begin ^ (s.cur & 1);
    const int have = std::min(s.iter, LOG_CAP);
    if (have > log_read) {
      log.resize(have);
      if (rows_landed && have - log_read <= maybe)
        std::memcpy(log.data() + log_read, h_land, sizeof(sba_lm_iter_log) * (have - log_read));
      else
        HIPCHK(hipMemcpy(log.data() + log_read, d_log.p + log_read, sizeof(sba_lm_iter_log) * (have - log_read), hipMemcpyDeviceToHost));
      log_read = have;
    }
    poll_clean = true;
    if (status_out) *status_out = s.status;
    if (iterations_out) *iterations_out = s.iter;
    return SBA_OK;
  }

  int lm_decide(const double* scal_all, int n_ranks, int32_t* status_out, int32_t* accepted_out, sba_lm_iter_log* row) override {
    int rc = lm_decide_async(scal_all, n_ranks);
    if (rc) return rc;
    int32_t st = -1, it = 0;
    rc = lm_poll(&st, &it);
    if (rc) return rc;
    if (row && !log.empty()) *row = log.back();
    if (status_out) *status_out = st;
    if (accepted_out) *accepted_out = h_state->accepted;
    return SBA_OK;
  }

  int lm_finish(double* cams_out, double* pts_out, sba_lm_report* rep) override {
    if (!lm_active) { err = "sba_lm_begin has not been called"; return SBA_ERR_STATE; }
    int32_t st = -1, it = 0;
    int rc = poll_clean ? SBA_OK : lm_poll(&st, &it);          // refreshes `cur` and the log (unless the caller just polled)
    if (rc) return rc;
    push_ptrs();                         // table consistent with `cur` for the unconditional launches below
    if (sq_mode()) {
      launch_sq_linearize(nullptr);
      double cost = 0, gmax = 0;
      sq_read(cost, gmax);
      if (opts.mode == SBA_MODE_TRANSFORM_SQ) {
        HIPCHK(hipMemcpyAsync(h_theta, theta[cur].p, sizeof h_theta, hipMemcpyDeviceToHost, stream));
        std::vector<double> X((size_t)N * 3);
        HIPCHK(hipMemcpyAsync(X.data(), pts[cur].p, sizeof(double) * X.size(), hipMemcpyDeviceToHost, stream));
        sync();
        if (pts_out)
          for (int p = 0; p < N; ++p)
            for (int k = 0; k < 3; ++k)
              pts_out[3 * (size_t)p + k] = h_theta[4 * k] * X[3 * (size_t)p] + h_theta[4 * k + 1] * X[3 * (size_t)p + 1] +
                                           h_theta[4 * k + 2] * X[3 * (size_t)p + 2] + h_theta[4 * k + 3];
      } else if (pts_out) {
        HIPCHK(hipMemcpyAsync(pts_out, pts[cur].p, sizeof(double) * (size_t)N * 3, hipMemcpyDeviceToHost, stream));
      }
      if (cams_out) HIPCHK(hipMemcpyAsync(cams_out, cams[cur].p, sizeof(double) * n, hipMemcpyDeviceToHost, stream));
      sync();
      if (rep) {
        const LMState& s = *h_state;
        rep->cost = cost; rep->initial_cost = initial_cost; rep->optimality = gmax; rep->step_norm = s.step_norm;
        rep->lambda = s.lam; rep->nfev = s.nfev; rep->njev = s.njev; rep->iterations = s.iter; rep->accepted = s.n_accepted;
        rep->status = s.status < 0 ? 0 : s.status;
        rep->reserved = s.chol_f64_retries;
      }
      lm_active = false;
      return SBA_OK;
    }
    // gradient norm at the returned point (scipy reports optimality there, trf.py:546-551)
    launch_linearize_points(nullptr);
    double gmax = 0;
    // the small results land in pinned memory: [gmax partials | cost partials | camera gradient | cameras]
    const int nlp = nblk ? n_linp_blocks() : 0;          // partials of the linearisation launched above
    const size_t need = 2 * (size_t)nlp + 2 * (size_t)n;
    std::vector<double> land_v(need > LAND_DOUBLES ? need : 0);
    double* land = land_v.empty() ? h_land : land_v.data();
    double *gm = land, *cp = land + nlp, *gch = land + 2 * (size_t)nlp, *cams_l = gch + n;
    if (nlp) {
      HIPCHK(hipMemcpyAsync(gm, gmax_part.p, sizeof(double) * nlp, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipMemcpyAsync(cp, cost_part.p, sizeof(double) * nlp, hipMemcpyDeviceToHost, stream));
    }
    if (h_state->free_cams) {
      launch_linearize_cams(nullptr);
      HIPCHK(hipMemcpyAsync(gch, gc.p, sizeof(double) * n, hipMemcpyDeviceToHost, stream));
    } else {
      gc.zero(stream);
      for (int i = 0; i < n; ++i) gch[i] = 0.0;
    }
    if (cams_out) HIPCHK(hipMemcpyAsync(cams_l, cams[cur].p, sizeof(double) * n, hipMemcpyDeviceToHost, stream));
    // the points (1.2 MB at 50k points, into the caller's pageable array: a staged copy that holds the calling thread) go through the
    // copy stream, beside the two gradient kernels enqueued above instead of behind them: the solve has been polled, nothing in
    // flight writes them any more
    if (pts_out) HIPCHK(hipMemcpyAsync(pts_out, pts[cur].p, sizeof(double) * (size_t)N * 3, hipMemcpyDeviceToHost, hres.copy_stream));
    sync_spin();
    if (pts_out) HIPCHK(hipStreamSynchronize(hres.copy_stream));
    HIPCHK(hipGetLastError());
    if (cams_out) std::memcpy(cams_out, cams_l, sizeof(double) * n);
    double cost = 0;
    for (int i = 0; i < nlp; ++i) { gmax = std::max(gmax, gm[i]); cost += cp[i]; }
    if (multi()) {       // whole-job figures: cost and camera gradient are sums over the ranks, the point-gradient maximum a max
      std::vector<double> v(n + 1);
      for (int i = 0; i < n; ++i) v[i] = gch[i];
      v[n] = cost;
      comm_sum(v.data(), n + 1);
      for (int i = 0; i < n; ++i) gch[i] = v[i];
      cost = v[n];
      comm_max(&gmax, 1);
    }
    if (opts.mode == SBA_MODE_SHARED_INTR && (int)h_tie.size() == n) {   // gradient in the tied unknowns
      std::vector<double> gs(n_tied, 0.0);
      for (int i = 0; i < n; ++i) gs[h_tie[i]] += gch[i];
      for (double v : gs) gmax = std::max(gmax, std::fabs(v));
    } else {
      for (int i = 0; i < n; ++i) gmax = std::max(gmax, std::fabs(gch[i]));
    }
    if (rep) {
      const LMState& s = *h_state;
      rep->cost = cost; rep->initial_cost = initial_cost; rep->optimality = gmax; rep->step_norm = s.step_norm;
      rep->lambda = s.lam; rep->nfev = s.nfev; rep->njev = s.njev; rep->iterations = s.iter; rep->accepted = s.n_accepted;
      rep->status = s.status < 0 ? 0 : s.status;
      rep->reserved = s.chol_f64_retries;
    }
    lm_active = false;
    return SBA_OK;
  }

  // the iteration loop of a solve between lm_begin and lm_finish: batches of iterations enqueued back to back, one poll per batch
  int run_loop(const sba_lm_opts* o, int32_t& status, int32_t& iters) {
    int rc = SBA_OK;
    while (status < 0) {
      // a batch of iterations is enqueued back to back; the kernels turn into no-ops once the device-side state says the
      // solve has terminated, and a rejected step skips its re-linearization on the device, not on the host
      // (profiling: one event pair per kernel class, read at every poll.  Two iterations per poll, so that the pairs time the
      //  SECOND one, whose fused kernel carries the previous step's decision in its prologue like every iteration of a normal batch)
      // With a communicator the number of iterations (= collectives) enqueued per poll must not depend on anything rank-local
      // (bf3_path() follows the shard's own visibility density): a rank that enqueues one more all-reduce than its peers after
      // the device-side termination waits for it forever.
      const int pbatch = multi() ? 2 : (bf3_path() && !kn.decide_kernel ? 2 : 1);
      int batch = prof_on ? pbatch : BATCH;
      if (o->max_iter > 0) batch = std::min(std::max(1, o->max_iter - iters), prof_on ? pbatch : 64);
      for (int b = 0; b < batch; ++b) {
        lm_linearize();
        if (!multi()) {
          form_reduced(E_own.p, nullptr, true);
          lm_solve_trial(E_own.p, nullptr);
          lm_decide_async(nullptr, 1);
        } else if (ipc_on) {
          // the same two exchange points through the peer-mapped areas (sba_ipc.hpp): every rank writes its packed system /
          // its 8 trial scalars into its own area, raises a flag, waits (one wave, bounded) for the peers' flags and adds the
          // n_ranks copies in rank order -- no RCCL launch on the iteration's critical path
          const bool fc = h_state->free_cams != 0;
          const unsigned long long s0 = ++ipc_seq[0];
          const size_t sys_off = ipc_L.sys_slot(n, (int)(s0 & 1));
          form_reduced(E_own.p, ipc_mine + sys_off);
          ipc_publish(0, s0, d_state.p);
          ipc_gate(0, s0, d_state.p, 0, 0, nullptr);
          hipLaunchKernelGGL(k_ipc_sum_system, dim3(fc ? std::min(1024, (n * n + 255) / 256) : 1), dim3(256), 0, stream, ipc_ptrs.p, comm_n,
                             sys_off, n, (int)fc, E_own.p, d_state.p);
          const unsigned long long s1 = ++ipc_seq[1];
          const size_t sc_off = ipc_L.scal_slot((int)(s1 & 1));
          lm_solve_trial(E_own.p, ipc_mine + sc_off);
          ipc_publish(1, s1, d_state.p);
          ipc_gate(1, s1, d_state.p, sc_off, NSCAL, sc_all.p);
          lm_decide_async(sc_all.p, comm_n);
        } else {
          // one all-reduce of the packed reduced camera system, one all-gather of 8 scalars per rank; every rank then solves
          // the same system and takes the same decision.  A finished solve turns the kernels into no-ops on the device; the
          // collectives of such a tail still match because every rank enqueues the same number of them.
          if (xpack.n < exch_packed_size(n)) xpack.alloc(exch_packed_size(n));
          form_reduced(E_own.p, xpack.p);
          const bool fc = h_state->free_cams != 0;
          double* xb = fc ? xpack.p : xpack.p + exch_packed_size(n) - 1;       // points-only mode: the cost is all there is
          RCCLCHK(Rccl::get().all_reduce(xb, xb, fc ? exch_packed_size(n) : 1, Rccl::kFloat64, Rccl::kSum, comm, stream));
          hipLaunchKernelGGL(k_unpack_exchange, dim3(fc ? std::min(1024, (n * n + 255) / 256) : 1), dim3(256), 0, stream, xpack.p, n,
                             (int)fc, E_own.p, d_state.p);
          lm_solve_trial(E_own.p, sc_loc.p);
          RCCLCHK(Rccl::get().all_gather(sc_loc.p, sc_all.p, NSCAL, Rccl::kFloat64, comm, stream));
          lm_decide_async(sc_all.p, comm_n);
        }
      }
      rc = lm_poll(&status, &iters);
      if (rc) return rc;
    }
    return SBA_OK;
  }

  // sba_lm_run: the loop alone on a solve begun with sba_lm_begin (bench.py times exactly the iterations with it)
  int lm_run(int32_t* status_out, int32_t* iterations_out) override {
    if (!lm_active) { err = "sba_lm_begin has not been called"; return SBA_ERR_STATE; }
    int32_t status = -1, iters = 0;
    const int rc = run_loop(&opts, status, iters);
    if (rc) return rc;
    if (status_out) *status_out = status;
    if (iterations_out) *iterations_out = iters;
    return SBA_OK;
  }

  int solve(const sba_lm_opts* o, double* cams_out, double* pts_out, sba_lm_report* rep, sba_lm_iter_log* lg, int cap,
            int32_t* rows) override {
    const auto t0 = std::chrono::steady_clock::now();
    auto since = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e6; };
    int rc = lm_begin(o);
    if (rc) return rc;
    const double t_begin = since();
    HIPCHK(hipEventRecord(ev0, stream));
    int32_t status = -1, iters = 0;
    rc = run_loop(o, status, iters);
    if (rc) return rc;
    const double t_loop = since();
    HIPCHK(hipEventRecord(ev1, stream));
    HIPCHK(hipEventSynchronize(ev1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ev0, ev1));
    rc = lm_finish(cams_out, pts_out, rep);
    if (rc) return rc;
    if (kn.solve_debug)
      fprintf(stderr, "[solve] lm_begin %.0f us | loop (enqueue + polls) %.0f us (device %.0f us) | lm_finish %.0f us | %d iterations\n",
              t_begin, t_loop - t_begin, ms * 1e3, since() - t_loop, (int)iters);
    if (rep) {
      rep->status = status;
      rep->seconds_device = ms * 1e-3;
      rep->seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    const int nrow = std::min<int>(cap, (int)log.size());
    if (lg) for (int i = 0; i < nrow; ++i) lg[i] = log[i];
    if (rows) *rows = (int32_t)log.size();
    return SBA_OK;
  }

  // ------------------------------------------------------------------ measurement hook
  int time_kernel(const char* name, int reps, double* mean_us) override {
    if (!uploaded) { err = "sba_upload has not been called"; return SBA_ERR_STATE; }
    HIPCHK(hipSetDevice(device));
    const std::string k(name);
    if (reps < 1) reps = 1;
    // make sure everything the kernel reads exists
    if (k == "resjac" && Jc_pm.n != (size_t)M * 2 * NCP) { r_pm.alloc(M); Jc_pm.alloc((size_t)M * 2 * NCP); Jp_pm.alloc((size_t)M * 6); }
    if (k == "schur" || k == "backsub") {
      sba_lm_opts o{}; o.ftol = o.xtol = o.gtol = 0; o.mode = SBA_MODE_FULL;
      if (!lm_active) { int rc = lm_begin(&o); if (rc) return rc; }
      lm_linearize(); lm_form_reduced(E_own.p); lm_solve_trial(E_own.p, scal_own.p);
    } else {
      push_ptrs();
    }
    auto once = [&]() {
      if (k == "residual") launch_residual(nullptr);
      else if (k == "resjac") launch_resjac(r_pm.p);
      else if (k == "linearize_points") launch_linearize_points(nullptr);
      else if (k == "linearize_cams") launch_linearize_cams(nullptr);
      else if (k == "schur") launch_schur();
      else if (k == "backsub") launch_backsub_trial();
      else return false;
      return true;
    };
    if (!once()) { err = "unknown kernel name"; return SBA_ERR_INVALID; }
    sync();
    HIPCHK(hipEventRecord(ev0, stream));
    for (int i = 0; i < reps; ++i) once();
    HIPCHK(hipEventRecord(ev1, stream));
    HIPCHK(hipEventSynchronize(ev1));
    HIPCHK(hipGetLastError());
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ev0, ev1));
    *mean_us = (double)ms * 1e3 / reps;
    return SBA_OK;
  }

  // ------------------------------------------------------------------ opt-in extensions
  int set_fixed_points(const uint8_t* mask) override {
    if (!uploaded) { err = "sba_upload has not been called"; return SBA_ERR_STATE; }
    has_fixed = false;
    if (mask) {
      std::vector<unsigned char> m(mask, mask + N);
      for (auto& v : m) { v = v ? 1 : 0; has_fixed = has_fixed || v; }
      if (has_fixed) { pt_fixed_mask.upload(m, stream); sync(); }
    }
    push_ptrs();
    return SBA_OK;
  }
  int set_robust_loss(int loss, double f_scale) override {
    static_assert(SBA_LOSS_HUBER == LOSS_HUBER && SBA_LOSS_SOFT_L1 == LOSS_SOFT_L1 && SBA_LOSS_CAUCHY == LOSS_CAUCHY, "sba_loss values");
    if (loss < SBA_LOSS_LINEAR || loss > SBA_LOSS_CAUCHY) { err = "unknown loss"; return SBA_ERR_INVALID; }
    if (loss != SBA_LOSS_LINEAR && !(f_scale > 0 && std::isfinite(f_scale))) { err = "f_scale must be positive"; return SBA_ERR_INVALID; }
    loss_delta = loss != SBA_LOSS_LINEAR ? f_scale : 0.0;
    loss_kind = loss;
    push_ptrs();
    return SBA_OK;
  }

  // ------------------------------------------------------------------ calls beside the LM loop, on the current parameters
  // uploaded, single-rank and (refuse_lm_active) not between sba_lm_begin and sba_lm_finish; then the device is set and the stream idle
  int aux_ready(const char* who, bool refuse_lm_active, const char* multi_note = "") {
    if (!uploaded) { err = "sba_upload has not been called"; return SBA_ERR_STATE; }
    if (multi()) { err = std::string(who) + ": a handle of a multi-rank job is not supported" + multi_note; return SBA_ERR_UNSUPPORTED; }
    if (refuse_lm_active && lm_active) { err = std::string(who) + ": the handle is between sba_lm_begin and sba_lm_finish"; return SBA_ERR_STATE; }
    HIPCHK(hipSetDevice(device));
    sync();
    return SBA_OK;
  }
  TriIn<T> tri_in() {          // what sba_triangulate.hpp and sba_unproject.hpp work on
    return {stream, C, N, M, cams[cur].p, pts[cur].p, ptsT[cur].p, uv_pm.p, has_w ? w_pm.p : nullptr, ci_pm.p, pt_start.p,
            blk_desc.p, nblk, has_fixed ? pt_fixed_mask.p : nullptr, identity_perm ? nullptr : perm.data()};
  }

  // ------------------------------------------------------------------ parameter covariance (sba_covariance.hpp)
  int covariance(const sba_cov_opts* o, double* cam_full, double* cam_blocks, double* pt_cov, sba_cov_report* rep) override {
    if (int rc = aux_ready("sba_covariance", false, " (sharded covariance)")) return rc;
    CovIn<T> in{stream, C, N, M, cams[cur].p, pts[cur].p, uv_pm.p, has_w ? w_pm.p : nullptr, ci_pm.p, pt_start.p,
                has_fixed ? pt_fixed_mask.p : nullptr, RLoss<double>{loss_delta, loss_kind}};
    return cov_run<T>(in, *o, cam_full, cam_blocks, pt_cov, rep, err);
  }

  // ------------------------------------------------------------------ triangulation (sba_triangulate.hpp)
  int triangulate(const sba_tri_opts* o, double* points_out, int32_t* status_out, int32_t* n_views_out, double* rms_out,
                  double* max_out, double* spread_out, uint8_t* inlier_out, sba_tri_report* rep) override {
    if (int rc = aux_ready("sba_triangulate", false)) return rc;
    return tri_run<T>(tri_in(), *o, points_out, status_out, n_views_out, rms_out, max_out, spread_out, inlier_out, rep, err);
  }

  // ------------------------------------------------------------------ similarity registration (sba_align.hpp)
  int align(const sba_align_opts* o, const double* target_points, const double* point_weights, const double* target_centres,
            const double* centre_weights, sba_align_report* rep) override {
    if (int rc = aux_ready("sba_align", true)) return rc;
    AlignIn<T> in{stream, C, N, cams[cur].p, pts[cur].p, ptsT[cur].p, campre[cur].p};
    return align_run<T>(in, *o, target_points, point_weights, target_centres, centre_weights, rep, err);
  }
  int apply_similarity(double scale, const double* R, const double* t) override {
    if (int rc = aux_ready("sba_apply_similarity", true)) return rc;
    AlignIn<T> in{stream, C, N, cams[cur].p, pts[cur].p, ptsT[cur].p, campre[cur].p};
    return align_apply_run<T>(in, scale, R, t, err);
  }

  // ------------------------------------------------------------------ points on known planes (sba_unproject.hpp)
  int unproject(const sba_unp_opts* o, const double* planes, int64_t n_planes, double* points_out, int32_t* status_out,
                int32_t* n_views_out, double* rms_out, double* max_out, uint8_t* used_out, sba_unp_report* rep) override {
    if (int rc = aux_ready("sba_unproject", true)) return rc;
    return unp_run<T>(tri_in(), *o, planes, n_planes, points_out, status_out, n_views_out, rms_out, max_out, used_out, rep, err);
  }

  // ------------------------------------------------------------------ reprojection diagnostics (sba_reproj.hpp)
  int reproj_stats(const sba_reproj_opts* o, double* cam_stats, int64_t* cam_hist, double* cam_grid, double* cam_radial,
                   double* pt_stats, double* err_out, int64_t* worst_idx, double* worst_err, sba_reproj_report* rep) override {
    if (int rc = aux_ready("sba_reproj_stats", true)) return rc;
    RpIn<T> in{stream, C, N, M, cams[cur].p, pts[cur].p, uv_cm.p, uv_pm.p, has_w ? w_cm.p : nullptr, has_w ? w_pm.p : nullptr,
               pi_cm.p, ci_pm.p, pi_pm.p, pt_start.p, chunk_cam.p, chunk_begin.p, chunk_end.p, cam_chunk_start.p, nchunk,
               identity_perm ? nullptr : perm.data()};
    return rp_run<T>(in, *o, cam_stats, cam_hist, cam_grid, cam_radial, pt_stats, err_out, worst_idx, worst_err, rep, err);
  }

  // ------------------------------------------------------------------ small accessors of the C ABI
  int set_params_x(const double* x) override {
    if (!uploaded) { err = "not uploaded"; return SBA_ERR_STATE; }
    set_params(x, x + (size_t)C * NCP);
    return SBA_OK;
  }
  int get_params(double* cams_out, double* points_out) override {
    if (!uploaded) { err = "not uploaded"; return SBA_ERR_STATE; }
    if (cams_out) HIPCHK(hipMemcpyAsync(cams_out, cams[cur].p, sizeof(double) * n, hipMemcpyDeviceToHost, stream));
    if (points_out) HIPCHK(hipMemcpyAsync(points_out, pts[cur].p, sizeof(double) * (size_t)N * 3, hipMemcpyDeviceToHost, stream));
    sync();
    return SBA_OK;
  }
  int get_gradient(double* gc_out, double* gp_out) override {
    if (!uploaded) { err = "not uploaded"; return SBA_ERR_STATE; }
    if (gc_out) HIPCHK(hipMemcpyAsync(gc_out, gc.p, sizeof(double) * n, hipMemcpyDeviceToHost, stream));
    if (gp_out) HIPCHK(hipMemcpyAsync(gp_out, gp.p, sizeof(double) * (size_t)N * 3, hipMemcpyDeviceToHost, stream));
    sync();
    return SBA_OK;
  }
  int get_step(double* delta_c_out) override {
    if (!uploaded) { err = "not uploaded"; return SBA_ERR_STATE; }
    HIPCHK(hipMemcpyAsync(delta_c_out, delta_c.p, sizeof(double) * n, hipMemcpyDeviceToHost, stream));
    sync();
    return SBA_OK;
  }
  int get_transform(double* theta12) override { for (int i = 0; i < 12; ++i) theta12[i] = h_theta[i]; return SBA_OK; }
  int get_log(sba_lm_iter_log* lg, int32_t cap, int32_t* rows) override {
    const int nrow = std::min<int>(cap, (int)log.size());
    if (lg) for (int i = 0; i < nrow; ++i) lg[i] = log[i];
    *rows = (int32_t)log.size();
    return SBA_OK;
  }
  int get_kernel_profile(double* total_us, int64_t* count) override {
    for (int k = 0; k < SBA_PROFILE_SLOTS; ++k) { total_us[k] = prof_us[k]; count[k] = prof_cnt[k]; }
    return SBA_OK;
  }
};

// stateless gathered-row calls (sba_rotate / sba_project)
template <typename T>
int rows_call(bool project, int device, int64_t nrows, const double* pts, const double* other, double* out) {
  HIPCHK(hipSetDevice(device));
  if (nrows == 0) return SBA_OK;
  const int64_t ow = project ? NCP : 3, rw = project ? 2 : 3;
  DevBuf<double> d_pts, d_o, d_out;
  d_pts.alloc(nrows * 3); d_o.alloc(nrows * ow); d_out.alloc(nrows * rw);
  HIPCHK(hipMemcpy(d_pts.p, pts, sizeof(double) * nrows * 3, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_o.p, other, sizeof(double) * nrows * ow, hipMemcpyHostToDevice));
  const int g = (int)((nrows + 255) / 256);
  if (project) hipLaunchKernelGGL(k_project_rows<T>, dim3(g), dim3(256), 0, 0, d_pts.p, d_o.p, d_out.p, nrows);
  else hipLaunchKernelGGL(k_rotate_rows<T>, dim3(g), dim3(256), 0, 0, d_pts.p, d_o.p, d_out.p, nrows);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, d_out.p, sizeof(double) * nrows * rw, hipMemcpyDeviceToHost));
  return SBA_OK;
}



inline EngineBase* make_engine(int dtype) {
  if (dtype == SBA_F32) return new Engine<float>();
  return new Engine<double>();
}
inline int rows_call_dtype(int dtype, bool project, int device, int64_t n, const double* pts, const double* other, double* out) {
  return dtype == SBA_F32 ? rows_call<float>(project, device, n, pts, other, out) : rows_call<double>(project, device, n, pts, other, out);
}

}  // namespace SBA_NS
