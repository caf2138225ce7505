// sba_chol_solve.hpp -- the host side of the reduced camera solve: which factorisation a system takes (plan_chol), the buffers
// and the launch bookkeeping of all of them (CholSolver).  The kernels are in sba_chol_blocked.hpp, sba_chol_ll.hpp and
// sba_chol_big.hpp; the engine (sba_engine.hpp) hands a CholSolver the system and keeps k_tie_system and the profiling brackets.
#pragma once
#include "sba_knobs.hpp"
#include "sba_chol_blocked.hpp"
#include "sba_chol_ll.hpp"
#include "sba_chol_big.hpp"

namespace SBA_NS {
using namespace sba_host;

// ============================================================================================== plan
// The factorisation of the reduced camera system (n_sys unknowns: C * NCP, or the tied ones of SBA_MODE_SHARED_INTR)
enum class CholRoute {
  LL,              // k_cholesky_ll: left-looking, factor on chip, up to 256 unknowns (sba_chol_ll.hpp)
  LL_F32,          // ... behind k_cholesky_blocked on f32 lanes: k_cholesky_ll only runs when that one refused the system
  BLOCKED,         // k_cholesky_blocked: right-looking, all in LDS, up to 176 unknowns (fp32 engine: on f32 lanes, f64 on a refusal)
  STREAM,          // k_cholesky_stream: one workgroup, finished block columns streamed through L2, up to chol_big_min_n
  BIG_DAG,         // k_chol_big_dag<double>: one launch, walker + tiles (sba_chol_big.hpp), then k_chol_big_back_all
  BIG_DAG_F32,     // ... k_chol_big_dag<float>, the f64 instance behind it for the systems it refuses
  BIG_LAUNCHES,    // k_chol_big_prepare + one k_chol_big_step per block column, then k_chol_big_back_all
};

template <typename T>
CholRoute chol_route(int n_sys, int ncam /* C * NCP */, const Knobs& k, bool card_shared) {
  if (k.chol_ll && (n_sys > CHOL_LDS_MAX_N || k.chol_ll_all) && n_sys <= CLL_MAX_NB * CB && ncam <= CLL_THREADS) {
    // fp32 engine (round 4): the right-looking all-in-LDS kernel on f32 lanes in front of it
    const bool f32 = sizeof(T) == 4 && k.chol_f32 && !k.chol_ll_all && n_sys > CHOL_LDS_MAX_N && ncam <= CHOLB_LDS_THREADS;
    return f32 ? CholRoute::LL_F32 : CholRoute::LL;
  }
  // (up to 176 unknowns C * NCP <= CHOLB_LDS_THREADS holds: a tied system has 3 + 8 C or 3 + 10 C unknowns)
  if (n_sys <= CHOL_LDS_MAX_N) return CholRoute::BLOCKED;
  if (n_sys <= k.chol_big_min_n) return CholRoute::STREAM;             // (chol_big_min_n <= CS_MAX_NB * CB)
  // ranks that share a card: k_chol_big_dag's progress argument (in-order dispatch of ONE launch) does not cover several such
  // launches holding each other's CUs
  if (!k.chol_big_dag || card_shared) return CholRoute::BIG_LAUNCHES;
  return sizeof(T) == 4 && k.chol_f32 ? CholRoute::BIG_DAG_F32 : CholRoute::BIG_DAG;
}

// Dynamic LDS of the kernels, each formula once: the plan takes a launch's bytes from here and CholSolver::set_attrs the largest
// a kernel may ask for.
constexpr size_t CU_LDS_BYTES = 160 * 1024;
// k_cholesky_blocked: the lower block triangle of nb block rows (16 rows of ld elements per block) + two vectors
constexpr size_t cholb_tri(int nb, int ld) { return (size_t)(nb * (nb + 1) / 2) * CB * ld; }
constexpr size_t cholb_lds(int nb, int ld, size_t elem) { return (cholb_tri(nb, ld) + 2 * (size_t)nb * CB) * elem; }
// ... its f32 triangle of up to 16 block rows fits the LDS on 20-float rows (conflict-free, CholNum<float>) up to 14 block rows,
// on 17-float rows at 15 and 16
constexpr int CHOLB_LD20_MAX_NB = 14;
constexpr int cholb_ld32(int nb) { return nb <= CHOLB_LD20_MAX_NB ? 20 : 17; }
// k_cholesky_stream: panel (nb blocks) + rhs + as much staging as the budget leaves (fewer, larger streaming rounds)
constexpr size_t CHOL_STREAM_LDS_BUDGET = 150 * 1024;
constexpr size_t chol_stream_fixed(int nb) { return ((size_t)nb * CBS + (size_t)nb * CB) * sizeof(double); }
constexpr int chol_stream_cap(int nb) { return std::min(64, std::max(nb, (int)((CHOL_STREAM_LDS_BUDGET - chol_stream_fixed(nb)) / (CBS * sizeof(double))))); }
constexpr size_t chol_stream_lds(int nb) { return chol_stream_fixed(nb) + (size_t)chol_stream_cap(nb) * CBS * sizeof(double); }
// k_chol_big_step / k_chol_big_dag<S>
template <typename S> constexpr size_t cholbig_lds() { return (size_t)CHOLBIG_LDS_BLOCKS * CholLay<S>::BS * sizeof(S); }

// The kernels' static LDS comes on top of the dynamic: k_cholesky_blocked's tables, damping, right-hand side (CholbShared), its
// reduction scratch and the trial cameras; a few hundred bytes in the others (k_cholesky_ll: sba_chol_ll.hpp).
template <int MAXNB> constexpr size_t CHOLB_STATIC_LDS = sizeof(CholbShared<MAXNB>) + (4 * (CHOLB_LDS_THREADS / 64) + CHOLB_LDS_THREADS) * sizeof(double);
static_assert(cholb_lds(CHOLB_MAX_NB, CLD, sizeof(double)) + CHOLB_STATIC_LDS<CHOLB_MAX_NB> <= CU_LDS_BYTES &&
              cholb_lds(CHOLB_LD20_MAX_NB, 20, sizeof(float)) + CHOLB_STATIC_LDS<16> <= CU_LDS_BYTES &&
              cholb_lds(16, 17, sizeof(float)) + CHOLB_STATIC_LDS<16> <= CU_LDS_BYTES, "k_cholesky_blocked: dynamic + static LDS must fit a CU");
static_assert(chol_stream_lds(CS_MAX_NB) <= CHOL_STREAM_LDS_BUDGET && CHOL_STREAM_LDS_BUDGET + 8 * 1024 <= CU_LDS_BYTES, "k_cholesky_stream LDS");
static_assert(cholbig_lds<double>() + 4 * 1024 <= CU_LDS_BYTES && cholbig_lds<float>() <= cholbig_lds<double>(), "k_chol_big_step / _dag LDS");

// Everything a solve of an n_sys system launches with.  The same plan tells form_reduced which f32 image to have written and the
// solve which kernel instance reads it: one statement of the row stride for the writer and the reader.
struct CholPlan {
  CholRoute route = CholRoute::BLOCKED;
  int nb = 0;              // block rows of 16
  int ld32 = 0;            // k_cholesky_blocked factors on f32 lanes first, on rows of this many floats (17 or 20); 0 = it does not
  int img_ld = 0;          // row stride of the f32 image of the system the route can start from (= ld32), 0 = it takes none:
                           // an image is only ever written of the untied system (n_sys == C * NCP)
  size_t lds = 0;          // dynamic LDS of the route's f64-capable kernel (k_cholesky_ll / _blocked / _stream, k_chol_big_step / _dag<double>)
  size_t lds_f32 = 0;      // ... of the f32 kernel in front of it (LL_F32: k_cholesky_blocked<T, 16, ld32>, BIG_DAG_F32: k_chol_big_dag<float>)
  int stream_cap = 0;      // STREAM: staging blocks of a streaming round
  float f32_tau = 0.f;     // pivot threshold of the f32 factorisations (Knobs::chol_f32_tau)
};

// No HIP call, no allocation, no environment: the system's size and the switches in, the launch parameters out
template <typename T>
CholPlan plan_chol(int n_sys, int ncam /* C * NCP */, const Knobs& k, bool card_shared) {
  CholPlan p;
  p.route = chol_route<T>(n_sys, ncam, k, card_shared);
  p.nb = (n_sys + CB - 1) / CB;
  p.f32_tau = k.chol_f32_tau;
  switch (p.route) {
    case CholRoute::LL_F32: p.ld32 = cholb_ld32(p.nb); p.lds_f32 = cholb_lds(p.nb, p.ld32, sizeof(float)); [[fallthrough]];
    case CholRoute::LL: p.lds = CLL_LDS_BYTES; break;
    // (the f32 attempt shares the f64 triangle's LDS)
    case CholRoute::BLOCKED: p.ld32 = (sizeof(T) == 4 && k.chol_f32) ? 20 : 0; p.lds = cholb_lds(p.nb, CLD, sizeof(double)); break;
    case CholRoute::STREAM: p.stream_cap = chol_stream_cap(p.nb); p.lds = chol_stream_lds(p.nb); break;
    case CholRoute::BIG_DAG_F32: p.lds_f32 = cholbig_lds<float>(); [[fallthrough]];
    default: p.lds = cholbig_lds<double>(); break;
  }
  p.img_ld = n_sys == ncam ? p.ld32 : 0;
  return p;
}

// ============================================================================================== SBA_CHOL_DEBUG
inline void print_ll_stamps(const std::vector<long long>& st, int nb) {
  if (nb > 6) {
    const long long x0 = st[2 + 2 * 3], y0 = st[3 + 2 * 3];      // start of X_3 / Y_3 (thread 0)
    fprintf(stderr, "[chol_ll step 3, cycles after the step's barrier, per wave] X done:");
    for (int w = 0; w < 8; ++w) fprintf(stderr, " %lld", st[64 + w] - x0);
    fprintf(stderr, " | Y done:");
    for (int w = 0; w < 8; ++w) fprintf(stderr, " %lld", st[72 + w] - y0);
    fprintf(stderr, "\n[chol_ll back substitution, block row 5] x done (per wave, from wave 0's):");
    for (int w = 0; w < 8; ++w) fprintf(stderr, " %lld", st[80 + w] - st[80]);
    fprintf(stderr, " | barrier passed %lld | update done:", st[96] - st[80]);
    for (int w = 0; w < 8; ++w) fprintf(stderr, " %lld", st[88 + w] - st[96]);
    fprintf(stderr, " | barrier passed %lld\n", st[97] - st[96]);
  }
  fprintf(stderr, "[chol_ll stamps, cycles] setup %lld  chol0 %lld |", st[1] - st[0], st[2] - st[1]);
  for (int j = 0; j < nb; ++j) fprintf(stderr, " X%d %lld Y%d %lld |", j, st[3 + 2 * j] - st[2 + 2 * j], j, st[4 + 2 * j] - st[3 + 2 * j]);
  fprintf(stderr, " backsub %lld  epilogue %lld  total %lld\n", st[3 + 2 * nb] - st[2 + 2 * nb], st[4 + 2 * nb] - st[3 + 2 * nb], st[4 + 2 * nb] - st[0]);
}

inline void print_blocked_stamps(const std::vector<long long>& st, int nb) {
  fprintf(stderr, "[chol stamps, cycles] load %lld  chol0 %lld |", st[1] - st[0], st[2] - st[1]);
  for (int j = 0; j < nb; ++j) fprintf(stderr, " B%d %lld C%d %lld |", j, st[3 + 2 * j] - st[2 + 2 * j], j, st[4 + 2 * j] - st[3 + 2 * j]);
  fprintf(stderr, " backsub %lld  epilogue %lld  total %lld\n", st[3 + 2 * nb] - st[2 + 2 * nb], st[4 + 2 * nb] - st[3 + 2 * nb], st[4 + 2 * nb] - st[0]);
  fprintf(stderr, "[chol C0, cycles after B0's barrier, per wave]");
  for (int w = 0; w < CHOLB_LDS_THREADS / 64; ++w) fprintf(stderr, " %lld", st[40 + w] - st[3]);
  fprintf(stderr, "\n");
}

inline void print_stream_stamps(const std::vector<long long>& st) {
  fprintf(stderr, "[chol_stream cycles] update %lld  factor %lld  solve %lld  write-back %lld  back-substitution %lld\n", st[0], st[1], st[2], st[3], st[4]);
}

inline void print_dag_stamps(const std::vector<long long>& sv, int nbr, bool f32) {
  fprintf(stderr, "[chol_dag%s, the walker, x10 ns: wait for W(c,c-1), W(c,c) | load | panel | downdate | factor+inverse | image stored | flag]\n", f32 ? " on f32 lanes" : "");
  for (int cc = 0; cc < nbr; ++cc) {
    const long long* v = sv.data() + 8 * cc;
    fprintf(stderr, "  c=%2d at %6lld:", cc, v[4] - sv[0]);
    if (cc > 0) fprintf(stderr, " wait %4lld | load %4lld | panel %4lld | downdate %4lld |", v[1] - sv[8 * (cc - 1) + 7], v[2] - v[1], v[3] - v[2], v[4] - v[3]);
    fprintf(stderr, " factor %4lld | image %4lld | flag %4lld | column %5lld\n", v[5] - v[4], v[6] - v[5], v[7] - v[6], cc > 0 ? v[7] - sv[8 * (cc - 1) + 7] : v[7] - v[0]);
  }
}

// ============================================================================================== solver
// A = S + lam D (n_sys x n_sys, in Esys) -> delta_c = A^-1 rhs and the LM epilogue, by the route of the plan
template <typename T>
struct CholSolver {
  DevBuf<double> sol, work, W, Minv, Ld, yv;
  DevBuf<int> info;
  unsigned epoch = 0;                   // k_chol_big_back_all: launches so far (its parity picks the copy of x the launch works in)
  int yv_ext[2] = {0, 0};               // ... entries at the front of each copy of x that a launch may have left non-empty (solve_big)
  DevBuf<unsigned> dag_flags;           // k_chol_big_dag: Mimg_j / W(r,c) published (value = the launch's epoch)
  unsigned dag_epoch = 0;
  DevBuf<double> Mimg;                  // k_chol_big_dag: the factored diagonal blocks and their inverses, as they lie in LDS
  // fp32 engine: f32 image of the reduced system in k_cholesky_blocked's LDS layout, written by k_build_exchange beside E_own in the
  // library's own single-rank loop (row stride: CholPlan::img_ld).  img_ok: the image is the system in E_own -- form_reduced raises it
  // when it passes the image and lowers it on every other call, which covers all other writers of E_own (the phase API, the
  // multi-rank exchanges); a tied solve (k_tie_system) never uses it.
  DevBuf<float> img;
  bool img_ok = false;
  // SBA_CHOL_DEBUG: armed from the switch at sba_create, cleared once the stamps of the first factorisation are printed
  bool debug = false;
  DevBuf<long long> dbg;
  static constexpr size_t DBG_N = 8 * (CHOLDAG_MAX_NBR + 1);      // the most stamps a kernel writes (k_chol_big_dag; k_cholesky_ll: 128)
  static_assert(DBG_N >= 128, "stamps of k_cholesky_ll");

  // the dynamic LDS the kernels may ask for (once per process and device)
  static void set_attrs() {
    constexpr size_t b64 = cholb_lds(CHOLB_MAX_NB, CLD, sizeof(double));
    constexpr size_t b20 = cholb_lds(CHOLB_LD20_MAX_NB, 20, sizeof(float)), b17 = cholb_lds(16, 17, sizeof(float));
    set_lds(&k_cholesky_blocked<T>, b64);
    if constexpr (sizeof(T) == 4) {
      set_lds(&k_cholesky_blocked<T, 16, 20>, b20);
      set_lds(&k_cholesky_blocked<T, 16, 17>, b17);
      set_lds(&k_cholesky_blocked<T, CHOLB_MAX_NB, 20, true>, b64);
      set_lds(&k_cholesky_blocked<T, 16, 20, true>, b20);
      set_lds(&k_cholesky_blocked<T, 16, 17, true>, b17);
    }
    set_lds(&k_cholesky_stream, CHOL_STREAM_LDS_BUDGET);
    set_lds(&k_cholesky_ll<T>, CLL_LDS_BYTES);
    set_lds(&k_chol_big_step, cholbig_lds<double>());
    set_lds(&k_chol_big_dag<double>, cholbig_lds<double>());
    set_lds(&k_chol_big_dag<float>, cholbig_lds<float>());
  }

  void arm_debug(bool on, hipStream_t stream) { debug = on; if (on) { dbg.alloc(DBG_N); dbg.zero(stream); } }

  void on_upload(hipStream_t stream) {
    if constexpr (sizeof(T) == 4) {
      // the largest triangle a one-workgroup f32 factorisation takes (16 block rows of 17-float rows; 14 of 20-float rows are fewer),
      // whatever this upload's system: zero once -- n and the route, hence the layout, stay what they are until the next upload
      img.alloc(cholb_tri(CLL_MAX_NB, 17));
      img.zero(stream);
    }
    img_ok = false;
  }

  // form_reduced: where k_build_exchange stores the f32 image for the solve of `untied` (the plan of the C * NCP system), or null.
  // wanted: the library's own single-rank loop building the free cameras' untied system in E_own
  float* image_for(const CholPlan& untied, bool wanted) const { return (wanted && untied.img_ld != 0 && img.n != 0) ? img.p : nullptr; }
  void image_written(bool yes) { img_ok = yes; }

  // what the kernels of a solve are passed: the system (E: n unknowns, tie / first: its map to the C cameras' parameters, or null)
  struct Sys { hipStream_t stream; double* E; int n, C; LMState* st; double* D2c; ParamSets<T> ps; double* delta_c; const int32_t *tie, *first; };

  // every k_cholesky_blocked launch; with an image (fp32 engine only) the instance that copies it
  template <int MAXNB, int LD32, bool IMG = false>
  void launch_blocked(const Sys& s, const CholPlan& p, size_t lds, long long* stamps, const float* image) {
    if constexpr (!IMG && sizeof(T) == 4) {
      if (image) return launch_blocked<MAXNB, LD32, true>(s, p, lds, stamps, image);
    }
    hipLaunchKernelGGL((k_cholesky_blocked<T, MAXNB, LD32, IMG>), dim3(1), dim3(CHOLB_LDS_THREADS), lds, s.stream, s.E, s.C, s.st, s.D2c,
                       s.ps, s.delta_c, s.n, s.tie, s.first, stamps, p.ld32 != 0 ? 1 : 0, p.f32_tau, image);
  }

  // image_usable: s.E is the untied system form_reduced built in E_own
  void solve(const CholPlan& p, const Sys& s, bool image_usable) {
    hipStream_t stream = s.stream;
    const int nb = p.nb, n_sys = s.n;
    // the f32 image k_build_exchange left beside E_own (img_ok: nothing has written E_own since)
    const float* image = (img_ok && image_usable && p.img_ld != 0) ? img.p : nullptr;
    long long* stamps = debug ? dbg.p : nullptr;
    switch (p.route) {
      case CholRoute::LL:
      case CholRoute::LL_F32:
        // up to 256 unknowns (23 cameras): left-looking, factor on chip (sba_chol_ll.hpp)
        if (work.n < (size_t)nb * (nb + 1) / 2 * CB * CB) work.alloc((size_t)CLL_MAX_NB * (CLL_MAX_NB + 1) / 2 * CB * CB);
        // fp32 engine (round 4): the right-looking all-in-LDS kernel on f32 lanes in front of it; the f64 kernel then only runs when
        // that factorisation refused the system (LMState::chol_retry)
        if constexpr (sizeof(T) == 4) {
          if (p.route == CholRoute::LL_F32) {
            if (p.ld32 == 20) launch_blocked<16, 20>(s, p, p.lds_f32, nullptr, image);
            else launch_blocked<16, 17>(s, p, p.lds_f32, nullptr, image);
          }
        }
        hipLaunchKernelGGL(k_cholesky_ll<T>, dim3(1), dim3(CLL_THREADS), p.lds, stream, s.E, s.C, s.st, s.D2c, s.ps, s.delta_c, n_sys, s.tie,
                           s.first, work.p, stamps, p.route == CholRoute::LL_F32 ? 1 : 0);
        break;
      case CholRoute::BLOCKED:
        launch_blocked<CHOLB_MAX_NB, 20>(s, p, p.lds, stamps, image);
        break;
      case CholRoute::STREAM:
        // 17 .. 46 cameras: one workgroup, left-looking, finished block columns streamed through L2
        if (sol.n < (size_t)n_sys) { sol.alloc(n_sys); info.alloc(1); }
        if (work.n < (size_t)nb * (nb + 1) / 2 * CB * CB) work.alloc((size_t)nb * (nb + 1) / 2 * CB * CB);
        hipLaunchKernelGGL(k_chol_prepare, dim3((n_sys + 255) / 256), dim3(256), 0, stream, s.E, n_sys, s.st, s.D2c, sol.p);
        hipLaunchKernelGGL(k_cholesky_stream, dim3(1), dim3(CHOLB_THREADS), p.lds, stream, s.E, n_sys, work.p, sol.p, info.p, s.st,
                           p.stream_cap, stamps);
        hipLaunchKernelGGL(k_chol_epilogue<T>, dim3(1), dim3(1024), 0, stream, s.E, s.C, n_sys, s.st, s.D2c, s.ps, s.delta_c, sol.p, info.p,
                           s.tie, s.first);
        break;
      default:
        // 24 .. 128 cameras: multi-workgroup factorisation (sba_chol_big.hpp)
        solve_big(s, p);
        break;
    }
    if (debug) print_stamps(p, n_sys, stream);
  }

  // SBA_CHOL_DEBUG: the stamps of the solve just enqueued on stderr (waits for it)
  void print_stamps(const CholPlan& p, int n_sys, hipStream_t stream) {
    const bool dag32 = p.route == CholRoute::BIG_DAG_F32;
    switch (p.route) {
      case CholRoute::LL:
      case CholRoute::LL_F32: print_ll_stamps(read_stamps(dbg, 128, stream), p.nb); break;
      case CholRoute::BLOCKED: print_blocked_stamps(read_stamps(dbg, 64, stream), p.nb); break;
      case CholRoute::STREAM: print_stream_stamps(read_stamps(dbg, 8, stream)); break;
      case CholRoute::BIG_LAUNCHES: return;      // its kernels write none: the next solve with another route prints
      default: print_dag_stamps(read_stamps(dbg, DBG_N, stream), cholbig_npad(n_sys) / BB, dag32); break;
    }
    debug = false;
  }

  // factorisation, both substitutions and the LM epilogue (k_chol_epilogue's work) of a large reduced system
  void solve_big(const Sys& s, const CholPlan& p) {
    hipStream_t stream = s.stream;
    const int n_sys = s.n;
    const int npad = cholbig_npad(n_sys), nbr = npad / BB, nbx = (n_sys + BB - 1) / BB;
    if (W.n < (size_t)npad * npad) {
      W.alloc((size_t)npad * npad); Minv.alloc((size_t)nbr * BB * BB); Ld.alloc((size_t)nbr * BB * BB);
      // k_chol_big_back_all: x, one copy per parity of its epoch, "empty" until stored.  The copies lie yv.n / 2 apart, the npad
      // of the largest system the handle has solved, whatever the system of a launch (a smaller one uses the front of each copy)
      yv.alloc(2 * (size_t)npad);
      std::vector<long long> empty(2 * (size_t)npad, CHOLBIG_X_EMPTY);
      HIPCHK(hipMemcpyAsync(yv.p, empty.data(), empty.size() * sizeof(long long), hipMemcpyHostToDevice, stream));
      HIPCHK(hipStreamSynchronize(stream));
      yv_ext[0] = yv_ext[1] = 0;
    }
    if (sol.n < (size_t)n_sys) { sol.alloc(n_sys); info.alloc(1); }
    const bool dag = p.route != CholRoute::BIG_LAUNCHES, dag32 = p.route == CholRoute::BIG_DAG_F32;
    if (dag) {
      // factorisation (and k_chol_big_prepare's work) in one launch: a walker workgroup on the diagonal, workgroup = tile behind it,
      // columns handed over through flags (sba_chol_big.hpp).  fp32 engine: on f32 lanes first, the f64 instance behind it only
      // runs when that one refused the system (LMState::chol_retry)
      if (dag_flags.n == 0) { dag_flags.alloc(choldag_nflags(CHOLDAG_MAX_NBR)); dag_flags.zero(stream); }
      if (Mimg.n == 0) Mimg.alloc((size_t)CHOLDAG_MAX_NBR * choldag_img<double>());
      const dim3 grid(1 + nbr * (nbr + 1) / 2);
      if (dag32)
        hipLaunchKernelGGL(k_chol_big_dag<float>, grid, dim3(CHOLBIG_THREADS), p.lds_f32, stream, s.E, n_sys, s.st, s.D2c,
                           reinterpret_cast<float*>(W.p), npad, reinterpret_cast<float*>(Mimg.p), dag_flags.p, ++dag_epoch, info.p, 0,
                           p.f32_tau, debug ? dbg.p : nullptr);
      hipLaunchKernelGGL(k_chol_big_dag<double>, grid, dim3(CHOLBIG_THREADS), p.lds, stream, s.E, n_sys, s.st, s.D2c, W.p, npad, Mimg.p,
                         dag_flags.p, ++dag_epoch, info.p, dag32 ? 1 : 0, 0.0, (debug && !dag32) ? dbg.p : nullptr);
    } else {
      hipLaunchKernelGGL(k_chol_big_prepare, dim3(nbr * (nbr + 1) / 2), dim3(256), 0, stream, s.E, n_sys, s.st, s.D2c, W.p, npad, info.p);
      for (int j = 0; j < nbr; ++j) {
        const int q = nbr - 1 - j;
        hipLaunchKernelGGL(k_chol_big_step, dim3(std::max(1, q * (q + 1) / 2)), dim3(CHOLBIG_THREADS), p.lds, stream, W.p, npad, j, Minv.p,
                           Ld.p, info.p, s.st);
      }
    }
    // the whole back substitution in one launch: block row = workgroup, x_b handed over as its own flag; block row 0 runs the epilogue.
    // The launch stores its x into the first nbx * BB entries of the copy of its parity and empties the other copy as far as any
    // launch before it -- of this solve or of an earlier one with another system size -- may have stored into it: after every launch
    // the other copy is empty as a whole, so the next launch finds nothing but its own x there, whatever its size.
    const int par = (int)(++epoch & 1), xstride = (int)(yv.n / 2);
    const int nclear = std::max(yv_ext[1 - par], nbx * BB);
    hipLaunchKernelGGL(k_chol_big_back_all<T>, dim3(nbx), dim3(256), 0, stream, (const void*)W.p, npad, n_sys, Ld.p, Minv.p, yv.p, xstride,
                       nclear, epoch, sol.p, info.p, s.st, dag ? (const void*)Mimg.p : (const void*)nullptr, dag32 ? 1 : 0, s.E, s.C, s.D2c,
                       s.ps, s.delta_c, s.tie, s.first);
    yv_ext[1 - par] = 0;
    yv_ext[par] = nbx * BB;
  }
};

}  // namespace SBA_NS
