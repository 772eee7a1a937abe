// MultiLevelPoisson handle (struct src/MultiLevelPoisson.jl:61-77) — internal C++ definition behind `wl_mg`.
#pragma once
#include <algorithm>
#include <functional>
#include <vector>

#include "wl_comm.hpp"

bool wl_mg_divisible(int n);      // divisible(N)  src/MultiLevelPoisson.jl:52
// result slots of the z-split smoother's plane ranges: written by smooth!'s kernel B, summed by solver!
struct WlNormSlots { int d, f; };
inline constexpr WlNormSlots WL_ZS_NORMS[3] = {{WL_RD_L1, WL_RF_LINF}, {WL_RD_L1_Z1, WL_RF_LINF_Z1}, {WL_RD_L1_Z2, WL_RF_LINF_Z2}};

struct wl_mg {
  struct Level {            // one `Poisson` (src/Poisson.jl:22-39)
    wl_grid g; GridX x_;
    float *L = nullptr, *D = nullptr, *iD = nullptr, *x = nullptr, *eps = nullptr, *r = nullptr, *z = nullptr;
    float *em = nullptr, *rs = nullptr;   // scratch of the fused smoother: ϵ after sweep 2, new residual (ghosts stay zero)
    float* wx = nullptr;                  // exchange buffer W (wl_abwide.hpp): both of them as one float4 per pair, for the smooth! that plan_smooth calls wide; null: the level has none
    wl::ConstL cl{};                 // constant-coefficient level (verified at update!)
    bool xzero = false;              // x ≡ 0 is implied (the V-cycle's fill!(x,0) was skipped): the next Jacobi! writes x instead of updating it
    // body levels: the coefficients deviate from the constant pattern only on planes [za,zb]; smooth! runs the pair kernels on the other planes
    bool part = false; int za = 0, zb = -1; wl::ConstL clp{};
    bool pend = false;       // the V-cycle's prolongate!+increment! of this level is deferred into the next smooth! (fused kernel A)
    bool dist = false;       // z-slab distributed level (halo exchanges) vs replicated on every rank
    GridX view;              // replicated level fed by a distributed parent: the planes of the full array this rank computes
    bool has_view = false;
  };
  wl_comm* comm = nullptr;   // not owned
  std::vector<Level> lv;
  std::vector<int16_t> n;   // pois.n :66
  unsigned perdir = 0;
  bool use_constl = true;   // allow the constant-coefficient specialisations where the pattern is verified
  bool store_eps = true;    // the blocked smoother also stores the final ϵ (p.ϵ of the reference); the mom_step! composite turns it off
  // skip_r: kernel B of the pair smoother does not store the residual where nobody reads it (wl::B_XONLY).  Acts only on a single-domain level (not dist,
  // part, perdir) that runs the constant-coefficient pair kernels with a pending prolongation, with store_eps off and the norms coming out of the kernel.
  //   coarse levels, inside vcycle(): always — the caller reads only coarse.x and the next restrict! overwrites coarse.r, so a coarse level's r (and what
  //     wl_mg_level_field hands out for it) is unspecified scratch under skip_r;
  //   finest level, inside solve(): iteration k skips iff the previous solve of the same slot (rskip_slot, set by the caller for the next solves; −1: never
  //     skip) stopped at exactly k iterations.  If the loop goes on after a skipped store, the r-only instance (wl::B_RONLY, same arguments) produces r
  //     before the next V-cycle; if the loop ends there, r stays stale until somebody asks for it (settle_r: wl_mg_level_field, wl_mg_smooth, wl_mg_vcycle) —
  //     the next solve rebuilds r from scratch and forgets the debt.
  // Off by default: wl_mg_* users see every store; the mom_step! composite turns it on (option "rskip").
  bool skip_r = false;
  int rskip_slot = -1;
  int rskip_hist[2] = {0, 0};      // iterations of the last solve that stood, per slot (0: none yet — store)
  bool r_stale_wide = false;                        // … and where that launch read ϵ_mid and r′: the level's exchange buffer W (the late store reads the same)
  bool r_stale = false; float r_stale_w = 0.f;      // lv[0].r was not written by the last smooth!(0): kernel B's inputs lv[0].em, lv[0].rs are intact, ω as given
  hipStream_t r_stale_stream = nullptr;             // … and the stream that launch ran on: where a stream-less reader (wl_mg_level_field) has r produced, and waits for it
  wl::ConstL r_stale_cl{};                          // … and the coefficients it ran with: the late store is that pair kernel again, whatever "pair" or "constl" have been set to since
  long n_rskip = 0, n_rskip_redo = 0;      // finest-level launches that skipped the store / r-only launches (lazy ones included)
  long n_wide = 0;                         // finest-level smooth! calls that went through the exchange buffer W
  int settle_r(hipStream_t s);
  int settle_r_for_reader();
  bool use_fused = true;    // temporally blocked GaussSeidelRB! on eligible levels (wl_fused.hip)
  bool use_zsplit = true;   // body levels: constant-coefficient pair kernels on the planes away from the body, general kernels on the rest
  long zsplit_min = 16L << 20;   // ... on levels of at least this many cells (smaller ranges do not fill 256 CUs; with the 16-row pair tiles a 256³ level gains 2 %, 384³ 4 %, 512³ 7 %; 128³ levels lose)
  bool skip_fill = true;    // Vcycle!'s fill!(coarse.x,0) folded into the coarse level's Jacobi! (x = ω·ϵ instead of x += ω·ϵ)
  bool defer_shift = true;  // residual!'s mean shift and solver!'s first norms are folded into the finest level's Jacobi! (z-march kernel) when that is what runs next
  bool shift_pending = false;
  bool deep_halo = true;     // z-slabs with >= 5 ghost planes: one r exchange (5 planes) per smooth! instead of r (2) + ϵ_mid (3) + r' (2)
  // One-shot hook of the next solve(): the projection tail, queued behind every iteration's smoother BEFORE the host reads that iteration's norms and gated on the
  // device by the break test (wl::decide_converged → res_f[WL_RF_GO], also the host's decision): no idle GPU while the host decides, nothing happens if the loop goes on.
  // check_head: 1 — the flag of the first iteration first carries the fused head's mean-shift test (wl_sim's early V-cycle), 2 — declares that shift due
  // (test hook).  Results: tail_stood — the tail ran; head_decided — the device took the head's decision, head_due — and found the shift due (the loop stopped
  // after that iteration: the caller discards the solve).
  struct Spec {
    std::function<int(const float*)> tail; int check_head = 0; bool tail_stood = false, head_decided = false, head_due = false;
    void disarm() { tail = nullptr; check_head = 0; }
    void begin_solve(std::function<int(const float*)>* t, int* check) { t->swap(tail); *check = check_head; disarm(); tail_stood = head_decided = head_due = false; }   // the one place that resets it
  } spec;
  int shift_path = -1;      // how the last solve applied residual!'s mean shift (src/Poisson.jl:95-97): 0 its own pass (k_shift_norms), 1 inside the finest level's
                            // z-marching Jacobi! (deferred), 2 left to the caller (the fused projection head); −1 no solve yet
  hipStream_t side = nullptr; hipEvent_t ev_decided = nullptr;   // the host waits for the copy of such an iteration's norms (this event), not for the tail queued behind it
  double first_hd0 = 0.0;   // res_d[0] as the first iteration's read found it (the fused head's Σr when its check is deferred: wl_sim)
  bool jacobi0_done = false; // the fused projection head (wl_resjac.hip) already ran the V-cycle's first Jacobi! on the finest level and left solver!'s first norms
  int norm_slots = 0;       // z-split smoother: which plane ranges left an (L₁, L∞) pair in their own result slots (WL_ZS_NORMS)
  bool par_ranges = false;  // levels with a body: the plane ranges of the z-split on concurrent streams (wl::par_fork / par_join) — measured SLOWER (sphere 256³ 2.84 -> 3.07 ms: the fork/join events cost more than the overlap of 35–76 µs launches returns); "zsplit_par" turns it on
  int x_halo_depth = 1;     // z-slabs: ghost planes of x refreshed at the end of solver! (the projection tail reads 1; the fused projection head of the NEXT solve reads 2)
  int last_xdefer = -1;     // what the finest level's last smooth! with a pending prolongation decided: 1 = x += ω·x_c↓ deferred to kernel B, 0 = applied by kernel A (−1: none yet)
  bool use_xdefer = true;   // pair smoother: the V-cycle's `x += ω·x_c↓` is applied by kernel B together with its own increment (wl::XDefer)
  bool use_wide = true;     // … and kernel A then hands r′ and ϵ_mid to kernel B through the level's exchange buffer W, where plan_smooth finds the launch eligible
  bool overlap_smooth = true;   // z-slabs: the one deep r exchange of a smooth! overlaps kernel A's interior planes (boundary slices after the wait)
  bool use_tail = true;     // levels of <= WL_TAIL_CELLS cells: the rest of the V-cycle in one launch (k_vcycle_tail)
  bool tail_ok(int first) const;
  int tail(int first, float w, hipStream_t s);
  float* slab = nullptr;    // owns r,ϵ,D,iD of every level and L,x,z of the coarse levels
  void* red = nullptr;      // reduction workspace
  RedWs ws;
  std::vector<double> log_r1, log_rinf, log_w;

  int build(float* x, float* L, float* z, const wl_grid& g0, unsigned per, int maxlevels, wl_comm* c = nullptr);
  int halo(Level& v, float* a, int ncomp, hipStream_t s, int depth = 1, bool wrap = true) { return v.dist ? wl::halo(comm, a, v.x_, ncomp, depth, s, wrap) : 0; }
  // a distributed level whose smooth! runs as the blocked pair kernels (constant coefficients, 3 ghost planes)
  bool pair_slab(const Level& v) const { return v.dist && v.g.k0 >= 3 && use_fused && !perdir && wl::gsrb_pair_ok(v.x_, v.cl); }
  // ---- the predicates the stages of the V-cycle share, each stated once (DESIGN §4.3c lists their users)
  // smooth!(it = 4) of this level runs as kernel A + kernel B (and absorbs a deferred prolongation)
  bool blocked(const Level& v) const { return use_fused && (wl::gsrb_fused_ok(v.x_, perdir, v.dist) || pair_slab(v)); }
  // z-slab with >= 5 ghost planes: one five-plane exchange of r per smooth! — kernel A starts five planes out
  bool deep_slab(const Level& v) const { return v.dist && deep_halo && v.g.k0 >= 5 && v.g.k1 - v.g.k0 >= 5; }
  // ghost planes of coarse.x the prolongation into `fine` reads: the coarse cells under the planes kernel A of fine's smooth! starts on
  int coarse_x_depth(const Level& fine, const Level& coarse) const {
    if (!(fine.dist && blocked(fine))) return 1;
    return deep_slab(fine) && coarse.g.k0 >= 3 && coarse.g.k1 - coarse.g.k0 >= 3 ? 3 : 2;
  }
  // a level with a body: planes [na, nb) around it take the general-coefficient kernels, [k0, na) and [nb, k1) the constant-coefficient ones.
  // na, nb follow za, zb whether or not the split is on (update! decides `part` from them)
  static constexpr int ZSPLIT_MARGIN = 4;      // planes between the body's last deviating plane and the first constant-coefficient one: the reach of one smooth!
  struct ZRanges { bool on; int na, nb; };
  ZRanges zsplit_ranges(const Level& v) const { return {v.part && use_zsplit && !v.dist, std::max(v.g.k0, v.za - ZSPLIT_MARGIN), std::min(v.g.k1, v.zb + ZSPLIT_MARGIN + 1)}; }
  // kernel B of this launch may leave r' unstored (wl::B_XONLY; see skip_r)
  bool b_xonly_ok(const Level& p, int bout, bool want_norms) const {
    return bout == wl::B_XONLY && skip_r && !store_eps && !comm && !p.dist && !p.part && !perdir && wl::gsrb_pair_B_ok(nullptr, p.r, p.x, p.em, p.rs, p.x_, p.cl) &&
           (!want_norms || wl::gsrb_pair_B_kernel_norms(p.x_));
  }
  // ---- smooth! in forms: decided once per call (plan_smooth), one function per form, one epilogue (smooth)
  //   Passes           gs_init (+ sweep 1), one kernel per further sweep, increment!; a pending prolongation is flushed first
  //   Blocked          kernel A, kernel B; z-slabs: r (2 planes) before A, ϵ_mid (3) [+ r' (2)] before B
  //   DeepSlab         z-slab with a pending prolongation and >= 5 ghost planes: r five planes deep, then A on the extended range, then B
  //   DeepSlabOverlap  … that exchange in flight while A computes the interior planes; the two boundary slices follow the wait
  //   ZSplit           Blocked on the three plane ranges of zsplit_ranges, each with its own coefficients and result slots
  enum class Smooth { Passes, Blocked, DeepSlab, DeepSlabOverlap, ZSplit };
  struct SmoothPlan {
    Smooth form; bool pro;      // pro: the level's pending prolongate!+increment! runs as a stage of kernel A (every form but Passes)
    bool xdefer;                // … and its `x += ω·x_c↓` is handed on to kernel B (wl::XDefer); ZSplit decides per range and reports the last range's
    int bout;                   // wl::BOut of kernel B
    bool want_norms;
    bool wide = false;          // Blocked with pro and xdefer, no store_eps, on a level that has W: r′ and ϵ_mid travel through W; every other launch uses p.rs and p.em
  };
  SmoothPlan plan_smooth(const Level& p, int it, bool want_norms, int bout) const;
  int smooth_passes(Level& p, int l, int it, float w, hipStream_t s);
  int smooth_blocked(Level& p, Level* coarse, int l, float w, const SmoothPlan& plan, hipStream_t s);
  int smooth_deep_slab(Level& p, Level& coarse, int l, float w, const SmoothPlan& plan, hipStream_t s);
  int smooth_zsplit(Level& p, Level* coarse, int l, float w, SmoothPlan* plan, hipStream_t s);
  int exchange_for_B(Level& p, bool with_rs, hipStream_t s);
  // ---- Vcycle! in stages
  int jacobi_fine(int l, hipStream_t s);
  int restrict_to_coarse(int l, bool to_tail, hipStream_t s);
  int descend(int l, bool to_tail, float w, hipStream_t s);
  int prolong(int l, float w, bool defer, hipStream_t s);
  // ---- solver! in stages
  struct SolveRun;
  int initial_residual(int itmx, bool have_residual, bool head_read, hipStream_t s);
  int iteration(SolveRun& st, hipStream_t s);
  void apply_norms(SolveRun& st);
  ~wl_mg();
  int update(hipStream_t s);
  int smooth(int l, int it, float w, hipStream_t s, bool want_norms = false, bool* norms_done = nullptr, int bout = 0);   // bout = wl::B_XONLY: r' need not be stored (honoured where skip_r acts)
  int vcycle(int l, float w, hipStream_t s, bool defer = false);
  int flush_pending(int l, float w, hipStream_t s);
  // have_residual: r and the local Σr (ws.res_d[0]) were already produced by the caller's fused div+residual kernel
  // pre_r1 / pre_rinf: the norms of the initial residual are already on the host (the fused projection head's read-back, combined over ranks)
  int solve(double tol, int itmx, int* host_n, double* host_r1, float* host_rinf, hipStream_t s, bool have_residual = false, const double* pre_r1 = nullptr, const float* pre_rinf = nullptr);
};
