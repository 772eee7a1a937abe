// The MultiLevelPoisson handle `wl_mg` (wl_mg.hpp): build, update!, smooth!, Vcycle!, solver!.  Host code only — the kernels are in namespace wl.
#include <cmath>
#include <cstdlib>
#include <utility>

#include "wl_common.hpp"
#include "wl_mg.hpp"

bool wl_mg_divisible(int n) { return (n % 2 == 0) && n > 4; }   // src/MultiLevelPoisson.jl:52

int wl_mg::build(float* x, float* L, float* z, const wl_grid& g0, unsigned per, int maxlevels, wl_comm* c) {
  perdir = per; comm = (c && c->size > 1) ? c : nullptr;
  WL_TRY(wl_ctx_ensure());
  WL_HIP(hipMalloc(&red, wl_red_bytes()));
  ws = wl_red_ws(red);
  const bool dist0 = comm && g0.D == 3 && g0.nz != g0.gnz;
  if (dist0 && ((per >> 2) & 1u) && !comm->zperiodic) { wl_set_error("z-periodic z-slabs need a communicator in periodic mode (wl_comm_set_periodic)"); return WL_EINVAL; }
  // level 1 aliases the caller's arrays; r,ϵ,D,iD owned                                 src/Poisson.jl:32-38
  std::vector<wl_grid> grids; std::vector<char> isdist; std::vector<wl_grid> views; std::vector<char> hasview;
  grids.push_back(g0); isdist.push_back(dist0); views.push_back(g0); hasview.push_back(0);
  while ((int)grids.size() <= maxlevels) {                                               // :70
    const wl_grid f = grids.back(); const bool fd = isdist.back();
    const bool cx = wl_mg_divisible(f.nx), cy = wl_mg_divisible(f.ny), cz = (f.D == 3) && wl_mg_divisible(f.gnz);
    if (!(cx || cy || cz)) break;                                                        // wl_mg_divisible(l) :54
    wl_grid cgr = f; wl_grid vw = f; bool cd = fd, hv = false;
    if (cx) cgr.nx = 1 + f.nx / 2;                                                       // restrictML :36
    if (cy) cgr.ny = 1 + f.ny / 2;
    const int gnz_c = cz ? 1 + f.gnz / 2 : f.gnz;
    if (!fd) { if (f.D == 3) { cgr.gnz = gnz_c; cgr.nz = gnz_c; cgr.k0 = 1; cgr.k1 = gnz_c - 1; cgr.gk = 0; } }
    else {
      const int nloc = f.k1 - f.k0;
      const int nc = cz ? nloc / 2 : nloc;
      // stay distributed while the local planes pair up and the level is still big; otherwise replicate on every rank
      // levels of <= 64 planes are replicated: their halo exchanges would be pure latency (7 per V-cycle and level) while the
      // whole level costs less than that to recompute on every rank
      // (WL_REPLICATE_PLANES overrides the 64: the tests use it to build, with 4 ranks, the small distributed slabs an 8-rank run has)
      static const int repl = [] { const char* e = getenv("WL_REPLICATE_PLANES"); const int v = e ? atoi(e) : 64; return v >= 8 ? v : 64; }();
      // … and a level whose local plane count is odd cannot be coarsened slab by slab (its plane pairs would straddle the ranks): the level that
      // would come out odd AND is coarsened again in z is replicated right away — any nz with an even number of planes per rank works, not only P·2^k
      const bool odd_next = wl_mg_divisible(gnz_c) && (nc % 2 != 0);
      const bool keep = (!cz || (nloc % 2 == 0)) && nc >= 1 && (gnz_c - 2) > repl && !odd_next;
      if (cz && (nloc % 2 != 0)) { wl_set_error("z-slab: the finest level needs an even number of planes per rank"); return WL_EINVAL; }
      if (keep) {
        cgr.gnz = gnz_c; cgr.k0 = f.k0; cgr.k1 = cgr.k0 + nc; cgr.nz = nc + 2 * cgr.k0;
        cgr.gk = (cz ? (f.gk + f.k0 + 1) / 2 : f.gk + f.k0) - cgr.k0;
      } else {   // replicated: full array; this rank computes the planes below its own fine planes, then all-gathers
        cd = false; hv = true;
        cgr.gnz = gnz_c; cgr.nz = gnz_c; cgr.k0 = 1; cgr.k1 = gnz_c - 1; cgr.gk = 0;
        vw = cgr; vw.k0 = cz ? (f.gk + f.k0 + 1) / 2 : f.gk + f.k0; vw.k1 = vw.k0 + nc;
      }
    }
    grids.push_back(cgr); isdist.push_back(cd); views.push_back(vw); hasview.push_back(hv);
  }
  if (grids.size() <= 2) { wl_set_error("MultiLevelPoisson requires size=a2ⁿ, where n>2"); return WL_ELEVELS; }   // :73-74
  // one slab allocation for everything the handle owns
  size_t total = 0;
  for (size_t l = 0; l < grids.size(); l++) { const size_t nc = (size_t)wl_ncell(grids[l]); total += (l == 0 ? 6 : 6 + 2 + (size_t)grids[l].D) * nc; }
  WL_HIP(hipMalloc((void**)&slab, total * sizeof(float)));
  WL_HIP(hipMemset(slab, 0, total * sizeof(float)));
  float* p = slab;
  lv.resize(grids.size());
  for (size_t l = 0; l < grids.size(); l++) {
    Level& v = lv[l]; v.g = grids[l]; v.x_ = gx(grids[l]); v.dist = isdist[l]; v.has_view = hasview[l]; v.view = gx(views[l]);
    const size_t nc = (size_t)wl_ncell(grids[l]);
    v.r = p; p += nc; v.eps = p; p += nc; v.D = p; p += nc; v.iD = p; p += nc; v.em = p; p += nc; v.rs = p; p += nc;
    if (l == 0) { v.x = x; v.L = L; v.z = z; }
    else { v.L = p; p += nc * (size_t)grids[l].D; v.x = p; p += nc; v.z = p; p += nc; }
  }
  // the exchange buffers W of the levels that can run the pair kernels on a single domain (512-byte aligned by hipMalloc, zeroed once: its ghost rows and planes
  // are never written).  A level whose allocation fails keeps the dense exchange.
  if (!c && !per) for (Level& v : lv) {
    const size_t wb = v.dist ? 0 : wl::gsrb_pair_wide_bytes(v.x_);
    if (!wb) continue;
    if (hipMalloc((void**)&v.wx, wb) != hipSuccess) { (void)hipGetLastError(); v.wx = nullptr; continue; }
    WL_HIP(hipMemset(v.wx, 0, wb));
  }
  hipStream_t s = 0;
  WL_TRY(update(s));                                                                       // restrictML :39 + Poisson ctor :36
  WL_HIP(hipStreamSynchronize(s));
  return 0;
}
wl_mg::~wl_mg() { for (Level& v : lv) if (v.wx) (void)hipFree(v.wx); if (slab) (void)hipFree(slab); if (red) (void)hipFree(red); if (side) (void)hipStreamDestroy(side); if (ev_decided) (void)hipEventDestroy(ev_decided); }

// coarse face coefficients of level l from level l-1 (restrictL! :42-48), slab aware
static int restrictL_level(wl_mg& m, size_t l, hipStream_t s) {
  wl_mg::Level& c = m.lv[l]; wl_mg::Level& f = m.lv[l - 1];
  if (c.has_view) {          // distributed parent -> replicated child: compute my planes, all-gather, then BC!(a,0) on the full array
    const float zero[3] = {0.f, 0.f, 0.f};
    WL_TRY(wl::restrictL(c.L, c.view, f.L, f.x_, m.perdir, s));     // (its BC pass is redone below on the complete array)
    WL_TRY(wl::allgather_planes(m.comm, c.L, c.view, c.g.D, s));
    return wl::bc_vec(c.L, c.x_, zero, 0, m.perdir, s);
  }
  WL_TRY(wl::restrictL(c.L, c.x_, f.L, f.x_, m.perdir, s));
  return m.halo(c, c.L, c.g.D, s);
}
int wl_mg::update(hipStream_t s) {                                                        // update! :79-86
  WL_TRY(halo(lv[0], lv[0].L, lv[0].g.D, s));
  WL_TRY(wl::set_diag(lv[0].D, lv[0].iD, lv[0].L, lv[0].x_, s));
  for (size_t l = 1; l < lv.size(); l++) {
    WL_TRY(restrictL_level(*this, l, s));
    WL_TRY(wl::set_diag(lv[l].D, lv[l].iD, lv[l].L, lv[l].x_, s));
  }
  // constant-coefficient detection (exact, on device): only the levels that run the specialised kernels are checked
  for (size_t l = 0; l < lv.size(); l++) {
    lv[l].cl.on = 0; lv[l].part = false;
    // (the levels of the single-launch tail too, when the finest level passed: the LDS-resident tail then evaluates L, D, iD instead of loading them)
    const bool tail_level = l > 0 && use_tail && lv[0].cl.on && lv[l].g.D == 3 && !lv[l].dist && lv[l].x_.cs <= WL_TAIL_CELLS;
    if (use_constl && !perdir && (l == 0 || tail_level || wl::gsrb_fused_ok(lv[l].x_, perdir, lv[l].dist) || (lv[l].dist && wl::gsrb_pair_geom_ok(lv[l].x_)))) {
      WL_TRY(wl::check_const_L(lv[l].L, lv[l].x_, &lv[l].cl, (int*)(ws.res_f + WL_RF_IFLAG), s));
      if (lv[l].dist && comm && comm->size > 1) {   // every rank must take the same path (the slab kernels differ in their halo exchanges)
        const float bad = lv[l].cl.on ? 0.f : 1.f; float any = 1.f;
        WL_HIP(hipMemcpyAsync(ws.res_f + WL_RF_IFLAG, &bad, sizeof(float), hipMemcpyHostToDevice, s));
        WL_TRY(wl::combine_results(comm, ws, s));                                          // res_f: max over ranks
        WL_HIP(hipMemcpyAsync(&any, ws.res_f + WL_RF_IFLAG, sizeof(float), hipMemcpyDeviceToHost, s));
        WL_HIP(hipStreamSynchronize(s));
        if (any != 0.f) lv[l].cl.on = 0;
      }
      // a body: the pattern holds on most planes — find the planes where it does not (z-split smoother)
      Level& v = lv[l];
      if (!v.cl.on && !v.dist && v.g.D == 3 && wl::gsrb_fused_ok(v.x_, perdir, v.dist) && wl::gsrb_pair_geom_ok(v.x_) && v.cl.c[0] != 0.f) {
        WL_TRY(wl::const_plane_range(v.L, v.x_, v.cl.c, &v.za, &v.zb, s));
        const ZRanges z = zsplit_ranges(v);
        const int far = (z.na - v.g.k0) + (v.g.k1 - z.nb);
        v.part = v.zb >= v.za && far >= 16 && far * 4 >= (v.g.k1 - v.g.k0) && v.x_.cs >= zsplit_min;     // worth it: at least a quarter of the planes are far
        v.clp = v.cl; v.clp.on = 1;
      }
    }
  }
  return 0;
}
// the deferred `prolongate!; increment!` of level l, executed on its own (when the next smooth! cannot absorb it)
int wl_mg::flush_pending(int l, float w, hipStream_t s) {
  Level& fine = lv[(size_t)l]; Level& coarse = lv[(size_t)l + 1];
  fine.pend = false;
  ProfScope pp(l == 0 ? WL_PROF_PROLONG : -1, s);
  if (perdir) {
    WL_TRY(wl::prolongate(fine.eps, fine.x_, coarse.x, coarse.x_, s));
    WL_TRY(wl::bc_per_scalar(fine.eps, fine.x_, perdir, s));
    WL_TRY(halo(fine, fine.eps, 1, s));
    return wl::increment(fine.r, fine.x, fine.eps, fine.L, fine.D, fine.x_, w, s);
  }
  return wl::prolong_increment(fine.r, fine.x, fine.eps, coarse.x, fine.L, fine.D, fine.x_, coarse.x_, w, true, s);
}
// the residual of the finest level that a smooth! with skip_r left unwritten: kernel B again with the same arguments, storing r' only
int wl_mg::settle_r(hipStream_t s) {
  if (!r_stale) return 0;
  Level& p = lv[0];
  r_stale = false; n_rskip_redo++;
  // the pair kernel itself, with the coefficients of the launch that skipped the store — not gsrb_fused_B's choice of today: the process-wide "pair" switch or
  // "constl" (update!) may have withdrawn the pair kernels since, and only they store r' alone
  return wl::gsrb_pair_B(nullptr, p.r, p.x, p.em, p.rs, p.x_, r_stale_w, nullptr, WL_RD_L1, WL_RF_LINF, r_stale_cl, s, nullptr, wl::B_RONLY, r_stale_wide ? p.wx : nullptr);
}
// … for a reader that names no stream: behind the launch that skipped the store, on its stream (stream 0 if that stream is gone), and complete on return —
// whichever stream the caller then reads r on finds it current
int wl_mg::settle_r_for_reader() {
  if (!r_stale) return 0;
  hipStream_t s = r_stale_stream;
  if (s) { const hipError_t q = hipStreamQuery(s); if (q != hipSuccess && q != hipErrorNotReady) { (void)hipGetLastError(); s = nullptr; } }
  WL_TRY(settle_r(s));
  WL_HIP(hipStreamSynchronize(s));
  return 0;
}
// ================================================================================================
// GaussSeidelRB!(p;it,ω)                                                                 src/Poisson.jl:141-148
// ================================================================================================
// the plane ranges of a level with a body, in launch order: around the body (the level's own coefficients), below it, above it (the constant pattern)
struct ZPart { int a, b; const wl::ConstL* cl; bool any() const { return b > a; } GridX of(GridX g) const { g.k0 = a; g.k1 = b; return g; } };
static void zsplit_parts(const wl_mg& m, const wl_mg::Level& v, ZPart out[3]) {
  const wl_mg::ZRanges z = m.zsplit_ranges(v);
  out[0] = {z.na, z.nb, &v.cl}; out[1] = {v.g.k0, z.na, &v.clp}; out[2] = {z.nb, v.g.k1, &v.clp};
}
wl_mg::SmoothPlan wl_mg::plan_smooth(const Level& p, int it, bool want_norms, int bout) const {
  SmoothPlan q{Smooth::Passes, false, false, wl::B_BOTH, want_norms};
  if (!(it == 4 && blocked(p))) return q;
  q.pro = p.pend;
  q.form = zsplit_ranges(p).on ? Smooth::ZSplit : !(q.pro && deep_slab(p)) ? Smooth::Blocked : (overlap_smooth && p.x_.k1 - p.x_.k0 >= 16) ? Smooth::DeepSlabOverlap : Smooth::DeepSlab;
  q.xdefer = q.pro && use_xdefer && wl::gsrb_pair_B_ok(store_eps ? p.eps : nullptr, p.r, p.x, p.em, p.rs, p.x_, p.cl);
  if (q.pro && q.form == Smooth::Blocked && b_xonly_ok(p, bout, want_norms)) q.bout = wl::B_XONLY;   // skip_r: r' stays in kernel B's registers (the norms) — p.em and p.rs are left as they are, so settle_r can still produce it
  // the wide exchange: only the one-launch form on a single domain, with x left to kernel B (kernel A's wide form has no x stage) and the norms, if any, from kernel B
  q.wide = q.form == Smooth::Blocked && q.pro && q.xdefer && use_wide && !store_eps && p.wx && !p.dist && !comm && !perdir && (!want_norms || wl::gsrb_pair_B_kernel_norms(p.x_));
  return q;
}
int wl_mg::smooth(int l, int it, float w, hipStream_t s, bool want_norms, bool* norms_done, int bout) {
  Level& p = lv[(size_t)l];
  if (norms_done) *norms_done = false;
  SmoothPlan plan = plan_smooth(p, it, want_norms, bout);
  if (p.pend && !plan.pro) WL_TRY(flush_pending(l, w, s));
  Level* coarse = plan.pro ? &lv[(size_t)l + 1] : nullptr;
  p.pend = false;
  ProfScope ps(l == 0 ? WL_PROF_SMOOTH : -1, s);   // only the finest level is a named slot
  switch (plan.form) {
    case Smooth::Passes: return smooth_passes(p, l, it, w, s);      // in place, no norms, nothing below applies
    case Smooth::Blocked: WL_TRY(smooth_blocked(p, coarse, l, w, plan, s)); break;
    case Smooth::DeepSlab: case Smooth::DeepSlabOverlap: WL_TRY(smooth_deep_slab(p, *coarse, l, w, plan, s)); break;
    case Smooth::ZSplit: WL_TRY(smooth_zsplit(p, coarse, l, w, &plan, s)); break;
  }
  // the epilogue of every blocked form
  if (!plan.pro) std::swap(p.r, p.rs);      // without the prolongation stage kernel B went from p.r to p.rs
  norm_slots = 0;
  if (plan.form == Smooth::ZSplit && want_norms) { ZPart parts[3]; zsplit_parts(*this, p, parts); for (int i = 0; i < 3; i++) if (parts[i].any()) norm_slots |= 1 << i; }
  if (norms_done) *norms_done = want_norms;
  if (l == 0 && plan.pro) last_xdefer = plan.xdefer ? 1 : 0;
  if (l == 0 && plan.bout == wl::B_XONLY) { r_stale = true; r_stale_w = w; r_stale_stream = s; r_stale_cl = p.cl; r_stale_wide = plan.wide; n_rskip++; }
  if (l == 0 && plan.wide) n_wide++;
  return 0;
}
// kernel B of the level, or of the plane range g of it.  coarse (a prolongation was absorbed): kernel A's extra stage left r' in p.rs and B stores the final
// residual to p.r — and applies `x += ω·x_c↓` too where A handed it on (xdef); else B goes from p.r to p.rs
static int launch_B(wl_mg& m, wl_mg::Level& p, const GridX& g, const wl_mg::Level* coarse, bool xdef, float w, const RedWs* nws, WlNormSlots sl, const wl::ConstL& cl, hipStream_t s, int out = wl::B_BOTH, const float* wide = nullptr) {
  const bool pro = coarse != nullptr;
  const wl::XDefer xd{pro ? coarse->x : nullptr, pro ? coarse->x_ : g, w};
  return wl::gsrb_fused_B(m.store_eps ? p.eps : nullptr, pro ? p.r : p.rs, p.x, p.em, pro ? p.rs : p.r, p.L, g, w, nws, sl.d, sl.f, cl, s, pro && xdef ? &xd : nullptr, out, wide);
}
// z-slab: what kernel B reads across the slab faces — ϵ_mid (3 planes) and, behind a prolongation stage, r' (2 planes) in one RCCL group: one exchange latency instead of two
int wl_mg::exchange_for_B(Level& p, bool with_rs, hipStream_t s) {
  if (!with_rs) return halo(p, p.em, 1, s, 3);
  const bool grp = comm && comm->size > 1 && p.dist;
  if (grp) { WL_TRY(comm->group_begin()); comm->n_halo++; }   // one network round for both arrays
  int rc = halo(p, p.em, 1, s, 3);
  if (rc == 0) rc = halo(p, p.rs, 1, s, 2);
  if (grp) { const int rc2 = comm->group_end(); if (rc == 0) rc = rc2; }
  return rc;
}
// two z-marching kernels instead of six passes (+ the pending prolongation as an extra stage of kernel A).  z-slab: the tile pipeline recomputes the neighbour's
// planes it needs, so the exchanges are r (2 planes) before A and exchange_for_B before B — instead of one exchange per colour sweep
int wl_mg::smooth_blocked(Level& p, Level* coarse, int l, float w, const SmoothPlan& plan, hipStream_t s) {
  bool xdef = plan.xdefer;      // `x += ω·x_c↓` handed from kernel A to kernel B
  WL_TRY(halo(p, p.r, 1, s, 2));
  {
    ProfScope pa(l == 0 ? WL_PROF_GS_A : -1, s);
    if (coarse) WL_TRY(wl::gsrb_fused_A_pro(p.em, p.rs, p.x, p.r, coarse->x, p.L, p.x_, coarse->x_, w, p.cl, s, -(1 << 30), 1 << 30, &xdef, false, plan.wide ? p.wx : nullptr));
    else WL_TRY(wl::gsrb_fused_A(p.em, p.r, p.L, p.x_, p.cl, s));
  }
  WL_TRY(exchange_for_B(p, coarse != nullptr, s));
  ProfScope pb(l == 0 ? WL_PROF_GS_B : -1, s);
  return launch_B(*this, p, p.x_, coarse, xdef, w, plan.want_norms ? &ws : nullptr, WL_ZS_NORMS[0], p.cl, s, plan.bout, plan.wide ? p.wx : nullptr);
}
// z-slab, ONE exchange round per smooth!: r travels 5 planes deep and kernel A also computes r' and ϵ_mid on the 3 (2) ghost planes kernel B reads, instead of
// receiving them (x is updated on the owned planes only).  5 planes instead of 2+3+2, one latency instead of two, ≈6 redundant planes of kernel A per rank.
int wl_mg::smooth_deep_slab(Level& p, Level& coarse, int l, float w, const SmoothPlan& plan, hipStream_t s) {
  bool xdef = plan.xdefer;
  auto sub = [&](int a, int b) { GridX g = p.x_; g.k0 = a; g.k1 = b; return g; };
  const int k0 = p.x_.k0, k1 = p.x_.k1;
  auto A = [&](const GridX& g, bool* xdf, bool range) { return wl::gsrb_fused_A_pro(p.em, p.rs, p.x, p.r, coarse.x, p.L, g, coarse.x_, w, p.cl, s, k0, k1, xdf, range); };
  if (plan.form == Smooth::DeepSlabOverlap) {
    // the exchange runs on the communicator's own stream while kernel A computes the planes that need no ghost plane of r (its outputs [k0+2,k1−2) read r on
    // [k0,k1) only); the two boundary slices (5 planes each, ghost planes included) follow the wait — as conv_diff! does with u
    WL_TRY(wl::halo_async_begin(comm, p.r, p.x_, 1, 5, s));
    ProfScope pa(l == 0 ? WL_PROF_GS_A : -1, s);
    bool xd_i = xdef, xd_l = xdef, xd_h = xdef;
    WL_TRY(A(sub(k0 + 2, k1 - 2), &xd_i, true));
    WL_TRY(wl::halo_async_wait(comm, s));
    WL_TRY(A(sub(k0 - 3, k0 + 2), &xd_l, true));
    WL_TRY(A(sub(k1 - 2, k1 + 3), &xd_h, true));
    if (xd_i != xdef || xd_l != xdef || xd_h != xdef) { wl_set_error("smooth!: the slices of kernel A disagree on the deferred x increment"); return WL_EINVAL; }
  } else {
    WL_TRY(halo(p, p.r, 1, s, 5));
    ProfScope pa(l == 0 ? WL_PROF_GS_A : -1, s);
    WL_TRY(A(sub(k0 - 3, k1 + 3), &xdef, false));
  }
  ProfScope pb(l == 0 ? WL_PROF_GS_B : -1, s);
  return launch_B(*this, p, p.x_, &coarse, xdef, w, plan.want_norms ? &ws : nullptr, WL_ZS_NORMS[0], p.cl, s);
}
// Level with a body: the blocked kernels take plane sub-ranges (k0/k1 of the grid they are given only delimit the planes a launch outputs; inputs are read across
// the cut, outputs are separate arrays).  Planes at least ZSPLIT_MARGIN away from the body run the constant-coefficient pair kernels, the others the general
// kernels — the same bits either way.
// The three plane ranges write disjoint planes and read only what the previous phase left: their launches are independent, and each of them is a latency-bound
// march on an under-filled chip (sphere 256³: 35–76 µs each).  With par_ranges they run concurrently on the main stream and two auxiliary streams (fork: the aux
// streams wait for an event of the main stream; join: the main stream waits for theirs); kernel B needs ALL of kernel A's ranges (its halo reaches across the
// cuts): one join between the two phases.  Partial norms of the ranges land in disjoint thirds of the workspace, their L₁/L∞ in WL_ZS_NORMS; solver! adds them.
int wl_mg::smooth_zsplit(Level& p, Level* coarse, int l, float w, SmoothPlan* plan, hipStream_t s) {
  ZPart parts[3]; zsplit_parts(*this, p, parts);
  bool xdef[3] = {false, false, false};                    // per range: `x += ω·x_c↓` handed from kernel A to kernel B (wl::XDefer)
  const bool par = par_ranges && wl::par_streams_ok() && (long)p.g.nx * p.g.ny <= 520L * 520L;
  hipStream_t sr[3] = {s, par ? wl::par_stream(0) : s, par ? wl::par_stream(1) : s};
  {
    ProfScope pa(l == 0 ? WL_PROF_GS_A : -1, s);
    if (par) WL_TRY(wl::par_fork(s));
    for (int i = 0; i < 3; i++) if (parts[i].any()) {
      const GridX g = parts[i].of(p.x_);
      if (coarse) {
        plan->xdefer = xdef[i] = use_xdefer && wl::gsrb_pair_B_ok(store_eps ? p.eps : nullptr, p.r, p.x, p.em, p.rs, g, *parts[i].cl);
        WL_TRY(wl::gsrb_fused_A_pro(p.em, p.rs, p.x, p.r, coarse->x, p.L, g, coarse->x_, w, *parts[i].cl, sr[i], -(1 << 30), 1 << 30, &xdef[i]));
      } else WL_TRY(wl::gsrb_fused_A(p.em, p.r, p.L, g, *parts[i].cl, sr[i]));
    }
    if (par) WL_TRY(wl::par_join(s));
  }
  ProfScope pb(l == 0 ? WL_PROF_GS_B : -1, s);
  if (par) WL_TRY(wl::par_fork(s));
  for (int i = 0; i < 3; i++) if (parts[i].any()) {
    RedWs wsi = ws;
    if (par) { wsi.pa += (size_t)i * (WL_MAXPART / 3); wsi.pm += (size_t)i * (WL_MAXPART / 3); }
    WL_TRY(launch_B(*this, p, parts[i].of(p.x_), coarse, xdef[i], w, plan->want_norms ? &wsi : nullptr, WL_ZS_NORMS[i], *parts[i].cl, sr[i]));
  }
  if (par) WL_TRY(wl::par_join(s));
  return 0;
}
// one kernel per pass
int wl_mg::smooth_passes(Level& p, int l, int it, float w, hipStream_t s) {
  const bool fuse = !perdir && !p.dist && it >= 1;   // ghost ϵ are plain memory reads only on these levels
  if (fuse) WL_TRY(wl::gs_init_sweep1(p.eps, p.r, p.L, p.iD, p.x_, s));
  else {
    WL_TRY(wl::gs_init(p.eps, p.r, p.iD, p.x_, s));
    WL_TRY(wl::bc_per_scalar(p.eps, p.x_, perdir, s));
    WL_TRY(halo(p, p.eps, 1, s));
  }
  for (int k0 = fuse ? 2 : 1; k0 <= it; k0++) {
    ProfScope pk(l == 0 ? WL_PROF_GS_SWEEP : -1, s);
    WL_TRY(wl::gs_sweep(p.eps, p.r, p.L, p.iD, p.x_, k0, s));
    WL_TRY(halo(p, p.eps, 1, s, 1, false));                                                // neighbour slabs need this colour before the next sweep (no periodic wrap: the reference's ghost cells are stale here)
  }
  WL_TRY(wl::bc_per_scalar(p.eps, p.x_, perdir, s));                                      // perBC!(ϵ) inside increment! :101
  if (comm && comm->zperiodic) WL_TRY(halo(p, p.eps, 1, s));                              // … across the periodic z boundary too
  return wl::increment(p.r, p.x, p.eps, p.L, p.D, p.x_, w, s);
}
// the levels first..end as one launch: "if (first is not the coarsest) Vcycle!(first); smooth!(first)"
bool wl_mg::tail_ok(int first) const {
  if (!use_tail || perdir || first < 1 || first >= (int)lv.size() || (int)lv.size() - first > WL_TAIL_MAXLV) return false;
  if (lv[(size_t)first].g.D != 3 || lv[(size_t)first].x_.cs > WL_TAIL_CELLS) return false;
  for (size_t l = (size_t)first; l < lv.size(); l++) if (lv[l].dist || lv[l].pend) return false;
  return true;
}
int wl_mg::tail(int first, float w, hipStream_t s) {
  wl::TailLevelHost h[WL_TAIL_MAXLV];
  const int n = (int)lv.size() - first;
  for (int q = 0; q < n; q++) {
    const Level& v = lv[(size_t)(first + q)];
    h[q] = wl::TailLevelHost{v.x_, v.L, v.D, v.iD, v.x, v.eps, v.r, 0, 0, 0, &v.cl};
    if (q + 1 < n) { const Level& c = lv[(size_t)(first + q + 1)]; h[q].cx = c.g.nx < v.g.nx; h[q].cy = c.g.ny < v.g.ny; h[q].cz = c.g.gnz < v.g.gnz; }
  }
  return wl::vcycle_tail(h, n, w, s);
}
// ================================================================================================
// Vcycle!(ml;l,ω)                                                                        src/MultiLevelPoisson.jl:88-101
// ================================================================================================
// Jacobi!(fine): ϵ=r·iD; increment!(ω=1)   (perBC!(ϵ) inside increment!)
int wl_mg::jacobi_fine(int l, hipStream_t s) {
  Level& fine = lv[(size_t)l];
  if (l == 0 && jacobi0_done) { jacobi0_done = false; return 0; }   // fused into the projection head (wl_sim::project → wl::resjac)
  ProfScope pj(l == 0 ? WL_PROF_JACOBI : -1, s);
  if (perdir || (fine.dist && !fine.cl.on)) {
    WL_TRY(wl::gs_init(fine.eps, fine.r, fine.iD, fine.x_, s));
    WL_TRY(wl::bc_per_scalar(fine.eps, fine.x_, perdir, s));
    WL_TRY(halo(fine, fine.eps, 1, s));
    return wl::increment(fine.r, fine.x, fine.eps, fine.L, fine.D, fine.x_, 1.f, s);
  }
  // one pass; new residual lands in the ϵ buffer, then the two buffers trade places
  WL_TRY(halo(fine, fine.r, 1, s));              // (slab: ϵ=r·iD of the neighbour's boundary plane is recomputed from its r; iD is evaluated from the position)
  if (l == 0 && shift_pending) { shift_pending = false; WL_TRY(wl::jacobi_pp_shift(fine.eps, fine.r, fine.x, fine.x_, 1.f, fine.cl, ws, WL_RD_L1_INIT, WL_RF_LINF_INIT, s)); }
  else {
    const int xz = fine.xzero ? 1 : 0; fine.xzero = false;      // fill!(x,0) was left to this pass (restrict_to_coarse)
    if (zsplit_ranges(fine).on) {
      // level with a body: constant-coefficient (z-marching) Jacobi on the plane ranges away from it, the general kernel around it —
      // same ranges as the z-split smoother (the output is a separate array, r is read across the cuts)
      ZPart parts[3]; zsplit_parts(*this, fine, parts);
      for (int i = 0; i < 3; i++) if (parts[i].any()) WL_TRY(wl::jacobi_pp(fine.eps, fine.r, fine.x, fine.L, fine.D, fine.iD, parts[i].of(fine.x_), 1.f, *parts[i].cl, s, xz));
    } else WL_TRY(wl::jacobi_pp(fine.eps, fine.r, fine.x, fine.L, fine.D, fine.iD, fine.x_, 1.f, fine.cl, s, xz));
  }
  std::swap(fine.r, fine.eps);
  return 0;
}
// restrict!(coarse.r, fine.r); fill!(coarse.x,0) :91-92
int wl_mg::restrict_to_coarse(int l, bool to_tail, hipStream_t s) {
  Level& fine = lv[(size_t)l]; Level& coarse = lv[(size_t)l + 1];
  if (coarse.has_view) {
    WL_TRY(wl::restrict_(coarse.r, coarse.view, fine.r, fine.x_, s));
    WL_TRY(wl::allgather_planes(comm, coarse.r, coarse.view, 1, s));
  } else WL_TRY(wl::restrict_(coarse.r, coarse.x_, fine.r, fine.x_, s));
  // the fill! is folded into the coarse level's Jacobi! when that is what touches x next (single-domain level, one-pass Jacobi kernels): that launch writes
  // x = ω·ϵ on the interior and clears x's ghost cells (wl_xzero_ghosts) — every cell, as fill! does, whatever the array held
  coarse.xzero = skip_fill && !to_tail && l + 2 < (int)lv.size() && !perdir && !coarse.dist && !coarse.has_view;
  return coarse.xzero ? 0 : wl::fill(coarse.x, 0.f, (size_t)coarse.x_.cs, s);
}
// "if (coarse is not the coarsest) Vcycle!(coarse); smooth!(coarse)" — as one launch where the levels are small enough — and coarse.x ready for the prolongation
int wl_mg::descend(int l, bool to_tail, float w, hipStream_t s) {
  Level& fine = lv[(size_t)l]; Level& coarse = lv[(size_t)l + 1];
  if (to_tail) WL_TRY(tail(l + 1, w, s));
  else {
    if (l + 2 < (int)lv.size()) WL_TRY(vcycle(l + 1, w, s, true));                         // its last step may be deferred into the smooth! below
    WL_TRY(smooth(l + 1, 4, w, s, false, nullptr, skip_r ? wl::B_XONLY : wl::B_BOTH));     // only coarse.x is read from here on; the next restrict! overwrites coarse.r
  }
  return halo(coarse, coarse.x, 1, s, coarse_x_depth(fine, coarse));
}
// prolongate!(fine.ϵ,coarse.x); increment!(fine;ω): the caller's next operation is smooth!(fine;ω) with the same ω — when that smooth! runs as the temporally
// blocked kernel pair it absorbs this step as an extra pipeline stage (defer).
int wl_mg::prolong(int l, float w, bool defer, hipStream_t s) {
  lv[(size_t)l].pend = true;
  return defer && blocked(lv[(size_t)l]) ? 0 : flush_pending(l, w, s);
}
int wl_mg::vcycle(int l, float w, hipStream_t s, bool defer) {
  WL_TRY(jacobi_fine(l, s));
  {
    ProfScope pc(l == 0 ? WL_PROF_COARSE : -1, s);   // everything below the finest level
    const bool to_tail = tail_ok(l + 1);
    WL_TRY(restrict_to_coarse(l, to_tail, s));
    WL_TRY(descend(l, to_tail, w, s));
  }
  return prolong(l, w, defer, s);
}
// ================================================================================================
// solver!(ml;tol,itmx)                                                                   src/MultiLevelPoisson.jl:108-128
// ================================================================================================
struct wl_mg::SolveRun {
  double hd[WL_RD_COUNT]; float hf[WL_RF_COUNT];      // the last read of the result slots
  double r1tol, rinftol;
  int hit_at;                                          // skip_r: the iteration this slot's last solve stopped at — its r' is not stored
  std::function<int(const float*)> tail; int check_head = 0; bool spec = false;      // the one-shot hooks (wl_mg::Spec) / this iteration's break test ran on the device
  float w = 1.f, r1 = 0.f, rinf = 0.f; int np = 0;
  bool have_r1 = false;                                // r₁ of the initial residual is only needed for the ω rule after the first V-cycle: fetched with the first iteration's norms
  bool converged() const { return (double)r1 < r1tol && (double)rinf < rinftol; }
};
// residual! :93-97.  head_read: the fused projection head's Σr, r₁, r∞ were combined and read by the caller
int wl_mg::initial_residual(int itmx, bool have_residual, bool head_read, hipStream_t s) {
  Level& p = lv[0];
  ProfScope pr(WL_PROF_RESIDUAL, s);
  if (!have_residual) {
    WL_TRY(wl::bc_per_scalar(p.x, p.x_, perdir, s));                                      // residual!: perBC!(x) :93
    WL_TRY(halo(p, p.x, 1, s));
    WL_TRY(wl::residual_part(p.r, p.x, p.z, p.L, p.D, p.iD, p.x_, ws, s));               // r and the local Σr -> WL_RD_SUM
  }
  if (!head_read) WL_TRY(wl::combine_results(comm, ws, s));
  // mean shift + r₁ -> WL_RD_L1_INIT, r∞ -> WL_RF_LINF_INIT — unless the V-cycle's first operation is the z-marching Jacobi! on this level
  // (always run: nᵖ ≥ 1): that kernel applies the shift as it loads r and accumulates the norms, no pass over r at all
  shift_pending = !jacobi0_done && defer_shift && itmx >= 1 && !(comm && comm->size > 1) && !perdir && lv.size() > 1 && wl::jacobi_takes_shift(p.x_, p.cl);
  if (!shift_pending && !jacobi0_done) WL_TRY(wl::shift_norms_dev(p.r, p.x_, ws, WL_RD_L1_INIT, WL_RF_LINF_INIT, s));
  shift_path = jacobi0_done ? 2 : (shift_pending ? 1 : 0);
  return 0;
}
// Vcycle!; smooth!; the norms of the new residual on the host (st.hd, st.hf) — with the projection tail queued behind the device's own break test where one is armed
int wl_mg::iteration(SolveRun& st, hipStream_t s) {
  Level& p = lv[0];
  WL_TRY(settle_r(s));                                                                   // the loop goes on after a skipped store: r' from the r-only instance
  WL_TRY(vcycle(0, st.w, s, true));
  bool nd = false;
  norm_slots = 0;
  WL_TRY(smooth(0, 4, st.w, s, true, &nd, st.np + 1 == st.hit_at ? wl::B_XONLY : wl::B_BOTH));   // fused path: norms come out of kernel B
  if (!nd) { norm_slots = 0; WL_TRY(wl::norms_dev(p.r, p.x_, ws, WL_RD_L1, WL_RF_LINF, s)); }
  WL_TRY(wl::combine_results(comm, ws, s));                                             // (WL_RD_SUM becomes P·Σr: not used again)
  st.spec = (bool)st.tail && norm_slots == 0 && !comm;
  constexpr int nd_read = wl_upto(WL_RD_L1_Z2), nf_read = wl_upto(WL_RF_GO);
  if (!st.spec) return wl::read_results(ws, st.hd, nd_read, st.hf, nf_read, s);
  // the break test on the device, and the projection tail behind it: runs iff this iteration is the last one
  WL_TRY(wl::decide_converged(ws, st.r1tol, st.rinftol, (double)wl_ninside_global(p.g), st.np == 0 ? st.check_head : 0, WL_RD_L1, WL_RF_LINF, WL_RF_GO, s));
  if (!ev_decided) WL_HIP(hipEventCreateWithFlags(&ev_decided, hipEventDisableTiming));
  const float* go = ws.res_f + WL_RF_GO;
  // the copy of the norms sits between the decision and the tail: the host wakes for the copy and goes on queueing work behind the running tail
  return wl::read_results_overlapped(ws, st.hd, nd_read, st.hf, nf_read, s, ev_decided, [&]() -> int { return st.tail(go); });
}
// what solver! does with the norms it read: the log, the ω rule :118-121, nᵖ
void wl_mg::apply_norms(SolveRun& st) {
  if (norm_slots) {   // z-split smoother: one (L₁, L∞) pair per plane range
    double a = 0.0; float m = 0.f;
    for (int i = 0; i < 3; i++) if (norm_slots & (1 << i)) { a += st.hd[WL_ZS_NORMS[i].d]; m = std::fmax(m, st.hf[WL_ZS_NORMS[i].f]); }
    st.hd[WL_RD_L1] = a; st.hf[WL_RF_LINF] = m;
  }
  if (st.np == 0) first_hd0 = st.hd[WL_RD_SUM];
  if (!st.have_r1) { st.r1 = (float)st.hd[WL_RD_L1_INIT]; log_r1.push_back(st.hd[WL_RD_L1_INIT]); log_rinf.push_back(st.hf[WL_RF_LINF_INIT]); log_w.push_back(1.0); st.have_r1 = true; }
  const float rnew = (float)st.hd[WL_RD_L1]; st.rinf = st.hf[WL_RF_LINF]; st.np++;
  log_r1.push_back((double)rnew); log_rinf.push_back((double)st.rinf); log_w.push_back((double)st.w);
  if (rnew >= st.r1) st.w = (float)std::fmax(0.2, 0.9 * (double)st.w);                   // :118-119
  else if (rnew < st.r1) st.w = (float)std::fmin(1.0, 1.02 * (double)st.w);              // :120-121
  st.r1 = rnew;
}
int wl_mg::solve(double tol, int itmx, int* host_n, double* host_r1, float* host_rinf, hipStream_t s, bool have_residual, const double* pre_r1, const float* pre_rinf) {
  Level& p = lv[0];
  r_stale = false;   // r is rebuilt from scratch below, or was by the caller
  SolveRun st;
  st.hit_at = (skip_r && rskip_slot >= 0 && rskip_slot < 2) ? rskip_hist[rskip_slot] : 0;
  st.r1tol = (tol / 10.0) * (double)wl_ninside_global(p.g);                              // l1n_tol  src/Poisson.jl:194
  st.rinftol = tol;
  WL_TRY(initial_residual(itmx, have_residual, jacobi0_done && pre_r1, s));
  log_r1.clear(); log_rinf.clear(); log_w.clear();
  if (jacobi0_done && pre_r1 && pre_rinf) { st.r1 = (float)*pre_r1; log_r1.push_back(*pre_r1); log_rinf.push_back((double)*pre_rinf); log_w.push_back(1.0); st.have_r1 = true; }
  spec.begin_solve(&st.tail, &st.check_head);
  while (st.np < itmx) {
    WL_TRY(iteration(st, s));
    apply_norms(st);
    if (!st.spec) { if (st.converged()) break; continue; }
    // the device's flag IS the decision (the same statements on the same two numbers; with check_head, first the head's mean-shift test — −1: the caller
    // discards this solve, stop here, the tail has not run)
    if (st.check_head && st.np == 1) { spec.head_decided = true; if (st.hf[WL_RF_GO] < 0.f) { spec.head_due = true; break; } }
    if (st.hf[WL_RF_GO] > 0.f) { spec.tail_stood = true; break; }
  }
  WL_TRY(wl::bc_per_scalar(p.x, p.x_, perdir, s));                                        // :126
  WL_TRY(halo(p, p.x, 1, s, x_halo_depth));                                               // projection reads x[I-δz] across the slab face (the next solve's fused head two planes deep)
  n.push_back((int16_t)st.np);
  if (rskip_slot >= 0 && rskip_slot < 2 && !spec.head_due) rskip_hist[rskip_slot] = st.np;   // (a solve the caller discards is nobody's history)
  if (host_n) *host_n = st.np;
  if (host_r1) *host_r1 = (double)st.r1;
  if (host_rinf) *host_rinf = st.rinf;
  return 0;
}
