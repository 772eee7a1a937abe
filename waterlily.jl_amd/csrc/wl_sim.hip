// Simulation/Flow composite handle: mom_step! orchestration (src/Flow.jl:156-237) on one HIP stream and the handle's life cycle, plus the
// TGV / uniform initial conditions.  Bodies: wl_bodyset.hip; observers of a step: wl_observe.hip; exitBC!'s kernels: wl_exit.hip.
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "wl_common.hpp"
#include <algorithm>
#include "wl_mg.hpp"
#include "wl_abwide.hpp"
#include "wl_body.hpp"
#include "wl_pdefer.hpp"
#include "wl_project.hpp"
#include "wl_forces.hpp"
#include "wl_meanflow.hpp"
#include "wl_observe.hpp"
#include "wl_terms.hpp"

namespace {
// apply!(u0,u): u[I,i] = u0(i, loc(i,I))   src/Flow.jl:81-83, loc src/core.jl:177 (Float32)
// kind 1: wall-bounded TGV κ=π/N ; kind 2: periodic TGV κ=2π/N  
template <int D>
__global__ void k_apply_tgv(GridX g, float* __restrict__ u, float kx, float ky, float kz) {
  int i, j; long m; int pz;
  wl_tile(g, m, pz);
  if (!cell_ij(g, m, i, j)) return;
  const int k = pz;
  const long o = m + (long)k * g.sz;
  const int I[3] = {i + 1, j + 1, (D == 3) ? g.gk + k + 1 : 1};
  for (int a = 0; a < D; a++) {
    float x[3];
    for (int c = 0; c < 3; c++) x[c] = (float)I[c] - 1.5f - ((c == a) ? 1.f : 0.f) / 2.f;
    const double X = (double)x[0] * kx, Y = (double)x[1] * ky, Z = (D == 3) ? (double)x[2] * kz : 0.0;
    double v;
    if (a == 0) v = -sin(X) * cos(Y) * ((D == 3) ? cos(Z) : 1.0);
    else if (a == 1) v = cos(X) * sin(Y) * ((D == 3) ? cos(Z) : 1.0);
    else v = 0.0;
    u[(long)a * g.cs + o] = (float)v;
  }
}
template <int D>
__global__ void k_apply_const(GridX g, float* __restrict__ u, float U0, float U1, float U2) {
  int i, j; long m; int pz;
  wl_tile(g, m, pz);
  if (!cell_ij(g, m, i, j)) return;
  const long o = m + (long)pz * g.sz;
  u[o] = U0; u[g.cs + o] = U1; if (D == 3) u[2 * g.cs + o] = U2;
}

// Δt = min(10, 1/(max σ + 5ν))  (src/Flow.jl:166, CFL :234-237) on the device: the statement wl_sim::cfl evaluates on the host from the same maximum
__global__ void k_dt_from_cfl(float* __restrict__ res_f, int in_slot, int out_slot, float nu) { res_f[out_slot] = fminf(10.f, 1.0f / (res_f[in_slot] + 5 * nu)); }
// wl_sim_scratch_fill: `bits` into the interior cells of a dense single-domain array — ghost cells keep what they hold.  One thread per interior cell, by a flat
// index over the interior box; keep: every cell gets back the word it held (the same launch, nothing changes)
__global__ void k_fill_interior_bits(uint32_t* __restrict__ a, int nx, int ny, long sz, int k0, int k1, long n, uint32_t bits, int keep) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int wx = nx - 2, wy = ny - 2;
  const long q = t / wx;
  const int i = 1 + (int)(t - q * wx), j = 1 + (int)(q % wy), k = k0 + (int)(q / wy);
  if (k >= k1) return;
  const long o = i + (long)j * nx + (long)k * sz;
  a[o] = keep ? a[o] : bits;
}
}  // namespace

#define DSEL(D, KERN, ...)                                                           \
  do { if ((D) == 3) hipLaunchKernelGGL(KERN<3>, __VA_ARGS__); else hipLaunchKernelGGL(KERN<2>, __VA_ARGS__); } while (0)

// ================================================================================================
struct wl_sim {
  wl_sim_desc d;
  wl_grid g; GridX G;
  float *u = nullptr, *u0 = nullptr, *f = nullptr, *p = nullptr, *sigma = nullptr, *V = nullptr, *mu0 = nullptr, *mu1 = nullptr;
  float* own = nullptr;
  wl_mg* mg = nullptr;
  wl_comm* comm = nullptr;   // not owned; NULL for a single domain
  bool swap_ok = false;      // u and u⁰ are handle-owned and every ghost of u is rewritten by BC! (no exitBC)
  float* ps = nullptr;       // spare pressure array (out-of-place x·dt and x/dt around the solve; two swaps restore p's identity)
  bool use_fuse_p = true;
  double* exit_sc = nullptr; // exitBC! on slabs: global face means (device)
  bool forcing = false;      // the host supplies g+dU/dt or boundary values for the current step — uniform (acc_uniform) or as separable terms (terms_on()): the staged sequence
  bool acc_uniform = false;  // uniform g(i,t)+dU(i,t)/dt (wl_sim_set_forcing; accelerate!, src/Flow.jl:69-73)
  float acc0[3] = {0, 0, 0}, acc1[3] = {0, 0, 0};   // at t₀ (predictor) and t₁ (corrector)
  float* us = nullptr;       // spare velocity array: the fused corrector writes here, then u and us trade places
  // sgs! as the step's udf (wl_sim_set_sgs; src/Flow.jl:191-193,206-208 with udf=sgs!, src/util.jl:66-76): the model adds to r = conv_diff!'s output, so both
  // phases take the staged sequence conv_diff! -> sgs! -> accelerate! -> BDIM! -> scale_u! -> BC!; everything that assumes the fused conv_diff!+BDIM! launch
  // ran (bcdefer, tailfuse, lazydt, the body hybrid) stands down, as it does for `forcing`
  int sgs_model = 0;         // 0 off, 1 Smagorinsky–Lilly
  float sgs_Cs = 0.f, sgs_Delta = 1.f;
  int sgs_udf(const float* uadv, hipStream_t s) { return sgs_model ? wl::sgs(f, sigma, uadv, G, sgs_Cs, sgs_Delta, s) : 0; }   // udf!(a,sgs!,uadv,t)
  // separable terms (wl_sim_set_terms, wl_terms.hip): uBC(i,x,t) = Σₖ bₖ(t)·Fₖ and g + ∂ₜuBC = Σₖ aₖ(t)·Fₖ with K handle-owned fields of the shape of u and the
  // coefficients the host left in force (wl_sim_set_term_coeffs).  Acceleration coefficients: the staged sequence, like `forcing`; boundary coefficients: every
  // BC!(u) is k_bc_vec_terms and nothing folds or defers it (fold_ok) — the projection tails get no tuple U
  int tK = 0;
  float* tmem = nullptr;                          // K·cs·D floats
  const float* tF[wl::TERMS_MAX] = {nullptr, nullptr, nullptr, nullptr};
  bool t_acc = false, t_bc = false;
  float tacc0[wl::TERMS_MAX] = {0, 0, 0, 0}, tacc1[wl::TERMS_MAX] = {0, 0, 0, 0}, tb1[wl::TERMS_MAX] = {0, 0, 0, 0};   // aₖ(t₀), aₖ(t₁), bₖ(t₁)
  long n_term_accel = 0, n_term_bc = 0;           // launches of the two kernels (wl_sim_counter "term_accel", "term_bc")
  bool terms_on() const { return t_acc || t_bc; }
  void forcing_changed() { forcing = acc_uniform || terms_on(); }      // everything that stands down for `forcing` stands down for terms of either kind
  int accel_terms(const float* c, hipStream_t s) {      // accelerate!(f,t,g,uBC) from the terms, behind the uniform launch
    if (!t_acc) return 0;
    n_term_accel++;
    return wl::accel_terms(f, tK, tF, c, (size_t)G.cs * (size_t)d.D, s);
  }
  int bc_launch(hipStream_t s) {                        // BC!(u,uBC,exitBC,perdir,t₁): the tuple, or the terms with the coefficients in force
    if (t_bc) { n_term_bc++; return wl::bc_vec_terms(u, tK, tF, tb1, G, d.exitBC, d.perdir_mask, s); }
    return wl::bc_vec(u, G, d.uBC, d.exitBC, d.perdir_mask, s);
  }
  bool fused_nobody_conv() const { return us && !d.has_body && !forcing && !sgs_model; }   // predict/correct run conv_diff!+BDIM! as one launch (the NoBody form; `us`: the corrector writes out of place)
  std::vector<float> dt;
  bool own_mg = true;        // false: the multigrid handle belongs to the caller (wl_sim_create_on)
  // WHAT MEMORY DOES NOT HOLD YET (DESIGN.md §4.3b has the same table).  Each field: who sets it -> who consumes it; what makes memory current without it.
  struct Deferred {
    bool u_pending = false;          // bc_u (slabs, "overlap"): an exchange of the array that is now u or u⁰ is in flight -> the first reader of the halo planes; sync_u
    bool bc_deferred = false;        // bc_u_or_defer: BC!(u) after the fused conv launch is not applied -> the fused head / the pair tail put U on load, every tail rewrites the boundary; flush_bc
    bool bc_folded = false;          // a producer with folded stores (wl_bcfold.hpp) wrote every boundary location -> the next bc_u, which then launches nothing; nothing to settle
    const float* proj_pending = nullptr;   // the tail left to the corrector's loader: u still lacks −L∇x of this x -> conv_fused, inside the same step (it fails the step otherwise); never outlives mom_step
    float p_scale_pending = 0.f;     // a tail that skipped its store ("pdefer"): ≠ 0, p holds the solver's scaled x, the pressure is p / p_scale_pending -> the next fused head divides on load; materialise_p
    bool dt_pending = false;         // cfl(more_follow): Δt of the next step is on the device only -> the next mom_step of the same call reads it back behind its predictor; never outlives wl_sim_mom_steps
    bool cfl_done = false;           // the pair tail: max σ is already in WL_RF_CFL -> cfl(), which then launches nothing; nothing to settle
  } df;
  // makes memory current for a reader outside the step (fields handed out, force read-outs, wl_sim_phase, a failed step).  Between calls nothing is pending but, on
  // slabs, the exchange — "a call never returns with the divisor pending", every projection ends with BC! applied — so this launches nothing there.
  int settle(hipStream_t s) { WL_TRY(sync_u(s)); WL_TRY(materialise_p(s)); return flush_bc(s); }
  ~wl_sim() { if (df.u_pending && comm && comm->cs) (void)hipStreamSynchronize(comm->cs); if (own_mg) delete mg; if (own) (void)hipFree(own); if (exit_sc) (void)hipFree(exit_sc); if (farmask) (void)hipFree(farmask); if (mnear) (void)hipFree(mnear); if (mneedf) (void)hipFree(mneedf); if (mm0var) (void)hipFree(mm0var); if (tmem) (void)hipFree(tmem); }

  // BC!(u) on the physical faces this rank holds, then the z-halo planes (depth 2: QUICK reads f[I-2δ], src/Flow.jl:8)
  // On slabs the exchange runs on the communicator's own stream; the compute stream waits for it (sync_u) only where the halo
  // planes are first read, so the interior planes of the next conv_diff! overlap with the transfer.
  bool use_overlap = true;
  int sync_u(hipStream_t s) { if (df.u_pending) { df.u_pending = false; return wl::halo_async_wait(comm, s); } return 0; }
  // BC!(u,U) folded into the stores of the kernel that produced u (wl_bcfold.hpp): single domain, tuple U, no exit, no periodic direction
  // measured at 512³: projection tails −0.04 ms/step (kept), tiled conv_diff! +0.2…0.4 ms/step — the ghost writes are sector-granular
  // wherever they happen, and inside the tiled kernel they sit on the wall tiles' critical path (off; `bcfold` = 3 turns it on)
  int use_bcfold = 1;         // bit 0: projection tails, bit 1: tiled conv_diff!+BDIM!
  bool fold_ok(int bit) const { return (use_bcfold & bit) && !comm && !d.exitBC && !d.perdir_mask && !t_bc && wl_bc_fold_geom_ok(G); }
  int bc_u(hipStream_t s) {
    WL_TRY(sync_u(s));
    if (df.bc_folded) { df.bc_folded = false; return 0; }      // the producer already wrote every boundary location
    WL_TRY(bc_launch(s));
    if (comm && use_overlap) { WL_TRY(wl::halo_async_begin(comm, u, G, d.D, 2, s)); df.u_pending = true; return 0; }
    return wl::halo(comm, u, G, d.D, 2, s);
  }
  // fused conv_diff!+BDIM! (NoBody): interior planes first when the advecting field's halo is still in flight
  bool store_f = false;      // the fused paths materialise the intermediates f = u⁰+Δt·r and z = ∇·u only on request: nothing on the time-step path reads them again
  // want_q1: also leave conv_diff!'s stale Φ in σ's ghost cells (quirk Q1: CFL's maximum(σ) sees them) — one small launch.  The predictor's are dead inside
  // mom_step!: the corrector's conv_diff! overwrites every one of them before anything reads σ's ghost cells.
  int conv_fused(const float* uadv, float* uout, float pre, float post, hipStream_t s, bool want_q1 = true, const float* dt_dev = nullptr) {
    const wl::ConstL& cl = mg->lv[0].cl;
    float* f = store_f ? this->f : nullptr;
    if (df.u_pending && G.D == 3 && G.k1 - G.k0 > 4) {
      if (dt_dev) { wl_set_error("conv_fused: Δt on the device is for the single domain"); return WL_EINVAL; }
      WL_TRY(wl::conv_diff_bdim(f, uadv, sigma, u0, mu0, uout, G, d.nu, d.perdir_mask, d.scheme, dt.back(), pre, post, cl, s, G.k0 + 2, G.k1 - 2, false));
      WL_TRY(sync_u(s));
      WL_TRY(wl::conv_diff_bdim(f, uadv, sigma, u0, mu0, uout, G, d.nu, d.perdir_mask, d.scheme, dt.back(), pre, post, cl, s, -(1 << 30), G.k0 + 2, false));
      return wl::conv_diff_bdim(f, uadv, sigma, u0, mu0, uout, G, d.nu, d.perdir_mask, d.scheme, dt.back(), pre, post, cl, s, G.k1 - 2, 1 << 30, want_q1);
    }
    WL_TRY(sync_u(s));
    BcFold fr{fold_ok(2) ? 1 : 0, {d.uBC[0], d.uBC[1], d.uBC[2]}};
    fr.proj_x = df.proj_pending;
    fr.dt_dev = dt_dev;
    WL_TRY(wl::conv_diff_bdim(f, uadv, sigma, u0, mu0, uout, G, d.nu, d.perdir_mask, d.scheme, dt.back(), pre, post, cl, s, -(1 << 30), 1 << 30, want_q1, &fr));
    if (df.proj_pending && !fr.proj_done) { wl_set_error("mom_step!: the corrector did not take the deferred projection"); return WL_EINVAL; }
    df.proj_pending = nullptr;
    df.bc_folded = fr.on != 0;
    return 0;
  }
  // mom_project!'s first tail deferred into the corrector's conv_diff! (wl_convf.hip, PROJ): the projected predictor velocity has exactly one reader — the
  // corrector — so inside mom_step! the tail's u −= L∇x and the BC! after it are evaluated by that kernel's loader and the field is never written back
  // (−24 B/cell, one launch); p = x/Δt keeps its own small launch.  Only where the loader's closed form is the whole story (fold_ok: single domain, tuple U,
  // no periodic direction, no convective exit) and the corrector is the fused NoBody launch on whole tiles.
  // ON BY DEFAULT on grids of at least `tailfuse_min` interior cells (option "tailfuse", bit-identical): since "pdefer" the predictor's tail launches nothing at
  // all in this form, and with the lean loader (wl_convf.hip: x[k−1] carried from the plane before, x[i−1] from the neighbouring lane, the operands requested
  // at the top of the plane and used behind the x/y fluxes, no spill reload in the loop) the corrector pays 0.19 ms at 512³ for the 0.76 ms tail it replaces
  // (profiles/tailfuse_experiments.md).  Below the gate the separate tail is kept: it can be queued ahead of the solver's convergence read ("tailspec"), which
  // the loader form cannot, and the counters of that speculation are what the small-grid tests pin.
  // An explicit tailfuse = 1 lowers the gate to 0 (the path at any whole-tile size); "tailfuse_min" sets the gate itself.
  static constexpr long TAILFUSE_MIN_DEFAULT = 16L << 20;      // interior cells = 256³: the smallest of 128³ / 256³ / 512³ at which every fused run beat every unfused one (−3.8 %; at 128³ −1 % in the mean, ranges touching)
  bool use_tailfuse = true;
  long tailfuse_min = TAILFUSE_MIN_DEFAULT;
  bool tailfuse_ok() const {
    return use_tailfuse && fold_ok(3) && fused_nobody_conv() && !store_f && !use_convz && !df.u_pending && mg->lv[0].cl.on && !mg->lv[0].part &&
           (long)(G.nx - 2) * (G.ny - 2) * (G.gnz - 2) >= tailfuse_min && wl::conv_proj_ok(G, d.perdir_mask);
  }
  bool use_convz = false;    // z-marching conv_diff! (each flux once): bit-identical but measured 6 % SLOWER than the gather kernel at 512³ (opt-in)
  int conv_only(const float* uadv, hipStream_t s) {     // conv_diff!(f,uadv,σ) without BDIM!
    WL_TRY(sync_u(s));
    if (use_convz && wl::conv_z_ok(G, d.perdir_mask)) {
      WL_TRY(wl::conv_diff_z(f, uadv, nullptr, nullptr, nullptr, G, d.nu, d.scheme, 0.f, 0.f, 1.f, s));
      return wl::conv_q1(sigma, uadv, G, d.nu, d.perdir_mask, d.scheme, s);
    }
    return wl::conv_diff(f, uadv, sigma, G, d.nu, d.perdir_mask, d.scheme, s);
  }
  unsigned char* farmask = nullptr;   // per workgroup of BDIM's u pass: 1 = μ₁ ≡ 0 and V ≡ 0 there (refreshed by measure!/update!)
  bool use_farmask = true, mask_valid = false;   // handing out V or μ₁ (wl_sim_field) invalidates the mask until the next update!
  // body-aware conv_diff!+BDIM! (k_conv_diff<…,FUSE=2>): near / needf masks per (plane, in-plane workgroup)
  unsigned char *mnear = nullptr, *mneedf = nullptr, *mm0var = nullptr;
  int near_box[4] = {0, -1, 0, -1};   // {b0,b1,k0,k1}: bounding box of the near workgroups
  int dirty_z[2] = {0, -1};           // first / last plane with any near / f-keeping / μ₀-loading workgroup (the other planes are NoBody planes)
  bool use_hybrid = true;
  long n_hybrid = 0;                  // predict/correct calls that went through conv_bdim_body
  wl::MaskCensus census;              // what the masks held at the last refresh (read-outs only: wl_sim_counter "mask_*")
  bool hybrid_ok() const { return d.has_body && use_hybrid && mask_valid && mnear && us && !comm && !forcing && !sgs_model && !d.exitBC; }
  int refresh_body_mask(hipStream_t s) {
    if (!d.has_body || !mu1 || !V) return 0;
    if (!farmask) WL_HIP(hipMalloc((void**)&farmask, wl::body_mask_bytes(G)));
    if (!mnear) { const size_t nb = (size_t)wl::body_masks_nbm(G) * (size_t)G.nz; WL_HIP(hipMalloc((void**)&mnear, nb)); WL_HIP(hipMalloc((void**)&mneedf, nb)); WL_HIP(hipMalloc((void**)&mm0var, nb)); }
    mask_valid = true;
    WL_TRY(wl::body_masks(mnear, mneedf, mm0var, V, mu1, mu0, G, s));
    WL_TRY(wl::body_masks_box(mnear, G, near_box, s));
    WL_TRY(wl::body_masks_planes(mnear, mneedf, mm0var, G, dirty_z, s, near_box, &census));
    return wl::body_mask(farmask, V, mu1, G, s);
  }
  // conv_diff!(f,uadv) + BDIM! with a body: fused NoBody form far from the body, two-pass BDIM! on the near workgroups only
  int conv_bdim_body(const float* uadv, float* uout, float pre, float post, hipStream_t s) {
    WL_TRY(sync_u(s));
    n_hybrid++;
    { ProfScope pc(WL_PROF_CONVDIFF, s);
      WL_TRY(wl::conv_diff_bdim_body(f, uadv, sigma, u0, mu0, uout, G, d.nu, d.perdir_mask, d.scheme, dt.back(), pre, post, mnear, mneedf, mm0var, wl::body_masks_nbm(G), store_f ? 1 : 0, s, dirty_z[0], dirty_z[1])); }
    ProfScope pb(WL_PROF_BDIM, s);
    return wl::bdim_near(uout, u, u0, f, V, mu0, mu1, G, dt.back(), pre, post, mnear, wl::body_masks_nbm(G), near_box, s);
  }
  int bdim_step(float pre, float post, hipStream_t s) {
    ProfScope pb(WL_PROF_BDIM, s);
    if (d.has_body) {
      WL_TRY(wl::bdim_f(f, u0, V, G, dt.back(), s));
      if (comm) WL_TRY(wl::halo(comm, f, G, d.D, 1, s));   // μddn reads f[I±δz] across the slab face: exchange f between the two passes
      return wl::bdim_u(u, f, V, mu0, mu1, G, pre, post, s, (use_farmask && mask_valid) ? farmask : nullptr);
    }
    return wl::bdim(u, u0, f, nullptr, mu0, nullptr, G, dt.back(), pre, post, s);
  }
  int exit_bc(hipStream_t s);      // (kernels and the single-domain form: wl_exit.hip)
  int copy_exit_face(float* dst, const float* src, hipStream_t s) { return wl::copy_exit_face(dst, src, G, s); }
  // BC!(u,U) after the fused conv_diff!+BDIM! DEFERRED inside mom_step! (option "bcdefer", df.bc_deferred): until the projection's tail rewrites every boundary
  // location through its folded stores, boundary locations are read only where a component is normal to the face, where BC! writes the constant U — the fused
  // head and the pair tail substitute U on load (wl_resjac_body.inc, k_project_cfl2) and the two k_bc_vec launches per step (2 × 0.07 ms at 512³: strided x
  // faces) disappear.  Every other reader calls flush_bc first.
  bool use_bcdefer = true, in_step = false;
  long n_bcdefer = 0;
  bool head_fused_path() const {    // project() starts with the fused head (wl_resjac.hip): exactly what it tests before it launches wl::resjac
    const wl_mg::Level& l0 = mg->lv[0];
    return ps && use_fuse_p && use_resjac && !resjac_backoff && !d.exitBC && !store_f && !d.perdir_mask && !l0.part && mg->defer_shift && mg->lv.size() > 1 && wl::resjac_ok(G, l0.cl) &&
           (!comm || (l0.dist && mg->x_halo_depth >= 2));   // (exitBC: the convective exit leaves a net flux imbalance to the solver's tolerance — the shift is usually due; z-slab: p's ghost planes are current two deep)
  }
  // … and a deferral (bcdefer, pdefer) may count on it.  !comm: the path allows distributed levels, the deferrals are built for the single domain; an announced
  // forced redo (resjac = 2) is known to end on the two-kernel head, an unannounced one (3) is not — as a real shift is not
  bool head_fused_ok() const { return head_fused_path() && !comm && (!resjac_force_redo || redo_unannounced); }
  bool bcdefer_ok(bool second) const {
    if (!(use_bcdefer && in_step && !df.bc_folded && fold_ok(1) && head_fused_ok())) return false;
    return !second || (use_fuse_cfl && us && wl::tail_caps_cfl(G, mg->lv[0].cl).usub);      // (the corrector's tail must put U on load: wl_project.hpp)
  }
  int bc_u_or_defer(bool second, hipStream_t s) {
    if (bcdefer_ok(second)) { df.bc_deferred = true; n_bcdefer++; return 0; }
    return bc_u(s);
  }
  int flush_bc(hipStream_t s) {       // apply a deferred BC! now (somebody is about to read u's boundary locations from memory)
    if (!df.bc_deferred) return 0;
    df.bc_deferred = false;
    return bc_launch(s);
  }
  int predict(hipStream_t s, const float* dt_dev = nullptr) {                            // mom_predict! src/Flow.jl:190-196 (dt_dev: Δt still on the device — lazydt_ok() paths only)
    if (hybrid_ok()) {
      WL_TRY(conv_bdim_body(u0, u, 0.f, 1.f, s));
      return bc_u(s);
    }
    bool fused_conv = false;
    if (fused_nobody_conv()) {   // conv_diff!(f,u⁰) + BDIM! in one launch (u⁰ is the advecting field, u the output)
      ProfScope pc(WL_PROF_CONVDIFF, s);
      if (use_convz && wl::conv_z_ok(G, d.perdir_mask)) {
        WL_TRY(sync_u(s));
        WL_TRY(wl::conv_diff_z(store_f ? f : nullptr, u0, u0, mu0, u, G, d.nu, d.scheme, dt.back(), 0.f, 1.f, s));
        WL_TRY(wl::conv_q1(sigma, u0, G, d.nu, d.perdir_mask, d.scheme, s));
      } else { WL_TRY(conv_fused(u0, u, 0.f, 1.f, s, !(in_step && !store_f), dt_dev)); fused_conv = true; }
    } else {
      { ProfScope pc(WL_PROF_CONVDIFF, s); WL_TRY(conv_only(u0, s)); }
      WL_TRY(sgs_udf(u0, s));                                                              // udf!(a,udf,a.u⁰,t₀): the model sees u⁰ (a.u is zeroed)
      if (acc_uniform) WL_TRY(wl::accelerate(f, G, acc0, s));                                  // accelerate!(f,t₀,g,uBC)
      WL_TRY(accel_terms(tacc0, s));                                                       // … its position-dependent part
      WL_TRY(bdim_step(0.f, 1.f, s));   // scale_u!(a,0) folded (pre=0)
    }
    WL_TRY(fused_conv ? bc_u_or_defer(false, s) : bc_u(s));      // (deferral implies !exitBC: fold_ok)
    if (d.exitBC) WL_TRY(exit_bc(s));
    return 0;
  }
  int correct(hipStream_t s) {                                                           // mom_correct! :205-210
    if (hybrid_ok()) {
      WL_TRY(conv_bdim_body(u, us, 1.f, 0.5f, s));
      std::swap(u, us);
      return bc_u(s);
    }
    if (fused_nobody_conv()) {   // the advecting field is u itself: write the new u to the spare array and swap
      bool fused_conv = false;
      { ProfScope pc(WL_PROF_CONVDIFF, s);
        if (use_convz && wl::conv_z_ok(G, d.perdir_mask)) {
          WL_TRY(sync_u(s));
          WL_TRY(wl::conv_diff_z(store_f ? f : nullptr, u, u0, mu0, us, G, d.nu, d.scheme, dt.back(), 1.f, 0.5f, s));
          WL_TRY(wl::conv_q1(sigma, u, G, d.nu, d.perdir_mask, d.scheme, s));
        } else { WL_TRY(conv_fused(u, us, 1.f, 0.5f, s)); fused_conv = true; } }
      std::swap(u, us);
      if (d.exitBC) WL_TRY(copy_exit_face(u, us, s));   // BC!(…,saveexit) keeps the predictor's exit face
      return fused_conv ? bc_u_or_defer(true, s) : bc_u(s);
    }
    { ProfScope pc(WL_PROF_CONVDIFF, s); WL_TRY(conv_only(u, s)); }
    WL_TRY(sgs_udf(u, s));                                                                 // udf!(a,udf,a.u,t): the model sees the projected u
    if (acc_uniform) WL_TRY(wl::accelerate(f, G, acc1, s));                                    // accelerate!(f,t₁,g,uBC)
    WL_TRY(accel_terms(tacc1, s));
    WL_TRY(bdim_step(1.f, 0.5f, s));  // scale_u!(a,0.5) folded (post)
    return bc_u(s);
  }
  int itmx = 32;             // solver!'s iteration cap (src/MultiLevelPoisson.jl:108); the multi-GPU rehearsal (tools/slab_rank_bench.py) lowers it to the 1 V-cycle the real run takes
  bool use_resjac = true;    // projection head + first Jacobi! in one launch (wl_resjac.hip) where eligible
  bool use_headspec = true;  // … and the first V-cycle queued behind it without waiting for Σr (single GPU)
  bool resjac_force_redo = false;   // test hook: behave as if the mean shift were always due (exercises the redo path; with the tail armed, k_decide declares it)
  bool redo_unannounced = false;    // test hook: … and do not let the BC! deferral know in advance (as with a real shift)
  long n_tailfuse = 0;       // projections whose velocity update ran inside the corrector's conv_diff!
  long n_resjac = 0, n_resjac_redo = 0;   // how often the fused head stood / had to be redone because the mean shift was due
  int resjac_redo_run = 0;                // consecutive redos: after WL_RESJAC_BACKOFF of them the fused head is switched off for this handle
  bool resjac_backoff = false;            // (a flow whose residual needs the mean shift on every solve would pay launch + sync + two-kernel path each time); re-armed by update!
  int p_shell = -1;          // ghost shell of p / the spare pressure array: -1 unknown (check before the next fused head), 0 all +0, 1 something else, 2 caller-owned p (never assumed)
  bool use_fuse_cfl = true;  // the corrector's projection tail also produces CFL's σ and max(σ)
  bool use_tailspec = true;  // the projection tail is queued behind the smoother before the host has read the norms, gated on the device by the break test (single GPU)
  long n_tailspec = 0, n_tailspec_armed = 0;   // projection tails that ran gated / solves the gated tail was armed for (the difference: withheld — capped, or the head redone)
  // p = x/Δt NOT STORED between the solves of a time step (option "pdefer", wl_pdefer.hpp, df.p_scale_pending).  The unscaled pressure a projection tail writes has
  // one reader inside mom_step! / wl_sim_mom_steps — the next projection's head, which multiplies it by its own Δt — so where that head is known to be the fused one
  // the tail skips the store (4 of its 32 B/cell) and leaves the divisor; the head divides on load (same two roundings: same bits).  Every other reader calls
  // materialise_p first.  skip_p_now() says which tails qualify; the last tail of a call always stores, so a call never returns with the divisor pending.
  // Pointer parity: every head and every STORING tail calls swap_p(); a skipped store is a skipped swap_p(), and materialise_p is that store and swap made late.
  // Handle-owned p: wl_sim_field("p") reports whichever array holds the pressure — a single step with one skipped store makes three swaps and ends on the other
  // array, a K-step call makes 2K + 1.  Caller-owned p (p_home): the results must land in the caller's array, so the LAST step's first tail skips only if that
  // leaves an even number of swaps to go (the solver's x is then p_home itself); in a multi-step call this gives 2(K−1) skipped stores, in a single step none.
  // Should a redo in that last step break the parity after all, mom_step copies the pressure home (one D2D copy, mean-shift flows on caller-owned arrays only).
  bool use_pdefer = true;
  long n_pdefer = 0;             // tails that skipped the store
  float* p_home = nullptr;       // caller-owned p
  // the projection tails with four cells per thread and 16-byte accesses (option "tailwide", k_project_wide in wl_project.hip): the same statements per cell, the
  // same launches; taken where the launchers find that the shape and the arrays allow it (they report it: TailRep::wide), everything else runs the one- and two-cell kernels
  bool use_tailwide = true;
  long n_tailwide = 0;           // tails that ran in that form
  // not fused_nobody_conv(): nothing between a tail and the next head goes through the spare velocity array, so `us` is not asked for
  bool pdefer_ok() const { return use_pdefer && in_step && !sgs_model && !forcing && !d.has_body && head_fused_ok(); }   // (head_fused_ok: no slab, store_f, exitBC, periodic direction, body, back-off)
  void swap_p() { std::swap(p, ps); mg->lv[0].x = p; }      // the pressure pair trades places: `p` is always the array the solver and the next reader take
  int materialise_p(hipStream_t s) {
    if (df.p_scale_pending == 0.f) return 0;
    WL_TRY(wl::div_scalar_to(ps, p, std::exchange(df.p_scale_pending, 0.f), (size_t)G.cs, s));
    swap_p();
    return 0;
  }
  // ---- mom_project! :223-232 in stages: head -> solve -> tail -> finish.  Who calls, by name:
  struct ProjCall {
    float w; bool with_cfl, corrector_follows, step_follows;      // Δt weight; the tail also produces CFL's maximum; inside mom_step!, the corrector reads u next; another step of the same call does
    static ProjCall step_first(bool more_follow) { return {1.f, false, true, more_follow}; }
    static ProjCall step_second(bool more_follow) { return {0.5f, true, false, more_follow}; }
    static ProjCall bare(float w) { return {w, false, false, false}; }                    // wl_sim_phase 2 and 4: CFL is a phase of its own, every tail is launched and stores
    static ProjCall score(float w, bool with_cfl) { return {w, with_cfl, false, false}; }    // placement trials: outside in_step, counters reset afterwards
  };
  struct ZSplit { bool on; int na, nb; };      // a body: the plane range [na, nb) around it takes the general-coefficient kernels, the ranges below and above the constant-coefficient ones (as in smooth!)
  ZSplit zsplit() const {
    const wl_mg::ZRanges z = mg->zsplit_ranges(mg->lv[0]);      // the smoother's ranges; a slab handle runs the whole-level forms
    return {z.on && !comm, z.na, z.nb};
  }
  // the tail's form, decided once per projection (before the head: it reads df.bc_deferred as the head will find it)
  //   PairCfl        u −= L∇x, flux_out and its maximum into the spare velocity array (the pair kernels; with a body: their z-split form)
  //   InPlace        u −= L∇x and p = x/Δt in place
  //   SplitInPlace   the same on the three plane ranges of a body
  //   Loader         left to the corrector's loader ("tailfuse"): at most p = x/Δt is launched here
  enum class Tail { PairCfl, InPlace, SplitInPlace, Loader };
  // caps: what the launcher of the form can do on this level (wl_project.hpp; nothing for the split forms and the loader); gateable: the tail may be queued ahead
  // of the solver's convergence read behind a device flag `go` ("tailspec")
  struct TailPlan { Tail form; ZSplit z; wl::TailCaps caps; bool gateable; };
  struct TailDone { wl::TailRep rep; bool skips_p = false; };      // what the launch did: the launcher's report (folded stores, four cells per thread) / left p = x/Δt to the next fused head
  bool pair_tail_cfl(bool with_cfl) const { return with_cfl && use_fuse_cfl && us && !d.exitBC && !d.perdir_mask; }
  TailPlan plan_tail(const ProjCall& c) const {
    TailPlan t; t.z = zsplit();
    t.form = pair_tail_cfl(c.with_cfl) ? Tail::PairCfl : t.z.on ? Tail::SplitInPlace : (c.corrector_follows && tailfuse_ok()) ? Tail::Loader : Tail::InPlace;
    t.caps = t.form == Tail::InPlace ? wl::tail_caps_inplace(G, mg->lv[0].cl) : (t.form == Tail::PairCfl && !t.z.on) ? wl::tail_caps_cfl(G, mg->lv[0].cl) : wl::TailCaps{};
    t.gateable = t.caps.gate && (t.form == Tail::InPlace || !df.bc_deferred || takes_deferred_bc(t));
    return t;
  }
  bool takes_deferred_bc(const TailPlan& t) const { return fold_ok(1) && t.caps.usub; }      // the corrector's tail reads u as the deferred BC! would have left it; otherwise flush_bc comes first
  bool skip_p_now(const ProjCall& c) const {      // decided per launch: a back-off during the head withdraws it
    if (!pdefer_ok()) return false;
    if (c.with_cfl) return c.step_follows && !obs.reads_p_after_this_step();   // the corrector's tail: the next reader is the next step's head — unless an observer of this step reads p first
    return c.corrector_follows && (!p_home || c.step_follows || p == p_home);   // the predictor's tail: the corrector's head (caller-owned p, last step of the call: see the parity rule above)
  }
  // go != nullptr: queued inside the solver loop ahead of its read — runs iff the flag says "converged"; a gated tail that was withheld is launched again with go = nullptr.
  // (p is the solver's x by now, ps the array the unscaled pressure goes to: every head has called swap_p())
  int launch_tail(const TailPlan& plan, const ProjCall& c, float dtl, const float* go, TailDone* done, hipStream_t s) {
    const wl_mg::Level& l0 = mg->lv[0];
    *done = TailDone{};
    wl::TailReq rq; rq.U = fold_ok(1) ? d.uBC : nullptr; rq.go = go; rq.wide = use_tailwide;
    switch (plan.form) {
      case Tail::PairCfl:
        if (plan.z.on) { WL_TRY(flush_bc(s)); WL_TRY(wl::project_cfl_split(us, u, mu0, p, ps, sigma, G, dtl, l0.cl, l0.clp, plan.z.na, plan.z.nb, mg->ws, WL_RF_CFL, s, store_f ? 1 : 0)); break; }
        if (df.bc_deferred && !takes_deferred_bc(plan)) WL_TRY(flush_bc(s));
        rq.usub = df.bc_deferred;      // flux_out reads the wall-normal boundary faces of the corrector's output: U on load
        rq.skip_p = done->skips_p = plan.caps.skip_p && skip_p_now(c);
        WL_TRY(wl::project_cfl(us, u, mu0, p, ps, sigma, G, dtl, l0.cl, mg->ws, WL_RF_CFL, s, store_f ? 1 : 0, rq, &done->rep)); df.bc_folded = done->rep.folded;
        break;
      case Tail::SplitInPlace: WL_TRY(wl::project_unscale_split(u, mu0, p, ps, G, dtl, l0.cl, l0.clp, plan.z.na, plan.z.nb, s)); break;
      case Tail::Loader:        // (with the store skipped this tail launches nothing at all: the corrector's head takes x with the pending divisor)
        done->skips_p = skip_p_now(c);
        if (!done->skips_p) WL_TRY(wl::div_scalar_to(ps, p, dtl, (size_t)G.cs, s));
        break;
      case Tail::InPlace:
        rq.skip_p = done->skips_p = plan.caps.skip_p && skip_p_now(c);
        WL_TRY(wl::project_unscale(u, mu0, p, ps, G, dtl, l0.cl, s, rq, &done->rep)); df.bc_folded = done->rep.folded;
        break;
    }
    return 0;
  }
  // what a head leaves for project(): the fused results stand / its solve too / and the gated tail behind it ran; the norms a read-back brought;
  // taken: the fused head's outputs are the solver's x and r at the moment (a speculative solve runs, or ran, on them)
  struct Head { bool stood = false, solved = false, tail_ran = false, taken = false; double pre_r1 = 0.0; float pre_rinf = 0.f; };
  void head_swap() { swap_p(); std::swap(mg->lv[0].r, mg->lv[0].eps); }      // x·Δt in the spare pressure array, r in ϵ's <-> the solver's x and r: undoes itself
  void head_take(Head* h) { head_swap(); mg->jacobi0_done = h->taken = true; }
  void head_accept(Head* h) {      // no mean shift (src/Poisson.jl:96): the fused results stand — and the head took a pending divisor on load
    if (!h->taken) head_take(h);
    n_resjac++; resjac_redo_run = 0; h->stood = true; df.p_scale_pending = 0.f;
  }
  void head_discard(Head* h) {     // the shift was due: the head's inputs are untouched, the two-kernel head follows; a speculative solve is forgotten
    if (h->taken) { head_swap(); mg->jacobi0_done = h->taken = false; mg->n.pop_back(); }
    n_resjac_redo++;
    if (!resjac_force_redo && ++resjac_redo_run >= 3) resjac_backoff = true;
  }
  // solver! runs its V-cycle at least once whatever the initial norms are (src/MultiLevelPoisson.jl:113-123), so Σr is not needed before the first cycle is
  // queued: the cycle is launched behind the head at once and Σr comes back with the first iteration's norms (one host round trip per solve fewer, no idle
  // GPU while the host decides).  If the shift turns out to be due, that solve is discarded.
  int head_speculate(const ProjCall& c, float dtl, const TailPlan& plan, TailDone* done, Head* h, hipStream_t s) {
    head_take(h);
    // armed: the device decides whether the head stands (k_decide: −1 = shift due; the resjac=2/3 hook declares it due there too), the host reads that flag
    struct SpecClear { wl_mg* m; ~SpecClear() { m->spec.disarm(); } } spec_clear{mg};   // the hook captures this frame: never outlives it
    if (use_tailspec && plan.gateable) {
      mg->spec.tail = [&, dtl, done, s](const float* go) { return launch_tail(plan, c, dtl, go, done, s); };
      mg->spec.check_head = resjac_force_redo ? 2 : 1; n_tailspec_armed++;
    }
    const int slot = mg->rskip_slot, hist = slot >= 0 ? mg->rskip_hist[slot] : 0;
    WL_TRY(mg->solve(2e-3, itmx, nullptr, nullptr, nullptr, s, true, nullptr, nullptr));
    h->tail_ran = mg->spec.tail_stood; if (h->tail_ran) n_tailspec++;
    const bool due = mg->spec.head_decided ? mg->spec.head_due : (resjac_force_redo || wl_shift_due(mg->first_hd0, (double)wl_ninside_global(mg->lv[0].g)));
    if (due) { head_discard(h); if (slot >= 0) mg->rskip_hist[slot] = hist; }      // (a discarded solve is nobody's "rskip" history)
    else { head_accept(h); h->solved = true; }
    return 0;
  }
  int head_read_back(Head* h, hipStream_t s) {
    WL_TRY(wl::combine_results(comm, mg->ws, s));            // z-slabs: Σr, L₁ (sums) and L∞ (max) over the ranks — every rank takes the same branch below
    double hd[WL_RD_COUNT]; float hf[WL_RF_COUNT]; WL_TRY(wl::read_results(mg->ws, hd, wl_upto(WL_RD_L1_INIT), hf, wl_upto(WL_RF_LINF_INIT), s));
    h->pre_r1 = hd[WL_RD_L1_INIT]; h->pre_rinf = hf[WL_RF_LINF_INIT];
    if (!wl_shift_due(hd[WL_RD_SUM], (double)wl_ninside_global(mg->lv[0].g)) && !resjac_force_redo) head_accept(h);
    else head_discard(h);
    return 0;
  }
  // head + the V-cycle's first Jacobi!(fine) in one launch, assuming residual!'s mean shift is not due (wl_resjac.hip); Σr decides
  int head_fused(const ProjCall& c, float dtl, const TailPlan& plan, TailDone* done, Head* h, hipStream_t s) {
    { ProfScope pr(WL_PROF_RESIDUAL, s);
      // p's and the spare's ghost cells are +0 unless someone wrote them from outside (checked once after a pointer to p was handed out): no shell pass then
      if (comm) p_shell = 1;   // (a slab's ghost planes hold the neighbours' pressure: always scaled with the rest)
      if (p_shell < 0) p_shell = (wl::shell_nonzero(p, G, (int*)(mg->ws.res_f + WL_RF_IFLAG), s) || wl::shell_nonzero(ps, G, (int*)(mg->ws.res_f + WL_RF_IFLAG), s)) ? 1 : 0;
      WL_TRY(wl::resjac(ps, mg->lv[0].eps, p, u, G, dtl, 1.f, mg->lv[0].cl, mg->ws, WL_RD_L1_INIT, WL_RF_LINF_INIT, s, p_shell != 0, df.bc_deferred ? d.uBC : nullptr, df.p_scale_pending)); }
    return use_headspec && !comm && itmx >= 1 ? head_speculate(c, dtl, plan, done, h, s) : head_read_back(h, s);
  }
  // z=div(u); x.*=dt; residual! — the scaled pressure goes to the spare array, which becomes p.  After a discarded solve p is the scaled x again, untouched: the head only read it
  int head_two_kernel(float dtl, hipStream_t s) {
    wl_mg::Level& l0 = mg->lv[0];
    WL_TRY(settle(s));            // reads p as the unscaled pressure and u's boundary faces from memory
    { ProfScope pr(WL_PROF_RESIDUAL, s);
      const ZSplit z = zsplit();
      if (z.on) WL_TRY(wl::div_residual_split(store_f ? sigma : nullptr, ps, l0.r, p, u, mu0, l0.D, l0.iD, G, dtl, mg->ws, l0.cl, l0.clp, z.na, z.nb, s));
      else WL_TRY(wl::div_residual(store_f ? sigma : nullptr, ps, l0.r, p, u, mu0, l0.D, l0.iD, G, dtl, mg->ws, l0.cl, s)); }
    swap_p();
    return 0;
  }
  int project_finish(const TailPlan& plan, const TailDone& done, float dtl, hipStream_t s) {
    df.bc_deferred = false;     // every form leaves the boundary current: folded stores, the bc_u below, or the corrector's loader, which reads u through the projection AND BC!
    if (plan.form == Tail::Loader) { df.proj_pending = p; n_tailfuse++; }      // (the scaled x stays untouched in what is the spare pressure array from here on)
    if (plan.form == Tail::PairCfl) {
      WL_TRY(wl::combine_results(comm, mg->ws, s));   // max over ranks — issued BEFORE the u exchange starts on the other stream, so that
      std::swap(u, us); df.cfl_done = true;           // exchange stays in flight across the Δt read-back and the next predictor's interior
    }
    if (done.rep.wide) n_tailwide++;
    if (done.skips_p) { df.p_scale_pending = dtl; n_pdefer++; }      // p stays the solver's x; no store, no swap
    else swap_p();
    return plan.form == Tail::Loader ? 0 : bc_u(s);
  }
  int project_plain(float dtl, hipStream_t s) {      // no spare pressure array, or fuse_p = 0: the reference's statements one by one
    WL_TRY(settle(s));             // (guard: nothing defers on a handle that takes this path)
    WL_TRY(wl::div_scale(sigma, p, u, G, dtl, s));                                       // z=div(u); x.*=dt
    WL_TRY(mg->solve(2e-3, itmx, nullptr, nullptr, nullptr, s));
    WL_TRY(wl::project(u, mu0, p, G, s));
    WL_TRY(wl::div_scalar(p, dtl, (size_t)G.cs, s));                                     // x./=dt
    return bc_u(s);
  }
  int project(const ProjCall& c, hipStream_t s) {
    const float dtl = c.w * dt.back();
    // "rskip": the solves of this projection keep their own history of where they stopped — the predictor's (Δt weight 1) and the corrector's (½) differ
    struct RSlot { wl_mg* m; ~RSlot() { m->rskip_slot = -1; } } rslot{mg};
    mg->rskip_slot = c.w == 1.f ? 0 : 1;
    df.cfl_done = false;
    if (df.p_scale_pending != 0.f && !head_fused_ok()) WL_TRY(materialise_p(s));          // (the fused head was switched off since the tail ran: back-off, an option)
    WL_TRY(sync_u(s));                                                                     // div(u) reads the halo planes
    if (df.bc_deferred && !head_fused_ok()) WL_TRY(flush_bc(s));                           // (cannot happen: the deferral tested the same condition — kept as the invariant's guard)
    if (!ps || !use_fuse_p || (comm && d.perdir_mask)) return project_plain(dtl, s);      // (z-slabs: p's ghost planes are current — exchanged at the end of the last solve, scaled with the rest)
    WL_TRY(wl::bc_per_scalar(p, G, d.perdir_mask, s));                                     // residual!: perBC!(x) :93 (copies commute with the scaling)
    const TailPlan plan = plan_tail(c);
    TailDone done; Head h;
    if (head_fused_path()) WL_TRY(head_fused(c, dtl, plan, &done, &h, s));
    if (!h.stood) WL_TRY(head_two_kernel(dtl, s));
    if (!h.solved) WL_TRY(mg->solve(2e-3, itmx, nullptr, nullptr, nullptr, s, true, h.stood ? &h.pre_r1 : nullptr, h.stood ? &h.pre_rinf : nullptr));
    if (!h.tail_ran) WL_TRY(launch_tail(plan, c, dtl, nullptr, &done, s));      // u -= L∇x ; x./=dt — the unscaled pressure goes back to the original array
    return project_finish(plan, done, dtl, s);
  }
  // Δt of the NEXT step left on the device (wl_sim_mom_steps only: more steps follow inside the same call, nobody can look at the history in between): the finaliser
  // of CFL's maximum is followed by a one-thread kernel with mom_step!'s formula, the next predictor reads Δt through a pointer and is queued at once; the host
  // copies the maximum while that predictor runs and appends the same Δt to the history (same statements on the same number: same bits).
  bool use_lazydt = true;
  hipEvent_t ev_dt = nullptr;
  bool lazydt_ok() const {      // the next predictor will be the flux-once tiled launch on the single domain
    return use_lazydt && in_step && !comm && fused_nobody_conv() && !use_convz && !d.exitBC && !d.perdir_mask && !store_f && wl::conv_flux_on() &&
           wl::conv_tile_ok(G, d.perdir_mask, G.k1 - G.k0) && mg->lv[0].cl.on;
  }
  int cfl(hipStream_t s, bool more_follow = false) {                                     // CFL :234-237
    if (!df.cfl_done) { WL_TRY(sync_u(s)); WL_TRY(wl::cfl_dev(u, sigma, G, mg->ws, WL_RF_CFL, s)); WL_TRY(wl::combine_results(comm, mg->ws, s)); }   // max over ranks
    df.cfl_done = false;
    if (more_follow && lazydt_ok()) {
      hipLaunchKernelGGL(k_dt_from_cfl, dim3(1), dim3(1), 0, s, mg->ws.res_f, WL_RF_CFL, WL_RF_DT, d.nu);
      df.dt_pending = true;
      return 0;
    }
    float hf[WL_RF_COUNT]; WL_TRY(wl::read_results(mg->ws, nullptr, 0, hf, wl_upto(WL_RF_CFL), s)); const float mx = hf[WL_RF_CFL];
    dt.push_back(std::fmin(10.f, 1.0f / (mx + 5 * d.nu)));
    return 0;
  }
  // ---- observers of a completed step (wl_observe.hpp): probe and force records, tracers, the mean flow.  One member; the step asks it one question (skip_p_now)
  // and calls it once, after the second projection and before CFL
  wl::Observers obs;
  long n_step_launches = 0;                            // kernel launches of this handle's mom_step! calls (wl_sim_counter "launches")
  wl::StepView view() const { return {G, d.D, u, u0, p, d.nu, dt, d.perdir_mask}; }      // (the roles rotate: taken where it is used)
  int observe(hipStream_t s) {      // dt.back() is still the Δt this step ran with: cfl appends the next one afterwards
    if (obs.reads_p_after_this_step()) WL_TRY(materialise_p(s));     // (guard: skip_p_now keeps the corrector's tail storing on such a step)
    return obs.after_step(view(), s);
  }
  int mom_step(hipStream_t s, bool more_follow = false) {
    WL_TRY(obs.before_step(d.D));
    const long l0 = g_wl_launches;
    const int rc = mom_step_body(s, more_follow);
    n_step_launches += g_wl_launches - l0;
    // A failed step leaves nothing pending for the next call to take.  BC! of a u nobody can use is dropped, not launched.
    // The divisor is applied: pdefer is single-domain, so settle's slab wait, the only step before it, does nothing there.
    // On slabs that wait (no launch) lets the exchange finish before its flag goes; the rest of the record is cleared.
    if (rc != 0) { df.bc_deferred = false; (void)settle(s); df = Deferred{}; return rc; }
    if (!more_follow && p_home && p != p_home) {      // caller-owned p that ended on the spare array (a redo inside the last step): copy it home
      WL_HIP(hipMemcpyAsync(p_home, p, sizeof(float) * (size_t)G.cs, hipMemcpyDeviceToDevice, s));
      swap_p();      // (the pair is {p_home, spare}: ps was p_home)
    }
    return rc;
  }
  int mom_step_body(hipStream_t s, bool more_follow) {                                   // mom_step! :156-167 (more_follow: wl_sim_mom_steps — another step comes inside the same call)
    ProfScope pstep(WL_PROF_STEP, s);
    // u⁰ .= u ; scale_u!(a,0): when the handle owns both arrays the copy is a pointer swap — the predictor overwrites
    // every interior cell of u (BDIM! with pre=0) and BC! every ghost cell, so nothing of the old u survives anyway.
    if (swap_ok) { std::swap(u, u0); if (d.exitBC) WL_TRY(copy_exit_face(u, u0, s)); }   // (an exchange still in flight belongs to the array that is now u⁰ — the predictor's advecting field)
    else { WL_TRY(sync_u(s)); WL_HIP(hipMemcpyAsync(u0, u, sizeof(float) * (size_t)G.cs * d.D, hipMemcpyDeviceToDevice, s)); }   // u⁰ .= u
    struct InStep { bool& f; InStep(bool& b) : f(b) { f = true; } ~InStep() { f = false; } } guard(in_step);
    if (df.dt_pending) {   // the CFL maximum of the previous step is copied back between ITS finaliser and THIS predictor, which takes Δt from the device
      if (!ev_dt) WL_HIP(hipEventCreateWithFlags(&ev_dt, hipEventDisableTiming));
      double hd[WL_RD_COUNT]; float hf[WL_RF_COUNT];
      WL_TRY(wl::read_results_overlapped(mg->ws, hd, wl_upto(WL_RD_SUM), hf, wl_upto(WL_RF_DT), s, ev_dt, [&]() -> int { return predict(s, mg->ws.res_f + WL_RF_DT); }));
      dt.push_back(std::fmin(10.f, 1.0f / (hf[WL_RF_CFL] + 5 * d.nu)));
      df.dt_pending = false;
    } else
    WL_TRY(predict(s));
    WL_TRY(project(ProjCall::step_first(more_follow), s));
    WL_TRY(correct(s));
    WL_TRY(project(ProjCall::step_second(more_follow), s));
    WL_TRY(observe(s));      // u and p are final; ahead of the CFL reduction
    return cfl(s, more_follow);
  }
};
int wl_sim::exit_bc(hipStream_t s) {
  if (comm) {   // z-slabs: the exit face is shared by all ranks — global means from per-rank sums (one 128-byte all-gather each)
    if (!exit_sc) WL_HIP(hipMalloc((void**)&exit_sc, 2 * sizeof(double)));
    WL_TRY(sync_u(s));
    double* sum = mg->ws.res_d + WL_RD_EXIT;
    for (int mode = 0; mode < 2; mode++) {
      WL_TRY(wl::exit_bc_slab_sum(G, u, sum, mode, s));
      WL_TRY(wl::combine_results(comm, mg->ws, s));
      WL_TRY(wl::exit_bc_slab_update(G, u, u0, sum, exit_sc, dt.back(), mode, s));
    }
    return wl::halo(comm, u, G, d.D, 2, s);      // the exit face changed after BC!'s exchange
  }
  return wl::exit_bc_single(G, u, u0, mg->ws.res_d + WL_RD_EXIT, dt.back(), s);
}
extern "C" {

static int sim_create_common(wl_sim** out, const wl_sim_desc* desc, wl_comm* comm, wl_mg* adopt = nullptr) {
  WL_CHECK(out && desc, "null pointer"); WL_CHECK(desc->D == 2 || desc->D == 3, "D must be 2 or 3");
  WL_TRY(wl_ctx_ensure());
  const bool slab = comm && comm->size > 1;
  wl_sim* s = new wl_sim(); s->d = *desc; s->comm = slab ? comm : nullptr;
  if (slab && desc->D == 3 && ((desc->perdir_mask >> 2) & 1u)) comm->zperiodic = true;      // the halo exchanges wrap around (rank 0 <-> rank size-1)
  int32_t ng[3] = {desc->dims[0] + 2, desc->dims[1] + 2, desc->D == 3 ? desc->dims[2] + 2 : 1};
  if (slab) {
    if (desc->u || desc->u0 || desc->f || desc->p || desc->sigma || desc->V || desc->mu0 || desc->mu1) { delete s; wl_set_error("slab simulations own their arrays"); return WL_EINVAL; }
    static const int ghost = [] { const char* e = getenv("WL_SLAB_GHOST"); const int v = e ? atoi(e) : 5; return v >= 3 ? v : 5; }();
    const int rc = wl_grid_slab(&s->g, desc->D, ng, comm->rank, comm->size, ghost);   // ghost planes: QUICK needs 2, kernel B of the blocked smoother 3, the one-exchange smooth! 5
    if (rc != 0) { delete s; return rc; }
  } else s->g = wl_grid_single(desc->D, ng);
  s->G = gx(s->g);
  const size_t nc = (size_t)s->G.cs; const int D = desc->D;
  float** ptrs[8] = {&s->u, &s->u0, &s->f, &s->p, &s->sigma, &s->V, &s->mu0, &s->mu1};
  float* given[8] = {desc->u, desc->u0, desc->f, desc->p, desc->sigma, desc->V, desc->mu0, desc->mu1};
  const size_t sz[8] = {nc * D, nc * D, nc * D, nc, nc, nc * D, nc * D, nc * D * D};
  size_t total = 0;
  const bool none = !desc->u && !desc->u0, all3 = desc->u && desc->u0 && desc->us;
  const bool rot_ok = !desc->exitBC || !slab;               // convective exit: the buffers rotate on a single domain only (the exit face travels with the role, k_copy_exit_face)
  const bool want_us = none && !desc->us && rot_ok;         // spare velocity array of the out-of-place fused kernels (handle-owned)
  if (want_us) total += nc * D;
  total += nc;   // ps
  for (int q = 0; q < 8; q++) if (!given[q] && !(q == 7 && !desc->has_body) && !(q == 5 && !desc->has_body)) total += sz[q];
  if (total) { hipError_t e = hipMalloc((void**)&s->own, total * sizeof(float)); if (e != hipSuccess) { delete s; wl_set_error("hipMalloc failed for flow arrays"); return (int)e; } (void)hipMemset(s->own, 0, total * sizeof(float)); }
  float* pcur = s->own;
  for (int q = 0; q < 8; q++) {
    if (given[q]) *ptrs[q] = given[q];
    else if ((q == 7 || q == 5) && !desc->has_body) *ptrs[q] = nullptr;
    else { *ptrs[q] = pcur; pcur += sz[q]; }
  }
  if (want_us) { s->us = pcur; pcur += nc * D; }
  else if (desc->us && (none || all3) && rot_ok) s->us = desc->us;   // caller-owned spare: the roles of {u,u0,us} rotate (wlhip.h)
  s->ps = pcur; pcur += nc;
  s->dt.assign(1, desc->dt0);
  if (desc->p) s->p_home = desc->p;
  if (desc->p) s->p_shell = 2;     // a caller-owned p can be written behind the library's back: its ghost shell is always scaled
  s->swap_ok = (none || all3) && rot_ok;
  // μ₀ = 1 with BC!(μ₀,0)   src/Flow.jl:144-145  (only when the handle owns μ₀; a caller-owned μ₀ is taken as is)
  if (!desc->mu0) {
    int rc = wl::fill(s->mu0, 1.f, nc * D, 0); const float zero[3] = {0, 0, 0};
    if (rc == 0) rc = wl::bc_vec(s->mu0, s->G, zero, 0, desc->perdir_mask, 0);
    if (rc == 0) rc = wl::halo(s->comm, s->mu0, s->G, D, 2, 0);
    if (rc != 0) { delete s; return rc; }
  }
  if (adopt) {   // the caller's MultiLevelPoisson (wl_mg_create on the same p, μ₀, σ): used, not owned
    if (slab || adopt->lv.empty() || adopt->lv[0].x != s->p || adopt->lv[0].L != s->mu0 || adopt->lv[0].z != s->sigma) {
      delete s; *out = nullptr; wl_set_error("wl_sim_create_on: the wl_mg handle was not built on this flow's p, mu0, sigma"); return WL_EINVAL;
    }
    if (adopt->perdir != desc->perdir_mask) {   // the hierarchy's perBC! pattern is fixed at wl_mg_create: it has to be the flow's
      delete s; *out = nullptr; wl_set_error("wl_sim_create_on: the wl_mg handle was created with a different perdir mask than desc->perdir_mask"); return WL_EINVAL;
    }
    s->mg = adopt; s->own_mg = false;
  } else {
    s->mg = new wl_mg();
    int rc = s->mg->build(s->p, s->mu0, s->sigma, s->g, desc->perdir_mask, 10, s->comm);   // pois_ctor default  src/WaterLily.jl:97
    if (rc != 0) { delete s; *out = nullptr; return rc; }
  }
  s->mg->store_eps = false;   // p.ϵ is pure scratch on the time-step path
  s->mg->skip_r = true;       // … and so is the residual a solve ends on, and every coarse level's (option "rskip")
  if (slab && s->G.k0 >= 2 && s->G.nz - s->G.k1 >= 2) s->mg->x_halo_depth = 2;   // z-slab: the fused projection head recomputes the residual of the neighbour's boundary plane (x two planes deep)
  *out = s; return 0;
}
// Placement trials.  Where the driver puts a multi-GB allocation decides what the z-marching kernels get out of HBM: the same binary ran the
// finest-level smoother kernels 7–12 % and the fused projection head 9 % slower on one allocation than on the next (one process, simulations created
// one after the other: profiles/r03_placement_trial.txt; a plain z-marching copy: 3.6 vs 4.7 TB/s, profiles/r03_place_probe2.txt) — element-wise
// kernels do not care.  A handle that owns all its arrays therefore creates up to `trials` candidates (each in new memory: the others are held meanwhile),
// times mom_project! once on each (zero fields: every kernel of the projection runs, nothing changes) and keeps the fastest.  Results are placement-
// independent; only large grids take part (small ones live in the caches).
// OFF by default (WL_PLACEMENT_TRIALS=1; set it to 2…8 to try): six default bench runs with 6 candidates against six without (profiles/r03_bench_distribution.txt) —
// mean step 9.88 vs 9.89 ms, the smoother pair in its fast state in 2 of 6 vs 3 of 6 runs.  Candidates allocated after the first one are rarely in the fast state,
// so holding memory to force new placements buys almost nothing; the finding (placement decides 7–12 % of the pair) stands, the remedy does not work.
static double placement_score(wl_sim* s) {
  hipStream_t q = 0;
  const size_t n0 = s->mg->n.size();
  if (s->project(wl_sim::ProjCall::score(1.f, false), q) != 0) return 1e30;            // warm-up (first-launch costs)
  if (hipStreamSynchronize(q) != hipSuccess) return 1e30;
  hipEvent_t a, b; if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return 1e30;
  float ms = 1e30f; int rc = 0;
  for (int rep = 0; rep < 2 && rc == 0; rep++) {        // the faster of two timed pairs (each holds host read-backs of the solver)
    (void)hipEventRecord(a, q);
    rc = s->project(wl_sim::ProjCall::score(1.f, false), q); if (rc == 0) rc = s->project(wl_sim::ProjCall::score(0.5f, true), q);
    (void)hipEventRecord(b, q); (void)hipEventSynchronize(b);
    float t = 1e30f; (void)hipEventElapsedTime(&t, a, b);
    if (t < ms) ms = t;
  }
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  // back to the state of a fresh handle: pois.n, counters, Δt untouched by mom_project!; u, p are still zero (BC! wrote the boundary values the
  // initial condition / init_flow will write again)
  s->mg->n.resize(n0); s->n_resjac = 0; s->n_resjac_redo = 0; s->resjac_redo_run = 0; s->resjac_backoff = false; s->df.cfl_done = false;
  s->mg->log_r1.clear(); s->mg->log_rinf.clear(); s->mg->log_w.clear();
  s->mg->rskip_hist[0] = s->mg->rskip_hist[1] = 0; s->mg->n_rskip = s->mg->n_rskip_redo = 0;
  return rc == 0 ? (double)ms : 1e30;
}
static double g_last_placement[8]; static int g_last_placement_n = 0;
int wl_sim_create(wl_sim** out, const wl_sim_desc* desc) {
  WL_CHECK(out && desc, "null pointer");
  static const int trials_env = [] { const char* e = getenv("WL_PLACEMENT_TRIALS"); const int v = e ? atoi(e) : 1; return v < 1 ? 1 : (v > 8 ? 8 : v); }();
  const bool owned = !desc->u && !desc->u0 && !desc->f && !desc->p && !desc->sigma && !desc->V && !desc->mu0 && !desc->mu1 && !desc->us;
  const long cells = (long)desc->dims[0] * desc->dims[1] * (desc->D == 3 ? desc->dims[2] : 1);
  int trials = (owned && desc->D == 3 && cells >= (48L << 20)) ? trials_env : 1;      // (≥ 48 Mi cells: the arrays are far larger than the Infinity Cache)
  if (trials > 1) {   // all candidates are alive until the choice is made: never take more than half of the free memory for them (≈160 B per cell and candidate)
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) { const long fit = (long)(fr / 2 / ((size_t)cells * 160 + 1)); if (fit < trials) trials = fit < 1 ? 1 : (int)fit; }
  }
  g_last_placement_n = 0;
  if (trials == 1) return sim_create_common(out, desc, nullptr);
  wl_sim* cand[8] = {nullptr}; double score[8]; int best = -1;
  for (int i = 0; i < trials; i++) {
    const int rc = sim_create_common(&cand[i], desc, nullptr);
    if (rc != 0) { cand[i] = nullptr; if (best < 0 && i == trials - 1) return rc; break; }      // (out of memory for another candidate: go with what exists)
    score[i] = placement_score(cand[i]);
    g_last_placement[g_last_placement_n++] = score[i];
    if (best < 0 || score[i] < score[best]) best = i;
  }
  if (best < 0) return WL_EINVAL;
  for (int i = 0; i < trials; i++) if (cand[i] && i != best) delete cand[i];
  *out = cand[best];
  return 0;
}
// scores (ms of the timed mom_project! pair) of the candidates of the last wl_sim_create: measurement interface
int wl_placement_scores(double* out, int cap) { int k = 0; for (; k < g_last_placement_n && k < cap; k++) out[k] = g_last_placement[k]; return g_last_placement_n; }
int wl_sim_create_on(wl_sim** out, const wl_sim_desc* desc, wl_mg* mg) { WL_CHECK(mg, "null wl_mg"); return sim_create_common(out, desc, nullptr, mg); }
int wl_sim_create_slab(wl_sim** out, const wl_sim_desc* desc, wl_comm* comm) { return sim_create_common(out, desc, comm); }
int wl_sim_destroy(wl_sim* s) { delete s; return 0; }
float* wl_sim_field(wl_sim* s, const char* name) {
  const std::string n(name);
  (void)s->settle(0);        // the caller is about to read or write the arrays: finish an exchange that is still in flight (the rest is a guard: nothing else is pending between calls)
  if (n == "V" || n == "mu1" || n == "mu0") s->mask_valid = false;
  if (n == "u") return s->u; if (n == "u0") return s->u0; if (n == "f") return s->f; if (n == "p") { if (s->p_shell != 2) s->p_shell = -1; return s->p; }
  if (n == "sigma") return s->sigma; if (n == "V") return s->V; if (n == "mu0") return s->mu0; if (n == "mu1") return s->mu1;
  if (n == "us") return s->us;
  return nullptr;
}
wl_mg* wl_sim_pois(wl_sim* s) { return s->mg; }
// ---- wl_sim_scratch_fill / wl_sim_scratch_keep (wlhip_bench.h): a word into everything the handle and its wl_mg own that no public call reaches and that is dead
// between public calls.  Not on the step path.  write = false: the same settling and the same launches, every word stays
static long scratch_fill(wl_sim* s, uint32_t bits, uint32_t regions, bool write, hipStream_t q) {
  if (!s || s->comm) { wl_set_error("wl_sim_scratch_fill: single-domain handles only"); return -1; }
  if (s->settle(q) != 0 || s->mg->settle_r(q) != 0) return -1;      // nothing pending: p is the pressure, the finest r is stored (the r-only launch reads em, rs, W)
  long words = 0;
  auto whole = [&](void* a, size_t n) -> int {
    words += (long)n;
    if (write && n) WL_HIP(hipMemsetD32Async((hipDeviceptr_t)a, (int)bits, n, q));
    return 0;
  };
  auto interior = [&](float* a, const GridX& g) -> int {
    const int k0 = g.D == 3 ? 1 : 0, k1 = g.D == 3 ? g.nz - 1 : 1;
    const long n = (long)(g.nx - 2) * (g.ny - 2) * (k1 - k0);
    if (!a || n <= 0) return 0;
    words += n;
    hipLaunchKernelGGL(k_fill_interior_bits, dim3((unsigned)((n + WL_BLOCK - 1) / WL_BLOCK)), dim3(WL_BLOCK), 0, q, (uint32_t*)a, g.nx, g.ny, g.sz, k0, k1, n, bits, write ? 0 : 1);
    WL_LAUNCH_CHECK(); return 0;
  };
  // the pressure pair: p lives in one array, the other one is rewritten by the next head or tail — its ghost cells too, so what is known of the shell is forgotten
  if (regions & 1u) { if (whole(s->ps, (size_t)s->G.cs) != 0) return -1; if (s->p_shell != 2) s->p_shell = -1; }
  for (wl_mg::Level& v : s->mg->lv) {
    if ((regions & 2u) && (interior(v.em, v.x_) != 0 || interior(v.rs, v.x_) != 0)) return -1;      // ϵ_mid and r′ of the blocked smoother (their ghost cells stay zero: kernel B reads them)
    if ((regions & 4u) && v.wx && v.g.D == 3) {      // W: the interior rows of an interior plane are contiguous — whole segments, the padding slots included
      const size_t row = wl::abw_pitch(v.g.nx) / sizeof(float), n = (size_t)(v.g.ny - 2) * row;
      for (int k = 1; k < v.g.nz - 1; k++) if (whole(v.wx + ((size_t)k * v.g.ny + 1) * row, n) != 0) return -1;
    }
  }
  // the per-block partials of the reduction workspace (two double arrays and one float array of WL_MAXPART entries): every reduction writes the partials it reads;
  // the 16 result slots behind them keep their values
  if ((regions & 8u) && whole(s->mg->ws.pa, (size_t)WL_MAXPART * 5) != 0) return -1;
  // the observers' staging: the partial sums of the force bands (12 doubles per tile of their capacity, written by every run before its finish reads them)
  if (regions & 16u) for (wl::ForceBand* b : {&s->obs.fband, &s->obs.fimm}) if (b->part && whole(b->part, (size_t)b->part_cap * 24) != 0) return -1;
  if (words > 0x7fffffffL) { wl_set_error("wl_sim_scratch_fill: more than 2^31 words"); return -1; }
  return words;
}
int wl_sim_scratch_fill(wl_sim* s, uint32_t bits, void* st) { return (int)scratch_fill(s, bits, ~0u, true, wl_stream(st)); }
int wl_sim_scratch_fill_regions(wl_sim* s, uint32_t bits, uint32_t regions, void* st) { return (int)scratch_fill(s, bits, regions, true, wl_stream(st)); }
int wl_sim_scratch_keep(wl_sim* s, void* st) { return (int)scratch_fill(s, 0u, ~0u, false, wl_stream(st)); }
int wl_sim_grid(const wl_sim* s, wl_grid* out) { *out = s->g; return 0; }
int wl_sim_init_flow(wl_sim* s, void* st) {                                               // Flow ctor :141-142
  hipStream_t q = wl_stream(st);
  WL_TRY(s->bc_u(q));
  if (s->d.exitBC) {   // exitBC!(u,u,zero(T)): u⁰ aliases u, Δt = 0
    const float keep = s->dt.back(); float* keep0 = s->u0;
    s->dt.back() = 0.f; s->u0 = s->u;
    const int rc = s->exit_bc(q);
    s->dt.back() = keep; s->u0 = keep0;
    if (rc != 0) return rc;
  }
  WL_HIP(hipMemcpyAsync(s->u0, s->u, sizeof(float) * (size_t)s->G.cs * s->d.D, hipMemcpyDeviceToDevice, q));
  return 0;
}
int wl_sim_set_option(wl_sim* s, const char* name, int value) {
  const std::string n(name);
  if (n == "convz") { s->use_convz = value != 0; return 0; }
  if (n == "fused_smoother") { s->mg->use_fused = value != 0; return 0; }
  if (n == "store_eps") { s->mg->store_eps = value != 0; return 0; }
  if (n == "constl") { s->mg->use_constl = value != 0; return s->mg->update(0); }
  if (n == "tail") { s->mg->use_tail = value != 0; return 0; }
  if (n == "tail_lds") { wl::tail_lds_enable(value); return 0; }
  if (n == "xdefer") { s->mg->use_xdefer = value != 0; s->mg->use_wide = value == 1; return 0; }   // 1: … and kernel A hands r′ and ϵ_mid to kernel B through the level's exchange buffer where eligible; 2: deferred x with the two dense arrays
  if (n == "overlap_smooth") { s->mg->overlap_smooth = value != 0; return 0; }
  if (n == "body_tile") { wl::conv_body_tile_enable(value); return 0; }
  if (n == "skip_fill") { s->mg->skip_fill = value != 0; return 0; }
  if (n == "defer_shift") { s->mg->defer_shift = value != 0; return 0; }
  if (n == "zsplit") {   // 0 off, 1 default size gate, 2 levels of any size, v >= 4: levels of at least v·2^20 cells (takes effect at the next update!)
    s->mg->use_zsplit = value != 0; s->mg->zsplit_min = value == 2 ? 0 : (value >= 4 ? (long)value << 20 : 16L << 20); return 0;
  }
  if (n == "hybrid") { s->use_hybrid = value != 0; return 0; }
  if (n == "farmask") { s->use_farmask = value != 0; return 0; }
  if (n == "store_f") { s->store_f = value != 0; return 0; }
  if (n == "overlap") { WL_TRY(s->sync_u(0)); s->use_overlap = value != 0; return 0; }
  if (n == "fuse_cfl") { s->use_fuse_cfl = value != 0; return 0; }
  if (n == "jacobi_march") { wl::jacobi_march_enable(value); return 0; }
  if (n == "convm") { wl::conv_march_enable(value); return 0; }
  if (n == "deep_halo") { s->mg->deep_halo = value != 0; return 0; }
  if (n == "x_halo") { if (value < 1 || value > s->G.k0) { wl_set_error("x_halo: 1 .. ghost depth of the slab"); return WL_EINVAL; } s->mg->x_halo_depth = value; return 0; }   // 1: the fused head stays off on z-slabs
  if (n == "bcfold") { s->use_bcfold = value; return 0; }   // bit 0: projection tails, bit 1: tiled conv_diff!+BDIM!
  if (n == "resjac") { s->use_resjac = value != 0; s->resjac_force_redo = value == 2 || value == 3; s->redo_unannounced = value == 3; return 0; }   // 2: always take the redo path (tests); 3: the same, unknown to the BC! deferral (tests: its flush before the two-kernel head)
  if (n == "resjac_min") { wl::resjac_enable(1, value); return 0; }                            // cells threshold of the fused head (tests: 0)
  if (n == "convt_min") { wl::conv_tile_min(value); return 0; }                               // tile-planes threshold of the tiled conv_diff! (tests: 0)
  if (n == "lazydt") { s->use_lazydt = value != 0; return 0; }                                 // wl_sim_mom_steps: between its steps Δt stays on the device until the next predictor is queued (default 1)
  if (n == "tailspec") { s->use_tailspec = value != 0; return 0; }                             // the projection tail is queued ahead of the solver's convergence read, gated by the device's break test (default 1)
  if (n == "headspec") { s->use_headspec = value != 0; return 0; }                             // the first V-cycle is queued behind the fused head before Σr is known (default 1)
  if (n == "bcdefer") { s->use_bcdefer = value != 0; return 0; }                               // mom_step!: BC! after the fused conv_diff!+BDIM! left to the projection (its head reads U on the wall-normal faces, its tail rewrites the boundary); default 1
  if (n == "pdefer") { s->use_pdefer = value != 0; return 0; }                                 // mom_step!: a projection tail whose p = x/Δt is read next by a fused head of the same call does not store it (default 1)
  if (n == "rskip") { WL_TRY(s->mg->settle_r_for_reader()); s->mg->skip_r = value != 0; return 0; }      // smoother kernel B does not store the residual nobody reads: every coarse level's, and the finest level's in the iteration the slot's last solve stopped at (default 1); 0: every store
  if (n == "tailwide") { s->use_tailwide = value != 0; return 0; }                             // the projection tails with four cells per thread and 16-byte accesses where the shape allows (default 1); 0: the one- and two-cell kernels
  if (n == "tailfuse") { s->use_tailfuse = value != 0; if (value != 0) s->tailfuse_min = 0; return 0; }   // mom_step!: the first projection's u −= L∇x + BC! inside the corrector's conv_diff! (default 1 on grids of at least "tailfuse_min" cells; an explicit 1 also drops that gate)
  if (n == "tailfuse_min") { if (value < 0) { wl_set_error("tailfuse_min: interior cells, >= 0"); return WL_EINVAL; } s->tailfuse_min = value; return 0; }   // interior-cells gate of "tailfuse" (default 16 Mi = 256³; tests: 0 or a small whole-tile shape)
  if (n == "convf") { wl::conv_flux_enable(value != 0); return 0; }                            // 1: tiled conv_diff! evaluates every flux once (default), 0: k_conv_tile
  if (n == "convt") { wl::conv_tile_enable(value != 0, value > 1 ? value : 0); return 0; }   // 0 off, 1 on, >1: on with that z-chunk
  if (n == "pair") { wl::gsrb_pair_enable(value); return 0; }
  if (n == "fuse_p") { s->use_fuse_p = value != 0; return 0; }
  if (n == "zsplit_par") { s->mg->par_ranges = value != 0; return 0; }
  if (n == "itmx") { if (value < 1) { wl_set_error("itmx must be >= 1"); return WL_EINVAL; } s->itmx = value; return 0; }
  wl_set_error("unknown option " + n); return WL_EINVAL;
}
int wl_sim_update(wl_sim* s, void* st) { s->resjac_backoff = false; s->resjac_redo_run = 0; WL_TRY(s->refresh_body_mask(wl_stream(st))); return s->mg->update(wl_stream(st)); }

long wl_launch_count(void) { return g_wl_launches; }
// the size gates and kernel-family switches that wl_sim_set_option / wl_mg_set_fused keep PROCESS-wide (they select code, not results): back to the defaults
int wl_reset_process_options(void) {
  wl::resjac_enable(1, 6L << 20); wl::conv_tile_min(2048); wl::conv_tile_enable(1, 0); wl::conv_flux_enable(1); wl::tail_lds_enable(1); wl::conv_body_tile_enable(1);
  wl::gsrb_pair_enable(1); wl::jacobi_march_enable(1); wl::conv_march_enable(0);
  return 0;
}
int wl_sim_counter(wl_sim* s, const char* name, long* out) {
  WL_CHECK(s && name && out, "bad argument");
  const std::string n(name);
  if (n == "resjac") { *out = s->n_resjac; return 0; }
  if (n == "resjac_redo") { *out = s->n_resjac_redo; return 0; }
  if (n == "resjac_backoff") { *out = s->resjac_backoff ? 1 : 0; return 0; }
  if (n == "tailfuse") { *out = s->n_tailfuse; return 0; }
  if (n == "tailfuse_min") { *out = s->tailfuse_min; return 0; }      // (the gate in force, not a count: the per-handle options have no other read-out)
  if (n == "bcdefer") { *out = s->n_bcdefer; return 0; }
  if (n == "pdefer") { *out = s->n_pdefer; return 0; }
  if (n == "tailwide") { *out = s->n_tailwide; return 0; }
  if (n == "rskip") { *out = s->mg->n_rskip; return 0; }
  if (n == "rskip_redo") { *out = s->mg->n_rskip_redo; return 0; }
  if (n == "tailspec") { *out = s->n_tailspec; return 0; }
  if (n == "tailspec_armed") { *out = s->n_tailspec_armed; return 0; }
  if (n == "xdefer") { *out = s->mg->last_xdefer; return 0; }
  if (n == "abwide") { *out = s->mg->n_wide; return 0; }                          // finest-level smooth! calls whose r′ and ϵ_mid went through the exchange buffer W
  // which body-aware path ran, and what the masks held at the last refresh (measure!/update!)
  if (n == "hybrid") { *out = s->n_hybrid; return 0; }
  if (n == "body_tile") { *out = wl::conv_body_tile_launches(); return 0; }      // (process-wide, like the switch: read it as a difference)
  if (n == "mask_valid") { *out = s->mask_valid ? 1 : 0; return 0; }
  if (n == "mask_near") { *out = s->census.near; return 0; }
  if (n == "mask_needf_only") { *out = s->census.needf_only; return 0; }
  if (n == "mask_m0var_only") { *out = s->census.m0var_only; return 0; }
  if (n == "mask_clean_in_box") { *out = s->census.clean_in_box; return 0; }
  if (n == "dirty_z0") { *out = s->dirty_z[0]; return 0; }
  if (n == "dirty_z1") { *out = s->dirty_z[1]; return 0; }
  if (n == "near_b0") { *out = s->near_box[0]; return 0; }
  if (n == "near_b1") { *out = s->near_box[1]; return 0; }
  if (n == "near_k0") { *out = s->near_box[2]; return 0; }
  if (n == "near_k1") { *out = s->near_box[3]; return 0; }
  if (n == "part") { *out = s->mg->lv[0].part ? 1 : 0; return 0; }                 // the finest level's z-split: decided / planes [za, zb] off the constant pattern
  if (n == "part_za") { *out = s->mg->lv[0].za; return 0; }
  if (n == "part_zb") { *out = s->mg->lv[0].zb; return 0; }
  if (n == "term_accel") { *out = s->n_term_accel; return 0; }                     // launches of k_accel_terms / k_bc_vec_terms by this handle (wl_sim_set_terms)
  if (n == "term_bc") { *out = s->n_term_bc; return 0; }
  if (n == "launches") { *out = s->n_step_launches; return 0; }                    // kernel launches of this handle's mom_step! calls so far
  if (n == "probe_records") { *out = s->obs.probes.n; return 0; }                       // probe records held / refused by a full buffer
  if (n == "probe_dropped") { *out = s->obs.probes.dropped; return 0; }
  if (n == "force_records") { *out = s->obs.forces.n; return 0; }                       // force records held / refused by a full buffer / active tiles of the list in use
  if (n == "force_dropped") { *out = s->obs.forces.dropped; return 0; }
  if (n == "mean_updates") { *out = s->obs.n_mean_updates; return 0; }                 // updates of the mean-flow observer since wl_sim_set_meanflow / its period (0: off)
  if (n == "mean_every") { *out = s->obs.mean_mode ? s->obs.mean_every : 0; return 0; }
  if (n == "force_tiles") { *out = s->obs.force_on ? s->obs.fband.n_active : s->obs.fimm.n_active; return 0; }
  wl_set_error("unknown counter " + n); return WL_EINVAL;
}
int wl_sim_set_forcing(wl_sim* s, const float* U1, const float* a0, const float* a1) {
  const int D = s->d.D;
  if (U1) for (int c = 0; c < D; c++) s->d.uBC[c] = U1[c];
  s->acc_uniform = a0 != nullptr || a1 != nullptr; s->forcing_changed();
  for (int c = 0; c < 3; c++) { s->acc0[c] = (a0 && c < D) ? a0[c] : 0.f; s->acc1[c] = (a1 && c < D) ? a1[c] : 0.f; }
  return 0;
}
// separable terms (wlhip.h): every refusal is decided on the host, before any launch or allocation
int wl_sim_set_terms(wl_sim* s, int K, const float* const* host_F, void* st) {
  WL_CHECK(s, "null wl_sim");
  if (s->comm) { wl_set_error("wl_sim_set_terms: z-slab handles are not supported (single domain only)"); return WL_EINVAL; }
  if (K < 0 || K > wl::TERMS_MAX) { wl_set_error("wl_sim_set_terms: K outside 0 ... 4"); return WL_EINVAL; }
  const size_t n = (size_t)s->G.cs * (size_t)s->d.D;
  if (K > 0) {
    if (!host_F) { wl_set_error("wl_sim_set_terms: a NULL field"); return WL_EINVAL; }
    for (int k = 0; k < K; k++) {
      if (!host_F[k]) { wl_set_error("wl_sim_set_terms: a NULL field"); return WL_EINVAL; }
      for (size_t q = 0; q < n; q++) if (!std::isfinite(host_F[k][q])) { wl_set_error("wl_sim_set_terms: a non-finite value in a field"); return WL_EINVAL; }
    }
  }
  hipStream_t q = wl_stream(st);
  WL_TRY(s->settle(q));
  if (s->tmem) { WL_HIP(hipStreamSynchronize(q)); WL_HIP(hipFree(s->tmem)); s->tmem = nullptr; }      // (hipFree waits for every stream that may still read the old fields)
  s->tK = 0; s->t_acc = s->t_bc = false; s->forcing_changed();
  for (int k = 0; k < wl::TERMS_MAX; k++) { s->tF[k] = nullptr; s->tacc0[k] = s->tacc1[k] = s->tb1[k] = 0.f; }
  if (K == 0) return 0;
  WL_HIP(hipMalloc((void**)&s->tmem, sizeof(float) * n * (size_t)K));
  for (int k = 0; k < K; k++) {
    s->tF[k] = s->tmem + n * (size_t)k;
    WL_HIP(hipMemcpyAsync(s->tmem + n * (size_t)k, host_F[k], sizeof(float) * n, hipMemcpyHostToDevice, q));
  }
  WL_HIP(hipStreamSynchronize(q));      // the host arrays are the caller's again
  s->tK = K;
  return 0;
}
float* wl_sim_term(wl_sim* s, int k) { return (s && k >= 0 && k < s->tK) ? s->tmem + (size_t)s->G.cs * (size_t)s->d.D * (size_t)k : nullptr; }
int wl_sim_set_term_coeffs(wl_sim* s, const float* acc0, const float* acc1, const float* bc1) {
  WL_CHECK(s, "null wl_sim");
  if (s->comm) { wl_set_error("wl_sim_set_term_coeffs: z-slab handles are not supported (single domain only)"); return WL_EINVAL; }
  if (s->tK == 0 && (acc0 || acc1 || bc1)) { wl_set_error("wl_sim_set_term_coeffs: coefficients given while K = 0 (wl_sim_set_terms)"); return WL_EINVAL; }
  for (const float* c : {acc0, acc1, bc1}) if (c) for (int k = 0; k < s->tK; k++) if (!std::isfinite(c[k])) { wl_set_error("wl_sim_set_term_coeffs: a non-finite coefficient"); return WL_EINVAL; }
  s->t_acc = acc0 != nullptr || acc1 != nullptr;
  s->t_bc = bc1 != nullptr; s->forcing_changed();
  for (int k = 0; k < wl::TERMS_MAX; k++) {
    s->tacc0[k] = (acc0 && k < s->tK) ? acc0[k] : 0.f; s->tacc1[k] = (acc1 && k < s->tK) ? acc1[k] : 0.f; s->tb1[k] = (bc1 && k < s->tK) ? bc1[k] : 0.f;
  }
  return 0;
}
int wl_sim_set_sgs(wl_sim* s, int model, float Cs, float Delta) {
  WL_CHECK(s, "null wl_sim"); WL_CHECK(model == 0 || model == 1, "wl_sim_set_sgs: model must be 0 (off) or 1 (Smagorinsky-Lilly)");
  if (model) {
    if (s->d.D != 3) { wl_set_error("wl_sim_set_sgs: the Smagorinsky model is built for 3-D flows only"); return WL_EINVAL; }
    if (s->comm) { wl_set_error("wl_sim_set_sgs: z-slab handles are not supported (single domain only)"); return WL_EINVAL; }
  }
  s->sgs_model = model; s->sgs_Cs = Cs; s->sgs_Delta = Delta;
  return 0;
}
int wl_sim_mom_step(wl_sim* s, void* st) { return s->mom_step(wl_stream(st)); }
int wl_sim_mom_steps(wl_sim* s, int n, void* st) {
  WL_CHECK(s && n >= 0, "bad argument");
  for (int k = 0; k < n; k++) WL_TRY(s->mom_step(wl_stream(st), k + 1 < n));
  return 0;
}
int wl_sim_dt(const wl_sim* s, float* out, int cap) { const int n = (int)s->dt.size(); for (int k = 0; k < n && k < cap; k++) out[k] = s->dt[(size_t)k]; return n; }
float wl_sim_dt_last(const wl_sim* s) { return s->dt.back(); }
int wl_sim_set_dt_last(wl_sim* s, float dt) { WL_CHECK(s && dt > 0.f, "bad Δt"); s->dt.back() = dt; return 0; }
double wl_sim_time(const wl_sim* s) { float t = 0.f; for (size_t k = 0; k + 1 < s->dt.size(); k++) t += s->dt[k]; return (double)t; }
int wl_sim_phase(wl_sim* s, int phase, void* st) {
  hipStream_t q = wl_stream(st);
  // settle() without its sync_u: the phases wait for an exchange where they first read the halo planes (the slab predictor overlaps its interior with it)
  WL_TRY(s->materialise_p(q));      // (guards, as in wl_sim_field)
  WL_TRY(s->flush_bc(q));
  switch (phase) {
    case 0: WL_TRY(s->sync_u(q)); WL_HIP(hipMemcpyAsync(s->u0, s->u, sizeof(float) * (size_t)s->G.cs * s->d.D, hipMemcpyDeviceToDevice, q)); return wl::scale_u(s->u, s->G, 0.f, q);
    case 1: return s->predict(q);
    case 2: return s->project(wl_sim::ProjCall::bare(1.f), q);
    case 3: return s->correct(q);
    case 4: return s->project(wl_sim::ProjCall::bare(0.5f), q);
    case 5: return s->cfl(q);
  }
  wl_set_error("bad phase"); return WL_EINVAL;
}
int wl_sim_apply_ic(wl_sim* s, int kind, void* st) {
  hipStream_t q = wl_stream(st); const GridX& G = s->G; const int D = s->d.D;
  if (kind == 0) { DSEL(D, k_apply_const, wl_plane_grid(G, G.nz), dim3(WL_BLOCK), 0, q, G, s->u, s->d.uBC[0], s->d.uBC[1], s->d.uBC[2]); }
  else {
    const float two = (kind == 2) ? 2.f : 1.f;
    const float kx = two * 3.14159265358979323846f / (float)s->d.dims[0], ky = two * 3.14159265358979323846f / (float)s->d.dims[1];
    const float kz = (D == 3) ? two * 3.14159265358979323846f / (float)s->d.dims[2] : 0.f;
    DSEL(D, k_apply_tgv, wl_plane_grid(G, G.nz), dim3(WL_BLOCK), 0, q, G, s->u, kx, ky, kz);
  }
  WL_LAUNCH_CHECK(); return 0;
}
static wl_body sphere_body(const float* c, float R) {
  wl_body b{}; b.kind = WL_BODY_SPHERE; b.R = R;
  for (int q = 0; q < 3; q++) { b.c[q] = c[q]; b.m[q] = 1.f; }
  return b;
}
// measure!(sim) of the body program P: the fields, their halos, the masks, the force recorder's band, update!(pois)   src/Body.jl:28-51, WaterLily.jl:148
static int sim_measure(wl_sim* s, const SetArg& P, float eps, void* st) {
  hipStream_t q = wl_stream(st); const GridX& G = s->G; const int D = s->d.D;
  WL_TRY(wl::bodyset_measure_fields(s->sigma, s->mu0, s->mu1, s->V, G, P, eps, s->d.exitBC, s->d.perdir_mask, q));
  WL_TRY(wl::halo(s->comm, s->mu0, G, D, 2, q)); WL_TRY(wl::halo(s->comm, s->V, G, D, 2, q));
  WL_TRY(s->refresh_body_mask(q));
  WL_TRY(s->obs.body_changed(G, P, q));
  return s->mg->update(q);
}
// the handle's p (which = 0) or u (1) on the body program P; x0: the moment about that point.  Float64 partial sums, flow.f untouched; on z-slabs every rank
// sums its own planes and the per-rank sums are added on device
static int sim_force(int which, wl_sim* s, const float* x0, const SetArg& P, double* out, void* st) {
  hipStream_t q = wl_stream(st);
  WL_TRY(wl::bodyset_lattice_margin(P, 2.f, "force"));
  WL_TRY(s->settle(q));                              // (∂u/∂z at the slab faces reads the neighbours' planes)
  const float* a = which == 0 ? s->p : s->u; const float nu = which == 0 ? 0.f : s->d.nu; const GridX& G = s->G;
  return wl::force_reduce_with(G, s->mg->ws, s->comm, out, q,
                               [&](dim3 grid, double* part, hipStream_t qq) { return wl::bodyset_force_partials(which, a, nu, G, P, x0, grid, part, qq); });
}
static int sim_force_body(int which, wl_sim* s, const float* x0, const wl_body* body, double* out, void* st) {
  SetArg P; WL_TRY(wl::bodyset_from_body(s->d.D, body, &P));
  return sim_force(which, s, x0, P, out, st);
}
int wl_sim_pressure_moment_body(wl_sim* s, const float* x0, const wl_body* body, double* out, void* st) { WL_CHECK(x0, "null x0"); return sim_force_body(0, s, x0, body, out, st); }
int wl_sim_viscous_moment_body(wl_sim* s, const float* x0, const wl_body* body, double* out, void* st) { WL_CHECK(x0, "null x0"); return sim_force_body(1, s, x0, body, out, st); }
int wl_sim_measure_body(wl_sim* s, const wl_body* body, float eps, void* st) {
  WL_CHECK(s->d.has_body && s->mu1 && s->V, "simulation was created with has_body=0");
  SetArg P; WL_TRY(wl::bodyset_from_body(s->d.D, body, &P));
  return sim_measure(s, P, eps, st);
}
int wl_sim_pressure_force_body(wl_sim* s, const wl_body* body, double* out, void* st) { return sim_force_body(0, s, nullptr, body, out, st); }
int wl_sim_viscous_force_body(wl_sim* s, const wl_body* body, double* out, void* st) { return sim_force_body(1, s, nullptr, body, out, st); }
int wl_sim_measure_bodyset(wl_sim* s, const wl_bodyset* set, float eps, void* st) {
  WL_CHECK(s, "null wl_sim"); WL_CHECK(s->d.has_body && s->mu1 && s->V, "simulation was created with has_body=0");
  SetArg P; WL_TRY(wl::bodyset_prepare(s->d.D, set, &P));
  return sim_measure(s, P, eps, st);
}
static int sim_force_bodyset(int which, wl_sim* s, const float* x0, const wl_bodyset* set, double* out, void* st) {
  WL_CHECK(s && out, "null wl_sim / out");
  SetArg P; WL_TRY(wl::bodyset_prepare(s->d.D, set, &P));
  return sim_force(which, s, x0, P, out, st);
}
int wl_sim_pressure_force_bodyset(wl_sim* s, const float* x0, const wl_bodyset* set, double* out, void* st) { return sim_force_bodyset(0, s, x0, set, out, st); }
int wl_sim_viscous_force_bodyset(wl_sim* s, const float* x0, const wl_bodyset* set, double* out, void* st) { return sim_force_bodyset(1, s, x0, set, out, st); }
int wl_sim_measure_sphere(wl_sim* s, const float* c, float R, float eps, void* st) { const wl_body b = sphere_body(c, R); return wl_sim_measure_body(s, &b, eps, st); }
int wl_sim_pressure_force_sphere(wl_sim* s, const float* c, float R, double* out, void* st) { const wl_body b = sphere_body(c, R); return wl_sim_pressure_force_body(s, &b, out, st); }
// flow diagnostics on the handle's current velocity (wl_metrics.hip): reads u, writes the caller's outputs and the library's reduction workspace — nothing of the step
int wl_sim_flow_stats(wl_sim* s, const float* U, double* out, void* st) {
  WL_CHECK(s && out, "wl_sim_flow_stats: null handle or result");
  if (s->comm) { wl_set_error("wl_sim_flow_stats: z-slab handles are not supported (single domain only)"); return WL_EINVAL; }
  WL_TRY(s->settle(wl_stream(st))); WL_TRY(wl_ctx_ensure());
  const RedWs ws = wl_red_ws(wl_ctx().red);          // the library's workspace, not the solver's: the handle's state is left alone
  WL_TRY(wl::metrics_stats_dev(s->u, s->G, U, ws, wl_stream(st)));
  float mx; WL_TRY(wl::read_results(ws, out, wl_upto(WL_RD_SUM2), &mx, wl_upto(WL_RF_LEAF), wl_stream(st)));
  out[2] = (double)mx;
  return 0;
}
int wl_sim_flow_fields(wl_sim* s, const float* U, float* ke, float* w3, float* wmag, float* l2, void* st) {
  WL_CHECK(s, "wl_sim_flow_fields: null handle");
  if (s->comm) { wl_set_error("wl_sim_flow_fields: z-slab handles are not supported (single domain only)"); return WL_EINVAL; }
  WL_TRY(s->settle(wl_stream(st)));
  return wl::metrics_fields(s->u, s->G, U, ke, w3, wmag, l2, wl_stream(st));
}
// interp at n points of the handle's CURRENT u and p (roles rotate), both outputs in one launch (wl_interp.hip)
int wl_sim_sample(wl_sim* s, const float* x, size_t n, float* u_out, float* p_out, void* st) {
  WL_CHECK(s, "wl_sim_sample: null handle");
  if (s->comm) { wl_set_error("wl_sim_sample: z-slab handles are not supported (single domain only)"); return WL_EINVAL; }
  WL_CHECK(u_out || p_out, "wl_sim_sample: both outputs are null");
  if (n == 0) return 0;
  WL_CHECK(x, "wl_sim_sample: null points");
  WL_TRY(s->settle(wl_stream(st)));
  const size_t D = (size_t)s->d.D, nc = (size_t)s->G.cs;
  auto ov = [](const float* a, size_t na, const float* b, size_t nb) { return a && b && a < b + nb && b < a + na; };
  WL_CHECK(!ov(u_out, n * D, s->u, nc * D) && !ov(u_out, n * D, s->p, nc) && !ov(p_out, n, s->u, nc * D) && !ov(p_out, n, s->p, nc) && !ov(u_out, n * D, x, n * D) &&
           !ov(p_out, n, x, n * D) && !ov(u_out, n * D, p_out, n), "wl_sim_sample: an output overlaps the flow arrays, the points or the other output");
  return wl::interp_points(u_out ? s->u : nullptr, p_out ? s->p : nullptr, s->G, x, n, u_out, (long)D, p_out, 1, wl_stream(st));
}
int wl_sim_set_probes(wl_sim* s, const float* host_x, int m, int capacity) {
  WL_CHECK(s && m >= 0, "wl_sim_set_probes: null handle or negative m");
  if (s->comm) { wl_set_error("wl_sim_set_probes: z-slab handles are not supported (single domain only)"); return WL_EINVAL; }
  WL_CHECK(m == 0 || (host_x && capacity >= 1), "wl_sim_set_probes: null points or capacity < 1");
  return s->obs.set_probes(s->d.D, host_x, m, capacity);
}
int wl_sim_read_probes(wl_sim* s, float* host_out, int cap_records, int* n_records, int* first_step) {
  WL_CHECK(s && n_records && first_step, "wl_sim_read_probes: null handle or result");
  return s->obs.probes.read(host_out, cap_records, n_records, first_step, "wl_sim_read_probes");
}
static int force_handle_ok(wl_sim* s, const char* who) {
  WL_CHECK(s, "null wl_sim");
  if (s->comm) { wl_set_error(std::string(who) + ": z-slab handles are not supported (single domain only)"); return WL_EINVAL; }
  if (!s->d.has_body) { wl_set_error(std::string(who) + ": the simulation was created with has_body=0"); return WL_EINVAL; }
  return 0;
}
int wl_sim_set_force_record(wl_sim* s, const wl_bodyset* host_set, const float* host_x0, int capacity) {
  WL_TRY(force_handle_ok(s, "wl_sim_set_force_record"));
  SetArg P;
  if (host_set) { WL_CHECK(capacity >= 1, "wl_sim_set_force_record: capacity < 1"); WL_TRY(wl::bodyset_prepare(s->d.D, host_set, &P)); WL_TRY(wl::bodyset_lattice_margin(P, 2.f, "wl_sim_set_force_record")); }
  return s->obs.set_force_record(s->G, s->d.D, host_set ? &P : nullptr, host_x0, capacity);
}
int wl_sim_read_forces(wl_sim* s, double* host_out, int cap_records, int* n_records, int* first_step) {
  WL_CHECK(s && n_records && first_step, "wl_sim_read_forces: null handle or result");
  return s->obs.forces.read(host_out, cap_records, n_records, first_step, "wl_sim_read_forces");
}
int wl_sim_forces_bodyset(wl_sim* s, const float* host_x0, const wl_bodyset* host_set, double out[12], void* st) {
  WL_TRY(force_handle_ok(s, "wl_sim_forces_bodyset"));
  WL_CHECK(out, "wl_sim_forces_bodyset: null result");
  SetArg P; WL_TRY(wl::bodyset_prepare(s->d.D, host_set, &P));
  WL_TRY(wl::bodyset_lattice_margin(P, 2.f, "wl_sim_forces_bodyset"));
  hipStream_t q = wl_stream(st);
  WL_TRY(s->settle(q));
  return s->obs.forces_now(s->view(), P, host_x0, out, q);
}
int wl_sim_set_tracers(wl_sim* s, const float* host_x, size_t n) {
  WL_CHECK(s, "wl_sim_set_tracers: null handle");
  if (s->comm) { wl_set_error("wl_sim_set_tracers: z-slab handles are not supported (single domain only)"); return WL_EINVAL; }
  WL_CHECK(n == 0 || host_x, "wl_sim_set_tracers: null points");
  return s->obs.set_tracers(s->d.D, host_x, n);
}
static int mean_handle_ok(wl_sim* s, const char* who, int need_mode) {
  WL_CHECK(s, "null wl_sim");
  if (s->comm) { wl_set_error(std::string(who) + ": z-slab handles are not supported (single domain only)"); return WL_EINVAL; }
  if (s->obs.mean_mode < need_mode) { wl_set_error(std::string(who) + (need_mode == 2 ? ": the observer keeps no UU (wl_sim_set_meanflow mode 2)" : ": no mean-flow observer is set (wl_sim_set_meanflow)")); return WL_EINVAL; }
  return 0;
}
int wl_sim_set_meanflow(wl_sim* s, int mode, int every, float t_init, void* st) {
  WL_TRY(mean_handle_ok(s, "wl_sim_set_meanflow", 0));
  WL_CHECK(mode >= 0 && mode <= 2, "wl_sim_set_meanflow: mode must be 0 (off), 1 (P, U) or 2 (P, U, UU)");
  WL_CHECK(mode == 0 || every >= 1, "wl_sim_set_meanflow: every < 1");
  return s->obs.set_meanflow(s->view(), mode, every, std::isnan(t_init) ? (float)wl_sim_time(s) : t_init, wl_stream(st));
}
int wl_sim_meanflow_reset(wl_sim* s, float t_init, void* st) {
  WL_TRY(mean_handle_ok(s, "wl_sim_meanflow_reset", 1));
  return s->obs.mean_reset(std::isnan(t_init) ? (float)wl_sim_time(s) : t_init, wl_stream(st));
}
int wl_sim_meanflow_update(wl_sim* s, void* st) {
  WL_TRY(mean_handle_ok(s, "wl_sim_meanflow_update", 1));
  WL_TRY(s->settle(wl_stream(st)));      // (guards: between calls neither the divisor nor BC! is pending)
  return s->obs.mean_update(s->view(), wl::Observers::time_f(s->dt, s->dt.size() - 1), wl_stream(st));
}
float* wl_sim_meanflow(wl_sim* s, int which, size_t* n) {
  if (!s || !s->obs.mean_mode || which < 0 || which > 2 || (which == 2 && s->obs.mean_mode != 2)) return nullptr;
  const size_t cs = (size_t)s->G.cs;
  if (n) *n = cs * (size_t)(which == 0 ? 1 : which == 1 ? s->d.D : wl::meanflow_packed_planes(s->d.D));
  return which == 0 ? s->obs.mean_P() : which == 1 ? s->obs.mean_U() : s->obs.mean_UU();
}
int wl_sim_meanflow_uu(wl_sim* s, float* out, int tau, void* st) {
  WL_TRY(mean_handle_ok(s, "wl_sim_meanflow_uu", 2));
  WL_CHECK(out, "wl_sim_meanflow_uu: null output");
  return wl::meanflow_expand(out, s->obs.mean_UU(), s->obs.mean_U(), s->G, tau, wl_stream(st));
}
int wl_sim_meanflow_t(const wl_sim* s, float* out, int cap) {
  if (!s) return 0;
  const int n = (int)s->obs.mean_t.size();
  for (int k = 0; k < n && k < cap && out; k++) out[k] = s->obs.mean_t[(size_t)k];
  return n;
}
float* wl_sim_tracers(wl_sim* s, int which, size_t* n) {
  if (!s || (which != 0 && which != 1)) return nullptr;
  if (n) *n = s->obs.tr_n;
  return which == 0 ? s->obs.tr_x : s->obs.tr_x0;
}
int wl_sim_viscous_force_sphere(wl_sim* s, const float* c, float R, double* out, void* st) { const wl_body b = sphere_body(c, R); return wl_sim_viscous_force_body(s, &b, out, st); }
}  // extern "C"
