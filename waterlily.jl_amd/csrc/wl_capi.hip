// C ABI of libwlhip.so (see include/wlhip.h): context, scratch, profiling scopes, the fork/join streams and the extern "C" wrappers (the MultiLevelPoisson handle itself: wl_mg.hip).
#include <cmath>
#include <string>

#include "wl_common.hpp"
#include "wl_mg.hpp"
#include "wl_terms.hpp"

static thread_local std::string g_err;
void wl_set_error(const std::string& s) { g_err = s; }

WlCtx& wl_ctx() { static WlCtx c; return c; }
int wl_ctx_ensure() {
  WlCtx& c = wl_ctx();
  if (c.inited) return 0;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { wl_set_error("libwlhip: no HIP device visible — the HIP path has no CPU fallback"); return WL_ENOGPU; }
  WL_HIP(hipGetDevice(&c.device));
  WL_HIP(hipMalloc(&c.red, wl_red_bytes()));
  // one pinned 128-byte record, laid out like RedWs' device record (8 doubles, then floats): both halves come back in ONE copy
  WL_HIP(hipHostMalloc((void**)&c.h_d, 128, hipHostMallocDefault));
  c.h_f = (float*)((char*)c.h_d + 64);
  c.inited = true;
  return 0;
}

void* wl_scratch(size_t bytes) {
  static void* buf = nullptr; static size_t cap = 0;
  if (bytes <= cap) return buf;
  if (buf) { (void)hipFree(buf); buf = nullptr; cap = 0; }
  const size_t want = bytes < 4096 ? 4096 : bytes;
  if (hipMalloc(&buf, want) != hipSuccess) { buf = nullptr; wl_set_error("hipMalloc failed for the scratch buffer"); return nullptr; }
  cap = want;
  return buf;
}

long g_wl_launches = 0;
// two auxiliary streams for launches that are independent of each other (plane ranges of a level with a body): fork/join with events
namespace wl {
namespace { hipStream_t g_par[2] = {nullptr, nullptr}; hipEvent_t g_par_fork = nullptr, g_par_join[2] = {nullptr, nullptr}; int g_par_state = 0; }
bool par_streams_ok() {
  if (g_par_state == 0) {
    g_par_state = -1;
    if (hipStreamCreateWithFlags(&g_par[0], hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithFlags(&g_par[1], hipStreamNonBlocking) == hipSuccess &&
        hipEventCreateWithFlags(&g_par_fork, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&g_par_join[0], hipEventDisableTiming) == hipSuccess &&
        hipEventCreateWithFlags(&g_par_join[1], hipEventDisableTiming) == hipSuccess) g_par_state = 1;
  }
  return g_par_state == 1;
}
hipStream_t par_stream(int i) { return g_par[i]; }
int par_fork(hipStream_t s) {
  WL_HIP(hipEventRecord(g_par_fork, s));
  WL_HIP(hipStreamWaitEvent(g_par[0], g_par_fork, 0)); WL_HIP(hipStreamWaitEvent(g_par[1], g_par_fork, 0));
  return 0;
}
int par_join(hipStream_t s) {
  for (int i = 0; i < 2; i++) { WL_HIP(hipEventRecord(g_par_join[i], g_par[i])); WL_HIP(hipStreamWaitEvent(s, g_par_join[i], 0)); }
  return 0;
}
}  // namespace wl
WlProf& wl_prof() { static WlProf p; return p; }
ProfScope::ProfScope(int id_, hipStream_t s_) : id(id_), s(s_), active(false), idx(0) {
  WlProf& p = wl_prof();
  if (!p.on || id < 0) return;
  if (p.only_roofline && id != WL_PROF_GS_A && id != WL_PROF_GS_B) return;
  WlProf::Slot& sl = p.slot[id];
  if (sl.used >= 16384) return;
  if (sl.used >= sl.a.size()) { hipEvent_t ea, eb; if (hipEventCreate(&ea) != hipSuccess || hipEventCreate(&eb) != hipSuccess) return; sl.a.push_back(ea); sl.b.push_back(eb); }
  idx = sl.used++; active = true;
  (void)hipEventRecord(sl.a[idx], s);
}
ProfScope::~ProfScope() { if (active) (void)hipEventRecord(wl_prof().slot[id].b[idx], s); }

// ================================================================================================
extern "C" {

int wl_version(void) { return 100; }
int wl_prof_enable(int on) {
  WlProf& p = wl_prof();
  WL_HIP(hipDeviceSynchronize());
  for (int q = 0; q < WL_PROF_NSLOTS; q++) p.slot[q].used = 0;
  p.on = on != 0; p.only_roofline = on == 2;
  return 0;
}
int wl_prof_read(int slot, int* count, double* total_ms) {
  WL_CHECK(slot >= 0 && slot < WL_PROF_NSLOTS, "bad profiling slot");
  WL_HIP(hipDeviceSynchronize());
  WlProf::Slot& sl = wl_prof().slot[slot];
  double tot = 0.0;
  for (size_t q = 0; q < sl.used; q++) { float ms = 0.f; WL_HIP(hipEventElapsedTime(&ms, sl.a[q], sl.b[q])); tot += (double)ms; }
  if (count) *count = (int)sl.used;
  if (total_ms) *total_ms = tot;
  return 0;
}
const char* wl_last_error_string(void) { return g_err.c_str(); }
int wl_init(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { wl_set_error("libwlhip: no HIP device visible"); return WL_ENOGPU; }
  WL_CHECK(device >= 0 && device < n, "device index out of range");
  WL_HIP(hipSetDevice(device));
  hipDeviceProp_t prop; WL_HIP(hipGetDeviceProperties(&prop, device));
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) { wl_set_error(std::string("libwlhip is built for gfx950 only, device is ") + prop.gcnArchName); return WL_ENOGPU; }
  return wl_ctx_ensure();
}
int wl_malloc(void** p, size_t bytes) { WL_CHECK(p != nullptr, "null out pointer"); WL_HIP(hipMalloc(p, bytes)); return 0; }
int wl_free(void* p) { WL_HIP(hipFree(p)); return 0; }
int wl_h2d(void* dst, const void* src, size_t bytes, void* stream) { WL_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, wl_stream(stream))); return 0; }
int wl_d2h(void* dst, const void* src, size_t bytes, void* stream) { WL_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, wl_stream(stream))); WL_HIP(hipStreamSynchronize(wl_stream(stream))); return 0; }
int wl_d2d(void* dst, const void* src, size_t bytes, void* stream) { WL_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, wl_stream(stream))); return 0; }
int wl_stream_sync(void* stream) { WL_HIP(hipStreamSynchronize(wl_stream(stream))); return 0; }
wl_grid wl_grid_single(int D, const int32_t* d) {
  wl_grid g; g.D = D; g.nx = d[0]; g.ny = d[1];
  if (D == 3) { g.nz = d[2]; g.k0 = 1; g.k1 = d[2] - 1; g.gk = 0; g.gnz = d[2]; }
  else { g.nz = 1; g.k0 = 0; g.k1 = 1; g.gk = 0; g.gnz = 1; }
  return g;
}
size_t wl_reduce_workspace_bytes(void) { return wl_red_bytes(); }

#define GRID_ARG(g) WL_CHECK(wl_grid_ok(g), "bad wl_grid"); const GridX G = gx(*g)
#define DEFAULT_WS() WL_TRY(wl_ctx_ensure()); const RedWs ws = wl_red_ws(wl_ctx().red)

int wl_fill(float* a, float v, size_t n, void* st) { return wl::fill(a, v, n, wl_stream(st)); }
int wl_scale(float* a, float s, size_t n, void* st) { return wl::scale(a, s, n, wl_stream(st)); }
int wl_div_scalar(float* a, float s, size_t n, void* st) { return wl::div_scalar(a, s, n, wl_stream(st)); }
int wl_sum(const float* a, size_t n, double* out, void* st) { DEFAULT_WS(); WL_TRY(wl::sum_dev(a, n, ws, WL_RD_SUM, wl_stream(st))); return wl::read_results(ws, out, wl_upto(WL_RD_SUM), nullptr, 0, wl_stream(st)); }
int wl_sum_abs_max_abs(const float* a, size_t n, double* l1, float* linf, void* st) { DEFAULT_WS(); WL_TRY(wl::l1_linf_dev(a, n, ws, WL_RD_SUM, WL_RF_LEAF, wl_stream(st))); return wl::read_results(ws, l1, wl_upto(WL_RD_SUM), linf, wl_upto(WL_RF_LEAF), wl_stream(st)); }
int wl_max(const float* a, size_t n, float* out, void* st) { DEFAULT_WS(); WL_TRY(wl::max_dev(a, n, ws, WL_RF_LEAF, wl_stream(st))); return wl::read_results(ws, nullptr, 0, out, wl_upto(WL_RF_LEAF), wl_stream(st)); }
int wl_dot(const float* a, const float* b, size_t n, double* out, void* st) { DEFAULT_WS(); WL_TRY(wl::dot_dev(a, b, n, ws, WL_RD_SUM, wl_stream(st))); return wl::read_results(ws, out, wl_upto(WL_RD_SUM), nullptr, 0, wl_stream(st)); }

int wl_bc_vec(float* a, const wl_grid* g, const float* U, int saveexit, unsigned per, void* st) { GRID_ARG(g); return wl::bc_vec(a, G, U, saveexit, per, wl_stream(st)); }
int wl_bc_vec_fn(float* a, const float* Ub, const wl_grid* g, int saveexit, unsigned per, void* st) { GRID_ARG(g); WL_CHECK(a && Ub && a != Ub, "bad argument"); return wl::bc_vec_fn(a, Ub, G, saveexit, per, wl_stream(st)); }
int wl_meanflow_update(float* P, float* U, float* UU, const float* p, const float* u, const wl_grid* g, float eps, void* st) { GRID_ARG(g); WL_CHECK(P && U && p && u, "bad argument"); return wl::meanflow_update(P, U, UU, p, u, G, eps, wl_stream(st)); }
int wl_meanflow_uu(float* tau, const float* UU, const float* U, const wl_grid* g, void* st) { GRID_ARG(g); WL_CHECK(tau && UU && U, "bad argument"); return wl::meanflow_uu(tau, UU, U, G, wl_stream(st)); }
int wl_accelerate_field(float* r, const float* gfield, const wl_grid* g, void* st) { GRID_ARG(g); WL_CHECK(r && gfield, "bad argument"); return wl::add_field(r, gfield, (size_t)G.cs * (size_t)G.D, wl_stream(st)); }
// separable terms (wl_terms.hip): every refusal on the host, before the launch
static int terms_leaf_ok(const char* who, const float* out, int K, const float* const* F, const float* c) {
  if (!out || !F || !c) { wl_set_error(std::string(who) + ": null argument"); return WL_EINVAL; }
  if (K < 1 || K > wl::TERMS_MAX) { wl_set_error(std::string(who) + ": K outside 1 ... 4"); return WL_EINVAL; }
  for (int k = 0; k < K; k++) {
    if (!F[k]) { wl_set_error(std::string(who) + ": a NULL field"); return WL_EINVAL; }
    if (F[k] == out) { wl_set_error(std::string(who) + ": a field is the output array"); return WL_EINVAL; }
    if (!std::isfinite(c[k])) { wl_set_error(std::string(who) + ": a non-finite coefficient"); return WL_EINVAL; }
  }
  return 0;
}
int wl_accel_terms(float* r, int K, const float* const* F, const float* host_c, const wl_grid* g, void* st) {
  GRID_ARG(g); WL_TRY(terms_leaf_ok("wl_accel_terms", r, K, F, host_c));
  return wl::accel_terms(r, K, F, host_c, (size_t)G.cs * (size_t)G.D, wl_stream(st));
}
int wl_bc_vec_terms(float* a, int K, const float* const* F, const float* host_b, const wl_grid* g, int saveexit, unsigned per, void* st) {
  GRID_ARG(g); WL_TRY(terms_leaf_ok("wl_bc_vec_terms", a, K, F, host_b));
  return wl::bc_vec_terms(a, K, F, host_b, G, saveexit, per, wl_stream(st));
}
int wl_bc_per_scalar(float* a, const wl_grid* g, unsigned per, void* st) { GRID_ARG(g); return wl::bc_per_scalar(a, G, per, wl_stream(st)); }
int wl_conv_diff(float* r, const float* u, float* Phi, const wl_grid* g, float nu, unsigned per, int scheme, void* st) { GRID_ARG(g); return wl::conv_diff(r, u, Phi, G, nu, per, scheme, wl_stream(st)); }
int wl_bdim(float* u, const float* u0, float* f, const float* V, const float* mu0, const float* mu1, const wl_grid* g, float dt, float pre, float post, void* st) {
  GRID_ARG(g); return wl::bdim(u, u0, f, V, mu0, mu1, G, dt, pre, post, wl_stream(st));
}
// sgs!(flow,u,t; νₜ=smagorinsky,S,Cs,Δ)   src/util.jl:66-76 — f = flow.f, sigma = flow.σ (scratch: receives νₜ)
int wl_sgs(float* f, float* sigma, const float* u, const wl_grid* g, float Cs, float Delta, void* st) { GRID_ARG(g); return wl::sgs(f, sigma, u, G, Cs, Delta, wl_stream(st)); }
// flow diagnostics   src/Metrics.jl:27-109 (wl_metrics.hip).  The single-field leaves run the instantiations wl_flow_fields runs.
int wl_flow_fields(const float* u, const wl_grid* g, const float* U, float* ke, float* w3, float* wmag, float* l2, void* st) { GRID_ARG(g); return wl::metrics_fields(u, G, U, ke, w3, wmag, l2, wl_stream(st)); }
int wl_ke(float* out, const float* u, const wl_grid* g, const float* U, void* st) { WL_CHECK(out, "wl_ke: null output"); return wl_flow_fields(u, g, U, out, nullptr, nullptr, nullptr, st); }
int wl_omega(float* out3, const float* u, const wl_grid* g, void* st) { WL_CHECK(out3, "wl_omega: null output"); return wl_flow_fields(u, g, nullptr, nullptr, out3, nullptr, nullptr, st); }
int wl_omega_mag(float* out, const float* u, const wl_grid* g, void* st) { WL_CHECK(out, "wl_omega_mag: null output"); return wl_flow_fields(u, g, nullptr, nullptr, nullptr, out, nullptr, st); }
int wl_lambda2(float* out, const float* u, const wl_grid* g, void* st) { WL_CHECK(out, "wl_lambda2: null output"); return wl_flow_fields(u, g, nullptr, nullptr, nullptr, nullptr, out, st); }
int wl_omega_theta(float* out, const float* u, const wl_grid* g, const float* z, const float* c, void* st) { GRID_ARG(g); return wl::metrics_omega_theta(out, u, G, z, c, wl_stream(st)); }
int wl_curl(float* out, const float* u, const wl_grid* g, int i, void* st) { GRID_ARG(g); return wl::metrics_curl(out, u, G, i, wl_stream(st)); }
int wl_helicity(float* out, const float* u, const float* w3, const wl_grid* g, void* st) { GRID_ARG(g); return wl::metrics_helicity(out, u, w3, G, wl_stream(st)); }
int wl_flow_stats(const float* u, const wl_grid* g, const float* U, double* out, void* scratch, void* st) {
  GRID_ARG(g); WL_CHECK(out, "wl_flow_stats: null result"); WL_TRY(wl_ctx_ensure());
  const RedWs ws = wl_red_ws(scratch ? scratch : wl_ctx().red);
  WL_TRY(wl::metrics_stats_dev(u, G, U, ws, wl_stream(st)));
  float mx; WL_TRY(wl::read_results(ws, out, wl_upto(WL_RD_SUM2), &mx, wl_upto(WL_RF_LEAF), wl_stream(st)));
  out[2] = (double)mx;
  return 0;
}
int wl_scale_u(float* u, const wl_grid* g, float s, void* st) { GRID_ARG(g); return wl::scale_u(u, G, s, wl_stream(st)); }
int wl_div(float* z, const float* u, const wl_grid* g, void* st) { GRID_ARG(g); return wl::div(z, u, G, wl_stream(st)); }
int wl_project(float* u, const float* L, const float* x, const wl_grid* g, void* st) { GRID_ARG(g); return wl::project(u, L, x, G, wl_stream(st)); }
int wl_cfl(const float* u, float* sigma, const wl_grid* g, float nu, float dt_max, float* host_dt, void* st) {
  GRID_ARG(g); DEFAULT_WS();
  WL_TRY(wl::cfl_dev(u, sigma, G, ws, WL_RF_LEAF, wl_stream(st)));
  float mx; WL_TRY(wl::read_results(ws, nullptr, 0, &mx, wl_upto(WL_RF_LEAF), wl_stream(st)));
  *host_dt = std::fmin(dt_max, 1.0f / (mx + 5 * nu));                                    // src/Flow.jl:236
  return 0;
}
int wl_set_diag(float* D, float* iD, const float* L, const wl_grid* g, void* st) { GRID_ARG(g); return wl::set_diag(D, iD, L, G, wl_stream(st)); }
int wl_mult(float* z, const float* L, const float* D, const float* x, const wl_grid* g, void* st) { GRID_ARG(g); return wl::mult(z, L, D, x, G, wl_stream(st)); }
int wl_residual(float* r, const float* x, const float* z, const float* L, const float* D, const float* iD, const wl_grid* g, void* scratch, void* st) {
  GRID_ARG(g); WL_TRY(wl_ctx_ensure());
  const RedWs ws = wl_red_ws(scratch ? scratch : wl_ctx().red);
  return wl::residual(r, x, z, L, D, iD, G, ws, wl_stream(st));
}
int wl_increment(float* r, float* x, const float* eps, const float* L, const float* D, const wl_grid* g, float w, void* st) { GRID_ARG(g); return wl::increment(r, x, eps, L, D, G, w, wl_stream(st)); }
int wl_jacobi(float* eps, float* r, float* x, const float* L, const float* D, const float* iD, const wl_grid* g, int it, float w, unsigned per, void* st) {
  GRID_ARG(g); hipStream_t s = wl_stream(st);
  for (int k = 0; k < (it <= 0 ? 1 : it); k++) {
    WL_TRY(wl::gs_init(eps, r, iD, G, s));
    WL_TRY(wl::bc_per_scalar(eps, G, per, s));       // perBC!(ϵ) inside increment!  src/Poisson.jl:101
    WL_TRY(wl::increment(r, x, eps, L, D, G, w, s));
  }
  return 0;
}
int wl_gsrb(float* eps, float* r, float* x, const float* L, const float* D, const float* iD, const wl_grid* g, int it, float w, unsigned per, void* st) {
  GRID_ARG(g); hipStream_t s = wl_stream(st);
  WL_TRY(wl::gs_init(eps, r, iD, G, s));
  WL_TRY(wl::bc_per_scalar(eps, G, per, s));
  for (int k0 = 1; k0 <= it; k0++) WL_TRY(wl::gs_sweep(eps, r, L, iD, G, k0, s));
  WL_TRY(wl::bc_per_scalar(eps, G, per, s));
  return wl::increment(r, x, eps, L, D, G, w, s);
}
// pcg!(p;it)   src/Poisson.jl:166-186.  The scalars ρ, α, β steer early exits exactly as in the reference, so each is read
// back (two host reads per iteration, like the reference's blocking `⋅`).  Single domain only.
static int pcg_impl(float* eps, float* r, float* x, float* z, const float* L, const float* D, const float* iD, const GridX& G, int it, unsigned per, const RedWs& ws, hipStream_t s) {
  const float tiny = 10 * 1.1920929e-07f;                                                  // 10eps(T)
  double h;
  WL_TRY(wl::pcg_stage(0, eps, r, x, z, L, D, iD, G, 0.f, 0, ws, s));                       // z = ϵ = r·iD ; rho = r⋅z
  WL_TRY(wl::read_results(ws, &h, wl_upto(WL_RD_SUM), nullptr, 0, s));
  float rho = (float)h;
  if (std::fabs(rho) < tiny) return 0;
  for (int i = 1; i <= it; i++) {
    WL_TRY(wl::bc_per_scalar(eps, G, per, s));                                             // perBC!(ϵ)
    WL_TRY(wl::pcg_stage(1, eps, r, x, z, L, D, iD, G, 0.f, 0, ws, s));                     // z = Aϵ ; perdot(z,ϵ)
    WL_TRY(wl::read_results(ws, &h, wl_upto(WL_RD_SUM), nullptr, 0, s));
    const float alpha = rho / (float)h;
    if (std::fabs(alpha) < 1e-2f || std::fabs(alpha) > 1e2f) return 0;                      // alpha should be O(1)
    const int more = i < it;
    WL_TRY(wl::pcg_stage(2, eps, r, x, z, L, D, iD, G, alpha, more, ws, s));                // x += αϵ ; r -= αz [; z = r·iD ; rho2 = r⋅z]
    if (!more) return 0;
    WL_TRY(wl::read_results(ws, &h, wl_upto(WL_RD_SUM), nullptr, 0, s));
    const float rho2 = (float)h;
    if (std::fabs(rho2) < tiny) return 0;
    const float beta = rho2 / rho;
    WL_TRY(wl::pcg_stage(3, eps, r, x, z, L, D, iD, G, beta, 0, ws, s));                    // ϵ = βϵ + z
    rho = rho2;
  }
  return 0;
}
int wl_pcg(float* eps, float* r, float* x, float* z, const float* L, const float* D, const float* iD, const wl_grid* g, int it, unsigned per, void* st) {
  GRID_ARG(g); WL_CHECK(g->D == 2 || g->nz == g->gnz, "pcg! is single-domain"); DEFAULT_WS();
  return pcg_impl(eps, r, x, z, L, D, iD, G, it <= 0 ? 6 : it, per, ws, wl_stream(st));
}
// solver!(p::Poisson;tol,itmx)   src/Poisson.jl:212-223
int wl_poisson_solve(float* eps, float* r, float* x, float* z, const float* L, const float* D, const float* iD, const wl_grid* g, double tol, int itmx, unsigned per,
                     int* host_n, double* host_r1, float* host_rinf, void* st) {
  GRID_ARG(g); WL_CHECK(g->D == 2 || g->nz == g->gnz, "solver!(::Poisson) is single-domain"); DEFAULT_WS();
  hipStream_t s = wl_stream(st);
  const double r1tol = (tol / 10.0) * (double)wl_ninside_global(*g);
  WL_TRY(wl::bc_per_scalar(x, G, per, s));                                                 // residual!: perBC!(x) :93
  WL_TRY(wl::residual(r, x, z, L, D, iD, G, ws, s));
  double r1 = 0.0; float rinf = 0.f;
  int np = 0;
  const int cap = itmx <= 0 ? 1000 : itmx;
  while (np < cap) {
    WL_TRY(pcg_impl(eps, r, x, z, L, D, iD, G, 6, per, ws, s));
    WL_TRY(wl::norms_dev(r, G, ws, WL_RD_L1_INIT, WL_RF_LINF_INIT, s));
    double hd[WL_RD_COUNT]; float hf[WL_RF_COUNT];
    WL_TRY(wl::read_results(ws, hd, wl_upto(WL_RD_L1_INIT), hf, wl_upto(WL_RF_LINF_INIT), s));
    r1 = (double)(float)hd[WL_RD_L1_INIT]; rinf = hf[WL_RF_LINF_INIT]; np++;
    if (r1 < r1tol && (double)rinf < tol) break;
  }
  WL_TRY(wl::bc_per_scalar(x, G, per, s));                                                 // :221
  if (host_n) *host_n = np;
  if (host_r1) *host_r1 = r1;
  if (host_rinf) *host_rinf = rinf;
  return 0;
}
int wl_norms(const float* r, const wl_grid* g, double* l1, float* linf, void* scratch, void* st) {
  GRID_ARG(g); WL_TRY(wl_ctx_ensure());
  const RedWs ws = wl_red_ws(scratch ? scratch : wl_ctx().red);
  WL_TRY(wl::norms_dev(r, G, ws, WL_RD_SUM, WL_RF_LEAF, wl_stream(st)));
  return wl::read_results(ws, l1, wl_upto(WL_RD_SUM), linf, wl_upto(WL_RF_LEAF), wl_stream(st));
}
int wl_restrict(float* a, const wl_grid* gc, const float* b, const wl_grid* gf, void* st) { WL_CHECK(wl_grid_ok(gc) && wl_grid_ok(gf), "bad wl_grid"); return wl::restrict_(a, gx(*gc), b, gx(*gf), wl_stream(st)); }
int wl_prolongate(float* a, const wl_grid* gf, const float* b, const wl_grid* gc, void* st) { WL_CHECK(wl_grid_ok(gc) && wl_grid_ok(gf), "bad wl_grid"); return wl::prolongate(a, gx(*gf), b, gx(*gc), wl_stream(st)); }
int wl_restrictL(float* a, const wl_grid* gc, const float* b, const wl_grid* gf, unsigned per, void* st) { WL_CHECK(wl_grid_ok(gc) && wl_grid_ok(gf), "bad wl_grid"); return wl::restrictL(a, gx(*gc), b, gx(*gf), per, wl_stream(st)); }
int wl_coarsen_dims(int D, const int32_t* fine, int32_t* coarse) {
  int c = 0;
  for (int d = 0; d < D; d++) { if (wl_mg_divisible(fine[d])) { coarse[d] = 1 + fine[d] / 2; c++; } else coarse[d] = fine[d]; }
  return c;
}

int wl_mg_create(wl_mg** out, float* x, float* L, float* z, const wl_grid* g, unsigned per, int maxlevels) {
  WL_CHECK(out && x && L && z, "null pointer"); WL_CHECK(wl_grid_ok(g), "bad wl_grid");
  wl_mg* mg = new wl_mg();
  int rc = mg->build(x, L, z, *g, per, maxlevels <= 0 ? 10 : maxlevels, nullptr);
  if (rc != 0) { delete mg; *out = nullptr; return rc; }
  *out = mg; return 0;
}
int wl_mg_destroy(wl_mg* mg) { delete mg; return 0; }
int wl_mg_update(wl_mg* mg, void* st) { return mg->update(wl_stream(st)); }
int wl_mg_nlevels(const wl_mg* mg) { return (int)mg->lv.size(); }
int wl_mg_level_grid(const wl_mg* mg, int l, wl_grid* out) { WL_CHECK(l >= 0 && l < (int)mg->lv.size(), "level out of range"); *out = mg->lv[(size_t)l].g; return 0; }
float* wl_mg_level_field(const wl_mg* mg, int l, const char* name) {
  if (l < 0 || l >= (int)mg->lv.size()) return nullptr;
  const wl_mg::Level& v = mg->lv[(size_t)l]; const std::string s(name);
  if (l == 0 && s == "r" && const_cast<wl_mg*>(mg)->settle_r_for_reader() != 0) return nullptr;   // skip_r: the finest residual is produced when somebody asks for it
  if (s == "L") return v.L; if (s == "D") return v.D; if (s == "iD") return v.iD; if (s == "x") return v.x;
  if (s == "eps") return v.eps; if (s == "r") return v.r; if (s == "z") return v.z;
  return nullptr;
}
int wl_mg_smooth(wl_mg* mg, int l, int it, float w, void* st) { WL_CHECK(l >= 0 && l < (int)mg->lv.size(), "level out of range"); if (l == 0) WL_TRY(mg->settle_r(wl_stream(st))); return mg->smooth(l, it <= 0 ? 4 : it, w, wl_stream(st)); }
int wl_mg_smoother_kind(const wl_mg* mg, int l) {   // 0 one kernel per pass, 1 temporally blocked (one cell per thread), 2 blocked pair kernels (constant coefficients)
  if (l < 0 || l >= (int)mg->lv.size()) return -1;
  const wl_mg::Level& p = mg->lv[(size_t)l];
  switch (mg->plan_smooth(p, 4, false, wl::B_BOTH).form) {      // the plan smooth!(it = 4) would take
    case wl_mg::Smooth::Passes: return 0;
    case wl_mg::Smooth::ZSplit: return 3;
    default: return wl::gsrb_pair_ok(p.x_, p.cl) ? 2 : 1;
  }
}
int wl_mg_level_is_const(const wl_mg* mg, int l) { return (l >= 0 && l < (int)mg->lv.size()) ? mg->lv[(size_t)l].cl.on : 0; }
int wl_mg_set_fused(wl_mg* mg, int on) { mg->use_fused = (on & 1) != 0; mg->store_eps = (on & 2) == 0; wl::gsrb_pair_enable((on & 4) == 0); mg->use_tail = (on & 8) == 0; mg->use_zsplit = (on & 16) == 0; wl::tail_lds_enable((on & 32) == 0); mg->use_xdefer = (on & 64) == 0; mg->overlap_smooth = (on & 128) == 0; mg->use_wide = (on & 256) == 0; return 0; }
int wl_mg_vcycle(wl_mg* mg, int l, float w, void* st) { WL_CHECK(l >= 0 && l + 1 < (int)mg->lv.size(), "level out of range"); if (l == 0) WL_TRY(mg->settle_r(wl_stream(st))); return mg->vcycle(l, w, wl_stream(st), false); }
int wl_mg_solve(wl_mg* mg, double tol, int itmx, int* n, double* r1, float* rinf, void* st) { return mg->solve(tol, itmx <= 0 ? 32 : itmx, n, r1, rinf, wl_stream(st)); }
int wl_mg_history(const wl_mg* mg, int16_t* out, int cap) { const int n = (int)mg->n.size(); for (int k = 0; k < n && k < cap; k++) out[k] = mg->n[(size_t)k]; return n; }
int wl_mg_shift_path(const wl_mg* mg) { return mg->shift_path; }
int wl_mg_last_log(const wl_mg* mg, double* r1, double* rinf, double* w, int cap) {
  const int n = (int)mg->log_r1.size();
  for (int k = 0; k < n && k < cap; k++) { r1[k] = mg->log_r1[(size_t)k]; rinf[k] = mg->log_rinf[(size_t)k]; w[k] = mg->log_w[(size_t)k]; }
  return n;
}
}  // extern "C"
