// The projection tails (wl_project.hip): what a tail can do on a level, what a caller asks of it, what the launcher reports.
//
// The capabilities are a function of the level alone and are computed here, once: the time-step path (wl_sim.hip) plans with the same record the launchers
// check a request against, so the two cannot disagree.  Whether the four-cells-per-thread form runs ("tailwide") is no capability: it honours whatever the
// narrower form does, depends on the alignment of the arrays actually passed, and is decided by the launcher, which reports it.
#pragma once
#include "wl_common.hpp"
#include "wl_bcfold.hpp"

namespace wl {
struct TailCaps {
  bool fold = false;      // BC!(u,U) can go into the tail's stores (wl_bc_fold_geom_ok)
  bool gate = false;      // the form honours a device flag `go` (queued ahead of the solver's convergence read)
  bool skip_p = false;    // the form can leave p = x/Δt unstored (wl_pdefer.hpp)
  bool usub = false;      // the form can read the wall-normal boundary faces of u_in as U (a deferred BC!), which takes folded stores as well
  bool pair = false;      // the corrector's tail runs with two cells per thread (k_project_cfl2) or, where the arrays allow, four (k_project_wide)
};
// the in-place tail u −= L∇x ; p = x/Δt (project_unscale)
inline TailCaps tail_caps_inplace(const GridX& g, const ConstL& cl) {
  TailCaps c; c.fold = wl_bc_fold_geom_ok(g); c.gate = true; c.skip_p = g.D == 3 && cl.on;
  return c;
}
// the corrector's out-of-place tail with flux_out and its maximum (project_cfl): everything beyond the fold rests on the pair form
inline TailCaps tail_caps_cfl(const GridX& g, const ConstL& cl) {
  TailCaps c; c.fold = wl_bc_fold_geom_ok(g);
  c.pair = g.D == 3 && cl.on && (g.nx & 1) == 0 && g.k0 >= 1 && g.k1 <= g.nz - 1;
  c.gate = c.skip_p = c.pair; c.usub = c.pair && c.fold;
  return c;
}
struct TailReq {
  const float* U = nullptr;      // BC!(u,U) folded into the stores where the level allows it (host, three values); null: not asked for
  bool usub = false;             // BC!(u_in,U) was deferred: U on load for the wall-normal boundary faces
  bool skip_p = false;           // do not store p = x/Δt (and do not touch p_out)
  bool wide = false;             // the four-cells-per-thread form may run (option "tailwide")
  const float* go = nullptr;     // device flag: the kernel does nothing unless *go > 0 (wl::decide_converged)
};
struct TailRep { bool folded = false, wide = false; };      // BC!(u,U) went into the stores / the four-cells-per-thread form ran

// A request outside the level's capabilities (usub, skip_p, go) is WL_EINVAL before any launch, never a silent other form; a fold that the level cannot
// take is not an error: the report says what happened.
int project_unscale(float* u, const float* L, const float* x, float* pout, const GridX& g, float dt, const ConstL& cl, hipStream_t s, const TailReq& rq, TailRep* rep);
int project_cfl(float* uout, const float* uin, const float* L, const float* x, float* pout, float* sigma, const GridX& g, float dt, const ConstL& cl, const RedWs& ws, int slot_f, hipStream_t s,
                int store_sigma, const TailReq& rq, TailRep* rep);
// a level with a body: the planes [0,na) and [nb,nz) with the constant-coefficient pattern `far`, [na,nb) reading L; nothing folded, substituted, skipped or gated
int project_unscale_split(float* u, const float* L, const float* x, float* pout, const GridX& g, float dt, const ConstL& near, const ConstL& far, int na, int nb, hipStream_t s);
int project_cfl_split(float* uout, const float* uin, const float* L, const float* x, float* pout, float* sigma, const GridX& g, float dt, const ConstL& near, const ConstL& far,
                      int na, int nb, const RedWs& ws, int slot_f, hipStream_t s, int store_sigma = 1);
}  // namespace wl
