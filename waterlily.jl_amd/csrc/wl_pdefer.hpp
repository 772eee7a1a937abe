// The unscaled pressure that is not stored between the solves of a time step (wl_sim, option "pdefer").
//
// mom_project! ends with `b.x ./= dt` (src/Flow.jl:229) and starts with `b.x .*= dt` (:225).  Inside a time step the only reader of the quotient is the next
// projection's head, so a tail may leave the SCALED x where the solver put it and hand the divisor on: the fused head (wl_resjac.hip) forms
// fl(fl(x/dt_prev)·dt) on load — the two roundings of the stored form in the same order, hence the same bits — and the tails lose 4 of their 32 bytes per cell.
// Everything that forms x/dt goes through wl_unscale below (every file of the library is compiled with the same floating-point flags, csrc/Makefile).
#pragma once
#include "wl_common.hpp"

#ifdef __HIPCC__
__device__ __forceinline__ float wl_unscale(float x, float dt) { return x / dt; }
#endif

namespace wl {
// the fused head on a scaled pressure whose `./= dt_prev` is pending (dt_prev = 0: x is an unscaled p — wl_common.hpp's resjac)
int resjac(float* xout, float* rout, const float* x, const float* u, const GridX& g, float dt, float w, const ConstL& cl, const RedWs& ws, int slot_d, int slot_f, hipStream_t s,
           bool shell, const float* bcU, float dt_prev);
// (the tails that leave the store out: TailReq::skip_p, wl_project.hpp — k_project_unscale on 3-D constant-coefficient levels, k_project_cfl2, k_project_wide)
}  // namespace wl
