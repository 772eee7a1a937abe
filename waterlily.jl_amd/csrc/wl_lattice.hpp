// Sampled distance fields (include/wlhip.h wl_sdf_lattice): the process-wide table of live lattices (wl_lattice.hip, host code) and the device side of the
// lattice leaf of a body program — sdf(ξ) = interp((ξ − c)/s, A) − R, its gradient and, for a lattice that carries velocity samples, the body-frame surface
// velocity ωξ(ξ) = interp((ξ − c)/s, W_c) per component, through the statements of wl_interp_dev.hpp.
#pragma once
#include "wl_common.hpp"
#include "wl_interp_dev.hpp"

#define WL_LATTICE_MAX 8      // live lattices of a process; also the lattices one body program can name

// A lattice as a kernel takes it (inside SetArg, kernarg memory): the device samples, first index fastest, and their extents.  id: the table entry it was
// resolved from — a stored program is resolved again by it before every launch (wl::bodyset_resolve).  w: the velocity samples, D component planes of
// n[0]·n[1]·n[2] floats each (component-major, first index fastest inside a plane), NULL for a lattice without them.  gen: how often the lattice has been
// re-filled in place (wl_sdf_lattice_update_mesh, _set_velocity) — the pointers stay, so this is what tells a stored program that its tile list is stale.
struct LatRef { const float* a; const float* w; int32_t n[3]; int32_t id; int32_t gen; };

namespace wl {
// the live lattice `id` -> its samples and extents, and min|A| over the samples a clamped query reads (0: mixed signs there); WL_EINVAL for an unknown
// or destroyed id.  band / spacing (either may be NULL): the band the lattice was made with (0: none) and the spacing it was baked at (0: not from a mesh)
int lattice_resolve(int id, int D, LatRef* out, float* edge_min, float* band = nullptr, float* spacing = nullptr);
}  // namespace wl

#pragma clang fp contract(off)
namespace {
// q = (ξ − c)/s, the lower corner and y of its cell; act: bit d set where _interp_clamp moves q_d (there ∂q_d/∂ξ_d = 0)
template <int D>
__device__ __forceinline__ long lattice_cell(const LatRef& L, const float* c, float s, const float* xi, const long (&st)[3], float (&y)[D], unsigned& act) {
  const int ng[3] = {L.n[0], L.n[1], L.n[2]};
  float q[D];
  act = 0u;
#pragma unroll
  for (int d = 0; d < D; d++) {
    q[d] = (xi[d] - c[d]) / s;
    if (!(q[d] >= 0.f && q[d] <= (float)(ng[d] - 2))) act |= 1u << d;
  }
  return ip_cell<D>(ng, st, q, y);
}
template <int D>
__device__ __forceinline__ float lattice_sdf(const LatRef& L, const float* c, float s, float R, const float* xi) {
  const long st[3] = {1, (long)L.n[0], (long)L.n[0] * (long)L.n[1]};
  float y[D]; unsigned act;
  const long o = lattice_cell<D>(L, c, s, xi, st, y, act);
  return ip_sum<D>(L.a, st, o, y) - R;
}
// ∇_ξ sdf as ForwardDiff gives it through _interp: i = floor(x) is held fixed (the cell to the right of a node), 0 in a clamped direction
template <int D>
__device__ __forceinline__ void lattice_grad(const LatRef& L, const float* c, float s, const float* xi, float* g) {
  const long st[3] = {1, (long)L.n[0], (long)L.n[0] * (long)L.n[1]};
  float y[D], gy[D]; unsigned act;
  const long o = lattice_cell<D>(L, c, s, xi, st, y, act);
  ip_grad<D>(L.a, st, o, y, gy);
#pragma unroll
  for (int d = 0; d < D; d++) g[d] = ((act >> d) & 1u) ? 0.f : gy[d] / s;
}
// the same gradient and, for a lattice with velocity samples (returns true), ωξ_c = interp(q, W_c), c < D: the cell, the weights and the clamp of the distance
// (one lattice_cell for both), ip_sum on component plane c
template <int D>
__device__ __forceinline__ bool lattice_grad_vel(const LatRef& L, const float* c, float s, const float* xi, float* g, float* wx) {
  const long st[3] = {1, (long)L.n[0], (long)L.n[0] * (long)L.n[1]};
  float y[D], gy[D]; unsigned act;
  const long o = lattice_cell<D>(L, c, s, xi, st, y, act);
  ip_grad<D>(L.a, st, o, y, gy);
#pragma unroll
  for (int d = 0; d < D; d++) g[d] = ((act >> d) & 1u) ? 0.f : gy[d] / s;
  const float* w = L.w;
  if (w == nullptr) return false;
  const long plane = st[2] * (long)L.n[2];
#pragma unroll
  for (int d = 0; d < D; d++) wx[d] = ip_sum<D>(w + (long)d * plane, st, o, y);
  return true;
}
}  // namespace
