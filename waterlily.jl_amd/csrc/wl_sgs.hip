// sgs!(flow,u,t; νₜ=smagorinsky,S,Cs,Δ) (src/util.jl:66-76) — the Smagorinsky–Lilly eddy-viscosity force added to flow.f, 3-D Float32.
//
// The model is the docstring's own code example (src/util.jl:62): νₜ(I) = (Cs·Δ)²·sqrt(S[I]:S[I]) — sqrt(S:S), NOT the sqrt(2S:S) of the
// prose above it.  The code is followed; a user who wants |S| = sqrt(2S:S) scales Cs by 2^¼.
//
// What the reference does: S[I,:,:] = S(I,u) on inside(σ) (a 3×3 tensor per cell, src/Metrics.jl:42-44,140), then for each (i,j)
//   σ[I] = −νₜ(I)·(u[I,i]−u[I−δⱼ,i]);  f[I,i] += σ[I]   over inside_u(N,j)   (src/core.jl:55-57: 3:Nⱼ−1 along j, 2:Nₖ elsewhere)
//   f[I−δⱼ,i] −= σ[I]                                    over inside_u(N,j)
// Outside inside(σ) the reference reads whatever the user's S buffer held there; the library DEFINES that as zero (a zero-initialised
// buffer, as the docstring's usage implies): νₜ ≡ 0 on the ghost layer.  Per element of f the nine sweeps are a fixed order,
//   f[I,i] = (((((r + σᵢ₁[I]) − σᵢ₁[I+δ₁]) + σᵢ₂[I]) − σᵢ₂[I+δ₂]) + σᵢ₃[I]) − σᵢ₃[I+δ₃],
// each term present where its index lies in inside_u(N,j) — written here as a gather in that order, no atomics.  With νₜ = 0 on the
// ghost layer every term that touches a ghost cell of f is ±0, so only inside cells of f are rewritten.
//
// Two launches (16 + 40 B/cell of own traffic):
//   k_sgs_nut    u → νₜ on inside(σ), stored in flow.σ (the reference uses flow.σ as scratch here too; conv_diff! has finished with it)
//   k_sgs_apply  u, νₜ, f → f; it also leaves in σ's ghost cells what the reference's sweeps leave there: ±0 where a sweep's range
//                covers a ghost cell (every coordinate ≥ 2, one of them inside 3:N−1), the stale values everywhere else — CFL's
//                maximum(σ) reads those cells (src/Flow.jl:234-237).  σ's inside cells hold νₜ afterwards (the reference: σ₃₃);
//                nothing reads them before `@inside σ = …` rewrites them.
// Linear block order, one plane per slot (wl_tile_lin): the ±z neighbours of a plane are hits in the same XCD's L2.
// The products must not be contracted into the sums (the order above is the reference's statement order): -ffp-contract=off.
#include "wl_common.hpp"

#pragma clang fp contract(off)

namespace {
// ∂(a,b,I,u) at the cell centre   src/Metrics.jl:42-44 (@fastmath in the reference: its association is not defined; this is the written order)
__device__ __forceinline__ float sgs_d(const float* __restrict__ u, const GridX& g, long o, const long* st, int a, int b) {
  const float* __restrict__ f = u + (long)a * g.cs;
  if (a == b) return f[o + st[a]] - f[o];
  return (f[o + st[b]] + f[o + st[b] + st[a]] - f[o - st[b]] - f[o - st[b] + st[a]]) / 4;
}

__global__ void __launch_bounds__(WL_BLOCK) k_sgs_nut(GridX g, float* __restrict__ nut, const float* __restrict__ u, float c2) {
  long m; int pz;
  if (!wl_tile_lin(g, m, pz) || m >= g.sz) return;
  const int j = (int)(m / g.nx), i = (int)(m - (long)j * g.nx);
  if (i < 1 || i > g.nx - 2 || j < 1 || j > g.ny - 2) return;
  const int k = 1 + pz;                                   // inside planes 1 .. nz-2
  const long o = m + (long)k * g.sz;
  const long st[3] = {1, g.sy, g.sz};
  // S = (∂ᵢuⱼ + ∂ⱼuᵢ)/2   src/Metrics.jl:140 ; S:S over the nine entries in storage order
  const float s11 = sgs_d(u, g, o, st, 0, 0), s22 = sgs_d(u, g, o, st, 1, 1), s33 = sgs_d(u, g, o, st, 2, 2);
  const float s12 = (sgs_d(u, g, o, st, 0, 1) + sgs_d(u, g, o, st, 1, 0)) / 2;
  const float s13 = (sgs_d(u, g, o, st, 0, 2) + sgs_d(u, g, o, st, 2, 0)) / 2;
  const float s23 = (sgs_d(u, g, o, st, 1, 2) + sgs_d(u, g, o, st, 2, 1)) / 2;
  float ss = s11 * s11;
  ss += s12 * s12; ss += s13 * s13;
  ss += s12 * s12; ss += s22 * s22; ss += s23 * s23;
  ss += s13 * s13; ss += s23 * s23; ss += s33 * s33;
  nut[o] = c2 * sqrtf(ss);                                // smagorinsky(I;S,Cs,Δ)   src/util.jl:62
}

__global__ void __launch_bounds__(WL_BLOCK) k_sgs_apply(GridX g, float* __restrict__ f, float* __restrict__ nut, const float* __restrict__ u) {
  long m; int pz;
  if (!wl_tile_lin(g, m, pz) || m >= g.sz) return;
  const int j = (int)(m / g.nx), i = (int)(m - (long)j * g.nx);
  if (i < 1 || j < 1) return;                              // Julia index 1: in no sweep's range
  const int k = 1 + pz;                                   // planes 1 .. nz-1
  const long o = m + (long)k * g.sz;
  const int c[3] = {i, j, k}, n[3] = {g.nx, g.ny, g.nz};
  if (i > g.nx - 2 || j > g.ny - 2 || k > g.nz - 2) {     // an upper ghost cell: ±0 if some sweep's inside_u(N,j) covers it, else untouched
    if ((i >= 2 && i <= g.nx - 2) || (j >= 2 && j <= g.ny - 2) || (k >= 2 && k <= g.nz - 2)) nut[o] = 0.f;
    return;
  }
  const long st[3] = {1, g.sy, g.sz};
  const float n0 = nut[o];
  float nup[3];
#pragma unroll
  for (int b = 0; b < 3; b++) nup[b] = (c[b] <= n[b] - 3) ? nut[o + st[b]] : 0.f;      // νₜ(I+δ_b); a ghost neighbour lies in no sweep's range along b
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float* __restrict__ ua = u + (long)a * g.cs;
    const float uc = ua[o];
    float r = f[(long)a * g.cs + o];
#pragma unroll
    for (int b = 0; b < 3; b++) {
      if (c[b] >= 2) r += -n0 * (uc - ua[o - st[b]]);                                  // f[I,a] += σ_ab[I],      I ∈ inside_u(N,b)
      if (c[b] <= n[b] - 3) r -= -nup[b] * (ua[o + st[b]] - uc);                       // f[I,a] −= σ_ab[I+δ_b],  I+δ_b ∈ inside_u(N,b)
    }
    f[(long)a * g.cs + o] = r;
  }
}
}  // namespace

namespace wl {
int sgs(float* f, float* sigma, const float* u, const GridX& g, float Cs, float Delta, hipStream_t s) {
  if (g.D != 3) { wl_set_error("sgs!: the Smagorinsky model is built for 3-D grids only"); return WL_EINVAL; }
  if (!(g.k0 == 1 && g.k1 == g.nz - 1 && g.gk == 0 && g.gnz == g.nz)) { wl_set_error("sgs!: z-slab grids are not supported (single domain only)"); return WL_EINVAL; }
  if (!f || !sigma || !u) { wl_set_error("sgs!: null field"); return WL_EINVAL; }
  const float cd = Cs * Delta, c2 = cd * cd;              // (Cs*Δ)^2
  hipLaunchKernelGGL(k_sgs_nut, wl_plane_grid(g, g.nz - 2), dim3(WL_BLOCK), 0, s, g, sigma, u, c2);
  hipLaunchKernelGGL(k_sgs_apply, wl_plane_grid(g, g.nz - 1), dim3(WL_BLOCK), 0, s, g, f, sigma, u);
  WL_LAUNCH_CHECK(); return 0;
}
}  // namespace wl
