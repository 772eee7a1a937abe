// BC!(a,uBC::Function,saveexit,perdir,t) (src/core.jl:201-219) as one launch, for any source of the boundary values: the cells BC! touches, the chain of a
// touched cell collected from the last direction inwards and evaluated from its innermost cell outwards, (U(c) + v) − U(c′) per Neumann step.  Two kernels are
// built on it: k_bc_vec_fn (wl_flow.hip: U is a table the host filled) and k_bc_vec_terms (wl_terms.hip: U is Σₖ bₖ·Fₖ, formed on the fly).
// A value source is a callable U(o) -> float for the offset o = a·cs + cell into an array of the shape of `a`.
#pragma once
#include "wl_common.hpp"

// the cells of component a that BC! writes
template <int D>
__device__ __forceinline__ bool bc_touched(const int* I, const int* N, int a, int saveexit, unsigned per) {
  for (int b = 0; b < D; b++) {
    const bool pb = (per >> b) & 1u;
    if (pb) { if (I[b] == 1 || I[b] == N[b]) return true; }
    else if (a == b) { if (I[b] == 1 || I[b] == 2 || (I[b] == N[b] && !(saveexit && a == 0))) return true; }
    else { if (I[b] == 1 || I[b] == N[b]) return true; }
  }
  return false;
}
struct BcTableSrc {      // the tabulated uBC(i,loc(i,I),t): read on the two outermost layers of the non-periodic directions only
  const float* __restrict__ Ub;
  __device__ __forceinline__ float operator()(long o) const { return Ub[o]; }
};
// the body of a kernel launched on bc_chain_grid(): blockIdx.y = plane id (dir d = id/3, which = id%3 -> Julia index {1,2,N_d}), one thread per cell of the plane
template <int D, class Src>
__device__ __forceinline__ void bc_vec_chain(const GridX& g, float* __restrict__ a_, const Src& U, int saveexit, unsigned per, int zwalls) {
  const int pid = blockIdx.y, d = pid / 3, which = pid % 3;
  const int N[3] = {g.nx, g.ny, (D == 3) ? g.gnz : 1};
  const int d1 = (d == 0) ? 1 : 0, d2 = (d == 2) ? 1 : 2;
  const int n1 = (d1 == 0) ? g.nx : g.ny;
  const long cnt = (long)n1 * ((D == 3) ? ((d2 == 1) ? g.ny : g.nz) : 1);
  const long q = (long)blockIdx.x * WL_BLOCK + threadIdx.x;
  if (q >= cnt) return;
  int loc[3] = {0, 0, 0};
  loc[d1] = (int)(q % n1);
  if (D == 3) loc[d2] = (int)(q / n1);
  const int Id = (which == 0) ? 1 : (which == 1 ? 2 : N[d]);
  int I[3];
  if (d == 2) { const int kl = Id - 1 - g.gk; if (kl < 0 || kl >= g.nz) return; loc[2] = kl; if (!zwalls) return; }
  else loc[d] = Id - 1;
  I[0] = loc[0] + 1; I[1] = loc[1] + 1; I[2] = (D == 3) ? g.gk + loc[2] + 1 : 1;
  if (D == 3 && d != 2) {
    const int K = I[2];
    const bool owned = (loc[2] >= g.k0 && loc[2] < g.k1) || (zwalls && (K == 1 || K == N[2]));   // (z-periodic slabs: planes 1 and N are halo planes too)
    if (!owned) return;
  }
  auto off = [&](const int* J) -> long { return (long)(J[0] - 1) + (long)(J[1] - 1) * g.sy + ((D == 3) ? (long)(J[2] - 1 - g.gk) * g.sz : 0); };
  for (int a = 0; a < D; a++) {
    if (!bc_touched<D>(I, N, a, saveexit, per)) continue;
    long chain[4]; bool neu[4]; int nc = 0;        // cells from I inwards; neu[q]: step q→q+1 is a Neumann (function) step, else a periodic copy
    int J[3] = {I[0], I[1], I[2]};
    chain[0] = off(J);
    bool dirichlet = false;
    for (int b = D - 1; b >= 0; b--) {
      const bool pb = (per >> b) & 1u;
      int moved = 0;
      if (pb) { if (J[b] == 1) { J[b] = N[b] - 1; moved = 1; } else if (J[b] == N[b]) { J[b] = 2; moved = 1; } }
      else if (a == b) { if (J[b] == 1 || J[b] == 2 || (J[b] == N[b] && !(saveexit && a == 0))) { dirichlet = true; break; } }
      else { if (J[b] == 1) { J[b] = 2; moved = 2; } else if (J[b] == N[b]) { J[b] = N[b] - 1; moved = 2; } }
      if (moved) { neu[nc] = moved == 2; nc++; chain[nc] = off(J); }
    }
    const long ao = (long)a * g.cs;
    float v = dirichlet ? U(ao + chain[nc]) : a_[ao + chain[nc]];
    for (int qk = nc - 1; qk >= 0; qk--) if (neu[qk]) v = (U(ao + chain[qk]) + v) - U(ao + chain[qk + 1]);
    a_[ao + chain[0]] = v;
  }
}
// launch geometry of such a kernel: the largest plane cross-section decides grid.x; zwalls: this rank applies the z faces
static inline dim3 bc_chain_grid(const GridX& g, unsigned per, int* zwalls) {
  long cmax = (long)g.ny * (g.D == 3 ? g.nz : 1);
  cmax = cmax > (long)g.nx * (g.D == 3 ? g.nz : 1) ? cmax : (long)g.nx * (g.D == 3 ? g.nz : 1);
  cmax = cmax > g.sz ? cmax : g.sz;
  const bool dist = (g.D == 3) && (g.nz != g.gnz);
  *zwalls = (g.D == 3) ? ((dist && ((per >> 2) & 1u)) ? 0 : 1) : 0;
  return dim3((unsigned)((cmax + WL_BLOCK - 1) / WL_BLOCK), (unsigned)(3 * g.D), 1);
}
