// interp(x, arr) of src/util.jl:17-43 at n points on the device, and what is built on it: the probe records of a time step and
// one step of a tracer-particle swarm (the reference's pathline extension keeps `position`, `position⁰` and advances them once per
// step with the current flow, ext/WaterLilyPathlinesExt.jl).
//
//   ip_one<D>      _interp(x, arr) :29-43 for one scalar array after _interp_clamp :17-18: ip_cell then ip_sum of wl_interp_dev.hpp, where the
//                  statements and their order are written down (the lattice leaf of a body program samples through the same two)
//   ip_vec<D>      interp(x, varr) :20-25 — component i is queried at x + ½·eᵢ (shift :23), then clamped like a scalar query (:24)
//   k_interp<D>    one thread per point: the D coordinates are loaded once, then the vector array (D·2^D gathers) and/or the scalar array
//                  (2^D gathers) is interpolated.  Outputs are point-major with a leading dimension each, so that wl_interp (n×ncomp),
//                  wl_sim_sample (u n×D and p n in ONE launch) and a probe record (m×(D+1): u then p per probe) are the same kernel.
//   k_advect<D>    x⁰ ← x;  x* = x⁰ + Δt·u⁰(x⁰);  x ← x⁰ + ½Δt·(u⁰(x⁰) + u¹(x*)); periodic directions wrapped into [0, N)
// The clamp is the bounds check (:17-18): a clamped coordinate lies in [0, Ng_d − 2], so the lower corner index is in [0, Ng_d − 2] and
// the upper one is Ng_d − 1 at most.  It is written with fmaxf/fminf, which send a NaN coordinate to 0 (Julia's floor(Int, NaN) throws; a
// kernel must not index with it).  All gathers use 64-bit offsets.  Nothing is contracted into FMAs.
#include "wl_common.hpp"
#include "wl_interp_dev.hpp"

#pragma clang fp contract(off)

namespace {
template <int D>
__device__ __forceinline__ float ip_one(const float* __restrict__ a, const GridX& g, const float (&xq)[D]) {
  const int ng[3] = {g.nx, g.ny, g.nz};
  const long st[3] = {1, g.sy, g.sz};
  float y[D];
  const long o = ip_cell<D>(ng, st, xq, y);
  return ip_sum<D>(a, st, o, y);
}
// interp(x, varr) :20-25: out[i] = _interp(clamp(x + shift(i)), varr[..,i])
template <int D>
__device__ __forceinline__ void ip_vec(const float* __restrict__ v, const GridX& g, const float (&x)[D], float (&out)[D]) {
#pragma unroll
  for (int i = 0; i < D; i++) {
    float xs[D];
#pragma unroll
    for (int d = 0; d < D; d++) xs[d] = x[d] + (d == i ? 0.5f : 0.f);      // shift(i) :23
    out[i] = ip_one<D>(v + (long)i * g.cs, g, xs);
  }
}

template <int D>
__global__ void __launch_bounds__(WL_BLOCK) k_interp(GridX g, const float* __restrict__ vec, const float* __restrict__ sca, const float* __restrict__ x, size_t n,
                                                     float* __restrict__ out_v, long ldv, float* __restrict__ out_s, long lds) {
  const size_t t = (size_t)blockIdx.x * WL_BLOCK + threadIdx.x;
  if (t >= n) return;
  float xp[D];
#pragma unroll
  for (int d = 0; d < D; d++) xp[d] = x[t * D + d];
  if (vec) {
    float v[D]; ip_vec<D>(vec, g, xp, v);
#pragma unroll
    for (int i = 0; i < D; i++) out_v[t * (size_t)ldv + i] = v[i];
  }
  if (sca) out_s[t * (size_t)lds] = ip_one<D>(sca, g, xp);
}

struct AdvN { float N[3]; };      // interior cells per direction (the period of a periodic one)
template <int D>
__global__ void __launch_bounds__(WL_BLOCK) k_advect(GridX g, float* __restrict__ x, float* __restrict__ x_prev, const float* __restrict__ u0, const float* __restrict__ u1,
                                                     size_t n, float dt, unsigned per, AdvN nn) {
  const size_t t = (size_t)blockIdx.x * WL_BLOCK + threadIdx.x;
  if (t >= n) return;
  float xo[D], xs[D], v0[D], v1[D];
#pragma unroll
  for (int d = 0; d < D; d++) { xo[d] = x[t * D + d]; x_prev[t * D + d] = xo[d]; }      // x⁰ ← x
  ip_vec<D>(u0, g, xo, v0);
#pragma unroll
  for (int d = 0; d < D; d++) xs[d] = xo[d] + dt * v0[d];                               // x* = x⁰ + Δt·u⁰(x⁰)
  ip_vec<D>(u1, g, xs, v1);
#pragma unroll
  for (int d = 0; d < D; d++) {
    float xn = xo[d] + (0.5f * dt) * (v0[d] + v1[d]);                                   // x = x⁰ + ½Δt·(u⁰(x⁰) + u¹(x*))
    if ((per >> d) & 1u) {                                                              // periodic direction: into [0, N)
      const float N = nn.N[d];
      xn = xn - N * floorf(xn / N);
      if (!(xn >= 0.f) || xn >= N) xn = 0.f;                                            // (−tiny + N rounds to N; a non-finite position restarts at 0)
    }
    x[t * D + d] = xn;
  }
}

bool ip_single(const GridX& g) { return g.D == 2 || (g.k0 == 1 && g.k1 == g.nz - 1 && g.gk == 0 && g.gnz == g.nz); }
// byte ranges [a, a+na) and [b, b+nb) floats overlap
bool ip_overlap(const float* a, size_t na, const float* b, size_t nb) { return na && nb && a < b + nb && b < a + na; }
#define IP_REJECT(cond, msg) do { if (cond) { wl_set_error(msg); return WL_EINVAL; } } while (0)
int ip_blocks(size_t n, unsigned* nb) {
  const size_t b = (n + WL_BLOCK - 1) / WL_BLOCK;
  IP_REJECT(b > 0x7fffffffull, "interp: more points than one launch takes (2^31·256)");
  *nb = (unsigned)b; return 0;
}
}  // namespace

namespace wl {
// vec (Ng...,D) and/or sca (Ng...) at the n points of x; out_v[t·ldv + i], out_s[t·lds]; one launch (none for n = 0)
int interp_points(const float* vec, const float* sca, const GridX& g, const float* x, size_t n, float* out_v, long ldv, float* out_s, long lds, hipStream_t s) {
  IP_REJECT(!ip_single(g), "interp: z-slab grids are not supported (single domain only)");
  IP_REJECT((!vec && !sca) || (vec && !out_v) || (sca && !out_s), "interp: no array to interpolate, or an array without its output");
  if (n == 0) return 0;
  IP_REJECT(!x, "interp: null points");
  unsigned nb; WL_TRY(ip_blocks(n, &nb));
  if (g.D == 3) hipLaunchKernelGGL(k_interp<3>, dim3(nb), dim3(WL_BLOCK), 0, s, g, vec, sca, x, n, out_v, ldv, out_s, lds);
  else hipLaunchKernelGGL(k_interp<2>, dim3(nb), dim3(WL_BLOCK), 0, s, g, vec, sca, x, n, out_v, ldv, out_s, lds);
  WL_LAUNCH_CHECK(); return 0;
}
int advect(float* x, float* x_prev, const float* u0, const float* u1, const GridX& g, size_t n, float dt, unsigned per, hipStream_t s) {
  IP_REJECT(!ip_single(g), "advect: z-slab grids are not supported (single domain only)");
  IP_REJECT(!u0 || !u1, "advect: null velocity array");
  if (n == 0) return 0;
  IP_REJECT(!x || !x_prev, "advect: null particle array");
  const size_t nx = n * (size_t)g.D, nu = (size_t)g.D * (size_t)g.cs;
  IP_REJECT(ip_overlap(x, nx, x_prev, nx) || ip_overlap(x, nx, u0, nu) || ip_overlap(x, nx, u1, nu) || ip_overlap(x_prev, nx, u0, nu) || ip_overlap(x_prev, nx, u1, nu),
            "advect: the particle arrays overlap each other or a velocity array");
  unsigned nb; WL_TRY(ip_blocks(n, &nb));
  AdvN nn; nn.N[0] = (float)(g.nx - 2); nn.N[1] = (float)(g.ny - 2); nn.N[2] = g.D == 3 ? (float)(g.nz - 2) : 1.f;
  if (g.D == 3) hipLaunchKernelGGL(k_advect<3>, dim3(nb), dim3(WL_BLOCK), 0, s, g, x, x_prev, u0, u1, n, dt, per, nn);
  else hipLaunchKernelGGL(k_advect<2>, dim3(nb), dim3(WL_BLOCK), 0, s, g, x, x_prev, u0, u1, n, dt, per, nn);
  WL_LAUNCH_CHECK(); return 0;
}
}  // namespace wl

extern "C" {
int wl_interp(float* out, const float* arr, const wl_grid* g, const float* x, size_t n, int ncomp, void* st) {
  WL_CHECK(wl_grid_ok(g), "bad wl_grid"); WL_TRY(wl_ctx_ensure());
  const GridX G = gx(*g);
  IP_REJECT(ncomp != 1 && ncomp != G.D, "wl_interp: ncomp must be 1 (scalar array) or D (staggered vector array)");
  IP_REJECT(!arr, "wl_interp: null array");
  IP_REJECT(!ip_single(G), "wl_interp: z-slab grids are not supported (single domain only)");
  if (n == 0) return 0;
  IP_REJECT(!out || !x, "wl_interp: null output or points");
  const bool vec = ncomp == G.D && ncomp != 1;
  const size_t na = (size_t)(vec ? G.D : 1) * (size_t)G.cs, no = n * (size_t)ncomp, nx = n * (size_t)G.D;
  IP_REJECT(ip_overlap(out, no, arr, na) || ip_overlap(out, no, x, nx), "wl_interp: the output overlaps the array or the points");
  return vec ? wl::interp_points(arr, nullptr, G, x, n, out, ncomp, nullptr, 0, wl_stream(st))
             : wl::interp_points(nullptr, arr, G, x, n, nullptr, 0, out, 1, wl_stream(st));
}
int wl_advect(float* x, float* x_prev, const float* u0, const float* u1, const wl_grid* g, size_t n, float dt, unsigned perdir_mask, void* st) {
  WL_CHECK(wl_grid_ok(g), "bad wl_grid"); WL_TRY(wl_ctx_ensure());
  return wl::advect(x, x_prev, u0, u1, gx(*g), n, dt, perdir_mask, wl_stream(st));
}
}  // extern "C"
