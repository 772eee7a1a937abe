// Closed-form body helpers of the measure!/force kernels (wl_bodyset.hip, wl_forces.hip; device code, gfx950) and the host side of a body program.
#pragma once
#include "wl_common.hpp"
#include "wl_lattice.hpp"

namespace {
// BDIM kernel moments   src/Body.jl:54-60
__device__ __forceinline__ float kern_(float d) { return (1 + cosf(3.14159265358979323846f * d)) / 2; }
__device__ __forceinline__ float kern0_(float d) { return (1 + d + sinf(3.14159265358979323846f * d) / 3.14159265358979323846f) / 2; }
__device__ __forceinline__ float kern1_(float d) { return (1 - d * d) / 4 - (d * sinf(3.14159265358979323846f * d) + (1 + cosf(3.14159265358979323846f * d)) / 3.14159265358979323846f) / (2 * 3.14159265358979323846f); }
__device__ __forceinline__ float eps_at(float d) { d = fabsf(d); return d == 0.f ? 1.4e-45f : nextafterf(d, INFINITY) - d; }
__device__ __forceinline__ float mu0_(float d, float e) { return d / e < -1 + sqrtf(eps_at(d)) ? 0.f : kern0_(fminf(d / e, 1.f)); }
__device__ __forceinline__ float mu1_(float d, float e) { return e * kern1_(fminf(fmaxf(d / e, -1.f), 1.f)); }
// Closed-form AutoBody (src/AutoBody.jl:21,29-37): kind 1 sdf = |m∘(x−c)|−R (sphere/circle; an axis with m=0 is dropped: cylinder
// along it), kind 2 sdf = m·(x−c) (plane, m need not be unit).  The map x−V·t is folded into c by the caller.
struct BodyArg { int kind; float c[3], R, m[3]; };
template <int D>
__device__ __forceinline__ float body_sdf(const BodyArg& b, const float* x) {
  float s = 0.f;
  if (b.kind == 2) { for (int q = 0; q < D; q++) s += b.m[q] * (x[q] - b.c[q]); return s; }
  for (int q = 0; q < D; q++) { const float dx = b.m[q] * (x[q] - b.c[q]); s += dx * dx; }
  return sqrtf(s) - b.R;
}
// measure(body,x;fastd²): returns true when n was evaluated (then V = the body's velocity), false on the early exits (n = V = 0)
template <int D>
__device__ __forceinline__ bool body_measure(const BodyArg& b, const float* x, float fastd2, float& d, float* n) {
  float rr = 0.f;
  for (int q = 0; q < D; q++) n[q] = 0.f;
  if (b.kind == 2) d = body_sdf<D>(b, x);
  else { float s = 0.f; for (int q = 0; q < D; q++) { const float dx = b.m[q] * (x[q] - b.c[q]); s += dx * dx; } rr = sqrtf(s); d = rr - b.R; }
  if (d * d > fastd2) return false;
  float gq[3]; bool nan = false;
  for (int q = 0; q < D; q++) { gq[q] = b.kind == 2 ? b.m[q] : (b.m[q] * (x[q] - b.c[q])) / rr; nan = nan || isnan(gq[q]); }
  if (nan) return false;
  float mm = 0.f; for (int q = 0; q < D; q++) mm += gq[q] * gq[q];
  mm = sqrtf(mm); d /= mm;
  for (int q = 0; q < D; q++) n[q] = gq[q] / mm;
  return true;
}
// cross(a,b) as the reference's broadcast stores it: the 3-D vector product, in 2-D the scalar a₁b₂−a₂b₁ in every component
template <int D>
__device__ __forceinline__ void cross_(const float* a, const float* b, float* o) {
  if (D == 2) { const float m = a[0] * b[1] - a[1] * b[0]; o[0] = m; o[1] = m; o[2] = 0.f; }
  else { o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0]; }
}
struct MomArg { int on; float x0[3]; };      // on: moments about x0 (pressure_moment / viscous_moment, src/Metrics.jl:169-188) instead of forces
}  // namespace

// A validated wl_bodyset as the kernels take it (by value, kernarg memory): components beyond D zeroed, capsule axes normalised; depth = the deepest the stack gets
// A WL_BODY_LATTICE leaf: node.h holds the BITS of its index into lat[] (an int32, read with __float_as_int: never arithmetic on it), m[0] = s; lat[] are the
// nlat distinct lattices of the program as bodyset_prepare resolved them; lat_margin = min over its lattice leaves of edge_min − |R| (wlhip.h: out of range)
// band_left, band_cell: of the lattice leaves over BANDED lattices the one with the smallest band − |R| − s·√D, its band − |R| and its s·√D (s: the spacing the
// lattice was baked at); band_left = ∞ when the program has none (wlhip.h: the band rule).  Host-side bookkeeping like lat_margin: no kernel reads them.
struct SetArg { int32_t n; int32_t leaf_root; int32_t depth; int32_t nlat; float lat_margin; wl_body_node node[WL_BODYSET_MAX]; LatRef lat[WL_LATTICE_MAX];
                float band_left; float band_cell; };
static_assert(sizeof(SetArg) + 256 < 4096, "a kernel's arguments (the program and at most 256 bytes besides) must stay under 4 KB");
namespace {
__host__ __device__ __forceinline__ BodyArg body_arg(const wl_body_node& b) {
  BodyArg a; a.kind = b.kind; a.R = b.R;
  for (int q = 0; q < 3; q++) { a.c[q] = b.c[q]; a.m[q] = b.m[q]; }
  return a;
}
}  // namespace
struct wl_comm;
namespace wl {
int bodyset_prepare(int D, const wl_bodyset* s, SetArg* out);      // WL_EINVAL (and the reason) for a malformed program
// The only way a wl_body reaches a kernel: the program of one unmapped leaf.  The body's translation velocity travels in node[0].map.V (a leaf's measure returns
// it where n was evaluated); bodyset_prepare keeps map zero for unmapped leaves, so there V = 0 as wlhip.h promises.  WL_EINVAL for a bad kind or a zero m.
int bodyset_from_body(int D, const wl_body* b, SetArg* out);
// A STORED program (the force recorder's band, the immediate force list) before a launch that uses it: every lattice it names is looked up again by id.
// WL_EINVAL when one has been destroyed since — no kernel is ever launched with a freed pointer.  A program without lattice leaves: nothing to do.
int bodyset_resolve(int D, SetArg* P);
// the out-of-range rule of wlhip.h: WL_EINVAL unless every lattice leaf of P keeps edge_min − |R| > need (a program without lattice leaves passes) and every
// leaf over a banded lattice band − |R| > need + s·√D; the message names the condition that failed and both numbers
int bodyset_lattice_margin(const SetArg& P, float need, const char* who);
int bodyset_measure_fields(float* sigma, float* mu0, float* mu1, float* V, const GridX& G, const SetArg& P, float eps, int exitBC, unsigned perdir, hipStream_t q);
int bodyset_force_partials(int which, const float* a, float nu, const GridX& G, const SetArg& P, const float* x0, dim3 grid, double* part, hipStream_t q);
// force/moment read-out: `partials` writes 3·grid.x Float64 partial sums, then the fixed-order finish, the sum over ranks and the read-back
int force_reduce_with(const GridX& G, const RedWs& ws, wl_comm* comm, double* out, hipStream_t q, const std::function<int(dim3, double*, hipStream_t)>& partials);
}  // namespace wl
