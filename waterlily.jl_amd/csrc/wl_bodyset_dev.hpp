// Device side of the composite bodies (wl_bodyset.hip) for every file whose kernels evaluate a body program: the leaves, the postfix evaluation
// and the per-cell force and moment terms.  Device code only (gfx950); include after wl_body.hpp.
#pragma once
#include <cmath>

#include "wl_common.hpp"
#include "wl_body.hpp"

namespace {
// Julia's isless / isequal on Float32: NaN after everything, −0 before +0
__device__ __forceinline__ bool jl_isless(float a, float b) {
  if (isnan(a) || isnan(b)) return !isnan(a) && isnan(b);
  if (a == b) return signbit(a) && !signbit(b);
  return a < b;
}
__device__ __forceinline__ bool jl_isequal(float a, float b) {
  if (isnan(a) || isnan(b)) return isnan(a) && isnan(b);
  return a == b && signbit(a) == signbit(b);
}

// body-frame point ξ = R̂(x−x₀−xₚ)+xₚ of a mapped leaf (b = x−x₀−xₚ is kept for the velocity)   src/RigidMap.jl:37
template <int D>
__device__ __forceinline__ void to_body_frame(const wl_body_node& nd, const float* x, float* xi, float* b) {
  for (int q = 0; q < D; q++) b[q] = (x[q] - nd.map.x0[q]) - nd.map.xp[q];
  for (int q = 0; q < D; q++) { float s = 0.f; for (int r = 0; r < D; r++) s += nd.map.R[q * 3 + r] * b[r]; xi[q] = s + nd.map.xp[q]; }
}
// sdf of a leaf at the body-frame point ξ (src/AutoBody.jl:21): closed form, or sampled from lat[] for a lattice leaf (wl_lattice.hpp)
template <int D>
__device__ __forceinline__ float leaf_sdf_at(const wl_body_node& b, const LatRef* lat, const float* xi) {
  if (b.kind == WL_BODY_LATTICE) return lattice_sdf<D>(lat[__float_as_int(b.h)], b.c, b.m[0], b.R, xi);
  if (b.kind == WL_BODY_PLANE) { float s = 0.f; for (int q = 0; q < D; q++) s += b.m[q] * (xi[q] - b.c[q]); return s; }
  if (b.kind == WL_BODY_SPHERE) { float s = 0.f; for (int q = 0; q < D; q++) { const float dx = b.m[q] * (xi[q] - b.c[q]); s += dx * dx; } return sqrtf(s) - b.R; }
  float t = 0.f; for (int q = 0; q < D; q++) t += b.m[q] * (xi[q] - b.c[q]);
  t = fminf(fmaxf(t, -b.h), b.h);
  float s = 0.f; for (int q = 0; q < D; q++) { const float dx = xi[q] - (b.c[q] + t * b.m[q]); s += dx * dx; }
  return sqrtf(s) - b.R;
}
// raw sdf of a leaf at x: sdf(map(x)); an unmapped sphere/plane is body_sdf itself
template <int D>
__device__ __forceinline__ float leaf_sdf(const wl_body_node& b, const LatRef* lat, const float* x) {
  if (!b.mapped) return (b.kind == WL_BODY_SPHERE || b.kind == WL_BODY_PLANE) ? body_sdf<D>(body_arg(b), x) : leaf_sdf_at<D>(b, lat, x);
  float xi[3], bq[3];
  to_body_frame<D>(b, x, xi, bq);
  return leaf_sdf_at<D>(b, lat, xi);
}
// measure(leaf,x;fastd²) -> d, n, V (n = V = 0 on the early exits)   src/AutoBody.jl:29-37.  VEL: the instantiation that adds a lattice's velocity samples to V —
// launched only for a program that names a lattice which has some (setarg_has_velocity), and never by the force kernels, which do not read V: every other
// launch runs the statements it ran before the samples existed
template <int D, bool VEL>
__device__ __forceinline__ void leaf_measure(const wl_body_node& b, const LatRef* lat, const float* x, float fastd2, float& d, float* n, float* v) {
  for (int q = 0; q < 3; q++) { n[q] = 0.f; v[q] = 0.f; }
  if (!b.mapped && (b.kind == WL_BODY_SPHERE || b.kind == WL_BODY_PLANE)) {          // the closed-form wl_body: V = its translation velocity (wl::bodyset_from_body; 0 in every public program)
    if (body_measure<D>(body_arg(b), x, fastd2, d, n)) for (int q = 0; q < D; q++) v[q] = b.map.V[q];
    return;
  }
  float xi[3] = {x[0], x[1], x[2]}, bq[3] = {0.f, 0.f, 0.f};
  if (b.mapped) to_body_frame<D>(b, x, xi, bq);
  d = leaf_sdf_at<D>(b, lat, xi);
  if (d * d > fastd2) return;
  float g[3] = {0.f, 0.f, 0.f}; bool nan = false;
  float wx[3] = {0.f, 0.f, 0.f}; bool hasw = false;        // a lattice leaf with velocity samples: ωξ, sampled with the gradient (one cell, one set of weights)
  if (b.kind == WL_BODY_PLANE) { for (int q = 0; q < D; q++) g[q] = b.m[q]; }
  else if (b.kind == WL_BODY_SPHERE) {
    float s = 0.f; for (int q = 0; q < D; q++) { const float dx = b.m[q] * (xi[q] - b.c[q]); s += dx * dx; }
    const float rr = sqrtf(s);
    for (int q = 0; q < D; q++) g[q] = (b.m[q] * (xi[q] - b.c[q])) / rr;
  } else if (b.kind == WL_BODY_LATTICE) {                  // the one leaf whose |∇sdf| is whatever the samples say: d /= m below does real work
    if constexpr (VEL) hasw = lattice_grad_vel<D>(lat[__float_as_int(b.h)], b.c, b.m[0], xi, g, wx);
    else lattice_grad<D>(lat[__float_as_int(b.h)], b.c, b.m[0], xi, g);
  } else {
    float t = 0.f; for (int q = 0; q < D; q++) t += b.m[q] * (xi[q] - b.c[q]);
    t = fminf(fmaxf(t, -b.h), b.h);
    float dl[3] = {0.f, 0.f, 0.f}, s = 0.f; for (int q = 0; q < D; q++) { dl[q] = xi[q] - (b.c[q] + t * b.m[q]); s += dl[q] * dl[q]; }
    const float rr = sqrtf(s);
    for (int q = 0; q < D; q++) g[q] = dl[q] / rr;
  }
  for (int q = 0; q < D; q++) nan = nan || isnan(g[q]);
  if (nan) return;
  float nn[3] = {0.f, 0.f, 0.f};
  if (b.mapped) { for (int a = 0; a < D; a++) { float s = 0.f; for (int q = 0; q < D; q++) s += b.map.R[q * 3 + a] * g[q]; nn[a] = s; } }   // J'n
  else { for (int a = 0; a < D; a++) nn[a] = g[a]; }
  float mm = 0.f; for (int q = 0; q < D; q++) mm += nn[q] * nn[q];
  mm = sqrtf(mm); d /= mm;
  for (int q = 0; q < D; q++) n[q] = nn[q] / mm;
  if (b.mapped) {                                         // −J⁻¹∂ₜmap = V + ω×(x−x₀−xₚ)   src/RigidMap.jl:40-46
    if (D == 2) { v[0] = b.map.V[0] + b.map.w[0] * -bq[1]; v[1] = b.map.V[1] + b.map.w[0] * bq[0]; }
    else {
      v[0] = b.map.V[0] + (b.map.w[1] * bq[2] - b.map.w[2] * bq[1]);
      v[1] = b.map.V[1] + (b.map.w[2] * bq[0] - b.map.w[0] * bq[2]);
      v[2] = b.map.V[2] + (b.map.w[0] * bq[1] - b.map.w[1] * bq[0]);
    }
  }
  if (VEL && hasw) {                                      // a deforming surface: ẋ = R̂ᵀξ̇ + the rigid part (wave-uniform: the lattices are kernel arguments)
    if (b.mapped) { for (int a = 0; a < D; a++) { float s = 0.f; for (int q = 0; q < D; q++) s += b.map.R[q * 3 + a] * wx[q]; v[a] = v[a] + s; } }
    else { for (int a = 0; a < D; a++) v[a] = wx[a]; }
  }
}

// measure(body::SetBody,x;fastd²): the postfix program on a per-lane stack of S tuples (d,n,V).  The stack pointer is wave-uniform
// (it follows the program), so every access is an unrolled compare against a scalar: the stack lives in registers, never in scratch.
template <int D, int S, bool VEL = false>
__device__ __forceinline__ void set_measure(const SetArg& P, const float* x, float fastd2, float& d, float* n, float* v) {
  constexpr int W = 2 * D + 1;                            // tuple width
  float st[S][W];
  int sp = 0;
  for (int i = 0; i < P.n; i++) {
    const wl_body_node& nd = P.node[i];
    if (nd.op == WL_OP_LEAF) {
      float dd, nq[3], vq[3];
      leaf_measure<D, VEL>(nd, P.lat, x, fastd2, dd, nq, vq);
#pragma unroll
      for (int s = 0; s < S; s++)
        if (s == sp) { st[s][0] = dd; for (int q = 0; q < D; q++) { st[s][1 + q] = nq[q]; st[s][1 + D + q] = vq[q]; } }
      sp++;
    } else if (nd.op == WL_OP_NEGATE) {
#pragma unroll
      for (int s = 0; s < S; s++)
        if (s == sp - 1) for (int q = 0; q <= D; q++) st[s][q] = -st[s][q];
    } else {                                              // min / max on tuples: isless(b,a) ? b : a  /  isless(b,a) ? a : b
#pragma unroll
      for (int s = 1; s < S; s++)
        if (s == sp - 1) {
          bool less = false, eq = true;
          for (int q = 0; q < W; q++)
            if (eq) { less = jl_isless(st[s][q], st[s - 1][q]); eq = !less && jl_isequal(st[s][q], st[s - 1][q]); }
          const bool takeb = (nd.op == WL_OP_UNION) ? less : !less;
          if (takeb) for (int q = 0; q < W; q++) st[s - 1][q] = st[s][q];
        }
      sp--;
    }
  }
  d = st[0][0];
  for (int q = 0; q < 3; q++) { n[q] = q < D ? st[0][1 + q] : 0.f; v[q] = q < D ? st[0][1 + D + q] : 0.f; }
}

// The Float32 term ONE cell adds to a force or moment sum (src/Metrics.jl:116-188) — the statements of k_pforce_set / k_vforce_set, shared with the
// one-pass band kernel of wl_forces.hip so that both accumulate the same numbers.  mom = 0: the force; mom != 0: the moment about x0.
//   pressure: p[I]·nds  /  p[I]·cross(x−x₀, nds),  nds = n·kern(clamp(d,−1,1))
template <int D>
__device__ __forceinline__ void pforce_cell(int mom, const float* x0, float pv, const float* n, float kk, const float* x, float* t) {
  if (mom) {
    float nds[3] = {0.f, 0.f, 0.f}, rr[3] = {0.f, 0.f, 0.f}, cr[3];
    for (int a = 0; a < D; a++) { nds[a] = n[a] * kk; rr[a] = x[a] - x0[a]; }
    cross_<D>(rr, nds, cr);
    for (int a = 0; a < D; a++) t[a] = pv * cr[a];
  } else {
    for (int a = 0; a < D; a++) t[a] = pv * (n[a] * kk);
  }
}
//   viscous: −2ν·S(I,u)·nds  /  −2ν·cross(x−x₀, S·nds),  S = (∇u+∇uᵀ)/2 from ∂(i,j,I,u) (:42-44) at the cell with offset o; st: the three strides
template <int D>
__device__ __forceinline__ void vforce_cell(int mom, const float* x0, const float* __restrict__ u, long cs, long o, const long* st, float nu, const float* n, float kk,
                                            const float* x, float* t) {
  auto du = [&](int a, int b) -> float {
    const float* __restrict__ f = u + (long)a * cs;
    if (a == b) return f[o + st[a]] - f[o];
    return (f[o + st[b]] + f[o + st[b] + st[a]] - f[o - st[b]] - f[o - st[b] + st[a]]) / 4;
  };
  if (mom) {
    float sn[3] = {0.f, 0.f, 0.f}, rr[3] = {0.f, 0.f, 0.f}, cr[3];
    for (int a = 0; a < D; a++) {
      float vs = 0.f;
      for (int b = 0; b < D; b++) { const float Sab = (du(a, b) + du(b, a)) / 2; vs += Sab * (n[b] * kk); }
      sn[a] = vs; rr[a] = x[a] - x0[a];
    }
    cross_<D>(rr, sn, cr);
    for (int a = 0; a < D; a++) t[a] = (-2 * nu) * cr[a];
  } else {
    for (int a = 0; a < D; a++) {
      float vs = 0.f;
      for (int b = 0; b < D; b++) { const float Sab = (du(a, b) + du(b, a)) / 2; vs += ((-2 * nu) * Sab) * (n[b] * kk); }
      t[a] = vs;
    }
  }
}
// the centre of the cell with 0-based array indices (i, j, k): loc(0,I) with I the Julia index   src/core.jl:177
template <int D>
__device__ __forceinline__ void cell_centre(const GridX& g, int i, int j, int k, float* x) {
  const int I[3] = {i + 1, j + 1, (D == 3) ? g.gk + k + 1 : 1};
  for (int q = 0; q < 3; q++) x[q] = (float)I[q] - 1.5f;
}
}  // namespace
// kernels are templated on DS = 16·D + S (dimension, stack slots; + 64: the instantiation that reads a lattice's velocity samples) so that one DSEL-style
// macro picks the instantiation
#define DS_D ((DS / 16) % 4)
#define DS_S (DS % 16)
#define DS_V (DS / 64 != 0)
// whether a program names a lattice that carries velocity samples (host; the lattices as last resolved)
static inline bool setarg_has_velocity(const SetArg& P) { for (int q = 0; q < P.nlat; q++) if (P.lat[q].w) return true; return false; }

// instantiations: stack of 2 (every left-deep chain a∘b∘c∘…, a single leaf) or WL_BODYSET_STACK slots
#define BSEL(D, S, KERN, ...)                                                                                                        \
  do {                                                                                                                                \
    if ((D) == 3) { if ((S) <= 2) hipLaunchKernelGGL(KERN<50>, __VA_ARGS__); else hipLaunchKernelGGL(KERN<48 + WL_BODYSET_STACK>, __VA_ARGS__); } \
    else { if ((S) <= 2) hipLaunchKernelGGL(KERN<34>, __VA_ARGS__); else hipLaunchKernelGGL(KERN<32 + WL_BODYSET_STACK>, __VA_ARGS__); }           \
  } while (0)
// … for the kernels that hand V on (measure!, the point probe): V != 0 picks the instantiations with the velocity samples
#define BSELV(D, S, V, KERN, ...)                                                                                                     \
  do {                                                                                                                                \
    if (!(V)) { BSEL(D, S, KERN, __VA_ARGS__); }                                                                                      \
    else if ((D) == 3) { if ((S) <= 2) hipLaunchKernelGGL(KERN<64 + 50>, __VA_ARGS__); else hipLaunchKernelGGL(KERN<64 + 48 + WL_BODYSET_STACK>, __VA_ARGS__); } \
    else { if ((S) <= 2) hipLaunchKernelGGL(KERN<64 + 34>, __VA_ARGS__); else hipLaunchKernelGGL(KERN<64 + 32 + WL_BODYSET_STACK>, __VA_ARGS__); }               \
  } while (0)
