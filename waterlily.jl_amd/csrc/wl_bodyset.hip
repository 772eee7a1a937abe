// Composite bodies (include/wlhip.h wl_bodyset): closed-form leaves under rigid maps (src/RigidMap.jl, src/AutoBody.jl:29-37),
// combined by the set operations of src/Body.jl:91-107, evaluated as a postfix program.  measure! (src/Body.jl:28-51) in one pass
// over every element of σ, μ₀, μ₁, V, the force/moment partial sums (src/Metrics.jl:116-188) and a point probe.
//
// The program is a kernel argument (2 KB, kernarg memory): every node field is a scalar load and every branch on it is
// wave-uniform.  The evaluation stack is per lane, at most WL_BODYSET_STACK entries of (d, n, V) in registers.
#include <cmath>
#include <vector>

#include "wl_common.hpp"
#include "wl_body.hpp"

namespace {
__device__ __forceinline__ bool cell_ij_(const GridX& g, long m, int& i, int& j) {
  if (m >= g.sz) return false;
  j = (int)(m / g.nx);
  i = (int)(m - (long)j * g.nx);
  return true;
}
__device__ __forceinline__ bool interior_ij_(const GridX& g, int i, int j) { return i >= 1 && i <= g.nx - 2 && j >= 1 && j <= g.ny - 2; }

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
// closed-form sdf of a leaf at the body-frame point ξ (src/AutoBody.jl:21)
template <int D>
__device__ __forceinline__ float leaf_sdf_at(const wl_body_node& b, const float* xi) {
  if (b.kind == WL_BODY_PLANE) { float s = 0.f; for (int q = 0; q < D; q++) s += b.m[q] * (xi[q] - b.c[q]); return s; }
  if (b.kind == WL_BODY_SPHERE) { float s = 0.f; for (int q = 0; q < D; q++) { const float dx = b.m[q] * (xi[q] - b.c[q]); s += dx * dx; } return sqrtf(s) - b.R; }
  float t = 0.f; for (int q = 0; q < D; q++) t += b.m[q] * (xi[q] - b.c[q]);
  t = fminf(fmaxf(t, -b.h), b.h);
  float s = 0.f; for (int q = 0; q < D; q++) { const float dx = xi[q] - (b.c[q] + t * b.m[q]); s += dx * dx; }
  return sqrtf(s) - b.R;
}
// raw sdf of a leaf at x: sdf(map(x)); an unmapped sphere/plane is body_sdf itself
template <int D>
__device__ __forceinline__ float leaf_sdf(const wl_body_node& b, const float* x) {
  if (!b.mapped) return b.kind == WL_BODY_CAPSULE ? leaf_sdf_at<D>(b, x) : body_sdf<D>(body_arg(b), x);
  float xi[3], bq[3];
  to_body_frame<D>(b, x, xi, bq);
  return leaf_sdf_at<D>(b, xi);
}
// measure(leaf,x;fastd²) -> d, n, V (n = V = 0 on the early exits)   src/AutoBody.jl:29-37
template <int D>
__device__ __forceinline__ void leaf_measure(const wl_body_node& b, const float* x, float fastd2, float& d, float* n, float* v) {
  for (int q = 0; q < 3; q++) { n[q] = 0.f; v[q] = 0.f; }
  if (!b.mapped && b.kind != WL_BODY_CAPSULE) {          // exactly wl_body's measure (V = 0)
    BodyArg ba; ba.kind = b.kind; ba.R = b.R;
    for (int q = 0; q < 3; q++) { ba.c[q] = b.c[q]; ba.m[q] = b.m[q]; ba.V[q] = 0.f; }
    body_measure<D>(ba, x, fastd2, d, n);
    return;
  }
  float xi[3] = {x[0], x[1], x[2]}, bq[3] = {0.f, 0.f, 0.f};
  if (b.mapped) to_body_frame<D>(b, x, xi, bq);
  d = leaf_sdf_at<D>(b, xi);
  if (d * d > fastd2) return;
  float g[3] = {0.f, 0.f, 0.f}; bool nan = false;
  if (b.kind == WL_BODY_PLANE) { for (int q = 0; q < D; q++) g[q] = b.m[q]; }
  else if (b.kind == WL_BODY_SPHERE) {
    float s = 0.f; for (int q = 0; q < D; q++) { const float dx = b.m[q] * (xi[q] - b.c[q]); s += dx * dx; }
    const float rr = sqrtf(s);
    for (int q = 0; q < D; q++) g[q] = (b.m[q] * (xi[q] - b.c[q])) / rr;
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
}

// measure(body::SetBody,x;fastd²): the postfix program on a per-lane stack of S tuples (d,n,V).  The stack pointer is wave-uniform
// (it follows the program), so every access is an unrolled compare against a scalar: the stack lives in registers, never in scratch.
template <int D, int S>
__device__ __forceinline__ void set_measure(const SetArg& P, const float* x, float fastd2, float& d, float* n, float* v) {
  constexpr int W = 2 * D + 1;                            // tuple width
  float st[S][W];
  int sp = 0;
  for (int i = 0; i < P.n; i++) {
    const wl_body_node& nd = P.node[i];
    if (nd.op == WL_OP_LEAF) {
      float dd, nq[3], vq[3];
      leaf_measure<D>(nd, x, fastd2, dd, nq, vq);
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
// kernels are templated on DS = 16·D + S (dimension, stack slots) so that one DSEL-style macro picks the instantiation
#define DS_D (DS / 16)
#define DS_S (DS % 16)

// measure!(flow,body;ϵ)   src/Body.jl:28-51 without the two BC! calls: every element of μ₀, μ₁, V and the interior of σ in one pass
// (the fill of :29 folded in).  Grid: every plane of the array.
template <int DS>
__global__ void __launch_bounds__(WL_BLOCK) k_measure_set(GridX g, float* __restrict__ sig, float* __restrict__ mu0, float* __restrict__ mu1, float* __restrict__ V, SetArg P, float e) {
  constexpr int D = DS_D, S = DS_S;
  int i, j; long m; int pz;
  wl_tile(g, m, pz);                                      // (the linear order of wl_tile_lin measured slower here: 2.67 against 2.18 ms at 512³)
  if (!cell_ij_(g, m, i, j)) return;
  const int k = pz;
  const long o = m + (long)k * g.sz;
  float m0[3] = {1.f, 1.f, 1.f}, m1[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, vv[3] = {0.f, 0.f, 0.f};
  if (interior_ij_(g, i, j) && k >= g.k0 && k < g.k1) {
    const int I[3] = {i + 1, j + 1, (D == 3) ? g.gk + k + 1 : 1};
    float x[3]; for (int q = 0; q < 3; q++) x[q] = (float)I[q] - 1.5f;
    const float d2 = (2 + e) * (2 + e);
    float dc;
    if (P.leaf_root) dc = leaf_sdf<D>(P.node[0], x);
    else { float nq[3], vq[3]; set_measure<D, S>(P, x, d2, dc, nq, vq); }
    sig[o] = dc;
    if (dc * dc < d2) {
#pragma unroll
      for (int a = 0; a < D; a++) {
        float xf[3]; for (int q = 0; q < 3; q++) xf[q] = x[q] - ((q == a) ? 0.5f : 0.f);
        float di, ni[3], vi[3];
        set_measure<D, S>(P, xf, d2, di, ni, vi);
        di = fabsf(di) <= 0.5f ? di : copysignf(di, dc);
        vv[a] = vi[a];
        m0[a] = mu0_(di, e);
        for (int b = 0; b < D; b++) m1[a + b * D] = mu1_(di, e) * ni[b];
      }
    } else if (dc < 0.f) {
      for (int a = 0; a < D; a++) m0[a] = 0.f;
    }
  }
  for (int a = 0; a < D; a++) { V[(long)a * g.cs + o] = vv[a]; mu0[(long)a * g.cs + o] = m0[a]; }
  for (int q = 0; q < D * D; q++) mu1[(long)q * g.cs + o] = m1[q];
}

// pressure_force / pressure_moment with nds(body,x) = n·kern(clamp(d,−1,1)) at fastd² = 1   src/Metrics.jl:116-133,169-174
template <int DS>
__global__ void __launch_bounds__(WL_BLOCK) k_pforce_set(GridX g, const float* __restrict__ p, SetArg P, MomArg mo, double* __restrict__ part) {
  constexpr int D = DS_D, S = DS_S;
  int i, j; long m; int pz;
  wl_tile(g, m, pz);
  double acc[3] = {0, 0, 0};
  const int nsl = wl_nslots(g);
  if (cell_ij_(g, m, i, j) && interior_ij_(g, i, j)) {
    for (int k = g.k0 + pz; k < g.k1; k += nsl) {
      const int I[3] = {i + 1, j + 1, (D == 3) ? g.gk + k + 1 : 1};
      float x[3]; for (int q = 0; q < 3; q++) x[q] = (float)I[q] - 1.5f;
      float d, n[3], v[3]; set_measure<D, S>(P, x, 1.f, d, n, v);
      const float kk = kern_(fminf(fmaxf(d, -1.f), 1.f));
      const float pv = p[m + (long)k * g.sz];
      if (mo.on) {
        float nds[3] = {0.f, 0.f, 0.f}, rr[3] = {0.f, 0.f, 0.f}, cr[3];
        for (int a = 0; a < D; a++) { nds[a] = n[a] * kk; rr[a] = x[a] - mo.x0[a]; }
        cross_<D>(rr, nds, cr);
        for (int a = 0; a < D; a++) acc[a] += (double)(pv * cr[a]);
      } else {
        for (int a = 0; a < D; a++) acc[a] += (double)(pv * (n[a] * kk));
      }
    }
  }
  const long b = blockIdx.x, nb = gridDim.x;
  for (int a = 0; a < 3; a++) { const double v = block_sum(acc[a]); if (threadIdx.x == 0) part[a * nb + b] = v; __syncthreads(); }
}
// viscous_force / viscous_moment   src/Metrics.jl:140-154,181-188
template <int DS>
__global__ void __launch_bounds__(WL_BLOCK) k_vforce_set(GridX g, const float* __restrict__ u, float nu, SetArg P, MomArg mo, double* __restrict__ part) {
  constexpr int D = DS_D, S = DS_S;
  int i, j; long m; int pz;
  wl_tile(g, m, pz);
  double acc[3] = {0, 0, 0};
  const long st[3] = {1, g.sy, g.sz};
  const int nsl = wl_nslots(g);
  if (cell_ij_(g, m, i, j) && interior_ij_(g, i, j)) {
    for (int k = g.k0 + pz; k < g.k1; k += nsl) {
      const int I[3] = {i + 1, j + 1, (D == 3) ? g.gk + k + 1 : 1};
      float x[3]; for (int q = 0; q < 3; q++) x[q] = (float)I[q] - 1.5f;
      float d, n[3], v[3]; set_measure<D, S>(P, x, 1.f, d, n, v);
      const float kk = kern_(fminf(fmaxf(d, -1.f), 1.f));
      const long o = m + (long)k * g.sz;
      auto du = [&](int a, int b) -> float {
        const float* __restrict__ f = u + (long)a * g.cs;
        if (a == b) return f[o + st[a]] - f[o];
        return (f[o + st[b]] + f[o + st[b] + st[a]] - f[o - st[b]] - f[o - st[b] + st[a]]) / 4;
      };
      if (mo.on) {
        float sn[3] = {0.f, 0.f, 0.f}, rr[3] = {0.f, 0.f, 0.f}, cr[3];
        for (int a = 0; a < D; a++) {
          float vs = 0.f;
          for (int b = 0; b < D; b++) { const float Sab = (du(a, b) + du(b, a)) / 2; vs += Sab * (n[b] * kk); }
          sn[a] = vs; rr[a] = x[a] - mo.x0[a];
        }
        cross_<D>(rr, sn, cr);
        for (int a = 0; a < D; a++) acc[a] += (double)((-2 * nu) * cr[a]);
      } else {
        for (int a = 0; a < D; a++) {
          float vs = 0.f;
          for (int b = 0; b < D; b++) { const float Sab = (du(a, b) + du(b, a)) / 2; vs += ((-2 * nu) * Sab) * (n[b] * kk); }
          acc[a] += (double)vs;
        }
      }
    }
  }
  const long b = blockIdx.x, nb = gridDim.x;
  for (int a = 0; a < 3; a++) { const double v = block_sum(acc[a]); if (threadIdx.x == 0) part[a * nb + b] = v; __syncthreads(); }
}
// measure(body,x;fastd²) at a list of points (x point-major)
template <int DS>
__global__ void __launch_bounds__(WL_BLOCK) k_points_set(SetArg P, const float* __restrict__ x, int npts, float fastd2, float* __restrict__ d, float* __restrict__ n, float* __restrict__ v) {
  constexpr int D = DS_D, S = DS_S;
  const int p = blockIdx.x * WL_BLOCK + threadIdx.x;
  if (p >= npts) return;
  float xp[3] = {0.f, 0.f, 0.f}; for (int q = 0; q < D; q++) xp[q] = x[(long)p * D + q];
  float dd, nn[3], vv[3]; set_measure<D, S>(P, xp, fastd2, dd, nn, vv);
  d[p] = dd;
  for (int q = 0; q < D; q++) { n[(long)p * D + q] = nn[q]; v[(long)p * D + q] = vv[q]; }
}
}  // namespace

// instantiations: stack of 2 (every left-deep chain a∘b∘c∘…, a single leaf) or WL_BODYSET_STACK slots
#define BSEL(D, S, KERN, ...)                                                                                                        \
  do {                                                                                                                                \
    if ((D) == 3) { if ((S) <= 2) hipLaunchKernelGGL(KERN<50>, __VA_ARGS__); else hipLaunchKernelGGL(KERN<48 + WL_BODYSET_STACK>, __VA_ARGS__); } \
    else { if ((S) <= 2) hipLaunchKernelGGL(KERN<34>, __VA_ARGS__); else hipLaunchKernelGGL(KERN<32 + WL_BODYSET_STACK>, __VA_ARGS__); }           \
  } while (0)

namespace wl {
int bodyset_prepare(int D, const wl_bodyset* s, SetArg* out) {
  WL_CHECK(D == 2 || D == 3, "bad dimension");
  WL_CHECK(s, "null wl_bodyset");
  WL_CHECK(s->n >= 1 && s->n <= WL_BODYSET_MAX, "wl_bodyset.n must be 1..WL_BODYSET_MAX");
  *out = SetArg{};
  out->n = s->n;
  int sp = 0;
  for (int i = 0; i < s->n; i++) {
    const wl_body_node& a = s->node[i];
    wl_body_node& b = out->node[i];
    b.op = a.op;
    if (a.op == WL_OP_LEAF) {
      WL_CHECK(a.kind == WL_BODY_SPHERE || a.kind == WL_BODY_PLANE || a.kind == WL_BODY_CAPSULE, "wl_body_node.kind must be WL_BODY_SPHERE, WL_BODY_PLANE or WL_BODY_CAPSULE");
      b.kind = a.kind; b.R = a.R; b.h = a.h; b.mapped = a.mapped ? 1 : 0;
      float mm = 0.f;
      for (int q = 0; q < 3; q++) { b.c[q] = q < D ? a.c[q] : 0.f; b.m[q] = q < D ? a.m[q] : 0.f; mm += b.m[q] * b.m[q]; }
      WL_CHECK(mm > 0.f, "wl_body_node.m (axis mask / normal / capsule axis) is zero");
      if (a.kind == WL_BODY_CAPSULE) {
        WL_CHECK(a.h >= 0.f, "wl_body_node.h (capsule half-length) must be >= 0");
        const float l = sqrtf(mm);
        for (int q = 0; q < D; q++) b.m[q] = b.m[q] / l;
      } else {
        b.h = 0.f;
      }
      if (b.mapped) {
        for (int q = 0; q < 3; q++) {
          b.map.x0[q] = q < D ? a.map.x0[q] : 0.f; b.map.xp[q] = q < D ? a.map.xp[q] : 0.f; b.map.V[q] = q < D ? a.map.V[q] : 0.f;
          b.map.w[q] = (D == 3 || q == 0) ? a.map.w[q] : 0.f;
          for (int r = 0; r < 3; r++) b.map.R[q * 3 + r] = (q < D && r < D) ? a.map.R[q * 3 + r] : 0.f;
        }
      }
      sp++;
      out->depth = sp > out->depth ? sp : out->depth;
      WL_CHECK(sp <= WL_BODYSET_STACK, "wl_bodyset: evaluation stack deeper than WL_BODYSET_STACK");
    } else if (a.op == WL_OP_NEGATE) {
      WL_CHECK(sp >= 1, "wl_bodyset: stack underflow (NEGATE)");
    } else if (a.op == WL_OP_UNION || a.op == WL_OP_INTERSECT) {
      WL_CHECK(sp >= 2, "wl_bodyset: stack underflow (UNION/INTERSECT)");
      sp--;
    } else {
      WL_CHECK(false, "wl_body_node.op must be WL_OP_LEAF, WL_OP_UNION, WL_OP_INTERSECT or WL_OP_NEGATE");
    }
  }
  WL_CHECK(sp == 1, "wl_bodyset: the program must leave exactly one value on the stack");
  out->leaf_root = s->n == 1 ? 1 : 0;
  return 0;
}
int bodyset_measure_fields(float* sigma, float* mu0, float* mu1, float* V, const GridX& G, const SetArg& P, float eps, int exitBC, unsigned perdir, hipStream_t q) {
  BSEL(G.D, P.depth, k_measure_set, wl_plane_grid(G, G.nz), dim3(WL_BLOCK), 0, q, G, sigma, mu0, mu1, V, P, eps);
  WL_LAUNCH_CHECK();
  const float zero[3] = {0, 0, 0};
  WL_TRY(wl::bc_vec(mu0, G, zero, 0, perdir, q));                                                                                   // Body.jl:49
  return wl::bc_vec(V, G, zero, exitBC, perdir, q);                                                                                 // Body.jl:50
}
int bodyset_force_partials(int which, const float* a, float nu, const GridX& G, const SetArg& P, const float* x0, dim3 grid, double* part, hipStream_t q) {
  MomArg mo{}; if (x0) { mo.on = 1; for (int c = 0; c < G.D; c++) mo.x0[c] = x0[c]; }
  if (which == 0) { BSEL(G.D, P.depth, k_pforce_set, grid, dim3(WL_BLOCK), 0, q, G, a, P, mo, part); }
  else { BSEL(G.D, P.depth, k_vforce_set, grid, dim3(WL_BLOCK), 0, q, G, a, nu, P, mo, part); }
  WL_LAUNCH_CHECK();
  return 0;
}
}  // namespace wl

extern "C" {
int wl_bodyset_measure_points(const wl_bodyset* set, int D, const float* hx, int npts, float fastd2, float* hd, float* hn, float* hV, void* st) {
  SetArg P; WL_TRY(wl::bodyset_prepare(D, set, &P));
  WL_CHECK(npts >= 0 && (npts == 0 || (hx && hd && hn && hV)), "bad points");
  if (npts == 0) return 0;
  WL_TRY(wl_ctx_ensure());
  hipStream_t q = wl_stream(st);
  const size_t nx = (size_t)npts * D;
  float* buf = (float*)wl_scratch(sizeof(float) * (2 * nx + nx + npts));   // (no allocation or free per call: hipFree would wait for every stream of the device)
  if (!buf) return (int)hipErrorOutOfMemory;
  float *dx = buf, *dn = buf + nx, *dv = buf + 2 * nx, *dd = buf + 3 * nx;
  int rc = 0;
  auto run = [&]() -> int {
    WL_HIP(hipMemcpyAsync(dx, hx, sizeof(float) * nx, hipMemcpyHostToDevice, q));
    BSEL(D, P.depth, k_points_set, dim3((unsigned)((npts + WL_BLOCK - 1) / WL_BLOCK)), dim3(WL_BLOCK), 0, q, P, dx, npts, fastd2, dd, dn, dv);
    WL_LAUNCH_CHECK();
    WL_HIP(hipMemcpyAsync(hd, dd, sizeof(float) * npts, hipMemcpyDeviceToHost, q));
    WL_HIP(hipMemcpyAsync(hn, dn, sizeof(float) * nx, hipMemcpyDeviceToHost, q));
    WL_HIP(hipMemcpyAsync(hV, dv, sizeof(float) * nx, hipMemcpyDeviceToHost, q));
    WL_HIP(hipStreamSynchronize(q));
    return 0;
  };
  rc = run();
  return rc;
}
int wl_measure_bodyset(float* sigma, float* mu0, float* mu1, float* V, const wl_grid* g, const wl_bodyset* set, float eps, int exitBC, uint32_t perdir_mask, void* st) {
  WL_CHECK(wl_grid_ok(g), "bad wl_grid"); WL_CHECK(sigma && mu0 && mu1 && V, "null field");
  SetArg P; WL_TRY(wl::bodyset_prepare(g->D, set, &P));
  return wl::bodyset_measure_fields(sigma, mu0, mu1, V, gx(*g), P, eps, exitBC, perdir_mask, wl_stream(st));
}
int wl_pressure_force_bodyset(const float* x0, const float* p, const wl_grid* g, const wl_bodyset* set, double* out, void* st) {
  WL_CHECK(wl_grid_ok(g) && p && out, "bad wl_grid / p / out");
  SetArg P; WL_TRY(wl::bodyset_prepare(g->D, set, &P));
  WL_TRY(wl_ctx_ensure());
  const GridX G = gx(*g);
  return wl::force_reduce_with(G, wl_red_ws(wl_ctx().red), nullptr, out, wl_stream(st),
                               [&](dim3 grid, double* part, hipStream_t q) { return wl::bodyset_force_partials(0, p, 0.f, G, P, x0, grid, part, q); });
}
int wl_viscous_force_bodyset(const float* x0, const float* u, const wl_grid* g, float nu, const wl_bodyset* set, double* out, void* st) {
  WL_CHECK(wl_grid_ok(g) && u && out, "bad wl_grid / u / out");
  SetArg P; WL_TRY(wl::bodyset_prepare(g->D, set, &P));
  WL_TRY(wl_ctx_ensure());
  const GridX G = gx(*g);
  return wl::force_reduce_with(G, wl_red_ws(wl_ctx().red), nullptr, out, wl_stream(st),
                               [&](dim3 grid, double* part, hipStream_t q) { return wl::bodyset_force_partials(1, u, nu, G, P, x0, grid, part, q); });
}
}  // extern "C"
