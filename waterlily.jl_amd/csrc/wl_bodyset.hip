// Composite bodies (include/wlhip.h wl_bodyset): closed-form leaves under rigid maps (src/RigidMap.jl, src/AutoBody.jl:29-37),
// combined by the set operations of src/Body.jl:91-107, evaluated as a postfix program.  measure! (src/Body.jl:28-51) in one pass
// over every element of σ, μ₀, μ₁, V, the force/moment partial sums (src/Metrics.jl:116-188) and a point probe.
//
// The program is a kernel argument (2 KB, kernarg memory): every node field is a scalar load and every branch on it is
// wave-uniform.  The evaluation stack is per lane, at most WL_BODYSET_STACK entries of (d, n, V) in registers.
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "wl_common.hpp"
#include "wl_body.hpp"
#include "wl_bodyset_dev.hpp"
#include "wl_comm.hpp"

namespace {
// measure!(flow,body;ϵ)   src/Body.jl:28-51 without the two BC! calls: every element of μ₀, μ₁, V and the interior of σ in one pass
// (the fill of :29 folded in).  Grid: every plane of the array.
template <int DS>
__global__ void __launch_bounds__(WL_BLOCK) k_measure_set(GridX g, float* __restrict__ sig, float* __restrict__ mu0, float* __restrict__ mu1, float* __restrict__ V, SetArg P, float e) {
  constexpr int D = DS_D, S = DS_S;
  int i, j; long m; int pz;
  wl_tile(g, m, pz);                                      // (the linear order of wl_tile_lin measured slower here: 2.67 against 2.18 ms at 512³)
  if (!cell_ij(g, m, i, j)) return;
  const int k = pz;
  const long o = m + (long)k * g.sz;
  float m0[3] = {1.f, 1.f, 1.f}, m1[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, vv[3] = {0.f, 0.f, 0.f};
  if (interior_ij(g, i, j) && k >= g.k0 && k < g.k1) {
    const int I[3] = {i + 1, j + 1, (D == 3) ? g.gk + k + 1 : 1};
    float x[3]; for (int q = 0; q < 3; q++) x[q] = (float)I[q] - 1.5f;
    const float d2 = (2 + e) * (2 + e);
    float dc;
    if (P.leaf_root) dc = leaf_sdf<D>(P.node[0], P.lat, x);
    else { float nq[3], vq[3]; set_measure<D, S>(P, x, d2, dc, nq, vq); }      // (d alone: no velocity samples read)
    sig[o] = dc;
    if (dc * dc < d2) {
#pragma unroll
      for (int a = 0; a < D; a++) {
        float xf[3]; for (int q = 0; q < 3; q++) xf[q] = x[q] - ((q == a) ? 0.5f : 0.f);
        float di, ni[3], vi[3];
        set_measure<D, S, DS_V>(P, xf, d2, di, ni, vi);
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
  if (cell_ij(g, m, i, j) && interior_ij(g, i, j)) {
    for (int k = g.k0 + pz; k < g.k1; k += nsl) {
      const int I[3] = {i + 1, j + 1, (D == 3) ? g.gk + k + 1 : 1};
      float x[3]; for (int q = 0; q < 3; q++) x[q] = (float)I[q] - 1.5f;
      float d, n[3], v[3]; set_measure<D, S>(P, x, 1.f, d, n, v);
      const float kk = kern_(fminf(fmaxf(d, -1.f), 1.f));
      const float pv = p[m + (long)k * g.sz];
      float t[3]; pforce_cell<D>(mo.on, mo.x0, pv, n, kk, x, t);
      for (int a = 0; a < D; a++) acc[a] += (double)t[a];
    }
  }
  const long b = blockIdx.x, nb = gridDim.x;
  for (int a = 0; a < 3; a++) { const double v = block_sum(acc[a]); if (threadIdx.x == 0) part[a * nb + b] = v; __syncthreads(); }
}
// … of a program that is one unmapped sphere or plane (every wl_body): the same terms without the evaluation stack and with the body as a 44-byte argument
// instead of the 2 KB program — 0.085 against 0.098 ms per read-out at 256³ (profiles/onebody_experiments.md); the viscous sums gain nothing from it
template <int D>
__global__ void __launch_bounds__(WL_BLOCK) k_pforce_body(GridX g, const float* __restrict__ p, BodyArg bd, MomArg mo, double* __restrict__ part) {
  int i, j; long m; int pz;
  wl_tile(g, m, pz);
  double acc[3] = {0, 0, 0};
  const int nsl = wl_nslots(g);
  if (cell_ij(g, m, i, j) && interior_ij(g, i, j)) {
    for (int k = g.k0 + pz; k < g.k1; k += nsl) {
      float x[3]; cell_centre<D>(g, i, j, k, x);
      float d, n[3]; body_measure<D>(bd, x, 1.f, d, n);
      const float kk = kern_(fminf(fmaxf(d, -1.f), 1.f));
      const float pv = p[m + (long)k * g.sz];
      float t[3]; pforce_cell<D>(mo.on, mo.x0, pv, n, kk, x, t);
      for (int a = 0; a < D; a++) acc[a] += (double)t[a];
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
  if (cell_ij(g, m, i, j) && interior_ij(g, i, j)) {
    for (int k = g.k0 + pz; k < g.k1; k += nsl) {
      const int I[3] = {i + 1, j + 1, (D == 3) ? g.gk + k + 1 : 1};
      float x[3]; for (int q = 0; q < 3; q++) x[q] = (float)I[q] - 1.5f;
      float d, n[3], v[3]; set_measure<D, S>(P, x, 1.f, d, n, v);
      const float kk = kern_(fminf(fmaxf(d, -1.f), 1.f));
      const long o = m + (long)k * g.sz;
      float t[3]; vforce_cell<D>(mo.on, mo.x0, u, g.cs, o, st, nu, n, kk, x, t);
      for (int a = 0; a < D; a++) acc[a] += (double)t[a];
    }
  }
  const long b = blockIdx.x, nb = gridDim.x;
  for (int a = 0; a < 3; a++) { const double v = block_sum(acc[a]); if (threadIdx.x == 0) part[a * nb + b] = v; __syncthreads(); }
}
__global__ void k_fin3(const double* __restrict__ part, int nb, double* __restrict__ out) {
  for (int a = 0; a < 3; a++) {
    double s = 0.0; for (int q = threadIdx.x; q < nb; q += WL_BLOCK) s += part[(long)a * nb + q];
    s = block_sum(s); if (threadIdx.x == 0) out[a] = s; __syncthreads();
  }
}
// measure(body,x;fastd²) at a list of points (x point-major)
template <int DS>
__global__ void __launch_bounds__(WL_BLOCK) k_points_set(SetArg P, const float* __restrict__ x, int npts, float fastd2, float* __restrict__ d, float* __restrict__ n, float* __restrict__ v) {
  constexpr int D = DS_D, S = DS_S;
  const int p = blockIdx.x * WL_BLOCK + threadIdx.x;
  if (p >= npts) return;
  float xp[3] = {0.f, 0.f, 0.f}; for (int q = 0; q < D; q++) xp[q] = x[(long)p * D + q];
  float dd, nn[3], vv[3]; set_measure<D, S, DS_V>(P, xp, fastd2, dd, nn, vv);
  d[p] = dd;
  for (int q = 0; q < D; q++) { n[(long)p * D + q] = nn[q]; v[(long)p * D + q] = vv[q]; }
}
}  // namespace

namespace wl {
// a WL_BODY_LATTICE leaf (wlhip.h): c the position of lattice coordinate 0, m[0] = s, R the offset, h the id -> the prepared node, its lattice in out->lat[]
static int prepare_lattice_leaf(int D, const wl_body_node& a, wl_body_node& b, SetArg* out) {
  WL_CHECK(a.m[0] > 0.f && std::isfinite(a.m[0]), "wl_body_node.m[0] (grid cells per sample interval of a lattice leaf) must be > 0");
  WL_CHECK(std::isfinite(a.R), "wl_body_node.R (offset of a lattice leaf) is not finite");
  WL_CHECK(a.h >= 1.f && a.h < 16777216.f && a.h == std::floor(a.h), "wl_body_node.h of a lattice leaf must hold a lattice id (a positive integer)");
  const int id = (int)a.h;
  int32_t slot = 0;
  while (slot < out->nlat && out->lat[slot].id != id) slot++;
  LatRef L; float edge = 0.f, band = 0.f, baked = 0.f;
  WL_TRY(wl::lattice_resolve(id, D, &L, &edge, &band, &baked));
  if (slot == out->nlat) {
    WL_CHECK(slot < WL_LATTICE_MAX, "wl_bodyset: more than WL_LATTICE_MAX lattices in one program");      // (guard: no more than that many are alive)
    out->lat[slot] = L; out->nlat++;
  }
  out->lat_margin = std::fmin(out->lat_margin, edge - std::fabs(a.R));
  if (band > 0.f) {      // a banded lattice (wlhip.h, band-limited baking): the leaf whose band − |R| − s·√D is smallest decides, s the spacing of the BAKE
    const float left = band - std::fabs(a.R), cell = baked * sqrtf((float)D);
    if (left - cell < out->band_left - out->band_cell) { out->band_left = left; out->band_cell = cell; }
  }
  b.m[0] = a.m[0]; b.m[1] = b.m[2] = 0.f;
  static_assert(sizeof(slot) == sizeof(b.h), "the slot index travels as the bits of h");
  std::memcpy(&b.h, &slot, sizeof(slot));
  return 0;
}
int bodyset_resolve(int D, SetArg* P) {
  // gen stays what it was when the program was stored: a tile list built from it belongs to that filling of the lattice, and the next build against a freshly
  // prepared program (ForceBand::build compares the bytes) then sees that the lattice has been re-filled in place since
  for (int q = 0; q < P->nlat; q++) { float edge; const int32_t gen = P->lat[q].gen; WL_TRY(wl::lattice_resolve(P->lat[q].id, D, &P->lat[q], &edge)); P->lat[q].gen = gen; }
  return 0;
}
int bodyset_lattice_margin(const SetArg& P, float need, const char* who) {
  const bool band_ok = P.nlat == 0 || P.band_left > need + P.band_cell;
  if (band_ok && (P.nlat == 0 || P.lat_margin > need)) return 0;
  if (P.lat_margin > need) {
    wl_set_error(std::string(who) + ": a banded lattice leaf's band − |R| = " + std::to_string(P.band_left) + " is not above need + s·√D = " + std::to_string(need) +
                 " + " + std::to_string(P.band_cell) + " = " + std::to_string(need + P.band_cell) +
                 " — a cell that reads a clipped sample could miss the early exit (wlhip.h, band-limited baking: the band rule)");
    return WL_EINVAL;
  }
  wl_set_error(std::string(who) + ": a lattice leaf's edge_min − |R| = " + std::to_string(P.lat_margin) + " is not above " + std::to_string(need) +
               " — a cell outside the lattice's box could miss the early exit (wlhip.h, sampled bodies: out of range)");
  return WL_EINVAL;
}
int bodyset_prepare(int D, const wl_bodyset* s, SetArg* out) {
  WL_CHECK(D == 2 || D == 3, "bad dimension");
  WL_CHECK(s, "null wl_bodyset");
  WL_CHECK(s->n >= 1 && s->n <= WL_BODYSET_MAX, "wl_bodyset.n must be 1..WL_BODYSET_MAX");
  *out = SetArg{}; out->lat_margin = INFINITY; out->band_left = INFINITY; out->band_cell = 0.f;
  out->n = s->n;
  int sp = 0;
  for (int i = 0; i < s->n; i++) {
    const wl_body_node& a = s->node[i];
    wl_body_node& b = out->node[i];
    b.op = a.op;
    if (a.op == WL_OP_LEAF) {
      WL_CHECK(a.kind == WL_BODY_SPHERE || a.kind == WL_BODY_PLANE || a.kind == WL_BODY_CAPSULE || a.kind == WL_BODY_LATTICE,
               "wl_body_node.kind must be WL_BODY_SPHERE, WL_BODY_PLANE, WL_BODY_CAPSULE or WL_BODY_LATTICE");
      b.kind = a.kind; b.R = a.R; b.h = a.h; b.mapped = a.mapped ? 1 : 0;
      float mm = 0.f;
      for (int q = 0; q < 3; q++) { b.c[q] = q < D ? a.c[q] : 0.f; b.m[q] = q < D ? a.m[q] : 0.f; mm += b.m[q] * b.m[q]; }
      WL_CHECK(mm > 0.f || a.kind == WL_BODY_LATTICE, "wl_body_node.m (axis mask / normal / capsule axis) is zero");
      if (a.kind == WL_BODY_LATTICE) {
        WL_TRY(prepare_lattice_leaf(D, a, b, out));
      } else if (a.kind == WL_BODY_CAPSULE) {
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
int bodyset_from_body(int D, const wl_body* b, SetArg* out) {
  WL_CHECK(b && (b->kind == WL_BODY_SPHERE || b->kind == WL_BODY_PLANE), "wl_body.kind must be WL_BODY_SPHERE or WL_BODY_PLANE");
  *out = SetArg{}; out->lat_margin = INFINITY; out->band_left = INFINITY; out->band_cell = 0.f;
  out->n = 1; out->leaf_root = 1; out->depth = 1;
  wl_body_node& nd = out->node[0];
  nd.op = WL_OP_LEAF; nd.kind = b->kind; nd.R = b->R;
  float mm = 0.f;
  for (int q = 0; q < 3; q++) {
    nd.c[q] = q < D ? b->c[q] : 0.f; nd.m[q] = q < D ? b->m[q] : 0.f; mm += nd.m[q] * nd.m[q];
    nd.map.V[q] = (q < D && b->V[q] != 0.f) ? b->V[q] : 0.f;      // (either zero becomes +0: measure! leaves the fill's +0 where the body does not move)
  }
  WL_CHECK(mm > 0.f, "wl_body.m (axis mask / plane normal) is zero");
  return 0;
}
int bodyset_measure_fields(float* sigma, float* mu0, float* mu1, float* V, const GridX& G, const SetArg& P, float eps, int exitBC, unsigned perdir, hipStream_t q) {
  WL_TRY(bodyset_lattice_margin(P, 2.f + eps + 1.f, "measure!"));      // every interior cell and face outside a lattice's box takes the early exit at fastd² = (2+ϵ)²
  BSELV(G.D, P.depth, setarg_has_velocity(P), k_measure_set, wl_plane_grid(G, G.nz), dim3(WL_BLOCK), 0, q, G, sigma, mu0, mu1, V, P, eps);
  WL_LAUNCH_CHECK();
  const float zero[3] = {0, 0, 0};
  WL_TRY(wl::bc_vec(mu0, G, zero, 0, perdir, q));                                                                                   // Body.jl:49
  return wl::bc_vec(V, G, zero, exitBC, perdir, q);                                                                                 // Body.jl:50
}
int bodyset_force_partials(int which, const float* a, float nu, const GridX& G, const SetArg& P, const float* x0, dim3 grid, double* part, hipStream_t q) {
  WL_TRY(bodyset_lattice_margin(P, 2.f, "force"));
  MomArg mo{}; if (x0) { mo.on = 1; for (int c = 0; c < G.D; c++) mo.x0[c] = x0[c]; }
  const wl_body_node& n0 = P.node[0];
  if (which == 0 && P.leaf_root && !n0.mapped && (n0.kind == WL_BODY_SPHERE || n0.kind == WL_BODY_PLANE)) {
    if (G.D == 3) hipLaunchKernelGGL(k_pforce_body<3>, grid, dim3(WL_BLOCK), 0, q, G, a, body_arg(n0), mo, part);
    else hipLaunchKernelGGL(k_pforce_body<2>, grid, dim3(WL_BLOCK), 0, q, G, a, body_arg(n0), mo, part);
  } else if (which == 0) { BSEL(G.D, P.depth, k_pforce_set, grid, dim3(WL_BLOCK), 0, q, G, a, P, mo, part); }
  else { BSEL(G.D, P.depth, k_vforce_set, grid, dim3(WL_BLOCK), 0, q, G, a, nu, P, mo, part); }
  WL_LAUNCH_CHECK();
  return 0;
}
// which: 0 pressure_force(p) (src/Metrics.jl:116-133), 1 viscous_force(u,ν) (:140-154); Float64 partial sums, flow.f untouched.
// On z-slabs every rank sums its own planes and the per-rank sums are added on device (one 128-byte all-gather).
int force_reduce_with(const GridX& G, const RedWs& ws, wl_comm* comm, double* out, hipStream_t q, const std::function<int(dim3, double*, hipStream_t)>& partials) {
  const int D = G.D;
  dim3 grid = wl_plane_grid(G, wl_red_slots(G, G.k1 - G.k0));
  // partials need 3*grid.x doubles (<= 3*WL_REDPART): pa and pb are contiguous (2*WL_MAXPART doubles)
  WL_TRY(partials(grid, ws.pa, q));
  hipLaunchKernelGGL(k_fin3, dim3(1), dim3(WL_BLOCK), 0, q, ws.pa, (int)grid.x, ws.res_d + WL_RD_FORCE);
  WL_LAUNCH_CHECK();
  WL_TRY(wl::combine_results(comm, ws, q));
  std::lock_guard<std::mutex> lock(wl::wl_read_mutex());
  WlCtx& cx = wl_ctx();
  WL_HIP(hipMemcpyAsync(cx.h_d, ws.res_d + WL_RD_FORCE, 3 * sizeof(double), hipMemcpyDeviceToHost, q));
  WL_HIP(hipStreamSynchronize(q));
  for (int c = 0; c < D; c++) out[c] = cx.h_d[c];
  return 0;
}
}  // namespace wl

// a force (x0 == NULL) or moment of the body program P on the caller's p (which = 0) or u (1), single domain, the library's workspace
static int force_on_arrays(int which, const float* a, float nu, const GridX& G, const SetArg& P, const float* x0, double* out, void* st) {
  return wl::force_reduce_with(G, wl_red_ws(wl_ctx().red), nullptr, out, wl_stream(st),
                               [&](dim3 grid, double* part, hipStream_t q) { return wl::bodyset_force_partials(which, a, nu, G, P, x0, grid, part, q); });
}
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
    BSELV(D, P.depth, setarg_has_velocity(P), k_points_set, dim3((unsigned)((npts + WL_BLOCK - 1) / WL_BLOCK)), dim3(WL_BLOCK), 0, q, P, dx, npts, fastd2, dd, dn, dv);
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
  return force_on_arrays(0, p, 0.f, gx(*g), P, x0, out, st);
}
int wl_viscous_force_bodyset(const float* x0, const float* u, const wl_grid* g, float nu, const wl_bodyset* set, double* out, void* st) {
  WL_CHECK(wl_grid_ok(g) && u && out, "bad wl_grid / u / out");
  SetArg P; WL_TRY(wl::bodyset_prepare(g->D, set, &P));
  WL_TRY(wl_ctx_ensure());
  return force_on_arrays(1, u, nu, gx(*g), P, x0, out, st);
}
// ---- the closed-form wl_body: the same calls on its one-leaf program
int wl_measure_body(float* sigma, float* mu0, float* mu1, float* V, const wl_grid* g, const wl_body* body, float eps, int exitBC, uint32_t perdir_mask, void* st) {
  WL_CHECK(wl_grid_ok(g), "bad wl_grid"); WL_CHECK(sigma && mu0 && mu1 && V, "null field");
  SetArg P; WL_TRY(wl::bodyset_from_body(g->D, body, &P));
  return wl::bodyset_measure_fields(sigma, mu0, mu1, V, gx(*g), P, eps, exitBC, perdir_mask, wl_stream(st));
}
static int body_force_on_arrays(int which, const float* a, float nu, const wl_grid* g, const wl_body* body, const float* x0, double* out, void* st) {
  WL_TRY(wl_ctx_ensure());
  SetArg P; WL_TRY(wl::bodyset_from_body(g->D, body, &P));
  return force_on_arrays(which, a, nu, gx(*g), P, x0, out, st);
}
int wl_pressure_force_body(const float* p, const wl_grid* g, const wl_body* body, double* out, void* st) {
  WL_CHECK(wl_grid_ok(g), "bad wl_grid"); return body_force_on_arrays(0, p, 0.f, g, body, nullptr, out, st);
}
int wl_viscous_force_body(const float* u, const wl_grid* g, float nu, const wl_body* body, double* out, void* st) {
  WL_CHECK(wl_grid_ok(g), "bad wl_grid"); return body_force_on_arrays(1, u, nu, g, body, nullptr, out, st);
}
int wl_pressure_moment_body(const float* x0, const float* p, const wl_grid* g, const wl_body* body, double* out, void* st) {
  WL_CHECK(wl_grid_ok(g) && x0, "bad wl_grid / x0"); return body_force_on_arrays(0, p, 0.f, g, body, x0, out, st);
}
int wl_viscous_moment_body(const float* x0, const float* u, const wl_grid* g, float nu, const wl_body* body, double* out, void* st) {
  WL_CHECK(wl_grid_ok(g) && x0, "bad wl_grid / x0"); return body_force_on_arrays(1, u, nu, g, body, x0, out, st);
}
}  // extern "C"
