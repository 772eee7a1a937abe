// Flow diagnostics of src/Metrics.jl:27-109 on the device: ke, ∂(i,j,I,u), λ₂, curl, ω, ω_mag, ω_θ, helicity, and their sums.
//
//   k_metrics<OUT>   one z-marching kernel for everything that is built from the cell-centred velocity-gradient tensor
//                    J[i][j] = ∂(i,j,I,u) (:42-44): ke (:33-35), ω (:74), ω_mag (:80), ω_θ (:87-91), λ₂ (:54-58) — OUT is the
//                    compile-time set of outputs — and, with no field store, the sums Σke, Σ½|ω|², max|ω| (M_STATS).
//                    A 256-thread workgroup owns a 64×8-cell tile of the x-y plane (two rows per thread) and walks a chunk of
//                    z-planes.  The three components of planes k−1, k, k+1 (+ the plane being filled) live in a four-slot LDS ring
//                    with a one-cell halo: every u value is fetched from global memory once per tile (+ halo), the loads of plane
//                    k+2 are issued before plane k's arithmetic and stay in flight across it, one barrier per plane.  Every
//                    stencil operand is an LDS read at an immediate offset from one per-thread base.
//                    Own bytes: 12 B/cell read + 4 B per scalar field written.
//   k_curl           curl(i,I,u) (:68), the two-point EDGE stencil — element-wise, linear block order, 2-D (i = 3) and 3-D
//   k_helicity       helicity(I,u,ω) (:99-109) from a caller-supplied collocated ω — element-wise
//   k_ke2 / k_stats2 the 2-D forms: ke with two components; Σke, Σ½·curl(3)², max|curl(3)|
// Only inside cells are written (the reference's @inside); every read of an inside cell is in bounds (I±δⱼ+δᵢ ≤ N): no clamping.
// The differences are evaluated in the written order of :42-44 ((a+b−c)−d, then /4) — @fastmath leaves the reference's own
// association undefined — and nothing is contracted into FMAs, so that a field has the same bits whichever instantiation wrote it.
//
// λ₂: the tests bound its error by a multiple of eps32·‖S²+Ω²‖ in EVERY cell, the cells where the gradient nearly vanishes included (the
// TGV has such points).  Two things had to give for that (tests/test_gpu_metrics.py records the figures):
//   * the cross terms of the J that λ₂ uses are associated as ((a−c)+(b−d))/4 — differences of neighbouring values first, which are
//     exact or nearly so, instead of the written (a+b−c)−d whose first sum rounds at eps32·|u| ≫ eps32·|J| (@fastmath leaves the
//     association to the compiler in the reference, so both are the reference's statement); still float32, still the same loads;
//   * S, Ω and A = S²+Ω² are formed in float64 from that float32 J, and the middle eigenvalue is the trigonometric closed form in
//     float64.  In float32 the closed form loses half the digits of the middle eigenvalue wherever two eigenvalues coincide (acos near
//     ±1: every symmetry plane of the TGV, any locally 2-D or rigidly rotating region); in float64 the same loss leaves √eps64 ≈ 1.5e-8
//     relative to ‖A‖, below float32 resolution.  A float32 A alone costs ≈ 13 eps32·‖A‖ on the TGV's weak-gradient cells (NumPy model).
// A = q·I (A = 0 included) returns q exactly.  ω, ω_mag, ω_θ and the sums keep the written order (they equal the float32 NumPy yardstick).
#include "wl_common.hpp"

#pragma clang fp contract(off)

namespace {
enum : unsigned { M_KE = 1u, M_W = 2u, M_WMAG = 4u, M_L2 = 8u, M_WTH = 16u, M_STATS = 32u };

#define MT_TX 64                  // core cells (= threads) along x
#define MT_TY 4                   // thread rows
#define MT_RY 2                   // rows per thread: rows ly and ly + MT_TY (a wave stays on one row: LDS rows are read conflict-free)
#define MT_CY (MT_TY * MT_RY)     // 8 core rows
#define MT_W (MT_TX + 2)          // LDS row: core + one halo cell per side
#define MT_H (MT_CY + 2)
#define MT_P (MT_W * MT_H)        // floats per component-plane (660)
#define MT_SLOT (3 * MT_P)        // floats per plane slot
#define MT_NSLOT 4                // ring: planes k−1, k, k+1 are read while k+2 is written
#define MT_NLD ((MT_P + WL_BLOCK - 1) / WL_BLOCK)   // loads per thread, component and plane (3)
static_assert(MT_TX * MT_TY == WL_BLOCK, "one thread per cell of a half tile");

struct MetricsArgs {
  float *ke, *w, *wmag, *l2, *wth;     // outputs (those of OUT are non-null)
  float U[3];                          // ke: background flow
  float z[3], c[3];                    // ω_θ: axis and a point on it
  double *pa, *pb; float* pm;          // M_STATS: per-workgroup partials Σke, Σ½|ω|², max|ω|
};

// middle eigenvalue of the symmetric A (upper triangle given): trigonometric closed form
__device__ __forceinline__ float mt_mid_eig(double a00, double a01, double a02, double a11, double a12, double a22) {
  const double q = (a00 + a11 + a22) / 3.0;
  const double b00 = a00 - q, b11 = a11 - q, b22 = a22 - q;
  const double p2 = b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * (a01 * a01 + a02 * a02 + a12 * a12);
  if (!(p2 > 0.0)) return (float)q;                        // A = q·I: a triple eigenvalue (A = 0 gives exactly 0)
  const double p = sqrt(p2 / 6.0), ip = 1.0 / p;
  const double c00 = b00 * ip, c11 = b11 * ip, c22 = b22 * ip, c01 = a01 * ip, c02 = a02 * ip, c12 = a12 * ip;
  double r = 0.5 * (c00 * (c11 * c22 - c12 * c12) - c01 * (c01 * c22 - c12 * c02) + c02 * (c01 * c12 - c11 * c02));
  r = r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r);              // |det/2| ≤ 1 up to rounding
  const double phi = acos(r) / 3.0;                        // ∈ [0, π/3]: q + 2p·cos(φ + 2πm/3), m = 0 largest, 1 smallest, 2 middle
  return (float)(q + 2.0 * p * cos(phi - 2.0943951023931954923));
}

// λ₂(I,u) from the float32 J   src/Metrics.jl:54-58 — S, Ω, S²+Ω² and the eigenvalue in float64
__device__ __forceinline__ float mt_lambda2(const float (&J)[3][3]) {
  double S[3][3], W[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) { S[i][j] = ((double)J[i][j] + (double)J[j][i]) / 2; W[i][j] = ((double)J[i][j] - (double)J[j][i]) / 2; }
  double A[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = i; j < 3; j++) {
      double s = S[i][0] * S[0][j]; s += S[i][1] * S[1][j]; s += S[i][2] * S[2][j];
      double t = W[i][0] * W[0][j]; t += W[i][1] * W[1][j]; t += W[i][2] * W[2][j];
      A[i][j] = s + t;
    }
  return mt_mid_eig(A[0][0], A[0][1], A[0][2], A[1][1], A[1][2], A[2][2]);
}

// ke(I,u,U) from the two face values of each component   src/Metrics.jl:33-35
__device__ __forceinline__ float mt_ke3(float x0, float x1, float y0, float y1, float z0, float z1, const float* U) {
  const float a = x0 + x1 - 2 * U[0], b = y0 + y1 - 2 * U[1], c = z0 + z1 - 2 * U[2];
  return 0.125f * (a * a + b * b + c * c);
}
__device__ __forceinline__ float mt_norm2(float a, float b, float c) { return sqrtf(a * a + b * b + c * c); }   // norm2(x) = √(x'x) :6

// workgroup -> (tile, z-chunk) in linear order, as wl_tile_lin does for 256-cell chunks: block h takes tile h mod nb8 of chunk h / nb8
// (nb8 = the tile count rounded up to a multiple of 8, so that a tile position belongs to the same XCD in every chunk)
__device__ __forceinline__ bool mt_tile(const GridX& g, int& x0, int& y0, int& c) {
  const int ntx = (g.nx - 2 + MT_TX - 1) / MT_TX, nty = (g.ny - 2 + MT_CY - 1) / MT_CY;
  const unsigned nb8 = (unsigned)(((ntx * nty + 7) >> 3) << 3);
  const unsigned h = blockIdx.x;
  c = (int)(h / nb8);
  const int tl = (int)(h - (unsigned)c * nb8);
  x0 = 1 + (tl % ntx) * MT_TX; y0 = 1 + (tl / ntx) * MT_CY;
  return tl < ntx * nty;
}

template <unsigned OUT>
__global__ void __launch_bounds__(WL_BLOCK) k_metrics(GridX g, const float* __restrict__ u, int zchunk, MetricsArgs a) {
  __shared__ float lds[MT_NSLOT * MT_SLOT];
  int x0, y0, ch;
  const bool tile_ok = mt_tile(g, x0, y0, ch);
  const int ks = 1 + ch * zchunk, ke = (ks + zchunk < g.nz - 1) ? ks + zchunk : g.nz - 1;   // inside planes [ks, ke) ⊂ [1, nz−1)
  const int tid = threadIdx.x, lx = tid & (MT_TX - 1), ly = tid >> 6;
  double s_ke = 0.0, s_en = 0.0; float s_mx = 0.f;
  if (tile_ok && ks < ke) {                                  // block-uniform
    // loader: element e = tid + 256·q of the halo-inclusive 66×10 tile, the same for every component and plane
    long loff[MT_NLD]; bool lok[MT_NLD];
#pragma unroll
    for (int q = 0; q < MT_NLD; q++) {
      const int e = tid + q * WL_BLOCK, row = e / MT_W, col = e - row * MT_W;
      const int X = x0 - 1 + col, Y = y0 - 1 + row;          // ≥ 0; cells past the array are never read by an inside cell
      lok[q] = e < MT_P && X < g.nx && Y < g.ny;
      loff[q] = (long)Y * g.sy + X;
    }
    float st[3 * MT_NLD];
    auto load = [&](int k) {
#pragma unroll
      for (int cmp = 0; cmp < 3; cmp++)
#pragma unroll
        for (int q = 0; q < MT_NLD; q++) st[cmp * MT_NLD + q] = lok[q] ? u[(long)cmp * g.cs + (long)k * g.sz + loff[q]] : 0.f;
    };
    auto stage = [&](int k) {
      float* __restrict__ d = lds + (k & (MT_NSLOT - 1)) * MT_SLOT;
#pragma unroll
      for (int cmp = 0; cmp < 3; cmp++)
#pragma unroll
        for (int q = 0; q < MT_NLD; q++) if (tid + q * WL_BLOCK < MT_P) d[cmp * MT_P + tid + q * WL_BLOCK] = st[cmp * MT_NLD + q];
    };
    load(ks - 1); stage(ks - 1); load(ks); stage(ks); load(ks + 1); stage(ks + 1);      // ks+1 ≤ nz−1
    __syncthreads();
    const int x = x0 + lx;
    for (int k = ks; k < ke; k++) {
      const bool more = k + 1 < ke;                          // plane k+2 ≤ ke ≤ nz−1 exists and the next plane needs it
      if (more) load(k + 2);
      const float* __restrict__ Lm = lds + ((k - 1) & (MT_NSLOT - 1)) * MT_SLOT;
      const float* __restrict__ L0 = lds + (k & (MT_NSLOT - 1)) * MT_SLOT;
      const float* __restrict__ Lp = lds + ((k + 1) & (MT_NSLOT - 1)) * MT_SLOT;
#pragma unroll
      for (int r = 0; r < MT_RY; r++) {
        const int yl = ly + r * MT_TY, y = y0 + yl;
        if (x > g.nx - 2 || y > g.ny - 2) continue;           // not an inside cell
        const int ci = (yl + 1) * MT_W + lx + 1;
#define UX(L, dy, dx) (L)[ci + (dy) * MT_W + (dx)]
#define UY(L, dy, dx) (L)[MT_P + ci + (dy) * MT_W + (dx)]
#define UZ(L, dy, dx) (L)[2 * MT_P + ci + (dy) * MT_W + (dx)]
        const long o = (long)k * g.sz + (long)y * g.sy + x;
        const float ux0 = UX(L0, 0, 0), ux1 = UX(L0, 0, 1), uy0 = UY(L0, 0, 0), uy1 = UY(L0, 1, 0), uz0 = UZ(L0, 0, 0), uz1 = UZ(Lp, 0, 0);
        float kev = 0.f;
        if (OUT & (M_KE | M_STATS)) kev = mt_ke3(ux0, ux1, uy0, uy1, uz0, uz1, a.U);
        if (OUT & M_KE) a.ke[o] = kev;
        if (OUT & ~M_KE) {
          float J[3][3];                                      // J[i][j] = ∂(i,j,I,u)   :42-44
          J[0][1] = (UX(L0, 1, 0) + UX(L0, 1, 1) - UX(L0, -1, 0) - UX(L0, -1, 1)) / 4;
          J[0][2] = (UX(Lp, 0, 0) + UX(Lp, 0, 1) - UX(Lm, 0, 0) - UX(Lm, 0, 1)) / 4;
          J[1][0] = (UY(L0, 0, 1) + UY(L0, 1, 1) - UY(L0, 0, -1) - UY(L0, 1, -1)) / 4;
          J[1][2] = (UY(Lp, 0, 0) + UY(Lp, 1, 0) - UY(Lm, 0, 0) - UY(Lm, 1, 0)) / 4;
          J[2][0] = (UZ(L0, 0, 1) + UZ(Lp, 0, 1) - UZ(L0, 0, -1) - UZ(Lp, 0, -1)) / 4;
          J[2][1] = (UZ(L0, 1, 0) + UZ(Lp, 1, 0) - UZ(L0, -1, 0) - UZ(Lp, -1, 0)) / 4;
          J[0][0] = ux1 - ux0; J[1][1] = uy1 - uy0; J[2][2] = uz1 - uz0;
          // ω(I,u)ᵢ = ∂(k,j) − ∂(j,k), (j,k) the two directions after i   :74
          const float w0 = J[2][1] - J[1][2], w1 = J[0][2] - J[2][0], w2 = J[1][0] - J[0][1];
          if (OUT & M_W) { a.w[o] = w0; a.w[g.cs + o] = w1; a.w[2 * g.cs + o] = w2; }
          float wm = 0.f;
          if (OUT & (M_WMAG | M_STATS)) wm = mt_norm2(w0, w1, w2);                            // ω_mag :80
          if (OUT & M_WMAG) a.wmag[o] = wm;
          if (OUT & M_L2) {                                   // the same operands, neighbour differences first (see the head of the file)
            float Jp[3][3];
            Jp[0][1] = ((UX(L0, 1, 0) - UX(L0, -1, 0)) + (UX(L0, 1, 1) - UX(L0, -1, 1))) / 4;
            Jp[0][2] = ((UX(Lp, 0, 0) - UX(Lm, 0, 0)) + (UX(Lp, 0, 1) - UX(Lm, 0, 1))) / 4;
            Jp[1][0] = ((UY(L0, 0, 1) - UY(L0, 0, -1)) + (UY(L0, 1, 1) - UY(L0, 1, -1))) / 4;
            Jp[1][2] = ((UY(Lp, 0, 0) - UY(Lm, 0, 0)) + (UY(Lp, 1, 0) - UY(Lm, 1, 0))) / 4;
            Jp[2][0] = ((UZ(L0, 0, 1) - UZ(L0, 0, -1)) + (UZ(Lp, 0, 1) - UZ(Lp, 0, -1))) / 4;
            Jp[2][1] = ((UZ(L0, 1, 0) - UZ(L0, -1, 0)) + (UZ(Lp, 1, 0) - UZ(Lp, -1, 0))) / 4;
            Jp[0][0] = J[0][0]; Jp[1][1] = J[1][1]; Jp[2][2] = J[2][2];
            a.l2[o] = mt_lambda2(Jp);
          }
          if (OUT & M_WTH) {                                  // ω_θ(I,z,center,u) :87-91; loc(0,I) = I − 1.5 (Julia index) = index − 0.5 here
            const float r0 = ((float)x - 0.5f) - a.c[0], r1 = ((float)y - 0.5f) - a.c[1], r2 = ((float)k - 0.5f) - a.c[2];
            const float t0 = a.z[1] * r2 - a.z[2] * r1, t1 = a.z[2] * r0 - a.z[0] * r2, t2 = a.z[0] * r1 - a.z[1] * r0;      // z × r  :18
            const float n = mt_norm2(t0, t1, t2);
            a.wth[o] = n <= 1.401298464e-45f ? 0.f : (t0 * w0 + t1 * w1 + t2 * w2) / n;        // n ≤ eps(n) ⇔ n ∈ {0, the smallest subnormal}
          }
          if (OUT & M_STATS) {
            const float en = 0.5f * (w0 * w0 + w1 * w1 + w2 * w2);
            s_ke += (double)kev; s_en += (double)en; s_mx = fmaxf(s_mx, wm);
          }
        }
#undef UX
#undef UY
#undef UZ
      }
      if (more) stage(k + 2);                                // slot of plane k−2: every thread left it before the last barrier
      __syncthreads();
    }
  }
  if (OUT & M_STATS) {                                       // every workgroup of the launch writes its partial (empty ones: zeros)
    s_ke = block_sum(s_ke); s_en = block_sum(s_en); s_mx = block_max(s_mx);
    if (threadIdx.x == 0) { a.pa[blockIdx.x] = s_ke; a.pb[blockIdx.x] = s_en; a.pm[blockIdx.x] = s_mx; }
  }
}

// curl(i,I,u) = ∂(j,CI(I,k),u) − ∂(k,CI(I,j),u), (j,k) the two directions after i; ∂(a,CI(I,c),u) = u[I,c] − u[I−δₐ,c]   src/Metrics.jl:68, src/Flow.jl:1
__device__ __forceinline__ float mt_curl(const float* __restrict__ u, const GridX& g, long o, const long* st, int i) {
  const int j = (i + 1) % 3, k = (i + 2) % 3;
  const float* __restrict__ uk = u + (long)k * g.cs;
  const float* __restrict__ uj = u + (long)j * g.cs;
  return (uk[o] - uk[o - st[j]]) - (uj[o] - uj[o - st[k]]);
}
// inside cell of this thread in linear block order: one plane per slot (3-D: planes 1 … nz−2; 2-D: the plane)
__device__ __forceinline__ bool mt_inside_lin(const GridX& g, long& o) {
  long m; int pz;
  if (!wl_tile_lin(g, m, pz) || m >= g.sz) return false;
  const int j = (int)(m / g.nx), i = (int)(m - (long)j * g.nx);
  if (i < 1 || i > g.nx - 2 || j < 1 || j > g.ny - 2) return false;
  o = m + (g.D == 3 ? (long)(1 + pz) * g.sz : 0);
  return true;
}
__global__ void __launch_bounds__(WL_BLOCK) k_curl(GridX g, float* __restrict__ out, const float* __restrict__ u, int i) {
  long o;
  if (!mt_inside_lin(g, o)) return;
  const long st[3] = {1, g.sy, g.sz};
  out[o] = mt_curl(u, g, o, st, i);
}
// helicity(I,u,ω)   src/Metrics.jl:99-109
__global__ void __launch_bounds__(WL_BLOCK) k_helicity(GridX g, float* __restrict__ out, const float* __restrict__ u, const float* __restrict__ w) {
  long o;
  if (!mt_inside_lin(g, o)) return;
  const long st[3] = {1, g.sy, g.sz};
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < 3; d++) {
    const long s1 = st[(d + 1) % 3], s2 = st[(d + 2) % 3];
    const float* __restrict__ ud = u + (long)d * g.cs;
    const float* __restrict__ wd = w + (long)d * g.cs;
    const float umid = ud[o] + ud[o + st[d]];
    s += umid * wd[o]; s += umid * wd[o + s2]; s += umid * wd[o + s1]; s += umid * wd[o + s1 + s2];      // id1 outer, id2 inner
  }
  out[o] = s / 8;
}
__device__ __forceinline__ float mt_ke2(const float* __restrict__ u, const GridX& g, long o, const float* U) {
  const float a = u[o] + u[o + 1] - 2 * U[0], b = u[g.cs + o] + u[g.cs + o + g.sy] - 2 * U[1];
  return 0.125f * (a * a + b * b);
}
struct U3 { float v[3]; };
__global__ void __launch_bounds__(WL_BLOCK) k_ke2(GridX g, float* __restrict__ out, const float* __restrict__ u, U3 U) {
  long o;
  if (!mt_inside_lin(g, o)) return;
  out[o] = mt_ke2(u, g, o, U.v);
}
// 2-D sums: Σke, Σ½·curl(3)², max|curl(3)| over inside (grid-stride over the plane; one partial per workgroup)
__global__ void __launch_bounds__(WL_BLOCK) k_stats2(GridX g, const float* __restrict__ u, U3 U, double* __restrict__ pa, double* __restrict__ pb, float* __restrict__ pm) {
  const long st[3] = {1, g.sy, g.sz};
  double s_ke = 0.0, s_en = 0.0; float s_mx = 0.f;
  for (long m = (long)blockIdx.x * WL_BLOCK + threadIdx.x; m < g.sz; m += (long)gridDim.x * WL_BLOCK) {
    const int j = (int)(m / g.nx), i = (int)(m - (long)j * g.nx);
    if (i < 1 || i > g.nx - 2 || j < 1 || j > g.ny - 2) continue;
    const float c = mt_curl(u, g, m, st, 2);
    s_ke += (double)mt_ke2(u, g, m, U.v); s_en += (double)(0.5f * (c * c)); s_mx = fmaxf(s_mx, fabsf(c));
  }
  s_ke = block_sum(s_ke); s_en = block_sum(s_en); s_mx = block_max(s_mx);
  if (threadIdx.x == 0) { pa[blockIdx.x] = s_ke; pb[blockIdx.x] = s_en; pm[blockIdx.x] = s_mx; }
}
// finishing pass: the partials of one launch -> res_d[0], res_d[1], res_f[0]
__global__ void __launch_bounds__(WL_BLOCK) k_stats_final(const double* __restrict__ pa, const double* __restrict__ pb, const float* __restrict__ pm, int n,
                                                          double* __restrict__ res_d, float* __restrict__ res_f) {
  double a = 0.0, b = 0.0; float mx = 0.f;
  for (int q = threadIdx.x; q < n; q += WL_BLOCK) { a += pa[q]; b += pb[q]; mx = fmaxf(mx, pm[q]); }
  a = block_sum(a); b = block_sum(b); mx = block_max(mx);
  if (threadIdx.x == 0) { res_d[WL_RD_SUM] = a; res_d[WL_RD_SUM2] = b; res_f[WL_RF_LEAF] = mx; }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
bool mt_single(const GridX& g) { return g.D == 2 || (g.k0 == 1 && g.k1 == g.nz - 1 && g.gk == 0 && g.gnz == g.nz); }
bool mt_overlap(const float* out, long n_out, const float* u, const GridX& g) { return out < u + (long)g.D * g.cs && u < out + n_out; }
int mt_ntiles8(const GridX& g) { const int nt = ((g.nx - 2 + MT_TX - 1) / MT_TX) * ((g.ny - 2 + MT_CY - 1) / MT_CY); return ((nt + 7) >> 3) << 3; }
// planes per workgroup: 4 … 32, about 2048 workgroups on grids that allow it (the two planes loaded ahead of a chunk are its overhead);
// the per-workgroup partials of the sums must fit the reduction workspace
int mt_chunk(const GridX& g) {
  const long np = g.nz - 2, nb = mt_ntiles8(g);
  long c = np * nb / 2048; if (c < 4) c = 4; if (c > 32) c = 32; if (c > np) c = np;
  while ((np + c - 1) / c * nb > WL_MAXPART && c < np) c++;
  return (int)c;
}
#define MT_REJECT(cond, msg) do { if (cond) { wl_set_error(msg); return WL_EINVAL; } } while (0)
int mt_common(const char* who, const float* u, const GridX& g) {
  MT_REJECT(!u, std::string(who) + ": null velocity array");
  MT_REJECT(!mt_single(g), std::string(who) + ": z-slab grids are not supported (single domain only)");
  return 0;
}

template <unsigned OUT>
void mt_launch(const GridX& g, const float* u, const MetricsArgs& a, hipStream_t s, unsigned* nblocks = nullptr) {
  const int c = mt_chunk(g);
  const unsigned nb = (unsigned)(mt_ntiles8(g) * ((g.nz - 2 + c - 1) / c));
  hipLaunchKernelGGL(k_metrics<OUT>, dim3(nb), dim3(WL_BLOCK), 0, s, g, u, c, a);
  if (nblocks) *nblocks = nb;
}
void mt_set3(float* d, const float* s) { for (int q = 0; q < 3; q++) d[q] = s ? s[q] : 0.f; }
}  // namespace

namespace wl {
// ke / ω / ω_mag / λ₂ in one pass over u: any null output is skipped.  2-D: ke only.
int metrics_fields(const float* u, const GridX& g, const float* U, float* ke, float* w3, float* wmag, float* l2, hipStream_t s) {
  WL_TRY(mt_common("flow_fields", u, g));
  MT_REJECT(!ke && !w3 && !wmag && !l2, "flow_fields: every output is null");
  MT_REJECT(g.D != 3 && (w3 || wmag || l2), "flow_fields: ω, ω_mag and λ₂ are defined for 3-D grids only (CartesianIndex{3} methods, src/Metrics.jl:54,74,80)");
  MT_REJECT((ke && mt_overlap(ke, g.cs, u, g)) || (w3 && mt_overlap(w3, 3 * g.cs, u, g)) || (wmag && mt_overlap(wmag, g.cs, u, g)) || (l2 && mt_overlap(l2, g.cs, u, g)),
            "flow_fields: an output aliases the velocity array");
  if (g.D == 2) {
    U3 Uv; mt_set3(Uv.v, nullptr); if (U) { Uv.v[0] = U[0]; Uv.v[1] = U[1]; }
    hipLaunchKernelGGL(k_ke2, wl_plane_grid(g, 1), dim3(WL_BLOCK), 0, s, g, ke, u, Uv);
    WL_LAUNCH_CHECK(); return 0;
  }
  MetricsArgs a{}; a.ke = ke; a.w = w3; a.wmag = wmag; a.l2 = l2; mt_set3(a.U, U);
  const unsigned m = (ke ? M_KE : 0u) | (w3 ? M_W : 0u) | (wmag ? M_WMAG : 0u) | (l2 ? M_L2 : 0u);
  switch (m) {
#define MT_CASE(v) case v: mt_launch<v>(g, u, a, s); break;
    MT_CASE(1) MT_CASE(2) MT_CASE(3) MT_CASE(4) MT_CASE(5) MT_CASE(6) MT_CASE(7) MT_CASE(8)
    MT_CASE(9) MT_CASE(10) MT_CASE(11) MT_CASE(12) MT_CASE(13) MT_CASE(14) MT_CASE(15)
#undef MT_CASE
    default: break;
  }
  WL_LAUNCH_CHECK(); return 0;
}
int metrics_omega_theta(float* out, const float* u, const GridX& g, const float* z, const float* c, hipStream_t s) {
  WL_TRY(mt_common("omega_theta", u, g));
  MT_REJECT(!out || !z || !c, "omega_theta: null output, axis or center");
  MT_REJECT(g.D != 3, "omega_theta: ω_θ is defined for 3-D grids only (src/Metrics.jl:87)");
  MT_REJECT(mt_overlap(out, g.cs, u, g), "omega_theta: the output aliases the velocity array");
  MetricsArgs a{}; a.wth = out; mt_set3(a.z, z); mt_set3(a.c, c);
  mt_launch<M_WTH>(g, u, a, s);
  WL_LAUNCH_CHECK(); return 0;
}
int metrics_curl(float* out, const float* u, const GridX& g, int i, hipStream_t s) {
  WL_TRY(mt_common("curl", u, g));
  MT_REJECT(!out, "curl: null output");
  MT_REJECT(i < 1 || i > 3, "curl: component i must be 1, 2 or 3");
  MT_REJECT(g.D == 2 && i != 3, "curl: a 2-D grid has the component i = 3 only");
  MT_REJECT(mt_overlap(out, g.cs, u, g), "curl: the output aliases the velocity array");
  hipLaunchKernelGGL(k_curl, wl_plane_grid(g, g.D == 3 ? g.nz - 2 : 1), dim3(WL_BLOCK), 0, s, g, out, u, i - 1);
  WL_LAUNCH_CHECK(); return 0;
}
int metrics_helicity(float* out, const float* u, const float* w3, const GridX& g, hipStream_t s) {
  WL_TRY(mt_common("helicity", u, g));
  MT_REJECT(!out || !w3, "helicity: null output or vorticity array");
  MT_REJECT(g.D != 3, "helicity: defined for 3-D grids only (src/Metrics.jl:99)");
  MT_REJECT(mt_overlap(out, g.cs, u, g) || mt_overlap(out, g.cs, w3, g), "helicity: the output aliases an input array");
  hipLaunchKernelGGL(k_helicity, wl_plane_grid(g, g.nz - 2), dim3(WL_BLOCK), 0, s, g, out, u, w3);
  WL_LAUNCH_CHECK(); return 0;
}
// Σ_inside ke(I,u,U), Σ_inside ½|ω|², max_inside |ω| (2-D: curl(3) for ω) -> ws.res_d[0], ws.res_d[1], ws.res_f[0]; two launches
int metrics_stats_dev(const float* u, const GridX& g, const float* U, const RedWs& ws, hipStream_t s) {
  WL_TRY(mt_common("flow_stats", u, g));
  unsigned nb = 0;
  if (g.D == 2) {
    U3 Uv; mt_set3(Uv.v, nullptr); if (U) { Uv.v[0] = U[0]; Uv.v[1] = U[1]; }
    const long nbx = (g.sz + WL_BLOCK - 1) / WL_BLOCK;
    nb = (unsigned)(nbx < WL_REDPART ? nbx : WL_REDPART);
    hipLaunchKernelGGL(k_stats2, dim3(nb), dim3(WL_BLOCK), 0, s, g, u, Uv, ws.pa, ws.pb, ws.pm);
  } else {
    MetricsArgs a{}; mt_set3(a.U, U); a.pa = ws.pa; a.pb = ws.pb; a.pm = ws.pm;
    MT_REJECT((long)mt_ntiles8(g) * ((g.nz - 2 + mt_chunk(g) - 1) / mt_chunk(g)) > WL_MAXPART, "flow_stats: the x-y plane has more tiles than the reduction workspace has partials");
    mt_launch<M_STATS>(g, u, a, s, &nb);
  }
  hipLaunchKernelGGL(k_stats_final, dim3(1), dim3(WL_BLOCK), 0, s, ws.pa, ws.pb, ws.pm, (int)nb, ws.res_d, ws.res_f);
  WL_LAUNCH_CHECK(); return 0;
}
}  // namespace wl
