// The projection tails: mom_project!'s `u −= L∇x ; p = x/Δt` (src/Flow.jl:227-230) and, for the corrector, CFL's flux_out and its maximum
// (:234-244) in the same pass.  What a tail can do on a level, what the caller asks for and what the launcher reports: wl_project.hpp.
//
// Forms, all with the same statements per cell (compiled with the flags of wl_poisson.hip, -ffp-contract=off: same bits):
//   k_project_unscale   one cell per thread; the in-place tail of every level, and of the three plane ranges of a body
//   k_project_cfl       one cell per thread, z-marching; the corrector's tail wherever the pair form does not apply
//   k_project_cfl2      two x-adjacent cells per thread, one plane per block; the corrector's tail on 3-D constant-coefficient levels of even nx
//   k_project_wide      four cells per thread, 16-byte accesses (option "tailwide"); both tails where project_wide_path holds
// Block order, as measured at 512³ (profiles/r03_experiments.md §4, §8):
//   first tail (k_project_unscale): linear block order, one plane per block, one cell per thread — 1.04 -> 0.875 ms.  A two-cells-per-thread form of
//   this tail measured 0.915 ms and was never the default; it was removed with its switch (profiles/projfile_experiments.md);
//   second tail (+ flux_out + max σ): in linear order the one-cell kernel is L1-bound (13 dword loads per cell: 1.33 -> 1.55 ms), so k_project_cfl keeps
//   the XCD-tiled order of wl_tile and per-block maxima; with two cells per thread (k_project_cfl2, ≈6.5 loads per cell) linear order wins: 1.34 -> 1.18 ms.
#include "wl_project.hpp"
#include "wl_pdefer.hpp"

namespace {
// what the tail kernels read of a request (wl::TailReq): BC!(u,U) folded into the stores (on, U: wl_bcfold.hpp); U on load for the wall-normal boundary
// faces of u_in (usub); the device flag of a tail queued ahead of the solver's convergence read (go: runs iff *go > 0; null: runs)
struct TailBc { int on; float U[3]; int usub; const float* go; };
// float -> int that orders like the float (−0 < +0 aside): maxima of many blocks through integer atomicMax into a few slots
#define WL_ENC_SLOTS 1024
__device__ __forceinline__ int wl_enc_f(float v) { const int b = __float_as_int(v); return b >= 0 ? b : (b ^ 0x7FFFFFFF); }
__device__ __forceinline__ float wl_dec_f(int k) { return __int_as_float(k >= 0 ? k : (k ^ 0x7FFFFFFF)); }
// mom_project! tail (src/Flow.jl:227-230): u[I,i] -= L[I,i]·∂ᵢx ; p_out = x/dt (ALL cells), p_out ≠ x
// SP = 0: p_out is not stored (skip_p, wl_pdefer.hpp — the next fused head divides on load, wl_resjac_body.inc); the store and its division are compiled out
template <int D, int CL, int SP = 1>
__global__ void k_project_unscale(GridX g, float* __restrict__ u, const float* __restrict__ L, const float* __restrict__ x, float* __restrict__ pout, float dt, wl::ConstL cl, int zchunk,
                                  int p0, int p1, TailBc bc, int lin) {   // local planes [p0,p1) of this launch; bc.on: BC!(u,U) folded into the stores (wl_bcfold.hpp); lin: linear block order (wl_tile_lin)
  if (bc.go && !(*bc.go > 0.f)) return;   // queued before the host knew whether the solve had converged: it had not (0), or the solve is discarded (−1)
  int i, j; long m; int pz;
  if (lin) wl_tile_lin(g, m, pz); else wl_tile(g, m, pz);
  if (!cell_ij(g, m, i, j)) return;
  const bool inij = interior_ij(g, i, j);
  const int ks = p0 + pz * zchunk, ke = (ks + zchunk < p1) ? ks + zchunk : p1;
  long o = m + (long)ks * g.sz;
  float xkm = (D == 3 && ks > 0 && ks < ke) ? x[o - g.sz] : 0.f;      // x[k-1] stays in a register while marching
  const float lxc = CL ? wl::wl_cl_coef(i + 1, g.nx, cl.c[0]) : 0.f, lyc = CL ? wl::wl_cl_coef(j + 1, g.ny, cl.c[1]) : 0.f;
  for (int k = ks; k < ke; k++, o += g.sz) {
    const float xc = x[o];
    if (SP) pout[o] = wl_unscale(xc, dt);
    bool in = inij;
    if (D == 3) in = in && k >= g.k0 && k < g.k1;
    if (in) {
      const float lx = CL ? lxc : L[o], ly = CL ? lyc : L[g.cs + o];
      if (D == 3 && bc.on) {
        const float lz = CL ? wl::wl_cl_coef(g.gk + k + 1, g.gnz, cl.c[2]) : L[2 * g.cs + o];
        const float v[3] = {u[o] - lx * (xc - x[o - 1]), u[g.cs + o] - ly * (xc - x[o - g.sy]), u[2 * g.cs + o] - lz * (xc - xkm)};
        if (wl_bc_fold_plain(g, i, j, k)) { u[o] = v[0]; u[g.cs + o] = v[1]; u[2 * g.cs + o] = v[2]; }
        else wl_bc_fold_store(u, g, i, j, k, v, bc.U);
      } else {
      u[o] -= lx * (xc - x[o - 1]);
      u[g.cs + o] -= ly * (xc - x[o - g.sy]);
      if (D == 3) { const float lz = CL ? wl::wl_cl_coef(g.gk + k + 1, g.gnz, cl.c[2]) : L[2 * g.cs + o]; u[2 * g.cs + o] -= lz * (xc - xkm); }
      }
    }
    xkm = xc;
  }
}
// The corrector's mom_project! tail with CFL's flux_out folded in (src/Flow.jl:227-230 + :234-244): out-of-place u (u_out ≠ u_in, so
// the +δ neighbours' projected values can be recomputed from u_in — the same statements their owners execute, hence the same
// bits), σ = flux_out of the projected field, per-workgroup max over the planes [kfirst,klast) of σ (ghost cells: stale Φ, Q1).
// Valid when BC! does not change what flux_out reads: wall-normal boundary faces already hold U and L is 0 there
// (non-periodic, no exitBC).  Cells outside the interior of u_out are left for BC! to write.
template <int D, int CL>
__global__ void k_project_cfl(GridX g, float* __restrict__ uout, const float* __restrict__ uin, const float* __restrict__ L, const float* __restrict__ x, float* __restrict__ pout,
                              float* __restrict__ sigma, float dt, wl::ConstL cl, int zchunk, int kfirst, int klast, float* __restrict__ pmax, int p0, int p1, int store_sigma, TailBc bc) {
  int i, j; long m; int pz;
  wl_tile(g, m, pz);
  float mx = -INFINITY;
  if (cell_ij(g, m, i, j)) {
    const bool inij = interior_ij(g, i, j);
    const int ks = p0 + pz * zchunk, ke = (ks + zchunk < p1) ? ks + zchunk : p1;
    long o = m + (long)ks * g.sz;
    float xkm = (D == 3 && ks > 0 && ks < ke) ? x[o - g.sz] : 0.f, xc = (ks < ke) ? x[o] : 0.f;
    float lx = 0.f, lxp = 0.f, ly = 0.f, lyp = 0.f;
    if (CL) {
      lx = wl::wl_cl_coef(i + 1, g.nx, cl.c[0]); lxp = wl::wl_cl_coef(i + 2, g.nx, cl.c[0]);
      ly = wl::wl_cl_coef(j + 1, g.ny, cl.c[1]); lyp = wl::wl_cl_coef(j + 2, g.ny, cl.c[1]);
    }
    for (int k = ks; k < ke; k++, o += g.sz) {
      const float xkp = (D == 3 && k + 1 < g.nz) ? x[o + g.sz] : 0.f;
      pout[o] = wl_unscale(xc, dt);
      bool in = inij;
      if (D == 3) in = in && k >= g.k0 && k < g.k1;
      float sg;
      if (in) {
        float lz = 0.f, lzp = 0.f;
        if (CL) { if (D == 3) { lz = wl::wl_cl_coef(g.gk + k + 1, g.gnz, cl.c[2]); lzp = wl::wl_cl_coef(g.gk + k + 2, g.gnz, cl.c[2]); } }
        else {
          lx = L[o]; lxp = L[o + 1]; ly = L[g.cs + o]; lyp = L[g.cs + o + g.sy];
          if (D == 3) { lz = L[2 * g.cs + o]; lzp = L[2 * g.cs + o + g.sz]; }
        }
        const float uxn = uin[o] - lx * (xc - x[o - 1]), uxp = uin[o + 1] - lxp * (x[o + 1] - xc);
        const float uyn = uin[g.cs + o] - ly * (xc - x[o - g.sy]), uyp = uin[g.cs + o + g.sy] - lyp * (x[o + g.sy] - xc);
        const bool foldc = D == 3 && bc.on && !wl_bc_fold_plain(g, i, j, k);      // BC!(u_out,U) folded into the stores of the cells near the boundary
        if (!foldc) { uout[o] = uxn; uout[g.cs + o] = uyn; }
        sg = 0.f;
        sg += (fmaxf(0.f, uxp) + fmaxf(0.f, -uxn));
        sg += (fmaxf(0.f, uyp) + fmaxf(0.f, -uyn));
        if (D == 3) {
          const float uzn = uin[2 * g.cs + o] - lz * (xc - xkm), uzp = uin[2 * g.cs + o + g.sz] - lzp * (xkp - xc);
          if (!foldc) uout[2 * g.cs + o] = uzn;
          else { const float v[3] = {uxn, uyn, uzn}; wl_bc_fold_store(uout, g, i, j, k, v, bc.U); }
          sg += (fmaxf(0.f, uzp) + fmaxf(0.f, -uzn));
        }
        if (store_sigma) sigma[o] = sg;       // σ = flux_out is only read by the maximum taken here: materialised on request
      } else sg = sigma[o];
      if (k >= kfirst && k < klast) mx = fmaxf(mx, sg);
      xkm = xc; xc = xkp;
    }
  }
  mx = block_max(mx);
  if (threadIdx.x == 0) pmax[blockIdx.x] = mx;      // one float per block: k_fin_max2 finishes
}
__global__ void k_enc_init(int* __restrict__ p) { p[threadIdx.x] = (int)0x80000000; }
// ---- the corrector's tail with TWO x-adjacent cells per thread, one plane per block, linear block order (3-D, constant coefficients, even nx) -----------
// Same statements per cell as k_project_cfl.  Why a second form: in linear order (the order HBM serves best, wl_tile_lin) the one-cell
// kernel is bound by L1 requests — 13 dword loads per cell; as float2 pairs the same cells need about half of them.
// Block h: chunk (h mod nb8) of 512 consecutive floats of plane (h div nb8); a pair never straddles a row (nx even, pairs start at even columns).
__device__ __forceinline__ float2 pl_ld2(const float* __restrict__ p, long o) { return *reinterpret_cast<const float2*>(p + o); }
__device__ __forceinline__ void pl_st2(float* __restrict__ p, long o, float2 v) { *reinterpret_cast<float2*>(p + o) = v; }
__device__ __forceinline__ bool pl_pair(const GridX& g, long& m, int& k, int p0) {
  const long np2 = (g.sz / 2 + WL_BLOCK - 1) / WL_BLOCK;          // 256-pair chunks per plane
  const unsigned nb8 = (unsigned)(((np2 + 7) >> 3) << 3);
  const unsigned h = blockIdx.x;
  const unsigned p = h / nb8;
  k = p0 + (int)p;
  m = 2 * ((long)(h - p * nb8) * WL_BLOCK + threadIdx.x);
  return m < g.sz;
}
static inline unsigned pl_grid(const GridX& g, int nplanes) { const long np2 = (g.sz / 2 + WL_BLOCK - 1) / WL_BLOCK; return (unsigned)((((np2 + 7) >> 3) << 3) * nplanes); }
template <int SP>      // SP = 0: p_out is not stored (skip_p, wl_pdefer.hpp)
__global__ void __launch_bounds__(WL_BLOCK) k_project_cfl2(GridX g, float* __restrict__ uout, const float* __restrict__ uin, const float* __restrict__ x, float* __restrict__ pout,
                                                              float* __restrict__ sigma, float dt, wl::ConstL cl, int kfirst, int klast, float* __restrict__ pmax, int p0, int p1,
                                                              int store_sigma, TailBc bc) {
  if (bc.go && !(*bc.go > 0.f)) return;   // (block-uniform; the maximum's slots keep k_enc_init's −∞)
  long m; int k;
  float mx = -INFINITY;
  if (pl_pair(g, m, k, p0) && k < p1) {
    const int j = (int)(m / g.nx), i0 = (int)(m - (long)j * g.nx);
    const long o = m + (long)k * g.sz;
    const float2 xc = pl_ld2(x, o);
    if (SP) pl_st2(pout, o, make_float2(wl_unscale(xc.x, dt), wl_unscale(xc.y, dt)));
    const bool row = j >= 1 && j <= g.ny - 2 && k >= g.k0 && k < g.k1;
    const bool in0 = row && i0 >= 1, in1 = row && i0 + 1 <= g.nx - 2;
    const bool want = k >= kfirst && k < klast;
    float sg0 = 0.f, sg1 = 0.f;
    if (in0 || in1) {
      const float lx0 = wl::wl_cl_coef(i0 + 1, g.nx, cl.c[0]), lx1 = wl::wl_cl_coef(i0 + 2, g.nx, cl.c[0]), lx2 = wl::wl_cl_coef(i0 + 3, g.nx, cl.c[0]);
      const float ly = wl::wl_cl_coef(j + 1, g.ny, cl.c[1]), lyp = wl::wl_cl_coef(j + 2, g.ny, cl.c[1]);
      const float lz = wl::wl_cl_coef(g.gk + k + 1, g.gnz, cl.c[2]), lzp = wl::wl_cl_coef(g.gk + k + 2, g.gnz, cl.c[2]);
      const float xl = in0 ? x[o - 1] : 0.f, xr = in1 ? x[o + 2] : 0.f;
      const float2 xym = pl_ld2(x, o - g.sy), xyp = pl_ld2(x, o + g.sy), xzm = pl_ld2(x, o - g.sz), xzp = pl_ld2(x, o + g.sz);
      float2 a0 = pl_ld2(uin, o), a1 = pl_ld2(uin, g.cs + o), a2 = pl_ld2(uin, 2 * g.cs + o);
      const float axr = in1 ? uin[o + 2] : 0.f;
      float2 a1p = pl_ld2(uin, g.cs + o + g.sy), a2p = pl_ld2(uin, 2 * g.cs + o + g.sz);
      if (bc.usub) {   // BC!(u_in,U) deferred: the values BC! would have put on the wall-normal faces this stencil reads (index 1 and N−1 along the component's direction)
        if (i0 == 0 || i0 == g.nx - 2) a0.y = bc.U[0];
        if (j == 1) a1 = make_float2(bc.U[1], bc.U[1]);
        if (j + 1 == g.ny - 1) a1p = make_float2(bc.U[1], bc.U[1]);
        if (g.gk + k == 1) a2 = make_float2(bc.U[2], bc.U[2]);
        if (g.gk + k + 1 == g.gnz - 1) a2p = make_float2(bc.U[2], bc.U[2]);
      }
      // cell 0 (i0): same statements as k_project_cfl
      const float uxn0 = a0.x - lx0 * (xc.x - xl), uxp0 = a0.y - lx1 * (xc.y - xc.x);
      const float uyn0 = a1.x - ly * (xc.x - xym.x), uyp0 = a1p.x - lyp * (xyp.x - xc.x);
      const float uzn0 = a2.x - lz * (xc.x - xzm.x), uzp0 = a2p.x - lzp * (xzp.x - xc.x);
      // cell 1 (i0+1)
      const float uxn1 = a0.y - lx1 * (xc.y - xc.x), uxp1 = axr - lx2 * (xr - xc.y);
      const float uyn1 = a1.y - ly * (xc.y - xym.y), uyp1 = a1p.y - lyp * (xyp.y - xc.y);
      const float uzn1 = a2.y - lz * (xc.y - xzm.y), uzp1 = a2p.y - lzp * (xzp.y - xc.y);
      if (in0) { sg0 = 0.f; sg0 += (fmaxf(0.f, uxp0) + fmaxf(0.f, -uxn0)); sg0 += (fmaxf(0.f, uyp0) + fmaxf(0.f, -uyn0)); sg0 += (fmaxf(0.f, uzp0) + fmaxf(0.f, -uzn0)); }
      if (in1) { sg1 = 0.f; sg1 += (fmaxf(0.f, uxp1) + fmaxf(0.f, -uxn1)); sg1 += (fmaxf(0.f, uyp1) + fmaxf(0.f, -uyn1)); sg1 += (fmaxf(0.f, uzp1) + fmaxf(0.f, -uzn1)); }
      const float va[3] = {uxn0, uyn0, uzn0}, vb[3] = {uxn1, uyn1, uzn1};
      const bool plain0 = !bc.on || wl_bc_fold_plain(g, i0, j, k), plain1 = !bc.on || wl_bc_fold_plain(g, i0 + 1, j, k);
      if (in0 && in1 && plain0 && plain1) { pl_st2(uout, o, make_float2(va[0], vb[0])); pl_st2(uout, g.cs + o, make_float2(va[1], vb[1])); pl_st2(uout, 2 * g.cs + o, make_float2(va[2], vb[2])); }
      else {
        if (in0) { if (plain0) { uout[o] = va[0]; uout[g.cs + o] = va[1]; uout[2 * g.cs + o] = va[2]; } else wl_bc_fold_store(uout, g, i0, j, k, va, bc.U); }
        if (in1) { if (plain1) { uout[o + 1] = vb[0]; uout[g.cs + o + 1] = vb[1]; uout[2 * g.cs + o + 1] = vb[2]; } else wl_bc_fold_store(uout, g, i0 + 1, j, k, vb, bc.U); }
      }
      if (store_sigma) { if (in0) sigma[o] = sg0; if (in1) sigma[o + 1] = sg1; }
    }
    if (want) {      // cells outside the interior: the stale Φ the reference leaves in σ's ghost cells takes part in maximum(σ)  (quirk Q1)
      if (!in0) sg0 = sigma[o];
      if (!in1) sg1 = sigma[o + 1];
      mx = fmaxf(sg0, sg1);
    }
  }
  mx = block_max(mx);
  if (threadIdx.x == 0) atomicMax(reinterpret_cast<int*>(pmax) + (blockIdx.x & (WL_ENC_SLOTS - 1)), wl_enc_f(mx));
}
// ---- the projection tails with FOUR x-adjacent cells per thread and 16-byte accesses (option "tailwide"; 3-D, constant coefficients, even nx, nx·ny ≡ 0 mod 4) ----
// Same statements per cell as k_project_unscale / k_project_cfl.  A block owns WL_TW_CHUNK consecutive floats of ONE plane (about two rows at 512³), blocks in the
// linear order of pl_pair (a chunk position keeps its XCD from plane to plane).  The plane is taken as a linear array: with nx·ny a multiple of 4 every quad
// m = 4q of every plane and component starts on a 16-byte boundary, and so do its ±z neighbours — u, x[k∓1] and u_z[k+1] are one 16-byte load per quad, u one
// 16-byte store per component.  The in-plane neighbours of x (±1, ±nx: nx ≡ 2 mod 4 puts the rows 8 bytes off) go through LDS: the block stages the window
// [m0 − nx, m0 + CHUNK + nx) of x once with 16-byte loads, every x operand of the plane is then an LDS read.  u_y[j+1] is two 8-byte loads, u_x of the cell after
// the quad one 4-byte load.  A quad may straddle a row seam (its cells are then the ghosts i = nx−1, i = 0 and their interior neighbours): every cell carries its
// own (i,j), and only a quad of four cells that take a plain store is stored 16 bytes wide — the others go through the per-cell path of the pair kernels.
// LDS cells of the window that lie outside the plane (before its first cell, past its last) are staged as 0: only ghost cells read them, and discard the result.
// One quad per thread: two (2048-float chunks) measured slower, profiles/tailwide_experiments.md §5.
#define WL_TW_CHUNK (4 * WL_BLOCK)
__device__ __forceinline__ float4 tw_ld4(const float* __restrict__ p, long o) { return *reinterpret_cast<const float4*>(p + o); }
__device__ __forceinline__ void tw_st4(float* __restrict__ p, long o, float4 v) { *reinterpret_cast<float4*>(p + o) = v; }
static inline unsigned tw_nb8(const GridX& g) { const long nb = (g.sz + WL_TW_CHUNK - 1) / WL_TW_CHUNK; return (unsigned)(((nb + 7) >> 3) << 3); }
static inline unsigned tw_grid(const GridX& g, int nplanes) { return tw_nb8(g) * (unsigned)nplanes; }
static inline size_t tw_lds_bytes(const GridX& g) { return (size_t)(WL_TW_CHUNK + 2 * g.sy + 8) * sizeof(float); }
// CFL = 0: the in-place tail (u_out is u, u_in unused); CFL = 1: out of place + flux_out + max σ.  SP = 0: p_out is not stored (skip_p, wl_pdefer.hpp)
template <int CFL, int SP>
__global__ void __launch_bounds__(WL_BLOCK) k_project_wide(GridX g, float* __restrict__ uout, const float* __restrict__ uin, const float* __restrict__ x, float* __restrict__ pout,
                                                              float* __restrict__ sigma, float dt, wl::ConstL cl, int kfirst, int klast, float* __restrict__ pmax, int p0, int p1,
                                                              int store_sigma, TailBc bc, unsigned nb8) {
  if (bc.go && !(*bc.go > 0.f)) return;   // (block-uniform; the maximum's slots keep k_enc_init's −∞)
  extern __shared__ float4 tw_sh[];
  float* __restrict__ xs = reinterpret_cast<float*>(tw_sh);
  const float* __restrict__ ui = CFL ? uin : uout;
  const unsigned h = blockIdx.x, p = h / nb8;
  const int k = p0 + (int)p;
  const long m0 = (long)(h - p * nb8) * WL_TW_CHUNK;
  float mx = -INFINITY;
  if (m0 < g.sz && k < p1) {            // (block-uniform)
    const long ko = (long)k * g.sz;
    const int sy = (int)g.sy;
    const long base = (m0 - sy) & ~3L;  // plane index of xs[0] (negative on the first chunk)
    const bool zin = k >= g.k0 && k < g.k1;
    if (zin) {                          // stage x[base .. m0 + CHUNK (+ nx)) of plane k: every LDS cell a quad of this block reads; 0 outside the plane
      const long whi = (m0 + WL_TW_CHUNK + (CFL ? sy : 0) + 3) & ~3L;
      for (long q = base + 4 * (long)threadIdx.x; q < whi; q += 4 * WL_BLOCK)
        *reinterpret_cast<float4*>(xs + (q - base)) = (q >= 0 && q < g.sz) ? tw_ld4(x, ko + q) : make_float4(0.f, 0.f, 0.f, 0.f);
      __syncthreads();
    }
    const float lz = wl::wl_cl_coef(g.gk + k + 1, g.gnz, cl.c[2]), lzp = wl::wl_cl_coef(g.gk + k + 2, g.gnz, cl.c[2]);
    const bool want = CFL && k >= kfirst && k < klast;
    const long m = m0 + 4 * (long)threadIdx.x;
    if (m < g.sz) {
      const long o = ko + m;
      const int r = (int)(m - base);    // xs[r] is cell 0 of the quad
      const float4 xq = zin ? *reinterpret_cast<const float4*>(xs + r) : tw_ld4(x, o);
      const float X[6] = {zin ? xs[r - 1] : 0.f, xq.x, xq.y, xq.z, xq.w, (CFL && zin) ? xs[r + 4] : 0.f};
      if (SP) tw_st4(pout, o, make_float4(wl_unscale(xq.x, dt), wl_unscale(xq.y, dt), wl_unscale(xq.z, dt), wl_unscale(xq.w, dt)));
      const int j0 = (int)(m / g.nx), i0 = (int)(m - (long)j0 * g.nx);
      int ii[4], jj[4]; bool in[4];
#pragma unroll
      for (int c = 0; c < 4; c++) {
        int i = i0 + c, j = j0;
        if (i >= g.nx) { i -= g.nx; j++; }
        ii[c] = i; jj[c] = j;
        in[c] = zin && i >= 1 && i <= g.nx - 2 && j >= 1 && j <= g.ny - 2;
      }
      float sg[4] = {0.f, 0.f, 0.f, 0.f};
      if (in[0] || in[1] || in[2] || in[3]) {
        const float2 ym0 = *reinterpret_cast<const float2*>(xs + r - sy), ym1 = *reinterpret_cast<const float2*>(xs + r - sy + 2);
        const float XYM[4] = {ym0.x, ym0.y, ym1.x, ym1.y};
        const float4 zmq = tw_ld4(x, o - g.sz);
        const float XZM[4] = {zmq.x, zmq.y, zmq.z, zmq.w};
        const float4 a0q = tw_ld4(ui, o), a1q = tw_ld4(ui, g.cs + o), a2q = tw_ld4(ui, 2 * g.cs + o);
        float A0[5] = {a0q.x, a0q.y, a0q.z, a0q.w, 0.f};
        const float A1[4] = {a1q.x, a1q.y, a1q.z, a1q.w}, A2[4] = {a2q.x, a2q.y, a2q.z, a2q.w};
        float XYP[4] = {0.f, 0.f, 0.f, 0.f}, XZP[4] = {0.f, 0.f, 0.f, 0.f}, A1P[4] = {0.f, 0.f, 0.f, 0.f}, A2P[4] = {0.f, 0.f, 0.f, 0.f};
        if (CFL) {
          const float2 yp0 = *reinterpret_cast<const float2*>(xs + r + sy), yp1 = *reinterpret_cast<const float2*>(xs + r + sy + 2);
          XYP[0] = yp0.x; XYP[1] = yp0.y; XYP[2] = yp1.x; XYP[3] = yp1.y;
          const float4 zpq = tw_ld4(x, o + g.sz), a2pq = tw_ld4(ui, 2 * g.cs + o + g.sz);     // (zin: plane k+1 exists)
          XZP[0] = zpq.x; XZP[1] = zpq.y; XZP[2] = zpq.z; XZP[3] = zpq.w;
          A2P[0] = a2pq.x; A2P[1] = a2pq.y; A2P[2] = a2pq.z; A2P[3] = a2pq.w;
          A0[4] = ui[o + 4];                                                                    // (at the plane's end these reach into plane k+1, which exists)
          const float2 b0 = *reinterpret_cast<const float2*>(ui + g.cs + o + sy), b1 = *reinterpret_cast<const float2*>(ui + g.cs + o + sy + 2);
          A1P[0] = b0.x; A1P[1] = b0.y; A1P[2] = b1.x; A1P[3] = b1.y;
        }
        float V[4][3]; bool plain[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
          const int i = ii[c], j = jj[c];
          const float xc = X[c + 1];
          const float lx = wl::wl_cl_coef(i + 1, g.nx, cl.c[0]), ly = wl::wl_cl_coef(j + 1, g.ny, cl.c[1]);
          float a0 = A0[c], a0n = A0[c + 1], a1 = A1[c], a1p = A1P[c], a2 = A2[c], a2p = A2P[c];
          if (CFL && bc.usub) {   // BC!(u_in,U) deferred: U on the wall-normal faces this stencil reads (index 1 and N−1 along the component's direction), as in k_project_cfl2
            if (i == 1) a0 = bc.U[0];
            if (i + 2 == g.nx) a0n = bc.U[0];
            if (j == 1) a1 = bc.U[1];
            if (j + 2 == g.ny) a1p = bc.U[1];
            if (g.gk + k == 1) a2 = bc.U[2];
            if (g.gk + k + 2 == g.gnz) a2p = bc.U[2];
          }
          const float uxn = a0 - lx * (xc - X[c]);
          const float uyn = a1 - ly * (xc - XYM[c]);
          const float uzn = a2 - lz * (xc - XZM[c]);
          V[c][0] = uxn; V[c][1] = uyn; V[c][2] = uzn;
          if (CFL) {
            const float lxp = wl::wl_cl_coef(i + 2, g.nx, cl.c[0]), lyp = wl::wl_cl_coef(j + 2, g.ny, cl.c[1]);
            const float uxp = a0n - lxp * (X[c + 2] - xc);
            const float uyp = a1p - lyp * (XYP[c] - xc);
            const float uzp = a2p - lzp * (XZP[c] - xc);
            if (in[c]) { float s = 0.f; s += (fmaxf(0.f, uxp) + fmaxf(0.f, -uxn)); s += (fmaxf(0.f, uyp) + fmaxf(0.f, -uyn)); s += (fmaxf(0.f, uzp) + fmaxf(0.f, -uzn)); sg[c] = s; }
          }
          plain[c] = in[c] && (!bc.on || wl_bc_fold_plain(g, i, j, k));
        }
        if (plain[0] && plain[1] && plain[2] && plain[3]) {
          tw_st4(uout, o, make_float4(V[0][0], V[1][0], V[2][0], V[3][0]));
          tw_st4(uout, g.cs + o, make_float4(V[0][1], V[1][1], V[2][1], V[3][1]));
          tw_st4(uout, 2 * g.cs + o, make_float4(V[0][2], V[1][2], V[2][2], V[3][2]));
        } else {
#pragma unroll
          for (int c = 0; c < 4; c++) {
            if (!in[c]) continue;
            if (plain[c]) { uout[o + c] = V[c][0]; uout[g.cs + o + c] = V[c][1]; uout[2 * g.cs + o + c] = V[c][2]; }
            else wl_bc_fold_store(uout, g, ii[c], jj[c], k, V[c], bc.U);
          }
        }
        if (CFL && store_sigma) {
#pragma unroll
          for (int c = 0; c < 4; c++) if (in[c]) sigma[o + c] = sg[c];
        }
      }
      if (want) {      // cells outside the interior: the stale Φ the reference leaves in σ's ghost cells takes part in maximum(σ)  (quirk Q1)
#pragma unroll
        for (int c = 0; c < 4; c++) if (!in[c]) sg[c] = sigma[o + c];
        mx = fmaxf(mx, fmaxf(fmaxf(sg[0], sg[1]), fmaxf(sg[2], sg[3])));
      }
    }
  }
  if (CFL) {
    mx = block_max(mx);
    if (threadIdx.x == 0) atomicMax(reinterpret_cast<int*>(pmax) + (blockIdx.x & (WL_ENC_SLOTS - 1)), wl_enc_f(mx));
  }
}

__global__ void k_fin_max_enc(const int* __restrict__ p, float* __restrict__ om) {
  float mx = -INFINITY;
  for (int q = threadIdx.x; q < WL_ENC_SLOTS; q += WL_BLOCK) { const int k = p[q]; if (k != (int)0x80000000) mx = fmaxf(mx, wl_dec_f(k)); }
  mx = block_max(mx); if (threadIdx.x == 0) *om = mx;
}
__global__ void k_fin_max2(const float* __restrict__ pmax, int n, float* __restrict__ om) {
  float mx = -INFINITY, m1 = -INFINITY, m2 = -INFINITY, m3 = -INFINITY;
  int q = threadIdx.x;
  for (; q + 3 * WL_BLOCK < n; q += 4 * WL_BLOCK) { mx = fmaxf(mx, pmax[q]); m1 = fmaxf(m1, pmax[q + WL_BLOCK]); m2 = fmaxf(m2, pmax[q + 2 * WL_BLOCK]); m3 = fmaxf(m3, pmax[q + 3 * WL_BLOCK]); }
  for (; q < n; q += WL_BLOCK) mx = fmaxf(mx, pmax[q]);
  mx = fmaxf(fmaxf(mx, m1), fmaxf(m2, m3));
  mx = block_max(mx); if (threadIdx.x == 0) *om = mx;
}
}  // namespace
namespace wl {
#define DSEL2(D, CLF, KERN, ...)                                                                                     \
  do { if ((D) == 3) { if (CLF) hipLaunchKernelGGL((KERN<3, 1>), __VA_ARGS__); else hipLaunchKernelGGL((KERN<3, 0>), __VA_ARGS__); } \
       else { if (CLF) hipLaunchKernelGGL((KERN<2, 1>), __VA_ARGS__); else hipLaunchKernelGGL((KERN<2, 0>), __VA_ARGS__); } } while (0)
// The four-cells-per-thread tails (k_project_wide) run where the pair tails do, on planes that are a whole number of quads, with every array on a 16-byte boundary
// and a staging window that fits the LDS of a block.  The one choice left to launch time — it depends on the arrays actually passed — and no capability: the
// form honours whatever the narrower one does.  A launcher that takes it says so in its report (TailRep::wide).
static bool project_wide_path(const GridX& g, const ConstL& cl, const void* a, const void* b, const void* c, const void* d = nullptr, const void* e = nullptr) {
  if (!(g.D == 3 && cl.on && (g.nx & 1) == 0 && g.nx >= 8 && g.ny >= 4 && (g.sz & 3) == 0 && g.k0 >= 1 && g.k1 <= g.nz - 1)) return false;
  if (tw_lds_bytes(g) > 48 * 1024 || (long)tw_nb8(g) * g.nz > 0x7fffffffL) return false;
  const void* ptr[5] = {a, b, c, d, e};
  for (int q = 0; q < 5; q++) if ((reinterpret_cast<uintptr_t>(ptr[q]) & 15) != 0) return false;
  return true;
}
// the kernels' view of a request on a level with the capabilities `caps`; *folded: BC!(u,U) goes into the stores
static TailBc tail_bc(const TailReq& rq, const TailCaps& caps, bool* folded) {
  TailBc bc{0, {0.f, 0.f, 0.f}, rq.usub ? 1 : 0, rq.go};
  *folded = rq.U && caps.fold;
  if (*folded) { bc.on = 1; for (int c = 0; c < 3; c++) bc.U[c] = rq.U[c]; }
  return bc;
}
static const TailBc no_bc{0, {0.f, 0.f, 0.f}, 0, nullptr};      // the z-split launches: nothing folded, substituted or gated
int project_unscale(float* u, const float* L, const float* x, float* pout, const GridX& g, float dt, const ConstL& cl, hipStream_t s, const TailReq& rq, TailRep* rep) {
  const TailCaps caps = tail_caps_inplace(g, cl);
  if (rq.usub) { wl_set_error("project_unscale: the in-place tail reads no boundary face of u, there is nothing to substitute (usub)"); return WL_EINVAL; }
  if (rq.skip_p && !caps.skip_p) { wl_set_error("project_unscale: the tail without the p store needs a 3-D constant-coefficient level"); return WL_EINVAL; }
  const int lin = g.D == 3;      // linear block order, one plane per block (wl_tile_lin)
  const int zc = lin ? 1 : wl_march_chunk(g, g.nz);
  bool folded;
  const TailBc bc = tail_bc(rq, caps, &folded);
  const bool wide = rq.wide && lin && project_wide_path(g, cl, u, x, rq.skip_p ? nullptr : pout);
  *rep = TailRep{folded, wide};
  if (wide) {   // four cells per thread, 16-byte accesses (k_project_wide)
    const dim3 grid(tw_grid(g, g.nz));
    if (rq.skip_p) hipLaunchKernelGGL((k_project_wide<0, 0>), grid, dim3(WL_BLOCK), tw_lds_bytes(g), s, g, u, nullptr, x, pout, nullptr, dt, cl, 0, 0, nullptr, 0, g.nz, 0, bc, tw_nb8(g));
    else hipLaunchKernelGGL((k_project_wide<0, 1>), grid, dim3(WL_BLOCK), tw_lds_bytes(g), s, g, u, nullptr, x, pout, nullptr, dt, cl, 0, 0, nullptr, 0, g.nz, 0, bc, tw_nb8(g));
    WL_LAUNCH_CHECK(); return 0;
  }
  if (rq.skip_p) {   // the store-free form exists for the 3-D constant-coefficient kernel (the only levels a fused head follows)
    hipLaunchKernelGGL((k_project_unscale<3, 1, 0>), wl_plane_grid(g, wl_march_slots(g.nz, zc)), dim3(WL_BLOCK), 0, s, g, u, L, x, pout, dt, cl, zc, 0, g.nz, bc, lin);
    WL_LAUNCH_CHECK(); return 0;
  }
  DSEL2(g.D, cl.on, k_project_unscale, wl_plane_grid(g, wl_march_slots(g.nz, zc)), dim3(WL_BLOCK), 0, s, g, u, L, x, pout, dt, cl, zc, 0, g.nz, bc, lin);
  WL_LAUNCH_CHECK(); return 0;
}
// level with a body: planes [0,na) and [nb,nz) with the constant-coefficient pattern `far`, [na,nb) reading L (see div_residual_split)
int project_unscale_split(float* u, const float* L, const float* x, float* pout, const GridX& g, float dt, const ConstL& near, const ConstL& far, int na, int nb, hipStream_t s) {
  const int lo[3] = {0, na, nb}, hi[3] = {na, nb, g.nz};
  for (int q = 0; q < 3; q++) {
    const int np = hi[q] - lo[q];
    if (np <= 0) continue;
    const ConstL& cl = q == 1 ? near : far;
    const int zc = wl_march_chunk(g, np);
    DSEL2(g.D, cl.on, k_project_unscale, wl_plane_grid(g, wl_march_slots(np, zc)), dim3(WL_BLOCK), 0, s, g, u, L, x, pout, dt, cl, zc, lo[q], hi[q], no_bc, 0);
  }
  WL_LAUNCH_CHECK(); return 0;
}
// projection tail + CFL's σ and max(σ) -> ws.res_f[slot_f]; u_out must not alias u_in
int project_cfl(float* uout, const float* uin, const float* L, const float* x, float* pout, float* sigma, const GridX& g, float dt, const ConstL& cl, const RedWs& ws, int slot_f, hipStream_t s,
                int store_sigma, const TailReq& rq, TailRep* rep) {
  if (uout == uin) { wl_set_error("project_cfl: output aliases input"); return WL_EINVAL; }
  const TailCaps caps = tail_caps_cfl(g, cl);
  bool folded;
  const TailBc bc = tail_bc(rq, caps, &folded);
  if (rq.go && !caps.gate) { wl_set_error("project_cfl: a tail queued ahead of the convergence read needs the two-cells-per-thread form"); return WL_EINVAL; }
  if (rq.usub && !(folded && caps.usub)) { wl_set_error("project_cfl: deferred BC! needs the folded two-cells-per-thread tail"); return WL_EINVAL; }
  if (rq.skip_p && !caps.skip_p) { wl_set_error("project_cfl: the tail without the p store needs the two-cells-per-thread form"); return WL_EINVAL; }
  int kfirst = 0, klast = 1;
  if (g.D == 3) { kfirst = (g.gk + g.k0 == 1) ? g.k0 - 1 : g.k0; klast = (g.gk + g.k1 == g.gnz - 1) ? g.k1 + 1 : g.k1; }
  if (caps.pair) {   // two cells per thread, linear order (k_project_cfl2)
    const bool wide = rq.wide && project_wide_path(g, cl, uout, uin, x, sigma, rq.skip_p ? nullptr : pout);
    *rep = TailRep{folded, wide};
    hipLaunchKernelGGL(k_enc_init, dim3(1), dim3(WL_ENC_SLOTS), 0, s, reinterpret_cast<int*>(ws.pm));
    if (wide) {   // four cells per thread, 16-byte accesses (k_project_wide)
      const dim3 grid(tw_grid(g, g.nz));
      if (rq.skip_p) hipLaunchKernelGGL((k_project_wide<1, 0>), grid, dim3(WL_BLOCK), tw_lds_bytes(g), s, g, uout, uin, x, pout, sigma, dt, cl, kfirst, klast, ws.pm, 0, g.nz, store_sigma, bc, tw_nb8(g));
      else hipLaunchKernelGGL((k_project_wide<1, 1>), grid, dim3(WL_BLOCK), tw_lds_bytes(g), s, g, uout, uin, x, pout, sigma, dt, cl, kfirst, klast, ws.pm, 0, g.nz, store_sigma, bc, tw_nb8(g));
    }
    else if (rq.skip_p) hipLaunchKernelGGL(k_project_cfl2<0>, dim3(pl_grid(g, g.nz)), dim3(WL_BLOCK), 0, s, g, uout, uin, x, pout, sigma, dt, cl, kfirst, klast, ws.pm, 0, g.nz, store_sigma, bc);
    else hipLaunchKernelGGL(k_project_cfl2<1>, dim3(pl_grid(g, g.nz)), dim3(WL_BLOCK), 0, s, g, uout, uin, x, pout, sigma, dt, cl, kfirst, klast, ws.pm, 0, g.nz, store_sigma, bc);
    hipLaunchKernelGGL(k_fin_max_enc, dim3(1), dim3(WL_BLOCK), 0, s, reinterpret_cast<const int*>(ws.pm), ws.res_f + slot_f);
    WL_LAUNCH_CHECK(); return 0;
  }
  *rep = TailRep{folded, false};
  const int zc = wl_march_chunk(g, g.nz);
  const dim3 grid = wl_plane_grid(g, wl_march_slots(g.nz, zc));
  DSEL2(g.D, cl.on, k_project_cfl, grid, dim3(WL_BLOCK), 0, s, g, uout, uin, L, x, pout, sigma, dt, cl, zc, kfirst, klast, ws.pm, 0, g.nz, store_sigma, bc);
  hipLaunchKernelGGL(k_fin_max2, dim3(1), dim3(WL_BLOCK), 0, s, ws.pm, (int)grid.x, ws.res_f + slot_f);
  WL_LAUNCH_CHECK(); return 0;
}
int project_cfl_split(float* uout, const float* uin, const float* L, const float* x, float* pout, float* sigma, const GridX& g, float dt, const ConstL& near, const ConstL& far,
                      int na, int nb, const RedWs& ws, int slot_f, hipStream_t s, int store_sigma) {
  if (uout == uin) { wl_set_error("project_cfl: output aliases input"); return WL_EINVAL; }
  int kfirst = 0, klast = 1;
  if (g.D == 3) { kfirst = (g.gk + g.k0 == 1) ? g.k0 - 1 : g.k0; klast = (g.gk + g.k1 == g.gnz - 1) ? g.k1 + 1 : g.k1; }
  const int lo[3] = {0, na, nb}, hi[3] = {na, nb, g.nz};
  int off = 0;
  for (int q = 0; q < 3; q++) {
    const int np = hi[q] - lo[q];
    if (np <= 0) continue;
    const ConstL& cl = q == 1 ? near : far;
    const int zc = wl_march_chunk(g, np);
    const dim3 grid = wl_plane_grid(g, wl_march_slots(np, zc));
    if (off + (int)grid.x > WL_MAXPART) { wl_set_error("project_cfl_split: too many partial maxima"); return WL_EINVAL; }
    DSEL2(g.D, cl.on, k_project_cfl, grid, dim3(WL_BLOCK), 0, s, g, uout, uin, L, x, pout, sigma, dt, cl, zc, kfirst, klast, ws.pm + off, lo[q], hi[q], store_sigma, no_bc);
    off += (int)grid.x;
  }
  hipLaunchKernelGGL(k_fin_max2, dim3(1), dim3(WL_BLOCK), 0, s, ws.pm, off, ws.res_f + slot_f);
  WL_LAUNCH_CHECK(); return 0;
}
}  // namespace wl
