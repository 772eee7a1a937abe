// Position-dependent boundary profiles and body forces on the device, in separable form (include/wlhip.h, separable terms):
//   uBC(i,x,t) = Σₖ bₖ(t)·Fₖ[I,i]      g(i,x,t) + ∂ₜuBC(i,x,t) = Σₖ aₖ(t)·Fₖ[I,i]      k < K ≤ 4
// Fₖ: device arrays of the shape of u holding the spatial factor at loc(i,I); the K coefficients come from the host with every launch.
//
// The combination is formed in ONE order everywhere (tests/terms_ref.py restates it): s = c₀·F₀ ; s = s + cₖ·Fₖ for k = 1 … K−1, every product and every
// sum rounded to Float32 (the build is -ffp-contract=off), no term skipped — a zero coefficient is multiplied and added like any other.
//
// k_accel_terms<K, T>: accelerate!(r,t,g,uBC) on ALL cells (src/Flow.jl:69-73), r[q] = r[q] + s.  Element-wise, linear block order, grid-stride.  T = float4:
// four consecutive elements per thread as 16-byte accesses — needs a count that is a multiple of 4 and 16-byte aligned r and Fₖ; anything else takes T = float
// (one element per thread, the same statements).  (K+2)·4 B per element: K reads, r read and written.
// k_bc_vec_terms<D, K>: BC!(a,uBC::Function,saveexit,perdir,t) (src/core.jl:201-219) — the chain logic of k_bc_vec_fn (wl_bc_chain.hpp) with every table
// read replaced by the combination; only the two outermost layers of the non-periodic directions of the Fₖ are read.
#include "wl_common.hpp"
#include "wl_bc_chain.hpp"
#include "wl_terms.hpp"

namespace {
inline unsigned tm_grid1d(size_t n) { size_t b = (n + WL_BLOCK - 1) / WL_BLOCK; if (b > 4096) b = 4096; if (b < 1) b = 1; return (unsigned)b; }      // (grid1d of wl_flow.hip: the same cap)

__device__ __forceinline__ float tm_mul(float c, float x) { return c * x; }
__device__ __forceinline__ float4 tm_mul(float c, const float4& x) { return make_float4(c * x.x, c * x.y, c * x.z, c * x.w); }
__device__ __forceinline__ float tm_add(float a, float b) { return a + b; }
__device__ __forceinline__ float4 tm_add(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

template <int K, typename T> struct TermSet { const T* F[K]; float c[K]; };      // kernel argument: K pointers and K coefficients (constant indices only: they stay in SGPRs)
// the combination at element q, in the written order
template <int K, typename T>
__device__ __forceinline__ T tm_combine(const TermSet<K, T>& A, long q) {
  T s = tm_mul(A.c[0], A.F[0][q]);
#pragma unroll
  for (int k = 1; k < K; k++) s = tm_add(s, tm_mul(A.c[k], A.F[k][q]));
  return s;
}
// T = float (n elements) or float4 (n quads)
template <int K, typename T>
__global__ void __launch_bounds__(WL_BLOCK) k_accel_terms(T* __restrict__ r, TermSet<K, T> A, long n) {
  for (long q = (long)blockIdx.x * WL_BLOCK + threadIdx.x; q < n; q += (long)gridDim.x * WL_BLOCK) r[q] = tm_add(r[q], tm_combine<K, T>(A, q));
}
template <int K> struct BcTermSrc {
  TermSet<K, float> A;
  __device__ __forceinline__ float operator()(long o) const { return tm_combine<K, float>(A, o); }
};
template <int D, int K>
__global__ void k_bc_vec_terms(GridX g, float* __restrict__ a_, TermSet<K, float> A, int saveexit, unsigned per, int zwalls) {
  bc_vec_chain<D>(g, a_, BcTermSrc<K>{A}, saveexit, per, zwalls);
}

template <int K>
void accel_launch(float* r, const float* const* F, const float* c, size_t n, hipStream_t s) {
  size_t al = (size_t)r;
  for (int k = 0; k < K; k++) al |= (size_t)F[k];
  if (n % 4 == 0 && (al & 15) == 0) {
    TermSet<K, float4> A;
    for (int k = 0; k < K; k++) { A.F[k] = (const float4*)F[k]; A.c[k] = c[k]; }
    hipLaunchKernelGGL((k_accel_terms<K, float4>), dim3(tm_grid1d(n / 4)), dim3(WL_BLOCK), 0, s, (float4*)r, A, (long)(n / 4));
  } else {
    TermSet<K, float> A;
    for (int k = 0; k < K; k++) { A.F[k] = F[k]; A.c[k] = c[k]; }
    hipLaunchKernelGGL((k_accel_terms<K, float>), dim3(tm_grid1d(n)), dim3(WL_BLOCK), 0, s, r, A, (long)n);
  }
}
template <int D, int K>
void bc_launch(float* a, const float* const* F, const float* b, const GridX& g, int saveexit, unsigned per, hipStream_t s) {
  TermSet<K, float> A;
  for (int k = 0; k < K; k++) { A.F[k] = F[k]; A.c[k] = b[k]; }
  int zwalls; const dim3 grid = bc_chain_grid(g, per, &zwalls);
  hipLaunchKernelGGL((k_bc_vec_terms<D, K>), grid, dim3(WL_BLOCK), 0, s, g, a, A, saveexit, per, zwalls);
}
int terms_args_ok(const char* who, const void* a, int K, const float* const* F, const float* c) {
  if (!a || !F || !c || K < 1 || K > wl::TERMS_MAX) { wl_set_error(std::string(who) + ": null argument or K outside 1 … 4"); return WL_EINVAL; }
  for (int k = 0; k < K; k++) if (!F[k]) { wl_set_error(std::string(who) + ": a NULL field"); return WL_EINVAL; }
  return 0;
}
}  // namespace

namespace wl {
int accel_terms(float* r, int K, const float* const* F, const float* c, size_t n, hipStream_t s) {
  WL_TRY(terms_args_ok("accel_terms", r, K, F, c));
  if (n == 0) return 0;
  switch (K) {
    case 1: accel_launch<1>(r, F, c, n, s); break;
    case 2: accel_launch<2>(r, F, c, n, s); break;
    case 3: accel_launch<3>(r, F, c, n, s); break;
    default: accel_launch<4>(r, F, c, n, s); break;
  }
  WL_LAUNCH_CHECK(); return 0;
}
int bc_vec_terms(float* a, int K, const float* const* F, const float* b, const GridX& g, int saveexit, unsigned per, hipStream_t s) {
  WL_TRY(terms_args_ok("bc_vec_terms", a, K, F, b));
  if (g.D != 2 && g.D != 3) { wl_set_error("bc_vec_terms: bad D"); return WL_EINVAL; }
#define WL_TERMS_BC(KK) do { if (g.D == 3) bc_launch<3, KK>(a, F, b, g, saveexit, per, s); else bc_launch<2, KK>(a, F, b, g, saveexit, per, s); } while (0)
  switch (K) {
    case 1: WL_TERMS_BC(1); break;
    case 2: WL_TERMS_BC(2); break;
    case 3: WL_TERMS_BC(3); break;
    default: WL_TERMS_BC(4); break;
  }
#undef WL_TERMS_BC
  WL_LAUNCH_CHECK(); return 0;
}
}  // namespace wl
