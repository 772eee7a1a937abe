// MeanFlow as an observer of a handle (wl_sim_set_meanflow; src/Metrics.jl:205-262): the update of the time averages P, U and UU = ⟨u⊗u⟩ over every cell of the
// arrays, ghost cells included, and the expansion of the packed UU into the reference's (N…, D, D) layout (or uu!'s τ = UU − U⊗U).
//
// UU is stored PACKED: only the components i ≤ j, plane mf_pk(i,j) = i + j(j+1)/2 of cs floats each — 6 planes in 3-D, 3 in 2-D.  UU[I,i,j] and UU[I,j,i]
// receive the same statement with commuted factors (Float32 multiplication commutes bit for bit), so the lower triangle is the upper one and nothing is lost.
// Own bytes per cell in 3-D with UU: 16 read of p and u, 40 read + 40 written of the averages = 96 (the leaf k_meanflow, wl_flow.hip: 120).
//
// k_mean_update<D, UUON, VEC>: element-wise, linear block order, grid-stride.  VEC: four consecutive cells per thread as 16-byte quads — every plane base is a
// multiple of cs floats, so this form needs cs % 4 == 0 and 16-byte aligned arrays; anything else takes the scalar instance (one cell per thread, same statements).
// The build is -ffp-contract=off: the bits are the unfused Float32 statements of update!, the ones k_meanflow produces.
#include "wl_common.hpp"
#include "wl_meanflow.hpp"

namespace {
__host__ __device__ constexpr int mf_pk(int i, int j) { return i + j * (j + 1) / 2; }      // i ≤ j
inline unsigned mf_grid1d(size_t n) { size_t b = (n + WL_BLOCK - 1) / WL_BLOCK; if (b > 4096) b = 4096; if (b < 1) b = 1; return (unsigned)b; }      // (grid1d of wl_flow.hip: the same cap)

__device__ __forceinline__ float mf_avg(float e, float one_m, float x, float X) { return e * x + one_m * X; }
__device__ __forceinline__ float4 mf_avg(float e, float one_m, const float4& x, const float4& X) {
  return make_float4(mf_avg(e, one_m, x.x, X.x), mf_avg(e, one_m, x.y, X.y), mf_avg(e, one_m, x.z, X.z), mf_avg(e, one_m, x.w, X.w));
}
__device__ __forceinline__ float mf_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float4 mf_mul(const float4& a, const float4& b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }

// T = float (n = cs cells) or float4 (n = cs/4 quads, pl = cs/4 quads per plane)
template <int D, bool UUON, typename T>
__global__ void __launch_bounds__(WL_BLOCK) k_mean_update(T* __restrict__ P, T* __restrict__ U, T* __restrict__ UU, const T* __restrict__ p, const T* __restrict__ u, long n, float e) {
  const float one_m = 1 - e;
  for (long q = (long)blockIdx.x * WL_BLOCK + threadIdx.x; q < n; q += (long)gridDim.x * WL_BLOCK) {
    T uv[D];
#pragma unroll
    for (int i = 0; i < D; i++) uv[i] = u[(long)i * n + q];
    P[q] = mf_avg(e, one_m, p[q], P[q]);
#pragma unroll
    for (int i = 0; i < D; i++) U[(long)i * n + q] = mf_avg(e, one_m, uv[i], U[(long)i * n + q]);
    if (UUON) {
#pragma unroll
      for (int j = 0; j < D; j++)
#pragma unroll
        for (int i = 0; i <= j; i++) { const long o = (long)mf_pk(i, j) * n + q; UU[o] = mf_avg(e, one_m, mf_mul(uv[i], uv[j]), UU[o]); }
    }
  }
}
// out[I,i,j] = UU[I,i,j] (tau = 0) or UU[I,i,j] − U[I,i]·U[I,j] (uu!, :250-252), from the packed planes
template <int D>
__global__ void __launch_bounds__(WL_BLOCK) k_mean_expand(float* __restrict__ out, const float* __restrict__ UU, const float* __restrict__ U, long cs, int tau) {
  for (long q = (long)blockIdx.x * WL_BLOCK + threadIdx.x; q < cs; q += (long)gridDim.x * WL_BLOCK) {
    float Uv[D];
#pragma unroll
    for (int i = 0; i < D; i++) Uv[i] = tau ? U[(long)i * cs + q] : 0.f;
#pragma unroll
    for (int j = 0; j < D; j++)
#pragma unroll
      for (int i = 0; i < D; i++) {
        const float v = UU[(long)(i <= j ? mf_pk(i, j) : mf_pk(j, i)) * cs + q];
        out[(long)(i + j * D) * cs + q] = tau ? v - Uv[i] * Uv[j] : v;
      }
  }
}
template <int D, bool UUON>
void mean_launch(float* P, float* U, float* UU, const float* p, const float* u, long cs, float e, hipStream_t s) {
  const size_t al = (size_t)P | (size_t)U | (size_t)UU | (size_t)p | (size_t)u;
  if (cs % 4 == 0 && (al & 15) == 0) {
    const long n4 = cs / 4;
    hipLaunchKernelGGL((k_mean_update<D, UUON, float4>), dim3(mf_grid1d((size_t)n4)), dim3(WL_BLOCK), 0, s, (float4*)P, (float4*)U, (float4*)UU, (const float4*)p, (const float4*)u, n4, e);
  } else {
    hipLaunchKernelGGL((k_mean_update<D, UUON, float>), dim3(mf_grid1d((size_t)cs)), dim3(WL_BLOCK), 0, s, P, U, UU, p, u, cs, e);
  }
}
}  // namespace

namespace wl {
int meanflow_packed_planes(int D) { return D * (D + 1) / 2; }
// one launch: P, U (and the packed UU unless it is NULL) take the sample (p, u) with weight e
int meanflow_observe(float* P, float* U, float* UU, const float* p, const float* u, const GridX& g, float e, hipStream_t s) {
  if (!P || !U || !p || !u || (g.D != 2 && g.D != 3)) { wl_set_error("meanflow_observe: null array or bad D"); return WL_EINVAL; }
  if (g.D == 3) { if (UU) mean_launch<3, true>(P, U, UU, p, u, g.cs, e, s); else mean_launch<3, false>(P, U, nullptr, p, u, g.cs, e, s); }
  else { if (UU) mean_launch<2, true>(P, U, UU, p, u, g.cs, e, s); else mean_launch<2, false>(P, U, nullptr, p, u, g.cs, e, s); }
  WL_LAUNCH_CHECK(); return 0;
}
int meanflow_expand(float* out, const float* UU, const float* U, const GridX& g, int tau, hipStream_t s) {
  if (!out || !UU || !U || (g.D != 2 && g.D != 3)) { wl_set_error("meanflow_expand: null array or bad D"); return WL_EINVAL; }
  if (g.D == 3) hipLaunchKernelGGL(k_mean_expand<3>, dim3(mf_grid1d((size_t)g.cs)), dim3(WL_BLOCK), 0, s, out, UU, U, g.cs, tau);
  else hipLaunchKernelGGL(k_mean_expand<2>, dim3(mf_grid1d((size_t)g.cs)), dim3(WL_BLOCK), 0, s, out, UU, U, g.cs, tau);
  WL_LAUNCH_CHECK(); return 0;
}
}  // namespace wl
