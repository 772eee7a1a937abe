// _interp(_interp_clamp(x, size(arr)), arr) of src/util.jl:17-18,29-43 as device statements, for every file that samples an array at a point: the point
// samples, probes and tracers of wl_interp.hip and the lattice leaf of a body program (wl_lattice.hpp).  Device code only (gfx950).
//   ip_cell<D>   clamp :17-18, x += 1.5f :31, i = floor(x), y = x − i -> the offset of the lower corner and y
//   ip_sum<D>    the sum over the 2^D corners of CartesianIndices(I:I+1) in its own order (first dimension fastest), each weight the product over d of
//                (J_d == I_d ? 1−y_d : y_d) taken left to right, `s += arr[J]*weight` as a multiply and an add (@fastmath @simd leaves the reference's
//                association open; this is the written one, and tests/interp_ref.py states the same)
//   ip_grad<D>   ∂s/∂x_d with i held fixed — what ForwardDiff gives through _interp: the same corners in the same order, the factor of direction d
//                replaced by its derivative ∓1, the remaining factors multiplied on left to right
// The clamp is the bounds check: a clamped coordinate lies in [0, n_d − 2], so the lower corner index is in [0, n_d − 2] and the upper one is n_d − 1 at
// most.  It is written with fmaxf/fminf, which send a NaN coordinate to 0 (Julia's floor(Int, NaN) throws; a kernel must not index with it).  Offsets are
// 64-bit.  Nothing is contracted into FMAs.
#pragma once
#include "wl_common.hpp"

#pragma clang fp contract(off)

namespace {
template <int D>
__device__ __forceinline__ long ip_cell(const int (&ng)[3], const long (&st)[3], const float (&xq)[D], float (&y)[D]) {
  long o = 0;
#pragma unroll
  for (int d = 0; d < D; d++) {
    float c = fminf(fmaxf(xq[d], 0.f), (float)(ng[d] - 2));      // _interp_clamp :17-18
    c += 1.5f;                                                   // x = x .+ 1.5f0 :31
    const float fl = floorf(c);                                  // i = floor.(Int,x)
    y[d] = c - fl;                                               // y = x.-i
    o += (long)((int)fl - 1) * st[d];                            // Julia index i -> offset i − 1
  }
  return o;
}
template <int D>
__device__ __forceinline__ float ip_sum(const float* __restrict__ a, const long (&st)[3], long o, const float (&y)[D]) {
  float s = 0.f;                                                 // s = zero(T) :37
#pragma unroll
  for (int q = 0; q < (1 << D); q++) {                           // for J in I:I+oneunit(I) :38 — first dimension fastest
    float w = (q & 1) ? y[0] : 1.f - y[0];                       // prod(@. ifelse(J.I==I.I,1-y,y)) :39
    long oq = o + (q & 1);
#pragma unroll
    for (int d = 1; d < D; d++) { const int up = (q >> d) & 1; w = w * (up ? y[d] : 1.f - y[d]); oq += up ? st[d] : 0; }
    s += a[oq] * w;                                              // s += arr[J]*weight :40
  }
  return s;
}
template <int D>
__device__ __forceinline__ void ip_grad(const float* __restrict__ a, const long (&st)[3], long o, const float (&y)[D], float (&g)[D]) {
#pragma unroll
  for (int d = 0; d < D; d++) g[d] = 0.f;
#pragma unroll
  for (int q = 0; q < (1 << D); q++) {
    long oq = o;
#pragma unroll
    for (int d = 0; d < D; d++) oq += ((q >> d) & 1) ? st[d] : 0;
    const float v = a[oq];
#pragma unroll
    for (int d = 0; d < D; d++) {
      float w = ((q >> d) & 1) ? 1.f : -1.f;                     // ∂/∂y_d of ifelse(J_d==I_d, 1−y_d, y_d)
#pragma unroll
      for (int e = 0; e < D; e++) if (e != d) w = w * (((q >> e) & 1) ? y[e] : 1.f - y[e]);
      g[d] += v * w;
    }
  }
}
}  // namespace
