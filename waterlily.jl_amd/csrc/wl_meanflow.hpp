// The MeanFlow observer's kernels (wl_meanflow.hip): the update of P, U and the packed UU, and the expansion of the packed UU.
#pragma once
#include "wl_common.hpp"

namespace wl {
int meanflow_packed_planes(int D);      // D(D+1)/2 planes of cs floats: the components i ≤ j, plane i + j(j+1)/2
// P = e·p + (1−e)·P ; U[·,i] = e·u[·,i] + (1−e)·U[·,i] ; UU[·,i,j] = e·(u[·,i]·u[·,j]) + (1−e)·UU[·,i,j] (i ≤ j; UU may be NULL) on all g.cs cells: one launch
int meanflow_observe(float* P, float* U, float* UU, const float* p, const float* u, const GridX& g, float e, hipStream_t s);
// out (cs·D·D floats, the reference's layout) = UU, or UU − U⊗U with tau != 0
int meanflow_expand(float* out, const float* UU, const float* U, const GridX& g, int tau, hipStream_t s);
}  // namespace wl
