// Position-dependent boundary profiles and body forces in separable form (wl_terms.hip): uBC(i,x,t) = Σₖ bₖ(t)·Fₖ[I,i], g(i,x,t) = Σₖ gₖ(t)·Fₖ[I,i], k < K ≤ 4.
#pragma once
#include "wl_common.hpp"

namespace wl {
constexpr int TERMS_MAX = 4;
// r[q] += Σₖ c[k]·F[k][q] over n elements, the sum formed in the order k = 0 … K−1 (one launch; K = 1 … TERMS_MAX, host pointers F[k] to device arrays)
int accel_terms(float* r, int K, const float* const* F, const float* c, size_t n, hipStream_t s);
// BC!(a,uBC::Function,saveexit,perdir,t) with uBC = Σₖ b[k]·F[k] formed on the fly (one launch, the launch geometry of bc_vec_fn)
int bc_vec_terms(float* a, int K, const float* const* F, const float* b, const GridX& g, int saveexit, unsigned per, hipStream_t s);
}  // namespace wl
