// exitBC!(u,u⁰,Δt)   src/core.jl:226-233: the convective exit on the x-exit face of the normal component, all on the device.
// mode 0: U = mean of the inflow face u[2, inside, 1], then u[N,…] = u⁰[N,…] − U·Δt·(u⁰[N,…] − u⁰[N−1,…]);
// mode 1: the mean of the updated exit face minus U is taken off it (mass flux correction).
// The face is the rows 1..ny−2 of the planes [k0, k1): the whole inside on a single domain, the owned planes of a z-slab rank.
#include "wl_common.hpp"

namespace {
// Face sum by ONE block (deterministic).  mean_cnt == 0: *out = the sum of these planes (slabs: summed over the ranks before k_exit_mean).
// mean_cnt > 0 (single domain, out = sc): the arithmetic of k_exit_mean in the same launch.
__global__ void k_exit_facesum(GridX g, const float* __restrict__ u, int k0, int k1, double* __restrict__ out, long mean_cnt, int mode) {
  const int ny = g.ny - 2;
  const long cnt = (long)ny * (k1 - k0);
  const int ix = (mode == 0) ? 1 : g.nx - 1;
  double acc = 0.0;
  for (long q = threadIdx.x; q < cnt; q += blockDim.x) {
    const int j = 1 + (int)(q % ny), k = k0 + (int)(q / ny);
    acc += (double)u[ix + (long)j * g.sy + (long)k * g.sz];
  }
  __shared__ double sh[16];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0; for (int w = 0; w < (int)(blockDim.x >> 6); w++) s += sh[w];
    if (!mean_cnt) { *out = s; return; }
    const float mean = (float)s / (float)mean_cnt;
    if (mode == 0) out[0] = (double)mean; else out[1] = (double)(mean - (float)out[0]);
  }
}
// sc[0] = U, sc[1] = the correction: float division by the GLOBAL face size, exactly as above
__global__ void k_exit_mean(const double* __restrict__ gsum, double* __restrict__ sc, long cnt, int mode) {
  const float mean = (float)(*gsum) / (float)cnt;
  if (mode == 0) sc[0] = (double)mean; else sc[1] = (double)(mean - (float)sc[0]);
}
__global__ void k_exit_update(GridX g, float* __restrict__ u, const float* __restrict__ u0, const double* __restrict__ sc, float dt, int k0, int k1, int mode) {
  const int ny = g.ny - 2;
  const long cnt = (long)ny * (k1 - k0);
  const long q = (long)blockIdx.x * WL_BLOCK + threadIdx.x;
  if (q >= cnt) return;
  const int j = 1 + (int)(q % ny), k = k0 + (int)(q / ny);
  const long o = (g.nx - 1) + (long)j * g.sy + (long)k * g.sz;
  if (mode == 0) { const float U = (float)sc[0]; u[o] = u0[o] - U * dt * (u0[o] - u0[o - 1]); }
  else u[o] -= (float)sc[1];
}
// The x-exit face of the normal component (Julia index N of u[:,:,:,1], every row and plane): with the convective exit BC! leaves it alone
// (saveexit, src/core.jl:207) and only exitBC! rewrites its interior rows — so when the roles of the velocity buffers rotate instead of
// `u⁰ .= u` being a copy, the face has to travel with the role.
__global__ void k_copy_exit_face(GridX g, float* __restrict__ dst, const float* __restrict__ src) {
  const long cnt = (long)g.ny * g.nz;        // (2-D: nz = 1)
  const long q = (long)blockIdx.x * WL_BLOCK + threadIdx.x;
  if (q >= cnt) return;
  const long o = (g.nx - 1) + q * g.sy;      // (rows are contiguous over planes: j + k·ny)
  dst[o] = src[o];
}
unsigned face_blocks(const GridX& G, int k0, int k1) { return (unsigned)(((long)(G.ny - 2) * (k1 - k0) + WL_BLOCK - 1) / WL_BLOCK); }
}  // namespace

namespace wl {
int copy_exit_face(float* dst, const float* src, const GridX& G, hipStream_t s) {
  const long cnt = (long)G.ny * G.nz;
  hipLaunchKernelGGL(k_copy_exit_face, dim3((unsigned)((cnt + WL_BLOCK - 1) / WL_BLOCK)), dim3(WL_BLOCK), 0, s, G, dst, src);
  WL_LAUNCH_CHECK(); return 0;
}
// the whole face on this rank: inflow mean -> convective update (mode 0), its mean -> flux correction (mode 1); two launches per mode
int exit_bc_single(const GridX& G, float* u, const float* u0, double* sc, float dt, hipStream_t s) {
  const int k0 = G.D == 3 ? 1 : 0, k1 = G.D == 3 ? G.nz - 1 : 1;
  const long cnt = (long)(G.ny - 2) * (k1 - k0);
  for (int mode = 0; mode < 2; mode++) {
    hipLaunchKernelGGL(k_exit_facesum, dim3(1), dim3(1024), 0, s, G, (const float*)u, k0, k1, sc, cnt, mode);
    hipLaunchKernelGGL(k_exit_update, dim3(face_blocks(G, k0, k1)), dim3(WL_BLOCK), 0, s, G, u, u0, (const double*)sc, dt, k0, k1, mode);
  }
  WL_LAUNCH_CHECK(); return 0;
}
// z-slabs: this rank's planes of the face summed into *sum; the caller adds the ranks' sums (combine_results) …
int exit_bc_slab_sum(const GridX& G, const float* u, double* sum, int mode, hipStream_t s) {
  hipLaunchKernelGGL(k_exit_facesum, dim3(1), dim3(1024), 0, s, G, u, G.k0, G.k1, sum, 0L, mode);
  WL_LAUNCH_CHECK(); return 0;
}
// … then the global mean into sc and the update of this rank's planes
int exit_bc_slab_update(const GridX& G, float* u, const float* u0, const double* gsum, double* sc, float dt, int mode, hipStream_t s) {
  hipLaunchKernelGGL(k_exit_mean, dim3(1), dim3(1), 0, s, gsum, sc, (long)(G.ny - 2) * (G.gnz - 2), mode);
  hipLaunchKernelGGL(k_exit_update, dim3(face_blocks(G, G.k0, G.k1)), dim3(WL_BLOCK), 0, s, G, u, u0, (const double*)sc, dt, G.k0, G.k1, mode);
  WL_LAUNCH_CHECK(); return 0;
}
}  // namespace wl

extern "C" int wl_exit_bc(float* u, const float* u0, const wl_grid* g, float dt, void* st) {
  WL_CHECK(wl_grid_ok(g), "bad wl_grid"); WL_CHECK(g->D == 2 || g->nz == g->gnz, "exitBC! needs the whole x-exit face on one rank");
  WL_TRY(wl_ctx_ensure());
  return wl::exit_bc_single(gx(*g), u, u0, wl_red_ws(wl_ctx().red).res_d + WL_RD_EXIT, dt, wl_stream(st));
}
