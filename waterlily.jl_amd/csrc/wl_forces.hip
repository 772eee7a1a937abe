// Force and moment read-outs from the body's band only (src/Metrics.jl:116-188).  nds(body,x) = n·kern(clamp(d,−1,1)) at fastd² = 1 is exactly zero
// outside |d| ≤ 1, so the four sums — pressure force, viscous force and their moments — need the cells of the band and nothing else.  A body program
// is classified once per measure! into a compact, ordered list of active tiles (two launches); afterwards one launch with one workgroup per active
// tile evaluates the body once per cell and accumulates all twelve Float64 sums, and a single-workgroup finish adds the per-tile partials in list
// order: a fixed number of launches per read-out, no atomics, the same bits run to run.
#include "wl_common.hpp"
#include "wl_body.hpp"
#include "wl_bodyset_dev.hpp"
#include "wl_forces.hpp"

#include <cstring>

static_assert(WL_FT_X == WL_WAVE && WL_FT_X * WL_FT_Y == WL_BLOCK, "one wave per row of a tile, one workgroup per plane of a tile");

namespace {
struct TileGeom { int ntx, nty, nz_t; };      // tiles per row, rows of tiles per plane, planes a tile spans (1 in 2-D)
// thread -> its cell (i, j) of the tile and the tile's first plane k; false for a cell that is not an interior cell in x or y
__device__ __forceinline__ bool tile_cell(const GridX& g, const TileGeom& t, int tile, int& i, int& j, int& kfirst) {
  const int tx = tile % t.ntx, r = tile / t.ntx, ty = r % t.nty, tz = r / t.nty;
  i = tx * WL_FT_X + (int)(threadIdx.x & 63);
  j = ty * WL_FT_Y + (int)(threadIdx.x >> 6);
  kfirst = tz * t.nz_t;
  return i >= 1 && i <= g.nx - 2 && j >= 1 && j <= g.ny - 2;
}
__device__ __forceinline__ bool plane_inside(const GridX& g, int k) { return k >= g.k0 && k < g.k1; }

// flag[tile] = 1 iff an interior cell of the tile has d² ≤ 1, d from the same set_measure call the force kernels make.  One workgroup per tile.
template <int DS>
__global__ void __launch_bounds__(WL_BLOCK) k_band_classify(GridX g, TileGeom t, SetArg P, int* __restrict__ flag) {
  constexpr int D = DS_D, S = DS_S;
  int i, j, kf;
  const bool in = tile_cell(g, t, (int)blockIdx.x, i, j, kf);
  int any = 0;
  if (in)
    for (int kz = 0; kz < t.nz_t; kz++) {
      const int k = kf + kz;
      if (!plane_inside(g, k)) continue;
      float x[3]; cell_centre<D>(g, i, j, k, x);
      float d, n[3], v[3]; set_measure<D, S>(P, x, 1.f, d, n, v);
      any |= (d * d <= 1.f) ? 1 : 0;
    }
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) flag[blockIdx.x] = any ? 1 : 0;
}
// list = the indices of the set flags in ascending order, *count = their number.  ONE workgroup: thread q owns a contiguous chunk of tiles, the chunk
// counts are scanned in LDS, every thread writes its indices behind those of the threads before it.
__global__ void __launch_bounds__(WL_BLOCK) k_band_scan(const int* __restrict__ flag, int nt, int* __restrict__ list, int* __restrict__ count) {
  __shared__ int sh[WL_BLOCK];
  const int tid = (int)threadIdx.x, per = (nt + WL_BLOCK - 1) / WL_BLOCK;
  const int a = tid * per < nt ? tid * per : nt, b = a + per < nt ? a + per : nt;
  int c = 0;
  for (int q = a; q < b; q++) c += flag[q] != 0;
  sh[tid] = c;
  __syncthreads();
  for (int o = 1; o < WL_BLOCK; o <<= 1) {
    const int v = tid >= o ? sh[tid - o] : 0;
    __syncthreads();
    sh[tid] += v;
    __syncthreads();
  }
  int pos = sh[tid] - c;                                  // (pos + c ≤ the total ≤ nt: inside `list`)
  for (int q = a; q < b; q++) if (flag[q] != 0) list[pos++] = q;
  if (tid == WL_BLOCK - 1) *count = sh[tid];
}
// One workgroup per ACTIVE tile: per cell one set_measure, one kern_, p[I] and the ∂(i,j,I,u) stencil; the twelve sums in Float64.
// part[q·na + b]: quantity q (0-2 pressure force, 3-5 viscous force, 6-8 pressure moment, 9-11 viscous moment) of list entry b.
template <int DS>
__global__ void __launch_bounds__(WL_BLOCK) k_forces_band(GridX g, TileGeom t, const int* __restrict__ list, int na, const float* __restrict__ p, const float* __restrict__ u,
                                                          float nu, SetArg P, MomArg mo, double* __restrict__ part) {
  constexpr int D = DS_D, S = DS_S;
  int i, j, kf;
  const bool in = tile_cell(g, t, list[blockIdx.x], i, j, kf);
  double acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const long st[3] = {1, g.sy, g.sz};
  if (in)
    for (int kz = 0; kz < t.nz_t; kz++) {
      const int k = kf + kz;
      if (!plane_inside(g, k)) continue;
      float x[3]; cell_centre<D>(g, i, j, k, x);
      float d, n[3], v[3]; set_measure<D, S>(P, x, 1.f, d, n, v);
      const float kk = kern_(fminf(fmaxf(d, -1.f), 1.f));
      const long o = (long)i + (long)j * g.sy + (long)k * g.sz;
      const float pv = p[o];
      float tm[3];
      pforce_cell<D>(0, mo.x0, pv, n, kk, x, tm);
      for (int a = 0; a < D; a++) acc[a] += (double)tm[a];
      vforce_cell<D>(0, mo.x0, u, g.cs, o, st, nu, n, kk, x, tm);
      for (int a = 0; a < D; a++) acc[3 + a] += (double)tm[a];
      pforce_cell<D>(1, mo.x0, pv, n, kk, x, tm);
      for (int a = 0; a < D; a++) acc[6 + a] += (double)tm[a];
      vforce_cell<D>(1, mo.x0, u, g.cs, o, st, nu, n, kk, x, tm);
      for (int a = 0; a < D; a++) acc[9 + a] += (double)tm[a];
    }
  const long b = blockIdx.x;
  for (int q = 0; q < 12; q++) { const double s = block_sum(acc[q]); if (threadIdx.x == 0) part[(long)q * na + b] = s; __syncthreads(); }
}
// dst[q] = Σ_b part[q·na + b], the entries of one thread in list order, the threads by block_sum's fixed tree.  na = 0: zeros.  ONE workgroup.
__global__ void __launch_bounds__(WL_BLOCK) k_forces_fin(const double* __restrict__ part, int na, double* __restrict__ dst) {
  for (int q = 0; q < 12; q++) {
    double s = 0.0;
    for (int b = (int)threadIdx.x; b < na; b += WL_BLOCK) s += part[(long)q * na + b];
    s = block_sum(s);
    if (threadIdx.x == 0) dst[q] = s;
    __syncthreads();
  }
}
}  // namespace

namespace wl {
int ForceBand::tiles(const GridX& G, int* ntx, int* nty) {
  const int tx = (G.nx + WL_FT_X - 1) / WL_FT_X, ty = (G.ny + WL_FT_Y - 1) / WL_FT_Y, tz = G.D == 3 ? (G.nz + WL_FT_Z - 1) / WL_FT_Z : 1;
  if (ntx) *ntx = tx;
  if (nty) *nty = ty;
  return tx * ty * tz;
}
static TileGeom tile_geom(const GridX& G) { TileGeom t; (void)ForceBand::tiles(G, &t.ntx, &t.nty); t.nz_t = G.D == 3 ? WL_FT_Z : 1; return t; }

int ForceBand::build(const GridX& G, const SetArg& prog, hipStream_t s) {
  WL_TRY(bodyset_lattice_margin(prog, 2.f, "force band"));
  const long nt = tiles(G);
  WL_CHECK(nt >= 1 && nt < (1L << 30), "force band: tile count out of range");
  if (valid && n_tiles == (int)nt && std::memcmp(&P, &prog, sizeof(SetArg)) == 0) return 0;
  valid = false;
  if (!flag || n_tiles != (int)nt) {
    release();
    WL_HIP(hipMalloc((void**)&flag, sizeof(int) * (size_t)(2 * nt + 1)));
    list = flag + nt; count = list + nt;
    WL_HIP(hipMalloc((void**)&out, sizeof(double) * 12));
    n_tiles = (int)nt;
  }
  std::memcpy(&P, &prog, sizeof(SetArg));
  const TileGeom t = tile_geom(G);
  BSEL(G.D, P.depth, k_band_classify, dim3((unsigned)nt), dim3(WL_BLOCK), 0, s, G, t, P, flag);
  hipLaunchKernelGGL(k_band_scan, dim3(1), dim3(WL_BLOCK), 0, s, (const int*)flag, (int)nt, list, count);
  WL_LAUNCH_CHECK();
  int na = 0;
  WL_HIP(hipMemcpyAsync(&na, count, sizeof(int), hipMemcpyDeviceToHost, s));
  WL_HIP(hipStreamSynchronize(s));
  WL_CHECK(na >= 0 && na <= (int)nt, "force band: the scan returned a count outside the tile range");
  if (na > part_cap) {
    if (part) WL_HIP(hipFree(part));
    part = nullptr; part_cap = 0;
    WL_HIP(hipMalloc((void**)&part, sizeof(double) * 12 * (size_t)na));
    part_cap = na;
  }
  n_active = na;
  valid = true;
  return 0;
}
int ForceBand::run(const GridX& G, const float* p, const float* u, float nu, const float* x0, double* dst, hipStream_t s) {
  WL_CHECK(valid && p && u && dst, "force band: not built, or a null array");
  WL_TRY(recheck(G.D));
  MomArg mo{}; mo.on = 1; for (int c = 0; c < G.D; c++) mo.x0[c] = x0 ? x0[c] : 0.f;
  if (n_active > 0) {      // (never a zero-sized launch)
    const TileGeom t = tile_geom(G);
    BSEL(G.D, P.depth, k_forces_band, dim3((unsigned)n_active), dim3(WL_BLOCK), 0, s, G, t, (const int*)list, n_active, p, u, nu, P, mo, part);
  }
  hipLaunchKernelGGL(k_forces_fin, dim3(1), dim3(WL_BLOCK), 0, s, (const double*)part, n_active, dst);
  WL_LAUNCH_CHECK();
  return 0;
}
int ForceBand::recheck(int D) { return valid ? bodyset_resolve(D, &P) : 0; }      // (resolving keeps LatRef::gen as stored: see wl::bodyset_resolve)
void ForceBand::release() {
  if (flag) (void)hipFree(flag);
  if (out) (void)hipFree(out);
  if (part) (void)hipFree(part);
  flag = list = count = nullptr; part = out = nullptr;
  n_tiles = n_active = part_cap = 0; valid = false;
}
}  // namespace wl
