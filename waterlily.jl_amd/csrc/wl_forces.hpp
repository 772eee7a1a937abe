// Band list of a body program and the one-pass force/moment kernel over it (wl_forces.hip).
#pragma once
#include "wl_common.hpp"
#include "wl_body.hpp"

// A tile is WL_FT_X × WL_FT_Y × WL_FT_Z cells of the ARRAY (ghost cells included in the count, never evaluated), aligned to the array origin: one wave reads
// one contiguous row of 64 cells, the four waves of a workgroup the four rows of a plane, and the workgroup walks the tile's planes.  2-D: one plane.
#define WL_FT_X 64
#define WL_FT_Y 4
#define WL_FT_Z 4

namespace wl {
// The active tiles of one body program on one grid — those with at least one interior cell at d² ≤ 1, where nds(body,x) can be non-zero — in ascending
// tile order, and the workspace of the one-pass kernel.  Owned by whoever holds it (release() frees); an empty list is legal.
struct ForceBand {
  int *flag = nullptr, *list = nullptr, *count = nullptr;   // device: one flag per tile; the compacted tile indices; their number
  double *part = nullptr, *out = nullptr;                   // device: 12 × n_active partial sums (quantity-major); 12 results of an immediate read-out
  int n_tiles = 0, n_active = 0, part_cap = 0;
  bool valid = false;                                       // `list` is the list of `P` on `tiles_of`'s grid
  SetArg P;
  static int tiles(const GridX& G, int* ntx = nullptr, int* nty = nullptr);
  // two launches (classify, single-workgroup scan) and one read-back of the count; reuses the list if the program is the one it was built for
  int build(const GridX& G, const SetArg& prog, hipStream_t s);
  // k_forces_band over the list + k_forces_fin: 12 doubles to dst (device) — pressure force, viscous force, pressure moment, viscous moment about x0,
  // three slots each.  An empty list launches the finish alone, which writes zeros.
  // The stored program is resolved again first: WL_EINVAL, and no launch, when a lattice it names has been destroyed since the list was built.
  int run(const GridX& G, const float* p, const float* u, float nu, const float* x0, double* dst, hipStream_t s);
  int recheck(int D);      // that resolution alone (a time step with a recorder asks before it launches anything)
  void release();
};
}  // namespace wl
