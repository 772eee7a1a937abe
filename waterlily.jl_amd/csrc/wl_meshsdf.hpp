// Distance fields from closed meshes (include/wlhip.h wl_sdf_lattice_from_mesh): the host side — the refusals and the tables a mesh is turned into — and the
// launcher of the all-pairs search with culling (wl_meshsdf.hip).  wl_lattice.hip owns the table of live lattices and calls these.
#pragma once
#include <vector>

#include "wl_common.hpp"

namespace wl {
// What the kernel reads, built on the host in Float64 and rounded to Float32 once.  Per element (triangle / segment) t:
//   elem[t·D·D …]      its D vertices, D coordinates each (the indices are resolved here: the device follows no index)
//   sph[t·4 …]         a bounding sphere (centre, radius; 2-D: z = 0), the smallest one, its radius rounded outwards
//   nrm[(t·NR + r)·D …] the unit pseudonormal of region r of the closest-point walk, NR = 7 (3-D: face, edges AB BC CA, vertices A B C) or 3 (2-D: interior, A, B)
//   wtab[t·D·D …]      (moving meshes only, else empty) the velocities of its D vertices, laid out like elem: a sample gathers its winner's row once
struct MeshTables {
  int D = 0; int32_t ne = 0;
  std::vector<float> elem, sph, nrm, wtab;
  double scale = 0;      // max |coordinate| of the mesh
  // the topology, left by meshsdf_prepare for the caller to keep: adj[t·D + k] — 3-D: the triangle across edge k of t; 2-D: the segment into A (k = 0) / out of
  // B (k = 1).  It depends on the connectivity alone, so a re-bake with moved vertices passes it to meshsdf_prepare_geometry instead of building it again
  std::vector<int32_t> adj;
};
// the refusals of wl_sdf_lattice_from_mesh that concern the mesh (counts, finite vertices, indices, zero area, the edge rule, orientation) in that order —
// WL_EINVAL with the reason, prefixed with `who` — then the tables.  Host only: nothing is allocated on the device, nothing launched.
int meshsdf_prepare(int D, const float* v, int32_t nv, const int32_t* e, int32_t ne, MeshTables* out, const char* who = "wl_sdf_lattice_from_mesh");
// the geometry part alone, for vertices that moved under a connectivity meshsdf_prepare has accepted (adj: what it left): the finite check, normals, zero-area
// and orientation refusals, angle weights, spheres and the rounded tables — the statements of meshsdf_prepare in their order, so the same table bits; the
// index checks, the edge map and the 2-D in/out tables are not repeated.  out->adj is left alone.
int meshsdf_prepare_geometry(int D, const float* v, int32_t nv, const int32_t* e, int32_t ne, const std::vector<int32_t>& adj, MeshTables* out, const char* who);
// wtab of `out` from the vertex velocities w (nv×D) and the (already checked) indices; WL_EINVAL for a velocity that is not finite.  Host only.
int meshsdf_velocities(int D, const float* w, int32_t nv, const int32_t* e, int32_t ne, MeshTables* out, const char* who);
// the samples of a lattice of n[0..D) samples at c + s·(i − ½) into a_dev on stream st, and from there into a_host; synchronises st.  flags: WL_MESH_BRUTE.
// band > 0: the band-limited instantiations — every sample clip(d, −band, +band), zero velocity beyond, bricks wholly beyond the band not searched; 0: as ever
// w_dev non-NULL (m.wtab filled): the instantiation that also stores the closest-point extension of the vertex velocities, D component planes, into w_dev
int meshsdf_run(const MeshTables& m, const int32_t* n, const float* c, float s, float band, unsigned flags, float* a_dev, float* a_host, float* w_dev, hipStream_t st);
void meshsdf_note_tables_ms(double ms);      // wl_meshsdf_last_times[0]: what the caller spent in meshsdf_prepare / meshsdf_velocities
}  // namespace wl
