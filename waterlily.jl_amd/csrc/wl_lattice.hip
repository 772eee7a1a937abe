// Sampled distance fields (include/wlhip.h wl_sdf_lattice): what measure_sdf!(a, body) (src/Body.jl:74) leaves in a scalar array, copied to the device and
// entered into a process-wide table of at most WL_LATTICE_MAX live lattices.  A body program names a lattice by its id; bodyset_prepare looks the id up here
// and a stored program is looked up again before every launch, so a kernel only ever sees the pointer of a live lattice.  Host code only: the leaf's device
// statements are in wl_lattice.hpp.
#include <chrono>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "wl_common.hpp"
#include "wl_lattice.hpp"
#include "wl_meshsdf.hpp"

// w: the velocity samples (D planes of count floats, device) or NULL; gen: in-place re-fills so far (LatRef::gen).  A lattice from a mesh keeps on the host what a
// re-bake needs: where its samples sit, the connectivity and the vertices of its last bake.
struct wl_sdf_lattice {
  int32_t id; int32_t D; int32_t n[3]; float* a; float edge_min;
  float* w = nullptr; int32_t gen = 0;
  bool from_mesh = false; float origin[3] = {0.f, 0.f, 0.f}; float spacing = 0.f; int32_t nv = 0, ne = 0;
  std::vector<int32_t> elems; std::vector<float> verts;
  std::vector<int32_t> adj;      // the topology of elems (MeshTables::adj), computed once at creation: a re-bake rebuilds the geometry tables only
  float band = 0.f;              // > 0: made by wl_sdf_lattice_from_mesh_band — the samples are clip(d, −band, +band), every re-bake keeps it
};

namespace {
std::mutex g_lat_mutex;
wl_sdf_lattice* g_lat[WL_LATTICE_MAX] = {};
int g_lat_next_id = 1;      // ids are never reused within a process

// min|A| over the samples a query clamped in some direction reads — the two outermost layers of every direction — or 0 when they differ in sign: the value
// outside the box is a convex combination of such samples, so with one sign its magnitude is at least this
float edge_min_of(int D, const int32_t* n, const float* a) {
  float lo = INFINITY; bool pos = false, neg = false;
  const long nx = n[0], ny = n[1], nz = D == 3 ? n[2] : 1;
  for (long k = 0; k < nz; k++)
    for (long j = 0; j < ny; j++)
      for (long i = 0; i < nx; i++) {
        const bool edge = i < 2 || i >= nx - 2 || j < 2 || j >= ny - 2 || (D == 3 && (k < 2 || k >= nz - 2));
        if (!edge) continue;
        const float v = a[i + nx * (j + ny * k)];
        lo = std::fmin(lo, std::fabs(v)); pos = pos || v > 0.f; neg = neg || v < 0.f;
      }
  return (pos && neg) ? 0.f : lo;
}
}  // namespace

namespace wl {
int lattice_resolve(int id, int D, LatRef* out, float* edge_min, float* band, float* spacing) {
  std::lock_guard<std::mutex> lock(g_lat_mutex);
  for (const wl_sdf_lattice* L : g_lat)
    if (L && L->id == id) {
      if (L->D != D) { wl_set_error("lattice " + std::to_string(id) + " has " + std::to_string(L->D) + " dimensions, the body program is evaluated in " + std::to_string(D)); return WL_EINVAL; }
      out->a = L->a; out->w = L->w; out->id = id; out->gen = L->gen;
      for (int q = 0; q < 3; q++) out->n[q] = L->n[q];
      *edge_min = L->edge_min;
      if (band) *band = L->band;
      if (spacing) *spacing = L->spacing;
      return 0;
    }
  wl_set_error("lattice id " + std::to_string(id) + " is unknown or has been destroyed (wl_sdf_lattice_create / _destroy)");
  return WL_EINVAL;
}
}  // namespace wl

extern "C" {
int wl_sdf_lattice_create(wl_sdf_lattice** out, int D, const int32_t* dims, const float* host_values, void* st) {
  WL_CHECK(out, "wl_sdf_lattice_create: null result"); *out = nullptr;
  WL_CHECK(D == 2 || D == 3, "wl_sdf_lattice_create: D must be 2 or 3");
  WL_CHECK(dims && host_values, "wl_sdf_lattice_create: null dims or values");
  size_t count = 1;
  for (int q = 0; q < D; q++) {
    WL_CHECK(dims[q] >= 3, "wl_sdf_lattice_create: every extent must be at least 3 (one cell and its ghost layer)");
    WL_CHECK(dims[q] <= (1 << 20), "wl_sdf_lattice_create: extent out of range");
    count *= (size_t)dims[q];
  }
  for (size_t q = 0; q < count; q++)
    if (!std::isfinite(host_values[q])) { wl_set_error("wl_sdf_lattice_create: sample " + std::to_string(q) + " is not finite"); return WL_EINVAL; }
  std::lock_guard<std::mutex> lock(g_lat_mutex);
  int slot = 0;
  while (slot < WL_LATTICE_MAX && g_lat[slot]) slot++;
  if (slot == WL_LATTICE_MAX) { wl_set_error("wl_sdf_lattice_create: WL_LATTICE_MAX (8) lattices are alive — destroy one first"); return WL_EINVAL; }
  WL_TRY(wl_ctx_ensure());
  wl_sdf_lattice* L = new wl_sdf_lattice{};
  L->D = D;
  for (int q = 0; q < 3; q++) L->n[q] = q < D ? dims[q] : 1;
  L->edge_min = edge_min_of(D, L->n, host_values);
  hipStream_t s = wl_stream(st);
  hipError_t e = hipMalloc((void**)&L->a, count * sizeof(float));
  if (e == hipSuccess) e = hipMemcpyAsync(L->a, host_values, count * sizeof(float), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);      // the caller's host_values are free again, and every stream may read the samples, when this returns
  if (e != hipSuccess) {
    wl_set_error(std::string("wl_sdf_lattice_create: ") + hipGetErrorString(e));
    if (L->a) (void)hipFree(L->a);
    delete L;
    return (int)e;
  }
  L->id = g_lat_next_id++;
  g_lat[slot] = L;
  *out = L;
  return 0;
}
// wl_sdf_lattice_from_mesh (host_velocity NULL), wl_sdf_lattice_from_moving_mesh and wl_sdf_lattice_from_mesh_band (banded: `band` must be finite and
// positive; else band = 0 and the search is the un-banded one): `who` names the entry point in every refusal
static int lattice_from_mesh(const char* who_, wl_sdf_lattice** out, int D, const int32_t* dims, const float* host_origin, float spacing, const float* host_vertices,
                             int32_t nv, const int32_t* host_elems, int32_t ne, const float* host_velocity, bool moving, unsigned flags, void* st,
                             bool banded = false, float band = 0.f) {
  const std::string who = who_;
  if (!out) { wl_set_error(who + ": null result"); return WL_EINVAL; }
  *out = nullptr;
  if (!(D == 2 || D == 3)) { wl_set_error(who + ": D must be 2 or 3"); return WL_EINVAL; }
  if (!(dims && host_origin && host_vertices && host_elems)) { wl_set_error(who + ": null dims, origin, vertices or elements"); return WL_EINVAL; }
  if (moving && !host_velocity) { wl_set_error(who + ": null vertex velocities"); return WL_EINVAL; }
  if ((flags & ~(unsigned)WL_MESH_BRUTE) != 0) { wl_set_error(who + ": unknown flag"); return WL_EINVAL; }
  size_t count = 1;
  for (int q = 0; q < D; q++) {
    if (dims[q] < 3) { wl_set_error(who + ": every extent must be at least 3 (one cell and its ghost layer)"); return WL_EINVAL; }
    if (dims[q] > (1 << 20)) { wl_set_error(who + ": extent out of range"); return WL_EINVAL; }
    count *= (size_t)dims[q];
  }
  if (!(std::isfinite(spacing) && spacing > 0.f)) { wl_set_error(who + ": the spacing must be finite and positive"); return WL_EINVAL; }
  for (int q = 0; q < D; q++)
    if (!std::isfinite(host_origin[q])) { wl_set_error(who + ": the origin is not finite"); return WL_EINVAL; }
  if (banded && !(std::isfinite(band) && band > 0.f)) { wl_set_error(who + ": the band must be finite and positive"); return WL_EINVAL; }
  const auto t0 = std::chrono::steady_clock::now();
  wl::MeshTables tab;
  WL_TRY(wl::meshsdf_prepare(D, host_vertices, nv, host_elems, ne, &tab, who_));      // the refusals that concern the mesh; host only
  if (moving) WL_TRY(wl::meshsdf_velocities(D, host_velocity, nv, host_elems, ne, &tab, who_));
  wl::meshsdf_note_tables_ms(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  std::lock_guard<std::mutex> lock(g_lat_mutex);
  int slot = 0;
  while (slot < WL_LATTICE_MAX && g_lat[slot]) slot++;
  if (slot == WL_LATTICE_MAX) { wl_set_error(who + ": WL_LATTICE_MAX (8) lattices are alive — destroy one first"); return WL_EINVAL; }
  WL_TRY(wl_ctx_ensure());
  wl_sdf_lattice* L = new wl_sdf_lattice{};
  L->D = D;
  for (int q = 0; q < 3; q++) L->n[q] = q < D ? dims[q] : 1;
  std::vector<float> host(count);
  hipError_t e = hipMalloc((void**)&L->a, count * sizeof(float));
  if (e == hipSuccess && moving) e = hipMalloc((void**)&L->w, (size_t)D * count * sizeof(float));
  int rc = (int)e;
  if (e != hipSuccess) wl_set_error(who + ": " + hipGetErrorString(e));
  else rc = wl::meshsdf_run(tab, L->n, host_origin, spacing, band, flags, L->a, host.data(), L->w, wl_stream(st));      // synchronises the stream, like create
  if (rc != 0) {
    if (L->a) (void)hipFree(L->a);
    if (L->w) (void)hipFree(L->w);
    delete L;
    return rc;
  }
  L->edge_min = edge_min_of(D, L->n, host.data());
  L->from_mesh = true; L->spacing = spacing; L->nv = nv; L->ne = ne; L->band = band;
  L->adj = std::move(tab.adj);
  for (int q = 0; q < D; q++) L->origin[q] = host_origin[q];
  L->elems.assign(host_elems, host_elems + (size_t)ne * D);
  L->verts.assign(host_vertices, host_vertices + (size_t)nv * D);
  L->id = g_lat_next_id++;
  g_lat[slot] = L;
  *out = L;
  return 0;
}
int wl_sdf_lattice_from_mesh(wl_sdf_lattice** out, int D, const int32_t* dims, const float* host_origin, float spacing, const float* host_vertices, int32_t nv,
                             const int32_t* host_elems, int32_t ne, unsigned flags, void* st) {
  return lattice_from_mesh("wl_sdf_lattice_from_mesh", out, D, dims, host_origin, spacing, host_vertices, nv, host_elems, ne, nullptr, false, flags, st);
}
int wl_sdf_lattice_from_moving_mesh(wl_sdf_lattice** out, int D, const int32_t* dims, const float* host_origin, float spacing, const float* host_vertices, int32_t nv,
                                    const int32_t* host_elems, int32_t ne, const float* host_vertex_velocity, unsigned flags, void* st) {
  return lattice_from_mesh("wl_sdf_lattice_from_moving_mesh", out, D, dims, host_origin, spacing, host_vertices, nv, host_elems, ne, host_vertex_velocity, true, flags, st);
}
int wl_sdf_lattice_from_mesh_band(wl_sdf_lattice** out, int D, const int32_t* dims, const float* host_origin, float spacing, const float* host_vertices, int32_t nv,
                                  const int32_t* host_elems, int32_t ne, const float* host_vertex_velocity, float band, unsigned flags, void* st) {
  return lattice_from_mesh("wl_sdf_lattice_from_mesh_band", out, D, dims, host_origin, spacing, host_vertices, nv, host_elems, ne, host_vertex_velocity,
                           host_vertex_velocity != nullptr, flags, st, true, band);
}
float wl_sdf_lattice_band(const wl_sdf_lattice* L) {
  if (!L) return 0.f;
  std::lock_guard<std::mutex> lock(g_lat_mutex);
  for (const wl_sdf_lattice* q : g_lat) if (q == L) return L->band;
  return 0.f;
}
int wl_sdf_lattice_update_mesh(wl_sdf_lattice* L, const float* host_vertices, const float* host_vertex_velocity, unsigned flags, void* st) {
  const char* who = "wl_sdf_lattice_update_mesh";
  WL_CHECK(L && host_vertices, "wl_sdf_lattice_update_mesh: null lattice or vertices");
  WL_CHECK((flags & ~(unsigned)WL_MESH_BRUTE) == 0, "wl_sdf_lattice_update_mesh: unknown flag");
  std::lock_guard<std::mutex> lock(g_lat_mutex);
  int slot = 0;
  while (slot < WL_LATTICE_MAX && g_lat[slot] != L) slot++;
  WL_CHECK(slot < WL_LATTICE_MAX, "wl_sdf_lattice_update_mesh: not a live lattice");
  WL_CHECK(L->from_mesh, "wl_sdf_lattice_update_mesh: the lattice was not made from a mesh (wl_sdf_lattice_from_mesh / _from_moving_mesh)");
  WL_CHECK(L->w || !host_vertex_velocity, "wl_sdf_lattice_update_mesh: vertex velocities for a lattice made without velocity samples (wl_sdf_lattice_from_moving_mesh makes one with)");
  const int D = L->D;
  const auto t0 = std::chrono::steady_clock::now();
  wl::MeshTables tab;
  // every mesh refusal that the moved vertices can meet (the connectivity passed at creation and is kept with its adjacency); host only
  WL_TRY(wl::meshsdf_prepare_geometry(D, host_vertices, L->nv, L->elems.data(), L->ne, L->adj, &tab, who));
  if (L->w) {
    const std::vector<float> zeros(host_vertex_velocity ? 0 : (size_t)L->nv * D, 0.f);
    WL_TRY(wl::meshsdf_velocities(D, host_vertex_velocity ? host_vertex_velocity : zeros.data(), L->nv, L->elems.data(), L->ne, &tab, who));
  }
  wl::meshsdf_note_tables_ms(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  // from here on nothing is refused: the samples are overwritten in place, on the caller's stream — behind whatever that stream still reads them with
  const size_t count = (size_t)L->n[0] * (size_t)L->n[1] * (size_t)L->n[2];
  std::vector<float> host(count);
  WL_TRY(wl::meshsdf_run(tab, L->n, L->origin, L->spacing, L->band, flags, L->a, host.data(), L->w, wl_stream(st)));
  L->edge_min = edge_min_of(D, L->n, host.data());
  L->verts.assign(host_vertices, host_vertices + (size_t)L->nv * D);
  L->gen++;
  return 0;
}
int wl_sdf_lattice_set_velocity(wl_sdf_lattice* L, const float* host_w, void* st) {
  WL_CHECK(L && host_w, "wl_sdf_lattice_set_velocity: null lattice or samples");
  std::lock_guard<std::mutex> lock(g_lat_mutex);
  int slot = 0;
  while (slot < WL_LATTICE_MAX && g_lat[slot] != L) slot++;
  WL_CHECK(slot < WL_LATTICE_MAX, "wl_sdf_lattice_set_velocity: not a live lattice");
  const size_t total = (size_t)L->D * (size_t)L->n[0] * (size_t)L->n[1] * (size_t)L->n[2];
  for (size_t q = 0; q < total; q++)
    if (!std::isfinite(host_w[q])) { wl_set_error("wl_sdf_lattice_set_velocity: velocity sample " + std::to_string(q) + " is not finite"); return WL_EINVAL; }
  hipStream_t s = wl_stream(st);
  float* w = L->w;
  if (!w) WL_HIP(hipMalloc((void**)&w, total * sizeof(float)));
  hipError_t e = hipMemcpyAsync(w, host_w, total * sizeof(float), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    if (!L->w) (void)hipFree(w);
    wl_set_error(std::string("wl_sdf_lattice_set_velocity: ") + hipGetErrorString(e));
    return (int)e;
  }
  L->w = w;                                 // attached only once it is filled: a program resolved from here on reads it
  L->gen++;
  return 0;
}
int wl_sdf_lattice_read_velocity(const wl_sdf_lattice* L, float* host_w, void* st) {
  WL_CHECK(L && host_w, "wl_sdf_lattice_read_velocity: null lattice or samples");
  std::lock_guard<std::mutex> lock(g_lat_mutex);
  int slot = 0;
  while (slot < WL_LATTICE_MAX && g_lat[slot] != L) slot++;
  WL_CHECK(slot < WL_LATTICE_MAX, "wl_sdf_lattice_read_velocity: not a live lattice");
  WL_CHECK(L->w, "wl_sdf_lattice_read_velocity: the lattice has no velocity samples");
  const size_t total = (size_t)L->D * (size_t)L->n[0] * (size_t)L->n[1] * (size_t)L->n[2];
  hipStream_t s = wl_stream(st);
  WL_HIP(hipMemcpyAsync(host_w, L->w, total * sizeof(float), hipMemcpyDeviceToHost, s));
  WL_HIP(hipStreamSynchronize(s));
  return 0;
}
int wl_sdf_lattice_has_velocity(const wl_sdf_lattice* L) {
  if (!L) return 0;
  std::lock_guard<std::mutex> lock(g_lat_mutex);
  for (const wl_sdf_lattice* q : g_lat) if (q == L) return L->w ? 1 : 0;
  return 0;
}
int wl_sdf_lattice_read(const wl_sdf_lattice* L, float* host_values, void* st) {
  WL_CHECK(L && host_values, "wl_sdf_lattice_read: null lattice or values");
  std::lock_guard<std::mutex> lock(g_lat_mutex);
  int slot = 0;
  while (slot < WL_LATTICE_MAX && g_lat[slot] != L) slot++;
  WL_CHECK(slot < WL_LATTICE_MAX, "wl_sdf_lattice_read: not a live lattice");
  const size_t count = (size_t)L->n[0] * (size_t)L->n[1] * (size_t)L->n[2];
  hipStream_t s = wl_stream(st);
  WL_HIP(hipMemcpyAsync(host_values, L->a, count * sizeof(float), hipMemcpyDeviceToHost, s));
  WL_HIP(hipStreamSynchronize(s));
  return 0;
}
float wl_sdf_lattice_edge_min(const wl_sdf_lattice* L) {
  if (!L) return 0.f;
  std::lock_guard<std::mutex> lock(g_lat_mutex);
  for (const wl_sdf_lattice* q : g_lat) if (q == L) return L->edge_min;
  return 0.f;
}
int wl_sdf_lattice_destroy(wl_sdf_lattice* L) {
  if (!L) return 0;
  std::lock_guard<std::mutex> lock(g_lat_mutex);
  int slot = 0;
  while (slot < WL_LATTICE_MAX && g_lat[slot] != L) slot++;
  WL_CHECK(slot < WL_LATTICE_MAX, "wl_sdf_lattice_destroy: not a live lattice");
  g_lat[slot] = nullptr;                    // from here on no program resolves it: nothing new can be launched on its samples
  const hipError_t e = hipDeviceSynchronize();      // … and what was launched has finished before the memory goes
  (void)hipFree(L->a);
  if (L->w) (void)hipFree(L->w);
  delete L;
  if (e != hipSuccess) { wl_set_error(std::string("wl_sdf_lattice_destroy: ") + hipGetErrorString(e)); return (int)e; }
  return 0;
}
int wl_sdf_lattice_id(const wl_sdf_lattice* L) {
  if (!L) return 0;
  std::lock_guard<std::mutex> lock(g_lat_mutex);
  for (const wl_sdf_lattice* q : g_lat) if (q == L) return L->id;
  return 0;
}
}  // extern "C"
