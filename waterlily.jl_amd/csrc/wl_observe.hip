// Observers of a completed time step: life cycle and per-step launches (host code only; see wl_observe.hpp).
#include "wl_observe.hpp"
#include "wl_meanflow.hpp"

namespace wl {
int RecordBuffer::alloc(size_t record_bytes, int capacity) {
  WL_HIP(hipMalloc(&rec, (size_t)capacity * record_bytes));
  rec_bytes = record_bytes; cap = capacity;
  return 0;
}
void* RecordBuffer::next_slot(long step, hipStream_t s) {
  if (n == cap) { dropped++; return nullptr; }
  if (n == 0) first = step;
  stream = s;
  return (char*)rec + (size_t)n++ * rec_bytes;
}
int RecordBuffer::read(void* host, int cap_records, int* n_records, int* first_step, const char* who) {
  *n_records = n; *first_step = (int)first;
  if (!host) return 0;
  if (cap_records < n) { wl_set_error(std::string(who) + ": host_out takes fewer records than the buffer holds (nothing was read)"); return WL_EINVAL; }
  if (n) {
    WL_HIP(hipMemcpyAsync(host, rec, (size_t)n * rec_bytes, hipMemcpyDeviceToHost, stream));
    WL_HIP(hipStreamSynchronize(stream));
  }
  n = 0;
  return 0;
}
void RecordBuffer::release() { if (rec) (void)hipFree(rec); rec = nullptr; cap = n = 0; }

void Observers::free_probes() { if (probe_x) (void)hipFree(probe_x); probe_x = nullptr; probe_m = 0; probes.release(); }
void Observers::free_forces() { forces.release(); force_on = false; fband.release(); }
void Observers::free_tracers() { if (tr_x) (void)hipFree(tr_x); if (tr_x0) (void)hipFree(tr_x0); tr_x = tr_x0 = nullptr; tr_n = 0; }
void Observers::free_mean() { if (mean_own) (void)hipFree(mean_own); mean_own = nullptr; mean_mode = 0; mean_every = 1; mean_steps = 0; mean_t.clear(); }

int Observers::after_step(const StepView& v, hipStream_t s) {
  const long step = (long)v.dt.size() - 1;
  if (probe_m)
    if (float* rec = (float*)probes.next_slot(step, s)) WL_TRY(wl::interp_points(v.u, v.p, v.G, probe_x, (size_t)probe_m, rec, v.D + 1, rec + v.D, v.D + 1, s));
  if (force_on)
    if (double* rec = (double*)forces.next_slot(step, s)) WL_TRY(fband.run(v.G, v.p, v.u, v.nu, force_x0, rec, s));
  if (tr_n) WL_TRY(wl::advect(tr_x, tr_x0, v.u0, v.u, v.G, tr_n, v.dt.back(), v.perdir_mask, s));
  if (mean_mode) {
    const bool due = mean_due();
    mean_steps++;
    if (due) WL_TRY(mean_update(v, time_f(v.dt, v.dt.size()), s));
  }
  return 0;
}

int Observers::set_probes(int D, const float* host_x, int m, int capacity) {
  WL_HIP(hipDeviceSynchronize());      // records may still be in flight on the stream of the last step
  free_probes(); probes.dropped = 0;
  if (m == 0) return 0;
  const size_t nx = (size_t)m * D;
  WL_HIP(hipMalloc((void**)&probe_x, nx * sizeof(float)));
  if (probes.alloc((size_t)m * (D + 1) * sizeof(float), capacity) != 0) { free_probes(); wl_set_error("wl_sim_set_probes: hipMalloc failed for the record buffer"); return (int)hipErrorOutOfMemory; }
  WL_HIP(hipMemcpy(probe_x, host_x, nx * sizeof(float), hipMemcpyHostToDevice));
  probe_m = m;
  return 0;
}
int Observers::set_force_record(const GridX& G, int D, const SetArg* P, const float* host_x0, int capacity) {
  WL_HIP(hipDeviceSynchronize());      // records may still be in flight on the stream of the last step
  free_forces(); forces.dropped = 0;
  if (!P) return 0;
  WL_TRY(forces.alloc(12 * sizeof(double), capacity));
  for (int c = 0; c < 3; c++) force_x0[c] = (host_x0 && c < D) ? host_x0[c] : 0.f;
  const int rc = fband.build(G, *P, 0);
  if (rc != 0) { free_forces(); return rc; }
  force_on = true;
  return 0;
}
int Observers::forces_now(const StepView& v, const SetArg& P, const float* host_x0, double out[12], hipStream_t s) {
  WL_TRY(fimm.build(v.G, P, s));      // (a repeated call with the same body finds the list built: no launch, no read-back)
  WL_TRY(fimm.run(v.G, v.p, v.u, v.nu, host_x0, fimm.out, s));
  WL_HIP(hipMemcpyAsync(out, fimm.out, 12 * sizeof(double), hipMemcpyDeviceToHost, s));
  WL_HIP(hipStreamSynchronize(s));
  return 0;
}
int Observers::set_tracers(int D, const float* host_x, size_t n) {
  WL_HIP(hipDeviceSynchronize());      // the last step's launch may still be moving the old swarm
  free_tracers();
  if (n == 0) return 0;
  const size_t nb = n * (size_t)D * sizeof(float);
  WL_HIP(hipMalloc((void**)&tr_x, nb));
  if (hipMalloc((void**)&tr_x0, nb) != hipSuccess) { free_tracers(); wl_set_error("wl_sim_set_tracers: hipMalloc failed"); return (int)hipErrorOutOfMemory; }
  WL_HIP(hipMemcpy(tr_x, host_x, nb, hipMemcpyHostToDevice));
  WL_HIP(hipMemcpy(tr_x0, host_x, nb, hipMemcpyHostToDevice));      // position⁰ = position until the first step
  tr_n = n;
  return 0;
}

size_t Observers::mean_floats(int mode) const { return mean_cs * (size_t)(1 + mean_D + (mode == 2 ? wl::meanflow_packed_planes(mean_D) : 0)); }
int Observers::set_meanflow(const StepView& v, int mode, int every, float t_init, hipStream_t s) {
  if (mean_own) WL_HIP(hipStreamSynchronize(mean_stream));      // an update may still be in flight on the stream of the last step
  free_mean(); n_mean_updates = 0;
  if (mode == 0) return 0;
  mean_cs = (size_t)v.G.cs; mean_D = v.D;
  if (hipMalloc((void**)&mean_own, mean_floats(mode) * sizeof(float)) != hipSuccess) { mean_own = nullptr; free_mean(); wl_set_error("wl_sim_set_meanflow: hipMalloc failed for the averages"); return (int)hipErrorOutOfMemory; }
  mean_mode = mode; mean_every = every;
  const int rc = mean_reset(t_init, s);
  if (rc != 0) free_mean();
  return rc;
}
int Observers::mean_reset(float t_init, hipStream_t s) {
  WL_HIP(hipMemsetAsync(mean_own, 0, mean_floats(mean_mode) * sizeof(float), s));
  mean_t.assign(1, t_init); mean_steps = 0; mean_stream = s;
  return 0;
}
int Observers::mean_update(const StepView& v, float t_flow, hipStream_t s) {
  const float dtm = t_flow - mean_t.back();
  float e = dtm / (dtm + (mean_t.back() - mean_t.front()) + 1.1920929e-7f);
  if (mean_t.size() == 1) e = 1.f;                   // the first update takes the instantaneous field
  WL_TRY(wl::meanflow_observe(mean_P(), mean_U(), mean_UU(), v.p, v.u, v.G, e, s));
  mean_t.push_back(mean_t.back() + dtm);
  n_mean_updates++; mean_stream = s;
  return 0;
}
}  // namespace wl
