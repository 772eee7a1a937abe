// Observers of a completed time step (wl_observe.hip, host code): probe records, force records, tracer particles and the mean flow.  All of them read the
// step's final u — the probes, forces and the mean flow p as well, the tracers the array in the u⁰ role, which no kernel of the step writes: it still holds the
// velocity the step started from (src/Flow.jl:157) — after the second projection and before CFL; none writes anything the step reads, so a handle with
// observers computes the bits of one without.  Kernels: wl_interp.hip, wl_forces.hip, wl_meanflow.hip.
#pragma once
#include <vector>

#include "wl_common.hpp"
#include "wl_body.hpp"
#include "wl_forces.hpp"

namespace wl {
// what the observers may see of the handle
struct StepView {
  const GridX& G; int D;
  const float *u, *u0, *p;
  float nu;
  const std::vector<float>& dt;      // the Δt history: dt.back() is the Δt the step ran with until cfl appends the next one
  unsigned perdir_mask;
};
// One record per completed step in a device buffer of fixed capacity; a full buffer refuses (and counts) further records until it is read.
struct RecordBuffer {
  void* rec = nullptr;               // device: cap records of rec_bytes
  size_t rec_bytes = 0;
  int cap = 0, n = 0;                // records the buffer takes / holds
  long first = 0, dropped = 0;       // index into Δt of the first held record's step; records a full buffer refused
  hipStream_t stream = nullptr;      // the stream the last record went to (read waits for it)
  int alloc(size_t record_bytes, int capacity);
  void* next_slot(long step, hipStream_t s);      // where the record of `step` goes, or null (counted) when the buffer is full
  // host == null is a query: nothing is copied, the buffer keeps its records; otherwise the held records are copied on the recording stream and given up
  int read(void* host, int cap_records, int* n_records, int* first_step, const char* who);
  void release();
};
struct Observers {
  // probes (wl_sim_set_probes): one record of m×(D+1) floats — u then p at every point — per step, one launch
  float* probe_x = nullptr; int probe_m = 0;      // device: m×D points
  RecordBuffer probes;
  // the force recorder (wl_sim_set_force_record): 12 doubles per step — pressure force, viscous force, pressure and viscous moment about force_x0 — of the
  // recorder's body, from the body's band only.  Two launches per step (one for an empty band), no host round trip.  fimm: the band of the immediate
  // read-out wl_sim_forces_bodyset, kept so that a repeated call finds its list built.
  ForceBand fband, fimm;
  bool force_on = false;
  float force_x0[3] = {0.f, 0.f, 0.f};
  RecordBuffer forces;
  // tracers (wl_sim_set_tracers): positions and positions before the last step (n×D each), one launch per step
  float *tr_x = nullptr, *tr_x0 = nullptr; size_t tr_n = 0;
  // the mean flow (wl_sim_set_meanflow): MeanFlow's P, U and — mode 2 — UU = ⟨u⊗u⟩ (src/Metrics.jl:205-262), updated by ONE launch after every mean_every-th
  // completed step, every cell of the arrays.  ε and the time vector are update!'s Float32 statements on the host (:237-239,247); time(flow) is the in-order
  // sum of the Δt history, this step's Δt included.  UU is packed (i ≤ j: wl_meanflow.hip).  Steps on which no update is due launch nothing.
  float* mean_own = nullptr;                      // device: P (cs) | U (D·cs) | packed UU (D(D+1)/2·cs, mode 2), zero-initialised
  size_t mean_cs = 0; int mean_D = 0;             // the grid the averages were allocated for
  int mean_mode = 0, mean_every = 1;              // 0 off, 1 P and U, 2 with UU; an update every mean_every-th completed step
  long mean_steps = 0, n_mean_updates = 0;        // completed steps since set/reset; updates since set
  std::vector<float> mean_t;                      // meanflow.t
  hipStream_t mean_stream = nullptr;              // the stream the last update or reset went to (set_meanflow waits for it before it frees)

  ~Observers() { free_probes(); free_forces(); fimm.release(); free_tracers(); free_mean(); }

  // ---- what the step asks
  // the probe or force record or the mean-flow update of the step now running reads p: its last projection tail has to store it ("pdefer")
  bool reads_p_after_this_step() const { return probe_m || force_on || mean_due(); }
  // a step with a force recorder will launch the recorder's stored program: WL_EINVAL now, before anything runs, if a lattice it names has been destroyed
  int before_step(int D) { return force_on ? fband.recheck(D) : 0; }
  int after_step(const StepView& v, hipStream_t s);      // probes, forces, tracers, mean — in this launch order; p is current (the caller sees to that)
  // measure!(sim) replaced the body: pressure_force(sim) always means sim.body as it is now, so the recorder follows it
  int body_changed(const GridX& G, const SetArg& P, hipStream_t s) { return force_on ? fband.build(G, P, s) : 0; }

  // ---- behind the C entry points (arguments checked there)
  int set_probes(int D, const float* host_x, int m, int capacity);
  int set_force_record(const GridX& G, int D, const SetArg* P, const float* host_x0, int capacity);      // P == null: off
  int forces_now(const StepView& v, const SetArg& P, const float* host_x0, double out[12], hipStream_t s);
  int set_tracers(int D, const float* host_x, size_t n);
  int set_meanflow(const StepView& v, int mode, int every, float t_init, hipStream_t s);

  float* mean_P() const { return mean_own; }
  float* mean_U() const { return mean_own ? mean_own + mean_cs : nullptr; }
  float* mean_UU() const { return mean_own && mean_mode == 2 ? mean_own + mean_cs * (size_t)(1 + mean_D) : nullptr; }
  size_t mean_floats(int mode) const;
  bool mean_due() const { return mean_mode && (mean_steps + 1) % mean_every == 0; }      // the step now running (or the next one) ends with an update
  static float time_f(const std::vector<float>& dt, size_t n_dt) { float t = 0.f; for (size_t k = 0; k < n_dt; k++) t += dt[k]; return t; }      // Float32, in order: sum(Δt[1:n])
  int mean_reset(float t_init, hipStream_t s);                            // reset!(meanflow; t_init) :229-234
  int mean_update(const StepView& v, float t_flow, hipStream_t s);        // update!(meanflow, flow) :236-248 with time(flow) = t_flow; p is current

  void free_probes(); void free_forces(); void free_tracers(); void free_mean();
};
}  // namespace wl
