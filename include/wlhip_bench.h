/* wlhip_bench.h — MEASUREMENT interface of libwlhip.so (bench.py, tools/): HIP-event pairs on the launch stream, launch and
 * path counters.  NOT part of the drop-in boundary: nothing in the reference binds these (the reference-facing surface is wlhip.h);
 * they exist because the harness contract asks for kernel durations measured live inside the timed region, on the stream the
 * kernels are launched on. */
#ifndef WLHIP_BENCH_H
#define WLHIP_BENCH_H
#include "wlhip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- measurement hooks (bench.py): HIP-event pairs recorded on the launch stream around named launches ----
 * slots: 0 fine-level GS colour sweep (one launch), 1 fine-level smooth! (GaussSeidelRB! as a whole),
 *        2 fine-level Jacobi!, 3 conv_diff!, 4 fine-level residual!+norms, 5 BDIM!, 6 fine-level prolongate+increment,
 *        7 coarse levels (everything below level 1 of a V-cycle), 8 mom_step! as a whole,
 *        9 / 10 fine-level kernels A / B of the temporally blocked smoother (wl_fused.hip)                        */
enum { WL_PROF_GS_SWEEP = 0, WL_PROF_SMOOTH = 1, WL_PROF_JACOBI = 2, WL_PROF_CONVDIFF = 3, WL_PROF_RESIDUAL = 4,
       WL_PROF_BDIM = 5, WL_PROF_PROLONG = 6, WL_PROF_COARSE = 7, WL_PROF_STEP = 8, WL_PROF_GS_A = 9, WL_PROF_GS_B = 10, WL_PROF_NSLOTS = 11 };
int wl_prof_enable(int on);                                     /* 0 off, 1 all slots, 2 only slots 9 and 10 (each event pair costs a few µs of
                                                                    stream time); also resets all slots */
int wl_prof_read(int slot, int* host_count, double* host_total_ms);   /* synchronises the device */

/* kernel launches issued by the library in this process so far (every hipLaunchKernelGGL of libwlhip; copies and memsets are not counted) */
long wl_launch_count(void);
/* With WL_PLACEMENT_TRIALS=2…8 (default 1 = off) wl_sim_create on a large 3-D grid whose arrays the handle owns tries that many placements of its
 * allocations and keeps the fastest (wl_sim.hip "Placement trials" — measured: not a reliable remedy): the candidates' scores, ms of a timed mom_project! pair */
int wl_placement_scores(double* out, int cap);
/* per-handle path counters: "resjac" = solves whose fused projection head (div + x·dt + residual! + first Jacobi!) stood,
 * "resjac_redo" = solves where residual!'s mean shift was due after all and the head was redone on the two-kernel path,
 * "resjac_backoff" = 1 once three consecutive redos switched the fused head off for this handle (re-armed by wl_sim_update),
 * "bcdefer" = BC!(u,U) applications after conv_diff!+BDIM! that were left to the following projection (two per step when the option is live),
 * "tailspec" = projection tails that ran from inside the solver loop, ahead of the convergence read,
 * "tailspec_armed" = solves the gated tail was queued for (the difference to "tailspec": withheld — the cap was hit, or the fused head's mean shift was due),
 * "pdefer" = projection tails that did not store p = x/Δt (the next fused head divided on load): 2k − 1 for a k-step wl_sim_mom_steps call where the option is live,
 * "rskip" = finest-level launches of smoother kernel B that did not store the residual (option "rskip": the iteration at which the slot's previous solve stopped),
 * "rskip_redo" = launches of its r-only form that produced such a residual after all (the loop went on, or wl_mg_level_field / wl_mg_smooth / wl_mg_vcycle asked),
 * "tailwide" = projection tails that ran in the four-cells-per-thread form (two per step where the option is live and the shape allows it),
 * "tailfuse" = projections whose velocity update (u −= L∇x, BC!) was evaluated by the corrector's conv_diff! loader instead of a tail launch,
 * "tailfuse_min" = no count: the size gate of that path in force on this handle (interior cells; option "tailfuse_min"),
 * "xdefer" = what the finest level's last smooth! decided: 1 the V-cycle's x += ω·x_c↓ was applied by smoother kernel B, 0 by kernel A, −1 none yet
 * (decides which bytes bench.py books to kernels A and B),
 * "abwide" = finest-level smooth! calls in which kernel A handed r′ and ϵ_mid to kernel B through the level's exchange buffer (one float4 per cell pair,
 * csrc/wl_abwide.hpp) instead of the two dense arrays,
 * flows with a body — which body-aware path ran: "hybrid" = predict/correct calls that took the body-aware conv_diff!+BDIM! (two per step where live),
 * "body_tile" = tiled far-range launches of that path (PROCESS-wide, like the option: read it as a difference), "mask_valid" = 1 while the masks of the last
 * measure!/update! are in force (0 after wl_sim_field handed out V, mu0 or mu1), "part" / "part_za" / "part_zb" = the finest level runs the z-split smoother /
 * the planes whose coefficients are off the constant pattern;
 * the mask census of the last refresh, per (plane, workgroup of 256 in-plane cells): "mask_near", "mask_needf_only" (f kept for a neighbour, not near),
 * "mask_m0var_only" (only μ₀ off the wall pattern), "mask_clean_in_box" (inside the near bounding box, not near), "dirty_z0" / "dirty_z1" (first / last plane
 * with any mark; z1 < z0: none), "near_b0" / "near_b1" / "near_k0" / "near_k1" (the bounding box; b1 < b0: empty);
 * "launches" = kernel launches issued inside this handle's mom_step! calls so far (wl_launch_count is process-wide),
 * "probe_records" / "probe_dropped" = probe records held since the last wl_sim_read_probes / records a full buffer refused since wl_sim_set_probes;
 * "force_records" / "force_dropped" = the same for the force recorder (wl_sim_set_force_record); "force_tiles" = active tiles of the band list in use
 * (the recorder's, or without a recorder that of the last wl_sim_forces_bodyset);
 * "mean_updates" = updates of the mean-flow observer since wl_sim_set_meanflow (the observer's and wl_sim_meanflow_update's), "mean_every" = its period (0: off) */
int wl_sim_counter(wl_sim* s, const char* name, long* out);
/* the last wl_sdf_lattice_from_mesh of this process: exact (sample, element) closest-point tests made — the per-brick counts the kernel wrote, summed on the
 * host — and samples × elements; equal under WL_MESH_BRUTE */
int wl_meshsdf_last_pairs(uint64_t* tested, uint64_t* total);
/* the last mesh search of this process: bricks whose samples were searched (sweep 2) and bricks skipped because they lie wholly beyond the lattice's band
 * (wlhip.h, band-limited baking) — searched + skipped = the brick count; skipped = 0 without a band and under WL_MESH_BRUTE.  With a band
 * wl_meshsdf_last_pairs' `tested` counts candidates × live samples per searched brick, and per skipped brick the elements tested for its one sign sample */
int wl_meshsdf_last_bricks(uint64_t* searched, uint64_t* skipped);
/* wl_meshsdf_time(1): every later mesh bake of this process (wl_sdf_lattice_from_mesh, _from_moving_mesh, _update_mesh) fences its phases with stream
 * synchronisations and times them on the host; wl_meshsdf_last_times then gives the last bake's ms4 = {host tables, uploads, kernel, read-back}.  Off (the
 * default) nothing is fenced; ms4[0], which needs no fence, is recorded either way.  For tools/meshvel_bench.py. */
int wl_meshsdf_time(int on);
int wl_meshsdf_last_times(double* ms4);
/* ---- test hook (tests/deadstore.py): the scratch no entry point hands out.  wl_sim_scratch_fill first settles whatever is pending, as wl_sim_field does (and the
 * finest level's residual where option "rskip" left it unstored), then writes the 32-bit word `bits` on `stream` into everything the handle and its wl_mg own
 * that is DEAD between public calls — written by the library before it is read again, whatever it holds:
 *   1. the pressure array of the pair {p, spare} that does not hold the pressure: every cell, ghost cells included — cells(level 0) words
 *      (what the handle knows of the ghost shells of the pair is forgotten: the next fused head checks them again);
 *   2. every level's ϵ_mid and r′ of the blocked smoother (wl_mg::Level::em, rs): interior cells — 2·interior(level) words per level;
 *   3. every exchange buffer W (csrc/wl_abwide.hpp; 3-D levels that have one): on the interior planes the interior rows, whole 512-byte segments, padding slots
 *      included — (nz − 2)·(ny − 2)·⌈(nx − 1)/60⌉·128 words per such level;
 *   4. the per-block partials of the reduction workspace: 65536 × (two doubles + one float) = 327680 words;
 *   5. the partial sums of the force bands that exist (the recorder's, the immediate read-out's): 24 words per tile of their capacity — none before
 *      wl_sim_set_force_record / wl_sim_forces_bodyset.
 * It leaves alone what must keep a value: the ghost cells of em and rs and W's ghost rows and planes (zero since allocation, read by kernel B), the 16 result
 * slots of the reduction workspace, the body masks, the band lists, probe, force and tracer records and positions, the mean-flow sums.  Caller-visible arrays
 * (f, σ, us, the levels' r, ϵ, x, z) are the caller's to overwrite through wl_sim_field / wl_mg_level_field.
 * Returns the number of 4-byte words written, −1 on error (z-slab handles: single domain only).  wl_sim_scratch_keep is the same call — the same settling, the
 * same launches, the same return value — with every word left as it is: for the twin that a filled handle is compared with.  wl_sim_scratch_fill_regions
 * writes only the regions whose bit is set (bit i − 1: region i of the list) and counts those: for finding which region a difference comes from.  None of them
 * is on the step path. */
int wl_sim_scratch_fill(wl_sim* s, uint32_t bits, void* stream);
int wl_sim_scratch_fill_regions(wl_sim* s, uint32_t bits, uint32_t regions, void* stream);
int wl_sim_scratch_keep(wl_sim* s, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WLHIP_BENCH_H */
