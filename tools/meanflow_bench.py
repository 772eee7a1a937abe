#!/usr/bin/env python3
"""Cost of time-averaging on a handle (wl_meanflow.hip) on a developed wall-bounded TGV at 256³ and 512³, one process, HIP events, median of 30:
(a) the leaf wl_meanflow_update with UU on arrays of the handle's size, (b) wl_sim_meanflow_update alone, (c) wl_sim_mom_step without the observer and
with it at every = 1 and every = 10, alternated on ONE handle, (d) per step: mom_steps_(8) with the observer against eight single steps each followed by
MeanFlow.update_ through the leaf, (e) a device copy moving (b)'s bytes, as the ceiling.
Every GPU step runs under a watchdog of its own (the process exits if one does not finish in time: nothing more is started).
usage (GPU box): python tools/meanflow_bench.py [out.json] [N ...]      default: profiles/meanflow_bench_256_512.json 256 512"""
import faulthandler
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import waterlily_jl_amd as w
from waterlily_jl_amd._lib import check, lib

OUT = sys.argv[1] if len(sys.argv) > 1 else "profiles/meanflow_bench_256_512.json"
SIZES = [int(v) for v in sys.argv[2:]] or [256, 512]
WARM, REPS, NSTEPS, DEVELOP = 3, 30, 8, 24
L = lib()


class step:
    """one GPU step under its own time limit"""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *a):
        torch.cuda.synchronize()
        faulthandler.cancel_dump_traceback_later()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def stats(ts, **extra):
    return dict({"ms_median": statistics.median(ts), "ms_min": min(ts), "reps": len(ts)}, **extra)


class HandleFlow:
    """what MeanFlow reads of a flow, over the handle's own arrays (their current role holders)"""

    def __init__(self, sim):
        self.sim, self.D = sim, sim.D

    p = property(lambda self: self.sim._view("p"))
    u = property(lambda self: self.sim._view("u"))

    def time(self):
        return self.sim.time()


def bench(N):
    with step(300):
        sim = w.FusedSimulation((N, N, N), (0.0, 0.0, 0.0), N, U=1, nu=N / 1600.0, ic="tgv")
        sim.mom_steps_(DEVELOP)
    cs = int((N + 2) ** 3)
    res = {"N": N, "cells_with_ghosts": cs, "developed_steps": DEVELOP}
    flow = HandleFlow(sim)
    # (a) the leaf, with UU in full, on arrays of the handle's size
    with step(120):
        mf = w.MeanFlow(flow, uu_stats=True)
        for _ in range(WARM):
            mf.update_(flow)
        a = [timed(lambda: mf.update_(flow)) for _ in range(REPS)]
    res["a_leaf_update_uu"] = stats(a, bytes_per_cell=120, GBps=120 * cs / statistics.median(a) / 1e6)
    del mf
    torch.cuda.empty_cache()
    # (b) the handle's own update
    with step(120):
        sim.set_meanflow(uu_stats=True, every=1 << 30)
        for _ in range(WARM):
            sim.update_meanflow()
        n0 = L.wl_launch_count()
        b = [timed(sim.update_meanflow) for _ in range(REPS)]
        lb = (L.wl_launch_count() - n0) / REPS
        sim.set_meanflow(None)
    res["b_handle_update_uu"] = stats(b, bytes_per_cell=96, launches=lb, GBps=96 * cs / statistics.median(b) / 1e6)
    # (e) the ceiling: a device copy that moves (b)'s 96 B/cell (48 read + 48 written)
    with step(120):
        src = torch.empty(12 * cs, dtype=torch.float32, device="cuda").normal_()
        dst = torch.empty_like(src)
        for _ in range(WARM):
            dst.copy_(src)
        e = [timed(lambda: dst.copy_(src)) for _ in range(REPS)]
        del src, dst
        torch.cuda.empty_cache()
    res["e_device_copy_96B_per_cell"] = stats(e, GBps=96 * cs / statistics.median(e) / 1e6)
    # (c) single steps without the observer, with every = 1, and ten with every = 10, alternated on one handle (every step is a new flow state: all arms see the same drift)
    off, on1, on10 = [], [], []
    for rep in range(REPS + 2):
        with step(120):
            sim.set_meanflow(None)
            t_off = timed(sim.mom_step_)
        with step(120):
            sim.set_meanflow(uu_stats=True, every=1)
            t_on1 = timed(sim.mom_step_)
        with step(300):
            sim.set_meanflow(uu_stats=True, every=10)
            t_on10 = sum(timed(sim.mom_step_) for _ in range(10)) / 10
            assert sim.counter("mean_updates") == 1
        if rep >= 2:
            off.append(t_off); on1.append(t_on1); on10.append(t_on10)
    sim.set_meanflow(None)
    res["c_step_without_observer"] = stats(off)
    res["c_step_every_1"] = stats(on1, ms_median_of_differences=statistics.median([q - p for p, q in zip(off, on1)]))
    res["c_step_every_10_mean_of_ten"] = stats(on10, ms_median_of_differences=statistics.median([q - p for p, q in zip(off, on10)]))
    # (d) NSTEPS steps with an update after each: one mom_steps_ call with the observer / single steps each followed by the leaf's update_
    obs, loop = [], []
    with step(120):
        mf = w.MeanFlow(flow, uu_stats=True)

    def hand_loop():
        for _ in range(NSTEPS):
            sim.mom_step_()
            mf.update_(flow)

    for rep in range(REPS // 3 + 1):
        with step(300):
            sim.set_meanflow(uu_stats=True, every=1)
            t_obs = timed(lambda: sim.mom_steps_(NSTEPS))
            assert sim.counter("mean_updates") == NSTEPS
            sim.set_meanflow(None)
        with step(300):
            t_loop = timed(hand_loop)
        if rep >= 1:
            obs.append(t_obs / NSTEPS); loop.append(t_loop / NSTEPS)
    res["d_observed_mom_steps_per_step"] = stats(obs, steps_per_call=NSTEPS)
    res["d_single_steps_plus_leaf_per_step"] = stats(loop, steps_per_call=NSTEPS)
    res["conditions"] = {
        "b_ms": res["b_handle_update_uu"]["ms_median"], "a_ms": res["a_leaf_update_uu"]["ms_median"],
        "b_not_slower_than_a": res["b_handle_update_uu"]["ms_median"] <= res["a_leaf_update_uu"]["ms_median"],
        "d_observed_ms_per_step": res["d_observed_mom_steps_per_step"]["ms_median"], "d_loop_ms_per_step": res["d_single_steps_plus_leaf_per_step"]["ms_median"],
        "d_observed_faster": res["d_observed_mom_steps_per_step"]["ms_median"] < res["d_single_steps_plus_leaf_per_step"]["ms_median"]}
    del mf, sim
    torch.cuda.empty_cache()
    return res


def main():
    check(L.wl_init(0))
    out = {"what": __doc__.split("\n")[0], "device": torch.cuda.get_device_name(0), "results": []}
    for N in SIZES:
        out["results"].append(bench(N))
        os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
        with open(OUT, "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
