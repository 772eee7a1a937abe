#!/usr/bin/env python3
"""Cost of a force history (wl_forces.hip) for the sphere of radius 32 at 256³, one process, HIP events, median of 30:
(a) the four existing immediate read-outs after a step, (b) forces(), (c) the step with and without the recorder, alternated on ONE handle,
(d) mom_steps_(n) with the recorder against n single steps each followed by the four read-outs.
Every GPU step runs under a watchdog of its own (the process exits if one does not finish in time: nothing more is started).
usage (GPU box): python tools/forces_bench.py [out.json] [N]      default: bench_out/forces_bench.json 256"""
import faulthandler
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import waterlily_jl_amd as w
from waterlily_jl_amd._lib import check, lib

OUT = sys.argv[1] if len(sys.argv) > 1 else "bench_out/forces_bench.json"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 256
WARM, REPS, NSTEPS = 3, 30, 8
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


def main():
    check(L.wl_init(0))
    R = N / 8
    c = (N / 2 + 0.3, N / 2 - 0.4, N / 2 + 0.2)
    body = w.Body(("sphere", c, R))
    x0 = c
    with step(300):
        sim = w.FusedSimulation((N, N, N), (1.0, 0.0, 0.0), 2 * R, U=1, nu=2 * R / 250, has_body=True)
        sim.set_body(body)
        sim.mom_steps_(5)

    def four():
        sim.pressure_force_body(body); sim.viscous_force_body(body)
        sim.pressure_moment_body(x0, body); sim.viscous_moment_body(x0, body)

    res = {"N": N, "radius": R, "tile": [64, 4, 4]}
    with step(120):
        n0 = L.wl_launch_count()
        for _ in range(WARM):
            four()
        l4 = (L.wl_launch_count() - n0) / WARM
        a = [timed(four) for _ in range(REPS)]
    res["a_four_immediate_calls"] = stats(a, launches=l4)
    with step(120):
        for _ in range(WARM):
            sim.forces(body, x0=x0)
        n0 = L.wl_launch_count()
        b = [timed(lambda: sim.forces(body, x0=x0)) for _ in range(REPS)]
        l1 = (L.wl_launch_count() - n0) / REPS
    res["b_forces"] = stats(b, launches=l1)
    res["force_tiles"] = sim.counter("force_tiles")
    # (c) the step with and without the recorder, alternated on one handle (every step is a new flow state: both arms see the same drift)
    off, on = [], []
    for rep in range(REPS + 2):
        with step(120):
            sim.set_force_record(None)
            t_off = timed(sim.mom_step_)
        with step(120):
            sim.set_force_record(body, x0=x0, capacity=4)
            t_on = timed(sim.mom_step_)
            sim.read_forces()
        if rep >= 2:
            off.append(t_off); on.append(t_on)
    res["c_step_without_recorder"] = stats(off)
    res["c_step_with_recorder"] = stats(on, ms_median_of_differences=statistics.median([q - p for p, q in zip(off, on)]))
    sim.set_force_record(None)
    # (d) the history of NSTEPS steps: one mom_steps_ call with the recorder / single steps each followed by the four read-outs
    rec, loop = [], []

    def hand_loop():
        for _ in range(NSTEPS):
            sim.mom_step_()
            four()

    for rep in range(REPS // 3 + 1):
        with step(300):
            sim.set_force_record(body, x0=x0, capacity=NSTEPS)
            t_rec = timed(lambda: sim.mom_steps_(NSTEPS))
            assert len(sim.read_forces()[0]) == NSTEPS
            sim.set_force_record(None)
        with step(300):
            t_loop = timed(hand_loop)
        if rep >= 1:
            rec.append(t_rec / NSTEPS); loop.append(t_loop / NSTEPS)
    res["d_recorded_mom_steps_per_step"] = stats(rec, steps_per_call=NSTEPS)
    res["d_single_steps_plus_four_calls_per_step"] = stats(loop, steps_per_call=NSTEPS)
    added = res["c_step_with_recorder"]["ms_median_of_differences"]
    res["conditions"] = {
        "c_added_ms_per_step": added, "a_ms": res["a_four_immediate_calls"]["ms_median"], "c_added_below_a": added < res["a_four_immediate_calls"]["ms_median"],
        "d_recorded_ms_per_step": res["d_recorded_mom_steps_per_step"]["ms_median"], "d_loop_ms_per_step": res["d_single_steps_plus_four_calls_per_step"]["ms_median"],
        "d_recorded_faster": res["d_recorded_mom_steps_per_step"]["ms_median"] < res["d_single_steps_plus_four_calls_per_step"]["ms_median"]}
    out = {"what": __doc__.split("\n")[0], "device": torch.cuda.get_device_name(0), "result": res}
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
