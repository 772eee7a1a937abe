#!/usr/bin/env python3
"""Cost of the Smagorinsky–Lilly model (wl_sgs / wl_sim_set_sgs) on the 256³ and 512³ wall-bounded TGV, one process, HIP events:
  * the model's two launches alone (one wl_sgs call on a developed field): median ms and the fraction of 8 TB/s on their own bytes
    (56 B/cell: 16 for u → νₜ, 40 for u, νₜ, f → f);
  * ms per mom_step! with the model off (the default fused path) and on (the staged path), in blocks of wl_sim_mom_steps alternated on
    ONE handle, and the overhead split into "the model's launches" (2 × the leaf time: predictor + corrector) and "the rest" (what
    losing the fused conv_diff!+BDIM! launch, the deferred BC! and the device-side Δt costs).
Every GPU step runs under a watchdog of its own (the process exits if one does not finish in time: nothing more is started).
usage (GPU box): python tools/sgs_bench.py [out.json] [sizes...]      default: bench_out/sgs_bench.json 256 512"""
import ctypes as C
import faulthandler
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import waterlily_jl_amd as w
from waterlily_jl_amd._lib import check, lib
from waterlily_jl_amd.core import ptr, stream, vgrid

OUT = sys.argv[1] if len(sys.argv) > 1 else "bench_out/sgs_bench.json"
SIZES = [int(v) for v in sys.argv[2:]] or [256, 512]
CS, DELTA = 0.17, 1.0
WARM, REPS, BLOCK, ALT = 5, 30, 5, 6      # leaf: 30 timed calls; steps: 6 alternations of 5-step blocks = 30 timed steps per variant
PEAK = 8e12
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


def bench(N):
    res = {"N": N}
    with step(120):
        sim = w.FusedSimulation((N, N, N), (0, 0, 0), N, U=1, nu=N / 1600.0, ic="tgv")
        sim.mom_steps_(WARM)
    cells = float(N) ** 3
    # ---- the leaf alone, on arrays of its own (a copy of the developed u)
    with step(60):
        Ng = sim.Ng
        u = w.jl_zeros(Ng + (3,)); f = w.jl_zeros(Ng + (3,)); sg = w.jl_zeros(Ng)
        check(L.wl_d2d(ptr(u), L.wl_sim_field(sim._h, b"u"), 4 * u.numel(), stream()))
        g = vgrid(u)
        call = lambda: check(L.wl_sgs(ptr(f), ptr(sg), ptr(u), C.byref(g), CS, DELTA, stream()))      # noqa: E731
        n0 = L.wl_launch_count()
        for _ in range(WARM):
            call()
        launches = (L.wl_launch_count() - n0) / WARM
    with step(60):
        ts = [timed(call) for _ in range(REPS)]
    ms = statistics.median(ts)
    res["leaf"] = {"launches": launches, "ms_median": ms, "ms_min": min(ts), "reps": REPS, "bytes_per_cell": 56,
                   "fraction_of_8TBps": 56 * cells / (ms * 1e-3) / PEAK}
    del u, f, sg
    # ---- the step, off / on alternated on one handle
    per = {"off": [], "on": []}
    launches = {}
    pois = {"off": [], "on": []}
    for k in range(ALT + 1):                  # block 0 of each variant is warm-up
        for name in ("off", "on"):
            with step(120):
                sim.set_sgs(CS if name == "on" else None, DELTA)
                n0, p0 = L.wl_launch_count(), len(sim.pois_n)
                t = timed(lambda: sim.mom_steps_(BLOCK))
                if k:
                    per[name].append(t / BLOCK)
                    launches[name] = (L.wl_launch_count() - n0) / BLOCK
                    pois[name] += sim.pois_n[p0:]
    off, on = statistics.median(per["off"]), statistics.median(per["on"])
    res["step"] = {"blocks": ALT, "steps_per_block": BLOCK,
                   "off": {"ms_per_step_median": off, "ms_per_step_min": min(per["off"]), "launches_per_step": launches["off"], "mean_pois_n": sum(pois["off"]) / len(pois["off"])},
                   "on": {"ms_per_step_median": on, "ms_per_step_min": min(per["on"]), "launches_per_step": launches["on"], "mean_pois_n": sum(pois["on"]) / len(pois["on"])},
                   "overhead_ms": on - off, "model_launches_ms": 2 * ms, "rest_ms": on - off - 2 * ms}
    with step(30):
        assert all(bool(torch.isfinite(torch.as_tensor(sim.field(k))).all()) for k in ("u", "p"))
    del sim
    torch.cuda.empty_cache()
    return res


def main():
    check(L.wl_init(0))
    out = {"what": __doc__.split("\n")[0], "Cs": CS, "Delta": DELTA, "device": torch.cuda.get_device_name(0), "cases": [bench(N) for N in SIZES]}
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
