#!/usr/bin/env python3
"""Cost of point samples, probe records and tracers (wl_interp.hip) on a developed 256³ and 512³ wall-bounded TGV, one process, HIP events,
median of 30: wl_interp of u at 10⁶ uniformly random points and at 10⁶ points of one z-plane lattice, wl_advect of 10⁶ particles, the time of a
step with and without 64 probes + 10⁶ tracers registered (off/on alternated on ONE handle, wl_sim_mom_step), and next to them the wl_d2h of u
that the feature replaces and a plain device copy of 16 B/cell as that box's ceiling.
Every GPU step runs under a watchdog of its own (the process exits if one does not finish in time: nothing more is started).
usage (GPU box): python tools/interp_bench.py [out.json] [sizes...]      default: bench_out/interp_bench.json 256 512"""
import ctypes as C
import faulthandler
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import waterlily_jl_amd as w
from waterlily_jl_amd._lib import check, lib
from waterlily_jl_amd.core import stream

OUT = sys.argv[1] if len(sys.argv) > 1 else "bench_out/interp_bench.json"
SIZES = [int(v) for v in sys.argv[2:]] or [256, 512]
WARM, REPS = 5, 30
NPTS, NPROBES = 1_000_000, 64
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


def measure(call, limit=60, **extra):
    with step(limit):
        n0 = L.wl_launch_count()
        for _ in range(WARM):
            call()
        launches = (L.wl_launch_count() - n0) / WARM
    with step(limit):
        ts = [timed(call) for _ in range(REPS)]
    return dict({"launches": launches, "ms_median": statistics.median(ts), "ms_min": min(ts), "reps": REPS}, **extra)


def P(t):
    return C.c_void_p(t.data_ptr())


def bench(N):
    res = {"N": N, "points": NPTS, "probes": NPROBES}
    rng = np.random.default_rng(1)
    with step(240):
        sim = w.FusedSimulation((N, N, N), (0, 0, 0), N, U=1, nu=N / 1600.0, ic="tgv")
        sim.mom_steps_(5)
    h = sim._h
    g = w._lib.wl_grid()
    check(L.wl_sim_grid(h, C.byref(g)))
    cells = float(N) ** 3
    xr = torch.from_numpy((rng.uniform(0, 1, (NPTS, 3)) * N).astype(np.float32)).cuda()
    side = int(round(NPTS ** 0.5))
    ax = (np.arange(side, dtype=np.float32) + 0.5) * (N / side)
    lat = np.stack(np.meshgrid(ax, ax, indexing="xy"), axis=-1).reshape(-1, 2)            # x fastest, as a plane cut is drawn
    xl = torch.from_numpy(np.concatenate([lat, np.full((side * side, 1), N / 2, dtype=np.float32)], axis=1).astype(np.float32)).cuda()
    out = torch.empty((NPTS, 3), dtype=torch.float32, device="cuda")
    u = lambda: L.wl_sim_field(h, b"u")      # noqa: E731
    # own bytes of a sample: 12 B of position + 12 B of result per point; the gathers touch up to 3·8 distinct cells (4 B each) per point
    res["wl_interp_u_random"] = measure(lambda: check(L.wl_interp(P(out), u(), C.byref(g), P(xr), NPTS, 3, stream())), gathers_per_point=24)
    res["wl_interp_u_plane_lattice"] = measure(lambda: check(L.wl_interp(P(out), u(), C.byref(g), P(xl), side * side, 3, stream())), points=side * side, gathers_per_point=24)
    xa, xb = xr.clone(), torch.empty_like(xr)
    u0 = lambda: L.wl_sim_field(h, b"u0")      # noqa: E731
    res["wl_advect"] = measure(lambda: check(L.wl_advect(P(xa), P(xb), u0(), u(), C.byref(g), NPTS, 0.1, 0, stream())), gathers_per_point=48)
    # the step with and without observers, alternated on one handle (every step is a new flow state: both arms see the same drift)
    probes = (rng.uniform(0, 1, (NPROBES, 3)) * N).astype(np.float32)
    tracers = (rng.uniform(0, 1, (NPTS, 3)) * N).astype(np.float32)
    off, on = [], []
    for rep in range(REPS + 2):
        with step(120):
            sim.set_probes(None, 0); sim.set_tracers(None)
            t_off = timed(sim.mom_step_)
        with step(120):
            sim.set_probes(probes, 4); sim.set_tracers(tracers)
            t_on = timed(sim.mom_step_)
            sim.read_probes()
        if rep >= 2:
            off.append(t_off); on.append(t_on)
    sim.set_probes(None, 0); sim.set_tracers(None)
    res["step_without_observers"] = {"ms_median": statistics.median(off), "ms_min": min(off), "reps": REPS}
    res["step_with_64_probes_1e6_tracers"] = {"ms_median": statistics.median(on), "ms_min": min(on), "reps": REPS,
                                              "ms_median_of_differences": statistics.median([b - a for a, b in zip(off, on)])}
    # what the feature replaces: u to the host (pinned memory), and the box's copy ceiling
    nu = int(g.nx) * int(g.ny) * int(g.nz) * 3
    host = torch.empty(nu, dtype=torch.float32).pin_memory()
    res["wl_d2h_of_u"] = measure(lambda: check(L.wl_d2h(C.c_void_p(host.data_ptr()), u(), 4 * nu, stream())), limit=240, bytes=4 * nu)
    n = int(cells) * 2
    src, dst = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
    m = measure(lambda: check(L.wl_d2d(dst.data_ptr(), src.data_ptr(), 4 * n, stream())))
    m["fraction_of_8TBps"] = 16 * cells / (m["ms_median"] * 1e-3) / PEAK
    res["device_copy_16B_per_cell"] = m
    with step(30):
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(xa).all())
    del sim, src, dst, host, out, xr, xl, xa, xb
    torch.cuda.empty_cache()
    return res


def main():
    check(L.wl_init(0))
    out = {"what": __doc__.split("\n")[0], "device": torch.cuda.get_device_name(0), "peak_Bps": PEAK, "cases": [bench(N) for N in SIZES]}
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
