#!/usr/bin/env python3
"""Cost of the flow diagnostics (wl_metrics.hip) on a developed 256³ and 512³ wall-bounded TGV, one process, HIP events:
per call of wl_lambda2, wl_omega_mag, wl_flow_fields with all four outputs (ke, ω, ω_mag, λ₂) and wl_flow_stats: median ms and the
fraction of 8 TB/s on the call's OWN bytes, 12 + 4·n_scalars B/cell (u read once; ω counts as three scalars; the sums write nothing).
In the same process a plain device copy of 16 B/cell (8 read + 8 written) is timed as the ceiling of that box's placement state.
Every GPU step runs under a watchdog of its own (the process exits if one does not finish in time: nothing more is started).
usage (GPU box): python tools/metrics_bench.py [out.json] [sizes...]      default: bench_out/metrics_bench.json 256 512"""
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

OUT = sys.argv[1] if len(sys.argv) > 1 else "bench_out/metrics_bench.json"
SIZES = [int(v) for v in sys.argv[2:]] or [256, 512]
WARM, REPS = 5, 30
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


def measure(call, nbytes_per_cell, cells):
    with step(60):
        n0 = L.wl_launch_count()
        for _ in range(WARM):
            call()
        launches = (L.wl_launch_count() - n0) / WARM
    with step(60):
        ts = [timed(call) for _ in range(REPS)]
    ms = statistics.median(ts)
    return {"launches": launches, "ms_median": ms, "ms_min": min(ts), "reps": REPS, "bytes_per_cell": nbytes_per_cell,
            "fraction_of_8TBps": nbytes_per_cell * cells / (ms * 1e-3) / PEAK}


def bench(N):
    res = {"N": N}
    with step(180):
        sim = w.FusedSimulation((N, N, N), (0, 0, 0), N, U=1, nu=N / 1600.0, ic="tgv")
        sim.mom_steps_(5)
        Ng = sim.Ng
        u = w.jl_zeros(Ng + (3,))
        check(L.wl_d2d(ptr(u), L.wl_sim_field(sim._h, b"u"), 4 * u.numel(), stream()))
        torch.cuda.synchronize()
        del sim
        torch.cuda.empty_cache()
    cells = float(N) ** 3
    g = vgrid(u)
    ke, om, wm, l2 = w.jl_zeros(Ng), w.jl_zeros(Ng + (3,)), w.jl_zeros(Ng), w.jl_zeros(Ng)
    out3 = (C.c_double * 3)()
    res["wl_lambda2"] = measure(lambda: check(L.wl_lambda2(ptr(l2), ptr(u), C.byref(g), stream())), 16, cells)
    res["wl_omega_mag"] = measure(lambda: check(L.wl_omega_mag(ptr(wm), ptr(u), C.byref(g), stream())), 16, cells)
    res["wl_flow_fields_all4"] = measure(lambda: check(L.wl_flow_fields(ptr(u), C.byref(g), None, ptr(ke), ptr(om), ptr(wm), ptr(l2), stream())), 12 + 4 * 6, cells)
    res["wl_flow_fields_ke_omega_mag"] = measure(lambda: check(L.wl_flow_fields(ptr(u), C.byref(g), None, ptr(ke), None, ptr(wm), None, stream())), 12 + 4 * 2, cells)
    res["wl_flow_stats"] = measure(lambda: check(L.wl_flow_stats(ptr(u), C.byref(g), None, out3, None, stream())), 12, cells)
    res["stats"] = {"KE": out3[0], "enstrophy": out3[1], "max_omega": out3[2]}
    # ceiling: a device copy that moves 16 B per cell of the N³ box (8 read + 8 written)
    n = int(cells) * 2
    src, dst = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
    res["device_copy_16B_per_cell"] = measure(lambda: check(L.wl_d2d(dst.data_ptr(), src.data_ptr(), 4 * n, stream())), 16, cells)
    with step(30):
        assert bool(torch.isfinite(l2).all()) and bool(torch.isfinite(wm).all())
    del u, ke, om, wm, l2, src, dst
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
