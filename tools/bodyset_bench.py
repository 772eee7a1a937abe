#!/usr/bin/env python3
"""measure! and the force / moment read-outs of a closed-form wl_body against the same body as a one-leaf wl_bodyset, and a 3-leaf rotated
set, on the arrays of an N³ composite handle; plus update!(pois) and one mom_step! of the same flow for scale.  HIP events, the variants
alternate inside one process.  Usage: bodyset_bench.py [N ...] (default 256 512).

The wl_body entry points ARE the one-leaf program now (wl::bodyset_from_body): the first two measure! variants, and each *_body / *_bodyset
pair of read-outs, run the same kernels (the pressure sums of a single sphere or plane k_pforce_body, whichever way they come) and differ only in how
the host builds the program.  On the commit before that they were two kernel families (3 fills + k_measure_body; k_pforce_body / k_vforce_body
against k_*_set), which is what the figures in profiles/onebody_experiments.md compare."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import waterlily_jl_amd as w  # noqa: E402
from waterlily_jl_amd._lib import check, make_body, wl_grid  # noqa: E402


def timed(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def run(N, rounds=5, reps=10):
    lib = w.lib()
    R, c = N / 8, (N / 2 - 1,) * 3
    sim = w.FusedSimulation((N, N, N), (1, 0, 0), 2 * R, U=1, nu=2 * R / 3700, has_body=True)
    f = {k: lib.wl_sim_field(sim._h, k.encode()) for k in ("sigma", "mu0", "mu1", "V", "p", "u")}
    g = wl_grid(); check(lib.wl_sim_grid(sim._h, C.byref(g)))
    old = make_body(("sphere", c, R), 3)
    leaf = w.Body(("sphere", c, R)).program(3)
    rot = (w.Body(("capsule", (0, 0, 0), R / 4, (1, 0, 0), R), w.RigidMap(c, (0.1, 0.3, 0.2), omega=(0, 0, 0.05)))
           | w.Body(("sphere", (0, 0, 0), R / 2), w.RigidMap(c, (0, 0, 0.4), xp=(R, 0, 0), omega=(0, 0, 0.05)))
           | w.Body(("cylinder", (0, 0, 0), R / 3, 2), w.RigidMap(c, (0.3, 0, 0), xp=(-R, 0, 0)))).program(3)
    args = lambda: (f["sigma"], f["mu0"], f["mu1"], f["V"], C.byref(g))   # noqa: E731
    x0 = (C.c_float * 3)(N / 2 + 0.3, N / 2 - 1.3, N / 2 + 2.1)
    out = (C.c_double * 3)()
    nu = 2 * R / 3700
    variants = {
        "wl_measure_body(sphere)": lambda: check(lib.wl_measure_body(*args(), C.byref(old), 1.0, 0, 0, None)),
        "wl_measure_bodyset(sphere leaf)": lambda: check(lib.wl_measure_bodyset(*args(), C.byref(leaf), 1.0, 0, 0, None)),
        "wl_measure_bodyset(3-leaf rotated set)": lambda: check(lib.wl_measure_bodyset(*args(), C.byref(rot), 1.0, 0, 0, None)),
        "wl_pressure_force_body": lambda: check(lib.wl_pressure_force_body(f["p"], C.byref(g), C.byref(old), out, None)),
        "wl_pressure_force_bodyset(leaf)": lambda: check(lib.wl_pressure_force_bodyset(None, f["p"], C.byref(g), C.byref(leaf), out, None)),
        "wl_viscous_force_body": lambda: check(lib.wl_viscous_force_body(f["u"], C.byref(g), nu, C.byref(old), out, None)),
        "wl_viscous_force_bodyset(leaf)": lambda: check(lib.wl_viscous_force_bodyset(None, f["u"], C.byref(g), nu, C.byref(leaf), out, None)),
        "wl_pressure_moment_body": lambda: check(lib.wl_pressure_moment_body(x0, f["p"], C.byref(g), C.byref(old), out, None)),
        "wl_pressure_moment_bodyset(leaf)": lambda: check(lib.wl_pressure_force_bodyset(x0, f["p"], C.byref(g), C.byref(leaf), out, None)),
        "wl_viscous_moment_body": lambda: check(lib.wl_viscous_moment_body(x0, f["u"], C.byref(g), nu, C.byref(old), out, None)),
        "wl_viscous_moment_bodyset(leaf)": lambda: check(lib.wl_viscous_force_bodyset(x0, f["u"], C.byref(g), nu, C.byref(leaf), out, None)),
        "update!(pois)": lambda: sim.update_(),
        "mom_step!": lambda: sim.mom_step_(),
    }
    sim.measure_sphere_(c, R, 1.0)
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            if k == "mom_step!":
                sim.measure_sphere_(c, R, 1.0)
            res[k] += timed(fn, reps)
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "n": len(v)} for k, v in res.items()}


if __name__ == "__main__":
    check(w.lib().wl_init(0))
    sizes = [int(a) for a in sys.argv[1:]] or [256, 512]
    for N in sizes:
        print(json.dumps({f"{N}^3": run(N)}), flush=True)
