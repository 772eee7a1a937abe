#!/usr/bin/env python3
"""What a sampled body costs next to a closed-form one: measure!, update!(pois) and one mom_step! at N³ for
  - a closed-form sphere as a one-leaf program,
  - the same sphere baked into a lattice at spacing 1 (SdfLattice.bake),
  - a three-leaf set with one lattice leaf (the baked sphere ∪ a rotated capsule − a small sphere),
alternating on ONE handle inside one process, HIP events, the median of rounds × reps runs each.  With --parent-lib PATH the closed-form one-leaf measure!
is also timed through that library (a build of the parent commit: same C ABI, the same device arrays) in the same alternation — the A/B that says whether
the lattice branch slowed the existing leaves down.  Usage: lattice_bench.py [N] [--parent-lib PATH] [--out FILE] (default 256, profiles/lattice_bench_<N>.json)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import waterlily_jl_amd as w  # noqa: E402
from waterlily_jl_amd._lib import check, wl_bodyset, wl_grid  # noqa: E402


def timed(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def run(N, parent=None, rounds=3, reps=10):
    lib = w.lib()
    R, c = N / 8, (N / 2 - 1,) * 3
    sim = w.FusedSimulation((N, N, N), (1, 0, 0), 2 * R, U=1, nu=2 * R / 3700, has_body=True)
    f = {k: lib.wl_sim_field(sim._h, k.encode()) for k in ("sigma", "mu0", "mu1", "V")}
    g = wl_grid(); check(lib.wl_sim_grid(sim._h, C.byref(g)))
    sphere = w.Body(("sphere", c, R))
    n = int(2 * (R + 6)) + 2                                     # samples per direction: the sphere and 6 cells around it (edge_min − |R| > 2 + ϵ + 1)
    origin = tuple(v - (n - 2) / 2 for v in c)
    lat = w.SdfLattice.bake(sphere, (n, n, n), origin, 1.0)
    baked = w.Body(("lattice", lat, origin, 1.0, 0.0))
    mp = w.RigidMap(c, (0.1, 0.3, 0.2), omega=(0, 0, 0.05))
    three = (w.Body(("lattice", lat, tuple(o - v for o, v in zip(origin, c)), 1.0, 0.0), w.RigidMap(c, (0, 0, 0)))
             | w.Body(("capsule", (0, 0, 0), R / 4, (1, 0, 0), 1.5 * R), mp)) - w.Body(("sphere", (0, R, 0), R / 2), mp)
    bodies = {"sphere leaf": sphere, "baked sphere": baked, "3-leaf set with a lattice": three}
    progs = {k: b.program(3) for k, b in bodies.items()}
    args = lambda: (f["sigma"], f["mu0"], f["mu1"], f["V"], C.byref(g))   # noqa: E731
    variants = {}
    for k, b in bodies.items():
        variants[f"measure!({k})"] = lambda k=k: check(lib.wl_measure_bodyset(*args(), C.byref(progs[k]), 1.0, 0, 0, None))
        variants[f"update!(pois) after {k}"] = lambda: sim.update_()
        variants[f"mom_step! with {k}"] = lambda: sim.mom_step_()
    if parent:
        P = C.CDLL(parent)
        P.wl_measure_bodyset.restype = C.c_int
        P.wl_measure_bodyset.argtypes = [C.c_void_p] * 4 + [C.POINTER(wl_grid), C.POINTER(wl_bodyset), C.c_float, C.c_int, C.c_uint32, C.c_void_p]
        assert P.wl_init(0) == 0
        variants["measure!(sphere leaf) through the parent library"] = lambda: check(P.wl_measure_bodyset(*args(), C.byref(progs["sphere leaf"]), 1.0, 0, 0, None))
    for k, b in bodies.items():                                  # warm-up: every variant once, each body's own fields under its update! and step
        sim.measure_bodyset_(b, 1.0)
        for name, fn in variants.items():
            if k in name:
                fn()
    torch.cuda.synchronize()
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, b in bodies.items():
            res[f"measure!({k})"] += timed(variants[f"measure!({k})"], reps)
            if parent and k == "sphere leaf":
                res["measure!(sphere leaf) through the parent library"] += timed(variants["measure!(sphere leaf) through the parent library"], reps)
            sim.measure_bodyset_(b, 1.0)                         # the handle's masks and multigrid levels follow the body that is timed next
            res[f"update!(pois) after {k}"] += timed(variants[f"update!(pois) after {k}"], reps)
            res[f"mom_step! with {k}"] += timed(variants[f"mom_step! with {k}"], reps)
    out = {k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "n": len(v)} for k, v in res.items()}
    out["lattice"] = {"dims": list(lat.dims), "edge_min": lat.edge_min, "samples_MiB": 4 * n ** 3 / 2 ** 20}
    lat.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("N", nargs="?", type=int, default=256)
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    a = ap.parse_args()
    check(w.lib().wl_init(0))
    r = {f"{a.N}^3": run(a.N, a.parent_lib)}
    path = a.out or os.path.join(ROOT, "profiles", f"lattice_bench_{a.N}.json")
    with open(path, "w") as fh:
        json.dump(r, fh, indent=1)
        fh.write("\n")
    print(json.dumps(r), flush=True)
