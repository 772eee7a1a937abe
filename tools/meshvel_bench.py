#!/usr/bin/env python3
"""What deforming meshes cost, and whether they cost the existing paths anything.  One process on one MI355X; the variants of a series alternate, the median,
minimum and maximum of 10 runs each (host wall time of the synchronous calls, HIP events around the asynchronous ones).

Against the parent commit (--parent-lib PATH: a build of it, the same C ABI on the same device arrays), each series alternating the two libraries:
  from_mesh without velocities on the 20 480-face icosphere at 78³ and the 20 480-face torus; measure! of a closed-form one-leaf sphere at 256³; measure! of
  a baked lattice (no velocity samples) at 256³.  Verdict per series: |median_new − median_parent| against the parent's own max − min.
New, reported only:
  from_moving_mesh against from_mesh on the two cases; update_mesh split into host tables / uploads / kernel / read-back (wl_meshsdf_time) for icospheres of
  1 280 and 20 480 faces; measure! of a lattice with velocity samples against one without; one remeasured mom_step! at 128³ around an R = 16 sphere with and
  without the per-step update_mesh.
Usage: meshvel_bench.py [--parent-lib PATH] [--out FILE] (default profiles/meshvel_bench.json)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import waterlily_jl_amd as w  # noqa: E402
from waterlily_jl_amd._lib import check, wl_bodyset, wl_grid  # noqa: E402
from meshsdf_bench import icosphere, torus  # noqa: E402

REPS = 10
FP, IP = C.POINTER(C.c_float), C.POINTER(C.c_int32)


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "n": len(v)}


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(variants, timer, reps=REPS):
    for fn in variants.values():
        fn()
    res = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            res[k].append(timer(fn))
    return {k: stats(v) for k, v in res.items()}


def verdict(series, new, parent):
    spread = series[parent]["max_ms"] - series[parent]["min_ms"]
    diff = series[new]["median_ms"] - series[parent]["median_ms"]
    return {"new_median_ms": series[new]["median_ms"], "parent_median_ms": series[parent]["median_ms"], "parent_spread_ms": spread, "diff_ms": diff,
            "within_parent_spread": bool(abs(diff) <= spread)}


def raw_from_mesh(L, V, E, dims, origin):
    h = C.c_void_p()
    rc = L.wl_sdf_lattice_from_mesh(C.byref(h), 3, (C.c_int32 * 3)(*dims), (C.c_float * 3)(*origin), C.c_float(1.0), V.ctypes.data_as(FP), len(V),
                                    E.ctypes.data_as(IP), len(E), 0, None)
    assert rc == 0, rc
    return h


def load_parent(path):
    P = C.CDLL(path)
    P.wl_measure_bodyset.restype = C.c_int
    P.wl_measure_bodyset.argtypes = [C.c_void_p] * 4 + [C.POINTER(wl_grid), C.POINTER(wl_bodyset), C.c_float, C.c_int, C.c_uint32, C.c_void_p]
    P.wl_sdf_lattice_from_mesh.argtypes = [C.POINTER(C.c_void_p), C.c_int, IP, FP, C.c_float, FP, C.c_int32, IP, C.c_int32, C.c_uint, C.c_void_p]
    P.wl_sdf_lattice_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, IP, FP, C.c_void_p]
    P.wl_sdf_lattice_destroy.argtypes = [C.c_void_p]
    P.wl_sdf_lattice_id.argtypes = [C.c_void_p]
    assert P.wl_init(0) == 0
    return P


def run(parent):
    lib = w.lib()
    out = {}
    n = 78
    R, c = 32.0, (63.0,) * 3
    origin = tuple(v - (n - 2) / 2 for v in c)
    ico = icosphere(5, R, c)
    tor = torus(160, 64, 24.0, 8.0)
    tdims, torigin = w.bodies.mesh_placement(tor[0], 1.0, 5.0)
    cases = {"icosphere 20480 faces, 78^3": (ico, (n, n, n), origin), f"torus 20480 faces, {'x'.join(map(str, tdims))}": (tor, tdims, torigin)}
    P = load_parent(parent) if parent else None

    # ---- from_mesh: new against parent, and from_moving_mesh against from_mesh (the destroy is outside the timed region)
    for name, ((V, E), dims, org) in cases.items():
        V, E = np.ascontiguousarray(V), np.ascontiguousarray(E)
        Wv = np.ascontiguousarray((0.05 * (V - V.mean(axis=0))).astype(np.float32))
        hold = {}

        def static(L=lib, key="s"):
            hold[key] = raw_from_mesh(L, V, E, dims, org)

        def moving():
            hold["m"] = w.SdfLattice.from_mesh(V, E, dims, org, 1.0, vertex_velocity=Wv)

        def timer(fn):
            t = host_ms(fn)
            for k in list(hold):
                h = hold.pop(k)
                (h.close() if hasattr(h, "close") else (P if k == "p" else lib).wl_sdf_lattice_destroy(h))
            return t
        variants = {"from_mesh": static, "from_moving_mesh": moving}
        if P:
            variants["from_mesh, parent library"] = lambda: static(P, "p")
        for fn in variants.values():
            timer(fn)
        series = {k: [] for k in variants}
        for _ in range(REPS):
            for k, fn in variants.items():
                series[k].append(timer(fn))
        series = {k: stats(v) for k, v in series.items()}
        out[f"bake, {name}"] = series
        if P:
            out[f"bake, {name}"]["verdict from_mesh"] = verdict(series, "from_mesh", "from_mesh, parent library")

    # ---- update_mesh, split (the phases fenced: wl_meshsdf_time) and whole (not fenced)
    for level, faces in ((3, 1280), (5, 20480)):
        V, E = icosphere(level, R, c)
        lat = w.SdfLattice.from_mesh(V, E, (n, n, n), origin, 1.0, vertex_velocity=np.zeros_like(V))
        V1 = (np.asarray(c, np.float32) + (V - np.asarray(c, np.float32)) * np.float32(1.01)).astype(np.float32)
        whole = [host_ms(lambda: lat.advance(V1 if k % 2 == 0 else V, 0.25)) for k in range(REPS + 1)][1:]
        check(lib.wl_meshsdf_time(1))
        phases = []
        for k in range(REPS + 1):
            lat.advance(V1 if k % 2 == 0 else V, 0.25)
            ms = (C.c_double * 4)()
            check(lib.wl_meshsdf_last_times(ms))
            phases.append(list(ms))
        check(lib.wl_meshsdf_time(0))
        ph = np.median(np.array(phases[1:]), axis=0)
        out[f"update_mesh, icosphere {faces} faces, 78^3"] = {"call": stats(whole), "host_tables_ms": float(ph[0]), "uploads_ms": float(ph[1]), "kernel_ms": float(ph[2]),
                                                             "read_back_ms": float(ph[3])}
        lat.close()

    # ---- measure! at 256³: closed form and baked lattice against the parent; a lattice with velocity samples against one without
    N = 256
    Rb, cb = N / 8, (N / 2 - 1,) * 3
    sim = w.FusedSimulation((N, N, N), (1, 0, 0), 2 * Rb, U=1, nu=2 * Rb / 3700, has_body=True)
    f = {k: lib.wl_sim_field(sim._h, k.encode()) for k in ("sigma", "mu0", "mu1", "V")}
    g = wl_grid(); check(lib.wl_sim_grid(sim._h, C.byref(g)))
    args = lambda: (f["sigma"], f["mu0"], f["mu1"], f["V"], C.byref(g))   # noqa: E731
    sphere = w.Body(("sphere", cb, Rb))
    nb = int(2 * (Rb + 6)) + 2
    ob = tuple(v - (nb - 2) / 2 for v in cb)
    lat = w.SdfLattice.bake(sphere, (nb, nb, nb), ob, 1.0)
    vals = lat.values()
    latw = w.SdfLattice(vals)
    latw.set_velocity(np.full(latw.dims + (3,), 0.125, np.float32))
    progs = {"sphere leaf": sphere.program(3), "baked lattice": w.Body(("lattice", lat, ob, 1.0, 0.0)).program(3),
             "baked lattice with velocity samples": w.Body(("lattice", latw, ob, 1.0, 0.0)).program(3)}
    variants = {f"measure!({k})": (lambda k=k: check(lib.wl_measure_bodyset(*args(), C.byref(progs[k]), 1.0, 0, 0, None))) for k in progs}
    if P:
        hp = C.c_void_p()
        flat = np.ascontiguousarray(vals.reshape(-1, order="F"))
        assert P.wl_sdf_lattice_create(C.byref(hp), 3, (C.c_int32 * 3)(nb, nb, nb), flat.ctypes.data_as(FP), None) == 0

        class Named:
            D, id = 3, int(P.wl_sdf_lattice_id(hp))
        pprog = w.Body(("lattice", Named(), ob, 1.0, 0.0)).program(3)
        variants["measure!(sphere leaf), parent library"] = lambda: check(P.wl_measure_bodyset(*args(), C.byref(progs["sphere leaf"]), 1.0, 0, 0, None))
        variants["measure!(baked lattice), parent library"] = lambda: check(P.wl_measure_bodyset(*args(), C.byref(pprog), 1.0, 0, 0, None))
    series = alternate(variants, event_ms)
    out["measure! at 256^3"] = series
    if P:
        series["verdict sphere leaf"] = verdict(series, "measure!(sphere leaf)", "measure!(sphere leaf), parent library")
        series["verdict baked lattice"] = verdict(series, "measure!(baked lattice)", "measure!(baked lattice), parent library")
        P.wl_sdf_lattice_destroy(hp)
    lat.close(); latw.close()
    del sim

    # ---- one remeasured mom_step! at 128³ around an R = 16 sphere, with and without the per-step update_mesh
    N = 128
    V, E = icosphere(3, 16.0, (0.0, 0.0, 0.0))
    body = w.mesh_body(V, E, margin=6.0, map=w.RigidMap((N / 2 - 1,) * 3, (0, 0, 0)), vertex_velocity=np.zeros_like(V))
    sim = w.FusedSimulation((N, N, N), (1, 0, 0), 32, U=1, nu=32 / 3700, has_body=True)
    sim.set_body(body)
    V1 = (V * np.float32(1.002)).astype(np.float32)
    k = [0]

    def step_only():
        sim.sim_step_(remeasure=True)

    def update_and_step():
        k[0] += 1
        body.shape[1].advance(V1 if k[0] % 2 else V, 0.25)
        sim.sim_step_(remeasure=True)

    def update_only():
        k[0] += 1
        body.shape[1].advance(V1 if k[0] % 2 else V, 0.25)
    out["remeasured mom_step! at 128^3, icosphere 1280 faces R = 16"] = alternate(
        {"sim_step_(remeasure=True)": step_only, "advance + sim_step_(remeasure=True)": update_and_step, "advance alone": update_only},
        lambda fn: host_ms(lambda: (fn(), torch.cuda.synchronize())))
    out["remeasured mom_step! at 128^3, icosphere 1280 faces R = 16"]["lattice"] = list(body.shape[1].dims)
    body.shape[1].close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    a = ap.parse_args()
    check(w.lib().wl_init(0))
    r = run(a.parent_lib)
    path = a.out or os.path.join(ROOT, "profiles", "meshvel_bench.json")
    with open(path, "w") as fh:
        json.dump(r, fh, indent=1)
        fh.write("\n")
    print(json.dumps(r), flush=True)
