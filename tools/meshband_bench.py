#!/usr/bin/env python3
"""What band-limited baking gains, and whether it costs the un-banded calls anything.  One process on one MI355X; the variants of a series alternate, the
median, minimum and maximum of 10 runs each: host wall time of the synchronous calls (they synchronise their stream), the kernel from the fenced phases of
wl_meshsdf_time, ms4[2] (a stream synchronisation on either side of the one launch).

Against the parent commit (--parent-lib PATH: a build of it, the same C ABI), each series alternating the two libraries:
  from_mesh, from_moving_mesh and update_mesh, un-banded, on the 20 480-face icosphere at 78³ and the 20 480-face torus.  Verdict per series:
  |median_new − median_parent| against the parent's own max − min.  The host-table time of update_mesh (wl_meshsdf_last_times[0]) of either library.
Banded re-bakes (band = mesh_band()) against the un-banded call of the same build, call and kernel, on both meshes and on the 1 280-face R = 16 sphere;
the verdict: the banded median below the un-banded one by more than the larger of the two max − min spreads; bricks skipped and pairs tested next to it.
Against the step: at 128³ with the 1 280-face sphere, remeasured mom_step! + advance, banded and un-banded, alternated on one handle.
Usage: meshband_bench.py [--parent-lib PATH] [--out FILE] (default profiles/meshband_bench.json)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import waterlily_jl_amd as w  # noqa: E402
from waterlily_jl_amd._lib import check  # noqa: E402
from meshsdf_bench import icosphere, torus  # noqa: E402
from meshvel_bench import REPS, alternate, host_ms, stats, verdict  # noqa: E402

FP, IP = C.POINTER(C.c_float), C.POINTER(C.c_int32)
f32 = np.float32


def load_parent(path):
    P = C.CDLL(path)
    common = [C.POINTER(C.c_void_p), C.c_int, IP, FP, C.c_float, FP, C.c_int32, IP, C.c_int32]
    P.wl_sdf_lattice_from_mesh.argtypes = common + [C.c_uint, C.c_void_p]
    P.wl_sdf_lattice_from_moving_mesh.argtypes = common + [FP, C.c_uint, C.c_void_p]
    P.wl_sdf_lattice_update_mesh.argtypes = [C.c_void_p, FP, FP, C.c_uint, C.c_void_p]
    P.wl_sdf_lattice_destroy.argtypes = [C.c_void_p]
    P.wl_meshsdf_last_times.argtypes = [C.POINTER(C.c_double)]
    assert P.wl_init(0) == 0
    return P


def create(L, V, E, dims, origin, Wv=None):
    h = C.c_void_p()
    a = (C.byref(h), 3, (C.c_int32 * 3)(*dims), (C.c_float * 3)(*origin), C.c_float(1.0), V.ctypes.data_as(FP), len(V), E.ctypes.data_as(IP), len(E))
    rc = L.wl_sdf_lattice_from_mesh(*a, 0, None) if Wv is None else L.wl_sdf_lattice_from_moving_mesh(*a, Wv.ctypes.data_as(FP), 0, None)
    assert rc == 0, rc
    return h


def last(fn_name):
    a, b = C.c_uint64(), C.c_uint64()
    check(getattr(w.lib(), fn_name)(C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


def banded_verdict(series, banded, plain):
    sb, sp = series[banded], series[plain]
    spread = max(sb["max_ms"] - sb["min_ms"], sp["max_ms"] - sp["min_ms"])
    gain = sp["median_ms"] - sb["median_ms"]
    return {"banded_median_ms": sb["median_ms"], "unbanded_median_ms": sp["median_ms"], "larger_spread_ms": spread, "gain_ms": gain,
            "ratio": sb["median_ms"] / sp["median_ms"], "faster_by_more_than_the_spread": bool(gain > spread)}


def run(parent):
    lib = w.lib()
    out = {}
    n = 78
    R, c = 32.0, (63.0,) * 3
    origin = tuple(v - (n - 2) / 2 for v in c)
    tor = torus(160, 64, 24.0, 8.0)
    tdims, torigin = w.bodies.mesh_placement(tor[0], 1.0, 5.0)
    small = icosphere(3, 16.0, (0.0, 0.0, 0.0))
    sdims, sorigin = w.bodies.mesh_placement(small[0], 1.0, 6.0)
    cases = {"icosphere 20480 faces, 78^3": (icosphere(5, R, c), (n, n, n), origin),
             f"torus 20480 faces, {'x'.join(map(str, tdims))}": (tor, tdims, torigin),
             f"icosphere 1280 faces R = 16, {'x'.join(map(str, sdims))}": (small, sdims, sorigin)}
    P = load_parent(parent) if parent else None
    band = w.mesh_band()

    for name, ((V, E), dims, org) in cases.items():
        V, E = np.ascontiguousarray(V, dtype=f32), np.ascontiguousarray(E, dtype=np.int32)
        ctr = V.mean(axis=0).astype(f32)
        Wv = np.ascontiguousarray((0.05 * (V - ctr)).astype(f32))
        V1 = np.ascontiguousarray((ctr + (V - ctr) * f32(1.01)).astype(f32))
        big = "20480" in name
        # ---- the un-banded creation calls, new against parent (the destroy is outside the timed region)
        if P and big:
            hold = []

            def timer(fn):
                t = host_ms(fn)
                while hold:
                    L, h = hold.pop()
                    L.wl_sdf_lattice_destroy(h)
                return t
            variants = {"from_mesh": lambda: hold.append((lib, create(lib, V, E, dims, org))),
                        "from_mesh, parent library": lambda: hold.append((P, create(P, V, E, dims, org))),
                        "from_moving_mesh": lambda: hold.append((lib, create(lib, V, E, dims, org, Wv))),
                        "from_moving_mesh, parent library": lambda: hold.append((P, create(P, V, E, dims, org, Wv)))}
            series = alternate(variants, timer)
            for k in ("from_mesh", "from_moving_mesh"):
                series[f"verdict {k}"] = verdict(series, k, f"{k}, parent library")
            out[f"bake, {name}"] = series
        # ---- update_mesh: un-banded (new, parent) and banded, the whole call
        h_new = create(lib, V, E, dims, org, Wv)
        h_par = create(P, V, E, dims, org, Wv) if P else None
        lat_b = w.SdfLattice.from_mesh(V, E, dims, org, 1.0, vertex_velocity=Wv, band=band)
        k = [0]

        def upd(L, h):
            k[0] += 1
            assert L.wl_sdf_lattice_update_mesh(h, (V1 if k[0] % 2 else V).ctypes.data_as(FP), Wv.ctypes.data_as(FP), 0, None) == 0
        variants = {"update_mesh": lambda: upd(lib, h_new), "update_mesh, band": lambda: upd(lib, lat_b._h)}
        if P:
            variants["update_mesh, parent library"] = lambda: upd(P, h_par)
        series = alternate(variants, host_ms)
        if P:
            series["verdict update_mesh"] = verdict(series, "update_mesh", "update_mesh, parent library")
        series["verdict band, call"] = banded_verdict(series, "update_mesh, band", "update_mesh")
        # ---- the phases, fenced: host tables and the kernel
        check(lib.wl_meshsdf_time(1))
        if P:
            P.wl_meshsdf_time(1)
        ph = {q: [] for q in variants}
        for _ in range(REPS + 1):
            for q, fn in variants.items():
                fn()
                ms = (C.c_double * 4)()
                (P if q.endswith("parent library") else lib).wl_meshsdf_last_times(ms)
                ph[q].append(list(ms))
        check(lib.wl_meshsdf_time(0))
        if P:
            P.wl_meshsdf_time(0)
        for q in variants:
            a = np.array(ph[q][1:])
            series[f"{q}: host tables"] = stats(a[:, 0])
            series[f"{q}: kernel"] = stats(a[:, 2])
        series["verdict band, kernel"] = banded_verdict(series, "update_mesh, band: kernel", "update_mesh: kernel")
        upd(lib, h_new)
        tested_full, total = last("wl_meshsdf_last_pairs")
        upd(lib, lat_b._h)
        tested_band, _ = last("wl_meshsdf_last_pairs")
        searched, skipped = last("wl_meshsdf_last_bricks")
        series["counts"] = {"pairs_unbanded": tested_full, "pairs_banded": tested_band, "pairs_ratio": tested_band / tested_full, "pairs_all": total,
                            "bricks_searched": searched, "bricks_skipped": skipped, "band": band}
        out[f"update_mesh, {name}"] = series
        lib.wl_sdf_lattice_destroy(h_new)
        if P:
            P.wl_sdf_lattice_destroy(h_par)
        lat_b.close()

    # ---- against the step: remeasured mom_step! + advance at 128³, banded and un-banded lattices alternated on one handle
    N = 128
    V, E = small
    mp = w.RigidMap((N / 2 - 1,) * 3, (0, 0, 0))
    bodies = {q: w.mesh_body(V, E, margin=6.0, map=mp, vertex_velocity=np.zeros_like(V), band=b) for q, b in (("band", True), ("no band", None))}
    sim = w.FusedSimulation((N, N, N), (1, 0, 0), 32, U=1, nu=32 / 3700, has_body=True)
    V1 = (V * f32(1.002)).astype(f32)
    k = [0]

    def step(q, advance):
        sim.body = bodies[q]                                  # the stored body: sim_step_(remeasure=True) measures it, nothing else does
        if advance:
            k[0] += 1
            bodies[q].shape[1].advance(V1 if k[0] % 2 else V, 0.25)
        sim.sim_step_(remeasure=True)
    sim.set_body(bodies["no band"])
    variants = {"sim_step_(remeasure=True)": lambda: step("no band", False)}
    for q in bodies:
        variants[f"advance + sim_step_(remeasure=True), {q}"] = lambda q=q: step(q, True)
        variants[f"advance alone, {q}"] = lambda q=q: (k.__setitem__(0, k[0] + 1), bodies[q].shape[1].advance(V1 if k[0] % 2 else V, 0.25))
    series = alternate(variants, lambda fn: host_ms(lambda: (fn(), torch.cuda.synchronize())))
    series["verdict band, advance alone"] = banded_verdict(series, "advance alone, band", "advance alone, no band")
    series["lattice"] = list(bodies["band"].shape[1].dims)
    out["remeasured mom_step! at 128^3, icosphere 1280 faces R = 16"] = series
    for b in bodies.values():
        b.shape[1].close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    a = ap.parse_args()
    check(w.lib().wl_init(0))
    r = run(a.parent_lib)
    path = a.out or os.path.join(ROOT, "profiles", "meshband_bench.json")
    with open(path, "w") as fh:
        json.dump(r, fh, indent=1)
        fh.write("\n")
    print(json.dumps(r), flush=True)
