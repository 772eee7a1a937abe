#!/usr/bin/env python3
"""What a distance field from a mesh costs (wl_sdf_lattice_from_mesh, csrc/wl_meshsdf.hip): the whole call — tables built on the host, uploads, the search,
the read-back — culled and brute force, with the exact pair tests made of samples × elements, for
  - an icosphere of 20 480 faces, R = 32, into the 78³ lattice of tools/lattice_bench.py (spacing 1),
  - a torus of 20 480 faces (R = 24, r = 8) into a lattice laid by mesh_body's placement rule,
and beside them SdfLattice.bake of the closed-form sphere at the same 78³ (the device's point probe).  One process, the variants alternating, the median of
--reps runs each (at least 10).  HIP events are recorded on the default stream around the library call: the call synchronises, so the event pair spans the
uploads, the launch and the read-back; "host_ms" is the wall time of the same call and includes the host-side tables.
Usage: meshsdf_bench.py [--reps N] [--out FILE] (default 10, profiles/meshsdf_bench.json)."""
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
import waterlily_jl_amd as w  # noqa: E402
from waterlily_jl_amd._lib import check  # noqa: E402


def icosphere(level, R, centre):
    t = (1 + 5 ** 0.5) / 2
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    V = [np.array(v, np.float64) / np.linalg.norm(v) for v in V]
    for _ in range(level):
        mid, G = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                q = V[a] + V[b]
                V.append(q / np.linalg.norm(q))
                mid[k] = len(V) - 1
            return mid[k]
        for a, b, c in F:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            G += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = G
    return (np.array(V) * R + np.asarray(centre, np.float64)).astype(np.float32), np.array(F, np.int32)


def torus(nu, nv, R, r):
    a, b = 2 * np.pi * np.arange(nu) / nu, 2 * np.pi * np.arange(nv) / nv
    V = np.array([((R + r * np.cos(q)) * np.cos(p), (R + r * np.cos(q)) * np.sin(p), r * np.sin(q)) for p in a for q in b])
    ix = lambda i, j: (i % nu) * nv + (j % nv)      # noqa: E731
    E = [t for i in range(nu) for j in range(nv) for t in ((ix(i, j), ix(i + 1, j), ix(i + 1, j + 1)), (ix(i, j), ix(i + 1, j + 1), ix(i, j + 1)))]
    return V.astype(np.float32), np.array(E, np.int32)


def pairs():
    a, b = C.c_uint64(), C.c_uint64()
    check(w.lib().wl_meshsdf_last_pairs(C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record(); fn(); b.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return a.elapsed_time(b), 1e3 * host


def run(reps):
    n = 78
    R, c = 32.0, (63.0,) * 3                                     # tools/lattice_bench.py at N = 256: R = N/8, c = N/2 − 1, n = 2(R + 6) + 2
    origin = tuple(v - (n - 2) / 2 for v in c)
    sphere = w.Body(("sphere", c, R))
    ico = icosphere(5, R, c)
    tor = torus(160, 64, 24.0, 8.0)
    tdims, torigin = w.bodies.mesh_placement(tor[0], 1.0, 5.0)
    assert len(ico[1]) == 20480 and len(tor[1]) == 20480
    cases = {"icosphere 20480 faces, R = 32, 78^3": (ico, (n, n, n), origin), f"torus 20480 faces, R = 24, r = 8, {'x'.join(map(str, tdims))}": (tor, tdims, torigin)}
    variants = {}
    for name, ((V, E), dims, org) in cases.items():
        for brute in (False, True):
            def one(V=V, E=E, dims=dims, org=org, brute=brute):
                w.SdfLattice.from_mesh(V, E, dims, org, 1.0, brute=brute).close()
            variants[f"from_mesh({name}){', brute force' if brute else ''}"] = one
    variants["bake(closed-form sphere, 78^3)"] = lambda: w.SdfLattice.bake(sphere, (n, n, n), origin, 1.0).close()
    res = {k: {"event_ms": [], "host_ms": []} for k in variants}
    for k, fn in variants.items():                               # warm-up: code objects, the scratch at its size
        fn()
        if k.startswith("from_mesh"):
            res[k]["pairs_tested"], res[k]["pairs_total"] = pairs()
    for _ in range(max(10, reps)):
        for k, fn in variants.items():
            e, h = timed(fn)
            res[k]["event_ms"].append(e); res[k]["host_ms"].append(h)
    out = {}
    for k, r in res.items():
        out[k] = {"median_event_ms": float(np.median(r["event_ms"])), "min_event_ms": float(np.min(r["event_ms"])), "max_event_ms": float(np.max(r["event_ms"])),
                  "median_host_ms": float(np.median(r["host_ms"])), "n": len(r["event_ms"])}
        if "pairs_tested" in r:
            out[k].update(pairs_tested=r["pairs_tested"], pairs_total=r["pairs_total"], tested_fraction=r["pairs_tested"] / r["pairs_total"])
    # the culled and the brute-force samples, as bits
    for name, ((V, E), dims, org) in cases.items():
        with w.SdfLattice.from_mesh(V, E, dims, org, 1.0) as a, w.SdfLattice.from_mesh(V, E, dims, org, 1.0, brute=True) as b:
            out[f"from_mesh({name})"]["bits_equal_brute"] = bool(np.array_equal(a.values().view(np.uint32), b.values().view(np.uint32)))
            out[f"from_mesh({name})"]["edge_min"] = a.edge_min
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    check(w.lib().wl_init(0))
    r = run(a.reps)
    path = a.out or os.path.join(ROOT, "profiles", "meshsdf_bench.json")
    with open(path, "w") as fh:
        json.dump(r, fh, indent=1)
        fh.write("\n")
    print(json.dumps(r), flush=True)
