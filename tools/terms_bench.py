"""Separable terms: what the two kernels and a step with terms cost (writes profiles/terms_bench.json; discussion: profiles/terms_experiments.md).

  python tools/terms_bench.py [--parent-lib PATH] [--sizes 256 512] [--reps 30] [--no-leaf-sim]

One process, HIP events, variants alternating inside every repetition, median of --reps (the spread max − min is reported next to it).

  leaf      k_accel_terms<1> (wl_accel_terms, K = 1) against wl_accelerate_field on the same arrays — the latter from --parent-lib when given (a build of the
            parent commit loaded next to this one), else from this library; K = 2, 3, 4 next to a device copy of the same bytes, (K+2)·4 B per element.
  step      one mom_step! of the handle at 256³ (TGV): default / uniform forcing (the staged step) / K = 1 profile + acceleration / the K = 4 rotating set.
  leaf_sim  one step of the leaf-path Simulation with closures at 64³, host tabulation included: what position-dependent uBC and g cost without the terms.
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "spread_ms": ms[-1] - ms[0], "n": len(ms)}


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(torch, variants, reps, warm=3):
    """variants: {name: callable}; every repetition runs each once, in turn"""
    out = {k: [] for k in variants}
    for r in range(warm + reps):
        for k, fn in variants.items():
            t = timed(torch, fn)
            if r >= warm:
                out[k].append(t)
    return {k: stats(v) for k, v in out.items()}


def leaf_bench(w, torch, parent, N, reps):
    L = w.lib()
    Ng = (N + 2,) * 3
    n = int(np.prod(Ng)) * 3
    g = w.core.grid_of(Ng)
    r = w.jl_zeros(Ng + (3,))
    F = [w.jl_zeros(Ng + (3,), fill=0.25 * (k + 1)) for k in range(4)]
    Fp = (C.c_void_p * 4)(*[w.core.ptr(f) for f in F])
    cp = (C.c_float * 4)(1e-3, -2e-3, 3e-3, -4e-3)
    st = w.core.stream()
    P = w.core.ptr
    acc_field = (parent or L).wl_accelerate_field
    res = {"N": N, "elements": n}
    v = {"accelerate_field": lambda: acc_field(P(r), P(F[0]), C.byref(g), st), "accel_terms_K1": lambda: L.wl_accel_terms(P(r), 1, Fp, cp, C.byref(g), st)}
    res["K1"] = alternate(torch, v, reps)
    res["K1"]["bytes"] = 12 * n
    for K in (2, 3, 4):
        m = (K + 2) * n // 2      # floats read and as many written: (K+2)·4 B per element in all
        src, dst = torch.empty(m, dtype=torch.float32, device="cuda"), torch.empty(m, dtype=torch.float32, device="cuda")
        src.fill_(1.0)
        v = {"copy": lambda: L.wl_d2d(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), 4 * m, st),
             f"accel_terms_K{K}": lambda K=K: L.wl_accel_terms(P(r), K, Fp, cp, C.byref(g), st)}
        res[f"K{K}"] = alternate(torch, v, reps)
        res[f"K{K}"]["bytes"] = (K + 2) * 4 * n
        del src, dst
    m = 3 * n // 2
    src, dst = torch.empty(m, dtype=torch.float32, device="cuda"), torch.empty(m, dtype=torch.float32, device="cuda")
    src.fill_(1.0)
    res["K1_copy"] = alternate(torch, {"copy": lambda: L.wl_d2d(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), 4 * m, st)}, reps)["copy"]
    for K in (1, 2, 3, 4):
        e = res[f"K{K}"]
        t = e[f"accel_terms_K{K}"]["median_ms"]
        c = (res["K1_copy"] if K == 1 else e["copy"])["median_ms"]
        e["TB_per_s"] = e["bytes"] / t * 1e-9
        e["rate_vs_copy"] = c / t
    return res


def step_bench(w, torch, N, reps):
    dims = (N, N, N)
    Ng = tuple(n + 2 for n in dims)
    nu = N / 1600.0
    om = 1.0 / N
    mk = lambda **kw: w.FusedSimulation(dims, (0, 0, 0), N, U=1, nu=nu, ic="tgv", **kw)      # noqa: E731
    prof = w.tabulate(lambda i, x: 1e-3 * x[1] / np.float32(N) if i == 1 else 0.0, dims)
    y = lambda x, d: np.float32(om) * (x[d] - np.float32(N / 2))      # noqa: E731
    rot = [w.tabulate(lambda i, x, j=j, d=d: 1e-3 * y(x, d) if i == j else 0.0, dims) for j in (1, 2) for d in (0, 1)]
    sc = lambda t: (math.sin(om * t), math.cos(om * t))      # noqa: E731
    sims = {
        "default": mk(),
        "uniform_forcing": mk(g=lambda i, t: 1e-3 if i == 1 else 0.0),
        "K1_profile_accel": mk(terms=[prof], g_t=[1.0], b_t=[0.0]),
        "K4_rotating": mk(terms=rot, b_t=lambda t: [0.0] * 4, db_t=lambda t: [0.0] * 4,      # (walls at rest: the TGV stays the flow; the coefficients are evaluated per step)
                          g_t=lambda t: [-2 * om * sc(t)[1] + om, 2 * om * sc(t)[0], -2 * om * sc(t)[0], -2 * om * sc(t)[1] + om]),
    }
    del prof, rot
    res = alternate(torch, {k: s.mom_step_ for k, s in sims.items()}, reps)
    base = res["uniform_forcing"]["median_ms"]
    for k in ("K1_profile_accel", "K4_rotating"):
        res[k]["cost_over_uniform_forcing_ms"] = res[k]["median_ms"] - base
    res["N"] = N
    res["solver_iterations_total"] = {k: int(sum(s.pois_n)) for k, s in sims.items()}      # the same for all four, or the step times compare different solves
    res["launches_per_step"] = {}
    for k, s in sims.items():
        l0 = s.counter("launches"); s.mom_step_(); res["launches_per_step"][k] = s.counter("launches") - l0
    return res


def leaf_sim_bench(w, N):
    L = N
    prof = lambda i, x, t: float(x[1]) / L if i == 1 else 0.0      # noqa: E731
    gfn = lambda i, x, t: -0.1 * float(x[1]) / L if i == 3 else 0.0      # noqa: E731
    t0 = time.perf_counter()
    sim = w.Simulation((N, N, N), prof, L, nu=0.01, U=1, g=gfn, duBC_dt=lambda i, x, t: 0.0)
    t1 = time.perf_counter()
    sim.sim_step_(remeasure=False)
    w.lib().wl_stream_sync(w.core.stream())
    t2 = time.perf_counter()
    return {"N": N, "construct_s": t1 - t0, "one_step_s": t2 - t1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--sizes", type=int, nargs="*", default=[256, 512])
    ap.add_argument("--step-size", type=int, default=256)
    ap.add_argument("--leaf-sim-size", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--no-leaf-sim", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "terms_bench.json"))
    a = ap.parse_args()
    import torch
    import waterlily_jl_amd as w
    w.core.device()
    parent = None
    if a.parent_lib:
        parent = C.CDLL(os.path.abspath(a.parent_lib))
        parent.wl_accelerate_field.restype, parent.wl_accelerate_field.argtypes = w.SIGNATURES["wl_accelerate_field"]
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "accelerate_field_from": "parent build" if parent else "this build", "leaf": [], }
    for N in a.sizes:
        out["leaf"].append(leaf_bench(w, torch, parent, N, a.reps))
        torch.cuda.empty_cache()
    out["step"] = step_bench(w, torch, a.step_size, a.reps)
    if not a.no_leaf_sim:
        out["leaf_sim"] = leaf_sim_bench(w, a.leaf_sim_size)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
