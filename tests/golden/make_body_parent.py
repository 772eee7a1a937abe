#!/usr/bin/env python3
"""Writes tests/golden/body_parent.npz: what the closed-form wl_body entry points computed BEFORE they became one-leaf programs.

Run once on the MI355X against a library built from the commit that still has both kernel families:

    WLHIP_LIB=/path/to/parent/libwlhip.so python tests/golden/make_body_parent.py <parent commit id>

Per case the fixture holds wl_measure_body's σ, μ₀, μ₁, V (arrays NaN-poisoned first, as tests/test_gpu_bodyset.py::_poison does) and the
four Float64 read-outs — pressure and viscous force, pressure and viscous moment about the off-lattice X0 — on the integer-formula p and u
below (exact in float32: no RNG, nothing stored).  `cases` is the case list as JSON, `parent` the commit id.  An array that repeats an earlier
one bit for bit (the translating sphere's σ, μ₀, μ₁ are the resting sphere's) is stored as the earlier key's name; load() resolves that.  Nothing is
read from the reference."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SPHERE = ["sphere", [7.3, 8.6, 6.9], 4.0]
CASES = [      # name, N, body (make_body's tuple form), ϵ
    ["sphere3", [16, 16, 16], SPHERE, 1.0],
    ["sphere3_eps2", [16, 16, 16], SPHERE, 2.0],
    ["cylinder3", [16, 16, 16], ["cylinder", [0.0, 8.4, 7.7], 3.5, 0], 1.0],
    ["plane3", [16, 16, 16], ["plane", [8.0, 5.0, 0.0], [0.3, 1.0, -0.5]], 1.0],
    ["sphere3_moving", [16, 16, 16], SPHERE + [[0.25, -0.125, 0.0]], 1.0],
    ["circle2", [24, 24], ["sphere", [11.3, 13.6], 4.0], 1.0],
    ["plane2", [24, 24], ["plane", [16.0, 8.0], [0.3, 1.0]], 1.0],
]
X0 = [7.3, 8.7, 6.1]
NU = 0.02


def pack(out):
    """replace every array that equals an earlier one of the same shape and dtype, bit for bit, by that one's key"""
    seen, packed = {}, {}
    for k, v in out.items():
        v = np.asarray(v)
        sig = (v.shape, v.dtype.str, v.tobytes())
        packed[k] = np.array("=" + seen[sig]) if v.ndim and sig in seen else v
        if v.ndim:
            seen.setdefault(sig, k)
    return packed


def load(path):
    z = np.load(path)
    out = {k: z[k] for k in z.files}
    return {k: (out[str(v)[1:]] if v.dtype.kind == "U" and str(v).startswith("=") else v) for k, v in out.items()}


def body_tuple(spec):
    return tuple(tuple(v) if isinstance(v, list) else v for v in spec)


def int_field(shape, c):
    """((7i + 13j + 29k + 5c) mod 17 − 8) / 4 on the 0-based array indices (ghost cells included)"""
    idx = np.indices(shape)
    s = 5 * c + sum(w * ix for w, ix in zip((7, 13, 29), idx))
    return ((s % 17 - 8) / 4).astype(np.float32)


def fill_pu(w, f):
    D = f.D
    f.p.copy_(w.to_device(int_field(tuple(f.p.shape), 0)))
    f.u.copy_(w.to_device(np.stack([int_field(tuple(f.p.shape), c + 1) for c in range(D)], -1)))


def poison(f):
    for k in ("sigma", "mu0", "mu1", "V"):
        getattr(f, k).fill_(float("nan"))
    f.sigma.fill_(0.0)


if __name__ == "__main__":
    import waterlily_jl_amd as w
    w.core.device()
    out = {"cases": np.array(json.dumps(CASES)), "parent": np.array(sys.argv[1] if len(sys.argv) > 1 else "unknown")}
    for name, N, spec, eps in CASES:
        D = len(N)
        body = body_tuple(spec)
        f = w.Flow(tuple(N), (1.0,) + (0.0,) * (D - 1), nu=NU)
        poison(f)
        w.measure_(f, body, eps)
        for k in ("sigma", "mu0", "mu1", "V"):
            out[f"{name}/{k}"] = w.to_host(getattr(f, k))
        fill_pu(w, f)
        x0 = X0[:D]
        out[f"{name}/pforce"] = w.pressure_force(f, body)
        out[f"{name}/vforce"] = w.viscous_force(f, body)
        out[f"{name}/pmoment"] = w.pressure_moment(x0, f, body)
        out[f"{name}/vmoment"] = w.viscous_moment(x0, f, body)
        print(name, out[f"{name}/pforce"], out[f"{name}/vmoment"], float(np.abs(out[f"{name}/V"]).max()))
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "body_parent.npz")
    dst = os.environ.get("BODY_PARENT_OUT", dst)
    np.savez_compressed(dst, **pack(out))
    print("wrote", dst, os.path.getsize(dst), "bytes")
