"""interp at points, and one step of a tracer swarm, on device arrays — mirror of /root/reference/src/util.jl:17-43 (`interp.(x, Ref(arr))`)
and of the particle update the reference's pathline extension drives (ext/WaterLilyPathlinesExt.jl).  Points are device arrays of shape
(n, D), row-major: point-major like a Julia Vector{SVector{D,Float32}}."""
import ctypes as C

import numpy as np
import torch

from ._lib import check, lib
from .core import device, grid_of, perdir_mask, ptr, stream


def points(x, D=None):
    """an (n, D) set of points as a dense row-major float32 device tensor (host arrays are copied over)"""
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32))).to(device())
    assert x.dtype == torch.float32 and x.is_cuda and x.dim() == 2 and x.is_contiguous(), "points: a dense (n, D) float32 device array"
    assert D is None or x.shape[1] == D, f"points have {x.shape[1]} coordinates, the array has {D} dimensions"
    return x


def _pp(t):
    return C.c_void_p(t.data_ptr()) if t.numel() else None


def interp_(out, arr, x):
    """out .= interp.(x, Ref(arr))   src/util.jl:20-43.  arr: a scalar array (Ng...) -> out (n,), or the staggered vector array (Ng...,D) ->
    out (n, D); x: (n, D) points.  Queries are clamped to the array (:17-18)."""
    D = x.shape[1]
    x = points(x, D)
    n = x.shape[0]
    vec = arr.dim() == D + 1
    assert arr.dim() in (D, D + 1), "arr: a scalar array (Ng...) or a vector array (Ng...,D)"
    ncomp = int(arr.shape[-1]) if vec else 1
    assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == ((n, ncomp) if vec else (n,))
    g = grid_of(tuple(arr.shape[:D]))
    check(lib().wl_interp(_pp(out), ptr(arr), C.byref(g), _pp(x), n, ncomp, stream()))
    return out


def interp(arr, x):
    """interp.(x, Ref(arr)) into a new device array"""
    x = points(x)
    vec = arr.dim() == x.shape[1] + 1
    out = torch.empty((x.shape[0], int(arr.shape[-1])) if vec else (x.shape[0],), dtype=torch.float32, device=x.device)
    return interp_(out, arr, x)


def advect_(x, x_prev, u0, u1, dt, perdir=()):
    """x⁰ ← x;  x* = x⁰ + Δt·u⁰(x⁰);  x ← x⁰ + ½Δt·(u⁰(x⁰) + u¹(x*)) for the (n, D) device positions x (x_prev receives x⁰); coordinates of a
    periodic direction are wrapped into [0, N)"""
    D = u0.dim() - 1
    x, x_prev = points(x, D), points(x_prev, D)
    assert x.shape == x_prev.shape and tuple(u0.shape) == tuple(u1.shape)
    g = grid_of(tuple(u0.shape[:D]))
    check(lib().wl_advect(_pp(x), _pp(x_prev), ptr(u0), ptr(u1), C.byref(g), x.shape[0], float(dt), perdir_mask(perdir), stream()))
    return x
