"""Flow diagnostics on device arrays — ke, curl, ω, ω_mag, ω_θ, λ₂, helicity and their sums, mirror of /root/reference/src/Metrics.jl:27-109
(whole-field forms of the reference's per-index functions: `@inside σ[I] = f(I,u)`); MeanFlow — temporal averages of pressure, velocity
and u⊗u on device, mirror of src/Metrics.jl:200-255; and a plain checkpoint of (u, p, Δt) (the reference's JLD2 extension,
ext/WaterLilyJLD2Ext.jl, stores the same three)."""
import ctypes as C

import numpy as np

from ._lib import check, lib
from .core import jl_zeros, ptr, sgrid, stream, to_device, to_host, vgrid


def _f3(v, D=3):
    """host float[3] of a tuple (None stays NULL)"""
    return None if v is None else (C.c_float * 3)(*([float(x) for x in v] + [0.0] * (3 - len(v))))


def ke_(out, u, U=None):
    """@inside out[I] = ke(I,u,U)   src/Metrics.jl:33-35 (2-D and 3-D)"""
    g = vgrid(u)
    check(lib().wl_ke(ptr(out), ptr(u), C.byref(g), _f3(U), stream()))
    return out


def curl_(out, u, i):
    """@inside out[I] = curl(i,I,u)   :68 — component i (1-based, as in the reference) at the cell EDGE; 2-D: i = 3"""
    g = vgrid(u)
    check(lib().wl_curl(ptr(out), ptr(u), C.byref(g), int(i), stream()))
    return out


def omega_(out3, u):
    """@inside out3[I,:] = ω(I,u)   :74 — out3 is a vector array (Ng...,3)"""
    g = vgrid(u)
    check(lib().wl_omega(ptr(out3), ptr(u), C.byref(g), stream()))
    return out3


def omega_mag_(out, u):
    """@inside out[I] = ω_mag(I,u)   :80"""
    g = vgrid(u)
    check(lib().wl_omega_mag(ptr(out), ptr(u), C.byref(g), stream()))
    return out


def omega_theta_(out, u, z, center):
    """@inside out[I] = ω_θ(I,z,center,u)   :87-91"""
    g = vgrid(u)
    check(lib().wl_omega_theta(ptr(out), ptr(u), C.byref(g), _f3(z), _f3(center), stream()))
    return out


def lambda2_(out, u):
    """@inside out[I] = λ₂(I,u)   :54-58"""
    g = vgrid(u)
    check(lib().wl_lambda2(ptr(out), ptr(u), C.byref(g), stream()))
    return out


def helicity_(out, u, omega):
    """@inside out[I] = helicity(I,u,ω)   :99-109 — ω a collocated (Ng...,3) device array"""
    g = vgrid(u)
    check(lib().wl_helicity(ptr(out), ptr(u), ptr(omega), C.byref(g), stream()))
    return out


def flow_fields_(u, ke=None, omega=None, omega_mag=None, lambda2=None, U=None):
    """any of ke, ω, ω_mag, λ₂ in ONE pass over u (each the same bits as its own leaf); outputs that are None are skipped"""
    g = vgrid(u)
    check(lib().wl_flow_fields(ptr(u), C.byref(g), _f3(U), ptr(ke), ptr(omega), ptr(omega_mag), ptr(lambda2), stream()))


def flow_stats(u, U=None):
    """(Σ_inside ke(I,u,U), Σ_inside ½|ω|², max_inside |ω|) — kinetic energy, enstrophy and peak vorticity without a field leaving the
    device; 2-D: ω is curl(3,I,u).  Float64 sums of the per-cell Float32 values."""
    g = vgrid(u)
    out = (C.c_double * 3)()
    check(lib().wl_flow_stats(ptr(u), C.byref(g), _f3(U), out, None, stream()))
    return out[0], out[1], out[2]


class MeanFlow:
    """MeanFlow(flow; t_init=time(flow), uu_stats=false)   src/Metrics.jl:205-226"""

    def __init__(self, flow, t_init=None, uu_stats=False):
        D = flow.D
        self.D = D
        self.P = jl_zeros(tuple(flow.p.shape))
        self.U = jl_zeros(tuple(flow.u.shape))
        self.UU = jl_zeros(tuple(flow.p.shape) + (D, D)) if uu_stats else None
        self.t = [np.float32(flow.time() if t_init is None else t_init)]
        self.uu_stats = bool(uu_stats)

    def time(self):
        """time(meanflow) = t[end] - t[1]   :228"""
        return np.float32(self.t[-1] - self.t[0])

    def reset_(self, t_init=0.0):
        """reset!(meanflow; t_init)   :230-235"""
        for a in (self.P, self.U) + ((self.UU,) if self.UU is not None else ()):
            a.zero_()
        self.t = [np.float32(t_init)]

    def update_(self, flow):
        """update!(meanflow, flow)   :236-248"""
        dt = np.float32(flow.time() - self.t[-1])
        eps = np.float32(dt / np.float32(dt + self.time() + np.finfo(np.float32).eps))
        if len(self.t) == 1:
            eps = np.float32(1)          # the first update takes the instantaneous field
        g = sgrid(flow.p)
        check(lib().wl_meanflow_update(ptr(self.P), ptr(self.U), ptr(self.UU) if self.UU is not None else None, ptr(flow.p), ptr(flow.u),
                                       C.byref(g), float(eps), stream()))
        self.t.append(np.float32(self.t[-1] + dt))

    def uu(self):
        """uu(a): Reynolds stresses τ = UU - U⊗U   :250-258"""
        assert self.UU is not None
        tau = jl_zeros(tuple(self.UU.shape))
        g = sgrid(self.P)
        check(lib().wl_meanflow_uu(ptr(tau), ptr(self.UU), ptr(self.U), C.byref(g), stream()))
        return tau


def save_checkpoint(path, flow):
    """u, p and the Δt history of a Flow (what ext/WaterLilyJLD2Ext.jl's save! writes), as an .npz"""
    np.savez(path, u=to_host(flow.u), p=to_host(flow.p), dt=np.asarray(flow.dt, dtype=np.float32))


def load_checkpoint(path, flow):
    """load!(flow): restore u, p, Δt (allow_pickle stays off)"""
    with np.load(path) as z:
        assert tuple(z["u"].shape) == tuple(flow.u.shape) and tuple(z["p"].shape) == tuple(flow.p.shape)
        flow.u.copy_(to_device(np.asfortranarray(z["u"])))
        flow.p.copy_(to_device(np.asfortranarray(z["p"])))
        flow.dt[:] = [np.float32(v) for v in z["dt"]]
