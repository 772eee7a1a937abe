"""Simulation — host-side mirror of /root/reference/src/WaterLily.jl:86-149, plus the fused composite
handle (`wl_sim`) that bench.py times."""
import ctypes as C

import numpy as np

from . import core
from ._lib import WlError, check, lib, wl_grid, wl_sim_desc
from .core import perdir_mask, ptr, stream
from .flow import Flow, mom_step_
from .poisson import MultiLevelPoisson


def _is_set(body):
    from .bodies import AbstractBody
    return isinstance(body, AbstractBody)


def _x0(x0, D):
    return None if x0 is None else (C.c_float * 3)(*([float(v) for v in x0] + [0.0] * (3 - D)))


def _as_set(body):
    """a composite body as it is; a closed-form tuple — ("sphere", c, R), ("cylinder", c, R, axis), ("plane", point, normal), ("capsule", …) — as its leaf"""
    from .bodies import Body
    if _is_set(body):
        return body
    if isinstance(body, (tuple, list)) and body and isinstance(body[0], str):
        return Body(tuple(body))
    raise TypeError(f"a body of bodies.py or a closed-form tuple is expected, not {type(body).__name__}")


def _x0_checked(x0, D):
    if x0 is None:
        return None
    x0 = [float(v) for v in x0]
    if len(x0) != D:
        raise ValueError(f"x0 has {len(x0)} components, the flow has {D}")
    return _x0(x0, D)


def _split_forces(rec, D):
    """[k,12] records -> pF[k,D], vF[k,D], pM[k,·], vM[k,·] (the moment is a scalar in 2-D: one column)"""
    M = 3 if D == 3 else 1
    return rec[:, 0:D].copy(), rec[:, 3:3 + D].copy(), rec[:, 6:6 + M].copy(), rec[:, 9:9 + M].copy()


def _bodyset_force(which, a, body, x0=None):
    """pressure (which 0) / viscous (1) force, or the moment about x0, of a composite body (bodies.py) on a Flow"""
    from .core import sgrid
    prog = body.program(a.D)
    g = sgrid(a.p)
    out = (C.c_double * 3)()
    if which == 0:
        check(lib().wl_pressure_force_bodyset(_x0(x0, a.D), ptr(a.p), C.byref(g), C.byref(prog), out, stream()))
    else:
        check(lib().wl_viscous_force_bodyset(_x0(x0, a.D), ptr(a.u), C.byref(g), float(a.nu), C.byref(prog), out, stream()))
    return np.array(out[: a.D])


def measure_(a, body, eps=1.0):
    """measure!(a::Flow, body; ϵ) for a closed-form AutoBody, or a composite body of bodies.py (RigidMap leaves, set operations)
    src/Body.jl:28-51"""
    if _is_set(body):
        from .core import ptr, sgrid, perdir_mask
        prog = body.program(a.D)
        g = sgrid(a.sigma)
        check(lib().wl_measure_bodyset(ptr(a.sigma), ptr(a.mu0), ptr(a.mu1), ptr(a.V), C.byref(g), C.byref(prog), float(eps), int(a.exitBC),
                                       perdir_mask(a.perdir), stream()))
        a.has_body = True
        return
    from ._lib import make_body
    from .core import ptr, sgrid, perdir_mask
    b = make_body(body, a.D)
    g = sgrid(a.sigma)
    check(lib().wl_measure_body(ptr(a.sigma), ptr(a.mu0), ptr(a.mu1), ptr(a.V), C.byref(g), C.byref(b), float(eps), int(a.exitBC), perdir_mask(a.perdir), stream()))
    a.has_body = True


def pressure_force(a, body):
    """pressure_force(p,df,body)   src/Metrics.jl:116-133 (Float64 sums; flow.f is not used as scratch)"""
    if _is_set(body):
        return _bodyset_force(0, a, body)
    from ._lib import make_body
    from .core import ptr, sgrid
    b = make_body(body, a.D)
    g = sgrid(a.p)
    out = (C.c_double * 3)()
    check(lib().wl_pressure_force_body(ptr(a.p), C.byref(g), C.byref(b), out, stream()))
    return np.array(out[: a.D])


def viscous_force(a, body):
    """viscous_force(u,ν,df,body)   src/Metrics.jl:140-154"""
    if _is_set(body):
        return _bodyset_force(1, a, body)
    from ._lib import make_body
    from .core import ptr, sgrid
    b = make_body(body, a.D)
    g = sgrid(a.p)
    out = (C.c_double * 3)()
    check(lib().wl_viscous_force_body(ptr(a.u), C.byref(g), float(a.nu), C.byref(b), out, stream()))
    return np.array(out[: a.D])


def pressure_moment(x0, a, body):
    """pressure_moment(x₀,flow,body)   src/Metrics.jl:168-174"""
    if _is_set(body):
        return _bodyset_force(0, a, body, x0)
    from ._lib import make_body
    from .core import ptr, sgrid
    b = make_body(body, a.D)
    g = sgrid(a.p)
    out = (C.c_double * 3)()
    xx = (C.c_float * 3)(*([float(v) for v in x0] + [0.0] * (3 - a.D)))
    check(lib().wl_pressure_moment_body(xx, ptr(a.p), C.byref(g), C.byref(b), out, stream()))
    return np.array(out[: a.D])


def viscous_moment(x0, a, body):
    """viscous_moment(x₀,flow,body)   src/Metrics.jl:182-188"""
    if _is_set(body):
        return _bodyset_force(1, a, body, x0)
    from ._lib import make_body
    from .core import ptr, sgrid
    b = make_body(body, a.D)
    g = sgrid(a.p)
    out = (C.c_double * 3)()
    xx = (C.c_float * 3)(*([float(v) for v in x0] + [0.0] * (3 - a.D)))
    check(lib().wl_viscous_moment_body(xx, ptr(a.u), C.byref(g), float(a.nu), C.byref(b), out, stream()))
    return np.array(out[: a.D])


METRICS = ("ke", "curl", "omega", "omega_mag", "omega_theta", "lambda2")


def _metric_leaf(u, sigma, name, out, **kw):
    """one diagnostic field of the device velocity array `u` through the leaf functions of metrics.py"""
    from . import metrics as m
    from .core import jl_zeros
    if name not in METRICS:
        raise ValueError(f"unknown metric {name!r}: one of {METRICS}")
    Ng = tuple(u.shape[:-1])
    if isinstance(out, str):
        assert out == "sigma" and name != "omega", "out='sigma' names the scalar scratch array flow.σ"
        out = sigma
    if out is None:
        out = jl_zeros(Ng + (3,) if name == "omega" else Ng)
    if name == "ke":
        return m.ke_(out, u, kw.get("U"))
    if name == "curl":
        return m.curl_(out, u, kw.get("i", 3))
    if name == "omega_theta":
        return m.omega_theta_(out, u, kw["z"], kw["center"])
    return {"omega": m.omega_, "omega_mag": m.omega_mag_, "lambda2": m.lambda2_}[name](out, u)


class Simulation:
    """Simulation(dims,uBC,L;U,Δt,ν,ϵ,perdir,exitBC,λ,body,T) over leaf operations (reference orchestration)."""

    def __init__(self, dims, uBC, L, U=None, dt=0.25, nu=0.0, eps=1, perdir=(), u0=None, exitBC=False, lam=core.QUICK,
                 body=None, T=np.float32, g=None, duBC_dt=None):
        if U is None:
            assert not callable(uBC), "`U` (velocity scale) must be specified if boundary conditions `uBC` is a `Function`"   # :99
            U = float(np.sqrt(sum(float(v) ** 2 for v in uBC)))                  # :100
        self.U, self.L, self.eps = float(U), float(L), eps
        self.flow = Flow(dims, uBC, dt=dt, nu=nu, g=g, u0=u0, perdir=perdir, exitBC=exitBC, lam=lam, T=T, duBC_dt=duBC_dt)   # :103
        self.body = body          # None (NoBody), a closed-form AutoBody: ("sphere", c, R) | ("cylinder", c, R, axis) | ("plane", point, normal) [+ velocity],
                                  # or a composite body of bodies.py (Body leaves under RigidMaps, set operations); setmap + remeasure moves it
        if body is not None:
            measure_(self.flow, body, eps=self.eps)                                                 # :104
        self.pois = MultiLevelPoisson(self.flow.p, self.flow.mu0, self.flow.sigma, perdir=perdir)   # :97,105

    def sim_time(self):
        return float(self.flow.time()) * self.U / self.L                          # :117

    def sim_step_(self, t_end=None, remeasure=True, max_steps=2**31 - 1, udf=None, **kw):
        """sim_step!(sim[,t_end];remeasure,max_steps,udf,kwargs...)   :128-139 — `udf` and its keywords go to mom_step! (eg. udf=sgs, Cs=0.17, Delta=1)"""
        if t_end is None:
            if remeasure:
                self.measure_()
            mom_step_(self.flow, self.pois, udf=udf, **kw)
            return
        steps0 = len(self.flow.dt)
        while self.sim_time() < t_end and len(self.flow.dt) - steps0 < max_steps:
            self.sim_step_(remeasure=remeasure, udf=udf, **kw)

    def measure_(self, body=None):
        """measure!(sim): measure!(flow,body) + update!(pois)   :146-149 (quirk Q3: runs every step when remeasure=true; NoBody => only
        update!).  `body`: the body's new description (position, velocity) — the stand-in for the reference's map(x,t)."""
        if body is not None:
            self.body = body
        if self.body is not None:
            measure_(self.flow, self.body, eps=self.eps)
        self.pois.update_()

    def flow_stats(self, U=None):
        """(Σke, Σ½|ω|², max|ω|) of flow.u over inside   src/Metrics.jl:33-35,74,80"""
        from .metrics import flow_stats
        return flow_stats(self.flow.u, U)

    def metric(self, name, out=None, **kw):
        """`@inside out[I] = <name>(I,flow.u)` — see FusedSimulation.metric; out="sigma" writes into flow.σ"""
        return _metric_leaf(self.flow.u, self.flow.sigma, name, out, **kw)

    def sample(self, points):
        """(interp.(x, Ref(flow.u)), interp.(x, Ref(flow.p))) at the (n, D) points x   src/util.jl:20-43"""
        from .interp import interp, points as _points
        x = _points(points, self.flow.D)
        return interp(self.flow.u, x), interp(self.flow.p, x)

    def pressure_force(self):
        return pressure_force(self.flow, self.body)

    def viscous_force(self):
        return viscous_force(self.flow, self.body)

    def total_force(self):
        """total_force(sim) = pressure_force + viscous_force   src/Metrics.jl:156-161"""
        return self.pressure_force() + self.viscous_force()

    def pressure_moment(self, x0):
        return pressure_moment(x0, self.flow, self.body)

    def viscous_moment(self, x0):
        return viscous_moment(x0, self.flow, self.body)

    def total_moment(self, x0):
        """total_moment(x₀,sim)   src/Metrics.jl:195"""
        return self.pressure_moment(x0) + self.viscous_moment(x0)


class FusedSimulation:
    """The composite path: one `wl_sim` handle holds every field in HBM and runs mom_step! (src/Flow.jl:156-167)
    as a fixed sequence of fused HIP kernels on one stream.  This is what bench.py times."""

    def __init__(self, dims, uBC, L, U=None, dt=0.25, nu=0.0, perdir=(), exitBC=False, lam=core.QUICK, has_body=False, ic="uBC", u0=None,
                 g=None, duBC_dt=None, terms=None, g_t=None, b_t=None, db_t=None):
        """uBC: tuple, or a function uBC(i,t) that is uniform in space (i = 1..D as in the reference) together with its time
        derivative duBC_dt(i,t) (the reference differentiates it with ForwardDiff, src/Flow.jl:72-73); g: body force g(i,t),
        uniform in space.

        Position-dependent uBC(i,x,t) and g(i,x,t) in separable form (include/wlhip.h, separable terms):
            uBC(i,x,t) = Σₖ b_t(t)[k]·terms[k][I,i]      g(i,x,t) = Σₖ g_t(t)[k]·terms[k][I,i]      K = len(terms) ≤ 4
        terms: K arrays of shape Ng + (D,) holding the spatial factors at loc(i,I) (core.tabulate(fn, dims) makes one); g_t, b_t and db_t (the time
        derivative of b_t: accelerate! adds g + ∂ₜuBC) are each None, K constants, or a callable t -> K floats.  With b_t given every BC!(u) takes its
        values from the terms, and with u0=None the initial field is Σₖ b_t(0)[k]·terms[k] (the reference's u0 = uBC at t = 0).  `uBC` is then only the
        tuple the handle is created with and `U` the velocity scale."""
        core.device()
        D = len(dims)
        self._ufn = uBC if callable(uBC) else None
        self._dufn, self._gfn = duBC_dt, g
        if self._ufn is not None:
            assert U is not None, "`U` (velocity scale) must be specified if boundary conditions `uBC` is a `Function`"   # src/WaterLily.jl:99
            uBC = tuple(float(self._ufn(i + 1, 0.0)) for i in range(D))
        if U is None:
            U = float(np.sqrt(sum(float(v) ** 2 for v in uBC)))
        self.U, self.L, self.D = float(U), float(L), D
        self.dims = tuple(int(n) for n in dims)
        self.Ng = tuple(n + 2 for n in self.dims)
        d = wl_sim_desc()
        d.D = D
        for k in range(3):
            d.dims[k] = self.dims[k] if k < D else 1
            d.uBC[k] = float(uBC[k]) if k < D else 0.0
        d.nu, d.dt0 = float(nu), float(dt)
        d.perdir_mask, d.exitBC, d.scheme, d.has_body = perdir_mask(perdir), int(bool(exitBC)), int(lam), int(bool(has_body))
        h = C.c_void_p()
        check(lib().wl_sim_create(C.byref(h), C.byref(d)))
        self._h = h
        self.nu = float(nu)
        self.has_body = bool(has_body)
        self._tK, self._tcoef, self._tdyn = 0, (None, None, None), False
        if terms is not None:
            self.set_terms(terms, g_t=g_t, b_t=b_t, db_t=db_t)
        else:
            assert g_t is None and b_t is None and db_t is None, "g_t, b_t and db_t are the coefficients of `terms`"
        if u0 is None and ic == "uBC" and self._tcoef[1] is not None:      # u0 = uBC(i,x,0)   src/WaterLily.jl:100
            u0 = self._combine(self._terms_host, self._coef(self._tcoef[1], 0.0))
        self._terms_host = None      # (the handle owns the device copies; the host arrays were needed for the initial field only)
        if u0 is not None:
            self.set_field("u", np.asfortranarray(u0, dtype=np.float32))
        else:
            check(lib().wl_sim_apply_ic(h, {"uBC": 0, "tgv": 1, "tgv_periodic": 2}[ic], stream()))
        check(lib().wl_sim_init_flow(h, stream()))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                lib().wl_sim_destroy(h)
            except Exception:
                pass
            self._h = None

    def _shape(self, name):
        D = self.D
        return {"p": self.Ng, "sigma": self.Ng, "mu1": self.Ng + (D, D)}.get(name, self.Ng + (D,))

    def field(self, name):
        """`Array(flow.<name>)`"""
        out = np.empty(self._shape(name), dtype=np.float32, order="F")
        p = lib().wl_sim_field(self._h, name.encode())
        if not p:
            raise KeyError(name)
        check(lib().wl_d2h(out.ctypes.data_as(C.c_void_p), p, out.nbytes, stream()))
        return out

    def set_field(self, name, a):
        a = np.asfortranarray(a, dtype=np.float32)
        assert a.shape == self._shape(name)
        check(lib().wl_h2d(lib().wl_sim_field(self._h, name.encode()), a.ctypes.data_as(C.c_void_p), a.nbytes, stream()))
        check(lib().wl_stream_sync(stream()))

    @staticmethod
    def _combine(F, c):
        """Σₖ c[k]·F[k] in Float32 in the order of the device kernels: s = c₀·F₀ ; s = s + cₖ·Fₖ"""
        s = np.float32(c[0]) * F[0]
        for k in range(1, len(F)):
            s = s + np.float32(c[k]) * F[k]
        return np.asfortranarray(s, dtype=np.float32)

    def _coef(self, c, t):
        """K coefficients at time t: constants, or a callable t -> K floats"""
        v = c(float(t)) if callable(c) else c
        v = [float(x) for x in v]
        if len(v) != self._tK:
            raise ValueError(f"{len(v)} coefficients for {self._tK} terms")
        return v

    def set_terms(self, terms, g_t=None, b_t=None, db_t=None):
        """register (or, with terms=None, remove) the separable terms and their coefficients — see __init__.  Constant coefficients are handed to the
        handle once and stay in force; callables are evaluated by the host before every step."""
        K = 0 if terms is None else len(terms)
        host = [np.asfortranarray(f, dtype=np.float32) for f in (terms or [])]
        for f in host:
            if f.shape != self.Ng + (self.D,):
                raise ValueError(f"a term has shape {f.shape}, the flow's velocity has {self.Ng + (self.D,)}")
        Fp = (C.c_void_p * max(K, 1))(*[f.ctypes.data_as(C.c_void_p) for f in host])
        check(lib().wl_sim_set_terms(self._h, K, Fp, stream()))
        self._tK, self._terms_host = K, host
        self._tcoef = (g_t, b_t, db_t)
        self._tdyn = any(callable(c) for c in self._tcoef)
        if K == 0:
            if any(c is not None for c in self._tcoef):
                raise ValueError("coefficients without terms")
            return
        self._term_coeffs(0.0, 0.0)      # in force for init_flow; the constant ones for good

    def term(self, k):
        """term k as a device array over the handle's memory (for callers that fill it on the device)"""
        import torch
        p = lib().wl_sim_term(self._h, int(k))
        if not p:
            raise KeyError(k)
        shape = self.Ng + (self.D,)
        n, addr = int(np.prod(shape)), int(p)

        class _Mem:      # __cuda_array_interface__ of memory the handle owns
            __cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (addr, False), "version": 2}
        t = torch.as_tensor(_Mem(), device=core.device())
        return t.view(tuple(reversed(shape))).permute(*reversed(range(len(shape))))

    def _term_coeffs(self, t0, t1):
        """aₖ(t₀), aₖ(t₁) = gₖ + bₖ′ and bₖ(t₁) into the handle (wl_sim_set_term_coeffs)"""
        g_t, b_t, db_t = self._tcoef
        K = self._tK
        arr = lambda v: (C.c_float * K)(*v)      # noqa: E731
        acc = None
        if g_t is not None or (b_t is not None and db_t is not None):
            def acc(t):
                gv = self._coef(g_t, t) if g_t is not None else [0.0] * K
                dv = self._coef(db_t, t) if (b_t is not None and db_t is not None) else [0.0] * K
                return arr([a + b for a, b in zip(gv, dv)])
        check(lib().wl_sim_set_term_coeffs(self._h, acc(t0) if acc else None, acc(t1) if acc else None,
                                           arr(self._coef(b_t, t1)) if b_t is not None else None))

    def _forcing(self):
        """uBC(i,t₁) and g(i,t)+dU(i,t)/dt at t₀, t₁ for the coming step (mom_step!, src/Flow.jl:157; accelerate! :69-73)"""
        if self._ufn is None and self._gfn is None and not self._tdyn:
            return
        D = self.D
        dtl = np.float32(lib().wl_sim_dt_last(self._h))
        t1 = np.float32(np.float32(lib().wl_sim_time(self._h)) + dtl)      # t₁ = sum(Δt) ; t₀ = t₁ - Δt[end]   src/Flow.jl:157
        t0 = np.float32(t1 - dtl)
        if self._tdyn:
            self._term_coeffs(t0, t1)
        if self._ufn is None and self._gfn is None:
            return
        arr = lambda v: (C.c_float * 3)(*([float(x) for x in v] + [0.0] * (3 - D)))
        U1 = arr([self._ufn(i + 1, float(t1)) for i in range(D)]) if self._ufn is not None else None
        acc = lambda t: arr([(self._gfn(i + 1, float(t)) if self._gfn else 0.0) + (self._dufn(i + 1, float(t)) if (self._ufn and self._dufn) else 0.0) for i in range(D)])
        check(lib().wl_sim_set_forcing(self._h, U1, acc(t0), acc(t1)))

    def mom_step_(self):
        self._forcing()
        check(lib().wl_sim_mom_step(self._h, stream()))

    def mom_steps_(self, n):
        """n × mom_step! in one library call (no time-dependent uBC / g between the steps: those are evaluated by the host per step — use mom_step_)"""
        if self._ufn is not None or self._gfn is not None or self._tdyn:
            for _ in range(int(n)):
                self.mom_step_()
            return
        check(lib().wl_sim_mom_steps(self._h, int(n), stream()))

    def set_sgs(self, Cs, Delta=1.0):
        """the built-in Smagorinsky–Lilly model as the step's udf (sim_step!(sim; udf=sgs!, νₜ=smagorinsky, S, Cs, Δ), src/util.jl:45-76):
        set_sgs(0.17, 1.0) switches it on for every following step, set_sgs(None) off (the default).  3-D single-domain flows."""
        if Cs is None:
            check(lib().wl_sim_set_sgs(self._h, 0, 0.0, 1.0))
        else:
            check(lib().wl_sim_set_sgs(self._h, 1, float(Cs), float(Delta)))

    def phase_(self, k):
        check(lib().wl_sim_phase(self._h, int(k), stream()))

    def set_body(self, body, eps=1.0):
        """store a composite body (bodies.py) and measure it on the device (measure!(sim), src/WaterLily.jl:146-149); afterwards
        sim_step_(remeasure=True) remeasures the stored body — replace it with set_body(setmap(...)) or by assigning `.body`"""
        assert self.has_body, "FusedSimulation was created with has_body=False"
        self.body, self.eps = body, float(eps)
        self.measure_bodyset_(body, eps)

    def measure_bodyset_(self, body, eps=1.0):
        """measure!(sim) for a composite body on the device + update!(pois)"""
        prog = body.program(self.D)
        check(lib().wl_sim_measure_bodyset(self._h, C.byref(prog), float(eps), stream()))

    def sim_step_(self, t_end=None, remeasure=False, max_steps=2**31 - 1):
        if t_end is None:
            if remeasure:
                if getattr(self, "body", None) is not None:
                    self.measure_bodyset_(self.body, self.eps)      # at t = sum(Δt): the stored body's current map
                else:
                    check(lib().wl_sim_update(self._h, stream()))
            self.mom_step_()
            return
        n = 0
        while self.sim_time() < t_end and n < max_steps:
            self.sim_step_(remeasure=remeasure)
            n += 1

    def update_(self):
        check(lib().wl_sim_update(self._h, stream()))

    def set_option(self, name, value):
        """implementation switches: "convz", "fused_smoother" (1 = default fast path, 0 = one kernel per pass)"""
        check(lib().wl_sim_set_option(self._h, name.encode(), int(value)))

    def counter(self, name):
        """path counters of the handle (include/wlhip_bench.h wl_sim_counter): "resjac", "resjac_redo", "resjac_backoff", "xdefer", "abwide", "tailfuse", "bcdefer", "pdefer", "tailwide", "rskip", "rskip_redo", "tailspec", "tailspec_armed", "launches", "probe_records", "probe_dropped", "force_records", "force_dropped", "force_tiles", "mean_updates", "mean_every", "term_accel", "term_bc"; "tailfuse_min" reads the size gate of "tailfuse" in force;
        with a body: "hybrid", "body_tile", "mask_valid", "part", "part_za", "part_zb" and the mask census "mask_near", "mask_needf_only", "mask_m0var_only",
        "mask_clean_in_box", "dirty_z0", "dirty_z1", "near_b0", "near_b1", "near_k0", "near_k1" """
        v = C.c_long(0)
        check(lib().wl_sim_counter(self._h, name.encode(), C.byref(v)))
        return int(v.value)

    @property
    def dt(self):
        out = (C.c_float * 1000000)()
        k = lib().wl_sim_dt(self._h, out, 1000000)
        return [np.float32(v) for v in out[:k]]

    def time(self):
        return lib().wl_sim_time(self._h)

    def sim_time(self):
        return self.time() * self.U / self.L

    @property
    def pois_n(self):
        mg = lib().wl_sim_pois(self._h)
        out = (C.c_int16 * 65536)()
        k = lib().wl_mg_history(mg, out, 65536)
        return [int(v) for v in out[:k]]

    def pois_level(self, name, l=0):
        mg = lib().wl_sim_pois(self._h)
        g = wl_grid()
        check(lib().wl_mg_level_grid(mg, l, C.byref(g)))
        dims = (g.nx, g.ny) if g.D == 2 else (g.nx, g.ny, g.nz)
        shape = dims + (g.D,) if name == "L" else dims
        out = np.empty(shape, dtype=np.float32, order="F")
        check(lib().wl_d2h(out.ctypes.data_as(C.c_void_p), lib().wl_mg_level_field(mg, l, name.encode()), out.nbytes, stream()))
        return out

    def nlevels(self):
        return lib().wl_mg_nlevels(lib().wl_sim_pois(self._h))

    def const_levels(self):
        """per level: was L verified to be 'constant inside, zero on wall faces' (constant-coefficient kernels in use)"""
        mg = lib().wl_sim_pois(self._h)
        return [bool(lib().wl_mg_level_is_const(mg, l)) for l in range(self.nlevels())]

    def smoother_kinds(self):
        """per level: 0 one kernel per pass, 1 temporally blocked smoother, 2 blocked pair kernels (constant coefficients),
        3 z-split (pair kernels on the planes away from the body, general blocked kernels around it)"""
        mg = lib().wl_sim_pois(self._h)
        return [int(lib().wl_mg_smoother_kind(mg, l)) for l in range(self.nlevels())]

    def measure_sphere_(self, center, R, eps=1.0):
        """measure!(sim) for AutoBody(|x-c|-R): closed form on device + update!(pois)"""
        c = (C.c_float * 3)(*([float(v) for v in center] + [0.0] * (3 - self.D)))
        check(lib().wl_sim_measure_sphere(self._h, c, float(R), float(eps), stream()))

    def measure_body_(self, body, eps=1.0):
        """measure!(sim) for a closed-form AutoBody — ("sphere", c, R) | ("cylinder", c, R, axis) | ("plane", point, normal), optionally
        followed by the body's translation velocity (stored in flow.V, src/AutoBody.jl:36-37) — on device + update!(pois)"""
        from ._lib import make_body
        b = make_body(body, self.D)
        check(lib().wl_sim_measure_body(self._h, C.byref(b), float(eps), stream()))

    def _bodyset_force(self, fn, body, x0=None):
        prog = body.program(self.D)
        out = (C.c_double * 3)()
        check(fn(self._h, _x0(x0, self.D), C.byref(prog), out, stream()))
        return np.array(out[: self.D])

    def pressure_force_body(self, body):
        if _is_set(body):
            return self._bodyset_force(lib().wl_sim_pressure_force_bodyset, body)
        from ._lib import make_body
        b = make_body(body, self.D)
        out = (C.c_double * 3)()
        check(lib().wl_sim_pressure_force_body(self._h, C.byref(b), out, stream()))
        return np.array(out[: self.D])

    def viscous_force_body(self, body):
        if _is_set(body):
            return self._bodyset_force(lib().wl_sim_viscous_force_bodyset, body)
        from ._lib import make_body
        b = make_body(body, self.D)
        out = (C.c_double * 3)()
        check(lib().wl_sim_viscous_force_body(self._h, C.byref(b), out, stream()))
        return np.array(out[: self.D])

    def total_force_body(self, body):
        return self.pressure_force_body(body) + self.viscous_force_body(body)

    def _moment(self, fn, x0, body):
        from ._lib import make_body
        b = make_body(body, self.D)
        out = (C.c_double * 3)()
        xx = (C.c_float * 3)(*([float(v) for v in x0] + [0.0] * (3 - self.D)))
        check(fn(self._h, xx, C.byref(b), out, stream()))
        return np.array(out[: self.D])

    def pressure_moment_body(self, x0, body):
        """pressure_moment(x₀,sim)   src/Metrics.jl:167-174"""
        if _is_set(body):
            return self._bodyset_force(lib().wl_sim_pressure_force_bodyset, body, x0)
        return self._moment(lib().wl_sim_pressure_moment_body, x0, body)

    def viscous_moment_body(self, x0, body):
        """viscous_moment(x₀,sim)   src/Metrics.jl:181-188"""
        if _is_set(body):
            return self._bodyset_force(lib().wl_sim_viscous_force_bodyset, body, x0)
        return self._moment(lib().wl_sim_viscous_moment_body, x0, body)

    def total_moment_body(self, x0, body):
        return self.pressure_moment_body(x0, body) + self.viscous_moment_body(x0, body)

    def pressure_force_sphere(self, center, R):
        c = (C.c_float * 3)(*([float(v) for v in center] + [0.0] * (3 - self.D)))
        out = (C.c_double * 3)()
        check(lib().wl_sim_pressure_force_sphere(self._h, c, float(R), out, stream()))
        return np.array(out[: self.D])

    def viscous_force_sphere(self, center, R):
        """viscous_force(sim) for the sphere/circle   src/Metrics.jl:148-154"""
        c = (C.c_float * 3)(*([float(v) for v in center] + [0.0] * (3 - self.D)))
        out = (C.c_double * 3)()
        check(lib().wl_sim_viscous_force_sphere(self._h, c, float(R), out, stream()))
        return np.array(out[: self.D])

    def total_force_sphere(self, center, R):
        """total_force(sim) = pressure_force + viscous_force   src/Metrics.jl:156-161"""
        return self.pressure_force_sphere(center, R) + self.viscous_force_sphere(center, R)

    def _view(self, name):
        """the handle's array `name` (its CURRENT role holder) as a device array — valid until the next step rotates the roles"""
        import torch
        shape = self._shape(name)
        p = lib().wl_sim_field(self._h, name.encode())
        if not p:
            raise KeyError(name)
        n = int(np.prod(shape))

        class _Mem:      # __cuda_array_interface__ of memory the handle owns
            __cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (int(p), False), "version": 2}
        t = torch.as_tensor(_Mem(), device=core.device())
        return t.view(tuple(reversed(shape))).permute(*reversed(range(len(shape))))

    def flow_stats(self, U=None):
        """(Σ_inside ke(I,u,U), Σ_inside ½|ω|², max_inside |ω|) of the current velocity: the kinetic-energy and enstrophy read-out of a
        run without u leaving the device (src/Metrics.jl:33-35,74,80; 2-D: ω = curl(3,I,u)).  Does not touch the step."""
        out = (C.c_double * 3)()
        check(lib().wl_sim_flow_stats(self._h, _x0(U, self.D), out, stream()))
        return out[0], out[1], out[2]

    def metric(self, name, out=None, **kw):
        """`@inside out[I] = <name>(I,flow.u)` on the device, name ∈ "ke" (U=…), "curl" (i=…), "omega", "omega_mag", "omega_theta" (z=…, center=…),
        "lambda2".  out: a device array, None (a new one) or "sigma" (the handle's σ, the reference's scratch).  Returns the device array."""
        if name not in METRICS:
            raise ValueError(f"unknown metric {name!r}: one of {METRICS}")
        if isinstance(out, str):
            assert out == "sigma" and name != "omega", "out='sigma' names the scalar scratch array flow.σ"
            out = self._view("sigma")
        if out is None:
            out = core.jl_zeros(self.Ng + (3,) if name == "omega" else self.Ng)
        L = lib()
        if name in ("ke", "omega", "omega_mag", "lambda2"):
            k = {"ke": 0, "omega": 1, "omega_mag": 2, "lambda2": 3}[name]
            args = [ptr(out) if q == k else None for q in range(4)]
            check(L.wl_sim_flow_fields(self._h, _x0(kw.get("U"), self.D), *args, stream()))
            return out
        g = wl_grid()
        check(L.wl_sim_grid(self._h, C.byref(g)))
        u = L.wl_sim_field(self._h, b"u")
        if name == "curl":
            check(L.wl_curl(ptr(out), u, C.byref(g), int(kw.get("i", 3)), stream()))
        else:
            check(L.wl_omega_theta(ptr(out), u, C.byref(g), _x0(kw["z"], 3), _x0(kw["center"], 3), stream()))
        return out

    def sample(self, points):
        """(u, p) = (interp.(x, Ref(flow.u)), interp.(x, Ref(flow.p))) at the (n, D) points x, as device arrays (n, D) and (n,): one launch on the
        handle's current u and p (src/util.jl:20-43) — a wake probe or a line cut without a field leaving the device"""
        import torch
        from .interp import _pp, points as _points
        x = _points(points, self.D)
        n = x.shape[0]
        u = torch.empty((n, self.D), dtype=torch.float32, device=x.device)
        p = torch.empty((n,), dtype=torch.float32, device=x.device)
        check(lib().wl_sim_sample(self._h, _pp(x), n, _pp(u), _pp(p), stream()))
        return u, p

    def set_probes(self, points, capacity):
        """record u and p at the (m, D) host points after every completed step of this handle — mom_step_ and each step inside mom_steps_ — for up to
        `capacity` steps between two read_probes(); points=None (or empty) switches recording off"""
        x = np.zeros((0, self.D), dtype=np.float32) if points is None else np.ascontiguousarray(np.asarray(points, dtype=np.float32)).reshape(-1, self.D)
        self._probe_m = int(x.shape[0])
        check(lib().wl_sim_set_probes(self._h, x.ctypes.data_as(C.POINTER(C.c_float)), self._probe_m, int(capacity)))

    def read_probes(self):
        """(t, u[k,m,D], p[k,m]) of the k records taken since the last read, oldest first; t[r] is time(flow) at the end of record r's step (the
        Float32 running sum of the Δt history, as time() forms it).  Empties the buffer."""
        m, D = getattr(self, "_probe_m", 0), self.D
        k, first = C.c_int(0), C.c_int(0)
        check(lib().wl_sim_read_probes(self._h, None, 0, C.byref(k), C.byref(first)))
        rec = np.empty((k.value, m, D + 1), dtype=np.float32)
        check(lib().wl_sim_read_probes(self._h, rec.ctypes.data_as(C.POINTER(C.c_float)), k.value, C.byref(k), C.byref(first)))
        ends = np.cumsum(np.asarray(self.dt, dtype=np.float32), dtype=np.float32)      # ends[j] = sum(Δt[1:j+1]), summed in order in Float32
        t = ends[first.value:first.value + k.value].astype(np.float64)
        return t, rec[:, :, :D].copy(), rec[:, :, D].copy()

    def set_force_record(self, body, x0=None, capacity=1024):
        """record pressure force, viscous force and both moments about x0 (None: the origin) of `body` after every completed step of this handle —
        mom_step_ and each step inside mom_steps_ — for up to `capacity` steps between two read_forces(); evaluated on the device from the body's band
        only (two launches per step, no host round trip).  body: a body of bodies.py or a closed-form tuple; None switches recording off.  A later
        measure!(sim) of this handle (set_body, measure_body_, measure_sphere_, sim_step_(remeasure=True)) makes the body it measures the recorded one."""
        if body is None:
            check(lib().wl_sim_set_force_record(self._h, None, None, 0))
            return
        if int(capacity) < 1:
            raise ValueError("capacity must be at least 1")
        prog = _as_set(body).program(self.D)
        check(lib().wl_sim_set_force_record(self._h, C.byref(prog), _x0_checked(x0, self.D), int(capacity)))

    def read_forces(self):
        """(t, pF[k,D], vF[k,D], pM[k,·], vM[k,·]) of the k records taken since the last read, oldest first (Float64; the moments have three columns in
        3-D, one in 2-D); t as in read_probes.  Empties the buffer."""
        k, first = C.c_int(0), C.c_int(0)
        check(lib().wl_sim_read_forces(self._h, None, 0, C.byref(k), C.byref(first)))
        rec = np.empty((k.value, 12), dtype=np.float64)
        check(lib().wl_sim_read_forces(self._h, rec.ctypes.data_as(C.POINTER(C.c_double)), k.value, C.byref(k), C.byref(first)))
        ends = np.cumsum(np.asarray(self.dt, dtype=np.float32), dtype=np.float32)
        t = ends[first.value:first.value + k.value].astype(np.float64)
        return (t,) + _split_forces(rec, self.D)

    def forces(self, body, x0=None):
        """(pF[D], vF[D], pM[·], vM[·]) of `body` on the current p and u in one pass over the body's band and one read-back: what pressure_force_body,
        viscous_force_body, pressure_moment_body and viscous_moment_body return, summed from the same per-cell terms"""
        prog = _as_set(body).program(self.D)
        out = (C.c_double * 12)()
        check(lib().wl_sim_forces_bodyset(self._h, _x0_checked(x0, self.D), C.byref(prog), out, stream()))
        return tuple(a[0] for a in _split_forces(np.array(out[:], dtype=np.float64)[None, :], self.D))

    def set_tracers(self, points):
        """a swarm of tracer particles at the (n, D) host points, advanced by every completed step of this handle (wl_advect with u⁰, the final u and
        the step's Δt); points=None (or empty) removes it"""
        x = np.zeros((0, self.D), dtype=np.float32) if points is None else np.ascontiguousarray(np.asarray(points, dtype=np.float32)).reshape(-1, self.D)
        check(lib().wl_sim_set_tracers(self._h, x.ctypes.data_as(C.POINTER(C.c_float)), int(x.shape[0])))

    def tracers(self):
        """(x, x_prev): positions and positions before the last step, as (n, D) device tensors over the handle's memory (valid until set_tracers)"""
        import torch
        out = []
        for which in (0, 1):
            n = C.c_size_t(0)
            p = lib().wl_sim_tracers(self._h, which, C.byref(n))
            if not p or n.value == 0:
                out.append(torch.empty((0, self.D), dtype=torch.float32, device=core.device()))
                continue
            cnt, addr = int(n.value) * self.D, int(p)

            class _Mem:      # __cuda_array_interface__ of memory the handle owns
                __cuda_array_interface__ = {"shape": (cnt,), "typestr": "<f4", "data": (addr, False), "version": 2}
            out.append(torch.as_tensor(_Mem(), device=core.device()).view(int(n.value), self.D))
        return out[0], out[1]

    def set_meanflow(self, uu_stats=False, every=1, t_init=None):
        """MeanFlow(flow; t_init=time(flow), uu_stats) as an observer of this handle (src/Metrics.jl:205-226): after every `every`-th completed step —
        mom_step_ and each step inside mom_steps_ — update! runs on the device in one launch, with no host round trip and the other steps' deferrals
        left alone.  set_meanflow(None) switches it off and frees the averages."""
        if uu_stats is None:
            check(lib().wl_sim_set_meanflow(self._h, 0, 1, 0.0, stream()))
            return
        if int(every) < 1:
            raise ValueError("every must be at least 1")
        check(lib().wl_sim_set_meanflow(self._h, 2 if uu_stats else 1, int(every), float("nan") if t_init is None else float(t_init), stream()))

    def reset_meanflow(self, t_init=0.0):
        """reset!(meanflow; t_init)   :229-234"""
        check(lib().wl_sim_meanflow_reset(self._h, float(t_init), stream()))

    def update_meanflow(self):
        """update!(meanflow, flow) now, on the current u and p (independent of `every`)   :236-248"""
        check(lib().wl_sim_meanflow_update(self._h, stream()))

    def _mean_view(self, which, shape):
        import torch
        n = C.c_size_t(0)
        p = lib().wl_sim_meanflow(self._h, which, C.byref(n))
        if not p:
            raise WlError("no mean-flow observer is set (set_meanflow)" if which < 2 else "the mean-flow observer keeps no UU (set_meanflow(uu_stats=True))")
        cnt, addr = int(np.prod(shape)), int(p)
        assert cnt == int(n.value)

        class _Mem:      # __cuda_array_interface__ of memory the handle owns
            __cuda_array_interface__ = {"shape": (cnt,), "typestr": "<f4", "data": (addr, False), "version": 2}
        t = torch.as_tensor(_Mem(), device=core.device())
        return t.view(tuple(reversed(shape))).permute(*reversed(range(len(shape))))

    def _mean_uu(self, tau):
        if not lib().wl_sim_meanflow(self._h, 2, None):
            raise WlError("the mean-flow observer keeps no UU (set_meanflow(uu_stats=True))")
        out = core.jl_zeros(self.Ng + (self.D, self.D))
        check(lib().wl_sim_meanflow_uu(self._h, ptr(out), int(tau), stream()))
        return out

    def meanflow_t(self):
        """meanflow.t as a list of Float32"""
        k = lib().wl_sim_meanflow_t(self._h, None, 0)
        out = (C.c_float * max(k, 1))()
        lib().wl_sim_meanflow_t(self._h, out, k)
        return [np.float32(v) for v in out[:k]]

    def meanflow(self):
        """(P, U, UU, t): P and U are device tensors over the handle's memory in the shapes of field("p") and field("u") (valid until the next
        set_meanflow); UU is a NEW (N…, D, D) device tensor expanded from the packed upper triangle the handle keeps, None without uu_stats; t = meanflow.t"""
        P, U = self._mean_view(0, self.Ng), self._mean_view(1, self.Ng + (self.D,))
        UU = self._mean_uu(0) if lib().wl_sim_meanflow(self._h, 2, None) else None
        return P, U, UU, self.meanflow_t()

    def meanflow_uu(self):
        """uu(meanflow): the Reynolds stresses τ = UU − U⊗U as a new (N…, D, D) device tensor   :250-257"""
        return self._mean_uu(1)

    def load_meanflow_(self):
        """copy!(flow, meanflow): flow.u .= U; flow.p .= P   :259-262"""
        P, U, _, _ = self.meanflow()
        self.set_field("u", core.to_host(U))
        self.set_field("p", core.to_host(P))

    def sync(self):
        check(lib().wl_stream_sync(stream()))
