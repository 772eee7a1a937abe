"""The stream contract (include/wlhip.h, Conventions) on every entry point that takes a `stream`: each scenario runs once on the default stream and
once on non-blocking side streams behind delays, with the default stream blocked (tests/stream_harness.py), and must produce the same bits.
tests/test_stream_contract_cpu.py checks that every such entry point of the header appears here: a leaf in LEAF, a handle call in a
`step("wl_...")` of a handle scenario.

Handles are created after a synchronisation on the default stream (wl_mg_create, wl_sim_create* work there and return finished) and before the
blocker is queued; from then on nothing here touches the default stream.
"""
import ctypes as C

import numpy as np
import pytest

from stream_harness import Raw, Step, run_on_streams

pytestmark = pytest.mark.gpu
f32 = np.float32

S3A, S3B, S2 = (34, 18, 10), (10, 9, 8), (12, 7)          # the shapes of test_gpu_ops.py
RED_N = (1, 255, 257, 1_000_003)


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    return w


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def F3(*v):
    return (C.c_float * 3)(*([float(x) for x in v] + [0.0] * (3 - len(v))))


class Ctx:
    """the arrays of one leaf row: seeded, created on the default stream; everything made through it is armed and compared"""

    def __init__(self, w, shape, seed):
        self.w, self.L, self.shape, self.D = w, w.lib(), tuple(shape), len(shape)
        self.rng = np.random.default_rng(seed)
        self.arrays = []
        self.g = w.core.grid_of(self.shape)
        self.G = C.byref(self.g)
        self.keep = []

    def _mk(self, shape, lo, hi):
        t = self.w.to_device(np.asfortranarray(self.rng.uniform(lo, hi, size=shape).astype(f32)))
        self.arrays.append(t)
        return t

    def s(self, lo=-1.0, hi=1.0, shape=None):
        return self._mk(self.shape if shape is None else tuple(shape), lo, hi)

    def v(self, lo=-1.0, hi=1.0, shape=None):
        sh = self.shape if shape is None else tuple(shape)
        return self._mk(sh + (len(sh),), lo, hi)

    def t(self, lo=-1.0, hi=1.0):
        return self._mk(self.shape + (self.D, self.D), lo, hi)

    def flat(self, n, lo=-1.0, hi=1.0):
        import torch
        t = torch.from_numpy(self.rng.uniform(lo, hi, size=n).astype(f32)).cuda()
        self.arrays.append(t)
        return t

    def coefL(self):
        """face coefficients in (0.2, 1), zero on the wall faces (BC!(L,0))"""
        Lc = self.v(0.2, 1.0)
        assert self.L.wl_bc_vec(P(Lc), self.G, F3(0, 0, 0), 0, 0, None) == 0
        return Lc

    def poisson(self):
        """x, z, r, eps, L, D, iD of a single-level Poisson (D, iD from set_diag! on the default stream)"""
        x, z, r, eps, Lc, D, iD = self.s(), self.s(), self.s(), self.s(), self.coefL(), self.s(), self.s()
        assert self.L.wl_set_diag(P(D), P(iD), P(Lc), self.G, None) == 0
        return x, z, r, eps, Lc, D, iD

    def coarse(self):
        sh = tuple(1 + n // 2 if (n % 2 == 0 and n > 4) else n for n in self.shape)
        g = self.w.core.grid_of(sh)
        self.keep.append(g)
        return sh, C.byref(g)


LEAF = []          # (entry point, variant, shape, builder, sync)


def leaf(name, shapes=(S3A, S3B, S2), sync=False, variant=""):
    def deco(f):
        for sh in shapes:
            LEAF.append((name, variant, sh, f, sync))
        return f
    return deco


ONLY3 = (S3A, S3B)

# ---- copies, element-wise ------------------------------------------------------------------------------------------------------------------
@leaf("wl_h2d")
def _(c):
    import torch
    a = c.s()
    h = torch.from_numpy(c.rng.uniform(-1, 1, size=a.numel()).astype(f32)).pin_memory()
    c.keep.append(h)
    return lambda sp: c.L.wl_h2d(P(a), C.c_void_p(h.data_ptr()), a.numel() * 4, sp)


@leaf("wl_d2h", sync=True)
def _(c):
    a = c.s()
    h = np.zeros(a.numel(), dtype=f32)
    return (lambda sp: c.L.wl_d2h(h.ctypes.data_as(C.c_void_p), P(a), h.nbytes, sp)), h


@leaf("wl_d2d")
def _(c):
    a, b = c.s(), c.s()
    return lambda sp: c.L.wl_d2d(P(a), P(b), a.numel() * 4, sp)


@leaf("wl_stream_sync", shapes=(S3B,), sync=True)
def _(c):
    a = c.s()
    return lambda sp: c.L.wl_fill(P(a), 0.25, a.numel(), sp) or c.L.wl_stream_sync(sp)


@leaf("wl_fill")
def _(c):
    a = c.s()
    return lambda sp: c.L.wl_fill(P(a), 0.5, a.numel(), sp)


@leaf("wl_scale")
def _(c):
    a = c.s()
    return lambda sp: c.L.wl_scale(P(a), 0.3, a.numel(), sp)


@leaf("wl_div_scalar")
def _(c):
    a = c.s()
    return lambda sp: c.L.wl_div_scalar(P(a), 0.3, a.numel(), sp)


# ---- the generic reductions (process-wide workspace, pinned read-back record) ---------------------------------------------------------------
def _red(name, n):
    def sum_(c):
        a, out = c.flat(n), C.c_double()
        return (lambda sp: c.L.wl_sum(P(a), n, C.byref(out), sp)), out

    def l1_(c):
        a, o1, o2 = c.flat(n), C.c_double(), C.c_float()
        return (lambda sp: c.L.wl_sum_abs_max_abs(P(a), n, C.byref(o1), C.byref(o2), sp)), (o1, o2)

    def max_(c):
        a, out = c.flat(n), C.c_float()
        return (lambda sp: c.L.wl_max(P(a), n, C.byref(out), sp)), out

    def dot_(c):
        a, b, out = c.flat(n), c.flat(n), C.c_double()
        return (lambda sp: c.L.wl_dot(P(a), P(b), n, C.byref(out), sp)), out
    return {"wl_sum": sum_, "wl_sum_abs_max_abs": l1_, "wl_max": max_, "wl_dot": dot_}[name]


for _name in ("wl_sum", "wl_sum_abs_max_abs", "wl_max", "wl_dot"):
    for _n in RED_N:
        LEAF.append((_name, f"n{_n}", "reductions", _red(_name, _n), True))


@leaf("wl_L2_inside", sync=True)
def _(c):
    a, out = c.s(), C.c_double()
    return (lambda sp: c.L.wl_L2_inside(P(a), c.G, C.byref(out), sp)), out


@leaf("wl_norms", sync=True)
def _(c):
    a, o1, o2 = c.s(), C.c_double(), C.c_float()
    return (lambda sp: c.L.wl_norms(P(a), c.G, C.byref(o1), C.byref(o2), None, sp)), (o1, o2)


@leaf("wl_cfl", sync=True)
def _(c):
    u, sg, out = c.v(), c.s(0, 3), C.c_float()
    return (lambda sp: c.L.wl_cfl(P(u), P(sg), c.G, 0.01, 10.0, C.byref(out), sp)), out


# ---- boundary conditions -----------------------------------------------------------------------------------------------------------------------
@leaf("wl_bc_vec")
def _(c):
    a, U = c.v(), F3(1.0, 0.5, -0.25)
    return lambda sp: c.L.wl_bc_vec(P(a), c.G, U, 1, 0b10, sp)


@leaf("wl_bc_vec_fn")
def _(c):
    a, Ub = c.v(), c.v()
    return lambda sp: c.L.wl_bc_vec_fn(P(a), P(Ub), c.G, 0, 0, sp)


@leaf("wl_bc_per_scalar")
def _(c):
    a = c.s()
    return lambda sp: c.L.wl_bc_per_scalar(P(a), c.G, 0b11, sp)


@leaf("wl_exit_bc")
def _(c):
    u, u0 = c.v(0, 1), c.v(0, 1)
    return lambda sp: c.L.wl_exit_bc(P(u), P(u0), c.G, 0.3, sp)


@leaf("wl_accelerate_field")
def _(c):
    r, G = c.v(), c.v()
    return lambda sp: c.L.wl_accelerate_field(P(r), P(G), c.G, sp)


@leaf("wl_accelerate")
def _(c):
    r, a = c.v(), F3(0.1, -0.2, 0.3)
    return lambda sp: c.L.wl_accelerate(P(r), c.G, a, sp)


# ---- Flow ----------------------------------------------------------------------------------------------------------------------------------------
@leaf("wl_conv_diff")
def _(c):
    r, u, Phi = c.v(), c.v(), c.s()
    return lambda sp: c.L.wl_conv_diff(P(r), P(u), P(Phi), c.G, 0.07, 0, 0, sp)


@leaf("wl_bdim")
def _(c):
    u, u0, f, V, mu0, mu1 = c.v(), c.v(), c.v(), c.v(), c.v(), c.t()
    return lambda sp: c.L.wl_bdim(P(u), P(u0), P(f), P(V), P(mu0), P(mu1), c.G, 0.37, 1.0, 0.5, sp)


@leaf("wl_scale_u")
def _(c):
    u = c.v()
    return lambda sp: c.L.wl_scale_u(P(u), c.G, 0.5, sp)


@leaf("wl_div")
def _(c):
    z, u = c.s(), c.v()
    return lambda sp: c.L.wl_div(P(z), P(u), c.G, sp)


@leaf("wl_project")
def _(c):
    u, Lc, x = c.v(), c.v(0, 1), c.s()
    return lambda sp: c.L.wl_project(P(u), P(Lc), P(x), c.G, sp)


@leaf("wl_sgs", shapes=ONLY3)
def _(c):
    f, sg, u = c.v(), c.s(), c.v()
    return lambda sp: c.L.wl_sgs(P(f), P(sg), P(u), c.G, 0.17, 1.0, sp)


# ---- Poisson leaves ----------------------------------------------------------------------------------------------------------------------------
@leaf("wl_set_diag")
def _(c):
    D, iD, Lc = c.s(), c.s(), c.coefL()
    return lambda sp: c.L.wl_set_diag(P(D), P(iD), P(Lc), c.G, sp)


@leaf("wl_mult")
def _(c):
    x, z, r, eps, Lc, D, iD = c.poisson()
    return lambda sp: c.L.wl_mult(P(z), P(Lc), P(D), P(x), c.G, sp)


@leaf("wl_residual")
def _(c):
    x, z, r, eps, Lc, D, iD = c.poisson()
    return lambda sp: c.L.wl_residual(P(r), P(x), P(z), P(Lc), P(D), P(iD), c.G, None, sp)


@leaf("wl_increment")
def _(c):
    x, z, r, eps, Lc, D, iD = c.poisson()
    return lambda sp: c.L.wl_increment(P(r), P(x), P(eps), P(Lc), P(D), c.G, 0.7, sp)


@leaf("wl_jacobi")
def _(c):
    x, z, r, eps, Lc, D, iD = c.poisson()
    return lambda sp: c.L.wl_jacobi(P(eps), P(r), P(x), P(Lc), P(D), P(iD), c.G, 2, 0.9, 0, sp)


@leaf("wl_gsrb")
def _(c):
    x, z, r, eps, Lc, D, iD = c.poisson()
    return lambda sp: c.L.wl_gsrb(P(eps), P(r), P(x), P(Lc), P(D), P(iD), c.G, 4, 0.8, 0, sp)


@leaf("wl_pcg", sync=True)
def _(c):
    x, z, r, eps, Lc, D, iD = c.poisson()
    return lambda sp: c.L.wl_pcg(P(eps), P(r), P(x), P(z), P(Lc), P(D), P(iD), c.G, 6, 0, sp)


@leaf("wl_poisson_solve", sync=True)
def _(c):
    x, z, r, eps, Lc, D, iD = c.poisson()
    n, r1, ri = C.c_int(), C.c_double(), C.c_float()
    return (lambda sp: c.L.wl_poisson_solve(P(eps), P(r), P(x), P(z), P(Lc), P(D), P(iD), c.G, 1e-4, 3, 0, C.byref(n), C.byref(r1), C.byref(ri), sp)), (n, r1, ri)


# ---- multigrid transfer ------------------------------------------------------------------------------------------------------------------------
@leaf("wl_restrict")
def _(c):
    sh, gc = c.coarse()
    a, b = c.s(shape=sh), c.s()
    return lambda sp: c.L.wl_restrict(P(a), gc, P(b), c.G, sp)


@leaf("wl_prolongate")
def _(c):
    sh, gc = c.coarse()
    a, b = c.s(), c.s(shape=sh)
    return lambda sp: c.L.wl_prolongate(P(a), c.G, P(b), gc, sp)


@leaf("wl_restrictL")
def _(c):
    sh, gc = c.coarse()
    a, b = c.v(shape=sh), c.v(0, 1)
    return lambda sp: c.L.wl_restrictL(P(a), gc, P(b), c.G, 0, sp)


# ---- temporal averages, sub-grid-scale force ---------------------------------------------------------------------------------------------------
@leaf("wl_meanflow_update")
def _(c):
    Pm, U, UU, p, u = c.s(), c.v(), c.t(), c.s(), c.v()
    return lambda sp: c.L.wl_meanflow_update(P(Pm), P(U), P(UU), P(p), P(u), c.G, 0.25, sp)


@leaf("wl_meanflow_uu")
def _(c):
    tau, UU, U = c.t(), c.t(), c.v()
    return lambda sp: c.L.wl_meanflow_uu(P(tau), P(UU), P(U), c.G, sp)


# ---- flow diagnostics ------------------------------------------------------------------------------------------------------------------------------
@leaf("wl_ke")
def _(c):
    out, u, U = c.s(), c.v(), F3(0.1, 0.2, 0.3)
    return lambda sp: c.L.wl_ke(P(out), P(u), c.G, U, sp)


@leaf("wl_curl")
def _(c):
    out, u = c.s(), c.v()
    return lambda sp: c.L.wl_curl(P(out), P(u), c.G, 3, sp)


@leaf("wl_omega", shapes=ONLY3)
def _(c):
    out, u = c.v(), c.v()
    return lambda sp: c.L.wl_omega(P(out), P(u), c.G, sp)


@leaf("wl_omega_mag", shapes=ONLY3)
def _(c):
    out, u = c.s(), c.v()
    return lambda sp: c.L.wl_omega_mag(P(out), P(u), c.G, sp)


@leaf("wl_omega_theta", shapes=ONLY3)
def _(c):
    out, u, z, ce = c.s(), c.v(), F3(0, 0, 1), F3(4, 4, 4)
    return lambda sp: c.L.wl_omega_theta(P(out), P(u), c.G, z, ce, sp)


@leaf("wl_lambda2", shapes=ONLY3)
def _(c):
    out, u = c.s(), c.v()
    return lambda sp: c.L.wl_lambda2(P(out), P(u), c.G, sp)


@leaf("wl_helicity", shapes=ONLY3)
def _(c):
    out, u, om = c.s(), c.v(), c.v()
    return lambda sp: c.L.wl_helicity(P(out), P(u), P(om), c.G, sp)


@leaf("wl_flow_fields", shapes=ONLY3)
def _(c):
    u, ke, w3, wm, l2 = c.v(), c.s(), c.v(), c.s(), c.s()
    return lambda sp: c.L.wl_flow_fields(P(u), c.G, None, P(ke), P(w3), P(wm), P(l2), sp)


@leaf("wl_flow_stats", sync=True)          # scratch NULL: the library's process-wide workspace
def _(c):
    u, out = c.v(), (C.c_double * 3)()
    return (lambda sp: c.L.wl_flow_stats(P(u), c.G, None, out, None, sp)), out


# ---- closed-form bodies and composite bodies: measure!, forces, moments ----------------------------------------------------------------------------
def _body(c):
    from waterlily_jl_amd._lib import make_body
    ctr = [n / 2.0 for n in c.shape]
    b = make_body(("sphere", ctr, 2.5), c.D)
    c.keep.append(b)
    return C.byref(b)


def _bodyset(c):
    from waterlily_jl_amd.bodies import Body
    ctr = [n / 2.0 for n in c.shape]
    prog = (Body(("sphere", ctr, 2.5)) | Body(("plane", [2.0] * c.D, [1.0] + [0.0] * (c.D - 1)))).program(c.D)
    c.keep.append(prog)
    return C.byref(prog)


@leaf("wl_measure_body")
def _(c):
    sg, mu0, mu1, V, b = c.s(), c.v(), c.t(), c.v(), _body(c)
    return lambda sp: c.L.wl_measure_body(P(sg), P(mu0), P(mu1), P(V), c.G, b, 1.0, 0, 0, sp)


@leaf("wl_measure_bodyset")
def _(c):
    sg, mu0, mu1, V, b = c.s(), c.v(), c.t(), c.v(), _bodyset(c)
    return lambda sp: c.L.wl_measure_bodyset(P(sg), P(mu0), P(mu1), P(V), c.G, b, 1.0, 0, 0, sp)


@leaf("wl_pressure_force_body", sync=True)
def _(c):
    p, b, out = c.s(), _body(c), (C.c_double * 3)()
    return (lambda sp: c.L.wl_pressure_force_body(P(p), c.G, b, out, sp)), out


@leaf("wl_viscous_force_body", sync=True)
def _(c):
    u, b, out = c.v(), _body(c), (C.c_double * 3)()
    return (lambda sp: c.L.wl_viscous_force_body(P(u), c.G, 0.01, b, out, sp)), out


@leaf("wl_pressure_moment_body", sync=True)
def _(c):
    p, b, out, x0 = c.s(), _body(c), (C.c_double * 3)(), F3(1, 2, 3)
    return (lambda sp: c.L.wl_pressure_moment_body(x0, P(p), c.G, b, out, sp)), out


@leaf("wl_viscous_moment_body", sync=True)
def _(c):
    u, b, out, x0 = c.v(), _body(c), (C.c_double * 3)(), F3(1, 2, 3)
    return (lambda sp: c.L.wl_viscous_moment_body(x0, P(u), c.G, 0.01, b, out, sp)), out


@leaf("wl_pressure_force_bodyset", sync=True)
def _(c):
    p, b, out = c.s(), _bodyset(c), (C.c_double * 3)()
    return (lambda sp: c.L.wl_pressure_force_bodyset(None, P(p), c.G, b, out, sp)), out


@leaf("wl_viscous_force_bodyset", sync=True)
def _(c):
    u, b, out, x0 = c.v(), _bodyset(c), (C.c_double * 3)(), F3(1, 2, 3)
    return (lambda sp: c.L.wl_viscous_force_bodyset(x0, P(u), c.G, 0.01, b, out, sp)), out


@leaf("wl_bodyset_measure_points", sync=True)
def _(c):
    b, n = _bodyset(c), 37
    x = c.rng.uniform(0, 8, size=n * c.D).astype(f32)
    d, nn, V = np.zeros(n, f32), np.zeros(n * c.D, f32), np.zeros(n * c.D, f32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    return (lambda sp: c.L.wl_bodyset_measure_points(b, c.D, fp(x), n, 1e30, fp(d), fp(nn), fp(V), sp)), (d, nn, V)


# ---- the communicator's entry points on ONE rank: a callback transport in loopback mode (both neighbours are this rank) whose callbacks move
# the planes with wl_d2d on the stream they are given — the compute stream, or the communicator's own stream behind ev_ready / ahead of ev_done
class LoopComm:
    def __init__(self, L):
        from waterlily_jl_amd._lib import ALLGATHER_FN, SENDRECV_FN

        def sendrecv(ctx, slo, rlo, shi, rhi, nbytes, st):
            rc = 0
            if rlo and shi:
                rc |= L.wl_d2d(rlo, shi, nbytes, st)
            if rhi and slo:
                rc |= L.wl_d2d(rhi, slo, nbytes, st)
            return rc

        def allgather(ctx, send, recv, nbytes, st):
            return L.wl_d2d(recv, send, nbytes, st) if send != recv else 0
        self._sr, self._ag, self.L = SENDRECV_FN(sendrecv), ALLGATHER_FN(allgather), L
        h = C.c_void_p()
        assert L.wl_comm_callbacks_create(C.byref(h), 0, 1, None, C.cast(self._sr, C.c_void_p), C.cast(self._ag, C.c_void_p)) == 0
        assert L.wl_comm_set_loopback(h, 1) == 0
        self.h = h

    def __del__(self):
        if getattr(self, "h", None):
            self.L.wl_comm_destroy(self.h)
            self.h = None


def _slab(c):
    """a slab that is not the whole domain (nz < gnz), two ghost planes per side, and a communicator whose streams and scratch exist already"""
    import torch
    from waterlily_jl_amd import slab
    g = slab.slab_grid((c.shape[0], c.shape[1], 2 + 12), 0, 2, halo=2)
    cm = LoopComm(c.L)
    c.keep += [g, cm]
    a = c.s(shape=(g.nx, g.ny, g.nz))
    warm = torch.zeros(g.nx * g.ny * g.nz, dtype=torch.float32, device="cuda")
    rec = torch.zeros(32, dtype=torch.float32, device="cuda")
    assert c.L.wl_comm_halo_async(cm.h, P(warm), C.byref(g), 1, 1, None) == 0          # creates the communicator's stream and events
    assert c.L.wl_comm_combine_test(cm.h, P(rec), C.c_void_p(rec.data_ptr() + 64), None) == 0   # … and its gather scratch
    torch.cuda.synchronize()
    return g, cm, a


@leaf("wl_halo_exchange", shapes=(S3A,))
def _(c):
    g, cm, a = _slab(c)
    return lambda sp: c.L.wl_halo_exchange(cm.h, P(a), C.byref(g), 1, 2, sp)


@leaf("wl_comm_halo_async", shapes=(S3A,))
def _(c):
    g, cm, a = _slab(c)
    return lambda sp: c.L.wl_comm_halo_async(cm.h, P(a), C.byref(g), 1, 2, sp)


@leaf("wl_allgather_planes", shapes=(S3A,))
def _(c):
    g, cm, _a = _slab(c)
    view = c.w.core.grid_of((6, 5, 5))
    c.keep.append(view)
    t = c.flat(6 * 5 * 5)
    return lambda sp: c.L.wl_allgather_planes(cm.h, P(t), C.byref(view), 1, sp)


@leaf("wl_comm_combine_test", shapes=(S3A,))
def _(c):
    g, cm, _a = _slab(c)
    rec = c.flat(32)
    return lambda sp: c.L.wl_comm_combine_test(cm.h, P(rec), C.c_void_p(rec.data_ptr() + 64), sp)


LEAF_NAMES = sorted({r[0] for r in LEAF})


def _leaf_steps(w, group):
    def make():
        import torch
        steps, keep = [], []
        for k, (name, variant, shape, build, sync) in enumerate(r for r in LEAF if r[2] == group):
            c = Ctx(w, S3B if shape == "reductions" else shape, 1000 + k)
            r = build(c)
            fn, host = r if isinstance(r, tuple) else (r, None)

            def call(sp, fn=fn, host=host, name=name):
                rc = fn(sp)
                assert rc == 0, (name, rc, w.lib().wl_last_error_string())
                return host
            steps.append(Step(f"{name}{'[' + variant + ']' if variant else ''}", call, list(c.arrays), sync=sync))
            keep.append(c)
        torch.cuda.synchronize()
        return steps, keep
    return make


@pytest.mark.parametrize("group", [S3A, S3B, S2, "reductions"], ids=["34x18x10", "10x9x8", "12x7", "reductions"])
def test_leaf_operations_keep_the_stream_contract(w, group):
    """every exported leaf with a `stream` parameter, one step each: the same bits on a delayed side stream with the default stream blocked"""
    run_on_streams(w.lib(), _leaf_steps(w, group), label=f"leaves {group}")


# ====================================================================================================================================================
# handles
# ====================================================================================================================================================
def step(name, call, arrays, sync=False, **kw):
    """one handle call as a Step; `name` is what tests/test_stream_contract_cpu.py reads"""
    def run(sp):
        r = call(sp)
        rc, host = r if isinstance(r, tuple) else (r, None)
        assert rc == 0, (name, rc)
        return host
    return Step(name, run, arrays, sync=sync, **kw)


def mg_fields(L, mg, levels=None):
    out = []
    g = w_grid()
    for l in range(L.wl_mg_nlevels(mg)) if levels is None else levels:
        assert L.wl_mg_level_grid(mg, l, C.byref(g)) == 0
        nc = g.nx * g.ny * g.nz
        for nm in ("L", "D", "iD", "x", "eps", "r", "z"):
            out.append(Raw(f"level {l} {nm}", (lambda l=l, nm=nm: L.wl_mg_level_field(mg, l, nm.encode())), nc * (g.D if nm == "L" else 1)))
    return out


def w_grid():
    from waterlily_jl_amd._lib import wl_grid
    return wl_grid()


def sim_fields(L, sg, names=("u", "u0", "us", "f", "p", "sigma", "mu0")):
    g = w_grid()
    assert L.wl_sim_grid(sg._h, C.byref(g)) == 0
    nc, D = g.nx * g.ny * g.nz, g.D
    size = {"p": 1, "sigma": 1, "mu1": D * D}
    out = []
    for nm in names:
        if L.wl_sim_field(sg._h, nm.encode()):
            out.append(Raw(nm, (lambda nm=nm: L.wl_sim_field(sg._h, nm.encode())), nc * size.get(nm, D)))
    return out


def _mg_steps(L, mg, arrays, itmx=(1, 3)):
    nlev = L.wl_mg_nlevels(mg)
    steps = [step("wl_mg_update", lambda sp: L.wl_mg_update(mg, sp), arrays, sync=True)]      # update! reads flags back on some levels
    for l in range(nlev - 1):
        steps.append(step("wl_mg_vcycle", (lambda sp, l=l: L.wl_mg_vcycle(mg, l, 0.9, sp)), arrays))
    for l in range(nlev):
        steps.append(step("wl_mg_smooth", (lambda sp, l=l: L.wl_mg_smooth(mg, l, 4, 0.9, sp)), arrays))
    for it in itmx:
        n, r1, ri = C.c_int(), C.c_double(), C.c_float()
        steps.append(step("wl_mg_solve", (lambda sp, it=it, n=n, r1=r1, ri=ri: (L.wl_mg_solve(mg, 1e-4, it, C.byref(n), C.byref(r1), C.byref(ri), sp), (n, r1, ri))),
                          arrays, sync=True))
    return steps


def test_multigrid_handle_random_L(w):
    """wl_mg_update, wl_mg_vcycle and wl_mg_smooth per level, wl_mg_solve with itmx 1 and 3 on (66,34,18) with random coefficients"""
    L = w.lib()

    def make():
        import torch
        c = Ctx(w, (66, 34, 18), 5)
        x, z, Lc = c.s(), c.s(-1e-2, 1e-2), c.coefL()
        torch.cuda.synchronize()
        mg = w.MultiLevelPoisson(x, Lc, z)
        torch.cuda.synchronize()
        return _mg_steps(L, mg._h, mg_fields(L, mg._h)), (c, mg)
    run_on_streams(L, make, label="mg random L")


def _body_sim(w, n=(128, 64, 96), R=8.0, **opts):
    import torch
    sg = w.FusedSimulation(n, (1, 0, 0), 2 * R, U=1, nu=2 * R / 250, has_body=True)
    for k, v in opts.items():
        sg.set_option(k, v)
    sg.measure_sphere_((n[0] / 4, n[1] / 2 - 1, n[2] / 2 - 1), R, 1.0)
    sg.mom_step_()
    torch.cuda.synchronize()
    return sg


def test_multigrid_body_level_forks_onto_the_auxiliary_streams(w):
    """the z-split smoother of a level with a body, its three plane ranges on the main stream and the two auxiliary streams (fork/join with the shared
    events): the case of test_zsplit_smoother_on_body_levels_is_bit_identical, V-cycle, smooth!, solver! and a whole step.
    What this arms: a fork whose wait is missing or taken from another stream (the auxiliary streams would read the sentinel).  A missing JOIN is detected
    only with some probability: the three ranges start together once S's delay is over and their kernels take 35–76 µs each, so the main stream passes the
    point of the missing wait after the auxiliary kernel has finished unless that kernel happens to be the slowest — the harness cannot delay a stream the
    library owns.  With one hipStreamWaitEvent of par_join removed this test passed in the one run that was made."""
    L = w.lib()

    def make():
        sg = _body_sim(w, zsplit=2, zsplit_par=1)
        assert sg.smoother_kinds()[0] == 3          # z-split: the forked path
        mg = L.wl_sim_pois(sg._h)
        arrays = sim_fields(L, sg, ("u", "p", "sigma", "f")) + mg_fields(L, mg, levels=(0, 1))
        n, r1, ri = C.c_int(), C.c_double(), C.c_float()
        steps = [step("wl_mg_vcycle", lambda sp: L.wl_mg_vcycle(mg, 0, 0.9, sp), arrays),
                 step("wl_mg_smooth", lambda sp: L.wl_mg_smooth(mg, 0, 4, 0.9, sp), arrays),
                 step("wl_mg_solve", lambda sp: (L.wl_mg_solve(mg, 1e-4, 3, C.byref(n), C.byref(r1), C.byref(ri), sp), (n, r1, ri)), arrays, sync=True),
                 step("wl_sim_mom_step", lambda sp: L.wl_sim_mom_step(sg._h, sp), arrays, sync=True)]
        return steps, sg
    run_on_streams(L, make, label="mg body, z-split on three streams")


def test_body_mask_fast_path_and_remeasure(w):
    """the case of test_body_mask_fast_path_is_bit_identical (64³, sphere): steps, a remeasure that moves the body (wl_sim_measure_sphere, wl_sim_measure_body,
    wl_sim_measure_bodyset + wl_sim_update), the force and moment read-outs of the handle"""
    L = w.lib()
    from waterlily_jl_amd._lib import make_body
    from waterlily_jl_amd.bodies import Body
    N, R = 64, 8.0

    def make():
        sg = _body_sim(w, (N, N, N), R)
        h = sg._h
        arrays = sim_fields(L, sg, ("u", "u0", "us", "f", "p", "sigma", "mu0", "mu1", "V"))
        ctr = (N / 4 + 3.5, N / 2 + 2, N / 2 - 1)
        body = make_body(("sphere", ctr, R), 3)
        prog = Body(("sphere", ctr, R)).program(3)
        c3, x0 = F3(*ctr), F3(1, 2, 3)
        outs = [(C.c_double * 3)() for _ in range(10)]
        steps = [step("wl_sim_mom_step", lambda sp: L.wl_sim_mom_step(h, sp), arrays, sync=True),
                 step("wl_sim_measure_sphere", lambda sp: L.wl_sim_measure_sphere(h, c3, R, 1.0, sp), arrays, sync=True),
                 step("wl_sim_mom_step", lambda sp: L.wl_sim_mom_step(h, sp), arrays, sync=True),
                 step("wl_sim_measure_body", lambda sp: L.wl_sim_measure_body(h, C.byref(body), 1.0, sp), arrays, sync=True),
                 step("wl_sim_measure_bodyset", lambda sp: L.wl_sim_measure_bodyset(h, C.byref(prog), 1.0, sp), arrays, sync=True),
                 step("wl_sim_update", lambda sp: L.wl_sim_update(h, sp), arrays, sync=True),
                 step("wl_sim_mom_step", lambda sp: L.wl_sim_mom_step(h, sp), arrays, sync=True),
                 step("wl_sim_pressure_force_sphere", lambda sp: (L.wl_sim_pressure_force_sphere(h, c3, R, outs[0], sp), outs[0]), arrays, sync=True),
                 step("wl_sim_viscous_force_sphere", lambda sp: (L.wl_sim_viscous_force_sphere(h, c3, R, outs[1], sp), outs[1]), arrays, sync=True),
                 step("wl_sim_pressure_force_body", lambda sp: (L.wl_sim_pressure_force_body(h, C.byref(body), outs[2], sp), outs[2]), arrays, sync=True),
                 step("wl_sim_viscous_force_body", lambda sp: (L.wl_sim_viscous_force_body(h, C.byref(body), outs[3], sp), outs[3]), arrays, sync=True),
                 step("wl_sim_pressure_moment_body", lambda sp: (L.wl_sim_pressure_moment_body(h, x0, C.byref(body), outs[4], sp), outs[4]), arrays, sync=True),
                 step("wl_sim_viscous_moment_body", lambda sp: (L.wl_sim_viscous_moment_body(h, x0, C.byref(body), outs[5], sp), outs[5]), arrays, sync=True),
                 step("wl_sim_pressure_force_bodyset", lambda sp: (L.wl_sim_pressure_force_bodyset(h, None, C.byref(prog), outs[6], sp), outs[6]), arrays, sync=True),
                 step("wl_sim_viscous_force_bodyset", lambda sp: (L.wl_sim_viscous_force_bodyset(h, x0, C.byref(prog), outs[7], sp), outs[7]), arrays, sync=True)]
        return steps, (sg, body, prog)
    run_on_streams(L, make, label="sim 64³ sphere, remeasured")


def test_discarded_speculation_on_a_side_stream(w):
    """a due mean shift (the spike of test_gpu_speculation.py, one float above the edge): the speculative solve queued behind the fused head is discarded
    and the two-kernel path taken, all of it on S; the counters say that it happened"""
    L = w.lib()
    from test_gpu_speculation import shift_edge, sim, spike_u
    dims = (64, 32, 32)
    lo, hi = shift_edge(int(np.prod(dims)))
    seen = []

    def make():
        import torch
        sg = sim(w, dims, spike_u(dims, hi))
        torch.cuda.synchronize()
        arrays = sim_fields(L, sg) + mg_fields(L, L.wl_sim_pois(sg._h), levels=(0,))
        seen.append(sg)
        return [step("wl_sim_phase", lambda sp: L.wl_sim_phase(sg._h, 2, sp), arrays, sync=True)], sg
    run_on_streams(L, make, label="due mean shift")
    for sg in seen[1:]:          # (the first is the warm-up)
        assert (sg.counter("resjac"), sg.counter("resjac_redo"), sg.counter("tailspec"), sg.counter("tailspec_armed")) == (0, 1, 0, 1)


def _tgv(w, dims=(64, 32, 24), **kw):
    opts = kw.pop("opts", {})
    sgs = kw.pop("sgs", None)
    D = len(dims)
    sg = w.FusedSimulation(dims, (0,) * D, dims[0], U=1, nu=dims[0] / 1600.0, ic=kw.pop("ic", "tgv" if D == 3 else "uBC"), **kw)
    for k, v in opts.items():
        sg.set_option(k, v)
    if sgs:
        sg.set_sgs(0.17, 1.0)
    return sg


def _sim_steps(L, sg, arrays, stats=True):
    h = sg._h
    dts = (C.c_float * 16)()
    out3 = (C.c_double * 3)()
    steps = [step("wl_sim_phase", (lambda sp, k=k: L.wl_sim_phase(h, k, sp)), arrays, sync=True) for k in range(6)]
    steps.append(step("wl_sim_mom_step", lambda sp: L.wl_sim_mom_step(h, sp), arrays, sync=True))
    if stats:
        steps.append(step("wl_sim_flow_stats", lambda sp: (L.wl_sim_flow_stats(h, None, out3, sp), out3), arrays, sync=True))
    steps.append(step("wl_sim_mom_steps", lambda sp: (L.wl_sim_mom_steps(h, 3, sp), (C.c_float(L.wl_sim_dt_last(h)), L.wl_sim_dt(h, dts, 16), dts)), arrays, sync=True))
    return steps


SIM_CASES = {
    "tgv": dict(),
    "periodic": dict(ic="tgv_periodic", perdir=(1, 2, 3)),
    "exit": dict(uBC=(1, 0, 0), exitBC=True),
    "2d": dict(dims=(64, 48)),
    "tailfuse": dict(opts={"tailfuse": 1, "resjac_min": 0, "convt_min": 0}),
    "sgs": dict(sgs=True),
}


@pytest.mark.parametrize("case", list(SIM_CASES))
def test_simulation_handle(w, case):
    """wl_sim_phase per phase, wl_sim_mom_step, wl_sim_mom_steps(3) (lazy Δt, pdefer) followed by wl_sim_dt_last / wl_sim_dt, flow statistics between steps"""
    L = w.lib()
    kw = dict(SIM_CASES[case])

    def make():
        import torch
        k2 = dict(kw)
        uBC = k2.pop("uBC", None)
        dims = k2.pop("dims", (64, 32, 24))
        if uBC is not None:
            sg = w.FusedSimulation(dims, uBC, dims[0], U=1, nu=dims[0] / 1600.0, **k2)
        else:
            sg = _tgv(w, dims, **k2)
        if len(dims) == 2 or uBC is not None:       # a flow that is not at rest / not uniform
            rng = np.random.default_rng(3)
            sg.set_field("u", np.asfortranarray((uBC[0] if uBC else 0.0) + rng.uniform(-0.3, 0.3, size=sg._shape("u")).astype(f32)))
            assert L.wl_sim_init_flow(sg._h, None) == 0
        torch.cuda.synchronize()
        arrays = sim_fields(L, sg) + mg_fields(L, L.wl_sim_pois(sg._h), levels=(0,))
        return _sim_steps(L, sg, arrays, stats=len(dims) == 3), sg
    run_on_streams(L, make, label=f"sim {case}")


def test_simulation_handle_setup_calls_and_fields(w):
    """wl_sim_apply_ic and wl_sim_init_flow on S, then a step; wl_sim_flow_fields into the handle's sigma and a caller's arrays between steps"""
    L = w.lib()

    def make():
        import torch
        sg = _tgv(w)
        h = sg._h
        c = Ctx(w, sg.Ng, 9)
        ke, w3, l2 = c.s(), c.v(), c.s()
        torch.cuda.synchronize()
        arrays = sim_fields(L, sg) + c.arrays
        steps = [step("wl_sim_apply_ic", lambda sp: L.wl_sim_apply_ic(h, 1, sp), arrays),
                 step("wl_sim_init_flow", lambda sp: L.wl_sim_init_flow(h, sp), arrays),
                 step("wl_sim_mom_step", lambda sp: L.wl_sim_mom_step(h, sp), arrays, sync=True),
                 step("wl_sim_flow_fields", lambda sp: L.wl_sim_flow_fields(h, None, P(ke), P(w3), L.wl_sim_field(h, b"sigma"), P(l2), sp), arrays),
                 step("wl_sim_mom_step", lambda sp: L.wl_sim_mom_step(h, sp), arrays, sync=True)]
        return steps, (sg, c)
    run_on_streams(L, make, label="sim setup calls, flow_fields")


def test_caller_owned_arrays_on_an_adopted_multigrid_handle(w):
    """wl_sim_create_on: the caller's arrays (armed as torch tensors) and the caller's wl_mg"""
    L = w.lib()
    from waterlily_jl_amd._lib import wl_sim_desc
    dims = (64, 32, 24)

    def make():
        import torch
        Ng = tuple(n + 2 for n in dims)
        z3, z1 = (lambda: w.jl_zeros(Ng + (3,))), (lambda: w.jl_zeros(Ng))
        u, u0, us, f, mu0, p, sg_ = z3(), z3(), z3(), z3(), w.jl_zeros(Ng + (3,), 1.0), z1(), z1()
        assert L.wl_bc_vec(P(mu0), C.byref(w.core.grid_of(Ng)), F3(0, 0, 0), 0, 0, None) == 0
        torch.cuda.synchronize()
        mg = w.MultiLevelPoisson(p, mu0, sg_)
        d = wl_sim_desc()
        d.D = 3
        for k in range(3):
            d.dims[k], d.uBC[k] = dims[k], 0.0
        d.nu, d.dt0, d.perdir_mask, d.exitBC, d.scheme, d.has_body = dims[0] / 1600.0, 0.25, 0, 0, 0, 0
        V, mu1 = z3(), w.jl_zeros(Ng + (3, 3))
        d.u, d.u0, d.us, d.f, d.p, d.sigma, d.mu0, d.V, d.mu1 = (t.data_ptr() for t in (u, u0, us, f, p, sg_, mu0, V, mu1))
        h = C.c_void_p()
        assert L.wl_sim_create_on(C.byref(h), C.byref(d), mg._h) == 0
        assert L.wl_sim_apply_ic(h, 1, None) == 0 and L.wl_sim_init_flow(h, None) == 0
        torch.cuda.synchronize()
        arrays = [u, u0, us, f, mu0, p, sg_, V, mu1]
        steps = [step("wl_sim_mom_step", lambda sp: L.wl_sim_mom_step(h, sp), arrays, sync=True),
                 step("wl_sim_mom_steps", lambda sp: L.wl_sim_mom_steps(h, 2, sp), arrays, sync=True)]

        class Keep:
            def __del__(self, h=h, L=L, mg=mg, a=arrays):
                L.wl_sim_destroy(h)
        return steps, (Keep(), mg, arrays)
    run_on_streams(L, make, label="caller-owned arrays")


# ---- one handle, changing streams --------------------------------------------------------------------------------------------------------------------
def test_changing_streams_on_one_handle(w):
    """two steps on S1, S2.wait_stream(S1), two steps on S2 behind a delay, one on the default stream after S2.synchronize(): equal to five steps on the
    default stream, bit for bit, with pdefer, tailspec and lazydt at their defaults"""
    L = w.lib()

    def make():
        import torch
        sg = _tgv(w)
        h = sg._h
        torch.cuda.synchronize()
        arrays = sim_fields(L, sg)
        one = lambda sp: L.wl_sim_mom_step(h, sp)   # noqa: E731
        dtl = lambda sp: (L.wl_sim_mom_step(h, sp), C.c_float(L.wl_sim_dt_last(h)))   # noqa: E731
        steps = [step("wl_sim_mom_step", one, arrays, sync=True, stream=0),
                 step("wl_sim_mom_steps", lambda sp: L.wl_sim_mom_steps(h, 1, sp), arrays, sync=True, stream=0),
                 step("wl_sim_mom_step", one, arrays, sync=True, stream=1, pre=lambda st: st[1].wait_stream(st[0])),
                 step("wl_sim_mom_step", dtl, arrays, sync=True, stream=1),
                 step("wl_sim_mom_step", dtl, arrays, sync=True, stream=-1, pre=lambda st: st[1].synchronize())]
        return steps, sg
    run_on_streams(L, make, nstreams=2, label="one handle, S1 -> S2 -> default")


# ---- two handles, two streams, one host thread --------------------------------------------------------------------------------------------------------
def test_two_handles_on_two_streams(w):
    """handles A and B take alternating steps on S1 and S2, each behind its own delay, with reductions on the process-wide workspace in between (the fork/join
    events, the pinned read-back record and that workspace are shared by all handles and streams): each handle equals its solo run"""
    L = w.lib()

    def make_pair(which):
        def make():
            import torch
            A = _tgv(w) if "A" in which else None
            B = _tgv(w, (32, 32, 32)) if "B" in which else None
            c = Ctx(w, (10, 9, 8), 4)
            a, out = c.flat(100_003), C.c_double()
            torch.cuda.synchronize()
            steps = []
            for k in range(3):
                if A:
                    steps.append(step("wl_sim_mom_step", lambda sp: (L.wl_sim_mom_step(A._h, sp), C.c_float(L.wl_sim_dt_last(A._h))), sim_fields(L, A), sync=True, stream=0))
                if "r" in which:
                    steps.append(step("wl_sum", lambda sp: (L.wl_sum(P(a), 100_003, C.byref(out), sp), out), [a], sync=True, stream=k % 2))
                if B:
                    steps.append(step("wl_sim_mom_step", lambda sp: (L.wl_sim_mom_step(B._h, sp), C.c_float(L.wl_sim_dt_last(B._h))), sim_fields(L, B), sync=True, stream=1))
            return steps, (A, B, c)
        return make

    from stream_harness import run_armed, run_baseline

    def solo(which):
        steps, keep = make_pair(which)()
        arr, host, _, _ = run_baseline(L, steps)
        return arr, host
    run_baseline(L, make_pair("ArB")()[0])                     # warm-up
    soloA, soloB = solo("A"), solo("B")
    steps, keep = make_pair("ArB")()
    _, _, enq, T = run_baseline(L, make_pair("ArB")()[0])
    report = {}
    arr, host = run_armed(L, steps, enq, T, nstreams=2, report=report)
    assert report["armed"]
    print(f"[streams] two handles: armed, T = {report['T_ms']:.1f} ms, blocker {report['block_ms']:.0f} ms, step delays {report['delays_ms']}")
    ia = [k for k, s in enumerate(steps) if s.name == "wl_sim_mom_step" and s.stream == 0]
    ib = [k for k, s in enumerate(steps) if s.name == "wl_sim_mom_step" and s.stream == 1]
    for idx, (sarr, shost), tag in ((ia, soloA, "A"), (ib, soloB, "B")):
        for q, k in enumerate(idx):
            assert host[k] == shost[q], (tag, q, "Δt")
            for x, y in zip(arr[k], sarr[q]):
                assert np.array_equal(x, y), (tag, q)


# ---- z-slabs: the communicator's stream and events under a side stream -------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dims", [(2, "64x64x64"), (3, "128x32x96")])
def test_slab_ranks_on_a_side_stream_match_single_domain(n, dims):
    from test_slab_cpu import run_ranks
    out = run_ranks(n, "gpu_sim", dims, "3", timeout=600, extra_env={"WL_SLAB_SIDE_STREAM": "1"})
    for r in range(n):
        assert f"rank {r}: gpu_sim ok" in out
        assert f"rank {r}: side stream armed" in out
