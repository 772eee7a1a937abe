"""Smagorinsky–Lilly LES (the reference's sgs! udf, src/util.jl:45-76) on the device: the leaf wl_sgs against the NumPy yardstick
(tests/sgs_ref.py), the composite's wiring against oracle leaves + the yardstick, composite = leaves, udf dispatch, dissipation,
rejections and the launch budget."""
import ctypes as C
import math

import numpy as np
import pytest

import sgs_ref

pytestmark = pytest.mark.gpu
CS, DELTA = 0.17, 1.0
WL_EINVAL = -1


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    return w


def _f32(a):
    return np.asfortranarray(a, dtype=np.float32)


def _ghost_mask(Ng):
    g = np.ones(Ng, bool)
    g[tuple(slice(1, n - 1) for n in Ng)] = False
    return g


def _dev_sgs(w, f, sigma, u, Cs, Delta):
    class A:
        pass
    a = A()
    a.f, a.sigma = w.to_device(f), w.to_device(sigma)
    ud = w.to_device(u)
    w.sgs_(a, ud, Cs, Delta)
    return w.to_host(a.f), w.to_host(a.sigma)


# ------------------------------------------------------------------------------------------------ 3. leaf vs yardstick
@pytest.mark.parametrize("dims", [(32, 32, 32), (20, 28, 36), (8, 24, 16)])
def test_leaf_matches_the_yardstick(w, dims):
    """wl_sgs on random smooth u and non-zero random f, compared over the WHOLE array (ghosts included).  S(I,u) is @fastmath in the
    reference, so bit equality with NumPy is not defined; the tolerance is measured per input: e32 = max|ref(float32) − ref(float64)|,
    and the device must satisfy max|dev − ref(float64)| ≤ 4·e32 (margin 4: reassociation of the four-term cross differences and of the
    nine-term S:S, plus one sqrt).  One run on an MI355X (Cs = 0.2, Δ = 1.5):
        dims (32, 32, 32): e32 = 5.454e-07  device error = 5.454e-07
        dims (20, 28, 36): e32 = 6.025e-07  device error = 6.025e-07
        dims (8, 24, 16):  e32 = 4.271e-07  device error = 4.271e-07
    (the device reproduced the float32 yardstick exactly in that run).
    Also: σ's ghost cells hold what the reference's sweeps leave there (±0 where a sweep's range covers the cell, untouched elsewhere)."""
    rng = np.random.default_rng(11)
    Ng = tuple(n + 2 for n in dims)
    u = _f32(np.stack([sgs_ref.smooth_field(Ng, rng) for _ in range(3)], -1))
    f0 = _f32(rng.standard_normal(Ng + (3,)))
    s0 = _f32(rng.standard_normal(Ng))
    Cs, Delta = 0.2, 1.5
    r64, _, _ = sgs_ref.sgs(f0, u, Cs, Delta, sigma=s0, dtype=np.float64)
    r32, s32, _ = sgs_ref.sgs(f0, u, Cs, Delta, sigma=s0, dtype=np.float32)
    e32 = float(np.abs(r32.astype(np.float64) - r64).max())
    fd, sd = _dev_sgs(w, f0, s0, u, Cs, Delta)
    err = float(np.abs(fd.astype(np.float64) - r64).max())
    print(f"dims {dims}: e32 = {e32:.3e}  device error = {err:.3e}  max|Δf| = {np.abs(r64 - f0).max():.3e}")
    assert np.abs(r64 - f0).max() > 1e-4           # the model did something
    assert e32 > 0 and err <= 4 * e32, (err, e32)
    gm = _ghost_mask(Ng)
    assert np.array_equal(sd[gm], s32[gm])
    assert np.array_equal(fd[gm], f0[gm])         # ghost cells of f only ever receive ±0


# ------------------------------------------------------------------------------------------------ 4. Cs = 0 is off
def _tgv(w, dims, nu=None, **kw):
    return w.FusedSimulation(dims, (0, 0, 0), dims[0], U=1, nu=dims[0] / 1600.0 if nu is None else nu, ic="tgv", **kw)


def _sphere(w, dims, R=4.0):
    s = w.FusedSimulation(dims, (1, 0, 0), 2 * R, U=1, nu=2 * R / 250, has_body=True)
    s.measure_sphere_(tuple(n / 2 - 1 for n in dims), R, 1.0)
    return s


@pytest.mark.parametrize("case", ["tgv", "sphere"])
def test_cs_zero_equals_off(w, case):
    """set_sgs(0.0, 1.0) takes the staged route and adds ±0: u, p and the Δt history equal the default (fused) path bit for bit"""
    mk = (lambda: _tgv(w, (32, 32, 32))) if case == "tgv" else (lambda: _sphere(w, (32, 32, 32)))
    off, on = mk(), mk()
    on.set_sgs(0.0, 1.0)
    for step in range(3):
        off.mom_step_(); on.mom_step_()
        assert np.array_equal(on.field("u"), off.field("u")), step
        assert np.array_equal(on.field("p"), off.field("p")), step
    assert np.array_equal(np.array(on.dt), np.array(off.dt))
    assert on.pois_n == off.pois_n


# ------------------------------------------------------------------------------------------------ 5. wiring
@pytest.mark.parametrize("dims", [(32, 32, 32), (24, 32, 40)])
@pytest.mark.parametrize("body", [False, True])
def test_phases_against_oracle_leaves_and_the_yardstick(w, oracle, dims, body):
    """From a developed state, wl_sim_phase(s,1) against oracle.conv_diff → sgs_ref(float32) → oracle.BDIM → oracle.BC on copies of the same
    fields (the model sees u⁰), and wl_sim_phase(s,3) likewise (the model sees the projected u; then scale_u(½)).  Tolerance on u:
    4·e32·Δt with e32 = max|sgs_ref(float32) − sgs_ref(float64)| on that phase's (r, u).  One run on an MI355X: e32 = 9.1e-9 … 3.5e-8,
    Δt = 0.59 … 0.91, bounds 3.2e-8 … 8.3e-8, device error 0 in all eight comparisons (max|sgs force| 4e-4 TGV, 2e-2 sphere)."""
    s = _sphere(w, dims) if body else _tgv(w, dims)
    U = (1.0, 0.0, 0.0) if body else (0.0, 0.0, 0.0)
    nu = s.nu
    s.set_sgs(CS, DELTA)
    s.mom_steps_(3)
    Ng = s.Ng
    mu0 = s.field("mu0")
    V = s.field("V") if body else np.zeros(Ng + (3,), np.float32, order="F")
    mu1 = s.field("mu1") if body else np.zeros(Ng + (3, 3), np.float32, order="F")
    s.update_()                                        # (handing out μ₀/μ₁/V invalidates the body masks until update!)
    dt = float(s.dt[-1])

    def expect(uadv, uin, u0, post):
        r, Phi = np.zeros(Ng + (3,), np.float32, order="F"), np.zeros(Ng, np.float32, order="F")
        oracle.conv_diff(r, uadv, Phi, nu=nu)
        f32, _, _ = sgs_ref.sgs(r, uadv, CS, DELTA, dtype=np.float32)
        f64, _, _ = sgs_ref.sgs(r, uadv, CS, DELTA, dtype=np.float64)
        e32 = float(np.abs(f32.astype(np.float64) - f64).max())
        force = float(np.abs(f64 - r).max())
        f32 = np.asfortranarray(f32)
        uo = uin.copy(order="F")
        oracle.BDIM(uo, u0, f32, V, mu0, mu1, dt)
        if post != 1.0:
            oracle.scale_u(uo, post)
        oracle.BC(uo, U)
        return uo, e32, force

    s.phase_(0)                                        # u⁰ .= u ; scale_u!(0)
    u0 = s.field("u0")
    s.phase_(1)
    uo, e32, force = expect(u0, np.zeros_like(u0), u0, 1.0)
    err = float(np.abs(s.field("u").astype(np.float64) - uo).max())
    print(f"dims {dims} body {body} predictor: e32 = {e32:.3e} Δt = {dt:.4f} bound = {4 * e32 * dt:.3e} device error = {err:.3e} max|sgs force| = {force:.3e}")
    assert force > 1e-6
    assert err <= 4 * e32 * dt, (err, e32, dt)
    s.phase_(2)
    up = s.field("u")
    s.phase_(3)
    uo, e32, force = expect(up, up, u0, 0.5)
    err = float(np.abs(s.field("u").astype(np.float64) - uo).max())
    print(f"dims {dims} body {body} corrector: e32 = {e32:.3e} Δt = {dt:.4f} bound = {4 * e32 * dt:.3e} device error = {err:.3e} max|sgs force| = {force:.3e}")
    assert force > 1e-6
    assert err <= 4 * e32 * dt, (err, e32, dt)


# ------------------------------------------------------------------------------------------------ 6. composite = leaves
def _rand_u(dims, seed=5):
    rng = np.random.default_rng(seed)
    Ng = tuple(n + 2 for n in dims)
    u = np.asfortranarray(rng.uniform(-0.3, 0.3, size=Ng + (3,)).astype(np.float32))
    u[..., 0] += 1.0
    return u


def test_composite_equals_the_leaf_path(w):
    """wl_sim_mom_step ×3 with the model on equals mom_step_(a, b, udf=sgs, Cs=…, Delta=…) on the leaf operations, bit for bit"""
    dims, uBC = (32, 32, 32), (1.0, 0.0, 0.0)
    u_init = _rand_u(dims)
    sl = w.Simulation(dims, uBC, dims[0], nu=0.02, u0=u_init)
    sf = w.FusedSimulation(dims, uBC, dims[0], U=1, nu=0.02, u0=u_init)
    sf.set_sgs(CS, DELTA)
    for step in range(3):
        w.mom_step_(sl.flow, sl.pois, udf=w.sgs, Cs=CS, Delta=DELTA)
        sf.mom_step_()
        du = float(np.abs(sf.field("u") - w.to_host(sl.flow.u)).max())
        dp = float(np.abs(sf.field("p") - w.to_host(sl.flow.p)).max())
        print(f"step {step}: max|Δu| = {du:.3e} max|Δp| = {dp:.3e} Δt {float(sf.dt[-1])!r} {float(sl.flow.dt[-1])!r}")
        assert np.array_equal(sf.field("u"), w.to_host(sl.flow.u)), step
        assert np.array_equal(sf.field("p"), w.to_host(sl.flow.p)), step
    assert [float(v) for v in sf.dt] == [float(v) for v in sl.flow.dt]
    assert sf.pois_n == sl.pois.n


def test_mom_steps_equals_single_steps(w):
    a, b = _tgv(w, (32, 32, 32)), _tgv(w, (32, 32, 32))
    a.set_sgs(CS, DELTA); b.set_sgs(CS, DELTA)
    a.mom_steps_(3)
    for _ in range(3):
        b.mom_step_()
    assert np.array_equal(a.field("u"), b.field("u")) and np.array_equal(a.field("p"), b.field("p"))
    assert np.array_equal(np.array(a.dt), np.array(b.dt))
    off = _tgv(w, (32, 32, 32)); off.mom_steps_(3)
    assert not np.array_equal(a.field("u"), off.field("u"))           # the model is not a no-op


@pytest.mark.parametrize("with_spare", [True, False])
def test_caller_owned_arrays_equal_handle_owned(w, with_spare):
    from test_gpu_callerowned import CallerOwnedSim
    dims, uBC = (32, 24, 40), (1.0, 0.0, 0.0)
    u_init = _rand_u(dims)
    ref = w.FusedSimulation(dims, uBC, dims[0], U=1, nu=0.02, u0=u_init)
    ref.set_sgs(CS, DELTA)
    sim = CallerOwnedSim(w, dims, uBC, 0.02, u_init, with_spare)
    sim.check(sim.lib.wl_sim_set_sgs(sim.h, 1, CS, DELTA))
    for step in range(3):
        ref.mom_step_(); sim.mom_step()
        assert np.array_equal(sim.field("u"), ref.field("u")), step
        assert np.array_equal(sim.field("u0"), ref.field("u0")), step
        assert np.array_equal(sim.field("p"), ref.field("p")), step
    assert [float(v) for v in sim.dt] == [float(v) for v in ref.dt]
    sim.close()


def test_exit_bc_and_periodic_directions_run_with_the_model(w, oracle):
    """convective exit and periodic directions take the same staged route: finite fields, and equal to the oracle's step with the yardstick
    spliced in is covered by the phase test; here the composite must equal the leaf path to rounding"""
    dims = (32, 24, 24)
    for kw in ({"exitBC": True}, {"perdir": (2, 3)}):
        u_init = _rand_u(dims)
        sl = w.Simulation(dims, (1.0, 0, 0), dims[0], nu=0.02, u0=u_init, **kw)
        sf = w.FusedSimulation(dims, (1.0, 0, 0), dims[0], U=1, nu=0.02, u0=u_init, **kw)
        sf.set_sgs(CS, DELTA)
        for step in range(2):
            w.mom_step_(sl.flow, sl.pois, udf=w.sgs, Cs=CS, Delta=DELTA)
            sf.mom_step_()
        u = sf.field("u")
        assert np.all(np.isfinite(u))
        assert np.abs(u - w.to_host(sl.flow.u)).max() < 5e-5, kw


# ------------------------------------------------------------------------------------------------ 7. udf dispatch (test/test_les.jl)
def test_udf_sees_the_advecting_velocity(w):
    """test/test_les.jl on the Python leaf path: a 3-argument udf is handed u⁰ in the predictor (flow.u is zeroed) and the projected u in
    the corrector; a 2-argument force runs once per phase"""
    saw = []
    inner = lambda t: t[1:-1, 1:-1, :]      # noqa: E731  inside_u(u); device arrays are indexed like the Julia arrays

    def rec(flow, u, t, **kw):
        saw.append((float(inner(u).abs().max()), float(inner(flow.u).abs().max())))

    sim = w.Simulation((16, 16), (1.0, 0.0), 16, U=1.0)
    sim.sim_step_(udf=rec)
    assert len(saw) == 2
    assert saw[0][0] > 1e-8          # predictor udf sees nonzero u⁰
    assert saw[0][1] < 1e-8          # while flow.u's interior is zeroed
    assert saw[-1][0] > 1e-8         # corrector udf sees the nonzero projected field
    NG = [0]

    def grav(flow, t, *, g=0.5):
        flow.f.add_(g); NG[0] += 1

    sim2 = w.Simulation((16, 16), (1.0, 0.0), 16, U=1.0)
    sim2.sim_step_(udf=grav, g=0.5)
    assert NG[0] == 2 and np.all(np.isfinite(w.to_host(sim2.flow.u)))


def test_constant_jerk_udf(w, oracle):
    """test/test_flow.jl:111-132: the body force t·jerk through the udf path, exact uₓ = uₓ₀ + ½·jerk·t² to its 1e-4"""
    N, jerk = 8, 4
    Us = math.sqrt(N)

    def gravity(flow, t, *, jerk=4):
        flow.f[..., 0].add_(float(t) * jerk)          # component 1 of f on every cell (helper.jl:34-36)

    sim = w.Simulation((N, N), (Us, 0.0), N, nu=0.001, dt=0.001, perdir=(1,))
    sim.sim_step_(1.0, udf=gravity, jerk=jerk)
    u = w.to_host(sim.flow.u)
    uFinal = np.float32(Us + 0.5 * jerk * float(sim.flow.time()) ** 2)
    assert oracle.L2(u[:, :, 0] - uFinal) < 1e-4 and oracle.L2(u[:, :, 1]) < 1e-4


# ------------------------------------------------------------------------------------------------ 8. it dissipates
def test_model_dissipates_energy(w):
    N = 64
    nu = N / 1e5
    ke = lambda u: 0.5 * float((u[1:-1, 1:-1, 1:-1].astype(np.float64) ** 2).sum())      # noqa: E731
    off, on = _tgv(w, (N, N, N), nu=nu), _tgv(w, (N, N, N), nu=nu)
    on.set_sgs(0.17, 1.0)
    off.mom_steps_(50); on.mom_steps_(50)
    uoff, uon = off.field("u"), on.field("u")
    nut = sgs_ref.smagorinsky(sgs_ref.strain(uon), np.float32(0.17), np.float32(1.0))
    print(f"max νₜ/ν = {float(nut.max()) / nu:.2f}   KE off = {ke(uoff):.6e}  KE sgs = {ke(uon):.6e}")
    assert float(nut.max()) / nu > 1
    for s in (off, on):
        assert all(np.all(np.isfinite(s.field(k))) for k in ("u", "p", "f", "sigma"))
    assert ke(uon) < ke(uoff)


# ------------------------------------------------------------------------------------------------ 9. rejections
def test_rejections(w):
    from waterlily_jl_amd._lib import ALLGATHER_FN, SENDRECV_FN, lib, wl_grid, wl_sim_desc
    from waterlily_jl_amd.slab import slab_grid
    L = lib()
    s3 = _tgv(w, (16, 16, 16))
    for model in (-1, 2, 7):
        assert L.wl_sim_set_sgs(s3._h, model, 0.17, 1.0) == WL_EINVAL
        assert L.wl_last_error_string()
    assert L.wl_sim_set_sgs(s3._h, 1, 0.17, 1.0) == 0 and L.wl_sim_set_sgs(s3._h, 0, 0.0, 1.0) == 0
    s2 = w.FusedSimulation((16, 16), (1.0, 0.0), 16)
    assert L.wl_sim_set_sgs(s2._h, 1, 0.17, 1.0) == WL_EINVAL
    assert b"3-D" in L.wl_last_error_string()
    with pytest.raises(w.WlError):
        s2.set_sgs(0.17)
    s2.mom_step_()                                                     # still an unmodelled 2-D step, as before
    # the leaf: a 2-D grid and a z-slab grid
    a2 = w.jl_zeros((10, 10, 2)); sg2 = w.jl_zeros((10, 10))
    g2 = w.core.vgrid(a2)
    assert L.wl_sgs(w.core.ptr(a2), w.core.ptr(sg2), w.core.ptr(a2), C.byref(g2), 0.17, 1.0, None) == WL_EINVAL
    gs = slab_grid((18, 18, 34), 0, 2)
    a3 = w.jl_zeros((gs.nx, gs.ny, gs.nz, 3)); sg3 = w.jl_zeros((gs.nx, gs.ny, gs.nz))
    assert L.wl_sgs(w.core.ptr(a3), w.core.ptr(sg3), w.core.ptr(a3), C.byref(gs), 0.17, 1.0, None) == WL_EINVAL
    assert b"slab" in L.wl_last_error_string()
    # a z-slab handle (rank 0 of 2; the transport does nothing: no step is taken)
    sr = SENDRECV_FN(lambda *a: 0); ag = ALLGATHER_FN(lambda *a: 0)
    comm = C.c_void_p()
    assert L.wl_comm_callbacks_create(C.byref(comm), 0, 2, None, C.cast(sr, C.c_void_p), C.cast(ag, C.c_void_p)) == 0
    d = wl_sim_desc()
    d.D = 3
    for k in range(3):
        d.dims[k] = (16, 16, 32)[k]
    d.nu, d.dt0 = 0.01, 0.25
    h = C.c_void_p()
    assert L.wl_sim_create_slab(C.byref(h), C.byref(d), comm) == 0
    assert L.wl_sim_set_sgs(h, 1, 0.17, 1.0) == WL_EINVAL
    assert b"slab" in L.wl_last_error_string()
    assert L.wl_sim_destroy(h) == 0 and L.wl_comm_destroy(comm) == 0


# ------------------------------------------------------------------------------------------------ 10. launch budget
def test_launch_budget(w):
    from waterlily_jl_amd._lib import lib
    L = lib()
    Ng = (34, 34, 34)
    f, sg, u = w.jl_zeros(Ng + (3,)), w.jl_zeros(Ng), w.jl_zeros(Ng + (3,))

    class A:
        pass
    a = A(); a.f, a.sigma = f, sg
    n0 = L.wl_launch_count()
    w.sgs_(a, u, CS, DELTA)
    assert L.wl_launch_count() - n0 <= 2
    per = {}
    for name in ("off", "on"):
        s = _tgv(w, (64, 64, 64))
        if name == "on":
            s.set_sgs(CS, DELTA)
        s.mom_steps_(2)
        n0 = L.wl_launch_count(); s.mom_steps_(4); per[name] = (L.wl_launch_count() - n0) / 4
    print(f"launches per mom_step! at 64³: sgs off {per['off']:.1f}, sgs on {per['on']:.1f}")
