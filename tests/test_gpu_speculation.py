"""The speculative projection where its guess fails: residual!'s mean shift really due (src/Poisson.jl:95-97) behind the fused head with the
first V-cycle and the gated tail queued (headspec, tailspec), the back-off after three redos and its re-arming by update!, the forced redo
with the tail armed, solver!'s iteration cap (src/MultiLevelPoisson.jl:108) with the tail gated, and a bare solve after a discarded
speculation.  Every HIP mode against every other bit for bit, and against the oracle.

A shift is made due, or not, with one nonzero ∇·u: uBC = 0 and u_x on ONE outflow face equal to δ.  With p = 0 the residual is that
spike, Σr = δ exactly in any summation order, and the decision is float32(δ)/float32(N) against 2eps (tests/test_mean_shift_threshold.py
pins it on the oracle)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

f32 = np.float32
NU = 0.02


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    return w


def shift_edge(n):
    """(largest float32 δ with float32(δ)/float32(n) ≤ 2eps, the next float above it): the shift is not due / due"""
    n, lim, inf = f32(n), f32(2) * np.finfo(f32).eps, f32(np.inf)
    d = f32(lim * n)
    while d / n > lim:
        d = np.nextafter(d, f32(0))
    while np.nextafter(d, inf) / n <= lim:
        d = np.nextafter(d, inf)
    return d, np.nextafter(d, inf)


def spike_u(dims, delta):
    u = np.zeros(tuple(n + 2 for n in dims) + (3,), dtype=f32, order="F")
    u[dims[0] + 1, dims[1] // 2, dims[2] // 2, 0] = delta        # the outflow face of one (j,k): ∇·u = δ in cell (nx, j, k) only
    return u


def unbalanced_u(oracle, dims, seed):
    """a random field that satisfies BC!(u,0) except on the outflow face, where the flux is positive everywhere: Σ∇·u/N ≫ 2eps"""
    rng = np.random.default_rng(seed)
    u = np.asfortranarray(rng.uniform(-0.4, 0.4, size=tuple(n + 2 for n in dims) + (3,)).astype(f32))
    oracle.BC(u, (0.0, 0.0, 0.0))
    u[dims[0] + 1, 1:-1, 1:-1, 0] = rng.uniform(0.01, 0.05, size=(dims[1], dims[2])).astype(f32)
    return u


def sim(w, dims, u, **opts):
    """a handle on uBC = 0 whose u is exactly `u` (the constructor's BC! would remove the outflow flux: u is written afterwards)"""
    sg = w.FusedSimulation(dims, (0.0, 0.0, 0.0), dims[0], U=1, nu=NU)
    sg.set_option("resjac_min", 0)
    sg.set_option("convt_min", 0)
    for k, v in opts.items():
        sg.set_option(k, v)
    sg.set_field("u", u)
    return sg


def oracle_sim(oracle, dims, u, **kw):
    so = oracle.Simulation(dims, (0.0, 0.0, 0.0), dims[0], U=1, nu=NU, T=f32, **kw)
    so.field("u")[...] = u
    so.field("u0")[...] = u
    return so


def snap(sg):
    return (sg.field("u"), sg.field("u0"), sg.field("p"), sg.pois_n, [float(v) for v in sg.dt])


def assert_same(a, b, what):
    assert a[3] == b[3] and a[4] == b[4], (what, a[3], b[3])
    for q in range(3):
        assert np.array_equal(a[q], b[q]), (what, ("u", "u0", "p")[q])


def counters(sg):
    return {k: sg.counter(k) for k in ("resjac", "resjac_redo", "resjac_backoff", "tailspec", "tailspec_armed")}


def mg_log(w, mg):
    cap = 80
    a, b, c = (C.c_double * cap)(), (C.c_double * cap)(), (C.c_double * cap)()
    k = w.lib().wl_mg_last_log(mg, a, b, c, cap)
    return np.array(a[:k]), np.array(b[:k]), np.array(c[:k])


def sim_log(w, sg):
    return mg_log(w, w.lib().wl_sim_pois(sg._h))


def first_l1_says_due(l1, delta, N):
    """the first logged L₁ of a spike: |δ| unshifted, |δ − s| + (N−1)|s| ≈ 2|δ| shifted"""
    d = abs(float(delta))
    if l1 == d:
        return False
    s = abs(float(f32(delta) / f32(N)))
    assert abs(l1 - ((d - s) + (N - 1) * s)) < 1e-4 * d, (l1, d)
    return True


# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [(34, 34, 34), (66, 18, 10), (130, 18)])
@pytest.mark.parametrize("Lkind", ["one", "random"])
def test_mean_shift_threshold_in_the_standalone_solver(w, oracle, N, Lkind):
    """wl_mg_solve on a residual at the shift's edge — a spike at the largest δ that is not due, the float below and above it, both signs — and on a random z
    with mean 1e-3 (due): per iteration as test_solver_matches_oracle_per_iteration, and the same decision.  L ≡ 1 on 3-D levels: the shift is deferred into the
    finest level's z-marching Jacobi! (k_jacobi_march_cl<1>), and bit for bit with the pass of its own; a random L (and 2-D): the pass (k_shift_norms).
    The random z: Σr is a sum of 10⁴ terms, which the kernels add in Float64 and the reference in Float32 pairwise (k_mean_shift) — the shifts differ in
    their last bits and that constant moves x along the null space of the Neumann operator (a constant), so x is compared with its mean removed there."""
    rng = np.random.default_rng(83)
    D = len(N)
    n_in = int(np.prod([n - 2 for n in N]))
    lo, hi = shift_edge(n_in)
    below = np.nextafter(lo, f32(0))
    if Lkind == "one":
        L = np.ones(N + (D,), dtype=f32, order="F")
    else:
        L = np.asfortranarray(rng.uniform(0.2, 1.0, size=N + (D,)).astype(f32))
    oracle.BC(L, (0,) * D)
    sl = tuple(slice(1, -1) for _ in range(D))
    spike = tuple(n // 2 for n in N)
    cases = [(f32(s * d), due) for s in (1, -1) for d, due in ((below, False), (lo, False), (hi, True))] + [("random", True)]
    for delta, due in cases:
        z = np.zeros(N, dtype=f32, order="F")
        x0 = np.zeros(N, dtype=f32, order="F")
        if isinstance(delta, str):
            zz = rng.uniform(-1, 1, size=tuple(n - 2 for n in N)).astype(f32)
            z[sl] = zz - zz.mean() + f32(1e-3)
            x0 = np.asfortranarray(rng.uniform(-1, 1, size=N).astype(f32))
        else:
            z[spike] = delta
        xo, Lo, zo = x0.copy(order="F"), L.copy(order="F"), z.copy(order="F")
        po = oracle.MultiLevelPoisson(xo, Lo, zo)
        xg, Lg, zg = w.to_device(x0), w.to_device(L), w.to_device(z)
        pg = w.MultiLevelPoisson(xg, Lg, zg)
        no, ng = po.solve(), pg.solver_()
        r1o, rio, wo = po.log()
        r1g, rig, wg = pg.log()
        what = (Lkind, "random" if isinstance(delta, str) else float(delta))
        assert pg.shift_path() == (1 if (Lkind == "one" and D == 3) else 0), what
        assert ng == no, what
        assert np.allclose(r1g, r1o, rtol=2e-4) and np.allclose(rig, rio, rtol=2e-3, atol=1e-6) and np.array_equal(wg, wo), what
        xh = w.to_host(xg)
        if isinstance(delta, str):
            dx = (xh - xo)[sl]
            assert np.abs(dx - dx.mean()).max() < 1e-5 * max(1.0, np.abs(xo).max()), what
        else:       # a spike: Σr = δ exactly on both sides
            assert np.allclose(xh, xo, rtol=0, atol=1e-5 * max(1.0, np.abs(xo).max())), what
            assert first_l1_says_due(r1g[0], delta, n_in) == due and first_l1_says_due(r1o[0], delta, n_in) == due, what
        if Lkind == "one" and D == 3:       # the deferred shift against its own pass (process-wide switch; the conftest restores it)
            w.FusedSimulation((16, 16, 16), (0, 0, 0), 16, U=1, nu=0.01).set_option("jacobi_march", 0)
            xp = w.to_device(x0)
            pp = w.MultiLevelPoisson(xp, w.to_device(L), w.to_device(z))
            assert pp.solver_() == ng and pp.shift_path() == 0, what
            assert all(np.array_equal(a, b) for a, b in zip(pp.log(), (r1g, rig, wg))) and np.array_equal(w.to_host(xp), xh), what
            w.lib().wl_reset_process_options()


# ------------------------------------------------------------------------------------------------------------------------------------
MODES = {                     # option sets of the projection: every one must give the same bits
    "default": {},                                        # fused head, first V-cycle queued before Σr is read, tail gated on the device
    "tailspec0": {"tailspec": 0},
    "headspec0": {"headspec": 0},                         # fused head, Σr read before the V-cycle is queued
    "twokernel": {"resjac": 0, "defer_shift": 1},         # two-kernel head, shift inside the finest Jacobi!
    "twokernel_pass": {"resjac": 0, "defer_shift": 0},    # two-kernel head, shift in a pass of its own
}


@pytest.mark.parametrize("dims", [(64, 32, 32), (70, 44, 18), (128, 36, 12)])
@pytest.mark.parametrize("case", ["edge", "above", "unbalanced"])
def test_projection_with_a_due_mean_shift(w, oracle, dims, case):
    """mom_project! (phase 2) on a spike at the shift's edge (not due: the fused head and its speculative solve stand) and one float above it (due: the device
    withholds the gated tail, the loop breaks, the solve is discarded and the two-kernel head runs), and on a random u with an unbalanced boundary flux: every
    mode bit for bit on u, u⁰, p with the same pois.n and Δt; the counters of the default mode; the oracle."""
    N = int(np.prod(dims))
    lo, hi = shift_edge(N)
    delta = {"edge": lo, "above": hi, "unbalanced": None}[case]
    u = unbalanced_u(oracle, dims, 89) if case == "unbalanced" else spike_u(dims, delta)
    due = case != "edge"
    res = {}
    for mode, opts in MODES.items():
        sg = sim(w, dims, u, **opts)
        sg.phase_(2)
        res[mode] = snap(sg)
        if delta is not None:
            assert first_l1_says_due(sim_log(w, sg)[0][0], delta, N) == due, mode
        if mode == "default":
            c = counters(sg)
            assert c["tailspec_armed"] == 1, c
            if due:
                assert (c["resjac"], c["resjac_redo"], c["tailspec"]) == (0, 1, 0), c
            else:
                assert (c["resjac"], c["resjac_redo"], c["tailspec"]) == (1, 0, 1), c
                assert res[mode][3][-1] < 32, "the solve at the edge must converge before the cap"
    for mode in MODES:
        assert_same(res[mode], res["default"], mode)
    so = oracle_sim(oracle, dims, u)
    so.phase(2)
    assert res["default"][3] == so.pois_n
    assert np.abs(res["default"][0] - so.u).max() < 5e-5 and np.abs(res["default"][2] - so.p).max() < 5e-4


# ------------------------------------------------------------------------------------------------------------------------------------
def test_back_off_after_three_real_redos_and_update_rearms(w, oracle):
    """three projections in a row whose shift is really due (not the test hook) switch the fused head off for the handle; the fourth takes the two-kernel head
    at once; update! switches it back on and the head of a balanced projection stands again — all bit for bit with a handle that never fuses the head."""
    dims = (64, 32, 32)
    u_unb = unbalanced_u(oracle, dims, 97)
    rng = np.random.default_rng(101)
    u_bal = np.asfortranarray(rng.uniform(-0.4, 0.4, size=tuple(n + 2 for n in dims) + (3,)).astype(f32))
    oracle.BC(u_bal, (0.0, 0.0, 0.0))
    sg = sim(w, dims, u_unb)
    ref = sim(w, dims, u_unb, resjac=0)
    so = oracle_sim(oracle, dims, u_unb)
    for k in range(4):
        for s in (sg, ref):
            s.set_field("u", u_unb)
            s.phase_(2)
        so.field("u")[...] = u_unb
        so.phase(2)
        assert_same(snap(sg), snap(ref), k)
        assert snap(sg)[3] == so.pois_n, k
        c = counters(sg)
        assert c["resjac"] == 0 and c["resjac_redo"] == min(k + 1, 3) and c["resjac_backoff"] == (1 if k >= 2 else 0), (k, c)
        assert c["tailspec_armed"] == min(k + 1, 3) and c["tailspec"] == 0, (k, c)
    assert np.abs(sg.field("u") - so.u).max() < 5e-5 and np.abs(sg.field("p") - so.p).max() < 5e-4
    for s in (sg, ref):
        s.update_()
    assert sg.counter("resjac_backoff") == 0
    for s in (sg, ref):
        s.set_field("u", u_bal)
        s.phase_(2)
    assert_same(snap(sg), snap(ref), "balanced")
    c = counters(sg)
    assert c["resjac"] == 1 and c["resjac_redo"] == 3 and c["resjac_backoff"] == 0 and c["tailspec_armed"] == 4, c


# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(64, 32, 24), (128, 48, 12)])
def test_forced_redo_keeps_the_tail_armed(w, oracle, dims):
    """the resjac=2 hook declares the shift due on the device (k_decide), so inside mom_step! the gated tail stays armed and is withheld on every solve, as with a
    real shift — single steps and mom_steps_(n) batches (lazydt on), and resjac=3 (the redo not announced to the BC! deferral): bit for bit with resjac=0 and
    with single steps, and the oracle."""
    rng = np.random.default_rng(103)
    Ng = tuple(n + 2 for n in dims)
    uBC = (0.3, -0.2, 0.1)
    u_init = np.asfortranarray(rng.uniform(-0.4, 0.4, size=Ng + (3,)).astype(f32))
    oracle.BC(u_init, uBC)
    res = {}
    nstep = 5
    for mode, (rj, batch) in {"rj0": (0, False), "rj2": (2, False), "rj2_batch": (2, True), "rj3_batch": (3, True)}.items():
        sg = w.FusedSimulation(dims, uBC, dims[0], U=1, nu=NU, u0=u_init)
        sg.set_option("convt_min", 0)
        sg.set_option("resjac_min", 0)
        sg.set_option("lazydt", 1)
        sg.set_option("resjac", rj)
        if batch:
            sg.mom_steps_(3)
            sg.mom_steps_(2)
        else:
            for _ in range(nstep):
                sg.mom_step_()
        res[mode] = snap(sg)
        c = counters(sg)
        if rj:      # every head redone (the hook does not count toward the back-off), the gated tail armed and withheld on every discarded solve
            assert c["resjac"] == 0 and c["resjac_redo"] == 2 * nstep and c["tailspec"] == 0 and c["resjac_backoff"] == 0, (mode, c)
            assert c["tailspec_armed"] == 2 * nstep if rj == 2 else c["tailspec_armed"] >= nstep, (mode, c)
    for mode in ("rj2", "rj2_batch", "rj3_batch"):
        assert_same(res[mode], res["rj0"], mode)
    so = oracle.Simulation(dims, uBC, dims[0], U=1, nu=NU, T=f32)
    so.field("u")[...] = u_init
    so.field("u0")[...] = u_init
    for _ in range(nstep):
        so.step(remeasure=False)
    assert res["rj2"][3] == so.pois_n
    assert np.abs(res["rj2"][0] - so.u).max() < 5e-5 and np.abs(res["rj2"][2] - so.p).max() < 5e-4


# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("itmx", [1, 2, 3])
def test_iteration_cap_with_the_speculative_tail(w, oracle, itmx):
    """solver!'s cap below what the first solves need (the random field of test_tail_queued_ahead_of_the_convergence_read_is_bit_identical): with the tail
    gated, a solve that stops at the cap has not run it and launches it after the read — once.  tailspec/headspec on and off bit for bit; every pois.n ≤ itmx
    and one = itmx; the gated tail ran for exactly the solves whose last iteration passed the break test; the oracle with the same cap."""
    dims = (64, 32, 24)
    rng = np.random.default_rng(71)
    Ng = tuple(n + 2 for n in dims)
    uBC = (0.3, -0.2, 0.1)
    u_init = np.asfortranarray(rng.uniform(-0.4, 0.4, size=Ng + (3,)).astype(f32))
    oracle.BC(u_init, uBC)
    nstep = 4

    def make(**opts):
        sg = w.FusedSimulation(dims, uBC, dims[0], U=1, nu=NU, u0=u_init)
        sg.set_option("convt_min", 0)
        sg.set_option("resjac_min", 0)
        sg.set_option("itmx", itmx)
        for k, v in opts.items():
            sg.set_option(k, v)
        return sg

    res = {}
    for ts in (1, 0):
        for hs in (1, 0):
            sg = make(tailspec=ts, headspec=hs)
            for _ in range(nstep):
                sg.mom_step_()
            res[(ts, hs)] = snap(sg)
            if (ts, hs) == (1, 1):
                c11 = counters(sg)
            else:       # the tail is armed only behind the early V-cycle (headspec) and only with tailspec
                assert sg.counter("tailspec") == 0 and sg.counter("tailspec_armed") == 0, (ts, hs)
    for k in res:
        assert_same(res[k], res[(1, 1)], k)
    n = res[(1, 1)][3]
    assert len(n) == 2 * nstep and max(n) <= itmx and itmx in n, n
    # the same steps phase by phase: the log of every solve says whether its last iteration passed the break test (the numbers the host and k_decide compare);
    # a solve whose head was redone ran unarmed (its log is the redo's)
    sp = make()
    r1tol = (2e-3 / 10.0) * float(np.prod(dims))
    converged = []
    for _ in range(nstep):
        for ph in range(6):
            redo = sp.counter("resjac_redo")
            sp.phase_(ph)
            if ph in (2, 4):
                r1, rinf, _ = sim_log(w, sp)
                converged.append(bool(r1[-1] < r1tol and rinf[-1] < 2e-3) and sp.counter("resjac_redo") == redo)
    assert sp.pois_n == n
    assert sp.counter("tailspec") == sum(converged) and sp.counter("tailspec_armed") == 2 * nstep, (converged, counters(sp))
    assert c11["tailspec"] == sum(converged) and c11["tailspec_armed"] == 2 * nstep, (converged, c11)
    assert not all(converged), "the cap must stop some solve"
    so = oracle.Simulation(dims, uBC, dims[0], U=1, nu=NU, T=f32, itmx=itmx)
    oracle.BC(u_init, uBC)
    so.field("u")[...] = u_init
    so.field("u0")[...] = u_init
    for _ in range(nstep):
        so.step(remeasure=False)
    assert so.pois_n == n
    assert np.abs(res[(1, 1)][0] - so.u).max() < 5e-5 and np.abs(res[(1, 1)][2] - so.p).max() < 5e-4


# ------------------------------------------------------------------------------------------------------------------------------------
def test_bare_solve_after_a_discarded_speculation(w, oracle):
    """a projection whose speculative solve was discarded (shift due), then solver! on the handle's own MultiLevelPoisson (wl_mg_solve on wl_sim_pois): a plain
    solve — no projection tail runs (u unchanged), the shift is applied by the solve itself — equal to the oracle's solve of the same x, L and z."""
    dims = (64, 32, 32)
    sg = sim(w, dims, unbalanced_u(oracle, dims, 107))
    sg.phase_(2)
    c0 = counters(sg)
    assert c0["resjac_redo"] == 1 and c0["tailspec_armed"] == 1 and c0["tailspec"] == 0, c0
    lib, chk = w.lib(), w._lib.check
    mg = lib.wl_sim_pois(sg._h)
    Ng = tuple(n + 2 for n in dims)

    def level(name):
        shape = Ng + (3,) if name == "L" else Ng
        out = np.empty(shape, dtype=f32, order="F")
        chk(lib.wl_d2h(out.ctypes.data_as(C.c_void_p), lib.wl_mg_level_field(mg, 0, name.encode()), out.nbytes, w.core.stream()))
        return out

    rng = np.random.default_rng(109)
    z = np.zeros(Ng, dtype=f32, order="F")
    z[1:-1, 1:-1, 1:-1] = rng.uniform(-1e-2, 1e-2, size=dims).astype(f32) + f32(1e-4)      # the level's z is scratch of the step (σ): a due shift
    chk(lib.wl_h2d(lib.wl_mg_level_field(mg, 0, b"z"), z.ctypes.data_as(C.c_void_p), z.nbytes, w.core.stream()))
    chk(lib.wl_stream_sync(w.core.stream()))
    x, L = level("x"), level("L")
    u_before = sg.field("u")
    po = oracle.MultiLevelPoisson(x.copy(order="F"), L.copy(order="F"), z.copy(order="F"))
    no = po.solve()
    n, r1, rinf = C.c_int(), C.c_double(), C.c_float()
    chk(lib.wl_mg_solve(mg, 2e-3, 32, C.byref(n), C.byref(r1), C.byref(rinf), w.core.stream()))
    assert np.array_equal(sg.field("u"), u_before)
    assert counters(sg) == c0
    assert lib.wl_mg_shift_path(mg) in (0, 1)
    assert n.value == no
    r1o, rio, wo = po.log()
    r1g, rig, wg = mg_log(w, mg)
    assert np.allclose(r1g, r1o, rtol=2e-4) and np.allclose(rig, rio, rtol=2e-3, atol=1e-6) and np.array_equal(wg, wo)
    xo = po.x
    assert np.allclose(level("x"), xo, rtol=0, atol=1e-5 * max(1.0, np.abs(xo).max()))
