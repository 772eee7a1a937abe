"""MeanFlow as an observer of a handle (wl_sim_set_meanflow, csrc/wl_meanflow.hip): the time averages P, U and the packed UU = ⟨u⊗u⟩ updated on the device
after every k-th completed step of wl_sim_mom_step / wl_sim_mom_steps.

1. the kernel against the NumPy Float32 restatement of tests/meanflow_ref.py on the smallest shapes that can go wrong (cs % 4 = 0 and 2 — a handle's cs is
   even; below, at and above whole workgroups; 2-D and 3-D; with and without UU): every cell, ghost cells included, as raw bits;
2. the observer inside ONE mom_steps_ call against the existing leaf (w.MeanFlow.update_ after single steps), as raw bits, every = 1 and every = 3;
3. the step is untouched: u, u⁰, p, Δt and pois.n of an observed handle, one stepped singly and read after every step, and one never observed;
4. the deferrals: "pdefer" stands down on the corrector of exactly the steps that end with an update, and an update costs exactly one launch;
5. the life cycle: reset, off, an immediate update, copy!(flow, meanflow), and the error paths."""
import ctypes as C

import numpy as np
import pytest

import meanflow_ref as mr

pytestmark = pytest.mark.gpu
f32 = np.float32
FUSED = dict(tailfuse=1, resjac_min=0, convt_min=0)      # at 64×32×24 the fused head, pdefer, tailfuse and lazydt are live (asserted below)
NEVER = 1 << 30                                          # a period no test reaches: the averages move by update_meanflow() alone


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    yield w
    w.lib().wl_reset_process_options()      # resjac_min / convt_min are process-wide


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def tbits(t):
    return [int(f32(v).view(np.uint32)) for v in t]


def same(a, b, what):
    x, y = bits(a), bits(b)
    assert x.shape == y.shape, (what, x.shape, y.shape)
    assert np.array_equal(x, y), (what, int((x != y).sum()), x.size)


def assert_same_state(a, b, what):
    for name in ("u", "u0", "p"):
        same(a.field(name), b.field(name), (what, name))
    assert tbits(a.dt) == tbits(b.dt), (what, [float(v) for v in a.dt], [float(v) for v in b.dt])
    assert a.pois_n == b.pois_n, (what, a.pois_n, b.pois_n)


def tgv(w, dims=(64, 32, 24), **opts):
    sg = w.FusedSimulation(dims, (0.0,) * len(dims), dims[0], U=1, nu=dims[0] / 1600.0, ic="tgv")
    for k, v in opts.items():
        sg.set_option(k, v)
    return sg


def sphere32(w):
    N, R = 32, 4.0
    sg = w.FusedSimulation((N, N, N), (1.0, 0.0, 0.0), 2 * R, U=1, nu=2 * R / 250, has_body=True)
    sg.measure_sphere_((N / 4, N / 2 - 1, N / 2 - 1), R, 1.0)
    return sg


def circle2d(w):
    n, m = 96, 64
    radius, center = m / 8, m / 2 - 1
    sg = w.FusedSimulation((n, m), (1.0, 0.0), 2 * radius, U=1, nu=2 * radius / 100, has_body=True)
    sg.measure_sphere_((center, center), radius, 1.0)
    return sg


CONFIGS = {"tgv64x32x24_fused": lambda w: tgv(w, **FUSED), "sphere32": sphere32, "circle96x64": circle2d}


def mean_host(w, sg):
    """(P, U, UU | None, t) of the observer on the host; UU expanded to (N…, D, D)"""
    P, U, UU, t = sg.meanflow()
    return w.to_host(P), w.to_host(U), (None if UU is None else w.to_host(UU)), t


class LeafFlow:
    """what w.MeanFlow reads of a flow — p, u, D, time() — taken from a handle's current fields"""

    def __init__(self, w, sg):
        self.w, self.sg, self.D = w, sg, sg.D
        self.refresh()

    def refresh(self):
        self.p, self.u = self.w.to_device(self.sg.field("p")), self.w.to_device(self.sg.field("u"))

    def time(self):
        return self.sg.time()


# ---- 1. kernel against restatement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("uu", [False, True], ids=["PU", "PUUU"])
@pytest.mark.parametrize("dims", mr.SHAPES, ids=["x".join(map(str, d)) for d in mr.SHAPES])
def test_kernel_equals_the_restatement_on_every_cell(w, dims, uu):
    D, Ng = len(dims), tuple(n + 2 for n in dims)
    u0, _ = mr.fields(dims, 7, 99)
    sg = w.FusedSimulation(dims, (0.0,) * D, dims[0], U=1, nu=0.05, u0=u0)
    sg.set_meanflow(uu_stats=uu, every=NEVER, t_init=0.0)
    assert sg.counter("mean_every") == NEVER
    ref = mr.MeanRef(Ng, 0.0, uu)
    ts = mr.times(mr.DT_HISTORY)
    for k in range(mr.N_UPDATES):
        w._lib.check(w.lib().wl_sim_set_dt_last(sg._h, float(mr.DT_HISTORY[k])))      # time(flow) advances by a Δt of the test's choosing
        sg.mom_step_()
        assert f32(sg.time()) == ts[k], (k, sg.time(), ts[k])
        u, p = mr.fields(dims, 7, k)
        sg.set_field("u", u)
        sg.set_field("p", p)
        sg.update_meanflow()
        ref.update(p, u, ts[k])
    assert sg.counter("mean_updates") == mr.N_UPDATES
    P, U, UU, t = mean_host(w, sg)
    print(f"[meanflow] {dims} cs {mr.cells(dims)} (cs % 4 = {mr.cells(dims) % 4}) uu {uu}: ε {[float(e) for e in ref.eps_log]}, max|P| {np.abs(P).max():.3f}, max|U| {np.abs(U).max():.3f}")
    assert tbits(t) == tbits(ref.t), (t, ref.t)
    same(P, ref.P, "P")
    same(U, ref.U, "U")
    assert np.abs(ref.P).max() > 0.05 and np.abs(ref.U).max() > 0.02 and all(0 < e < 1 for e in ref.eps_log[1:])
    if uu:
        same(UU, ref.UU, "UU")
        same(w.to_host(sg.meanflow_uu()), ref.uu(), "tau")
        assert np.abs(ref.UU).max() > 1e-3
    else:
        assert UU is None
        with pytest.raises(w.WlError, match="UU"):
            sg.meanflow_uu()


@pytest.mark.parametrize("dims", mr.NO_HANDLE, ids=["x".join(map(str, d)) for d in mr.NO_HANDLE])
def test_shapes_without_three_levels_have_no_handle(w, dims):
    """cs % 4 = 1 and 3 cannot be observed: a handle needs an even side (tests/meanflow_ref.py SHAPES)"""
    with pytest.raises(w.WlError, match="MultiLevelPoisson requires"):
        w.FusedSimulation(dims, (0.0,) * len(dims), dims[0], U=1, nu=0.05)


# ---- 2. observer against leaf -----------------------------------------------------------------------------------------------------------------------------
def leaf_run(w, B, steps, every):
    flow = LeafFlow(w, B)
    mf = w.MeanFlow(flow, uu_stats=True)
    for s in range(1, steps + 1):
        B.mom_step_()
        if s % every == 0:
            flow.refresh()
            mf.update_(flow)
    return mf


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_observer_equals_the_leaf_after_single_steps(w, cfg, every):
    steps = 7
    A, B = CONFIGS[cfg](w), CONFIGS[cfg](w)
    A.set_meanflow(uu_stats=True, every=every)
    A.mom_steps_(steps)
    mf = leaf_run(w, B, steps, every)
    assert A.counter("mean_updates") == steps // every and A.counter("mean_every") == every
    P, U, UU, t = mean_host(w, A)
    assert len(t) == 1 + steps // every and tbits(t) == tbits(mf.t), (t, mf.t)
    same(P, w.to_host(mf.P), (cfg, "P"))
    same(U, w.to_host(mf.U), (cfg, "U"))
    same(UU, w.to_host(mf.UU), (cfg, "UU"))
    same(w.to_host(A.meanflow_uu()), w.to_host(mf.uu()), (cfg, "tau"))
    assert np.isfinite(P).all() and np.abs(U).max() > 0.05 and np.abs(UU).max() > 1e-3
    assert_same_state(A, B, cfg)
    print(f"[meanflow] {cfg} every {every}: pdefer {A.counter('pdefer')}, tailfuse {A.counter('tailfuse')}, resjac {A.counter('resjac')}")
    if cfg == "tgv64x32x24_fused":
        # the deferred paths ran under the observer: every predictor tail skipped its store, and every corrector tail of a step without an update but the call's last
        due = steps // every
        assert A.counter("pdefer") == steps + (steps - due - (0 if steps % every == 0 else 1)) and A.counter("tailfuse") >= 1 and A.counter("resjac") >= 1


# ---- 3. the step is untouched -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [{}, FUSED], ids=["default", "fused"])
def test_the_step_is_untouched(w, opts):
    steps = 5
    A, B, Cc = tgv(w, **opts), tgv(w, **opts), tgv(w, **opts)
    A.set_meanflow(uu_stats=True, every=2)
    B.set_meanflow(uu_stats=True, every=2)
    A.mom_steps_(steps)
    Cc.mom_steps_(steps)
    for _ in range(steps):
        B.mom_step_()
        got = mean_host(w, B)
    assert_same_state(A, Cc, "observer vs none")
    assert_same_state(A, B, "one call vs single steps read after each")
    for x, y, name in zip(mean_host(w, A)[:3], got[:3], "P U UU".split()):
        same(x, y, name)
    assert tbits(A.meanflow_t()) == tbits(got[3]) and A.counter("mean_updates") == B.counter("mean_updates") == steps // 2


def test_the_step_is_untouched_on_caller_owned_arrays(w):
    from test_gpu_callerowned import CallerOwnedSim
    from waterlily_jl_amd.core import stream
    dims, uBC, steps = (64, 32, 24), (0.3, -0.2, 0.1), 5
    rng = np.random.default_rng(137)
    Ng = tuple(n + 2 for n in dims)
    u_init = np.asfortranarray(rng.uniform(-0.4, 0.4, size=Ng + (3,)).astype(f32))
    sims = [CallerOwnedSim(w, dims, uBC, 0.02, u_init, True) for _ in range(3)]
    A, B, Cc = sims
    L, check = A.lib, A.check
    for s in sims:
        for k, v in (("resjac_min", 0), ("convt_min", 0)):
            check(L.wl_sim_set_option(s.h, k.encode(), v))

    def follow(s):
        for role in s.role:
            s.role[role] = s._ptr2name[L.wl_sim_field(s.h, role.encode())]
        assert L.wl_sim_field(s.h, b"p") == w.core.ptr(s.arr["p"]).value      # the pressure is in the CALLER's array after every call
        out = (C.c_float * 64)()
        n = L.wl_sim_dt(s.h, out, 64)
        return tbits(out[:n])

    def raw_mean(s, which, ncomp):
        n = C.c_size_t(0)
        p = L.wl_sim_meanflow(s.h, which, C.byref(n))
        assert p and n.value == mr.cells(dims) * ncomp
        out = np.empty(n.value, dtype=f32)
        check(L.wl_d2h(out.ctypes.data_as(C.c_void_p), p, out.nbytes, stream()))
        return out

    for s in (A, B):
        check(L.wl_sim_set_meanflow(s.h, 2, 2, float("nan"), stream()))
    check(L.wl_sim_mom_steps(A.h, steps, stream()))
    check(L.wl_sim_mom_steps(Cc.h, steps, stream()))
    for _ in range(steps):
        B.mom_step()
        got = [raw_mean(B, q, nc) for q, nc in ((0, 1), (1, 3), (2, 6))]
    dts = [follow(s) for s in sims]
    assert dts[0] == dts[1] == dts[2], dts
    for name in ("u", "u0", "p"):
        same(A.field(name), Cc.field(name), ("caller-owned, observer vs none", name))
        same(A.field(name), B.field(name), ("caller-owned, one call vs single steps", name))
    assert A.pois_n() == B.pois_n() == Cc.pois_n()
    for q, nc in ((0, 1), (1, 3), (2, 6)):
        same(raw_mean(A, q, nc), got[q], ("caller-owned averages", q))
    v = C.c_long(0)
    check(L.wl_sim_counter(A.h, b"pdefer", C.byref(v)))
    assert v.value > 0, "pdefer was live on the observed caller-owned handle"
    for s in sims:
        s.close()


# ---- 4. deferrals and launches ----------------------------------------------------------------------------------------------------------------------------
def test_pdefer_stands_down_only_where_an_update_is_due(w):
    """per k-step call every predictor tail skips its store (k), and every corrector tail but the call's last (k − 1) — minus those of steps that end with an update"""
    # one call of 8 with every = 4: updates after steps 4 and 8; step 8's corrector stores anyway, step 4's stores because of the update
    A, Cc = tgv(w, **FUSED), tgv(w, **FUSED)
    A.set_meanflow(uu_stats=True, every=4)
    A.mom_steps_(8)
    Cc.mom_steps_(8)
    assert Cc.counter("pdefer") == 8 + 7
    assert A.counter("pdefer") == 8 + 6, A.counter("pdefer")      # the correctors of steps 1, 2, 3, 5, 6, 7
    assert A.counter("mean_updates") == 2
    assert_same_state(A, Cc, "every = 4, one call")
    # calls of 5 and 3: step 4 sits inside the first call (its corrector would have skipped), step 8 ends the second
    A2, C2 = tgv(w, **FUSED), tgv(w, **FUSED)
    A2.set_meanflow(uu_stats=True, every=4)
    rises = []
    for k in (5, 3):
        a0, c0 = A2.counter("pdefer"), C2.counter("pdefer")
        A2.mom_steps_(k)
        C2.mom_steps_(k)
        rises.append((A2.counter("pdefer") - a0, C2.counter("pdefer") - c0))
    assert rises == [(5 + 3, 5 + 4), (3 + 2, 3 + 2)], rises
    assert A2.counter("mean_updates") == 2
    assert_same_state(A2, C2, "every = 4, calls of 5 and 3")
    for x, y, name in zip(mean_host(w, A)[:3], mean_host(w, A2)[:3], "P U UU".split()):
        same(x, y, name)


def launches(sg, n):
    l0 = sg.counter("launches")
    sg.mom_steps_(n)
    return sg.counter("launches") - l0


@pytest.mark.parametrize("opts", [{}, FUSED], ids=["default", "fused"])
def test_an_update_costs_exactly_one_launch(w, opts):
    dims = (16, 16, 16) if not opts else (64, 32, 24)
    A, Cc = tgv(w, dims, **opts), tgv(w, dims, **opts)
    assert launches(A, 3) == launches(Cc, 3)                     # nothing registered: the same launches
    A.set_meanflow(uu_stats=True, every=1)
    la, lc = launches(A, 4), launches(Cc, 4)
    assert la - lc == 4, (la, lc)
    A.set_meanflow(uu_stats=False, every=4)
    la, lc = launches(A, 8), launches(Cc, 8)
    assert la - lc == 2, (la, lc)                                # steps 4 and 8; none on the six others
    la, lc = launches(A, 3), launches(Cc, 3)
    assert la - lc == 0, (la, lc)                                # steps 9, 10, 11: no update is due
    A.set_meanflow(None)
    assert launches(A, 2) == launches(Cc, 2)
    assert_same_state(A, Cc, "after registering and unregistering")


# ---- 5. life cycle ----------------------------------------------------------------------------------------------------------------------------------------
def test_life_cycle(w):
    sg = tgv(w, **FUSED)
    with pytest.raises(w.WlError, match="observer"):
        sg.meanflow()
    with pytest.raises(w.WlError, match="observer"):
        sg.update_meanflow()
    sg.set_meanflow(uu_stats=True, every=1)
    assert tbits(sg.meanflow_t()) == tbits([0.0])
    sg.mom_steps_(3)
    P, U, UU, t = mean_host(w, sg)
    assert len(t) == 4 and np.abs(U).max() > 0.05 and float(t[-1]) == sg.time()
    assert P.shape == sg.field("p").shape and U.shape == sg.field("u").shape and UU.shape == P.shape + (3, 3)
    # reset!
    sg.reset_meanflow(t_init=0.5)
    P, U, UU, t = mean_host(w, sg)
    assert not P.any() and not U.any() and not UU.any() and tbits(t) == tbits([0.5])
    assert sg.counter("mean_updates") == 3
    # the first update after a reset takes the instantaneous field; right after mom_steps_ it sees the materialised p
    sg.mom_steps_(2)                     # two observer updates …
    sg.reset_meanflow(t_init=sg.time())
    sg.update_meanflow()                 # … and an immediate one on the current u and p
    P, U, UU, t = mean_host(w, sg)
    same(P, sg.field("p"), "P after a first update")
    same(U, sg.field("u"), "U after a first update")
    assert tbits(t) == tbits([sg.time(), sg.time()])
    # copy!(flow, meanflow)
    sg.mom_steps_(3)
    P, U, _, _ = mean_host(w, sg)
    assert not np.array_equal(bits(U), bits(sg.field("u")))
    sg.load_meanflow_()
    same(sg.field("u"), U, "load: u")
    same(sg.field("p"), P, "load: p")
    # mode 1 keeps no UU
    sg.set_meanflow(uu_stats=False)
    assert sg.counter("mean_updates") == 0 and sg.meanflow()[2] is None
    with pytest.raises(w.WlError, match="UU"):
        sg.meanflow_uu()
    # off: a step performs no update
    sg.set_meanflow(None)
    sg.mom_step_()
    assert sg.counter("mean_updates") == 0 and sg.counter("mean_every") == 0
    with pytest.raises(w.WlError, match="observer"):
        sg.meanflow()
    with pytest.raises(ValueError):
        sg.set_meanflow(True, every=0)


def test_error_paths(w):
    from waterlily_jl_amd._lib import ALLGATHER_FN, SENDRECV_FN, wl_sim_desc
    L = w.lib()
    sg = tgv(w, (16, 16, 16))
    assert L.wl_sim_set_meanflow(sg._h, 3, 1, 0.0, None) == -1
    assert L.wl_sim_set_meanflow(sg._h, 1, 0, 0.0, None) == -1
    assert L.wl_sim_meanflow_uu(sg._h, None, 0, None) == -1
    assert not L.wl_sim_meanflow(sg._h, 0, None) and L.wl_sim_meanflow_t(sg._h, None, 0) == 0
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
    assert L.wl_sim_set_meanflow(h, 2, 1, 0.0, None) == -1 and b"slab" in L.wl_last_error_string()
    assert L.wl_sim_meanflow_update(h, None) == -1 and b"slab" in L.wl_last_error_string()
    assert L.wl_sim_destroy(h) == 0 and L.wl_comm_destroy(comm) == 0
