"""The unscaled pressure that is not stored between the solves of a time step (option "pdefer", csrc/wl_pdefer.hpp): a projection tail whose p = x/Δt is read
next by the fused projection head of the same call skips the store, and that head forms fl(fl(x/Δt_prev)·Δt) on load.  A handle with pdefer=1 against a handle
with pdefer=0 — u, u⁰, p on every cell (ghosts included) as raw bits, pois.n and the Δt history — over single-step and multi-step calls, with p read between
the calls, with the speculation switched off piecewise, on the redo paths (the pending division materialised before the two-kernel head) and with the first tail
inside the corrector's loader; and the counter says the stores were really skipped: 2k − 1 per k-step call, none where the option has to stand down."""
import numpy as np
import pytest

from callseq import assert_same_state, bits      # u, u⁰, p on every cell as raw bits, pois.n, the Δt history

pytestmark = pytest.mark.gpu

f32 = np.float32
DIMS = (64, 32, 24)      # with ghosts 66 × 34 × 26: the smallest shape class the fused head takes (nx ≥ 66 and even, ny ≥ 34), whole tiles for "tailfuse"


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    yield w
    w.lib().wl_reset_process_options()      # resjac_min / convt_min are process-wide


def tgv(w, dims=DIMS, **opts):
    sg = w.FusedSimulation(dims, (0.0,) * len(dims), dims[0], U=1, nu=dims[0] / 1600.0, ic="tgv")
    sg.set_option("resjac_min", 0)
    sg.set_option("convt_min", 0)
    for k, v in opts.items():
        sg.set_option(k, v)
    return sg


def run_calls(w, sg, calls):
    """the calls one after the other; per call the launches it made and the rise of the counter"""
    out = []
    for k in calls:
        l0, c0 = w.lib().wl_launch_count(), sg.counter("pdefer")
        if k == 0:
            sg.mom_step_()          # wl_sim_mom_step
        else:
            sg.mom_steps_(k)        # wl_sim_mom_steps
        out.append((w.lib().wl_launch_count() - l0, sg.counter("pdefer") - c0))
    return out


# skipped stores per k-step call: every tail but the last (k = 0 stands for a wl_sim_mom_step call: one step)
def expected(k):
    return 2 * max(k, 1) - 1


MODES = {
    "default": ({}, True),
    "tailspec0": ({"tailspec": 0}, True),
    "headspec0": ({"headspec": 0}, True),
    "redo_announced": ({"resjac": 2}, False),     # the handle knows its heads will be redone: no head is "fused" for the predicate, every tail stores
    "redo_unannounced": ({"resjac": 3}, True),    # the tails skip, every head is discarded: x/Δt_prev is materialised before the two-kernel head, every time
    "tailfuse": ({"tailfuse": 1}, True),          # the predictor's tail launches nothing: u −= L∇x in the corrector's loader, p left to the corrector's head
    "lazydt0": ({"lazydt": 0}, True),
}


SHORT, LONG = [(1,), (2,)], [(5,), (0, 3, 0, 0, 2)]      # k per call; 0 = one wl_sim_mom_step
CASES = [(m, c) for m in MODES for c in (SHORT + LONG if m in ("default", "redo_unannounced") else LONG)]


@pytest.mark.parametrize("mode,calls", CASES, ids=[m + "-" + "_".join(map(str, c)) for m, c in CASES])
def test_pdefer_is_bit_identical(w, mode, calls):
    opts, live = MODES[mode]
    on, off = tgv(w, pdefer=1, **opts), tgv(w, pdefer=0, **opts)
    for q, k in enumerate(calls):
        (lon, con), = run_calls(w, on, (k,))
        (loff, coff), = run_calls(w, off, (k,))
        print(f"{mode} call {q} k={k}: pdefer counter +{con} (off: +{coff}), launches {lon} vs {loff}")
        assert coff == 0, (mode, q)
        assert con == (expected(k) if live else 0), (mode, q, k, con)
        # launches: a skipped store is part of a tail launch that runs anyway (or, with "tailfuse", a launch less), so the count never rises — except where every
        # head is discarded: there each skipped store comes back as the one element-wise x/Δt_prev launch that materialises it before the two-kernel head
        assert lon <= loff + (con if mode == "redo_unannounced" else 0), (mode, q, "launches", lon, loff)
        if mode == "tailfuse":
            assert lon == loff - max(k, 1), (q, lon, loff)      # the predictor's tail launched p = x/Δt alone: gone
        assert_same_state(on, off, (mode, q, k))          # reads p (wl_sim_field) between the calls
    if mode == "tailfuse":
        assert on.counter("tailfuse") == off.counter("tailfuse") == sum(max(k, 1) for k in calls)
    nsolve = 2 * sum(max(k, 1) for k in calls)
    for c in ("resjac", "resjac_redo"):
        assert on.counter(c) == off.counter(c), c
    if mode.startswith("redo"):
        assert on.counter("resjac") == 0 and on.counter("resjac_redo") == nsolve


def test_pdefer_on_ragged_tiles(w):
    """a shape whose tiles and z-chunks are ragged (the head's halo cells take the division too)"""
    dims = (70, 44, 18)
    on, off = tgv(w, dims, pdefer=1), tgv(w, dims, pdefer=0)
    for s in (on, off):
        s.mom_steps_(4)
    assert on.counter("pdefer") == 7 and off.counter("pdefer") == 0
    assert_same_state(on, off, dims)


def test_pdefer_after_p_was_written_from_outside(w):
    """p set by the caller with nonzero ghost cells (the head's ghost-shell pass runs, and takes the pending division like the march does)"""
    rng = np.random.default_rng(131)
    Ng = tuple(n + 2 for n in DIMS)
    p0 = np.asfortranarray(rng.uniform(-1, 1, size=Ng).astype(f32))
    on, off = tgv(w, pdefer=1), tgv(w, pdefer=0)
    for s in (on, off):
        s.set_field("p", p0)
        s.mom_steps_(3)
    assert on.counter("pdefer") == 5
    assert_same_state(on, off, "p from outside")


def test_pdefer_stands_down(w):
    """the option is live only where the next reader of p is the fused head: not with the sgs model (staged sequence), not in 2-D (no fused head), not below the
    head's size gate, not in wl_sim_phase — and the results are those of pdefer=0 there too"""
    on, off = tgv(w, pdefer=1), tgv(w, pdefer=0)
    for s in (on, off):
        s.set_sgs(0.17, 1.0)
        s.mom_steps_(3)
    assert on.counter("pdefer") == 0
    assert_same_state(on, off, "sgs")
    for s in (on, off):      # model off again on the same handles: the option comes back
        s.set_sgs(None)
        s.mom_steps_(2)
    assert on.counter("pdefer") == 3 and off.counter("pdefer") == 0
    assert_same_state(on, off, "sgs off again")

    d2 = (128, 64)
    on2, off2 = tgv(w, d2, pdefer=1), tgv(w, d2, pdefer=0)
    for s in (on2, off2):
        s.mom_steps_(3)
    assert on2.counter("pdefer") == 0
    assert_same_state(on2, off2, "2-D")

    ph = tgv(w, pdefer=1)
    ref = tgv(w, pdefer=0)
    for s in (ph, ref):
        for k in range(6):
            s.phase_(k)
    assert ph.counter("pdefer") == 0
    assert_same_state(ph, ref, "phases")
    ph.mom_steps_(2)         # … and a call after the phases defers again
    ref.mom_steps_(2)
    assert ph.counter("pdefer") == 3
    assert_same_state(ph, ref, "steps after phases")


def test_pdefer_lands_in_a_caller_owned_p(w):
    """caller-owned arrays (the Julia binding's mode): the pressure must be in the CALLER's p after every call, so the stores that are skipped come in pairs —
    2(k − 1) per k-step call, none in a single step — and u, u⁰, p, pois.n, Δt equal the handle-owned pdefer=0 run"""
    import ctypes as C
    from test_gpu_callerowned import CallerOwnedSim
    from waterlily_jl_amd.core import stream
    rng = np.random.default_rng(137)
    Ng = tuple(n + 2 for n in DIMS)
    uBC = (0.3, -0.2, 0.1)
    u_init = np.asfortranarray(rng.uniform(-0.4, 0.4, size=Ng + (3,)).astype(f32))
    ref = w.FusedSimulation(DIMS, uBC, DIMS[0], U=1, nu=0.02, u0=u_init)
    for k, v in (("resjac_min", 0), ("convt_min", 0), ("pdefer", 0)):
        ref.set_option(k, v)
    sim = CallerOwnedSim(w, DIMS, uBC, 0.02, u_init, True)
    lib, check = sim.lib, sim.check

    def counter():
        v = C.c_long(0)
        check(lib.wl_sim_counter(sim.h, b"pdefer", C.byref(v)))
        return int(v.value)

    for k in (3, 1, 2, 4):
        c0 = counter()
        check(lib.wl_sim_mom_steps(sim.h, k, stream()))
        ref.mom_steps_(k)
        assert counter() - c0 == 2 * (k - 1), (k, counter() - c0)
        for role in sim.role:
            sim.role[role] = sim._ptr2name[lib.wl_sim_field(sim.h, role.encode())]
        assert lib.wl_sim_field(sim.h, b"p") == w.core.ptr(sim.arr["p"]).value, k
        for name in ("u", "u0", "p"):
            assert np.array_equal(bits(sim.field(name)), bits(ref.field(name))), (k, name)
        out = (C.c_float * 64)()
        n = lib.wl_sim_dt(sim.h, out, 64)
        assert [f32(v).view(np.uint32) for v in out[:n]] == [f32(v).view(np.uint32) for v in ref.dt], k
        assert sim.pois_n() == ref.pois_n, k
    sim.close()
