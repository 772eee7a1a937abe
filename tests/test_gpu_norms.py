"""r₁ and r∞ of solver!'s log on every route that forms them, against a float64 sum and a float32 maximum (tests/norms_ref.py) over the residual the same call
left behind; tests/test_norms_cpu.py shows on the oracle that the cases put their extreme where a reducer can lose it.

Per case (right-hand side = the scaled _rhs plus one spike, iteration cap k, tol = 1e-30 so that the cap ends the loop) and per route:
  * the last entry of wl_mg_last_log and the host_r1 / host_rinf of wl_mg_solve against r of level 0 read through wl_mg_level_field: r∞ = linf(r) as raw bits,
    |r₁ − l1(r)| ≤ l1(r)·(2⁻²⁴ + n·2⁻⁵³);
  * the first entry against the initial residual formed on the host (x = 0: r = z, minus the mean float32(Σz)/float32(N) where residual! applies it), same two
    comparisons — the routes differ in who forms it: shift_norms_dev, or the z-marching Jacobi! under defer_shift;
  * the whole log against the log of the passes route (one kernel per pass, norms_dev, shift_norms_dev) on the same input: r∞ and ω raw bits in every entry,
    r₁ within the bound, pois.n equal;
  * wl_mg_smoother_kind, wl_mg_shift_path and the counters say that the intended route ran.
Routes on the multigrid handle of a simulation (where the counters live), chosen with wl_mg_set_fused: see ROUTES.  The z-split runs on _zsplit_sim of
tests/test_gpu_mg_paths.py (three partial slots added on the host), 2-D and periodic handles and a default handle per shape on bare MultiLevelPoisson handles.
The x-only mode of kernel B exists only inside a time step: test_in_step_* runs default handles against the eager handle of tests/callseq.py on a random u⁰
and makes the comparisons on the last solve's log against pois_level("r"), once after a step that ended on a skipped store and once after one that stored.

The break test at its edge: solver! stops when r₁ < tol/10·N AND r∞ < tol (wl_mg::SolveRun::converged, k_decide: both, on the logged float32 values).  The
edge is taken on r∞ — with a spike r₁ is far inside its limit, which the test asserts first: tol = r∞ of iteration k must go on, tol = the next float above
must stop at k.  Inside mom_step! the tolerance is the reference's 2e-3 and not an argument, so the edge itself cannot be set there; what is checked in the
step is that the device's decision (tailspec) left the loop where the logged norms say: the last entry passes the test, no earlier one does, and pois.n, u, p
equal the tailspec = 0 handle's.

Observed on an MI355X: 0.1–0.5 s per case, 1.2–1.5 s for the passes and bare cases at 450×370×10 (README)."""
import ctypes as C
import math

import numpy as np
import pytest

import callseq
import norms_ref as nr
import test_gpu_mg_paths as mp
import test_gpu_rskip as rk

pytestmark = pytest.mark.gpu

f32 = np.float32
# name -> (wl_mg_set_fused bits, smoother kind of level 0, finest smooth! calls through the exchange buffer per iteration, x increment left to kernel B)
ROUTES = {
    "passes": (2, 0, 0, None),                 # bit0 off: one kernel per pass + norms_dev; "defer_shift" = 0: shift_norms_dev
    "onecell": (1 | 2 | 4, 1, 0, None),        # bit2: the one-cell blocked kernel B of wl_fused.hip
    "pair_W": (1 | 2, 2, 1, 1),                # the pair kernels, r′ and ϵ_mid through W
    "pair_dense": (1 | 2 | 256, 2, 0, 1),      # bit8: through the two dense arrays
    "pair_xA": (1 | 2 | 64, 2, 0, 0),          # bit6: kernel A applies the x increment
    "pair_eps": (1, 2, 0, 1),                  # the final ϵ stored: the EPS instance of kernel B
    "tail_off": (1 | 2 | 8, 2, 1, 1),          # bit3 / bit5: the coarse tails, which must not matter
    "tail_global": (1 | 2 | 32, 2, 1, 1),
}
SIM_SHAPES = ("66x34x26", "62x34x12", "66x66x18", "450x370x10")
BARE_SHAPES = {"66x34x26": 2, "62x34x12": 2, "66x66x18": 2, "450x370x10": 2, "66x34x34-periodic": 0, "34x34": 0, "130x18": 0}      # -> smoother kind


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    yield w
    _SIMS.clear()
    _REF.clear()
    w.lib().wl_reset_process_options()


_SIMS, _REF, _L1 = {}, {}, {}


def l1_of(r):
    key = hash(r.tobytes())
    if key not in _L1:
        if len(_L1) > 64:
            _L1.clear()
        _L1[key] = nr.l1(r)
    return _L1[key]


def bits64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def bits32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=f32)).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------------------- plumbing
def put(w, mg, name, a):
    lib, chk = w.lib(), w._lib.check
    a = np.asfortranarray(a, dtype=f32)
    chk(lib.wl_h2d(lib.wl_mg_level_field(mg, 0, name.encode()), a.ctypes.data_as(C.c_void_p), a.nbytes, w.core.stream()))
    chk(lib.wl_stream_sync(w.core.stream()))


def get(w, mg, name, shape):
    lib, chk = w.lib(), w._lib.check
    out = np.empty(shape, dtype=f32, order="F")
    chk(lib.wl_d2h(out.ctypes.data_as(C.c_void_p), lib.wl_mg_level_field(mg, 0, name.encode()), out.nbytes, w.core.stream()))
    chk(lib.wl_stream_sync(w.core.stream()))
    return out


def last_log(w, mg):
    cap = 80
    a, b, c = (C.c_double * cap)(), (C.c_double * cap)(), (C.c_double * cap)()
    k = w.lib().wl_mg_last_log(mg, a, b, c, cap)
    return np.array(a[:k]), np.array(b[:k]), np.array(c[:k])


def solve(w, mg, z, k, tol=1e-30, fused=None):
    """x = 0, the right-hand side z, solver!(tol, itmx = k) -> what it returned, its log, r of level 0"""
    lib, chk = w.lib(), w._lib.check
    if fused is not None:
        chk(lib.wl_mg_set_fused(mg, fused))
    put(w, mg, "x", np.zeros(z.shape, dtype=f32, order="F"))
    put(w, mg, "z", z)
    n, r1, rinf = C.c_int(), C.c_double(), C.c_float()
    chk(lib.wl_mg_solve(mg, float(tol), int(k), C.byref(n), C.byref(r1), C.byref(rinf), w.core.stream()))
    chk(lib.wl_stream_sync(w.core.stream()))
    return dict(n=int(n.value), r1=float(r1.value), rinf=f32(rinf.value), log=last_log(w, mg), r=get(w, mg, "r", z.shape), shift=int(lib.wl_mg_shift_path(mg)))


def initial_residual(z, perdir=()):
    """residual! at x = 0 on the host: r = z, minus the mean where it is due (wl_shift_mean / wl_shift_due of csrc/wl_common.hpp)"""
    inner = tuple(slice(1, n - 1) for n in z.shape)
    r = np.zeros(z.shape, dtype=f32, order="F")
    r[inner] = z[inner]
    s = f32(math.fsum(z[inner].astype(np.float64).ravel().tolist())) / f32(float(np.prod([n - 2 for n in z.shape])))
    if not abs(s) <= f32(2) * f32(1.1920929e-7):
        r[inner] = r[inner] - s
    return r


def check_against_r(what, r1, rinf, r):
    """one logged (r₁, r∞) against the field: raw bits and the derived bound; prints the figures first"""
    ref, n = l1_of(r), r.size
    err, bound = abs(float(r1) - ref), nr.r1_bound(ref, n)
    print(f"{what}: r∞ {float(rinf):.9e} vs {float(nr.linf(r)):.9e}; r₁ {float(r1):.12e} vs {ref:.12e}: |Δ| {err:.3e}, bound {bound:.3e}")
    assert nr.bits(rinf) == nr.bits(nr.linf(r)), (what, "rinf", float(rinf), float(nr.linf(r)))
    assert err <= bound, (what, "r1", float(r1), ref, err, bound)


def check_result(what, res, z, k, perdir=()):
    a, b, c = res["log"]
    assert res["n"] == k and len(a) == k + 1, (what, res["n"], len(a))
    check_against_r(what + " last entry", a[-1], b[-1], res["r"])
    check_against_r(what + " returned", res["r1"], res["rinf"], res["r"])
    check_against_r(what + " initial entry", a[0], b[0], initial_residual(z, perdir))
    assert float(c[0]) == 1.0


def check_logs(what, res, ref, ncells):
    """the route's log against the passes route's on the same input"""
    (a, b, c), (a0, b0, c0) = res["log"], ref["log"]
    assert res["n"] == ref["n"] and len(a) == len(a0), (what, res["n"], ref["n"])
    assert np.array_equal(bits64(b), bits64(b0)), (what, "rinf", b.tolist(), b0.tolist())
    assert np.array_equal(bits64(c), bits64(c0)), (what, "omega", c.tolist(), c0.tolist())
    eps = 2.0 ** -24 + ncells * 2.0 ** -53
    for q, (x, y) in enumerate(zip(a, a0)):      # the bound once, on the larger of the two (two float64 sums of the same terms, each rounded once to float32)
        assert abs(x - y) <= eps * max(x, y), (what, "r1", q, x, y)


def sim_for(w, sid):
    """one simulation handle per shape, only for its multigrid handle and its counters (the wall-bounded TGV: constant coefficients, no body)"""
    if sid not in _SIMS:
        if sid == "66x34x34-zsplit":
            _SIMS[sid] = mp._zsplit_sim(w)
        else:
            _SIMS[sid] = rk.make(w, tuple(n - 2 for n in nr.SHAPES[sid]["shape"]), None)
    return _SIMS[sid]


def cases_of(sid):
    e = nr.SHAPES[sid]
    return [(c, nr.rhs_with_spike(e["shape"], c[3])) for c in nr.CASES if c[0] == sid]


def reference(w, sid):
    """the passes route on every case of the handle, computed once"""
    if sid not in _REF:
        sim = sim_for(w, sid)
        mg = w.lib().wl_sim_pois(sim._h)
        sim.set_option("defer_shift", 0)
        out = {}
        for c, z in cases_of(sid):
            out[(c[3], c[4])] = solve(w, mg, z, c[4], fused=2 | 16)
            assert out[(c[3], c[4])]["shift"] == 0
        assert sim.smoother_kinds()[0] == 0
        sim.set_option("defer_shift", 1)
        w._lib.check(w.lib().wl_mg_set_fused(mg, 1 | 2))
        _REF[sid] = out
    return _REF[sid]


# --------------------------------------------------------------------------------------------------------------------------- bare solves
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("sid", SIM_SHAPES)
def test_route_log_against_its_own_residual_and_the_passes_log(w, sid, route):
    fused, kind, wide, xdefer = ROUTES[route]
    e = nr.SHAPES[sid]
    ref = reference(w, sid)
    sim = sim_for(w, sid)
    mg = w.lib().wl_sim_pois(sim._h)
    sim.set_option("defer_shift", 0 if route == "passes" else 1)
    try:
        for c, z in cases_of(sid):
            what = f"{sid} {route} spike {c[3]} k={c[4]}"
            c0 = {n: sim.counter(n) for n in ("abwide", "rskip", "rskip_redo", "resjac", "part")}
            res = solve(w, mg, z, c[4], fused=fused | (16 if route == "passes" else 0))
            assert sim.smoother_kinds()[0] == kind, (what, sim.smoother_kinds())
            assert res["shift"] == (0 if route == "passes" else 1), (what, res["shift"])
            assert sim.counter("abwide") - c0["abwide"] == wide * c[4], (what, "abwide", sim.counter("abwide") - c0["abwide"])
            if xdefer is not None:
                assert sim.counter("xdefer") == xdefer, (what, "xdefer")
            for n in ("rskip", "rskip_redo", "resjac", "part"):      # a bare solve is in no slot of a step: every r′ stored, no fused head, no plane ranges
                assert sim.counter(n) == c0[n], (what, n)
            check_result(what, res, z, c[4])
            check_logs(what, res, ref[(c[3], c[4])], z.size)
    finally:
        sim.set_option("defer_shift", 1)
        w._lib.check(w.lib().wl_mg_set_fused(mg, 1 | 2))
    assert nr.rows_of(e["shape"]) == (32 if e["tiling"] == "r32" else 16)


def test_zsplit_adds_three_partial_slots_on_the_host(w):
    sid = "66x34x34-zsplit"
    sim = sim_for(w, sid)
    assert sim.counter("part") == 1 and sim.smoother_kinds()[0] == 3
    za, zb = sim.counter("part_za"), sim.counter("part_zb")
    nz = nr.SHAPES[sid]["shape"][2]
    assert ((1, max(1, za - 4)), (max(1, za - 4), min(nz - 1, zb + 5)), (min(nz - 1, zb + 5), nz - 1)) == nr.ZSPLIT_RANGES, (za, zb)
    mg = w.lib().wl_sim_pois(sim._h)
    got = {}
    for c, z in cases_of(sid):      # the handle as _zsplit_sim left it
        what = f"{sid} zsplit spike {c[3]} k={c[4]}"
        a0 = sim.counter("abwide")
        got[(c[3], c[4])] = res = solve(w, mg, z, c[4])
        assert sim.smoother_kinds()[0] == 3 and sim.counter("abwide") == a0 and res["shift"] == 0, what
        check_result(what, res, z, c[4])
    ref = reference(w, sid)
    for c, z in cases_of(sid):
        check_result(f"{sid} passes spike {c[3]} k={c[4]}", ref[(c[3], c[4])], z, c[4])
        check_logs(f"{sid} zsplit spike {c[3]} k={c[4]}", got[(c[3], c[4])], ref[(c[3], c[4])], z.size)


@pytest.mark.parametrize("sid", list(BARE_SHAPES))
def test_bare_handle_default_route(w, sid):
    """MultiLevelPoisson as _bare builds it: 3-D the pair kernels with the final ϵ stored, periodic and 2-D the passes; against the handle itself with bit0 off"""
    e = nr.SHAPES[sid]
    ml, keep = mp._bare(w, e["shape"], perdir=e["perdir"])
    lib = w.lib()
    for c, z in cases_of(sid):
        what = f"{sid} bare spike {c[3]} k={c[4]}"
        res = solve(w, ml._h, z, c[4])
        assert int(lib.wl_mg_smoother_kind(ml._h, 0)) == BARE_SHAPES[sid], what
        assert res["shift"] == (1 if BARE_SHAPES[sid] == 2 else 0), (what, res["shift"])
        check_result(what, res, z, c[4], e["perdir"])
        assert ml.n[-1] == c[4]
        ref = solve(w, ml._h, z, c[4], fused=0)
        assert int(lib.wl_mg_smoother_kind(ml._h, 0)) == 0
        check_result(what + " (bit0 off)", ref, z, c[4], e["perdir"])
        check_logs(what, res, ref, z.size)
        w._lib.check(lib.wl_mg_set_fused(ml._h, 1))


# -------------------------------------------------------------------------------------------------------------------- the break test's edge
def test_break_test_at_its_edge_on_a_bare_handle(w):
    sid, k = "66x34x26", 2
    e = nr.SHAPES[sid]
    c = next(c for c in nr.CASES if c[0] == sid and c[4] == k)
    z = nr.rhs_with_spike(e["shape"], c[3])
    ninside = float(np.prod([n - 2 for n in e["shape"]]))

    def fresh(tol, itmx):
        ml, keep = mp._bare(w, e["shape"])
        return solve(w, ml._h, z, itmx, tol=tol)

    first = fresh(1e-30, k)
    a, b, _ = first["log"]
    edge = f32(b[k])
    up = np.nextafter(edge, f32(np.inf))
    print(f"edge: r∞ per entry {b.tolist()}, r₁ {a.tolist()}, r₁ limit at tol = r∞[k]: {float(edge) / 10.0 * ninside:.6e}")
    assert all(b[q] > float(up) for q in range(1, k)), "an earlier iteration would pass the r∞ test"
    assert a[k] < (float(edge) / 10.0) * ninside, "r₁ must be inside its limit, so that r∞ decides"
    on = fresh(float(edge), k + 2)            # r∞ < tol is false at iteration k: the loop goes on
    assert on["n"] > k, on["n"]
    assert np.array_equal(bits64(on["log"][1][:k + 1]), bits64(b)), "the same iterations up to k"
    stop = fresh(float(up), k + 2)            # the next float above: stops at k
    assert stop["n"] == k, stop["n"]
    assert np.array_equal(bits32(stop["r"]), bits32(first["r"]))


# ------------------------------------------------------------------------------------------------------------------------------ in a step
def step_log_checks(w, sg, what):
    """the last solve of the step: its last log entry against pois_level("r"); the loop left where the logged norms say"""
    mg = w.lib().wl_sim_pois(sg._h)
    a, b, c = last_log(w, mg)
    r = sg.pois_level("r")
    check_against_r(what, a[-1], b[-1], r)
    n = sg.pois_n[-1]
    assert len(a) == n + 1, (what, len(a), n)
    tol, ninside = 2e-3, float(np.prod(sg.dims))
    ok = [bool(float(f32(a[q])) < tol / 10.0 * ninside and b[q] < tol) for q in range(1, n + 1)]
    assert not any(ok[:-1]) and (ok[-1] or n == 32), (what, "break test", ok)
    return a, b, c


@pytest.mark.parametrize("dims", [rk.SMALL, rk.WIDE], ids=["66x34x26", "450x370x10"])
def test_in_step_logs_default_against_eager(w, oracle, dims):
    u0 = rk.random_u(oracle, dims, 71)
    on = rk.make(w, dims, u0, tailfuse_min=0)
    off = rk.make(w, dims, u0, tailfuse_min=0, **callseq.EAGER)
    seen = set()
    for step in range(10):
        for s in (on, off):
            s.mom_step_()
        stale = rk.policy(on.pois_n)[2]
        what = f"{'x'.join(map(str, dims))} step {step} pois.n {on.pois_n[-2:]} {'skipped' if stale else 'stored'}"
        if stale in seen:
            continue
        seen.add(stale)
        r0 = on.counter("rskip_redo")
        la = step_log_checks(w, on, what + " default")
        assert on.counter("rskip_redo") - r0 == (1 if stale else 0), (what, "the read of r launches the r-only instance iff the store was skipped")
        lb = step_log_checks(w, off, what + " eager")
        assert off.counter("rskip_redo") == 0 and off.counter("rskip") == 0
        check_logs(what, dict(n=on.pois_n[-1], log=la), dict(n=off.pois_n[-1], log=lb), int(np.prod([n + 2 for n in dims])))
        rk.assert_same_state(on, off, what)
        if len(seen) == 2:
            break
    assert seen == {True, False}, (seen, on.pois_n)
    assert on.smoother_kinds()[0] == 2 and on.counter("abwide") > 0 and on.counter("resjac") > 0 and on.counter("xdefer") == 1
    assert (on.counter("rskip"), on.counter("rskip_redo")) == (rk.policy(on.pois_n)[0], rk.policy(on.pois_n)[1] + 1)      # + the one read above
    assert on.counter("tailspec") <= on.counter("tailspec_armed") and off.counter("tailspec") == 0 and off.counter("tailspec_armed") == 0
    if dims == rk.SMALL:      # (the device's break test gating the queued tail: tests/test_gpu_speculation.py pins where it is armed)
        assert on.counter("tailspec") > 0


@pytest.mark.parametrize("option", ["rskip", "defer_shift", "resjac", "tailspec", "headspec", "xdefer"])
def test_in_step_logs_with_one_route_switched_off(w, oracle, option):
    """each in-step route off in turn: the logs of the last solve still match the residual, and the default handle's log entry by entry"""
    u0 = rk.random_u(oracle, rk.SMALL, 71)
    on, off = rk.make(w, rk.SMALL, u0), rk.make(w, rk.SMALL, u0, **{option: 0})
    for step in range(3):
        for s in (on, off):
            s.mom_step_()
        what = f"{option}=0 step {step} pois.n {off.pois_n[-2:]}"
        la, lb = step_log_checks(w, on, what + " default"), step_log_checks(w, off, what)
        check_logs(what, dict(n=off.pois_n[-1], log=lb), dict(n=on.pois_n[-1], log=la), int(np.prod([n + 2 for n in rk.SMALL])))
        rk.assert_same_state(on, off, what)
    if option != "headspec":      # (no counter of its own)  the fused head needs the folded mean shift: "defer_shift" = 0 takes it out
        assert off.counter("resjac" if option == "defer_shift" else option) == 0, option
    assert on.counter("rskip") > 0 and on.counter("resjac") > 0 and on.counter("tailspec") > 0 and on.counter("xdefer") == 1


def test_tailspec_leaves_the_loop_where_the_host_would(w, oracle):
    """the device's WL_RF_GO gates the queued tail: pois.n, u, p as with tailspec = 0, where the host alone decides — on the same logged norms"""
    u0 = rk.random_u(oracle, rk.SMALL, 71)
    on, off = rk.make(w, rk.SMALL, u0, tailspec=1), rk.make(w, rk.SMALL, u0, tailspec=0)
    for step in range(4):
        for s in (on, off):
            s.mom_step_()
        what = f"tailspec step {step}"
        la, lb = step_log_checks(w, on, what + " on"), step_log_checks(w, off, what + " off")
        for x, y in zip(la, lb):
            assert np.array_equal(bits64(x), bits64(y)), what      # the same kernels form both logs: every entry, r₁ included, as raw bits
        rk.assert_same_state(on, off, what)
    assert off.counter("tailspec") == 0 and off.counter("tailspec_armed") == 0
    assert 0 < on.counter("tailspec") <= on.counter("tailspec_armed") <= len(on.pois_n)


# --------------------------------------------------------------------------------------------------------------------------- the leaf
def leaf_positions(shape):
    """(name, index): first and last interior cell, the last interior cell of a plane's last (ragged) 256-cell block, either side of a block seam — k_norms
    reduces 256 consecutive in-plane cells (WL_BLOCK, m = i + j·nx) per block and strides the planes over the plane slots (csrc/wl_poisson.hip)"""
    nx, ny = shape[0], shape[1]
    D = len(shape)
    tail = lambda k: (() if D == 2 else (k,))
    klast = None if D == 2 else shape[2] - 2
    out = [("first", (1, 1) + tail(1)), ("last", (nx - 2, ny - 2) + tail(klast)), ("last of the last block, first plane", (nx - 2, ny - 2) + tail(1))]
    q = (nx * ny // 2) // 256
    while True:      # a seam with an interior cell on either side
        lo, hi = 256 * q - 1, 256 * q
        (il, jl), (ih, jh) = (lo % nx, lo // nx), (hi % nx, hi // nx)
        if 1 <= il <= nx - 2 and 1 <= ih <= nx - 2 and 1 <= jl <= ny - 2 and 1 <= jh <= ny - 2:
            break
        q += 1
    kmid = None if D == 2 else shape[2] // 2
    out += [("below a block seam", (il, jl) + tail(kmid)), ("above a block seam", (ih, jh) + tail(kmid))]
    return out


@pytest.mark.parametrize("shape", [(66, 34, 26), (450, 370, 10), (130, 18)], ids=["66x34x26", "450x370x10", "130x18"])
def test_leaf_norms_wherever_the_extreme_sits(w, shape):
    lib, chk = w.lib(), w._lib.check
    inner = tuple(slice(1, n - 1) for n in shape)
    base = np.zeros(shape, dtype=f32, order="F")
    base[inner] = (1e-3 * np.random.default_rng(17).standard_normal(tuple(n - 2 for n in shape))).astype(f32)
    for name, idx in leaf_positions(shape):
        for sign in (1.0, -1.0):
            a = base.copy(order="F")
            a[idx] = f32(sign)
            t = w.to_device(a)
            g = w.core.sgrid(t)
            l1, linf = C.c_double(), C.c_float()
            chk(lib.wl_norms(w.core.ptr(t), C.byref(g), C.byref(l1), C.byref(linf), None, w.core.stream()))
            check_against_r(f"{shape} {name} {idx} {sign:+.0f}", l1.value, f32(linf.value), a)
            assert float(linf.value) == 1.0
