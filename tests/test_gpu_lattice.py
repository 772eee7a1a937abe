"""Sampled distance-field bodies on the device (include/wlhip.h, sampled bodies): the lattice leaf of a body program at points, on linear data next to the plane
leaf, as measure! fields, under the set operations, on a handle (body-aware shortcuts against the general kernels, the force recorder) and the refusals —
which launch nothing.  The yardstick is tests/lattice_ref.py; the bound is the project's standing rule |device − ref64| ≤ 4·max|ref32 − ref64| over the case;
tests/test_lattice_cpu.py shows without a GPU that every case holds the classes of points it is here for.  Lattices of at most 20×18×16 samples, grids of at
most 32×16×16."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import forces_ref as fr
import lattice_ref as lr
from test_gpu_bodypaths import FAST, PLAIN, assert_same_state, handle, step, w  # noqa: F401  (w: the module-scoped fixture)

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
WL_EINVAL = -1


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def bake_values(w):
    """bake(body, dims, origin, spacing) -> the samples, taken on the device as SdfLattice.bake takes them (d alone, fastd² = 0)"""
    def bake(body, dims, origin, spacing):
        d, _, _ = w.bodies.measure(body, w.SdfLattice.centres(dims, origin, spacing), fastd2=0.0)
        return d.reshape(tuple(dims), order="F")
    return bake


@contextlib.contextmanager
def lattice(w, values):
    """a device lattice that also carries its samples for the restatement; closed on the way out (at most 8 are alive)"""
    lat = w.SdfLattice(values)
    lat.values = np.asarray(values, dtype=f32)
    try:
        yield lat
    finally:
        lat.close()


def check(name, what, dev, r32, r64):
    tol = lr.bound(r32, r64)
    err = float(np.abs(np.asarray(dev, dtype=f64) - r64).max(initial=0.0))
    print(f"[lattice] {name} {what}: max|dev − ref64| {err:.3e}, bound 4·max|ref32 − ref64| {tol:.3e}")
    assert err <= tol, (name, what, err, tol)


# ---- 1. points ----
@pytest.mark.parametrize("name", sorted(lr.POINT_CASES))
def test_points_against_the_restatement(w, name):
    c = lr.point_case(name, bake=bake_values(w))
    with lattice(w, c["values"]) as lat:
        b, X = c["body"](lat), c["X"]
        got = lr.classes(b, X, lr.FASTD2)
        for k in c["claims"]:
            assert got[k] >= 5, (name, k, got)
        q, _ = lr.lattice_coords(b, [X[:, k] for k in range(X.shape[1])])
        out = lr.clamp_active(q, lat.values.shape).any(axis=1)
        for fastd2 in (lr.FASTD2, np.inf):                       # (2+ϵ)² as measure! asks, and no early exit at all
            d, n, V = w.bodies.measure(b, X, fastd2=fastd2)
            d32, n32, V32 = lr.points(b, X, fastd2, f32)
            d64, n64, V64 = lr.points(b, X, fastd2, f64)
            raw = lr.points(b, X, -1.0, f32)[0]                  # (fastd² < 0: every point exits, d stays the sampled value)
            ex = raw * raw > f32(fastd2)                         # the early exits (most points outside the box among them): n = V = 0, d the raw value
            if fastd2 != np.inf:
                assert (ex & out).sum() >= 5 and (ex & ~out).sum() >= 5, name      # (as for the claimed classes: tests/test_lattice_cpu.py)
            assert np.array_equal(bits(d[ex]), bits(d32[ex])), (name, int((bits(d[ex]) != bits(d32[ex])).sum()))
            assert not n[ex].any() and not V[ex].any(), name
            # a point clamped in every direction that is not an early exit has g = 0: m = 0, n = 0/0 — in the reference, the restatement and on the device
            ok = ~ex & np.isfinite(n32).all(axis=1) & np.isfinite(n64).all(axis=1)
            bad = np.isnan(n).any(axis=1) != (~ex & np.isnan(n32).any(axis=1))
            assert not bad.any(), (name, X[bad][:3].tolist(), q[bad][:3].tolist(), n[bad][:3].tolist(), n32[bad][:3].tolist(), n64[bad][:3].tolist())
            assert ok.sum() >= 50 and np.abs(n[ok]).max(axis=1).min() > 0.1, name
            check(name, f"d (fastd² = {fastd2})", d[ok], d32[ok], d64[ok])
            check(name, f"n (fastd² = {fastd2})", n[ok], n32[ok], n64[ok])
            check(name, f"V (fastd² = {fastd2})", V[ok], V32[ok], V64[ok])


def test_bake_is_the_point_probe_at_fastd2_zero(w):
    c = lr.point_case("sphere", bake=bake_values(w))
    lat = w.SdfLattice.bake(c["src"](), c["dims"], c["origin"], c["spacing"])
    try:
        assert lat.dims == c["dims"] and lat.D == 3 and lat.id >= 1
        assert lat.edge_min == w.bodies.edge_min(c["values"])
        with lattice(w, c["values"]) as same:
            assert same.id == lat.id + 1                         # ids count up
            a = w.bodies.measure(c["body"](lat), c["X"], fastd2=lr.FASTD2)
            b = w.bodies.measure(c["body"](same), c["X"], fastd2=lr.FASTD2)
            for x, y in zip(a, b):
                assert np.array_equal(bits(x), bits(y))
    finally:
        lat.close()
    lat.close()                                                  # closing twice is harmless


# ---- 2. linear data ----
def test_linear_data_next_to_the_plane_leaf(w):
    """a lattice baked from a plane leaf at spacing 2: |∇sdf| = |m| ≠ 1, so d /= m does real work"""
    from waterlily_jl_amd.bodies import Body
    m, p0 = (0.6, -1.5, 0.8), (7.0, 6.0, 5.0)
    dims, origin, s = (10, 9, 8), (-1.0, 0.5, 0.0), 2.0
    plane = Body(("plane", p0, m))
    vals = bake_values(w)(plane, dims, origin, s)
    X = np.random.default_rng(1).uniform((0.0, 1.5, 1.0), (13.0, 13.5, 11.0), size=(200, 3)).astype(f32)
    with lattice(w, vals) as lat:
        b = lr.lattice_body(lat, origin, s)
        assert lr.classes(b, X)["inside"] == 200
        d, n, V = w.bodies.measure(b, X)
        dp, npl, _ = w.bodies.measure(plane, X)
        d32, n32, _ = lr.points(b, X, T=f32)
        d64, n64, _ = lr.points(b, X, T=f64)
        check("linear", "d", d, d32, d64)
        check("linear", "n", n, n32, n64)
        assert not V.any()
        # … and next to the plane leaf itself: the same plane, up to the rounding of the samples (values up to 30, Float32) carried through the differences
        mm = float(np.sqrt(sum(v * v for v in m)))
        # (at most 32 roundings — 8 samples, 8 products, 8 sums, the weights — each of a number below 32: half an ulp of it, 2⁻²⁰ … on g·s and on the value)
        r = 32 * 2.0 ** -20
        assert np.abs(vals).max() < 32 and np.abs(n - npl).max() <= r / s / mm * 2 and np.abs(d - dp).max() <= (r + r / s / mm * np.abs(dp).max()) / mm * 2


# ---- 3. fields ----
@pytest.mark.parametrize("name", sorted(lr.FIELD_CASES))
def test_fields_against_the_grid_restatement(w, name):
    c = lr.field_case(name, bake=bake_values(w))
    D, Ng = len(c["grid"]), c["Ng"]
    with lattice(w, c["values"]) as lat:
        b = c["body"](lat)
        got = lr.grid_classes(b, Ng)
        assert got["clamped"] > 100 and got["band"] > 50, got
        f = w.Flow(c["grid"], (1.0,) + (0.0,) * (D - 1))
        for k in ("mu0", "mu1", "V"):
            getattr(f, k).fill_(float("nan"))
        f.sigma.fill_(0.25)                                      # σ's ghost layer is not written (measure_sdf! is @inside): it keeps this
        w.measure_(f, b)
        dev = [w.to_host(getattr(f, k)) for k in ("sigma", "mu0", "mu1", "V")]
        r32 = lr.measure_fields(b, Ng, 1.0, f32, sigma_fill=0.25)
        r64 = lr.measure_fields(b, Ng, 1.0, f64, sigma_fill=0.25)
        ghost = ~fr.inside(Ng)
        for k, a, x32, x64 in zip(("sigma", "mu0", "mu1", "V"), dev, r32, r64):
            assert a.shape == x32.shape, (k, a.shape, x32.shape)
            assert np.array_equal(bits(a[ghost]), bits(x32[ghost])), (name, k, "ghost cells")
            check(name, k, a, x32, x64)
        assert (dev[1] < 1).sum() > 50 and np.abs(dev[2]).max() > 0.05 and (name != "sphere3" or np.abs(dev[3]).max() > 0.1)


# ---- 4. composition ----
@pytest.mark.parametrize("op", ["union_capsule", "minus_sphere"])
def test_composition_takes_the_winning_leaf_bit_for_bit(w, op):
    from waterlily_jl_amd.bodies import Body
    c = lr.point_case("sphere_mapped", bake=bake_values(w))
    with lattice(w, c["values"]) as lat:
        a = c["body"](lat)
        mp = a.map
        if op == "union_capsule":
            other = Body(("capsule", (13.0, 8.0, 7.0), 2.0, (1.0, 0.2, 0.0), 3.0), mp)
            both = a | other
        else:
            other = Body(("sphere", (12.0, 9.0, 7.5), 3.0), mp)
            both = a - other
        X = c["X"]
        D = X.shape[1]
        for fastd2 in (lr.FASTD2, np.inf):
            ta = np.concatenate([v.reshape(len(X), -1) for v in w.bodies.measure(a, X, fastd2=fastd2)], axis=1)
            tb = np.concatenate([v.reshape(len(X), -1) for v in w.bodies.measure(other, X, fastd2=fastd2)], axis=1)
            tc = np.concatenate([v.reshape(len(X), -1) for v in w.bodies.measure(both, X, fastd2=fastd2)], axis=1)
            if op == "minus_sphere":
                tb[:, :D + 1] = -tb[:, :D + 1]
            less = np.zeros(len(X), dtype=bool)
            eq = np.ones(len(X), dtype=bool)
            for k in range(2 * D + 1):                           # isless(b, a) on the tuples, lexicographic
                lq = fr._isless(tb[:, k], ta[:, k])
                less = np.where(eq, lq, less)
                eq = eq & ~lq & fr._isequal(tb[:, k], ta[:, k])
            takeb = less if op == "union_capsule" else ~less
            want = np.where(takeb[:, None], tb, ta)
            assert takeb.sum() >= 10 and (~takeb).sum() >= 10, (op, int(takeb.sum()))
            same = (bits(tc) == bits(want)) | (np.isnan(tc) & np.isnan(want))
            assert same.all(), (op, fastd2, np.argwhere(~same)[:4].tolist())


# ---- 5. a handle ----
def _case5():
    return dict(id="lattice_sphere", dims=(32, 16, 16), perdir=(), exitBC=False, lam=0, store_f=False)


def test_handle_fast_paths_and_force_records(w):
    c = lr.field_case("sphere3", bake=bake_values(w))
    case = _case5()
    x0 = (12.0, 8.0, 8.0)
    with lattice(w, c["values"]) as lat:
        fast, plain = handle(w, case, FAST), handle(w, case, PLAIN)
        hyb0 = fast.counter("hybrid")
        for k in range(5):                                       # the baked sphere moves with its map: remeasured before every step
            t = float(np.sum(fast.dt[:-1], dtype=f64))
            body = c["body"](lat, t)
            plain.measure_bodyset_(body, 1.0); step(plain, False)
            fast.measure_bodyset_(body, 1.0); step(fast, True)
            assert_same_state(fast, plain, ("lattice_sphere", k))
        assert fast.counter("hybrid") > hyb0 and plain.counter("hybrid") == 0
        assert float(np.abs(fast.field("u") - 0).max()) > 0.1
        # the recorder on one call of three steps against forces() after single steps
        body = c["body"](lat, float(np.sum(fast.dt[:-1], dtype=f64)))
        A, B = fast, plain
        A.measure_bodyset_(body, 1.0); B.measure_bodyset_(body, 1.0)
        A.set_force_record(body, x0=x0, capacity=8)
        active, nt, nb, _ = fr.band(body, c["Ng"])
        assert A.counter("force_tiles") == len(active) and 0 < len(active) < nt, (A.counter("force_tiles"), len(active), nt)
        step(A, True, 3, one_call=True)
        t_, pF, vF, pM, vM = A.read_forces()
        assert pF.shape == (3, 3)
        for r in range(3):
            step(B, False)
            want = np.concatenate(B.forces(body, x0=x0))
            tp, tv, tpm, tvm = fr.tolerances(body, B.field("p"), B.field("u"), B.nu, x0)
            tol = np.repeat([tp, tv, tpm, tvm], 3)
            rec = np.concatenate([pF[r], vF[r], pM[r], vM[r]])
            err = np.abs(rec - want)
            print(f"[lattice] record {r}: max|Δ| {err.reshape(4, 3).max(axis=1)}, tolerance {tol[::3]}, |pF| {np.linalg.norm(want[:3]):.3e}, n_b {nb}")
            assert np.all(err <= tol), (r, err, tol)
        assert np.linalg.norm(pF[-1]) > 1e-3
        assert_same_state(A, B, "recorder, one call vs single steps")
        A.set_force_record(None)
        del fast, plain, A, B


# ---- 6. refusals: host-side checks, nothing is launched, and the next valid call goes through ----
def test_refusals_launch_nothing(w):
    from waterlily_jl_amd import core
    from waterlily_jl_amd._lib import wl_bodyset
    L = w.lib()
    c = lr.field_case("sphere3", bake=bake_values(w))
    f = w.Flow(c["grid"], (1.0, 0.0, 0.0))
    g = core.sgrid(f.sigma)

    def measure_rc(prog, eps=1.0):
        return L.wl_measure_bodyset(core.ptr(f.sigma), core.ptr(f.mu0), core.ptr(f.mu1), core.ptr(f.V), C.byref(g), C.byref(prog), eps, 0, 0, None)

    def force_rc(prog):
        out = (C.c_double * 3)()
        return L.wl_pressure_force_bodyset(None, core.ptr(f.p), C.byref(g), C.byref(prog), out, None)

    def refused(call, reason):
        before = L.wl_launch_count()
        rc = call()
        assert rc == WL_EINVAL, (reason, rc)
        assert L.wl_launch_count() == before, reason
        msg = L.wl_last_error_string().decode()
        assert msg, reason
        return msg

    def create_rc(values, D=None, dims=None):
        a = np.asarray(values, dtype=f32)
        h = C.c_void_p()
        dims = a.shape if dims is None else dims
        rc = L.wl_sdf_lattice_create(C.byref(h), a.ndim if D is None else D, (C.c_int32 * len(dims))(*dims),
                                     np.ascontiguousarray(a.reshape(-1, order="F")).ctypes.data_as(C.POINTER(C.c_float)), None)
        assert rc != 0 and not h.value
        return rc

    with lattice(w, c["values"]) as lat:
        good = c["body"](lat)
        ok = lambda: measure_rc(good.program(3)) == 0 and force_rc(good.program(3)) == 0      # noqa: E731
        assert ok()
        # kind 4 with an unknown id
        prog = good.program(3); prog.node[0].h = float(lat.id + 1000)
        assert "unknown" in refused(lambda: measure_rc(prog), "unknown id") and ok()
        prog = good.program(3); prog.node[0].h = 0.0
        refused(lambda: measure_rc(prog), "id 0"); assert ok()
        prog = good.program(3); prog.node[0].h = float(lat.id) + 0.5
        refused(lambda: measure_rc(prog), "an id that is no integer"); assert ok()
        # m[0] ≤ 0
        for s in (0.0, -1.5):
            prog = good.program(3); prog.node[0].m[0] = s
            assert "m[0]" in refused(lambda: measure_rc(prog), "spacing") and ok()
        # the edge rule violated for measure! (edge_min − |R| ≤ 2 + ϵ + 1) but satisfied for the forces (> 2)
        off = lat.edge_min - 3.0
        assert off > 0 and lat.edge_min - off > 2
        edgy = lr.lattice_body(lat, c["origin"], c["spacing"], off, good.map)
        assert not w.bodies.lattice_margin_ok(edgy, 3, 4.0) and w.bodies.lattice_margin_ok(edgy, 3, 2.0)
        assert "edge_min" in refused(lambda: measure_rc(edgy.program(3)), "edge rule, measure!")
        before = L.wl_launch_count()
        assert force_rc(edgy.program(3)) == 0 and L.wl_launch_count() > before
        worse = lr.lattice_body(lat, c["origin"], c["spacing"], lat.edge_min - 1.0, good.map)
        refused(lambda: force_rc(worse.program(3)), "edge rule, forces"); assert ok()
        # a 3-D lattice in a 2-D program
        f2 = w.Flow((16, 16), (1.0, 0.0)); g2 = core.sgrid(f2.sigma)
        prog2 = wl_bodyset(); prog2.n = 1; prog2.node[0] = good.program(3).node[0]
        refused(lambda: L.wl_measure_bodyset(core.ptr(f2.sigma), core.ptr(f2.mu0), core.ptr(f2.mu1), core.ptr(f2.V), C.byref(g2), C.byref(prog2), 1.0, 0, 0, None), "3-D lattice, 2-D grid")
        # create: dims < 3, a NaN sample, D ∉ {2, 3}
        before = L.wl_launch_count()
        assert create_rc(np.ones((2, 5, 5))) == WL_EINVAL and "3" in L.wl_last_error_string().decode()
        bad = np.ones((4, 4, 4), dtype=f32); bad[1, 2, 3] = np.nan
        assert create_rc(bad) == WL_EINVAL and "finite" in L.wl_last_error_string().decode()
        bad[1, 2, 3] = np.inf
        assert create_rc(bad) == WL_EINVAL
        assert create_rc(np.ones(64), D=1, dims=(64,)) == WL_EINVAL and create_rc(np.ones(81), D=4, dims=(3, 3, 3, 3)) == WL_EINVAL
        # a ninth live lattice
        more = [w.SdfLattice(np.ones((3, 3, 3), dtype=f32)) for _ in range(7)]
        try:
            assert create_rc(np.ones((3, 3, 3))) == WL_EINVAL and "alive" in L.wl_last_error_string().decode()
            with pytest.raises(w.WlError):
                w.SdfLattice(np.ones((3, 3, 3), dtype=f32))
        finally:
            for m in more:
                m.close()
        assert L.wl_launch_count() == before and ok()
        ids = [m.id for m in more]
        assert ids == list(range(ids[0], ids[0] + 7)) and ids[0] > lat.id      # never reused
        # a handle whose force recorder names the lattice
        case = _case5()
        sim = handle(w, case, {})
        sim.measure_bodyset_(good, 1.0)
        sim.set_force_record(good, x0=(12.0, 8.0, 8.0), capacity=4)
        sim.mom_step_()
        assert sim.counter("force_records") == 1
        good_prog, dead_id = good.program(3), lat.id
    # … destroyed now: named by a fresh program
    refused(lambda: measure_rc(good_prog), "destroyed, fresh program")
    refused(lambda: force_rc(good_prog), "destroyed, fresh program, force")
    assert L.wl_sdf_lattice_id(None) == 0
    # … and by the handle's recorder at the next mom_step!
    n_dt = len(sim.dt)
    msg = refused(lambda: L.wl_sim_mom_step(sim._h, None), "destroyed, recorder")
    assert str(dead_id) in msg and len(sim.dt) == n_dt and sim.counter("force_records") == 1
    refused(lambda: L.wl_sim_mom_steps(sim._h, 2, None), "destroyed, recorder, mom_steps")
    out = (C.c_double * 12)()
    refused(lambda: L.wl_sim_forces_bodyset(sim._h, None, C.byref(good_prog), out, None), "destroyed, forces()")
    refused(lambda: L.wl_sim_measure_bodyset(sim._h, C.byref(good_prog), 1.0, None), "destroyed, measure!(sim)")
    # the handle goes on once the recorder has a body that is alive
    from waterlily_jl_amd.bodies import Body
    sphere = Body(("sphere", (12.0, 8.0, 8.0), 3.0))
    sim.set_body(sphere)                                         # measure!(sim): the recorder follows the body
    sim.mom_step_()
    assert len(sim.dt) == n_dt + 1 and sim.counter("force_records") == 2
    sim.set_force_record(None)
    sim.mom_step_()
    # and a new lattice of the same samples serves the same program under its new id
    with lattice(w, c["values"]) as again:
        assert again.id > dead_id
        assert measure_rc(c["body"](again).program(3)) == 0
