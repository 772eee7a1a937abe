"""Deforming mesh bodies on the device (include/wlhip.h, deforming meshes; csrc/wl_meshsdf.hip k_meshsdf<D, true>, csrc/wl_lattice.hpp lattice_grad_vel): the
velocity samples wl_sdf_lattice_from_moving_mesh makes against the NumPy restatement (tests/meshvel_ref.py) within the project's standing rule
|device − ref64| ≤ 4·max|ref32 − ref64| on every sample off the medial axis, its distances against wl_sdf_lattice_from_mesh and the culled search against the
brute-force flag as raw bits; re-baking in place (wl_sdf_lattice_update_mesh, advance) against a fresh lattice as raw bits; the leaf through the point probe on
linear velocity samples; a translation described by the map and by the vertices; a breathing sphere on a handle, shortcuts against the general kernels bit for
bit with a force recorder that keeps recording; the refusals, which launch nothing and change nothing.  tests/test_meshvel_cpu.py shows without a GPU that
the cases hold what they are here for.  Lattices of at most 30×30×16 samples, 1280 triangles, grids of at most 64×32×24.

Whether the device equals the Float32 restatement bit for bit is printed per case by test_velocity_samples (see its docstring)."""
import ctypes as C

import numpy as np
import pytest

import forces_ref as fr
import lattice_ref as lr
import meshsdf_ref as mr
import meshvel_ref as mv
from test_gpu_bodypaths import PLAIN, assert_same_state, handle, w  # noqa: F401  (w: the module-scoped fixture)

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
WL_EINVAL = -1
FP, IP = C.POINTER(C.c_float), C.POINTER(C.c_int32)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def pairs(w):
    a, b = C.c_uint64(), C.c_uint64()
    assert w.lib().wl_meshsdf_last_pairs(C.byref(a), C.byref(b)) == 0
    return int(a.value), int(b.value)


def from_case(w, c, brute=False, moving=True, V=None, Wv=None):
    return w.SdfLattice.from_mesh(c["V"] if V is None else V, c["E"], c["dims"], c["origin"], c["spacing"], brute=brute,
                                  vertex_velocity=(c["Wv"] if Wv is None else Wv) if moving else None)


def state(lat):
    return bits(lat.values()), (bits(lat.velocity()) if lat.has_velocity else None), np.float32(lat.edge_min).view(np.uint32)


def same_state(a, b):
    return np.array_equal(a[0], b[0]) and (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(a[1], b[1])) and a[2] == b[2]


# ---- samples ----
@pytest.mark.parametrize("name", sorted(mv.CASES))
def test_velocity_samples(w, name):
    """Measured on the MI355X: the device's W equals the Float32 restatement bit for bit on every sample of every case (the printed count of differing
    samples is 0), as its distances do; the bound below is what the project's rule asks."""
    c = mv.case(name)
    D = c["D"]
    r32, r64 = mv.ref(name, "f32"), mv.ref(name, "f64")
    ok = ~mv.ambiguous(name)
    tol = 4 * mv.gap(name)
    with from_case(w, c) as lat:
        tested, total = pairs(w)
        assert lat.has_velocity and lat.D == D
        Wd, d = lat.velocity(), lat.values()
        assert Wd.shape == c["dims"] + (D,) and Wd.dtype == f32
        err = float(np.abs(Wd.astype(f64) - r64["W"])[ok].max())
        nb = int((bits(Wd) != bits(r32["W"])).any(axis=-1).sum())
        print(f"[meshvel] {name}: max|W_dev − W_ref64| off the medial axis {err:.3e}, bound 4·max|W_ref32 − W_ref64| {tol:.3e}; samples whose W differs from "
              f"ref32 in bits: {nb} of {d.size} ({int(((bits(Wd) != bits(r32['W'])).any(axis=-1) & ok).sum())} of them off the medial axis); "
              f"ambiguous {int((~ok).sum())}; pairs tested {tested} of {total}")
        assert err <= tol, (name, err, tol)
        with from_case(w, c, moving=False) as static:                 # the distances: those of the static call, bit for bit
            assert not static.has_velocity
            assert np.array_equal(bits(static.values()), bits(d)) and static.edge_min == lat.edge_min
            with pytest.raises(w.WlError, match="no velocity"):
                static.velocity()
        with from_case(w, c, brute=True) as brute:                    # culled = brute on distances and W
            tb, total_b = pairs(w)
            assert np.array_equal(bits(brute.values()), bits(d)), name
            assert np.array_equal(bits(brute.velocity()), bits(Wd)), (name, int((bits(brute.velocity()) != bits(Wd)).sum()))
        assert tb == total_b == total == d.size * len(c["E"]) and tested <= total
        if name in ("torus-linear", "ico1280-rotation"):
            assert tested < total, (name, tested, total)


@pytest.mark.parametrize("name", ["cube-linear", "ico80-radial", "cube-3x3x3-rotation", "foil2d-wave"])
def test_a_uniform_vertex_velocity_is_stored_exactly(w, name):
    c = mv.case(name)
    U = mv.uniform(c["V"])
    with from_case(w, c, Wv=U) as lat:
        Wd = lat.velocity()
        assert np.array_equal(bits(Wd), bits(np.broadcast_to(U[0], Wd.shape)))


# ---- re-bake ----
def _moved(c, k=1):
    ctr = c["V"].astype(f64).mean(axis=0)
    return (ctr + (c["V"].astype(f64) - ctr) * (1 + 0.03 * k) + 0.11 * k).astype(f32)


@pytest.mark.parametrize("name", ["ico80-radial", "foil2d-wave"])
def test_update_mesh_equals_a_fresh_lattice(w, name):
    c = mv.case(name)
    V1, W1 = _moved(c), mv.linear(c["V"])
    with from_case(w, c) as lat:
        id0, s0 = lat.id, state(lat)
        lat.update_mesh(V1, W1)
        with from_case(w, c, V=V1, Wv=W1) as fresh:
            assert same_state(state(lat), state(fresh)) and lat.id == id0 != fresh.id
        assert not same_state(state(lat), s0) and np.array_equal(lat.vertices, V1)
        lat.update_mesh(c["V"], c["Wv"])                              # back: the original bits
        assert same_state(state(lat), s0) and lat.id == id0
        lat.update_mesh(V1)                                           # no velocities given: zeros
        with from_case(w, c, V=V1, moving=False) as still:
            assert not lat.velocity().any() and np.array_equal(state(lat)[0], bits(still.values()))
        # advance(new, dt) is update_mesh(new, (new − old)/dt)
        lat.update_mesh(c["V"], c["Wv"])
        dt = 0.37
        lat.advance(V1, dt)
        s_adv = state(lat)
        lat.update_mesh(c["V"], c["Wv"])
        lat.update_mesh(V1, ((V1 - c["V"]) / f32(dt)).astype(f32))
        assert same_state(state(lat), s_adv) and np.abs(lat.velocity()).max() > 0.1


def test_twenty_updates_take_no_table_entry(w):
    c = mv.case("cube-3x3x3-rotation")
    others = [from_case(w, c, moving=False) for _ in range(w.bodies.LATTICE_MAX - 1)]
    try:
        with from_case(w, c) as lat:                                   # the eighth
            for k in range(20):
                lat.update_mesh(_moved(c, k % 3), c["Wv"])
            assert lat.id == others[-1].id + 1
            with pytest.raises(w.WlError, match="alive"):              # … and still eight alive: a ninth is refused
                from_case(w, c)
        with from_case(w, c) as again:                                 # one closed: the next goes through, ids were not spent by the updates
            assert again.id == others[-1].id + 2
    finally:
        for m in others:
            m.close()


# ---- the leaf, through the point probe ----
A_LIN, B_LIN = mv._A, (0.3, -0.2, 0.1)


def _check(name, what, dev, r32, r64):
    tol = lr.bound(r32, r64)
    err = float(np.abs(np.asarray(dev, dtype=f64) - r64).max(initial=0.0))
    print(f"[meshvel] {name} {what}: max|dev − ref64| {err:.3e}, bound 4·max|ref32 − ref64| {tol:.3e}")
    assert err <= tol, (name, what, err, tol)


@pytest.mark.parametrize("name", ["sphere", "sphere_mapped", "spacing_half", "spacing_two", "capsule2d"])
def test_leaf_velocity_at_points(w, name):
    """linear velocity samples attached with set_velocity — no mesh involved: unmapped, under a rotated map with V and ω, at spacings ½ and 2, in 2-D; the
    point sets of tests/lattice_ref.py hold points clamped outside the box in one, two and three directions"""
    c = lr.point_case(name)
    D = len(c["dims"])
    Wl = mv.linear_W(c["dims"], c["origin"], c["spacing"], A_LIN, B_LIN)
    X = c["X"]
    with w.SdfLattice(c["values"]) as lat:
        body = c["body"](lat)
        plain = [bits(v) for v in w.bodies.measure(body, X, fastd2=lr.FASTD2)]
        p32 = lr.points(mv.host_twin(body, c["values"], None), X, lr.FASTD2, f32)
        assert not lat.has_velocity
        lat.set_velocity(Wl)
        assert lat.has_velocity and np.array_equal(bits(lat.velocity()), bits(Wl))
        twin = mv.host_twin(body, c["values"], Wl)
        q, _ = lr.lattice_coords(twin, [X[:, k] for k in range(D)])
        out = lr.clamp_active(q, c["values"].shape).any(axis=1)
        for fastd2 in (lr.FASTD2, np.inf):
            d, n, V = w.bodies.measure(body, X, fastd2=fastd2)
            d32, n32, V32 = mv.points(twin, X, fastd2, f32)
            d64, n64, V64 = mv.points(twin, X, fastd2, f64)
            raw = lr.points(twin, X, -1.0, f32)[0]
            ex = raw * raw > f32(fastd2)
            assert not bits(n[ex]).any() and not bits(V[ex]).any(), name          # n = V = +0 past fastd², bit for bit
            ok = ~ex & np.isfinite(n32).all(axis=1) & np.isfinite(n64).all(axis=1)
            assert ok.sum() >= 50 and (ok & out).sum() >= (5 if fastd2 == np.inf else 0), (name, int(ok.sum()), int((ok & out).sum()))
            _check(name, f"V (fastd² = {fastd2})", V[ok], V32[ok], V64[ok])
            _check(name, f"n (fastd² = {fastd2})", n[ok], n32[ok], n64[ok])
            assert np.abs(V[ok]).max() > 0.2
            if fastd2 == lr.FASTD2:                                    # d and n do not know about W
                assert np.array_equal(bits(d), plain[0]) and np.array_equal(bits(n)[ok], plain[1][ok])
        # without W the lattice gave what the existing restatement says (the bits of the parent are held by tests/test_gpu_lattice.py, which still passes)
        ex = ~np.asarray(p32[1]).any(axis=1)
        assert np.array_equal(plain[0][ex], bits(p32[0])[ex])


@pytest.mark.parametrize("op", ["union_capsule", "minus_sphere"])
def test_composition_still_takes_the_winning_tuple(w, op):
    from waterlily_jl_amd.bodies import Body
    c = lr.point_case("sphere_mapped")
    Wl = mv.linear_W(c["dims"], c["origin"], c["spacing"], A_LIN, B_LIN)
    with w.SdfLattice(c["values"]) as lat:
        lat.set_velocity(Wl)
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
            ta, tb, tc = (np.concatenate([v.reshape(len(X), -1) for v in w.bodies.measure(b, X, fastd2=fastd2)], axis=1) for b in (a, other, both))
            if op == "minus_sphere":
                tb[:, :D + 1] = -tb[:, :D + 1]
            less, eq = np.zeros(len(X), dtype=bool), np.ones(len(X), dtype=bool)
            for k in range(2 * D + 1):                               # isless(b, a) on the tuples (d, n, V), lexicographic: V still sits last
                lq = fr._isless(tb[:, k], ta[:, k])
                less = np.where(eq, lq, less)
                eq = eq & ~lq & fr._isequal(tb[:, k], ta[:, k])
            takeb = less if op == "union_capsule" else ~less
            want = np.where(takeb[:, None], tb, ta)
            assert takeb.sum() >= 10 and (~takeb).sum() >= 10
            same = (bits(tc) == bits(want)) | (np.isnan(tc) & np.isnan(want))
            assert same.all(), (op, fastd2, np.argwhere(~same)[:4].tolist())
            assert np.abs(ta[:, D + 1:]).max() > 0.2                 # the lattice's V carries the samples


# ---- two descriptions of one motion ----
def test_translation_by_the_map_and_by_the_vertices(w):
    """(i) a static lattice under RigidMap(V = U); (ii) the same mesh with the uniform vertex velocity U under a map at rest.  σ, μ₀, μ₁ see the same
    distances: equal bits.  V: (i) stores U + (0·b − 0·b) = U exactly.  (ii) stores 0 + Σ_q R̂[q][a]·ωξ_q with R̂ = 1 — exactly ωξ_a = Σ_k W_k·w_k over the
    2^D corners with W_k = U_a on every sample.  Each weight is a product of D factors, each 1 − y or y (at most one rounding each, D − 1 more for the
    products: relative error ≤ (2D − 1)·u, u = 2⁻²⁴); the exact weights sum to 1; each product U_a·w_k rounds once more, and the 2^D − 1 additions round
    partial sums that never exceed |U_a|·(1 + 2D·u).  So |ωξ_a − U_a| ≤ (2D + 2^D − 1)·u·|U_a|·(1 + 2⁻²⁰) — of the order (2^D + D)·2⁻²⁴·|U| the issue expects."""
    from waterlily_jl_amd.bodies import RigidMap
    U = np.array([0.25, -0.125, 0.0625], f32) * f32(1.1)
    V0, E = mr.icosphere(2, 5.0, (0.2, -0.1, 0.15))
    x0 = (14.3, 13.1, 11.7)
    by_map = w.mesh_body(V0, E, map=RigidMap(x0, (0.0, 0.0, 0.0), V=U))
    by_vert = w.mesh_body(V0, E, map=RigidMap(x0, (0.0, 0.0, 0.0)), vertex_velocity=np.broadcast_to(U, V0.shape))
    try:
        out = []
        for b in (by_map, by_vert):
            f = w.Flow((28, 26, 24), (1.0, 0.0, 0.0))
            for k in ("mu0", "mu1", "V"):
                getattr(f, k).fill_(float("nan"))
            f.sigma.fill_(0.25)
            w.measure_(f, b)
            out.append([w.to_host(getattr(f, k)) for k in ("sigma", "mu0", "mu1", "V")])
        for k, x, y in zip(("sigma", "mu0", "mu1"), *out):
            assert np.array_equal(bits(x), bits(y)), k
        Va, Vb = out[0][3], out[1][3]
        D = 3
        moving = Va != 0
        assert moving.sum() > 300 and np.array_equal(moving, Vb != 0)
        for a in range(D):
            assert np.array_equal(bits(Va[..., a][moving[..., a]]), bits(np.full(int(moving[..., a].sum()), U[a], f32)))
            bound = (2 * D + 2 ** D - 1) * 2.0 ** -24 * abs(float(U[a])) * (1 + 2.0 ** -20)
            err = float(np.abs(Vb[..., a].astype(f64) - Va[..., a].astype(f64)).max())
            print(f"[meshvel] translation, component {a}: max|V_vertices − V_map| {err:.3e}, bound {bound:.3e}")
            assert err <= bound, (a, err, bound)
    finally:
        by_map.shape[1].close(); by_vert.shape[1].close()


# ---- on a handle ----
def test_breathing_sphere_on_a_handle(w):
    from waterlily_jl_amd.bodies import RigidMap
    case = dict(id="breathing", dims=(64, 32, 24), perdir=(), exitBC=False, lam=0, store_f=False)
    centre = (0.1, -0.2, 0.15)
    V0, E = mr.icosphere(2, 5.0, centre)
    mp = RigidMap((20.3, 15.7, 11.9), (0.0, 0.0, 0.1))
    x0 = (20.0, 16.0, 12.0)
    body = w.mesh_body(V0, E, margin=7.0, map=mp, vertex_velocity=np.zeros_like(V0))
    lat = body.shape[1]
    try:
        id0 = lat.id
        A, B = handle(w, case, {}), handle(w, case, PLAIN)
        for sim in (A, B):
            sim.set_body(body)
        A.set_force_record(body, x0=x0, capacity=8)
        for k in range(4):
            dt = float(A.dt[-1])
            assert f32(dt).view(np.uint32) == f32(B.dt[-1]).view(np.uint32)
            lat.advance(mv.breathing(V0, centre, k + 1), dt)          # one call: re-bake + velocities
            assert lat.id == id0 and lat.edge_min > 4.0
            A.sim_step_(remeasure=True); B.sim_step_(remeasure=True)
            assert_same_state(A, B, ("breathing", k))
            t_, pF, vF, pM, vM = A.read_forces()                        # the recorder went on recording across the update
            assert pF.shape == (1, 3), (k, pF.shape)
            want = np.concatenate(B.forces(body, x0=x0))
            twin = mv.host_twin(body, lat.values(), lat.velocity())
            with mv.velocity_leaf():
                tp, tv, tpm, tvm = fr.tolerances(twin, B.field("p"), B.field("u"), B.nu, x0)
            rec = np.concatenate([pF[0], vF[0], pM[0], vM[0]])
            err, tol = np.abs(rec - want), np.repeat([tp, tv, tpm, tvm], 3)
            print(f"[meshvel] breathing step {k}: record − forces() {err.reshape(4, 3).max(axis=1)}, tolerance {tol[::3]}, |pF| {np.linalg.norm(want[:3]):.3e}")
            assert np.all(err <= tol), (k, err, tol)
        assert A.counter("force_dropped") == 0 and np.linalg.norm(want[:3]) > 1e-3
        # the V field of the last measure!: the radial surface velocity, against the restatement
        Ng = tuple(n + 2 for n in case["dims"])
        with mv.velocity_leaf():
            r32 = lr.measure_fields(twin, Ng, 1.0, f32)
            r64 = lr.measure_fields(twin, Ng, 1.0, f64)
        Vd = A.field("V")
        assert (Vd != 0).sum() > 300 and np.abs(Vd).max() > 0.05
        _check("breathing", "V field", Vd, r32[3], r64[3])
        _check("breathing", "mu0 field", A.field("mu0"), r32[1], r64[1])
        A.set_force_record(None)
        del A, B
    finally:
        lat.close()


# ---- refusals: decided on the host, nothing launched, nothing changed ----
def _raw_update(L, h, V, Wv=None, flags=0):
    V = np.ascontiguousarray(V, dtype=f32)
    Wv = None if Wv is None else np.ascontiguousarray(Wv, dtype=f32)
    return L.wl_sdf_lattice_update_mesh(h, V.ctypes.data_as(FP), None if Wv is None else Wv.ctypes.data_as(FP), flags, None)


def test_refusals_launch_nothing_and_change_nothing(w):
    L = w.lib()
    c = mv.case("ico80-radial")
    V, Wv = c["V"], c["Wv"]
    ctr = V.astype(f64).mean(axis=0)
    inverted = (2 * ctr - V.astype(f64)).astype(f32)                  # mirrored through the centre: every triangle faces inward
    collapsed = V.copy(); collapsed[c["E"][0, 1]] = collapsed[c["E"][0, 0]]      # an edge of zero length: triangles of zero area
    nanv = V.copy(); nanv[3, 1] = np.nan
    nanw = Wv.copy(); nanw[5, 0] = np.inf
    dims, origin = w.bodies.mesh_placement(V, 1.0, 5.5)               # a margin measure! accepts (edge_min − 0 > 4)
    c = dict(c, dims=dims, origin=origin, spacing=1.0)
    with from_case(w, c) as lat, from_case(w, c, moving=False) as static, w.SdfLattice(mr.ref("cube", "f32")["d"]) as plain:
        def refused(what, token, h, *a, keep=lat, **kw):
            before, s0, v0 = L.wl_launch_count(), state(keep), None if keep.vertices is None else keep.vertices.copy()
            n0 = L.wl_launch_count()
            assert n0 == before                                        # (reading back launches nothing)
            rc = _raw_update(L, h, *a, **kw)
            msg = L.wl_last_error_string().decode()
            assert rc == WL_EINVAL and token in msg, (what, rc, msg)
            assert L.wl_launch_count() == n0, what
            assert same_state(state(keep), s0), what
            assert keep.vertices is None or np.array_equal(keep.vertices, v0)
        refused("inverted", "inward", lat._h, inverted, Wv)
        refused("a collapsed triangle", "zero area", lat._h, collapsed, Wv)
        refused("a NaN vertex", "not finite", lat._h, nanv, Wv)
        refused("an infinite velocity", "velocity of vertex", lat._h, V, nanw)
        refused("an unknown flag", "flag", lat._h, V, Wv, flags=4)
        refused("velocities for a lattice without", "without velocity samples", static._h, V, Wv, keep=static)
        refused("not from a mesh", "not made from a mesh", plain._h, V, keep=plain)
        with pytest.raises(w.WlError, match="inward"):                 # the Python surface: the same refusal, and its copy of the vertices stays
            lat.update_mesh(inverted, Wv)
        assert np.array_equal(lat.vertices, V)
        with pytest.raises(ValueError):
            plain.update_mesh(V)
        # set_velocity / read_velocity
        bad = np.zeros(tuple(c["dims"]) + (3,), f32); bad[2, 3, 1, 0] = np.nan
        s0, n0 = state(lat), L.wl_launch_count()
        with pytest.raises(w.WlError, match="not finite"):
            lat.set_velocity(bad)
        with pytest.raises(w.WlError, match="no velocity"):
            static.velocity()
        assert same_state(state(lat), s0) and L.wl_launch_count() == n0 and not static.has_velocity
        # past the margin: the update is accepted, measure! refuses through the edge_min rule with nothing launched, a valid update goes on
        body = w.Body(("lattice", lat, c["origin"], c["spacing"], 0.0))
        f = w.Flow((24, 24, 24), (1.0, 0.0, 0.0))
        w.measure_(f, body)
        shifted = (V.astype(f64) + np.array([4.5, 0.0, 0.0])).astype(f32)
        lat.update_mesh(shifted, Wv)
        assert lat.edge_min < 4.0
        n0 = L.wl_launch_count()
        with pytest.raises(w.WlError, match="edge_min"):
            w.measure_(f, body)
        assert L.wl_launch_count() == n0
        lat.update_mesh(V, Wv)
        w.measure_(f, body)
        assert (w.to_host(f.mu0) < 1).sum() > 50
        dead, hd = lat.id, lat._h
    # an update of a closed lattice: the handle is no longer in the table (the library compares it, it never follows it)
    n0 = L.wl_launch_count()
    assert _raw_update(L, hd, V, Wv) == WL_EINVAL and "not a live lattice" in L.wl_last_error_string().decode() and L.wl_launch_count() == n0
    with pytest.raises(ValueError):
        lat.update_mesh(V, Wv)
    with pytest.raises(ValueError):
        lat.velocity()
    assert L.wl_sdf_lattice_has_velocity(hd) == 0 and not lat.has_velocity and dead >= 1
