"""Bodies from meshes on the device (include/wlhip.h, sampled bodies from meshes; csrc/wl_meshsdf.hip): the samples wl_sdf_lattice_from_mesh makes against the
NumPy restatement (tests/meshsdf_ref.py) within the project's standing rule |device − ref64| ≤ 4·max|ref32 − ref64| over the case and with its sign on every
sample; the culled search against the brute-force flag as raw bits, with the pair counts; ragged bricks; the result as a first-class lattice (measure! fields
and whole steps with a force recorder against a lattice made of the read-back samples, bit for bit); mesh_body of an icosphere against the sphere leaf; the
refusals, which launch nothing; the 2-D form; an STL file to a step.  tests/test_meshsdf_cpu.py shows without a GPU that the cases hold what they are here
for.  Lattices of at most 30×30×16 samples, 1280 triangles, grids of at most 64×32×24."""
import ctypes as C

import numpy as np
import pytest

import meshsdf_ref as mr
from test_gpu_bodypaths import assert_same_state, handle, w  # noqa: F401  (w: the module-scoped fixture)

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
WL_EINVAL = -1


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def pairs(w):
    a, b = C.c_uint64(), C.c_uint64()
    assert w.lib().wl_meshsdf_last_pairs(C.byref(a), C.byref(b)) == 0
    return int(a.value), int(b.value)


def from_case(w, name, brute=False):
    c = mr.case(name)
    return w.SdfLattice.from_mesh(c["V"], c["E"], c["dims"], c["origin"], c["spacing"], brute=brute)


# ---- 1., 2., 3., 7. values, sign, edge_min; the cull exact and live; ragged bricks; the 2-D cases ----
@pytest.mark.parametrize("name", sorted(mr.CASES))
def test_values_sign_and_brute_force_bits(w, name):
    c = mr.case(name)
    r32, r64 = mr.ref(name, "f32")["d"], mr.ref(name, "f64")["d"]
    tol = 4 * mr.gap(name)
    with from_case(w, name) as lat:
        tested, total = pairs(w)
        dev = lat.values()
        assert dev.shape == c["dims"] and dev.dtype == f32 and lat.D == c["D"] and lat.id >= 1
        err = float(np.abs(dev.astype(f64) - r64).max())
        print(f"[meshsdf] {name}: max|dev − ref64| {err:.3e}, bound 4·max|ref32 − ref64| {tol:.3e}; samples that differ from ref32 in bits: "
              f"{int((bits(dev) != bits(r32)).sum())} of {dev.size}; pairs tested {tested} of {total}")
        assert err <= tol, (name, err, tol)
        assert np.array_equal(np.sign(dev), np.sign(r64)), name
        assert not np.signbit(dev[dev == 0]).any()
        assert lat.edge_min == w.bodies.edge_min(dev), (lat.edge_min, w.bodies.edge_min(dev))
        with from_case(w, name, brute=True) as all_pairs:
            tb, total_b = pairs(w)
            assert np.array_equal(bits(all_pairs.values()), bits(dev)), (name, int((bits(all_pairs.values()) != bits(dev)).sum()))
            assert all_pairs.edge_min == lat.edge_min and all_pairs.id == lat.id + 1
        n_samples = int(np.prod(c["dims"]))
        assert total == total_b == n_samples * len(c["E"]) and tb == total_b
        nbricks = mr.cull_census(name)["nbricks"]
        assert nbricks <= tested <= total, (name, nbricks, tested, total)
        if name in ("torus", "ico1280-centred"):
            assert tested < total, (name, tested, total)


# ---- 4. a first-class lattice ----
def test_measure_fields_equal_those_of_the_copied_lattice(w):
    c = mr.case("ico320")
    V = c["V"] + np.array([3.0, 2.0, 1.5], f32)
    body = w.mesh_body(V, c["E"])
    lat = body.shape[1]
    try:
        assert lat.edge_min - 0.0 > 4.0
        with w.SdfLattice(lat.values()) as copy:
            assert copy.edge_min == lat.edge_min and copy.dims == lat.dims
            twin = w.Body(("lattice", copy) + body.shape[2:], body.map)
            out = []
            for b in (body, twin):
                f = w.Flow((28, 26, 24), (1.0, 0.0, 0.0))
                for k in ("mu0", "mu1", "V"):
                    getattr(f, k).fill_(float("nan"))
                f.sigma.fill_(0.25)
                w.measure_(f, b)
                out.append([w.to_host(getattr(f, k)) for k in ("sigma", "mu0", "mu1", "V")])
            for k, x, y in zip(("sigma", "mu0", "mu1", "V"), *out):
                assert np.array_equal(bits(x), bits(y)), k
            assert (out[0][1] < 1).sum() > 100 and (out[0][0] < 0).sum() > 100      # the body is on the grid
    finally:
        lat.close()


def _run_with_recorder(sim, body, x0):
    sim.set_body(body)
    sim.set_force_record(body, x0=x0, capacity=8)
    sim.mom_step_(); sim.mom_step_(); sim.mom_steps_(3)
    rec = sim.read_forces()
    sim.set_force_record(None)
    return rec


def test_steps_and_force_records_equal_those_of_the_copied_lattice(w):
    from waterlily_jl_amd.bodies import RigidMap
    c = mr.case("ico320")
    case = dict(id="mesh_ico320", dims=(64, 32, 24), perdir=(), exitBC=False, lam=0, store_f=False)
    mp = RigidMap((10.0, 5.0, 2.0), (0.0, 0.0, 0.1), V=(0.15, 0.05, 0.0))
    body = w.mesh_body(c["V"], c["E"], map=mp)
    lat = body.shape[1]
    try:
        with w.SdfLattice(lat.values()) as copy:
            twin = w.Body(("lattice", copy) + body.shape[2:], mp)
            A, B = handle(w, case, {}), handle(w, case, {})
            x0 = (20.0, 15.0, 12.0)
            ra, rb = _run_with_recorder(A, body, x0), _run_with_recorder(B, twin, x0)
            assert_same_state(A, B, "mesh lattice against its copy")
            assert len(ra[0]) == 5
            for x, y in zip(ra, rb):
                assert np.array_equal(np.asarray(x, f64).view(np.uint64), np.asarray(y, f64).view(np.uint64))
            assert np.linalg.norm(ra[1][-1]) > 1e-3 and np.isfinite(A.field("u")).all()
            del A, B
    finally:
        lat.close()


# ---- 5. against the closed form ----
def test_mesh_body_of_an_icosphere_against_the_sphere_leaf(w):
    R, s, centre = 8.0, 1.0, np.array([0.3, -0.2, 0.1])
    V, E = mr.icosphere(2, R, centre)
    body = w.mesh_body(V, E, spacing=s)
    lat = body.shape[1]
    try:
        rng = np.random.default_rng(5)
        u = rng.normal(size=(500, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
        X = (centre + u * (R + rng.uniform(-3, 3, size=(500, 1)))).astype(f32)      # within 3 cells of the surface, either side
        d_mesh, _, _ = w.bodies.measure(body, X, fastd2=0.0)              # d alone: the sampled value, as bake takes it
        d_sph, _, _ = w.bodies.measure(w.Body(("sphere", tuple(centre), R)), X, fastd2=0.0)
        # r_in: the smallest centre-to-face-plane distance of the mesh (it is inscribed: R − r_in is how far it departs from the sphere)
        P = V.astype(f64)
        a, b, cc = P[E[:, 0]], P[E[:, 1]], P[E[:, 2]]
        n = np.cross(b - a, cc - a); n /= np.linalg.norm(n, axis=1)[:, None]
        r_in = float(np.einsum("ij,ij->i", a - centre, n).min())
        assert 0 < R - r_in < 0.5
        # the samples the 500 stencils read, restated: the gap of the rule over them
        dims, origin = w.bodies.mesh_placement(V, s, 5.0)
        q = (X.astype(f64) - np.asarray(origin)) / s
        i0 = np.floor(q + 0.5).astype(int)
        corners = np.unique(np.concatenate([i0 + np.array(o) for o in np.ndindex(2, 2, 2)]), axis=0)
        assert (corners >= 0).all() and (corners < np.array(dims)).all()
        Xs = (np.asarray(origin, f32) + f32(s) * (corners.astype(f32) - f32(0.5))).astype(f32)
        g = float(np.abs(mr.sdf_points(3, V, E, Xs, f32)["d"].astype(f64) - mr.sdf_points(3, V, E, Xs, f64)["d"]).max())
        # trilinear interpolation of a 1-Lipschitz function: |Σ wₖ f(cₖ) − f(x)| ≤ Σ wₖ|cₖ − x| ≤ s·√(Σ_d y_d(1 − y_d)) ≤ (√3/2)·s
        bound = (R - r_in) + np.sqrt(3) / 2 * s + 4 * g
        err = float(np.abs(d_mesh.astype(f64) - d_sph.astype(f64)).max())
        print(f"[meshsdf] icosphere against the sphere leaf: max|Δd| {err:.3e}, bound {bound:.3e} (R − r_in {R - r_in:.3e}, gap {g:.2e})")
        assert err <= bound
        assert (d_sph < 0).sum() > 100 and (d_sph > 0).sum() > 100 and np.array_equal(np.sign(d_mesh[np.abs(d_sph) > bound]), np.sign(d_sph[np.abs(d_sph) > bound]))
    finally:
        lat.close()


# ---- 6. refusals: decided on the host, nothing is launched, and the next valid call goes through ----
def _raw_from_mesh(L, D, dims, origin, spacing, V, E, flags=0):
    V = np.ascontiguousarray(V, dtype=f32); E = np.ascontiguousarray(E, dtype=np.int32)
    h = C.c_void_p()
    rc = L.wl_sdf_lattice_from_mesh(C.byref(h), D, (C.c_int32 * len(dims))(*dims), (C.c_float * len(origin))(*origin), spacing,
                                    V.ctypes.data_as(C.POINTER(C.c_float)), len(V), E.ctypes.data_as(C.POINTER(C.c_int32)), len(E), flags, None)
    return rc, h


def test_refusals_launch_nothing(w):
    L = w.lib()
    c = mr.case("cube-5x3x3")

    def refused(what, token, D=3, dims=c["dims"], origin=(0.0, 0.0, 0.0), spacing=5.0, V=c["V"], E=c["E"], flags=0):
        before = L.wl_launch_count()
        rc, h = _raw_from_mesh(L, D, dims, origin, spacing, V, E, flags)
        msg = L.wl_last_error_string().decode()
        assert rc == WL_EINVAL and not h.value, (what, rc)
        assert L.wl_launch_count() == before, what
        assert token in msg, (what, token, msg)

    def next_id():
        with from_case(w, "cube-5x3x3") as lat:
            return lat.id

    first = next_id()
    n_ref = 0
    for name, D, V, E, why in mr.broken_variants():
        dims = c["dims"] if D == 3 else (5, 5)
        refused(name, mr.REASONS[why], D=D, dims=dims, origin=(0.0,) * D, V=V, E=E)
        n_ref += 1
        assert next_id() == first + n_ref, name          # no table entry was taken, no id spent: the next valid call has the next id
    refused("D = 1", "D must be", D=1, dims=(5,), origin=(0.0,))
    refused("D = 4", "D must be", D=4, dims=(5, 3, 3, 3), origin=(0.0,) * 4)
    refused("an extent of 2", "at least 3", dims=(5, 2, 3))
    for s in (0.0, -1.0, float("nan"), float("inf")):
        refused(f"spacing {s}", "spacing", spacing=s)
    refused("a NaN origin", "origin", origin=(0.0, float("nan"), 0.0))
    refused("an unknown flag", "flag", flags=2)
    assert "weld" in mr.REASONS["edge"]
    assert next_id() == first + n_ref + 1
    # a ninth live lattice
    more = [from_case(w, "cube-3x3x3") for _ in range(8)]
    try:
        refused("a ninth lattice", "alive")
        with pytest.raises(w.WlError):
            from_case(w, "cube-3x3x3")
    finally:
        for m in more:
            m.close()
    assert [m.id for m in more] == list(range(more[0].id, more[0].id + 8))
    # after close() a program that names the lattice is refused, as for any lattice
    body = w.mesh_body(mr.case("cube")["V"], mr.case("cube")["E"])
    X = np.array([[8.0, 8.0, 7.0], [1.0, 1.0, 1.0]], f32)
    d, _, _ = w.bodies.measure(body, X, fastd2=0.0)
    assert d[0] < 0 < d[1]
    dead = body.shape[1].id
    body.shape[1].close()
    before = L.wl_launch_count()
    with pytest.raises(w.WlError, match="destroyed"):
        w.bodies.measure(body, X, fastd2=0.0)
    assert L.wl_launch_count() == before
    with pytest.raises(ValueError):
        body.shape[1].values()
    assert L.wl_sdf_lattice_edge_min(None) == 0.0
    assert next_id() > dead


# ---- 7. the 2-D form on a handle ----
def test_2d_polygon_steps_equal_those_of_the_copied_lattice(w):
    c = mr.case("lpoly")
    case = dict(id="mesh_lpoly", dims=(48, 40), perdir=(), exitBC=False, lam=0, store_f=False)
    V = c["V"] + np.array([8.0, 9.0], f32)
    body = w.mesh_body(V, c["E"])
    lat = body.shape[1]
    try:
        assert lat.D == 2 and lat.edge_min > 4.0
        with w.SdfLattice(lat.values()) as copy:
            twin = w.Body(("lattice", copy) + body.shape[2:], None)
            A, B = handle(w, case, {}), handle(w, case, {})
            for sim, b in ((A, body), (B, twin)):
                sim.set_body(b)
                sim.mom_step_(); sim.mom_step_()
            assert_same_state(A, B, "2-D mesh lattice against its copy")
            mu0 = A.field("mu0")
            assert (mu0 < 1).sum() > 50 and np.isfinite(A.field("u")).all()
            del A, B
    finally:
        lat.close()


# ---- 8. from a file to a step ----
def test_stl_file_to_a_step(w, tmp_path):
    V, E = mr.icosphere(1, 4.0, (12.3, 10.2, 9.9))
    path = tmp_path / "ball.stl"
    mr.write_binary_stl(path, V, E)
    Vr, Er = w.read_stl(str(path))
    assert Vr.shape == (42, 3) and Er.shape == (80, 3)
    body = w.mesh_body(Vr, Er)
    try:
        sim = w.FusedSimulation((32, 24, 20), (1, 0, 0), 8.0, U=1, nu=0.05, has_body=True)
        sim.set_body(body)
        sim.sim_step_(remeasure=True)                       # raises on any return code but 0
        assert len(sim.dt) == 2 and np.isfinite(sim.field("u")).all() and (sim.field("mu0") < 1).sum() > 50
        del sim
    finally:
        body.shape[1].close()
