"""Composite bodies on the device (include/wlhip.h wl_bodyset): identity with the closed-form wl_body path, the reference's known
answers for RigidMap and SetBody (test/test_bodies.jl:21-27,54-107, test/test_simulation.jl:31-35), the moving-body time step on the
leaf-op and composite paths, and the host validation of malformed programs."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BODIES_3D = [
    ("cylinder", (11.0, 13.5, 0.0), 4.0, 2),
    ("cylinder", (0.0, 14.0, 12.5), 3.5, 0),
    ("plane", (0.0, 5.0, 0.0), (0.0, 1.0, 0.0)),
    ("plane", (16.0, 8.0, 0.0), (0.3, 1.0, 0.0)),
    ("sphere", (12.0, 15.0, 15.5), 4.0, (0.25, -0.125, 0.0)),
]
BODIES_2D = [("sphere", (11.0, 13.5), 4.0), ("plane", (16.0, 8.0), (0.3, 1.0))]
RTOL = float(np.sqrt(np.finfo(np.float32).eps))


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    return w


def _fields(w, f):
    return {k: w.to_host(getattr(f, k)) for k in ("sigma", "mu0", "mu1", "V")}


def _poison(w, f):
    for k in ("sigma", "mu0", "mu1", "V"):
        getattr(f, k).fill_(float("nan"))
    f.sigma.fill_(0.0)          # σ's ghosts are not written by measure! (measure_sdf! is @inside)


def _strip_velocity(body):
    return body[:4] if body[0] == "cylinder" else body[:3]


def _same(a, b):
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("body", BODIES_3D + BODIES_2D, ids=lambda b: b[0] + str(len(b[1])) + "_" + str(len(b)))
def test_one_leaf_program_equals_wl_measure_body(w, body):
    from waterlily_jl_amd import bodies
    D = len(body[1])
    N = (32,) * D
    still = _strip_velocity(body)
    f0 = w.Flow(N, (1.0,) + (0.0,) * (D - 1), nu=0.02)
    w.measure_(f0, still)
    ref = _fields(w, f0)
    n0 = w.lib().wl_launch_count()
    f1 = w.Flow(N, (1.0,) + (0.0,) * (D - 1), nu=0.02)
    _poison(w, f1)
    w.measure_(f1, bodies.Body(still))
    _same(ref, _fields(w, f1))
    # the identity map gives the same arrays
    f2 = w.Flow(N, (1.0,) + (0.0,) * (D - 1), nu=0.02)
    _poison(w, f2)
    w.measure_(f2, bodies.Body(still, bodies.RigidMap((0.0,) * D, 0.0 if D == 2 else (0.0, 0.0, 0.0))))
    _same(ref, _fields(w, f2))
    # θ = 0, ω = 0, V ≠ 0 reproduces the translating wl_body, V included
    Vb = (0.25, -0.125, 0.0)[:D]
    fv = w.Flow(N, (1.0,) + (0.0,) * (D - 1), nu=0.02)
    w.measure_(fv, tuple(still) + (Vb,))
    f3 = w.Flow(N, (1.0,) + (0.0,) * (D - 1), nu=0.02)
    _poison(w, f3)
    w.measure_(f3, bodies.Body(still, bodies.RigidMap((0.0,) * D, 0.0 if D == 2 else (0.0, 0.0, 0.0), V=Vb)))
    _same(_fields(w, fv), _fields(w, f3))
    assert np.abs(_fields(w, f3)["V"]).max() == 0.25
    # forces and moments: exactly the wl_body read-outs (on a non-trivial p, u)
    rng = np.random.default_rng(3)
    f0.p.copy_(w.to_device(rng.standard_normal(f0.p.shape).astype(np.float32)))
    f0.u.copy_(w.to_device(rng.standard_normal(f0.u.shape).astype(np.float32)))
    lb = bodies.Body(still)
    assert np.array_equal(w.pressure_force(f0, lb), w.pressure_force(f0, still))
    assert np.array_equal(w.viscous_force(f0, lb), w.viscous_force(f0, still))
    x0 = (14.0, 12.5, 17.0)[:D]
    assert np.array_equal(w.pressure_moment(x0, f0, lb), w.pressure_moment(x0, f0, still))
    assert np.array_equal(w.viscous_moment(x0, f0, lb), w.viscous_moment(x0, f0, still))
    assert w.lib().wl_launch_count() > n0


# ---- the closed-form wl_body entry points against what they computed before they became one-leaf programs (tests/golden/make_body_parent.py) ----
_X0_PARENT = (7.3, 8.7, 6.1)


@pytest.fixture(scope="module")
def parent():
    import json
    import os
    raw = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "body_parent.npz"))
    raw = {k: raw[k] for k in raw.files}
    # (an array that repeats an earlier one bit for bit is stored as "=<that key>": make_body_parent.py pack)
    z = {k: (raw[str(v)[1:]] if v.dtype.kind == "U" and str(v).startswith("=") else v) for k, v in raw.items()}
    return z, json.loads(str(z["cases"]))


def _int_field(shape, c):
    """((7i + 13j + 29k + 5c) mod 17 − 8) / 4 on the 0-based array indices: exact in float32"""
    idx = np.indices(shape)
    s = 5 * c + sum(wt * ix for wt, ix in zip((7, 13, 29), idx))
    return ((s % 17 - 8) / 4).astype(np.float32)


def _body_tuple(spec):
    return tuple(tuple(v) if isinstance(v, list) else v for v in spec)


def _as_leaf(w, body):
    """the same closed-form body as a one-leaf program; a translation velocity becomes the θ = 0 map's V"""
    from waterlily_jl_amd import bodies
    still = _strip_velocity(body)
    if len(body) == len(still):
        return bodies.Body(still)
    D = len(body[1])
    return bodies.Body(still, bodies.RigidMap((0.0,) * D, 0.0 if D == 2 else (0.0, 0.0, 0.0), V=body[-1]))


@pytest.mark.parametrize("case", range(7))
def test_wl_body_entry_points_equal_the_parent_commit(w, parent, case):
    """σ, μ₀, μ₁, V of wl_measure_body and the four Float64 read-outs, bit for bit what the commit recorded in the fixture computed with its own
    k_measure_body / k_pforce_body / k_vforce_body — through wl_*_body and through the one-leaf wl_*_bodyset calls"""
    z, cases = parent
    name, N, spec, eps = cases[case]
    D, body = len(N), _body_tuple(spec)
    moving = len(body) != len(_strip_velocity(body))
    x0 = _X0_PARENT[:D]
    still = _strip_velocity(body)
    for measured, read in ((body, still), (_as_leaf(w, body), _as_leaf(w, still))):
        f = w.Flow(tuple(N), (1.0,) + (0.0,) * (D - 1), nu=0.02)
        _poison(w, f)
        w.measure_(f, measured, eps)
        got = _fields(w, f)
        for k in got:
            assert np.array_equal(got[k], z[f"{name}/{k}"]), (name, k)
        f.p.copy_(w.to_device(_int_field(tuple(f.p.shape), 0)))
        f.u.copy_(w.to_device(np.stack([_int_field(tuple(f.p.shape), c + 1) for c in range(D)], -1)))
        assert np.array_equal(w.pressure_force(f, read), z[f"{name}/pforce"]), name
        assert np.array_equal(w.viscous_force(f, read), z[f"{name}/vforce"]), name
        assert np.array_equal(w.pressure_moment(x0, f, read), z[f"{name}/pmoment"]), name
        assert np.array_equal(w.viscous_moment(x0, f, read), z[f"{name}/vmoment"]), name
    assert z[f"{name}/pforce"].any() and (np.abs(z[f"{name}/V"]).max() == 0.25) == moving


def test_sim_measure_body_leaves_the_arrays_of_wl_measure_body(w, parent):
    """wl_sim_measure_body on a has_body handle against wl_measure_body on a Flow (the fixture's translating sphere); the force recorder follows the body"""
    z, cases = parent
    name, N, spec, eps = cases[4]
    body = _body_tuple(spec)
    sf = w.FusedSimulation(tuple(N), (1.0, 0.0, 0.0), 8, nu=0.02, has_body=True)
    sf.set_force_record(w.Body(("sphere", (4.0, 4.0, 4.0), 2.0)), x0=_X0_PARENT, capacity=4)
    t0 = sf.counter("force_tiles")
    sf.measure_body_(body, eps)
    f = w.Flow(tuple(N), (1.0, 0.0, 0.0), nu=0.02)
    w.measure_(f, body, eps)
    ref = _fields(w, f)
    for k in ("sigma", "mu0", "mu1", "V"):
        assert np.array_equal(sf.field(k), ref[k]), k
        assert np.array_equal(ref[k], z[f"{name}/{k}"]), k
    sg = w.FusedSimulation(tuple(N), (1.0, 0.0, 0.0), 8, nu=0.02, has_body=True)
    sg.set_force_record(w.Body(_strip_velocity(body)), x0=_X0_PARENT, capacity=4)
    assert sf.counter("force_tiles") == sg.counter("force_tiles") > t0 > 0


def _approx(a, b):
    """Julia's ≈ with the default rtol = √eps(Float32), norm-based on vectors"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) <= RTOL * max(np.linalg.norm(a), np.linalg.norm(b))


def _check(w, body, x, d, n, V):
    from waterlily_jl_amd import bodies
    dd, nn, vv = bodies.measure(body, np.array([x], dtype=np.float32))
    assert _approx(dd[0], d), (x, dd[0], d)
    assert _approx(nn[0], n), (x, nn[0], n)
    assert _approx(vv[0], V), (x, vv[0], V)


def test_rigidmap_known_answers(w):
    """test/test_bodies.jl:56-88 (Float32)"""
    from waterlily_jl_amd.bodies import Body, RigidMap, setmap
    unit = lambda D: ("sphere", (0.0,) * D, 1.0)     # noqa: E731
    body = Body(unit(2), RigidMap((0, 0), 0.0))
    _check(w, body, (1.5, 0), 0.5, (1, 0), (0, 0))
    body = setmap(body, theta=np.float32(np.pi / 4), V=(1.0, 0))
    _check(w, body, (1.5, 0), 0.5, (1, 0), (1, 0))
    body = setmap(body, omega=0.1)
    _check(w, body, (1.5, 0), 0.5, (1, 0), (1, 1.5 * 0.1))
    b3 = Body(unit(3), RigidMap((0, 0, 0), (0, 0, 0), xp=(-0.5, 0, 0)))
    _check(w, b3, (1.5, 0, 0), 0.5, (1, 0, 0), (0, 0, 0))
    b3 = setmap(b3, theta=(np.pi, 0, 0))
    _check(w, b3, (1.5, 0, 0), 0.5, (1, 0, 0), (0, 0, 0))
    b3 = setmap(b3, theta=(0, np.pi, 0), V=(1.0, 0, 0))
    _check(w, b3, (1.5, 0, 0), 1.5, (1, 0, 0), (1, 0, 0))
    b3 = setmap(b3, theta=(0, 0, np.pi), V=(1.0, 0, 0))
    _check(w, b3, (1.5, 0, 0), 1.5, (1, 0, 0), (1, 0, 0))
    b3 = setmap(b3, theta=(0, 0, 0), V=(1.0, 0, 0), omega=(0, 0, 0.1))
    _check(w, b3, (1.5, 0, 0), 0.5, (1, 0, 0), (1, 0.2, 0))
    _check(w, b3, (0, 1.5, 0), 0.5, (0, 1, 0), (0.85, 0.05, 0))
    s = np.sqrt(1 / 3)
    _check(w, b3, (1.5, 1.5, 1.5), np.sqrt(3 * 1.5 ** 2) - 1, (s, s, s), (0.85, 0.2, 0))
    b3 = setmap(b3, V=(1.0, 0, 0), omega=(0, -0.1, 0.1))
    _check(w, b3, (1.5, 0, 0), 0.5, (1, 0, 0), (1, 0.2, 0.2))
    h = np.sqrt(1 / 2)
    _check(w, b3, (0, 1.5, 1.5), np.sqrt(2 * 1.5 ** 2) - 1, (0, h, h), (0.7, 0.05, 0.05))


def test_annulus_and_booleans_known_answers(w):
    """test/test_bodies.jl:104-106 (annulus: difference and negation) and :21-27 (booleans at t = 1, exactly equal distances)"""
    from waterlily_jl_amd.bodies import Body, RigidMap, setmap
    rm = RigidMap((0.0, 0.0), np.pi / 4)
    ann = Body(("sphere", (0, 0), 1.0), rm) - Body(("sphere", (0, 0), 0.5), rm)
    _check(w, setmap(ann, omega=1.0), (0.25, 0), 0.25, (-1, 0), (0, 0.25))
    # body1 = circle of radius 2+t, body2 = circ under x .+ t² at t = 1: c = (−1,−1), velocity −J⁻¹∂ₜmap = (−2,−2)
    body1 = Body(("sphere", (0, 0), 3.0))
    body2 = Body(("sphere", (0, 0), 2.0), RigidMap((-1.0, -1.0), 0.0, V=(-2.0, -2.0)))
    r = np.sqrt(2.0)
    _check(w, body1 | body2, (-r, -r), -r, (-np.sqrt(.5), -np.sqrt(.5)), (-2, -2))
    _check(w, body1 + body2, (-r, -r), -r, (-np.sqrt(.5), -np.sqrt(.5)), (-2, -2))
    _check(w, body1 - body2, (-r, -r), r, (np.sqrt(.5), np.sqrt(.5)), (-2, -2))
    circ = ("sphere", (0, 0), 2.0)
    eq = Body(circ) + Body(circ, RigidMap((6.0, 0.0), 0.0))
    d, _, _ = w.bodies.measure(eq, np.array([[3.0, 0.0]], dtype=np.float32), fastd2=0.0)
    assert d[0] == 1


PLATE = ("capsule", (0.0, 0.0), 2.0, (1.0, 0.0), 6.0)       # the reference's plate(x,t) with radius = 8


def _plate(w, t):
    return w.Body(PLATE, w.RigidMap((16.0, 16.0), np.float32(t / 8 + 1), omega=1 / 8))


@pytest.mark.parametrize("exitBC", (True, False))
def test_nonuniform_V_does_not_break(w, exitBC):
    """test/test_simulation.jl:31-35: the rotating plate, on the composite handle and on the leaf-op Simulation"""
    sf = w.FusedSimulation((32, 32), (0, 0), 8, U=1, nu=8 / 250, exitBC=exitBC, has_body=True)
    sf.set_body(_plate(w, 0.0))
    sf.sim_step_(remeasure=True)
    assert len(sf.pois_n) == 2 and all(n < 5 for n in sf.pois_n)
    assert 1 > sf.dt[-1] > 0.5
    sl = w.Simulation((32, 32), (0, 0), 8, U=1, nu=8 / 250, exitBC=exitBC, body=_plate(w, 0.0))
    sl.sim_step_(remeasure=True)
    assert len(sl.pois.n) == 2 and all(n < 5 for n in sl.pois.n)
    assert 1 > sl.flow.dt[-1] > 0.5


def test_spinning_sphere_known_answer(w):
    """test/test_bodies.jl:94-102"""
    b = w.Body(("sphere", (0.0, 0.0, 0.0), 4.0), w.RigidMap((16, 16, 16), (0, 0, 0), omega=(0, -0.1, 0.1)))
    sf = w.FusedSimulation((32, 32, 32), (1, 0, 0), 8, has_body=True)
    sf.set_body(b)
    V = sf.field("V")
    assert _approx(V.min(), -0.9) and _approx(V.max(), 0.9)
    sim = w.Simulation((32, 32, 32), (1, 0, 0), 8, body=b)
    V2 = w.to_host(sim.flow.V)
    assert np.array_equal(V, V2)
    sim.body = w.setmap(sim.body, x0=(16, 16, 12))
    assert np.all(w.to_host(sim.flow.mu0)[16, 16, 16, :] == 0)


@pytest.mark.parametrize("D", (2, 3))
def test_pitching_plate_leafop_and_composite_agree(w, D):
    """setmap + device remeasure on each of 10 steps: the leaf-op Simulation and the composite FusedSimulation measure the same
    arrays, solve the same number of iterations and step to the same velocity"""
    from waterlily_jl_amd.bodies import Body, RigidMap, setmap
    if D == 2:
        N, shape = (48, 32), PLATE
        mk = lambda th, om: Body(shape, RigidMap((16.0, 16.0), np.float32(th), omega=om))   # noqa: E731
    else:
        N, shape = (32, 32, 32), ("capsule", (0.0, 0.0, 0.0), 2.0, (1.0, 0.0, 0.0), 6.0)
        mk = lambda th, om: Body(shape, RigidMap((16.0, 16.0, 16.0), (0.0, 0.0, np.float32(th)), omega=(0.0, 0.0, om)))   # noqa: E731
    uBC = (1.0,) + (0.0,) * (D - 1)
    sl = w.Simulation(N, uBC, 8, nu=0.02, body=mk(0.0, 0.0))
    sf = w.FusedSimulation(N, uBC, 8, nu=0.02, has_body=True)
    sf.set_body(mk(0.0, 0.0))
    for step in range(10):
        t = float(np.sum(sl.flow.dt[:-1])) if step else 0.0
        th, om = 0.3 * np.sin(0.2 * t), 0.06 * np.cos(0.2 * t)
        sl.body = mk(th, om)
        sf.body = sl.body
        sl.sim_step_(remeasure=True)
        sf.sim_step_(remeasure=True)
        for k in ("sigma", "mu0", "mu1", "V"):
            if k == "sigma":
                continue                                    # σ is overwritten by the step (conv_diff!'s Φ / the projection's z)
            assert np.array_equal(sf.field(k), w.to_host(getattr(sl.flow, k))), (step, k)
        assert sf.pois_n == sl.pois.n, step
        assert np.abs(sf.field("u") - w.to_host(sl.flow.u)).max() < 5e-5, step
    b = sl.body | Body(("sphere", (30.0,) + (16.0,) * (D - 1), 3.0))
    x0 = (16.0,) * D
    for fl, fs in ((w.pressure_force(sl.flow, b), sf.pressure_force_body(b)), (w.viscous_force(sl.flow, b), sf.viscous_force_body(b)),
                   (w.pressure_moment(x0, sl.flow, b), sf.pressure_moment_body(x0, b)), (w.viscous_moment(x0, sl.flow, b), sf.viscous_moment_body(x0, b))):
        assert np.allclose(fs, fl, rtol=2e-3, atol=2e-3 * max(np.abs(fl).max(), 1e-6))


def test_forces_on_a_set_body_match_a_restatement(w):
    """pressure_force / pressure_moment of a union of two rotated cylinders (2-D) against src/Metrics.jl:116-133,169-174 restated with the
    point probe's nds on the device's p"""
    from waterlily_jl_amd.bodies import Body, RigidMap, measure
    b = Body(("capsule", (0.0, 0.0), 2.0, (1.0, 0.0), 5.0), RigidMap((14.0, 16.0), 0.4)) | Body(("sphere", (0.0, 0.0), 3.0), RigidMap((22.0, 15.0), 1.1, xp=(1.0, 0.0)))
    f = w.Flow((40, 32), (1.0, 0.0), nu=0.02)
    rng = np.random.default_rng(5)
    p = rng.standard_normal(f.p.shape).astype(np.float32)
    f.p.copy_(w.to_device(p))
    I = np.stack(np.meshgrid(np.arange(2, 41), np.arange(2, 33), indexing="ij"), -1).reshape(-1, 2)
    x = (I - 1.5).astype(np.float32)
    d, n, _ = measure(b, x, fastd2=1.0)
    kk = (1 + np.cos(np.pi * np.clip(d, -1, 1))) / 2
    nds = n * kk[:, None]
    pv = p[I[:, 0] - 1, I[:, 1] - 1].astype(np.float64)
    F = (pv[:, None] * nds).sum(0)
    assert np.allclose(w.pressure_force(f, b), F, rtol=2e-3, atol=2e-3 * np.abs(F).max())
    x0 = np.array([16.0, 15.0])
    r = x - x0
    M = (pv * (r[:, 0] * nds[:, 1] - r[:, 1] * nds[:, 0])).sum()
    assert np.allclose(w.pressure_moment(x0, f, b), [M, M], rtol=2e-3, atol=2e-3 * abs(M))


def test_malformed_programs_launch_nothing(w):
    from waterlily_jl_amd._lib import wl_bodyset
    from waterlily_jl_amd.bodies import Body, OP_INTERSECT, OP_LEAF, OP_NEGATE, OP_UNION
    f = w.Flow((16, 16), (1.0, 0.0))
    g = w.core.sgrid(f.sigma)

    def good_leaf():
        return Body(("sphere", (8.0, 8.0), 3.0)).program(2).node[0]

    def run(nodes, n=None, launches=0):
        s = wl_bodyset()
        s.n = len(nodes) if n is None else n
        for i, nd in enumerate(nodes):
            s.node[i] = nd
        before = w.lib().wl_launch_count()
        rc = w.lib().wl_measure_bodyset(w.core.ptr(f.sigma), w.core.ptr(f.mu0), w.core.ptr(f.mu1), w.core.ptr(f.V), C.byref(g), C.byref(s), 1.0, 0, 0, None)
        assert w.lib().wl_launch_count() == before + launches
        return rc

    def op(o):
        nd = good_leaf(); nd.op = o
        return nd

    WL_EINVAL = -1
    assert run([op(OP_UNION)]) == WL_EINVAL                                     # stack underflow
    assert run([good_leaf(), op(OP_NEGATE), op(OP_INTERSECT)]) == WL_EINVAL
    assert run([good_leaf(), good_leaf()]) == WL_EINVAL                         # final depth 2
    assert run([good_leaf()] * 9 + [op(OP_UNION)] * 7) == WL_EINVAL             # stack of 9
    assert run([good_leaf()], n=17) == WL_EINVAL                                # more than 16 nodes
    assert run([good_leaf()], n=0) == WL_EINVAL
    bad = good_leaf(); bad.kind = 7
    assert run([bad]) == WL_EINVAL                                              # unknown kind
    assert run([op(9)]) == WL_EINVAL                                            # unknown op
    zero = good_leaf(); zero.m[0] = zero.m[1] = 0.0
    assert run([zero]) == WL_EINVAL                                             # zero axis / normal
    cap = Body(("capsule", (8.0, 8.0), 2.0, (1.0, 0.0), 3.0)).program(2).node[0]; cap.h = -1.0
    assert run([cap]) == WL_EINVAL                                              # h < 0
    msg = w.lib().wl_last_error_string().decode()
    assert "h" in msg
    assert run([good_leaf()], launches=3) == 0 and OP_LEAF == 0                 # measure kernel + BC!(μ₀) + BC!(V)


def test_rotating_plate_across_a_slab_boundary():
    """2 z-slab ranks on one GPU (gloo): the measured fields equal the single domain's, 3 remeasured steps match within 5e-5"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(29500 + (os.getpid() + 211) % 400), os.path.join(root, "tests", "bodyset_slab_worker.py"), "48x32x64", "3"]
    r = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for rank in (0, 1):
        assert f"rank {rank}: bodyset_slab ok" in r.stdout


# ---- measure! restated in NumPy float32, in the kernel's operation order (src/Body.jl:28-48, src/AutoBody.jl:29-37, src/RigidMap.jl) ----
f32 = np.float32


def _leaf_np(nd, X, fastd2, D):
    """measure(leaf, x; fastd²) for the rows of X: d, n, V"""
    M = X.shape[0]
    c, m = np.array(nd.c[:D], f32), np.array(nd.m[:D], f32)
    if nd.mapped:
        x0, xp = np.array(nd.map.x0[:D], f32), np.array(nd.map.xp[:D], f32)
        R = np.array(nd.map.R, f32).reshape(3, 3)
        b = (X - x0) - xp
        xi = np.empty_like(X)
        for q in range(D):
            s = np.zeros(M, f32)
            for r in range(D):
                s = s + R[q, r] * b[:, r]
            xi[:, q] = s + xp[q]
    else:
        xi, b = X, np.zeros_like(X)
    g = np.zeros((M, D), f32)
    if nd.kind == 2:
        d = np.zeros(M, f32)
        for q in range(D):
            d = d + m[q] * (xi[:, q] - c[q])
        g[:] = m
    elif nd.kind == 1:
        s = np.zeros(M, f32)
        for q in range(D):
            dx = m[q] * (xi[:, q] - c[q]); s = s + dx * dx
        rr = np.sqrt(s); d = rr - f32(nd.R)
        with np.errstate(invalid="ignore", divide="ignore"):
            for q in range(D):
                g[:, q] = (m[q] * (xi[:, q] - c[q])) / rr
    else:
        t = np.zeros(M, f32)
        for q in range(D):
            t = t + m[q] * (xi[:, q] - c[q])
        t = np.minimum(np.maximum(t, -f32(nd.h)), f32(nd.h))
        s = np.zeros(M, f32); dl = np.empty((M, D), f32)
        for q in range(D):
            dl[:, q] = xi[:, q] - (c[q] + t * m[q]); s = s + dl[:, q] * dl[:, q]
        rr = np.sqrt(s); d = rr - f32(nd.R)
        with np.errstate(invalid="ignore", divide="ignore"):
            g = dl / rr[:, None]
    full = ~(d * d > f32(fastd2)) & ~np.isnan(g).any(1)
    if nd.mapped:
        nn = np.zeros((M, D), f32)
        for a in range(D):
            s = np.zeros(M, f32)
            for q in range(D):
                s = s + R[q, a] * g[:, q]
            nn[:, a] = s
    else:
        nn = g
    mm = np.zeros(M, f32)
    for q in range(D):
        mm = mm + nn[:, q] * nn[:, q]
    mm = np.sqrt(mm)
    with np.errstate(invalid="ignore", divide="ignore"):
        dn, n = d / mm, nn / mm[:, None]
    V = np.zeros((M, D), f32)
    if nd.mapped:
        Vm, wv = np.array(nd.map.V[:D], f32), np.array(nd.map.w, f32)
        if D == 2:
            V[:, 0] = Vm[0] + wv[0] * -b[:, 1]; V[:, 1] = Vm[1] + wv[0] * b[:, 0]
        else:
            V[:, 0] = Vm[0] + (wv[1] * b[:, 2] - wv[2] * b[:, 1])
            V[:, 1] = Vm[1] + (wv[2] * b[:, 0] - wv[0] * b[:, 2])
            V[:, 2] = Vm[2] + (wv[0] * b[:, 1] - wv[1] * b[:, 0])
    d = np.where(full, dn, d)
    n = np.where(full[:, None], n, f32(0))
    V = np.where(full[:, None], V, f32(0))
    return np.concatenate([d[:, None], n, V], 1).astype(f32)


def _isless(b, a):
    """Julia's lexicographic isless on the rows of the (d, n, V) tuples (no NaNs arise here)"""
    less = np.zeros(a.shape[0], bool); eq = np.ones(a.shape[0], bool)
    for q in range(a.shape[1]):
        lq = (b[:, q] < a[:, q]) | ((b[:, q] == a[:, q]) & np.signbit(b[:, q]) & ~np.signbit(a[:, q]))
        eqq = (b[:, q] == a[:, q]) & (np.signbit(b[:, q]) == np.signbit(a[:, q]))
        less |= eq & lq; eq &= eqq
    return less


def _set_np(prog, X, fastd2, D):
    st = []
    for i in range(prog.n):
        nd = prog.node[i]
        if nd.op == 0:
            st.append(_leaf_np(nd, X, fastd2, D))
        elif nd.op == 3:
            t = st[-1].copy(); t[:, :D + 1] = -t[:, :D + 1]; st[-1] = t
        else:
            b, a = st.pop(), st.pop()
            less = _isless(b, a)
            take = less if nd.op == 1 else ~less
            st.append(np.where(take[:, None], b, a))
    return st[0]


def _measure_np(body, N, eps=1.0):
    """σ, μ₀, μ₁, V on the inside cells (src/Body.jl:28-48), in the kernel's order; one-leaf programs take σ = the raw sdf"""
    D = len(N)
    prog = body.program(D)
    I = np.stack(np.meshgrid(*[np.arange(2, n + 2) for n in N], indexing="ij"), -1).reshape(-1, D)
    X = (I - f32(1.5)).astype(f32)
    d2 = f32((2 + eps) * (2 + eps))
    if prog.n == 1:
        nd = prog.node[0]
        raw = _leaf_np(nd, X, np.inf, D)
        # raw sdf: the early exit at fastd² = −1 keeps d unnormalised
        dc = _leaf_np(nd, X, -1.0, D)[:, 0]
    else:
        dc = _set_np(prog, X, d2, D)[:, 0]
    M = X.shape[0]
    mu0 = np.ones((M, D), f32); mu1 = np.zeros((M, D, D), f32); V = np.zeros((M, D), f32)
    band = dc * dc < d2
    pi = f32(np.pi)
    for a in range(D):
        xf = X.copy(); xf[:, a] -= f32(0.5)
        t = _set_np(prog, xf, d2, D)
        di = t[:, 0]
        di = np.where(np.abs(di) <= f32(0.5), di, np.copysign(di, dc)).astype(f32)
        de = di / f32(eps)
        k0 = (1 + np.minimum(de, f32(1)) + np.sin(pi * np.minimum(de, f32(1))) / pi) / 2
        m0 = np.where(de < -1 + np.sqrt(np.spacing(np.abs(di))), f32(0), k0).astype(f32)
        dcl = np.clip(de, -1, 1).astype(f32)
        k1 = f32(eps) * ((1 - dcl * dcl) / 4 - (dcl * np.sin(pi * dcl) + (1 + np.cos(pi * dcl)) / pi) / (2 * pi))
        mu0[:, a] = np.where(band, m0, np.where(dc < 0, f32(0), f32(1)))
        V[:, a] = np.where(band, t[:, 1 + D + a], f32(0))
        for b in range(D):
            mu1[:, a, b] = np.where(band, k1 * t[:, 1 + b], f32(0))
    sh = tuple(N)
    return dc.reshape(sh, order="C"), mu0.reshape(sh + (D,)), mu1.reshape(sh + (D, D)), V.reshape(sh + (D,)), dc.reshape(sh)


def _bodies_for_fields(w):
    from waterlily_jl_amd.bodies import Body, RigidMap
    plate = Body(PLATE, RigidMap((20.0, 17.0), 0.7, omega=0.125))
    rm = RigidMap((19.0, 18.0), np.pi / 4, omega=1.0)
    annulus = Body(("sphere", (0.0, 0.0), 8.0), rm) - Body(("sphere", (0.0, 0.0), 4.5), rm)
    th = (0.2, -0.3, 0.5)
    box = None
    for q in range(3):
        for sgn in (1.0, -1.0):
            nrm = [0.0, 0.0, 0.0]; nrm[q] = sgn
            p = Body(("plane", tuple(sgn * 5.0 if k == q else 0.0 for k in range(3)), tuple(nrm)), RigidMap((12.0, 12.5, 11.0), th, V=(0.1, 0, 0), omega=(0, 0, 0.05)))
            box = p if box is None else box & p
    cyl = (Body(("cylinder", (0.0, 0.0, 0.0), 3.0, 2), RigidMap((10.0, 12.0, 12.0), (0.4, 0.0, 0.0), omega=(0.1, 0, 0)))
           | Body(("cylinder", (0.0, 0.0, 0.0), 3.0, 0), RigidMap((14.0, 12.0, 12.0), (0.0, 0.3, 0.2), xp=(1.0, 0, 0), omega=(0, 0.05, 0))))
    return [("plate2", plate, (40, 34)), ("annulus2", annulus, (40, 36)), ("box3", box, (24, 24, 24)), ("cylinders3", cyl, (24, 24, 24))]


@pytest.mark.parametrize("case", range(4))
def test_fields_against_a_restatement(w, case):
    name, body, N = _bodies_for_fields(w)[case]
    D = len(N)
    f = w.Flow(N, (1.0,) + (0.0,) * (D - 1))
    w.measure_(f, body)
    inner = tuple(slice(1, n + 1) for n in N)
    sg, m0, m1, V = (w.to_host(getattr(f, k)) for k in ("sigma", "mu0", "mu1", "V"))
    sg, m0, m1, V = sg[inner], m0[inner], m1[inner], V[inner]
    rs, r0, r1, rV, dc = _measure_np(body, N)
    for a in range(D):                                                        # BC!(μ₀, 0) and BC!(V, 0): the wall-normal face of the first cell
        idx = [slice(None)] * D; idx[a] = 0
        r0[tuple(idx) + (a,)] = 0; rV[tuple(idx) + (a,)] = 0
    assert np.abs(m0 < 1).sum() > 10, name                                    # the body is on the grid
    assert np.abs(sg - rs).max() <= 2e-6, name
    assert np.abs(m0 - r0).max() <= 2e-6 and np.abs(m1 - r1).max() <= 2e-6, name
    edge = np.abs(np.abs(dc) - 3.0) < 1e-4                                    # σ at the band edge (2+ϵ): V may be either value there
    ok = (V == rV) | (edge[..., None] & (V == 0))
    assert ok.all(), (name, np.abs(V - rV).max())
