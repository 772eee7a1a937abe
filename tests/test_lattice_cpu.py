"""The lattice leaf of a body program without a GPU: the NumPy restatement (tests/lattice_ref.py) against its own finite differences and against the plane
leaf on linear data, the out-of-range rule, the node packing of Body(("lattice", …)), and that every case tests/test_gpu_lattice.py measures holds the
classes of points it is there for."""
import ctypes as C

import numpy as np
import pytest

import forces_ref as fr
import lattice_ref as lr
from waterlily_jl_amd import bodies
from waterlily_jl_amd._lib import WL_BODYSET_MAX, wl_body_node, wl_bodyset
from waterlily_jl_amd.bodies import Body, RigidMap

f32, f64 = np.float32, np.float64


def _away_from_planes(rng, lo, hi, n, origin, s, dims, margin=0.05):
    """n points in [lo, hi) whose lattice coordinates stay `margin` (in cells of the lattice) away from every node plane (q = i − ½) and from the clamp's
    bounds (q = 0, n_d − 2)"""
    D = len(dims)
    out = []
    while len(out) < n:
        x = rng.uniform(lo, hi, size=D)
        q = (x - origin) / s
        far_node = np.abs((q + 0.5) - np.round(q + 0.5)) >= margin
        far_clamp = (np.abs(q) >= margin) & (np.abs(q - (np.asarray(dims) - 2)) >= margin)
        if far_node.all() and far_clamp.all():
            out.append(x)
    return np.array(out)


@pytest.mark.parametrize("dims,s", [((9, 8, 7), 1.0), ((9, 8, 7), 2.0), ((9, 8, 7), 0.5), ((10, 9), 1.25)])
def test_gradient_equals_central_differences_of_the_value(dims, s):
    """random samples (nothing smooth about them): inside a cell the value is multilinear, so a central difference that stays inside the cell is exact up to
    rounding; a clamped direction has derivative 0"""
    rng = np.random.default_rng(3)
    D = len(dims)
    A = rng.uniform(-3, 3, size=dims).astype(f32)
    origin = np.array((0.75, -1.5, 2.0)[:D])
    lo, hi = origin - 2.5 * s, origin + s * (np.array(dims) - 2) + 2.5 * s
    X = _away_from_planes(rng, lo, hi, 400, origin, s, dims)
    # float32-exact inputs, as the restatement takes them
    X = X.astype(f32).astype(f64)
    origin32 = origin.astype(f32)
    val = lambda P: lr.ir._interp_scalar(((P - origin32.astype(f64)) / f64(f32(s))), A, f64)      # noqa: E731
    q = (X - origin32.astype(f64)) / f64(f32(s))
    g = np.where(lr.clamp_active(q, dims), 0.0, lr.interp_grad(q, A, f64) / f64(f32(s)))
    h = 0.01 * s
    clamped = lr.clamp_active(q, dims)
    assert (clamped.sum(axis=1) == 0).sum() > 50 and clamped.any(axis=0).all()
    for d in range(D):
        e = np.zeros(D); e[d] = h
        fd = (val(X + e) - val(X - e)) / (2 * h)
        assert np.abs(fd - g[:, d]).max() <= 1e-9 * max(1.0, np.abs(g).max()), d


def test_linear_data_returns_the_plane():
    """samples of m·x + b at spacing 2: the gradient with respect to ξ is m (index differences m·s, divided by s), so n = m/|m| and d = (m·x + b)/|m| —
    what the plane leaf gives (this is the m ≠ 1 of d /= m)"""
    m, p0 = np.array((0.6, -1.5, 0.8)), np.array((7.0, 6.0, 5.0))
    dims, origin, s = (10, 9, 8), (-1.0, 0.5, 0.0), 2.0
    P = lr.sample_positions(dims, origin, s)
    A = sum(m[k] * (P[k].astype(f64) - p0[k]) for k in range(3)).astype(f32)
    b = lr.lattice_body(lr.HostLattice(A), origin, s)
    rng = np.random.default_rng(1)
    X = rng.uniform((0.0, 1.5, 1.0), (13.0, 13.5, 11.0), size=(200, 3)).astype(f32)
    assert lr.classes(b, X)["inside"] == 200
    plane = fr._leaf(Body(("plane", tuple(p0), tuple(m))), [X[:, k] for k in range(3)], np.inf)
    d64, n64, _ = lr.points(b, X, T=f64)
    d32, n32, _ = lr.points(b, X, T=f32)
    mm = np.sqrt((m ** 2).sum())
    assert mm > 1.5                                              # |∇sdf| is far from 1: d /= m does real work
    assert np.abs(n64 - m / mm).max() <= 1e-6                    # (the samples are Float32: their rounding is all that separates the two)
    assert np.abs(d64 - plane[0]).max() <= 1e-5 and np.abs(n64 - np.stack(plane[1:4], axis=1)).max() <= 1e-6
    assert np.abs(d32 - d64).max() <= 1e-5 and np.abs(n32 - n64).max() <= 1e-5


def test_edge_rule():
    A = np.full((8, 7, 6), 9.0, dtype=f32)
    A[3, 3, 3] = -1.0                                            # the inside does not count
    assert bodies.edge_min(A) == 9.0
    A[1, 3, 3] = 4.5                                             # second layer: a clamped query reads it
    assert bodies.edge_min(A) == 4.5
    A[2, 3, 3] = 0.5                                             # third layer: it does not
    assert bodies.edge_min(A) == 4.5
    lat = lr.HostLattice(A)
    assert lat.edge_min == 4.5
    for off, measure_ok, force_ok in [(0.0, True, True), (0.5, False, True), (-0.5, False, True), (2.5, False, False), (-2.6, False, False)]:
        b = lr.lattice_body(lat, 0.0, 1.0, off) | Body(("sphere", (3.0, 3.0, 3.0), 1.0))
        assert bodies.lattice_margin_ok(b, 3, 2 + 1.0 + 1) == measure_ok, off      # edge_min − |R| > 2 + ϵ + 1
        assert bodies.lattice_margin_ok(b, 3, 2) == force_ok, off                  # edge_min − |R| > 2
    A[0, 0, 0] = -9.0                                            # mixed signs on the edge: no bound holds
    assert bodies.edge_min(A) == 0.0
    # the rule's reason: outside the box the restatement's |d| never falls below edge_min − |R|
    rng = np.random.default_rng(2)
    B = rng.uniform(3.0, 8.0, size=(8, 7, 6)).astype(f32)
    lb = lr.lattice_body(lr.HostLattice(B), 0.0, 1.0, 0.25)
    X = rng.uniform(-6.0, 12.0, size=(4000, 3)).astype(f32)
    q, _ = lr.lattice_coords(lb, [X[:, k] for k in range(3)])
    out = lr.clamp_active(q, B.shape).any(axis=1)
    d = lr.leaf(lb, [X[:, k] for k in range(3)], -1.0)[0]
    assert out.sum() > 1000 and np.abs(d[out]).min() >= bodies.edge_min(B) - 0.25 - 1e-5


def test_node_packing():
    assert C.sizeof(wl_body_node) == 128 and C.sizeof(wl_bodyset) == 4 + WL_BODYSET_MAX * 128 and WL_BODYSET_MAX == 16
    offs = {n: getattr(wl_body_node, n).offset for n in ("op", "kind", "c", "R", "m", "h", "mapped", "map")}
    assert offs == dict(op=0, kind=4, c=8, R=20, m=24, h=36, mapped=40, map=44)
    A = np.ones((5, 4, 3), dtype=f32)
    mp = RigidMap((1.0, 2.0, 3.0), (0.1, 0.2, 0.3), V=(0.5, 0, 0), omega=(0, 0, 0.25))
    for id in (1, 7, 1000, 2 ** 24 - 1):
        prog = Body(("lattice", lr.HostLattice(A, id=id), (1.5, -2.0, 0.25), 1.25, 0.75), map=mp).program(3)
        nd = prog.node[0]
        assert prog.n == 1 and nd.op == bodies.OP_LEAF and nd.kind == bodies.LATTICE == 4
        assert list(nd.c) == [1.5, -2.0, 0.25] and nd.R == 0.75 and list(nd.m) == [1.25, 0.0, 0.0]
        assert nd.h == float(id) and int(nd.h) == id             # the id round-trips through the float
        assert nd.mapped == 1 and list(nd.map.x0) == [1.0, 2.0, 3.0] and list(nd.map.w) == [0.0, 0.0, 0.25]
    lat = lr.HostLattice(A, id=3)
    leafb = Body(("lattice", lat, 0.0, 1.0))                     # scalar origin, default offset
    nd = leafb.program(3).node[0]
    assert list(nd.c) == [0.0, 0.0, 0.0] and nd.R == 0.0 and nd.mapped == 0
    prog = ((leafb | Body(("capsule", (1.0, 1.0, 1.0), 1.0, (1.0, 0.0, 0.0), 2.0))) - Body(("sphere", (0.0, 0.0, 0.0), 1.0))).program(3)
    assert [prog.node[i].op for i in range(prog.n)] == [0, 0, 1, 0, 3, 2] and prog.node[0].kind == 4
    moved = bodies.setmap(Body(("lattice", lat, 0.0, 1.0), map=mp), x0=(4.0, 5.0, 6.0)).program(3).node[0]
    assert moved.kind == 4 and list(moved.map.x0) == [4.0, 5.0, 6.0] and moved.h == 3.0
    with pytest.raises(ValueError):
        Body(("lattice", lat, 0.0, 1.0)).program(2)              # a 3-D lattice in a 2-D program
    with pytest.raises(ValueError):
        Body(("lattice", lat, 0.0, 0.0)).program(3)              # spacing must be > 0


@pytest.mark.parametrize("name", sorted(lr.POINT_CASES))
def test_point_cases_hold_the_classes_they_claim(name):
    c = lr.point_case(name)
    assert max(c["dims"]) <= 20 and np.prod(c["dims"]) <= 20 * 18 * 16
    b = c["body"](lr.HostLattice(c["values"]))
    got = lr.classes(b, c["X"], lr.FASTD2)
    for k in c["claims"]:
        assert got[k] >= 5, (name, k, got)
    d32, n32, _ = lr.points(b, c["X"], lr.FASTD2, f32)
    d64, n64, _ = lr.points(b, c["X"], lr.FASTD2, f64)
    assert np.isfinite(n32).all() and np.isfinite(d32).all()
    assert lr.bound(d32, d64) < 1e-3 and lr.bound(n32, n64) < 1e-4, name      # no point sits on a kink of one precision and not the other: the bound means something


@pytest.mark.parametrize("name", sorted(lr.FIELD_CASES))
def test_field_cases_end_inside_the_domain_and_keep_the_rule(name):
    c = lr.field_case(name)
    lat = lr.HostLattice(c["values"])
    b = c["body"](lat)
    assert bodies.lattice_margin_ok(b, len(c["grid"]), 2 + 1.0 + 1), lat.edge_min
    got = lr.grid_classes(b, c["Ng"])
    assert got["inside"] > 100 and got["clamped"] > 100 and got["band"] > 50 and got["band_clamped"] == 0, got
    if name == "sphere3":                                        # the handle case: still so after the five remeasured steps (t < 2)
        b2 = c["body"](lat, 2.0)
        assert lr.grid_classes(b2, c["Ng"])["band_clamped"] == 0
