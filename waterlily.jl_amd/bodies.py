"""Composite bodies — the device form of the reference's RigidMap (src/RigidMap.jl) and SetBody (src/Body.jl:91-107).

A body is a tree of leaves — closed-form shapes, or a distance field sampled on a lattice (SdfLattice) — each optionally under a rigid map, combined with `|` (∪, min), `&` (∩, max), unary `-`
and binary `-` (a ∩ (−b)).  `.program(D)` flattens it into the postfix wl_bodyset of include/wlhip.h; every measure!/force call
validates the program on the host before anything is launched.

    plate = Body(("capsule", (0, 0), 2, (1, 0), 6), map=RigidMap((16, 16), 1.0, omega=1 / 8))
    sim = Simulation((32, 32), (0, 0), 8, U=1, body=plate)
    sim.body = setmap(sim.body, theta=1.0 + t / 8); sim.sim_step_(remeasure=True)
"""
import ctypes as C

import numpy as np

from ._lib import WL_BODYSET_MAX, WL_BODYSET_STACK, check, lib, wl_bodyset

OP_LEAF, OP_UNION, OP_INTERSECT, OP_NEGATE = 0, 1, 2, 3
SPHERE, PLANE, CAPSULE, LATTICE = 1, 2, 3, 4
LATTICE_MAX = 8                                     # live lattices of a process (include/wlhip.h)
f32 = np.float32


def rotation(theta):
    """rotation(θ) of src/RigidMap.jl:50-53 in Float32: a 2x2 matrix for a scalar θ, 3x3 for the three Euler angles"""
    th = np.asarray(theta, dtype=f32)
    if th.ndim == 0:
        c, s = np.cos(th), np.sin(th)
        return np.array([[c, s], [-s, c]], dtype=f32)
    c1, c2, c3 = np.cos(th[0]), np.cos(th[1]), np.cos(th[2])
    s1, s2, s3 = np.sin(th[0]), np.sin(th[1]), np.sin(th[2])
    return np.array([[c3 * c2, c3 * s2 * s1 + s3 * c1, -c3 * s2 * c1 + s3 * s1],
                     [-s3 * c2, -s3 * s2 * s1 + c3 * c1, s3 * s2 * c1 + c3 * s1],
                     [s2, -c2 * s1, c2 * c1]], dtype=f32)


class RigidMap:
    """RigidMap(x₀, θ; xₚ, V, ω): map(x) = R̂(x−x₀−xₚ)+xₚ, velocity V + ω×(x−x₀−xₚ).  θ (and ω) scalar in 2-D, Euler angles in 3-D."""

    def __init__(self, x0, theta, xp=0, V=0, omega=0):
        self.x0 = np.asarray(x0, dtype=f32)
        D = len(self.x0)
        self.theta = f32(theta) if D == 2 else np.asarray(theta, dtype=f32)
        self.xp = np.broadcast_to(np.asarray(xp, dtype=f32), (D,)).copy()
        self.V = np.broadcast_to(np.asarray(V, dtype=f32), (D,)).copy()
        self.omega = f32(omega) if D == 2 else np.broadcast_to(np.asarray(omega, dtype=f32), (3,)).copy()
        self.R = rotation(self.theta)                     # R̂, precomputed as the reference does

    def replace(self, **kw):
        """setproperties(map; kw...) — R̂ recomputed (src/RigidMap.jl:55)"""
        a = dict(x0=self.x0, theta=self.theta, xp=self.xp, V=self.V, omega=self.omega)
        for k, v in kw.items():
            if k not in a:
                raise TypeError(f"RigidMap has no field {k!r}")
            a[k] = v
        return RigidMap(**a)


class AbstractBody:
    def __or__(self, other):
        return SetBody(OP_UNION, self, other)

    __add__ = __or__

    def __and__(self, other):
        return SetBody(OP_INTERSECT, self, other)

    def __neg__(self):
        return SetBody(OP_NEGATE, self, None)

    def __sub__(self, other):
        return self & (-other)

    def program(self, D):
        """the postfix wl_bodyset of this body (ValueError beyond WL_BODYSET_MAX nodes / WL_BODYSET_STACK stack entries)"""
        nodes = []
        self._emit(nodes, D)
        if len(nodes) > WL_BODYSET_MAX:
            raise ValueError(f"body has {len(nodes)} nodes, at most {WL_BODYSET_MAX} fit a wl_bodyset")
        depth = sp = 0
        for nd in nodes:
            sp += 1 if nd.op == OP_LEAF else (-1 if nd.op in (OP_UNION, OP_INTERSECT) else 0)
            depth = max(depth, sp)
        if depth > WL_BODYSET_STACK:
            raise ValueError(f"body needs an evaluation stack of {depth}, at most {WL_BODYSET_STACK}")
        s = wl_bodyset()
        s.n = len(nodes)
        for i, nd in enumerate(nodes):
            s.node[i] = nd
        return s


def _pad(v, n=3):
    v = [float(x) for x in np.atleast_1d(np.asarray(v, dtype=f32))]
    return v + [0.0] * (n - len(v))


class Body(AbstractBody):
    """A leaf: ("sphere", c, R) | ("cylinder", c, R, axis) | ("plane", point, normal) | ("capsule", c, R, axis_vector, h) |
    ("lattice", SdfLattice, origin, spacing, offset) — sdf(ξ) = interp((ξ − origin)/spacing, A) − offset: sample i sits at origin + spacing·(i − ½),
    the samples are distances in flow-grid cells whatever the spacing — optionally under a RigidMap (evaluated at ξ = map(x))."""

    def __init__(self, shape, map=None):
        self.shape, self.map = tuple(shape), map

    def _emit(self, nodes, D):
        from ._lib import wl_body_node
        name = self.shape[0]
        nd = wl_body_node()
        nd.op = OP_LEAF
        c, h = self.shape[1], 0.0
        if name == "sphere":
            nd.kind, R, m = SPHERE, self.shape[2], [1.0] * D
        elif name == "cylinder":
            nd.kind, R, m = SPHERE, self.shape[2], [0.0 if k == int(self.shape[3]) else 1.0 for k in range(D)]
        elif name == "plane":
            nd.kind, R, m = PLANE, 0.0, self.shape[2]
        elif name == "capsule":
            nd.kind, R, m, h = CAPSULE, self.shape[2], self.shape[3], self.shape[4]
        elif name == "lattice":
            lat, c, spacing = self.shape[1], self.shape[2], self.shape[3]
            if lat.D != D:
                raise ValueError(f"a {lat.D}-D lattice in a {D}-D body program")
            if not float(spacing) > 0:
                raise ValueError("lattice spacing must be > 0")
            c = np.broadcast_to(np.asarray(c, dtype=f32), (D,))
            nd.kind, R, m, h = LATTICE, (self.shape[4] if len(self.shape) > 4 else 0.0), [spacing], lat.id      # the id travels as a float: a small integer, exact
        else:
            raise ValueError(f"unknown body {name!r}")
        nd.c[:] = _pad(c)
        nd.R, nd.h = float(R), float(h)
        nd.m[:] = _pad(m)
        if self.map is not None:
            mp = self.map
            nd.mapped = 1
            nd.map.x0[:] = _pad(mp.x0)
            nd.map.xp[:] = _pad(mp.xp)
            nd.map.V[:] = _pad(mp.V)
            nd.map.w[:] = _pad(mp.omega)
            R3 = np.zeros((3, 3), dtype=f32)
            R3[:D, :D] = mp.R[:D, :D]
            nd.map.R[:] = [float(v) for v in R3.reshape(-1)]
        nodes.append(nd)

    def setmap(self, **kw):
        if self.map is None:
            raise ValueError("setmap: this leaf has no RigidMap")
        return Body(self.shape, self.map.replace(**kw))


class SdfLattice:
    """A sampled distance field on the device (wl_sdf_lattice of include/wlhip.h): what measure_sdf!(a, body) leaves in a scalar array — distances in
    flow-grid cells at the cell centres of the lattice's own grid, one ghost layer included.  Owns the handle: close() — or leaving a `with` block —
    destroys it (waits for the device); a program that still names it is then refused.  At most LATTICE_MAX are alive in a process.

        with SdfLattice(values) as lat:                       # values: (n_x, n_y[, n_z]) floats, every extent >= 3
            hull = Body(("lattice", lat, origin, spacing, 0.0), map=RigidMap(x0, theta))
    """

    def __init__(self, values):
        a = np.asarray(values, dtype=f32)
        if a.ndim not in (2, 3):
            raise ValueError("SdfLattice: values must be a 2-D or 3-D array")
        self.D, self.dims = a.ndim, tuple(int(n) for n in a.shape)
        self.edge_min = edge_min(a) if min(self.dims) >= 3 else 0.0
        flat = np.ascontiguousarray(a.reshape(-1, order="F"))        # first index fastest, as every array of the library
        h = C.c_void_p()
        self._h = None
        check(lib().wl_sdf_lattice_create(C.byref(h), self.D, (C.c_int32 * self.D)(*self.dims), flat.ctypes.data_as(C.POINTER(C.c_float)), None))
        self._h = h
        self.id = int(lib().wl_sdf_lattice_id(h))

    def close(self):
        if self._h is not None:
            h, self._h = self._h, None
            check(lib().wl_sdf_lattice_destroy(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:      # interpreter shutdown: the library may be gone already
            pass

    @staticmethod
    def centres(dims, origin=0, spacing=1):
        """the positions of the samples of a lattice of `dims` samples: origin + spacing·(i − ½), as (prod(dims), D) Float32 rows, first index fastest"""
        D = len(dims)
        o = np.broadcast_to(np.asarray(origin, dtype=f32), (D,))
        ax = [(o[q] + f32(spacing) * (np.arange(dims[q], dtype=f32) - f32(0.5))).astype(f32) for q in range(D)]
        g = np.meshgrid(*ax, indexing="ij")
        return np.stack([v.reshape(-1, order="F") for v in g], axis=1)

    @classmethod
    def bake(cls, body, dims, origin=0, spacing=1):
        """sample an existing body program at the lattice's cell centres — measure_sdf!(a, body): d alone, fastd² = 0 — through the device's point probe;
        Body(("lattice", bake(body, dims, origin, spacing), origin, spacing)) then stands where `body` stood"""
        d, _, _ = measure(body, cls.centres(dims, origin, spacing), fastd2=0.0)
        return cls(d.reshape(tuple(dims), order="F"))


def edge_min(values):
    """min |A| over the samples a clamped query reads — the two outermost layers of every direction — or 0 where they differ in sign (include/wlhip.h, out of
    range): outside the lattice's box |sdf| >= edge_min − |offset|"""
    a = np.asarray(values, dtype=f32)
    edge = np.zeros(a.shape, dtype=bool)
    for q in range(a.ndim):
        ix = [slice(None)] * a.ndim
        for sl in (slice(0, 2), slice(-2, None)):
            ix[q] = sl
            edge[tuple(ix)] = True
    v = a[edge]
    return 0.0 if (v > 0).any() and (v < 0).any() else float(np.abs(v).min())


def lattice_margin_ok(body, D, need):
    """the out-of-range rule of include/wlhip.h for `body`: every lattice leaf keeps edge_min − |offset| > need (2 + ϵ + 1 for measure!, 2 for the forces)"""
    return all(f32(b.shape[1].edge_min) - abs(f32(b.shape[4] if len(b.shape) > 4 else 0.0)) > f32(need) for b in leaves(body) if b.shape[0] == "lattice")


class SetBody(AbstractBody):
    """SetBody(op, a, b): op ∈ (OP_UNION, OP_INTERSECT, OP_NEGATE); b is None for a negation"""

    def __init__(self, op, a, b):
        self.op, self.a, self.b = op, a, b

    def _emit(self, nodes, D):
        from ._lib import wl_body_node
        self.a._emit(nodes, D)
        if self.b is not None:
            self.b._emit(nodes, D)
        nd = wl_body_node()
        nd.op = self.op
        nodes.append(nd)

    def setmap(self, **kw):
        """setmap(body::SetBody; kw...) reaches every leaf   src/RigidMap.jl:57"""
        return SetBody(self.op, self.a.setmap(**kw), None if self.b is None else self.b.setmap(**kw))


def setmap(body, **kw):
    """setmap(body; x0, theta, xp, V, omega): a copy of `body` whose rigid maps carry the new values (R̂ recomputed)"""
    return body.setmap(**kw)


def leaves(body):
    """the leaves of a body, left to right"""
    return [body] if isinstance(body, Body) else leaves(body.a) + ([] if body.b is None else leaves(body.b))


def measure(body, points, fastd2=np.inf):
    """measure(body, x; fastd²) at every row of `points` (npts × D) on the device -> d (npts), n (npts × D), V (npts × D)"""
    x = np.ascontiguousarray(points, dtype=f32)
    if x.ndim == 1:
        x = x[None, :]
    npts, D = x.shape
    prog = body.program(D)
    d = np.zeros(npts, dtype=f32)
    n = np.zeros((npts, D), dtype=f32)
    V = np.zeros((npts, D), dtype=f32)
    fp = C.POINTER(C.c_float)
    check(lib().wl_bodyset_measure_points(C.byref(prog), D, x.ctypes.data_as(fp), npts, float(fastd2), d.ctypes.data_as(fp),
                                          n.ctypes.data_as(fp), V.ctypes.data_as(fp), None))
    return d, n, V
