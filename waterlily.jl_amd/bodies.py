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
        self.vertices = None                                         # not from a mesh
        flat = np.ascontiguousarray(a.reshape(-1, order="F"))        # first index fastest, as every array of the library
        h = C.c_void_p()
        self._h = None
        check(lib().wl_sdf_lattice_create(C.byref(h), self.D, (C.c_int32 * self.D)(*self.dims), flat.ctypes.data_as(C.POINTER(C.c_float)), None))
        self._h = h
        self.id = int(lib().wl_sdf_lattice_id(h))

    @classmethod
    def from_mesh(cls, vertices, elems, dims, origin=0, spacing=1, brute=False, vertex_velocity=None, band=None):
        """the exact signed distance to a closed surface, sampled on the device (wl_sdf_lattice_from_mesh): `vertices` (nv × D) in the body frame, in flow-grid
        cells; `elems` (ne × 3) triangles in 3-D, (ne × 2) segments of closed polygons in 2-D, oriented outward (counter-clockwise seen from the fluid);
        sample i sits at origin + spacing·(i − ½), as for centres().  Negative inside.  brute=True tests every (sample, element) pair instead of culling: the
        same bits, for tests and timings.  A mesh that is open, non-manifold, unwelded (see weld) or oriented inward raises WlError with the reason.
        `vertex_velocity` (nv × D, body frame, cells per unit time) makes a DEFORMING body of it (wl_sdf_lattice_from_moving_mesh): the lattice also samples
        the velocity of the closest surface point, the leaf adds it to V, and update_mesh / advance re-bake it in place as the vertices move.
        `band` (a positive number, flow-grid cells; wl_sdf_lattice_from_mesh_band) makes the lattice the full one clipped to ±band, with zero velocity samples
        beyond it: the search skips the bricks wholly beyond the band, and every re-bake keeps the band.  measure! and the forces then also ask
        band − |offset| > need + spacing·√D (mesh_band gives the smallest band with a quarter cell to spare).  band=None: today's call, today's bits."""
        v = np.ascontiguousarray(vertices, dtype=f32)
        e = np.ascontiguousarray(elems, dtype=np.int32)
        if v.ndim != 2 or v.shape[1] not in (2, 3) or e.ndim != 2 or e.shape[1] != v.shape[1]:
            raise ValueError("from_mesh: vertices must be (nv, D) and elems (ne, D) — triangles in 3-D, segments in 2-D")
        D = v.shape[1]
        dims = tuple(int(n) for n in dims)
        if len(dims) != D:
            raise ValueError(f"from_mesh: {len(dims)} extents for a {D}-D mesh")
        o = np.ascontiguousarray(np.broadcast_to(np.asarray(origin, dtype=f32), (D,)))
        self = cls.__new__(cls)
        self.D, self.dims, self._h = D, dims, None
        h = C.c_void_p()
        fp = C.POINTER(C.c_float)
        if band is not None:
            wv = None if vertex_velocity is None else self._velocity_rows(vertex_velocity, v)
            check(lib().wl_sdf_lattice_from_mesh_band(C.byref(h), D, (C.c_int32 * D)(*dims), o.ctypes.data_as(fp), float(spacing), v.ctypes.data_as(fp), len(v),
                                                      e.ctypes.data_as(C.POINTER(C.c_int32)), len(e), None if wv is None else wv.ctypes.data_as(fp),
                                                      float(band), 1 if brute else 0, None))
        elif vertex_velocity is None:
            check(lib().wl_sdf_lattice_from_mesh(C.byref(h), D, (C.c_int32 * D)(*dims), o.ctypes.data_as(fp), float(spacing),
                                                 v.ctypes.data_as(fp), len(v), e.ctypes.data_as(C.POINTER(C.c_int32)), len(e), 1 if brute else 0, None))
        else:
            wv = self._velocity_rows(vertex_velocity, v)
            check(lib().wl_sdf_lattice_from_moving_mesh(C.byref(h), D, (C.c_int32 * D)(*dims), o.ctypes.data_as(fp), float(spacing), v.ctypes.data_as(fp), len(v),
                                                        e.ctypes.data_as(C.POINTER(C.c_int32)), len(e), wv.ctypes.data_as(fp), 1 if brute else 0, None))
        self._h = h
        self.id = int(lib().wl_sdf_lattice_id(h))
        self.edge_min = float(lib().wl_sdf_lattice_edge_min(h))      # recorded by the library from the samples it made
        self.vertices = v.copy()                                     # of the last bake: what advance differences against
        return self

    @staticmethod
    def _velocity_rows(vertex_velocity, v):
        wv = np.ascontiguousarray(vertex_velocity, dtype=f32)
        if wv.shape != v.shape:
            raise ValueError(f"vertex_velocity must have the shape of the vertices {v.shape}, not {wv.shape}")
        return wv

    def _live(self, who):
        if self._h is None:
            raise ValueError(f"SdfLattice.{who}: the lattice has been closed")
        return self._h

    @property
    def band(self):
        """the band the lattice was made with (wl_sdf_lattice_band): 0.0 without one, or once the lattice is closed"""
        return 0.0 if self._h is None else float(lib().wl_sdf_lattice_band(self._h))

    @property
    def has_velocity(self):
        """whether the lattice carries velocity samples (wl_sdf_lattice_has_velocity)"""
        return self._h is not None and bool(lib().wl_sdf_lattice_has_velocity(self._h))

    def update_mesh(self, vertices, vertex_velocity=None, brute=False):
        """re-bake this lattice IN PLACE from moved vertices (wl_sdf_lattice_update_mesh): the connectivity of its creation, the same id, dims, origin and
        spacing — every body, recorder and handle that names it picks the new shape up at its next launch (sim_step_(remeasure=True)).  vertex_velocity=None
        stores zero velocities (on a lattice made with velocity samples).  A refused update (WlError: an inverted or degenerate mesh, a non-finite value,
        a lattice not from a mesh) changes nothing."""
        h = self._live("update_mesh")
        if self.vertices is None:
            raise ValueError("SdfLattice.update_mesh: the lattice was not made from a mesh")
        v = np.ascontiguousarray(vertices, dtype=f32)
        if v.shape != self.vertices.shape:
            raise ValueError(f"update_mesh: vertices must keep the shape {self.vertices.shape} of the lattice's mesh, not {v.shape}")
        fp = C.POINTER(C.c_float)
        wv = None if vertex_velocity is None else self._velocity_rows(vertex_velocity, v)
        check(lib().wl_sdf_lattice_update_mesh(h, v.ctypes.data_as(fp), None if wv is None else wv.ctypes.data_as(fp), 1 if brute else 0, None))
        self.edge_min = float(lib().wl_sdf_lattice_edge_min(h))
        self.vertices = v.copy()

    def advance(self, new_vertices, dt):
        """move the surface to `new_vertices` over the time dt: vertex velocities (new − vertices)/dt in Float32, then update_mesh — one call per time step
        of a deforming body"""
        if self.vertices is None:
            raise ValueError("SdfLattice.advance: the lattice was not made from a mesh")
        new = np.ascontiguousarray(new_vertices, dtype=f32)
        if new.shape != self.vertices.shape:
            raise ValueError(f"advance: vertices must keep the shape {self.vertices.shape} of the lattice's mesh, not {new.shape}")
        self.update_mesh(new, ((new - self.vertices) / f32(dt)).astype(f32))

    def set_velocity(self, W):
        """attach or replace the velocity samples from W of shape dims + (D,) (wl_sdf_lattice_set_velocity) — on any lattice, from any tool"""
        h = self._live("set_velocity")
        W = np.asarray(W, dtype=f32)
        if W.shape != self.dims + (self.D,):
            raise ValueError(f"set_velocity: W must have the shape {self.dims + (self.D,)}, not {W.shape}")
        flat = np.ascontiguousarray(W.reshape(-1, order="F"))          # component-major, first index fastest inside a plane
        check(lib().wl_sdf_lattice_set_velocity(h, flat.ctypes.data_as(C.POINTER(C.c_float)), None))

    def velocity(self):
        """the velocity samples as an ndarray of shape dims + (D,), read back from the device (wl_sdf_lattice_read_velocity)"""
        h = self._live("velocity")
        flat = np.empty(int(np.prod(self.dims)) * self.D, dtype=f32)
        check(lib().wl_sdf_lattice_read_velocity(h, flat.ctypes.data_as(C.POINTER(C.c_float)), None))
        return flat.reshape(self.dims + (self.D,), order="F")

    def values(self):
        """the samples as an ndarray of shape `dims`, read back from the device (wl_sdf_lattice_read)"""
        if self._h is None:
            raise ValueError("SdfLattice.values: the lattice has been closed")
        flat = np.empty(int(np.prod(self.dims)), dtype=f32)
        check(lib().wl_sdf_lattice_read(self._h, flat.ctypes.data_as(C.POINTER(C.c_float)), None))
        return flat.reshape(self.dims, order="F")

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


def mesh_placement(vertices, spacing=1.0, margin=5.0):
    """the lattice mesh_body lays around the bounding box of `vertices`: (dims, origin) with origin_d = lo_d − margin − spacing/2 and
    n_d = ceil((hi_d − lo_d + 2·margin)/spacing) + 3, so that samples 1 and n_d − 2 sit at least `margin` outside the box"""
    v = np.asarray(vertices, dtype=np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    dims = tuple(int(np.ceil((hi[d] - lo[d] + 2.0 * margin) / spacing)) + 3 for d in range(v.shape[1]))
    return dims, tuple(float(lo[d] - margin - spacing / 2.0) for d in range(v.shape[1]))


def mesh_band(eps=1.0, offset=0.0, spacing=1.0, D=3):
    """the smallest band with a quarter cell to spare over the band rule of include/wlhip.h for measure! at ϵ = eps: 2 + eps + 1 + |offset| + spacing·√D + ¼"""
    return 2.0 + float(eps) + 1.0 + abs(float(offset)) + float(spacing) * float(np.sqrt(float(D))) + 0.25


def mesh_body(vertices, elems, spacing=1.0, margin=None, offset=0.0, map=None, vertex_velocity=None, band=None):
    """A closed triangle mesh (2-D: closed polygons of segments) as a body: its exact signed distance sampled at `spacing` into a lattice around its
    bounding box (SdfLattice.from_mesh, mesh_placement) and the lattice leaf over it — Body(("lattice", lat, origin, spacing, offset), map).  Vertices are
    in the body frame, in flow-grid cells; `map` places and moves the body.  The lattice every sample of which lies `margin` or more outside the box has
    edge_min ≥ margin; margin=None takes 5 + |offset|, which satisfies measure!'s rule edge_min − |offset| > 2 + ϵ + 1 at ϵ = 1 — a larger ϵ needs a
    larger margin (ϵ + 4 + |offset|).  The lattice is the body's: body.shape[1].close() frees it (at most LATTICE_MAX are alive).  With `vertex_velocity`
    (nv × D) the body deforms: body.shape[1].advance(new_vertices, dt) re-bakes it in place each step — lay the lattice (margin) around every shape it takes.
    `band`: a number is passed to from_mesh; True takes mesh_band(1.0, offset, spacing, D).  The margin default stays: edge_min is then min(margin-ish, band),
    which the edge rule accepts whenever the band rule does."""
    margin = 5.0 + abs(float(offset)) if margin is None else float(margin)
    dims, origin = mesh_placement(vertices, float(spacing), margin)
    if band is True:
        band = mesh_band(1.0, offset, spacing, np.asarray(vertices).shape[1])
    lat = SdfLattice.from_mesh(vertices, elems, dims, origin, spacing, vertex_velocity=vertex_velocity, band=band)
    return Body(("lattice", lat, origin, float(spacing), float(offset)), map)


def weld(vertices, faces):
    """merge exactly equal vertex rows and re-index: (vertices, faces) with every position named once, in order of first appearance — what a triangle soup
    (an STL file) needs before from_mesh can tell which triangles share an edge"""
    v = np.asarray(vertices)
    f = np.asarray(faces)
    # (−0.0 and +0.0 are the same position)
    _, first, inverse = np.unique(v + v.dtype.type(0), axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first)                      # unique rows in order of first appearance
    rank = np.empty_like(order); rank[order] = np.arange(len(order))
    return v[first[order]], rank[np.asarray(inverse).reshape(-1)][f].astype(np.int32)


def read_stl(path):
    """a binary STL file as welded (vertices (nv × 3) Float32, faces (ne × 3) int32); the file's normals are ignored (the index order orients a triangle).
    An ASCII STL raises ValueError."""
    with open(path, "rb") as fh:
        raw = fh.read()
    n = int(np.frombuffer(raw[80:84], dtype="<u4")[0]) if len(raw) >= 84 else -1
    if n < 0 or len(raw) != 84 + 50 * n:
        if raw[:5].lower() == b"solid":
            raise ValueError(f"{path}: an ASCII STL file — only binary STL is read (convert it first)")
        raise ValueError(f"{path}: not a binary STL file ({len(raw)} bytes, header says {n} triangles)")
    rec = np.frombuffer(raw, dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]), count=n, offset=84)
    return weld(rec["v"].reshape(-1, 3).astype(f32), np.arange(3 * n, dtype=np.int32).reshape(n, 3))


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
