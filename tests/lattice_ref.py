"""NumPy restatement of the lattice leaf of a body program (include/wlhip.h, sampled bodies; waterlily.jl_amd/csrc/wl_lattice.hpp) — the yardstick of
tests/test_lattice_cpu.py and tests/test_gpu_lattice.py.

The leaf is the reference body AutoBody((ξ,t) -> interp((ξ .- c) ./ s, A) - R, map) measured by measure(::AutoBody, x, t; fastd²) (src/AutoBody.jl:29-37):
  value     d = interp(q, A) − R, q = (ξ − c)/s — interp through tests/interp_ref.py (clamp, + 1.5, floor, corners in CartesianIndices order, weights left to right)
  gradient  what ForwardDiff gives through _interp with i = floor(x) held fixed: g_d = (Σ_J A[J]·(±1)_d·Π_{e≠d} w_e(J))/s over the same corners in the same
            order, the factors e ≠ d multiplied on left to right starting from the sign; g_d = 0 where the clamp moves q_d
  then      the NaN test, n = R̂ᵀg, m = |n|, d /= m, n /= m, V = V₀ + ω×(x − x₀ − xₚ) — the statements of every leaf (tests/forces_ref.py _leaf)
T = float32 keeps the device's operation order; T = float64 is the same formula on the same float32 inputs, the value the error bound is measured from.

A lattice here is anything with .values (the samples, indexed [x, y(, z)]), .D, .edge_min and .id: HostLattice below without a device, a w.SdfLattice that the
test gave its .values on one.  Importing this module teaches tests/forces_ref.py the leaf (its _leaf is wrapped), so that its measure, band, terms, sums and
tolerances evaluate programs that contain one."""
import numpy as np

import forces_ref as fr
import interp_ref as ir
from waterlily_jl_amd.bodies import Body, edge_min

f32 = np.float32


class HostLattice:
    """a lattice without a device: the samples and what w.SdfLattice keeps of them"""

    def __init__(self, values, id=1):
        self.values = np.asarray(values, dtype=f32)
        self.D, self.dims, self.id = self.values.ndim, self.values.shape, id
        self.edge_min = edge_min(self.values)


def clamp_active(q, shape):
    """(n, D) bool: _interp_clamp moves q_d (strictly outside [0, n_d − 2]; a coordinate on the bound keeps its derivative)"""
    return np.stack([~((q[:, d] >= 0) & (q[:, d] <= q.dtype.type(shape[d] - 2))) for d in range(q.shape[1])], axis=1)


def interp_grad(q, A, T):
    """∂interp(q, A)/∂q for (n, D) points q of type T, the floor held fixed; not yet zeroed where the clamp is active"""
    n, D = q.shape
    y = np.empty((n, D), dtype=T)
    i0 = np.empty((n, D), dtype=np.int64)
    for d in range(D):
        c = np.clip(q[:, d], T(0), T(A.shape[d] - 2))
        c = (c + T(1.5)).astype(T)
        fl = np.floor(c)
        y[:, d] = (c - fl).astype(T)
        i0[:, d] = fl.astype(np.int64) - 1
    a = A.astype(T)
    g = np.zeros((n, D), dtype=T)
    for k in range(1 << D):
        v = a[tuple(i0[:, d] + ((k >> d) & 1) for d in range(D))]
        for d in range(D):
            w = np.full(n, 1 if (k >> d) & 1 else -1, dtype=T)
            for e in range(D):
                if e != d:
                    w = (w * (y[:, e] if (k >> e) & 1 else (T(1) - y[:, e]).astype(T))).astype(T)
            g[:, d] = (g[:, d] + (v * w).astype(T)).astype(T)
    return g


def _seqsum(terms):
    s = np.zeros_like(terms[0])
    for t in terms:
        s = s + t
    return s


def lattice_coords(b, x, T=f32):
    """(q, bq): the lattice coordinates (n, D) of the points x (a list of D equal-shaped arrays) and x − x₀ − xₚ (zeros without a map)"""
    D = len(x)
    x = [np.asarray(v, dtype=f32).astype(T).reshape(-1) for v in x]
    c = np.broadcast_to(np.asarray(b.shape[2], dtype=f32), (D,)).astype(T)
    s = T(f32(b.shape[3]))
    mp = b.map
    if mp is not None:
        bq = [(x[k] - T(mp.x0[k])) - T(mp.xp[k]) for k in range(D)]
        xi = [_seqsum([T(mp.R[k, r]) * bq[r] for r in range(D)]) + T(mp.xp[k]) for k in range(D)]
    else:
        bq, xi = [np.zeros_like(x[0])] * D, x
    return np.stack([((xi[k] - c[k]) / s).astype(T) for k in range(D)], axis=1), bq


def leaf(b, x, fastd2=np.inf, T=f32):
    """measure(leaf, x; fastd²) of Body(("lattice", lat, origin, spacing[, offset]), map) -> [d, n_1..n_D, V_1..V_D], each shaped like x[0]"""
    D, shape = len(x), np.shape(x[0])
    A = b.shape[1].values
    s, R = T(f32(b.shape[3])), T(f32(b.shape[4] if len(b.shape) > 4 else 0.0))
    mp = b.map
    q, bq = lattice_coords(b, x, T)
    d = (ir._interp_scalar(q, A, T) - R).astype(T)
    g = np.where(clamp_active(q, A.shape), T(0), (interp_grad(q, A, T) / s).astype(T))
    g = [g[:, k] for k in range(D)]
    nn = [_seqsum([T(mp.R[k, a]) * g[k] for k in range(D)]) for a in range(D)] if mp is not None else g
    with np.errstate(invalid="ignore", divide="ignore"):
        mm = np.sqrt(_seqsum([v * v for v in nn]))
        dn = d / mm
        n = [v / mm for v in nn]
        full = ~(d * d > T(fastd2)) & ~np.any([np.isnan(v) for v in g], axis=0)
    zero = np.zeros_like(d)
    if mp is None:
        vel = [zero] * D
    elif D == 2:
        w = T(mp.omega)
        vel = [T(mp.V[0]) + w * -bq[1], T(mp.V[1]) + w * bq[0]]
    else:
        w = [T(v) for v in mp.omega]
        vel = [T(mp.V[0]) + (w[1] * bq[2] - w[2] * bq[1]), T(mp.V[1]) + (w[2] * bq[0] - w[0] * bq[2]), T(mp.V[2]) + (w[0] * bq[1] - w[1] * bq[0])]
    out = [np.where(full, dn, d)] + [np.where(full, v, zero) for v in n] + [np.where(full, v + zero, zero) for v in vel]
    return [np.asarray(v, dtype=T).reshape(shape) for v in out]


def points(b, X, fastd2=np.inf, T=f32):
    """the same at the rows of X (npts × D) -> d (npts), n (npts × D), V (npts × D)"""
    X = np.asarray(X, dtype=f32)
    D = X.shape[1]
    t = leaf(b, [X[:, k] for k in range(D)], fastd2, T)
    return t[0], np.stack(t[1:1 + D], axis=1), np.stack(t[1 + D:], axis=1)


_fr_leaf = fr._leaf


def _leaf_any(b, x, fastd2):
    return leaf(b, x, fastd2, f32) if b.shape[0] == "lattice" else _fr_leaf(b, x, fastd2)


fr._leaf = _leaf_any      # forces_ref evaluates lattice leaves from here on (every other leaf goes where it went)


def tuple_at(body, X, fastd2=np.inf):
    """the Float32 tuple of any program — lattice leaves included — at the rows of X, through forces_ref's postfix evaluation: (npts, 2D+1)"""
    X = np.asarray(X, dtype=f32)
    return np.stack(fr._tuple(body, [X[:, k] for k in range(X.shape[1])], fastd2), axis=1)


# ---- measure!(flow, body; ϵ) of a one-leaf lattice program on every array cell   src/Body.jl:28-51 ----
def bc_zero(a, D):
    """BC!(a, 0): the loops of src/core.jl:201-219 for a zero boundary value on an (Ng..., D) array, no periodic direction, no exit"""
    for i in range(D):
        for j in range(D):
            lo, lo1, hi, hi1 = ([slice(None)] * D for _ in range(4))
            lo[j], lo1[j], hi[j], hi1[j] = 0, 1, -1, -2
            lo, lo1, hi, hi1 = (tuple(v) + (i,) for v in (lo, lo1, hi, hi1))
            if i == j:
                a[lo] = 0
                a[lo1] = 0
                a[hi] = 0
            else:
                a[lo] = a[lo1]
                a[hi] = a[hi1]
    return a


def measure_fields(b, Ng, eps=1.0, T=f32, sigma_fill=0.0):
    """σ (Ng), μ₀ (Ng, D), μ₁ (Ng, D, D), V (Ng, D) as wl_measure_bodyset leaves them for the one-leaf program b: the kernel's statements on the interior (σ the
    raw sdf), μ₀ = 1, μ₁ = V = 0 on the ghost layer, σ's ghost layer untouched (sigma_fill), then BC!(μ₀, 0) and BC!(V, 0)"""
    D = len(Ng)
    e = T(f32(eps))
    pi = T(f32(3.14159265358979323846))
    core = tuple(slice(1, n - 1) for n in Ng)
    x = [v[core] for v in fr.centres(Ng)]
    d2 = (T(2) + e) * (T(2) + e)
    dc = leaf(b, x, -1.0, T)[0]                                  # the raw sdf: every point takes the early exit
    sigma = np.full(Ng, sigma_fill, dtype=T)
    sigma[core] = dc
    mu0 = np.ones(Ng + (D,), dtype=T)
    mu1 = np.zeros(Ng + (D, D), dtype=T)
    V = np.zeros(Ng + (D,), dtype=T)
    band = dc * dc < d2
    for a in range(D):
        xf = [v - f32(0.5 if k == a else 0.0) for k, v in enumerate(x)]
        t = leaf(b, xf, d2, T)
        di = np.where(np.abs(t[0]) <= T(0.5), t[0], np.copysign(t[0], dc)).astype(T)
        de = (di / e).astype(T)
        dm = np.minimum(de, T(1))
        k0 = (T(1) + dm + np.sin(pi * dm) / pi) / T(2)
        ad = np.abs(di)
        epsd = np.where(ad == 0, T(f32(1.4e-45)), np.spacing(ad.astype(f32)).astype(T))      # eps(Float32) at d, as the kernel takes it
        m0 = np.where(de < T(-1) + np.sqrt(epsd), T(0), k0)
        dcl = np.minimum(np.maximum(de, T(-1)), T(1))
        k1 = e * ((T(1) - dcl * dcl) / T(4) - (dcl * np.sin(pi * dcl) + (T(1) + np.cos(pi * dcl)) / pi) / (T(2) * pi))
        mu0[core + (a,)] = np.where(band, m0, np.where(dc < 0, T(0), T(1)))
        V[core + (a,)] = np.where(band, t[1 + D + a], T(0))
        for k in range(D):
            mu1[core + (a, k)] = np.where(band, k1 * t[1 + k], T(0))
    return sigma, bc_zero(mu0, D), mu1, bc_zero(V, D)


def bound(ref32, ref64):
    """the project's standing rule: |device − ref64| ≤ 4·max over the case of |ref32 − ref64|"""
    return 4.0 * float(np.abs(np.asarray(ref32, dtype=np.float64) - np.asarray(ref64, dtype=np.float64)).max(initial=0.0))


# ---- shapes the tests bake on the host ----
def sample_positions(dims, origin=0.0, spacing=1.0):
    """the positions of a lattice's samples, origin + spacing·(i − ½), as D arrays of shape dims (Float32)"""
    D = len(dims)
    o = np.broadcast_to(np.asarray(origin, dtype=f32), (D,))
    ax = [(o[k] + f32(spacing) * (np.arange(dims[k], dtype=f32) - f32(0.5))).astype(f32) for k in range(D)]
    return np.meshgrid(*ax, indexing="ij")


def torus_values(dims, origin, spacing, centre, R_major, r_minor):
    """the distance to a torus about the z axis through `centre` — a shape the leaf set does not hold — at the lattice's samples (Float64 formula, rounded once)"""
    X = [v.astype(np.float64) - float(centre[k]) for k, v in enumerate(sample_positions(dims, origin, spacing))]
    return (np.sqrt((np.sqrt(X[0] ** 2 + X[1] ** 2) - R_major) ** 2 + X[2] ** 2) - r_minor).astype(f32)


def sphere_values(dims, origin, spacing, centre, R):
    X = [v.astype(np.float64) - float(centre[k]) for k, v in enumerate(sample_positions(dims, origin, spacing))]
    return (np.sqrt(sum(v ** 2 for v in X)) - R).astype(f32)


def lattice_body(lat, origin=0.0, spacing=1.0, offset=0.0, map=None):
    return Body(("lattice", lat, origin, spacing, offset), map=map)


def classes(b, X, fastd2=np.inf):
    """what a point set exercises: counts of points inside the box, clamped in exactly one / two / three directions, exactly on a node plane of some
    direction (inside the box), within |d| ≤ 1 of the surface, and on the early exit"""
    D = np.asarray(X).shape[1]
    q, _ = lattice_coords(b, [np.asarray(X, dtype=f32)[:, k] for k in range(D)], f32)
    A = b.shape[1].values
    act = clamp_active(q, A.shape).sum(axis=1)
    node = ((q + f32(0.5)) == np.floor(q + f32(0.5))).any(axis=1) & (act == 0)
    d = leaf(b, [np.asarray(X, dtype=f32)[:, k] for k in range(D)], -1.0, f32)[0]
    return dict(inside=int((act == 0).sum()), clamp1=int((act == 1).sum()), clamp2=int((act == 2).sum()), clamp3=int((act == 3).sum()),
                node=int(node.sum()), band=int((np.abs(d) <= 1).sum()), exit=int((d * d > f32(fastd2)).sum()))


# ---- the cases tests/test_gpu_lattice.py measures at points; tests/test_lattice_cpu.py holds each to the classes it claims ----
def _rmap3():
    from waterlily_jl_amd.bodies import RigidMap
    return RigidMap((10.3, 9.2, 8.1), (0.3, -0.2, 0.5), xp=(0.5, 0.0, -0.25), V=(0.1, -0.2, 0.05), omega=(0.02, 0.01, -0.03))


ALL = ("inside", "clamp1", "clamp2", "clamp3", "node", "band", "exit")
POINT_CASES = {
    # source: the closed-form body the lattice is baked from (on the device: bodies.measure at fastd² = 0; here: forces_ref) or host values
    "sphere": dict(dims=(20, 18, 16), src=lambda: Body(("sphere", (9.0, 8.0, 7.0), 5.0)), claims=ALL),
    "sphere_mapped": dict(dims=(20, 18, 16), src=lambda: Body(("sphere", (9.0, 8.0, 7.0), 5.0)), map=_rmap3, claims=("inside", "clamp1", "clamp2", "clamp3", "band", "exit")),
    "spacing_half": dict(dims=(20, 18, 16), spacing=0.5, origin=(1.0, 2.0, 0.5), src=lambda: Body(("sphere", (5.5, 6.0, 4.0), 2.5)), claims=ALL),
    "spacing_two": dict(dims=(20, 18, 16), spacing=2.0, origin=(-2.0, 0.0, 1.0), src=lambda: Body(("sphere", (16.0, 16.0, 15.0), 5.0)), claims=ALL),
    "offset": dict(dims=(20, 18, 16), offset=0.75, src=lambda: Body(("sphere", (9.0, 8.0, 7.0), 4.0)), claims=ALL),
    "capsule2d": dict(dims=(20, 18), src=lambda: Body(("capsule", (9.0, 8.0), 1.5, (1.0, 0.5), 3.0)), claims=("inside", "clamp1", "clamp2", "node", "band", "exit")),
    "torus": dict(dims=(20, 18, 16), values=lambda dims: torus_values(dims, 0.0, 1.0, (9.5, 8.5, 7.5), 5.0, 1.5), claims=ALL),
}
FASTD2 = 9.0      # (2+ϵ)² at ϵ = 1: what measure! asks with


def point_case(name, bake=None):
    """the case with its samples: bake(body, dims, origin, spacing) -> values samples a closed-form source (the device's, in the GPU tests); without one
    forces_ref's Float32 restatement does.  Returns a dict with values, body(lat) and X"""
    c = dict(origin=0.0, spacing=1.0, offset=0.0, map=None, values=None, src=None)
    c.update(POINT_CASES[name])
    D = len(c["dims"])
    if c["values"] is not None:
        vals = c["values"](c["dims"])
    elif bake is not None:
        vals = bake(c["src"](), c["dims"], c["origin"], c["spacing"])
    else:
        vals = fr._tuple(c["src"](), sample_positions(c["dims"], c["origin"], c["spacing"]), 0.0)[0]
    c["values"] = np.asarray(vals, dtype=f32)
    mp = c["map"]() if c["map"] else None
    c["body"] = lambda lat: lattice_body(lat, c["origin"], c["spacing"], c["offset"], mp)
    c["X"] = case_points(c, D, mp)
    return c


def case_points(c, D, mp, seed=5):
    """body-frame points over the lattice's box and three cells around it (inside; clamped in one, two, three directions), on node planes, and close to the
    surface; carried to the flow frame through the inverse of the case's map (Float64, rounded once)"""
    rng = np.random.default_rng(seed)
    o = np.broadcast_to(np.asarray(c["origin"], dtype=np.float64), (D,))
    s = float(c["spacing"])
    lo, hi = o, o + s * (np.asarray(c["dims"], dtype=np.float64) - 2.0)
    P = [rng.uniform(lo - 3.0, hi + 3.0, size=(160, D)), rng.uniform(lo, hi, size=(96, D))]
    nodes = rng.uniform(lo, hi, size=(24, D))
    for r in range(24):                                          # coordinate r % D exactly on a sample plane: origin + s·(i − ½), exact in Float32 for these cases
        k = r % D
        nodes[r, k] = o[k] + s * (rng.integers(1, c["dims"][k] - 1) - 0.5)
    if mp is None:                                               # (under a map a rounded point falls to either side of the plane: Float32 and Float64 would differ by the kink)
        P.append(nodes)
    corner = np.where(rng.integers(0, 2, size=(24, D)) == 1, hi + rng.uniform(0.5, 3.0, size=(24, D)), lo - rng.uniform(0.5, 3.0, size=(24, D)))
    P.append(corner)                                             # clamped in every direction
    xi = np.concatenate(P)
    vals = c["values"].astype(np.float64)                        # near the surface: sample positions whose |A − offset| is small, jittered
    near = np.argwhere(np.abs(vals - c["offset"]) < 0.8)
    pick = near[rng.permutation(len(near))[:64]]
    xi = np.concatenate([xi, o + s * (pick - 0.5) + rng.uniform(-0.3, 0.3, size=(len(pick), D))])
    if mp is not None:
        R = np.asarray(mp.R, dtype=np.float64)[:D, :D]
        xi = (xi - mp.xp.astype(np.float64)) @ R + mp.x0.astype(np.float64) + mp.xp.astype(np.float64)      # x = R̂ᵀ(ξ − xₚ) + x₀ + xₚ
    return xi.astype(f32)


# ---- the cases measured as fields (wl_measure_bodyset) and on a handle: lattices that END INSIDE the domain and keep the out-of-range rule ----
def _fmap3(t=0.0):
    from waterlily_jl_amd.bodies import RigidMap
    V = np.array((0.3, 0.1, 0.0), dtype=f32)
    return RigidMap(np.array((12.3, 8.2, 7.9), dtype=f32) + f32(t) * V, (0.2, -0.1, 0.3), V=V, omega=(0.0, 0.02, 0.05))


FIELD_CASES = {
    # a sphere of R = 3.5 about the body-frame origin at 1.5 cells per sample, rotated, translating and spinning on 32×16×16 (its band stays clear of the
    # domain's faces: BC! copies nothing but exact zeros and ones into the ghost layer)
    "sphere3": dict(grid=(32, 16, 16), dims=(16, 16, 16), spacing=1.5, origin=-10.9, src=lambda: Body(("sphere", (0.0, 0.0, 0.0), 3.5)), map=_fmap3),
    # a plate at 1.25 cells per sample, unmapped, on 32×16
    "capsule2": dict(grid=(32, 16), dims=(20, 18), spacing=1.25, origin=(0.4, -2.0), src=lambda: Body(("capsule", (12.0, 8.0), 1.5, (1.0, 0.5), 3.0))),
}


def field_case(name, bake=None, t=0.0):
    c = dict(offset=0.0, map=None)
    c.update(FIELD_CASES[name])
    if bake is not None:
        vals = bake(c["src"](), c["dims"], c["origin"], c["spacing"])
    else:
        vals = fr._tuple(c["src"](), sample_positions(c["dims"], c["origin"], c["spacing"]), 0.0)[0]
    c["values"] = np.asarray(vals, dtype=f32)
    mk = c["map"]
    c["body"] = lambda lat, t=t: lattice_body(lat, c["origin"], c["spacing"], c["offset"], mk(t) if mk else None)
    c["Ng"] = tuple(n + 2 for n in c["grid"])
    return c


def grid_classes(b, Ng, eps=1.0):
    """interior cells of the grid inside the lattice's box, clamped (outside it), and within the band |d| < 2 + ϵ"""
    core = tuple(slice(1, n - 1) for n in Ng)
    x = [v[core] for v in fr.centres(Ng)]
    q, _ = lattice_coords(b, x, f32)
    act = clamp_active(q, b.shape[1].values.shape).any(axis=1)
    d = leaf(b, x, -1.0, f32)[0].reshape(-1)
    return dict(inside=int((~act).sum()), clamped=int(act.sum()), band=int((np.abs(d) < 2 + eps).sum()), band_clamped=int((act & (np.abs(d) < 2 + eps)).sum()))
