"""NumPy restatement of wl_sdf_lattice_from_mesh (include/wlhip.h, sampled bodies from meshes; waterlily.jl_amd/csrc/wl_meshsdf.hip) — the yardstick of
tests/test_meshsdf_cpu.py and tests/test_gpu_meshsdf.py.  The same statements in the same order, parametrised on the dtype: per (sample, element) the closest
point by Ericson's region walk, d² = |p − q|², the minimum over the elements in ascending index (np.argmin keeps the first), the sign from (p − q)·n with the
angle-weighted pseudonormal of the winning feature.  The tables (normals) are computed in Float64 and, for the Float32 form, rounded once.  Also: the refusal
rules (check_mesh) with a list of broken meshes, the registry of cases, and the baseline sphere-bound cull per brick (cull_census).  No GPU, no library."""
import functools
import struct

import numpy as np

f32, f64 = np.float32, np.float64
NREG = {3: 7, 2: 3}                      # rows of the pseudonormal table per element: face, AB, BC, CA, A, B, C / interior, A, B
EXT = {3: (4, 4, 4), 2: (4, 16)}         # a brick of samples (one wave)


# ------------------------------------------------------------------ meshes
def box(lo, hi):
    """an axis-aligned box as 8 vertices and 12 outward triangles"""
    lo, hi = np.asarray(lo, f64), np.asarray(hi, f64)
    V = np.array([[(lo, hi)[(q >> d) & 1][d] for d in range(3)] for q in range(8)])
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]      # z−, z+, y−, y+, x−, x+ : counter-clockwise from outside
    E = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return V.astype(f32), np.array(E, np.int32)


LPOLY = np.array([(0, 0), (8, 0), (8, 4), (4, 4), (4, 8), (0, 8)], f64)      # counter-clockwise, star-shaped about vertex 0, one concave corner


def lprism(shift=(4.3, 4.3, 4.3), h=5.0):
    """the L polygon extruded along z: 12 vertices, 2·4 cap + 6·2 side = 20 triangles, one concave edge"""
    n = len(LPOLY)
    V = np.array([(x, y, z) for z in (0.0, h) for x, y in LPOLY]) + np.asarray(shift)
    E = []
    for k in range(1, n - 1):
        E.append((0, k + 1, k))                          # bottom: seen from below
        E.append((n, n + k, n + k + 1))                  # top
    for k in range(n):
        a, b = k, (k + 1) % n
        E += [(a, b, n + b), (a, n + b, n + a)]
    return V.astype(f32), np.array(E, np.int32)


def icosphere(level, R, centre):
    t = (1 + 5 ** 0.5) / 2
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    V = [np.array(v, f64) / np.linalg.norm(v) for v in V]
    for _ in range(level):
        mid, G = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                w = V[a] + V[b]
                V.append(w / np.linalg.norm(w))
                mid[k] = len(V) - 1
            return mid[k]
        for a, b, c in F:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            G += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = G
    return (np.array(V) * R + np.asarray(centre, f64)).astype(f32), np.array(F, np.int32)


def torus(nu, nv, R, r, centre):
    """nu × nv × 2 triangles, the axis along z"""
    V = [((R + r * np.cos(2 * np.pi * j / nv)) * np.cos(2 * np.pi * i / nu), (R + r * np.cos(2 * np.pi * j / nv)) * np.sin(2 * np.pi * i / nu),
          r * np.sin(2 * np.pi * j / nv)) for i in range(nu) for j in range(nv)]
    ix = lambda i, j: (i % nu) * nv + (j % nv)      # noqa: E731
    E = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = ix(i, j), ix(i + 1, j), ix(i + 1, j + 1), ix(i, j + 1)
            E += [(a, b, c), (a, c, d)]
    return (np.array(V) + np.asarray(centre, f64)).astype(f32), np.array(E, np.int32)


def polygon(P):
    P = np.asarray(P, f64)
    n = len(P)
    return P.astype(f32), np.array([(k, (k + 1) % n) for k in range(n)], np.int32)


def _case(D, VE, dims, origin=0.0, spacing=1.0, **kw):
    V, E = VE
    return dict(D=D, V=V, E=E, dims=tuple(dims), origin=tuple(np.broadcast_to(np.asarray(origin, f32), (D,)).tolist()), spacing=float(spacing), **kw)


_CUBE = box((5.3, 5.3, 5.3), (12.3, 10.3, 8.3))          # 7 × 5 × 3
CASES = {
    "cube": lambda: _case(3, _CUBE, (19, 17, 15)),
    "lprism": lambda: _case(3, lprism(), (17, 17, 14)),
    "ico320": lambda: _case(3, icosphere(2, 5.0, (10.3, 10.1, 9.8)), (21, 21, 21)),
    "ico1280-centred": lambda: _case(3, icosphere(3, 5.8, (9.5, 9.5, 9.5)), (20, 20, 20), centre_sample=(10, 10, 10)),
    "torus": lambda: _case(3, torus(24, 12, 8.0, 3.0, (14.8, 14.6, 7.9)), (30, 30, 16), torus=(8.0, 3.0, (14.8, 14.6, 7.9))),
    "cube-11x9x6": lambda: _case(3, _CUBE, (11, 9, 6), (0.0, 0.0, 0.0), 2.0),
    "cube-5x3x3": lambda: _case(3, _CUBE, (5, 3, 3), (0.0, 0.0, 0.0), 5.0),
    "cube-3x3x3": lambda: _case(3, _CUBE, (3, 3, 3), (0.0, 0.0, 0.0), 8.0),
    "square": lambda: _case(2, polygon([(5.3, 5.3), (11.3, 5.3), (11.3, 9.3), (5.3, 9.3)]), (16, 14)),
    "lpoly": lambda: _case(2, polygon(LPOLY + 5.3), (18, 18)),
    "gon64": lambda: _case(2, polygon([(10.3 + 7 * np.cos(2 * np.pi * k / 64), 9.8 + 7 * np.sin(2 * np.pi * k / 64)) for k in range(64)]), (21, 20)),
}
CASES_3D = [k for k in CASES if k not in ("square", "lpoly", "gon64")]
CASES_2D = ["square", "lpoly", "gon64"]
RAGGED = ["cube-11x9x6", "cube-5x3x3", "cube-3x3x3"]


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


# ------------------------------------------------------------------ the refusals
REASONS = {"count": "at least", "finite": "not finite", "index": "outside [0, nv)", "degenerate": "zero", "edge": "weld", "vertex": "incoming", "inward": "inward"}


def check_mesh(D, V, E):
    """None for a mesh wl_sdf_lattice_from_mesh takes, else the key (REASONS) of the first rule it breaks, in the library's order"""
    V, E = np.asarray(V), np.asarray(E)
    nv, ne = len(V), len(E)
    if (nv < 4 or ne < 4) if D == 3 else (nv < 3 or ne < 3):
        return "count"
    if not np.isfinite(V).all():
        return "finite"
    if (E < 0).any() or (E >= nv).any():
        return "index"
    P = V.astype(f64)
    if D == 3:
        n = np.cross(P[E[:, 1]] - P[E[:, 0]], P[E[:, 2]] - P[E[:, 0]])
        if (np.linalg.norm(n, axis=1) == 0).any():
            return "degenerate"
        directed = {}
        for t, tri in enumerate(E.tolist()):
            for k in range(3):
                key = (tri[k], tri[(k + 1) % 3])
                if key in directed:
                    return "edge"
                directed[key] = t
        if any((j, i) not in directed for i, j in directed):
            return "edge"
        vol = np.einsum("ij,ij->i", P[E[:, 0]], np.cross(P[E[:, 1]], P[E[:, 2]])).sum()
    else:
        if (np.linalg.norm(P[E[:, 1]] - P[E[:, 0]], axis=1) == 0).any():
            return "degenerate"
        nin, nout = np.bincount(E[:, 1], minlength=nv), np.bincount(E[:, 0], minlength=nv)
        used = (nin + nout) > 0
        if ((nin != 1) | (nout != 1))[used].any():
            return "vertex"
        a, b = P[E[:, 0]], P[E[:, 1]]
        vol = (a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]).sum()
    return None if vol > 0 else "inward"


def broken_variants():
    """(name, D, V, E, reason): meshes the library refuses, each for the named rule"""
    V, E = _CUBE
    out = []
    out.append(("cube minus a face", 3, V, E[2:], "edge"))
    F = E.copy(); F[5] = F[5][::-1]
    out.append(("a triangle reversed", 3, V, F, "edge"))
    out.append(("the whole cube reversed", 3, V, E[:, ::-1].copy(), "inward"))
    F = E.copy(); F[3] = (F[3][0], F[3][0], F[3][1])
    out.append(("a degenerate triangle", 3, V, F, "degenerate"))
    W = np.vstack([V, V[:1] + f32(0)]); W[-1] = (V[0] + V[1]) / 2       # a vertex on an edge, three in a line
    F = E.copy(); F[0] = (0, 1, 8)
    out.append(("three vertices in a line", 3, W, F, "degenerate"))
    F = E.copy(); F[7, 1] = 8
    out.append(("an index out of range", 3, V, F, "index"))
    F = E.copy(); F[2, 0] = -1
    out.append(("a negative index", 3, V, F, "index"))
    W = np.vstack([V, [[8.0, 2.0, 6.8]]]).astype(f32)
    out.append(("a fin on an edge", 3, W, np.vstack([E, [[0, 1, 8]]]).astype(np.int32), "edge"))
    W = V.copy(); W[3, 1] = np.nan
    out.append(("a NaN vertex", 3, W, E, "finite"))
    W = V.copy(); W[6, 2] = np.inf
    out.append(("an infinite vertex", 3, W, E, "finite"))
    out.append(("unwelded triangle soup", 3, V[E.reshape(-1)].copy(), np.arange(36, dtype=np.int32).reshape(12, 3), "edge"))
    out.append(("three triangles", 3, V, E[:3], "count"))
    P, S = polygon(LPOLY + 5.3)
    out.append(("an open polyline", 2, P, S[:-1], "vertex"))
    out.append(("a branching polyline", 2, P, np.vstack([S, [[0, 3]]]).astype(np.int32), "vertex"))
    out.append(("a clockwise polygon", 2, P, S[:, ::-1].copy(), "inward"))
    T = S.copy(); T[2] = (2, 2)
    out.append(("a segment of zero length", 2, P, T, "degenerate"))
    out.append(("two segments", 2, P, S[:2], "count"))
    return out


# ------------------------------------------------------------------ the tables
def _unit(a, fallback):
    n = np.linalg.norm(a)
    return a / n if n > 0 and np.isfinite(1.0 / n) else fallback


def tables(D, V, E):
    """(elem (ne, D, D), nrm (ne, NREG, D)) in Float64: the vertices of every element and the unit pseudonormal of every region of its walk"""
    P, E = np.asarray(V).astype(f64), np.asarray(E)
    ne = len(E)
    elem = P[E]
    nrm = np.zeros((ne, NREG[D], D))
    if D == 3:
        n = np.cross(elem[:, 1] - elem[:, 0], elem[:, 2] - elem[:, 0])
        nf = n / np.linalg.norm(n, axis=1)[:, None]
        directed = {(tri[k], tri[(k + 1) % 3]): t for t, tri in enumerate(E.tolist()) for k in range(3)}
        vn = np.zeros((len(P), 3))
        for k in range(3):
            u, w = elem[:, (k + 1) % 3] - elem[:, k], elem[:, (k + 2) % 3] - elem[:, k]
            ang = np.arctan2(np.linalg.norm(np.cross(u, w), axis=1), np.einsum("ij,ij->i", u, w))
            np.add.at(vn, E[:, k], ang[:, None] * nf)
        for t, tri in enumerate(E.tolist()):
            nrm[t, 0] = nf[t]
            for k in range(3):
                nrm[t, 1 + k] = _unit(nf[t] + nf[directed[(tri[(k + 1) % 3], tri[k])]], nf[t])
                nrm[t, 4 + k] = _unit(vn[tri[k]], nf[t])
    else:
        d = elem[:, 1] - elem[:, 0]
        nf = np.stack([d[:, 1], -d[:, 0]], axis=1) / np.linalg.norm(d, axis=1)[:, None]
        into = {int(s[1]): t for t, s in enumerate(E)}
        outof = {int(s[0]): t for t, s in enumerate(E)}
        for t, s in enumerate(E.tolist()):
            nrm[t, 0] = nf[t]
            nrm[t, 1] = _unit(nf[t] + nf[into[s[0]]], nf[t])
            nrm[t, 2] = _unit(nf[t] + nf[outof[s[1]]], nf[t])
    return elem, nrm


def sample_positions(dims, origin, spacing):
    """the positions of the samples, Float32, first index fastest: origin + spacing·((float)i − 0.5f) (SdfLattice.centres' statement)"""
    D = len(dims)
    ax = [(f32(origin[q]) + f32(spacing) * (np.arange(dims[q], dtype=f32) - f32(0.5))).astype(f32) for q in range(D)]
    g = np.meshgrid(*ax, indexing="ij")
    return np.stack([v.reshape(-1, order="F") for v in g], axis=1)


# ------------------------------------------------------------------ the pair statements
def _dot(a, b):
    s = a[0] * b[0] + a[1] * b[1]
    return s + a[2] * b[2] if len(a) == 3 else s


def _pairs3(p, e):
    """p: 3 arrays (S,1); e: (T,3,3) -> d² (S,T), reg, r (3 arrays): Ericson's walk, every branch evaluated, the first that holds selected"""
    a, b, c = ([e[None, :, k, q] for q in range(3)] for k in range(3))
    ab = [b[q] - a[q] for q in range(3)]; ac = [c[q] - a[q] for q in range(3)]; ap = [p[q] - a[q] for q in range(3)]
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bp = [p[q] - b[q] for q in range(3)]
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    cp = [p[q] - c[q] for q in range(3)]
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    one = e.dtype.type(1)
    v_ab = d1 / (d1 - d3)
    w_ca = d2 / (d2 - d6)
    w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
    den = one / ((va + vb) + vc)
    fv, fw = vb * den, vc * den
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6), (vb <= 0) & (d2 >= 0) & (d6 <= 0),
             (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
    regs = [4, 5, 1, 6, 3, 2]
    qs = [a, b, [a[q] + v_ab * ab[q] for q in range(3)], c, [a[q] + w_ca * ac[q] for q in range(3)], [b[q] + w_bc * (c[q] - b[q]) for q in range(3)]]
    reg = np.zeros(d1.shape, np.int8)
    q = [(a[k] + ab[k] * fv) + ac[k] * fw for k in range(3)]
    for cnd, rg, qq in reversed(list(zip(conds, regs, qs))):
        reg = np.where(cnd, np.int8(rg), reg)
        q = [np.where(cnd, qq[k], q[k]) for k in range(3)]
    r = [p[k] - q[k] for k in range(3)]
    return (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2], reg, r


def _pairs2(p, e):
    a, b = ([e[None, :, k, q] for q in range(2)] for k in range(2))
    ab = [b[q] - a[q] for q in range(2)]; ap = [p[q] - a[q] for q in range(2)]
    t = ab[0] * ap[0] + ab[1] * ap[1]
    den = ab[0] * ab[0] + ab[1] * ab[1]
    v = t / den
    reg = np.where(t <= 0, np.int8(1), np.where(t >= den, np.int8(2), np.int8(0)))
    q = [np.where(reg == 1, a[k], np.where(reg == 2, b[k], a[k] + v * ab[k])) for k in range(2)]
    r = [p[k] - q[k] for k in range(2)]
    return r[0] * r[0] + r[1] * r[1], reg, r


def sdf_points(D, V, E, X, T, chunk=256):
    """the signed distance at the Float32 points X (S × D) in dtype T -> dict(d, elem, reg, r (S × D), s = (p − q)·n)"""
    elem64, nrm64 = tables(D, V, E)
    elem, nrm = elem64.astype(T), nrm64.astype(T)       # (the vertices are Float32 numbers: exact either way; the normals are rounded once)
    X = np.asarray(X, f32).astype(T)
    S = len(X)
    best = np.full(S, np.inf, T); bt = np.zeros(S, np.int64); breg = np.zeros(S, np.int8); br = np.zeros((S, D), T)
    pairs = _pairs3 if D == 3 else _pairs2
    rows = np.arange(S)
    with np.errstate(all="ignore"):
        for s0 in range(0, S, 512):
            sl = slice(s0, min(S, s0 + 512))
            p = [X[sl, q][:, None] for q in range(D)]
            for t0 in range(0, len(elem), chunk):
                d2, reg, r = pairs(p, elem[t0:t0 + chunk])
                j = np.argmin(d2, axis=1)                # the first of equal minima: ascending index, strict <
                rr = np.arange(d2.shape[0])
                m = d2[rr, j]
                win = m < best[sl]
                idx = rows[sl][win]
                best[idx] = m[win]; bt[idx] = t0 + j[win]; breg[idx] = np.broadcast_to(reg, d2.shape)[rr, j][win]
                for q in range(D):
                    br[idx, q] = np.broadcast_to(r[q], d2.shape)[rr, j][win]
    n = nrm[bt, breg]
    s = br[:, 0] * n[:, 0] + br[:, 1] * n[:, 1]
    if D == 3:
        s = s + br[:, 2] * n[:, 2]
    d = np.sqrt(best)
    return dict(d=np.where(s < 0, -d, d), elem=bt, reg=breg, r=br, s=s)


@functools.lru_cache(maxsize=None)
def ref(name, tname):
    """the restatement of a case in Float32 ("f32") or Float64 ("f64"); d has the lattice's shape"""
    c = case(name)
    out = sdf_points(c["D"], c["V"], c["E"], sample_positions(c["dims"], c["origin"], c["spacing"]), f32 if tname == "f32" else f64)
    out["d"] = out["d"].reshape(c["dims"], order="F")
    for v in out.values():
        v.setflags(write=False)
    return out


def gap(name):
    """max |ref32 − ref64| over the case; 4× this is the bound of the device (the project's standing rule)"""
    return float(np.abs(ref(name, "f32")["d"].astype(f64) - ref(name, "f64")["d"]).max())


# ------------------------------------------------------------------ independent checks
def box_distance(X, lo, hi):
    X, lo, hi = np.asarray(X, f64), np.asarray(lo, f64), np.asarray(hi, f64)
    q = np.maximum(lo - X, X - hi)
    return np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(q.max(axis=1), 0)


def torus_distance(X, R, r, centre):
    x = np.asarray(X, f64) - np.asarray(centre, f64)
    return np.hypot(np.hypot(x[:, 0], x[:, 1]) - R, x[:, 2]) - r


def winding_number(D, V, E, X):
    """the generalised winding number of the surface about every point: Σ solid angles / 4π (van Oosterom & Strackee), in 2-D Σ signed angles / 2π"""
    P, X = np.asarray(V).astype(f64), np.asarray(X, f64)
    w = np.zeros(len(X))
    for el in np.asarray(E):
        if D == 3:
            a, b, c = (P[el[k]][None, :] - X for k in range(3))
            la, lb, lc = (np.linalg.norm(v, axis=1) for v in (a, b, c))
            num = np.einsum("ij,ij->i", a, np.cross(b, c))
            den = la * lb * lc + np.einsum("ij,ij->i", a, b) * lc + np.einsum("ij,ij->i", b, c) * la + np.einsum("ij,ij->i", c, a) * lb
            w += 2 * np.arctan2(num, den)
        else:
            a, b = (P[el[k]][None, :] - X for k in range(2))
            w += np.arctan2(a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0], np.einsum("ij,ij->i", a, b))
    return w / (4 * np.pi if D == 3 else 2 * np.pi)


# ------------------------------------------------------------------ the cull, restated
def bounding_spheres(D, V, E):
    """the smallest sphere around every element (centre (ne, D), radius (ne)), Float64"""
    elem = np.asarray(V).astype(f64)[np.asarray(E)]
    ne = len(elem)
    C, R = np.zeros((ne, D)), np.zeros(ne)
    for t in range(ne):
        p = elem[t]
        best = None
        for a in range(D):
            for b in range(a + 1, D):
                m = (p[a] + p[b]) / 2
                rr = np.linalg.norm(p - m, axis=1).max()
                if rr <= np.linalg.norm(p[a] - p[b]) / 2 * (1 + 1e-12) and (best is None or rr < best[1]):
                    best = (m, rr)
        if best is None:
            ab, ac = p[1] - p[0], p[2] - p[0]
            n = np.cross(ab, ac)
            m = p[0] + (np.cross(n, ab) * (ac @ ac) + np.cross(ac, n) * (ab @ ab)) / (2 * (n @ n))
            best = (m, np.linalg.norm(p - m, axis=1).max())
        C[t], R[t] = best
    return C, R


def cull_census(name):
    """the baseline cull per brick, in Float64 and without slack: Ub = min_t(|c_b − c_t| + r_t) + r_b, element t is a candidate when |c_b − c_t| − r_t − r_b ≤ Ub
    -> dict(nbricks, cand (candidates per brick, bricks in first-index-fastest order), live (samples per brick), tested, total, nb)"""
    c = case(name)
    D, dims, s = c["D"], c["dims"], c["spacing"]
    C, R = bounding_spheres(D, c["V"], c["E"])
    ext = EXT[D]
    nb = [-(-dims[d] // ext[d]) for d in range(D)]
    rb = s * np.sqrt(sum(((e - 1) / 2) ** 2 for e in ext))
    cand, live = [], []
    for b in np.ndindex(*nb[::-1]):
        b = b[::-1]
        cb = np.array([c["origin"][d] + s * (b[d] * ext[d] + (ext[d] - 1) / 2 - 0.5) for d in range(D)])
        dist = np.linalg.norm(C - cb, axis=1)
        ub = (dist + R).min() + rb
        cand.append(int((dist - R - rb <= ub).sum()))
        live.append(int(np.prod([min(ext[d], dims[d] - b[d] * ext[d]) for d in range(D)])))
    cand, live = np.array(cand), np.array(live)
    return dict(nbricks=len(cand), cand=cand, live=live, tested=int((cand * live).sum()), total=int(np.prod(dims)) * len(c["E"]), nb=nb)


def mesh_body_placement(V, spacing=1.0, margin=5.0):
    """bodies.mesh_body's lattice around the bounding box of V: (dims, origin) with origin_d = lo_d − margin − spacing/2, n_d = ceil((hi_d − lo_d + 2·margin)/spacing) + 3"""
    V = np.asarray(V, f64)
    lo, hi = V.min(axis=0), V.max(axis=0)
    dims = tuple(int(np.ceil((hi[d] - lo[d] + 2 * margin) / spacing)) + 3 for d in range(V.shape[1]))
    return dims, tuple(float(lo[d] - margin - spacing / 2) for d in range(V.shape[1]))


def write_binary_stl(path, V, E):
    with open(path, "wb") as fh:
        fh.write(b"binary stl".ljust(80, b" "))
        fh.write(struct.pack("<I", len(E)))
        for tri in E:
            fh.write(struct.pack("<12fH", 0.0, 0.0, 0.0, *V[tri].reshape(-1).tolist(), 0))
