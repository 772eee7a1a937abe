"""NumPy restatement of the deforming-mesh additions (include/wlhip.h, deforming meshes; csrc/wl_meshsdf.hip k_meshsdf<D, true>, csrc/wl_lattice.hpp
lattice_vel) — the yardstick of tests/test_meshvel_cpu.py and tests/test_gpu_meshvel.py.

  sdf_points   tests/meshsdf_ref.py's sdf_points with the same statements in the same order, extended: per (sample, element) the barycentric pair (v, w) of the
               closest point read off the region the walk decides; the minimum keeps the winner's pair; W = wa + v·(wb − wa) + w·(wc − wa) per component
  leaf         tests/lattice_ref.py's leaf with the velocity samples on top: ωξ_c = interp(q, W_c); unmapped V = ωξ, mapped V_a = rigid_a + Σ_q R̂[q][a]·ωξ_q
  ambiguous    the samples on the medial axis of a case, where the closest-point extension is discontinuous (Float64); ambiguous_literal: the wider set
               that the same two thresholds give without the allowance for closest points on one sheet of the surface (see ambiguous)
  the registry of cases (mesh, lattice, vertex-velocity field).  No GPU, no library."""
import contextlib
import functools

import numpy as np

import interp_ref as ir
import lattice_ref as lr
import meshsdf_ref as mr

f32, f64 = np.float32, np.float64
_lr_leaf = lr.leaf                       # the leaf without velocity samples (velocity_leaf below swaps lattice_ref's for ours)
REGION_NAMES = {3: ("face", "AB", "BC", "CA", "A", "B", "C"), 2: ("interior", "A", "B")}


# ------------------------------------------------------------------ the pair statements, with the barycentric pair
def _pairs3(p, e):
    """meshsdf_ref._pairs3 -> d², reg, r and (v, w) of q = A + v·(B − A) + w·(C − A) by region: A (0,0), B (1,0), AB (v,0), C (0,1), CA (0,w), BC (1−w,w), face (v,w)"""
    a, b, c = ([e[None, :, k, q] for q in range(3)] for k in range(3))
    ab = [b[q] - a[q] for q in range(3)]; ac = [c[q] - a[q] for q in range(3)]; ap = [p[q] - a[q] for q in range(3)]
    d1, d2 = mr._dot(ab, ap), mr._dot(ac, ap)
    bp = [p[q] - b[q] for q in range(3)]
    d3, d4 = mr._dot(ab, bp), mr._dot(ac, bp)
    cp = [p[q] - c[q] for q in range(3)]
    d5, d6 = mr._dot(ab, cp), mr._dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    one, zero = e.dtype.type(1), e.dtype.type(0)
    v_ab = d1 / (d1 - d3)
    w_ca = d2 / (d2 - d6)
    w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
    den = one / ((va + vb) + vc)
    fv, fw = vb * den, vc * den
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6), (vb <= 0) & (d2 >= 0) & (d6 <= 0),
             (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
    regs = [4, 5, 1, 6, 3, 2]
    qs = [a, b, [a[q] + v_ab * ab[q] for q in range(3)], c, [a[q] + w_ca * ac[q] for q in range(3)], [b[q] + w_bc * (c[q] - b[q]) for q in range(3)]]
    Z, O = np.zeros_like(d1), np.ones_like(d1)
    vws = [(Z, Z), (O, Z), (v_ab + zero, Z), (Z, O), (Z, w_ca + zero), (one - w_bc, w_bc + zero)]
    reg = np.zeros(d1.shape, np.int8)
    q = [(a[k] + ab[k] * fv) + ac[k] * fw for k in range(3)]
    bv, bw = fv, fw
    for cnd, rg, qq, (v_, w_) in reversed(list(zip(conds, regs, qs, vws))):
        reg = np.where(cnd, np.int8(rg), reg)
        q = [np.where(cnd, qq[k], q[k]) for k in range(3)]
        bv, bw = np.where(cnd, v_, bv), np.where(cnd, w_, bw)
    r = [p[k] - q[k] for k in range(3)]
    return (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2], reg, r, bv, bw


def _pairs2(p, e):
    a, b = ([e[None, :, k, q] for q in range(2)] for k in range(2))
    ab = [b[q] - a[q] for q in range(2)]; ap = [p[q] - a[q] for q in range(2)]
    t = ab[0] * ap[0] + ab[1] * ap[1]
    den = ab[0] * ab[0] + ab[1] * ab[1]
    v = t / den
    reg = np.where(t <= 0, np.int8(1), np.where(t >= den, np.int8(2), np.int8(0)))
    q = [np.where(reg == 1, a[k], np.where(reg == 2, b[k], a[k] + v * ab[k])) for k in range(2)]
    r = [p[k] - q[k] for k in range(2)]
    bv = np.where(reg == 1, np.zeros_like(v), np.where(reg == 2, np.ones_like(v), v))
    return r[0] * r[0] + r[1] * r[1], reg, r, bv, np.zeros_like(bv)


def sdf_points(D, V, E, Wv, X, T, chunk=256):
    """the signed distance and the extended velocity at the Float32 points X (S × D) in dtype T -> dict(d, elem (winner), reg, r (S × D), s, v, w, W (S × D));
    Wv: the vertex velocities (nv × D), taken as Float32 numbers"""
    elem64, nrm64 = mr.tables(D, V, E)
    elem, nrm = elem64.astype(T), nrm64.astype(T)
    wtab = np.asarray(Wv, f32)[np.asarray(E)].astype(T)            # (ne, D, D): vertex-major like elem
    X = np.asarray(X, f32).astype(T)
    S = len(X)
    best = np.full(S, np.inf, T); bt = np.zeros(S, np.int64); breg = np.zeros(S, np.int8); br = np.zeros((S, D), T)
    bv = np.zeros(S, T); bw = np.zeros(S, T)
    pairs = _pairs3 if D == 3 else _pairs2
    rows = np.arange(S)
    with np.errstate(all="ignore"):
        for s0 in range(0, S, 512):
            sl = slice(s0, min(S, s0 + 512))
            p = [X[sl, q][:, None] for q in range(D)]
            for t0 in range(0, len(elem), chunk):
                d2, reg, r, pv, pw = pairs(p, elem[t0:t0 + chunk])
                j = np.argmin(d2, axis=1)                # the first of equal minima: ascending index, strict <
                rr = np.arange(d2.shape[0])
                m = d2[rr, j]
                win = m < best[sl]
                idx = rows[sl][win]
                best[idx] = m[win]; bt[idx] = t0 + j[win]; breg[idx] = np.broadcast_to(reg, d2.shape)[rr, j][win]
                bv[idx] = np.broadcast_to(pv, d2.shape)[rr, j][win]; bw[idx] = np.broadcast_to(pw, d2.shape)[rr, j][win]
                for q in range(D):
                    br[idx, q] = np.broadcast_to(r[q], d2.shape)[rr, j][win]
    n = nrm[bt, breg]
    s = br[:, 0] * n[:, 0] + br[:, 1] * n[:, 1]
    if D == 3:
        s = s + br[:, 2] * n[:, 2]
    d = np.sqrt(best)
    wa, wb = wtab[bt, 0], wtab[bt, 1]
    W = wa + bv[:, None] * (wb - wa)
    if D == 3:
        W = W + bw[:, None] * (wtab[bt, 2] - wa)
    return dict(d=np.where(s < 0, -d, d), elem=bt, reg=breg, r=br, s=s, v=bv, w=bw, W=W.astype(T))


# ------------------------------------------------------------------ vertex-velocity fields (Float64 formulas, rounded to Float32 once)
_A = np.array([[0.11, -0.07, 0.05], [0.03, 0.09, -0.12], [-0.06, 0.04, 0.08]])


def linear(V):
    D = V.shape[1]
    return (V.astype(f64) @ _A[:D, :D].T + np.array([0.3, -0.2, 0.1])[:D]).astype(f32)


def rotation(V, centre=(9.0, 9.0, 8.0), omega=(0.03, -0.02, 0.05)):
    return np.cross(np.asarray(omega), V.astype(f64) - np.asarray(centre)).astype(f32)


def radial(V, centre=(9.0, 9.0, 8.0)):
    x = V.astype(f64) - np.asarray(centre)[:V.shape[1]]
    return (0.02 * x * np.linalg.norm(x, axis=1)[:, None]).astype(f32)


def travelling_wave(V, k=0.7, phase=0.4, amp=0.25):
    """a swimming foil's lateral motion: (0, a·sin(k·x − φ))"""
    x = V.astype(f64)
    return np.stack([np.zeros(len(x)), amp * np.sin(k * x[:, 0] - phase)], axis=1).astype(f32)


def uniform(V, U=(0.25, -0.125, 0.0625)):
    return np.broadcast_to(np.asarray(U, f32)[:V.shape[1]], V.shape).copy()


# ------------------------------------------------------------------ the cases
def _foil(n=48, c=(10.3, 9.8), a=7.0, b=2.2):
    return mr.polygon([(c[0] + a * np.cos(2 * np.pi * k / n), c[1] + b * np.sin(2 * np.pi * k / n) * (1 + 0.3 * np.cos(2 * np.pi * k / n))) for k in range(n)])


def _mesh(name):
    c = mr.case(name)
    return dict(D=c["D"], V=c["V"], E=c["E"], dims=c["dims"], origin=c["origin"], spacing=c["spacing"])


CASES = {
    "cube-linear": lambda: dict(_mesh("cube"), field=linear),
    "lprism-rotation": lambda: dict(mr._case(3, mr.lprism(shift=(4.3, 4.57, 4.11)), (17, 17, 14)), field=rotation),      # (equal shifts put samples on the diagonal sheets)
    "ico80-radial": lambda: dict(mr._case(3, mr.icosphere(1, 4.0, (9.3, 9.1, 8.8)), (19, 19, 18)), field=radial),
    "ico1280-rotation": lambda: dict(mr._case(3, mr.icosphere(3, 5.8, (10.3, 10.1, 9.8)), (21, 21, 21)), field=rotation),
    "torus-linear": lambda: dict(_mesh("torus"), field=linear),
    "cube-11x9x6-radial": lambda: dict(_mesh("cube-11x9x6"), field=radial),
    "cube-5x3x3-linear": lambda: dict(_mesh("cube-5x3x3"), field=linear),
    "cube-3x3x3-rotation": lambda: dict(_mesh("cube-3x3x3"), field=rotation),
    "foil2d-wave": lambda: dict(mr._case(2, _foil(), (21, 20)), field=travelling_wave),
}
CASES_3D = [k for k in CASES if k != "foil2d-wave"]
TINY = ["cube-5x3x3-linear", "cube-3x3x3-rotation"]      # 45 and 27 samples at 5 and 8 cells per sample: too few for every region of the walk to win
BAND = 5.0


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    c["Wv"] = c["field"](c["V"])
    c["Wv"].setflags(write=False)
    return c


def positions(c):
    return mr.sample_positions(c["dims"], c["origin"], c["spacing"])


@functools.lru_cache(maxsize=None)
def ref(name, tname):
    """the restatement of a case in Float32 ("f32") or Float64 ("f64"); d has the lattice's shape, W dims + (D,)"""
    c = case(name)
    out = sdf_points(c["D"], c["V"], c["E"], c["Wv"], positions(c), f32 if tname == "f32" else f64)
    out["d"] = out["d"].reshape(c["dims"], order="F")
    out["W"] = out["W"].reshape(c["dims"] + (c["D"],), order="F")
    for v in out.values():
        v.setflags(write=False)
    return out


def scale_of(c):
    """the largest coordinate of the mesh and the lattice: the library's own slack is 1e-4 of it (wl_meshsdf.hip meshsdf_run)"""
    s = max(float(np.abs(c["V"]).max()), abs(c["spacing"]))
    for d in range(c["D"]):
        s = max(s, abs(c["origin"][d] - c["spacing"]), abs(c["origin"][d] + c["spacing"] * c["dims"][d]))
    return s


def ambiguous(name):
    """bool, shaped like the lattice: the medial-axis samples, where the closest-point extension jumps.  Some element other than the winner is within
    tol = 1e-4·scale of the minimum distance d, and its closest point lies farther from the winner's than two closest points ON ONE SHEET of the surface
    can: an element whose closest point is a lateral ℓ away on the same (locally flat) sheet has distance √(d² + ℓ²), so a tie within tol allows
    ℓ ≤ √(2·d·tol + tol²) there — 0.1 cells at d = 3, a third of the band of a 1280-face sphere — and W is continuous across it.  The threshold is
    1e-2·spacing + 2·√(2·d·tol + tol²) (the factor 2: the sheet may bend).  ambiguous_literal drops the allowance: every sample it clears this clears too,
    so the device is held to the restatement on MORE samples here, never fewer.  Float64."""
    return _ambiguous(name, True)


def ambiguous_literal(name):
    """… with the threshold 1e-2·spacing alone: it also flags the samples whose closest point lies within √(2·d·tol) of a shared edge, where nothing jumps"""
    return _ambiguous(name, False)


@functools.lru_cache(maxsize=None)
def _ambiguous(name, sheet):
    c = case(name)
    D = c["D"]
    elem = mr.tables(D, c["V"], c["E"])[0]
    X = positions(c).astype(f64)
    tol, far = 1e-4 * scale_of(c), 1e-2 * c["spacing"]
    pairs = _pairs3 if D == 3 else _pairs2
    out = np.zeros(len(X), bool)
    with np.errstate(all="ignore"):
        for s0 in range(0, len(X), 256):
            sl = slice(s0, min(len(X), s0 + 256))
            p = [X[sl, q][:, None] for q in range(D)]
            d2, _, r, _, _ = pairs(p, elem)
            dist = np.sqrt(d2)
            j = np.argmin(dist, axis=1)
            rr = np.arange(dist.shape[0])
            q = np.stack([np.broadcast_to(p[k] - r[k], dist.shape) for k in range(D)], axis=-1)      # the closest points (S, T, D)
            dmin = dist[rr, j][:, None]
            apart = np.linalg.norm(q - q[rr, j][:, None, :], axis=-1) > far + (2 * np.sqrt(2 * dmin * tol + tol * tol) if sheet else 0.0)
            near = dist <= dist[rr, j][:, None] + tol
            near[rr, j] = False
            out[sl] = (near & apart).any(axis=1)
    out = out.reshape(c["dims"], order="F")
    out.setflags(write=False)
    return out


def band(name):
    return np.abs(ref(name, "f64")["d"]) <= BAND


def gap(name, mask=None):
    """max |W_ref32 − W_ref64| over the (non-ambiguous) samples of the case; 4× this bounds the device"""
    m = ~ambiguous(name) if mask is None else mask
    return float(np.abs(ref(name, "f32")["W"].astype(f64) - ref(name, "f64")["W"])[m].max(initial=0.0))


# ------------------------------------------------------------------ the lattice leaf with velocity samples
class VelLattice(lr.HostLattice):
    """a lattice without a device that carries velocity samples W of shape dims + (D,) (None: none)"""

    def __init__(self, values, W=None, id=1):
        super().__init__(values, id)
        self.W = None if W is None else np.asarray(W, dtype=f32)


def leaf(b, x, fastd2=np.inf, T=f32):
    """lattice_ref.leaf of Body(("lattice", lat, …), map) with lat.W on top -> [d, n_1..n_D, V_1..V_D]"""
    D, shape = len(x), np.shape(x[0])
    t = [np.asarray(v).reshape(-1) for v in _lr_leaf(b, x, fastd2, T)]
    W = getattr(b.shape[1], "W", None)
    if W is None:
        return [v.reshape(shape) for v in t]
    q, _ = lr.lattice_coords(b, x, T)
    wx = [ir._interp_scalar(q, W[..., k], T) for k in range(D)]
    full = ~np.all([v == 0 for v in t[1:1 + D]], axis=0)            # n is a unit vector (or NaN) wherever the leaf went past its two exits
    mp = b.map
    for a in range(D):
        if mp is None:
            va = wx[a]
        else:
            va = (t[1 + D + a] + lr._seqsum([T(mp.R[k, a]) * wx[k] for k in range(D)])).astype(T)
        t[1 + D + a] = np.where(full, va, T(0)).astype(T)
    return [v.reshape(shape) for v in t]


@contextlib.contextmanager
def velocity_leaf():
    """inside the block tests/lattice_ref.py (measure_fields, tuple_at) and tests/forces_ref.py evaluate lattice leaves with their velocity samples"""
    import forces_ref as fr
    keep = lr.leaf, fr._leaf
    lr.leaf = leaf
    fr._leaf = lambda b, x, fastd2: leaf(b, x, fastd2, f32) if b.shape[0] == "lattice" else lr._fr_leaf(b, x, fastd2)
    try:
        yield
    finally:
        lr.leaf, fr._leaf = keep


def host_twin(w_body, values, W):
    """the body of the restatement for a device body: the same leaf over a VelLattice that holds what the device lattice was read back as"""
    from waterlily_jl_amd.bodies import Body
    return Body(("lattice", VelLattice(values, W, id=w_body.shape[1].id)) + tuple(w_body.shape[2:]), w_body.map)


def points(b, X, fastd2=np.inf, T=f32):
    X = np.asarray(X, dtype=f32)
    D = X.shape[1]
    t = leaf(b, [X[:, k] for k in range(D)], fastd2, T)
    return t[0], np.stack(t[1:1 + D], axis=1), np.stack(t[1 + D:], axis=1)


def linear_W(dims, origin, spacing, A, b):
    """velocity samples of the linear field A·ξ + b at a lattice's sample positions: dims + (D,), Float32"""
    X = np.stack(lr.sample_positions(dims, origin, spacing), axis=-1).astype(f64)
    D = len(dims)
    return (X @ np.asarray(A, f64)[:D, :D].T + np.asarray(b, f64)[:D]).astype(f32)


def breathing(V0, centre, k):
    """the vertices of a breathing body at step k (radius factor 1 + 0.01·k) — Float32"""
    c = np.asarray(centre, f64)
    return (c + (V0.astype(f64) - c) * (1.0 + 0.01 * k)).astype(f32)
