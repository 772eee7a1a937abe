"""NumPy restatement of the force band (waterlily.jl_amd/csrc/wl_forces.hip): measure(body,x;fastd²=1) of the test bodies in Float32 with the kernels'
operation order, the tile classification (a tile of 64×4×4 array cells — 64×4 in 2-D — is active iff an interior cell has d² ≤ 1), the band cell count
and the twelve sums (pressure force, viscous force, pressure moment, viscous moment; Float32 terms, Float64 sums).  Also the geometry matrix the CPU
and GPU tests share."""
import numpy as np

from waterlily_jl_amd.bodies import OP_INTERSECT, OP_NEGATE, OP_UNION, Body, RigidMap, SetBody

f32 = np.float32
TILE = (64, 4, 4)
PI = f32(3.14159265358979323846)


def centres(Ng):
    """cell centres loc(0,I) of every array cell, one (Ng...) Float32 array per direction"""
    ax = [np.arange(n, dtype=f32) - f32(0.5) for n in Ng]
    return [np.ascontiguousarray(a) for a in np.meshgrid(*ax, indexing="ij")]


def _seqsum(terms):
    s = np.zeros_like(terms[0])
    for t in terms:
        s = s + t
    return s


def _leaf(b, x, fastd2):
    D = len(x)
    name = b.shape[0]
    c = [f32(v) for v in b.shape[1]]
    zero = np.zeros_like(x[0])
    mp = b.map
    if mp is not None:
        bq = [(x[q] - f32(mp.x0[q])) - f32(mp.xp[q]) for q in range(D)]
        xi = [_seqsum([f32(mp.R[q, r]) * bq[r] for r in range(D)]) + f32(mp.xp[q]) for q in range(D)]
    else:
        bq, xi = [zero] * D, x
    if name in ("sphere", "cylinder"):
        m = [f32(1.0)] * D if name == "sphere" else [f32(0.0 if k == int(b.shape[3]) else 1.0) for k in range(D)]
        dx = [m[q] * (xi[q] - c[q]) for q in range(D)]
        rr = np.sqrt(_seqsum([v * v for v in dx]))
        d = rr - f32(b.shape[2])
        with np.errstate(invalid="ignore", divide="ignore"):
            g = [dx[q] / rr for q in range(D)]
    elif name == "plane":
        m = [f32(v) for v in b.shape[2]]
        d = _seqsum([m[q] * (xi[q] - c[q]) for q in range(D)])
        g = [m[q] + zero for q in range(D)]
    elif name == "capsule":
        ax = np.asarray(b.shape[3], dtype=f32)
        ax = ax / np.sqrt(f32(np.sum(ax * ax, dtype=f32)))
        h = f32(b.shape[4])
        t = np.minimum(np.maximum(_seqsum([ax[q] * (xi[q] - c[q]) for q in range(D)]), -h), h)
        dl = [xi[q] - (c[q] + t * ax[q]) for q in range(D)]
        rr = np.sqrt(_seqsum([v * v for v in dl]))
        d = rr - f32(b.shape[2])
        with np.errstate(invalid="ignore", divide="ignore"):
            g = [dl[q] / rr for q in range(D)]
    else:
        raise ValueError(name)
    if mp is not None:
        nn = [_seqsum([f32(mp.R[q, a]) * g[q] for q in range(D)]) for a in range(D)]
    else:
        nn = g
    with np.errstate(invalid="ignore", divide="ignore"):
        mm = np.sqrt(_seqsum([v * v for v in nn]))
        dn = d / mm
        n = [v / mm for v in nn]
    full = (d * d <= f32(fastd2)) & ~np.any([np.isnan(v) for v in g], axis=0)
    if mp is not None:
        if D == 2:
            w = f32(mp.omega)
            vel = [f32(mp.V[0]) + w * -bq[1], f32(mp.V[1]) + w * bq[0]]
        else:
            w = [f32(v) for v in mp.omega]
            vel = [f32(mp.V[0]) + (w[1] * bq[2] - w[2] * bq[1]), f32(mp.V[1]) + (w[2] * bq[0] - w[0] * bq[2]), f32(mp.V[2]) + (w[0] * bq[1] - w[1] * bq[0])]
    else:
        vel = [zero] * D
    return [np.where(full, dn, d)] + [np.where(full, v, zero) for v in n] + [np.where(full, v, zero) for v in vel]


def _isless(a, b):
    """Julia's isless on Float32 arrays: NaN after everything, −0 before +0"""
    na, nb = np.isnan(a), np.isnan(b)
    return np.where(na | nb, ~na & nb, np.where(a == b, np.signbit(a) & ~np.signbit(b), a < b))


def _isequal(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return np.where(na | nb, na & nb, (a == b) & (np.signbit(a) == np.signbit(b)))


def _tuple(body, x, fastd2):
    D = len(x)
    if isinstance(body, Body):
        return _leaf(body, x, fastd2)
    assert isinstance(body, SetBody)
    A = _tuple(body.a, x, fastd2)
    if body.op == OP_NEGATE:
        return [-v for v in A[:D + 1]] + A[D + 1:]
    B = _tuple(body.b, x, fastd2)
    less = np.zeros(A[0].shape, dtype=bool)       # isless(B, A) on tuples: lexicographic
    eq = np.ones(A[0].shape, dtype=bool)
    for q in range(len(A)):
        lq = _isless(B[q], A[q])
        less = np.where(eq, lq, less)
        eq = eq & ~lq & _isequal(B[q], A[q])
    assert body.op in (OP_UNION, OP_INTERSECT)
    takeb = less if body.op == OP_UNION else ~less
    return [np.where(takeb, vb, va) for va, vb in zip(A, B)]


def measure(body, Ng, fastd2=1.0):
    """(d, [n_1..n_D]) of measure(body,x;fastd²) at every array cell's centre (Float32)"""
    body = body if not isinstance(body, tuple) else Body(body)
    x = centres(Ng)
    t = _tuple(body, x, fastd2)
    return t[0], t[1:1 + len(Ng)]


def inside(Ng):
    m = np.zeros(Ng, dtype=bool)
    m[tuple(slice(1, n - 1) for n in Ng)] = True
    return m


def tile_index(Ng):
    """tile id of every array cell and the number of tiles: id = tx + ntx·(ty + nty·tz)"""
    D = len(Ng)
    nt = [-(-Ng[q] // TILE[q]) for q in range(D)]
    idx = np.meshgrid(*[np.arange(n) // TILE[q] for q, n in enumerate(Ng)], indexing="ij")
    tid = idx[0] + nt[0] * idx[1] + (nt[0] * nt[1] * idx[2] if D == 3 else 0)
    return tid, int(np.prod(nt))


def band(body, Ng):
    """(active tile ids ascending, number of tiles, band cells n_b, mask of the interior cells of active tiles)"""
    d, _ = measure(body, Ng)
    with np.errstate(invalid="ignore"):
        hit = inside(Ng) & (d * d <= f32(1.0))
    tid, nt = tile_index(Ng)
    active = np.unique(tid[hit])
    return active, nt, int(hit.sum()), inside(Ng) & np.isin(tid, active)


def kern(d):
    return (f32(1) + np.cos(PI * d)) / f32(2)


def _cross(a, b):
    if len(a) == 2:
        m = a[0] * b[1] - a[1] * b[0]
        return [m, m]
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def terms(body, p, u, nu, x0=None):
    """the Float32 term of every array cell (zero outside the interior) for the twelve sums: a (12, Ng...) array, unused slots zero"""
    Ng, D = p.shape, p.ndim
    p, u = np.asarray(p, dtype=f32), np.asarray(u, dtype=f32)
    d, n = measure(body, Ng)
    kk = kern(np.minimum(np.maximum(d, f32(-1)), f32(1)))
    x = centres(Ng)
    x0 = [f32(0)] * D if x0 is None else [f32(v) for v in x0]
    rr = [x[a] - x0[a] for a in range(D)]
    nds = [n[a] * kk for a in range(D)]
    ins = inside(Ng)
    core = tuple(slice(1, m - 1) for m in Ng)

    def sh(f, off):      # f at I + off on the interior, zero elsewhere
        out = np.zeros(Ng, dtype=f32)
        out[core] = f[tuple(slice(1 + o, m - 1 + o) for o, m in zip(off, Ng))]
        return out

    def e(a):
        return tuple(1 if q == a else 0 for q in range(D))

    def add(o1, o2):
        return tuple(a + b for a, b in zip(o1, o2))

    def neg(o):
        return tuple(-a for a in o)

    def du(a, b):
        f = u[..., a]
        if a == b:
            return sh(f, e(a)) - sh(f, (0,) * D)
        return (sh(f, e(b)) + sh(f, add(e(b), e(a))) - sh(f, neg(e(b))) - sh(f, add(neg(e(b)), e(a)))) / f32(4)

    S = [[(du(a, b) + du(b, a)) / f32(2) for b in range(D)] for a in range(D)]
    m2nu = f32(-2) * f32(nu)
    out = np.zeros((12,) + Ng, dtype=f32)
    for a in range(D):
        out[a] = p * nds[a]
        out[3 + a] = _seqsum([(m2nu * S[a][b]) * nds[b] for b in range(D)])
    pm = _cross(rr, nds)
    sn = [_seqsum([S[a][b] * nds[b] for b in range(D)]) for a in range(D)]
    vm = _cross(rr, sn)
    for a in range(D):
        out[6 + a] = p * pm[a]
        out[9 + a] = m2nu * vm[a]
    out[:, ~ins] = 0
    return out


def sums(body, p, u, nu, x0=None, mask=None):
    """the twelve Float64 sums (over `mask` if given)"""
    t = terms(body, p, u, nu, x0).astype(np.float64)
    if mask is not None:
        t = t * mask
    return t.reshape(12, -1).sum(axis=1)


def tolerances(body, p, u, nu, x0=None):
    """the bound of the issue for two Float64 sums of the same Float32 terms in different orders: |Δ| ≤ n_b²·2⁻⁵³·max|term|, with max|term| bounded
    by max|p| (pressure), 2ν·D·max|∂u| (viscous), each times the largest |x − x₀| of the interior for the moments -> (tol_pF, tol_vF, tol_pM, tol_vM)"""
    Ng, D = p.shape, p.ndim
    _, _, nb, _ = band(body, Ng)
    u = np.asarray(u, dtype=np.float64)
    dmax = 0.0
    for a in range(D):
        for b in range(D):
            dmax = max(dmax, float(np.abs(np.diff(u[..., a], axis=b)).max()))     # every ∂(i,j,I,u) is a difference, or a mean of differences, of neighbours
    x = centres(Ng)
    x0 = [0.0] * D if x0 is None else x0
    r = np.sqrt(sum((x[a].astype(np.float64) - float(x0[a])) ** 2 for a in range(D)))[inside(Ng)].max()
    k = float(nb) ** 2 * 2.0 ** -53
    tp, tv = k * float(np.abs(p).max()), k * 2 * float(nu) * D * dmax
    return tp, tv, tp * r, tv * r


# ---- the geometry matrix (every shape at most 64×32×24) ----
def _rot_set():
    mp = RigidMap((30.2, 15.7, 11.6), (0.3, -0.2, 0.5))
    return (Body(("sphere", (0.0, 0.0, 0.0), 4.0), mp) | Body(("capsule", (3.0, 0.0, 0.0), 2.5, (1.0, 0.5, 0.0), 4.0), mp)) - Body(("sphere", (-2.0, 1.0, 0.0), 2.0), mp)


CASES = {
    # name: dims, body factory, perdir, moment origin, [non-empty band, fewer active tiles than tiles]
    "sphere_inside": dict(dims=(64, 32, 24), body=lambda: Body(("sphere", (20.3, 15.6, 11.7), 5.0)), x0=(20.0, 16.0, 12.0)),
    "zcyl_periodic": dict(dims=(64, 32, 24), body=lambda: Body(("cylinder", (20.3, 15.6, 0.0), 4.0, 2)), perdir=(3,), x0=(20.0, 16.0, 12.0)),
    "xwall_cut": dict(dims=(64, 32, 24), body=lambda: Body(("sphere", (1.2, 15.6, 11.7), 5.0)), x0=(0.0, 16.0, 12.0)),
    "floor": dict(dims=(64, 32, 24), body=lambda: Body(("plane", (0.0, 6.4, 0.0), (0.0, 1.0, 0.0))), x0=(32.0, 0.0, 12.0)),
    "ragged_48x20x12": dict(dims=(48, 20, 12), body=lambda: Body(("sphere", (40.3, 16.6, 9.7), 3.0)), x0=(40.0, 16.0, 10.0)),
    "rotated_set": dict(dims=(64, 32, 24), body=_rot_set, x0=(30.0, 16.0, 12.0)),
    "circle2d": dict(dims=(32, 24), body=lambda: Body(("sphere", (11.0, 11.0), 3.0)), x0=(11.0, 11.0)),
    "outside": dict(dims=(32, 16, 16), body=lambda: Body(("sphere", (-20.0, 8.0, 8.0), 4.0)), x0=(0.0, 8.0, 8.0), nonempty=False),
    # built to violate "fewer active tiles than tiles": every one of its 9 tiles is cut by the shell
    "all_active": dict(dims=(16, 8, 8), body=lambda: Body(("sphere", (8.0, 4.0, 4.0), 4.5)), x0=(8.0, 4.0, 4.0), skips=False),
}


def case(name):
    c = dict(perdir=(), nonempty=True, skips=True)
    c.update(CASES[name])
    c["body"] = c["body"]()
    c["Ng"] = tuple(n + 2 for n in c["dims"])
    D = len(c["dims"])
    c["uBC"] = (1.0,) + (0.0,) * (D - 1)
    c["L"], c["nu"] = 8.0, 8.0 / 100
    return c
