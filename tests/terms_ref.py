"""NumPy restatement of the separable terms (include/wlhip.h, separable terms; csrc/wl_terms.hip) and the cases the tests run.

The combination  uBC(i,x,t) = Σₖ bₖ(t)·Fₖ[I,i]  is formed in ONE order by every kernel:  s = fl(c₀·F₀) ; s = fl(s + fl(cₖ·Fₖ)) for k = 1 … K−1 — combine32
states it in Float32 (NumPy rounds every array operation, nothing is fused), combine64 is its Float64 twin.  No GPU, no library: tests/test_terms_cpu.py shows
that the cases hold what they are there for, tests/test_gpu_terms.py runs them."""
import math

import numpy as np

f32 = np.float32


def combine32(F, c):
    s = f32(c[0]) * F[0]
    for k in range(1, len(F)):
        s = s + f32(c[k]) * F[k]
    return np.asfortranarray(s, dtype=f32)


def combine64(F, c):
    s = np.float64(f32(c[0])) * F[0].astype(np.float64)
    for k in range(1, len(F)):
        s = s + np.float64(f32(c[k])) * F[k].astype(np.float64)
    return s


def accel32(r, F, c):
    """k_accel_terms: r[q] = fl(r[q] + s)"""
    return np.asfortranarray(r + combine32(F, c), dtype=f32)


# ---- leaf cases ---------------------------------------------------------------------------------------------------------------
# (array shape with ghosts, K, offset of r in floats): element counts D·cs = 1080 (multiple of 4: the 16-byte instance), 630 and 126 (not: the one-element
# instance), and 1080 with r one float off a 16-byte boundary (the one-element instance on a count that IS a multiple of 4)
ACCEL_SHAPES = [((10, 6, 6), 0), ((7, 6, 5), 0), ((9, 7), 0), ((10, 6, 6), 1)]
ACCEL_CASES = [(sh, K, off) for sh, off in ACCEL_SHAPES for K in (1, 2, 3, 4)]


def count(shape):
    return int(np.prod(shape)) * len(shape)


def random_fields(shape, K, seed):
    """K fields and r of shape `shape + (D,)` with values of mixed sign and magnitude; field K−1 holds −0.0, +0.0 and r holds −0.0 at known places"""
    rng = np.random.default_rng(seed)
    D = len(shape)
    F = [np.asfortranarray((rng.standard_normal(shape + (D,)) * 10.0 ** rng.integers(-2, 3)).astype(f32)) for _ in range(K)]
    r = np.asfortranarray(rng.standard_normal(shape + (D,)).astype(f32))
    F[K - 1].reshape(-1, order="F")[3::17] = f32(-0.0)
    F[K - 1].reshape(-1, order="F")[5::19] = f32(0.0)
    r.reshape(-1, order="F")[3::34] = f32(-0.0)
    return F, r


def coefficients(K, seed):
    """K coefficients, not representable in few bits (products round); for K ≥ 2 coefficient 1 is exactly 0"""
    rng = np.random.default_rng(1000 + seed)
    c = [float(f32(v)) for v in rng.uniform(-2.0, 2.0, size=K)]
    if K >= 2:
        c[1] = 0.0
    return c


# BC!: (shape with ghosts, perdir tuples (1-based directions)); saveexit 0/1 and K = 1, 3 are crossed in by the test
BC_CASES = [((8, 7), ()), ((8, 7), (1,)), ((8, 7), (1, 2)), ((8, 7, 6), ()), ((8, 7, 6), (1,)), ((8, 7, 6), (3,)), ((8, 7, 6), (1, 2))]


def corner_chains(shape, perdir):
    """cells (0-based) of one corner chain and one edge chain as k_bc_vec_fn collects them: from the ghost cell inwards, last direction first, one step per
    non-periodic direction (periodic steps are copies and read no table)"""
    D = len(shape)
    out = []
    for start in ([0] * D, [0] * (D - 1) + [shape[-1] // 2] if D == 3 else [0, shape[1] // 2]):
        J = list(start)
        cells = [tuple(J)]
        for b in range(D - 1, -1, -1):
            if (b + 1) in perdir or J[b] != 0:
                continue
            J[b] = 1
            cells.append(tuple(J))
        out.append(cells)
    return out


# ---- flows --------------------------------------------------------------------------------------------------------------------
def loc_axes(i, Ng):
    """x = loc(i,I) as D broadcastable Float32 axes (core.tabulate builds the same)"""
    D = len(Ng)
    x = []
    for d in range(D):
        sh = [1] * D
        sh[d] = Ng[d]
        x.append((np.arange(1, Ng[d] + 1, dtype=f32) - f32(1.5) - f32(1 if d == i - 1 else 0) / f32(2)).reshape(sh))
    return x


def tabulate(fn, dims):
    Ng = tuple(n + 2 for n in dims)
    D = len(dims)
    F = np.empty(Ng + (D,), dtype=f32, order="F")
    for i in range(1, D + 1):
        F[..., i - 1] = np.broadcast_to(np.asarray(fn(i, loc_axes(i, Ng)), dtype=f32), Ng)
    return F


class Parabolic:
    """test/test_flow.jl:134-140 (make_bl_flow): a steady parabolic inflow profile, K = 1, b = 1"""
    L = 32
    dims = (32, 32)
    nu = 0.001

    @classmethod
    def uBC(cls, i, x, t):
        return float(f32(4.0 * (((x[1] + 0.5) / (2 * cls.L)) - ((x[1] + 0.5) / (2 * cls.L)) ** 2))) if i == 1 else 0.0

    @classmethod
    def terms(cls):
        def f(i, x):
            y = (x[1].astype(np.float64) + 0.5) / (2 * cls.L)
            return 4.0 * (y - y ** 2) if i == 1 else 0.0
        return [tabulate(f, cls.dims)]
    b = [1.0]


class Sheared:
    """a 3-D sheared inflow u₁ = y/16 with the body force g₃(x) = −0.1·y/16, a sphere, periodic in z: K = 2, b = (1, 0), g = (0, −0.1)"""
    dims = (24, 16, 16)
    nu = 0.01
    perdir = (3,)
    body = ("sphere", (8.0, 8.0, 8.0), 3.0)

    @staticmethod
    def uBC(i, x, t):
        return x[1] / 16.0 if i == 1 else 0.0

    @staticmethod
    def g(i, x, t):
        return -0.1 * x[1] / 16.0 if i == 3 else 0.0

    @classmethod
    def terms(cls):
        return [tabulate(lambda i, x: x[1] / f32(16) if i == 1 else 0.0, cls.dims), tabulate(lambda i, x: x[1] / f32(16) if i == 3 else 0.0, cls.dims)]
    b = [1.0, 0.0]
    g_t = [0.0, -0.1]


class Rotating:
    """test/test_flow.jl:142-158: solid-body rotation seen from the rotating frame.  y = ω(x − x₀);
         velocity = (s·y₁ + c·y₂, −c·y₁ + s·y₂)                 K = 4 fields: y₁ and y₂ on component 1, y₁ and y₂ on component 2
         b = (s, c, −c, s)        b′ = ω·(c, −s, s, c)           g = coriolis + centrifugal = (−2ωc + ω, 2ωs, −2ωs, −2ωc + ω)"""
    Lh = 4
    dims = (8, 8)
    om = 1.0 / 4
    x0 = (4.0, 4.0)

    @classmethod
    def velocity(cls, i, x, t):
        s, c = math.sin(cls.om * t), math.cos(cls.om * t)
        y = (cls.om * (x[0] - cls.x0[0]), cls.om * (x[1] - cls.x0[1]))
        return s * y[0] + c * y[1] if i == 1 else -c * y[0] + s * y[1]

    @classmethod
    def dvel(cls, i, x, t):
        s, c = math.sin(cls.om * t), math.cos(cls.om * t)
        y = (cls.om * (x[0] - cls.x0[0]), cls.om * (x[1] - cls.x0[1]))
        return cls.om * (c * y[0] - s * y[1]) if i == 1 else cls.om * (s * y[0] + c * y[1])

    @classmethod
    def g(cls, i, x, t):
        cor = 2 * cls.om * cls.velocity(2, x, t) if i == 1 else -2 * cls.om * cls.velocity(1, x, t)
        return cor + cls.om ** 2 * (x[i - 1] - cls.x0[i - 1])

    @classmethod
    def terms(cls):
        y = lambda x, d: f32(cls.om) * (x[d] - f32(cls.x0[d]))      # noqa: E731  (ω = 1/4 and x₀ are exact in Float32: so is y)
        return [tabulate(lambda i, x, j=j, d=d: y(x, d) if i == j else 0.0, cls.dims) for j in (1, 2) for d in (0, 1)]

    @classmethod
    def b_t(cls, t):
        s, c = math.sin(cls.om * t), math.cos(cls.om * t)
        return [s, c, -c, s]

    @classmethod
    def db_t(cls, t):
        s, c = math.sin(cls.om * t), math.cos(cls.om * t)
        return [cls.om * c, -cls.om * s, cls.om * s, cls.om * c]

    @classmethod
    def g_t(cls, t):
        s, c = math.sin(cls.om * t), math.cos(cls.om * t)
        return [-2 * cls.om * c + cls.om, 2 * cls.om * s, -2 * cls.om * s, -2 * cls.om * c + cls.om]


def closure_table(fn, dims, t):
    """fn(i, x, t) cell by cell at loc(i,I), Float64 (what the reference's closure returns before it is stored)"""
    Ng = tuple(n + 2 for n in dims)
    D = len(dims)
    out = np.empty(Ng + (D,), dtype=np.float64, order="F")
    for I in np.ndindex(*Ng):
        for i in range(1, D + 1):
            x = [float(I[d] + 1) - 1.5 - (0.5 if d == i - 1 else 0.0) for d in range(D)]
            out[I + (i - 1,)] = fn(i, x, t)
    return out
