"""NumPy restatement of the reference's flow diagnostics — the yardstick of the metrics tests.

Written from the reference's statements, literally (0-based component and direction indices below unless said otherwise):
  src/Metrics.jl:33-35   ke(I,u,U)        = 0.125·Σᵢ (u[I,i]+u[I+δᵢ,i]−2Uᵢ)²
  src/Metrics.jl:42-44   ∂(i,j,I,u)       sgs_ref.partial
  src/Metrics.jl:54-58   λ₂(I,u)          J = [∂(i,j,I,u)], S,Ω = (J+J')/2,(J−J')/2, eigvals(Hermitian(S²+Ω²))[2]
  src/Metrics.jl:68      curl(i,I,u)      = ∂(j,CI(I,k),u) − ∂(k,CI(I,j),u), (j,k) the two directions after i; ∂(a,CI(I,c),u) = u[I,c]−u[I−δₐ,c]
  src/Metrics.jl:74      ω(I,u)ᵢ          = ∂(k,j,I,u) − ∂(j,k,I,u)
  src/Metrics.jl:80      ω_mag(I,u)       = √(ω'ω)
  src/Metrics.jl:87-91   ω_θ(I,z,center,u): θ = z×(loc(0,I)−center), n = ‖θ‖, n ≤ eps(n) ? 0 : θ'ω/n
  src/Metrics.jl:99-109  helicity(I,u,ω)
Every function takes Julia-shaped arrays (u, ω: (Ng...,D)), computes in `dtype` and returns the values on the INSIDE cells."""
import numpy as np

from sgs_ref import _delta, _inside, partial


def _prep(u, dtype):
    u = np.asarray(u, dtype=dtype)
    return u, u.shape[:-1], u.shape[-1], np.dtype(dtype).type


def ke(u, U=None, dtype=np.float64):
    u, Ng, D, T = _prep(u, dtype)
    U = [T(0)] * D if U is None else [T(v) for v in U]
    acc = None
    for i in range(D):
        t = u[..., i][_inside(Ng)] + u[..., i][_inside(Ng, _delta(D, i))] - T(2) * U[i]
        acc = t * t if acc is None else acc + t * t
    return T(0.125) * acc


def jacobian(u, dtype=np.float64):
    """J[..., i, j] = ∂(i,j,I,u) on inside"""
    u, Ng, D, T = _prep(u, dtype)
    return np.stack([np.stack([partial(i, j, u) for j in range(D)], -1) for i in range(D)], -2)


def lambda2_matrix(u, dtype=np.float64):
    """S²+Ω² on inside, (…,3,3)"""
    J = jacobian(u, dtype)
    T = J.dtype.type
    Jt = np.swapaxes(J, -1, -2)
    S, W = (J + Jt) / T(2), (J - Jt) / T(2)
    return S @ S + W @ W


def lambda2(u, dtype=np.float64):
    return np.linalg.eigvalsh(lambda2_matrix(u, dtype))[..., 1]


def curl(i, u, dtype=np.float64):
    """curl(i,I,u) with the reference's 1-based i (2-D: i = 3)"""
    u, Ng, D, T = _prep(u, dtype)
    j, k = i % 3, (i + 1) % 3                      # 0-based directions after i
    d = lambda c, a: u[..., c][_inside(Ng)] - u[..., c][_inside(Ng, [-v for v in _delta(D, a)])]      # noqa: E731  ∂(a,CI(I,c),u)
    return d(k, j) - d(j, k)


def omega(u, dtype=np.float64):
    u, Ng, D, T = _prep(u, dtype)
    assert D == 3
    return np.stack([partial((i + 2) % 3, (i + 1) % 3, u) - partial((i + 1) % 3, (i + 2) % 3, u) for i in range(3)], -1)


def omega_mag(u, dtype=np.float64):
    w = omega(u, dtype)
    return np.sqrt(w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1] + w[..., 2] * w[..., 2])


def _cross(a, b):
    return [a[(i + 1) % 3] * b[(i + 2) % 3] - a[(i + 2) % 3] * b[(i + 1) % 3] for i in range(3)]


def omega_theta(u, z, center, dtype=np.float64):
    u, Ng, D, T = _prep(u, dtype)
    w = omega(u, dtype)
    x = np.meshgrid(*[np.arange(1, n - 1).astype(dtype) - T(0.5) for n in Ng], indexing="ij")      # loc(0,I) = I − 1.5 (Julia index)
    th = _cross([T(v) for v in z], [x[d] - T(center[d]) for d in range(3)])
    n = np.sqrt(th[0] * th[0] + th[1] * th[1] + th[2] * th[2])
    dot = th[0] * w[..., 0] + th[1] * w[..., 1] + th[2] * w[..., 2]
    small = n <= np.spacing(n)
    return np.where(small, T(0), dot / np.where(small, T(1), n))


def helicity(u, w, dtype=np.float64):
    u, Ng, D, T = _prep(u, dtype)
    w = np.asarray(w, dtype=dtype)
    assert D == 3
    s = np.zeros(tuple(n - 2 for n in Ng), dtype=dtype)
    for d in range(3):
        d1, d2 = (d + 1) % 3, (d + 2) % 3
        umid = u[..., d][_inside(Ng)] + u[..., d][_inside(Ng, _delta(3, d))]
        for i1 in (0, 1):
            for i2 in (0, 1):
                s = s + umid * w[..., d][_inside(Ng, _delta(3, *([d1] * i1 + [d2] * i2)))]
    return s / T(8)


# ---- inputs the tests share ------------------------------------------------------------------------------------------------
def kat_u(dtype=np.float32):
    """apply!((i,x)->x[i]+prod(x),u) on zeros(3,4,5,3)   test/test_metrics.jl:8 — x = loc(i,I): I − 1.5 − δᵢ/2 (Julia index)"""
    Ng = (3, 4, 5)
    u = np.zeros(Ng + (3,), dtype=np.float64, order="F")
    for i in range(3):
        x = np.meshgrid(*[np.arange(1, n + 1) - 1.5 - (0.5 if d == i else 0.0) for d, n in enumerate(Ng)], indexing="ij")
        u[..., i] = x[i] + x[0] * x[1] * x[2]
    return np.asfortranarray(u.astype(dtype))


def kat_helicity(dtype=np.float32):
    """u_h, ω_h of test/test_metrics.jl:25-26 on 6³"""
    Ng = (6, 6, 6)
    u, w = np.zeros(Ng + (3,), np.float64, order="F"), np.zeros(Ng + (3,), np.float64, order="F")
    x = np.meshgrid(*[np.arange(1, n + 1) - 1.5 - (0.5 if d == 0 else 0.0) for d, n in enumerate(Ng)], indexing="ij")      # loc(1,I)
    u[..., 0] = x[0]
    w[..., 0] = x[1] - 0.5 + 1
    return np.asfortranarray(u.astype(dtype)), np.asfortranarray(w.astype(dtype))


def analytic_u(kind, Ng, par, dtype=np.float32):
    """the three analytic λ₂ cases on the staggered grid (component i at loc(i,I)):
    "rotation" u = (−w·y, w·x, 0) → λ₂ = −w²; "shear" u = (a·y, 0, 0) → λ₂ = 0 (A ≡ 0); "expansion" u = c·(x, y, z) → λ₂ = c²"""
    u = np.zeros(tuple(Ng) + (3,), np.float64, order="F")
    for i in range(3):
        x = np.meshgrid(*[np.arange(1, n + 1) - 1.5 - (0.5 if d == i else 0.0) for d, n in enumerate(Ng)], indexing="ij")
        if kind == "rotation":
            u[..., i] = (-par * x[1], par * x[0], 0 * x[0])[i]
        elif kind == "shear":
            u[..., i] = (par * x[1], 0 * x[0], 0 * x[0])[i]
        else:
            u[..., i] = par * x[i]
    return np.asfortranarray(u.astype(dtype))
