"""NumPy restatement of the reference's `sgs!` with the docstring's `smagorinsky` νₜ — the yardstick of the sgs tests.

Written from the reference's statements, literally: the rate-of-strain tensor is materialised per cell and the (i,j) sweeps
run one after the other.
  src/util.jl:66-76      sgs!(flow,u,t; νₜ,S,Cs,Δ)
  src/util.jl:62         smagorinsky(I;S,Cs,Δ) = (Cs*Δ)^2*sqrt(dot(S[I,:,:],S[I,:,:]))     (sqrt(S:S), the code example — not the prose's sqrt(2S:S))
  src/Metrics.jl:42-44   ∂(i,j,I,u): i==j ? u[I+δᵢ,i]-u[I,i] : (u[I+δⱼ,i]+u[I+δⱼ+δᵢ,i]-u[I-δⱼ,i]-u[I-δⱼ+δᵢ,i])/4
  src/Metrics.jl:140     S(I,u) = (∂(i,j,I,u)+∂(j,i,I,u))/2
  src/core.jl:55-57      inside_u(dims,j): 3:dims[j]-1 along j, 2:dims[k] (upper ghost included) elsewhere
S is zero outside inside(σ) (a zero-initialised buffer: the library's definition of the cells the reference never writes).
Arrays are Julia-shaped: u, f (Ng...,D); σ (Ng...); indices below are 0-based."""
import numpy as np


def _sl(n, lo, hi, shift=0):
    """0-based slice of the Julia range lo:hi (1-based, inclusive) shifted by `shift` cells"""
    return slice(lo - 1 + shift, hi + shift)


def _inside(Ng, shift=None):
    """inside(a): 2:N-1 in every direction (src/core.jl:47); shift: per-direction offset"""
    D = len(Ng)
    shift = shift or (0,) * D
    return tuple(_sl(Ng[d], 2, Ng[d] - 1, shift[d]) for d in range(D))


def _delta(D, *dirs):
    s = [0] * D
    for d in dirs:
        s[d] += 1
    return s


def partial(i, j, u):
    """∂(i,j,I,u) for every I ∈ inside   src/Metrics.jl:42-44 (0-based i,j)"""
    Ng, D = u.shape[:-1], u.shape[-1]
    ui = u[..., i]
    at = lambda sh: ui[_inside(Ng, sh)]      # noqa: E731
    if i == j:
        return at(_delta(D, i)) - at([0] * D)
    pj, mj = _delta(D, j), [-v for v in _delta(D, j)]
    pji = [a + b for a, b in zip(pj, _delta(D, i))]
    mji = [a + b for a, b in zip(mj, _delta(D, i))]
    return (at(pj) + at(pji) - at(mj) - at(mji)) / u.dtype.type(4)


def strain(u):
    """S[I,:,:] .= S(I,u) over I ∈ inside(σ), zero elsewhere   src/util.jl:68, src/Metrics.jl:140"""
    Ng, D = u.shape[:-1], u.shape[-1]
    S = np.zeros(Ng + (D, D), dtype=u.dtype)
    two = u.dtype.type(2)
    for i in range(D):
        for j in range(D):
            S[_inside(Ng) + (i, j)] = (partial(i, j, u) + partial(j, i, u)) / two
    return S


def smagorinsky(S, Cs, Delta):
    """νₜ(I) = (Cs*Δ)^2*sqrt(dot(S[I,:,:],S[I,:,:])) for every I   src/util.jl:62 (dot runs over the storage order: first index fastest)"""
    T = S.dtype.type
    D = S.shape[-1]
    acc = np.zeros(S.shape[:-2], dtype=S.dtype)
    for j in range(D):
        for i in range(D):
            acc = acc + S[..., i, j] * S[..., i, j]
    c = T(Cs) * T(Delta)
    return (c * c) * np.sqrt(acc)


def sgs(f, u, Cs, Delta, sigma=None, dtype=np.float64):
    """sgs!(flow,u,t; νₜ=smagorinsky,S,Cs,Δ)   src/util.jl:66-76.  Returns (f, σ, νₜ) as new arrays of `dtype`; f and σ start from the
    given arrays (σ: zeros if None) so that what the sweeps leave in σ can be compared too."""
    T = np.dtype(dtype).type
    u = np.asarray(u, dtype=dtype)
    f = np.array(f, dtype=dtype, order="F")
    Ng, D = u.shape[:-1], u.shape[-1]
    sig = np.zeros(Ng, dtype=dtype, order="F") if sigma is None else np.array(sigma, dtype=dtype, order="F")
    S = strain(u)                                                                    # :68
    nut = smagorinsky(S, T(Cs), T(Delta))
    for i in range(D):                                                               # :69
        for j in range(D):
            R = tuple(_sl(Ng[d], 3, Ng[d] - 1) if d == j else _sl(Ng[d], 2, Ng[d]) for d in range(D))          # inside_u(N,j)  src/core.jl:55-57
            Rm = tuple(_sl(Ng[d], 3, Ng[d] - 1, -1) if d == j else _sl(Ng[d], 2, Ng[d]) for d in range(D))     # I-δ(j,I)
            sig[R] = -nut[R] * (u[R + (i,)] - u[Rm + (i,)])                          # :71  ∂(j,CI(I,i),u) = u[I,i]-u[I-δⱼ,i]
            f[R + (i,)] += sig[R]                                                    # :72
            f[Rm + (i,)] -= sig[R]                                                   # :74
    return f, sig, nut


def smooth_field(shape, rng, modes=3, amp=1.0):
    """a random smooth field on `shape` (sum of a few low-wavenumber products of sines), float64"""
    grids = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    out = np.zeros(shape)
    for _ in range(modes):
        term = np.full(shape, amp * rng.uniform(0.3, 1.0))
        for d, n in enumerate(shape):
            term = term * np.sin(2 * np.pi * rng.integers(1, 3) * grids[d] / n + rng.uniform(0, 2 * np.pi))
        out += term
    return out
