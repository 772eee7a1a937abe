"""residual!'s mean shift (src/Poisson.jl:95-97) at the edge of its threshold |Σr/N| ≤ 2eps(Float32), on the oracle (CPU).

The GPU tests of the speculative projection (tests/test_gpu_speculation.py) make the shift due — or not — with one nonzero
residual δ: Σr = δ exactly in any summation order, so the decision is float32(δ)/float32(N) against 2eps.  This pins that
construction: at the largest δ that is not due r stays as it is, one float above it r is shifted."""
import numpy as np
import pytest

f32 = np.float32


def shift_edge(n):
    """(largest float32 δ with float32(δ)/float32(n) ≤ 2eps, the next float above it): the shift is not due / due"""
    n, lim, inf = f32(n), f32(2) * np.finfo(f32).eps, f32(np.inf)
    d = f32(lim * n)
    while d / n > lim:
        d = np.nextafter(d, f32(0))
    while np.nextafter(d, inf) / n <= lim:
        d = np.nextafter(d, inf)
    return d, np.nextafter(d, inf)


@pytest.mark.parametrize("dims", [(64, 32, 32), (70, 44, 18), (32, 32)])
@pytest.mark.parametrize("sign", [1, -1])
def test_residual_shift_at_the_threshold_on_a_spike(oracle, dims, sign):
    D = len(dims)
    Ng = tuple(n + 2 for n in dims)
    N = int(np.prod(dims))
    lo, hi = shift_edge(N)
    lim = f32(2) * np.finfo(f32).eps
    assert lo / f32(N) <= lim < hi / f32(N)
    if N & (N - 1) == 0:
        assert lo == f32(2.0 ** -22 * N)         # a power of two: exactly 2eps
    L = np.ones(Ng + (D,), dtype=f32, order="F")
    oracle.BC(L, (0,) * D)
    spike = tuple(n // 2 for n in dims)
    for delta, due in ((np.nextafter(lo, f32(0)), False), (lo, False), (hi, True)):
        delta = f32(sign * delta)
        x = np.zeros(Ng, dtype=f32, order="F")
        z = np.zeros(Ng, dtype=f32, order="F")
        z[spike] = delta
        p = oracle.Poisson(x, L, z)
        p.residual()
        r = p.field("r").copy()
        inner = tuple(slice(1, -1) for _ in range(D))
        if not due:
            assert np.array_equal(r, z), float(delta)
            assert p.L1() == abs(float(delta))
        else:
            s = delta / f32(N)
            want = np.zeros(Ng, dtype=f32, order="F")
            want[inner] = -s
            want[spike] = delta - s
            assert np.array_equal(r, want), float(delta)
            l1 = abs(float(delta) - float(s)) + (N - 1) * abs(float(s))       # ≈ 2|δ|: the first logged L₁ tells the decision (|δ| or ≈ 2|δ|)
            assert abs(p.L1() - l1) < 1e-5 * l1
