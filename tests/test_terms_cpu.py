"""The separable terms without a GPU: the cases of tests/terms_ref.py hold what they are there for, the restatement is what the header states, and the new
entry points are declared alike in include/wlhip.h and _lib.py."""
import os
import re

import numpy as np
import pytest

import terms_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_entry_points_declared_and_bound():
    from waterlily_jl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "wlhip.h"), encoding="utf-8").read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    for name, arity in (("wl_accel_terms", 6), ("wl_bc_vec_terms", 8), ("wl_sim_set_terms", 4), ("wl_sim_term", 2), ("wl_sim_set_term_coeffs", 4)):
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == arity, name
        assert len(_lib.SIGNATURES[name][1]) == arity, name
        if m.group(1).count("void*"):
            assert re.search(r"void\*\s*hip_stream\b", m.group(1)), name      # the stream scenarios live in tests/test_gpu_streams_terms.py
    L = _lib.lib()
    assert all(hasattr(L, n) for n in ("wl_accel_terms", "wl_bc_vec_terms", "wl_sim_set_terms", "wl_sim_term", "wl_sim_set_term_coeffs"))


def test_element_counts_hit_both_instances():
    counts = {(sh, off): tr.count(sh) for sh, off in tr.ACCEL_SHAPES}
    assert any(n % 4 == 0 and off == 0 for (sh, off), n in counts.items())       # 16-byte instance
    assert any(n % 4 != 0 for n in counts.values())                             # one-element instance by the count
    assert any(n % 4 == 0 and off % 4 != 0 for (sh, off), n in counts.items())   # … and by the alignment, on a count that is a multiple of 4
    assert counts[((10, 6, 6), 0)] == 3 * 360 and counts[((7, 6, 5), 0)] == 3 * 210 and counts[((9, 7), 0)] == 2 * 63
    assert {K for _, K, _ in tr.ACCEL_CASES} == {1, 2, 3, 4}


def test_cases_hold_a_zero_coefficient_and_a_negative_zero():
    for q, (sh, K, off) in enumerate(tr.ACCEL_CASES):
        F, r = tr.random_fields(sh, K, q)
        c = tr.coefficients(K, q)
        assert np.any(np.signbit(F[K - 1]) & (F[K - 1] == 0)), (sh, K)
        assert np.any(np.signbit(r) & (r == 0))
        if K >= 2:
            assert c[1] == 0.0
        assert all(np.isfinite(c))
        # the order matters on these data: summing from the other end changes bits
        if K == 4:      # (with K = 3 the zero coefficient leaves two addends, and a sum of two commutes)
            assert not np.array_equal(tr.combine32(F, c), tr.combine32(F[::-1], c[::-1]))


@pytest.mark.parametrize("shape,perdir", tr.BC_CASES)
@pytest.mark.parametrize("K", [1, 3])
def test_bc_tables_differ_along_edge_and_corner_chains(shape, perdir, K):
    """consecutive cells of a chain hold different table values, so (U(c) + v) − U(c′) evaluated in another order, or on another cell, changes the bits"""
    F, _ = tr.random_fields(shape, K, 77 + K)
    Ub = tr.combine32(F, tr.coefficients(K, 5))
    nsteps = 0
    for cells in tr.corner_chains(shape, perdir):
        for a in range(len(shape)):
            vals = [Ub[c + (a,)] for c in cells]
            assert all(vals[q] != vals[q + 1] for q in range(len(vals) - 1)), (cells, a)
            nsteps = max(nsteps, len(cells) - 1)
    nonper = len(shape) - len(perdir)
    assert nsteps == nonper      # the corner chain has one Neumann step per non-periodic direction


def test_unit_fields_combine_to_the_coefficients_exactly():
    for dims in ((5, 4), (4, 3, 5)):
        D = len(dims)
        Ng = tuple(n + 2 for n in dims)
        F = []
        for k in range(D):
            f = np.zeros(Ng + (D,), dtype=f32, order="F")
            f[..., k] = 1
            F.append(f)
        a = [0.5, 0.3 * 0.7, -0.1][:D]
        s = tr.combine32(F, a)
        for k in range(D):
            assert np.all(s[..., k] == f32(a[k]))
        a0 = [0.5, 0.0, -0.1][:D]      # a(t₀) of test_forced_steps_match_oracle at t₀ = 0: the zero is +0 after the sum, as the uniform launch adds it
        s = tr.combine32(F, a0)
        assert np.all(s[..., 1] == 0) and not np.any(np.signbit(s[..., 1]))


@pytest.mark.parametrize("t", [0.0, 0.25, 1.7])
def test_rotating_frame_tables_reproduce_the_closures(t):
    R = tr.Rotating
    F = R.terms()
    K = len(F)
    assert K == 4
    for fn, coef in ((R.velocity, R.b_t(t)), (R.dvel, R.db_t(t)), (R.g, R.g_t(t))):
        want = tr.closure_table(fn, R.dims, t)
        got = tr.combine32(F, coef).astype(np.float64)
        tol = K * 2.0 ** -23 * np.abs(want).max()
        assert np.abs(got - want).max() <= tol, (fn.__name__, np.abs(got - want).max(), tol)
        assert np.abs(tr.combine64(F, coef) - want).max() <= tol


def test_profile_tables_are_the_closures():
    for case in (tr.Parabolic, tr.Sheared):
        F = case.terms()
        want = tr.closure_table(case.uBC, case.dims, 0.0)
        assert np.array_equal(tr.combine32(F, case.b), want.astype(f32))
    want = tr.closure_table(tr.Sheared.g, tr.Sheared.dims, 0.0)
    got = tr.combine32(tr.Sheared.terms(), tr.Sheared.g_t)
    assert np.abs(got - want).max() <= 2 * 2.0 ** -23 * np.abs(want).max()


def test_tabulate_is_loc():
    import waterlily_jl_amd as w
    dims = (5, 4, 3)
    F = w.tabulate(lambda i, x: x[0] + 10 * x[1] + 100 * x[2], dims)
    assert F.shape == (7, 6, 5, 3) and F.dtype == f32 and F.flags.f_contiguous
    for I in ((1, 1, 1), (7, 6, 5), (3, 2, 4)):
        for i in (1, 2, 3):
            x = w.loc(i, I)
            assert F[tuple(k - 1 for k in I) + (i - 1,)] == f32(x[0] + 10 * x[1] + 100 * x[2])
    assert np.array_equal(F, tr.tabulate(lambda i, x: x[0] + 10 * x[1] + 100 * x[2], dims))
