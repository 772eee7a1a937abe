"""Every fast path against the plain one on both sides of its shape gate: one case per shape of tests/shapegates.py (tests/test_shapegates_cpu.py shows that
the shapes cover what they claim).  A case builds three handles on the same seeded random u⁰ — A with default switches and the size gates opened, P with every
switch at its un-fused, un-deferred value (optmatrix.PLAIN), D with nothing set at all, what a user of a small grid gets — and makes optmatrix.CALLS on each.
After every call u, u⁰, p on every cell (ghosts included) as raw bits, pois.n and the Δt history of A and of D equal P's; A's levels, smoother kinds and path
counters are what shapegates.predicted() derives from the restated gates, and D's what it derives with the size gates shut (resjac = tailfuse = 0 among them).
No tolerance between handles.  P itself is tied to the oracle after the same calls with the comparison of tests/test_gpu_optmatrix.py::test_plain_is_the_oracle,
for every shape of at most 300 000 array cells; the seven larger shapes (the three 448-wide ones, 3072×8×8, 4096×8×8, 5624×8×8, 5632×8×8) are held to P only.

If A and P differ at some shape, the message carries solver!'s logged r₁ of both: a seed may be changed (shapegates.SEEDS) only for a reordering tie."""
import time

import numpy as np
import pytest

import callseq
import optmatrix as om
import shapegates as sg

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    yield w
    w.lib().wl_reset_process_options()


def same_bits(what, N, got, ref):
    assert got["err"] is None, "%s %r: a call returned an error: %s" % (what, N, got["err"])
    d = om.first_diff(got["snaps"], ref["snaps"])
    if d is not None:
        q = d[0]
        raise AssertionError("%s %r: after call %d %s differs from PLAIN in %s cells, first %s\nlogged r1 of the call's last solve: %r\nPLAIN's: %r\ncounters %r"
                             % ((what, N) + d[:4] + (got["logs"][q][0], ref["logs"][q][0], got["cnt"])))


def oracle_tie(oracle, N, P):
    """P after each call against the oracle after the same steps: the quantities and bounds of test_gpu_optmatrix.py::test_plain_is_the_oracle"""
    so = oracle.Simulation(tuple(N), callseq.UBC, N[0], U=1, nu=sg.NU, T=f32)
    so.field("u")[...] = P["u_init"]
    so.field("u0")[...] = P["u_init"]
    for q, c in enumerate(om.CALLS):
        for _ in range(c[1] if len(c) > 1 else 1):
            so.step(remeasure=False)
        s = P["snaps"][q]
        du, dp = float(np.abs(s.field("u") - so.u).max()), float(np.abs(s.field("p") - so.p).max())
        print("oracle: call", q, "pois_n", s.pois_n, so.pois_n, "max|du| %.3g max|dp| %.3g" % (du, dp))
        assert list(s.pois_n) == list(so.pois_n), (N, q)
        assert np.allclose(np.array(s.dt, dtype=np.float64), np.array(so.dt), rtol=1e-6), (N, q)
        assert du < 2e-5, (N, q, du)
        assert dp < 2e-4, (N, q, dp)


def check_case(w, oracle, case):
    N, extra = case
    t0 = time.perf_counter()
    P = sg.run(w, N, sg.PLAIN_ROW, True)
    assert P["err"] is None, (N, "PLAIN", P["err"])
    assert all(P["cnt"][a] <= 0 for a in sg.COUNTERS), (N, "a counted path ran on the PLAIN handle", P["cnt"])
    assert all(np.isfinite(s.field("u")).all() and np.isfinite(s.field("p")).all() for s in P["snaps"]), N
    A = sg.run(w, N, extra, True)
    print("A: kinds", A["kinds"], "levels", A["nlevels"], "counters", A["cnt"], "pois_n", A["snaps"][-1].pois_n if A["snaps"] else None)
    same_bits("default switches, gates opened %r" % (extra,), N, A, P)
    faults = sg.dispatch_faults(N, A, True, extra)
    assert not faults, "%r %r: %s; counters %r" % (N, extra, "; ".join(faults), A["cnt"])
    D = sg.run(w, N, extra, False)
    print("D: kinds", D["kinds"], "counters", D["cnt"])
    same_bits("nothing set %r" % (extra,), N, D, P)
    faults = sg.dispatch_faults(N, D, False, extra)
    assert not faults and D["cnt"]["resjac"] == 0 and D["cnt"]["tailfuse"] == 0, "%r nothing set: %s; counters %r" % (N, "; ".join(faults), D["cnt"])
    t1 = time.perf_counter()
    if not extra and sg.cells(sg.levels(N)[0]) <= sg.ORACLE_CELLS:
        oracle_tie(oracle, N, P)
    print("seconds: handles %.2f oracle %.2f" % (t1 - t0, time.perf_counter() - t1))


@pytest.mark.parametrize("case", sg.CASES, ids=sg.case_id)
def test_shape(w, oracle, case):
    check_case(w, oracle, case)
