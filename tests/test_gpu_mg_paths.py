"""The launch sequence of the multigrid handle, per form of smooth! and per stage of Vcycle! / solver! (csrc/wl_mg.hip).

The bitwise tests do not notice an extra flush of a deferred prolongation, a lost deferral or a fill! that came back: the numbers stay the same, a
launch is added.  So each handle below records `wl_launch_count()` across one Vcycle!(0), one smooth!(l) per level and one solver! capped at two
iterations, with `wl_mg_smoother_kind(l)` per level, and compares them with constants.  A pull request that means to change a count edits the constant.
The handles are the smallest at which each form exists; the z-slab forms stay with tests/test_gpu_slab.py and its workers."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N3 = (66, 34, 34)      # interior 64×32×32: level 0 runs the pair kernels (nx = 66 even ≥ 34, ny = 34, 32 planes), level 1 (34×18×18) the one-cell blocked
                       # kernels, the levels from 18×10×10 down the LDS tail

# measured with the library of commit 84a6086 (the parent of the change that introduced wl_mg.hip) and, in the same GPU visit, with that change's:
#   kinds per level, launches of Vcycle!(0), launches of smooth!(l) per level, (launches, nᵖ) of solver!(itmx = 2)
EXPECTED = {
    "nobody": ([2, 1, 0, 0, 0, 0], 8, [2, 2, 5, 5, 5, 5], (23, 2)),         # pair kernels, one-cell blocked kernels, the LDS tail below
    "zsplit": ([3, 1, 0, 0, 0, 0], 10, [6, 2, 5, 5, 5, 5], (40, 2)),        # three plane ranges on level 0: 3 Jacobi!, 3 + 3 smoother launches
    "periodic": ([0, 0, 0, 0, 0, 0], 75, [8, 8, 8, 8, 8, 8], (176, 2)),     # passes on every level, perBC! launches, every prolongation flushed
    "2d": ([0, 0, 0, 0, 0], 32, [5, 5, 5, 5, 5], (82, 2)),                  # passes, no tail
}
EXPECTED_RSKIP = ([45, 56], 2, 1)      # launches of mom_step! 1 and 2, then the counters rskip, rskip_redo


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    return w


def _rhs(shape):
    """a right-hand side with every wavelength in it and no mean inside"""
    z = np.zeros(shape, dtype=np.float32, order="F")
    inner = tuple(slice(1, n - 1) for n in shape)
    z[inner] = np.random.default_rng(11).standard_normal(tuple(n - 2 for n in shape)).astype(np.float32)
    z[inner] -= z[inner].mean(dtype=np.float64).astype(np.float32)
    return z


def _record(w, mg):
    """(kinds, Vcycle!(0), [smooth!(l)], (solver!, nᵖ)) of the handle `mg` (a wl_mg*)"""
    lib, st = w.lib(), w.core.stream()
    check = w._lib.check
    nl = lib.wl_mg_nlevels(mg)
    kinds = [int(lib.wl_mg_smoother_kind(mg, l)) for l in range(nl)]

    def launches(call):
        n0 = lib.wl_launch_count()
        check(call())
        return int(lib.wl_launch_count() - n0)

    vc = launches(lambda: lib.wl_mg_vcycle(mg, 0, 1.0, st))
    sm = [launches(lambda l=l: lib.wl_mg_smooth(mg, l, 4, 1.0, st)) for l in range(nl)]
    n, r1, rinf = C.c_int(), C.c_double(), C.c_float()
    so = launches(lambda: lib.wl_mg_solve(mg, 1e-30, 2, C.byref(n), C.byref(r1), C.byref(rinf), st))      # tol: the cap ends the loop
    check(lib.wl_stream_sync(st))
    assert np.isfinite(r1.value) and np.isfinite(rinf.value)
    return (kinds, vc, sm, (so, int(n.value)))


def _bare(w, shape, perdir=()):
    D = len(shape)
    L = w.to_device(np.full(shape + (D,), 1.0, dtype=np.float32, order="F"))
    w.BC_(L, (0,) * D, perdir=perdir)
    x, z = w.jl_zeros(shape), w.to_device(_rhs(shape))
    return w.MultiLevelPoisson(x, L, z, perdir=perdir), (x, L, z)


def _zsplit_sim(w):
    """the 64×32×32 grid with coefficients off the constant pattern on two middle planes, the z-split's size gate lowered"""
    sim = w.FusedSimulation(tuple(n - 2 for n in N3), (0, 0, 0), 32, U=1, nu=0.01, ic="tgv")
    mu0 = sim.field("mu0")
    mu0[20:40, 10:20, 16:18, :] = 0.5
    sim.set_field("mu0", mu0)
    sim.set_option("zsplit", 2)
    sim.update_()
    sim.set_field("sigma", _rhs(N3))
    assert sim.counter("part") == 1
    return sim


def _measure(w, case):
    if case == "nobody":
        ml, keep = _bare(w, N3)
        return _record(w, ml._h)
    if case == "periodic":
        ml, keep = _bare(w, N3, perdir=(1,))
        return _record(w, ml._h)
    if case == "2d":
        ml, keep = _bare(w, (34, 34))
        return _record(w, ml._h)
    sim = _zsplit_sim(w)
    return _record(w, w.lib().wl_sim_pois(sim._h))


def _measure_rskip(w):
    sim = w.FusedSimulation(tuple(n - 2 for n in N3), (0, 0, 0), 32, U=1, nu=32 / 1600.0, ic="tgv")
    sim.set_option("rskip", 1)
    steps = []
    for _ in range(2):
        n0 = sim.counter("launches")
        sim.mom_step_()
        steps.append(sim.counter("launches") - n0)
    return (steps, sim.counter("rskip"), sim.counter("rskip_redo"))


@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_launches_of_vcycle_smooth_and_solver(w, case):
    got = _measure(w, case)
    print("launches", case, repr(got))
    assert got == EXPECTED[case]


def test_launches_and_skipped_stores_of_two_steps_with_rskip(w):
    got = _measure_rskip(w)
    print("launches", "rskip", repr(got))
    assert got == EXPECTED_RSKIP
