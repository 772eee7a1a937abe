"""The first projection's tail inside the corrector's conv_diff! loader (option "tailfuse", csrc/wl_convf.hip PROJ) as the DEFAULT on grids of at least
"tailfuse_min" interior cells: with untouched options at or above the gate every step takes the path and u, u⁰, p (every cell, raw bits), pois.n and the Δt
history equal a tailfuse=0 run; below the gate the untouched default leaves the separate tail alone; an explicit tailfuse=1 forces the path at any whole-tile
shape.  The loader takes x[k−1] from the plane it projected before and x[i−1] from the neighbouring lane, so it is checked against tailfuse=0 on shapes that
exercise exactly that: several z-chunks (the carried plane crosses chunk starts), one chunk that holds both z walls, nonzero U on every face, multi-step
calls with p read in between."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

f32 = np.float32
DIMS = (64, 32, 24)      # whole tiles (64 × 16), the smallest shape class the fused head takes
UBC = (0.3, -0.2, 0.1)


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    yield w
    w.lib().wl_reset_process_options()      # resjac_min / convt_min / convt are process-wide


def cells(dims):
    return int(np.prod(dims))


def make(w, dims, uBC, seed, lam=0, **opts):
    """random initial velocity (the same for the same seed), the size gates of the tiled conv_diff! and the fused head lowered, then `opts` in order"""
    rng = np.random.default_rng(seed)
    Ng = tuple(n + 2 for n in dims)
    u_init = np.asfortranarray(rng.uniform(-0.4, 0.4, size=Ng + (3,)).astype(f32))
    sg = w.FusedSimulation(dims, uBC, dims[0], U=1, nu=0.02, u0=u_init, lam=lam)
    sg.set_option("resjac_min", 0)
    sg.set_option("convt_min", 0)
    for k, v in opts.items():
        sg.set_option(k, v)
    return sg


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_state(a, b, what):
    for name in ("u", "u0", "p"):
        x, y = bits(a.field(name)), bits(b.field(name))
        assert np.array_equal(x, y), (what, name, int((x != y).sum()))
    assert a.pois_n == b.pois_n, (what, a.pois_n, b.pois_n)
    da, db = [f32(v).view(np.uint32) for v in a.dt], [f32(v).view(np.uint32) for v in b.dt]
    assert da == db, (what, [float(v) for v in a.dt], [float(v) for v in b.dt])


def run(sg, calls):
    n = 0
    for k in calls:
        if k == 0:
            sg.mom_step_()
        else:
            sg.mom_steps_(k)
        n += max(k, 1)
    return n


def test_gate_default_is_a_large_grid_gate(w):
    """the untouched gate is one of the sizes it was measured at or lies between them: no lower than 128³, and the benchmark's 512³ passes it"""
    sg = make(w, DIMS, UBC, 5)
    gate = sg.counter("tailfuse_min")
    print("tailfuse_min default:", gate)
    assert 128 ** 3 <= gate <= 512 ** 3


def test_default_takes_the_path_at_the_gate_and_is_bit_identical(w):
    """untouched "tailfuse", the gate lowered to this shape's own cell count (at the gate counts as above it)"""
    on = make(w, DIMS, UBC, 11, tailfuse_min=cells(DIMS))
    off = make(w, DIMS, UBC, 11, tailfuse=0)
    steps = 0
    for calls in ((0,), (3,), (0, 2)):
        steps += run(on, calls)
        run(off, calls)
        assert_same_state(on, off, calls)       # reads p between the calls
    print("tailfuse counter:", on.counter("tailfuse"), "steps:", steps)
    assert on.counter("tailfuse") == steps
    assert off.counter("tailfuse") == 0


def test_below_the_gate_the_default_keeps_the_separate_tail(w):
    sg = make(w, DIMS, UBC, 11)                                   # untouched: the default gate
    just_above = make(w, DIMS, UBC, 11, tailfuse_min=cells(DIMS) + 1)
    off = make(w, DIMS, UBC, 11, tailfuse=0)
    run(off, (0, 2))
    assert off.counter("tailspec_armed") > 0
    for s in (sg, just_above):
        run(s, (0, 2))
        assert s.counter("tailfuse") == 0
        for c in ("tailspec", "tailspec_armed", "pdefer", "tailwide"):      # what the other tests pin under default options: as with the option off
            assert s.counter(c) == off.counter(c), c
        assert_same_state(s, off, "below the gate")


def test_explicit_option_forces_the_path(w):
    """tailfuse=1 alone (no word about the gate) takes the path at the small shape; tailfuse=0 after it switches it off again; the gate set after an
    explicit 1 applies again"""
    sg = make(w, DIMS, UBC, 13, tailfuse=1)
    assert sg.counter("tailfuse_min") == 0
    run(sg, (0, 2))
    assert sg.counter("tailfuse") == 3
    sg.set_option("tailfuse", 0)
    run(sg, (2,))
    assert sg.counter("tailfuse") == 3
    sg.set_option("tailfuse", 1)
    sg.set_option("tailfuse_min", cells(DIMS) + 1)
    run(sg, (2,))
    assert sg.counter("tailfuse") == 3
    sg.set_option("tailfuse_min", 0)
    run(sg, (2,))
    assert sg.counter("tailfuse") == 5
    ref = make(w, DIMS, UBC, 13, tailfuse=0)
    run(ref, (0, 2, 2, 2, 2))
    assert_same_state(sg, ref, "switched back and forth")


# (dims, z-chunk of the tiled conv_diff! — 0: the tests' default of 5 planes, i.e. several chunks; 32: one chunk that holds both z walls)
SHAPES = [((64, 32, 24), 0), ((128, 48, 16), 0), ((128, 48, 16), 32), ((64, 16, 12), 32), ((64, 32, 8), 32), ((192, 32, 9), 0), ((128, 32, 24), 7)]


@pytest.mark.parametrize("uBC", [UBC, (-0.25, 0.35, -0.15), (1.0, 0.0, 0.0)], ids=["U+-+", "U-+-", "Ux"])
@pytest.mark.parametrize("dims,zc", SHAPES, ids=[f"{d[0]}x{d[1]}x{d[2]}-zc{z}" for d, z in SHAPES])
def test_lean_loader_against_separate_tail(w, dims, zc, uBC):
    """wall tiles and interior tiles (128, 192 wide: the lane move crosses pairs of one row only; the first pair of a row loads), chunk starts, both z walls in
    one chunk, nonzero U on every face; single-step and multi-step calls with p read in between"""
    res = {}
    for fuse in (1, 0):
        sg = make(w, dims, uBC, 17 + dims[2], tailfuse=fuse)
        if zc:
            sg.set_option("convt", zc)
        res[fuse] = sg
    try:
        steps = 0
        for calls in ((0,), (3,), (0, 0), (2,)):
            steps += run(res[1], calls)
            run(res[0], calls)
            assert_same_state(res[1], res[0], (dims, zc, uBC, calls))
        assert res[1].counter("tailfuse") == steps and res[0].counter("tailfuse") == 0
    finally:
        w.lib().wl_reset_process_options()


def test_lean_loader_other_schemes(w):
    """vanLeer and central differences take their own instances of the kernel"""
    for lam in (1, 2):
        on, off = make(w, DIMS, UBC, 23, lam=lam, tailfuse=1), make(w, DIMS, UBC, 23, lam=lam, tailfuse=0)
        for calls in ((0,), (3,)):
            run(on, calls)
            run(off, calls)
            assert_same_state(on, off, (lam, calls))
            x, y = bits(on.field("sigma")), bits(off.field("sigma"))      # the stale Φ in σ's ghost cells: k_conv_q1's instance of this scheme
            assert np.array_equal(x, y), (lam, calls, "sigma", int((x != y).sum()))
        assert on.counter("tailfuse") == 4


def test_sigma_ghost_cells_after_a_step_are_those_of_the_separate_tail(w):
    """the reduced sequence of a mismatch the randomised call-sequence test found (tests/test_gpu_callseq.py, box seed 2: steps(3), metric("ke") into σ): one
    step, then σ read.  σ's upper ghost cells hold conv_diff!'s stale Φ of the corrector's advecting field (quirk Q1), and CFL's maximum(σ) sees them.  With
    the first tail inside the corrector's loader that field is never in memory, and the small launch that leaves the stale Φ (k_conv_q1) read the array — the
    predictor's velocity WITHOUT u −= L∇x and BC!: 4466 of σ's 9192 ghost cells differed at 64×32×24 (u, u⁰, p, pois.n and Δt were equal, the maximum being on
    an interior cell).  Fixed in wl_flow.hip: when the tiled launch took the deferred projection (fold->proj_x), k_conv_q1 forms every operand as the loader of
    wl_convf.hip does — U on wall-normal faces, u − c·(x[c] − x[c−δ]) at the clamped cell elsewhere.  One launch as before."""
    on, off = make(w, DIMS, (0.3, -0.2, 0.1), 211, tailfuse=1), make(w, DIMS, (0.3, -0.2, 0.1), 211, tailfuse=0)
    for s in (on, off):
        s.mom_step_()
    assert on.counter("tailfuse") == 1 and off.counter("tailfuse") == 0
    assert_same_state(on, off, "one step")
    x, y = bits(on.field("sigma")), bits(off.field("sigma"))
    assert np.array_equal(x, y), int((x != y).sum())
