"""Poisoned scratch on the device: a handle whose dead cells and spare buffers hold quiet NaNs, or finite garbage, against a clean twin — bit for bit after every call
(tests/deadstore.py has the dead set, the patterns, poison() and the runner; tests/test_deadstore_cpu.py proves on the oracle that the reference never reads these
cells before it writes them, which is what makes a difference here a device bug).

Every family of tests/callseq.py in both configurations — the default handle with the size gates opened, the eager handle — under both patterns: all of f and of
the spare velocity array, the interior of σ, of every level's r and ϵ and of the coarse levels' z, all of the coarse levels' x, and through wl_sim_scratch_fill the
pressure array that does not hold the pressure, every level's ϵ_mid and r′, the interior of the exchange buffers W, the reduction partials.  The hook's count is
recomputed from the level grids.  One more case per family with set_sgs on and one with a constant forcing (the staged sequence in place of the fused launch).
Caller-owned handles whose f, spare and σ hold the pattern AT CREATION — what the Julia binding's `similar(a.u)` really passes — against the handle-owned
FusedSimulation, with and without the spare, 3-D and 2-D.

σ's LIVE ghost cells against the oracle: a value above maximum(σ) written into a lower-face, a lower edge and a lower corner ghost cell through
set_field("sigma"), in the oracle too: Δt after each of three steps and after mom_steps_(3) is the oracle's, as raw bits — inv(v + 5ν), no reduction order in it —
and the three cells keep the value: every CFL route of tests/test_gpu_cfl_routes.py at handle level, with a σ the library did not write itself."""
import numpy as np
import pytest

import callseq as cs
import deadstore as ds

pytestmark = pytest.mark.gpu

f32 = np.float32
CONFIGS = ("default", "eager")


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    yield w
    w.lib().wl_reset_process_options()      # resjac_min / convt_min / body_tile are process-wide


def twins(w, family, config, setup=None):
    """two handles of one kind and one configuration: (clean, poisoned)"""
    out = []
    for _ in range(2):
        dev = cs.make_one(family, w, config == "eager", caller_eager=True)
        if setup:
            setup(dev)
        out.append(ds.DevTwin(w, dev))
    return out


def close(family, *ts):
    if family == "caller":
        for t in ts:
            t.dev.close()


def run_pair(w, family, config, pattern, setup=None):
    clean, dirty = twins(w, family, config, setup)
    try:
        wrote = ds.run(clean, dirty, pattern, family)
        # the hook reported what the level grids say it has to write, on both twins, at every poisoning — an omitted region would show
        want = dirty.scratch_words(perdir=family == "periodic")
        assert [x[("scratch", None)] for x in wrote] == [want] * len(wrote) and clean.last_scratch == want, (wrote[0][("scratch", None)], want)
        assert all(("us", None) in x and ("f", None) in x and ("x", 1) in x for x in wrote)
        return clean, dirty, wrote
    finally:
        close(family, clean, dirty)


@pytest.mark.parametrize("pattern", ds.PATTERNS)
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("family", cs.FAMILIES)
def test_poisoned_twin_equals_clean_twin(w, family, config, pattern):
    clean, dirty, wrote = run_pair(w, family, config, pattern)
    live = ("pdefer", "bcdefer", "rskip", "tailspec", "tailfuse", "hybrid", "abwide")
    a, b = {k: clean.dev.counter(k) for k in live}, {k: dirty.dev.counter(k) for k in live}
    print(f"[deadstore] {family} {config} {pattern}: {sum(wrote[0].values())} words per poisoning, {wrote[0][('scratch', None)]} of them through the hook; paths {b}")
    assert a == b      # the same paths ran on both twins
    if config == "eager":
        assert all(b[k] == 0 for k in ("pdefer", "bcdefer", "rskip", "tailspec", "tailfuse", "hybrid")), b
    elif family in ("box", "ragged", "caller"):      # the deferrals the poisoned arrays sit behind really ran
        assert all(b[k] > 0 for k in ("pdefer", "bcdefer", "rskip", "tailspec", "abwide")), b
    elif family == "moving":
        assert b["hybrid"] > 0, b


SGS = [f for f in cs.FAMILIES if f != "circle2d"]      # the model is built for 3-D flows


@pytest.mark.parametrize("pattern", ds.PATTERNS)
@pytest.mark.parametrize("family", SGS)
def test_poisoned_twin_with_the_sgs_model_on(w, family, pattern):
    """the staged sequence conv_diff! → sgs! → BDIM!: f and σ are read and written by launches of their own"""
    run_pair(w, family, "default", pattern, lambda dev: dev.set_sgs(1))


@pytest.mark.parametrize("pattern", ds.PATTERNS)
@pytest.mark.parametrize("family", cs.FAMILIES)
def test_poisoned_twin_with_a_constant_forcing(w, family, pattern):
    """accelerate!(f, …) adds to every cell of f between conv_diff! and BDIM!"""
    D = 2 if family == "circle2d" else 3
    run_pair(w, family, "default", pattern, lambda dev: dev.set_forcing(cs.ACC[:D]))


@pytest.mark.parametrize("pattern", ds.PATTERNS)
@pytest.mark.parametrize("with_spare", [True, False])
@pytest.mark.parametrize("dims", [(64, 32, 24), (48, 40)], ids=["64x32x24", "48x40"])
def test_caller_owned_arrays_that_start_as_garbage(w, dims, with_spare, pattern):
    """what the Julia binding passes: f, σ and the spare are `similar` arrays — against the handle-owned flow, as tests/test_gpu_callerowned.py compares zeros"""
    from test_gpu_callerowned import CallerOwnedSim
    D = len(dims)
    Ng = tuple(n + 2 for n in dims)
    uBC = (1.0,) + (0.0,) * (D - 1)
    u_init = np.asfortranarray(np.random.default_rng(5).uniform(-0.3, 0.3, size=Ng + (D,)).astype(f32))
    u_init[..., 0] += 1.0
    ref = w.FusedSimulation(dims, uBC, dims[0], U=1, nu=0.02, u0=u_init)
    sim = CallerOwnedSim(w, dims, uBC, 0.02, u_init, with_spare, fill=pattern)
    try:
        for k in ("f", "us", "sigma"):      # the fill is there
            if k in sim.arr:
                a = w.to_host(sim.arr[k])
                want = ds.values(pattern, a.shape, (k, "create"))
                m = ~ds.ghost_mask(a.shape) if k == "sigma" else np.ones(a.shape, dtype=bool)
                assert np.array_equal(cs.bits(a)[m], cs.bits(want)[m]) and (k != "sigma" or not a[~m].any()), k
        for k, v in cs.GATES.items():      # the fused head and the tiled conv_diff! at this size, on both
            ref.set_option(k, v)
            sim.check(sim.lib.wl_sim_set_option(sim.h, k.encode(), v))
        moved = False
        for step in range(3):
            ref.mom_step_(); sim.mom_step()
            for name in ("u", "u0", "p"):
                a, b = sim.field(name), ref.field(name)
                assert np.isfinite(a).all(), (step, name, int((~np.isfinite(a)).sum()))
                assert np.array_equal(cs.bits(a), cs.bits(b)), (step, name, int((cs.bits(a) != cs.bits(b)).sum()))
            assert [cs.bits(v).item() for v in sim.dt] == [cs.bits(v).item() for v in ref.dt], step
            g = ds.ghost_mask(Ng)
            assert np.array_equal(cs.bits(sim.field("sigma"))[g], cs.bits(ref.field("sigma"))[g]), step
            moved = moved or sim.role["u"] != "u"
        assert sim.pois_n() == ref.pois_n
        if with_spare and D == 3:
            assert moved                       # the fused out-of-place kernels ran: the roles of the three buffers rotated
    finally:
        sim.close()


# ------------------------------------------------------------------------------------------------------------- σ's live ghost cells
LIVE_CASES = [("box", "default"), ("box", "eager"), ("ragged", "default"), ("exit", "default"), ("circle2d", "default")]


@pytest.mark.parametrize("family,config", LIVE_CASES, ids=[f"{f}-{c}" for f, c in LIVE_CASES])
def test_sigma_ghost_cells_written_from_outside_decide_dt_as_in_the_oracle(w, oracle, family, config):
    dev = ds.DevTwin(w, cs.make_one(family, w, config == "eager"))
    orc = ds.oracle_twin(oracle, family, full=True)
    for name in ("u", "u0"):      # the same flow, bit for bit, from the first step on
        orc.so.field(name)[...] = dev.field(name)
    cells = ds.plant(dev)
    assert ds.plant(orc) == cells and dev.field("sigma").shape == orc.field("sigma").shape
    want = cs.bits(ds.dt_planted(orc.so.nu)).item()
    for step in range(3):
        dev.mom_step_(); orc.mom_step_()
        print(f"{family} {config} step {step}: Δt {float(dev.dt[-1]):.9e}, oracle {float(orc.dt[-1]):.9e}")
        assert cs.bits(dev.dt[-1]).item() == cs.bits(orc.dt[-1]).item() == want, (step, float(dev.dt[-1]), float(orc.dt[-1]))
    dev.mom_steps_(3); orc.mom_steps_(3)
    assert len(dev.dt) == len(orc.dt) == 7
    assert [cs.bits(v).item() for v in dev.dt[1:]] == [cs.bits(v).item() for v in orc.dt[1:]] == [want] * 6, ([float(v) for v in dev.dt], [float(v) for v in orc.dt])
    s, so = dev.field("sigma"), orc.field("sigma")
    assert all(s[c] == ds.SIGMA_VALUE and so[c] == ds.SIGMA_VALUE for c in cells), [(float(s[c]), float(so[c])) for c in cells]
    so[tuple(np.array(cells).T)] = 0
    assert float(so.max()) < float(ds.SIGMA_VALUE) / 2      # the planted value was the maximum all along
    assert np.abs(dev.field("u") - orc.field("u")).max() < 1e-3      # (and it is the same flow: the comparison of bits is other tests' business)
