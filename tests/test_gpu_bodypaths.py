"""The four body-aware shortcuts (farmask, hybrid, body_tile, zsplit) on the geometries they were not built on: a handle with the shortcuts
live against a handle on the general kernels, u, u⁰, p on every cell (ghosts included) as raw bits, pois.n and the Δt history; the
library's path counters say which path ran (and that it stood down where it has to); the mask census the library took at its last refresh
equals the NumPy restatement (tests/bodypaths_ref.py) on the fields read back.  tests/test_bodypaths_cpu.py shows without a GPU that every
geometry holds the mask class it is here for.  The general path itself is tied to the oracle on the geometries that had no such comparison."""
import numpy as np
import pytest

import bodypaths_ref as bp

pytestmark = pytest.mark.gpu

f32 = np.float32
NU = 0.02
PLAIN = {"zsplit": 0, "farmask": 0, "hybrid": 0, "body_tile": 0, "constl": 0}      # the general kernels everywhere
FAST = {"convt_min": 0, "zsplit": 2}                                                # no size gates: the shortcuts at these small shapes


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    yield w
    w.lib().wl_reset_process_options()      # convt_min / body_tile are process-wide


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def u_init(dims, seed=11):
    return np.asfortranarray(np.random.default_rng(seed).uniform(-0.4, 0.4, size=tuple(n + 2 for n in dims) + (len(dims),)).astype(f32))


def handle(w, case, opts, has_body=True):
    """the initial u is a seeded random field (BC! applied by the constructor): cells far from the body carry content"""
    D = len(case["dims"])
    sim = w.FusedSimulation(case["dims"], (1.0,) + (0.0,) * (D - 1), 8.0, U=1, nu=NU, perdir=case["perdir"], exitBC=case["exitBC"], lam=case["lam"],
                            has_body=has_body, u0=u_init(case["dims"]))
    for k, v in opts.items():
        sim.set_option(k, v)
    if case["store_f"]:
        sim.set_option("store_f", 1)
    return sim


def step(sim, fast, n=1, convt_min=None, one_call=False):
    """n × mom_step!; "body_tile" is a process-wide switch, so it is set for the handle that is about to run (and so is "convt_min", where the caller runs
    handles with different size gates side by side); one_call: the n steps as one wl_sim_mom_steps"""
    sim.set_option("body_tile", 1 if fast else 0)
    if convt_min is not None:
        sim.set_option("convt_min", convt_min)
    if one_call:
        sim.mom_steps_(n)
        return
    for _ in range(n):
        sim.mom_step_()


def measure(sim, body):
    if body is None:
        sim.update_()                        # a flow with a body that was never measured: update! alone refreshes the masks
    elif bp.is_set(body):
        sim.measure_bodyset_(bp.to_body(body), 1.0)
    else:
        sim.measure_body_(body, 1.0)


def assert_same_state(a, b, what, names=("u", "u0", "p")):
    for name in names:
        x, y = bits(a.field(name)), bits(b.field(name))
        assert np.array_equal(x, y), (what, name, int((x != y).sum()), np.argwhere(x != y)[:4].tolist())
    assert a.pois_n == b.pois_n, (what, a.pois_n, b.pois_n)
    da, db = [int(f32(v).view(np.uint32)) for v in a.dt], [int(f32(v).view(np.uint32)) for v in b.dt]
    assert da == db, (what, [float(v) for v in a.dt], [float(v) for v in b.dt])


def steps_of(case, q):
    """(body, steps) per measure! of position q: two steps per position; a moving body is measured again before each of four steps"""
    body = case["positions"][q][0]
    if case["remeasure_each_step"]:
        return [(body, 1)] * (4 if q == 0 else 2)
    return [(body, 2)]


CONVT_MIN_DEFAULT = 2048      # wl_sim_create's conv_tile_min


def run_position(w, case, q, fast, plain, default=None, each_call=False, steps3=False, check=None):
    """measure! + steps on both handles; on the fast handle the counters around the steps and the census against the restatement.
    default: a third handle with nothing set, held to plain as well (no tiled far range and no split level under its size gates, hybrid all the same);
    each_call: one call per step with the states compared after every call instead of after the position; steps3: one wl_sim_mom_steps(3) on top;
    check(what, fast, default, ref, fields, tr, kinds, n): the caller's own assertions in place of bp.CONDS (tests/test_gpu_bodyshapes.py)"""
    Ng = tuple(n + 2 for n in case["dims"])
    what = (case["id"], q)
    names = ("u", "u0", "p", "f") if case["store_f"] else ("u", "u0", "p")
    for body, n in steps_of(case, q):
        if case["remeasure_each_step"] and body is not None:
            body = bp.moving_position(body, float(np.sum(fast.dt[:-1], dtype=np.float64)))
        calls = ([(1, False)] * n if each_call else [(n, False)]) + ([(3, True)] if steps3 else [])
        n = sum(k for k, _ in calls)
        measure(plain, body)
        if not each_call:
            step(plain, False, n)
        measure(fast, body)
        assert fast.counter("mask_valid") == 1, what
        dev = {k: fast.counter(k) for k in bp.CENSUS_NAMES}
        kinds, part = fast.smoother_kinds(), fast.counter("part")
        if default is not None:
            measure(default, body)
            assert {k: default.counter(k) for k in bp.CENSUS_NAMES} == dev and default.counter("part") == 0, what
            hd = default.counter("hybrid")
        dh = dt_ = 0
        for i, (k, one) in enumerate(calls):
            if each_call:
                step(plain, False, k, one_call=one)
            h0, t0 = fast.counter("hybrid"), fast.counter("body_tile")
            step(fast, True, k, convt_min=0 if default is not None else None, one_call=one)
            dh, dt_ = dh + fast.counter("hybrid") - h0, dt_ + fast.counter("body_tile") - t0
            if default is not None:
                t0 = default.counter("body_tile")
                step(default, True, k, convt_min=CONVT_MIN_DEFAULT, one_call=one)
                assert default.counter("body_tile") == t0, (what, i)
            if each_call:
                assert_same_state(fast, plain, what + ("call", i), names)
                if default is not None:
                    assert_same_state(default, plain, what + ("default", "call", i), names)
        # (read after the steps: handing out V or μ₁ invalidates the masks until the next measure!/update!)
        mu0, mu1, V = fast.field("mu0"), fast.field("mu1"), fast.field("V")
        assert fast.counter("mask_valid") == 0, what
        ref = bp.census_plus(mu0, mu1, V)
        print(case["id"], q, "census", [dev[k] for k in bp.CENSUS_NAMES], "hybrid +%d" % dh, "body_tile +%d" % dt_, "kinds", kinds, "part", part,
              (fast.counter("part_za"), fast.counter("part_zb")))
        assert dev == {k: ref[k] for k in bp.CENSUS_NAMES}, (what, dev, ref)
        tr = bp.tile_ranges(ref, Ng, case["perdir"], case["store_f"])
        zp = bp.zsplit_plan(mu0, case["perdir"])
        if check is not None:
            check(what, fast, default, ref, (mu0, mu1, V), tr, kinds, n)
        else:
            for name in case["positions"][q][1]:                    # the class this geometry is here for, on the device's own fields
                assert bp.CONDS[name](ref, Ng, tr, zp), (what, name, ref, tr, zp)
        assert dh == (0 if case["exitBC"] else 2 * n), (what, dh)              # the convective exit: hybrid stands down, farmask stays
        assert dt_ == (0 if case["exitBC"] else tr[2] * 2 * n), (what, dt_, tr)
        assert part == int(zp[0]) and (kinds[0] == 3) == zp[0], (what, kinds, part, zp)
        if zp[0]:
            assert (fast.counter("part_za"), fast.counter("part_zb")) == zp[1:], (what, zp)
        assert plain.counter("hybrid") == 0 and plain.smoother_kinds()[0] != 3, what
        if default is not None:
            assert default.counter("hybrid") - hd == (0 if case["exitBC"] else 2 * n) and 3 not in default.smoother_kinds(), what
    assert_same_state(fast, plain, what, names)
    if default is not None:
        assert_same_state(default, plain, what + ("default",), names)
    return ref


@pytest.mark.parametrize("case", bp.CASES, ids=[c["id"] for c in bp.CASES])
def test_fast_paths_give_the_bits_of_the_general_kernels(w, case):
    """see the module docstring; the per-case classes are listed in tests/bodypaths_ref.py CASES"""
    fast, plain = handle(w, case, FAST), handle(w, case, PLAIN)
    for q in range(len(case["positions"])):
        run_position(w, case, q, fast, plain)
    assert np.isfinite(fast.field("u")).all(), case["id"]


@pytest.mark.parametrize("variant", ["unmeasured", "outside"])
def test_empty_masks_give_the_bits_of_a_flow_without_a_body(w, variant):
    """has_body with nothing on the grid — never measured, or a sphere centred far outside: empty near_box, unknown dirty_z from the first step on,
    bdim_near launches nothing.  Far from a body BDIM! degenerates to the NoBody form, so u, u⁰ and p equal those of a has_body=False handle
    bit for bit — through whole steps: the projection's kernels differ between the two handles (no pdefer, bcdefer or fused head decisions
    are shared) but every one of them is held to the bits of the same general kernels."""
    case = next(c for c in bp.CASES if c["id"] == "empty-" + variant)
    fast, nobody = handle(w, case, FAST), handle(w, case, {"convt_min": 0}, has_body=False)
    measure(fast, case["positions"][0][0])
    assert (fast.counter("mask_near"), fast.counter("near_k0"), fast.counter("near_k1"), fast.counter("dirty_z0"), fast.counter("dirty_z1")) == (0, 50, -1, 50, -1)
    l0 = w.lib().wl_launch_count(); step(fast, True); lf = w.lib().wl_launch_count() - l0
    step(fast, True, 2); step(nobody, True, 3)
    assert fast.counter("hybrid") == 6
    assert_same_state(fast, nobody, variant)
    # (printed for the record: a step on empty masks against the same step with a sphere on the grid, whose bdim_near and tiled far ranges launch)
    one = handle(w, case, FAST)
    measure(one, bp.sphere((20, 16, 24)))
    l0 = w.lib().wl_launch_count(); step(one, True); l1 = w.lib().wl_launch_count() - l0
    print("launches per step: empty masks", lf, "sphere", l1)
    assert lf < l1


def test_mask_invalidation_contract(w):
    """wl_sim_field("V" | "mu0" | "mu1") clears mask_valid until the next update!: the steps in between take the general path (hybrid does not
    rise) and still match; update!() brings the fast path back; after set_field("mu1", …) of another body + update!() the masks follow the
    new fields (census = restatement) and the bits still match."""
    case = next(c for c in bp.CASES if c["id"] == "twins")
    fast, plain = handle(w, case, FAST), handle(w, case, PLAIN)
    body = case["positions"][0][0]
    for s in (fast, plain):
        measure(s, body); step(s, s is fast, 2)
    assert fast.counter("hybrid") == 4 and fast.counter("mask_valid") == 1
    fast.field("V"); plain.field("V")
    assert fast.counter("mask_valid") == 0
    t0 = fast.counter("body_tile")
    for s in (fast, plain):
        step(s, s is fast, 2)
    assert fast.counter("hybrid") == 4 and fast.counter("body_tile") == t0
    assert_same_state(fast, plain, "invalidated")
    for s in (fast, plain):
        s.update_()
    assert fast.counter("mask_valid") == 1
    for s in (fast, plain):
        step(s, s is fast)
    assert fast.counter("hybrid") == 6 and fast.counter("body_tile") > t0
    assert_same_state(fast, plain, "after update!")
    # the fields of a different body written from outside (a third handle measures it), then update!()
    other = handle(w, case, PLAIN)
    measure(other, case["positions"][1][0])
    new = {k: other.field(k) for k in ("mu0", "mu1", "V")}
    before = {k: fast.counter(k) for k in bp.CENSUS_NAMES}
    for s in (fast, plain):
        for k in ("mu0", "mu1", "V"):
            s.set_field(k, new[k])
        assert s.counter("mask_valid") == 0
        s.update_()
    after = {k: fast.counter(k) for k in bp.CENSUS_NAMES}
    ref = bp.census(new["mu0"], new["mu1"], new["V"])
    assert after == {k: ref[k] for k in bp.CENSUS_NAMES} and after != before, (before, after, ref)
    for s in (fast, plain):
        step(s, s is fast, 2)
    assert fast.counter("hybrid") == 10
    assert_same_state(fast, plain, "after set_field + update!")


ORACLE_CASES = ["deepfloor", "zslab", "zcyl", "moving"]


@pytest.mark.parametrize("cid", ORACLE_CASES)
def test_general_path_on_these_geometries_matches_the_oracle(w, oracle, cid):
    """the plain handle, three steps from the uniform inflow against oracle.Simulation with the oracle's coefficient fields copied in, as in
    test_closed_form_bodies_measure_steps_and_forces and with that test's bounds (equal pois.n, |Δu| < 5e-5).  Since fast = plain in bits
    above, this ties the shortcuts to the reference as well.  The moving sphere is measured again before every step."""
    case = next(c for c in bp.CASES if c["id"] == cid)
    dims, body = case["dims"], case["positions"][0][0]
    so = oracle.Simulation(dims, (1, 0, 0), 8.0, U=1, nu=NU, body=body, T=f32)
    sg = w.FusedSimulation(dims, (1, 0, 0), 8.0, U=1, nu=NU, has_body=True)
    for k, v in PLAIN.items():
        sg.set_option(k, v)
    for step in range(3):
        if case["remeasure_each_step"]:
            so.set_body(bp.moving_position(body, float(np.sum(so.dt[:-1])))); so.measure()
        if step == 0 or case["remeasure_each_step"]:
            for k in ("mu0", "mu1", "V"):
                sg.set_field(k, so.field(k))
            sg.update_()
        so.step(remeasure=False); sg.mom_step_()
        du = float(np.abs(sg.field("u") - so.u).max())
        print(cid, step, "pois_n", sg.pois_n, so.pois_n, "max|du| %.3g" % du)
        assert sg.pois_n == so.pois_n, step
        assert du < 5e-5, step
