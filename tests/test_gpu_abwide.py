"""Smoother kernel A hands r′ and ϵ_mid to kernel B through the level's exchange buffer W (csrc/wl_abwide.hpp; the WIDE forms of k_gsrb2_A / k_gsrb2_B in
csrc/wl_fused2_body.inc; wl_mg::plan_smooth decides).  The statements per cell are those of the dense two-array exchange, so a handle with "xdefer" = 1 (wide
where eligible) against a handle with "xdefer" = 2 (deferred x, dense exchange) on the same library must agree on u, u⁰, p on every cell as raw bits, on pois.n
and on the Δt history, with the same number of launches per call; the finest residual read back through wl_mg_level_field must agree too, also where the r-only
instance of kernel B produces it from W.  The counter "abwide" (finest-level smooth! calls that went through W) is checked against the plan's rule restated
here: every V-cycle iteration of a solve ends in one smooth!(0) with a pending prolongation, which is the one launch that is eligible.

Shapes (with ghosts) and the call plan are those of tests/test_gpu_rskip.py: 66×34×26 (16-row instances, level 1 off the pair kernels), 66×66×18 (levels 0 and 1
on them), 450×370×10 (135 tiles: the 32-row instances), plus 62×34×12, where the last segment of a row of W holds a single pair."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_rskip as rk
from test_gpu_rskip import SMALL, TWO, WIDE, bits, assert_same_state, random_u, policy

pytestmark = pytest.mark.gpu

ONEPAIR = (60, 32, 10)      # nx = 62: pairs i0 = 0..60, the pair at i0 = 60 alone in segment 1


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    yield w
    w.lib().wl_reset_process_options()


def make_pair(w, oracle, dims, field, **opts):
    u0 = None if field == "tgv" else random_u(oracle, dims, 71)
    return rk.make(w, dims, u0, xdefer=1, **opts), rk.make(w, dims, u0, xdefer=2, **opts)


def run_pair(w, wide, dense, calls, what, exact=True):
    """the same calls on both handles: state as raw bits after each, equal launches; "abwide" rises by the V-cycle iterations of the call's solves on the wide handle
    (exact: no solve was discarded, so pois.n lists them all) and stays 0 on the dense one"""
    for q, k in enumerate(calls):
        res = []
        for s in (wide, dense):
            l0, c0, n0, d0 = w.lib().wl_launch_count(), s.counter("abwide"), len(s.pois_n), s.counter("resjac_redo")
            if k == 0:
                s.mom_step_()
            else:
                s.mom_steps_(k)
            res.append((w.lib().wl_launch_count() - l0, s.counter("abwide") - c0, sum(s.pois_n[n0:]), s.counter("resjac_redo") - d0))
        (lw, cw, itw, dw), (ld, cd, itd, dd) = res
        print(f"{what} call {q} k={k}: abwide +{cw} (dense: +{cd}), V-cycle iterations {itw}, discarded solves {dw}, launches {lw} vs {ld}")
        assert cd == 0, (what, q, cd)
        assert lw == ld, (what, q, "launches", lw, ld)
        assert (itw, dw) == (itd, dd), (what, q)
        if exact and dw == 0:
            assert cw == itw, (what, q, cw, itw)
        else:
            assert cw >= itw, (what, q, cw, itw)      # (a discarded solve smooths too)
        assert_same_state(wide, dense, (what, q, k))
    assert wide.counter("xdefer") == 1 and dense.counter("xdefer") == 1, what
    assert dense.counter("abwide") == 0 and wide.counter("abwide") > 0, what


def read_r_equal(wide, dense, what):
    a, b = bits(wide.pois_level("r")), bits(dense.pois_level("r"))
    assert np.array_equal(a, b), (what, "r", int((a != b).sum()))


@pytest.mark.parametrize("field", ["tgv", "random"])
@pytest.mark.parametrize("dims", [SMALL, TWO, WIDE, ONEPAIR], ids=["66x34x26", "66x66x18", "450x370x10", "62x34x12"])
def test_wide_exchange_is_bit_identical(w, oracle, dims, field):
    wide, dense = make_pair(w, oracle, dims, field)
    what = f"{'x'.join(map(str, dims))}-{field}"
    run_pair(w, wide, dense, rk.CALLS, what)
    kinds = wide.smoother_kinds()
    assert kinds[0] == 2, kinds
    if dims == SMALL:
        assert kinds[1] != 2, kinds
    if dims == TWO:
        assert kinds[1] == 2, kinds
    read_r_equal(wide, dense, what)


MODES = {
    "rskip0": {"rskip": 0},              # kernel B's both-outputs instance reads W
    "tailspec0": {"tailspec": 0},
    "headspec0": {"headspec": 0},
    "redo": {"resjac": 2},               # every speculative solve discarded after its first iteration
    "tailfuse1": {"tailfuse": 1},
    "pdefer0": {"pdefer": 0},
    "itmx2": {"itmx": 2},                # solves stop at the cap: stores skipped where the loop goes on or ends unconverged — the r-only instance reads W
}


@pytest.mark.parametrize("mode", list(MODES))
def test_wide_exchange_with_the_other_switches_moved(w, oracle, mode):
    wide, dense = make_pair(w, oracle, TWO, "random", **MODES[mode])
    run_pair(w, wide, dense, rk.CALLS, mode, exact=mode != "redo")
    read_r_equal(wide, dense, mode)
    if mode == "rskip0":
        assert wide.counter("rskip") == 0
    if mode == "itmx2":
        assert max(wide.pois_n) == 2 and wide.counter("rskip_redo") > 0, (wide.pois_n, wide.counter("rskip_redo"))
        assert wide.counter("rskip_redo") == dense.counter("rskip_redo")


def test_residual_after_a_skipped_store_comes_from_the_exchange_buffer(w, oracle):
    """steps until a call ends on a skipped store (the rule of tests/test_gpu_rskip.py): the read of the finest r launches the r-only instance once on either
    handle — on the wide one it reads W — and the two residuals are the same bits; so are the steps after it"""
    wide, dense = make_pair(w, oracle, SMALL, "random", rskip=1)
    for _ in range(6):
        for s in (wide, dense):
            s.mom_step_()
        if policy(wide.pois_n)[2]:
            break
    assert policy(wide.pois_n)[2] and wide.pois_n == dense.pois_n, wide.pois_n
    assert wide.counter("abwide") > 0 and dense.counter("abwide") == 0
    r0 = (wide.counter("rskip_redo"), dense.counter("rskip_redo"))
    read_r_equal(wide, dense, "stale r")
    assert (wide.counter("rskip_redo"), dense.counter("rskip_redo")) == (r0[0] + 1, r0[1] + 1)
    # the format of the launch that skipped the store is remembered: the switch moved in between does not change where the late store reads
    for _ in range(8):
        for s in (wide, dense):
            s.mom_step_()
        if policy(wide.pois_n)[2]:
            break
    assert policy(wide.pois_n)[2], wide.pois_n
    wide.set_option("xdefer", 2)
    read_r_equal(wide, dense, "stale r, switch moved")
    for s in (wide, dense):
        s.mom_step_()
    assert_same_state(wide, dense, "after the switch")


def test_counter_stays_zero_where_the_plan_says_dense(w, oracle):
    lib, st, check = w.lib(), w.core.stream(), w._lib.check
    # a periodic direction: passes, no pair kernels
    per = w.FusedSimulation(TWO, (0.0,) * 3, TWO[0], U=1, nu=TWO[0] / 1600.0, perdir=(1,), ic="tgv")
    per.mom_steps_(2)
    assert per.counter("abwide") == 0 and sum(per.pois_n) > 0
    # the z-split: coefficients off the constant pattern on two middle planes
    import test_gpu_mg_paths as mp
    zs = mp._zsplit_sim(w)
    assert zs.smoother_kinds()[0] == 3
    zs.mom_steps_(2)
    assert zs.counter("abwide") == 0 and sum(zs.pois_n) > 0
    # a bare smooth! (no pending prolongation) and a bare Vcycle! (its prolongation is not deferred) on an eligible handle; a solve on the same handle counts
    sim = rk.make(w, TWO, random_u(oracle, TWO, 71))
    mg = lib.wl_sim_pois(sim._h)
    check(lib.wl_mg_smooth(mg, 0, 4, 1.0, st))
    check(lib.wl_mg_vcycle(mg, 0, 1.0, st))
    check(lib.wl_stream_sync(st))
    assert sim.counter("abwide") == 0
    sim.mom_step_()
    assert sim.counter("abwide") >= sum(sim.pois_n) > 0
    # "xdefer" = 0: kernel A applies the x increment itself — the wide form has no x stage
    off = rk.make(w, TWO, random_u(oracle, TWO, 71), xdefer=0)
    off.mom_step_()
    assert off.counter("abwide") == 0 and off.counter("xdefer") == 0
