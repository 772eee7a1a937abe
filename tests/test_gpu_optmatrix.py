"""Every pair of implementation switches (every triple of the 13 step-level ones) against the PLAIN handle, bit for bit: tests/optmatrix.py draws the rows,
tests/test_optmatrix_cpu.py shows that they cover what they claim.  A row is a fresh handle with the row's switches set that makes two wl_sim_mom_step calls and
one wl_sim_mom_steps(3); after each call u, u⁰, p on every cell (ghosts included) as raw bits, pois.n and the Δt history equal those of the handle with every
switch at its un-fused, un-deferred value, no call returns an error, and the path counters agree with what the header says runs under the row.  The walk changes
many switches at once on a handle that carries state; the PLAIN handle itself is tied to the oracle."""
import numpy as np
import pytest

import callseq
import optmatrix as om

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    yield w
    w.lib().wl_reset_process_options()


def plain_row(family):
    return {n: om.PLAIN[n] for n in om.names(family)}


def plain_run(w, family, calls=om.CALLS):
    """the PLAIN handle, while the process-wide switches are at their plain values (om.apply sets them with the rest)"""
    w.lib().wl_reset_process_options()
    ref, cnt, err = om.run(family, w, plain_row(family), calls)
    assert err is None, (family, "PLAIN", err)
    assert all(cnt[a] <= 0 for a in om.COUNTED), (family, "a counted path ran on the PLAIN handle", cnt)
    assert all(np.isfinite(s.field("u")).all() and np.isfinite(s.field("p")).all() for s in ref), family
    return ref


def check_rows(w, family, rws, what):
    ref = plain_run(w, family)
    for i, row in enumerate(rws):
        w.lib().wl_reset_process_options()
        snaps, cnt, err = om.run(family, w, row)
        where = "%s %s row %d %r" % (family, what, i, row)
        assert err is None, "%s: a call returned an error: %s" % (where, err)
        d = om.first_diff(snaps, ref)
        assert d is None, "%s: after call %d %s differs from PLAIN in %s cells, first %s\n%s" % ((where,) + d[:4] + (om.shrink_hint(family, row),))
        faults = om.counter_faults(row, family, cnt)
        assert not faults, "%s: %s; counters %r" % (where, "; ".join(faults), cnt)


@pytest.mark.parametrize("family", list(om.FAMILIES))
def test_rows_equal_plain(w, family):
    check_rows(w, family, om.pair_rows(family), "pair")


def test_triples_equal_plain(w):
    """every triple of values of the 13 step-level switches, all other switches at their defaults, on the whole-tile box"""
    check_rows(w, "box", om.triple_rows(), "triple")


@pytest.mark.parametrize("family", ["box", "ragged", "moving"])
def test_walk_through_rows(w, family):
    """one live handle walks through the pair rows — the row applied between two calls, then wl_sim_mom_steps(2) — against the PLAIN trajectory of the same steps:
    the switches keep their contract on a handle that carries a pressure left in the other array, a remembered stopping iteration, masks and buffers in rotation"""
    rws = om.pair_rows(family)
    calls = (("mom_steps_", 2),) * len(rws)
    ref = plain_run(w, family, calls)
    w.lib().wl_reset_process_options()
    h = om.make(family, w, rws[0])
    for i, row in enumerate(rws):
        where = "%s walk: row %d %r after row %r" % (family, i, row, rws[i - 1] if i else None)
        try:
            om.apply(h, row)
            om.call(h, calls[i])
        except Exception as e:
            raise AssertionError("%s: a call returned an error: %s" % (where, e))
        d = callseq.state_diff(om.Snap(h), ref[i])
        assert d is None, "%s: %s differs from PLAIN in %s cells, first %s" % ((where,) + d[:3])


def test_plain_is_the_oracle(w, oracle):
    """every combination = PLAIN (above); PLAIN = the oracle, here: the ragged TGV box, three steps from the device's own initial u, with the bounds
    tests/test_gpu_solver.py::test_tgv_steps_match_oracle applies to the same quantities on a TGV at this scale"""
    family = "ragged"
    dims = callseq.DIMS[family]
    w.lib().wl_reset_process_options()
    sg = om.make(family, w, plain_row(family))
    u_init = sg.field("u")
    so = oracle.Simulation(dims, (0, 0, 0), dims[0], U=1, nu=dims[0] / 1600.0, T=f32)
    so.field("u")[...] = u_init
    so.field("u0")[...] = u_init
    for step in range(3):
        so.step(remeasure=False)
        sg.mom_step_()
        du, dp = float(np.abs(sg.field("u") - so.u).max()), float(np.abs(sg.field("p") - so.p).max())
        print("step", step, "pois_n", sg.pois_n, so.pois_n, "max|du| %.3g max|dp| %.3g" % (du, dp))
        assert list(sg.pois_n) == list(so.pois_n), step
        assert np.allclose(np.array(sg.dt, dtype=np.float64), np.array(so.dt), rtol=1e-6), step
        assert du < 2e-5, (step, du)
        assert dp < 2e-4, (step, dp)
