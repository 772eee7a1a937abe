"""The body-aware shortcuts on both sides of the gates a grid shape moves (tests/bodyshapes.py SHAPE_CASES): per case a handle with the shortcuts and no size
gates, a handle with nothing set and a handle on the general kernels; u, u⁰, p (f with store_f) on every cell, ghosts included, as raw bits after EVERY call,
pois.n and the Δt history; on the first handle the mask census against the restatement on the fields read back, the hybrid and body_tile counters,
wl_mg_smoother_kind of EVERY level against bodyshapes.smoother_kind_level on the level's own L (3 exactly where zsplit_plan_level splits it), part/part_za/part_zb,
and every class the position claims, on the device's own fields.  tests/test_bodyshapes_cpu.py shows without a GPU that the two sides of each gate differ.
The general path is tied to the oracle on every case of at most bodyshapes.ORACLE_CELLS array cells (all but bodyshapes.PLAIN_ONLY)."""
import numpy as np
import pytest

import bodypaths_ref as bp
import bodyshapes as bs
from test_gpu_bodypaths import FAST, NU, PLAIN, handle, run_position, w  # noqa: F401  (w: the module-scoped fixture)

pytestmark = pytest.mark.gpu

f32 = np.float32
DEFAULT = {}      # nothing set: convt_min = 2048 and the 16 M-cell gate of the z-split keep body_tile and part at 0 at these sizes; hybrid and farmask run


def checker(case, q):
    conds = case["positions"][q][1]

    def check(what, fast, default, ref, fields, tr, kinds, n):
        mu0, mu1, V = fields
        Ng = tuple(mu0.shape[:-1])
        Ls = [fast.pois_level("L", l) for l in range(fast.nlevels())]
        assert np.array_equal(Ls[0], mu0), what                                   # level 0's L is μ₀ itself
        e = bs.evaluate(case, mu0, mu1, V, Ls)
        assert kinds == e["kinds"], (what, kinds, e["kinds"], [tuple(p) for p in e["plans"]])      # every level; 3 exactly where the restated plan splits it
        assert [k == 3 for k in kinds] == [p.part for p in e["plans"]], what
        for name in conds:                                                         # every claimed class, on the device's own fields
            assert bs.cond(name)(e["c"], Ng, tr, e["plans"]), (what, name, e["c"], tr, e["plans"][:2])
        if default is not None:      # under the default size gates no level is split; the constant levels still take the pair kernels
            want = [bs.smoother_kind_level(L, L.shape[:-1], case["perdir"], True, bs.ZSPLIT_MIN_DEFAULT) for L in Ls]
            assert default.smoother_kinds() == want, (what, default.smoother_kinds(), want)
    return check


@pytest.mark.parametrize("case", bs.SHAPE_CASES, ids=[c["id"] for c in bs.SHAPE_CASES])
def test_fast_and_default_paths_give_the_bits_of_the_general_kernels(w, case):
    """see the module docstring; the classes of each position are listed in tests/bodyshapes.py SHAPE_CASES"""
    fast, default, plain = handle(w, case, FAST), handle(w, case, DEFAULT), handle(w, case, PLAIN)
    for q in range(len(case["positions"])):
        run_position(w, case, q, fast, plain, default=default, each_call=True, steps3=bs.needs_steps3(case["positions"][q][1]), check=checker(case, q))
    assert np.isfinite(fast.field("u")).all(), case["id"]
    assert all(k in (0, 1) for k in plain.smoother_kinds()), case["id"]


ORACLE_CASES = [c["id"] for c in bs.SHAPE_CASES if c["id"] not in bs.PLAIN_ONLY]


@pytest.mark.parametrize("cid", ORACLE_CASES)
def test_general_path_on_these_shapes_matches_the_oracle(w, oracle, cid):
    """the plain handle against oracle.Simulation with the oracle's coefficient fields copied in, after the calls of the case's first position (two steps,
    five where it also runs mom_steps(3)) from the uniform inflow — the comparison and the bounds of test_gpu_bodypaths' oracle tie (equal pois.n,
    |Δu| < 5e-5).  Since fast = default = plain in bits above, this ties the shortcuts to the reference as well."""
    case = next(c for c in bs.SHAPE_CASES if c["id"] == cid)
    dims, (body, conds) = case["dims"], case["positions"][0]
    D = len(dims)
    U = (1.0,) + (0.0,) * (D - 1)
    so = oracle.Simulation(dims, U, 8.0, U=1, nu=NU, body=body, exitBC=case["exitBC"], T=f32)
    sg = w.FusedSimulation(dims, U, 8.0, U=1, nu=NU, has_body=True, exitBC=case["exitBC"])
    for k, v in PLAIN.items():
        sg.set_option(k, v)
    for k in ("mu0", "mu1", "V"):
        sg.set_field(k, so.field(k))
    sg.update_()
    for step in range(5 if bs.needs_steps3(conds) else 2):
        so.step(remeasure=False); sg.mom_step_()
        du = float(np.abs(sg.field("u") - so.u).max())
        print(cid, step, "pois_n", sg.pois_n, so.pois_n, "max|du| %.3g" % du)
        assert sg.pois_n == so.pois_n, step
        assert du < 5e-5, step
