"""Randomised call sequences: the default handle against an eager one, bit for bit at every observation (tests/callseq.py has the generator, the runner and
the families; tests/test_callseq_cpu.py the conditions on the scripts).  Every per-feature test pairs one option against itself switched off on a few scripted
sequences; here one seeded script of user-level calls — steps in calls of 0..4, reads, samples, diagnostics into σ, probes with a full buffer, tracers, the sgs
model and forcing on and off, Δt[end] set by the host, p and u written from outside, capped solves, the redo hook, update!, a step taken as phases, an option
toggled between two calls, with a body measure!, μ₀ handed out and the forces — runs on a handle with every deferral live and on one with all of them off that
is stepped singly and read after each step.  Afterwards the path counters say the deferrals really ran on the first handle and never on the second.

Its first run found one defect, since fixed: with the first tail inside the corrector's loader ("tailfuse", live in the box family alone) the launch that
leaves conv_diff!'s stale Φ in σ's ghost cells read the unprojected velocity from memory — 4466 of σ's 9192 ghost cells differed at the first op that returned σ
in box seeds 1, 2, 4, 5, 6.  Reduced sequence, cause and fix: tests/test_gpu_tailfuse_default.py::test_sigma_ghost_cells_after_a_step_are_those_of_the_separate_tail.

A failure names family, seed, op index and the ops up to it; `python -c "import sys; sys.path.insert(0, 'tests'); import callseq; callseq.replay('box', 3, 17)"`
runs that prefix again."""
import pytest

import callseq as cs

pytestmark = pytest.mark.gpu

LIVE = ("pdefer", "bcdefer", "rskip", "tailspec", "tailfuse", "hybrid")


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    yield w
    w.lib().wl_reset_process_options()      # resjac_min / convt_min / body_tile are process-wide


@pytest.mark.parametrize("seed", cs.SEEDS)
@pytest.mark.parametrize("family", cs.FAMILIES)
def test_default_handle_equals_eager_handle(w, family, seed):
    ops = cs.script(family, seed)
    A, B = cs.make(family, w)
    try:
        cs.run(ops, A, B, w, family, seed)
        a, b = {k: A.counter(k) for k in LIVE}, {k: B.counter(k) for k in LIVE}
        print(f"[callseq] {family} seed {seed}: {len(ops)} ops, {sum(cs.nsteps(op) for op in ops)} steps; A {a}")
        assert all(v == 0 for v in b.values()), (family, seed, b)
        if family in ("box", "ragged"):
            assert all(a[k] > 0 for k in ("pdefer", "bcdefer", "rskip", "tailspec")), (family, seed, a)
        if family == "box":
            assert a["tailfuse"] > 0, (seed, a)
        if family == "ragged":
            assert a["tailfuse"] == 0, (seed, a)
        if family == "moving":
            assert a["hybrid"] > 0, (seed, a)
    finally:
        if family == "caller":
            A.close()
