"""Smoother kernel B without the store of the residual that nobody reads (option "rskip", wl_mg::skip_r; k_gsrb2_B's output modes in csrc/wl_fused2_body.inc).
The statements per cell are the same in every mode, so a handle with rskip=1 against a handle with rskip=0 on the same library must agree on u, u⁰, p on
every cell as raw bits, on pois.n and on the Δt history; the finest residual read back through wl_mg_level_field must agree too, produced on demand by the
r-only instance where the last smooth! skipped its store.  The counters are checked against the policy restated here and fed with the ORACLE's pois.n:
iteration k of a solve skips the store iff the previous solve of the same slot (predictor / corrector) stopped at exactly k; a skipped store after which the
loop goes on costs one r-only launch."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

f32 = np.float32
UBC = (0.3, -0.2, 0.1)
NU = 0.02
# interior sizes.  SMALL: finest level on the 16-row instance, level 1 (34×18×14 with ghosts) off the pair kernels.  TWO: levels 0 and 1 on the pair kernels.
# WIDE: 450×370 planes are ceil(450/56)·ceil(370/26) = 9·15 = 135 >= 128 tiles of 56×26 cells: rows16() sends kernel B to the 32-row instance.
SMALL, TWO, WIDE = (64, 32, 24), (64, 64, 16), (448, 368, 8)
WIDE_TILES = ((WIDE[0] + 2 + 55) // 56) * ((WIDE[1] + 2 + 25) // 26)
assert WIDE_TILES == 135


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    yield w
    w.lib().wl_reset_process_options()      # resjac_min / convt_min are process-wide


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_state(a, b, what):
    for name in ("u", "u0", "p"):
        x, y = bits(a.field(name)), bits(b.field(name))
        assert np.array_equal(x, y), (what, name, int((x != y).sum()))
    assert a.pois_n == b.pois_n, (what, a.pois_n, b.pois_n)
    da, db = [f32(v).view(np.uint32) for v in a.dt], [f32(v).view(np.uint32) for v in b.dt]
    assert da == db, (what, [float(v) for v in a.dt], [float(v) for v in b.dt])


def random_u(oracle, dims, seed):
    rng = np.random.default_rng(seed)
    u = np.asfortranarray(rng.uniform(-0.4, 0.4, size=tuple(n + 2 for n in dims) + (3,)).astype(f32))
    oracle.BC(u, UBC)
    return u


def make(w, dims, u0, **opts):
    """u0 = None: the wall-bounded TGV (U = 0); else a random field with U ≠ 0 on every axis"""
    if u0 is None:
        sg = w.FusedSimulation(dims, (0.0,) * 3, dims[0], U=1, nu=dims[0] / 1600.0, ic="tgv")
    else:
        sg = w.FusedSimulation(dims, UBC, dims[0], U=1, nu=NU, u0=u0)
    sg.set_option("resjac_min", 0)
    sg.set_option("convt_min", 0)
    for k, v in opts.items():
        sg.set_option(k, v)
    return sg


def policy(pois_n):
    """the rule, from the iteration counts alone (solves alternate predictor, corrector): -> (skipped stores, r-only launches inside the loops, r stale at the end)"""
    hist, skips, redos, stale = [0, 0], 0, 0, False
    for q, n in enumerate(pois_n):
        slot = q & 1
        stale = False                        # a solve rebuilds r from scratch
        k = hist[slot]
        if 1 <= k <= n:                      # iteration k does not store r'
            skips += 1
            if k < n:
                redos += 1                   # the loop went on: r' from the r-only instance before the next V-cycle
            else:
                stale = True                 # the loop ended there
        hist[slot] = n
    return skips, redos, stale


def run_pair(w, on, off, calls, what):
    """the same calls on both handles: state as raw bits after each; launches(on) = launches(off) + the r-only launches; rskip=0 counts nothing"""
    for q, k in enumerate(calls):
        res = []
        for s in (on, off):
            l0, c0, r0 = w.lib().wl_launch_count(), s.counter("rskip"), s.counter("rskip_redo")
            if k == 0:
                s.mom_step_()
            else:
                s.mom_steps_(k)
            res.append((w.lib().wl_launch_count() - l0, s.counter("rskip") - c0, s.counter("rskip_redo") - r0))
        (lon, con, ron), (loff, coff, roff) = res
        print(f"{what} call {q} k={k}: rskip +{con} redo +{ron} (off: +{coff} +{roff}), launches {lon} vs {loff}, pois.n {on.pois_n[-2 * max(k, 1):]}")
        assert coff == 0 and roff == 0, (what, q, coff, roff)
        assert lon == loff + ron, (what, q, "launches", lon, loff, ron)
        assert_same_state(on, off, (what, q, k))
    assert off.counter("rskip") == 0 and off.counter("rskip_redo") == 0


def read_r(w, on, off, what, expect_stale):
    """the finest residual through wl_mg_level_field: equal bits; the read launches the r-only instance iff r was stale"""
    r0, l0 = on.counter("rskip_redo"), w.lib().wl_launch_count()
    ron = on.pois_level("r")
    rose, launched = on.counter("rskip_redo") - r0, w.lib().wl_launch_count() - l0
    roff = off.pois_level("r")
    print(f"{what}: read of r: rskip_redo +{rose}, launches +{launched}, stale expected {expect_stale}")
    assert rose == (1 if expect_stale else 0) and launched == rose, (what, rose, launched, expect_stale)
    assert off.counter("rskip_redo") == 0
    assert np.array_equal(bits(ron), bits(roff)), (what, "r", int((bits(ron) != bits(roff)).sum()))
    r1 = on.counter("rskip_redo")
    assert np.array_equal(bits(on.pois_level("r")), bits(roff)) and on.counter("rskip_redo") == r1, (what, "second read")


MODES = {
    "default": {},
    "tailspec0": {"tailspec": 0},        # no tail is gated: the host decides every break test
    "headspec0": {"headspec": 0},        # no early V-cycle
    "redo": {"resjac": 2},               # every head redone: each speculative solve is discarded after its first iteration (which may have skipped)
    "tailfuse1": {"tailfuse": 1},        # the first tail inside the corrector's loader
    "pdefer0": {"pdefer": 0},
}
CALLS = (1, 2, 5, 0)


def check_pair(w, oracle, dims, field, mode):
    u0 = None if field == "tgv" else random_u(oracle, dims, 71)
    on, off = make(w, dims, u0, rskip=1, **MODES[mode]), make(w, dims, u0, rskip=0, **MODES[mode])
    what = f"{'x'.join(map(str, dims))}-{field}-{mode}"
    run_pair(w, on, off, CALLS, what)
    skips, redos, stale = policy(on.pois_n)
    print(f"{what}: pois.n {on.pois_n}; rskip {on.counter('rskip')} redo {on.counter('rskip_redo')}; the rule: {skips} {redos} stale {stale}")
    if mode != "redo":      # (a discarded solve may skip too: the rule only knows the solves that stood)
        assert (on.counter("rskip"), on.counter("rskip_redo")) == (skips, redos), what
    else:
        assert on.counter("rskip") >= skips and on.counter("rskip_redo") == redos, what
    assert skips > 0, what
    read_r(w, on, off, what, stale)
    return on


@pytest.mark.parametrize("field", ["tgv", "random"])
@pytest.mark.parametrize("dims", [SMALL, TWO, WIDE], ids=["66x34x26", "66x66x18", "450x370x10"])
def test_rskip_is_bit_identical(w, oracle, dims, field):
    on = check_pair(w, oracle, dims, field, "default")
    kinds = on.smoother_kinds()
    if dims == SMALL:
        assert kinds[0] == 2 and kinds[1] != 2, kinds
    if dims == TWO:
        assert kinds[0] == 2 and kinds[1] == 2, kinds
    if dims == WIDE:
        assert kinds[0] == 2, kinds


@pytest.mark.parametrize("mode", [m for m in MODES if m != "default"])
def test_rskip_with_the_speculation_switched_off_piecewise(w, oracle, mode):
    check_pair(w, oracle, TWO, "random", mode)


def test_counters_follow_the_rule_on_the_oracles_iteration_counts(w, oracle):
    """8 steps of the random field at 66×66×18: the CPU oracle needs [4,2,5,2,2,2,2,1,…] V-cycles — per slot one miss (the predictor's second solve: 4 then 5,
    the store skipped at iteration 4 is recomputed) and hits from the repeats"""
    nstep = 8
    u0 = random_u(oracle, TWO, 71)
    so = oracle.Simulation(TWO, UBC, TWO[0], U=1, nu=NU, T=f32)
    so.field("u")[...] = u0
    so.field("u0")[...] = u0
    for _ in range(nstep):
        so.step(remeasure=False)
    n = [int(v) for v in so.pois_n]
    skips, redos, stale = policy(n)
    print(f"oracle pois.n {n}: the rule gives rskip {skips}, rskip_redo {redos}, stale at the end {stale}")
    assert redos >= 1 and skips - redos >= 1, (n, skips, redos)      # at least one miss and one hit
    on, off = make(w, TWO, u0, rskip=1), make(w, TWO, u0, rskip=0)
    on.mom_steps_(3)
    for _ in range(nstep - 3):
        on.mom_step_()
    off.mom_steps_(nstep)
    assert on.pois_n == n, (on.pois_n, n)
    assert on.counter("resjac_redo") == 0      # no solve was discarded: every solve is in pois.n
    assert (on.counter("rskip"), on.counter("rskip_redo")) == (skips, redos), (on.counter("rskip"), on.counter("rskip_redo"), skips, redos)
    assert_same_state(on, off, "rule")
    read_r(w, on, off, "rule", stale)


def last_solve_converged(w, sg, dims):
    cap = 80
    a, b, c = (C.c_double * cap)(), (C.c_double * cap)(), (C.c_double * cap)()
    k = w.lib().wl_mg_last_log(w.lib().wl_sim_pois(sg._h), a, b, c, cap)
    return bool(a[k - 1] < (2e-3 / 10.0) * float(np.prod(dims)) and b[k - 1] < 2e-3)      # solver!'s break test on the logged norms


def test_iteration_cap_right_after_a_skipped_store(w, oracle):
    """itmx = 2 on the same field, whose first solves need more (the oracle: 4, 2, 5): a solve that stops at the cap twice in a row ends unconverged right
    after a skipped store.  The steps go on from x alone; r is produced when it is read"""
    u0 = random_u(oracle, TWO, 71)
    on, off = make(w, TWO, u0, rskip=1, itmx=2), make(w, TWO, u0, rskip=0, itmx=2)
    run_pair(w, on, off, (0,), "itmx=2")
    on.phase_(0); on.phase_(1); on.phase_(2)      # the second step up to the predictor's projection
    off.phase_(0); off.phase_(1); off.phase_(2)
    n = on.pois_n
    print(f"itmx=2: pois.n {n}, last solve converged: {last_solve_converged(w, on, TWO)}")
    assert n[0] == 2 and n[2] == 2 and not last_solve_converged(w, on, TWO), n      # the predictor's solve hit the cap in both steps, the second time unconverged
    skips, redos, stale = policy(n)
    assert stale and redos == 0
    assert (on.counter("rskip"), on.counter("rskip_redo")) == (skips, redos)
    read_r(w, on, off, "itmx=2", True)
    for ph in (3, 4, 5):
        on.phase_(ph); off.phase_(ph)
    assert_same_state(on, off, "itmx=2, rest of the step")
    run_pair(w, on, off, (2, 0), "itmx=2, after the read")
    assert max(on.pois_n) == 2
    read_r(w, on, off, "itmx=2, again", policy(on.pois_n)[2])


def test_bare_solve_on_the_handles_own_multigrid(w, oracle):
    """wl_mg_solve on wl_sim_pois after some steps (r is stale on the rskip handle): a plain solve in no slot — the finest level stores every r', the coarse
    levels still skip theirs — equal to the rskip=0 handle in x, r, the iteration count and the log; the steps after it too"""
    u0 = random_u(oracle, TWO, 71)
    on, off = make(w, TWO, u0, rskip=1), make(w, TWO, u0, rskip=0)
    run_pair(w, on, off, (6,), "bare")
    assert policy(on.pois_n)[2]      # the last smooth! skipped its store
    lib, chk = w.lib(), w._lib.check
    Ng = tuple(n + 2 for n in TWO)
    rng = np.random.default_rng(109)
    z = np.zeros(Ng, dtype=f32, order="F")
    z[1:-1, 1:-1, 1:-1] = rng.uniform(-1e-2, 1e-2, size=TWO).astype(f32)
    out = []
    for sg in (on, off):
        mg = lib.wl_sim_pois(sg._h)
        c0 = (sg.counter("rskip"), sg.counter("rskip_redo"))
        chk(lib.wl_h2d(lib.wl_mg_level_field(mg, 0, b"z"), z.ctypes.data_as(C.c_void_p), z.nbytes, w.core.stream()))
        chk(lib.wl_stream_sync(w.core.stream()))
        n, r1, rinf = C.c_int(), C.c_double(), C.c_float()
        chk(lib.wl_mg_solve(mg, 2e-3, 32, C.byref(n), C.byref(r1), C.byref(rinf), w.core.stream()))
        assert (sg.counter("rskip"), sg.counter("rskip_redo")) == c0, "a bare solve skips nothing on the finest level and owes nothing"
        out.append((n.value, r1.value, rinf.value, sg.pois_level("x"), sg.pois_level("r")))
        assert (sg.counter("rskip"), sg.counter("rskip_redo")) == c0
    (n1, a1, b1, x1, rr1), (n0, a0, b0, x0, rr0) = out
    print(f"bare solve: n = {n1} (off: {n0}), r1 = {a1:.6e}, rinf = {b1:.6e}")
    assert n1 == n0 and n1 >= 2 and a1 == a0 and b1 == b0
    assert np.array_equal(bits(x1), bits(x0)) and np.array_equal(bits(rr1), bits(rr0))
    run_pair(w, on, off, (2,), "after the bare solve")


def test_rskip_switched_off_counts_nothing_and_stores(w, oracle):
    """rskip = 0 from the start: both counters stay 0 and no read of r launches anything; switched off on a handle that owes r: the debt is paid first"""
    u0 = random_u(oracle, SMALL, 71)
    off = make(w, SMALL, u0, rskip=0)
    on = make(w, SMALL, u0, rskip=1)
    run_pair(w, on, off, (4,), "off")
    stale = policy(on.pois_n)[2]
    r0 = on.counter("rskip_redo")
    on.set_option("rskip", 0)
    assert on.counter("rskip_redo") - r0 == (1 if stale else 0)
    read_r(w, on, off, "switched off", False)
    c = (on.counter("rskip"), on.counter("rskip_redo"))
    run_pair(w, on, off, (2, 0), "both off")
    assert (on.counter("rskip"), on.counter("rskip_redo")) == c


@pytest.mark.parametrize("withdraw", ["pair", "constl"])
def test_late_store_after_the_pair_kernels_were_switched_off(w, oracle, withdraw):
    """found by tests/test_gpu_optmatrix.py (the walk, reduced): a solve ends on a skipped store, then "pair" (process-wide) or "constl" (update!) withdraws the
    pair kernels, then somebody asks for r — set_option("rskip"), wl_mg_level_field.  The late store is the launch that skipped it, made again: it may not go
    by today's switches (it returned WL_EINVAL: "storing only one of r' and x needs the pair kernel").  r equals the handle's that stored every time."""
    u0 = random_u(oracle, SMALL, 3)
    on, off = make(w, SMALL, u0), make(w, SMALL, u0, rskip=0)
    for _ in range(6):                             # until a call ends on a skipped store (the corrector's solve stops where its last one did)
        for s in (on, off):
            s.mom_step_()
        if policy(on.pois_n)[2]:
            break
    assert policy(on.pois_n)[2] and on.counter("rskip") > 0, (on.pois_n, "no solve of six steps ended on a skipped store")
    for s in (on, off):
        s.set_option(withdraw, 0)
    r0 = on.counter("rskip_redo")
    on.set_option("rskip", 0)                      # settles the debt before it switches
    assert on.counter("rskip_redo") == r0 + 1
    assert np.array_equal(bits(on.pois_level("r")), bits(off.pois_level("r")))
    for s in (on, off):
        s.mom_step_()
    assert_same_state(on, off, withdraw)
