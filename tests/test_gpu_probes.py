"""Probe records inside wl_sim_mom_step / wl_sim_mom_steps (wl_sim_set_probes, wl_sim_read_probes): one record of u and p at the probe
points per completed step, taken on the device between the second projection and CFL.

Three handles per configuration — A with probes, stepped by ONE mom_steps_(4) call; B without, stepped by four mom_step_() calls, each
followed by sample(points) and time(); C never observed, stepped like A.  The records of A, the samples of B and the times are equal bit
for bit, and u, u⁰, p (every cell, ghosts included) and the Δt history of A, B and C are: the recorder changes nothing the step computes.
Then what it costs in launches (wl_sim_counter "launches"), what a full buffer does, and the 2-D case with a body."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    yield w
    w.lib().wl_reset_process_options()      # resjac_min / convt_min are process-wide


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def tgv(w, dims, **opts):
    sg = w.FusedSimulation(dims, (0.0,) * len(dims), dims[0], U=1, nu=dims[0] / 1600.0, ic="tgv")
    for k, v in opts.items():
        sg.set_option(k, v)
    return sg


def circle(w):
    """BASELINE's 2-D circle case (radius m/8 at (m/2 − 1, m/2 − 1), Re = 100, U = 1) at 32×24"""
    n, m = 32, 24
    radius, center = m / 8, m / 2 - 1
    sg = w.FusedSimulation((n, m), (1.0, 0.0), 2 * radius, U=1, nu=2 * radius / 100, has_body=True)
    sg.measure_sphere_((center, center), radius, 1.0)
    return sg


def probe_points(dims, m, seed=2):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (m, len(dims))).astype(f32) * np.array(dims, dtype=f32)
    x[0] = np.array(dims, dtype=f32) + 3          # outside: clamped to the last cells
    return x


def assert_same_state(a, b, what):
    for name in ("u", "u0", "p"):
        x, y = bits(a.field(name)), bits(b.field(name))
        assert np.array_equal(x, y), (what, name, int((x != y).sum()))
    da, db = [f32(v).view(np.uint32) for v in a.dt], [f32(v).view(np.uint32) for v in b.dt]
    assert da == db, (what, [float(v) for v in a.dt], [float(v) for v in b.dt])
    assert a.pois_n == b.pois_n, (what, a.pois_n, b.pois_n)


FUSED = dict(tailfuse=1, resjac_min=0, convt_min=0)
CONFIGS = {
    "tgv16": (lambda w: tgv(w, (16, 16, 16)), (16, 16, 16)),
    "tgv32_fused": (lambda w: tgv(w, (32, 32, 32), **FUSED), (32, 32, 32)),            # the configuration the issue names
    "tgv64x32x24_fused": (lambda w: tgv(w, (64, 32, 24), **FUSED), (64, 32, 24)),      # the smallest shape class the fused head takes: pdefer and lazydt are live (asserted)
    "circle2d": (circle, (32, 24)),
}


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_records_equal_hand_sampling_and_the_flow_is_untouched(w, cfg):
    make, dims = CONFIGS[cfg]
    D, m, k = len(dims), 5, 4
    pts = probe_points(dims, m)
    A, B, Cc = make(w), make(w), make(w)
    A.set_probes(pts, capacity=8)
    A.mom_steps_(k)
    Cc.mom_steps_(k)
    hand_u, hand_p, hand_t = [], [], []
    for _ in range(k):
        B.mom_step_()
        u, p = B.sample(pts)
        hand_u.append(u.cpu().numpy()); hand_p.append(p.cpu().numpy()); hand_t.append(B.time())
    assert A.counter("probe_records") == k and A.counter("probe_dropped") == 0
    t, ru, rp = A.read_probes()
    assert ru.shape == (k, m, D) and rp.shape == (k, m) and t.shape == (k,)
    assert np.array_equal(bits(ru), bits(np.stack(hand_u))), cfg
    assert np.array_equal(bits(rp), bits(np.stack(hand_p))), cfg
    assert [float(v) for v in t] == [float(v) for v in hand_t], (t, hand_t)
    assert np.abs(ru).max() > 0.05 and np.isfinite(ru).all() and np.isfinite(rp).all()
    assert not np.array_equal(ru[0], ru[-1]), "the records are of different steps"
    assert A.counter("probe_records") == 0
    assert_same_state(A, Cc, cfg + ": probes vs none")
    assert_same_state(A, B, cfg + ": one call vs single steps")
    print(f"[probes] {cfg}: pdefer A {A.counter('pdefer')} / C {Cc.counter('pdefer')}, tailfuse {A.counter('tailfuse')}, resjac {A.counter('resjac')}")
    if cfg == "tgv64x32x24_fused":
        # the deferred paths really ran under the recorder: C skips every store but the call's last (2k − 1), A keeps the corrector's stores (k skipped)
        assert Cc.counter("pdefer") == 2 * k - 1 and A.counter("pdefer") == k and A.counter("tailfuse") >= 1 and A.counter("resjac") >= 1


def launches(sg, n):
    l0 = sg.counter("launches")
    sg.mom_steps_(n)
    return sg.counter("launches") - l0


def test_launch_counts(w):
    dims, n = (16, 16, 16), 3
    A, Cc = tgv(w, dims), tgv(w, dims)
    pts = probe_points(dims, 5)
    assert launches(A, n) == launches(Cc, n)                                  # nothing registered: the same launches
    A.set_probes(pts, capacity=64)
    la, lc = launches(A, n), launches(Cc, n)
    assert la - lc == n, (la, lc)                                             # one launch per step
    A.set_tracers(probe_points(dims, 300, seed=4))
    la, lc = launches(A, n), launches(Cc, n)
    assert la - lc == 2 * n, (la, lc)                                         # two with tracers too
    A.set_probes(None, 0)
    la, lc = launches(A, n), launches(Cc, n)
    assert la - lc == n, (la, lc)                                             # tracers alone
    A.set_tracers(None)
    assert launches(A, n) == launches(Cc, n)
    assert_same_state(A, Cc, "after registering and unregistering")


def test_overflow_drops_new_records_and_reading_resumes(w):
    dims, m = (16, 16, 16), 3
    pts = probe_points(dims, m)
    A, B = tgv(w, dims), tgv(w, dims)
    A.set_probes(pts, capacity=2)
    A.mom_steps_(4)
    hand = []
    for _ in range(6):
        B.mom_step_()
        u, p = B.sample(pts)
        hand.append((u.cpu().numpy(), p.cpu().numpy(), B.time()))
    assert A.counter("probe_records") == 2 and A.counter("probe_dropped") == 2
    t, ru, rp = A.read_probes()
    assert ru.shape == (2, m, 3)
    for r in range(2):                                                        # the two held are the FIRST two
        assert np.array_equal(bits(ru[r]), bits(hand[r][0])) and np.array_equal(bits(rp[r]), bits(hand[r][1])) and float(t[r]) == float(hand[r][2])
    assert A.counter("probe_records") == 0 and A.counter("probe_dropped") == 2
    t, ru, rp = A.read_probes()
    assert ru.shape == (0, m, 3) and t.shape == (0,)
    A.mom_step_(); A.mom_step_()                                              # recording resumes: steps 5 and 6
    assert A.counter("probe_records") == 2
    t, ru, rp = A.read_probes()
    for r in range(2):
        assert np.array_equal(bits(ru[r]), bits(hand[4 + r][0])) and np.array_equal(bits(rp[r]), bits(hand[4 + r][1])) and float(t[r]) == float(hand[4 + r][2])
