"""Force records inside wl_sim_mom_step / wl_sim_mom_steps (wl_sim_set_force_record, wl_sim_read_forces) and the one-pass read-out
wl_sim_forces_bodyset: pressure force, viscous force and both moments from the body's band only (csrc/wl_forces.hip).

Three handles per geometry of tests/forces_ref.py — A with the recorder, stepped by ONE mom_steps_(4); B without, four mom_step_() each followed by
the four existing read-outs; C never observed, stepped like A.  u, u⁰, p, Δt and pois.n of the three are equal bit for bit.  The records of A and the
read-outs of B are Float64 sums of the same Float32 terms in different orders, so they differ by at most n_b²·2⁻⁵³·max|term| (forces_ref.tolerances,
from B's host fields); nothing looser is accepted.

With the FUSED options of tests/test_gpu_probes.py at 64×32×24 the counters "pdefer", "tailfuse" and "resjac" are asserted too: the recorder needs a
has_body=1 handle, on which pdefer_ok() and tailfuse_ok() (no body) and the fused head (constant coefficients) stand down — all three count 0 on A, B
and C alike, which is what is asserted; the probe test's positive counts belong to its body-free TGV handles."""
import ctypes as C

import numpy as np
import pytest

import forces_ref as fr

pytestmark = pytest.mark.gpu
f32 = np.float32
FUSED = dict(tailfuse=1, resjac_min=0, convt_min=0)
K = 4


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    yield w
    w.lib().wl_reset_process_options()      # resjac_min / convt_min are process-wide


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make(w, c, body=None, **opts):
    sg = w.FusedSimulation(c["dims"], c["uBC"], c["L"], U=1, nu=c["nu"], perdir=c["perdir"], has_body=True)
    for k, v in opts.items():
        sg.set_option(k, v)
    sg.set_body(c["body"] if body is None else body)
    return sg


def assert_same_state(a, b, what):
    for name in ("u", "u0", "p"):
        x, y = bits(a.field(name)), bits(b.field(name))
        assert np.array_equal(x, y), (what, name, int((x != y).sum()))
    da, db = [f32(v).view(np.uint32) for v in a.dt], [f32(v).view(np.uint32) for v in b.dt]
    assert da == db, (what, [float(v) for v in a.dt], [float(v) for v in b.dt])
    assert a.pois_n == b.pois_n, (what, a.pois_n, b.pois_n)


def hand(sg, body, x0):
    """the four existing read-outs, as one 12-vector laid out like a record"""
    D = sg.D
    out = np.zeros(12)
    out[0:D] = sg.pressure_force_body(body)
    out[3:3 + D] = sg.viscous_force_body(body)
    out[6:6 + D] = sg.pressure_moment_body(x0, body)
    out[9:9 + D] = sg.viscous_moment_body(x0, body)
    return out


def as12(D, pF, vF, pM, vM):
    out = np.zeros(12)
    out[0:D], out[3:3 + D] = pF, vF
    if D == 3:
        out[6:9], out[9:12] = pM, vM
    else:
        out[6:8], out[9:11] = pM[0], vM[0]
    return out


def tol12(sg, body, x0):
    tp, tv, tpm, tvm = fr.tolerances(body, sg.field("p"), sg.field("u"), sg.nu, x0)
    return np.repeat([tp, tv, tpm, tvm], 3)


def check_close(got, want, tol, what):
    err = np.abs(got - want)
    print(f"[forces] {what}: max |Δ| by quantity {err.reshape(4, 3).max(axis=1)}, tolerance {tol[::3]}, |pF| {np.linalg.norm(want[:3]):.3e}")
    assert np.all(err <= tol), (what, err, tol)


RUNS = [(name, {}) for name in fr.CASES] + [("sphere_inside", FUSED)]


@pytest.mark.parametrize("name,opts", RUNS, ids=[n + ("_fused" if o else "") for n, o in RUNS])
def test_records_equal_hand_sampling_and_the_flow_is_untouched(w, name, opts):
    c = fr.case(name)
    D, body, x0 = len(c["dims"]), c["body"], c["x0"]
    active, _, nb, _ = fr.band(body, c["Ng"])
    A, B, Cc = make(w, c, **opts), make(w, c, **opts), make(w, c, **opts)
    A.set_force_record(body, x0=x0, capacity=8)
    assert A.counter("force_tiles") == len(active)
    A.mom_steps_(K)
    Cc.mom_steps_(K)
    hands, tols, times = [], [], []
    for _ in range(K):
        B.mom_step_()
        hands.append(hand(B, body, x0)); tols.append(tol12(B, body, x0)); times.append(B.time())
    assert A.counter("force_records") == K and A.counter("force_dropped") == 0
    t, pF, vF, pM, vM = A.read_forces()
    assert pF.shape == (K, D) and vF.shape == (K, D) and pM.shape == (K, 3 if D == 3 else 1) and t.shape == (K,)
    assert [float(v) for v in t] == [float(v) for v in times], (t, times)
    assert A.counter("force_records") == 0
    for r in range(K):
        rec = as12(D, pF[r], vF[r], pM[r], vM[r])
        if c["nonempty"]:
            check_close(rec, hands[r], tols[r], f"{name} step {r}")
        else:
            assert np.all(rec == 0.0) and np.all(hands[r] == 0.0)
    if c["nonempty"]:
        assert np.linalg.norm(pF[-1]) >= 100 * tols[-1][0] and not np.array_equal(pF[0], pF[-1])
    else:
        assert A.counter("force_tiles") == 0
    assert_same_state(A, Cc, name + ": recorder vs none")
    assert_same_state(A, B, name + ": one call vs single steps")
    cnt = {h: [s.counter(k) for k in ("pdefer", "tailfuse", "resjac")] for h, s in (("A", A), ("B", B), ("C", Cc))}
    print(f"[forces] {name}: pdefer/tailfuse/resjac {cnt}, force_tiles {len(active)}, n_b {nb}")
    if opts:
        assert cnt["A"] == cnt["C"] == cnt["B"] == [0, 0, 0], cnt      # see the module docstring


@pytest.mark.parametrize("name", list(fr.CASES))
def test_forces_equals_the_four_calls(w, name):
    c = fr.case(name)
    D, body, x0 = len(c["dims"]), c["body"], c["x0"]
    active, _, _, _ = fr.band(body, c["Ng"])
    sg = make(w, c)
    sg.mom_steps_(2)
    l0 = w.lib().wl_launch_count()
    got = as12(D, *sg.forces(body, x0=x0))
    assert w.lib().wl_launch_count() - l0 == (4 if c["nonempty"] else 3)      # classify, scan, band, finish
    assert sg.counter("force_tiles") == len(active), (sg.counter("force_tiles"), len(active))
    l0 = w.lib().wl_launch_count()
    again = as12(D, *sg.forces(body, x0=x0))
    assert w.lib().wl_launch_count() - l0 == (2 if c["nonempty"] else 1)      # the list is kept
    assert np.array_equal(got, again)
    want = hand(sg, body, x0)
    if c["nonempty"]:
        check_close(got, want, tol12(sg, body, x0), name)
    else:
        assert np.all(got == 0.0) and np.all(want == 0.0)
    # moments about the origin when x0 is left out; a closed-form tuple is its leaf
    if name == "sphere_inside":
        tup = ("sphere", (20.3, 15.6, 11.7), 5.0)
        o = as12(D, *sg.forces(tup))
        check_close(o, hand(sg, body, (0.0, 0.0, 0.0)), tol12(sg, body, (0.0, 0.0, 0.0)), name + " about the origin")
        assert np.array_equal(o[:6], got[:6])


def test_two_fresh_handles_give_the_same_bits(w):
    c = fr.case("rotated_set")
    recs = []
    for _ in range(2):
        sg = make(w, c)
        sg.set_force_record(c["body"], x0=c["x0"], capacity=4)
        sg.mom_steps_(3)
        recs.append(np.concatenate([a.reshape(3, -1) for a in sg.read_forces()[1:]], axis=1))
    assert np.array_equal(recs[0].view(np.uint64), recs[1].view(np.uint64)) and np.abs(recs[0]).max() > 0


def moving(w, y):
    return w.Body(("sphere", (0.0, 0.0, 0.0), 4.0), w.RigidMap((20.3, y, 11.7), (0.0, 0.0, 0.0), V=(0.0, 0.25, 0.0)))


def test_moving_body_keeps_a_correct_history(w):
    c = fr.case("sphere_inside")
    ys = [12.3 + 1.5 * k for k in range(K)]
    want_tiles = [len(fr.band(moving(w, y), c["Ng"])[0]) for y in ys]
    assert len(set(want_tiles)) > 1, want_tiles                 # the sphere crosses a tile boundary on the way
    A, B = make(w, c, body=moving(w, ys[0])), make(w, c, body=moving(w, ys[0]))
    A.set_force_record(moving(w, ys[0]), x0=c["x0"], capacity=8)      # once, at the start
    tiles, hands, tols = [], [], []
    for y in ys:
        for sg in (A, B):
            sg.body = w.setmap(sg.body, x0=(20.3, y, 11.7))
            sg.sim_step_(remeasure=True)
        tiles.append(A.counter("force_tiles"))
        hands.append(hand(B, B.body, c["x0"])); tols.append(tol12(B, B.body, c["x0"]))
    assert tiles == want_tiles, (tiles, want_tiles)
    t, pF, vF, pM, vM = A.read_forces()
    assert len(t) == K
    for r in range(K):
        check_close(as12(3, pF[r], vF[r], pM[r], vM[r]), hands[r], tols[r], f"moving step {r}")
    assert_same_state(A, B, "moving body")


def test_overflow_drops_new_records_and_reading_resumes(w):
    c = fr.case("ragged_48x20x12")
    A, B = make(w, c), make(w, c)
    A.set_force_record(c["body"], x0=c["x0"], capacity=2)
    A.mom_steps_(4)
    hands, tols, times = [], [], []
    for _ in range(6):
        B.mom_step_()
        hands.append(hand(B, c["body"], c["x0"])); tols.append(tol12(B, c["body"], c["x0"])); times.append(B.time())
    assert A.counter("force_records") == 2 and A.counter("force_dropped") == 2
    t, pF, vF, pM, vM = A.read_forces()
    assert pF.shape == (2, 3)
    for r in range(2):                                                        # the two held are the FIRST two
        check_close(as12(3, pF[r], vF[r], pM[r], vM[r]), hands[r], tols[r], f"overflow {r}")
        assert float(t[r]) == float(times[r])
    assert A.counter("force_records") == 0 and A.counter("force_dropped") == 2
    assert A.read_forces()[1].shape == (0, 3)
    A.mom_step_(); A.mom_step_()                                              # recording resumes: steps 5 and 6
    t, pF, vF, pM, vM = A.read_forces()
    assert pF.shape == (2, 3)
    for r in range(2):
        check_close(as12(3, pF[r], vF[r], pM[r], vM[r]), hands[4 + r], tols[4 + r], f"resumed {r}")
        assert float(t[r]) == float(times[4 + r])


def launches(sg, n):
    l0 = sg.counter("launches")
    sg.mom_steps_(n)
    return sg.counter("launches") - l0


def test_launch_counts(w):
    c, n = fr.case("ragged_48x20x12"), 3
    A, Cc = make(w, c), make(w, c)
    assert launches(A, n) == launches(Cc, n)
    A.set_force_record(c["body"], capacity=16)
    la, lc = launches(A, n), launches(Cc, n)
    assert la - lc == 2 * n, (la, lc)                                         # band + finish per step
    A.set_force_record(None)
    assert launches(A, n) == launches(Cc, n)
    assert_same_state(A, Cc, "after setting and unsetting the recorder")
    e = fr.case("outside")
    E, Ec = make(w, e), make(w, e)
    E.set_force_record(e["body"], capacity=16)
    la, lc = launches(E, n), launches(Ec, n)
    assert la - lc == n, (la, lc)                                             # an empty list: the finish alone
    assert E.counter("force_tiles") == 0 and E.counter("force_records") == n


def test_error_paths(w):
    from waterlily_jl_amd._lib import ALLGATHER_FN, SENDRECV_FN, wl_sim_desc
    L = w.lib()
    body = fr.case("sphere_inside")["body"]
    nb = w.FusedSimulation((16, 16, 16), (1.0, 0.0, 0.0), 8, nu=0.01)      # has_body=False
    with pytest.raises(w.WlError, match="has_body"):
        nb.set_force_record(body)
    with pytest.raises(w.WlError, match="has_body"):
        nb.forces(body)
    # a z-slab handle (rank 0 of 2; the transport does nothing: no step is taken)
    sr = SENDRECV_FN(lambda *a: 0); ag = ALLGATHER_FN(lambda *a: 0)
    comm = C.c_void_p()
    assert L.wl_comm_callbacks_create(C.byref(comm), 0, 2, None, C.cast(sr, C.c_void_p), C.cast(ag, C.c_void_p)) == 0
    d = wl_sim_desc()
    d.D, d.has_body = 3, 1
    for k in range(3):
        d.dims[k] = (16, 16, 32)[k]
    d.nu, d.dt0 = 0.01, 0.25
    h = C.c_void_p()
    assert L.wl_sim_create_slab(C.byref(h), C.byref(d), comm) == 0
    prog, out = body.program(3), (C.c_double * 12)()
    assert L.wl_sim_set_force_record(h, C.byref(prog), None, 4) == -1 and b"slab" in L.wl_last_error_string()
    assert L.wl_sim_forces_bodyset(h, None, C.byref(prog), out, None) == -1 and b"slab" in L.wl_last_error_string()
    assert L.wl_sim_destroy(h) == 0 and L.wl_comm_destroy(comm) == 0
    # a record buffer too small for what is held: nothing is read
    c = fr.case("ragged_48x20x12")
    sg = make(w, c)
    sg.set_force_record(c["body"], capacity=4)
    sg.mom_steps_(2)
    k, first = C.c_int(0), C.c_int(0)
    buf = (C.c_double * 12)()
    assert L.wl_sim_read_forces(sg._h, buf, 1, C.byref(k), C.byref(first)) == -1 and k.value == 2
    assert sg.counter("force_records") == 2
