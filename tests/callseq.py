"""Randomised call sequences on two handles (test infrastructure; imports without a GPU).

script(family, seed) is a list of user-level calls as plain tuples.  run(script, A, B, w) applies it to the DEFAULT handle A — every deferral the library has
(pdefer, bcdefer, lazydt, tailfuse, tailspec, headspec, rskip, tailwide; with a body: hybrid, farmask, zsplit, body_tile) live, only the size gates opened — and
to the EAGER handle B, which has them all switched off, takes every step as a wl_sim_mom_step of its own and has p and u read after each of them.  The kernel
families are the same on both (fuse_p, constl, fused_smoother, resjac … sum Σr and L₁ in another order: not bit-comparable), so after every op that observes,
u, u⁰, p on every cell (ghosts included) as raw bits, pois.n, the Δt history and whatever the op returned must be equal.  A mismatch raises Mismatch with the
family, the seed, the index of the op and the ops up to it; replay(family, seed, upto) runs that prefix again.

The handles are driven through small adapters (Dev, CallerDev) with one method per call the runner makes; tests/test_callseq_cpu.py runs the same runner on
pure-Python fakes with these method names to show that the two expansions of a script are the same sequence of elementary operations."""
import numpy as np


f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def state_diff(a, b):
    """None, or (field, differing cells, detail) of the first of u, u⁰, p (every cell, ghosts included, as raw bits), pois.n, Δt that differs"""
    for name in ("u", "u0", "p"):
        x, y = bits(a.field(name)), bits(b.field(name))
        if not np.array_equal(x, y):
            return name, int((x != y).sum()), np.argwhere(x != y)[:4].tolist()
    if list(a.pois_n) != list(b.pois_n):
        return "pois_n", -1, (list(a.pois_n), list(b.pois_n))
    da, db = [int(f32(v).view(np.uint32)) for v in a.dt], [int(f32(v).view(np.uint32)) for v in b.dt]
    if da != db:
        return "dt", -1, ([float(v) for v in a.dt], [float(v) for v in b.dt])
    return None


def assert_same_state(a, b, what):
    """the one definition of "same state" (tests/test_gpu_pdefer.py asserts through it as well)"""
    d = state_diff(a, b)
    assert d is None, (what,) + d


FAMILIES = ("box", "ragged", "moving", "exit", "periodic", "circle2d", "caller")
SEEDS = (1, 2, 3, 4, 5, 6)                       # the seeds tests/test_gpu_callseq.py runs; tests/test_callseq_cpu.py holds the conditions on them
DIMS = {"box": (64, 32, 24), "ragged": (70, 44, 18), "periodic": (64, 32, 24), "caller": (64, 32, 24)}      # body families: tests/bodypaths_ref.py
BODY_CASE = {"moving": "moving", "exit": "deepfloor-exit", "circle2d": "circle2d"}
UBC = (0.3, -0.2, 0.1)
ACC = (0.01, -0.02, 0.015)                       # the constant uniform acceleration of the forcing ops
EAGER = {"pdefer": 0, "bcdefer": 0, "tailfuse": 0, "tailspec": 0, "headspec": 0, "lazydt": 0, "rskip": 0, "tailwide": 0}
EAGER_BODY = {"hybrid": 0, "farmask": 0, "zsplit": 0}
GATES = {"resjac_min": 0, "convt_min": 0, "tailfuse_min": 0}
DEFERRALS = ("pdefer", "bcdefer", "lazydt", "tailspec", "headspec", "rskip", "tailfuse", "tailwide")
BODY_TOGGLES = ("hybrid", "farmask", "rskip", "tailspec", "headspec", "tailwide")
PROBE_CAP, N_PROBES, N_TRACERS, N_SAMPLES = 3, 4, 16, 7

OBSERVERS = ("read", "pois_level", "sample", "flow_stats", "metric", "read_probes", "tracers", "forces")
STEPPERS = ("steps", "phase_step")


def kind(op):
    """what the coverage conditions count: the call, and its argument where that selects another path"""
    return op[0] + (":" + str(op[1]) if op[0] in ("metric", "itmx", "resjac", "pois_level", "sgs", "forcing") else "") + (":%s:%d" % (op[1], op[2]) if op[0] == "toggle" else "")


def nsteps(op):
    return max(op[1], 1) if op[0] == "steps" else (1 if op[0] == "phase_step" else 0)


def observes(op):
    return op[0] in OBSERVERS


def mutates(op):
    return not observes(op) and op[0] not in STEPPERS


# ---------------------------------------------------------------------------------------------------------------------------- generator
def tracks(family, rng, seed=1):
    """the non-step ops of one script as ordered tracks (set before read before clear …): every kind the family supports, once"""
    D2, body, caller = family == "circle2d", family in BODY_CASE, family == "caller"
    s = lambda: int(rng.integers(1, 1 << 30))
    names = ("u", "u0", "p", "sigma")
    if caller:      # what CallerOwnedSim can express — each twice, so that the script is as long as the others
        t = [[("sgs", 1), ("sgs", 0)], [("sgs", 1), ("sgs", 0)]]
        t += [[("set_dt_last",)] for _ in range(3)] + [[("sample", s())] for _ in range(4)]
        t += [[("read", tuple(n for n in ("u", "u0", "p") if rng.random() < 0.6) or ("p",))] for _ in range(6)]
        return t
    t = [[("read", tuple(n for n in names if rng.random() < 0.6) or ("p",))], [("pois_level", "r")], [("pois_level", "x")], [("sample", s())], [("flow_stats",)]]
    t += [[("metric", m)] for m in (("ke",) if D2 else ("omega_mag", "lambda2", "ke"))]
    if not D2:
        t.append([("sgs", 1), ("sgs", 0)])
    t.append([("forcing", 1), ("forcing", 0)])
    t += [[("set_dt_last",)], [("set_p", s())], [("set_u", s())], [("phase_step",)]]
    t.append([("set_probes", s()), ("read_probes",), ("clear_probes",)])
    t.append([("set_tracers", s()), ("tracers",)])
    a, b = (1, 2) if rng.random() < 0.5 else (2, 1)
    t.append([("itmx", a), ("itmx", b), ("itmx", 32)])
    t.append([("resjac", 3), ("resjac", 1), ("update",)])
    # which option is toggled goes by the seed, so that over SEEDS every deferral is switched off and on again in the whole-tile families (two per script);
    # a script with a body has room for one: the body shortcuts and the deferrals that stay live next to a body
    q = (int(seed) - 1) % 6
    for opt in ((BODY_TOGGLES[q],) if body else (DEFERRALS[(2 * q) % 8], DEFERRALS[(2 * q + 1) % 8])):
        t.append([("toggle", opt, 0), ("toggle", opt, 1)])
    if body:
        t += [[("measure", int(rng.integers(0, 2)))], [("touch_mu0",)], [("forces",)]]
    return t


STEP_OPS = {"circle2d": 9}      # step ops per script (default 10; the mean call is 2.2 steps)


def _build(family, rng, seed):
    t = tracks(family, rng, seed)
    ops = []
    while t:      # a random merge that keeps the order inside a track
        w = np.array([len(x) for x in t], dtype=np.float64)
        q = int(rng.choice(len(t), p=w / w.sum()))
        ops.append(t[q].pop(0))
        if not t[q]:
            t.pop(q)
    n = STEP_OPS.get(family, 10)
    gaps = sorted(int(g) for g in rng.integers(0, len(ops) + 1, size=n - 1)) + [0]      # one call first: the first op meets a handle that has stepped
    out = []
    for j in range(len(ops) + 1):
        out += [("steps", int(rng.integers(0, 5))) for g in gaps if g == j]
        if j < len(ops):
            out.append(ops[j])

    def between(a, b):
        ia, ib = out.index(a), out.index(b)
        return ia, ib, [q for q in range(ia + 1, ib) if out[q][0] == "steps"]

    # the adjacencies the issue names, made certain: Δt[end] changed before a multi-step (lazydt) call, a multi-step call under tracers, a full probe buffer
    for q, op in enumerate(out):
        if op[0] == "set_dt_last":
            nxt = next((r for r in range(q + 1, len(out)) if out[r][0] in STEPPERS), None)
            if nxt is None:
                out.append(("steps", 2))
            elif out[nxt][0] == "steps":
                out[nxt] = ("steps", max(out[nxt][1], 2))
            else:
                out.insert(nxt, ("steps", 2))
    tr = [op for op in out if op[0] == "set_tracers"]
    if tr:
        ia, ib, st = between(tr[0], ("tracers",))
        if not st:
            out.insert(ib, ("steps", 2))
        elif not any(out[q][1] >= 2 for q in st):
            out[st[0]] = ("steps", 2)
    pr = [op for op in out if op[0] == "set_probes"]
    if pr:
        ia, ib, st = between(pr[0], ("read_probes",))
        if not st:
            out.insert(ib, ("steps", 4))
        elif sum(nsteps(out[q]) for q in st) <= PROBE_CAP:
            out[st[-1]] = ("steps", 4)
    out.append(("read", ("u", "u0", "p") if family == "caller" else ("u", "u0", "p", "sigma")))
    return out


def conditions(ops):
    """what keeps a script from being hollow (tests/test_callseq_cpu.py asserts them): None, or the condition that fails"""
    total = sum(nsteps(op) for op in ops)
    if not 12 <= total <= 40:
        return "steps %d" % total
    if len(ops) > 45:
        return "ops %d" % len(ops)
    if not any(a[0] == "steps" and a[1] >= 2 and observes(b) for a, b in zip(ops, ops[1:])):
        return "no multi-step call directly followed by an observing op"
    st = [q for q, op in enumerate(ops) if op[0] in STEPPERS]
    if not any(any(mutates(ops[q]) for q in range(a + 1, b)) for a, b in zip(st, st[1:])):
        return "no mutating op between two step ops"
    return None


def script(family, seed):
    """deterministic in (family, seed); the first draw that meets conditions()"""
    assert family in FAMILIES, family
    for attempt in range(200):
        ops = _build(family, np.random.default_rng([int(seed), FAMILIES.index(family), attempt]), seed)
        if conditions(ops) is None:
            return ops
    raise AssertionError(("no script", family, seed))


# ------------------------------------------------------------------------------------------------------------------------------- runner
class Mismatch(AssertionError):
    def __init__(self, family, seed, index, ops, field, ndiff, detail=None):
        self.family, self.seed, self.index, self.ops, self.field, self.ndiff = family, seed, index, ops, field, ndiff
        super().__init__(f"{family} seed {seed}: op {index} {ops[-1]}: {field}: {ndiff} differing cells {detail if detail is not None else ''}\n"
                         f"ops 0..{index}: {ops}\nreplay: callseq.replay({family!r}, {seed}, {index + 1})")


def points(dims, m, seed):
    """m points inside the box; the first one outside (clamped to the last cells)"""
    x = np.random.default_rng(seed).uniform(0, 1, (m, len(dims))).astype(f32) * np.array(dims, dtype=f32)
    x[0] = np.array(dims, dtype=f32) + 3
    return x


def rawbits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else (bits(a) if a.dtype == np.float32 else a)


def set_opt(h, name, v):
    """set_option, remembered on the handle: a toggle switches an option back to the value it had"""
    h.__dict__.setdefault("_options", {})[name] = int(v)
    h.set_option(name, int(v))


def apply(op, h, eager):
    """one op on one handle; what it returned (a list of arrays) for an observing op"""
    k = op[0]
    if k == "steps":
        if not eager:
            h.mom_step_() if op[1] == 0 else h.mom_steps_(op[1])
        else:
            for _ in range(max(op[1], 1)):      # the handle that is observed after every step
                h.mom_step_()
                h.field("p")
                h.field("u")
    elif k == "phase_step":
        for q in range(6):
            h.phase_(q)
    elif k == "read":
        return [h.field(n) for n in op[1]]
    elif k == "pois_level":
        return [h.pois_level(op[1])]
    elif k == "sample":
        return list(h.sample(points(h.dims, N_SAMPLES, op[1])))
    elif k == "flow_stats":
        return [np.array(h.flow_stats(), dtype=np.float64)]
    elif k == "metric":
        h.metric_sigma(op[1])      # into σ, CFL's scratch
        return [h.field("sigma")]
    elif k == "sgs":
        h.set_sgs(op[1])
    elif k == "forcing":
        h.set_forcing(ACC[:len(h.dims)] if op[1] else None)
    elif k == "set_dt_last":
        h.set_dt_last(f32(0.5) * f32(h.dt[-1]))
    elif k == "set_p":
        shape = h.shape("p")
        h.set_field("p", np.asfortranarray(np.random.default_rng(op[1]).uniform(-1, 1, size=shape).astype(f32)))      # non-zero ghost cells
    elif k == "set_u":
        u = h.field("u")
        h.set_field("u", np.asfortranarray(u + f32(1e-3) * np.random.default_rng(op[1]).uniform(-1, 1, size=u.shape).astype(f32)))
    elif k == "set_probes":
        h.set_probes(points(h.dims, N_PROBES, op[1]), PROBE_CAP)
    elif k == "clear_probes":
        h.set_probes(None, 0)
    elif k == "read_probes":
        counts = np.array(h.probe_counts(), dtype=np.int64)
        return [counts] + list(h.read_probes())
    elif k == "set_tracers":
        h.set_tracers(points(h.dims, N_TRACERS, op[1]))
    elif k == "tracers":
        return list(h.tracers())
    elif k in ("itmx", "resjac"):
        set_opt(h, k, op[1])
    elif k == "update":
        h.update_()
    elif k == "toggle":
        if not eager:      # the default handle alone: nothing is pending between calls, so an option may change there; switching on = the value it had
            held = h.__dict__.setdefault("_held", {})
            if op[2] == 0:
                held[op[1]] = h.__dict__.get("_options", {}).get(op[1], 1)      # never set: the library's default, 1 for every option toggled here
                set_opt(h, op[1], 0)
            else:
                set_opt(h, op[1], held.pop(op[1]))
    elif k == "measure":
        h.measure_(op[1])
    elif k == "touch_mu0":
        h.set_field("mu0", h.field("mu0"))      # the same values: handing the array out invalidates the masks
    elif k == "forces":
        return list(h.forces())
    else:
        raise ValueError(op)
    return None


def run(script, A, B, w, family=None, seed=None, upto=None):
    """every op on the default handle A and on the eager handle B (w: the package, None for fakes); compares after every observing op"""
    ops = script if upto is None else script[:upto]
    for i, op in enumerate(ops):
        ra, rb = apply(op, A, False), apply(op, B, True)
        if not observes(op):
            continue
        assert ra is not None and rb is not None and len(ra) == len(rb), (family, seed, i, op)
        for q, (x, y) in enumerate(zip(ra, rb)):
            x, y = rawbits(x), rawbits(y)
            if x.shape != y.shape or not np.array_equal(x, y):
                raise Mismatch(family, seed, i, ops[:i + 1], "result %d of %s" % (q, op[0]), int((x != y).sum()) if x.shape == y.shape else -1, (x.shape, y.shape))
        d = state_diff(A, B)
        if d is not None:
            raise Mismatch(family, seed, i, ops[:i + 1], *d)
    return A, B


# ---------------------------------------------------------------------------------------------------------------------- device handles
class Dev:
    """a FusedSimulation behind the method names the runner uses"""

    def __init__(self, w, sim, body_tile=None, case=None):
        self.w, self.sim, self.body_tile, self.case = w, sim, body_tile, case
        self.dims = sim.dims
        self.body = None
        for n in ("field", "set_field", "pois_level", "flow_stats", "set_probes", "set_option", "update_", "counter"):
            setattr(self, n, getattr(sim, n))

    dt = property(lambda self: self.sim.dt)
    pois_n = property(lambda self: self.sim.pois_n)

    def _lib(self):
        return self.w.lib()

    def _tile(self):
        if self.body_tile is not None:
            self.sim.set_option("body_tile", self.body_tile)      # process-wide: set for the handle that is about to run

    def shape(self, name):
        return self.sim._shape(name)

    def mom_step_(self):
        self._tile(); self.sim.mom_step_()

    def mom_steps_(self, k):
        self._tile(); self.sim.mom_steps_(k)

    def phase_(self, k):
        self._tile(); self.sim.phase_(k)

    def sample(self, x):
        u, p = self.sim.sample(x)
        return u.cpu().numpy(), p.cpu().numpy()

    def metric_sigma(self, name):
        self.sim.metric(name, out="sigma")
        self.sim.sync()

    def set_sgs(self, on):
        self.sim.set_sgs(0.17, 1.0) if on else self.sim.set_sgs(None)

    def set_forcing(self, acc):
        import ctypes as C
        from waterlily_jl_amd._lib import check
        a = None if acc is None else (C.c_float * 3)(*([float(v) for v in acc] + [0.0] * (3 - len(acc))))
        check(self._lib().wl_sim_set_forcing(self.sim._h, None, a, a))

    def set_dt_last(self, v):
        from waterlily_jl_amd._lib import check
        check(self._lib().wl_sim_set_dt_last(self.sim._h, float(v)))

    def probe_counts(self):
        return self.sim.counter("probe_records"), self.sim.counter("probe_dropped")

    def read_probes(self):
        return self.sim.read_probes()

    def set_tracers(self, x):
        self.sim.set_tracers(x)

    def tracers(self):
        x, x0 = self.sim.tracers()
        self.sim.sync()
        return x.cpu().numpy(), x0.cpu().numpy()

    def position(self, q):
        import bodypaths_ref as bp
        body = self.case["positions"][q][0]
        if self.case["remeasure_each_step"]:      # the translating sphere where it is now
            body = bp.moving_position(self.case["positions"][0][0], float(np.sum(self.sim.dt[:-1], dtype=np.float64)))
        return body

    def measure_(self, q):
        self.body = self.position(q)
        self.sim.measure_body_(self.body, 1.0)

    def forces(self):
        x0 = tuple(0.5 * n for n in self.dims)
        s = self.sim
        return s.pressure_force_body(self.body), s.viscous_force_body(self.body), s.pressure_moment_body(x0, self.body), s.viscous_moment_body(x0, self.body)


class CallerDev:
    """CallerOwnedSim (tests/test_gpu_callerowned.py: the Julia binding's call sequence, with a spare array) behind the same names; after every call
    wl_sim_field("p") must be the caller's array"""

    def __init__(self, w, sim):
        self.w, self.sim, self.dims = w, sim, tuple(n - 2 for n in sim.Ng)

    def _after(self):
        s = self.sim
        for role in s.role:
            s.role[role] = s._ptr2name[s.lib.wl_sim_field(s.h, role.encode())]
        assert s.lib.wl_sim_field(s.h, b"p") == self.w.core.ptr(s.arr["p"]).value, "the pressure is not in the caller's array"

    def _stream(self):
        from waterlily_jl_amd.core import stream
        return stream()

    def mom_step_(self):
        self.sim.check(self.sim.lib.wl_sim_mom_step(self.sim.h, self._stream())); self._after()

    def mom_steps_(self, k):
        self.sim.check(self.sim.lib.wl_sim_mom_steps(self.sim.h, int(k), self._stream())); self._after()

    def phase_(self, k):
        self.sim.check(self.sim.lib.wl_sim_phase(self.sim.h, int(k), self._stream())); self._after()

    def field(self, name):
        self._after()
        return self.sim.field(name)

    def set_sgs(self, on):
        self.sim.check(self.sim.lib.wl_sim_set_sgs(self.sim.h, 1 if on else 0, 0.17 if on else 0.0, 1.0)); self._after()

    def set_forcing(self, acc):
        import ctypes as C
        a = None if acc is None else (C.c_float * 3)(*([float(v) for v in acc] + [0.0] * (3 - len(acc))))
        self.sim.check(self.sim.lib.wl_sim_set_forcing(self.sim.h, None, a, a)); self._after()

    def set_dt_last(self, v):
        self.sim.check(self.sim.lib.wl_sim_set_dt_last(self.sim.h, float(v))); self._after()

    def set_option(self, name, v):
        self.sim.check(self.sim.lib.wl_sim_set_option(self.sim.h, name.encode(), int(v)))

    def counter(self, name):
        import ctypes as C
        v = C.c_long(0)
        self.sim.check(self.sim.lib.wl_sim_counter(self.sim.h, name.encode(), C.byref(v)))
        return int(v.value)

    def sample(self, x):
        import torch
        from waterlily_jl_amd.interp import _pp, points as dev_points
        x = dev_points(x, len(self.dims))
        n, D = x.shape[0], len(self.dims)
        u = torch.empty((n, D), dtype=torch.float32, device=x.device)
        p = torch.empty((n,), dtype=torch.float32, device=x.device)
        self.sim.check(self.sim.lib.wl_sim_sample(self.sim.h, _pp(x), n, _pp(u), _pp(p), self._stream())); self._after()
        return u.cpu().numpy(), p.cpu().numpy()

    @property
    def dt(self):
        import ctypes as C
        out = (C.c_float * 4096)()
        n = self.sim.lib.wl_sim_dt(self.sim.h, out, 4096)
        return [f32(v) for v in out[:n]]

    @property
    def pois_n(self):
        return self.sim.pois_n()

    def close(self):
        self.sim.close()


def make_one(family, w, eager, caller_eager=False, **caller_kw):
    """one handle of the family: the default one with the size gates opened, or the eager one.  The eager handle of the caller family is handle-owned, as make()
    pairs it; caller_eager: caller-owned with the deferrals off (tests/deadstore.py compares two handles of one kind).  caller_kw: further arguments of CallerOwnedSim"""
    if family in BODY_CASE:
        import bodypaths_ref as bp
        from test_gpu_bodypaths import handle
        case = next(c for c in bp.CASES if c["id"] == BODY_CASE[family])
        h = Dev(w, handle(w, case, dict(GATES, **EAGER, **EAGER_BODY)), 0, case) if eager else Dev(w, handle(w, case, dict(GATES, zsplit=2)), 1, case)
        h.measure_(0)
        return h
    dims = DIMS[family]
    if family in ("box", "caller"):
        u_init = np.asfortranarray(np.random.default_rng(137).uniform(-0.4, 0.4, size=tuple(n + 2 for n in dims) + (3,)).astype(f32))
        new = lambda: w.FusedSimulation(dims, UBC, dims[0], U=1, nu=0.02, u0=u_init)
    elif family == "ragged":
        new = lambda: w.FusedSimulation(dims, (0.0,) * 3, dims[0], U=1, nu=dims[0] / 1600.0, ic="tgv")
    else:
        new = lambda: w.FusedSimulation(dims, (0.0,) * 3, dims[0], U=1, nu=dims[0] / 1600.0, ic="tgv_periodic", perdir=(1, 3))
    if family == "caller" and (caller_eager or not eager):
        from test_gpu_callerowned import CallerOwnedSim
        h = CallerDev(w, CallerOwnedSim(w, dims, UBC, 0.02, u_init, caller_kw.pop("with_spare", True), **caller_kw))
    else:
        h = Dev(w, new())
    for k, v in (dict(GATES, **EAGER) if eager else GATES).items():
        set_opt(h, k, v)
    return h


def make(family, w):
    """(A, B): the default handle with the size gates opened, the eager handle"""
    if family in BODY_CASE:
        return make_one(family, w, False), make_one(family, w, True)
    B = make_one(family, w, True)
    return make_one(family, w, False), B


def replay(family, seed, upto=None, w=None):
    """run the first `upto` ops of script(family, seed) again on fresh handles (all of it by default); returns (A, B) for a closer look"""
    if w is None:
        import waterlily_jl_amd as w
        w.core.device()
    A, B = make(family, w)
    try:
        return run(script(family, seed), A, B, w, family, seed, upto)
    finally:
        w.lib().wl_reset_process_options()
