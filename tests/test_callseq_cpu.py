"""The conditions that keep the randomised call-sequence test (tests/callseq.py, tests/test_gpu_callseq.py) from being hollow — no GPU.

The scripts are deterministic, long enough, hold the adjacencies the test is there for, and over the seeds the GPU test runs every op kind of a family occurs
more than once.  A pure-Python FakeSim with the method names the runner uses — its state a running hash of the elementary operations applied, each hashed
with the mutable settings in force — passes run() for every family and seed: the default handle's expansion of a script (one mom_steps_(k) per step op) and
the eager handle's (k × mom_step_, p and u read after each) are the same sequence of elementary operations.  Three fakes that are broken the way a deferral can
be broken make run() fail, at the op where the damage first becomes observable."""
import hashlib
from collections import Counter

import numpy as np
import pytest

import callseq as cs

f32 = np.float32
ALL = [(f, s) for f in cs.FAMILIES for s in cs.SEEDS]


def H(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(p if isinstance(p, bytes) else repr(p).encode())
        h.update(b"|")
    return h.digest()


def arr(digest, shape=(8,)):
    """finite float32 values of a digest"""
    n = int(np.prod(shape))
    raw = b"".join(H(digest, q) for q in range((4 * n + 31) // 32))
    return (np.frombuffer(raw[:4 * n], dtype=np.uint32) % (1 << 20)).astype(f32).reshape(shape) / f32(1 << 20)


class FakeSim:
    """option names that select code and not results (the deferrals, the size gates, the body shortcuts) are accepted and ignored — as the library promises"""
    dims = (4, 4, 4)
    RESULT_OPTIONS = ("itmx",)

    def __init__(self):
        self.h = H("init")                 # the flow: u, u⁰ and everything a step reads but p
        self.hp = H("p0")                  # the pressure
        self.hu0 = self.h
        self.hsig = H("sigma0")
        self.dt = [f32(0.25)]
        self.pois_n = []
        self.settings = {"sgs": 0, "forcing": None, "itmx": 32}
        self.probes, self.records, self.dropped = None, [], 0
        self.tr = None
        self.multi = False                 # the last stepping call was a multi-step one (what the broken fakes key on)

    def _set(self):
        return tuple(sorted(self.settings.items()))

    # ---- elementary operations
    def _step(self):
        self.hu0 = self.h
        self.h = H("step", self.h, self.hp, self._set(), self.dt[-1].tobytes())
        self.hp, self.hsig = H("p", self.h), H("sigma", self.h)
        self.pois_n += [1 + self.h[0] % 30, 1 + self.h[1] % 30]
        self._observe()
        self.dt.append(f32(0.1) + f32(self.h[2]) / f32(1024))

    def _observe(self):
        if self.probes is not None:
            if len(self.records) == self.cap:
                self.dropped += 1
            else:
                self.records.append((len(self.dt) - 1, H("rec", self.probes, self.h, self.hp)))
        if self.tr is not None:
            self.tr = (H("adv", self.tr[0], self.hu0, self.h, self.dt[-1].tobytes()), self.tr[0])

    def mom_step_(self):
        self.multi = False
        self._step()

    def mom_steps_(self, k):
        self.multi = k >= 2
        for _ in range(k):
            self._step()

    def phase_(self, k):
        self.multi = False
        if k == 0:
            self.hu0 = self.h
        self.h = H("phase", k, self.h, self.hp, self._set(), self.dt[-1].tobytes())
        if k in (2, 4):
            self.hp = H("p", self.h)
            self.pois_n.append(1 + self.h[0] % 30)
        if k in (1, 3):
            self.hsig = H("sigma", self.h)
        if k == 5:
            self.dt.append(f32(0.1) + f32(self.h[2]) / f32(1024))

    # ---- observers
    def shape(self, name):
        return (4, 4, 4) if name in ("p", "sigma") else (4, 4, 4, 3)

    def field(self, name):
        src = {"u": self.h, "u0": self.hu0, "p": self.hp, "sigma": self.hsig, "mu0": H("mu0", self.settings.get("body"))}[name]
        return arr(H(name, src), self.shape(name))

    def pois_level(self, name):
        return arr(H("level", name, self.h, self.hp))

    def sample(self, x):
        return arr(H("su", x.tobytes(), self.h)), arr(H("sp", x.tobytes(), self.hp))

    def flow_stats(self):
        return tuple(float(v) for v in arr(H("stats", self.h), (3,)))

    def metric_sigma(self, name):
        self.hsig = H("metric", name, self.h)

    def probe_counts(self):
        return len(self.records), self.dropped

    def read_probes(self):
        rec, self.records = self.records, []
        t = np.array([float(np.sum(np.asarray(self.dt[:q + 1], dtype=f32), dtype=f32)) for q, _ in rec], dtype=np.float64)
        return t, np.stack([arr(r) for _, r in rec]) if rec else np.zeros((0, 8), f32), np.zeros((len(rec),), f32)

    def tracers(self):
        return arr(self.tr[0]), arr(self.tr[1])

    def forces(self):
        return tuple(arr(H("force", q, self.h, self.hp, self.settings.get("body")), (3,)).astype(np.float64) for q in range(4))

    # ---- mutators
    def set_field(self, name, a):
        if name == "p":
            self.hp = H("set_p", np.ascontiguousarray(a).tobytes())
        elif name == "u":
            self.h = H("set_u", np.ascontiguousarray(a).tobytes())
        else:
            assert name == "mu0"      # the same values: nothing a step computes changes

    def set_sgs(self, on):
        self.settings["sgs"] = int(on)

    def set_forcing(self, acc):
        self.settings["forcing"] = None if acc is None else tuple(acc)

    def set_dt_last(self, v):
        self.dt[-1] = f32(v)

    def set_probes(self, x, cap):
        self.probes, self.cap, self.records, self.dropped = (None if x is None else x.tobytes()), cap, [], 0

    def set_tracers(self, x):
        self.tr = (H("tr", x.tobytes()),) * 2

    def set_option(self, name, v):
        if name in self.RESULT_OPTIONS:
            self.settings[name] = int(v)

    def update_(self):
        pass

    def measure_(self, q):
        self.settings["body"] = (q, float(np.sum(self.dt[:-1], dtype=np.float64)))


class DropsDtLast(FakeSim):
    """Δt[end] set by the host is lost when the next call is a multi-step one (a Δt kept on the device that the call does not refresh)"""

    def __init__(self):
        super().__init__()
        self.before = None

    def set_dt_last(self, v):
        self.before = self.dt[-1]
        super().set_dt_last(v)

    def _step(self):
        super()._step()
        self.before = None

    def phase_(self, k):
        super().phase_(k)
        self.before = None

    def mom_steps_(self, k):
        if k >= 2 and self.before is not None:
            self.dt[-1] = self.before
        super().mom_steps_(k)


class StalePAfterMulti(FakeSim):
    """after a multi-step call the pressure handed out is the one of the step before the last (the wrong array of the pair)"""

    def _step(self):
        self.hp_prev = self.hp
        super()._step()

    def field(self, name):
        if name == "p" and self.multi:
            keep, self.hp = self.hp, self.hp_prev
            try:
                return super().field(name)
            finally:
                self.hp = keep
        return super().field(name)

    def set_field(self, name, a):
        super().set_field(name, a)
        if name == "p":
            self.multi = False


class ForgetsTracerStep(FakeSim):
    """the tracers miss the last step of a multi-step call"""

    def mom_steps_(self, k):
        self.multi = k >= 2
        for q in range(k):
            keep = self.tr
            self._step()
            if k >= 2 and q == k - 1:
                self.tr = keep


# where each broken fake first becomes observable, from the script alone
def first_observer_from(ops, q):
    return next(r for r in range(q, len(ops)) if cs.observes(ops[r]))


def expect_drops_dt_last(ops):
    pending = False
    for q, op in enumerate(ops):
        if op[0] == "set_dt_last":
            pending = True
        elif op[0] in cs.STEPPERS:
            if pending and op[0] == "steps" and op[1] >= 2:
                return first_observer_from(ops, q)
            pending = False
    return None


def expect_stale_p(ops):
    for q, op in enumerate(ops):
        if op[0] == "steps" and op[1] >= 2:
            for r in range(q + 1, len(ops)):
                if cs.observes(ops[r]):
                    return r
                if ops[r][0] in cs.STEPPERS + ("set_p",):
                    break
    return None


def expect_tracer(ops):
    live = hit = False
    for q, op in enumerate(ops):
        if op[0] == "set_tracers":
            live, hit = True, False
        elif live and op[0] == "steps" and op[1] >= 2:
            hit = True
        elif op[0] == "tracers" and hit:
            return q
    return None


# -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,seed", ALL)
def test_scripts_are_deterministic_and_not_hollow(family, seed):
    ops = cs.script(family, seed)
    assert ops == cs.script(family, seed)
    assert all(isinstance(op, tuple) for op in ops)
    total = sum(cs.nsteps(op) for op in ops)
    assert 12 <= total <= 40 and len(ops) <= 45, (total, len(ops))
    assert any(a[0] == "steps" and a[1] >= 2 and cs.observes(b) for a, b in zip(ops, ops[1:]))
    st = [q for q, op in enumerate(ops) if op[0] in cs.STEPPERS]
    assert any(any(cs.mutates(ops[q]) for q in range(a + 1, b)) for a, b in zip(st, st[1:]))
    assert cs.conditions(ops) is None
    assert all(op[1] in (0, 1, 2, 3, 4) for op in ops if op[0] == "steps")
    assert cs.observes(ops[-1])      # every script ends on a comparison
    if family != "caller":
        # the adjacencies of the issue: Δt[end] changed before a multi-step call; a full probe buffer; a multi-step call under tracers
        assert expect_drops_dt_last(ops) is not None and expect_tracer(ops) is not None
        a, b = ops.index(("read_probes",)), next(q for q, op in enumerate(ops) if op[0] == "set_probes")
        assert sum(cs.nsteps(op) for op in ops[b:a] if op[0] == "steps") > cs.PROBE_CAP
    assert cs.script(family, seed) != cs.script(family, seed + 100)


# what each family has to exercise, spelt out here (not derived from the generator): every kind at least twice over the seeds
COMMON = {"steps", "phase_step", "read", "pois_level:r", "pois_level:x", "sample", "flow_stats", "metric:ke", "forcing:1", "forcing:0", "set_dt_last", "set_p", "set_u",
          "set_probes", "read_probes", "clear_probes", "set_tracers", "tracers", "itmx:1", "itmx:2", "itmx:32", "resjac:3", "resjac:1", "update"}
THREE_D = {"metric:omega_mag", "metric:lambda2", "sgs:1", "sgs:0"}
BODY = {"measure", "touch_mu0", "forces"}
EXPECTED = {"box": COMMON | THREE_D, "ragged": COMMON | THREE_D, "periodic": COMMON | THREE_D, "moving": COMMON | THREE_D | BODY, "exit": COMMON | THREE_D | BODY,
            "circle2d": COMMON | BODY, "caller": {"steps", "read", "sample", "set_dt_last", "sgs:1", "sgs:0"}}


@pytest.mark.parametrize("family", cs.FAMILIES)
def test_every_op_kind_occurs_at_least_twice_over_the_seeds(family):
    seen = Counter(cs.kind(op) for s in cs.SEEDS for op in cs.script(family, s))
    assert all(seen[k] >= 2 for k in EXPECTED[family]), {k: seen[k] for k in EXPECTED[family] if seen[k] < 2}
    toggles = {k: n for k, n in seen.items() if k.startswith("toggle:")}
    assert set(seen) - set(toggles) == EXPECTED[family], set(seen) ^ (EXPECTED[family] | set(toggles))      # and nothing the family cannot express
    off, on = {k.split(":")[1] for k in toggles if k.endswith(":0")}, {k.split(":")[1] for k in toggles if k.endswith(":1")}
    assert off == on
    if family == "caller":
        assert not toggles
    elif family in cs.BODY_CASE:      # one toggle per script: the body shortcuts and the deferrals that stay live next to a body, each once
        assert off == set(cs.BODY_TOGGLES) and sum(toggles.values()) == 12
    else:                             # two per script: every deferral is switched off and on again in each of these families
        assert off == set(cs.DEFERRALS) and sum(toggles.values()) == 24
    ks = Counter(op[1] for s in cs.SEEDS for op in cs.script(family, s) if op[0] == "steps")
    assert all(ks[k] >= 2 for k in range(5)), ks


class Records(FakeSim):
    def __init__(self):
        super().__init__()
        self.calls = []

    def set_option(self, name, v):
        self.calls.append((name, v))


def test_a_toggle_switches_back_to_the_value_the_option_had():
    A, B = Records(), Records()
    cs.set_opt(A, "tailwide", 0)      # off before the script starts: the toggle must not switch it on
    cs.run([("toggle", "tailwide", 0), ("toggle", "tailwide", 1), ("toggle", "rskip", 0), ("toggle", "rskip", 1)], A, B, None, "box", 0)
    assert A.calls == [("tailwide", 0), ("tailwide", 0), ("tailwide", 0), ("rskip", 0), ("rskip", 1)] and B.calls == []


@pytest.mark.parametrize("family,seed", ALL)
def test_both_expansions_are_the_same_elementary_operations(family, seed):
    A, B = FakeSim(), FakeSim()
    cs.run(cs.script(family, seed), A, B, None, family, seed)
    assert A.h == B.h and A.dt == B.dt and len(A.dt) == 1 + sum(cs.nsteps(op) for op in cs.script(family, seed))


def test_the_fake_notices_a_setting():
    """the hash is of operations AND settings: the same calls with the iteration cap changed on one handle alone do not compare equal"""
    A, B = FakeSim(), FakeSim()
    B.set_option("itmx", 2)
    with pytest.raises(cs.Mismatch) as e:
        cs.run([("steps", 1), ("read", ("u",))], A, B, None, "box", 0)
    assert e.value.index == 1 and e.value.field == "result 0 of read" and "replay" in str(e.value) and "('steps', 1)" in str(e.value)


BROKEN = [(DropsDtLast, expect_drops_dt_last), (StalePAfterMulti, expect_stale_p), (ForgetsTracerStep, expect_tracer)]


@pytest.mark.parametrize("fake,expect", BROKEN, ids=[f.__name__ for f, _ in BROKEN])
def test_broken_fakes_fail_at_the_right_op(fake, expect):
    hits = Counter()
    for family, seed in ALL:
        ops = cs.script(family, seed)
        at = expect(ops)
        if at is None:      # the sequence that shows this fault is not in the script (the caller family has no tracers)
            cs.run(ops, fake(), fake(), None, family, seed)
            continue
        with pytest.raises(cs.Mismatch) as e:
            cs.run(ops, fake(), fake(), None, family, seed)
        assert e.value.index == at and e.value.family == family and e.value.seed == seed, (family, seed, e.value.index, at)
        assert e.value.ops == ops[:at + 1]
        hits[family] += 1
    # every family that has the op is caught on several seeds
    for family in cs.FAMILIES:
        if family != "caller" or fake is not ForgetsTracerStep:
            assert hits[family] >= 2, (fake.__name__, dict(hits))
