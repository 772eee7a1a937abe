"""What licenses tests/test_gpu_deadstore.py — no GPU.

The proof: for each family of tests/callseq.py, at a reduced size, the oracle run through deadstore.run — a clean Simulation next to one whose DEAD cells
(deadstore.DEAD: all of flow.f, the interior of flow.σ, of every level's r and ϵ and of the coarse levels' z, all of the coarse levels' x) are overwritten before
every call — is bit-identical, under quiet NaNs and under finite garbage.  A family whose oracle pair differed would be a wrong dead set, not a device bug.
Negative controls: the harness writes where it says — a NaN in ϵ's ghost layer changes the oracle's pois.n, a value in σ's lower ghost cells its Δt (those
layers are LIVE, which is why poison() leaves them alone).  The runner on pure-Python fakes: an honest one passes; one that accumulates into f without clearing
it, one that leaves the out-of-place buffer's ghost cells to the stale spare after a rotation, one that reads a coarse x before writing it are caught, each at the
call where it first differs.  σ's live ghost cells: on the oracle, at the sizes the device test uses, the planted value is above maximum(σ) of the clean run, the
planted cells keep it, and every Δt is inv(v + 5ν)."""
import numpy as np
import pytest

import callseq as cs
import deadstore as ds

f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------------------ the proof
@pytest.mark.parametrize("pattern", ds.PATTERNS)
@pytest.mark.parametrize("family", cs.FAMILIES)
def test_the_dead_set_is_dead_on_the_oracle(oracle, family, pattern):
    clean, dirty = ds.oracle_twin(oracle, family), ds.oracle_twin(oracle, family)
    assert clean.nlevels >= 3
    wrote = ds.run(clean, dirty, pattern, family)
    steps = sum(cs.nsteps(("steps", op[1])) if op[0] == "mom_steps" else 1 for op in ds.ops(family) if op[0] in ("mom_step", "mom_steps", "phase_step"))
    assert len(clean.dt) == 1 + steps == 8 and len(clean.pois_n) == 2 * steps
    # every poisoning wrote every entry of the dead set, and nothing else: the counts from the oracle's own extents
    Ng, D, L = clean.so.Ng, clean.so.D, clean.nlevels
    inner = lambda dims: int(np.prod([n - 2 for n in dims]))
    want = {("f", None): int(np.prod(Ng)) * D, ("sigma", None): inner(Ng)}
    for l in range(L):
        d = clean.so.level_dims(l)
        want[("r", l)] = want[("eps", l)] = inner(d)
        if l:
            want[("x", l)], want[("z", l)] = int(np.prod(d)), inner(d)
    assert len(wrote) == 4 and all(w == want for w in wrote), (wrote[0], want)


@pytest.mark.parametrize("pattern", ds.PATTERNS)
@pytest.mark.parametrize("family", ["box", "circle2d"])
def test_poison_writes_the_dead_cells_and_nothing_else(oracle, family, pattern):
    t = ds.oracle_twin(oracle, family)
    t.mom_step_()      # (arrays with content)
    flow = ("u", "u0", "f", "p", "sigma", "mu0") + (("V", "mu1") if family == "circle2d" else ())
    snap = lambda: {**{(n, None): np.array(t.so.field(n), order="F") for n in flow},
                    **{(n, l): np.array(t.so.level_field(n, l), order="F") for l in range(t.nlevels) for n in ("L", "D", "iD", "x", "eps", "r", "z") if l or n not in ("L", "x", "z")}}      # (the finest L, x, z are flow.μ₀, p, σ)
    before = snap()
    ds.poison(t, pattern, False, 4)
    assert all(np.array_equal(cs.bits(v), cs.bits(before[k])) for k, v in snap().items())      # the clean twin's form writes nothing
    ds.poison(t, pattern, True, 4)
    dead = {(n, l): c for n, l, c in ds.dead_entries(t.nlevels, False)}
    for k, v in snap().items():
        if k not in dead:
            assert np.array_equal(cs.bits(v), cs.bits(before[k])), k
            continue
        want = ds.values(pattern, v.shape, k + (4,))
        g = ds.ghost_mask(v.shape) if dead[k] == "interior" else np.zeros(v.shape, dtype=bool)
        assert np.array_equal(cs.bits(v)[~g], cs.bits(want)[~g]) and np.array_equal(cs.bits(v)[g], cs.bits(before[k])[g]), k
    assert set(dead) <= set(before)


def test_the_patterns():
    a = ds.values("nan", (5, 4, 3), 0)
    assert a.flags.f_contiguous and a.dtype == f32 and (cs.bits(a) == 0x7FC00000).all() and np.isnan(a).all()
    b, c = ds.values("garbage", (5, 4, 3), ("f", None, 0)), ds.values("garbage", (5, 4, 3), ("f", None, 2))
    assert np.isfinite(b).all() and np.abs(b).max() <= 1e3 and np.abs(b).max() > 500 and len(np.unique(b)) == b.size      # a field, not a constant
    assert np.array_equal(b, ds.values("garbage", (5, 4, 3), ("f", None, 0))) and not np.array_equal(b, c)
    base = np.arange(60, dtype=f32).reshape((5, 4, 3), order="F")
    m = ds.interior_of(b, base)
    g = ds.ghost_mask(base.shape)
    assert np.array_equal(m[g], base[g]) and np.array_equal(m[~g], b[~g]) and int((~g).sum()) == 3 * 2 * 1
    assert ds.word("nan") == 0x7FC00000 and np.array([ds.word("garbage")], dtype=np.uint32).view(f32)[0] == f32(-777.25)


# --------------------------------------------------------------------------------------------------------------------- negative controls
def test_control_nan_in_the_ghost_layer_of_eps_changes_pois_n(oracle):
    """ϵ's ghost cells are live: they are multiplied by L = 0, which stops a finite value and not a NaN"""
    clean, dirty, finite = (ds.oracle_twin(oracle, "box") for _ in range(3))
    for t, pattern in ((dirty, "nan"), (finite, "garbage")):
        slot = t.open("eps", 0)
        a = slot.read()
        g = ds.ghost_mask(a.shape)
        a[g] = ds.values(pattern, a.shape, 0)[g]
        slot.write(a)
    for t in (clean, dirty, finite):
        t.mom_step_()
    assert dirty.pois_n != clean.pois_n and max(dirty.pois_n) == 32, (clean.pois_n, dirty.pois_n)
    assert cs.state_diff(clean, finite) is None


@pytest.mark.parametrize("family", ["box", "circle2d"])
def test_control_a_value_in_the_lower_ghost_cells_of_sigma_changes_dt(oracle, family):
    clean, dirty = ds.oracle_twin(oracle, family), ds.oracle_twin(oracle, family)
    s = dirty.field("sigma")
    low = np.zeros(s.shape, dtype=bool)
    for a in range(s.ndim):
        low[(slice(None),) * a + (0,)] = True
    s[low] = ds.SIGMA_VALUE
    dirty.set_sigma(s)
    for t in (clean, dirty):
        t.mom_steps_(2)
    assert [cs.bits(v).item() for v in dirty.dt[1:]] == [cs.bits(ds.dt_planted(dirty.so.nu)).item()] * 2 and clean.dt[1] > 3 * dirty.dt[1]
    assert (dirty.field("sigma")[low] == ds.SIGMA_VALUE).all()      # nothing ever writes them again


# ------------------------------------------------------------------------------------------------------------------------------ the fakes
class Fake:
    """a toy flow on 1-D arrays with one ghost cell at either end, with the arrays and the dead set of the real thing: f (every cell written before it is read),
    σ (interior written, ghost cells live), three levels of r, ϵ, x, z, and a spare velocity buffer the corrector writes out of place"""
    is_handle, nlevels, N = True, 3, (10, 6, 4)

    def __init__(self):
        n = self.N[0]
        rng = np.random.default_rng(3)
        self.a = {"u": rng.uniform(-1, 1, n).astype(f32), "f": np.zeros(n, f32), "us": np.zeros(n, f32), "sigma": np.zeros(n, f32), "p": np.zeros(n, f32)}
        self.a["u"][[0, -1]] = f32(0.5)
        self.a["u0"] = self.a["u"].copy()
        self.lv = [{k: np.zeros(m, f32) for k in ("r", "eps", "x", "z")} for m in self.N]
        self.lv[0]["x"], self.lv[0]["z"] = self.a["p"], self.a["sigma"]
        self.dt, self.pois_n = [f32(0.25)], []
        self.path = None      # which call is running: the broken fakes are broken on one path each

    # ---- the names the runner and poison() use
    def field(self, name):
        return self.a[name].copy()

    def open(self, name, level):
        v = self.a[name] if level is None else self.lv[level][name]

        def write(a):
            v[...] = a
        return ds.Slot(v.shape, v.copy, write)

    def scratch(self, bits, regions=None):
        return None

    # ---- elementary operations
    def conv(self, uadv):
        f = self.a["f"]
        f[:] = 0                                      # every cell of f is written before it is read
        self.accumulate(f, uadv)

    def accumulate(self, f, uadv):
        f[1:-1] += f32(0.25) * (uadv[2:] - uadv[:-2]) * uadv[1:-1]
        f[[0, -1]] += uadv[[0, -1]]

    def bc(self, u):
        u[[0, -1]] = f32(0.5)

    def predict(self):
        u, u0 = self.a["u"], self.a["u0"]
        self.conv(u0)
        u[1:-1] = u0[1:-1] + self.dt[-1] * self.a["f"][1:-1]
        self.bc(u)

    def fill_x(self, x):
        x[:] = 0                                      # fill!(coarse.x, 0): ghost cells included

    def project(self, w):
        u, p, s = self.a["u"], self.a["p"], self.a["sigma"]
        s[1:-1] = u[1:-1] - u[:-2]                    # z = div(u): σ's interior
        l0 = self.lv[0]
        l0["r"][1:-1] = s[1:-1] - (2 * p[1:-1] - p[2:] - p[:-2]) * f32(w)
        l0["eps"][1:-1] = f32(0.5) * l0["r"][1:-1]
        fine = l0
        for c in self.lv[1:]:
            c["r"][1:-1] = fine["r"][1:-1:2] + fine["r"][2:-1:2]
            c["z"][1:-1] = c["r"][1:-1]
            self.fill_x(c["x"])
            c["eps"][1:-1] = f32(0.25) * c["z"][1:-1]
            c["x"][1:-1] += c["eps"][1:-1]
            fine = c
        for q in range(len(self.lv) - 1, 0, -1):
            c, fine = self.lv[q], self.lv[q - 1]
            up = np.repeat(c["x"][1:-1], 2)
            if q > 1:
                fine["x"][1:-1] += up
            else:
                p[1:-1] += up + fine["eps"][1:-1]
        u[1:-1] -= f32(0.1) * (p[2:] - p[1:-1])
        self.pois_n.append(2 if w == 1 else 1)

    def correct(self):
        u, u0, us = self.a["u"], self.a["u0"], self.a["us"]
        self.conv(u)
        us[1:-1] = f32(0.5) * (u0[1:-1] + u[1:-1] + self.dt[-1] * self.a["f"][1:-1])      # out of place, then the buffers trade places
        self.finish_rotation(us)
        self.a["u"], self.a["us"] = us, u

    def finish_rotation(self, us):
        self.bc(us)

    def cfl(self):
        s, u = self.a["sigma"], self.a["u"]
        s[1:-1] = np.abs(u[1:-1])
        s[-1] = np.abs(u[-2])                         # the upper ghost cell keeps a stale flux; the lower one is never written
        self.dt.append(f32(1) / (s.max() + f32(0.5)))

    def step(self):
        self.a["u0"][:] = self.a["u"]
        self.predict(); self.project(1); self.correct(); self.project(0.5); self.cfl()

    def mom_step_(self):
        self.path = "single"
        self.step()

    def mom_steps_(self, k):
        self.path = "multi"
        for _ in range(k):
            self.step()

    def phase_(self, q):
        self.path = "phases"
        if q == 0:
            self.a["u0"][:] = self.a["u"]
        else:
            (self.predict, lambda: self.project(1), self.correct, lambda: self.project(0.5), self.cfl)[q - 1]()


class AccumulatesIntoF(Fake):
    """the staged sequence (here: the step taken as phases) adds conv_diff!'s result to f without clearing it first"""

    def conv(self, uadv):
        if self.path != "phases":
            return super().conv(uadv)
        self.accumulate(self.a["f"], uadv)


class StaleGhostsAfterRotation(Fake):
    """in a multi-step call the corrector leaves the ghost cells of the out-of-place buffer to what the spare held"""

    def finish_rotation(self, us):
        if self.path != "multi":
            super().finish_rotation(us)


class ReadsCoarseXFirst(Fake):
    """x = ω·ϵ became x += ω·ϵ with nobody clearing x: right only while the coarse x starts as zeros"""

    def fill_x(self, x):
        pass


def _first(kind):
    return next(i for i, op in enumerate(ds.ops("box")) if op[0] == kind)


BROKEN = [(AccumulatesIntoF, _first("phase_step")), (StaleGhostsAfterRotation, _first("mom_steps")), (ReadsCoarseXFirst, _first("mom_step"))]


@pytest.mark.parametrize("pattern", ds.PATTERNS)
def test_the_honest_fake_passes(pattern):
    a, b = Fake(), Fake()
    wrote = ds.run(a, b, pattern, "box")
    assert len(a.dt) == 8 and all(np.isfinite(a.field(n)).all() for n in ("u", "u0", "p"))
    assert wrote[0] == {("f", None): 10, ("sigma", None): 8, ("r", 0): 8, ("eps", 0): 8, ("r", 1): 4, ("eps", 1): 4, ("r", 2): 2, ("eps", 2): 2, ("x", 1): 6, ("x", 2): 4,
                        ("z", 1): 4, ("z", 2): 2, ("us", None): 10}
    assert not np.array_equal(a.field("u"), Fake().field("u"))


@pytest.mark.parametrize("pattern", ds.PATTERNS)
@pytest.mark.parametrize("fake,at", BROKEN, ids=[f.__name__ for f, _ in BROKEN])
def test_broken_fakes_are_caught_at_the_call_where_they_first_differ(fake, at, pattern):
    with pytest.raises(ds.DeadRead) as e:
        ds.run(fake(), fake(), pattern, "box")
    assert e.value.index == at and e.value.op == ds.ops("box")[at] and e.value.pattern == pattern, (e.value.index, at, str(e.value))


# ------------------------------------------------------------------------------------------------------------- σ's live ghost cells
@pytest.mark.parametrize("family", ds.SIGMA_LIVE)
def test_sigma_planted_value_dominates_and_stays_on_the_oracle(oracle, family):
    """at the size the device test runs: the value is above maximum(σ) of the clean run over the six steps, the three cells keep it, every Δt is inv(v + 5ν)"""
    clean, planted = ds.oracle_twin(oracle, family, full=True), ds.oracle_twin(oracle, family, full=True)
    cells = ds.plant(planted)
    shape = planted.field("sigma").shape
    assert len(set(cells)) == 3 and [sum(c == 0 for c in cell) for cell in cells] == [1, len(shape) - 1, len(shape)] and all(ds.ghost_mask(shape)[c] for c in cells)
    top = 0.0
    for _ in range(6):
        clean.mom_step_(); planted.mom_step_()
        top = max(top, float(clean.field("sigma").max()))
        s = planted.field("sigma")
        assert all(s[c] == ds.SIGMA_VALUE for c in cells)
        s[tuple(np.array(cells).T)] = 0
        assert float(s.max()) < float(ds.SIGMA_VALUE) / 2      # … and in the planted run itself nothing else comes near it
    print(f"{family} {clean.so.dims}: maximum(σ) of the clean run {top:.4f} < {float(ds.SIGMA_VALUE)}; Δt clean {float(clean.dt[-1]):.4f}, planted {float(planted.dt[-1]):.8f}")
    assert top < float(ds.SIGMA_VALUE) / 2
    want = cs.bits(ds.dt_planted(planted.so.nu)).item()
    assert [cs.bits(v).item() for v in planted.dt[1:]] == [want] * 6
