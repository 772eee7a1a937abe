"""Poisoned scratch (test infrastructure; imports without a GPU): no dead cell and no spare buffer may decide a bit.

Every array the library owns starts as zeros, and so did every caller-owned array of the suite — the Julia binding hands wl_sim_desc.us a `similar(a.u)`,
uninitialised memory.  A kernel that reads a cell the reference overwrites first gets the right number only because that memory was 0.  Here the DEAD set — the
cells the reference (oracle/) provably never reads before it writes them — is data; poison(twin, pattern) overwrites exactly those cells, through the pointers the
public API hands out, with quiet NaNs or with a seeded field of finite garbage, and run() steps a poisoned twin next to a clean one: u, u⁰, p on every cell as raw
bits, pois.n, the Δt history and σ's ghost cells must stay equal after every call, and every value of u, u⁰, p finite.

tests/test_deadstore_cpu.py proves the dead set on the oracle (the condition that licenses the device test), shows that the harness writes where it says, and runs
the runner on pure-Python fakes; tests/test_gpu_deadstore.py runs it on the handles of tests/callseq.py.  The second half of this file is a second thing nobody
tested at handle level: σ's LIVE ghost cells — CFL's maximum(σ) sees them for good — against the oracle."""
import zlib

import numpy as np

import callseq as cs

f32 = np.float32
NAN_BITS = 0x7FC00000                            # the quiet NaN
PATTERNS = ("nan", "garbage")
GARBAGE_WORD = int(f32(-777.25).view(np.uint32))      # the one word the scratch hook takes under "garbage" (the arrays get a field: a wrong cell cannot cancel)

# (array, levels, cells): levels None — a Flow array; "every" — each level's; "coarse" — every level but the finest (whose x, z are flow.p, flow.σ).
# cells "all" — ghosts included; "interior" — the ghost layer is LIVE (ϵ's and σ's are read) or rests on an invariant of its own, and is left alone
DEAD = (("f", None, "all"), ("sigma", None, "interior"), ("r", "every", "interior"), ("eps", "every", "interior"), ("x", "coarse", "all"), ("z", "coarse", "interior"))
# what a handle adds: the spare velocity array (every cell) and, through wl_sim_scratch_fill, the scratch no entry point reaches (include/wlhip_bench.h lists it)
HANDLE_DEAD = (("us", None, "all"),)
VECTOR = ("f", "us")                             # (Ng..., D) arrays; every other one is (Ng...)


def interior(shape):
    return tuple(slice(1, n - 1) for n in shape)


def ghost_mask(shape):
    m = np.ones(shape, dtype=bool)
    m[interior(shape)] = False
    return m


def interior_of(v, base):
    """base with its interior cells replaced by v's (scalar arrays: every axis is a spatial one)"""
    out = np.array(base, dtype=f32, order="F")
    out[interior(out.shape)] = v[interior(out.shape)]
    return out


def values(pattern, shape, salt):
    """the pattern as a Fortran-ordered float32 array; garbage is seeded by `salt` (array, level, call): another field at every poisoning"""
    if pattern == "nan":
        return np.asfortranarray(np.full(shape, NAN_BITS, dtype=np.uint32).view(f32))
    assert pattern == "garbage", pattern
    rng = np.random.default_rng(zlib.crc32(repr(salt).encode()))
    return np.asfortranarray(rng.uniform(-1e3, 1e3, size=shape).astype(f32))


def word(pattern):
    return NAN_BITS if pattern == "nan" else GARBAGE_WORD


def dead_entries(nlevels, handle):
    for name, levels, cells in DEAD + (HANDLE_DEAD if handle else ()):
        if levels is None:
            yield name, None, cells
        else:
            for l in range(0 if levels == "every" else 1, nlevels):
                yield name, l, cells


class Slot:
    """one array as a getter handed it out: its extents (from the handle or the oracle), a read and a write of the WHOLE array"""

    def __init__(self, shape, read, write):
        self.shape, self.read, self.write = tuple(shape), read, write


SCRATCH_REGIONS = {"ps": 1, "em_rs": 2, "W": 4, "partials": 8, "force_bands": 16}      # wl_sim_scratch_fill_regions


def poison(t, pattern, write=True, salt=0, only=None):
    """the dead cells of twin t <- pattern.  write=False (the clean twin): the same getter calls — wl_mg_level_field(…,"r") settles a skipped store — and the scratch
    hook's keeping form; nothing is written.  only: a set of array names and SCRATCH_REGIONS — nothing else is written (for finding which array a difference
    comes from; the getter calls stay).  Returns the cells written per (array, level)"""
    done = {}
    for name, level, cells in dead_entries(t.nlevels, t.is_handle):
        slot = t.open(name, level)
        if slot is None or not write or (only is not None and name not in only):      # (None: no spare array on this handle)
            continue
        v = values(pattern, slot.shape, (name, level, salt))
        if cells == "all":
            slot.write(v)
            done[(name, level)] = int(np.prod(slot.shape))
        else:
            assert name not in VECTOR
            slot.write(interior_of(v, slot.read()))      # the ghost layer goes back as it was read
            done[(name, level)] = int(np.prod([n - 2 for n in slot.shape]))
    regions = None if only is None else sum(v for k, v in SCRATCH_REGIONS.items() if k in only)
    n = t.scratch(word(pattern) if write else None, regions)
    if n is not None:
        done[("scratch", None)] = n
    return done


# ------------------------------------------------------------------------------------------------------------------------------- runner
class DeadRead(AssertionError):
    def __init__(self, family, pattern, index, op, detail):
        self.family, self.pattern, self.index, self.op, self.detail = family, pattern, index, op, detail
        super().__init__(f"{family}, {pattern}: op {index} {op}: the poisoned twin differs from the clean one: {detail}")


def ops(family):
    """poison; mom_step; poison; mom_steps(3); poison; a full step by phases; [a body: measure!]; poison; mom_steps(2)"""
    body = family in cs.BODY_CASE
    return [("poison",), ("mom_step",), ("poison",), ("mom_steps", 3), ("poison",), ("phase_step",)] + ([("measure", 1)] if body else []) + [("poison",), ("mom_steps", 2)]


def check(clean, dirty, what):
    cs.assert_same_state(clean, dirty, what)
    a, b = clean.field("sigma"), dirty.field("sigma")
    g = ghost_mask(a.shape)
    nd = int((cs.bits(a)[g] != cs.bits(b)[g]).sum())
    assert nd == 0, (what, "ghost cells of sigma", nd)
    for h, who in ((clean, "clean"), (dirty, "poisoned")):
        for name in ("u", "u0", "p"):
            v = h.field(name)
            assert np.isfinite(v).all(), (what, who, name, "not finite", int((~np.isfinite(v)).sum()))


def apply(op, t):
    k = op[0]
    if k == "mom_step":
        t.mom_step_()
    elif k == "mom_steps":
        t.mom_steps_(op[1])
    elif k == "phase_step":
        for q in range(6):
            t.phase_(q)
    elif k == "measure":
        t.measure_(op[1])
    else:
        raise ValueError(op)


def run(clean, dirty, pattern, family, only=None):
    """the two twins through ops(family); raises DeadRead at the first call after which they differ.  Returns what each poisoning wrote"""
    wrote = []
    for i, op in enumerate(ops(family)):
        if op[0] == "poison":
            poison(clean, pattern, False, i, only)
            wrote.append(poison(dirty, pattern, True, i, only))
            continue
        apply(op, clean)
        apply(op, dirty)
        try:
            check(clean, dirty, (family, pattern, i, op))
        except AssertionError as e:
            raise DeadRead(family, pattern, i, op, e.args) from None
    return wrote


# ----------------------------------------------------------------------------------------------------------------------------- the twins
class OracleTwin:
    """an oracle.Simulation behind the names the runner and poison() use"""
    is_handle = False

    def __init__(self, so, case=None):
        self.so, self.case = so, case

    nlevels = property(lambda self: self.so.nlevels)
    pois_n = property(lambda self: self.so.pois_n)
    dt = property(lambda self: [f32(v) for v in self.so.dt])

    def field(self, name):
        return np.array(self.so.field(name), order="F")

    def mom_step_(self):
        self.so.step(remeasure=False)

    def mom_steps_(self, k):
        for _ in range(k):
            self.so.step(remeasure=False)

    def phase_(self, q):
        self.so.phase(q)

    def measure_(self, q):
        import bodypaths_ref as bp
        body = self.case["positions"][q][0]
        if self.case["remeasure_each_step"]:
            body = bp.moving_position(self.case["positions"][0][0], float(np.sum(self.so.dt[:-1], dtype=np.float64)))
        self.so.set_body(body)
        self.so.measure()

    def open(self, name, level):
        if name == "us":
            return None
        v = self.so.field(name) if level is None else self.so.level_field(name, level)      # extents: Simulation.Ng / level_dims

        def write(a):
            assert a.shape == v.shape
            v[...] = a
        return Slot(v.shape, lambda: np.array(v, order="F"), write)

    def scratch(self, bits, regions=None):
        return None

    def set_sigma(self, a):
        self.so.field("sigma")[...] = a


class DevTwin:
    """a callseq.Dev or callseq.CallerDev: the stepping calls go to it, the dead arrays are reached through wl_sim_field / wl_mg_level_field with the extents of
    wl_sim_grid / wl_mg_level_grid and copied with wl_d2h / wl_h2d"""
    is_handle = True

    def __init__(self, w, dev):
        self.w, self.dev, self.lib = w, dev, w.lib()
        self.h = dev.sim._h if hasattr(dev.sim, "_h") else dev.sim.h
        for n in ("mom_step_", "mom_steps_", "phase_", "field"):
            setattr(self, n, getattr(dev, n))
        self.last_scratch = None

    pois_n = property(lambda self: self.dev.pois_n)
    dt = property(lambda self: self.dev.dt)
    nlevels = property(lambda self: self.lib.wl_mg_nlevels(self.lib.wl_sim_pois(self.h)))

    def measure_(self, q):
        self.dev.measure_(q)

    def set_sigma(self, a):
        self.dev.set_field("sigma", a)

    def _grid(self, level):
        from waterlily_jl_amd._lib import check, wl_grid
        g = wl_grid()
        check(self.lib.wl_sim_grid(self.h, g) if level is None else self.lib.wl_mg_level_grid(self.lib.wl_sim_pois(self.h), level, g))
        assert g.nz == g.gnz or g.D == 2, "single-domain handles"
        return g

    def open(self, name, level):
        import ctypes as C
        from waterlily_jl_amd._lib import check
        from waterlily_jl_amd.core import stream
        lib = self.lib
        p = lib.wl_sim_field(self.h, name.encode()) if level is None else lib.wl_mg_level_field(lib.wl_sim_pois(self.h), level, name.encode())
        if not p:
            assert name == "us", (name, level)
            return None
        g = self._grid(level)
        shape = ((g.nx, g.ny) if g.D == 2 else (g.nx, g.ny, g.nz)) + ((g.D,) if name in VECTOR else ())

        def read():
            out = np.empty(shape, dtype=f32, order="F")
            check(lib.wl_d2h(out.ctypes.data_as(C.c_void_p), p, out.nbytes, stream()))
            check(lib.wl_stream_sync(stream()))
            return out

        def write(a):
            a = np.asfortranarray(a, dtype=f32)
            assert a.shape == shape, (name, level, a.shape, shape)      # never past the array the handle described
            check(lib.wl_h2d(p, a.ctypes.data_as(C.c_void_p), a.nbytes, stream()))
            check(lib.wl_stream_sync(stream()))
        return Slot(shape, read, write)

    def scratch(self, bits, regions=None):
        from waterlily_jl_amd.core import stream
        if bits is None:
            n = self.lib.wl_sim_scratch_keep(self.h, stream())
        else:
            n = self.lib.wl_sim_scratch_fill(self.h, int(bits), stream()) if regions is None else self.lib.wl_sim_scratch_fill_regions(self.h, int(bits), int(regions), stream())
        assert n >= 0, self.lib.wl_last_error_string()
        self.last_scratch = n
        return n

    def scratch_words(self, perdir=False, force_tiles=0):
        """what wl_sim_scratch_fill has to report, from the level grids alone (include/wlhip_bench.h lists the regions); perdir: the flow has a periodic direction"""
        g0 = self._grid(None)
        n = g0.nx * g0.ny * g0.nz                                                   # 1. the pressure array that does not hold the pressure
        for l in range(self.nlevels):
            g = self._grid(l)
            inner = (g.nx - 2) * (g.ny - 2) * ((g.nz - 2) if g.D == 3 else 1)
            n += 2 * inner                                                          # 2. ϵ_mid and r′
            if has_exchange_buffer(g, perdir):
                n += (g.nz - 2) * (g.ny - 2) * ((g.nx - 1 + 59) // 60) * 128         # 3. W's interior rows, whole 512-byte segments
        return n + 65536 * 5 + 24 * force_tiles                                     # 4. the partials; 5. the force bands


def has_exchange_buffer(g, perdir=False):
    """wl_mg::build gives a level an exchange buffer W: single domain, no periodic direction, 3-D, even nx ≥ 34, ny ≥ 34, at least 8 interior planes"""
    return (not perdir) and g.D == 3 and g.nx % 2 == 0 and g.nx >= 34 and g.ny >= 34 and g.nz >= 10


# ------------------------------------------------------------------------------------------------------------- the oracle's configurations
# each family of tests/callseq.py at a reduced size (three multigrid levels at least), for the proof; full=True: at the size the device test runs
REDUCED = {"box": (16, 16, 16), "caller": (24, 16, 16), "ragged": (20, 12, 8), "periodic": (16, 16, 16), "moving": (16, 16, 16), "exit": (16, 16, 16), "circle2d": (24, 16)}


def _reduced_case(family):
    import bodypaths_ref as bp
    if family == "moving":
        pos = [(bp.sphere((6, 8, 8), 3.0, V=bp.MOVING_V), ()), (bp.sphere((-60, 8, 8), 3.0, V=bp.MOVING_V), ())]
        return bp._case("moving-reduced", pos, dims=REDUCED[family], remeasure_each_step=True)
    if family == "exit":
        return bp._case("exit-reduced", [(bp.floor(6.0), ()), (bp.floor(4.5), ())], dims=REDUCED[family], exitBC=True)
    return bp._case("circle2d-reduced", [(bp.sphere((8, 8), 3.0), ()), (bp.sphere((14.5, 7), 3.0), ())], dims=REDUCED[family])


def tgv(dims, periodic):
    """apply!(u⁰,u) of the wall-bounded (κ = π/N) and the periodic (κ = 2π/N) Taylor–Green vortex at loc(i,I) = I − 1.5 − δᵢ/2"""
    Ng = tuple(n + 2 for n in dims)
    u = np.zeros(Ng + (3,), dtype=f32, order="F")
    kap = [(2.0 if periodic else 1.0) * np.pi / n for n in dims]
    idx = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in Ng], indexing="ij")
    X = lambda a: [(idx[c] - 0.5 - (0.5 if c == a else 0.0)) * kap[c] for c in range(3)]
    x = X(0); u[..., 0] = (-np.sin(x[0]) * np.cos(x[1]) * np.cos(x[2])).astype(f32)
    x = X(1); u[..., 1] = (np.cos(x[0]) * np.sin(x[1]) * np.cos(x[2])).astype(f32)
    return u


def oracle_twin(orc, family, full=False):
    """the family's configuration on the oracle: the boundary values, ν, the periodic directions, the exit, the body and the kind of initial flow of callseq.make"""
    import bodypaths_ref as bp
    case = None
    if family in cs.BODY_CASE:
        case = next(c for c in bp.CASES if c["id"] == cs.BODY_CASE[family]) if full else _reduced_case(family)
        dims, D = case["dims"], len(case["dims"])
        ubc, nu, L, perdir, ex = (1.0,) + (0.0,) * (D - 1), 0.02, 8.0, case["perdir"], case["exitBC"]
        ui = np.asfortranarray(np.random.default_rng(11).uniform(-0.4, 0.4, size=tuple(n + 2 for n in dims) + (D,)).astype(f32))
    else:
        dims = cs.DIMS[family] if full else REDUCED[family]
        L, ex = dims[0], False
        if family in ("box", "caller"):
            ubc, nu, perdir = cs.UBC, 0.02, ()
            ui = np.asfortranarray(np.random.default_rng(137).uniform(-0.4, 0.4, size=tuple(n + 2 for n in dims) + (3,)).astype(f32))
        else:
            ubc, nu, perdir = (0.0,) * 3, dims[0] / 1600.0, ((1, 3) if family == "periodic" else ())
            ui = tgv(dims, family == "periodic")
    so = orc.Simulation(dims, ubc, L, U=1, nu=nu, perdir=perdir, exitBC=ex, body=(case["positions"][0][0] if case else None), T=f32)
    orc.BC(ui, ubc, ex, perdir)                      # Flow(): BC!(u,uBC,exitBC,perdir); exitBC!(u,u,0)   src/Flow.jl:141
    if ex:
        orc.exitBC(ui, ui.copy(order="F"), 0.0)
    so.field("u")[...] = ui
    so.field("u0")[...] = ui
    return OracleTwin(so, case)


# ------------------------------------------------------------------------------------------------------- σ's live ghost cells
SIGMA_VALUE = f32(7.5)      # above maximum(σ) of every clean run below (velocities of order 1: σ ≲ 3) — tests/test_deadstore_cpu.py checks that on the oracle
SIGMA_LIVE = ("box", "ragged", "exit", "circle2d")      # 64×32×24 (default and eager), 70×44×18, the exit body case, the 2-D circle


def sigma_plants(shape):
    """one lower-face ghost cell, one lower edge cell, one lower corner cell of σ (2-D has no edges: a cell of the other lower face)"""
    mid = tuple(n // 2 for n in shape)
    return [(0,) + mid[1:], (0, 0) + mid[2:] if len(shape) == 3 else (mid[0], 0), (0,) * len(shape)]


def plant(t, value=SIGMA_VALUE):
    s = t.field("sigma")
    cells = sigma_plants(s.shape)
    for c in cells:
        s[c] = value
    t.set_sigma(s)
    return cells


def dt_planted(nu, value=SIGMA_VALUE):
    """Δt = min(10, inv(v + 5ν)) in Float32 (src/Flow.jl:166, :234-237): no reduction order in it"""
    return f32(min(f32(10), f32(f32(1) / f32(f32(value) + f32(f32(5) * f32(nu))))))
