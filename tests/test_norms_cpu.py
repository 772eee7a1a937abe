"""What keeps tests/test_gpu_norms.py and tests/test_gpu_cfl_routes.py from being hollow, shown without a GPU on the oracle's own fields.

Every committed case of tests/norms_ref.py (CASES: handle, spike, iteration cap k; SIGMA_CASES: stream, jet) is run through the oracle —
MultiLevelPoisson.solve capped at k gives r, Simulation.step gives σ — and held to this:
  * the arg-max of |r| (of σ) is the committed one and lies in every class the case is listed for, and exceeds the largest value outside each such class by
    at least 1 %: a last-bit difference between device and oracle (the mean shift) cannot move it out of the class;
  * over all cases every class of cell_classes is hit for every tiling that defines it (the table is printed: class × tiling × cases, with the routes of
    tests/test_gpu_norms.py that run on that tiling).  Not defined: `last_tile` where the tile count is a multiple of 8 (66×34×26, 62×34×12: 8 tiles), the
    z-chunk seams at 450×370×10 (the 32-row instance takes its 8 planes as one chunk — the largest array the suite may use);
  * r₁'s bound bites: the arg-max cell alone, dropped from l1 or counted twice, moves the sum by more than the bound, and so does the whole class (a reducer that
    masks a class loses all of it).  Not every single cell of a class does — a residual crosses zero somewhere — so the share that does is printed, not asserted;
  * cell_classes counts the tiles the other tests count: WIDE_TILES of tests/test_gpu_rskip.py, abw_segments of tests/test_abwide_cpu.py;
  * the tables are what candidates() draws under SEED.
The ghost-cell class of σ IS reached (see SIGMA_CASES for the amplitudes tried): on the upper x, y and z faces; lower ghost cells hold 0.
dt_from_sigma is held to the oracle's own Δt on every σ case, as raw bits."""
import numpy as np
import pytest

import norms_ref as nr
from test_abwide_cpu import slotmap      # noqa: F401  (the fixture that compiles csrc/wl_abwide.hpp)

f32 = np.float32

# the routes of tests/test_gpu_norms.py per tiling (for the printed table)
ROUTES = {
    "r16": ("passes", "onecell", "pair_W", "pair_dense", "pair_xA", "pair_eps", "tail_off", "tail_global", "bare", "in-step"),
    "r32": ("passes", "onecell", "pair_W", "pair_dense", "pair_xA", "pair_eps", "tail_off", "tail_global", "bare", "in-step"),
    "zsplit": ("passes", "zsplit"),
    None: ("passes",),
}


def oracle_r(oracle, sid, z, k):
    e = nr.SHAPES[sid]
    shape, D = e["shape"], len(e["shape"])
    L = np.ones(shape + (D,), dtype=f32, order="F")
    if e["tiling"] == "zsplit":
        nr.zsplit_coefficients(L)
    oracle.BC(L, (0,) * D, perdir=e["perdir"])
    x = np.zeros(shape, dtype=f32, order="F")
    ml = oracle.MultiLevelPoisson(x, L, np.asfortranarray(z.copy()), perdir=e["perdir"])
    n = ml.solve(tol=1e-30, itmx=k)
    assert n == k
    return np.array(ml.field("r"), copy=True)


def held_classes(cc, a, am, want):
    """the classes of `want` that hold the arg-max `am` of the non-negative array `a` with the 1 % margin"""
    return tuple(sorted(c for c in cc.of(am) if c in want and a[am] >= 1.01 * a[~cc.mask[c]].max()))


@pytest.mark.parametrize("q", range(len(nr.CASES)), ids=[f"{c[0]}-{c[1]}" for c in nr.CASES])
def test_residual_case_puts_its_maximum_in_its_class(oracle, q):
    sid, cls, pick, spike, k, arg, classes = nr.CASES[q]
    e = nr.SHAPES[sid]
    cc, want = nr.classes_of(sid)
    assert nr.candidates(e["shape"], cls, nr.SEED, zranges=e["zranges"])[pick] == spike      # the table is the draw
    r = oracle_r(oracle, sid, nr.rhs_with_spike(e["shape"], spike), k)
    a = np.abs(r)
    am = tuple(int(v) for v in np.unravel_index(int(a.argmax()), a.shape))
    held = held_classes(cc, a, am, want)
    ref = nr.l1(r)
    bound = nr.r1_bound(ref, r.size)
    print(f"{sid} {cls} k={k}: spike {spike} arg-max {am} |r| {float(a[am]):.4e} l1 {ref:.6e} bound {bound:.3e} classes {held}")
    assert am == tuple(arg) and cls in classes and set(classes) <= set(held), (am, arg, held, classes)
    assert nr.bits(nr.linf(r)) == nr.bits(a[am])
    for c in classes:
        m = cc.mask[c]
        inside = a[m].astype(np.float64)
        share = float((inside > bound).mean())
        print(f"   {c}: {int(m.sum())} cells, Σ {float(inside.sum()):.4e}, each above the bound alone: {share:.3f}")
        assert float(a[am]) > bound and float(inside.sum()) > bound, (c, float(a[am]), float(inside.sum()), bound)
    # … as the GPU test would see it: the sum without the cell, and with the cell twice, misses the bound
    for wrong in (ref - float(a[am]), ref + float(a[am])):
        assert abs(float(f32(wrong)) - ref) > bound


def test_every_class_is_hit_on_every_tiling_that_defines_it():
    table, missing = {}, []
    for tiling in ("r16", "r32", "zsplit", None):
        sids = [s for s, e in nr.SHAPES.items() if e["tiling"] == tiling]
        defined = set()
        for s in sids:
            defined |= set(nr.classes_of(s)[1])
        for c in (nr.R_CLASSES if tiling else nr.GENERIC):
            hits = [f"{k[0]}:{k[3]}/k{k[4]}" for k in nr.CASES if k[0] in sids and c in k[6]]
            table[(c, tiling)] = hits
            if c in defined and not hits:
                missing.append((c, tiling))
            if c not in defined:
                assert not hits
    print("class × tiling (routes) × cases")
    for (c, tiling), hits in table.items():
        print(f"  {c:12s} {str(tiling):7s} ({', '.join(ROUTES[tiling])}): {' '.join(hits) if hits else '— not defined at these shapes'}")
    assert not missing, missing
    # what is not defined, and why
    assert "last_tile" not in nr.classes_of("66x34x26")[1] and nr.workgroups((66, 34, 26), 24)[1] == 0
    assert "last_tile" in nr.classes_of("66x66x18")[1] and nr.workgroups((66, 66, 18), 16)[1] > 0
    assert nr.zchunk2((450, 370, 10), 8) == 8 and "zseam_lo" not in nr.classes_of("450x370x10")[1]
    for s in ("66x34x26", "62x34x12", "66x66x18"):
        assert nr.SHAPES[s]["tiling"] == "r16" and nr.rows_of(nr.SHAPES[s]["shape"]) == 16
    assert nr.rows_of((450, 370, 10)) == 32


def test_cell_classes_counts_the_tiles_the_other_tests_count(slotmap):      # noqa: F811
    import test_gpu_rskip as rk
    wide = tuple(n + 2 for n in rk.WIDE)
    ntx, nty = nr.tile_counts(wide, 32)
    assert ntx * nty == rk.WIDE_TILES == 135 and nr.rows_of(wide) == 32
    launched, dead = nr.workgroups(wide, rk.WIDE[2])
    assert (launched, dead) == (136, 1)      # one z-chunk of 17 workgroups per XCD: the last one has no tile
    for nx in (34, 62, 66, 122, 258, 450, 514):
        assert nr.tile_counts((nx, 34, 12), 16, kernel="A")[0] == slotmap.t_segments(nx), nx
    cc = nr.cell_classes(wide)
    assert (cc.ntx, cc.nty, cc.rows) == (9, 15, 32)
    assert int(cc.mask["last_tile"][:, :, 1].sum()) == 1 * 4      # the last tile's core: column 448 alone, rows 365..368
    assert cc.of((448, 367, 1)) >= {"last_tile", "ragged_col", "ragged_row", "row_last", "xseam_hi", "plane_first", "pair_even"}
    assert cc.of((1, 1, 8)) == {"row_first", "pair_odd", "plane_last"}
    small = nr.cell_classes((66, 34, 26))
    assert small.zchunks == [4] and small.of((55, 10, 4)) == {"pair_odd", "xseam_lo", "yseam_lo", "zseam_lo"}
    assert small.of((56, 11, 5)) == {"pair_even", "xseam_hi", "yseam_hi", "zseam_hi", "ragged_col"}
    zs = nr.cell_classes((66, 34, 34), zranges=nr.ZSPLIT_RANGES)
    assert {"zseam_lo"} <= zs.of((5, 5, 11)) and {"zseam_hi"} <= zs.of((5, 5, 12)) and {"zseam_lo"} <= zs.of((5, 5, 21)) and {"zseam_hi"} <= zs.of((5, 5, 22))
    sg = nr.cell_classes((66, 34, 26), "sigma")
    assert sg.of((65, 16, 14)) == {"ghost", "ghost_x1"} and sg.of((0, 0, 0)) == {"ghost", "ghost_x0", "ghost_y0", "ghost_z0"}
    assert "ghost" not in sg.of((1, 1, 1))


def test_case_tables_are_deterministic_under_the_seed():
    for sid, e in nr.SHAPES.items():
        for c in nr.classes_of(sid)[1]:
            a = nr.candidates(e["shape"], c, nr.SEED, zranges=e["zranges"])
            assert a == nr.candidates(e["shape"], c, nr.SEED, zranges=e["zranges"]) and len(set(a)) == len(a)
    assert len({(c[0], c[3], c[4]) for c in nr.CASES}) == len(nr.CASES)
    for dims, ubc, jets, cls, pick, arg, classes in nr.SIGMA_CASES:
        if pick >= 0:
            assert nr.candidates(tuple(n + 2 for n in dims), cls, nr.SEED, count=6)[pick] == jets[0][0]


@pytest.mark.parametrize("q", range(len(nr.SIGMA_CASES)), ids=[f"{'x'.join(map(str, c[0]))}-{c[3]}" for c in nr.SIGMA_CASES])
def test_sigma_case_puts_its_maximum_in_its_class(oracle, q):
    dims, ubc, jets, cls, pick, arg, classes = nr.SIGMA_CASES[q]
    u = nr.stream_and_jets(dims, ubc, jets, oracle.BC)
    body = None
    if len(dims) == 2:      # the circle of the circle2d family, as tests/test_gpu_cfl_routes.py measures it
        import bodypaths_ref as bp
        body = next(c for c in bp.CASES if c["id"] == "circle2d")["positions"][0][0]
    so = oracle.Simulation(dims, ubc, 8.0 if body else dims[0], U=1, nu=nr.SIGMA_NU, T=f32, body=body)
    so.field("u")[...] = u
    so.field("u0")[...] = u
    so.step(remeasure=False)
    s = np.array(so.field("sigma"), copy=True)
    assert np.isfinite(so.field("u")).all() and np.isfinite(s).all()
    cc = nr.cell_classes(s.shape, "sigma")
    inner = tuple(slice(1, n - 1) for n in s.shape)
    am = tuple(int(v) for v in np.unravel_index(int(s.argmax()), s.shape))
    held = held_classes(cc, s, am, nr.SIGMA_WANT + ("ghost",) + nr.GHOST_FACES)
    print(f"{dims} {cls}: jets {jets} arg-max {am} σ {float(s[am]):.5f}, largest interior σ {float(s[inner].max()):.5f}, classes {held}")
    assert am == tuple(arg) and cls in classes and set(classes) <= set(held), (am, arg, held, classes)
    assert nr.bits(nr.dt_from_sigma(s, nr.SIGMA_NU)) == nr.bits(so.dt[-1]), (float(nr.dt_from_sigma(s, nr.SIGMA_NU)), so.dt[-1])
    if "ghost" in classes:      # the maximum over the interior alone would give another Δt
        assert nr.bits(nr.dt_from_sigma(s[inner], nr.SIGMA_NU)) != nr.bits(so.dt[-1])


def test_sigma_cases_reach_the_interior_classes_and_the_upper_ghost_faces():
    for dims in ((64, 32, 24), (448, 368, 8)):
        cc = nr.cell_classes(tuple(n + 2 for n in dims), "sigma")
        hit = set()
        for c in nr.SIGMA_CASES:
            if c[0] == dims:
                hit |= set(c[6])
        for c in nr.SIGMA_WANT:
            if c in cc.names:
                assert c in hit, (dims, c)
        assert "ghost_x1" in hit
    hit = {c for k in nr.SIGMA_CASES for c in k[6]}
    assert {"ghost", "ghost_x1", "ghost_y1", "ghost_z1"} <= hit
    print("σ classes reached:", sorted(hit), "— lower ghost faces hold 0 after a step: pinned by the leaf test of tests/test_gpu_cfl_routes.py alone")


def test_reference_scalars():
    r = np.zeros((6, 5, 4), dtype=f32, order="F")
    r[1:-1, 1:-1, 1:-1] = np.random.default_rng(3).standard_normal((4, 3, 2)).astype(f32)
    assert nr.l1(r) == float(np.sum(np.abs(r.astype(np.float64)))) or abs(nr.l1(r) - float(np.abs(r.astype(np.float64)).sum())) < 1e-12
    assert nr.linf(r).dtype == f32 and float(nr.linf(r)) == float(np.abs(r).max())
    s = np.full((4, 4, 4), f32(0.25))
    s[3, 3, 3] = 3.0                                                # a ghost cell takes part
    d = f32(3.0) + f32(f32(5) * f32(0.02))
    assert nr.bits(nr.dt_from_sigma(s, 0.02)) == nr.bits(f32(1) / d)
    assert float(nr.dt_from_sigma(np.zeros((3, 3)), 0.0)) == 10.0   # 1/0 = inf: the cap
    err, bound = nr.r1_err(f32(nr.l1(r)), r)
    assert err <= bound
