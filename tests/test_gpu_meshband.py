"""Band-limited mesh baking on the device (include/wlhip.h, band-limited baking; csrc/wl_meshsdf.hip k_meshsdf<D, VEL, true>): a banded lattice is the full
one clipped, as raw bits — against a wl_sdf_lattice_from_mesh lattice of the same arguments made in the same test, against the NumPy restatement
(tests/meshband_ref.py) and against the brute-force flag; the velocity samples masked to the band; the bricks the search skips, counted; re-baking in place;
measure! and five steps of a handle, banded against un-banded, bit for bit; the refusals, which launch nothing.  Everything is raw bits: no tolerance.
tests/test_meshband_cpu.py shows without a GPU that the cases hold what they are here for.  Lattices of at most 47×46×46 samples and 320 triangles (1280 on
20³), grids of at most 64×48×48."""
import ctypes as C

import numpy as np
import pytest

import bodypaths_ref as bp
import meshband_ref as mb
import meshsdf_ref as mr
import meshvel_ref as mv
from test_gpu_bodypaths import PLAIN, assert_same_state, handle, w  # noqa: F401  (w: the module-scoped fixture)

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
WL_EINVAL = -1
FP, IP = C.POINTER(C.c_float), C.POINTER(C.c_int32)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def pairs(w):
    a, b = C.c_uint64(), C.c_uint64()
    assert w.lib().wl_meshsdf_last_pairs(C.byref(a), C.byref(b)) == 0
    return int(a.value), int(b.value)


def bricks(w):
    a, b = C.c_uint64(), C.c_uint64()
    assert w.lib().wl_meshsdf_last_bricks(C.byref(a), C.byref(b)) == 0
    return int(a.value), int(b.value)


def make(w, c, band=None, brute=False, V=None, Wv=None):
    return w.SdfLattice.from_mesh(c["V"] if V is None else V, c["E"], c["dims"], c["origin"], c["spacing"], brute=brute, vertex_velocity=Wv, band=band)


def clip(a, band):
    return np.clip(a, -f32(band), f32(band)).astype(f32)


# ---- 1. samples, 3. the skip ----
@pytest.mark.parametrize("name", mb.CASES)
def test_samples_are_the_full_lattice_clipped_and_far_bricks_are_skipped(w, name):
    c, band = mb.case(name), mb.BAND[name]
    nbricks = len(mb.bricks(name))
    with make(w, c) as full:
        tested_full, total = pairs(w)
        assert bricks(w) == (nbricks, 0) and full.band == 0.0
        a_full = full.values()
        with make(w, c, band=band) as lat:
            tested, total_b = pairs(w)
            searched, skipped = bricks(w)
            assert lat.band == float(f32(band))
            a = lat.values()
            assert np.array_equal(bits(a), bits(clip(a_full, band))), (name, int((bits(a) != bits(clip(a_full, band))).sum()))
            assert np.array_equal(bits(a), bits(mb.clip_ref(name, band))), name
            assert f32(lat.edge_min).view(np.uint32) == f32(w.bodies.edge_min(a)).view(np.uint32)
            lo, hi = int(mb.far_bricks(name, band, 2.0).sum()), int(mb.far_bricks(name, band, 0.0).sum())
            print(f"[meshband] {name}: bricks {nbricks}, skipped {skipped} (restated: {lo} with twice the slack, {hi} without), pairs {tested} banded / "
                  f"{tested_full} un-banded / {total} all")
            assert searched + skipped == nbricks and lo <= skipped <= hi, (name, searched, skipped, lo, hi)
            assert total_b == total
            if lo > 0:
                assert tested < tested_full, (name, tested, tested_full)
            with make(w, c, band=band, brute=True) as brute:      # every pair, no brick skipped, the same clip: the same bits
                assert bricks(w) == (nbricks, 0) and pairs(w) == (total, total)
                assert np.array_equal(bits(brute.values()), bits(a)), name
                assert brute.edge_min == lat.edge_min


# ---- 2. velocities ----
def _breathing_rate(V):
    ctr = V.astype(f64).mean(axis=0)
    return (0.05 * (V.astype(f64) - ctr)).astype(f32)


FIELDS = {"rotating": lambda V: mv.rotation(V, centre=tuple(V.astype(f64).mean(axis=0))) if V.shape[1] == 3 else mv.travelling_wave(V),
          "linear": mv.linear, "breathing": _breathing_rate}


@pytest.mark.parametrize("name,field", [("ico320-R16", "rotating"), ("ellipse2d", "linear"), ("torus", "linear"), ("lprism", "breathing"),
                                        ("cube-11x9x6", "rotating"), ("gon64", "breathing")])
def test_velocity_samples_are_masked_to_the_band(w, name, field):
    c, band = mb.case(name), mb.BAND[name]
    Wv = FIELDS[field](c["V"])
    with make(w, c, Wv=Wv) as full, make(w, c, band=band, Wv=Wv) as lat, make(w, c, band=band) as still, make(w, c, band=band, Wv=Wv, brute=True) as brute:
        assert lat.has_velocity and not still.has_velocity and lat.band == still.band
        a_full, w_full = full.values(), full.velocity()
        want = np.where((np.abs(a_full) <= f32(band))[..., None], w_full, f32(0)).astype(f32)
        got = lat.velocity()
        assert np.array_equal(bits(got), bits(want)), (name, int((bits(got) != bits(want)).sum()))
        assert np.abs(got).max() > 0.01 and not bits(got[np.abs(a_full) > f32(band)]).any()
        assert np.array_equal(bits(lat.values()), bits(still.values())) and np.array_equal(bits(lat.values()), bits(clip(a_full, band)))
        assert np.array_equal(bits(brute.velocity()), bits(got)) and np.array_equal(bits(brute.values()), bits(lat.values()))
        d_ref, w_ref = mb.clip_ref(name, band, Wv)
        assert np.array_equal(bits(lat.values()), bits(d_ref))
        nb = int((bits(got) != bits(w_ref)).any(axis=-1).sum())
        print(f"[meshband] {name} {field}: samples whose W differs from the Float32 restatement in bits: {nb} of {a_full.size}")


# ---- 4. update_mesh / advance ----
def state(lat):
    return bits(lat.values()), (bits(lat.velocity()) if lat.has_velocity else None), f32(lat.edge_min).view(np.uint32), lat.band


def same_state(a, b):
    return np.array_equal(a[0], b[0]) and (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(a[1], b[1])) and a[2] == b[2] and a[3] == b[3]


@pytest.mark.parametrize("name", ["ico320-R16", "ellipse2d"])
def test_a_rebake_keeps_the_band_and_a_refused_one_changes_nothing(w, name):
    L = w.lib()
    c, band = mb.case(name), mb.BAND[name]
    V0 = c["V"]
    ctr = V0.astype(f64).mean(axis=0)
    V1 = (ctr + (V0.astype(f64) - ctr) * 1.03 + 0.11).astype(f32)
    W0, W1 = mv.linear(V0), _breathing_rate(V0)
    with make(w, c, band=band, Wv=W0) as lat:
        s0, id0 = state(lat), lat.id
        lat.update_mesh(V1, W1)
        sk = bricks(w)[1]
        with make(w, c, band=band, V=V1, Wv=W1) as fresh:
            assert bricks(w)[1] == sk > 0
            assert same_state(state(lat), state(fresh)) and lat.id == id0 != fresh.id
        assert not same_state(state(lat), s0) and lat.band == float(f32(band))
        lat.update_mesh(V1, W1, brute=True)                           # WL_MESH_BRUTE is still accepted: the same bits
        s1 = state(lat)
        assert bricks(w)[1] == 0
        with make(w, c, band=band, V=V1, Wv=W1) as fresh:
            assert same_state(s1, state(fresh))
        dt = 0.37
        lat.advance(V0, dt)                                           # advance(new, dt) is update_mesh(new, (new − old)/dt)
        with make(w, c, band=band, Wv=((V0 - V1) / f32(dt)).astype(f32)) as fresh:
            assert same_state(state(lat), state(fresh))
        s2 = state(lat)
        inverted = V0.copy(); inverted[:, 0] = (2 * ctr[0] - V0[:, 0].astype(f64)).astype(f32)      # mirrored in x: every element faces inward, in 2-D and 3-D
        nanv = V0.copy(); nanv[3, 1] = np.nan
        for what, bad, token in (("inverted", inverted, "inward"), ("a NaN vertex", nanv, "not finite")):
            n0 = L.wl_launch_count()
            rc = L.wl_sdf_lattice_update_mesh(lat._h, np.ascontiguousarray(bad).ctypes.data_as(FP), W0.ctypes.data_as(FP), 0, None)
            assert rc == WL_EINVAL and token in L.wl_last_error_string().decode(), (what, rc)
            assert L.wl_launch_count() == n0, what
            assert same_state(state(lat), s2) and lat.band == float(f32(band)), what
        lat.update_mesh(V0, W0)                                       # back: the bits of the creation
        assert same_state(state(lat), s0)


# ---- 5. through measure! ----
def _measure(w, dims, body):
    f = w.Flow(dims, (1.0,) + (0.0,) * (len(dims) - 1))
    for k in ("mu0", "mu1", "V"):
        getattr(f, k).fill_(float("nan"))
    f.sigma.fill_(0.25)
    w.measure_(f, body)
    return [w.to_host(getattr(f, k)) for k in ("sigma", "mu0", "mu1", "V")]


def _same_fields(what, banded, full, eps=1.0):
    for k, x, y in zip(("mu0", "mu1", "V"), banded[1:], full[1:]):
        assert np.array_equal(bits(x), bits(y)), (what, k, int((bits(x) != bits(y)).sum()))
    inner = (slice(1, -1),) * banded[0].ndim                          # measure! writes σ on the interior; the ghost layer keeps the fill on both
    sb, sf = banded[0][inner], full[0][inner]
    assert np.array_equal(bits(banded[0]) != bits(full[0]), np.pad(bits(sb) != bits(sf), 1)), (what, "sigma outside the interior")
    near = np.abs(sf) <= f32(2.0 + eps)
    assert near.sum() > 50 and (~near).sum() > 50, what
    assert np.array_equal(bits(sb[near]), bits(sf[near])), (what, "sigma inside the band")
    assert np.array_equal(np.signbit(sb[~near]), np.signbit(sf[~near])) and (np.abs(sb[~near]) > f32(2.0 + eps)).all(), (what, "sigma beyond the band")
    assert (full[1] < 1).sum() > 50, what                             # the body is in the domain


@pytest.mark.parametrize("name", ["ico320-R16", "ellipse2d"])
def test_measure_reads_the_same_body_from_a_banded_lattice(w, name):
    from waterlily_jl_amd.bodies import Body, RigidMap
    c = mb.case(name)
    D = c["D"]
    dims = (64, 48, 48) if D == 3 else (72, 64)
    shift = np.array([30.0, 24.0, 24.0] if D == 3 else [34.0, 31.0], f32)
    Wv = _breathing_rate(c["V"])
    placed = (c["V"] + shift).astype(f32)
    made = []

    def twins(V, **kw):
        pair = [w.mesh_body(V, c["E"], band=b, **kw) for b in (True, None)]
        made.extend(p.shape[1] for p in pair)
        return pair
    try:
        # unmapped, with vertex velocities
        a, b = twins(placed, vertex_velocity=Wv)
        assert a.shape[1].band == float(f32(w.mesh_band(1.0, 0.0, 1.0, D))) and b.shape[1].band == 0.0
        assert a.shape[1].edge_min > 4.0
        _same_fields((name, "unmapped"), _measure(w, dims, a), _measure(w, dims, b))
        for lat in made:
            lat.close()
        del made[:]
        # under a RigidMap with V and ω
        if D == 3:
            mp = RigidMap(tuple(shift + f32(0.3)), (0.2, -0.1, 0.3), V=(0.1, -0.05, 0.02), omega=(0.01, 0.02, -0.015))
        else:
            mp = RigidMap(tuple(shift + f32(0.3)), 0.3, V=(0.1, -0.05), omega=0.02)
        a, b = twins(c["V"], map=mp, vertex_velocity=Wv)
        _same_fields((name, "mapped"), _measure(w, dims, a), _measure(w, dims, b))
        # composed: (lattice ∪ capsule) − sphere
        if D == 3:
            other = Body(("capsule", (30.0, 24.0, 24.0), 3.0, (1.0, 0.2, 0.0), 20.0), mp)
            hole = Body(("sphere", (44.0, 26.0, 25.0), 6.0))
        else:
            other = Body(("capsule", (34.0, 31.0), 3.0, (1.0, 0.2), 30.0), mp)
            hole = Body(("sphere", (56.0, 33.0), 6.0))
        _same_fields((name, "composed"), _measure(w, dims, (a | other) - hole), _measure(w, dims, (b | other) - hole))
    finally:
        for lat in made:
            lat.close()


# ---- 6. on a handle ----
def test_five_steps_of_a_breathing_body_on_a_handle(w):
    from waterlily_jl_amd.bodies import RigidMap
    case = dict(id="breathing-band", dims=(64, 48, 48), perdir=(), exitBC=False, lam=0, store_f=False)
    c = mb.case("ico320-R16")
    V0, E = c["V"], c["E"]
    centre = (0.2, -0.1, 0.3)
    mp = RigidMap((30.3, 23.7, 24.1), (0.0, 0.0, 0.1))
    x0 = (30.0, 24.0, 24.0)
    bodies = [w.mesh_body(V0, E, margin=7.0, map=mp, vertex_velocity=np.zeros_like(V0), band=b) for b in (True, None)]
    lats = [b.shape[1] for b in bodies]
    try:
        assert lats[0].band > 5.9 and lats[1].band == 0.0
        sims = [handle(w, case, {}) for _ in bodies]
        for sim, body in zip(sims, bodies):
            sim.set_body(body)
            sim.set_force_record(body, x0=x0, capacity=8)
        A, B = sims
        names = ("hybrid",) + tuple(bp.CENSUS_NAMES)
        for k in range(5):
            dt = float(A.dt[-1])
            for lat in lats:
                lat.advance(mv.breathing(V0, centre, k + 1), dt)
            assert bricks(w)[1] == 0                                  # the last bake was the un-banded one
            for sim in sims:
                sim.sim_step_(remeasure=True)
            assert_same_state(A, B, ("breathing-band", k))
            ra, rb = A.read_forces(), B.read_forces()
            assert ra[1].shape == (1, 3)
            for x, y in zip(ra, rb):
                assert np.array_equal(np.asarray(x, f64).view(np.uint64), np.asarray(y, f64).view(np.uint64)), k
            assert {n: A.counter(n) for n in names} == {n: B.counter(n) for n in names}, k
        assert np.linalg.norm(ra[1][0]) > 1e-3 and A.counter("force_dropped") == 0
        for sim in sims:
            sim.set_force_record(None)
        del sims, A, B
    finally:
        for lat in lats:
            lat.close()


# ---- 7. refusals ----
def _raw_band(L, c, band, V=None, E=None, Wv=None, flags=0):
    V = np.ascontiguousarray(c["V"] if V is None else V, dtype=f32)
    E = np.ascontiguousarray(c["E"] if E is None else E, dtype=np.int32)
    D = c["D"]
    h = C.c_void_p()
    rc = L.wl_sdf_lattice_from_mesh_band(C.byref(h), D, (C.c_int32 * D)(*c["dims"]), (C.c_float * D)(*c["origin"]), c["spacing"], V.ctypes.data_as(FP), len(V),
                                         E.ctypes.data_as(IP), len(E), None if Wv is None else np.ascontiguousarray(Wv, dtype=f32).ctypes.data_as(FP),
                                         band, flags, None)
    return rc, h


def test_refusals_launch_nothing(w):
    L = w.lib()
    c = mb.case("cube")
    for band in (0.0, -1.0, float("nan"), float("inf")):
        n0 = L.wl_launch_count()
        rc, h = _raw_band(L, c, band)
        assert rc == WL_EINVAL and "band must be finite and positive" in L.wl_last_error_string().decode() and not h, band
        assert L.wl_launch_count() == n0
    assert L.wl_sdf_lattice_band(None) == 0.0
    for what, D, V, E, reason in mr.broken_variants():                # every mesh refusal of from_mesh through the new call
        cc = dict(mb.case("cube" if D == 3 else "square"), V=V, E=E)
        n0 = L.wl_launch_count()
        rc, h = _raw_band(L, cc, 2.5)
        msg = L.wl_last_error_string().decode()
        assert rc == WL_EINVAL and mr.REASONS[reason] in msg and "wl_sdf_lattice_from_mesh_band" in msg and not h, (what, rc, msg)
        assert L.wl_launch_count() == n0, what
    n0 = L.wl_launch_count()
    bad = mv.linear(c["V"]); bad[2, 1] = np.inf
    rc, h = _raw_band(L, c, 2.5, Wv=bad)
    assert rc == WL_EINVAL and "velocity of vertex" in L.wl_last_error_string().decode() and L.wl_launch_count() == n0
    rc, h = _raw_band(L, c, 2.5, flags=4)
    assert rc == WL_EINVAL and "flag" in L.wl_last_error_string().decode() and L.wl_launch_count() == n0
    eight = [make(w, c, band=2.5) for _ in range(w.bodies.LATTICE_MAX)]
    try:
        n0 = L.wl_launch_count()
        with pytest.raises(w.WlError, match="alive"):                  # a ninth lattice
            make(w, c, band=2.5)
        assert L.wl_launch_count() == n0
        dead = eight[0]._h
        eight[0].close()
        assert L.wl_sdf_lattice_band(dead) == 0.0 and eight[0].band == 0.0 and eight[1].band == 2.5
    finally:
        for m in eight:
            m.close()


@pytest.mark.parametrize("D", [3, 2])
def test_the_band_rule_refuses_just_below_and_accepts_just_above(w, D):
    """need + s·√D in Float32, as the library forms it: a band equal to it is not above it (refused, the message names the band condition and both numbers);
    the next Float32 is (accepted).  The lattice's margin keeps the edge rule satisfied throughout, so it is the band condition that decides."""
    L = w.lib()
    c = mb.case("ico320-R16" if D == 3 else "ellipse2d")
    case = dict(id="rule", dims=(64, 48, 48) if D == 3 else (72, 64), perdir=(), exitBC=False, lam=0, store_f=False)
    shift = np.array([30.0, 24.0, 24.0] if D == 3 else [34.0, 31.0], f32)
    V = (c["V"] + shift).astype(f32)
    sim = handle(w, case, {})
    f = w.Flow(case["dims"], (1.0,) + (0.0,) * (D - 1))
    for need, call in ((4.0, "measure"), (2.0, "force")):
        at = f32(need) + f32(1.0) * np.sqrt(f32(D))
        for band, ok in ((float(at), False), (float(np.nextafter(at, f32(np.inf))), True)):
            body = w.mesh_body(V, c["E"], margin=5.5, band=band)
            try:
                assert body.shape[1].edge_min > need
                n0 = L.wl_launch_count()
                if ok:
                    w.measure_(f, body) if call == "measure" else sim.forces(body, x0=tuple(shift))
                    assert L.wl_launch_count() > n0
                else:
                    with pytest.raises(w.WlError, match="band") as e:
                        w.measure_(f, body) if call == "measure" else sim.forces(body, x0=tuple(shift))
                    msg = str(e.value)
                    assert "s·√D" in msg and f"{band:.6f}"[:6] in msg and "edge_min" not in msg, msg
                    assert L.wl_launch_count() == n0
                d, _, _ = w.bodies.measure(body, V[:8], fastd2=1.0)    # the point probe applies neither rule
                assert d.shape == (8,)
            finally:
                body.shape[1].close()
    del sim
