"""Distance fields from meshes without a GPU: the NumPy restatement (tests/meshsdf_ref.py) against the closed-form box and against the generalised winding
number, the refusal rules on a list of broken meshes, weld / read_stl, the placement rule of mesh_body, the declarations — and the conditions that keep
tests/test_gpu_meshsdf.py from being hollow, asserted from the Float64 restatement for every case."""
import os

import numpy as np
import pytest

import meshsdf_ref as mr
from waterlily_jl_amd import bodies

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def positions(c):
    return mr.sample_positions(c["dims"], c["origin"], c["spacing"])


def test_cube_is_the_analytic_box_distance():
    for name in ["cube"] + mr.RAGGED:
        c = mr.case(name)
        V = c["V"].astype(f64)                               # (the box the Float32 vertices describe)
        want = mr.box_distance(positions(c), V.min(axis=0), V.max(axis=0)).reshape(c["dims"], order="F")
        err = np.abs(mr.ref(name, "f64")["d"] - want).max()
        assert err <= 1e-12, (name, err)
        assert (want < 0).any() or name != "cube"
    assert mr.gap("cube") < 2e-6


@pytest.mark.parametrize("name", ["torus", "lprism", "lpoly"])
def test_sign_is_the_winding_number(name):
    c = mr.case(name)
    w = mr.winding_number(c["D"], c["V"], c["E"], positions(c)).reshape(c["dims"], order="F")
    assert np.abs(w - np.round(w)).max() < 1e-9              # a closed surface: 0 outside, 1 inside
    inside = np.round(w) == 1
    d = mr.ref(name, "f64")["d"]
    assert np.array_equal(d < 0, inside)
    assert inside.sum() >= 40 and (~inside).sum() >= 40              # (the L polygon covers 48 cells)


def test_torus_sign_is_the_analytic_torus_beyond_the_facet_error():
    c = mr.case("torus")
    R, r, centre = c["torus"]
    an = mr.torus_distance(positions(c), R, r, centre).reshape(c["dims"], order="F")
    d = mr.ref("torus", "f64")["d"]
    facet = np.abs(d - an).max()                             # the mesh is inscribed: it differs from the torus by its sagitta
    assert facet < 0.35
    far = np.abs(an) > facet
    assert far.sum() > 13000 and np.array_equal(d[far] < 0, an[far] < 0)


def test_broken_meshes_are_recognised_and_the_cases_pass():
    for name in mr.CASES:
        c = mr.case(name)
        assert mr.check_mesh(c["D"], c["V"], c["E"]) is None, name
    seen = set()
    for name, D, V, E, why in mr.broken_variants():
        assert mr.check_mesh(D, V, E) == why, (name, mr.check_mesh(D, V, E), why)
        assert why in mr.REASONS
        seen.add(why)
    assert seen == set(mr.REASONS)                           # every rule has a mesh that breaks it


@pytest.mark.parametrize("name", sorted(mr.CASES))
def test_conditions_that_keep_the_gpu_tests_from_being_hollow(name):
    c = mr.case(name)
    r64, r32 = mr.ref(name, "f64"), mr.ref(name, "f32")
    g = mr.gap(name)
    assert 0 < g < 1e-5, g
    # no sample within the bound of the surface: the sign is compared on every sample, no exemptions
    assert np.abs(r64["d"]).min() > 4 * g, (np.abs(r64["d"]).min(), g)
    assert np.array_equal(r32["d"] < 0, r64["d"] < 0)
    # the sign does not hang on rounding: (p − q)·n is a fair part of |p − q|
    ratio = np.abs(r64["s"]) / np.sqrt((r64["r"] ** 2).sum(axis=1))
    assert ratio.min() >= 1e-3, ratio.min()
    assert (r64["d"] < 0).any() or name in ("cube-3x3x3", "cube-5x3x3")
    # every region of the walk wins somewhere (over the 3-D cases together this is asserted below)
    assert r64["reg"].max() < mr.NREG[c["D"]]


def test_every_region_wins_somewhere():
    for names, D in ((["cube", "lprism", "torus"], 3), (["lpoly", "gon64"], 2)):
        for name in names:
            n = np.bincount(mr.ref(name, "f64")["reg"], minlength=mr.NREG[D])
            assert (n > 0).all() or name in ("gon64",), (name, n)


def test_ragged_cases_have_a_partial_brick_in_every_direction():
    for name in mr.RAGGED:
        c = mr.case(name)
        assert all(n % e != 0 for n, e in zip(c["dims"], mr.EXT[3])), name
    for name in mr.CASES_2D:
        c = mr.case(name)
        assert any(n % e != 0 for n, e in zip(c["dims"], mr.EXT[2])), name
    # more than one workgroup (four bricks), and a last workgroup that owns fewer than four
    assert mr.cull_census("ico1280-centred")["nbricks"] % 4 == 1 and mr.cull_census("cube-11x9x6")["nbricks"] % 4 == 2 and mr.cull_census("torus")["nbricks"] > 4


def test_centred_icosphere_holds_every_triangle_for_one_brick():
    c = mr.case("ico1280-centred")
    i = np.ravel_multi_index(c["centre_sample"], c["dims"], order="F")
    X = positions(c)[i:i + 1]
    assert np.array_equal(X[0], np.array([9.5, 9.5, 9.5], f32))
    # every vertex is equidistant from that sample …
    dv = np.linalg.norm(c["V"].astype(f64) - X.astype(f64), axis=1)
    assert dv.max() - dv.min() < 1e-5
    # … so the brick that holds it keeps all 1280 triangles: any fixed candidate capacity below 1280 overflows there
    cen = mr.cull_census("ico1280-centred")
    b = tuple(v // 4 for v in c["centre_sample"])
    assert cen["cand"][np.ravel_multi_index(b, cen["nb"], order="F")] == 1280 == len(c["E"])


@pytest.mark.parametrize("name", ["torus", "ico1280-centred"])
def test_the_cull_drops_pairs(name):
    cen = mr.cull_census(name)
    assert cen["nbricks"] <= cen["tested"] < cen["total"]
    assert (cen["cand"] >= 1).all() and (cen["cand"] < len(mr.case(name)["E"])).any()


@pytest.mark.parametrize("name", mr.CASES_3D)
def test_mesh_body_placement_leaves_the_margin(name):
    """edge_min − |offset| > 4 for the default margin of 5, from the restatement on the two outermost layers of mesh_body's lattice"""
    c = mr.case(name)
    dims, origin = bodies.mesh_placement(c["V"], 1.0, 5.0)
    assert (dims, origin) == mr.mesh_body_placement(c["V"], 1.0, 5.0)
    V = c["V"].astype(f64)
    ax = [origin[d] + (np.arange(dims[d]) - 0.5) for d in range(3)]
    for d in range(3):                                       # samples 1 and n − 2 sit at least the margin outside the box
        assert ax[d][1] <= V[:, d].min() - 5.0 + 1e-9 and ax[d][-2] >= V[:, d].max() + 5.0 - 1e-9
    X = mr.sample_positions(dims, origin, 1.0)
    I = np.stack(np.unravel_index(np.arange(len(X)), dims, order="F"), axis=1)
    edge = ((I < 2) | (I >= np.array(dims) - 2)).any(axis=1)
    d = mr.sdf_points(3, c["V"], c["E"], X[edge], f64)["d"]
    assert (d > 0).all() and d.min() > 4.0 + 0.5, d.min()      # edge_min (offset 0) — and so > 2 + ϵ + 1 at ϵ = 1
    if name == "cube":                                       # bodies.edge_min of the full field is this minimum
        full = mr.sdf_points(3, c["V"], c["E"], X, f64)["d"].reshape(dims, order="F")
        assert bodies.edge_min(full) == pytest.approx(d.min(), abs=1e-6)


def test_weld_merges_equal_rows_and_keeps_the_surface():
    c = mr.case("cube")
    soup = c["V"][c["E"].reshape(-1)]
    V, F = bodies.weld(soup, np.arange(36).reshape(12, 3))
    assert V.shape == (8, 3) and F.shape == (12, 3) and F.dtype == np.int32
    assert np.array_equal(V[F], c["V"][c["E"]])              # the same triangles, vertex for vertex
    assert mr.check_mesh(3, V, F) is None and mr.check_mesh(3, soup, np.arange(36).reshape(12, 3)) == "edge"
    z = np.array([[0.0, 1, 2], [-0.0, 1, 2], [3, 4, 5]], f32)
    assert len(bodies.weld(z, np.array([[0, 1, 2]]))[0]) == 2      # −0 and +0 are one position


def test_read_stl_round_trip_and_ascii_refusal(tmp_path):
    c = mr.case("cube")
    p = tmp_path / "cube.stl"
    mr.write_binary_stl(p, c["V"], c["E"])
    V, F = bodies.read_stl(str(p))
    assert V.dtype == f32 and V.shape == (8, 3) and F.shape == (12, 3)
    assert np.array_equal(V[F], c["V"][c["E"]])
    assert mr.check_mesh(3, V, F) is None
    a = tmp_path / "ascii.stl"
    a.write_text("solid cube\n facet normal 0 0 1\n  outer loop\n   vertex 0 0 0\n   vertex 1 0 0\n   vertex 0 1 0\n  endloop\n endfacet\nendsolid cube\n")
    with pytest.raises(ValueError, match="ASCII"):
        bodies.read_stl(str(a))
    t = tmp_path / "short.stl"
    t.write_bytes(p.read_bytes()[:-7])
    with pytest.raises(ValueError):
        bodies.read_stl(str(t))


def test_from_mesh_checks_its_shapes_before_the_library():
    c = mr.case("cube")
    with pytest.raises(ValueError):
        bodies.SdfLattice.from_mesh(c["V"], c["E"][:, :2], c["dims"])
    with pytest.raises(ValueError):
        bodies.SdfLattice.from_mesh(c["V"], c["E"], c["dims"][:2])


def test_entry_points_are_declared_bound_and_built():
    import waterlily_jl_amd as w
    L = w.lib()
    for name in ("wl_sdf_lattice_from_mesh", "wl_sdf_lattice_read", "wl_sdf_lattice_edge_min", "wl_meshsdf_last_pairs"):
        assert hasattr(L, name) and name in w.SIGNATURES, name
    hdr = open(os.path.join(ROOT, "include", "wlhip.h"), encoding="utf-8").read()
    assert "WL_MESH_BRUTE = 1" in hdr and "void* hip_stream);  /* the samples" in hdr
    assert len(w.SIGNATURES["wl_sdf_lattice_from_mesh"][1]) == 11
    mk = open(os.path.join(ROOT, "waterlily.jl_amd", "csrc", "Makefile"), encoding="utf-8").read()
    assert "wl_meshsdf.hip" in mk and "wl_meshsdf.hpp" in mk
    for name in ("mesh_body", "weld", "read_stl"):
        assert hasattr(w, name)
