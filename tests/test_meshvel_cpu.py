"""Deforming meshes without a GPU: the cases of tests/meshvel_ref.py hold what tests/test_gpu_meshvel.py needs of them, asserted on the restatement alone —
few samples on the medial axis (where the closest-point extension of the vertex velocities is discontinuous and no tolerance applies), every region of the
closest-point walk winning inside the band, velocity fields that vary across the winning elements, a uniform velocity reproduced exactly, and W continuous
across shared edges.  Also: the new entry points are declared, bound and built, and the Python surface checks its shapes before the library."""
import os

import numpy as np
import pytest

import meshsdf_ref as mr
import meshvel_ref as mv
from waterlily_jl_amd import bodies

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


@pytest.mark.parametrize("name", sorted(mv.CASES))
def test_ambiguous_share_of_the_band_is_small(name):
    """the cap is a condition on the cases: at most 2 % of the band |d| ≤ 5 on the medial axis (meshvel_ref.ambiguous; the literal pair of thresholds, which
    also flags the neighbourhood of every shared edge, is printed next to it: 34 % on the 1280-face sphere, at any offset)"""
    band, amb, lit = mv.band(name), mv.ambiguous(name), mv.ambiguous_literal(name)
    share = float((amb & band).sum()) / max(1, int(band.sum()))
    assert not (amb & ~lit).any()                                   # the mended set lies inside the literal one: more samples are held to the bound
    print(f"[meshvel] {name}: band {int(band.sum())} of {band.size} samples, ambiguous in the band {int((amb & band).sum())} ({100 * share:.2f} %); "
          f"by the literal thresholds {int((lit & band).sum())} ({100 * float((lit & band).sum()) / max(1, int(band.sum())):.2f} %)")
    assert band.sum() >= (20 if name not in mv.TINY else 1) and share <= 0.02, (name, share)


@pytest.mark.parametrize("name", sorted(mv.CASES))
def test_every_region_wins_in_the_band(name):
    c = mv.case(name)
    r = mv.ref(name, "f64")
    reg = r["reg"].reshape(c["dims"], order="F")[mv.band(name)]
    won = sorted(set(int(v) for v in reg))
    print(f"[meshvel] {name}: regions that win in the band: {[mv.REGION_NAMES[c['D']][q] for q in won]}")
    if name in mv.TINY:
        # 45 and 27 samples, 5 and 8 cells apart, around a 7×5×3 box: no sample has two coordinates inside the box's extent, so no face can win, and the
        # eight corners alone cannot spend all six edge and vertex labels of the triangles — these lattices are here for the ragged bricks
        assert len(won) >= 2, (name, won)
        return
    assert won == list(range(mr.NREG[c["D"]])), (name, won)


@pytest.mark.parametrize("name", sorted(mv.CASES))
def test_velocity_varies_across_every_winning_element(name):
    c = mv.case(name)
    winners = np.unique(mv.ref(name, "f64")["elem"])
    wt = c["Wv"][c["E"][winners]]                                   # (winners, D vertices, D)
    spread = np.abs(wt - wt[:, :1]).max(axis=(1, 2))
    assert (spread > 1e-4).all(), (name, int((spread <= 1e-4).sum()))


@pytest.mark.parametrize("name", ["cube-linear", "ico80-radial", "torus-linear", "cube-3x3x3-rotation", "foil2d-wave"])
def test_a_uniform_velocity_is_reproduced_exactly_in_float32(name):
    c = mv.case(name)
    U = mv.uniform(c["V"])
    W = mv.sdf_points(c["D"], c["V"], c["E"], U, mv.positions(c), f32)["W"]
    assert W.dtype == f32 and np.array_equal(W.view(np.uint32), np.broadcast_to(U[0], W.shape).astype(f32).view(np.uint32))


@pytest.mark.parametrize("name", ["cube-linear", "lprism-rotation", "ico80-radial", "torus-linear", "foil2d-wave"])
def test_W_is_continuous_across_shared_edges(name):
    """a sample whose closest point lies on a shared edge or vertex has several elements at the same distance, and which of them wins depends on the order
    of the elements and on rounding.  W must not care.
    (i) Float64, the elements in reverse order (the LAST of equal minima wins): W moves by rounding alone on every non-ambiguous sample.
    (ii) Float32 against Float64: where the two pick different winners, the loser's true d² exceeds the winner's by at most the two rounding errors, 2·G with
    G = max|d²₃₂ − d²₆₄|; on one sheet of the surface d₂² = d₁² + ℓ², so the two closest points lie ℓ ≤ √(2·G) apart (×2: the sheet may bend), and W, linear
    on every element, moves by at most Lip·ℓ with Lip = max over element edges of |w_i − w_j|/|x_i − x_j|, plus the gap where the winners agree."""
    c = mv.case(name)
    D = c["D"]
    r32, r64 = mv.ref(name, "f32"), mv.ref(name, "f64")
    ok = ~mv.ambiguous(name).reshape(-1, order="F")
    W32 = r32["W"].reshape(-1, D, order="F").astype(f64)
    W64 = r64["W"].reshape(-1, D, order="F")
    Wr = mv.sdf_points(D, c["V"], c["E"][::-1].copy(), c["Wv"], mv.positions(c), f64)["W"]
    assert np.abs(Wr - W64)[ok].max() <= 1e-9 * (1 + float(np.abs(W64).max())), name
    flips = (r32["elem"] != r64["elem"]) & ok
    dW = np.abs(W32 - W64).max(axis=1)
    G = float(np.abs(r32["d"].astype(f64) ** 2 - r64["d"] ** 2).max())
    P, Wv = c["V"].astype(f64)[c["E"]], c["Wv"].astype(f64)[c["E"]]
    lip = max(float((np.linalg.norm(Wv[:, a] - Wv[:, b], axis=1) / np.linalg.norm(P[:, a] - P[:, b], axis=1)).max()) for a in range(D) for b in range(a))
    same = float(dW[ok & ~flips].max(initial=0.0))
    bound = same + lip * 2 * np.sqrt(2 * G)
    print(f"[meshvel] {name}: winner flips between Float32 and Float64 on {int(flips.sum())} non-ambiguous samples; max|ΔW| there {dW[flips].max(initial=0):.2e}, "
          f"where the winners agree {same:.2e}; G {G:.2e}, Lip {lip:.3f}, bound {bound:.2e}")
    assert dW[flips].max(initial=0.0) <= bound


def test_barycentric_pair_reproduces_the_closest_point():
    """(v, w) is read off the region, never solved for: A + v·(B − A) + w·(C − A) must be the closest point p − r the walk computed"""
    for name in ("lprism-rotation", "ico80-radial", "foil2d-wave"):
        c = mv.case(name)
        r = mv.ref(name, "f64")
        P = c["V"].astype(f64)[c["E"][r["elem"]]]
        q = P[:, 0] + r["v"][:, None] * (P[:, 1] - P[:, 0])
        if c["D"] == 3:
            q = q + r["w"][:, None] * (P[:, 2] - P[:, 0])
        assert np.abs(q - (mv.positions(c).astype(f64) - r["r"])).max() < 1e-9, name
        assert (r["v"] >= 0).all() and (r["w"] >= 0).all() and (r["v"] + r["w"] <= 1 + 1e-12).all()


def test_distances_are_those_of_the_static_restatement():
    for name in ("cube-linear", "torus-linear", "foil2d-wave"):
        c = mv.case(name)
        for T in (f32, f64):
            a = mv.sdf_points(c["D"], c["V"], c["E"], c["Wv"], mv.positions(c), T)
            b = mr.sdf_points(c["D"], c["V"], c["E"], mv.positions(c), T)
            assert np.array_equal(a["d"], b["d"]) and np.array_equal(a["elem"], b["elem"]) and np.array_equal(a["reg"], b["reg"])


def test_leaf_velocity_restatement_on_a_linear_field():
    """interp of a linear field is exact up to rounding inside the box: unmapped the leaf returns A·x + b; under a map R̂ᵀ(A·ξ + b) on top of the rigid part"""
    import lattice_ref as lr
    from waterlily_jl_amd.bodies import RigidMap
    dims, origin, s = (12, 11, 10), (1.0, 0.5, -0.5), 1.0
    vals = lr.sphere_values(dims, origin, s, (6.0, 5.5, 4.0), 3.0)
    A, b = mv._A, np.array([0.3, -0.2, 0.1])
    lat = mv.VelLattice(vals, mv.linear_W(dims, origin, s, A, b))
    rng = np.random.default_rng(3)
    X = (np.array([6.0, 5.5, 4.0]) + rng.uniform(-3.4, 3.4, size=(200, 3))).astype(f32)      # inside the lattice's box: nothing is clamped
    body = lr.lattice_body(lat, origin, s)
    d, n, V = mv.points(body, X, np.inf, f64)
    assert np.abs(V - (X.astype(f64) @ A.T + b)).max() < 1e-6
    mp = RigidMap((0.5, -0.3, 0.2), (0.3, -0.2, 0.5), V=(0.1, -0.2, 0.05), omega=(0.02, 0.01, -0.03))
    body = lr.lattice_body(lat, origin, s, map=mp)
    X = ((X.astype(f64) - mp.xp) @ mp.R.astype(f64) + mp.x0 + mp.xp).astype(f32)      # the same body-frame points, carried to the flow frame
    d, n, V = mv.points(body, X, np.inf, f64)
    _, _, V0 = lr.points(lr.lattice_body(lr.HostLattice(vals), origin, s, map=mp), X, np.inf, f64)
    R = mp.R.astype(f64)
    xi = (X.astype(f64) - mp.x0 - mp.xp) @ R.T + mp.xp
    assert np.abs(V - (V0 + (xi @ A.T + b) @ R)).max() < 1e-6
    # the exits keep n = V = 0, and a lattice without W goes where it went
    d, n, V = mv.points(body, X, 0.25, f32)
    far = ~n.any(axis=1)                                            # (past the exit d is the raw sample, else d/|∇d|: the exit is read off n)
    assert far.any() and (~far).any() and (d[far] * d[far] > 0.25).all() and not V[far].any() and V[~far].all(axis=1).any()
    for T in (f32, f64):
        for x, y in zip(mv.points(lr.lattice_body(mv.VelLattice(vals), origin, s, map=mp), X, 9.0, T), lr.points(lr.lattice_body(lr.HostLattice(vals), origin, s, map=mp), X, 9.0, T)):
            assert np.array_equal(x, y)


def test_entry_points_are_declared_bound_and_built():
    import waterlily_jl_amd as w
    L = w.lib()
    hdr = open(os.path.join(ROOT, "include", "wlhip.h"), encoding="utf-8").read()
    for name, arity in (("wl_sdf_lattice_from_moving_mesh", 12), ("wl_sdf_lattice_update_mesh", 5), ("wl_sdf_lattice_set_velocity", 3),
                        ("wl_sdf_lattice_read_velocity", 3), ("wl_sdf_lattice_has_velocity", 1)):
        assert hasattr(L, name) and len(w.SIGNATURES[name][1]) == arity and name + "(" in hdr, name
    assert L.wl_sdf_lattice_has_velocity(None) == 0
    for name in ("update_mesh", "advance", "set_velocity", "velocity", "has_velocity"):
        assert hasattr(w.SdfLattice, name)


def test_python_surface_checks_shapes_before_the_library():
    c = mv.case("cube-linear")
    with pytest.raises(ValueError):
        bodies.SdfLattice.from_mesh(c["V"], c["E"], c["dims"], vertex_velocity=c["Wv"][:-1])
    with pytest.raises(ValueError):
        bodies.mesh_body(c["V"], c["E"], vertex_velocity=c["Wv"][:, :2])
