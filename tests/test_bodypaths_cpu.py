"""The geometries of tests/test_gpu_bodypaths.py really hold the mask classes they were chosen for — checked without a GPU: the coefficient
fields come from the oracle's measure! (closed forms) or from the NumPy restatement of the composite measure! (unions, intersections),
the classification from tests/bodypaths_ref.py.  Without this a device case could compare two runs of the same branch and prove nothing.
Also pins the restatement itself on fields small enough to classify by hand."""
import numpy as np
import pytest

import bodypaths_ref as bp

f32 = np.float32


def fields_cpu(oracle, body, dims, perdir=(), exitBC=False):
    """μ₀, μ₁, V with ghost cells, as measure!(flow, body) leaves them (None: a flow with a body that was never measured)"""
    D = len(dims)
    Ng = tuple(n + 2 for n in dims)
    if body is None or bp.is_set(body):
        mu0 = np.ones(Ng + (D,), f32, order="F"); mu1 = np.zeros(Ng + (D, D), f32, order="F"); V = np.zeros(Ng + (D,), f32, order="F")
        if body is not None:
            from test_gpu_bodyset import _measure_np
            _, r0, r1, rV, _ = _measure_np(bp.to_body(body), dims)
            inner = tuple(slice(1, n + 1) for n in dims)
            mu0[inner], mu1[inner], V[inner] = r0, r1, rV
        oracle.BC(mu0, (0.0,) * D, perdir=perdir)                       # src/Body.jl:49-50
        oracle.BC(V, (0.0,) * D, saveexit=exitBC, perdir=perdir)
        return mu0, mu1, V
    so = oracle.Simulation(dims, (1.0,) + (0.0,) * (D - 1), 8.0, U=1, nu=0.02, body=body, perdir=perdir, exitBC=exitBC, T=f32)
    return tuple(np.asfortranarray(so.field(k).copy()) for k in ("mu0", "mu1", "V"))


POSITIONS = [(c, q) for c in bp.CASES for q in range(len(c["positions"]))]


@pytest.mark.parametrize("case,q", POSITIONS, ids=[f"{c['id']}-{q}" for c, q in POSITIONS])
def test_geometry_holds_the_class_it_was_chosen_for(oracle, case, q):
    body, conds = case["positions"][q]
    Ng = tuple(n + 2 for n in case["dims"])
    mu0, mu1, V = fields_cpu(oracle, body, case["dims"], case["perdir"], case["exitBC"])
    c = bp.census_plus(mu0, mu1, V)
    tr = bp.tile_ranges(c, Ng, case["perdir"], case["store_f"])
    zp = bp.zsplit_plan(mu0, case["perdir"])
    assert conds, case["id"]
    for name in conds:
        assert bp.CONDS[name](c, Ng, tr, zp), (case["id"], q, name, c, tr, zp)


def test_every_class_of_the_matrix_is_claimed_by_some_geometry():
    claimed = {n for c in bp.CASES for _, conds in c["positions"] for n in conds}
    assert claimed == set(bp.CONDS), set(bp.CONDS) - claimed
    ids = [c["id"] for c in bp.CASES]
    assert len(ids) == len(set(ids)) and len(ids) <= 60
    for c in bp.CASES:
        assert all(n <= m for n, m in zip(c["dims"], (96, 48, 112))), c["id"]


def _blank(Ng):
    D = len(Ng)
    return bp.wall_pattern(Ng).copy(), np.zeros(tuple(Ng) + (D, D), f32), np.zeros(tuple(Ng) + (D,), f32)


def test_restatement_on_fields_classified_by_hand():
    """34 × 18 × 6 with ghosts: 612 cells per plane = workgroups 0, 1 (cells 256..511) and the partial 2 (512..611); nbm = 8"""
    Ng = (34, 18, 6)
    mu0, mu1, V = _blank(Ng)
    c = bp.census(mu0, mu1, V)
    assert c == {"mask_near": 0, "mask_needf_only": 0, "mask_m0var_only": 0, "mask_clean_in_box": 0, "dirty_z0": 6, "dirty_z1": -1,
                 "near_b0": 8, "near_b1": -1, "near_k0": 6, "near_k1": -1}
    # one cell with μ₁ ≠ 0 at m = 256 (i = 18, j = 7), plane 2: near (2,1); needf at m−1 -> (2,0), m+1, m±34 -> (2,1) and (2,0), planes 1 and 3 -> (1,1), (3,1)
    mu1[18, 7, 2, 0, 1] = 0.5
    near, needf, m0var = bp.masks(mu0, mu1, V)
    assert sorted(zip(*np.nonzero(near))) == [(2, 1)]
    assert sorted(zip(*np.nonzero(needf))) == [(1, 1), (2, 0), (2, 1), (3, 1)]
    assert m0var.sum() == 0
    c = bp.census(mu0, mu1, V)
    assert (c["mask_near"], c["mask_needf_only"], c["mask_m0var_only"], c["mask_clean_in_box"]) == (1, 3, 0, 0)
    assert (c["dirty_z0"], c["dirty_z1"], c["near_b0"], c["near_b1"], c["near_k0"], c["near_k1"]) == (1, 3, 1, 1, 2, 2)
    # V alone makes a workgroup near but asks for no f; μ₀ = 0 in the last partial workgroup of ghost plane 5 is m0var only
    V[3, 1, 4, 2] = 0.25                       # m = 37 -> (4,0)
    mu0[20, 16, 5, 0] = 0.0                    # m = 564 -> (5,2)
    c = bp.census(mu0, mu1, V)
    assert (c["mask_near"], c["mask_needf_only"], c["mask_m0var_only"]) == (2, 3, 1)
    assert (c["near_b0"], c["near_b1"], c["near_k0"], c["near_k1"]) == (0, 1, 2, 4)
    assert c["mask_clean_in_box"] == 6 - 2     # box: workgroups 0..1 × planes 2..4
    assert (c["dirty_z0"], c["dirty_z1"]) == (1, 5)
    # the wall pattern: a μ₀ of 1 on a wall-normal face is off the pattern, a μ₀ of 0 there is on it
    mu0, mu1, V = _blank(Ng)
    assert mu0[1, 5, 3, 0] == 0 and mu0[33, 5, 3, 0] == 0 and mu0[2, 5, 3, 0] == 1 and mu0[1, 5, 3, 1] == 1 and mu0[5, 5, 5, 2] == 0 and mu0[5, 5, 4, 2] == 1
    mu0[1, 5, 3, 0] = 1.0
    assert bp.census(mu0, mu1, V)["mask_m0var_only"] == 1


def test_restatement_in_2d_and_the_plane_ranges():
    Ng = (34, 18)
    mu0, mu1, V = _blank(Ng)
    mu1[18, 7, 1, 1] = 0.5                     # m = 256: near (0,1), needf (0,0) through m−1 and m−34
    c = bp.census(mu0, mu1, V)
    assert (c["mask_near"], c["mask_needf_only"], c["dirty_z0"], c["dirty_z1"], c["near_k0"], c["near_k1"]) == (1, 1, 0, 0, 0, 0)
    assert bp.tile_ranges(c, Ng)[2] == 0
    # conv_diff_bdim_body's ranges on 66 × 34 × 50: far ranges of 8 planes are tiled, of 7 they join the gather range
    Ng = (66, 34, 50)
    base = {"dirty_z0": 9, "dirty_z1": 40}
    assert bp.tile_ranges(base, Ng) == (9, 41, 2)
    assert bp.tile_ranges({"dirty_z0": 8, "dirty_z1": 40}, Ng) == (1, 41, 1)
    assert bp.tile_ranges({"dirty_z0": 8, "dirty_z1": 41}, Ng) == (1, 49, 0)
    assert bp.tile_ranges({"dirty_z0": 0, "dirty_z1": 49}, Ng) == (1, 49, 0)
    assert bp.tile_ranges({"dirty_z0": 50, "dirty_z1": -1}, Ng)[2] == 0
    assert bp.tile_ranges(base, Ng, perdir=(1,))[2] == 0 and bp.tile_ranges(base, Ng, store_f=True)[2] == 0
    # the z-split: planes 20..24 off the pattern -> ranges [1,16) and [29,49): 35 far planes
    mu0 = bp.wall_pattern(Ng).copy()
    assert bp.zsplit_plan(mu0) == (False, 50, -1)
    mu0[30, 10, 20:25, 1] = 0.5
    assert bp.zsplit_plan(mu0) == (True, 20, 24)
    mu0[30, 10, 8, 1] = 0.5; mu0[30, 10, 38, 1] = 0.5          # [1,4) and [43,49): 9 far planes
    assert bp.zsplit_plan(mu0) == (False, 8, 38)
