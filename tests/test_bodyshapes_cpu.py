"""What keeps tests/test_gpu_bodyshapes.py from being hollow, checked without a GPU: every restated body-side gate still quotes its source, every position of
tests/bodyshapes.py SHAPE_CASES holds the classes it claims (μ₀, μ₁, V from the oracle's measure!, the coarse L from the oracle's hierarchy), every class is
claimed, every gate has a position on each side and each pair flips what the table says, zsplit_plan_level is bodypaths_ref.zsplit_plan on level 0, the three
ranges of a split level tile its planes, and the restatement is pinned on fields small enough to classify by hand."""
import os

import numpy as np
import pytest

import bodypaths_ref as bp
import bodyshapes as bs
import shapegates as sg
from test_bodypaths_cpu import _blank, fields_cpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CASES, N_POSITIONS, N_PAIRS = 31, 41, 23      # the counts README.md states
_CACHE = {}


def levels_L(oracle, mu0):
    """L of every multigrid level from the oracle's hierarchy on L = μ₀ (restrictL! level by level)"""
    Ng = mu0.shape[:-1]
    x, z = np.zeros(Ng, f32, order="F"), np.zeros(Ng, f32, order="F")
    po = oracle.MultiLevelPoisson(x, np.asfortranarray(mu0.copy()), z)
    return [np.array(po.field("L", l)) for l in range(po.nlevels)]


def evaluated(oracle, cid, q):
    if (cid, q) not in _CACHE:
        case = bs.all_cases()[cid]
        mu0, mu1, V = fields_cpu(oracle, case["positions"][q][0], case["dims"], case["perdir"], case["exitBC"])
        _CACHE[(cid, q)] = bs.evaluate(case, mu0, mu1, V, levels_L(oracle, mu0))
        _CACHE[(cid, q)]["mu0"] = mu0
    return _CACHE[(cid, q)]


POSITIONS = [(c, q) for c in bs.SHAPE_CASES for q in range(len(c["positions"]))]


@pytest.mark.parametrize("case,q", POSITIONS, ids=[f"{c['id']}-{q}" for c, q in POSITIONS])
def test_position_holds_the_classes_it_claims(oracle, case, q):
    e = evaluated(oracle, case["id"], q)
    conds = case["positions"][q][1]
    assert conds, case["id"]
    for name in conds:
        assert bs.cond(name)(e["c"], e["Ng"], e["tr"], e["plans"]), (case["id"], q, name, e["c"], e["tr"], e["plans"][:2])
    assert [tuple(L.shape[:-1]) for L in levels_L(oracle, e["mu0"])] == sg.levels(case["dims"])      # the hierarchy parts() and state() index


def test_every_class_is_claimed_and_the_list_stays_under_its_caps():
    claimed = {n for c in bs.SHAPE_CASES for _, conds in c["positions"] for n in conds}
    assert set(bs.SHAPE_CONDS) <= claimed, set(bs.SHAPE_CONDS) - claimed
    assert claimed <= set(bs.SHAPE_CONDS) | set(bp.CONDS), claimed - set(bs.SHAPE_CONDS) - set(bp.CONDS)
    assert not set(bs.SHAPE_CONDS) & set(bp.CONDS)
    ids = [c["id"] for c in bs.SHAPE_CASES]
    assert len(ids) == len(set(ids)) == N_CASES <= bs.MAX_CASES and not set(ids) & {c["id"] for c in bp.CASES}
    assert len(POSITIONS) == N_POSITIONS
    big = []
    for c in bs.SHAPE_CASES:
        Ng = [n + 2 for n in c["dims"]]
        assert int(np.prod(Ng)) <= bs.CELL_CAP, c["id"]
        assert len(sg.levels(c["dims"])) >= 3, c["id"]
        assert not c["perdir"] and not c["remeasure_each_step"], c["id"]
        if int(np.prod(Ng)) > bs.ORACLE_CELLS:
            big.append(c["id"])
    assert big == bs.PLAIN_ONLY
    # V ≠ 0 where the issue asks for it: near is then wider than μ₁ ≠ 0
    for cls in ("whole_wgs", "row_over_wg", "part_low_short"):
        assert any(cls in conds and "v_cells" in conds for c in bs.SHAPE_CASES for _, conds in c["positions"]), cls
    assert all(any(ch.isdigit() for ch in why) for why in bs.UNREACHABLE.values()) and not set(bs.UNREACHABLE) & claimed      # (whatever is listed carries its arithmetic)
    assert {"part_level0_not_level1", "part_level1_not_level0"} <= claimed


def test_every_quoted_expression_is_still_in_its_file():
    """a gate edited in the library without this table fails here"""
    text = {}
    quotes = [(g.file, q) for g in bs.GATES.values() for q in g.quotes] + list(bs.QUOTED)
    assert len(quotes) >= 35
    for f, q in quotes:
        if f not in text:
            with open(os.path.join(ROOT, *bs.CSRC, f), encoding="utf-8") as fh:
                text[f] = fh.read()
        assert q in text[f], (f, q)
    assert {"conv_tile_ok_body", "join_low", "join_high", "body_masks_nbm", "needf_loop", "part", "zsplit_ranges", "gsrb_pair_ok_range", "hybrid_ok"} <= set(bs.GATES)
    for g in bs.GATES.values():
        assert g.quotes and g.doc, g.name
    # the constants the restatement carries
    assert "static constexpr int ZSPLIT_MARGIN = %d;" % bs.ZSPLIT_MARGIN in text["wl_mg.hpp"] and "#define WL_BLOCK %d" % bs.WG in open(os.path.join(ROOT, *bs.CSRC, "wl_common.hpp"), encoding="utf-8").read()


def test_every_gate_has_a_position_on_each_side_and_each_pair_flips_what_the_table_says(oracle):
    assert len(bs.PAIRS) == N_PAIRS
    assert set(bs.GATES) <= {p["gate"] for p in bs.PAIRS}, set(bs.GATES) - {p["gate"] for p in bs.PAIRS}
    want = {"conv_tile_ok_body": 2, "join_low": 1, "join_high": 2, "body_masks_nbm": 3, "needf_loop": 1, "row_over_wg": 2, "row_over_2wg": 1, "whole_wgs": 2, "part": 5, "zsplit_ranges": 1,
            "gsrb_pair_ok_range": 1, "hybrid_ok": 1, "far_tile_whole": 1}      # removing a pair fails here
    assert {g: sum(1 for p in bs.PAIRS if p["gate"] == g) for g in want} == want and {p["gate"] for p in bs.PAIRS} == set(want)
    for p in bs.PAIRS:
        a, b = (bs.view(evaluated(oracle, *p[k])["state"]) for k in ("a", "b"))
        assert a[p["gate"]] != b[p["gate"]], (p["gate"], p["clause"], a[p["gate"]], b[p["gate"]])
        flips = {k for k in a if a[k] != b[k]} - {p["gate"]}
        print("%-18s %-22s | %-22s %s: also flips %s" % (p["gate"], "%s/%d" % p["a"], "%s/%d" % p["b"], p["clause"], sorted(flips) or "nothing"))
        assert flips == set(p["flips"]), (p["gate"], p["clause"], sorted(flips))


def test_each_pair_has_a_read_out_or_says_why_not(oracle):
    """the predicted path set (hybrid, body_tile launches per call of conv_diff!, kind per level, part per level) differs between the two sides of a pair, or
    the gate's read-out is the census"""
    for p in bs.PAIRS:
        a, b = (bs.paths(evaluated(oracle, *p[k])["state"]) for k in ("a", "b"))
        if p["gate"] in bs.NO_READOUT or p["gate"] in ("row_over_wg", "row_over_2wg", "whole_wgs"):      # (the three thresholds of the mask kernels: the census)
            ea, eb = (evaluated(oracle, *p[k]) for k in ("a", "b"))      # no dispatch differs: the quantity named as the read-out must
            ra, rb = bs.READOUT[p["gate"]](ea), bs.READOUT[p["gate"]](eb)
            assert ra is not None and rb is not None and ra != rb, (p["gate"], p["clause"], ra, rb)
            continue
        assert a != b, (p["gate"], p["clause"], a)
    assert set(bs.NO_READOUT) <= set(bs.GATES) and set(bs.READOUT) == set(bs.NO_READOUT) | {"row_over_wg", "row_over_2wg", "whole_wgs"}
    # the ±sy neighbours are what the census of the long-row positions rests on: a loop without them counts fewer needf-only workgroups there
    for cid, q in (("row-256", 0), ("row-256", 1), ("row-512", 0), ("row-512", 1), ("c2d-300x20", 0)):
        c = evaluated(oracle, cid, q)["c"]
        assert c["_needf_only_wo_y"] < c["mask_needf_only"] and c["_needf_y_only"] > 0, (cid, q)


def test_plan_level_is_the_existing_plan_on_level_0_and_the_oracles_L_below(oracle):
    for case in list(bp.CASES) + bs.SHAPE_CASES:
        for q, (body, _) in enumerate(case["positions"]):
            if len(case["dims"]) != 3:
                continue
            e = evaluated(oracle, case["id"], q)
            assert tuple(e["plans"][0][:3]) == bp.zsplit_plan(e["mu0"], case["perdir"]), (case["id"], q)
    # the hierarchy on L = μ₀ is the one a Simulation builds: level_field("L", l) of the oracle, level by level
    for cid in ("part-short", "far-16-15", "pairgeom-33x32", "level1"):
        case = bs.all_cases()[cid]
        so = oracle.Simulation(case["dims"], (1.0, 0.0, 0.0), 8.0, U=1, nu=0.02, body=case["positions"][0][0], T=f32)
        Ls = levels_L(oracle, evaluated(oracle, cid, 0)["mu0"])
        assert so.nlevels == len(Ls)
        for l, L in enumerate(Ls):
            assert np.array_equal(np.array(so.level_field("L", l)), L), (cid, l)
            assert bs.zsplit_plan_level(np.array(so.level_field("L", l)), L.shape[:-1]) == evaluated(oracle, cid, 0)["plans"][l]
    e = evaluated(oracle, "level1", 0)
    assert [p.part for p in e["plans"]][:3] == [True, True, False] and e["kinds"][:3] == [3, 3, 1]
    assert e["plans"][1][:5] == (True, 19, 30, 15, 35)


def test_the_three_ranges_tile_the_planes_and_the_far_ranges_keep_clear_of_the_body(oracle):
    """for every position of a part_* class and every split level: parts() tiles [k0, k1) exactly, the middle range holds every deviating plane, and every plane
    that runs with the constant pattern is clear of the deviating operators by the blocked kernels' reach"""
    seen = 0
    for case, q in POSITIONS:
        if not any(n.startswith("part") for n in case["positions"][q][1]):
            continue
        e = evaluated(oracle, case["id"], q)
        lv = sg.levels(case["dims"])
        Ls = levels_L(oracle, e["mu0"])
        for l, plan in enumerate(e["plans"]):
            if not plan.part:
                continue
            seen += 1
            k0, k1 = 1, lv[l][2] - 1
            pr = bs.parts(plan, lv[l])
            planes = sorted(k for a, b in pr for k in range(a, b))
            assert planes == list(range(k0, k1)), (case["id"], q, l, pr)
            assert pr[0] == (max(k0, plan.za - 4), min(k1, plan.zb + 5)) and pr[1][0] == k0 and pr[2][1] == k1
            assert plan.far == sum(b - a for a, b in pr[1:]) and plan.far >= 16 and 4 * plan.far >= k1 - k0
            middle = set(range(*pr[0]))
            assert set(range(max(k0, plan.za), min(k1, plan.zb + 1))) <= middle
            # which ConstL a plane runs with: the far ranges take the constant pattern (clp), so the operator of every plane within kernel B's reach of 3 planes of
            # one must be ON the pattern in the level's own L (a cell reads L of its plane and the z-face coefficient of the plane above)
            c, pat = bs.const_pattern(Ls[l], lv[l])
            off, offz = (Ls[l] != pat).any((0, 1, 3)), (Ls[l][..., 2] != pat[..., 2]).any((0, 1))
            op_off = off | np.append(offz[1:], False)
            for a, b in pr[1:]:
                for k in range(a, b):
                    assert not op_off[max(0, k - 3):k + 4].any(), (case["id"], q, l, k)
            assert op_off[max(k0, plan.za):min(k1, plan.zb + 1)].any()
    assert seen >= 8
    # the class names say what they say
    e = evaluated(oracle, "part-short", 0)
    assert bs.parts(e["plans"][0], e["Ng"]) == [(4, 24), (1, 4), (24, 49)]
    e = evaluated(oracle, "part-middle-min", 0)
    assert bs.parts(e["plans"][0], e["Ng"]) == [(21, 30), (1, 21), (30, 49)]      # one deviating plane: 4 + 1 + 4 planes, [za − 4, za + 5)
    e = evaluated(oracle, "far-16-15", 0)
    assert bs.parts(e["plans"][0], e["Ng"]) == [(17, 49), (1, 17), (49, 49)]
    assert [bs.part_kernel(n) for n in (0, 1, 3, 7, 8, 16)] == [None, "one-cell", "one-cell", "one-cell", "pair", "pair"]


def test_restatement_on_a_plane_of_whole_workgroups_classified_by_hand():
    """64 × 32 × 6 with ghosts: 2048 cells per plane = workgroups 0..7, none partial; nbm = 8, so slot 7 is the last that exists"""
    Ng = (64, 32, 6)
    mu0, mu1, V = _blank(Ng)
    assert bp.nbm(Ng) == 8 and bp.census(mu0, mu1, V)["near_b0"] == 8
    # the very last cell of plane 3 (i = 63, j = 31: m = 2047): near (3,7); needf m−1 -> (3,7), m+1 = 2048 is outside the plane, m−64 -> (3,7), m+64 outside, planes 2 and 4 -> (2,7), (4,7)
    mu1[63, 31, 3, 0, 0] = 0.5
    near, needf, m0var = bp.masks(mu0, mu1, V)
    assert sorted(zip(*np.nonzero(near))) == [(3, 7)] and sorted(zip(*np.nonzero(needf))) == [(2, 7), (3, 7), (4, 7)] and m0var.sum() == 0
    # the first cell of workgroup 7 (m = 1792: i = 0, j = 28): m−1 -> (3,6), m−64 = 1728 -> (3,6)
    mu1[0, 28, 3, 1, 1] = 0.25
    near, needf, _ = bp.masks(mu0, mu1, V)
    assert sorted(zip(*np.nonzero(needf))) == [(2, 7), (3, 6), (3, 7), (4, 7)]
    c = bs.census_shapes(mu0, mu1, V)
    assert (c["mask_near"], c["mask_needf_only"], c["near_b0"], c["near_b1"], c["near_k0"], c["near_k1"], c["dirty_z0"], c["dirty_z1"]) == (1, 3, 7, 7, 3, 3, 2, 4)
    assert c["_last_wg_near"] == 1 and c["_needf_y_only"] == 0      # (3,6) is reached through m−1 as well
    assert bs.SHAPE_CONDS["whole_wgs"](c, Ng, (None, None, 0), []) and not bp.CONDS["last_wg_near"](c, Ng, (None, None, 0), (False, 6, -1))
    assert np.array_equal(bs.needf_mask(mu1), needf)
    # V alone in workgroup 0 of ghost plane 0 widens the box to every slot of the plane
    V[5, 0, 0, 0] = 0.25
    c = bp.census(mu0, mu1, V)
    assert (c["near_b0"], c["near_b1"], c["near_k0"], c["near_k1"], c["mask_clean_in_box"]) == (0, 7, 0, 3, 8 * 4 - 2)


def test_restatement_on_rows_longer_than_two_workgroups_classified_by_hand():
    """514 × 6 × 5 with ghosts: 3084 cells per plane = 12.05 workgroups, nbm = 16; a row is 2.008 workgroups long"""
    Ng = (514, 6, 5)
    mu0, mu1, V = _blank(Ng)
    assert bp.nbm(Ng) == 16
    # one cell at i = 300, j = 3: m = 1842 -> workgroup 7.  m±1 -> 7; m−514 = 1328 -> 5; m+514 = 2356 -> 9; planes 1 and 3 -> (1,7), (3,7).  Nothing in 6 or 8
    mu1[300, 3, 2, 0, 1] = 0.5
    near, needf, _ = bp.masks(mu0, mu1, V)
    assert sorted(zip(*np.nonzero(near))) == [(2, 7)]
    assert sorted(zip(*np.nonzero(needf))) == [(1, 7), (2, 5), (2, 7), (2, 9), (3, 7)]
    assert np.array_equal(bs.needf_mask(mu1), needf)
    assert sorted(zip(*np.nonzero(bs.needf_mask(mu1, ("x", "z"))))) == [(1, 7), (2, 7), (3, 7)]
    c = bs.census_shapes(mu0, mu1, V)
    assert (c["mask_near"], c["mask_needf_only"], c["_needf_y_only"], c["_needf_only_wo_y"]) == (1, 4, 2, 2)
    assert c["_y_wg_dist"] == (2,) and bs.SHAPE_CONDS["row_over_wg"](c, Ng, (None, None, 0), []) and not bs.SHAPE_CONDS["row_over_2wg"](c, Ng, (None, None, 0), [])
    # the last-but-one cell of workgroup 7, m = 2046 (i = 504, j = 3): m+514 = 2560 -> workgroup 10, three away; m−514 = 1532 -> 5
    mu0, mu1, V = _blank(Ng)
    mu1[504, 3, 2, 0, 1] = 0.5
    assert sorted(zip(*np.nonzero(bp.masks(mu0, mu1, V)[1]))) == [(1, 7), (2, 5), (2, 7), (2, 10), (3, 7)]
    c = bs.census_shapes(mu0, mu1, V)
    assert c["_y_wg_dist"] == (2, 3) and bs.SHAPE_CONDS["row_over_2wg"](c, Ng, (None, None, 0), [])
    # 258 cells per row: m = 100 + 3·258 = 874 -> 3; m−258 = 616 -> 2; m+258 = 1132 -> 4: the next workgroups, never the cell's own
    Ng = (258, 6, 5)
    mu0, mu1, V = _blank(Ng)
    mu1[100, 3, 2, 1, 0] = 0.5
    near, needf, _ = bp.masks(mu0, mu1, V)
    assert sorted(zip(*np.nonzero(needf))) == [(1, 3), (2, 2), (2, 3), (2, 4), (3, 3)]
    # the last cell of a workgroup, m = 1023 (i = 249, j = 3): m+1 -> 4, m+258 = 1281 -> 5: two workgroups away
    mu0, mu1, V = _blank(Ng)
    mu1[249, 3, 2, 1, 0] = 0.5
    assert sorted(zip(*np.nonzero(bp.masks(mu0, mu1, V)[1]))) == [(1, 3), (2, 2), (2, 3), (2, 4), (2, 5), (3, 3)]


def test_restatement_in_2d_classified_by_hand():
    """128 × 14 with ghosts: 1792 cells = 7 whole workgroups, nbm = 8 (slot 7 exists and no cell maps to it); 302 × 6: rows of 1.18 workgroups"""
    Ng = (128, 14)
    mu0, mu1, V = _blank(Ng)
    assert bp.nbm(Ng) == 8
    mu1[127, 13, 0, 0] = 0.5                   # m = 1791, the last cell: near (0,6); m−1, m−128 -> (0,6); m+1 and m+128 are outside
    V[0, 0, 1] = 0.25                          # m = 0: near (0,0), asks for no f
    near, needf, m0var = bp.masks(mu0, mu1, V)
    assert sorted(zip(*np.nonzero(near))) == [(0, 0), (0, 6)] and sorted(zip(*np.nonzero(needf))) == [(0, 6)] and m0var.sum() == 0
    c = bs.census_shapes(mu0, mu1, V)
    assert (c["near_b0"], c["near_b1"], c["near_k0"], c["near_k1"], c["dirty_z0"], c["dirty_z1"], c["mask_clean_in_box"]) == (0, 6, 0, 0, 0, 0, 5)
    assert bs.SHAPE_CONDS["whole_wgs_2d"](c, Ng, (None, None, 0), []) and bs.SHAPE_CONDS["nbm8_2d"](c, Ng, (None, None, 0), [])
    assert bp.tile_ranges(c, Ng)[2] == 0 and bs.zsplit_plan_level(mu0, Ng).part is False and bs.smoother_kind_level(mu0, Ng) == 0
    Ng = (302, 6)
    mu0, mu1, V = _blank(Ng)
    mu1[200, 2, 1, 1] = 0.5                    # m = 804 -> 3; m−302 = 502 -> 1; m+302 = 1106 -> 4: workgroup 2 is skipped below
    near, needf, _ = bp.masks(mu0, mu1, V)
    assert sorted(zip(*np.nonzero(needf))) == [(0, 1), (0, 3), (0, 4)]
    c = bs.census_shapes(mu0, mu1, V)
    assert c["_needf_y_only"] == 2 and bs.SHAPE_CONDS["row_over_wg_2d"](c, Ng, (None, None, 0), [])


def test_plan_level_on_fields_classified_by_hand():
    """the z-split's arithmetic at its edges on 66 × 34 × 50 (48 interior planes, k0 = 1, k1 = 49) and its geometry clauses"""
    Ng = (66, 34, 50)
    L = bp.wall_pattern(Ng).copy()
    assert bs.zsplit_plan_level(L, Ng) == bs.Plan(False, 50, -1, None, None, 0, 48, "const") and bs.smoother_kind_level(L, Ng) == 2
    L[30, 10, 25, 1] = 0.5                                        # one plane: [21, 30), 39 far planes
    assert bs.zsplit_plan_level(L, Ng) == bs.Plan(True, 25, 25, 21, 30, 39, 48, "far") and bs.smoother_kind_level(L, Ng) == 3
    assert bs.smoother_kind_level(L, Ng, min_cells=bs.ZSPLIT_MIN_DEFAULT) == 1 and bs.smoother_kind_level(L, Ng, constl=False) == 1
    L[30, 10, 3, 1] = 0.5                                         # 3..25: [1, 30): the lower range is empty, 19 far planes above
    assert bs.zsplit_plan_level(L, Ng)[:6] == (True, 3, 25, 1, 30, 19)
    L[30, 10, 28, 1] = 0.5                                        # 3..28: [1, 33), 16 far planes
    assert bs.zsplit_plan_level(L, Ng)[:6] == (True, 3, 28, 1, 33, 16)
    L[30, 10, 29, 1] = 0.5                                        # 15
    assert bs.zsplit_plan_level(L, Ng)[:6] == (False, 3, 29, 1, 34, 15)
    # the quarter rule: 16 far planes of 64 and of 65
    for nz, part in ((66, True), (67, False)):
        L = bp.wall_pattern((66, 34, nz)).copy()
        L[30, 10, 17:nz, 0] = 0.5                                 # 17..nz−1: [13, k1): 12 far planes … 21..: 16
        L[30, 10, 17:21, 0] = bp.wall_pattern((66, 34, nz))[30, 10, 17:21, 0]
        p = bs.zsplit_plan_level(L, (66, 34, nz))
        assert (p.part, p.za, p.far, p.np) == (part, 21, 16, nz - 2)
    # the geometry: ny = 32, odd nx, 7 planes, a periodic direction, c₀ = 0
    for shape in ((66, 32, 50), (67, 34, 50), (66, 34, 9)):
        L = bp.wall_pattern(shape).copy(); L[30, 10, 4, 1] = 0.5
        assert bs.zsplit_plan_level(L, shape).gate == "geom"
    assert bs.smoother_kind_level(bp.wall_pattern((66, 32, 50)), (66, 32, 50)) == 1 and bs.smoother_kind_level(bp.wall_pattern((32, 34, 50)), (32, 34, 50)) == 0
    L = bp.wall_pattern(Ng).copy(); L[30, 10, 25, 1] = 0.5
    assert bs.zsplit_plan_level(L, Ng, perdir=(1,)).gate == "geom" and bs.smoother_kind_level(L, Ng, perdir=(1,)) == 0
    L[2, 2, 2, 0] = 0.0
    assert bs.zsplit_plan_level(L, Ng).gate == "c0"
