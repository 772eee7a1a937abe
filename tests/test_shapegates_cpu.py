"""What keeps tests/test_gpu_shapegates.py from being hollow, checked without a GPU: every restated gate still quotes its source, every gate has a shape on
each side, each pair flips exactly the gates the table says it flips, the restated hierarchy is the oracle's, the list stays under its caps and predicted()
agrees with optmatrix.live() where the two overlap."""
import os

import numpy as np
import pytest

import callseq
import optmatrix as om
import shapegates as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_SHAPES = 40
N_SHAPES, N_CASES = 39, 45      # the counts README.md states


def text(name):
    with open(os.path.join(ROOT, *sg.CSRC, name), encoding="utf-8") as f:
        return f.read()


def test_every_quoted_expression_is_still_in_its_file():
    """a gate edited in the library without this table fails here"""
    quotes = [(g.file, q) for g in sg.GATES.values() for q in g.quotes] + [(c.file, q) for c in sg.CHOOSERS.values() for q in c.quotes] + list(sg.QUOTED)
    assert len(quotes) >= 50
    missing = [(f, q) for f, q in quotes if q not in text(f)]
    assert not missing, missing
    for g in sg.GATES.values():
        assert g.quotes and g.doc, g.name


def test_every_gate_has_a_shape_on_each_side():
    """every restated predicate is the subject of a pair whose two sides differ in it, or rests on one of the four named exemptions"""
    covered = {p["gate"] for p in sg.PAIRS}
    assert covered == set(sg.state((64, 32, 8))) - {"chunks:" + c for c in sg.CHOOSERS}, sorted(covered)
    assert set(sg.GATES) - {"check_const_L"} <= covered      # (check_const_L: every finest level here passes it; its bound is a coarse level's)
    for p in sg.PAIRS:
        assert sg.state(p["in"])[p["gate"]] != sg.state(p["out"])[p["gate"]], (p["gate"], p["clause"])
    assert sorted(sg.UNREACHABLE) == sorted(["WL_TAIL_MAXLV", "32-bit offsets (cs < 2^30, 3·cs < 2^31, tw_nb8·nz)", "WL_MAXPART in gsrb_pair_B_kernel_norms", "65536 partials in wl_march_chunk"])
    assert all(any(ch.isdigit() for ch in why) for why in sg.UNREACHABLE.values())      # the arithmetic is written next to the entry
    # the clauses of each predicate that a shape can flip, by name: removing a pair fails here
    want = {"gsrb_pair_geom_ok": 4, "gsrb_fused_ok": 3, "resjac_ok": 4, "conv_proj_ok": 4, "fold_ok": 1, "project_wide_path": 3, "conv_march_ok": 2, "conv_z_ok": 2, "conv_tile_ok": 1,
            "conv_tile_whole": 1, "rows16": 1, "tail_ok": 1, "level_cap": 2}
    assert {g: sum(1 for p in sg.PAIRS if p["gate"] == g) for g in covered} == want


def test_each_pair_flips_what_the_table_says():
    for p in sg.PAIRS:
        a, b = sg.state(p["in"]), sg.state(p["out"])
        flips = {k for k in a if a[k] != b[k]} - {p["gate"]}
        print("%-18s %-16s | %-16s %s: also flips %s" % (p["gate"], "×".join(map(str, p["in"])), "×".join(map(str, p["out"])), p["clause"], sorted(flips) or "nothing"))
        assert flips == set(p["flips"]), (p["gate"], p["clause"], sorted(flips))


def test_each_pair_has_a_read_out_or_says_why_not():
    """the two sides of a pair differ in the predicted kinds, counters or level count — what the GPU test holds the library to — unless the library has no read-out"""
    for p in sg.PAIRS:
        a, b = sg.predicted(p["in"], True, p["extra"]), sg.predicted(p["out"], True, p["extra"])
        differs = a["smoother_kinds"][0] != b["smoother_kinds"][0] or a["counters"] != b["counters"] or a["nlevels"] != b["nlevels"]
        if p["gate"] in sg.NO_READOUT:
            continue
        assert differs, (p["gate"], p["clause"])
    assert set(sg.NO_READOUT) <= {p["gate"] for p in sg.PAIRS}
    # the starting claims of the table, as predicted() sees them
    c = lambda N, ex=None: {k for k, v in sg.predicted(N, True, ex)["counters"].items() if v}
    assert c((64, 32, 8)) == set(sg.COUNTERS)
    assert c((62, 32, 8)) == {"rskip", "xdefer", "tailwide"}                               # pair kernels live; pdefer, bcdefer, tailspec read 0
    assert c((64, 16, 8)) == {"tailfuse", "tailwide"}                                      # tailfuse without the head
    assert c((64, 33, 8)) == set(sg.COUNTERS) - {"tailwide", "tailfuse"}                   # keeps the head and the pair kernels
    assert c((5632, 8, 8)) == set() and c((5624, 8, 8)) == {"tailwide"}                    # the LDS clause alone
    assert c((64, 32, 8), {"convz": 1}) == set(sg.COUNTERS) - {"bcdefer", "tailfuse"}
    assert [sg.predicted(N, True)["smoother_kinds"][0] for N in ((32, 32, 8), (32, 30, 8), (32, 16, 8), (30, 32, 8), (32, 14, 8), (32, 32, 6))] == [2, 1, 1, 0, 0, 0]
    assert sg.predicted((64, 32, 16), True)["smoother_kinds"][1] == 1 and sg.tail_first((64, 32, 16)) == 1 and sg.tail_first((64, 32, 32)) == 2
    # with nothing set the size gates keep the head, the tiled kernel and tailfuse out at every shape of the list
    for N in sg.SHAPES:
        assert c_default(N) <= {"tailwide", "rskip", "xdefer"}, N


def c_default(N):
    return {k for k, v in sg.predicted(N, False)["counters"].items() if v}


def test_chunk_classes():
    """every chooser has a shape per class it can reach on level 0 under the cap; the others carry their arithmetic"""
    for chooser, cls, N in sg.CHUNK_SHAPES:
        assert sg.chunk_classes(N)[chooser] == cls, (chooser, N, sg.chunk_classes(N))
    flat = lambda v: set(v) if isinstance(v, tuple) else {v}
    for chooser in sg.CHOOSERS:
        seen = set().union(*[flat(cls) for ch, cls, _ in sg.CHUNK_SHAPES if ch == chooser])
        missing = {"one", "whole", "ragged"} - seen
        assert missing <= {k[1].split()[0] for k in sg.CHUNK_UNREACHABLE if k[0] == chooser}, (chooser, missing)
    # N_z = 8 and 10 with the tests' 5-plane conv chunks: ragged (5 + 3) and whole (5 + 5)
    assert sg.conv_tile_chunk((66, 34, 10)) == 5 and sg.conv_tile_chunk((66, 34, 12)) == 5 and sg.conv_tile_chunk((66, 34, 6)) == 4
    # kernel B of the pair smoother at 448×365×8: 9 × 15 = 135 tiles of 56×26, 17 workgroups per XCD, one chunk; kernel A: 8 × 14 = 112 tiles, two chunks
    assert sg.ptile_count(450, 367, 4, 3, 32) == 135 and sg.zchunk2((450, 367, 10), 4, 3, 32) == 8 and sg.zchunk2((450, 367, 10), 2, 2, 32) == 4
    assert not sg.rows16((450, 367, 10)) and not sg.rows16((450, 366, 10)) and sg.rows16((450, 338, 10))


def test_caps():
    assert len(sg.SHAPES) == N_SHAPES <= MAX_SHAPES and len(sg.CASES) == N_CASES
    assert len({sg.case_id(c) for c in sg.CASES}) == len(sg.CASES)
    for N in sg.SHAPES:
        lv = sg.levels(N)
        assert len(lv) >= 3, N
        assert sg.cells(lv[0]) <= sg.CELL_CAP, N
        assert sg.const_L_ok(lv[0]), N
    assert sum(1 for N in sg.SHAPES if sg.cells(sg.levels(N)[0]) > sg.ORACLE_CELLS) <= 8      # the shapes held to the plain handle only
    assert sg.SEEDS == {} or all(len(v) == 3 for v in sg.SEEDS.values())


def test_levels_are_the_oracles(oracle):
    """levels(N) against oracle.coarsen_mask step by step and against the hierarchy the oracle's MultiLevelPoisson builds"""
    assert [sg.divisible(n) for n in range(1, 40)] == [oracle.divisible(n) for n in range(1, 40)]
    for N in sg.SHAPES:
        lv = sg.levels(N)
        for a, b in zip(lv, lv[1:]):
            assert tuple(1 + n // 2 if c else n for n, c in zip(a, oracle.coarsen_mask(a))) == b, (N, a, b)
        shape = lv[0]
        x, z = np.zeros(shape, dtype=np.float32, order="F"), np.zeros(shape, dtype=np.float32, order="F")
        L = np.ones(shape + (3,), dtype=np.float32, order="F")
        oracle.BC(L, (0, 0, 0))
        po = oracle.MultiLevelPoisson(x, L, z)
        assert [po.level_dims(l) for l in range(po.nlevels)] == lv, N
    assert sg.level_cap_cuts((4096, 8, 8)) and not sg.level_cap_cuts((2048, 8, 8)) and not sg.level_cap_cuts((3072, 8, 8))
    assert len(sg.levels((4096, 8, 8))) == len(sg.levels((3072, 8, 8))) == 11


@pytest.mark.parametrize("family", ["box", "ragged"])
def test_predicted_agrees_with_the_option_matrix(family):
    """at the shapes of the option matrix's body-free families, all switches at default"""
    N = callseq.DIMS[family]
    assert sg.conv_tile_whole(sg.levels(N)[0]) == om.FAMILIES[family]["whole_tiles"]
    got = {k for k, v in sg.predicted(N, True)["counters"].items() if v}
    assert got == om.live({}, family) & set(sg.COUNTERS), (family, sorted(got), sorted(om.live({}, family)))
    assert set(sg.COUNTERS) == set(om.COUNTED) - {"hybrid", "body_tile"}
