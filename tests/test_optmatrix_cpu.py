"""What keeps tests/test_gpu_optmatrix.py from being hollow, checked without a GPU: the matrix knows every switch the library has, the rows hold every pair (every
triple of the step-level switches), every counted path runs next to every value the header does not exempt, each exemption quotes the header, the generator is
deterministic and the row counts stay under the caps that bound the GPU time."""
import itertools
import os
import re

import pytest

import optmatrix as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR_CAP, TRIPLE_CAP = 32, 80
# the counts README.md states (a change of the generator, of live() or of STANDS_DOWN moves them: then both are updated together)
PAIR_ROWS = {"box": 26, "ragged": 26, "periodic": 18, "moving": 24, "exit": 26, "circle2d": 25}
TRIPLE_ROWS = 47


def text(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as f:
        return f.read()


def header_option_comment():
    h = text("include", "wlhip.h")
    a, b = h.index("/* implementation switches"), h.index("int wl_reset_process_options(void);")
    return h[a:b]


def one_line(s):
    return re.sub(r"\s+", " ", s)


def test_every_switch_of_the_library_is_a_factor_or_excluded():
    """a switch added later fails here until it joins the matrix"""
    quoted = set(re.findall(r'(?<!\()"([a-z_0-9]+)"', header_option_comment()))      # (not the argument of a call: wl_sim_field("p"))
    src = text("waterlily.jl_amd", "csrc", "wl_sim.hip")
    body = src[src.index("int wl_sim_set_option("):src.index("int wl_sim_update(")]
    accepted = set(re.findall(r'if \(n == "([a-z_0-9]+)"\)', body))
    assert len(accepted) >= 40 and len(quoted) >= 35, (len(accepted), len(quoted))      # the two regular expressions still find the lists
    known = set(om.FACTORS) | set(om.EXCLUDED)
    assert quoted - known == set(), sorted(quoted - known)
    assert accepted - known == set(), sorted(accepted - known)
    assert known - accepted == set(), sorted(known - accepted)                          # and the matrix sets nothing the library would refuse
    assert set(om.FACTORS) & set(om.EXCLUDED) == set()


def test_factor_table_and_plain():
    assert len(om.FACTORS) == 31 and sorted(n for n, f in om.FACTORS.items() if f[3]) == ["body_tile", "farmask", "hybrid", "zsplit"]
    assert sorted(n for n, f in om.FACTORS.items() if f[2]) == ["body_tile", "convf", "convm", "convt", "jacobi_march", "pair", "tail_lds"]
    assert om.values("bcfold") == (1, 0, 2, 3) and om.values("resjac") == (1, 0, 2, 3) and om.values("zsplit") == (2, 0)
    assert set(om.PLAIN) == set(om.FACTORS)
    for n, v in om.PLAIN.items():
        assert v in om.values(n), n
    for src in (om.callseq.EAGER, om.callseq.EAGER_BODY):
        assert all(om.PLAIN[k] == v for k, v in src.items())
    assert set(om.STEP13) <= set(om.FACTORS) and len(set(om.STEP13)) == 13
    assert set(om.COUNTED) <= set(om.FACTORS)


@pytest.mark.parametrize("family", list(om.FAMILIES))
def test_pair_rows_hold_every_pair_of_values(family):
    nm, rws = om.names(family), om.pair_rows(family)
    assert len(nm) == (31 if om.FAMILIES[family]["body"] else 27)
    assert rws[0] == om.defaults(nm)
    assert all(set(r) == set(nm) and all(r[n] in om.values(n) for n in nm) for r in rws)
    for a, b in itertools.combinations(nm, 2):      # exhaustive, written out: not the generator's own bookkeeping
        seen = {(r[a], r[b]) for r in rws}
        assert seen == set(itertools.product(om.values(a), om.values(b))), (family, a, b)
    assert om.uncovered(rws, nm, 2) == []
    assert len(rws) <= PAIR_CAP, len(rws)
    assert len(rws) == PAIR_ROWS[family], len(rws)


def test_triple_rows_hold_every_triple_of_the_step_level_switches():
    rws = om.triple_rows()
    assert rws[0] == om.defaults(om.STEP13)
    for c in itertools.combinations(om.STEP13, 3):
        seen = {tuple(r[n] for n in c) for r in rws}
        assert seen == set(itertools.product(*[om.values(n) for n in c])), c
    assert len(rws) <= TRIPLE_CAP, len(rws)
    assert len(rws) == TRIPLE_ROWS, len(rws)


@pytest.mark.parametrize("family", list(om.FAMILIES))
def test_every_counted_path_runs_next_to_every_value_not_exempt(family):
    nm, rws = om.names(family), om.pair_rows(family)
    exempt = {(p, f, v) for p, f, v, _ in om.STANDS_DOWN}
    for a in om.available(family):
        for b in nm:
            if b == a:
                continue
            for v in om.values(b):
                ran = any(r[b] == v and a in om.live(r, family) for r in rws)
                assert ran or (a, b, v) in exempt, (family, a, b, v)
                if (a, b, v) in exempt:      # an exemption is a statement: the path really is not claimed there
                    assert not any(r[b] == v and a in om.live(r, family) for r in rws), (family, a, b, v)
    assert om.liveness_left(rws, family) == set()


def test_families_have_the_paths_they_are_there_for():
    av = {f: om.available(f) for f in om.FAMILIES}
    assert av["box"] == {"pdefer", "bcdefer", "tailfuse", "tailwide", "tailspec", "rskip", "resjac", "xdefer"}
    assert av["ragged"] == av["box"] - {"tailfuse"}
    assert av["moving"] == {"hybrid", "body_tile"} and av["circle2d"] == {"hybrid"} and av["exit"] == set() and av["periodic"] == set()
    assert set().union(*av.values()) == set(om.COUNTED)
    assert om.live(om.PLAIN, "box") == set() and om.live(om.PLAIN, "moving") == set()


def test_every_stand_down_quotes_the_header():
    h = one_line(text("include", "wlhip.h"))
    assert om.STANDS_DOWN
    for path, factor, value, sentence in om.STANDS_DOWN:
        assert path in om.COUNTED and value in om.values(factor) and value != om.FACTORS[factor][0], (path, factor, value)
        assert one_line(sentence) in h, (path, factor, value, sentence)
    for path, cond, sentence in om.STANDS_DOWN_JOINT:
        assert path in om.COUNTED and all(v in om.values(f) for f, v in cond.items()) and one_line(sentence) in h, (path, cond)


def test_live_and_stood_down_never_claim_the_same_path():
    for family in om.FAMILIES:
        for r in om.pair_rows(family) + (om.triple_rows() if family == "box" else []):
            assert om.live(r, family) & om.stood_down(r, family) == set(), (family, r)


def test_readme_states_the_row_counts():
    r = one_line(text("README.md"))
    said = "Rows: " + ", ".join("%s %d" % (f, PAIR_ROWS[f]) for f in om.FAMILIES) + "; %d triples" % TRIPLE_ROWS
    assert said in r, said


def test_same_seed_same_rows():
    nm = om.names("box")
    om._rows.cache_clear()
    a = om.rows(2, nm, 7, "box")
    om._rows.cache_clear()
    assert om.rows(2, nm, 7, "box") == a
    assert om.rows(2, nm, 8, "box") != a
    a[0]["pair"] = 5                                # a caller's edit does not reach the kept rows
    assert om.rows(2, nm, 7, "box")[0]["pair"] == 1
    t = om.rows(3, om.STEP13[:6], 3)
    om._rows.cache_clear()
    assert om.rows(3, om.STEP13[:6], 3) == t


def test_counter_faults_reads_both_directions():
    row = om.defaults(om.names("box"))
    cnt = {a: 1 for a in om.COUNTED}
    assert om.counter_faults(row, "box", cnt) == []
    assert any("pdefer did not run" in s for s in om.counter_faults(row, "box", dict(cnt, pdefer=0)))
    off = dict(row, pdefer=0)
    assert any("pdefer ran 1 times with its switch off" in s for s in om.counter_faults(off, "box", cnt))
    assert om.counter_faults(off, "box", dict(cnt, pdefer=0)) == []
    down = dict(row, store_f=1)                     # the one-launch head does not run: pdefer, bcdefer, tailspec, resjac, tailfuse stand down
    assert {"pdefer", "bcdefer", "tailspec", "resjac", "tailfuse"} <= om.stood_down(down, "box")
    assert any("pdefer ran 1 times where the header says it stands down" in s for s in om.counter_faults(down, "box", cnt))
    assert om.counter_faults(down, "box", {a: (1 if a in om.live(down, "box") else 0) for a in om.COUNTED}) == []
    assert "bcdefer" in om.stood_down(dict(row, bcfold=3), "box") and "bcdefer" not in om.stood_down(dict(row, bcfold=3, convt=0), "box")


def test_shrink_on_fakes_reduces_to_the_two_switches(monkeypatch):
    """shrink() on a fake run(): the mismatch is there exactly when lazydt and convf are both on — it ends on those two"""
    class S:
        def __init__(self, v):
            self.v = v

    def fake_run(family, w, row, calls=om.CALLS):
        r = om.full(row)
        return [S(int(r["lazydt"] == 1 and r["convf"] == 1))], {}, None

    class W:
        class L:
            @staticmethod
            def wl_reset_process_options():
                return 0

        @staticmethod
        def lib():
            return W.L

    monkeypatch.setattr(om, "run", fake_run)
    monkeypatch.setattr(om, "first_diff", lambda snaps, ref: None if snaps[0].v == ref[0].v else (0, "u", 3, [[1, 1, 1, 0]]))
    said = []
    row = dict(om.defaults(om.names("box")), store_f=1, convz=1)
    assert om.shrink("box", row, w=W, out=said.append) == {"lazydt": 1, "convf": 1}
    assert "minimal set" in said[-1] and "lazydt" in said[-1]
    assert om.shrink("box", dict(om.PLAIN, convf=1), w=W, out=said.append) == {}
