"""Every pair of implementation switches against the plain path (test infrastructure; imports without a GPU).

wl_sim_set_option has about thirty switches that "choose between kernels that produce identical bits" (include/wlhip.h).  Whether a fast path runs is a conjunction
of other switches, tested once where the path is decided and again where it is consumed; the two agree only if they agree under EVERY setting of the others.
FACTORS lists the switches and their values, rows() draws a covering array over them (every pair of values of every pair of switches in some row; every triple for
the step-level switches), live() restates from the header which counted paths must run under a row, and rows() goes on adding rows until every counted path has
actually RUN next to every value of every other switch that the header does not say it stands down for (STANDS_DOWN, each entry resting on a quoted sentence).
tests/test_optmatrix_cpu.py checks all of that without a GPU; tests/test_gpu_optmatrix.py runs the rows against the PLAIN handle, bit for bit.

After a mismatch, by hand:  python -c "import sys; sys.path.insert(0, 'tests'); import optmatrix; optmatrix.shrink('box', {...the row...})"
(never on a row that ended in a GPU fault or a hang: find that cause by reading the code)."""
import functools
import itertools
import random

import callseq

# name -> (default, other values, process-wide, body-only).  The default of "zsplit" here is 2 (the path at any size): its library default is a size gate.
FACTORS = {}


def _factor(names, default, others, process=False, body=False):
    for n in names.split():
        FACTORS[n] = (default, tuple(others), process, body)


_factor("fused_smoother constl fuse_p fuse_cfl tail defer_shift skip_fill xdefer", 1, (0,))
_factor("pair tail_lds jacobi_march convt convf", 1, (0,), process=True)
_factor("store_f store_eps convz", 0, (1,))
_factor("convm", 0, (1,), process=True)
_factor("lazydt tailspec headspec bcdefer pdefer rskip tailwide tailfuse", 1, (0,))
_factor("bcfold resjac", 1, (0, 2, 3))
_factor("farmask hybrid", 1, (0,), body=True)
_factor("body_tile", 1, (0,), process=True, body=True)
_factor("zsplit", 2, (0,), body=True)

EXCLUDED = {
    "itmx": "solver!'s iteration cap: changes the results",
    "overlap": "z-slabs only: the u exchange on a second stream",
    "overlap_smooth": "z-slabs only: the smoother's deep r exchange overlapped with kernel A",
    "deep_halo": "z-slabs only: one five-plane exchange of r per smooth!",
    "x_halo": "z-slabs only: ghost depth of x",
    "zsplit_par": "the z-split's plane ranges on parallel streams: launch order only, for ranges",
    "resjac_min": "size gate: every handle here opens it to 0 (callseq.GATES)",
    "convt_min": "size gate: every handle here opens it to 0 (callseq.GATES)",
    "tailfuse_min": "size gate: every handle here opens it to 0 (callseq.GATES)",
}

# every factor at its un-fused, un-deferred value: one kernel per operation of the reference, everything materialised, nothing left pending
PLAIN = {"fused_smoother": 0, "fuse_p": 0, "constl": 0, "fuse_cfl": 0, "store_f": 1, "tail": 0, "jacobi_march": 0}      # the general kernels, one per pass, intermediates stored
PLAIN.update(callseq.EAGER)
PLAIN.update(callseq.EAGER_BODY)
PLAIN.update({"pair": 0, "tail_lds": 0, "store_eps": 1, "defer_shift": 0, "skip_fill": 0, "xdefer": 0, "convt": 0, "convf": 0, "convz": 0, "convm": 0,
              "bcfold": 0, "resjac": 0, "body_tile": 0})

STEP13 = ("pdefer", "bcdefer", "lazydt", "tailspec", "headspec", "rskip", "tailfuse", "tailwide", "resjac", "fuse_p", "fuse_cfl", "store_f", "bcfold")

# the families of tests/test_gpu_optmatrix.py: what the header's conditions ask about a flow and its shape (free_planes: a body with ranges of at least 8 whole
# body-free planes below or above it, which "body_tile" hands to the tiled kernel)
FAMILIES = {
    "box": {"body": False, "exit": False, "per": False, "D": 3, "whole_tiles": True, "free_planes": False},          # 64×32×24: whole 64×16 tiles
    "ragged": {"body": False, "exit": False, "per": False, "D": 3, "whole_tiles": False, "free_planes": False},      # 70×44×18
    "periodic": {"body": False, "exit": False, "per": True, "D": 3, "whole_tiles": True, "free_planes": False},
    "moving": {"body": True, "exit": False, "per": False, "D": 3, "whole_tiles": True, "free_planes": True},        # a sphere with body-free plane ranges below and above it
    "exit": {"body": True, "exit": True, "per": False, "D": 3, "whole_tiles": True, "free_planes": False},           # a floor: every plane holds body cells
    "circle2d": {"body": True, "exit": False, "per": False, "D": 2, "whole_tiles": False, "free_planes": False},
}
COUNTED = ("pdefer", "bcdefer", "tailfuse", "tailwide", "tailspec", "rskip", "resjac", "xdefer", "hybrid", "body_tile")


def names(family):
    return tuple(n for n, f in FACTORS.items() if FAMILIES[family]["body"] or not f[3])


def values(name):
    return (FACTORS[name][0],) + FACTORS[name][1]


def defaults(nm):
    return {n: FACTORS[n][0] for n in nm}


def full(row):
    """the row with every factor it does not name at its default"""
    out = defaults(FACTORS)
    out.update(row)
    return out


# ------------------------------------------------------------------------------------------------------------------------------------ live
def _fused_head(r, fam):
    """the one-launch projection head runs ("resjac": single-domain NoBody levels; not with a periodic direction, exitBC, "store_f", without the
    constant-coefficient kernels, the fused projection or the folded mean shift)"""
    return (not fam["body"] and not fam["per"] and not fam["exit"] and fam["D"] == 3 and r["fuse_p"] and r["resjac"] != 0 and r["constl"] and not r["store_f"]
            and r["defer_shift"])


def _fused_conv(r, fam):
    """predictor and corrector are the one-launch conv_diff!+BDIM! of a flow without a body, and not its z-marching variant"""
    return not fam["body"] and not (r["convz"] and fam["D"] == 3 and not fam["per"])


def _pair_smoother(r, fam):
    """the finest level runs the blocked pair kernels"""
    return not fam["body"] and not fam["per"] and fam["D"] == 3 and r["fused_smoother"] and r["pair"] and r["constl"]


def live(row, family):
    """the counted paths that MUST run under this row in this family (five steps: two single calls and one call of three): the header's conditions, restated"""
    fam, r = FAMILIES[family], full(row)
    out = set()
    plainbox = not fam["body"] and not fam["per"] and not fam["exit"] and fam["D"] == 3      # single domain, tuple U, no periodic direction / exit / body
    head = _fused_head(r, fam)
    head_counted_on = head and r["resjac"] != 2                # resjac 2 announces that the head will be redone: the deferrals stand down
    if head and r["resjac"] == 1:
        out.add("resjac")
    if r["pdefer"] and head_counted_on:                        # the predictor's tail, read next by the corrector's fused head
        out.add("pdefer")
    if r["bcdefer"] and plainbox and head_counted_on and (r["bcfold"] == 1 or (r["bcfold"] == 3 and not r["convt"])) and _fused_conv(r, fam):
        out.add("bcdefer")                                     # (bcfold bit 1 where the tiled kernel runs: BC! is already applied by the launch, nothing to defer)
    if (r["tailfuse"] and plainbox and fam["whole_tiles"] and r["fuse_p"] and r["bcfold"] != 0 and r["constl"] and not r["store_f"] and _fused_conv(r, fam)
            and r["convt"] and r["convf"] and not r["convm"]):
        out.add("tailfuse")
    if r["tailwide"] and plainbox and r["fuse_p"] and r["constl"]:
        out.add("tailwide")
    if r["tailspec"] and r["headspec"] and head and r["resjac"] == 1:
        out.add("tailspec")
    if r["rskip"] and _pair_smoother(r, fam) and not r["store_eps"]:
        out.add("rskip")
    if r["xdefer"] and _pair_smoother(r, fam):
        out.add("xdefer")
    if fam["body"] and r["hybrid"] and not fam["exit"]:
        out.add("hybrid")
        if fam["free_planes"] and r["body_tile"] and r["convt"] and not r["store_f"]:
            out.add("body_tile")
    return out


def own_switch_off(row, path):
    return full(row)[path] == 0


# (counted path, other factor, value, the header sentence the stand-down rests on) — filled from _SD below
STANDS_DOWN = []


def _sd(path, pairs, sentence):
    for spec in pairs.split():
        f, v = spec.split("=")
        STANDS_DOWN.append((path, f, int(v), sentence))


_S_HEAD = '"pdefer", "bcdefer" and "tailspec" build on that head: they stand down wherever it does'
_S_RESJAC = ('the one-launch head needs the constant-coefficient kernels ("constl"), the fused projection ("fuse_p") and the folded mean shift ("defer_shift"), and does not run with '
             '"store_f", a body, exitBC or a periodic direction')
_S_RJ2 = '2 (tests): every head is redone through the two-kernel path, and "bcdefer", "pdefer" and "tailspec" are told so in advance and stand down'
_S_RJ3 = '3 (tests): the same, not announced: "bcdefer" and "pdefer" defer and are flushed before the two-kernel head; the gated tail is withheld'
_S_BCDEFER = "Only where all of that holds (tuple U, single domain, no periodic direction / exit / body, fused head and folded tails in use)"
_S_BCDEFER2 = '"convz" is not the fused launch that "bcdefer" defers behind'
_S_BCDEFER3 = 'with bit 1 set, where the tiled kernel runs ("convt"), that kernel has applied BC! itself and "bcdefer" has nothing to defer'
_S_TAILFUSE2 = ('"tailfuse" needs the flux-once tiled launch ("convt", "convf"; not "convz", "convm"), the fused projection ("fuse_p"), constant coefficients ("constl"), '
                'a folded BC! ("bcfold" not 0) and f not stored ("store_f")')
_S_TAILWIDE2 = '"tailwide" needs the fused projection ("fuse_p") and the constant-coefficient kernels ("constl")'
_S_TAILSPEC = 'the gated tail is queued by the speculative first V-cycle: without "headspec", or where the one-launch head does not run, "tailspec" does nothing'
_S_RSKIP = ('"rskip"[1] the pair smoother\'s kernel B does not store the residual nobody reads; needs the pair kernels ("fused_smoother", "pair", "constl") and '
            'stands down with "store_eps", a periodic direction or a body')
_S_XDEFER = '"xdefer" needs the pair kernels ("fused_smoother", "pair", "constl")'
_S_BODYTILE = '"body_tile"[1] with a body: conv_diff!+BDIM! on the body-free plane ranges through the tiled NoBody kernel ("convt")'
_S_BODYTILE2 = '"body_tile" is a branch of the "hybrid" launch, taken for ranges of whole planes when f is not stored'

for _p in ("pdefer", "bcdefer", "tailspec", "resjac"):
    _sd(_p, "constl=0 fuse_p=0 defer_shift=0 store_f=1", _S_RESJAC if _p == "resjac" else _S_HEAD)
    _sd(_p, "resjac=0", _S_HEAD)
_sd("pdefer", "resjac=2", _S_RJ2)
_sd("bcdefer", "resjac=2", _S_RJ2)
_sd("tailspec", "resjac=2", _S_RJ2)
_sd("tailspec", "resjac=3", _S_RJ3)
_sd("tailspec", "headspec=0", _S_TAILSPEC)
_sd("bcdefer", "bcfold=0 bcfold=2", _S_BCDEFER)
_sd("bcdefer", "convz=1", _S_BCDEFER2)
_sd("tailfuse", "convt=0 convf=0 convz=1 convm=1 fuse_p=0 constl=0 bcfold=0 store_f=1", _S_TAILFUSE2)
_sd("tailwide", "fuse_p=0 constl=0", _S_TAILWIDE2)
_sd("rskip", "fused_smoother=0 pair=0 constl=0 store_eps=1", _S_RSKIP)
_sd("xdefer", "fused_smoother=0 pair=0 constl=0", _S_XDEFER)
_sd("body_tile", "convt=0", _S_BODYTILE)
_sd("body_tile", "hybrid=0 store_f=1", _S_BODYTILE2)
_STANDS = {(p, f, v) for p, f, v, _ in STANDS_DOWN}
# stand-downs that take two switches together: (counted path, {factor: value, ...}, header sentence) — held by the counters like STANDS_DOWN, exempting nothing
STANDS_DOWN_JOINT = [("bcdefer", {"bcfold": 3, "convt": 1}, _S_BCDEFER3)]


def stood_down(row, family):
    """the counted paths the header says do NOT run under this row: their counters must stay at 0"""
    r = full(row)
    out = {p for p, f, v, _ in STANDS_DOWN if r[f] == v}
    out |= {p for p, cond, _ in STANDS_DOWN_JOINT if all(r[f] == v for f, v in cond.items())}
    return out


def available(family):
    """the counted paths this family has at all: those live with every switch at its default"""
    return live({}, family)


def liveness_needs(family, nm=None):
    """every (counted path A, factor B, value v) that must have a row with B = v in which A runs"""
    nm = names(family) if nm is None else nm
    return {(a, b, v) for a in available(family) for b in nm if b != a for v in values(b) if (a, b, v) not in _STANDS}


def liveness_left(rws, family, nm=None):
    need = liveness_needs(family, nm)
    for r in rws:
        fr = full(r)
        for a in live(r, family):
            for b in r:
                need.discard((a, b, fr[b]))
    return need


# ------------------------------------------------------------------------------------------------------------------------------ generator
def uncovered(rws, nm, strength):
    """the value tuples of every `strength` factors of nm that no row holds (the exhaustive check of tests/test_optmatrix_cpu.py)"""
    out = []
    for c in itertools.combinations(nm, strength):
        seen = {tuple(r[n] for n in c) for r in rws}
        out += [(c, t) for t in itertools.product(*[values(n) for n in c]) if t not in seen]
    return out


def _nominal(strength, nm, rng, tries=40, family=None):
    k = len(nm)
    need = liveness_needs(family, nm) if family is not None else set()
    vals = [values(n) for n in nm]
    combos = list(itertools.combinations(range(k), strength))
    unc = {c: set(itertools.product(*[vals[i] for i in c])) for c in combos}
    of = [[c for c in combos if i in c] for i in range(k)]

    def mark(row):
        for c in combos:
            unc[c].discard(tuple(row[i] for i in c))

    def gain(row, f, v):      # tuples newly covered by setting factor f to v, among the combinations whose other factors are set
        n = 0
        for c in of[f]:
            t = tuple(v if i == f else row[i] for i in c)
            if None not in t and t in unc[c]:
                n += 1
        return n

    def live_gain(row):      # (path, factor = value) needs this row would meet: a row that keeps paths running is worth more than its tuples
        if not need:
            return set()
        r = dict(zip(nm, row))
        return {(a, b, r[b]) for a in live(r, family) for b in nm} & need

    first = [v[0] for v in vals]
    mark(first)
    need -= live_gain(first)
    out = [first]
    while True:
        open_ = [c for c in combos if unc[c]]
        if not open_:
            break
        best, best_n = None, -1
        for _ in range(tries):
            row = [None] * k
            c = open_[rng.randrange(len(open_))]
            t = sorted(unc[c])[rng.randrange(len(unc[c]))]
            for i, v in zip(c, t):
                row[i] = v
            rest = [i for i in range(k) if row[i] is None]
            rng.shuffle(rest)
            for f in rest:
                g = [gain(row, f, v) for v in vals[f]]
                top = max(g)
                pick = [v for v, q in zip(vals[f], g) if q == top]
                row[f] = pick[rng.randrange(len(pick))]
            n = sum(1 for c2 in combos if tuple(row[i] for i in c2) in unc[c2]) + LIVE_WEIGHT * len(live_gain(row))
            if n > best_n:
                best, best_n = row, n
        mark(best)
        need -= live_gain(best)
        out.append(best)
    return [dict(zip(nm, r)) for r in out]


def _liveness_rows(rws, family, nm, rng):
    """rows added until every needed (path, factor = value) has run together"""
    need = liveness_left(rws, family, nm)
    out = []
    while need:
        a, b, v = sorted(need)[rng.randrange(len(need))]
        row = defaults(nm)
        row[b] = v
        if a not in live(row, family):      # it may take one more switch (bcdefer next to bcfold = 3 runs where the tiled kernel does not: convt = 0)
            for f2, v2 in sorted((f2, v2) for f2 in nm if f2 not in (a, b) for v2 in values(f2)[1:]):
                if a in live(dict(row, **{f2: v2}), family):
                    row[f2] = v2
                    break
        if a not in live(row, family):
            raise AssertionError("%s does not run with %s = %d alone in %r: live() and STANDS_DOWN disagree" % (a, b, v, family))

        def covers(r):
            fr, lv = full(r), live(r, family)
            return {(x, y, fr[y]) for x in lv for y in nm} & need

        rest = [n for n in nm if n != b]
        rng.shuffle(rest)
        for f in rest:
            best, best_n = row, len(covers(row))
            for val in values(f):
                trial = dict(row)
                trial[f] = val
                c = covers(trial)
                if (a, b, v) in c and len(c) > best_n:
                    best, best_n = trial, len(c)
            row = best
        need -= covers(row)
        out.append(row)
    return out


@functools.lru_cache(maxsize=None)
def _rows(strength, nm, seed, family):
    rng = random.Random(seed)
    out = _nominal(strength, nm, rng, family=family)
    if family is not None:
        out += _liveness_rows(out, family, nm, rng)
    return tuple(tuple(sorted(r.items())) for r in out)


def rows(strength, nm, seed, family=None):
    """a covering array of the given strength over the factors nm: a list of dicts, row 0 all defaults, deterministic in its arguments (random.Random(seed)).
    With a family, rows are added after the nominal coverage until liveness_left() is empty for it.  Computed on first use and kept."""
    return [dict(r) for r in _rows(int(strength), tuple(nm), int(seed), family)]


SEED = 1
LIVE_WEIGHT = 3      # a liveness need met counts as three value tuples when the nominal rows are chosen


def pair_rows(family):
    return rows(2, names(family), SEED, family)


def triple_rows():
    return rows(3, STEP13, SEED)


# ----------------------------------------------------------------------------------------------------------------------------- on the GPU
def apply(h, row):
    """the row's switches on handle h — process-wide ones too (they go through the same call) — and then the size gates: an explicit tailfuse = 1
    rewrites its gate, so the gates come last"""
    for n, v in row.items():
        h.set_option(n, int(v))
    for n, v in callseq.GATES.items():
        h.set_option(n, int(v))


def make(family, w, row):
    """a fresh handle of the family, built as callseq.make builds them, with the row applied (a body is measured once, after the switches are set)"""
    import numpy as np
    if FAMILIES[family]["body"]:
        import bodypaths_ref as bp
        from test_gpu_bodypaths import handle
        case = next(c for c in bp.CASES if c["id"] == callseq.BODY_CASE[family])
        h = handle(w, case, {})
        apply(h, full(row))
        h.measure_body_(case["positions"][0][0], 1.0)
        return h
    dims = callseq.DIMS[family]
    if family == "box":
        u_init = np.asfortranarray(np.random.default_rng(137).uniform(-0.4, 0.4, size=tuple(n + 2 for n in dims) + (3,)).astype(np.float32))
        h = w.FusedSimulation(dims, callseq.UBC, dims[0], U=1, nu=0.02, u0=u_init)
    elif family == "ragged":
        h = w.FusedSimulation(dims, (0.0,) * 3, dims[0], U=1, nu=dims[0] / 1600.0, ic="tgv")
    else:
        h = w.FusedSimulation(dims, (0.0,) * 3, dims[0], U=1, nu=dims[0] / 1600.0, ic="tgv_periodic", perdir=(1, 3))
    apply(h, {n: v for n, v in full(row).items() if not FACTORS[n][3]})
    return h


class Snap:
    """u, u⁰, p on every cell, pois.n and the Δt history on the host: what callseq.state_diff compares"""

    def __init__(self, h):
        self._f = {n: h.field(n) for n in ("u", "u0", "p")}
        self.pois_n, self.dt = list(h.pois_n), list(h.dt)

    def field(self, name):
        return self._f[name]


CALLS = (("mom_step_",), ("mom_step_",), ("mom_steps_", 3))


def call(h, c):
    getattr(h, c[0])(*c[1:])


def run(family, w, row, calls=CALLS):
    """(snapshots after each call, counters after the last, error or None) of a fresh handle under the row.  "body_tile" is read as a difference; "xdefer" reports
    the last smooth! of the finest level that took a prolongation: 1 deferred, 0 not, -1 none yet — a path ran where its counter is > 0."""
    h = make(family, w, row)
    t0 = h.counter("body_tile")
    snaps, err = [], None
    for c in calls:
        try:
            call(h, c)
        except Exception as e:      # an error return of the library (WlError): reported, nothing more is run on this handle
            err = "%s%r: %s" % (c[0], c[1:], e)
            break
        snaps.append(Snap(h))
    cnt = {a: h.counter(a) for a in COUNTED}
    cnt["body_tile"] -= t0
    return snaps, cnt, err


def first_diff(snaps, ref):
    """None, or (call index, field, differing cells, detail)"""
    for q, (a, b) in enumerate(zip(snaps, ref)):
        d = callseq.state_diff(a, b)
        if d is not None:
            return (q,) + d
    return None


def counter_faults(row, family, cnt):
    """what the counters hold against live() and the switches: a list of readable lines"""
    out = ["%s did not run (counter 0) though the header says it does" % a for a in sorted(live(row, family)) if cnt[a] <= 0]
    out += ["%s ran %d times with its switch off" % (a, cnt[a]) for a in COUNTED if a in full(row) and own_switch_off(row, a) and cnt[a] > 0]
    out += ["%s ran %d times where the header says it stands down" % (a, cnt[a]) for a in sorted(stood_down(row, family)) if not own_switch_off(row, a) and cnt[a] > 0]
    return out


def shrink_hint(family, row):
    return "python -c \"import sys; sys.path.insert(0, 'tests'); import optmatrix; optmatrix.shrink(%r, %r)\"" % (family, row)


def shrink(family, row, w=None, out=print):
    """by hand, after a MISMATCH (never after a fault or a hang): move the row's factors back to PLAIN one at a time while the mismatch persists; prints and
    returns the minimal set of switches that still differs from the plain handle.  Stops at the first error return."""
    if w is None:
        import waterlily_jl_amd as w
        w.core.device()
    try:
        plain = {n: PLAIN[n] for n in names(family)}
        w.lib().wl_reset_process_options()
        ref, _, err = run(family, w, plain)
        assert err is None, err
        row = {n: full(row)[n] for n in names(family)}

        def fails(r):
            snaps, _, e = run(family, w, r)
            if e is not None:
                raise RuntimeError(e)
            return first_diff(snaps, ref)

        try:
            d = fails(row)
            if d is None:
                out("no mismatch under this row")
                return {}
            changed = True
            while changed:
                changed = False
                for n in names(family):
                    if row[n] == PLAIN[n]:
                        continue
                    trial = dict(row)
                    trial[n] = PLAIN[n]
                    dd = fails(trial)
                    if dd is not None:
                        row, d, changed = trial, dd, True
        except RuntimeError as e:
            out("stopped at an error return: %s" % e)
            return None
        small = {n: v for n, v in row.items() if v != PLAIN[n]}
        out("%s: minimal set %r (everything else PLAIN): call %d, %s, %s differing cells, first %s" % ((family, small) + tuple(d[:4])))
        return small
    finally:
        w.lib().wl_reset_process_options()
