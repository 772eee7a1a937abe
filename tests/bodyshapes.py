"""The body-aware shortcuts (farmask, hybrid, body_tile, zsplit) on both sides of the gates that only a GRID SHAPE can move (test infrastructure; imports
without a GPU).

tests/shapegates.py crosses every geometric predicate of csrc/ with shapes, without a body; tests/bodypaths_ref.py moves the body through every mask class,
on grids that leave every gate of the body code open.  This module crosses the two: GATES restates the body-side predicates — each with its file and the literal
source expressions it restates —, zsplit_plan_level restates wl_mg::update's decision on ANY level from that level's L, parts() the three plane ranges of
zsplit_parts, SHAPE_CONDS the classes a position is there for (next to bodypaths_ref.CONDS), SHAPE_CASES the geometries in the format of bodypaths_ref.CASES and
PAIRS the two sides of every gate with everything else that flips along.  tests/test_bodyshapes_cpu.py holds all of it to the source text, to the oracle's
measure! and hierarchy and to hand-classified fields without a GPU; tests/test_gpu_bodyshapes.py runs every case: shortcuts without size gates, the default
handle and the general kernels, bit for bit after every call, with the census, the counters and the smoother kind of every level held to this restatement.

Out of scope (other files own them or nothing reaches them): zsplit_par, z-slabs, periodic directions next to these shapes (bodypaths_ref.CASES has the
periodic bodies), the force recorder's tiles (tests/test_gpu_forces.py), grids above shapegates.CELL_CAP."""
from collections import namedtuple

import numpy as np

import bodypaths_ref as bp
import shapegates as sg

CSRC = sg.CSRC
CELL_CAP, ORACLE_CELLS = sg.CELL_CAP, sg.ORACLE_CELLS
MAX_CASES = 40
WG = bp.WG
ZSPLIT_MARGIN = 4                    # wl_mg::ZSPLIT_MARGIN
ZSPLIT_MIN_DEFAULT = 16 << 20        # wl_mg::zsplit_min of a handle with nothing set: no level under the cap is split


# ------------------------------------------------------------------------------------------------------------------ the restatement: masks
def needf_mask(mu1, dirs=("x", "y", "z")):
    """needf of k_body_mask2 as an (nz, nbm) array, with the neighbour loop restricted to `dirs`: what each direction of the loop contributes"""
    D = mu1.shape[-1]
    Ng = mu1.shape[:-2]
    nx, sz = Ng[0], Ng[0] * Ng[1]
    nz1 = bp._planes((mu1 != 0).any((-1, -2)), D)
    nz = nz1.shape[2]
    f1 = nz1.reshape(sz, nz, order="F")
    out = np.zeros((nz, bp.nbm(Ng)), np.uint8)
    for k in range(nz):
        m = np.nonzero(f1[:, k])[0]
        for name, step in (("x", 1), ("y", nx)):
            if name in dirs:
                for dm in (-step, step):
                    mm = m + dm
                    mm = mm[(mm >= 0) & (mm < sz)]
                    out[k, mm // WG] = 1
        if D == 3 and "z" in dirs and m.size:
            for kk in (k - 1, k + 1):
                if 0 <= kk < nz:
                    out[kk, m // WG] = 1
    return out


def census_shapes(mu0, mu1, V):
    """bodypaths_ref.census_plus + what only SHAPE_CONDS look at (leading underscore: not library counters)"""
    c = bp.census_plus(mu0, mu1, V)
    near, needf, _ = bp.masks(mu0, mu1, V)
    only = needf & (1 - near)
    c["_needf_y_only"] = int((only & (1 - needf_mask(mu1, ("x", "z")))).sum())      # needf-only workgroups that are such through a ±sy neighbour alone
    m = np.nonzero(bp._planes((mu1 != 0).any((-1, -2)), mu1.shape[-1]).reshape(mu0.shape[0] * mu0.shape[1], -1, order="F").any(1))[0]
    nx, sz = mu0.shape[0], mu0.shape[0] * mu0.shape[1]
    c["_y_wg_dist"] = tuple(sorted({abs(int(mm) // WG - int(k) // WG) for k in m for mm in (k - nx, k + nx) if 0 <= mm < sz}))      # how many workgroups away the ±sy neighbours of the μ₁ ≠ 0 cells fall
    c["_needf_only_wo_y"] = int((needf_mask(mu1, ("x", "z")) & (1 - near)).sum())    # mask_needf_only of a loop that leaves ±sy out
    return c


def far_planes(c, Ng):
    """the planes below and above conv_diff_bdim_body's gather range before the two joins — whatever nx and ny are"""
    k0, k1 = 1, Ng[2] - 1
    return max(c["dirty_z0"], k0) - k0, k1 - min(c["dirty_z1"] + 1, k1)


# ---------------------------------------------------------------------------------------------------------------- the restatement: z-split
Plan = namedtuple("Plan", "part za zb na nb far np gate za_z", defaults=(False,))      # gate: which clause decided ("geom", "const", "c0", "far"); za_z: the z-face coefficient of plane za deviates


def fused_geom(Ng, perdir=()):
    return len(Ng) == 3 and not perdir and bool(sg.gsrb_fused_ok(Ng))


def pair_geom(Ng, perdir=()):
    return fused_geom(Ng, perdir) and bool(sg.gsrb_pair_geom_ok(Ng))


def const_pattern(L, Ng):
    """check_const_L: the constants sampled at Julia cell (3,3,3) (0-based (2,2,2)) and the wall pattern scaled by them"""
    c = L[(2,) * len(Ng)]
    return c, bp.wall_pattern(Ng) * c


def zsplit_plan_level(L, Ng, perdir=(), min_cells=0):
    """wl_mg::update on one level, from that level's L (level 0: L = μ₀): the planes za..zb on which a coefficient is off the sampled constant pattern, the
    middle range [na, nb) = [za − 4, zb + 5) cut to the interior planes, the far planes outside it and the decision (at least 16 far planes and a quarter of
    all, on a level of at least min_cells cells: 0 under "zsplit" = 2).  plan[:3] is bodypaths_ref.zsplit_plan's (part, za, zb)."""
    Ng = tuple(Ng)
    if not pair_geom(Ng, perdir):
        return Plan(False, Ng[-1], -1, None, None, 0, (Ng[2] - 2) if len(Ng) == 3 else 0, "geom")
    k0, k1 = 1, Ng[2] - 1
    c, pat = const_pattern(L, Ng)
    bad = np.nonzero((L != pat).any((0, 1, 3)))[0]
    if bad.size == 0 or c[0] == 0:
        return Plan(False, Ng[2], -1, None, None, 0, k1 - k0, "const" if bad.size == 0 else "c0")
    za, zb = int(bad.min()), int(bad.max())
    na, nb = max(k0, za - ZSPLIT_MARGIN), min(k1, zb + ZSPLIT_MARGIN + 1)
    far = (na - k0) + (k1 - nb)
    part = bool(far >= 16 and far * 4 >= k1 - k0 and int(np.prod(Ng)) >= min_cells)
    return Plan(part, za, zb, na, nb, far, k1 - k0, "far", bool((L[:, :, za, 2] != pat[:, :, za, 2]).any()))


def parts(plan, Ng):
    """zsplit_parts: the three plane ranges [a, b) in launch order — around the body, below it, above it"""
    k0, k1 = 1, Ng[2] - 1
    return [(plan.na, plan.nb), (k0, plan.na), (plan.nb, k1)]


def part_kernel(n):
    """which kernels a range of n planes runs in smooth_zsplit: the launches pass no `range`, so gsrb_fused_A / _A_pro / _B ask gsrb_pair_ok on the range
    itself — a far range under 8 planes takes the one-cell blocked kernels with the constant pattern, not the pair kernels"""
    return None if n <= 0 else ("pair" if n >= 8 else "one-cell")


def smoother_kind_level(L, Ng, perdir=(), constl=True, min_cells=0):
    """wl_mg_smoother_kind of a single-domain level with a body: 0 where the blocked smoother's geometry fails (and in 2-D, and with a periodic direction),
    3 where the level is split, 2 on a level verified as constant whose geometry the pair kernels take, 1 elsewhere (and everywhere under "constl" = 0)"""
    Ng = tuple(Ng)
    if not fused_geom(Ng, perdir):
        return 0
    if not constl:
        return 1
    if zsplit_plan_level(L, Ng, perdir, min_cells).part:
        return 3
    _, pat = const_pattern(L, Ng)
    return 2 if pair_geom(Ng, perdir) and bool((L == pat).all()) else 1


# ------------------------------------------------------------------------------------------------------------------------------- the gates
GATES = {}


def _gate(name, file, quotes, fn, doc):
    GATES[name] = sg.Gate(name, file, quotes, fn, doc)


# each restatement is a function of state() below: which side of the gate a position is on (None: the gate is not asked there)
_gate("conv_tile_ok_body", "wl_flow.hip", ["if (nfar > 0 && nb > na && wl::conv_tile_ok(g, per, 2 * nfar)) {"], lambda s: s["tile_shape"],
      "the tiled far-range launches of conv_diff_bdim_body: array nx ≥ 34 and ny ≥ 18 (the size gate is asked with twice the far planes)")
_gate("join_low", "wl_flow.hip", ["if (na - g.k0 < 8) na = g.k0;"], lambda s: None if s["far_low"] == 0 else s["far_low"] >= 8, "a far range under 8 planes below the dirty planes joins the gather range")
_gate("join_high", "wl_flow.hip", ["if (g.k1 - nb < 8) nb = g.k1;"], lambda s: None if s["far_high"] == 0 else s["far_high"] >= 8, "… and above them")
_gate("body_masks_nbm", "wl_flow.hip", ["int body_masks_nbm(const GridX& g) { return 8 * wl_strip_blocks(g); }"], lambda s: min(s["nbm"], 24),
      "mask slots per plane: the plane's workgroups of 256 cells rounded up to a multiple of 8 (sides: 8, 16, 24 and more)")
_gate("needf_loop", "wl_flow.hip", ["const long st[3] = {1, g.sy, g.sz};", "for (int b = 0; b < D; b++) for (int sg = -1; sg <= 1; sg += 2) {", "if (b == 2) kk += sg; else mm += sg * st[b];",
                                    "if (kk < 0 || kk >= g.nz || mm < 0 || mm >= g.sz) continue;", "needf[(long)kk * nbm + mm / WL_BLOCK] = 1;"],
      lambda s: s["needf_y_only"] > 0, "a cell with μ₁ ≠ 0 marks the workgroups of its neighbours in x, y and z; True: some workgroup keeps f through a ±sy neighbour alone")
_gate("part", "wl_mg.hip", ["if (!v.cl.on && !v.dist && v.g.D == 3 && wl::gsrb_fused_ok(v.x_, perdir, v.dist) && wl::gsrb_pair_geom_ok(v.x_) && v.cl.c[0] != 0.f) {",
                            "const int far = (z.na - v.g.k0) + (v.g.k1 - z.nb);", "v.part = v.zb >= v.za && far >= 16 && far * 4 >= (v.g.k1 - v.g.k0) && v.x_.cs >= zsplit_min;"],
      lambda s: s["part"][0], "a level is split when the pair kernels take its geometry, at least 16 planes and a quarter of all are 4 planes away from the body")
_gate("zsplit_ranges", "wl_mg.hpp", ["ZRanges zsplit_ranges(const Level& v) const { return {v.part && use_zsplit && !v.dist, std::max(v.g.k0, v.za - ZSPLIT_MARGIN), std::min(v.g.k1, v.zb + ZSPLIT_MARGIN + 1)}; }",
                                     "static constexpr int ZSPLIT_MARGIN = 4;"], lambda s: tuple(l for l, on in enumerate(s["part"]) if on and l > 0),
      "the middle range [za − 4, zb + 5) cut to the interior, on EVERY level that is split (sides: which coarse levels are)")
_gate("gsrb_pair_ok_range", "wl_fused2.hip", ["bool gsrb_pair_ok_range(const GridX& g, const ConstL& cl) { GridX h = g; if (h.k1 - h.k0 < 8) h.k1 = h.k0 + 8; return g.k1 > g.k0 && gsrb_pair_ok(h, cl); }"],
      lambda s: s["part_kernels"], "quoted, NOT reached from the z-split: smooth_zsplit passes no `range`, so its launches ask gsrb_pair_ok on the range itself "
                                   "(sides: the kernels the two far ranges of a split level then run — pair from 8 planes, one-cell below; see part_kernel)")
_gate("hybrid_ok", "wl_sim.hip", ["bool hybrid_ok() const { return d.has_body && use_hybrid && mask_valid && mnear && us && !comm && !forcing && !sgs_model && !d.exitBC; }"],
      lambda s: s["hybrid"], "the hybrid conv_diff!+BDIM! stands down for the convective exit")
_gate("far_tile_whole", "wl_convf.hip", ["const bool full = (g.nx - 2) % CF_CX == 0 && (g.ny - 2) % CF_CY == 0;"], lambda s: s["far_tile_whole"],
      "whole 64×16 tiles choose the instance of the tiled kernel without the ragged-edge tests — in the far-range launches too")
QUOTED = [
    ("wl_convt.hip", "if (3L * g.cs >= (1L << 31) || g.nx < 34 || g.ny < 18) return false;"), ("wl_convt.hip", "return nplanes >= (g_convt_min > 0 ? 8 : 1) && ntiles * nplanes >= g_convt_min;"),
    ("wl_flow.hip", "if (g.D == 3 && g_body_tile && !store_all && per == 0 && dz1 >= dz0 && g.nz == g.gnz) {"),
    ("wl_flow.hip", "int na = dz0 > g.k0 ? dz0 : g.k0, nb = dz1 + 1 < g.k1 ? dz1 + 1 : g.k1;"), ("wl_flow.hip", "const int nfar = (na - g.k0) + (g.k1 - nb);"),
    ("wl_flow.hip", "return conv_diff_launch<3>(f, u_adv, Phi, g, nu, per, scheme, s, &bd, na == g.k0 ? -(1 << 30) : na, nb == g.k1 ? 1 << 30 : nb);"),
    ("wl_common.hpp", "static inline int wl_strip_blocks(const GridX& g) { const long nbx = (g.sz + WL_BLOCK - 1) / WL_BLOCK; return (int)((nbx + 7) >> 3); }"),
    ("wl_flow.hip", "if (nz1 || nzv) near[(long)k * nbm + m / WL_BLOCK] = 1;"), ("wl_flow.hip", "if (var) m0var[(long)k * nbm + m / WL_BLOCK] = 1;"),
    ("wl_flow.hip", "const long m = (long)(b0 + (int)blockIdx.x) * WL_BLOCK + threadIdx.x;"), ("wl_flow.hip", "const dim3 grid((unsigned)(box[1] - box[0] + 1), (unsigned)(box[3] - box[2] + 1), 1);"),
    ("wl_mg.hip", "out[0] = {z.na, z.nb, &v.cl}; out[1] = {v.g.k0, z.na, &v.clp}; out[2] = {z.nb, v.g.k1, &v.clp};"),
    ("wl_mg.hip", "for (size_t l = 0; l < lv.size(); l++) {"), ("wl_mg.hip", "q.form = zsplit_ranges(p).on ? Smooth::ZSplit :"),
    # smooth_zsplit passes no `range`: part_kernel
    ("wl_mg.hip", "WL_TRY(wl::gsrb_fused_A_pro(p.em, p.rs, p.x, p.r, coarse->x, p.L, g, coarse->x_, w, *parts[i].cl, sr[i], -(1 << 30), 1 << 30, &xdef[i]));"),
    ("wl_fused.hip", "if ((range ? gsrb_pair_ok_range(g, cl) : gsrb_pair_ok(g, cl)) && gc.cs < (1L << 30) && al8(emid, rnew, x, r)) {"),
    ("wl_fused.hip", "if (gsrb_pair_ok(g, cl) && al8(emid, r)) return gsrb_pair_A(emid, r, g, cl, s);"),
    # where the constants are sampled
    ("wl_poisson.hip", "int kk = (g.D == 3) ? g.k0 + ((g.gk + g.k0 + 1 >= 3) ? 0 : 1) : 0;"), ("wl_poisson.hip", "const long o = 2 + 2 * g.sy + (long)kk * g.sz;"),
    ("wl_sim.hip", "s->mg->use_zsplit = value != 0; s->mg->zsplit_min = value == 2 ? 0 : (value >= 4 ? (long)value << 20 : 16L << 20); return 0;"),
    ("wl_mg.hpp", "long zsplit_min = 16L << 20;"), ("wl_capi.hip", "case wl_mg::Smooth::ZSplit: return 3;"),
]


def state(c, Ng, tr, plans, kinds, case):
    """every restated decision of a position: what the two sides of a pair may differ in"""
    D = len(Ng)
    lo, hi = far_planes(c, Ng) if D == 3 and c["dirty_z1"] >= c["dirty_z0"] else (0, 0)
    sz = Ng[0] * Ng[1]
    lv = sg.levels(case["dims"])
    kern = tuple(sorted({part_kernel(b - a) for l, p in enumerate(plans) if p.part for a, b in parts(p, lv[l])[1:]} - {None})) or None
    return {
        "tile_shape": D == 3 and Ng[0] >= 34 and Ng[1] >= 18, "far_low": lo, "far_high": hi, "tile_launches": tr[2], "nbm": bp.nbm(Ng), "whole_wgs": sz % WG == 0,
        "row_over_wg": Ng[0] > WG, "row_over_2wg": Ng[0] > 2 * WG, "needf_y_only": c["_needf_y_only"], "part": tuple(p.part for p in plans), "part_kernels": kern,
        "hybrid": not case["exitBC"], "far_tile_whole": ((Ng[0] - 2) % 64 == 0 and (Ng[1] - 2) % 16 == 0) if tr[2] else None,
        "kinds": tuple(kinds), "eight_planes": D == 3 and Ng[2] - 2 == 8,
    }


def view(s):
    """state() as the sides of every gate plus the shape thresholds and the path set: what test_each_pair_flips_what_the_table_says compares"""
    out = {g: GATES[g](s) for g in GATES}
    out.update({k: s[k] for k in ("whole_wgs", "row_over_wg", "row_over_2wg", "eight_planes")})
    out["kinds"] = tuple(k for k in s["kinds"] if k)      # (the levels below the blocked smoother's geometry all read 0, however many there are)
    out["tile_launches"] = s["tile_launches"] if s["hybrid"] else 0
    return out


def evaluate(case, mu0, mu1, V, Ls, constl=True, min_cells=0):
    """everything the restatement says about a position from its fields and the L of every level (Ls[0] = μ₀): census, tile ranges, plan and kind per level, state"""
    Ng = tuple(mu0.shape[:-1])
    c = census_shapes(mu0, mu1, V)
    tr = bp.tile_ranges(c, Ng, case["perdir"], case["store_f"])
    plans = [zsplit_plan_level(L, L.shape[:-1], case["perdir"], min_cells) for L in Ls]
    kinds = [smoother_kind_level(L, L.shape[:-1], case["perdir"], constl, min_cells) for L in Ls]
    return {"c": c, "Ng": Ng, "tr": tr, "plans": plans, "kinds": kinds, "state": state(c, Ng, tr, plans, kinds, case)}


def paths(s):
    """the predicted path set the GPU test holds the library to"""
    return (s["hybrid"], s["tile_launches"] if s["hybrid"] else 0, s["kinds"], s["part"])


# ------------------------------------------------------------------------------------------------------------------------------ the classes
# predicates on (census_shapes, Ng, tile_ranges, [Plan per level]); a position may also claim a class of bodypaths_ref.CONDS (its zsplit_plan is plans[0][:3])
def _far_low(c, Ng):
    return far_planes(c, Ng)[0]


def _far_high(c, Ng):
    return far_planes(c, Ng)[1]


def _part_lens(p, Ng):
    return (p.na - 1, (Ng[2] - 1) - p.nb) if p.part else (None, None)


def _d3(Ng):
    return len(Ng) == 3


SHAPE_CONDS = {
    "tile_shape_out": lambda c, Ng, tr, pl: _d3(Ng) and max(far_planes(c, Ng)) >= 8 and tr[2] == 0 and (Ng[0] < 34 or Ng[1] < 18),
    "far_exactly_8_low": lambda c, Ng, tr, pl: _far_low(c, Ng) == 8 and tr[0] == 9 and tr[2] >= 1,
    "far_exactly_7_low": lambda c, Ng, tr, pl: _far_low(c, Ng) == 7 and tr[0] == 1,
    "far_exactly_8_high": lambda c, Ng, tr, pl: _far_high(c, Ng) == 8 and tr[1] == Ng[2] - 9 and tr[2] >= 1,
    "far_exactly_7_high": lambda c, Ng, tr, pl: _far_high(c, Ng) == 7 and tr[1] == Ng[2] - 1,
    "eight_planes": lambda c, Ng, tr, pl: _d3(Ng) and Ng[2] - 2 == 8 and c["mask_near"] > 0 and tr[2] == 0,
    "far_tiles_ragged_x": lambda c, Ng, tr, pl: tr[2] >= 1 and (Ng[0] - 2) % 64 != 0,
    "far_tiles_ragged_y": lambda c, Ng, tr, pl: tr[2] >= 1 and (Ng[1] - 2) % 16 != 0,
    "nbm8": lambda c, Ng, tr, pl: _d3(Ng) and bp.nbm(Ng) == 8 and c["mask_near"] > 0,
    "nbm16": lambda c, Ng, tr, pl: _d3(Ng) and bp.nbm(Ng) == 16 and c["mask_near"] > 0,
    "nbm24plus": lambda c, Ng, tr, pl: _d3(Ng) and bp.nbm(Ng) >= 24 and c["mask_near"] > 0,
    "whole_wgs": lambda c, Ng, tr, pl: _d3(Ng) and (Ng[0] * Ng[1]) % WG == 0 and c["near_b1"] == Ng[0] * Ng[1] // WG - 1,
    "row_over_wg": lambda c, Ng, tr, pl: _d3(Ng) and Ng[0] > WG and c["_needf_y_only"] > 0 and max(c["_y_wg_dist"]) >= 2,      # … and some ±sy neighbour is marked two workgroups away
    "row_over_2wg": lambda c, Ng, tr, pl: _d3(Ng) and Ng[0] > 2 * WG and c["_needf_y_only"] > 0 and max(c["_y_wg_dist"]) >= 3,     # … three workgroups away
    # the body level would be split for its far planes (a quarter, at least 16) but the pair kernels do not take its geometry: kind 1 as restated
    "pair_geom_out_ny": lambda c, Ng, tr, pl: fused_geom(Ng) and Ng[0] % 2 == 0 and Ng[1] < 34 and not pl[0].part and pl[0].gate == "geom",
    "pair_geom_out_oddnx": lambda c, Ng, tr, pl: fused_geom(Ng) and Ng[0] % 2 == 1 and Ng[1] >= 34 and not pl[0].part and pl[0].gate == "geom",
    "far_15": lambda c, Ng, tr, pl: pl[0].gate == "far" and pl[0].far == 15 and not pl[0].part,
    "far_16": lambda c, Ng, tr, pl: pl[0].gate == "far" and pl[0].far == 16,
    "quarter_in": lambda c, Ng, tr, pl: pl[0].far >= 16 and pl[0].far * 4 == pl[0].np and pl[0].part,
    "quarter_out": lambda c, Ng, tr, pl: pl[0].far >= 16 and pl[0].far * 4 == pl[0].np - 1 and not pl[0].part,
    "part_low_short": lambda c, Ng, tr, pl: pl[0].part and 1 <= _part_lens(pl[0], Ng)[0] <= 3 and _part_lens(pl[0], Ng)[1] >= 13,
    "part_high_short": lambda c, Ng, tr, pl: pl[0].part and 1 <= _part_lens(pl[0], Ng)[1] <= 3 and _part_lens(pl[0], Ng)[0] >= 13,
    "part_one_sided": lambda c, Ng, tr, pl: pl[0].part and 0 in _part_lens(pl[0], Ng),
    "part_middle_min": lambda c, Ng, tr, pl: pl[0].part and pl[0].za == pl[0].zb and pl[0].nb - pl[0].na == 2 * ZSPLIT_MARGIN + 1 and 0 not in _part_lens(pl[0], Ng),
    # the lower margin at its tightest: a cell reads L of its own plane and the z-face coefficient of the plane above, so the operator of plane za − 1 is off the
    # pattern exactly when L_z deviates on plane za — the planes between the lower far range and a deviating operator are then 3, not 4
    "margin_tight_low": lambda c, Ng, tr, pl: pl[0].part and pl[0].na > 1 and pl[0].za_z,
    "part_level1": lambda c, Ng, tr, pl: len(pl) > 1 and pl[1].part,
    "part_level0_not_level1": lambda c, Ng, tr, pl: len(pl) > 1 and pl[0].part and pl[1].gate == "far" and not pl[1].part,      # level 1 passes the geometry and fails on its far planes
    # level 0 is refused because the body clips the cell its constants are sampled at (every plane is then off pattern·c: far = 0) while level 1, sampled at
    # its own cell (2,2,2), is split: smooth_zsplit and the split Jacobi! on level 1 under a level 0 that runs the blocked smoother and absorbs level 1's prolongation
    "part_level1_not_level0": lambda c, Ng, tr, pl: len(pl) > 1 and pl[0].gate == "far" and not pl[0].part and pl[0].far == 0 and pl[1].part,
    "nbm8_2d": lambda c, Ng, tr, pl: len(Ng) == 2 and bp.nbm(Ng) == 8 and c["mask_near"] > 0,
    "whole_wgs_2d": lambda c, Ng, tr, pl: len(Ng) == 2 and (Ng[0] * Ng[1]) % WG == 0 and c["near_b1"] == Ng[0] * Ng[1] // WG - 1,
    "row_over_wg_2d": lambda c, Ng, tr, pl: len(Ng) == 2 and Ng[0] > WG and c["_needf_y_only"] > 0 and max(c["_y_wg_dist"]) >= 2,
}
# the classes whose positions also run one wl_sim_mom_steps(3)
STEPS3 = ("part_", "far_exactly_")
# classes of the issue's table that no shape under the cap reaches, with the arithmetic: none.  (Level 1 split without level 0 looked unreachable as long as both
# levels were taken to deviate from one pattern — a coarse plane deviates whenever one of its two fine planes does, so far₁ ≤ far₀/2 − 1.5 —, but check_const_L samples
# the constants of EVERY level at that level's own cell (2,2,2): a body that clips the fine one puts every fine plane off pattern·c while coarse cell (2,2,2), the mean
# of fine cells 3..4, stays clean.  The case "corner" is that.)
UNREACHABLE = {}


def cond(name):
    """the predicate of a class of either table, on (census, Ng, tile_ranges, plans)"""
    if name in SHAPE_CONDS:
        return SHAPE_CONDS[name]
    return lambda c, Ng, tr, pl: bp.CONDS[name](c, Ng, tr, tuple(pl[0][:3]))


def needs_steps3(conds):
    return any(n.startswith(STEPS3) for n in conds)


# ------------------------------------------------------------------------------------------------------------------------------- the cases
def ceiling(z):
    """solid above z (the constants of check_const_L are sampled near the floor: a solid floor reads c = 0 and is never split)"""
    return ("plane", (0.0, 0.0, float(z)), (0.0, 0.0, -1.0))


def zfloor(z):
    return ("plane", (0.0, 0.0, float(z)), (0.0, 0.0, 1.0))


VX = (0.25, 0.0, 0.0)
_case = bp._case
SHAPE_CASES = [
    # conv_tile_ok as conv_diff_bdim_body asks it: 34×18 arrays take the tiled far ranges, 32×18 and 34×16 leave every plane to the gather kernel
    _case("tile-32x16", [(bp.sphere((16, 8, 24)), ("tile2", "nbm8", "far_tiles_ragged_x"))], dims=(32, 16, 48)),
    _case("tile-30x16", [(bp.sphere((15, 8, 24)), ("tile_shape_out", "no_tile", "nbm8"))], dims=(30, 16, 48)),
    _case("tile-32x14", [(bp.sphere((16, 7, 24)), ("tile_shape_out", "no_tile", "nbm8"))], dims=(32, 14, 48)),
    _case("tile-32x16-exit", [(bp.sphere((16, 8, 24)), ("nbm8", "body"))], dims=(32, 16, 48), exitBC=True),
    # a plane of exactly 8 workgroups (64×32 array cells): no partial workgroup, the sphere is cut by the upper y wall and near_b1 is the last slot that exists
    _case("whole-62x30", [(bp.sphere((40, 27, 12), V=VX), ("whole_wgs", "nbm8", "v_cells")), (bp.sphere((20.5, 4, 10), V=VX), ("nbm8", "v_cells"))], dims=(62, 30, 24)),
    _case("whole-62x30-store_f", [(bp.sphere((40, 27, 12), V=VX), ("whole_wgs", "nbm8", "v_cells"))], dims=(62, 30, 24), store_f=True),
    _case("partial-62x28", [(bp.sphere((40, 25, 12), V=VX), ("last_wg_near", "nbm8", "v_cells"))], dims=(62, 28, 24)),
    _case("nbm32-126x62", [(bp.sphere((100, 59, 6), V=VX), ("whole_wgs", "nbm24plus", "v_cells"))], dims=(126, 62, 12)),
    # rows of 256, 258, 512 and 514 array cells: from 258 the ±sy neighbours of a cell are never in its own workgroup, from 514 never in the next one either
    _case("row-254", [(bp.sphere((100, 8, 12), V=VX), ("nbm24plus", "needf_only", "v_cells"))], dims=(254, 16, 24)),
    _case("row-256", [(bp.sphere((100, 8, 12), V=VX), ("needf_only", "nbm24plus", "v_cells")), (bp.sphere((251.5, 9, 14), V=VX), ("row_over_wg", "v_cells"))], dims=(256, 16, 24)),
    _case("row-510", [(bp.sphere((300, 8, 12)), ("row_over_wg", "nbm24plus"))], dims=(510, 16, 24)),
    _case("row-512", [(bp.sphere((300, 8, 12), V=VX), ("row_over_wg", "nbm24plus", "v_cells")), (bp.sphere((240, 9, 14), V=VX), ("row_over_2wg", "row_over_wg", "v_cells"))], dims=(512, 16, 24)),
    # eight interior planes: no far range can exist; sixteen: the same sphere, cut by the lower z wall and moving, leaves a far range above
    _case("planes-8", [(bp.sphere((32, 16, 2), 2.0, V=VX), ("eight_planes", "no_tile", "near_ghost_low", "v_cells"))], dims=(64, 32, 8)),
    _case("planes-16", [(bp.sphere((32, 16, 2), 2.0, V=VX), ("tile1", "near_ghost_low", "v_cells", "nbm16"))], dims=(64, 32, 16)),
    # the joins at 7 and 8 planes, a half-space moved by one plane
    _case("join-high", [(zfloor(36.0), ("far_exactly_8_high", "tile1")), (zfloor(37.0), ("far_exactly_7_high", "no_tile"))]),
    _case("join-low", [(ceiling(12.0), ("far_exactly_8_low", "tile1")), (ceiling(11.0), ("far_exactly_7_low", "no_tile"))]),
    # the z-split's far ≥ 16 at 16 and 15, one-sided (the ceiling reaches the upper wall: the upper far range is empty)
    _case("far-16-15", [(ceiling(21.0), ("far_16", "part", "part_one_sided")), (ceiling(20.0), ("far_15", "no_part")), (ceiling(20.75), ("far_16", "part_one_sided", "margin_tight_low"))]),
    # the quarter rule: 16 far planes of 64, and of 65
    _case("quarter-64", [(ceiling(21.0), ("quarter_in", "far_16", "part_one_sided"))], dims=(64, 32, 64)),
    _case("quarter-65", [(ceiling(21.0), ("quarter_out", "far_16", "no_part"))], dims=(64, 32, 65)),
    # far ranges of 1..3 planes next to a long one, and the thinnest middle range
    _case("part-short", [(bp.sphere((20, 16, 12.5), V=VX), ("part_low_short", "margin_tight_low", "v_cells")), (bp.sphere((40, 14, 35.5)), ("part_high_short", "margin_tight_low"))]),
    _case("part-middle-min", [(bp.sphere((31.6, 16, 24.5), -0.45), ("part_middle_min",))]),
    # the pair geometry under the z-split: 34×34 arrays are split, 34×32 and 35×34 keep the one-cell blocked kernels on the body level
    _case("pairgeom-32x32", [(bp.sphere((16, 16, 24)), ("part", "tile2"))], dims=(32, 32, 48)),
    _case("pairgeom-32x30", [(bp.sphere((16, 15, 24)), ("pair_geom_out_ny", "no_part", "tile2"))], dims=(32, 30, 48)),
    _case("pairgeom-33x32", [(bp.sphere((16.5, 16, 24)), ("pair_geom_out_oddnx", "no_part", "tile2"))], dims=(33, 32, 48)),
    # far-range launches on ragged tiles in both directions, and on whole tiles
    _case("ragged-66x34", [(bp.sphere((33, 17, 4), 3.0), ("far_tiles_ragged_x", "far_tiles_ragged_y", "tile1"))], dims=(66, 34, 24)),
    _case("whole-64x32", [(bp.sphere((32, 16, 4), 3.0), ("tile1", "nbm16"))], dims=(64, 32, 24)),
    # the z-split on a coarse level: level 1 of 128×64×96 is 66×34×50
    _case("level1", [(bp.sphere((64, 32, 48), 10.0), ("part", "part_level1")), (bp.sphere((64, 32, 48), 26.0), ("part", "part_level0_not_level1"))], dims=(128, 64, 96)),
    # … and on level 1 alone: a sphere in the low corner clips fine cell (2,2,2), where level 0's constants are sampled; moved along the floor it leaves it clean
    _case("corner", [(bp.sphere((0, 0, 0), 2.5), ("part_level1_not_level0", "no_part")), (bp.sphere((8, 8, 0), 2.5), ("part", "part_level1", "part_one_sided"))], dims=(64, 64, 48)),
    # 2-D
    _case("c2d-32x16", [(bp.sphere((16, 8), 4.0), ("nbm8_2d",))], dims=(32, 16)),
    _case("c2d-126x12", [(bp.sphere((100, 10.5), 3.0, V=VX[:2]), ("whole_wgs_2d", "nbm8_2d", "v_cells"))], dims=(126, 12)),
    _case("c2d-300x20", [(bp.sphere((150, 10), 5.0, V=VX[:2]), ("row_over_wg_2d", "v_cells"))], dims=(300, 20)),
]
# the cases above ORACLE_CELLS array cells: held to the plain handle only
PLAIN_ONLY = ["level1"]

# (gate, clause, (case id, position) on one side, (case id, position) on the other, the OTHER entries of state() that differ).  Ids of bodypaths_ref.CASES count too.
PAIRS = []


def _pair(gate, clause, a, b, flips=()):
    PAIRS.append({"gate": gate, "clause": clause, "a": a, "b": b, "flips": frozenset(flips)})


def side(gate, s):
    """the side of a gate of GATES — or of a bare entry of state(), for the thresholds that are no predicate of the library's — a position's state is on"""
    return view(s)[gate]


_pair("conv_tile_ok_body", "nx >= 34 (with gsrb_fused_ok: the same bound)", ("tile-32x16", 0), ("tile-30x16", 0), ["far_tile_whole", "kinds", "needf_loop", "tile_launches"])
_pair("conv_tile_ok_body", "ny >= 18 (with gsrb_fused_ok: the same bound)", ("tile-32x16", 0), ("tile-32x14", 0), ["far_tile_whole", "kinds", "needf_loop", "tile_launches"])
_pair("join_low", "8 planes are tiled, 7 join the gather range", ("join-low", 0), ("join-low", 1), ["far_tile_whole", "tile_launches"])
_pair("join_high", "8 planes are tiled, 7 join the gather range", ("join-high", 0), ("join-high", 1), ["far_tile_whole", "tile_launches"])
_pair("join_high", "k1 − k0 = 8: no far range can exist", ("planes-16", 0), ("planes-8", 0), ["eight_planes", "far_tile_whole", "kinds", "tile_launches"])
_pair("body_masks_nbm", "8 workgroups against 9", ("whole-62x30", 0), ("whole-64x32", 0), ["far_tile_whole", "join_high", "join_low", "kinds", "tile_launches", "whole_wgs"])
_pair("body_masks_nbm", "9 workgroups against 18", ("whole-64x32", 0), ("row-254", 0), ["far_tile_whole", "join_high", "join_low", "kinds", "tile_launches", "whole_wgs"])
_pair("needf_loop", "a workgroup that keeps f through ±sy alone", ("row-256", 0), ("partial-62x28", 0), ["body_masks_nbm", "row_over_wg"])
_pair("row_over_wg", "nx = 258 against 256: ±sy never in the cell's own workgroup", ("row-256", 1), ("row-254", 0), ["whole_wgs"])
_pair("row_over_2wg", "nx = 514 against 512: ±sy never in the next workgroup either", ("row-512", 1), ("row-510", 0), ["whole_wgs"])
_pair("whole_wgs", "2048 cells per plane against 1920", ("whole-62x30", 0), ("partial-62x28", 0), ["needf_loop"])
_pair("part", "far >= 16", ("far-16-15", 0), ("far-16-15", 1), ["gsrb_pair_ok_range", "kinds"])
_pair("part", "far * 4 >= k1 - k0", ("quarter-64", 0), ("quarter-65", 0), ["gsrb_pair_ok_range", "kinds"])
_pair("part", "gsrb_pair_geom_ok: ny >= 34", ("pairgeom-32x32", 0), ("pairgeom-32x30", 0), ["gsrb_pair_ok_range", "kinds", "needf_loop"])
_pair("part", "the sampled cell (2,2,2) of level 0 clean against clipped by the body: every plane off pattern·c, level 1 still split", ("corner", 1), ("corner", 0), ["kinds", "needf_loop"])
_pair("part", "gsrb_pair_geom_ok: even nx", ("pairgeom-32x32", 0), ("pairgeom-33x32", 0), ["gsrb_pair_ok_range", "kinds"])
_pair("zsplit_ranges", "level 1 split against level 1 refused for its far planes", ("level1", 0), ("level1", 1), ["kinds"])
_pair("gsrb_pair_ok_range", "a far range of 3 planes against two of at least 8", ("part-short", 0), ("zslab", 1), ["join_low", "tile_launches"])
_pair("hybrid_ok", "the convective exit", ("tile-32x16", 0), ("tile-32x16-exit", 0), ["tile_launches"])
_pair("far_tile_whole", "whole against ragged 64×16 tiles in the far-range launch", ("whole-64x32", 0), ("ragged-66x34", 0), [])
_pair("body_masks_nbm", "2-D: 3 workgroups against 13", ("c2d-32x16", 0), ("circle2d", 0), ["needf_loop"])
_pair("whole_wgs", "2-D: 1792 cells against 612", ("c2d-126x12", 0), ("c2d-32x16", 0), ["needf_loop"])
_pair("row_over_wg", "2-D: nx = 302 against 66", ("c2d-300x20", 0), ("circle2d", 0), ["body_masks_nbm"])

# gates whose two sides take the same path set: the library's read-out for them is the census, which the GPU test compares on every position
NO_READOUT = {
    "body_masks_nbm": "the number of mask slots per plane changes no dispatch; near_b0/near_b1 and the four mask counts of the census are the read-out",
    "needf_loop": "which workgroups keep f changes no dispatch; mask_needf_only of the census is the read-out (and u, where f was not kept)",
    "far_tile_whole": "instances of one kernel; body_tile counts both",
    "gsrb_pair_ok_range": "wl_mg_smoother_kind says 3 for a split level whatever kernels its ranges run; the bits are the read-out",
}


# … and the quantity that stands in for each, as a function of evaluate()'s result: tests/test_bodyshapes_cpu.py asserts that it differs between the two sides of every such
# pair (and that the far-range kernel, or the split, runs on both), so the device comparison of a side is never the other side's over again
READOUT = {
    "body_masks_nbm": lambda e: bp.nbm(e["Ng"]),                                                            # the slots per plane
    "needf_loop": lambda e: e["c"]["mask_needf_only"] - e["c"]["_needf_only_wo_y"] > 0,                     # what ±sy adds to mask_needf_only
    "row_over_wg": lambda e: e["c"]["_y_wg_dist"], "row_over_2wg": lambda e: e["c"]["_y_wg_dist"],          # how many workgroups away a ±sy neighbour is marked
    "whole_wgs": lambda e: ((e["Ng"][0] * e["Ng"][1]) % WG == 0, e["c"]["near_b1"] == (e["Ng"][0] * e["Ng"][1] + WG - 1) // WG - 1 and e["c"]["_last_wg_near"] > 0),
    "far_tile_whole": lambda e: e["state"]["far_tile_whole"] if e["tr"][2] > 0 else None,                  # (None on a side fails the test: the launch must run on both)
    "gsrb_pair_ok_range": lambda e: e["state"]["part_kernels"] if e["plans"][0].part else None,
}


def all_cases():
    return {c["id"]: c for c in list(bp.CASES) + SHAPE_CASES}
