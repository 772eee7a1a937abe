"""Every fast path against the plain one on both sides of its shape gate (test infrastructure; imports without a GPU).

Whether a fast kernel runs depends on the switches (tests/optmatrix.py), the call order (tests/callseq.py) and the SHAPE of the grid.  This module restates the
geometric predicates of csrc/ in Python — GATES, each with its file and the literal source expression it restates —, the level hierarchy (levels) and the
z-chunk choosers, derives from them what a body-free, non-periodic, tuple-U handle must dispatch (predicted), and lists for every gate the smallest shape just
inside it and the smallest just outside it (PAIRS; SHAPES is their union).  tests/test_shapegates_cpu.py holds the restatement to the source text and to the
oracle's hierarchy without a GPU; tests/test_gpu_shapegates.py runs every shape: default switches against optmatrix.PLAIN, bit for bit, and the dispatch the
library reports against predicted().

Out of scope, because other files own them: periodic directions, the z-split's own gates and every gate a body adds (tests/bodyshapes.py, which crosses them
with shapes; tests/bodypaths_ref.py), 2-D, z-slabs."""
import callseq
import optmatrix as om

CSRC = ("waterlily.jl_amd", "csrc")
MAXLEVELS = 10                       # wl_sim_create's pois_ctor default
WL_TAIL_CELLS, WL_TAIL_MAXLV, WL_MAXPART = 8192, 8, 65536
RESJAC_MIN_DEFAULT, CONVT_MIN_DEFAULT, TAILFUSE_MIN_DEFAULT = 6 << 20, 2048, 16 << 20      # the size gates callseq.GATES opens
CELL_CAP = 450 * 370 * 10            # no array larger than the suite's largest
ORACLE_CELLS = 300000                # the plain handle is tied to the oracle up to this many array cells
COUNTERS = ("resjac", "bcdefer", "pdefer", "tailspec", "tailfuse", "tailwide", "rskip", "xdefer")


# ---------------------------------------------------------------------------------------------------------------------------- the hierarchy
def divisible(n):
    return n % 2 == 0 and n > 4


def levels(N, maxlevels=MAXLEVELS):
    """the array dims (ghosts included) of every multigrid level of interior dims N.  The loop is the library's and the reference's: a level is added while the
    list holds AT MOST maxlevels entries, so a hierarchy that is cut holds maxlevels + 1 levels."""
    g = tuple(int(n) + 2 for n in N)
    out = [g]
    while len(out) <= maxlevels:
        c = [divisible(n) for n in g]
        if not any(c):
            break
        g = tuple(1 + n // 2 if d else n for n, d in zip(g, c))
        out.append(g)
    return out


def level_cap_cuts(N):
    lv = levels(N)
    return len(lv) == MAXLEVELS + 1 and any(divisible(n) for n in lv[-1])


def cells(g):
    return g[0] * g[1] * g[2]


# ------------------------------------------------------------------------------------------------------------------------------- the gates
class Gate:
    """name, source file under csrc/, the quoted source expressions it restates, and the restatement: a function of a level's (nx, ny, nz) with ghosts"""

    def __init__(self, name, file, quotes, fn, doc):
        self.name, self.file, self.quotes, self.fn, self.doc = name, file, tuple(quotes), fn, doc

    def __call__(self, g):
        return self.fn(g)


GATES = {}


def _gate(name, file, quotes, fn, doc):
    GATES[name] = Gate(name, file, quotes, fn, doc)
    return GATES[name]


gsrb_fused_ok = _gate("gsrb_fused_ok", "wl_fused.hip", ["g.nz == g.gnz && g.nx >= 34 && g.ny >= 18 && (g.k1 - g.k0) >= 8"],
                      lambda g: g[0] >= 34 and g[1] >= 18 and g[2] - 2 >= 8, "the temporally blocked smoother: nx ≥ 34, ny ≥ 18, at least 8 planes")
gsrb_pair_geom_ok = _gate("gsrb_pair_geom_ok", "wl_fused2.hip",
                          ["(g.nx & 1) == 0 && g.nx >= pair_min_nx() && g.ny >= 34 && g.gnz >= 10 && (g.k1 - g.k0) >= 8", 'wl_exp_int("WL_PAIR_MIN_NX", 34)'],
                          lambda g: g[0] % 2 == 0 and g[0] >= 34 and g[1] >= 34 and g[2] >= 10 and g[2] - 2 >= 8, "the pair kernels: even nx ≥ 34, ny ≥ 34, gnz ≥ 10")
rows16 = _gate("rows16", "wl_fused2.hip", ["const long tiles32 = (long)((g.nx + 55) / 56) * ((g.ny + 25) / 26);", "return tiles32 < 128;"],
               lambda g: ((g[0] + 55) // 56) * ((g[1] + 25) // 26) < 128, "16-row instances of kernels A and B below 128 tiles of 64×32, 32-row instances from there")
resjac_ok = _gate("resjac_ok", "wl_resjac.hip", ["(g.nx & 1) == 0 && g.nx >= 66 && g.ny >= 34 &&", "g.gnz >= 10 && g.cs < (1L << 30) && (long)(g.nx - 2) * (g.ny - 2) * (g.gnz - 2) >= g_resjac_min"],
                  lambda g: g[0] % 2 == 0 and g[0] >= 66 and g[1] >= 34 and g[2] >= 10, "the one-launch projection head: even nx ≥ 66, ny ≥ 34, gnz ≥ 10")
conv_tile_ok = _gate("conv_tile_ok", "wl_convt.hip", ["if (3L * g.cs >= (1L << 31) || g.nx < 34 || g.ny < 18) return false;", "return nplanes >= (g_convt_min > 0 ? 8 : 1) && ntiles * nplanes >= g_convt_min;"],
                     lambda g: g[0] >= 34 and g[1] >= 18, "the tiled conv_diff!+BDIM!: nx ≥ 34, ny ≥ 18")
conv_tile_whole = _gate("conv_tile_whole", "wl_convf.hip", ["const bool full = (g.nx - 2) % CF_CX == 0 && (g.ny - 2) % CF_CY == 0;", "#define CF_CX (2 * CF_TX)        // 64 core cells along x", "#define CF_CY CF_TY              // 16 core rows"],
                        lambda g: (g[0] - 2) % 64 == 0 and (g[1] - 2) % 16 == 0, "whole 64×16 tiles choose the instance of the tiled kernel without the ragged-edge tests")
conv_proj_ok = _gate("conv_proj_ok", "wl_convf.hip", ["g.nz >= 6 && (g.nx - 2) % CF_CX == 0 && (g.ny - 2) % CF_CY == 0 && conv_tile_ok(g, per, g.k1 - g.k0)"],
                     lambda g: g[2] >= 6 and (g[0] - 2) % 64 == 0 and (g[1] - 2) % 16 == 0 and conv_tile_ok(g), "the corrector's loader takes the projection tail: whole tiles only, nz ≥ 6")
conv_march_ok = _gate("conv_march_ok", "wl_convm.hip", ["g.cs < (1L << 30) && g.nx >= 8 && g.ny >= 8"], lambda g: g[0] >= 8 and g[1] >= 8,
                      'the z-marching conv_diff! ("convm" = 1, where the tiled kernel does not run): nx ≥ 8, ny ≥ 8')
conv_z_ok = _gate("conv_z_ok", "wl_convz.hip", ["per == 0 && g.nx >= 34 && g.ny >= 18 && g.cs < (1L << 30)"], lambda g: g[0] >= 34 and g[1] >= 18,
                  'the flux-once z-marching conv_diff! ("convz" = 1): nx ≥ 34, ny ≥ 18')
project_wide_path = _gate("project_wide_path", "wl_project.hip",
                          ["(g.nx & 1) == 0 && g.nx >= 8 && g.ny >= 4 && (g.sz & 3) == 0 && g.k0 >= 1 && g.k1 <= g.nz - 1", "if (tw_lds_bytes(g) > 48 * 1024 || (long)tw_nb8(g) * g.nz > 0x7fffffffL) return false;",
                           "return (size_t)(WL_TW_CHUNK + 2 * g.sy + 8) * sizeof(float); }", "#define WL_TW_CHUNK (4 * WL_BLOCK)"],
                          lambda g: g[0] % 2 == 0 and g[0] >= 8 and g[1] >= 4 and (g[0] * g[1]) % 4 == 0 and (1024 + 2 * g[0] + 8) * 4 <= 48 * 1024,
                          "the four-cells-per-thread projection tails: even nx ≥ 8, ny ≥ 4, nx·ny a multiple of 4, staged window (2·nx + 1032 floats) within 48 KiB of LDS")
fold_ok = _gate("fold_ok", "wl_bcfold.hpp", ["g.nz == g.gnz && g.nx >= 6 && g.ny >= 6 && g.nz >= 6"], lambda g: min(g) >= 6, "BC! folded into the producer's stores: every side ≥ 6")
tail_cells_ok = _gate("tail_ok", "wl_mg.hip", ["if (lv[(size_t)first].g.D != 3 || lv[(size_t)first].x_.cs > WL_TAIL_CELLS) return false;", "(int)lv.size() - first > WL_TAIL_MAXLV"],
                      lambda g: cells(g) <= WL_TAIL_CELLS, "the rest of the V-cycle in one launch from the first level of at most 8192 cells")
const_L_ok = _gate("check_const_L", "wl_poisson.hip", ["if (g.nx < 4 || g.ny < 4 || (g.D == 3 && (g.k1 - g.k0) < 1)) return 0;"], lambda g: g[0] >= 4 and g[1] >= 4 and g[2] >= 4,
                   "a level can be verified as constant-coefficient at all (every shape here: its finest level can)")
# quoted only: constants and loops the restatement above rests on
QUOTED = [
    ("wl_common.hpp", "#define WL_TAIL_MAXLV 8"), ("wl_common.hpp", "#define WL_TAIL_CELLS 8192"), ("wl_common.hpp", "#define WL_MAXPART 65536"),
    ("wl_mg.hip", "bool wl_mg_divisible(int n) { return (n % 2 == 0) && n > 4; }"), ("wl_mg.hip", "while ((int)grids.size() <= maxlevels) {"),
    ("wl_sim.hip", "desc->perdir_mask, 10, s->comm);"), ("wl_capi.hip", "maxlevels <= 0 ? 10 : maxlevels"),
    ("wl_sim.hip", "wl::resjac_enable(1, 6L << 20); wl::conv_tile_min(2048);"), ("wl_sim.hip", "TAILFUSE_MIN_DEFAULT = 16L << 20;"),
    ("wl_convt.hip", "#define CT_CX (2 * CT_TX)        // 64 core cells along x"), ("wl_convt.hip", "#define CT_CY CT_TY              // 16 core rows"),
    # the conjunctions predicted() follows
    ("wl_sim.hip", "(long)(G.nx - 2) * (G.ny - 2) * (G.gnz - 2) >= tailfuse_min && wl::conv_proj_ok(G, d.perdir_mask);"),
    ("wl_sim.hip", "mg->defer_shift && mg->lv.size() > 1 && wl::resjac_ok(G, l0.cl) &&"),
    ("wl_sim.hip", "if (!(use_bcdefer && in_step && !df.bc_folded && fold_ok(1) && head_fused_ok())) return false;"),
    ("wl_sim.hip", "bool pdefer_ok() const { return use_pdefer && in_step && !sgs_model && !forcing && !d.has_body && head_fused_ok(); }"),
    ("wl_sim.hip", "return use_tailfuse && fold_ok(3) && fused_nobody_conv() && !store_f && !use_convz && !df.u_pending && mg->lv[0].cl.on && !mg->lv[0].part &&"),
    ("wl_mg.hpp", "return bout == wl::B_XONLY && skip_r && !store_eps && !comm && !p.dist && !p.part && !perdir && wl::gsrb_pair_B_ok(nullptr, p.r, p.x, p.em, p.rs, p.x_, p.cl) &&"),
    ("wl_mg.hpp", "bool blocked(const Level& v) const { return use_fused && (wl::gsrb_fused_ok(v.x_, perdir, v.dist) || pair_slab(v)); }"),
    ("wl_capi.hip", "default: return wl::gsrb_pair_ok(p.x_, p.cl) ? 2 : 1;"),
    ("wl_sim.hip", "int itmx = 32;"), ("wl_mg.hip", "if (st.hf[WL_RF_GO] > 0.f) { spec.tail_stood = true; break; }"),
    ("wl_flow.hip", "const bool march = !tiled && D == 3 && wl::conv_march_ok(g);"),
]


# ------------------------------------------------------------------------------------------------------------------------ z-chunk choosers
class Chooser:
    def __init__(self, name, file, quotes, doc):
        self.name, self.file, self.quotes, self.doc = name, file, tuple(quotes), doc


CHOOSERS = {
    "zchunk_for": Chooser("zchunk_for", "wl_fused.hip", ["if (zc < (zmin_env ? zmin_env : 4)) break;", "if (W < 512) cost = (long)((zc + warm) * 1.25);", "if ((long)nt * ((np + 31) / 32) >= 2048) {",
                                                         "long cost = ((W + 511) / 512) * (zc + warm);"], "z-chunks of the one-cell blocked kernels A (H = 2) and B (H = 3)"),
    "zchunk2": Chooser("zchunk2", "wl_fused2_body.inc", ["if (W < SX) cost = (zc + warm) * 1.3;", "double cost = (double)rounds * (zc + warm) * (1.0 + 0.3 / (double)rounds);",
                                                         "const long per = (nt + 7) >> 3, SX = 32L * (1024 / PT_N);", "const int CX = 2 * PT_X - 2 * HX, CY = PT_Y - 2 * HY;"],
                       "z-chunks of the pair kernels A (HX, HY = 2, 2) and B (4, 3), per row instance"),
    "conv_tile": Chooser("conv_tile", "wl_convt.hip", ["if (g_convt_min == 0 && !g_convt_chunk && !envc) zc = 5;   // tests: several chunks on a small box", "if (zc > np) zc = np;"],
                         "z-chunks of the tiled conv_diff!+BDIM!: 5 planes once the size gate is opened"),
    "wl_march_chunk": Chooser("wl_march_chunk", "wl_common.hpp", ["long c = (long)nplanes * bp / 4096; if (c > cap) c = cap; if (c < 1) c = 1;", "while ((nplanes + c - 1) / c * bp > 65536 && c < nplanes) c++;"],
                              "z-chunks of the z-marching Jacobi! (the owned planes) and of the two-kernel head's residual pass (all planes)"),
}


def ztile_count(nx, ny, H):
    CX, CY = 64 - 2 * H, 16 - 2 * H
    return ((nx - 2 + CX - 1) // CX) * ((ny - 2 + CY - 1) // CY)


def zchunk_for(g, H):
    nt, np_ = ztile_count(g[0], g[1], H), g[2] - 2
    if nt * ((np_ + 31) // 32) >= 2048:
        chunks = (1536 + nt - 1) // nt
        return min(max((np_ + chunks - 1) // chunks, 16), np_)
    warm = (5 if H == 3 else 3) + 3
    best, best_zc = -1, np_
    for chunks in range(1, np_ + 1):
        zc = (np_ + chunks - 1) // chunks
        if zc < 4:
            break
        W = nt * ((np_ + zc - 1) // zc)
        cost = ((W + 511) // 512) * (zc + warm)
        if W < 512:
            cost = int((zc + warm) * 1.25)
        if best < 0 or cost < best:
            best, best_zc = cost, zc
    return best_zc


def ptile_count(nx, ny, HX, HY, rows):
    CX, CY = 64 - 2 * HX, rows - 2 * HY
    return ((nx - 1 + CX - 1) // CX) * ((ny - 2 + CY - 1) // CY)


def zchunk2(g, HX, HY, rows):
    nt, np_ = ptile_count(g[0], g[1], HX, HY, rows), g[2] - 2
    warm = (5 if HY == 3 else 3) + 3
    per, SX = (nt + 7) >> 3, 32 * (1024 // (32 * rows))
    best, best_zc = -1.0, np_
    for chunks in range(1, np_ + 1):
        zc = (np_ + chunks - 1) // chunks
        if zc < 4:
            break
        W = per * ((np_ + zc - 1) // zc)
        rounds = (W + SX - 1) // SX
        cost = float(rounds) * (zc + warm) * (1.0 + 0.3 / float(rounds))
        if W < SX:
            cost = (zc + warm) * 1.3
        if best < 0 or cost < best:
            best, best_zc = cost, zc
    return best_zc


def conv_tile_chunk(g, gates_lowered=True):
    np_ = g[2] - 2
    ntiles = ((g[0] - 2 + 63) // 64) * ((g[1] - 2 + 15) // 16)
    zc = 5 if gates_lowered else min(max(np_ * ntiles // 1024, 5), 64)
    return min(zc, np_)


def wl_march_chunk(g, nplanes):
    bp = 8 * ((((g[0] * g[1] + 255) // 256) + 7) >> 3)
    c = min(max(nplanes * bp // 4096, 1), 32)
    while (nplanes + c - 1) // c * bp > 65536 and c < nplanes:
        c += 1
    return c


def chunk_class(np_, zc):
    return "one" if zc >= np_ else ("whole" if np_ % zc == 0 else "ragged")


def smoother_kind(g):
    """wl_mg_smoother_kind of a body-free single-domain level under default switches"""
    return 0 if not gsrb_fused_ok(g) else (2 if gsrb_pair_geom_ok(g) else 1)


def tail_first(N):
    """the first level the single-launch tail takes (wl_mg::vcycle asks tail_ok(l + 1) on the way down), or None"""
    lv = levels(N)
    for first in range(1, len(lv)):
        if len(lv) - first <= WL_TAIL_MAXLV and tail_cells_ok(lv[first]):
            return first
    return None


def chunk_classes(N, gates_lowered=True):
    """which chooser decides what on level 0, as (one | whole | ragged) per launch that uses it; None where the chooser's kernel does not run there"""
    g = levels(N)[0]
    np_, kind = g[2] - 2, smoother_kind(g)
    r = 16 if rows16(g) else 32
    return {
        "zchunk_for": (chunk_class(np_, zchunk_for(g, 2)), chunk_class(np_, zchunk_for(g, 3))) if kind == 1 else None,
        "zchunk2": (chunk_class(np_, zchunk2(g, 2, 2, r)), chunk_class(np_, zchunk2(g, 4, 3, r))) if kind == 2 else None,
        "conv_tile": chunk_class(np_, conv_tile_chunk(g, gates_lowered)) if conv_tile_ok(g) else None,
        "wl_march_chunk": (chunk_class(np_, wl_march_chunk(g, np_)), chunk_class(g[2], wl_march_chunk(g, g[2]))),
    }


def state(N):
    """every restated decision of the finest level (and the two of the hierarchy) at interior dims N with the size gates open: what a pair of shapes may flip"""
    g = levels(N)[0]
    kind = smoother_kind(g)
    out = {n: bool(GATES[n](g)) for n in ("gsrb_fused_ok", "gsrb_pair_geom_ok", "resjac_ok", "conv_tile_ok", "conv_proj_ok", "conv_march_ok", "conv_z_ok", "project_wide_path", "fold_ok")}
    out["rows16"] = bool(rows16(g)) if kind == 2 else None
    out["conv_tile_whole"] = bool(conv_tile_whole(g)) if conv_tile_ok(g) else None
    out["tail_ok"] = tail_first(N)
    out["level_cap"] = level_cap_cuts(N)
    for n, v in chunk_classes(N).items():
        out["chunks:" + n] = v
    return out


# ------------------------------------------------------------------------------------------------------------------------------ predicted
def predicted(N, gates_lowered, extra=None):
    """what a body-free, non-periodic, tuple-U handle with default switches (plus `extra`) dispatches at interior dims N after optmatrix.CALLS:
    {"nlevels", "levels", "smoother_kinds", "counters": {name: True (must be > 0) | False (must not have run)}}.  The switch side is optmatrix.live() of the
    whole-tile or the ragged family; the geometry side is the restated gates, joined as wl_sim.hip (head_fused_path, bcdefer_ok, pdefer_ok, tailfuse_ok) and
    wl_mg.hpp (b_xonly_ok) join them."""
    lv = levels(N)
    g = lv[0]
    interior = (g[0] - 2) * (g[1] - 2) * (g[2] - 2)
    kinds = [smoother_kind(v) for v in lv]
    by_switch = om.live(dict(extra or {}), "box" if conv_tile_whole(g) else "ragged")
    cl0 = const_L_ok(g)
    head = cl0 and len(lv) > 1 and resjac_ok(g) and interior >= (0 if gates_lowered else RESJAC_MIN_DEFAULT)      # head_fused_path
    tile_gate = (1, 0) if gates_lowered else (8, CONVT_MIN_DEFAULT)
    ntiles = ((g[0] - 2 + 63) // 64) * ((g[1] - 2 + 15) // 16)
    tiled = conv_tile_ok(g) and g[2] - 2 >= tile_gate[0] and ntiles * (g[2] - 2) >= tile_gate[1]
    geom = {
        "resjac": head,
        "pdefer": head,                                                                       # pdefer_ok: head_fused_ok
        "bcdefer": head and fold_ok(g),                                                       # bcdefer_ok: fold_ok(1) && head_fused_ok
        "tailspec": head,                                                                     # armed by the speculative first V-cycle behind that head
        "tailfuse": cl0 and fold_ok(g) and conv_proj_ok(g) and tiled and interior >= (0 if gates_lowered else TAILFUSE_MIN_DEFAULT),      # tailfuse_ok
        "tailwide": cl0 and project_wide_path(g),
        "rskip": kinds[0] == 2,                                                               # b_xonly_ok: gsrb_pair_B_ok on the finest level
        "xdefer": kinds[0] == 2,                                                              # plan_smooth: gsrb_pair_B_ok
    }
    return {"nlevels": len(lv), "levels": lv, "smoother_kinds": kinds, "counters": {c: bool(geom[c] and c in by_switch) for c in COUNTERS}}


# ---------------------------------------------------------------------------------------------------------------------------------- shapes
# (gate, clause, inside N, outside N, the OTHER entries of state() that flip with it, extra switches on handle A).  The flips are asserted by
# tests/test_shapegates_cpu.py, so nobody believes a pair isolates a gate it does not.
PAIRS = []


def _pair(gate, clause, inside, outside, flips=(), extra=None):
    PAIRS.append({"gate": gate, "clause": clause, "in": tuple(inside), "out": tuple(outside), "flips": frozenset(flips), "extra": dict(extra or {})})


_C = "chunks:"
# level-0 smoother kind: 32×32×8 pair (2); 32×30×8, 33×32×8 and 32×16×8 blocked (1); 30×32×8, 32×14×8, 32×32×6 passes (0)
_pair("gsrb_pair_geom_ok", "ny >= 34", (32, 32, 8), (32, 30, 8), ["rows16", _C + "zchunk2", _C + "zchunk_for"])
_pair("gsrb_pair_geom_ok", "nx even", (32, 32, 8), (33, 32, 8), ["rows16", _C + "zchunk2", _C + "zchunk_for", "project_wide_path"])
_pair("gsrb_pair_geom_ok", "nx >= 34 (with gsrb_fused_ok, conv_tile_ok and conv_z_ok: the same bound)", (32, 32, 8), (30, 32, 8),
      ["gsrb_fused_ok", "conv_tile_ok", "conv_z_ok", "conv_tile_whole", "rows16", _C + "zchunk2", _C + "conv_tile"])
_pair("gsrb_pair_geom_ok", "gnz >= 10 (with gsrb_fused_ok's 8 planes: the same bound on a single domain)", (32, 32, 8), (32, 32, 6),
      ["gsrb_fused_ok", "rows16", _C + "zchunk2"])
_pair("gsrb_fused_ok", "nx >= 34", (32, 16, 8), (30, 16, 8), ["conv_tile_ok", "conv_z_ok", "conv_tile_whole", _C + "zchunk_for", _C + "conv_tile"])
_pair("gsrb_fused_ok", "ny >= 18", (32, 16, 8), (32, 14, 8), ["conv_tile_ok", "conv_z_ok", "conv_tile_whole", _C + "zchunk_for", _C + "conv_tile"])
_pair("gsrb_fused_ok", "8 planes", (32, 16, 8), (32, 16, 6), [_C + "zchunk_for"])
# the fused head: 64×32×8 in; out by each clause.  At 62×32×8 the pair kernels, rskip and xdefer stay live while pdefer, bcdefer and tailspec read 0
_pair("resjac_ok", "nx >= 66", (64, 32, 8), (62, 32, 8), ["conv_proj_ok", "conv_tile_whole"])
_pair("resjac_ok", "ny >= 34", (64, 32, 8), (64, 30, 8), ["gsrb_pair_geom_ok", "rows16", "conv_proj_ok", "conv_tile_whole", _C + "zchunk2", _C + "zchunk_for"])
_pair("resjac_ok", "nx even", (64, 32, 8), (63, 32, 8), ["gsrb_pair_geom_ok", "rows16", "conv_proj_ok", "conv_tile_whole", "project_wide_path", _C + "zchunk2", _C + "zchunk_for"])
_pair("resjac_ok", "gnz >= 10", (64, 32, 8), (64, 32, 6), ["gsrb_fused_ok", "gsrb_pair_geom_ok", "rows16", _C + "zchunk2"])
# whole tiles / tailfuse: 64×16×8 has tailfuse without the head (ny = 18 < 34); 66×32×8 and 64×34×8 are ragged in x and in y
_pair("conv_proj_ok", "(nx - 2) % 64 == 0", (64, 32, 8), (66, 32, 8), ["conv_tile_whole"])
_pair("conv_proj_ok", "(ny - 2) % 16 == 0", (64, 32, 8), (64, 34, 8), ["conv_tile_whole"])
_pair("conv_proj_ok", "whole tiles below the head and the pair kernels", (64, 16, 8), (62, 16, 8), ["conv_tile_whole"])
_pair("conv_proj_ok", "nz >= 6 (with fold_ok's: the same bound in z)", (64, 32, 4), (64, 32, 2), ["fold_ok"])
_pair("fold_ok", "nz >= 6 (with conv_proj_ok's)", (64, 32, 4), (64, 32, 2), ["conv_proj_ok"])
# tailwide: a plane that is no whole number of quads needs an odd ny, so it is ragged as well; the LDS clause and the small-side clause flip alone
_pair("project_wide_path", "nx·ny % 4 == 0", (64, 32, 8), (64, 33, 8), ["conv_proj_ok", "conv_tile_whole"])
_pair("project_wide_path", "staged window <= 48 KiB: 2·5626 + 1032 = 12284 floats = 49136 B against 2·5634 + 1032 = 12300 = 49200 B (the two hierarchies differ: the tail starts on another level)",
      (5624, 8, 8), (5632, 8, 8), ["tail_ok"])
_pair("project_wide_path", "nx >= 8", (6, 16, 8), (4, 16, 8), ["conv_march_ok"])
# the conv_diff! kernel: tiled / z-marching ("convm") / plane kernel, and "convz" where the tiled geometry holds
_pair("conv_march_ok", "nx >= 8", (30, 16, 8), (4, 16, 8), ["project_wide_path"], extra={"convm": 1})
_pair("conv_march_ok", "ny >= 8", (30, 16, 8), (64, 4, 16), extra={"convm": 1})
_pair("conv_z_ok", "nx >= 34", (32, 16, 8), (30, 16, 8), ["gsrb_fused_ok", "conv_tile_ok", "conv_tile_whole", _C + "zchunk_for", _C + "conv_tile"], extra={"convz": 1})
_pair("conv_z_ok", "ny >= 18", (32, 16, 8), (32, 14, 8), ["gsrb_fused_ok", "conv_tile_ok", "conv_tile_whole", _C + "zchunk_for", _C + "conv_tile"], extra={"convz": 1})
_pair("conv_tile_ok", "nx >= 34", (32, 16, 8), (30, 16, 8), ["gsrb_fused_ok", "conv_z_ok", "conv_tile_whole", _C + "zchunk_for", _C + "conv_tile"])
_pair("conv_tile_whole", "whole against ragged 64×16 tiles", (64, 16, 8), (32, 16, 8), ["conv_proj_ok"])
# row instance of the pair kernels: 9 × 15 = 135 tiles (32 rows) against 9 × 13 = 117 (16 rows)
_pair("rows16", "tiles32 < 128", (448, 336, 8), (448, 364, 8), ["conv_proj_ok", "conv_tile_whole", _C + "zchunk2", "tail_ok"])
# coarse tail: level 1 of 64×32×16 is 34×18×10 = 6120 cells and goes to the tail although it passes gsrb_fused_ok; level 1 of 64×32×32 is 34×18×18 = 11016
_pair("tail_ok", "first level of at most 8192 cells", (64, 32, 16), (64, 32, 32))
# level cap: 4096 = 2^12 has 12 possible levels and is cut at 11 (the loop adds a level while the list holds at most 10); 2048 and 3072 have 11 and are not
_pair("level_cap", "a level is added while the list holds at most 10", (2048, 8, 8), (4096, 8, 8), ["tail_ok"])
_pair("level_cap", "3·2^10: eleven possible levels, all built", (3072, 8, 8), (4096, 8, 8), ["tail_ok"])

# z-chunks: (chooser, class, N).  Classes are (kernel A, kernel B) for the two smoothers and (owned planes, all planes) for wl_march_chunk
CHUNK_SHAPES = [
    ("zchunk_for", ("whole", "whole"), (32, 30, 8)), ("zchunk_for", ("ragged", "ragged"), (32, 30, 9)),
    ("zchunk2", ("whole", "whole"), (32, 32, 8)), ("zchunk2", ("ragged", "ragged"), (32, 32, 9)), ("zchunk2", ("whole", "one"), (448, 365, 8)),
    ("conv_tile", "one", (64, 32, 4)), ("conv_tile", "ragged", (64, 32, 8)), ("conv_tile", "whole", (64, 32, 10)),
    ("wl_march_chunk", ("whole", "whole"), (64, 32, 8)), ("wl_march_chunk", ("whole", "whole"), (8, 8, 2046)), ("wl_march_chunk", ("ragged", "ragged"), (8, 8, 2047)),
]
# classes no shape under CELL_CAP reaches, with the arithmetic
CHUNK_UNREACHABLE = {
    ("zchunk_for", "one"): "a level of >= 8 planes always has a split into chunks of >= 4 planes, and below 512 workgroups the cost (zc + warm)·1.25 falls with zc; one chunk wins only "
                           "from 512 tiles of 60×12 cells = 368 640 cells per plane, ×10 planes = 3.7 M cells > 1 665 000",
    ("zchunk2", "one (kernel A)"): "kernel A keeps one chunk from per = 17, i.e. 129 tiles of 60×28 cells = 216 720 cells per plane > 166 500 (kernel B, 56×26 tiles, gets there at 448×365×8)",
    ("wl_march_chunk", "one"): "one chunk needs nplanes·bp >= 4096·nplanes, i.e. bp >= 4096 blocks per plane = 1 M cells per plane > 166 500",
}
# gates no shape under CELL_CAP reaches: the four the issue names, with the arithmetic
UNREACHABLE = {
    "WL_TAIL_MAXLV": "tail_ok refuses a first level with more than 8 levels from it down.  A level of <= 8192 cells that still has 8 coarser ones must halve 8 more times in one direction: "
                     ">= 512 interior cells there, so at most 8192 / 514 = 15 cells across (3×3 or 3×5 with ghosts: 1 to 3 interior cells) — 514×4×4 = 8224 already exceeds 8192.  "
                     "Only a one-cell-thick strip gets there: not a 3-D flow, and fold_ok, conv_march_ok and project_wide_path all refuse it",
    "32-bit offsets (cs < 2^30, 3·cs < 2^31, tw_nb8·nz)": "cs < 2^30 needs 1.07e9 cells in one array, 3·cs < 2^31 needs 7.2e8; tw_nb8·nz <= 2^31 − 1 needs 2^31 chunks of 1024 cells; CELL_CAP is 1 665 000",
    "WL_MAXPART in gsrb_pair_B_kernel_norms": "8·per·nch <= 65536 workgroups fails from 65537 workgroups of at least 56×10×4 core cells each = 1.5e8 cells > 1 665 000",
    "65536 partials in wl_march_chunk": "(nplanes / c)·bp > 65536 with c <= 32 needs nplanes·bp > 65536: at 256 cells per block more than 1.6e7 cells > 1 665 000 "
                                        "(a thin column has bp = 8 and would need 8192 planes of chunk 1, but its chunk is already nplanes·8 / 4096 = 16)",
}
# gates whose two sides are not told apart by kinds or counters: the library has no such read-out for them (every other pair asserts different kinds or counters on its two sides)
NO_READOUT = {
    "rows16": "the row instance is chosen inside gsrb_pair_A / gsrb_pair_B; wl_mg_smoother_kind says 2 for both",
    "tail_ok": "wl_mg_smoother_kind reports the form smooth! would take on the level, not that the tail absorbed it",
    "conv_march_ok": "no counter for the conv_diff! kernel",
    "conv_z_ok": "no counter for the conv_diff! kernel (bcdefer stands down with convz on both sides)",
    "conv_tile_ok": "no counter for the conv_diff! kernel",
    "conv_tile_whole": "instances of one kernel (tailfuse, which needs whole tiles, is conv_proj_ok's read-out)",
    "level_cap": "both sides have 11 levels: the read-out is wl_mg_level_grid per level against levels(), whose last entry at 4096×8×8 (6×4×4) could still be coarsened",
    "fold_ok": "its counters (tailfuse, bcdefer) need conv_proj_ok or the head as well: conv_proj_ok's pair is the read-out",
}


def _cases():
    """(N, extra) of every GPU case, in the order of PAIRS and CHUNK_SHAPES, each once"""
    out = []
    for p in PAIRS:
        for N in (p["in"], p["out"]):
            for ex in ({}, p["extra"]):
                if (N, tuple(sorted(ex.items()))) not in [(n, tuple(sorted(e.items()))) for n, e in out]:
                    out.append((N, ex))
    for _, _, N in CHUNK_SHAPES:
        if (N, ()) not in [(n, tuple(sorted(e.items()))) for n, e in out]:
            out.append((N, {}))
    return out


CASES = _cases()
SHAPES = sorted({N for N, _ in CASES})


def case_id(case):
    N, ex = case
    return "x".join(str(n) for n in N) + "".join("-%s%d" % kv for kv in sorted(ex.items()))


# ----------------------------------------------------------------------------------------------------------------------------- on the GPU
SEED = 137
# a seed changed for one shape: only where the first difference between A and P was a decision taken from r₁ or Σr and the two logged r₁ lay within
# l1·(2⁻²⁴ + n·2⁻⁵³) of each other (a reordering tie).  {N: (seed, old seed, the two r₁)}
SEEDS = {}
NU = 0.02
ITMX = 32      # solver!'s cap in mom_project! (the library's and the oracle's default)


def u_init(N):
    import numpy as np
    seed = SEEDS.get(tuple(N), (SEED,))[0]
    return np.asfortranarray(np.random.default_rng(seed).uniform(-0.4, 0.4, size=tuple(n + 2 for n in N) + (3,)).astype(np.float32))


PLAIN_ROW = {n: om.PLAIN[n] for n in om.names("box")}


def last_log(w, h):
    """solver!'s logged (r₁, r∞) of the handle's last solve"""
    import ctypes as C
    cap = 80
    a, b, c = (C.c_double * cap)(), (C.c_double * cap)(), (C.c_double * cap)()
    k = w.lib().wl_mg_last_log(w.lib().wl_sim_pois(h._h), a, b, c, cap)
    return list(a[:k]), list(b[:k])


def level_grids(w, h):
    import ctypes as C
    from waterlily_jl_amd._lib import wl_grid
    mg, out = w.lib().wl_sim_pois(h._h), []
    for l in range(h.nlevels()):
        g = wl_grid()
        assert w.lib().wl_mg_level_grid(mg, l, C.byref(g)) == 0
        out.append((g.nx, g.ny, g.nz))
    return out


def run(w, N, row, gates, calls=om.CALLS):
    """a fresh handle at interior dims N (seeded random u⁰ in (−0.4, 0.4), callseq.UBC, ν = 0.02) with the switches of `row` and, if `gates`, the size gates
    opened, through `calls`.  The process-wide switches are reset first: handles of different rows are run one after the other."""
    w.lib().wl_reset_process_options()
    h = w.FusedSimulation(tuple(N), callseq.UBC, N[0], U=1, nu=NU, u0=u_init(N))
    for n, v in row.items():
        h.set_option(n, int(v))
    if gates:
        for n, v in callseq.GATES.items():
            h.set_option(n, int(v))
    out = {"u_init": h.field("u"), "snaps": [], "err": None, "logs": []}
    for c in calls:
        try:
            om.call(h, c)
        except Exception as e:      # an error return of the library: reported, nothing more is run on this handle
            out["err"] = "%s%r: %s" % (c[0], c[1:], e)
            break
        out["snaps"].append(om.Snap(h))
        out["logs"].append(last_log(w, h))
    out["cnt"] = {a: h.counter(a) for a in COUNTERS + ("resjac_redo", "tailspec_armed", "rskip_redo")}
    out["kinds"], out["nlevels"], out["grids"] = h.smoother_kinds(), h.nlevels(), level_grids(w, h)
    return out


def dispatch_faults(N, got, gates_lowered, extra=None):
    """what the handle reports against predicted(): a list of readable lines"""
    want = predicted(N, gates_lowered, extra)
    out = []
    if got["nlevels"] != want["nlevels"] or got["grids"] != want["levels"]:
        out.append("levels %r, restated %r" % (got["grids"], want["levels"]))
    if got["kinds"] != want["smoother_kinds"]:
        out.append("smoother kinds %r, restated %r" % (got["kinds"], want["smoother_kinds"]))
    for c in COUNTERS:
        ran = got["cnt"][c] > 0      # ("xdefer" reads −1 where no smooth! of the finest level took a prolongation, 0 where kernel A applied it: neither ran)
        if c == "tailspec" and want["counters"][c]:
            # the gated tail is ARMED for every solve behind the fused head whose tail can be gated (the corrector's always can) and runs gated where that
            # solve converges; a solve that runs into solver!'s cap has it withheld (include/wlhip.h).  So: armed, and run wherever a corrector's solve
            # (every second entry of pois.n) stopped below the cap
            below_cap = got["snaps"] and any(n < ITMX for n in list(got["snaps"][-1].pois_n)[1::2])
            if got["cnt"]["tailspec_armed"] <= 0 or (below_cap and not ran):
                out.append("tailspec = %d of %d armed, pois.n %r, restated armed and > 0 below the cap" % (got["cnt"][c], got["cnt"]["tailspec_armed"], list(got["snaps"][-1].pois_n)))
            continue
        if ran != want["counters"][c] or (not ran and c != "xdefer" and got["cnt"][c] != 0):
            out.append("%s = %d, restated %s" % (c, got["cnt"][c], "> 0" if want["counters"][c] else "== 0"))
    if not want["counters"]["tailspec"] and got["cnt"]["tailspec_armed"] != 0:
        out.append("tailspec armed %d times, restated never" % got["cnt"]["tailspec_armed"])
    return out
