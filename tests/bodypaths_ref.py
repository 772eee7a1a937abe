"""NumPy restatement of what decides the body-aware fast paths (csrc/wl_flow.hip k_body_mask2, body_masks_box, body_masks_planes,
conv_diff_bdim_body; csrc/wl_mg.hip wl_mg::update, wl_mg::zsplit_ranges): from host copies of μ₀, μ₁, V (ghost cells included, as FusedSimulation.field
returns them) the three masks per (plane, workgroup of 256 consecutive in-plane cells), the two host scans, the census the library
reports through wl_sim_counter("mask_*"), and the plane ranges the tiled conv_diff! and the z-split smoother take.  Test infrastructure.
tests/bodyshapes.py crosses this matrix with grid shapes: the gates of the body code that only a shape moves, and the z-split on coarse levels."""
import numpy as np

WG = 256          # WL_BLOCK: a workgroup is 256 consecutive cells m = i + j·nx of one plane (ghosts included), workgroup index m // 256


def _planes(a, D):
    """(nx, ny, nz, ...) view with nz = 1 in 2-D"""
    return a if D == 3 else a.reshape(a.shape[:2] + (1,) + a.shape[2:])


def wall_pattern(Ng):
    """wl_cl_coef(I_a, N_a, 1) per cell and component: 0 on the faces BC!(μ₀,0) zeroes (Julia index ≤ 2 or ≥ N), 1 elsewhere"""
    D = len(Ng)
    pat = np.ones(tuple(Ng) + (D,), np.float32)
    for a in range(D):
        idx = np.arange(Ng[a])                      # 0-based: I = idx + 1
        wall = (idx <= 1) | (idx >= Ng[a] - 1)
        sl = [None] * D; sl[a] = slice(None)
        pat[..., a] = np.where(wall[tuple(sl)], np.float32(0), np.float32(1))
    return pat


def nbm(Ng):
    """body_masks_nbm: the plane's workgroups rounded up to a multiple of 8"""
    nbx = (Ng[0] * Ng[1] + WG - 1) // WG
    return 8 * ((nbx + 7) // 8)


def masks(mu0, mu1, V):
    """near, needf, m0var as (nz, nbm) arrays of 0/1 (k_body_mask2)"""
    D = mu0.shape[-1]
    Ng = mu0.shape[:-1]
    nx, ny = Ng[0], Ng[1]
    sz = nx * ny
    var = _planes((mu0 != wall_pattern(Ng)).any(-1), D)
    nz1 = _planes((mu1 != 0).any((-1, -2)), D)
    nzv = _planes((V != 0).any(-1), D)
    nz = var.shape[2]
    nb = nbm(Ng)
    flat = lambda a: a.reshape(sz, nz, order="F")      # m = i + j·nx
    wg = np.arange(sz) // WG
    near, needf, m0var = (np.zeros((nz, nb), np.uint8) for _ in range(3))
    fv, f1, fn = flat(var), flat(nz1), flat(nz1 | nzv)
    for k in range(nz):
        m0var[k, wg[fv[:, k]]] = 1
        near[k, wg[fn[:, k]]] = 1
        m = np.nonzero(f1[:, k])[0]                     # μddn of these cells reads f at the neighbours
        for dm in (-1, 1, -nx, nx):
            mm = m + dm
            mm = mm[(mm >= 0) & (mm < sz)]
            needf[k, mm // WG] = 1
        if D == 3 and m.size:
            for kk in (k - 1, k + 1):
                if 0 <= kk < nz:
                    needf[kk, m // WG] = 1
    return near, needf, m0var


def census(mu0, mu1, V):
    """the names wl_sim_counter reports after a refresh, from the fields alone"""
    near, needf, m0var = masks(mu0, mu1, V)
    nz, nb = near.shape
    ks, bs = np.nonzero(near)
    box = (int(bs.min()), int(bs.max()), int(ks.min()), int(ks.max())) if ks.size else (nb, -1, nz, -1)      # body_masks_box
    dirty = np.nonzero((near | needf | m0var).any(1))[0]
    dz = (int(dirty.min()), int(dirty.max())) if dirty.size else (nz, -1)                                     # body_masks_planes
    inbox = near[box[2]:box[3] + 1, box[0]:box[1] + 1] if ks.size else near[:0]
    return {"mask_near": int(near.sum()),
            "mask_needf_only": int((needf & (1 - near)).sum()),
            "mask_m0var_only": int((m0var & (1 - near) & (1 - needf)).sum()),
            "mask_clean_in_box": int((inbox == 0).sum()),
            "dirty_z0": dz[0], "dirty_z1": dz[1], "near_b0": box[0], "near_b1": box[1], "near_k0": box[2], "near_k1": box[3]}


CENSUS_NAMES = ("mask_near", "mask_needf_only", "mask_m0var_only", "mask_clean_in_box", "dirty_z0", "dirty_z1", "near_b0", "near_b1", "near_k0", "near_k1")


def tile_ranges(c, Ng, perdir=(), store_f=False):
    """conv_diff_bdim_body on a single 3-D domain with the tiled kernel's size gate at 0: the gather range [na, nb) and the number of tiled
    far-range launches per call.  A far range under 8 planes joins the gather range; nothing is tiled when every plane is in it."""
    if len(Ng) != 3 or store_f or perdir or c["dirty_z1"] < c["dirty_z0"] or Ng[0] < 34 or Ng[1] < 18:
        return None, None, 0
    k0, k1 = 1, Ng[2] - 1
    na, nb = max(c["dirty_z0"], k0), min(c["dirty_z1"] + 1, k1)
    if na - k0 < 8:
        na = k0
    if k1 - nb < 8:
        nb = k1
    if (na - k0) + (k1 - nb) == 0 or nb <= na:
        return na, nb, 0
    return na, nb, int(na > k0) + int(k1 > nb)


def zsplit_plan(mu0, perdir=()):
    """wl_mg::update on the finest level with the z-split's size gate at 0: (part, za, zb).  The constants are sampled at Julia cell (3,3,3);
    planes za..zb hold a coefficient off the pattern; the split is taken when the pair kernels take the level (even nx ≥ 34, ny ≥ 34, 8 planes) and at least 16
    planes and a quarter of all are 4 planes away.  tests/bodyshapes.py zsplit_plan_level is the same on any level."""
    D = mu0.shape[-1]
    Ng = mu0.shape[:-1]
    if D != 3 or perdir or Ng[0] < 34 or Ng[0] % 2 or Ng[1] < 34 or Ng[2] - 2 < 8:      # gsrb_fused_ok && gsrb_pair_geom_ok: even nx ≥ 34, ny ≥ 34, 8 planes
        return False, Ng[-1], -1
    c = mu0[2, 2, 2, :]
    pat = wall_pattern(Ng) * c
    bad = np.nonzero((mu0 != pat).any((0, 1, 3)))[0]
    if bad.size == 0 or c[0] == 0:
        return False, Ng[2], -1
    za, zb = int(bad.min()), int(bad.max())
    k0, k1 = 1, Ng[2] - 1
    na, nb = max(k0, za - 4), min(k1, zb + 5)
    far = (na - k0) + (k1 - nb)
    return bool(far >= 16 and far * 4 >= k1 - k0), za, zb


# ---- the geometry matrix shared by tests/test_bodypaths_cpu.py (is the class really there?) and tests/test_gpu_bodypaths.py (same bits?) ----
# a body: a closed-form tuple of FusedSimulation.measure_body_, or ("union" | "intersect", body, body) for bodies.Body set expressions
BASE = (64, 32, 48)      # with ghosts 66 × 34 × 50: the smallest shape the pair kernels and the tiled conv_diff! take; 2244 cells = 8.8 workgroups per plane


def sphere(c, R=5.0, V=None):
    return ("sphere", tuple(float(v) for v in c), float(R)) + ((tuple(V),) if V is not None else ())


def floor(y, D=3):
    return ("plane", (0.0, float(y), 0.0)[:D], (0.0, 1.0, 0.0)[:D])


ZSLAB = ("plane", (0.0, 0.0, 12.0), (0.0, 0.0, 1.0))                                               # solid below z = 12
ZPLATE = ("intersect", ("plane", (0.0, 0.0, 30.0), (0.0, 0.0, 1.0)), ("plane", (0.0, 0.0, 20.0), (0.0, 0.0, -1.0)))      # solid for 20 < z < 30
TWINS = (("union", sphere((20, 10, 24)), sphere((44, 22, 50))), ("union", sphere((24, 20, 22)), sphere((40, 11, 52))))
TWINS_DIMS = (64, 32, 80)      # two bodies 26 planes apart and still 16 far planes: the z-split needs a taller box than BASE

# what a geometry is there for, as predicates on (census, Ng, tile_ranges, zsplit_plan)
CONDS = {
    "m0var_only": lambda c, Ng, tr, zp: c["mask_m0var_only"] >= 2,                   # workgroups wholly inside the solid: μ₀ = 0 off the wall pattern, μ₁ ≡ 0, V ≡ 0
    "needf_only": lambda c, Ng, tr, zp: c["mask_needf_only"] >= 1,                   # f kept only because a neighbouring workgroup is near
    "all_dirty": lambda c, Ng, tr, zp: c["dirty_z1"] - c["dirty_z0"] + 1 == Ng[-1] and tr[2] == 0 and not zp[0],
    "clean_in_box": lambda c, Ng, tr, zp: c["mask_clean_in_box"] > 0,
    "clean_planes": lambda c, Ng, tr, zp: c["_clean_planes"] > 0,                    # planes inside dirty_z on which no workgroup is marked
    "tile1": lambda c, Ng, tr, zp: tr[2] == 1,
    "tile2": lambda c, Ng, tr, zp: tr[2] == 2,
    "no_tile": lambda c, Ng, tr, zp: tr[2] == 0,
    "part": lambda c, Ng, tr, zp: zp[0],
    "no_part": lambda c, Ng, tr, zp: not zp[0],
    "short_low": lambda c, Ng, tr, zp: 1 <= c["dirty_z0"] - 1 <= 7 and tr[0] == 1,                          # a far range of 1..7 planes joins the gather range
    "short_high": lambda c, Ng, tr, zp: 1 <= (Ng[2] - 1) - (c["dirty_z1"] + 1) <= 7 and tr[1] == Ng[2] - 1,
    "near_ghost_low": lambda c, Ng, tr, zp: c["near_k0"] == 0,                       # near workgroups on a ghost plane: k_bdim_u_m returns early for k < k0
    "near_ghost_high": lambda c, Ng, tr, zp: c["near_k1"] == Ng[2] - 1,
    "near_every_plane": lambda c, Ng, tr, zp: c["near_k0"] <= 1 and c["near_k1"] >= Ng[2] - 2,
    "last_wg": lambda c, Ng, tr, zp: (Ng[0] * Ng[1]) % WG != 0 and c["_last_wg_marked"] > 0,      # the body reaches the last, partial workgroup of a plane
    "last_wg_near": lambda c, Ng, tr, zp: (Ng[0] * Ng[1]) % WG != 0 and c["_last_wg_near"] > 0,
    "v_cells": lambda c, Ng, tr, zp: c["_v_cells"] > 0,
    "empty": lambda c, Ng, tr, zp: c["mask_near"] == 0 and c["near_k1"] < c["near_k0"] and c["dirty_z1"] < c["dirty_z0"] and c["mask_m0var_only"] == 0,
    "body": lambda c, Ng, tr, zp: c["mask_near"] > 0,
}


def census_plus(mu0, mu1, V):
    """census + what only the conditions above look at (keys with a leading underscore: not library counters)"""
    c = census(mu0, mu1, V)
    near, needf, m0var = masks(mu0, mu1, V)
    anyw = near | needf | m0var
    marked = anyw.any(1)
    c["_clean_planes"] = int((~marked[c["dirty_z0"]:c["dirty_z1"] + 1]).sum()) if c["dirty_z1"] >= c["dirty_z0"] else 0
    last = (mu0.shape[0] * mu0.shape[1] + WG - 1) // WG - 1
    c["_last_wg_marked"] = int(anyw[:, last].sum()); c["_last_wg_near"] = int(near[:, last].sum())
    c["_v_cells"] = int((V != 0).any(-1).sum())
    return c


def _case(id, positions, dims=BASE, **kw):
    d = {"id": id, "dims": tuple(dims), "positions": positions, "perdir": (), "lam": 0, "exitBC": False, "store_f": False, "remeasure_each_step": False}
    d.update(kw)
    return d


MOVING_V = (0.25, -0.125, 0.25)
_DEEPFLOOR = [(floor(20.0), ("m0var_only", "needf_only", "all_dirty")), (floor(14.5), ("m0var_only", "needf_only", "all_dirty"))]
_TWINS = [(TWINS[0], ("clean_in_box", "clean_planes", "tile2", "part")), (TWINS[1], ("clean_in_box", "clean_planes", "tile2", "part"))]
CASES = [
    _case("deepfloor", _DEEPFLOOR),
    _case("zslab", [(ZSLAB, ("m0var_only", "tile1", "no_part")), (ZPLATE, ("m0var_only", "tile2", "part"))]),
    _case("zcyl", [(("cylinder", (20.0, 16.0, 0.0), 5.0, 2), ("near_every_plane", "all_dirty")), (("cylinder", (41.5, 14.0, 0.0), 5.0, 2), ("near_every_plane", "all_dirty"))]),
    _case("twins", _TWINS, dims=TWINS_DIMS),
    _case("nearwalls", [(sphere((20, 16, 12)), ("short_low", "tile1", "body")), (sphere((23.5, 15, 36)), ("short_high", "tile1", "body")),
                        (sphere((20, 16, 2), V=(0.25, 0.0, 0.0)), ("near_ghost_low", "tile1", "v_cells")),
                        (sphere((20, 16, 46.5), V=(0.25, 0.0, 0.0)), ("near_ghost_high", "tile1", "v_cells")),
                        (("union", sphere((20, 16, 12)), sphere((40, 14, 36))), ("short_low", "short_high", "no_tile", "clean_planes"))]),
    _case("ycut", [(sphere((55, 39, 24)), ("last_wg", "tile2")), (sphere((58, 40.5, 20), V=(0.25, 0.0, 0.0)), ("last_wg_near", "v_cells"))], dims=(72, 40, 48)),
    # a translating sphere, measured again before every step at its position then; afterwards wholly outside the domain
    _case("moving", [(sphere((20, 16, 24), V=MOVING_V), ("v_cells", "tile2", "part")), (sphere((-60, 16, 24), V=MOVING_V), ("empty",))], remeasure_each_step=True),
    _case("empty-unmeasured", [(None, ("empty",))]),
    _case("empty-outside", [(sphere((-60, 16, 24)), ("empty",)), (sphere((20, 16, 140)), ("empty",))]),
    _case("periodic-x", [(sphere((4, 16, 24)), ("body",)), (sphere((61, 14, 20)), ("body",))], perdir=(1,)),
    _case("periodic-z", [(sphere((20, 16, 44)), ("body",)), (sphere((24, 15, 3.5)), ("body",))], perdir=(3,)),
    _case("periodic-yz", [(sphere((30, 28, 5)), ("body",)), (sphere((34, 3, 44)), ("body",))], perdir=(2, 3)),
    _case("deepfloor-vanleer", _DEEPFLOOR, lam=1), _case("deepfloor-cds", _DEEPFLOOR, lam=2),
    _case("twins-vanleer", _TWINS, dims=TWINS_DIMS, lam=1), _case("twins-cds", _TWINS, dims=TWINS_DIMS, lam=2),
    _case("deepfloor-exit", _DEEPFLOOR, exitBC=True), _case("twins-exit", _TWINS, dims=TWINS_DIMS, exitBC=True),
    _case("twins-store_f", [(TWINS[0], ("clean_in_box", "clean_planes", "part")), (TWINS[1], ("clean_in_box", "clean_planes", "part"))], dims=TWINS_DIMS, store_f=True),
    # 2-D, 66 × 50 with ghosts = 12.9 workgroups: every <2> instantiation of the mask kernels
    _case("circle2d", [(sphere((20, 24), 6.0), ("body",)), (sphere((41.5, 20), 6.0), ("body",))], dims=(64, 48)),
    _case("deepfloor2d", [(floor(26.0, 2), ("m0var_only", "needf_only")), (floor(17.5, 2), ("m0var_only", "needf_only"))], dims=(64, 48)),
    _case("twins2d", [(("union", sphere((14, 8), 4.0), sphere((50, 40), 4.0)), ("clean_in_box",)), (("union", sphere((16, 38), 4.0), sphere((48, 10), 4.0)), ("clean_in_box",))], dims=(64, 48)),
]


def moving_position(body, t):
    """a translating closed-form body at time t"""
    if len(body) == 4 and body[0] == "sphere":
        return sphere(tuple(c + v * t for c, v in zip(body[1], body[3])), body[2], body[3])
    return body


def is_set(body):
    return body is not None and body[0] in ("union", "intersect")


def to_body(body):
    """the device-side description: the tuple itself, or a bodies.Body set expression"""
    if not is_set(body):
        return body
    from waterlily_jl_amd.bodies import Body
    leaf = lambda b: to_body(b) if is_set(b) else Body(b)
    a, b = leaf(body[1]), leaf(body[2])
    return (a | b) if body[0] == "union" else (a & b)
