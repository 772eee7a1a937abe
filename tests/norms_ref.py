"""Reference for the three scalars that steer a time step (test infrastructure; plain NumPy / math, imports without a GPU): r₁ and r∞ of solver!'s log and
Δt from CFL's maximum, each as a float64 sum or a float32 maximum over the field the same call left behind — and the map from an array index to the places
where a reducing kernel can lose or double a cell (cell_classes), restated from the tile geometry of the pair smoother.

Bounds (derived, not measured).  r∞ and max σ are maxima of float32 values: no order of evaluation changes them, the comparison is on raw bits.  r₁ is a
float64 accumulation of n float32 terms in some order (per thread, per wave, per workgroup, the finaliser), and the log keeps it rounded once to float32: the
float64 accumulation is off by at most (n−1)·2⁻⁵³·Σ|r| whatever the order, the rounding by 2⁻²⁴ of the sum:
    |logged − l1(r)| ≤ l1(r)·(2⁻²⁴ + n·2⁻⁵³),   n = number of array cells.
Δt = min(10, 1/(max σ + 5ν)) is evaluated in float32 statement by statement as k_dt_from_cfl and wl_sim::cfl's host line write it (csrc/wl_sim.hip), from the
maximum over ALL cells of σ, ghost cells included (quirk Q1: σ's upper ghost cells keep conv_diff!'s stale Φ)."""
import math

import numpy as np

f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------------------ scalars
def l1(r):
    """Σ|r| over the whole array, exactly rounded (ghost cells of r are zero by construction: the reference's sum(abs, r) runs over the parent array too)"""
    return math.fsum(np.abs(np.asarray(r, dtype=np.float64)).ravel(order="K").tolist())


def linf(r):
    """max|r| as a float32"""
    return f32(np.abs(np.asarray(r, dtype=f32)).max())


def r1_bound(ref, ncells):
    return ref * (2.0 ** -24 + ncells * 2.0 ** -53)


def r1_err(logged, r):
    """(|logged − l1(r)|, the bound): the caller prints both and asserts err <= bound"""
    ref = l1(r)
    return abs(float(logged) - ref), r1_bound(ref, np.asarray(r).size)


def bits(v):
    """a float32 scalar as its 32 bits"""
    return int(np.asarray(v, dtype=f32).reshape(1).view(np.uint32)[0])


def dt_from_sigma(sigma, nu):
    """fminf(10.f, 1.0f / (mx + 5 * nu)) with mx = max over every cell of σ"""
    mx = f32(np.asarray(sigma, dtype=f32).max())
    five_nu = f32(f32(5) * f32(nu))
    den = f32(mx + five_nu)
    with np.errstate(divide="ignore"):
        q = f32(f32(1) / den)
    return f32(min(f32(10), q))


# ------------------------------------------------------------------------------------------------------------------------ tile geometry
CORE_X = 56                          # ptile<4,3>: 2·32 − 2·4 cells of a tile's core along x (kernel B, the one that reduces)
CORE_Y = {16: 10, 32: 26}            # PT_Y − 2·3 rows
SEG_X = 60                           # ptile<2,2>: kernel A's core columns = the segments of the exchange buffer W


def rows_of(shape):
    """rows16() of csrc/wl_fused2.hip: 16-row tiles unless the plane has at least 128 tiles of 56×26 cells"""
    nx, ny = shape[0], shape[1]
    return 16 if ((nx + 55) // 56) * ((ny + 25) // 26) < 128 else 32


def tile_counts(shape, rows=None, kernel="B"):
    """(ntx, nty) of ptile<4,3> (kernel B) or ptile<2,2> (kernel A) — ptile_count's two factors"""
    rows = rows or rows_of(shape)
    hx, hy = (4, 3) if kernel == "B" else (2, 2)
    cx, cy = 64 - 2 * hx, rows - 2 * hy
    return (shape[0] - 1 + cx - 1) // cx, (shape[1] - 2 + cy - 1) // cy


def zchunk2(shape, nplanes, rows=None, kernel="B"):
    """the planes per z-chunk of a launch over `nplanes` output planes (zchunk2 of csrc/wl_fused2_body.inc, its cost model with no experiment variable set)"""
    rows = rows or rows_of(shape)
    ntx, nty = tile_counts(shape, rows, kernel)
    nt = ntx * nty
    warm = (5 if kernel == "B" else 3) + 3
    per, sx = (nt + 7) >> 3, 32 * (1024 // (32 * rows))
    best, best_zc = -1.0, nplanes
    for chunks in range(1, nplanes + 1):
        zc = (nplanes + chunks - 1) // chunks
        if zc < 4:
            break
        nch = (nplanes + zc - 1) // zc
        wgs = per * nch
        rounds = (wgs + sx - 1) // sx
        cost = float(rounds) * (zc + warm) * (1.0 + 0.3 / float(rounds))
        if wgs < sx:
            cost = (zc + warm) * 1.3
        if best < 0 or cost < best:
            best, best_zc = cost, zc
    return best_zc


def workgroups(shape, nplanes, rows=None):
    """(workgroups launched, workgroups without a tile) of kernel B: 8·ceil(tiles/8) per z-chunk — the dead ones write a zero partial"""
    ntx, nty = tile_counts(shape, rows)
    nt = ntx * nty
    zc = zchunk2(shape, nplanes, rows)
    nch = (nplanes + zc - 1) // zc
    per = (nt + 7) >> 3
    return 8 * per * nch, (8 * per - nt) * nch


R_CLASSES = ("row_first", "row_last", "pair_even", "pair_odd", "xseam_lo", "xseam_hi", "yseam_lo", "yseam_hi", "ragged_col", "ragged_row", "last_tile",
             "plane_first", "plane_last", "zseam_lo", "zseam_hi")
GHOST_FACES = ("ghost_x0", "ghost_x1", "ghost_y0", "ghost_y1", "ghost_z0", "ghost_z1")


class CellClasses:
    """cell_classes(shape, kind): .mask[name] is a boolean array over the array's cells, .of(index) the names an index belongs to, .names those that are not
    empty at this shape.  Indices are 0-based with ghost cells.  Every class but the ghost ones holds interior cells only."""

    def __init__(self, shape, kind="r", rows=None, zranges=None):
        assert kind in ("r", "sigma"), kind
        self.shape, self.kind = tuple(shape), kind
        D = len(shape)
        nx, ny = shape[0], shape[1]
        nz = shape[2] if D == 3 else 1
        self.rows = rows or rows_of(shape)
        cy = CORE_Y[self.rows]
        self.ntx, self.nty = tile_counts(shape, self.rows)
        ix = np.arange(nx).reshape((nx,) + (1,) * (D - 1))
        jy = np.arange(ny).reshape((1, ny) + (1,) * (D - 2))
        inter = (ix >= 1) & (ix <= nx - 2) & (jy >= 1) & (jy <= ny - 2)
        if D == 3:
            kz = np.arange(nz).reshape((1, 1, nz))
            inter = inter & (kz >= 1) & (kz <= nz - 2)
        full = lambda m: np.broadcast_to(m, self.shape) & inter
        tx, ty = ix // CORE_X, (jy - 1) // cy
        m = {}
        m["row_first"], m["row_last"] = full(ix == 1), full(ix == nx - 2)
        m["pair_even"], m["pair_odd"] = full(ix % 2 == 0), full(ix % 2 == 1)                         # the pair of a thread: columns (i0, i0+1), i0 even
        m["xseam_lo"] = full((ix % CORE_X == CORE_X - 1) & (ix + 1 <= nx - 2))                       # last core column of a tile, a tile to its right
        m["xseam_hi"] = full((ix % CORE_X == 0) & (ix >= CORE_X))
        m["yseam_lo"] = full(((jy - 1) % cy == cy - 1) & (jy + 1 <= ny - 2))
        m["yseam_hi"] = full(((jy - 1) % cy == 0) & (jy > 1))
        m["ragged_col"] = full((tx == self.ntx - 1) & ((nx - 1) % CORE_X != 0))                      # the last tile column holds fewer than 56 columns
        m["ragged_row"] = full((ty == self.nty - 1) & ((ny - 2) % cy != 0))
        nt = self.ntx * self.nty
        m["last_tile"] = full((ty * self.ntx + tx == nt - 1) & (nt % 8 != 0))                        # … of all, with dead workgroups behind it
        if D == 3:
            m["plane_first"], m["plane_last"] = full(kz == 1), full(kz == nz - 2)
            self.zranges = list(zranges) if zranges else [(1, nz - 1)]                               # plane ranges [a, b) of separate launches (the z-split: three)
            lo, hi = np.zeros(nz, dtype=bool), np.zeros(nz, dtype=bool)
            self.zchunks = []
            for a, b in self.zranges:
                if b <= a:
                    continue
                zc = zchunk2(shape, b - a, self.rows)
                self.zchunks.append(zc)
                for k in range(a, b):
                    if (k - a) % zc == zc - 1 and k + 1 < b:
                        lo[k] = True
                    if (k - a) % zc == 0 and k > a:
                        hi[k] = True
                if a > 1:
                    hi[a], lo[a - 1] = True, True                                                    # the cut between two ranges is a seam too
            m["zseam_lo"], m["zseam_hi"] = full(lo.reshape(1, 1, nz)), full(hi.reshape(1, 1, nz))
        if kind == "sigma":
            g = ~np.broadcast_to(inter, self.shape)
            m["ghost"] = g
            m["ghost_x0"], m["ghost_x1"] = np.broadcast_to(ix == 0, self.shape), np.broadcast_to(ix == nx - 1, self.shape)
            m["ghost_y0"], m["ghost_y1"] = np.broadcast_to(jy == 0, self.shape), np.broadcast_to(jy == ny - 1, self.shape)
            if D == 3:
                m["ghost_z0"], m["ghost_z1"] = np.broadcast_to(kz == 0, self.shape), np.broadcast_to(kz == nz - 1, self.shape)
        self.mask = m
        self.names = tuple(n for n in m if m[n].any())

    def of(self, index):
        index = tuple(int(v) for v in index)
        return frozenset(n for n in self.names if self.mask[n][index])


def cell_classes(shape, kind="r", rows=None, zranges=None):
    return CellClasses(shape, kind, rows, zranges)


# ------------------------------------------------------------------------------------------------------------------------------- the cases
def base_rhs(shape):
    """_rhs of tests/test_gpu_mg_paths.py (every wavelength, no mean inside), scaled down so that one spike on top of it owns the maximum"""
    from test_gpu_mg_paths import _rhs
    return (_rhs(tuple(shape)) * f32(RHS_SCALE)).astype(f32)


RHS_SCALE = 0.01
SPIKE = 1.0


def rhs_with_spike(shape, spike, amp=SPIKE):
    z = np.asfortranarray(base_rhs(shape))
    z[tuple(spike)] += f32(amp)
    return z


# the handles of tests/test_gpu_norms.py: the smallest shapes (with ghost cells) at which each tiling exists.  tiling: whose geometry the classes are judged by
# (None: passes — only the classes no tiling defines); zsplit: coefficients off the constant pattern on planes 16 and 17, so that the smoother runs on the plane
# ranges [1,12), [12,22), [22,33) (wl_mg::zsplit_ranges: ZSPLIT_MARGIN = 4 planes around the deviating ones)
GENERIC = ("row_first", "row_last", "pair_even", "pair_odd", "plane_first", "plane_last")
ZSPLIT_PLANES = (16, 18)
ZSPLIT_RANGES = ((1, 12), (12, 22), (22, 33))
SHAPES = {
    "66x34x26": dict(shape=(66, 34, 26), perdir=(), tiling="r16", zranges=None),
    "62x34x12": dict(shape=(62, 34, 12), perdir=(), tiling="r16", zranges=None),
    "66x66x18": dict(shape=(66, 66, 18), perdir=(), tiling="r16", zranges=None),
    "450x370x10": dict(shape=(450, 370, 10), perdir=(), tiling="r32", zranges=None),
    "66x34x34-zsplit": dict(shape=(66, 34, 34), perdir=(), tiling="zsplit", zranges=ZSPLIT_RANGES),
    "66x34x34-periodic": dict(shape=(66, 34, 34), perdir=(1,), tiling=None, zranges=None),
    "34x34": dict(shape=(34, 34), perdir=(), tiling=None, zranges=None),
    "130x18": dict(shape=(130, 18), perdir=(), tiling=None, zranges=None),
}
SEED = 5


def classes_of(sid):
    """the classes a case of this handle may be listed for"""
    e = SHAPES[sid]
    cc = cell_classes(e["shape"], "r", zranges=e["zranges"])
    want = R_CLASSES if e["tiling"] else GENERIC
    return cc, tuple(n for n in want if n in cc.names)


def zsplit_coefficients(L):
    """the face coefficients of the z-split handle before BC!: μ₀ = ½ in a box of the two middle planes (_zsplit_sim of tests/test_gpu_mg_paths.py)"""
    L[20:40, 10:20, ZSPLIT_PLANES[0]:ZSPLIT_PLANES[1], :] = 0.5


def candidates(shape, cls, seed, rows=None, zranges=None, count=12):
    """the cells of class `cls` in the order a case is searched for: drawn with `seed`, away from nothing — the class decides, the oracle judges"""
    cc = cell_classes(shape, "r", rows, zranges)
    idx = np.argwhere(cc.mask[cls])
    rng = np.random.default_rng([int(seed), R_CLASSES.index(cls)] + [int(n) for n in shape])
    pick = rng.choice(len(idx), size=min(count, len(idx)), replace=False)
    return [tuple(int(v) for v in idx[q]) for q in pick]


# (handle, the class searched for, index into candidates() of the first cell the oracle accepted, that cell = where the spike goes, iteration cap k,
#  the oracle's arg-max of |r|, every class the arg-max holds with the 1 % margin).  A class already held by an earlier case of the handle is not searched again.
# tests/test_norms_cpu.py judges every row with the oracle and holds the table to candidates(…, SEED).
CASES = (
    ('66x34x26', 'row_first', 0, (1, 21, 21), 1, (1, 20, 20), ('pair_odd', 'row_first', 'yseam_lo', 'zseam_lo')),
    ('66x34x26', 'row_last', 1, (64, 31, 9), 1, (64, 31, 8), ('pair_even', 'ragged_col', 'ragged_row', 'row_last', 'yseam_hi', 'zseam_lo')),
    ('66x34x26', 'xseam_lo', 1, (55, 21, 14), 2, (55, 21, 15), ('pair_odd', 'xseam_lo', 'yseam_hi')),
    ('66x34x26', 'xseam_hi', 0, (56, 27, 17), 2, (56, 26, 17), ('pair_even', 'ragged_col', 'xseam_hi', 'zseam_hi')),
    ('66x34x26', 'plane_first', 0, (37, 27, 1), 1, (36, 26, 1), ('pair_even', 'plane_first')),
    ('66x34x26', 'plane_last', 1, (46, 10, 24), 1, (47, 10, 24), ('pair_odd', 'plane_last', 'yseam_lo')),
    ('62x34x12', 'row_first', 0, (1, 26, 3), 1, (1, 26, 2), ('pair_odd', 'row_first')),
    ('62x34x12', 'row_last', 1, (60, 29, 3), 1, (60, 28, 3), ('pair_even', 'ragged_col', 'row_last')),
    ('62x34x12', 'xseam_lo', 0, (55, 12, 1), 1, (55, 13, 1), ('pair_odd', 'plane_first', 'xseam_lo')),
    ('62x34x12', 'xseam_hi', 0, (56, 3, 10), 2, (56, 3, 10), ('pair_even', 'plane_last', 'ragged_col', 'xseam_hi')),
    ('62x34x12', 'yseam_lo', 1, (24, 20, 8), 2, (24, 20, 9), ('pair_even', 'yseam_lo', 'zseam_hi')),
    ('62x34x12', 'yseam_hi', 3, (23, 31, 5), 1, (22, 31, 4), ('pair_even', 'ragged_row', 'yseam_hi', 'zseam_lo')),
    ('66x66x18', 'row_first', 0, (1, 18, 3), 1, (1, 19, 3), ('pair_odd', 'row_first')),
    ('66x66x18', 'row_last', 0, (64, 58, 9), 2, (64, 58, 9), ('pair_even', 'ragged_col', 'row_last', 'zseam_hi')),
    ('66x66x18', 'xseam_lo', 1, (55, 38, 2), 2, (55, 38, 2), ('pair_odd', 'xseam_lo')),
    ('66x66x18', 'xseam_hi', 0, (56, 58, 1), 2, (56, 58, 1), ('pair_even', 'plane_first', 'ragged_col', 'xseam_hi')),
    ('66x66x18', 'yseam_lo', 0, (59, 20, 12), 1, (58, 20, 13), ('pair_even', 'ragged_col', 'yseam_lo', 'zseam_hi')),
    ('66x66x18', 'yseam_hi', 0, (23, 41, 11), 2, (23, 41, 11), ('pair_odd', 'yseam_hi')),
    ('66x66x18', 'ragged_row', 0, (36, 61, 10), 2, (36, 61, 10), ('pair_even', 'ragged_row', 'yseam_hi')),
    ('66x66x18', 'last_tile', 0, (59, 63, 9), 1, (58, 63, 8), ('last_tile', 'pair_even', 'ragged_col', 'ragged_row', 'zseam_lo')),
    ('66x66x18', 'plane_last', 0, (60, 48, 16), 1, (60, 49, 16), ('plane_last', 'ragged_col')),
    ('450x370x10', 'row_first', 0, (1, 222, 2), 1, (1, 223, 3), ('pair_odd', 'row_first')),
    ('450x370x10', 'row_last', 1, (448, 337, 5), 1, (448, 337, 4), ('pair_even', 'ragged_col', 'row_last', 'xseam_hi')),
    ('450x370x10', 'xseam_lo', 1, (335, 63, 8), 2, (335, 62, 6), ('pair_odd', 'xseam_lo')),
    ('450x370x10', 'yseam_lo', 1, (209, 364, 3), 2, (209, 364, 2), ('pair_odd', 'yseam_lo')),
    ('450x370x10', 'yseam_hi', 0, (401, 131, 3), 2, (401, 131, 3), ('pair_odd', 'yseam_hi')),
    ('450x370x10', 'ragged_row', 0, (403, 367, 6), 2, (403, 367, 7), ('pair_odd', 'ragged_row')),
    ('450x370x10', 'last_tile', 0, (448, 367, 1), 1, (448, 366, 1), ('last_tile', 'pair_even', 'plane_first', 'ragged_col', 'ragged_row', 'row_last', 'xseam_hi')),
    ('450x370x10', 'plane_last', 0, (105, 106, 8), 1, (104, 107, 8), ('pair_even', 'plane_last')),
    ('66x34x34-zsplit', 'row_first', 0, (1, 3, 13), 1, (1, 2, 12), ('pair_odd', 'row_first', 'zseam_hi')),
    ('66x34x34-zsplit', 'row_last', 0, (64, 20, 29), 2, (64, 20, 29), ('pair_even', 'ragged_col', 'row_last', 'yseam_lo', 'zseam_lo')),
    ('66x34x34-zsplit', 'xseam_lo', 0, (55, 9, 13), 1, (55, 8, 12), ('pair_odd', 'xseam_lo', 'zseam_hi')),
    ('66x34x34-zsplit', 'xseam_hi', 0, (56, 23, 5), 2, (56, 22, 5), ('pair_even', 'ragged_col', 'xseam_hi', 'zseam_hi')),
    ('66x34x34-zsplit', 'yseam_hi', 0, (62, 11, 2), 2, (62, 11, 2), ('pair_even', 'ragged_col', 'yseam_hi')),
    ('66x34x34-zsplit', 'ragged_row', 0, (26, 31, 6), 2, (26, 31, 6), ('pair_even', 'ragged_row', 'yseam_hi')),
    ('66x34x34-zsplit', 'plane_first', 0, (29, 21, 1), 1, (28, 20, 1), ('pair_even', 'plane_first', 'yseam_lo')),
    ('66x34x34-zsplit', 'plane_last', 1, (3, 11, 32), 1, (3, 10, 32), ('pair_odd', 'plane_last', 'yseam_lo')),
    ('66x34x34-periodic', 'row_first', 1, (1, 30, 11), 2, (1, 30, 11), ('pair_odd', 'row_first')),
    ('66x34x34-periodic', 'row_last', 0, (64, 20, 29), 2, (64, 20, 29), ('pair_even', 'row_last')),
    ('66x34x34-periodic', 'plane_first', 0, (29, 21, 1), 1, (28, 20, 1), ('pair_even', 'plane_first')),
    ('66x34x34-periodic', 'plane_last', 1, (3, 11, 32), 1, (2, 11, 32), ('plane_last',)),
    ('34x34', 'row_first', 1, (1, 25), 2, (1, 21), ('pair_odd', 'row_first')),
    ('34x34', 'row_last', 0, (32, 12), 2, (32, 16), ('pair_even', 'row_last')),
    ('130x18', 'row_first', 1, (1, 15), 2, (1, 11), ('pair_odd', 'row_first')),
    ('130x18', 'row_last', 3, (128, 4), 1, (128, 6), ('pair_even', 'row_last')),
)


# ------------------------------------------------------------------------------------------------------------------------------ σ and Δt
SIGMA_NU = 0.02
SIGMA_WANT = ("row_first", "row_last", "xseam_lo", "xseam_hi", "yseam_lo", "yseam_hi", "ragged_col", "ragged_row", "last_tile", "plane_first", "plane_last",
              "zseam_lo", "zseam_hi")


def stream_and_jets(dims, ubc, jets, bc):
    """u of a σ case: the uniform stream `ubc` plus `jets` = ((cell, component, amplitude), …), then BC! (bc(u, ubc): the oracle's)"""
    u = np.zeros(tuple(n + 2 for n in dims) + (len(dims),), dtype=f32, order="F")
    for c in range(len(dims)):
        u[..., c] = f32(ubc[c])
    for cell, c, a in jets:
        u[tuple(cell) + (c,)] += f32(a)
    bc(u, ubc)
    return u


# (interior dims, U, jets, the class searched for, index into candidates() (−1: placed by hand), the oracle's arg-max of σ after one step, the classes it holds
# with the 1 % margin).  The interior classes are those of the array's shape under cell_classes(…, "sigma"); a jet in the wall-normal component of a wall
# face is overwritten by BC!, hence the tangential jets of the row_first cases.
# The ghost cells: σ's UPPER ghost cells keep conv_diff!'s stale Φ of the corrector (the last flux written there: U_normal·u_tangential), the lower ones stay 0
# and cannot hold a maximum.  A jet of amplitude 8 in a tangential component beside the upper wall puts the oracle's maximum(σ) on the ghost cell behind it
# (amplitudes 1, 2, 4 leave it inside; 8 to 64 were tried and all stayed finite): x-face with U = (0.3, −0.2, 0.1), y- and z-face with U = (1.5, 1.5, 1.5).
SIGMA_CASES = (
    ((64, 32, 24), (0.3, -0.2, 0.1), (((1, 12, 5), 1, 2.0),), 'row_first', 0, (1, 12, 5), ('row_first',)),
    ((64, 32, 24), (0.3, -0.2, 0.1), (((64, 8, 22), 1, 2.0),), 'row_last', 0, (64, 7, 22), ('ragged_col', 'row_last')),
    ((64, 32, 24), (0.3, -0.2, 0.1), (((55, 10, 4), 2, 2.0),), 'xseam_lo', 0, (55, 10, 4), ('xseam_lo', 'yseam_lo', 'zseam_lo')),
    ((64, 32, 24), (0.3, -0.2, 0.1), (((56, 20, 16), 0, 2.0),), 'xseam_hi', 1, (56, 20, 16), ('ragged_col', 'xseam_hi', 'yseam_lo', 'zseam_lo')),
    ((64, 32, 24), (0.3, -0.2, 0.1), (((29, 31, 5), 2, 2.0),), 'yseam_hi', 0, (29, 31, 5), ('ragged_row', 'yseam_hi', 'zseam_hi')),
    ((64, 32, 24), (0.3, -0.2, 0.1), (((37, 30, 1), 0, 2.0),), 'plane_first', 0, (37, 30, 1), ('plane_first', 'yseam_lo')),
    ((64, 32, 24), (0.3, -0.2, 0.1), (((17, 30, 24), 1, 2.0),), 'plane_last', 0, (17, 29, 24), ('plane_last',)),
    ((448, 368, 8), (0.3, -0.2, 0.1), (((1, 123, 1), 1, 2.0),), 'row_first', 0, (1, 123, 1), ('row_first',)),
    ((448, 368, 8), (0.3, -0.2, 0.1), (((448, 78, 4), 1, 2.0),), 'row_last', 0, (448, 77, 4), ('ragged_col', 'row_last', 'xseam_hi')),
    ((448, 368, 8), (0.3, -0.2, 0.1), (((223, 304, 6), 2, 2.0),), 'xseam_lo', 0, (223, 304, 6), ('xseam_lo',)),
    ((448, 368, 8), (0.3, -0.2, 0.1), (((438, 208, 2), 1, 2.0),), 'yseam_lo', 0, (438, 208, 2), ('yseam_lo',)),
    ((448, 368, 8), (0.3, -0.2, 0.1), (((107, 131, 4), 2, 2.0),), 'yseam_hi', 0, (107, 131, 4), ('yseam_hi',)),
    ((448, 368, 8), (0.3, -0.2, 0.1), (((235, 367, 3), 1, 2.0),), 'ragged_row', 0, (235, 367, 3), ('ragged_row',)),
    ((448, 368, 8), (0.3, -0.2, 0.1), (((448, 367, 2), 2, 2.0),), 'last_tile', 0, (448, 367, 1), ('last_tile', 'plane_first', 'ragged_col', 'ragged_row', 'row_last', 'xseam_hi')),
    ((448, 368, 8), (0.3, -0.2, 0.1), (((223, 174, 8), 1, 2.0),), 'plane_last', 0, (223, 173, 8), ('plane_last', 'xseam_lo')),
    ((64, 32, 24), (0.3, -0.2, 0.1), (((64, 16, 12), 2, 8.0),), 'ghost_x1', -1, (65, 16, 14), ('ghost', 'ghost_x1')),
    ((64, 32, 24), (1.5, 1.5, 1.5), (((30, 32, 12), 0, 8.0),), 'ghost_y1', -1, (30, 33, 12), ('ghost', 'ghost_y1')),
    ((64, 32, 24), (1.5, 1.5, 1.5), (((30, 16, 24), 0, 8.0),), 'ghost_z1', -1, (30, 16, 25), ('ghost', 'ghost_z1')),
    ((448, 368, 8), (0.3, -0.2, 0.1), (((448, 200, 4), 2, 8.0),), 'ghost_x1', -1, (449, 200, 6), ('ghost', 'ghost_x1')),
    # the shape of the z-split handle (the oracle judges it without the μ₀ box) and the 2-D circle of tests/callseq.py's circle2d family (with its body)
    ((64, 32, 32), (0.3, -0.2, 0.1), (((30, 16, 32), 0, 2.0),), 'plane_last', -1, (29, 16, 32), ('plane_last',)),
    ((64, 32, 32), (0.3, -0.2, 0.1), (((64, 16, 1), 1, 2.0),), 'row_last', -1, (64, 15, 1), ('plane_first', 'ragged_col', 'row_last')),
    ((64, 32, 32), (0.3, -0.2, 0.1), (((64, 16, 16), 2, 8.0),), 'ghost_x1', -1, (65, 16, 18), ('ghost', 'ghost_x1')),
    ((64, 48), (1.0, 0.0), (((1, 40), 1, 4.0),), 'row_first', -1, (1, 40), ('row_first', 'yseam_lo')),
    ((64, 48), (1.0, 0.0), (((64, 30), 1, 8.0),), 'ghost_x1', -1, (65, 32), ('ghost', 'ghost_x1')),
)
