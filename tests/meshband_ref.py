"""NumPy restatement of band-limited mesh baking (include/wlhip.h, band-limited baking; csrc/wl_meshsdf.hip k_meshsdf<D, VEL, true>) — the yardstick of
tests/test_meshband_cpu.py and tests/test_gpu_meshband.py.  A banded lattice is the full one, clipped: clip_ref is one np.clip of the restatement that exists
(tests/meshsdf_ref.py, tests/meshvel_ref.py) and the velocity mask; far_bricks restates in Float64 which bricks lie wholly beyond the band by the bounding
spheres — Lb = min_t(|c_b − c_t| − r_t) − r_b above the band plus a slack.  The registry adds two cases with far bricks INSIDE the body to the committed
ones.  No GPU, no library."""
import functools

import numpy as np

import meshsdf_ref as mr
import meshvel_ref as mv

f32, f64 = np.float32, np.float64


def _placed(D, VE, margin=5.5):
    dims, origin = mr.mesh_body_placement(VE[0], 1.0, margin)
    return mr._case(D, VE, dims, origin, 1.0)


NEW = {
    "ico320-R16": lambda: _placed(3, mr.icosphere(2, 16.0, (0.2, -0.1, 0.3))),
    "ellipse2d": lambda: _placed(2, mr.polygon([(26 * np.cos(2 * np.pi * k / 64) + 0.3, 24 * np.sin(2 * np.pi * k / 64) - 0.2) for k in range(64)])),
}
INSIDE = ["ico320-R16", "ellipse2d"]                                     # far bricks on both sides of the surface
BAND = {"ico320-R16": 4.5, "ellipse2d": 4.5}
BAND.update({k: 2.5 for k in ("cube", "lprism", "ico320", "ico1280-centred", "torus", "square", "lpoly", "gon64")})
BAND.update({k: 2.0 * mr.case(k)["spacing"] for k in mr.RAGGED})          # nothing skipped: the per-sample clip alone, on ragged bricks
CASES = list(BAND)
# far bricks (outside, inside) in Float64 with the slack 1e-4·band + 4e-3
FAR = {"ico320-R16": (659, 14), "ellipse2d": (4, 8), "cube": (27, 0), "lprism": (18, 0), "ico320": (133, 0), "ico1280-centred": (32, 0), "torus": (51, 0),
       "cube-11x9x6": (0, 0), "cube-5x3x3": (0, 0), "cube-3x3x3": (0, 0)}


@functools.lru_cache(maxsize=None)
def case(name):
    return NEW[name]() if name in NEW else mr.case(name)


@functools.lru_cache(maxsize=None)
def full_ref(name):
    """the Float32 restatement of the un-banded lattice: d shaped like the lattice"""
    if name in mr.CASES:
        return mr.ref(name, "f32")["d"]
    c = case(name)
    d = mr.sdf_points(c["D"], c["V"], c["E"], mr.sample_positions(c["dims"], c["origin"], c["spacing"]), f32)["d"].reshape(c["dims"], order="F")
    d.setflags(write=False)
    return d


def clip_ref(name, band, Wv=None):
    """A_band = clip(A_full, −b, +b) in Float32 (a clipped sample is exactly ±b); with vertex velocities Wv also W_band = W_full where |A_full| ≤ b, else +0
    -> d, or (d, W)"""
    b = f32(band)
    d = full_ref(name)
    out = np.clip(d, -b, b).astype(f32)
    if Wv is None:
        return out
    c = case(name)
    r = mv.sdf_points(c["D"], c["V"], c["E"], Wv, mr.sample_positions(c["dims"], c["origin"], c["spacing"]), f32)
    W = r["W"].reshape(c["dims"] + (c["D"],), order="F")
    return out, np.where((np.abs(d) <= b)[..., None], W, f32(0)).astype(f32)


def bricks(name):
    """the bricks of a case in the kernel's order (first index fastest): a list of index tuples of slices into the lattice"""
    c = case(name)
    D, dims, ext = c["D"], c["dims"], mr.EXT[c["D"]]
    nb = [-(-dims[d] // ext[d]) for d in range(D)]
    return [tuple(slice(b[d] * ext[d], min(dims[d], (b[d] + 1) * ext[d])) for d in range(D)) for b in (q[::-1] for q in np.ndindex(*nb[::-1]))]


@functools.lru_cache(maxsize=None)
def brick_lower_bounds(name):
    """Lb = min_t(|c_b − c_t| − r_t) − r_b per brick, Float64, without slack (the census of tests/meshsdf_ref.cull_census, extended)"""
    c = case(name)
    D, s, ext = c["D"], c["spacing"], mr.EXT[c["D"]]
    C, R = mr.bounding_spheres(D, c["V"], c["E"])
    rb = s * np.sqrt(sum(((e - 1) / 2) ** 2 for e in ext))
    lb = []
    for sl in bricks(name):
        cb = np.array([c["origin"][d] + s * (sl[d].start + (ext[d] - 1) / 2 - 0.5) for d in range(D)])
        lb.append((np.linalg.norm(C - cb, axis=1) - R).min() - rb)
    lb = np.array(lb)
    lb.setflags(write=False)
    return lb


def far_bricks(name, band, slack_factor=1.0):
    """bool per brick (the kernel's order): Lb > band + slack_factor·(1e-4·band + 4e-3) in Float64.  4e-3 is 1e-4 of the largest coordinate any case
    reaches (below 40), the absolute part of the library's slack (wl_meshsdf.hip meshsdf_run: 1e-4·scale); the kernel adds Float32 rounding of positions
    and distances, below 1e-6 of that coordinate.  So the kernel skips at least the bricks of slack_factor = 2 and at most those of slack_factor = 0."""
    return brick_lower_bounds(name) > band + slack_factor * (1e-4 * band + 4e-3)


def mesh_band(eps=1.0, offset=0.0, spacing=1.0, D=3):
    """bodies.mesh_band's statement"""
    return 2.0 + eps + 1.0 + abs(offset) + spacing * float(np.sqrt(float(D))) + 0.25


def band_rule(band, offset, need, spacing, D):
    """the band rule of include/wlhip.h in Float32, as wl_bodyset.hip states it: band − |R| > need + s·√D"""
    return bool(f32(band) - abs(f32(offset)) > f32(need) + f32(spacing) * np.sqrt(f32(D)))
