"""NumPy Float32 restatement of MeanFlow (the reference's src/Metrics.jl:205-262) as the handle's observer keeps it: the ε and t arithmetic of update!, its three
statements on every cell, the packed index map of UU (components i ≤ j, plane i + j(j+1)/2) with its expansion, uu!, and the shapes and Δt histories the
GPU tests run (tests/test_gpu_meanflow.py), kept here so that tests/test_meanflow_cpu.py can hold them to what they were chosen for."""
import numpy as np

f32 = np.float32
EPS32 = np.finfo(np.float32).eps
BLOCK = 256                    # threads of a workgroup of k_mean_update (WL_BLOCK)
CELLS_PER_THREAD = 4           # the 16-byte form; cs % 4 != 0 takes the one-cell form

# interiors of the kernel-against-restatement cases; with ghosts cs = prod(n + 2).  A handle needs its MultiLevelPoisson, which needs three levels (the reference's
# "size=a2ⁿ, where n>2"): one side with ghosts must halve twice (even and > 4, twice), so cs is EVEN on every handle and cs % 4 is 0 or 2 — the one-cell instance
# that serves every cs % 4 != 0 is reached at 2.  Of the shapes first proposed for this test 5×7, 62×30, 9×7×5 and 14×6×4 (cs = 63, 2048, 693, 768) have no such
# side (NO_HANDLE: creation fails, asserted); 8×5, 8×5×3 and 14×30×8 stand in for them: a one-cell case below one workgroup, one above, and whole workgroups of quads.
SHAPES_2D = [(6, 8), (12, 9), (8, 5)]                              # cs = 80, 154, 70: cs % 4 = 0, 2, 2
SHAPES_3D = [(8, 8, 8), (8, 5, 3), (14, 30, 8), (64, 32, 24)]      # cs = 1000, 350, 5120, 58344: cs % 4 = 0, 2, 0, 0
NO_HANDLE = [(5, 7), (62, 30), (9, 7, 5), (14, 6, 4)]
SHAPES = SHAPES_2D + SHAPES_3D
N_UPDATES = 6
# the Δt the handle is given before each of the steps that separate the updates of a case (wl_sim_set_dt_last): time(flow) is their running Float32 sum
DT_HISTORY = [f32(v) for v in (0.25, 0.125, 0.3, 0.0625, 0.21, 0.17)]


def levels(dims):
    """levels of the MultiLevelPoisson on this interior (src/MultiLevelPoisson.jl:52-74): a side with ghosts is halved while it is even and > 4"""
    n, k = [d + 2 for d in dims], 1
    while any(v % 2 == 0 and v > 4 for v in n):
        n = [1 + v // 2 if (v % 2 == 0 and v > 4) else v for v in n]
        k += 1
    return k


def cells(dims):
    return int(np.prod([n + 2 for n in dims]))


def npk(D):
    return D * (D + 1) // 2


def pk(i, j):
    """plane of component (i, j), 0-based, either order"""
    i, j = (i, j) if i <= j else (j, i)
    return i + j * (j + 1) // 2


def times(dts, t0=f32(0)):
    """time(flow) after each step: the in-order Float32 sum of the Δt history"""
    out, t = [], f32(t0)
    for d in dts:
        t = f32(t + f32(d))
        out.append(t)
    return out


class MeanRef:
    """MeanFlow with UU kept in full, (N…, D, D), as the reference keeps it"""

    def __init__(self, Ng, t_init, uu_stats):
        D = len(Ng)
        self.D = D
        self.P = np.zeros(Ng, dtype=f32, order="F")
        self.U = np.zeros(tuple(Ng) + (D,), dtype=f32, order="F")
        self.UU = np.zeros(tuple(Ng) + (D, D), dtype=f32, order="F") if uu_stats else None
        self.t = [f32(t_init)]
        self.eps_log = []

    def reset(self, t_init=0.0):
        self.P[...] = 0
        self.U[...] = 0
        if self.UU is not None:
            self.UU[...] = 0
        self.t = [f32(t_init)]

    def weight(self, t_flow):
        """(dt, ε) of update! at time(flow) = t_flow   :237-239"""
        dt = f32(f32(t_flow) - self.t[-1])
        e = f32(dt / f32(f32(dt + f32(self.t[-1] - self.t[0])) + EPS32))
        if len(self.t) == 1:
            e = f32(1)
        return dt, e

    def update(self, p, u, t_flow):
        dt, e = self.weight(t_flow)
        om = f32(f32(1) - e)
        p, u = np.asarray(p, dtype=f32), np.asarray(u, dtype=f32)
        self.P[...] = e * p + om * self.P
        self.U[...] = e * u + om * self.U
        if self.UU is not None:
            for i in range(self.D):
                for j in range(self.D):
                    self.UU[..., i, j] = e * (u[..., i] * u[..., j]) + om * self.UU[..., i, j]
        self.t.append(f32(self.t[-1] + dt))
        self.eps_log.append(e)
        assert self.P.dtype == f32 and self.U.dtype == f32

    def uu(self):
        """uu!(τ, a)   :250-252"""
        tau = np.empty_like(self.UU)
        for i in range(self.D):
            for j in range(self.D):
                tau[..., i, j] = self.UU[..., i, j] - self.U[..., i] * self.U[..., j]
        return tau


def pack(UU):
    """(N…, D, D) -> (N…, D(D+1)/2): the components i ≤ j"""
    D = UU.shape[-1]
    out = np.empty(UU.shape[:-2] + (npk(D),), dtype=UU.dtype, order="F")
    for j in range(D):
        for i in range(j + 1):
            out[..., pk(i, j)] = UU[..., i, j]
    return out


def expand(packed, D):
    """(N…, D(D+1)/2) -> (N…, D, D)"""
    out = np.empty(packed.shape[:-1] + (D, D), dtype=packed.dtype, order="F")
    for i in range(D):
        for j in range(D):
            out[..., i, j] = packed[..., pk(i, j)]
    return out


def fields(dims, seed, k):
    """the seeded random (u, p) of update k of a case"""
    rng = np.random.default_rng([seed, k] + list(dims))
    Ng = tuple(n + 2 for n in dims)
    u = np.asfortranarray(rng.uniform(-0.3, 0.3, size=Ng + (len(dims),)).astype(f32))
    p = np.asfortranarray(rng.uniform(-1.0, 1.0, size=Ng).astype(f32))
    return u, p
