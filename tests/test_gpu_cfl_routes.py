"""Δt on every route that forms it, against min(10, 1/(max σ + 5ν)) evaluated in float32 (tests/norms_ref.py: dt_from_sigma) over ALL cells of the σ that the
plain handle left after the same step — ghost cells included: σ's upper ghost cells keep conv_diff!'s stale Φ (quirk Q1), and CFL's maximum sees them.

Cases: SIGMA_CASES of tests/norms_ref.py — a uniform stream plus one jet, written with set_field("u", …) before the first step; tests/test_norms_cpu.py shows
on the oracle where each puts maximum(σ): on the interior classes of the tilings, and on a ghost cell of the upper x, y and z face.  Routes (ROUTES):
cfl_dev behind the plain projection (also phase by phase), the pair tail project_cfl with four and with two cells per thread, with σ stored, lazydt on and off
(wl_sim_mom_steps(2): the one-thread k_dt_from_cfl leaves Δt on the device), the tail inside the corrector's loader (the k_conv_q1 operands), project_cfl_split
on a handle whose smoother is split in z, the 2-D circle of tests/callseq.py's circle2d family.  Per route: one mom_step!, then two more in one call.
  * every Δt appended equals dt_from_sigma(σ_plain, ν) as raw bits;
  * σ's ghost cells equal the plain handle's as raw bits on every route; where the route stores σ (cfl_dev, "store_f") all of σ does, and its own σ gives Δt;
  * the counters say which route ran.
The leaf wl_cfl: σ's ghost cells preset, the maximum planted on interior cells either side of the seams of k_cfl's 256-cell blocks and plane chunks, then on a
ghost cell of each of the six faces: the WHOLE array takes part."""
import ctypes as C

import numpy as np
import pytest

import callseq
import norms_ref as nr
import test_gpu_rskip as rk
from test_gpu_norms import bits32, leaf_positions

pytestmark = pytest.mark.gpu

f32 = np.float32
NU = nr.SIGMA_NU
PLAIN = {"fuse_cfl": 0, "fuse_p": 0}
# name -> (options, stepped phase by phase, stores σ)
ROUTES = {
    "plain_phases": (PLAIN, True, True),
    "default": ({}, False, False),                       # the pair tail, four cells per thread where the shape allows; lazydt
    "tailwide0": ({"tailwide": 0}, False, False),        # the pair tail, two cells per thread
    "store_f": ({"store_f": 1}, False, True),            # the pair tail stores σ
    "lazydt0": ({"lazydt": 0}, False, False),            # Δt on the host between the steps of one call
    "tailfuse1": ({"tailfuse": 1}, False, False),        # the first tail inside the corrector's loader: k_conv_q1 forms the stale Φ from other operands
    "fuse_cfl0": ({"fuse_cfl": 0}, False, True),         # cfl_dev behind the fused projection
}


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    yield w
    w.lib().wl_reset_process_options()


def make(w, dims, ubc, u, **opts):
    sg = w.FusedSimulation(dims, ubc, dims[0], U=1, nu=NU, u0=u)
    sg.set_option("resjac_min", 0)
    sg.set_option("convt_min", 0)
    for k, v in opts.items():
        sg.set_option(k, v)
    sg.set_field("u", u)      # (the constructor applied BC!: the same array again, as the issue's call sequence has it)
    return sg


def run_route(sg, phases):
    """one mom_step!, then two in one call -> the three Δt appended (the history starts with the constructor's Δt)"""
    n0 = len(sg.dt)
    if phases:
        for _ in range(3):
            for q in range(6):
                sg.phase_(q)
    else:
        sg.mom_step_()
        sg.mom_steps_(2)
    dt = sg.dt
    assert len(dt) == n0 + 3
    return dt[n0:]


def plain_reference(sg):
    """the plain handle stepped singly, σ read after every step -> [(σ, Δt appended)]"""
    out = []
    for _ in range(3):
        sg.mom_step_()
        out.append((sg.field("sigma"), sg.dt[-1]))
    return out


def ghost_mask(shape):
    m = np.ones(shape, dtype=bool)
    m[tuple(slice(1, n - 1) for n in shape)] = False
    return m


def check_dt(what, dts, ref, nu=NU):
    for q, (dt, (sigma, dt_plain)) in enumerate(zip(dts, ref)):
        want = nr.dt_from_sigma(sigma, nu)
        am = tuple(int(v) for v in np.unravel_index(int(sigma.argmax()), sigma.shape))
        print(f"{what} step {q}: Δt {float(dt):.9e}, from σ_plain {float(want):.9e} (max σ {float(sigma[am]):.6f} at {am}{', a ghost cell' if ghost_mask(sigma.shape)[am] else ''})")
        assert nr.bits(dt) == nr.bits(want), (what, q, float(dt), float(want))


def check_sigma(what, sg, ref_sigma, stores, dt_last):
    s = sg.field("sigma")
    g = ghost_mask(s.shape)
    nd = int((bits32(s)[g] != bits32(ref_sigma)[g]).sum())
    print(f"{what}: σ ghost cells differing from the plain handle's: {nd} of {int(g.sum())}; stores σ: {stores}")
    assert nd == 0, (what, "ghost cells of σ", nd)
    if stores:
        assert np.array_equal(bits32(s), bits32(ref_sigma)), (what, "σ", int((bits32(s) != bits32(ref_sigma)).sum()))
        assert nr.bits(nr.dt_from_sigma(s, NU)) == nr.bits(dt_last), what


CASES3 = [c for c in nr.SIGMA_CASES if len(c[0]) == 3 and c[0][2] != 32]


@pytest.mark.parametrize("q", range(len(CASES3)), ids=[f"{'x'.join(map(str, c[0]))}-{c[3]}" for c in CASES3])
def test_dt_on_every_route(w, oracle, q):
    dims, ubc, jets, cls, pick, arg, classes = CASES3[q]
    u = nr.stream_and_jets(dims, ubc, jets, oracle.BC)
    plain = make(w, dims, ubc, u, **PLAIN)
    ref = plain_reference(plain)
    assert plain.counter("resjac") == 0 and plain.counter("tailwide") == 0 and plain.counter("tailfuse") == 0
    check_dt(f"{dims} {cls} plain", [d for _, d in ref], ref)
    if "ghost" in classes:      # the case is here for it: the device's maximum sits on a ghost cell too
        for sigma, _ in ref[:1]:
            am = np.unravel_index(int(sigma.argmax()), sigma.shape)
            assert ghost_mask(sigma.shape)[am], (cls, am)
    for name, (opts, phases, stores) in ROUTES.items():
        what = f"{dims} {cls} {name}"
        sg = make(w, dims, ubc, u, **opts)
        dts = run_route(sg, phases)
        check_dt(what, dts, ref)
        assert sg.pois_n == plain.pois_n, (what, sg.pois_n, plain.pois_n)
        check_sigma(what, sg, ref[-1][0], stores, dts[-1])
        head = name not in ("plain_phases", "store_f")      # the one-launch head needs the fused projection and does not run with f stored
        assert (sg.counter("resjac") > 0) == head, (what, "resjac", sg.counter("resjac"))
        assert sg.counter("tailfuse") == (3 if name == "tailfuse1" else 0), (what, "tailfuse", sg.counter("tailfuse"))
        if name in ("plain_phases", "tailwide0"):
            assert sg.counter("tailwide") == 0, (what, "tailwide")
        if name == "default":
            assert sg.counter("tailwide") > 0 and sg.counter("tailspec_armed") > 0, what


def zsplit_handle(w, dims, ubc, u, **opts):
    """coefficients off the constant pattern on two middle planes: the smoother — and the tail, project_cfl_split — run on three plane ranges"""
    sg = w.FusedSimulation(dims, ubc, dims[0], U=1, nu=NU, u0=u)
    mu0 = sg.field("mu0")
    mu0[20:40, 10:20, nr.ZSPLIT_PLANES[0]:nr.ZSPLIT_PLANES[1], :] = 0.5
    sg.set_field("mu0", mu0)
    for k, v in dict(resjac_min=0, convt_min=0, **opts).items():
        sg.set_option(k, v)
    sg.update_()
    sg.set_field("u", u)
    return sg


CASES_ZS = [c for c in nr.SIGMA_CASES if len(c[0]) == 3 and c[0][2] == 32]


@pytest.mark.parametrize("q", range(len(CASES_ZS)), ids=[c[3] for c in CASES_ZS])
def test_dt_of_the_z_split_tail(w, oracle, q):
    dims, ubc, jets, cls, pick, arg, classes = CASES_ZS[q]
    u = nr.stream_and_jets(dims, ubc, jets, oracle.BC)
    plain = zsplit_handle(w, dims, ubc, u, zsplit=0, **PLAIN)
    assert plain.counter("part") == 0
    ref = plain_reference(plain)
    check_dt(f"z-split {cls} plain", [d for _, d in ref], ref)
    for name, opts in (("split", {"zsplit": 2}), ("split, σ stored", {"zsplit": 2, "store_f": 1}), ("split, cfl_dev", {"zsplit": 2, "fuse_cfl": 0})):
        sg = zsplit_handle(w, dims, ubc, u, **opts)
        assert sg.counter("part") == 1 and sg.smoother_kinds()[0] == 3, name
        dts = run_route(sg, False)
        check_dt(f"z-split {cls} {name}", dts, ref)
        assert sg.pois_n == plain.pois_n
        check_sigma(f"z-split {cls} {name}", sg, ref[-1][0], name != "split", dts[-1])


CASES2 = [c for c in nr.SIGMA_CASES if len(c[0]) == 2]


@pytest.mark.parametrize("q", range(len(CASES2)), ids=[c[3] for c in CASES2])
def test_dt_of_the_2d_circle(w, oracle, q):
    import bodypaths_ref as bp
    from test_gpu_bodypaths import handle
    dims, ubc, jets, cls, pick, arg, classes = CASES2[q]
    case = next(c for c in bp.CASES if c["id"] == callseq.BODY_CASE["circle2d"])
    assert tuple(case["dims"]) == tuple(dims) and tuple(ubc) == (1.0, 0.0)
    u = nr.stream_and_jets(dims, ubc, jets, oracle.BC)
    res = {}
    for name, opts in (("plain", dict(callseq.GATES, **callseq.EAGER, **callseq.EAGER_BODY, **PLAIN)), ("default", dict(callseq.GATES, zsplit=2))):
        sg = handle(w, case, opts)
        sg.measure_body_(case["positions"][0][0], 1.0)
        sg.set_field("u", u)
        res[name] = sg
    res["plain"].set_option("body_tile", 0)      # (process-wide: set for the handle that is about to run)
    ref = plain_reference(res["plain"])
    check_dt(f"circle2d {cls} plain", [d for _, d in ref], ref)
    res["default"].set_option("body_tile", 1)
    dts = run_route(res["default"], False)
    check_dt(f"circle2d {cls} default", dts, ref)
    assert res["default"].pois_n == res["plain"].pois_n
    check_sigma(f"circle2d {cls} default", res["default"], ref[-1][0], False, dts[-1])


# --------------------------------------------------------------------------------------------------------------------------------- the leaf
def flux_out(u):
    """σ on the interior as k_cfl writes it (float32, its order of additions), 0 elsewhere"""
    Ng = u.shape[:-1]
    s = np.zeros(Ng, dtype=f32, order="F")
    z = f32(0)
    ux, uy, uz = u[..., 0], u[..., 1], u[..., 2]
    a = np.maximum(z, ux[2:, 1:-1, 1:-1]) + np.maximum(z, -ux[1:-1, 1:-1, 1:-1])
    b = np.maximum(z, uy[1:-1, 2:, 1:-1]) + np.maximum(z, -uy[1:-1, 1:-1, 1:-1])
    c = np.maximum(z, uz[1:-1, 1:-1, 2:]) + np.maximum(z, -uz[1:-1, 1:-1, 1:-1])
    s[1:-1, 1:-1, 1:-1] = ((z + a) + b) + c
    return s


@pytest.mark.parametrize("shape", [(66, 34, 26), (450, 370, 10)], ids=["66x34x26", "450x370x10"])
def test_leaf_cfl_the_whole_array_takes_part(w, shape):
    lib, chk = w.lib(), w._lib.check
    rng = np.random.default_rng(29)
    u0 = np.asfortranarray(rng.uniform(-0.4, 0.4, size=shape + (3,)).astype(f32))
    pre = np.asfortranarray(rng.uniform(0.0, 0.05, size=shape).astype(f32))      # σ before the call: ghost cells preset, the interior to be overwritten
    nx, ny, nz = shape
    plants = [("interior " + n, idx, None) for n, idx in leaf_positions(shape)]
    faces = {"x0": (0, ny // 2, nz // 2), "x1": (nx - 1, 3, 2), "y0": (nx // 3, 0, nz - 2), "y1": (5, ny - 1, 1), "z0": (nx - 2, ny - 2, 0), "z1": (1, 1, nz - 1),
             "corner": (nx - 1, ny - 1, nz - 1)}
    plants += [("ghost " + n, None, idx) for n, idx in faces.items()]
    t_u = w.to_device(u0)
    g = w.core.sgrid(w.to_device(pre))
    for name, cell, ghost in plants:
        u, sig = u0, pre.copy(order="F")
        if cell is not None:      # flux_out of the cell: u_x on its upper face
            u = u0.copy(order="F")
            u[cell[0] + 1, cell[1], cell[2], 0] = f32(5.0)
            t_u = w.to_device(u)
        else:
            sig[ghost] = f32(9.0)
        ref = np.where(ghost_mask(shape), sig, flux_out(u))
        am = tuple(int(v) for v in np.unravel_index(int(ref.argmax()), ref.shape))
        assert am == (cell if cell is not None else ghost), (name, am)
        t_s = w.to_device(sig)
        out = C.c_float()
        chk(lib.wl_cfl(w.core.ptr(t_u), w.core.ptr(t_s), C.byref(g), NU, 10.0, C.byref(out), w.core.stream()))
        got = w.core.to_host(t_s)
        want = nr.dt_from_sigma(ref, NU)
        print(f"{shape} {name} at {am}: Δt {out.value:.9e} vs {float(want):.9e}")
        assert nr.bits(out.value) == nr.bits(want), (name, out.value, float(want))
        assert np.array_equal(bits32(got), bits32(ref)), (name, "σ", int((bits32(got) != bits32(ref)).sum()))
        if cell is not None:
            t_u = w.to_device(u0)
