"""Flow diagnostics on the device (src/Metrics.jl:27-109; wl_metrics.hip): the reference's known answers through every leaf, fields
against the NumPy yardstick (tests/metrics_ref.py), λ₂ against LAPACK on degenerate input, ghosts and aliasing, one pass = the leaves,
sums = the fields, a physics smoke that also shows the step is untouched, rejections and the launch budget."""
import ctypes as C
import functools

import numpy as np
import pytest

import metrics_ref as mr
import sgs_ref

pytestmark = pytest.mark.gpu
WL_EINVAL = -1
EPS32 = float(np.finfo(np.float32).eps)
SEED = 7
SHAPES3 = [(1, 2, 3), (8, 24, 16), (20, 28, 36), (32, 32, 32), (70, 12, 9), (12, 70, 5)]      # 70: a tile seam (64 in x, 8 in y) + a ragged tile; 9, 5: odd plane counts
SHAPES2 = [(1, 2), (16, 16), (70, 20)]
Z, UBG = (0.3, -0.5, 1.0), (0.25, -0.5, 0.125)


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    return w


@functools.lru_cache(maxsize=None)
def _smooth(dims, ncomp=None, seed=SEED):
    """seeded smooth float32 (Ng...,ncomp) field, computed once and shared by the tests (none of them writes to it)"""
    rng = np.random.default_rng(seed)
    Ng = tuple(n + 2 for n in dims)
    a = np.asfortranarray(np.stack([sgs_ref.smooth_field(Ng, rng) for _ in range(ncomp or len(dims))], -1), dtype=np.float32)
    return a


def _ins(Ng):
    return tuple(slice(1, n - 1) for n in Ng)


def _rand_out(w, shape, seed=3):
    h = np.asfortranarray(np.random.default_rng(seed).standard_normal(shape), dtype=np.float32)
    return h, w.to_device(h)


def _field(w, fn, u, *args, vec=False, **kw):
    """inside cells of the field a leaf writes for the host array u"""
    Ng = u.shape[:-1]
    out = w.jl_zeros(Ng + (3,) if vec else Ng)
    fn(out, w.to_device(u), *args, **kw)
    return w.to_host(out)[_ins(Ng)]


def _center(Ng):
    return tuple(n / 2 for n in Ng)


# ------------------------------------------------------------------------------------------------ 1. known answers
def test_reference_known_answers_on_the_device(w):
    """test/test_metrics.jl:8-30 through every leaf: ke, curl and ω bit-equal, ω_mag and ω_θ within 1 ulp, |λ₂−1| ≤ √eps32, helicity bit-equal"""
    u = mr.kat_u(np.float32)
    J, x = (0, 1, 2), np.array([0.5, 1.5, 2.5])
    px = float(np.prod(x))
    om = np.array([0.5, -3.0, 2.5], np.float32)
    assert _field(w, w.ke_, u)[J] == np.float32(0.5 * np.sum((x + px) ** 2))
    assert _field(w, w.ke_, u, tuple(x))[J] == np.float32(1.5 * px ** 2)
    assert abs(float(_field(w, w.lambda2_, u)[J]) - 1) <= np.sqrt(EPS32)
    assert _field(w, w.curl_, u, 2)[J] == om[1]
    assert np.array_equal(_field(w, w.omega_, u, vec=True)[J], om)
    mag = np.sqrt(np.sum(om * om, dtype=np.float32))
    assert abs(float(_field(w, w.omega_mag_, u)[J]) - float(mag)) <= float(np.spacing(mag))
    th = _field(w, w.omega_theta_, u, (0, 0, 1), tuple(x + (0, 1, 2)))[J]
    assert abs(float(th) - 0.5) <= float(np.spacing(np.float32(0.5)))
    uh, wh = mr.kat_helicity(np.float32)
    out = w.jl_zeros((6, 6, 6))
    w.helicity_(out, w.to_device(uh), w.to_device(wh))
    assert w.to_host(out)[2, 2, 2] == np.float32(1.5 * 2.5)


# ------------------------------------------------------------------------------------------------ 2. fields vs yardstick
@pytest.mark.parametrize("dims", SHAPES3)
def test_fields_match_the_yardstick(w, dims):
    """ke, ω, ω_mag, ω_θ, helicity, curl(1..3) on smooth seeded input.  ∂(i,j,I,u) is @fastmath in the reference, so bit equality with NumPy
    is not defined; per quantity e32 = max|ref(float32) − ref(float64)| and the device must satisfy max|dev − ref(float64)| ≤ 4·e32
    (the convention and margin of test_gpu_sgs.py::test_leaf_matches_the_yardstick).  One run on an MI355X (the device reproduced the float32
    yardstick exactly in all 66 comparisons; e32 ranged from 1.2e-08 to 3.4e-07):
        dims (1, 2, 3) ke: e32 = 1.169e-07  device error = 1.169e-07
        dims (20, 28, 36) ke: e32 = 2.973e-07  device error = 2.973e-07
        dims (20, 28, 36) omega[0]: e32 = 8.568e-08  device error = 8.568e-08
        dims (20, 28, 36) omega_mag: e32 = 1.322e-07  device error = 1.322e-07
        dims (20, 28, 36) omega_theta: e32 = 1.436e-07  device error = 1.436e-07
        dims (20, 28, 36) helicity: e32 = 2.615e-07  device error = 2.615e-07
        dims (20, 28, 36) curl1: e32 = 5.215e-08  device error = 5.215e-08
        dims (70, 12, 9) omega_theta: e32 = 2.610e-07  device error = 2.610e-07
        dims (12, 70, 5) curl3: e32 = 5.960e-08  device error = 5.960e-08"""
    u, wv = _smooth(dims), _smooth(dims, 3, SEED + 1)
    Ng = u.shape[:-1]
    c = _center(Ng)
    cases = {
        "ke": (lambda d: mr.ke(u, UBG, d), lambda: _field(w, w.ke_, u, UBG)),
        "omega": (lambda d: mr.omega(u, d), lambda: _field(w, w.omega_, u, vec=True)),
        "omega_mag": (lambda d: mr.omega_mag(u, d), lambda: _field(w, w.omega_mag_, u)),
        "omega_theta": (lambda d: mr.omega_theta(u, Z, c, d), lambda: _field(w, w.omega_theta_, u, Z, c)),
        "helicity": (lambda d: mr.helicity(u, wv, d), lambda: _field(w, lambda o, ud: w.helicity_(o, ud, w.to_device(wv)), u)),
        "curl1": (lambda d: mr.curl(1, u, d), lambda: _field(w, w.curl_, u, 1)),
        "curl2": (lambda d: mr.curl(2, u, d), lambda: _field(w, w.curl_, u, 2)),
        "curl3": (lambda d: mr.curl(3, u, d), lambda: _field(w, w.curl_, u, 3)),
    }
    bad = []
    for name, (ref, dev) in cases.items():
        r64, r32, d = ref(np.float64), ref(np.float32), dev()
        comps = [(name, Ellipsis)] if name != "omega" else [(f"omega[{i}]", (Ellipsis, i)) for i in range(3)]
        for label, sl in comps:
            e32 = float(np.abs(r32[sl].astype(np.float64) - r64[sl]).max())
            err = float(np.abs(d[sl].astype(np.float64) - r64[sl]).max())
            print(f"dims {dims} {label}: e32 = {e32:.3e}  device error = {err:.3e}")
            assert np.all(np.isfinite(d[sl]))
            if not (e32 > 0 and err <= 4 * e32):
                bad.append((label, err, e32))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 3. λ₂ vs the yardstick
@functools.lru_cache(maxsize=None)
def _K():
    """K = 4·r32, r32 = the largest error of the float32 LAPACK yardstick against the float64 one in units of eps32·‖S²+Ω²‖_F on the
    (20,28,36) smooth input of SEED — a property of the input, computed at run time"""
    u = _smooth((20, 28, 36))
    A = mr.lambda2_matrix(u, np.float64)
    nrm = np.sqrt((A * A).sum((-1, -2)))
    r32 = float((np.abs(mr.lambda2(u, np.float32).astype(np.float64) - np.linalg.eigvalsh(A)[..., 1]) / (EPS32 * nrm)).max())
    return 4 * r32, r32


def _l2_ratio(dev, u):
    """max over cells of |dev − λ₂(float64)| / (eps32·‖S²+Ω²‖_F); cells with A = 0 must be exactly 0"""
    A = mr.lambda2_matrix(u, np.float64)
    nrm = np.sqrt((A * A).sum((-1, -2)))
    err = np.abs(dev.astype(np.float64) - np.linalg.eigvalsh(A)[..., 1])
    assert np.all(np.isfinite(dev))
    zero = nrm == 0
    assert np.all(dev[zero] == 0)
    return float((err[~zero] / (EPS32 * nrm[~zero])).max()) if (~zero).any() else 0.0


def test_lambda2_against_the_yardstick(w):
    """Per cell, in units of eps32·‖S²+Ω²‖_F (norm from the float64 yardstick): the device's error must be ≤ K = 4·r32 in every cell of every
    shape, on the three analytic cases (rotation: every cell has a degenerate pair; shear: A ≡ 0 and the result exactly 0; c·I: c²) and on a
    developed wall-bounded TGV (32³, 5 steps: its symmetry planes are degenerate, and its gradient nearly vanishes at isolated points, where
    ‖A‖ is 1e-5 of its maximum).  One run on an MI355X:
        r32 = 6.450  K = 25.800
        device ratio: (1,2,3) 0.095, (8,24,16) 0.999, (20,28,36) 1.539, (32,32,32) 3.070, (70,12,9) 2.743, (12,70,5) 1.396
        rotation 0.299 (λ₂ ∈ [−0.49000007, −0.48999974]), shear 0.000 (λ₂ ≡ 0.0), expansion 0.157, TGV 32³ after 5 steps 1.530
    A NumPy model of other methods on the same inputs: the written (a+b−c)−d association of ∂(i,j,I,u) in float32 gives 52 on the TGV's
    weak-gradient cells whatever solves the eigenproblem (the float32 LAPACK yardstick included); neighbour differences first with S²+Ω² in
    float32 gives 13; the kernel's choice — neighbour differences first, S²+Ω² and the closed form in float64 — gives the figures above."""
    K, r32 = _K()
    print(f"r32 = {r32:.3f}  K = {K:.3f}")
    bad = []
    for dims in SHAPES3:
        u = _smooth(dims)
        ratio = _l2_ratio(_field(w, w.lambda2_, u), u)
        print(f"dims {dims}: device ratio = {ratio:.3f}")
        bad += [(dims, ratio)] if not ratio <= K else []
    for kind, par, exact in (("rotation", 0.7, -0.49), ("shear", 1.3, 0.0), ("expansion", 0.45, 0.2025)):
        u = mr.analytic_u(kind, (12, 11, 10), par)
        d = _field(w, w.lambda2_, u)
        ratio = _l2_ratio(d, u)
        print(f"{kind}: device ratio = {ratio:.3f}  λ₂ ∈ [{d.min()!r}, {d.max()!r}]")
        bad += [(kind, ratio)] if not ratio <= K else []
        if kind == "shear":
            assert np.all(d == 0)
        else:
            assert np.abs(d - exact).max() <= 1e-5 * abs(exact)
    s = w.FusedSimulation((32, 32, 32), (0, 0, 0), 32, U=1, nu=32 / 1600.0, ic="tgv")
    s.mom_steps_(5)
    d = w.to_host(s.metric("lambda2"))[_ins(s.Ng)]
    ratio = _l2_ratio(d, s.field("u"))
    print(f"TGV 32³ after 5 steps: device ratio = {ratio:.3f}")
    bad += [("tgv", ratio)] if not ratio <= K else []
    assert not bad, (bad, K)


# ------------------------------------------------------------------------------------------------ 4. ghosts and aliasing
@pytest.mark.parametrize("dims", [(8, 24, 16), (70, 12, 9), (16, 16), (70, 20)])
def test_only_inside_cells_are_written(w, dims):
    D = len(dims)
    u = _smooth(dims)
    Ng = u.shape[:-1]
    ud = w.to_device(u)
    ins = _ins(Ng)
    calls = {"ke": lambda o: w.ke_(o, ud, UBG[:D]), "curl": lambda o: w.curl_(o, ud, 3)}
    if D == 3:
        wd = w.to_device(_smooth(dims, 3, SEED + 1))
        calls.update({"omega": lambda o: w.omega_(o, ud), "omega_mag": lambda o: w.omega_mag_(o, ud), "omega_theta": lambda o: w.omega_theta_(o, ud, Z, _center(Ng)),
                      "lambda2": lambda o: w.lambda2_(o, ud), "helicity": lambda o: w.helicity_(o, ud, wd), "curl1": lambda o: w.curl_(o, ud, 1)})
    for name, call in calls.items():
        h, o = _rand_out(w, Ng + (3,) if name == "omega" else Ng)
        call(o)
        r = w.to_host(o)
        for c in range(3 if name == "omega" else 1):
            a, b = (r[..., c], h[..., c]) if name == "omega" else (r, h)
            ghost = np.ones(Ng, bool); ghost[ins] = False
            assert np.array_equal(a[ghost], b[ghost]), name
            assert np.all(a[ins] != b[ins]), name
    if D == 3:                                                            # the one-pass call, all four outputs
        hs = [_rand_out(w, Ng + (3,) if k == 1 else Ng, seed=10 + k) for k in range(4)]
        w.flow_fields_(ud, ke=hs[0][1], omega=hs[1][1], omega_mag=hs[2][1], lambda2=hs[3][1])
        for k, (h, o) in enumerate(hs):
            r = w.to_host(o)
            ghost = np.ones(r.shape, bool); ghost[ins] = False
            assert np.array_equal(r[ghost], h[ghost]) and np.all(r[ins] != h[ins]), k


def test_sigma_as_output_and_aliasing(w):
    from waterlily_jl_amd._lib import lib
    L = lib()
    s = w.FusedSimulation((16, 24, 8), (0, 0, 0), 16, U=1, nu=0.01, ic="tgv")
    s.mom_step_()
    own = w.to_host(s.metric("omega_mag"))
    before = s.field("sigma")
    out = s.metric("omega_mag", out="sigma")
    sig = s.field("sigma")
    ins = _ins(s.Ng)
    assert np.array_equal(sig[ins], own[ins]) and np.array_equal(w.to_host(out), sig)
    ghost = np.ones(s.Ng, bool); ghost[ins] = False
    assert np.array_equal(sig[ghost], before[ghost])
    s.mom_step_()                                                          # σ is scratch: the step goes on
    assert np.all(np.isfinite(s.field("u")))
    u = w.to_device(_smooth((8, 24, 16)))
    g = w.core.vgrid(u)
    p = w.core.ptr(u)
    p2 = C.c_void_p(p.value + 4 * int(np.prod(u.shape[:-1])))             # the second component
    for q in (p, p2):
        assert L.wl_ke(q, p, C.byref(g), None, None) == WL_EINVAL and b"alias" in L.wl_last_error_string()
        assert L.wl_lambda2(q, p, C.byref(g), None) == WL_EINVAL
        assert L.wl_curl(q, p, C.byref(g), 3, None) == WL_EINVAL and b"alias" in L.wl_last_error_string()
        assert L.wl_omega_theta(q, p, C.byref(g), (C.c_float * 3)(0, 0, 1), (C.c_float * 3)(), None) == WL_EINVAL
        assert L.wl_helicity(q, p, p, C.byref(g), None) == WL_EINVAL
    assert np.array_equal(w.to_host(u), _smooth((8, 24, 16)))


# ------------------------------------------------------------------------------------------------ 5. one pass = the leaves
@pytest.mark.parametrize("dims", [(8, 24, 16), (70, 12, 9)])
def test_one_pass_equals_the_leaves(w, dims):
    u = _smooth(dims)
    Ng = u.shape[:-1]
    ud = w.to_device(u)
    names = ("ke", "omega", "omega_mag", "lambda2")
    new = lambda k: w.jl_zeros(Ng + (3,) if k == "omega" else Ng)      # noqa: E731
    leaf = {"ke": w.ke_(new("ke"), ud, UBG), "omega": w.omega_(new("omega"), ud), "omega_mag": w.omega_mag_(new("omega_mag"), ud), "lambda2": w.lambda2_(new("lambda2"), ud)}
    leaf = {k: w.to_host(v) for k, v in leaf.items()}
    allo = {k: new(k) for k in names}
    w.flow_fields_(ud, U=UBG, **allo)
    for k in names:
        assert np.array_equal(w.to_host(allo[k]), leaf[k]), k
        one = new(k)
        w.flow_fields_(ud, U=UBG, **{k: one})
        assert np.array_equal(w.to_host(one), leaf[k]), k
    pair = {k: new(k) for k in ("omega", "lambda2")}
    w.flow_fields_(ud, **pair)
    assert all(np.array_equal(w.to_host(pair[k]), leaf[k]) for k in pair)


def _sim_fields(w, L, h, Ng):
    from waterlily_jl_amd.core import ptr, stream
    o = [w.jl_zeros(Ng), w.jl_zeros(Ng + (3,)), w.jl_zeros(Ng), w.jl_zeros(Ng)]
    assert L.wl_sim_flow_fields(h, (C.c_float * 3)(*UBG), ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), stream()) == 0
    return [w.to_host(a) for a in o]


def _leaf_fields(w, u):
    Ng = u.shape[:-1]
    ud = w.to_device(u)
    o = [w.jl_zeros(Ng), w.jl_zeros(Ng + (3,)), w.jl_zeros(Ng), w.jl_zeros(Ng)]
    w.flow_fields_(ud, ke=o[0], omega=o[1], omega_mag=o[2], lambda2=o[3], U=UBG)
    return [w.to_host(a) for a in o]


def test_handle_fields_follow_the_current_velocity(w):
    """wl_sim_flow_fields equals the leaf on wl_sim_field("u") after mom_step_ and after mom_steps_(3) (the velocity roles have rotated), on a
    handle-owned and on a caller-owned handle"""
    from test_gpu_callerowned import CallerOwnedSim
    from waterlily_jl_amd._lib import lib
    L = lib()
    dims = (32, 24, 40)
    s = w.FusedSimulation(dims, (0, 0, 0), 32, U=1, nu=0.02, ic="tgv")
    p0 = L.wl_sim_field(s._h, b"u")
    moved = False
    for n in (1, 3):
        s.mom_step_() if n == 1 else s.mom_steps_(n)
        moved = moved or L.wl_sim_field(s._h, b"u") != p0
        got, exp = _sim_fields(w, L, s._h, s.Ng), _leaf_fields(w, s.field("u"))
        assert all(np.array_equal(a, b) for a, b in zip(got, exp)), n
        assert s.flow_stats(UBG) == w.flow_stats(w.to_device(s.field("u")), UBG)
    assert moved
    rng = np.random.default_rng(5)
    u_init = np.asfortranarray(rng.uniform(-0.3, 0.3, size=s.Ng + (3,)).astype(np.float32))
    u_init[..., 0] += 1.0
    co = CallerOwnedSim(w, dims, (1.0, 0.0, 0.0), 0.02, u_init, True)
    for n in range(2):
        co.mom_step()
        got, exp = _sim_fields(w, L, co.h, co.Ng), _leaf_fields(w, co.field("u"))
        assert all(np.array_equal(a, b) for a, b in zip(got, exp)), n
    co.close()


# ------------------------------------------------------------------------------------------------ 6. sums = fields
def _sum64(a):
    return float(np.sum(a.astype(np.float64)))


@pytest.mark.parametrize("dims", [(1, 2, 3), (20, 28, 36), (70, 12, 9), (12, 70, 5)])
@pytest.mark.parametrize("U", [None, UBG])
def test_sums_equal_the_fields(w, dims, U):
    """flow_stats = Float64 sums of the per-cell Float32 values the field kernels write (only the order of the Float64 partial sums differs:
    rtol 1e-10), and the maximum bit for bit"""
    from waterlily_jl_amd._lib import lib
    L = lib()
    u = _smooth(dims)
    ud = w.to_device(u)
    kef, wf, wm = _field(w, w.ke_, u, U), _field(w, w.omega_, u, vec=True), _field(w, w.omega_mag_, u)
    n0 = L.wl_launch_count()
    ke, en, mx = w.flow_stats(ud, U)
    assert L.wl_launch_count() - n0 <= 2
    half = np.float32(0.5) * ((wf[..., 0] * wf[..., 0] + wf[..., 1] * wf[..., 1]) + wf[..., 2] * wf[..., 2])      # the per-cell Float32 ½ω·ω, then promoted
    assert half.dtype == np.float32
    print(f"dims {dims}: KE {ke!r} vs {_sum64(kef)!r}  enstrophy {en!r} vs {_sum64(half)!r}  max|ω| {mx!r}")
    assert np.isclose(ke, _sum64(kef), rtol=1e-10, atol=0) and np.isclose(en, _sum64(half), rtol=1e-10, atol=0)
    assert np.float32(mx) == wm.max() and mx == float(wm.max())


@pytest.mark.parametrize("dims", SHAPES2)
@pytest.mark.parametrize("U", [None, UBG[:2]])
def test_sums_equal_the_fields_2d(w, dims, U):
    from waterlily_jl_amd._lib import lib
    L = lib()
    u = _smooth(dims)
    kef, cf = _field(w, w.ke_, u, U), _field(w, w.curl_, u, 3)
    r32, r64 = mr.ke(u, U, np.float32), mr.ke(u, U, np.float64)
    e32 = float(np.abs(r32.astype(np.float64) - r64).max())
    assert e32 > 0 and np.abs(kef.astype(np.float64) - r64).max() <= 4 * e32
    c32, c64 = mr.curl(3, u, np.float32), mr.curl(3, u, np.float64)
    e32 = float(np.abs(c32.astype(np.float64) - c64).max())
    assert e32 > 0 and np.abs(cf.astype(np.float64) - c64).max() <= 4 * e32
    n0 = L.wl_launch_count()
    ke, en, mx = w.flow_stats(w.to_device(u), U)
    assert L.wl_launch_count() - n0 <= 2
    assert np.isclose(ke, _sum64(kef), rtol=1e-10, atol=0) and np.isclose(en, _sum64(np.float32(0.5) * (cf * cf)), rtol=1e-10, atol=0)
    assert mx == float(np.abs(cf).max())


def test_launch_budget(w):
    from waterlily_jl_amd._lib import lib
    L = lib()
    u = w.to_device(_smooth((20, 28, 36)))
    Ng = tuple(u.shape[:-1])
    s, v, wv = w.jl_zeros(Ng), w.jl_zeros(Ng + (3,)), w.to_device(_smooth((20, 28, 36), 3, SEED + 1))
    calls = [lambda: w.ke_(s, u), lambda: w.curl_(s, u, 1), lambda: w.omega_(v, u), lambda: w.omega_mag_(s, u), lambda: w.omega_theta_(s, u, Z, (1, 2, 3)),
             lambda: w.lambda2_(s, u), lambda: w.helicity_(s, u, wv), lambda: w.flow_fields_(u, ke=s, omega=v, omega_mag=w.jl_zeros(Ng), lambda2=w.jl_zeros(Ng))]
    for k, call in enumerate(calls):
        n0 = L.wl_launch_count()
        call()
        assert L.wl_launch_count() - n0 == 1, k
    n0 = L.wl_launch_count()
    w.flow_stats(u)
    assert L.wl_launch_count() - n0 <= 2


# ------------------------------------------------------------------------------------------------ 7. physics smoke
def test_energy_history_on_the_device_and_the_step_is_untouched(w):
    """wall-bounded TGV at 32³, ν = N/1600, flow_stats() after each of 20 steps: KE does not grow after the first few steps, enstrophy is positive
    and finite, both equal the host NumPy evaluation of field("u") (rtol 1e-10 on the Float64 sums of Float32 cell values, the maximum bit for
    bit), and u, p and the Δt history equal a run of 20 steps without diagnostics calls bit for bit"""
    N = 32
    mk = lambda: w.FusedSimulation((N, N, N), (0, 0, 0), N, U=1, nu=N / 1600.0, ic="tgv")      # noqa: E731
    a, b = mk(), mk()
    hist = []
    for step in range(20):
        a.mom_step_()
        ke, en, mx = a.flow_stats()
        a.metric("lambda2", out="sigma")                                  # a field call into the handle's σ between steps as well
        u = a.field("u")
        wf = mr.omega(u, np.float32)
        half = np.float32(0.5) * ((wf[..., 0] * wf[..., 0] + wf[..., 1] * wf[..., 1]) + wf[..., 2] * wf[..., 2])
        assert np.isclose(ke, _sum64(mr.ke(u, dtype=np.float32)), rtol=1e-10, atol=0), step
        assert np.isclose(en, _sum64(half), rtol=1e-10, atol=0), step
        assert mx == float(mr.omega_mag(u, np.float32).max()), step
        assert np.isfinite(en) and en > 0
        hist.append(ke)
    print("KE history:", " ".join(f"{v:.6e}" for v in hist))
    assert all(hist[k + 1] <= hist[k] for k in range(3, 19)), hist
    b.mom_steps_(20)
    assert np.array_equal(a.field("u"), b.field("u")) and np.array_equal(a.field("p"), b.field("p"))
    assert np.array_equal(np.array(a.dt), np.array(b.dt)) and a.pois_n == b.pois_n


# ------------------------------------------------------------------------------------------------ 8. rejections
def test_rejections(w):
    from waterlily_jl_amd._lib import ALLGATHER_FN, SENDRECV_FN, lib, wl_sim_desc
    from waterlily_jl_amd.core import ptr
    from waterlily_jl_amd.slab import slab_grid
    L = lib()
    z3 = (C.c_float * 3)(0, 0, 1)
    out3 = (C.c_double * 3)()

    def rejected(rc, word=None):
        msg = L.wl_last_error_string()
        assert rc == WL_EINVAL and msg, (rc, msg)
        assert word is None or word in msg, msg

    # a 2-D grid where 3-D is required
    u2, s2, v2 = w.to_device(_smooth((16, 16))), w.jl_zeros((18, 18)), w.jl_zeros((18, 18, 3))
    g2 = w.core.vgrid(u2)
    rejected(L.wl_omega(ptr(v2), ptr(u2), C.byref(g2), None), b"3-D")
    rejected(L.wl_omega_mag(ptr(s2), ptr(u2), C.byref(g2), None), b"3-D")
    rejected(L.wl_omega_theta(ptr(s2), ptr(u2), C.byref(g2), z3, z3, None), b"3-D")
    rejected(L.wl_lambda2(ptr(s2), ptr(u2), C.byref(g2), None), b"3-D")
    rejected(L.wl_helicity(ptr(s2), ptr(u2), ptr(v2), C.byref(g2), None), b"3-D")
    rejected(L.wl_flow_fields(ptr(u2), C.byref(g2), None, ptr(s2), ptr(v2), None, None, None), b"3-D")
    rejected(L.wl_flow_fields(ptr(u2), C.byref(g2), None, None, None, None, ptr(s2), None), b"3-D")
    assert L.wl_flow_fields(ptr(u2), C.byref(g2), None, ptr(s2), None, None, None, None) == 0          # ke alone is a 2-D method
    # curl's component
    u3, s3, v3 = w.to_device(_smooth((8, 24, 16))), w.jl_zeros((10, 26, 18)), w.jl_zeros((10, 26, 18, 3))
    g3 = w.core.vgrid(u3)
    for i in (0, 4):
        rejected(L.wl_curl(ptr(s3), ptr(u3), C.byref(g3), i, None), b"1, 2 or 3")
        rejected(L.wl_curl(ptr(s2), ptr(u2), C.byref(g2), i, None))
    for i in (1, 2):
        rejected(L.wl_curl(ptr(s2), ptr(u2), C.byref(g2), i, None), b"2-D")
    # null pointers and all-null outputs
    rejected(L.wl_flow_fields(ptr(u3), C.byref(g3), None, None, None, None, None, None), b"null")
    rejected(L.wl_ke(None, ptr(u3), C.byref(g3), None, None), b"null")
    rejected(L.wl_ke(ptr(s3), None, C.byref(g3), None, None), b"null")
    rejected(L.wl_omega(None, ptr(u3), C.byref(g3), None), b"null")
    rejected(L.wl_helicity(ptr(s3), ptr(u3), None, C.byref(g3), None), b"null")
    rejected(L.wl_omega_theta(ptr(s3), ptr(u3), C.byref(g3), None, z3, None), b"null")
    rejected(L.wl_flow_stats(None, C.byref(g3), None, out3, None, None), b"null")
    rejected(L.wl_flow_stats(ptr(u3), C.byref(g3), None, None, None, None), b"null")
    # a z-slab grid: every entry point
    gs = slab_grid((18, 18, 34), 0, 2)
    us, ss = w.jl_zeros((gs.nx, gs.ny, gs.nz, 3)), w.jl_zeros((gs.nx, gs.ny, gs.nz))
    vs = w.jl_zeros((gs.nx, gs.ny, gs.nz, 3))
    for rc in (lambda: L.wl_ke(ptr(ss), ptr(us), C.byref(gs), None, None), lambda: L.wl_curl(ptr(ss), ptr(us), C.byref(gs), 3, None),
               lambda: L.wl_omega(ptr(vs), ptr(us), C.byref(gs), None), lambda: L.wl_omega_mag(ptr(ss), ptr(us), C.byref(gs), None),
               lambda: L.wl_omega_theta(ptr(ss), ptr(us), C.byref(gs), z3, z3, None), lambda: L.wl_lambda2(ptr(ss), ptr(us), C.byref(gs), None),
               lambda: L.wl_helicity(ptr(ss), ptr(us), ptr(vs), C.byref(gs), None), lambda: L.wl_flow_fields(ptr(us), C.byref(gs), None, ptr(ss), None, None, None, None),
               lambda: L.wl_flow_stats(ptr(us), C.byref(gs), None, out3, None, None)):
        rejected(rc(), b"slab")
    # a z-slab handle (rank 0 of 2; the transport does nothing: no step is taken)
    sr = SENDRECV_FN(lambda *a: 0); ag = ALLGATHER_FN(lambda *a: 0)
    comm = C.c_void_p()
    assert L.wl_comm_callbacks_create(C.byref(comm), 0, 2, None, C.cast(sr, C.c_void_p), C.cast(ag, C.c_void_p)) == 0
    d = wl_sim_desc()
    d.D = 3
    for k in range(3):
        d.dims[k] = (16, 16, 32)[k]
    d.nu, d.dt0 = 0.01, 0.25
    h = C.c_void_p()
    assert L.wl_sim_create_slab(C.byref(h), C.byref(d), comm) == 0
    rejected(L.wl_sim_flow_stats(h, None, out3, None), b"slab")
    rejected(L.wl_sim_flow_fields(h, None, ptr(ss), None, None, None, None), b"slab")
    assert L.wl_sim_destroy(h) == 0 and L.wl_comm_destroy(comm) == 0
    # the Python surface raises
    with pytest.raises(w.WlError):
        w.lambda2_(s2, u2)
    with pytest.raises(ValueError):
        w.FusedSimulation((16, 16), (1.0, 0.0), 16).metric("enstrophy")
