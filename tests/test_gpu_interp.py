"""interp at points on the device (wl_interp, wl_sim_sample; csrc/wl_interp.hip) against the NumPy restatement of src/util.jl:17-43
(tests/interp_ref.py): the reference's known answers, random scalar and vector fields at points inside, outside and exactly on the
clamp, linear fields, the handle form on rotated array roles, and the argument checks.

Bound (set by the feature's issue): |device − ref64| ≤ 4·max over the points |ref32 − ref64|, floor 4·eps32·max|arr| — ref32 the
restatement in Float32 in the written order, ref64 the same formula in Float64.  The reference's @fastmath @simd sum has no fixed order,
so equality of bits with ref32 is printed (pytest -s), not required."""
import ctypes as C

import numpy as np
import pytest

import interp_ref as ir

pytestmark = pytest.mark.gpu
f32 = np.float32
GRIDS = {3: (12, 10, 9), 2: (11, 7)}      # with ghosts


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    return w


def point_set(Ng, n, seed):
    """n points: the corners of the clamp range and 0, points on integers and half-integers, points up to 3 cells outside on every side, the rest inside"""
    rng = np.random.default_rng(seed)
    D = len(Ng)
    hi = np.array(Ng, dtype=f32) - 2
    special = [hi.copy(), np.zeros(D, dtype=f32)]
    for d in range(D):                                   # upper clamp in one direction at a time, and just outside it
        p = rng.uniform(0, 1, D).astype(f32) * hi; p[d] = hi[d]; special.append(p)
        p = p.copy(); p[d] = hi[d] + f32(0.5); special.append(p)
    k = (n - len(special)) // 3
    ints = np.floor(rng.uniform(-3, 1, (k, D)) + rng.uniform(0, 1, (k, D)) * (hi + 4)).astype(f32)          # integers from −3 to Ng+1
    halves = ints[: k // 2] + f32(0.5)
    outside = (rng.uniform(-3, 3, (k, D)) + np.where(rng.uniform(0, 1, (k, D)) < 0.5, 0, hi)).astype(f32)   # within 3 cells of either end, both sides
    x = np.concatenate([np.array(special, dtype=f32), ints, halves, outside])
    inside = rng.uniform(0, 1, (n - len(x), D)).astype(f32) * hi
    x = np.concatenate([x, inside]).astype(f32)
    assert x.shape == (n, D)
    return x


def dev_interp(w, arr, x):
    import torch
    return w.interp(w.to_device(arr), torch.from_numpy(np.ascontiguousarray(x, dtype=f32)).to(w.core.device())).cpu().numpy()


def check_bound(dev, x, arr, what):
    r32, r64 = ir.interp(x, arr, np.float32), ir.interp(x, arr, np.float64)
    b = ir.bound(r32, r64, arr)
    err = float(np.abs(dev.astype(np.float64) - r64).max(initial=0.0))
    same = bool(np.array_equal(dev.view(np.uint32), r32.view(np.uint32)))
    print(f"[interp] {what}: n = {len(x)}, max|dev − ref64| = {err:.3e}, bound = {b:.3e}, bits equal to ref32: {same}")
    assert dev.shape == r32.shape and np.isfinite(dev).all()
    assert err <= b, (what, err, b)


def test_known_answers(w):
    """test/test_util.jl:3-14 in Float32"""
    a, b = ir.known_answer_arrays()
    rtol = float(np.sqrt(np.finfo(f32).eps))
    for point, name, expect in ir.KNOWN:
        got = dev_interp(w, {"a": a, "b": b}[name], np.array([point], dtype=f32))[0]
        assert np.allclose(got, np.asarray(expect, dtype=f32), rtol=rtol, atol=0.0), (point, name, got, expect)


@pytest.mark.parametrize("D", [3, 2])
@pytest.mark.parametrize("kind", ["scalar", "vector"])
@pytest.mark.parametrize("n", [257, 1, 0])
def test_random_fields(w, D, kind, n):
    Ng = GRIDS[D]
    rng = np.random.default_rng(100 * D + (kind == "vector"))
    arr = np.asfortranarray(rng.standard_normal(Ng + ((D,) if kind == "vector" else ())).astype(f32))
    x = point_set(Ng, 257, seed=7 + D)[:n]              # n = 1: the upper clamp corner itself (the first point of the set)
    assert x.shape == (n, D)
    dev = dev_interp(w, arr, x)
    check_bound(dev, x, arr, f"{D}-D {kind} n={n}")


@pytest.mark.parametrize("D", [3, 2])
def test_linear_fields_are_reproduced(w, D):
    Ng = GRIDS[D]
    rng = np.random.default_rng(3)
    I = np.indices(Ng).astype(np.float64)
    c = np.array([0.7, -1.3, 2.1][:D])
    lin = np.asfortranarray((sum(c[d] * I[d] for d in range(D)) + 0.4).astype(f32))
    hi = np.array(Ng, dtype=f32) - 2
    x = (rng.uniform(0, 1, (257, D)).astype(f32) * hi).astype(f32)
    x[0], x[1] = 0, hi                                   # both ends of the clamp range
    dev = dev_interp(w, lin, x)
    check_bound(dev, x, lin, f"{D}-D linear")
    want = sum(c[d] * (x[:, d].astype(np.float64) + 0.5) for d in range(D)) + 0.4      # 0-based index of x is x + 0.5
    # the field itself was rounded to float32 once per cell: eps32/2·max|lin| on top of the bound
    assert np.abs(dev - want).max() <= ir.bound(ir.interp(x, lin, np.float32), ir.interp(x, lin, np.float64), lin) + 0.5 * np.finfo(f32).eps * np.abs(lin).max()


def test_sim_sample_equals_interp_on_the_current_roles(w):
    import torch
    sg = w.FusedSimulation((16, 16, 16), (0.0, 0.0, 0.0), 16, U=1, nu=16 / 1600.0, ic="tgv")
    u_before = w.lib().wl_sim_field(sg._h, b"u")
    sg.mom_steps_(3)
    assert w.lib().wl_sim_field(sg._h, b"u") != u_before, "the array roles have rotated after 3 steps"
    x = torch.from_numpy(point_set(sg.Ng, 257, seed=11)).to(w.core.device())
    us, ps = sg.sample(x)
    ui, pi = w.interp(sg._view("u"), x), w.interp(sg._view("p"), x)
    assert torch.equal(us.view(torch.int32), ui.view(torch.int32)) and torch.equal(ps.view(torch.int32), pi.view(torch.int32))
    assert float(us.abs().max()) > 0.1 and float(ps.abs().max()) > 1e-3
    # either output alone: the same bits
    g = w._lib.wl_grid()
    w._lib.check(w.lib().wl_sim_grid(sg._h, C.byref(g)))
    only_p = torch.zeros_like(ps)
    w._lib.check(w.lib().wl_sim_sample(sg._h, C.c_void_p(x.data_ptr()), 257, None, C.c_void_p(only_p.data_ptr()), w.core.stream()))
    assert torch.equal(only_p.view(torch.int32), ps.view(torch.int32))
    # the leaf-level mirror samples the same numbers
    uh, ph = ir.interp(x.cpu().numpy(), sg.field("u")), ir.interp(x.cpu().numpy(), sg.field("p"))
    check_bound(us.cpu().numpy(), x.cpu().numpy(), sg.field("u"), "sample u")
    check_bound(ps.cpu().numpy(), x.cpu().numpy(), sg.field("p"), "sample p")
    assert uh.shape == (257, 3) and ph.shape == (257,)


def test_argument_checks(w):
    import torch
    L = w.lib()
    dev = w.core.device()
    Ng = GRIDS[3]
    arr = w.jl_zeros(Ng + (3,))
    x = torch.zeros((8, 3), dtype=torch.float32, device=dev)
    out = torch.zeros((8, 3), dtype=torch.float32, device=dev)
    g = w.core.grid_of(Ng)
    P, s = (lambda t: C.c_void_p(t.data_ptr())), w.core.stream()
    assert L.wl_interp(P(out), w.core.ptr(arr), C.byref(g), P(x), 8, 3, s) == 0
    assert L.wl_interp(P(out), w.core.ptr(arr), C.byref(g), P(x), 8, 1, s) == 0
    WL_EINVAL = -1
    for ncomp in (0, 2, 4):
        assert L.wl_interp(P(out), w.core.ptr(arr), C.byref(g), P(x), 8, ncomp, s) == WL_EINVAL, ncomp
    # the output inside the array, and the output on the points
    assert L.wl_interp(C.c_void_p(arr.data_ptr() + 64), w.core.ptr(arr), C.byref(g), P(x), 8, 3, s) == WL_EINVAL
    assert L.wl_interp(P(x), w.core.ptr(arr), C.byref(g), P(x), 8, 3, s) == WL_EINVAL
    # a z-slab grid
    slab = w._lib.wl_grid(3, Ng[0], Ng[1], Ng[2], 2, Ng[2] - 2, 0, Ng[2] + 3)      # the same memory read as the lower slab of a taller domain
    assert L.wl_interp(P(out), w.core.ptr(arr), C.byref(slab), P(x), 8, 3, s) == WL_EINVAL
    assert L.wl_advect(P(x), P(out), w.core.ptr(arr), w.core.ptr(arr), C.byref(slab), 8, 0.1, 0, s) == WL_EINVAL
    # n = 0 is legal and launches nothing
    l0 = L.wl_launch_count()
    assert L.wl_interp(None, w.core.ptr(arr), C.byref(g), None, 0, 3, s) == 0 and L.wl_launch_count() == l0
    w.lib().wl_stream_sync(s)
