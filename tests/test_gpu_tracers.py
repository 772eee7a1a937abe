"""Tracer particles (wl_advect, wl_sim_set_tracers; csrc/wl_interp.hip): the leaf against the Float32 restatement of tests/interp_ref.py, the
swarm a handle advances after every step — uniform flow, periodic wrap, a flow that does not notice — and the assumption the handle's launch
rests on: after a step the array in the u⁰ role holds the velocity the step started from."""
import numpy as np
import pytest

import interp_ref as ir

pytestmark = pytest.mark.gpu
f32 = np.float32
EPS = float(np.finfo(f32).eps)


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    yield w
    w.lib().wl_reset_process_options()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def seeds(dims, n, seed=9, spread=0.0):
    rng = np.random.default_rng(seed)
    d = np.array(dims, dtype=f32)
    return (rng.uniform(-spread, 1 + spread, (n, len(dims))).astype(f32) * d).astype(f32)


@pytest.mark.parametrize("perdir", [(), (1, 3)], ids=["free", "periodic_xz"])
def test_advect_against_the_restatement(w, perdir):
    """two random velocity fields on 12×10×9, 257 particles some of which leave the domain.  Bound: the interp bound applied through the two stages —
    per coordinate |dev − ref64| ≤ 4·max|ref32 − ref64| over the particles, floor 4·eps32·max|x|: the Float32 chain's own distance from the Float64 one"""
    import torch
    Ng = (12, 10, 9)
    rng = np.random.default_rng(21)
    u0 = np.asfortranarray(rng.standard_normal(Ng + (3,)).astype(f32))
    u1 = np.asfortranarray(rng.standard_normal(Ng + (3,)).astype(f32))
    x = seeds(tuple(n - 2 for n in Ng), 257, spread=0.3)
    dt = f32(0.8)
    r32, p32 = ir.advect(x, u0, u1, dt, perdir, np.float32)
    r64, _ = ir.advect(x, u0, u1, dt, perdir, np.float64)
    inside = np.all((r32 >= 0) & (r32 <= np.array(Ng, dtype=f32) - 2), axis=1)
    assert 0 < inside.sum() < 257 or perdir, "some particles end outside the domain, some inside"
    xd = torch.from_numpy(x.copy()).to(w.core.device())
    xp = torch.full_like(xd, -7.0)
    w.advect_(xd, xp, w.to_device(u0), w.to_device(u1), dt, perdir)
    got, gotp = xd.cpu().numpy(), xp.cpu().numpy()
    assert np.array_equal(bits(gotp), bits(x)), "x_prev is the old x exactly"
    assert np.array_equal(bits(p32), bits(x))
    same = bool(np.array_equal(bits(got), bits(r32)))
    # a wrapped coordinate may sit on the other side of the seam in the two precisions: compare on the circle
    diff = np.abs(got.astype(np.float64) - r64)
    for j in perdir:
        N = Ng[j - 1] - 2
        diff[:, j - 1] = np.minimum(diff[:, j - 1], N - diff[:, j - 1])
    d32 = np.abs(r32.astype(np.float64) - r64)
    for j in perdir:
        N = Ng[j - 1] - 2
        d32[:, j - 1] = np.minimum(d32[:, j - 1], N - d32[:, j - 1])
    bound = max(4.0 * float(d32.max()), 4.0 * EPS * float(np.abs(x).max()))
    print(f"[advect] perdir={perdir}: max|dev − ref64| = {diff.max():.3e}, bound = {bound:.3e}, bits equal to ref32: {same}")
    assert np.isfinite(got).all() and diff.max() <= bound, (diff.max(), bound)
    for j in perdir:
        assert (got[:, j - 1] >= 0).all() and (got[:, j - 1] < Ng[j - 1] - 2).all()


def test_uniform_flow_moves_every_tracer_by_the_time_stepped(w):
    dims = (16, 16, 16)
    sg = w.FusedSimulation(dims, (1.0, 0.0, 0.0), 16, U=1, nu=0.01, ic="uBC")
    x = seeds(dims, 300, seed=3)
    x[:, 0] *= f32(0.5)                                       # room to move downstream
    sg.set_tracers(x)
    x0, xp0 = sg.tracers()
    assert np.array_equal(bits(x0.cpu().numpy()), bits(x)) and np.array_equal(bits(xp0.cpu().numpy()), bits(x))
    sg.mom_steps_(3)
    for _ in range(3):
        sg.mom_step_()
    dts = np.asarray(sg.dt, dtype=np.float64)
    assert len(dts) == 7
    moved = dts[:6].sum()                                     # six steps: Δt[0..5]
    xn, xp = (t.cpu().numpy() for t in sg.tracers())
    tol = 6 * EPS * float(np.abs(xn).max())
    assert np.abs(xn[:, 0].astype(np.float64) - (x[:, 0].astype(np.float64) + moved)).max() <= tol
    assert np.array_equal(bits(xn[:, 1:]), bits(x[:, 1:])), "y and z are unchanged, bit for bit"
    assert np.abs(xn[:, 0].astype(np.float64) - xp[:, 0] - dts[5]).max() <= tol and np.array_equal(bits(xp[:, 1:]), bits(x[:, 1:]))


def test_periodic_directions_wrap(w):
    dims = (16, 16, 16)
    sg = w.FusedSimulation(dims, (0.0, 0.0, 0.0), 16, U=1, nu=16 / 1600.0, perdir=(1, 2, 3), ic="tgv_periodic")
    x = seeds(dims, 400, seed=5)
    x[:40] = np.where(np.arange(120).reshape(40, 3) % 2 == 0, f32(1e-4), f32(16 - 1e-4))      # particles next to the seam, on both sides
    sg.set_tracers(x)
    sg.mom_steps_(8)
    xn, xp = (t.cpu().numpy() for t in sg.tracers())
    assert np.isfinite(xn).all() and (xn >= 0).all() and (xn < 16).all()
    assert (xp >= 0).all() and (xp < 16).all()
    step = np.abs(xn - xp); step = np.minimum(step, 16 - step)
    assert 1e-3 < step.max() < 1.0, step.max()             # they moved, by less than a cell per step (CFL)


FUSED = dict(tailfuse=1, resjac_min=0, convt_min=0)


@pytest.mark.parametrize("dims,opts", [((16, 16, 16), {}), ((32, 32, 32), FUSED), ((64, 32, 24), FUSED)], ids=["tgv16", "tgv32_fused", "tgv64x32x24_fused"])
def test_u0_role_and_a_flow_that_does_not_notice(w, dims, opts):
    """after a step wl_sim_field("u0") holds the previous step's final u; a handle with tracers has the bits of one without; and the swarm is the one
    wl_advect produces from those two arrays and the step's Δt"""
    import torch

    def make():
        sg = w.FusedSimulation(dims, (0.0, 0.0, 0.0), dims[0], U=1, nu=dims[0] / 1600.0, ic="tgv")
        for k, v in opts.items():
            sg.set_option(k, v)
        return sg
    A, Cc = make(), make()
    x = seeds(dims, 257, seed=8, spread=0.05)
    A.set_tracers(x)
    A.mom_steps_(2); Cc.mom_steps_(2)
    u_prev = A.field("u")
    x_before = A.tracers()[0].cpu().numpy().copy()
    A.mom_step_(); Cc.mom_step_()
    assert np.array_equal(bits(A.field("u0")), bits(u_prev)), "u⁰ role after a single step"
    # the handle's launch = the leaf on (u⁰, u, Δt of that step)
    xd = torch.from_numpy(x_before.copy()).to(w.core.device()); xpd = torch.empty_like(xd)
    w.advect_(xd, xpd, A._view("u0"), A._view("u"), A.dt[-2])
    xn, xp = A.tracers()
    assert torch.equal(xn.view(torch.int32), xd.view(torch.int32)) and np.array_equal(bits(xp.cpu().numpy()), bits(x_before))
    u_prev = A.field("u")
    A.mom_steps_(3); Cc.mom_steps_(3)                        # inside a multi-step call: compare with a handle stepped 2 + 1 + 2
    B = make(); B.mom_steps_(2); B.mom_step_(); B.mom_steps_(2)
    u_mid = B.field("u")
    B.mom_step_()
    assert np.array_equal(bits(A.field("u0")), bits(u_mid)), "u⁰ role after the last step of a multi-step call"
    for name in ("u", "u0", "p"):
        assert np.array_equal(bits(A.field(name)), bits(Cc.field(name))), name
        assert np.array_equal(bits(A.field(name)), bits(B.field(name))), name
    assert [f32(v).view(np.uint32) for v in A.dt] == [f32(v).view(np.uint32) for v in Cc.dt]
    assert not np.array_equal(bits(A.field("u")), bits(u_prev))
