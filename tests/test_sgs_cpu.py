"""sgs! (Smagorinsky–Lilly): the NumPy yardstick of tests/sgs_ref.py pinned analytically in float64, and the public surface the feature
adds (no GPU needed)."""
import inspect
import os
import re

import numpy as np

import sgs_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS, DELTA = 0.17, 1.3


def _shear_field(Ng, fn):
    """u = (fn(y),0,0) with y = loc(1,I)[2] = J-1.5 (Julia index J): the x-face sits at the cell's y-centre   src/core.jl:177"""
    u = np.zeros(Ng + (3,), order="F")
    y = np.arange(Ng[1]) + 1 - 1.5
    u[..., 0] = fn(y)[None, :, None]
    return u, y


def _deep(Ng):
    """cells at least two cells from every wall (0-based 2 .. n-3)"""
    return tuple(slice(2, n - 2) for n in Ng)


def test_linear_shear_gives_constant_nut_and_no_force():
    """u = (a·y,0,0): ∂(1,2) = (2a(y+1) − 2a(y−1))/4 = a, S₁₂ = S₂₁ = a/2, S:S = a²/2, νₜ = (CsΔ)²·|a|/√2; σ₁₂ = −νₜ·a is uniform, so
    f[I,1] += σ₁₂[I] − σ₁₂[I+δ₂] = 0 away from the walls"""
    Ng, a = (12, 14, 10), -0.37
    u, _ = _shear_field(Ng, lambda y: a * y)
    S = sgs_ref.strain(u)
    ins = tuple(slice(1, n - 1) for n in Ng)
    assert np.abs(S[ins + (0, 1)] - a / 2).max() < 1e-12 and np.abs(S[ins + (1, 0)] - a / 2).max() < 1e-12
    assert np.abs(S[ins + (0, 0)]).max() == 0 and np.abs(S[ins + (2, 2)]).max() == 0
    f0 = np.zeros(Ng + (3,), order="F")
    f, sig, nut = sgs_ref.sgs(f0, u, CS, DELTA)
    assert np.abs(nut[ins] - (CS * DELTA) ** 2 * abs(a) / np.sqrt(2)).max() < 1e-12
    ghost = np.ones(Ng, bool); ghost[ins] = False
    assert np.all(nut[ghost] == 0)                      # νₜ ≡ 0 on the ghost layer
    assert np.abs(f[_deep(Ng)]).max() < 1e-12


def test_quadratic_shear_matches_the_closed_form():
    """u = (b·y²,0,0), y > 0 on every inside cell: ∂(1,2) = 2b((y+1)²−(y−1)²)/4 = 2by, S₁₂ = by, νₜ(y) = (CsΔ)²·√2·|b|·y;
    σ₁₂(y) = −νₜ(y)·b·(y²−(y−1)²) = −νₜ(y)·b·(2y−1), and
    f[I,1] = σ₁₂(y) − σ₁₂(y+1) = (CsΔ)²√2|b|b·[(y+1)(2y+1) − y(2y−1)] = (CsΔ)²√2|b|b·(4y+1); every other sweep and component gives 0"""
    Ng, b = (10, 16, 12), 0.013
    u, y = _shear_field(Ng, lambda y: b * y * y)
    f0 = np.zeros(Ng + (3,), order="F")
    f, sig, nut = sgs_ref.sgs(f0, u, CS, DELTA)
    c2 = (CS * DELTA) ** 2
    ins = tuple(slice(1, n - 1) for n in Ng)
    assert np.abs(nut[ins] - (c2 * np.sqrt(2) * abs(b) * y[1:-1])[None, :, None]).max() < 1e-12
    expect = (c2 * np.sqrt(2) * abs(b) * b * (4 * y + 1))[None, :, None]
    d = _deep(Ng)
    assert np.abs(f[d + (0,)] - np.broadcast_to(expect, Ng)[d]).max() < 1e-12
    assert np.abs(f[d + (1,)]).max() < 1e-12 and np.abs(f[d + (2,)]).max() < 1e-12


def test_sweeps_touch_only_inside_u_and_float32_follows_float64():
    """the lower ghost layer of f (Julia index 1) lies in no sweep's range, and ghost cells of f only ever receive ±0 (νₜ = 0 there)"""
    rng = np.random.default_rng(3)
    Ng = (9, 11, 10)
    u = np.stack([sgs_ref.smooth_field(Ng, rng) for _ in range(3)], -1)
    f0 = rng.standard_normal(Ng + (3,))
    f, _, _ = sgs_ref.sgs(f0, u, CS, DELTA)
    ghost = np.ones(Ng, bool); ghost[tuple(slice(1, n - 1) for n in Ng)] = False
    assert np.array_equal(f[ghost], f0[ghost])
    assert np.abs(f - f0).max() > 1e-4
    f32, _, _ = sgs_ref.sgs(f0, u, CS, DELTA, dtype=np.float32)
    assert f32.dtype == np.float32 and np.abs(f32 - f).max() < 1e-5


def test_public_surface_declares_the_model():
    hdr = open(os.path.join(ROOT, "include", "wlhip.h")).read()
    assert re.search(r"\bint\s+wl_sgs\s*\(\s*float\*\s*f,\s*float\*\s*sigma,\s*const float\*\s*u,\s*const wl_grid\*\s*g,\s*float Cs,\s*float Delta,\s*void\*\s*stream\)", hdr)
    assert re.search(r"\bint\s+wl_sim_set_sgs\s*\(\s*wl_sim\*\s*s,\s*int model,\s*float Cs,\s*float Delta\)", hdr)
    import waterlily_jl_amd as w
    from waterlily_jl_amd import flow
    assert "wl_sgs" in w.SIGNATURES and "wl_sim_set_sgs" in w.SIGNATURES
    for fn in (flow.mom_step_, flow.mom_predict_, flow.mom_correct_, w.Simulation.sim_step_):
        assert "udf" in inspect.signature(fn).parameters, fn
    assert hasattr(w.FusedSimulation, "set_sgs") and callable(w.sgs_) and callable(w.udf_)


def test_udf_dispatch_by_positional_arity():
    """src/Flow.jl:255-257: force!(flow,u,t; kw...) if it takes three positionals, else force!(flow,t; kw...)"""
    from waterlily_jl_amd.flow import udf_
    seen = []
    udf_("a", None, "u", 1.0)
    udf_("a", lambda flow, u, t, **kw: seen.append((3, flow, u, t, kw)), "u", 1.0, g=2)
    udf_("a", lambda flow, t, g=0.5: seen.append((2, flow, t, g)), "u", 1.0, g=2)
    assert seen == [(3, "a", "u", 1.0, {"g": 2}), (2, "a", 1.0, 2)]
