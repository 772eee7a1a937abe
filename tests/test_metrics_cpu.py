"""Flow diagnostics (src/Metrics.jl:27-109) without a GPU: the NumPy yardstick (tests/metrics_ref.py) reproduces the reference's own known
answers (test/test_metrics.jl:3-30) and three analytic λ₂ cases, and the C ABI / Python surface of the device implementation exists."""
import os
import re

import numpy as np
import pytest

import metrics_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
J = (0, 1, 2)                                   # CartesianIndex(2,3,4) as an index into the inside-cell arrays of a (3,4,5) grid
X = np.array([0.5, 1.5, 2.5])                   # loc(0,J)
PX = float(np.prod(X))
NEW_SYMBOLS = ("wl_ke", "wl_curl", "wl_omega", "wl_omega_mag", "wl_omega_theta", "wl_lambda2", "wl_helicity", "wl_flow_fields", "wl_flow_stats",
               "wl_sim_flow_stats", "wl_sim_flow_fields")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_known_answers(dtype):
    """test/test_metrics.jl:8-23 on the yardstick"""
    u = mr.kat_u(dtype)
    assert mr.ke(u, dtype=dtype)[J] == 0.5 * np.sum((X + PX) ** 2) == 18.0859375
    assert mr.ke(u, X, dtype=dtype)[J] == 1.5 * PX ** 2
    assert abs(mr.lambda2(u, dtype)[J] - 1) <= np.sqrt(np.finfo(dtype).eps)
    w = np.array(mr._cross(list(1 / X), [PX] * 3))                       # ω = (1 ./ x) × repeat([px],3)
    assert np.allclose(w, (0.5, -3, 2.5))
    assert mr.curl(2, u, dtype)[J] == w[1]
    assert np.array_equal(mr.omega(u, dtype)[J], w.astype(dtype))
    assert mr.omega_mag(u, dtype)[J] == np.sqrt(np.sum(w.astype(dtype) ** 2, dtype=dtype))
    assert np.isclose(mr.omega_theta(u, (0, 0, 1), X + (0, 1, 2), dtype)[J], w[0], rtol=np.sqrt(np.finfo(dtype).eps))
    if dtype == np.float32:
        assert mr.lambda2(u, dtype)[J] == 1.0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_helicity_known_answer(dtype):
    """test/test_metrics.jl:25-30: I = (3,3,3) of 6³, helicity == umid·ωmid with umid = loc(0,I)[1], ωmid = loc(0,I)[2]+1"""
    u, w = mr.kat_helicity(dtype)
    h = mr.helicity(u, w, dtype)
    assert h.dtype == dtype and h[1, 1, 1] == 1.5 * (1.5 + 1)


def test_analytic_lambda2():
    Ng = (7, 8, 9)
    w, a, c = 0.7, 1.3, 0.45
    l2 = mr.lambda2(mr.analytic_u("rotation", Ng, w, np.float64))
    assert np.abs(l2 + w * w).max() < 1e-13                              # degenerate pair −w², −w², 0
    l2 = mr.lambda2(mr.analytic_u("shear", Ng, a, np.float64))
    assert np.abs(l2).max() < 1e-13                                      # A ≡ 0
    assert np.abs(mr.lambda2_matrix(mr.analytic_u("shear", Ng, a, np.float64))).max() < 1e-13
    l2 = mr.lambda2(mr.analytic_u("expansion", Ng, c, np.float64))
    assert np.abs(l2 - c * c).max() < 1e-13


def test_two_dimensional_forms():
    rng = np.random.default_rng(3)
    u = rng.standard_normal((6, 7, 2))
    k = mr.ke(u, (0.25, -0.5))
    I = (2, 3)
    assert np.isclose(k[I[0] - 1, I[1] - 1], 0.125 * ((u[2, 3, 0] + u[3, 3, 0] - 0.5) ** 2 + (u[2, 3, 1] + u[2, 4, 1] + 1.0) ** 2))
    c = mr.curl(3, u)
    assert np.isclose(c[I[0] - 1, I[1] - 1], (u[2, 3, 1] - u[1, 3, 1]) - (u[2, 3, 0] - u[2, 2, 0]))


def test_surface():
    import waterlily_jl_amd as w
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wlhip.h"), encoding="utf-8").read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/wlhip.h"
        assert name in w.SIGNATURES, name
        assert hasattr(w.lib(), name), name
    for fn in ("ke_", "curl_", "omega_", "omega_mag_", "omega_theta_", "lambda2_", "helicity_", "flow_fields_", "flow_stats"):
        assert callable(getattr(w, fn)), fn
    for cls in (w.FusedSimulation, w.Simulation):
        assert callable(getattr(cls, "flow_stats")) and callable(getattr(cls, "metric"))
    src = open(os.path.join(ROOT, "waterlily.jl_amd", "julia", "WaterLilyHIPExt.jl"), encoding="utf-8").read()
    for name in NEW_SYMBOLS[:7] + ("wl_flow_stats",):
        assert f"(:{name}, libwlhip)" in src, f"the Julia binding has no method on {name}"
