"""interp (src/util.jl:17-43) without a GPU: the NumPy yardstick (tests/interp_ref.py) reproduces the reference's own known answers
(the Float32 analogue of test/test_util.jl:3-14), and the C ABI / Python surface of the device implementation exists."""
import os
import re

import numpy as np
import pytest

import interp_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("wl_interp", "wl_sim_sample", "wl_sim_set_probes", "wl_sim_read_probes", "wl_advect", "wl_sim_set_tracers", "wl_sim_tracers")
RTOL = float(np.sqrt(np.finfo(np.float32).eps))      # Julia's ≈ for Float32


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("point,name,expect", ir.KNOWN, ids=[f"{n}{p}" for p, n, _ in ir.KNOWN])
def test_reference_known_answers(dtype, point, name, expect):
    a, b = ir.known_answer_arrays()
    got = ir.interp(np.array([point], dtype=np.float32), {"a": a, "b": b}[name], dtype)[0]
    assert got.dtype == dtype
    assert np.allclose(got, np.asarray(expect, dtype=dtype), rtol=RTOL, atol=0.0), (point, name, got, expect)


def test_known_answer_arrays_are_the_reference_ones():
    """apply!((i,x)->x[i], a): a[I,i] = loc(i,I)[i]; apply!(x->x[1], b): b[I] = loc(0,I)[1]   src/core.jl:177 (Julia I is 1-based)"""
    a, b = ir.known_answer_arrays()
    assert a.shape == (8, 8, 2) and b.shape == (8, 8) and a.dtype == b.dtype == np.float32
    assert a[3, 5, 0] == 4 - 1.5 - 0.5 and a[3, 5, 1] == 6 - 1.5 - 0.5 and b[3, 5] == 4 - 1.5


def test_yardstick_clamps_and_is_exact_on_linear_fields():
    rng = np.random.default_rng(5)
    Ng = (7, 6, 5)
    I = np.indices(Ng).astype(np.float32)
    lin = (0.5 * I[0] - 0.25 * I[1] + 2.0 * I[2] + 1.0).astype(np.float32)      # exactly representable: the float32 chain makes no rounding error worth the name
    x = rng.uniform(0, 1, (64, 3)).astype(np.float32) * (np.array(Ng, dtype=np.float32) - 2)
    want = 0.5 * (x[:, 0] + 0.5) - 0.25 * (x[:, 1] + 0.5) + 2.0 * (x[:, 2] + 0.5) + 1.0      # index = x + 1.5 − 1
    assert np.allclose(ir.interp(x, lin, np.float64), want, rtol=0, atol=1e-5)
    assert np.allclose(ir.interp(x, lin, np.float32), want, rtol=0, atol=1e-5)
    far = np.array([[-3.0, 100.0, np.float32(Ng[2] - 2)]], dtype=np.float32)
    assert ir.interp(far, lin, np.float32)[0] == ir.interp(np.array([[0.0, Ng[1] - 2, Ng[2] - 2]], dtype=np.float32), lin, np.float32)[0]


def test_yardstick_particle_step():
    """uniform flow: every particle moves by Δt·U; x_prev is the old x; a periodic coordinate comes back into [0, N)"""
    Ng = (10, 8, 6)
    u = np.zeros(Ng + (3,), dtype=np.float32)
    u[..., 0] = 1.0
    x = np.array([[1.0, 2.0, 3.0], [7.75, 0.5, 1.0]], dtype=np.float32)
    xn, xp = ir.advect(x, u, u, 0.5, perdir=(1,))
    assert np.array_equal(xp, x) and xn.dtype == np.float32
    assert np.array_equal(xn, np.array([[1.5, 2.0, 3.0], [0.25, 0.5, 1.0]], dtype=np.float32))


def test_package_exports_the_new_surface():
    import waterlily_jl_amd as w
    assert callable(w.interp_) and callable(w.interp) and callable(w.advect_)
    for name in ("sample", "set_probes", "read_probes", "set_tracers", "tracers"):
        assert callable(getattr(w.FusedSimulation, name)), name
    assert callable(w.Simulation.sample)
    for sym in NEW_SYMBOLS:
        assert sym in w.SIGNATURES, sym


def test_header_declares_the_new_functions():
    hdr = open(os.path.join(ROOT, "include", "wlhip.h"), encoding="utf-8").read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b(?:int|float\s*\*)\s+" + sym + r"\s*\(", hdr), sym
    assert "src/util.jl:17-43" in open(os.path.join(ROOT, "include", "wlhip.h"), encoding="utf-8").read()


def test_stream_entry_points_of_the_section_have_scenarios():
    """the three new entry points that take a stream have their stream-contract scenarios in tests/test_gpu_streams_interp.py (a leaf row each,
    the handle call in a step of a handle scenario) — the rule tests/test_stream_contract_cpu.py keeps for the rest of the header"""
    src = open(os.path.join(ROOT, "tests", "test_gpu_streams_interp.py"), encoding="utf-8").read()
    for sym in ("wl_interp", "wl_advect", "wl_sim_sample", "wl_sim_mom_steps", "wl_sim_mom_step"):
        assert re.search(r"Step\(\s*\"" + sym + r"\"", src), sym
