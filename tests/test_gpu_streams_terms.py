"""The stream contract of include/wlhip.h for the separable terms: wl_accel_terms and wl_bc_vec_terms are asynchronous on the caller's stream,
wl_sim_set_terms copies the fields on its stream and synchronises it, a step with terms puts k_accel_terms and k_bc_vec_terms on the stream the step runs
on, and so does the BC! of wl_sim_init_flow.  The scenarios run once on the default stream and once on a delayed non-blocking side stream with the default
stream blocked (tests/stream_harness.py) and must produce the same bits.

The file's name makes it run after tests/test_gpu_streams.py (see tests/test_gpu_streams_interp.py for why that matters)."""
import ctypes as C

import numpy as np
import pytest

import terms_ref as tr
from stream_harness import Raw, Step, run_on_streams

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    yield w
    w.lib().wl_reset_process_options()


def checked(name, fn, host=None):
    def call(sp):
        rc = fn(sp)
        assert rc == 0, (name, rc)
        return host() if callable(host) else host
    return call


def test_leaves_on_caller_arrays(w):
    L = w.lib()
    shape, K = (34, 18, 10), 3

    def make():
        import torch
        F, r = tr.random_fields(shape, K, 11)
        Fd = [w.to_device(f) for f in F]
        rd, ad = w.to_device(r), w.to_device(r)
        g = w.core.grid_of(shape)
        Fp = (C.c_void_p * K)(*[w.core.ptr(f) for f in Fd])
        cp = (C.c_float * K)(*tr.coefficients(K, 3))
        torch.cuda.synchronize()
        P = w.core.ptr
        steps = [
            Step("wl_accel_terms", checked("wl_accel_terms", lambda sp: L.wl_accel_terms(P(rd), K, Fp, cp, C.byref(g), sp)), [rd] + Fd),
            Step("wl_bc_vec_terms", checked("wl_bc_vec_terms", lambda sp: L.wl_bc_vec_terms(P(ad), K, Fp, cp, C.byref(g), 0, 0, sp)), [ad] + Fd),
            Step("wl_bc_vec_terms", checked("wl_bc_vec_terms", lambda sp: L.wl_bc_vec_terms(P(rd), K, Fp, cp, C.byref(g), 1, 4, sp)), [rd] + Fd),
            Step("wl_accel_terms", checked("wl_accel_terms", lambda sp: L.wl_accel_terms(P(ad), 1, Fp, cp, C.byref(g), sp)), [ad, Fd[0]]),
        ]
        return steps, (Fd, rd, ad, Fp, cp, g)
    run_on_streams(L, make, label="terms leaves")


def test_set_terms_init_flow_and_steps_of_a_handle(w):
    L = w.lib()
    S = tr.Sheared

    def make():
        import torch
        sg = w.FusedSimulation(S.dims, (0, 0, 0), 16, U=1, nu=S.nu, perdir=S.perdir)
        h = sg._h
        g = w._lib.wl_grid()
        assert L.wl_sim_grid(h, C.byref(g)) == 0
        nc = g.nx * g.ny * g.nz
        host = [np.asfortranarray(f) for f in S.terms()]
        K = len(host)
        Fp = (C.c_void_p * K)(*[f.ctypes.data_as(C.c_void_p) for f in host])
        acc, b = (C.c_float * K)(*S.g_t), (C.c_float * K)(*S.b)
        torch.cuda.synchronize()
        flow = [Raw(nm, (lambda nm=nm: L.wl_sim_field(h, nm.encode())), nc * (1 if nm == "p" else 3)) for nm in ("u", "u0", "us", "f", "p")]
        terms = [Raw(f"term{k}", (lambda k=k: L.wl_sim_term(h, k)), nc * 3) for k in range(K)]

        def set_terms(sp):
            rc = L.wl_sim_set_terms(h, K, Fp, sp)
            return rc if rc != 0 else L.wl_sim_set_term_coeffs(h, acc, acc, b)

        def dts():
            return np.asarray(sg.dt, dtype=np.float32)
        steps = [
            Step("wl_sim_set_terms", checked("wl_sim_set_terms", set_terms), flow, sync=True),      # (the terms do not exist before the call)
            Step("wl_sim_init_flow", checked("wl_sim_init_flow", lambda sp: L.wl_sim_init_flow(h, sp)), flow + terms),      # BC!(u) from the terms, u⁰ = u
            Step("wl_sim_mom_step", checked("wl_sim_mom_step", lambda sp: L.wl_sim_mom_step(h, sp), dts), flow + terms, sync=True),
            Step("wl_sim_mom_steps", checked("wl_sim_mom_steps", lambda sp: L.wl_sim_mom_steps(h, 2, sp), dts), flow + terms, sync=True),
        ]
        return steps, (sg, host, Fp, acc, b)
    run_on_streams(L, make, label="terms on a handle")
