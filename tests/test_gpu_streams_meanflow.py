"""The stream contract of include/wlhip.h for the mean-flow observer: wl_sim_set_meanflow and wl_sim_meanflow_reset zero the averages on the caller's stream,
the update of a step goes to the stream the step runs on, wl_sim_meanflow_update and wl_sim_meanflow_uu are asynchronous on theirs.  The scenario runs once on
the default stream and once on a delayed non-blocking side stream with the default stream blocked (tests/stream_harness.py) and must produce the same bits:
the flow arrays, the averages and the expanded tensor after every call, and the time vector read back.

The file's name makes it run after tests/test_gpu_streams.py (see tests/test_gpu_streams_interp.py for why that matters)."""
import ctypes as C

import numpy as np
import pytest

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


def test_set_step_update_and_expansion_of_a_handle(w):
    L = w.lib()
    dims = (64, 32, 24)

    def make():
        import torch
        sg = w.FusedSimulation(dims, (0, 0, 0), dims[0], U=1, nu=dims[0] / 1600.0, ic="tgv")
        h = sg._h
        g = w._lib.wl_grid()
        assert L.wl_sim_grid(h, C.byref(g)) == 0
        nc = g.nx * g.ny * g.nz
        out = w.jl_zeros(sg.Ng + (3, 3))
        torch.cuda.synchronize()
        P = w.core.ptr
        flow = [Raw(nm, (lambda nm=nm: L.wl_sim_field(h, nm.encode())), nc * (1 if nm == "p" else 3)) for nm in ("u", "u0", "us", "p")]
        mean = [Raw(nm, (lambda q=q: L.wl_sim_meanflow(h, q, None)), nc * k) for q, (nm, k) in enumerate((("P", 1), ("U", 3), ("UU", 6)))]
        every = flow + mean + [out]

        def tvec():
            return np.asarray(sg.meanflow_t(), dtype=np.float32)
        steps = [
            Step("wl_sim_set_meanflow", checked("wl_sim_set_meanflow", lambda sp: L.wl_sim_set_meanflow(h, 2, 2, 0.0, sp)), flow),      # (the averages do not exist before the call)
            Step("wl_sim_meanflow_uu", checked("wl_sim_meanflow_uu", lambda sp: L.wl_sim_meanflow_uu(h, P(out), 0, sp)), every),         # reads the zero fill behind the call that queued it
            Step("wl_sim_mom_steps", checked("wl_sim_mom_steps", lambda sp: L.wl_sim_mom_steps(h, 3, sp), tvec), every, sync=True),      # the observer updates after step 2
            Step("wl_sim_meanflow_update", checked("wl_sim_meanflow_update", lambda sp: L.wl_sim_meanflow_update(h, sp), tvec), every),
            Step("wl_sim_meanflow_uu", checked("wl_sim_meanflow_uu", lambda sp: L.wl_sim_meanflow_uu(h, P(out), 1, sp)), every),
            Step("wl_sim_mom_step", checked("wl_sim_mom_step", lambda sp: L.wl_sim_mom_step(h, sp), tvec), every, sync=True),            # step 4: an update
            Step("wl_sim_meanflow_reset", checked("wl_sim_meanflow_reset", lambda sp: L.wl_sim_meanflow_reset(h, 1.5, sp), tvec), every),
            Step("wl_sim_meanflow_update", checked("wl_sim_meanflow_update", lambda sp: L.wl_sim_meanflow_update(h, sp), tvec), every),
        ]
        return steps, (sg, out)
    run_on_streams(L, make, label="mean-flow observer")
