"""The stream contract of include/wlhip.h for the force history: the band and finish launches of a step go to the stream the step runs on, a
remeasure rebuilds the recorder's list on the caller's stream, and wl_sim_forces_bodyset runs on — and synchronises — its stream.  Each scenario runs
once on the default stream and once on a delayed non-blocking side stream with the default stream blocked (tests/stream_harness.py) and must produce
the same bits: the flow arrays after every call, the records read back and the twelve numbers returned.

The file's name makes it run after tests/test_gpu_streams.py (see tests/test_gpu_streams_interp.py for why that matters)."""
import ctypes as C

import numpy as np
import pytest

import forces_ref as fr
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


def test_force_records_and_read_outs_of_a_handle(w):
    L = w.lib()
    c = fr.case("sphere_inside")
    moved = w.Body(("sphere", (24.3, 13.1, 11.7), 5.0))

    def make():
        import torch
        sg = w.FusedSimulation(c["dims"], c["uBC"], c["L"], U=1, nu=c["nu"], has_body=True)
        sg.set_body(c["body"])
        sg.set_force_record(c["body"], x0=c["x0"], capacity=8)
        h = sg._h
        torch.cuda.synchronize()
        g = w._lib.wl_grid()
        assert L.wl_sim_grid(h, C.byref(g)) == 0
        nc = g.nx * g.ny * g.nz
        arrays = [Raw(nm, (lambda nm=nm: L.wl_sim_field(h, nm.encode())), nc * (1 if nm == "p" else 3)) for nm in ("u", "u0", "us", "p")]
        prog, prog2 = c["body"].program(3), moved.program(3)
        x0 = (C.c_float * 3)(*c["x0"])
        outs = [(C.c_double * 12)() for _ in range(2)]

        def records():
            return tuple(sg.read_forces()) + (sg.counter("force_tiles"),)
        steps = [
            Step("wl_sim_mom_step", checked("wl_sim_mom_step", lambda sp: L.wl_sim_mom_step(h, sp), records), arrays, sync=True),
            Step("wl_sim_forces_bodyset", checked("wl_sim_forces_bodyset", lambda sp: L.wl_sim_forces_bodyset(h, x0, C.byref(prog), outs[0], sp), lambda: outs[0]), arrays, sync=True),
            Step("wl_sim_mom_steps", checked("wl_sim_mom_steps", lambda sp: L.wl_sim_mom_steps(h, 3, sp), records), arrays, sync=True),
            Step("wl_sim_measure_bodyset", checked("wl_sim_measure_bodyset", lambda sp: L.wl_sim_measure_bodyset(h, C.byref(prog2), 1.0, sp)), arrays, sync=True),
            Step("wl_sim_mom_step", checked("wl_sim_mom_step", lambda sp: L.wl_sim_mom_step(h, sp), records), arrays, sync=True),
            Step("wl_sim_forces_bodyset", checked("wl_sim_forces_bodyset", lambda sp: L.wl_sim_forces_bodyset(h, None, C.byref(prog2), outs[1], sp), lambda: outs[1]), arrays, sync=True),
        ]
        return steps, (sg, prog, prog2, x0, outs)
    run_on_streams(L, make, label="force records and read-outs")
