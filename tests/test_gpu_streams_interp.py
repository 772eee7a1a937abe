"""The stream contract of include/wlhip.h for the point-sample section: wl_interp, wl_advect and wl_sim_sample are asynchronous on the caller's
stream, and the probe and tracer launches of a step go to the stream the step runs on.  Each scenario runs once on the default stream and once
on a delayed non-blocking side stream with the default stream blocked (tests/stream_harness.py) and must produce the same bits.

The file's name makes it run after tests/test_gpu_streams.py.  The first armed run of a process makes torch create its pool of side streams, and the
runtime deals every later stream onto the hardware queue with the fewest streams: run earlier, this file changes which queue the communicator's own
stream of that file's wl_comm_halo_async row is dealt.  When that is the default stream's queue the row waits for the blocker and the run is "not armed"
(seen once: step 54 of the 34x18x10 leaf table).  pick_streams() probes the streams of the harness, not those the library owns."""
import ctypes as C

import numpy as np
import pytest

from stream_harness import Raw, Step, run_on_streams

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    yield w
    w.lib().wl_reset_process_options()


def P(t):
    return C.c_void_p(t.data_ptr())


def checked(name, fn, host=None):
    def call(sp):
        rc = fn(sp)
        assert rc == 0, (name, rc)
        return host() if callable(host) else host
    return call


@pytest.mark.parametrize("Ng", [(10, 9, 8), (12, 7)], ids=["10x9x8", "12x7"])
def test_leaves_keep_the_stream_contract(w, Ng):
    L = w.lib()

    def make():
        import torch
        rng = np.random.default_rng(17)
        D, n = len(Ng), 1000
        sca = w.to_device(np.asfortranarray(rng.standard_normal(Ng).astype(f32)))
        u0 = w.to_device(np.asfortranarray(rng.standard_normal(Ng + (D,)).astype(f32)))
        u1 = w.to_device(np.asfortranarray(rng.standard_normal(Ng + (D,)).astype(f32)))
        x = torch.from_numpy((rng.uniform(-0.2, 1.2, (n, D)) * (np.array(Ng) - 2)).astype(f32)).cuda()
        xp = torch.zeros_like(x)
        os_, ov = torch.zeros(n, dtype=torch.float32, device="cuda"), torch.zeros((n, D), dtype=torch.float32, device="cuda")
        g = w.core.grid_of(Ng)
        G = C.byref(g)
        torch.cuda.synchronize()
        steps = [
            Step("wl_interp", checked("wl_interp", lambda sp: L.wl_interp(P(os_), P(sca), G, P(x), n, 1, sp)), [sca, x, os_]),
            Step("wl_interp", checked("wl_interp", lambda sp: L.wl_interp(P(ov), P(u0), G, P(x), n, D, sp)), [u0, x, ov]),
            Step("wl_advect", checked("wl_advect", lambda sp: L.wl_advect(P(x), P(xp), P(u0), P(u1), G, n, 0.4, 1, sp)), [u0, u1, x, xp]),
        ]
        return steps, (g, sca, u0, u1, x, xp, os_, ov)
    run_on_streams(L, make, label=f"interp leaves {Ng}")


def test_sample_probes_and_tracers_of_a_handle(w):
    """wl_sim_sample between steps; wl_sim_mom_step and wl_sim_mom_steps(3) with 5 probes and 500 tracers registered: the flow arrays, the swarm
    and the records read back after each call"""
    L = w.lib()
    dims = (64, 32, 24)

    def make():
        import torch
        sg = w.FusedSimulation(dims, (0, 0, 0), dims[0], U=1, nu=dims[0] / 1600.0, ic="tgv")
        h = sg._h
        rng = np.random.default_rng(4)
        pts = (rng.uniform(0, 1, (5, 3)) * np.array(dims)).astype(f32)
        sg.set_probes(pts, capacity=8)
        sg.set_tracers((rng.uniform(0, 1, (500, 3)) * np.array(dims)).astype(f32))
        x = torch.from_numpy((rng.uniform(-0.1, 1.1, (300, 3)) * np.array(dims)).astype(f32)).cuda()
        us, ps = torch.zeros((300, 3), dtype=torch.float32, device="cuda"), torch.zeros(300, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        g = w._lib.wl_grid()
        assert L.wl_sim_grid(h, C.byref(g)) == 0
        nc = g.nx * g.ny * g.nz
        arrays = [Raw(nm, (lambda nm=nm: L.wl_sim_field(h, nm.encode())), nc * (1 if nm == "p" else 3)) for nm in ("u", "u0", "us", "p")]
        arrays += [Raw("tracers", lambda: L.wl_sim_tracers(h, 0, None), 1500), Raw("tracers0", lambda: L.wl_sim_tracers(h, 1, None), 1500)]

        def records():
            t, ru, rp = sg.read_probes()
            return (t, ru, rp)
        steps = [
            Step("wl_sim_mom_step", checked("wl_sim_mom_step", lambda sp: L.wl_sim_mom_step(h, sp), records), arrays, sync=True),
            Step("wl_sim_sample", checked("wl_sim_sample", lambda sp: L.wl_sim_sample(h, P(x), 300, P(us), P(ps), sp)), arrays + [x, us, ps]),
            Step("wl_sim_mom_steps", checked("wl_sim_mom_steps", lambda sp: L.wl_sim_mom_steps(h, 3, sp), records), arrays, sync=True),
            Step("wl_sim_sample", checked("wl_sim_sample", lambda sp: L.wl_sim_sample(h, P(x), 300, P(us), None, sp)), arrays + [x, us, ps]),
        ]
        return steps, (sg, x, us, ps)
    run_on_streams(L, make, label="sim sample, probes, tracers")
