"""The stream contract of include/wlhip.h for band-limited baking: the scenario of tests/test_gpu_streams_meshvel.py with wl_sdf_lattice_from_mesh_band as the
creating step.  wl_sdf_lattice_from_mesh_band and wl_sdf_lattice_update_mesh (which keeps the band) upload their tables, launch
the search and read the samples back on the caller's stream and synchronise that stream — an update is ordered behind a measure! queued on the same stream
that still reads the lattice; wl_sdf_lattice_set_velocity and wl_sdf_lattice_read_velocity copy on the caller's stream and synchronise it; the lattice is
measured on the caller's stream like any other.  The scenario runs once on the default stream and once on a delayed non-blocking side stream with the
default stream blocked (tests/stream_harness.py) and must produce the same bits.  (The file's name makes it run after tests/test_gpu_streams.py: see
tests/test_gpu_streams_interp.py.)"""
import ctypes as C
import gc

import numpy as np
import pytest

import meshsdf_ref as mr
import meshvel_ref as mv
from stream_harness import Step, run_on_streams

pytestmark = pytest.mark.gpu
f32 = np.float32
BAND = 2.0 + 1.0 + 1.0 + 3.0 ** 0.5 + 0.25      # mesh_band(): a quarter cell above measure!'s band rule


@pytest.fixture(scope="module")
def w():
    import waterlily_jl_amd as w
    w.core.device()
    yield w
    w.lib().wl_reset_process_options()


class Holder:
    """a lattice created by the scenario itself; destroyed with the scenario"""

    def __init__(self, L):
        self.L, self.h = L, C.c_void_p()

    def __del__(self):
        if self.h:
            self.L.wl_sdf_lattice_destroy(self.h)


def test_banded_mesh_update_and_velocity_calls_keep_the_stream_contract(w):
    L = w.lib()
    c = mr.case("ico320")
    V = np.ascontiguousarray(c["V"] + np.array([3.0, 2.0, 1.5], f32))
    E = np.ascontiguousarray(c["E"], dtype=np.int32)
    Wv = np.ascontiguousarray(mv.rotation(V, centre=(13.0, 12.0, 11.0)))
    V1 = np.ascontiguousarray(mv.breathing(V, (13.3, 12.1, 11.3), 3))
    W1 = np.ascontiguousarray(mv.linear(V))
    dims, origin = w.bodies.mesh_placement(V, 1.0, 5.5)
    count = int(np.prod(dims))
    Wset = np.ascontiguousarray(mv.linear_W(dims, origin, 1.0, mv._A, (0.1, 0.2, -0.3)).reshape(-1, order="F"))
    cdims, corigin = (C.c_int32 * 3)(*dims), (C.c_float * 3)(*origin)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)

    def make():
        import torch
        f = w.Flow((28, 26, 24), (1.0, 0.0, 0.0))
        g = w.core.sgrid(f.sigma)
        hold = Holder(L)
        torch.cuda.synchronize()

        class Named:                                        # what Body(("lattice", …)) needs of a lattice: its dimension and id
            D = 3

            @property
            def id(self):
                return L.wl_sdf_lattice_id(hold.h)

        def prog():
            return w.Body(("lattice", Named(), origin, 1.0, 0.0)).program(3)

        def create(sp):
            assert L.wl_sdf_lattice_from_mesh_band(C.byref(hold.h), 3, cdims, corigin, 1.0, V.ctypes.data_as(fp), len(V), E.ctypes.data_as(ip), len(E),
                                                   Wv.ctypes.data_as(fp), BAND, 0, sp) == 0
            assert L.wl_sdf_lattice_band(hold.h) == np.float32(BAND)
            return np.float32(L.wl_sdf_lattice_edge_min(hold.h))

        def measure(sp):
            p = prog()
            assert L.wl_measure_bodyset(w.core.ptr(f.sigma), w.core.ptr(f.mu0), w.core.ptr(f.mu1), w.core.ptr(f.V), C.byref(g), C.byref(p), 1.0, 0, 0, sp) == 0

        def update(sp):
            assert L.wl_sdf_lattice_update_mesh(hold.h, V1.ctypes.data_as(fp), W1.ctypes.data_as(fp), 0, sp) == 0
            assert L.wl_sdf_lattice_band(hold.h) == np.float32(BAND)
            return np.float32(L.wl_sdf_lattice_edge_min(hold.h))

        def read_w(sp):
            out = np.zeros(3 * count, f32)
            assert L.wl_sdf_lattice_read_velocity(hold.h, out.ctypes.data_as(fp), sp) == 0
            assert out.any()
            return out

        def read_a(sp):
            out = np.zeros(count, f32)
            assert L.wl_sdf_lattice_read(hold.h, out.ctypes.data_as(fp), sp) == 0
            assert np.abs(out).max() == np.float32(BAND)                  # clipped samples: the banded search ran
            return out

        def set_w(sp):
            assert L.wl_sdf_lattice_set_velocity(hold.h, Wset.ctypes.data_as(fp), sp) == 0

        arrays = [f.sigma, f.mu0, f.mu1, f.V]
        steps = [Step("wl_sdf_lattice_from_mesh_band", create, [], sync=True), Step("wl_measure_bodyset", measure, arrays),
                 Step("wl_sdf_lattice_read_velocity", read_w, [], sync=True),
                 Step("wl_measure_bodyset", measure, arrays),                         # queued, not waited for: the update below must fall in behind it
                 Step("wl_sdf_lattice_update_mesh", update, [], sync=True), Step("wl_sdf_lattice_read", read_a, [], sync=True),
                 Step("wl_sdf_lattice_read_velocity", read_w, [], sync=True), Step("wl_measure_bodyset", measure, arrays),
                 Step("wl_sdf_lattice_set_velocity", set_w, [], sync=True), Step("wl_measure_bodyset", measure, arrays),
                 Step("wl_sdf_lattice_read_velocity", read_w, [], sync=True)]
        return steps, (f, g, hold)
    run_on_streams(L, make, label="banded mesh + update + set/read velocity + measure")
    gc.collect()                                            # the scenarios' lattices go with their holders now, not whenever the cycles are collected: at most 8 are alive
