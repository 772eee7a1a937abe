"""The stream contract of include/wlhip.h for bodies from meshes: wl_sdf_lattice_from_mesh uploads its tables, launches the search and reads the samples back
on the caller's stream and synchronises that stream; the lattice it made is measured on the caller's stream like any other; wl_sdf_lattice_read copies the
samples on the caller's stream and synchronises it.  The scenario runs once on the default stream and once on a delayed non-blocking side stream with the
default stream blocked (tests/stream_harness.py) and must produce the same bits.  (The file's name makes it run after tests/test_gpu_streams.py: see
tests/test_gpu_streams_interp.py.)"""
import ctypes as C

import numpy as np
import pytest

import meshsdf_ref as mr
from stream_harness import Step, run_on_streams

pytestmark = pytest.mark.gpu
f32 = np.float32


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


def test_from_mesh_measure_and_read_keep_the_stream_contract(w):
    L = w.lib()
    c = mr.case("ico320")
    V = np.ascontiguousarray(c["V"] + np.array([3.0, 2.0, 1.5], f32))
    E = np.ascontiguousarray(c["E"], dtype=np.int32)
    dims, origin = w.bodies.mesh_placement(V, 1.0, 5.0)
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
            assert L.wl_sdf_lattice_from_mesh(C.byref(hold.h), 3, cdims, corigin, 1.0, V.ctypes.data_as(fp), len(V), E.ctypes.data_as(ip), len(E), 0, sp) == 0
            return np.float32(L.wl_sdf_lattice_edge_min(hold.h))

        def measure(sp):
            p = prog()
            assert L.wl_measure_bodyset(w.core.ptr(f.sigma), w.core.ptr(f.mu0), w.core.ptr(f.mu1), w.core.ptr(f.V), C.byref(g), C.byref(p), 1.0, 0, 0, sp) == 0

        def read(sp):
            out = np.zeros(int(np.prod(dims)), f32)
            assert L.wl_sdf_lattice_read(hold.h, out.ctypes.data_as(fp), sp) == 0
            assert (out < 0).any() and (out > 0).any()
            return out
        arrays = [f.sigma, f.mu0, f.mu1, f.V]
        steps = [Step("wl_sdf_lattice_from_mesh", create, [], sync=True), Step("wl_measure_bodyset", measure, arrays),
                 Step("wl_sdf_lattice_read", read, [], sync=True), Step("wl_measure_bodyset", measure, arrays)]
        return steps, (f, g, hold)
    run_on_streams(L, make, label="lattice from a mesh + measure + read")
