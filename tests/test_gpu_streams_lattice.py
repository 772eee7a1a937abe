"""The stream contract of include/wlhip.h for the sampled bodies: wl_sdf_lattice_create copies its samples on the caller's stream and synchronises that
stream, and a program with a lattice leaf is measured on the caller's stream like any other.  The scenario runs once on the default stream and once on a
delayed non-blocking side stream with the default stream blocked (tests/stream_harness.py) and must produce the same bits.  (The file's name makes it run
after tests/test_gpu_streams.py: see tests/test_gpu_streams_interp.py.)"""
import ctypes as C

import numpy as np
import pytest

import lattice_ref as lr
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


def test_create_and_measure_keep_the_stream_contract(w):
    L = w.lib()
    c = lr.field_case("sphere3")
    vals = np.ascontiguousarray(c["values"].reshape(-1, order="F"))
    dims = (C.c_int32 * 3)(*c["dims"])
    X = np.ascontiguousarray(lr.point_case("sphere")["X"][:128] * f32(0.5))
    fp = C.POINTER(C.c_float)

    def make():
        import torch
        f = w.Flow(c["grid"], (1.0, 0.0, 0.0))
        g = w.core.sgrid(f.sigma)
        hold = Holder(L)
        torch.cuda.synchronize()

        def prog():
            return c["body"](lr.HostLattice(c["values"], id=L.wl_sdf_lattice_id(hold.h))).program(3)

        def create(sp):
            assert L.wl_sdf_lattice_create(C.byref(hold.h), 3, dims, vals.ctypes.data_as(fp), sp) == 0
            return None

        def measure(sp):
            p = prog()
            assert L.wl_measure_bodyset(w.core.ptr(f.sigma), w.core.ptr(f.mu0), w.core.ptr(f.mu1), w.core.ptr(f.V), C.byref(g), C.byref(p), 1.0, 0, 0, sp) == 0

        def points(sp):
            p = prog()
            d, n, V = np.zeros(len(X), f32), np.zeros(X.shape, f32), np.zeros(X.shape, f32)
            assert L.wl_bodyset_measure_points(C.byref(p), 3, X.ctypes.data_as(fp), len(X), 9.0, d.ctypes.data_as(fp), n.ctypes.data_as(fp), V.ctypes.data_as(fp), sp) == 0
            return (d, n, V)
        arrays = [f.sigma, f.mu0, f.mu1, f.V]
        steps = [Step("wl_sdf_lattice_create", create, [], sync=True), Step("wl_measure_bodyset", measure, arrays),
                 Step("wl_bodyset_measure_points", points, [], sync=True), Step("wl_measure_bodyset", measure, arrays)]
        return steps, (f, g, hold)
    run_on_streams(L, make, label="lattice create + measure")
